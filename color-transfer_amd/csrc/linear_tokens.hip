// linear_tokens.hip -- nn.Linear and LayerNorm(128) on channels-last tokens [tokens][C] of the GMFlow transformer
// (transformer.py:26-43,131-147, attention.py:181-182): the exact-f32 LDS-tiled GEMM (linear_tokens_kernel), the
// three-piece bf16 "split" GEMMs (linear_split_kernel<MT>, linear_split_wres_kernel) and layernorm_tokens_kernel.
// The two-piece fp16 weights-resident form is linear_ws16.hip.
#include "ct_common.h"
#include "ct_split.h"

namespace ct {

// =================================================================================================
// nn.Linear on channels-last tokens: out[t][n] = act( sum_k x[t][k] W[n][k] + bias[n] )
// LDS-tiled "NT" GEMM: a workgroup owns 128 tokens x 128 features, each of its 4 waves a 64 x 64 quarter (2 x 2 MFMA
// tiles).  K is walked in 32-channel chunks: both operands are K-contiguous in memory ([T][K] and PyTorch's [N][K]),
// so a chunk of either is 128 rows x 128 bytes, fetched with fully coalesced 16-byte loads into registers while the
// previous chunk is multiplied, then written to LDS rows of 36 floats (16-byte aligned, conflict-free 16-byte reads).
// The contraction index of the two lane halves is split as k = 16*hl + p inside a chunk (any order is a valid dot
// product), so the MFMA operands come out of LDS as float4.  The result goes through a per-wave 32x32 LDS transpose so
// that it is stored 16 bytes per lane.  K % 16 == 0 (128, 256, 1024 here).  grid = (ceil(T/128), ceil(N/128)).
// =================================================================================================
constexpr int kLinLd = 36;   // LDS row stride in floats

// x2 != null: the input row is the concatenation [x[t][0:K1] | x2[t][0:K-K1]] (K1 % 32 == 0) -- the
// torch.cat([source, message]) in front of the FFN (transformer.py:131) without materialising it.
__global__ __launch_bounds__(256) void linear_tokens_kernel(const float *__restrict__ x, const float *__restrict__ x2, int K1,
                                                            const float *__restrict__ w, const float *__restrict__ bias,
                                                            float *__restrict__ out, long long T, int K, int N,
                                                            int act /*0 none, 6 gelu*/) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 128 * kLinLd];
    float *Xs = lds, *Ws = lds + 128 * kLinLd;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = lane & 31, hl = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    const long long t0 = (long long)blockIdx.x * 128;
    const int n0 = blockIdx.y * 128;

    // staging: thread -> 4 (row, 16-byte column) slots of each operand tile
    const int srow = tid >> 3, sq = tid & 7;
    const float *wg[4];
    long long xr[4];
    const int K2 = K - K1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long tr = t0 + srow + 32 * i;
        const int nr = n0 + srow + 32 * i;
        xr[i] = tr < T ? tr : T - 1;
        wg[i] = w + (size_t)(nr < N ? nr : N - 1) * K + 4 * sq;
    }
    float4 px[4], pw[4];
    auto fetch = [&](int kc) {
        const bool inb = (kc + 4 * sq) < K;    // K % 4 == 0: a float4 is in range or not at all
        const bool second = kc >= K1;          // uniform: a 32-channel chunk never straddles the two sources
        const float *xs = second ? x2 + (kc - K1) + 4 * sq : x + kc + 4 * sq;
        const int ld = second ? K2 : K1;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            px[i] = inb ? *reinterpret_cast<const float4 *>(xs + xr[i] * ld) : make_float4(0.f, 0.f, 0.f, 0.f);
            pw[i] = inb ? *reinterpret_cast<const float4 *>(wg[i] + kc) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<float4 *>(Xs + (srow + 32 * i) * kLinLd + 4 * sq) = px[i];
            *reinterpret_cast<float4 *>(Ws + (srow + 32 * i) * kLinLd + 4 * sq) = pw[i];
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    fetch(0);
    stage();
    const float *xa = Xs + (wm * 64 + nl) * kLinLd + hl * 16;
    const float *wb = Ws + (wn * 64 + nl) * kLinLd + hl * 16;
    for (int kc = 0; kc < K; kc += 32) {
        __syncthreads();                       // this chunk is visible
        const bool more = (kc + 32) < K;
        if (more) fetch(kc + 32);              // in flight under the MFMAs below
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 a0 = *reinterpret_cast<const float4 *>(xa + 4 * q);
            const float4 a1 = *reinterpret_cast<const float4 *>(xa + 32 * kLinLd + 4 * q);
            const float4 b0 = *reinterpret_cast<const float4 *>(wb + 4 * q);
            const float4 b1 = *reinterpret_cast<const float4 *>(wb + 32 * kLinLd + 4 * q);
            const float av[2][4] = {{a0.x, a0.y, a0.z, a0.w}, {a1.x, a1.y, a1.z, a1.w}};
            const float bv[2][4] = {{b0.x, b0.y, b0.z, b0.w}, {b1.x, b1.y, b1.z, b1.w}};
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][e], bv[j][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();                       // every wave is done with this chunk
        if (more) stage();
    }

    // D[token][feature]: lane = feature column, registers = token rows (r&3)+8(r>>2)+4hl of the 32x32 tile.
    // Per-wave transpose buffer (the operand tiles are dead after the last barrier): rows = tokens, 32 features each.
    float *stg = lds + wave * (32 * 32);
    const bool wide = ((N & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int f0 = n0 + wn * 64 + j * 32;
            const long long tt0 = t0 + wm * 64 + i * 32;
            const int nf = f0 + nl;
            const float bb = (bias && nf < N) ? bias[nf] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float v = acc[i][j][r] + bb;
                if (act == 6) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752f));   // exact GELU (nn.GELU default)
                acc[i][j][r] = v;
            }
            if (wide) {
#pragma unroll
                for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * hl) * 32 + nl] = acc[i][j][r];
                __builtin_amdgcn_wave_barrier();
                const int fc = f0 + 4 * (lane & 7);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int row = (lane >> 3) + 8 * g;
                    const float4 v = *reinterpret_cast<const float4 *>(stg + row * 32 + 4 * (lane & 7));
                    const long long t = tt0 + row;
                    if (t < T && fc < N) *reinterpret_cast<float4 *>(out + t * N + fc) = v;   // N % 4 == 0: all four or none
                }
                __builtin_amdgcn_wave_barrier();
            } else if (nf < N) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long t = tt0 + (r & 3) + 8 * (r >> 2) + 4 * hl;
                    if (t < T) out[t * N + nf] = acc[i][j][r];
                }
            }
        }
}

// LayerNorm over the last dim (C = 128, eps 1e-5, affine) of [T][128], optional residual: out = res + LN(x).
// One wave per token (2 channels per lane).
__global__ __launch_bounds__(256) void layernorm_tokens_kernel(const float *__restrict__ x, const float *__restrict__ g,
                                                               const float *__restrict__ b, const float *__restrict__ res,
                                                               float *__restrict__ out, long long T, int partials) {
    const int lane = threadIdx.x & 63;
    const long long t = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= T) return;
    float2 v = *reinterpret_cast<const float2 *>(x + t * 128 + 2 * lane);
    for (int p = 1; p < partials; ++p) {       // the K-sliced linear's partial slabs [partials][T][128], added in slab order
        const float2 u = *reinterpret_cast<const float2 *>(x + ((long long)p * T + t) * 128 + 2 * lane);
        v.x += u.x; v.y += u.y;
    }
    float s = v.x + v.y;
    s = wave_all_sum(s);
    const float mean = s * (1.0f / 128.0f);
    const float dx = v.x - mean, dy = v.y - mean;
    float ss = dx * dx + dy * dy;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / 128.0f) + 1e-5f);
    float o0 = dx * rstd * g[2 * lane] + b[2 * lane], o1 = dy * rstd * g[2 * lane + 1] + b[2 * lane + 1];
    if (res) { o0 += res[t * 128 + 2 * lane]; o1 += res[t * 128 + 2 * lane + 1]; }
    *reinterpret_cast<float2 *>(out + t * 128 + 2 * lane) = make_float2(o0, o1);
}

// =================================================================================================
// nn.Linear on channels-last tokens on the bf16 matrix pipe ("split", float32-grade accuracy: conv_split.hip's arithmetic).
// A workgroup owns MT (128 or 64) tokens x 128 features, its 4 waves MT/2 x 64 quarters; K is walked in chunks of 32
// channels = two v_mfma_f32_32x32x16_bf16 K steps, six MFMAs per product.
//   W: pre-split on the host in exactly the LDS image of a chunk ([piece][8-channel group][feature row] x 16 bytes,
//      ct_hip.pack_linear_weight_split): staging is a linear 24 KiB copy through registers, fetched one chunk ahead.
//   X: split in registers while it is staged (a thread owns 8 consecutive channels of a token = one MFMA fragment per
//      piece), into a DOUBLE-buffered LDS image: the split of chunk c+1 (VALU) runs between the MFMAs of chunk c, the raw
//      loads are issued two chunks ahead.  Group stride MT+4 rows: the 16 lanes of a ds_write_b128 pass hit 16 distinct
//      bank groups; fragment reads are 32 consecutive rows of one group = conflict free.
// Two barriers per chunk (X/W of the chunk visible; W consumed), only the short W copy sits between them.  LDS 73.5 KiB
// (MT = 128): two workgroups per CU, so one's prologue / epilogue (bias, GELU, transpose, stores) runs under the other's MFMAs.
// Several feature tiles (N > 128): 1-D grid ordered so that the tiles of one token block run at the same time on the same
// XCD (workgroup b is placed on XCD b % 8) -- the block's tokens come from HBM once and from that XCD's L2 afterwards.
// K % 32 == 0.
// =================================================================================================
constexpr int kLsW = 3 * 4 * 128;                 // uint4 entries of the W image (= one packed chunk)

template <int MT>
__global__ __launch_bounds__(256, 2) void linear_split_kernel(const float *__restrict__ x, const float *__restrict__ x2, int K1,
                                                              const uint4 *__restrict__ wp, const float *__restrict__ bias,
                                                              float *__restrict__ out, long long T, int K, int N, int act,
                                                              int n_nt) {
    constexpr int MI = MT / 64;                   // 32-token MFMA tiles per wave (and X staging units per thread)
    constexpr int XR = MT + 4;                    // rows per (piece, group) of an X image
    constexpr int XIMG = 3 * 4 * XR;              // uint4 entries of one X image
    __shared__ uint4 lds[2 * XIMG + kLsW];
    uint4 *Ws = lds + 2 * XIMG;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = lane & 31, hl = lane >> 5;
    const int wm = wave & 1, wn = wave >> 1;
    // tile of this workgroup: logical ids run XCD-major, feature tile fastest
    unsigned int lid = blockIdx.x;
    if (n_nt > 1 && (gridDim.x & 7) == 0) lid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int nt = (int)(lid % (unsigned)n_nt);
    const long long t0 = (long long)(lid / (unsigned)n_nt) * MT;
    const int n0 = nt * 128;
    const int n_chunks = K >> 5;
    const uint4 *wsrc = wp + (size_t)nt * n_chunks * kLsW + tid;
    // X staging: unit u = tid + 256 i -> (token row u >> 2, 8-channel group u & 3): four lanes read one token's 128 bytes
    const int srow = tid >> 2, sg = tid & 3;
    long long xr[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const long long tr = t0 + srow + 64 * i;
        xr[i] = tr < T ? tr : T - 1;
    }
    const int K2 = K - K1;
    float4 pa[MI][2], pb[MI][2];                  // raw X of chunk c+1 (being split) / chunk c+2 (in flight)
    uint4 pw[6];
    auto fetch_x = [&](int c, float4 (&px)[MI][2]) {
        const int kc = c << 5;
        const bool second = kc >= K1;          // uniform: a 32-channel chunk never straddles the two sources
        const float *xs = second ? x2 + (kc - K1) + 8 * sg : x + kc + 8 * sg;
        const int ld = second ? K2 : K1;
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            const float4 *p = reinterpret_cast<const float4 *>(xs + xr[i] * ld);
            px[i][0] = p[0];
            px[i][1] = p[1];
        }
    };
    auto fetch_w = [&](int c) {
#pragma unroll
        for (int j = 0; j < 6; ++j) pw[j] = wsrc[(size_t)c * kLsW + 256 * j];
    };
    auto split_unit = [&](const float4 (&px)[MI][2], int i, uint4 *img) {
        const float v[8] = {px[i][0].x, px[i][0].y, px[i][0].z, px[i][0].w, px[i][1].x, px[i][1].y, px[i][1].z, px[i][1].w};
        uint4 h, m, l;
        split3x8(v, h, m, l);
        uint4 *d = img + sg * XR + srow + 64 * i;
        d[0] = h;
        d[4 * XR] = m;
        d[8 * XR] = l;
    };
    auto store_w = [&]() {
#pragma unroll
        for (int j = 0; j < 6; ++j) Ws[tid + 256 * j] = pw[j];
    };

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    fetch_x(0, pb);
    fetch_w(0);
#pragma unroll
    for (int i = 0; i < MI; ++i) split_unit(pb, i, lds);
    store_w();
    if (n_chunks > 1) {
        fetch_x(1, pa);
        fetch_w(1);
    }
    const int xoff = hl * XR + wm * (MT / 2) + nl;
    const uint4 *wb = Ws + hl * 128 + wn * 64 + nl;
    // one chunk: `cur` holds the raw X of chunk c+1 (loaded a chunk ago), `nxt` receives chunk c+2
    auto chunk = [&](int c, float4 (&cur)[MI][2], float4 (&nxt)[MI][2]) {
        __syncthreads();                       // X image c & 1 and the W image hold chunk c
        if (c + 2 < n_chunks) fetch_x(c + 2, nxt);
        const uint4 *xa = lds + (c & 1) * XIMG + xoff;
        uint4 *xn = lds + ((c + 1) & 1) * XIMG;
#pragma unroll
        for (int s = 0; s < 2; ++s) {          // K step: channels 16 s + 8 hl + 0..7 of the chunk
            uint4 a[MI][3], b[2][3];
#pragma unroll
            for (int p = 0; p < 3; ++p) {
#pragma unroll
                for (int i = 0; i < MI; ++i) a[i][p] = xa[(4 * p + 2 * s) * XR + 32 * i];
#pragma unroll
                for (int j = 0; j < 2; ++j) b[j][p] = wb[(4 * p + 2 * s) * 128 + 32 * j];
            }
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) mfma_split6(acc[i][j], a[i], b[j]);
            // the split of chunk c+1 (one staging unit per K step) goes to the other image, its VALU work between the MFMAs
            // above (after the last chunk it re-splits stale registers into the dead image: no branch in the schedule region)
            if (s < MI) {
                split_unit(cur, s, xn);
#pragma unroll
                for (int q = 0; q < 12 * MI; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, MI == 2 ? 3 : 6, 0);
                }
            }
        }
        __syncthreads();                       // every wave is done with the W image
        if (c + 1 < n_chunks) {
            store_w();
            if (c + 2 < n_chunks) fetch_w(c + 2);
        }
    };
    for (int c = 0; c < n_chunks; c += 2) {    // unrolled by two: the raw-X register sets swap roles without copies
        chunk(c, pa, pb);
        if (c + 1 < n_chunks) chunk(c + 1, pb, pa);
    }

    // epilogue: per-wave LDS transpose (the operand images are dead after the last barrier), 16-byte stores
    float *stg = reinterpret_cast<float *>(lds) + wave * (32 * 32);
    const bool wide = ((N & 3) == 0) && ((reinterpret_cast<uintptr_t>(out) & 15) == 0);
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int f0 = n0 + wn * 64 + j * 32;
            const long long tt0 = t0 + wm * (MT / 2) + i * 32;
            const int nf = f0 + nl;
            const float bb = (bias && nf < N) ? bias[nf] : 0.f;
            if (act == 6) {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = gelu_as(acc[i][j][r] + bb);
            } else {
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] += bb;
            }
            if (wide) {
#pragma unroll
                for (int r = 0; r < 16; ++r) stg[((r & 3) + 8 * (r >> 2) + 4 * hl) * 32 + nl] = acc[i][j][r];
                __builtin_amdgcn_wave_barrier();
                const int fc = f0 + 4 * (lane & 7);
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int row = (lane >> 3) + 8 * g;
                    const float4 v = *reinterpret_cast<const float4 *>(stg + row * 32 + 4 * (lane & 7));
                    const long long t = tt0 + row;
                    if (t < T && fc < N) *reinterpret_cast<float4 *>(out + t * N + fc) = v;   // N % 4 == 0: all four or none
                }
                __builtin_amdgcn_wave_barrier();
            } else if (nf < N) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long t = tt0 + (r & 3) + 8 * (r >> 2) + 4 * hl;
                    if (t < T) out[t * N + nf] = acc[i][j][r];
                }
            }
        }
}

// -------------------------------------------------------------------------------------------------
// K = 128, N <= 128 (the q / k / v / merge projections: 8 of the 10 linears of a transformer layer): the whole pre-split W
// (4 chunks x 24 KiB = 96 KiB) stays RESIDENT in LDS for the lifetime of a persistent 8-wave workgroup, and the activations
// never touch LDS: a lane of v_mfma_f32_32x32x16_bf16 holds 8 consecutive channels of ONE token, which is what it gets from
// two 16-byte loads of a row-major [T][K] row.  Each wave walks 32-token tiles on its own (32 tokens x all 128 features:
// no wave needs another wave's tokens, so there is no barrier after the prologue); per chunk a lane loads its token's 64
// contiguous bytes (channels 16 hl .. 16 hl + 15: K step s of lane half hl is channels 16 hl + 8 s + j -- any bijection is
// a valid contraction order as long as W is read with the same one, group 2 hl + s), the next chunk's / tile's loads are
// in flight under the 48 MFMAs of the current chunk, and its split (VALU) is scheduled between them.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(512, 1) void linear_split_wres_kernel(const float *__restrict__ x, const uint4 *__restrict__ wp,
                                                                    const float *__restrict__ bias, float *__restrict__ out, long long T,
                                                                    int N, int act, int n_tiles) {
    constexpr int NC = 4;                          // K = 128
    __shared__ uint4 Ws[NC * kLsW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = lane & 31, hl = lane >> 5;
#pragma unroll
    for (int j = 0; j < NC * kLsW / 512; ++j) Ws[tid + 512 * j] = wp[tid + 512 * j];
    const uint4 *wb = Ws + 2 * hl * 128 + nl;
    float bb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bb[j] = (bias && 32 * j + nl < N) ? bias[32 * j + nl] : 0.f;
    __syncthreads();

    const int stride = gridDim.x * 8;
    int tile = blockIdx.x * 8 + wave;
    if (tile >= n_tiles) return;
    auto row_ptr = [&](int t) {
        const long long tr = (long long)t * 32 + nl;
        return reinterpret_cast<const float4 *>(x + (tr < T ? tr : T - 1) * 128 + 16 * hl);
    };
    float4 raw[2][4];                              // raw X of the chunk after the current one (ring of two)
    uint4 fa[2][2][3];                             // A fragments of the current / next chunk
    auto fetch = [&](const float4 *p, int c, float4 (&r)[4]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) r[q] = p[8 * c + q];
    };
    auto split_x = [&](const float4 (&px)[4], uint4 (&f)[2][3]) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float v[8] = {px[2 * s].x, px[2 * s].y, px[2 * s].z, px[2 * s].w, px[2 * s + 1].x, px[2 * s + 1].y, px[2 * s + 1].z, px[2 * s + 1].w};
            split3x8(v, f[s][0], f[s][1], f[s][2]);
        }
    };
    const float4 *xp = row_ptr(tile);
    fetch(xp, 0, raw[0]);
    fetch(xp, 1, raw[1]);
    split_x(raw[0], fa[0]);
    for (; tile < n_tiles; tile += stride) {
        const int next = tile + stride;
        const float4 *xn = row_ptr(next < n_tiles ? next : tile);
        f32x16 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            // raw[(c + 1) & 1] holds chunk c+1 (of this tile, or chunk 0 of the next tile): split it under the MFMAs of chunk c;
            // raw[c & 1] is free: fetch chunk c+2 into it
            if (c + 2 < NC) fetch(xp, c + 2, raw[c & 1]);
            else fetch(xn, c + 2 - NC, raw[c & 1]);
            const uint4 *wc = wb + c * kLsW;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                uint4 b[4][3];
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int j = 0; j < 4; ++j) b[j][p] = wc[(4 * p + s) * 128 + 32 * j];
#pragma unroll
                for (int j = 0; j < 4; ++j) mfma_split6(acc[j], fa[c & 1][s], b[j]);
            }
            split_x(raw[(c + 1) & 1], fa[(c + 1) & 1]);
#pragma unroll
            for (int q = 0; q < 24; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 5, 0);
            }
        }
        // epilogue: lane = feature column, registers = token rows; 32 lanes store 128 contiguous bytes of a token
        const long long t0 = (long long)tile * 32;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nf = 32 * j + nl;
            if (nf < N) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const long long t = t0 + (r & 3) + 8 * (r >> 2) + 4 * hl;
                    const float v = acc[j][r] + bb[j];
                    if (t < T) out[t * N + nf] = act == 6 ? gelu_as(v) : v;
                }
            }
        }
        xp = xn;
    }
}

}  // namespace ct

// -------------------------------------------------------------------------------------------------
// C ABI (include/ct_hip.h)
// -------------------------------------------------------------------------------------------------
extern "C" {

int ct_linear_tokens_f32(const float *x, const float *x2, int k1, const float *w, const float *bias, float *out, long long tokens,
                         int k, int n, int act, void *stream) {
    if (!x || !w || !out || tokens < 0 || k < 16 || (k % 16) || n < 1) return CT_E_BADARG;
    if (x2 ? (k1 < 32 || k1 >= k || (k1 % 32)) : (k1 != k)) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(x2)) & 15) return CT_E_ALIGN;
    if (tokens == 0) return CT_OK;
    dim3 grid((unsigned)((tokens + 127) / 128), (n + 127) / 128);
    hipLaunchKernelGGL(ct::linear_tokens_kernel, grid, dim3(256), 0, (hipStream_t)stream, x, x2, k1, w, bias, out, tokens, k, n, act);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

// wp: ct_hip.pack_linear_weight_split(weight): bf16 bit patterns [ceil(n/128)][k/32][piece hi/mid/lo][8-channel group 0..3]
// [feature row 0..127][8 channels], zero rows beyond n.  k % 32 == 0 (k1 % 32 == 0 with x2).
int ct_linear_tokens_split_f32(const float *x, const float *x2, int k1, const void *wp, const float *bias, float *out, long long tokens,
                               int k, int n, int act, void *stream) {
    if (!x || !wp || !out || tokens < 0 || k < 32 || (k % 32) || n < 1) return CT_E_BADARG;
    if (x2 ? (k1 < 32 || k1 >= k || (k1 % 32)) : (k1 != k)) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(wp) | reinterpret_cast<uintptr_t>(x2)) & 15) return CT_E_ALIGN;
    if (tokens == 0) return CT_OK;
    const int n_nt = (n + 127) / 128;
    // 64-token tiles while 128-token tiles would leave CUs without a workgroup (2 per CU are resident)
    const long long tiles128 = (tokens + 127) / 128 * n_nt;
    if (k == 128 && n <= 128 && !x2) {              // q / k / v / merge projections: W resident in LDS, X straight into MFMA fragments
        const long long tiles32 = (tokens + 31) / 32;
        long long g = (tiles32 + 7) / 8;
        if (g > 256) g = 256;
        hipLaunchKernelGGL(ct::linear_split_wres_kernel, dim3((unsigned)g), dim3(512), 0, (hipStream_t)stream, x, (const uint4 *)wp, bias, out,
                           tokens, n, act, (int)tiles32);
        CT_CHECK_LAUNCH();
        return CT_OK;
    }
    if (tiles128 >= 2 * 256) {
        hipLaunchKernelGGL(ct::linear_split_kernel<128>, dim3((unsigned)tiles128), dim3(256), 0, (hipStream_t)stream, x, x2, k1,
                           (const uint4 *)wp, bias, out, tokens, k, n, act, n_nt);
    } else {
        hipLaunchKernelGGL(ct::linear_split_kernel<64>, dim3((unsigned)((tokens + 63) / 64 * n_nt)), dim3(256), 0, (hipStream_t)stream, x,
                           x2, k1, (const uint4 *)wp, bias, out, tokens, k, n, act, n_nt);
    }
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_layernorm128_f32(const float *x, const float *gamma, const float *beta, const float *residual, float *out, long long tokens,
                        int partials, void *stream) {
    if (!x || !gamma || !beta || !out || tokens < 0 || partials < 1 || partials > 64) return CT_E_BADARG;
    if (tokens == 0) return CT_OK;
    hipLaunchKernelGGL(ct::layernorm_tokens_kernel, dim3((unsigned)((tokens + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, gamma,
                       beta, residual, out, tokens, partials);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
