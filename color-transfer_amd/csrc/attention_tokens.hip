// attention_tokens.hip -- streaming (online-softmax) attention on channels-last tokens with float32 operands as three bf16
// pieces (attention_tokens_kernel, its key-split merge attention_combine_kernel, the column sums attention_colsum_kernel),
// and the NCHW <-> token-rows transposes that feed it.  The C entry points dispatch to the two-piece fp16 kernels of
// attention16.hip unless CT_HIP_ATT16=0.
#include "ct_common.h"
#include "ct_split.h"
#include "ct_attention16.h"

namespace ct {

// =================================================================================================
// NCHW <-> token rows: rows[(b*H + y)*W + x][c0 + c] = nchw[b][c][y][x]  (and back).  The streaming parallax attention
// works on channels-last rows; torch's permute().contiguous() moves these tensors at < 1 TB/s.  One workgroup per
// (64 pixels of a row, b*H + y): 32-channel x 64-pixel tiles through LDS, 256-byte runs on the NCHW side, 128-byte
// runs on the row side.  grid = (ceil(W/64), B*H), block 256.
// =================================================================================================
template <bool TO_ROWS>
__global__ __launch_bounds__(256) void rows_transpose_kernel(const float *__restrict__ src, float *__restrict__ dst, int C, int H,
                                                             int W, long long nchw_bstride, int row_channels, int c0) {
    __shared__ float t[32][65];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * 64;
    const int by = blockIdx.y, b = by / H, y = by - b * H;
    const size_t plane = (size_t)H * W;
    const float *nsrc = src;
    float *ndst = dst;
    // full 64-pixel tiles with 16-byte aligned rows move as two float4 per thread on the global side (round 3: the scalar
    // form ran at 2.3 TB/s and cost DCMCS3DI 3.4 ms per 1080p pair); everything else takes the element-wise path
    const bool vec = (x0 + 64 <= W) && ((W & 3) == 0) && ((row_channels & 3) == 0) && ((c0 & 3) == 0) && ((nchw_bstride & 3) == 0) &&
                     (((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15) == 0);
    for (int cb = 0; cb < C; cb += 32) {
        const bool full = vec && (cb + 32 <= C);
        if (TO_ROWS) {
            // NCHW -> LDS: thread (c = tid>>3 [+0], x = 8*(tid&7)..) : 32 channels x 64 pixels, 8 floats per thread
            const int c = tid >> 3, xs = (tid & 7) * 8;
            const float *p = nsrc + (size_t)b * nchw_bstride + (size_t)(cb + c) * plane + (size_t)y * W + x0 + xs;
            if (full) {
                const float4 a = reinterpret_cast<const float4 *>(p)[0], bb = reinterpret_cast<const float4 *>(p)[1];
                t[c][xs] = a.x; t[c][xs + 1] = a.y; t[c][xs + 2] = a.z; t[c][xs + 3] = a.w;
                t[c][xs + 4] = bb.x; t[c][xs + 5] = bb.y; t[c][xs + 6] = bb.z; t[c][xs + 7] = bb.w;
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) t[c][xs + i] = (cb + c < C && x0 + xs + i < W) ? p[i] : 0.f;
            }
            __syncthreads();
            // LDS -> rows: thread (x = tid>>2, channel group g = tid&3 -> 8 channels)
            const int x = tid >> 2, g = (tid & 3) * 8;
            if (x0 + x < W) {
                float *q = ndst + ((size_t)by * W + x0 + x) * row_channels + c0 + cb + g;
                if (full) {
                    reinterpret_cast<float4 *>(q)[0] = make_float4(t[g][x], t[g + 1][x], t[g + 2][x], t[g + 3][x]);
                    reinterpret_cast<float4 *>(q)[1] = make_float4(t[g + 4][x], t[g + 5][x], t[g + 6][x], t[g + 7][x]);
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (cb + g + i < C) q[i] = t[g + i][x];
                }
            }
            __syncthreads();
        } else {
            const int x = tid >> 2, g = (tid & 3) * 8;
            if (x0 + x < W) {
                const float *q = nsrc + ((size_t)by * W + x0 + x) * row_channels + c0 + cb + g;
                if (full) {
                    const float4 a = reinterpret_cast<const float4 *>(q)[0], bb = reinterpret_cast<const float4 *>(q)[1];
                    t[g][x] = a.x; t[g + 1][x] = a.y; t[g + 2][x] = a.z; t[g + 3][x] = a.w;
                    t[g + 4][x] = bb.x; t[g + 5][x] = bb.y; t[g + 6][x] = bb.z; t[g + 7][x] = bb.w;
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i) t[g + i][x] = (cb + g + i < C) ? q[i] : 0.f;
                }
            }
            __syncthreads();
            const int c = tid >> 3, xs = (tid & 7) * 8;
            if (cb + c < C) {
                float *p = ndst + (size_t)b * nchw_bstride + (size_t)(cb + c) * plane + (size_t)y * W + x0 + xs;
                if (full) {
                    reinterpret_cast<float4 *>(p)[0] = make_float4(t[c][xs], t[c][xs + 1], t[c][xs + 2], t[c][xs + 3]);
                    reinterpret_cast<float4 *>(p)[1] = make_float4(t[c][xs + 4], t[c][xs + 5], t[c][xs + 6], t[c][xs + 7]);
                } else {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (x0 + xs + i < W) p[i] = t[c][xs + i];
                }
            }
            __syncthreads();
        }
    }
}

// =================================================================================================
// Streaming single-head attention on channels-last tokens (C = 128):
//   out[b][i][:] = sum_j softmax_j( q[b][i].k[b][j] / sqrt(C) + mask(i,j) ) v[b][j][:]
// One wave = 32 queries; keys are visited 32 at a time with an online softmax.  The score tile is computed
// TRANSPOSED (M = keys, N = queries), so a lane owns ONE query column: its running max / sum / rescale are
// per-lane scalars and the accumulator (also query-on-lane) rescales without any cross-lane traffic.
//   CV == 128: P.V on MFMA (M = value channels, N = queries, K = keys, P taken from the score registers)
//   CV == 2  : the two value channels (coordinates / flow) are accumulated by the VALU
//   region != null: additive -100 where region[i] != region[j] (shifted-window mask, utils.py:87-111)
// q/k/v rows are fetched with 16-byte loads (a lane needs C/2 consecutive channels of one token row).
// grid = (ceil(L/128), B); block = 4 waves.
// =================================================================================================
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

constexpr int kSsRow(int C) { return 2 * C + 16; }   // bytes per LDS row of a split tile: 16-byte fragment reads are conflict free

// two workgroups per CU where the registers allow it without spilling (the 64-channel parallax attention: 238 VGPRs; the
// 128-channel instances need 256 + 127 and stay at one): 99.1 -> 98.1 ms on DCMCS3DI at 1080p
template <int C, int CV, bool MAP, bool SS>
__global__ __launch_bounds__(256, C == 64 ? 2 : 1) void attention_tokens_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                               const float *__restrict__ v, const int *__restrict__ region,
                                                               const int *__restrict__ rowmap, float *__restrict__ out,
                                                               float *__restrict__ stats, int L, float scale,
                                                               float *__restrict__ part, long long kv_shift = 0, long long kv_total = 0) {
    // kv_shift (rowmap launches only): the keys / values of token (b, i) live kv_shift rows further (mod kv_total) than its
    // query -- the cross attention of transformer.py:281-287 attends every image to the OTHER half of the batch, which the
    // reference materialises as torch.cat(chunk(2)[::-1]) after every layer
    constexpr int CH = C / 2;                       // channels per lane half
    constexpr int NVT = CV >= 32 ? CV / 32 : 1;     // 32-channel value tiles on the MFMA path
    constexpr int KLD = C + 4;                      // padded LDS rows: the 16-lane column reads (b128) are conflict free
    constexpr int VLD = CV >= 32 ? CV + 4 : 4;
    constexpr int KV4 = (32 * C / 4) / 256;         // float4 per thread of one K tile (4 / 2)
    constexpr int VV4 = CV >= 32 ? (32 * CV / 4) / 256 : 1;   // V tile (4 / 3), or the 16 float4 of a 2-channel tile
    // The 4 waves of a workgroup attend 4 x 32 queries of the SAME batch item to the same keys: every 32-key tile
    // of K and V is fetched once per workgroup with 16-byte loads (next tile in flight in registers while the current
    // one is multiplied), staged in LDS, and read from there as MFMA operands.
    constexpr int SROW = kSsRow(C);                 // SS: K tile as [piece][key][C] bf16, rows padded to SROW bytes
    __shared__ __attribute__((aligned(16))) float Ks[SS ? 3 * 32 * SROW / 4 : 32 * KLD];
    // SS with an MFMA value path: V as [piece][key][CV] bf16 too, rows of VROWB bytes with (VROWB / 4) % 64 == 16 or 48, so the
    // four rows a transposed read gathers lie in four disjoint 16-bank windows (cdna_hip_programming.md T10)
    constexpr bool PVS = SS && CV >= 32;
    constexpr int VROWB = (CV * 2) % 256 == 0 ? CV * 2 + 64 : CV * 2;
    static_assert(!PVS || ((VROWB / 4) % 64 == 16 || (VROWB / 4) % 64 == 48), "V image rows must not share banks");
    __shared__ __attribute__((aligned(16))) float Vs[PVS ? 3 * 32 * VROWB / 4 : 32 * VLD];
    __shared__ int Rs[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = lane & 31, hl = lane >> 5;
    const int b = blockIdx.y;
    const int q0 = (blockIdx.x * 4 + wave) * 32;
    const size_t tb = (size_t)b * L;
    const int qi = q0 + nl;
    const bool qlive = qi < L;
    const int qclamp = qlive ? qi : L - 1;
    // rowmap (optional): token (b, i) of this launch lives in row rowmap[b*L + i] of q / k / v / out -- the shifted-window
    // partition of attention.py:60-92 as an index table instead of roll + permute copies
    auto row = [&](int i) -> size_t {
        if constexpr (MAP) return (size_t)rowmap[tb + i];
        else return tb + i;
    };
    auto kvrow = [&](int i) -> size_t {
        size_t r = row(i);
        if constexpr (MAP) {
            r += (size_t)kv_shift;
            if (r >= (size_t)kv_total && kv_total > 0) r -= (size_t)kv_total;
        }
        return r;
    };
    // B operand of S^T = K Q^T : lane (query nl, half hl) holds q[query][hl*C/2 + p], p < C/2
    float qb[SS ? 1 : CH];
    uint4 qf[SS ? C / 16 : 1][3];      // SS: B fragments, K step s = channels 16 s + 8 hl + j
    const float qs = scale * kLog2e;   // scores live in the log2 domain: softmax through v_exp_f32 (2^x) directly
    if constexpr (SS) {
        const float *qp = q + row(qclamp) * C + 8 * hl;
#pragma unroll
        for (int st = 0; st < C / 16; ++st) {
            const float4 t0 = *reinterpret_cast<const float4 *>(qp + 16 * st), t1 = *reinterpret_cast<const float4 *>(qp + 16 * st + 4);
            const float x[8] = {t0.x * qs, t0.y * qs, t0.z * qs, t0.w * qs, t1.x * qs, t1.y * qs, t1.z * qs, t1.w * qs};
            split3x8(x, qf[st][0], qf[st][1], qf[st][2]);
        }
    } else {
        const float *qp = q + row(qclamp) * C + hl * CH;
#pragma unroll
        for (int i = 0; i < CH / 4; ++i) {
            const float4 t = *reinterpret_cast<const float4 *>(qp + 4 * i);
            qb[4 * i] = t.x * qs; qb[4 * i + 1] = t.y * qs; qb[4 * i + 2] = t.z * qs; qb[4 * i + 3] = t.w * qs;
        }
    }
    const int qreg = region ? region[tb + qclamp] : 0;

    float4 kpre[KV4], vpre[VV4];
    int rpre = 0;
    // rows of the keys this thread stages, looked up ONE TILE AHEAD of the data loads that use them (a dependent
    // index -> data load pair inside fetch() would double the latency the MFMAs of one tile have to hide)
    size_t krow[KV4], vrow[CV >= 32 ? VV4 : 1];
    auto fetch_rows = [&](int j0) {
#pragma unroll
        for (int i = 0; i < KV4; ++i) {
            const int key = (tid + i * 256) / (C / 4);
            krow[i] = kvrow(j0 + key < L ? j0 + key : L - 1);
        }
        if constexpr (CV >= 32) {
#pragma unroll
            for (int i = 0; i < VV4; ++i) {
                const int key = (tid + i * 256) / (CV / 4);
                vrow[i] = kvrow(j0 + key < L ? j0 + key : L - 1);
            }
        }
    };
    auto fetch = [&](int j0) {
#pragma unroll
        for (int i = 0; i < KV4; ++i) {
            const int f = tid + i * 256, key = f / (C / 4), c4 = f - key * (C / 4);
            kpre[i] = (j0 + key < L) ? *reinterpret_cast<const float4 *>(k + krow[i] * C + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if constexpr (CV >= 32) {
#pragma unroll
            for (int i = 0; i < VV4; ++i) {
                const int f = tid + i * 256, key = f / (CV / 4), c4 = f - key * (CV / 4);
                vpre[i] = (j0 + key < L) ? *reinterpret_cast<const float4 *>(v + vrow[i] * CV + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else if constexpr (CV == 2) {
            if (tid < 16) {   // 32 keys x 2 channels = 16 float4
                const int key = 2 * tid;
                float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
                if constexpr (MAP) {
                    if (j0 + key < L) { const float2 u = *reinterpret_cast<const float2 *>(v + kvrow(j0 + key) * 2); t.x = u.x; t.y = u.y; }
                    if (j0 + key + 1 < L) { const float2 u = *reinterpret_cast<const float2 *>(v + kvrow(j0 + key + 1) * 2); t.z = u.x; t.w = u.y; }
                } else if (j0 + key + 1 < L) t = *reinterpret_cast<const float4 *>(v + (tb + j0 + key) * 2);
                else if (j0 + key < L) { const float2 u = *reinterpret_cast<const float2 *>(v + (tb + j0 + key) * 2); t.x = u.x; t.y = u.y; }
                vpre[0] = t;
            }
        }
        if (region && tid < 32) rpre = (j0 + tid < L) ? region[tb + j0 + tid] : 0;
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < KV4; ++i) {
            const int f = tid + i * 256, key = f / (C / 4), c4 = f - key * (C / 4);
            if constexpr (SS) {
                unsigned int h0, m0, l0, h1, m1, l1;
                split3x2(kpre[i].x, kpre[i].y, h0, m0, l0);
                split3x2(kpre[i].z, kpre[i].w, h1, m1, l1);
                unsigned char *kd = reinterpret_cast<unsigned char *>(Ks) + key * SROW + 8 * c4;
                *reinterpret_cast<uint2 *>(kd) = make_uint2(h0, h1);
                *reinterpret_cast<uint2 *>(kd + 32 * SROW) = make_uint2(m0, m1);
                *reinterpret_cast<uint2 *>(kd + 64 * SROW) = make_uint2(l0, l1);
            } else {
                *reinterpret_cast<float4 *>(Ks + key * KLD + 4 * c4) = kpre[i];
            }
        }
        if constexpr (PVS) {
#pragma unroll
            for (int i = 0; i < VV4; ++i) {
                const int f = tid + i * 256, key = f / (CV / 4), c4 = f - key * (CV / 4);
                unsigned int h0, m0, l0, h1, m1, l1;
                split3x2(vpre[i].x, vpre[i].y, h0, m0, l0);
                split3x2(vpre[i].z, vpre[i].w, h1, m1, l1);
                unsigned char *vd = reinterpret_cast<unsigned char *>(Vs) + key * VROWB + 8 * c4;
                *reinterpret_cast<uint2 *>(vd) = make_uint2(h0, h1);
                *reinterpret_cast<uint2 *>(vd + 32 * VROWB) = make_uint2(m0, m1);
                *reinterpret_cast<uint2 *>(vd + 64 * VROWB) = make_uint2(l0, l1);
            }
        } else if constexpr (CV >= 32) {
#pragma unroll
            for (int i = 0; i < VV4; ++i) {
                const int f = tid + i * 256, key = f / (CV / 4), c4 = f - key * (CV / 4);
                *reinterpret_cast<float4 *>(Vs + key * VLD + 4 * c4) = vpre[i];
            }
        } else if constexpr (CV == 2) {
            if (tid < 16) *reinterpret_cast<float4 *>(Vs + 4 * tid) = vpre[0];   // Vs[key*2 + ch]
        }
        if (region && tid < 32) Rs[tid] = rpre;
    };

    float m_run = -INFINITY, l_run = 0.f;
    f32x16 o[NVT];
    float o2x = 0.f, o2y = 0.f;
    if constexpr (CV >= 32) {
#pragma unroll
        for (int j = 0; j < NVT; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) o[j][r] = 0.f;
    }
    // key split (gridDim.z > 1): this workgroup attends its queries to keys [jb, je) only and leaves the unnormalised
    // partial (o, max, sum) in `part`; attention_combine_kernel merges the splits.  Fills the chip when batch*len/128
    // workgroups would not (global matching: 56 of them on 256 CUs).
    const int nsplit = gridDim.z, split = blockIdx.z;
    const int kchunk = ((L + nsplit - 1) / nsplit + 31) & ~31;
    const int jb = split * kchunk, je = (jb + kchunk < L) ? jb + kchunk : L;
    fetch_rows(jb);
    fetch(jb);
    fetch_rows(jb + 32);
    stage();
    __syncthreads();
    for (int j0 = jb; j0 < je; j0 += 32) {
        const bool more = j0 + 32 < je;
        if (more) {
            fetch(j0 + 32);
            fetch_rows(j0 + 64);
        }
        // ---- S^T tile: A = K rows (key nl) from LDS, B = Q.  LDS operand reads run one group ahead of the MFMAs that
        //      consume them (a single wave per SIMD lives here: nothing else would hide the LDS latency) ----
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        if constexpr (SS) {
            const unsigned char *kp = reinterpret_cast<const unsigned char *>(Ks) + nl * SROW + 16 * hl;
            uint4 ac[3], an[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) ac[p] = *reinterpret_cast<const uint4 *>(kp + p * 32 * SROW);
#pragma unroll
            for (int st = 0; st < C / 16; ++st) {
                if (st + 1 < C / 16) {
#pragma unroll
                    for (int p = 0; p < 3; ++p) an[p] = *reinterpret_cast<const uint4 *>(kp + p * 32 * SROW + 32 * (st + 1));
                }
                mfma_split6(s, ac, qf[st]);
#pragma unroll
                for (int p = 0; p < 3; ++p) ac[p] = an[p];
            }
        } else {
        const float *kp = Ks + nl * KLD + hl * CH;
        float4 tc = *reinterpret_cast<const float4 *>(kp), tn = tc;
#pragma unroll
        for (int i = 0; i < CH / 4; ++i) {
            if (i + 1 < CH / 4) tn = *reinterpret_cast<const float4 *>(kp + 4 * (i + 1));
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(tc.x, qb[4 * i], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(tc.y, qb[4 * i + 1], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(tc.z, qb[4 * i + 2], s, 0, 0, 0);
            s = __builtin_amdgcn_mfma_f32_32x32x2f32(tc.w, qb[4 * i + 3], s, 0, 0, 0);
            tc = tn;
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // the LDS read of group i+1
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // the MFMAs of group i
        }
        }
        // lane: query nl; s[r] = log2-domain score of key j0 + (r&3)+8(r>>2)+4hl (q carries scale * log2(e))
        if (region) {                                    // shifted-window mask, one uniform branch per tile
            int rk[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) rk[r] = Rs[(r & 3) + 8 * (r >> 2) + 4 * hl];
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] += (rk[r] != qreg) ? -100.0f * kLog2e : 0.0f;
        }
        if (j0 + 32 > L) {                               // ragged last tile
#pragma unroll
            for (int r = 0; r < 16; ++r) s[r] = (j0 + (r & 3) + 8 * (r >> 2) + 4 * hl < L) ? s[r] : -INFINITY;
        }
        float mx = s[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mx = fmaxf(mx, s[r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));          // the other half of the keys of this query
        const float m_new = fmaxf(m_run, mx);            // finite: key j0 exists and a mask only subtracts 100
        const float corr = __builtin_amdgcn_exp2f(m_run - m_new);   // exp2(-inf) = 0 on the first tile
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float p = __builtin_amdgcn_exp2f(s[r] - m_new);
            s[r] = p;
            psum += p;
        }
        psum += __shfl_xor(psum, 32, 64);
        l_run = l_run * corr + psum;
        m_run = m_new;
        if constexpr (PVS) {
#pragma unroll
            for (int j = 0; j < NVT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[j][r] *= corr;
            // O^T[c][query] += sum_key V[key][c] P[key][query] on the bf16 pipe (three pieces each, six MFMAs per product).
            // B = P: the score tile already has its column (query) on the lane and its rows (keys) in the registers, so the
            // registers 8t .. 8t+7 of a lane ARE its B fragment of K step t (keys 16t + 8(j>>2) + 4hl + (j&3), j = 0..7) --
            // no lane movement.  A = V^T: the same 8 keys of channel nl, i.e. two 4-key column gathers from the row-major
            // [key][channel] image: ds_read_b64_tr_b16 (lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3, and
            // receives its own column of the four rows).
            typedef short s16x4g __attribute__((ext_vector_type(4)));
            typedef __attribute__((address_space(3))) s16x4g *lds_s16x4;
            const unsigned char *vb = reinterpret_cast<const unsigned char *>(Vs) + (4 * hl + ((lane & 15) >> 2)) * VROWB +
                                      (16 * ((lane >> 4) & 1) + 4 * (lane & 3)) * 2;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float x[8] = {s[8 * t], s[8 * t + 1], s[8 * t + 2], s[8 * t + 3], s[8 * t + 4], s[8 * t + 5], s[8 * t + 6], s[8 * t + 7]};
                uint4 pf[3];
                split3x8(x, pf[0], pf[1], pf[2]);
#pragma unroll
                for (int j = 0; j < NVT; ++j) {
                    uint4 vf[3];
#pragma unroll
                    for (int p = 0; p < 3; ++p) {
                        const unsigned char *a = vb + (p * 32 + 16 * t) * VROWB + 64 * j;
                        const s16x4g lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(a));
                        const s16x4g hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(a + 8 * VROWB));
                        const uint2 l2 = __builtin_bit_cast(uint2, lo), h2 = __builtin_bit_cast(uint2, hi);
                        vf[p] = make_uint4(l2.x, l2.y, h2.x, h2.y);
                    }
                    mfma_split6(o[j], vf, pf);
                }
            }
        } else if constexpr (CV >= 32) {
#pragma unroll
            for (int j = 0; j < NVT; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) o[j][r] *= corr;
            // O^T[c][query] += sum_key V[key][c] P[key][query]: k-step r pairs the keys held by the two lane halves
            // in register r (keys kk and kk+4); A = V[key][channel nl of each 32-channel tile] from LDS
            float vc[NVT], vn[NVT];
#pragma unroll
            for (int j = 0; j < NVT; ++j) vc[j] = Vs[(4 * hl) * VLD + nl + 32 * j];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (r + 1 < 16) {
                    const float *vp = Vs + (((r + 1) & 3) + 8 * ((r + 1) >> 2) + 4 * hl) * VLD + nl;
#pragma unroll
                    for (int j = 0; j < NVT; ++j) vn[j] = vp[32 * j];
                }
#pragma unroll
                for (int j = 0; j < NVT; ++j) o[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(vc[j], s[r], o[j], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < NVT; ++j) vc[j] = vn[j];
                __builtin_amdgcn_sched_group_barrier(0x100, (NVT + 1) / 2, 0);   // ds_read2_b32 pairs of step r+1
                __builtin_amdgcn_sched_group_barrier(0x008, NVT, 0);             // the MFMAs of step r
            }
        } else if constexpr (CV == 2) {
            float ax = 0.f, ay = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float2 vv = *reinterpret_cast<const float2 *>(Vs + ((r & 3) + 8 * (r >> 2) + 4 * hl) * 2);
                ax += s[r] * vv.x;
                ay += s[r] * vv.y;
            }
            ax += __shfl_xor(ax, 32, 64);
            ay += __shfl_xor(ay, 32, 64);
            o2x = o2x * corr + ax;
            o2y = o2y * corr + ay;
        }
        __syncthreads();                 // every wave is done with this tile
        if (more) {
            stage();
            __syncthreads();
        }
    }
    if (nsplit > 1) {
        // part: [split][batch][len][CV + 2]
        float *pp = part + (((size_t)split * gridDim.y + b) * L + qclamp) * (CV + 2);
        if (qlive) {
            if constexpr (CV >= 32) {
#pragma unroll
                for (int j = 0; j < NVT; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) pp[j * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl] = o[j][r];
            } else if (CV == 2 && hl == 0) {
                pp[0] = o2x; pp[1] = o2y;
            }
            if (hl == 0) { pp[CV] = m_run; pp[CV + 1] = l_run; }
        }
        return;
    }
    const float inv = 1.0f / l_run;
    if (stats && qlive && hl == 0) {     // row statistics of the softmax (max, sum): used by the column-sum pass
        stats[(tb + qi) * 2] = m_run * kLn2;   // natural-log units for attention_colsum_kernel
        stats[(tb + qi) * 2 + 1] = l_run;
    }
    if constexpr (CV >= 32) {
        // O^T[c][query]: lane = query nl, registers = channels (r&3)+8(r>>2)+4hl of tile j
        if (qlive) {
            float *op = out + row(qi) * CV;
#pragma unroll
            for (int j = 0; j < NVT; ++j)
#pragma unroll
                for (int r = 0; r < 16; r += 4)   // registers r..r+3 are four consecutive channels
                    *reinterpret_cast<float4 *>(op + j * 32 + 8 * (r >> 2) + 4 * hl) =
                        make_float4(o[j][r] * inv, o[j][r + 1] * inv, o[j][r + 2] * inv, o[j][r + 3] * inv);
        }
    } else if constexpr (CV == 2) {
        if (qlive && hl == 0) *reinterpret_cast<float2 *>(out + row(qi) * 2) = make_float2(o2x * inv, o2y * inv);
    }
}

// Merge of the key splits of attention_tokens_kernel: out = sum_z o_z e^(m_z - M) / sum_z l_z e^(m_z - M).
// grid = ceil(batch*len*CV / 256); one thread per output element.
__global__ __launch_bounds__(256) void attention_combine_kernel(const float *__restrict__ part, const int *__restrict__ rowmap,
                                                                float *__restrict__ out, long long tokens, int CV, int nsplit) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= tokens * CV) return;
    const long long t = e / CV;
    const int ch = (int)(e - t * CV);
    const size_t zs = (size_t)tokens * (CV + 2);
    const float *p = part + (size_t)t * (CV + 2);
    float M = -INFINITY;
    for (int z = 0; z < nsplit; ++z) M = fmaxf(M, p[z * zs + CV]);
    float num = 0.f, den = 0.f;
    for (int z = 0; z < nsplit; ++z) {
        const float m = p[z * zs + CV];
        const float wgt = (m == -INFINITY) ? 0.f : exp2f(m - M);   // the partial maxima are log2-domain scores
        num += wgt * p[z * zs + ch];
        den += wgt * p[z * zs + CV + 1];
    }
    const size_t row = rowmap ? (size_t)rowmap[t] : (size_t)t;
    out[row * CV + ch] = num / den;
}

// Column sums of a row-softmax, given its row statistics: colsum[b][j] = sum_i exp(scale q_i.k_j - m_i) / l_i
// (pasmnet/utils.py:31,34: att_left2right.sum(dim=-2)).  One wave per 32 keys; the score tile is computed in the
// natural orientation (queries on the MFMA rows = registers, the key on the lane), so the sum over queries is a
// sum over registers plus one cross-half shuffle, in a fixed order (deterministic).
template <int C>
__global__ __launch_bounds__(256) void attention_colsum_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                               const float *__restrict__ stats, float *__restrict__ colsum, int L,
                                                               float scale) {
    constexpr int QV4 = (32 * C / 4) / 256;         // float4 per thread of one query tile
    // The 4 waves of a workgroup hold 4 x 32 keys of the SAME row and sweep the same queries: every 32-query tile of Q
    // and its (max, 1/sum) statistics are fetched once per workgroup (next tile in flight in registers), staged in LDS
    // and read from there as the MFMA A operand.  Scores live in the log2 domain: p = exp2(s' - m') * (1/l).
    constexpr int SROW = kSsRow(C);                 // Q tile as [piece][query][C] bf16 (split-bf16 scores, see mfma_split6)
    __shared__ __attribute__((aligned(16))) unsigned char Qs[3 * 32 * SROW];
    __shared__ float2 Ms[32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = lane & 31, hl = lane >> 5;
    const int b = blockIdx.y;
    const int j0 = (blockIdx.x * 4 + wave) * 32;
    const size_t tb = (size_t)b * L;
    const int kj = j0 + nl;
    uint4 kf[C / 16][3];                            // B fragments: this lane's key row (a workgroup's surplus waves clamp)
    {
        const float qs = scale * kLog2e;
        const float *kp = k + (tb + (kj < L ? kj : L - 1)) * C + 8 * hl;
#pragma unroll
        for (int st = 0; st < C / 16; ++st) {
            const float4 t0 = *reinterpret_cast<const float4 *>(kp + 16 * st), t1 = *reinterpret_cast<const float4 *>(kp + 16 * st + 4);
            const float x[8] = {t0.x * qs, t0.y * qs, t0.z * qs, t0.w * qs, t1.x * qs, t1.y * qs, t1.z * qs, t1.w * qs};
            split3x8(x, kf[st][0], kf[st][1], kf[st][2]);
        }
    }
    float4 qpre[QV4];
    float2 mpre = make_float2(0.f, 0.f);
    auto fetch = [&](int i0) {
#pragma unroll
        for (int i = 0; i < QV4; ++i) {
            const int f = tid + i * 256, qq = f / (C / 4), c4 = f - qq * (C / 4);
            qpre[i] = (i0 + qq < L) ? *reinterpret_cast<const float4 *>(q + (tb + i0 + qq) * C + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        if (tid < 32) {
            // an out-of-range query contributes exp2(0 - inf) * 0 = 0
            mpre = (i0 + tid < L) ? *reinterpret_cast<const float2 *>(stats + (tb + i0 + tid) * 2) : make_float2(INFINITY, INFINITY);
        }
    };
    auto stage = [&]() {
#pragma unroll
        for (int i = 0; i < QV4; ++i) {
            const int f = tid + i * 256, qq = f / (C / 4), c4 = f - qq * (C / 4);
            unsigned int h0, m0, l0, h1, m1, l1;
            split3x2(qpre[i].x, qpre[i].y, h0, m0, l0);
            split3x2(qpre[i].z, qpre[i].w, h1, m1, l1);
            unsigned char *qd = Qs + qq * SROW + 8 * c4;
            *reinterpret_cast<uint2 *>(qd) = make_uint2(h0, h1);
            *reinterpret_cast<uint2 *>(qd + 32 * SROW) = make_uint2(m0, m1);
            *reinterpret_cast<uint2 *>(qd + 64 * SROW) = make_uint2(l0, l1);
        }
        if (tid < 32) Ms[tid] = make_float2(mpre.x * kLog2e, 1.0f / mpre.y);   // (max in log2 units, 1 / sum)
    };
    float acc = 0.f;
    fetch(0);
    stage();
    __syncthreads();
    for (int i0 = 0; i0 < L; i0 += 32) {
        const bool more = i0 + 32 < L;
        if (more) fetch(i0 + 32);
        f32x16 s;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
        const unsigned char *qp = Qs + nl * SROW + 16 * hl;
        uint4 ac[3], an[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) ac[p] = *reinterpret_cast<const uint4 *>(qp + p * 32 * SROW);
#pragma unroll
        for (int st = 0; st < C / 16; ++st) {
            if (st + 1 < C / 16) {
#pragma unroll
                for (int p = 0; p < 3; ++p) an[p] = *reinterpret_cast<const uint4 *>(qp + p * 32 * SROW + 32 * (st + 1));
            }
            mfma_split6(s, ac, kf[st]);
#pragma unroll
            for (int p = 0; p < 3; ++p) ac[p] = an[p];
        }
        // lane: key nl; s[r] = log2-domain score of query i0 + (r&3)+8(r>>2)+4hl
        float2 ml[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) ml[r] = Ms[(r & 3) + 8 * (r >> 2) + 4 * hl];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc = fmaf(__builtin_amdgcn_exp2f(s[r] - ml[r].x), ml[r].y, acc);
        __syncthreads();                 // every wave is done with this tile
        if (more) {
            stage();
            __syncthreads();
        }
    }
    acc += __shfl_xor(acc, 32, 64);
    if (hl == 0 && kj < L) colsum[tb + kj] = acc;
}

}  // namespace ct

// -------------------------------------------------------------------------------------------------
// C ABI (include/ct_hip.h)
// -------------------------------------------------------------------------------------------------
extern "C" {

int ct_nchw_to_rows_f32(const float *nchw, float *rows, int batch, int c, int h, int w, long long nchw_bstride, int row_channels,
                        int c0, void *stream) {
    if (!nchw || !rows || batch < 0 || c < 1 || h < 1 || w < 1 || c0 < 0 || c0 + c > row_channels) return CT_E_BADARG;
    if (batch == 0) return CT_OK;
    hipLaunchKernelGGL((ct::rows_transpose_kernel<true>), dim3((w + 63) / 64, batch * h), dim3(256), 0, (hipStream_t)stream, nchw,
                       rows, c, h, w, nchw_bstride, row_channels, c0);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_rows_to_nchw_f32(const float *rows, float *nchw, int batch, int c, int h, int w, long long nchw_bstride, int row_channels,
                        int c0, void *stream) {
    if (!nchw || !rows || batch < 0 || c < 1 || h < 1 || w < 1 || c0 < 0 || c0 + c > row_channels) return CT_E_BADARG;
    if (batch == 0) return CT_OK;
    hipLaunchKernelGGL((ct::rows_transpose_kernel<false>), dim3((w + 63) / 64, batch * h), dim3(256), 0, (hipStream_t)stream, rows,
                       nchw, c, h, w, nchw_bstride, row_channels, c0);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

size_t ct_attention_workspace_bytes(int batch, int len, int cv, int nsplit) {
    if (batch < 0 || len < 0 || cv < 0 || nsplit < 2) return 0;
    return (size_t)nsplit * batch * len * (cv + 2) * sizeof(float);
}

int ct_attention_tokens_f32(const float *q, const float *k, const float *v, const int *region, const int *rowmap, float *out,
                            int batch, int len, int cv, float scale, int nsplit, float *ws, size_t ws_bytes, long long kv_shift,
                            void *stream) {
    if (!q || !k || !v || !out || batch < 0 || len < 1 || (cv != 2 && cv != 128) || nsplit < 1 || nsplit > 64) return CT_E_BADARG;
    const long long kv_total = (long long)batch * len;
    if (kv_shift < 0 || kv_shift >= (kv_total > 0 ? kv_total : 1) || (kv_shift != 0 && !rowmap)) return CT_E_BADARG;
    if (nsplit > 1 && (!ws || ws_bytes < ct_attention_workspace_bytes(batch, len, cv, nsplit))) return CT_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out)) & 15) return CT_E_ALIGN;
    if (batch == 0) return CT_OK;
    dim3 grid((len + 127) / 128, batch, nsplit);
    float *nostats = nullptr;
#define CT_ATT(CVV, MAPPED) hipLaunchKernelGGL((ct::attention_tokens_kernel<128, CVV, MAPPED, true>), grid, dim3(256), 0, (hipStream_t)stream, q, k, v, region, rowmap, out, nostats, len, scale, ws, kv_shift, kv_total)
    if (ct::attention16_enabled()) ct::attention16_tokens128(q, k, v, region, rowmap, out, batch, len, cv, scale, nsplit, ws, kv_shift, kv_total, (hipStream_t)stream);
    else if (cv == 128) { if (rowmap) CT_ATT(128, true); else CT_ATT(128, false); }
    else { if (rowmap) CT_ATT(2, true); else CT_ATT(2, false); }
#undef CT_ATT
    CT_CHECK_LAUNCH();
    if (nsplit > 1) {
        const long long tokens = (long long)batch * len;
        hipLaunchKernelGGL(ct::attention_combine_kernel, dim3((unsigned)((tokens * cv + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                           ws, rowmap, out, tokens, cv, nsplit);
        CT_CHECK_LAUNCH();
    }
    return CT_OK;
}

int ct_attention_rows64_f32(const float *q, const float *k, const float *v, float *out, float *stats, int batch, int len, float scale,
                            void *stream) {
    if (!q || !k || batch < 0 || len < 1 || (v && !out) || (!v && !stats)) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return CT_E_ALIGN;
    if (batch == 0) return CT_OK;
    dim3 grid((len + 127) / 128, batch);
    const int *noreg = nullptr;
    if (v && (reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out)) & 15) return CT_E_ALIGN;
    if (ct::attention16_enabled()) ct::attention16_rows64(q, k, v, out, stats, batch, len, scale, (hipStream_t)stream);
    else if (v) hipLaunchKernelGGL((ct::attention_tokens_kernel<64, 96, false, true>), grid, dim3(256), 0, (hipStream_t)stream, q, k, v, noreg, noreg, out, stats, len, scale, (float *)nullptr);
    else hipLaunchKernelGGL((ct::attention_tokens_kernel<64, 0, false, true>), grid, dim3(256), 0, (hipStream_t)stream, q, k, v, noreg, noreg, out, stats, len, scale, (float *)nullptr);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_attention_colsum64_f32(const float *q, const float *k, const float *stats, float *colsum, int batch, int len, float scale,
                              void *stream) {
    if (!q || !k || !stats || !colsum || batch < 0 || len < 1) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return CT_E_ALIGN;
    if (batch == 0) return CT_OK;
    dim3 grid((len + 127) / 128, batch);
    if (ct::attention16_enabled()) ct::attention16_colsum64(q, k, stats, colsum, batch, len, scale, (hipStream_t)stream);
    else hipLaunchKernelGGL((ct::attention_colsum_kernel<64>), grid, dim3(256), 0, (hipStream_t)stream, q, k, stats, colsum, len, scale);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
