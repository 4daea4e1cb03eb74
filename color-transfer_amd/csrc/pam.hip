// pam.hip -- DCMCS3DI's materialised parallax attention on gfx950 (MI355X), exact-float32 MFMA.
//
// Replaces the ATen op sequence B4 of the reference's CNN path:
//   cost = Q.K/c, softmax, warp(att @ V), valid mask (column sums > 0.1)
//   pasmnet/attention.py:39-46, pasmnet/utils.py:30-35,123-125, dcmcs3di.py:58,65
//   -> pam_attend_kernel<MODE> (+ pam_valid_kernel): never writes a [H,W,W] tensor unless the caller asks for the
//      attention maps.  Layout NCHW float32; float32 in, float32 accumulate (v_mfma_f32_32x32x2_f32).
#include "ct_common.h"
#include "ct_split16.h"   // f32x16

namespace ct {

// ---------------------------------------------------------------------------------------------
// Parallax attention for one direction (pasmnet/attention.py:39-46 + utils.py:30-35,123-125).
//   S[i][j] = (1/C) sum_c Q[c][h][i] K[c][h][j] ; P = softmax_j S
//   MODE 0 (attend): out[c][h][i] = sum_j P[i][j] V[c][h][j] for the CV channels of `v` and the 3 of `rgb`
//   MODE 1 (colsum): colpart[h][tile][j] = sum_{i in tile} P[i][j]      (valid mask numerator)
//   optional att[h][i][j] = P (the API's attention map), written only when the pointer is non-null
// grid = (ceil(W/32), H, N), block 256, dynamic LDS = 32*(W+1) floats + V staging
// ---------------------------------------------------------------------------------------------
struct PamArgs {
    const float *q, *k;        // [N][C][H][W]
    const float *v;            // [N][CV][H][W]      (MODE 0)
    const float *rgb;          // [N][3][H][W]       (MODE 0)
    float *out_v, *out_rgb;    // [N][CV][H][W], [N][3][H][W]
    float *colpart;            // [N][H][tiles][W]   (MODE 1)
    float *att;                // nullable [N][H][W][W]
    int C, CV, H, W;
};

constexpr int kPamKC = 128;  // keys staged per S step (one 32-key MFMA tile per wave)
constexpr int kPamJC = 64;   // keys staged per PV step
constexpr int kPamC = 64;    // channels of q/k (DCMCS3DI: channels = 64)

// Cooperative copy of rows [r][j0 .. j0+NCOLS) of a row-major [rows][plane-strided] slab into registers
// (NV4 float4 per thread), 16-byte loads when the row base is aligned, zero fill outside [0,W) x [0,rows).
template <int NROWS, int NCOLS>
struct RowChunk {
    static constexpr int V4_PER_ROW = NCOLS / 4;
    static constexpr int NV4 = (NROWS * V4_PER_ROW + 255) / 256;
    float4 v[NV4];
    // src(r) = row pointer of row r at column 0, or nullptr for a zero row
    template <typename RowPtr>
    __device__ __forceinline__ void fetch(RowPtr src, int j0, int W, bool vec, int tid) {
#pragma unroll
        for (int i = 0; i < NV4; ++i) {
            int f = tid + i * 256;
            asm volatile("" : "+v"(f));
            const int r = f / V4_PER_ROW, g = f - r * V4_PER_ROW;
            const int j = j0 + 4 * g;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            const float *p = (r < NROWS) ? src(r) : nullptr;
            if (p && j < W) {
                if (vec) x = *reinterpret_cast<const float4 *>(p + j);
                else {
                    x.x = p[j];
                    if (j + 1 < W) x.y = p[j + 1];
                    if (j + 2 < W) x.z = p[j + 2];
                    if (j + 3 < W) x.w = p[j + 3];
                }
            }
            v[i] = x;
        }
    }
    // LDS image [NROWS][LD]; LD % 4 == 0 -> one 16-byte store, else four scalar stores
    template <int LD>
    __device__ __forceinline__ void store(float *lds, int tid) const {
#pragma unroll
        for (int i = 0; i < NV4; ++i) {
            const int f = tid + i * 256;
            const int r = f / V4_PER_ROW, g = f - r * V4_PER_ROW;
            if (r < NROWS) {
                float *d = lds + r * LD + 4 * g;
                if (LD % 4 == 0) *reinterpret_cast<float4 *>(d) = v[i];
                else { d[0] = v[i].x; d[1] = v[i].y; d[2] = v[i].z; d[3] = v[i].w; }
            }
        }
    }
};

// TQ = queries per workgroup: 32, or 16 for wide images (one TQ x W tile of S must fit the 160 KiB LDS; the MFMA
// tile stays 32 x 32 with the upper 16 query rows idle)
template <int MODE, int TQ>
__global__ __launch_bounds__(256) void pam_attend_kernel(PamArgs a) {
    extern __shared__ float smem[];
    const int W = a.W, SW = W | 1;                 // odd row stride: column reads are conflict free
    constexpr int VST = kPamJC + 1;                // odd: the PV A-operand reads walk down a column
    float *S = smem;                               // [TQ][SW]
    float *Qs = smem + TQ * SW;                    // [64][TQ]
    float *Ks = Qs + kPamC * TQ;               // [64][128]   (S phase)  /  Vs [96][65] (PV phase), aliased
    float *Vs = Ks;
    const int i0 = blockIdx.x * TQ, h = blockIdx.y, n = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nl = lane & 31, hl = lane >> 5;
    const size_t plane = (size_t)a.H * W;
    const float *q = a.q + (size_t)n * kPamC * plane + (size_t)h * W;
    const float *k = a.k + (size_t)n * kPamC * plane + (size_t)h * W;
    const float inv_c = 1.0f / (float)kPamC;
    const bool vec = (W % 4 == 0) && (((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) == 0);

    // ---- S tile = Q^T K / C : M = query i (A = Q[c][i]), N = key j (B = K[c][j]), K = channels ----
    {
        RowChunk<kPamC, TQ> qc;
        qc.fetch([&](int r) { return q + (size_t)r * plane; }, i0, W, vec, tid);
        RowChunk<kPamC, kPamKC> kc;
        kc.fetch([&](int r) { return k + (size_t)r * plane; }, 0, W, vec, tid);
        qc.template store<TQ>(Qs, tid);
        kc.template store<kPamKC>(Ks, tid);
        __syncthreads();
        float qa[kPamC / 2];                        // this lane's A operands for all 32 k-steps
#pragma unroll
        for (int p = 0; p < kPamC / 2; ++p) qa[p] = (nl < TQ) ? Qs[(2 * p + hl) * TQ + nl] : 0.f;
        for (int j0 = 0; j0 < W; j0 += kPamKC) {
            const bool more = (j0 + kPamKC < W);
            if (more) kc.fetch([&](int r) { return k + (size_t)r * plane; }, j0 + kPamKC, W, vec, tid);   // next chunk in flight
            f32x16 acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.f;
            const float *brow = Ks + hl * kPamKC + wave * 32 + nl;
#pragma unroll
            for (int p = 0; p < kPamC / 2; ++p) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[p], brow[p * 2 * kPamKC], acc, 0, 0, 0);
            // D[i][j]: lane holds key column j, query rows (r&3)+8(r>>2)+4hl
            const int kj = j0 + wave * 32 + nl;
            if (kj < W) {
#pragma unroll
                for (int r = 0; r < TQ / 2; ++r) S[((r & 3) + 8 * (r >> 2) + 4 * hl) * SW + kj] = acc[r] * inv_c;   // rows < TQ
            }
            __syncthreads();                        // everyone is done with this K chunk
            if (more) {
                kc.template store<kPamKC>(Ks, tid);
                __syncthreads();
            }
        }
    }
    // prefetch the first V chunk while the softmax runs (MODE 0)
    const int CT = a.CV + 3;                        // feature channels + the 3 RGB channels of `right`
    const float *v = MODE == 0 ? a.v + (size_t)n * a.CV * plane + (size_t)h * W : nullptr;
    const float *rgb = MODE == 0 ? a.rgb + (size_t)n * 3 * plane + (size_t)h * W : nullptr;
    const bool vecv = MODE == 0 && (W % 4 == 0) &&
                      (((reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(rgb)) & 15) == 0);
    auto vrow = [&](int r) -> const float * {
        return r < a.CV ? v + (size_t)r * plane : (r < CT ? rgb + (size_t)(r - a.CV) * plane : nullptr);
    };
    RowChunk<96, kPamJC> vc;
    if (MODE == 0) vc.fetch(vrow, 0, W, vecv, tid);

    // ---- row softmax (F.softmax(dim=-1)): 8 rows per wave ----
    for (int rr = 0; rr < TQ / 4; ++rr) {
        const int row = wave * (TQ / 4) + rr;
        float *srow = S + row * SW;
        float mx = -INFINITY;
        for (int j = lane; j < W; j += 64) mx = fmaxf(mx, srow[j]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
        float sum = 0.f;
        for (int j = lane; j < W; j += 64) {
            const float e = expf(srow[j] - mx);
            srow[j] = e;
            sum += e;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        const float inv = 1.0f / sum;
        const bool live = (i0 + row) < W;
        for (int j = lane; j < W; j += 64) {
            const float p = live ? srow[j] * inv : 0.f;
            srow[j] = p;
            if (a.att && live) a.att[(((size_t)n * a.H + h) * W + (i0 + row)) * W + j] = p;
        }
    }
    __syncthreads();
    if (MODE == 1) {
        // column sums over this tile's (live) query rows, fixed order
        float *dst = a.colpart + (((size_t)n * a.H + h) * gridDim.x + blockIdx.x) * W;
        for (int j = tid; j < W; j += 256) {
            float s = 0.f;
#pragma unroll
            for (int r = 0; r < TQ; ++r) s += S[r * SW + j];
            dst[j] = s;
        }
        return;
    }
    // ---- out[c][i] = sum_j V[c][j] P[i][j] : M = channel (A = V, staged [c][JC+1]), N = query (B = P) ----
    const int mt_total = (CT + 31) / 32;            // 3 for CV = 64
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    vc.template store<VST>(Vs, tid);
    __syncthreads();
    for (int j0 = 0; j0 < W; j0 += kPamJC) {
        const bool more = (j0 + kPamJC < W);
        if (more) vc.fetch(vrow, j0 + kPamJC, W, vecv, tid);     // next chunk in flight under the MFMAs
        if (wave < mt_total) {
            const float *arow = Vs + (wave * 32 + nl) * VST + hl;
            const float *brow = S + (nl < TQ ? nl : 0) * SW + j0 + hl;
#pragma unroll
            for (int jj = 0; jj < kPamJC; jj += 2) {
                const float bv = (nl < TQ && j0 + jj + hl < W) ? brow[jj] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(arow[jj], bv, acc, 0, 0, 0);
            }
        }
        __syncthreads();
        if (more) {
            vc.template store<VST>(Vs, tid);
            __syncthreads();
        }
    }
    if (wave < mt_total) {
        const int x = i0 + nl;
        if (nl < TQ && x < W) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hl;
                if (c < a.CV) a.out_v[((size_t)n * a.CV + c) * plane + (size_t)h * W + x] = acc[r];
                else if (c < CT) a.out_rgb[((size_t)n * 3 + (c - a.CV)) * plane + (size_t)h * W + x] = acc[r];
            }
        }
    }
}

// valid[n][0][h][j] = (sum over query tiles of colpart) > 0.1, as 0.0 / 1.0 (bool -> float promotion of
// torch.cat, dcmcs3di.py:59); colsum (pre-threshold) is also written for the parity tests.
__global__ void pam_valid_kernel(const float *__restrict__ colpart, int tiles, int H, int W, float *__restrict__ valid,
                                 float *__restrict__ colsum) {
    const int n = blockIdx.z, h = blockIdx.y, j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= W) return;
    const float *p = colpart + (((size_t)n * H + h) * tiles) * W + j;
    float s = 0.f;
    for (int t = 0; t < tiles; ++t) s += p[(size_t)t * W];
    const size_t o = ((size_t)n * H + h) * W + j;
    valid[o] = s > 0.1f ? 1.0f : 0.0f;
    if (colsum) colsum[o] = s;
}

template <int MODE, int TQ>
static int launch_pam_tq(const PamArgs &a, int N, hipStream_t s, size_t lds) {
    static DynLdsAttr attr;             // per instantiation, per device
    {
        hipError_t e = attr.ensure(reinterpret_cast<const void *>(&pam_attend_kernel<MODE, TQ>), lds);
        if (e != hipSuccess) return (int)e;
    }
    dim3 grid((a.W + TQ - 1) / TQ, a.H, N);
    hipLaunchKernelGGL((pam_attend_kernel<MODE, TQ>), grid, dim3(256), lds, s, a);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

static int pam_tq(int W) {   // queries per workgroup such that S (TQ x W) + Q tile + K chunk fit the 160 KiB LDS
    const size_t lds32 = ((size_t)32 * (W | 1) + kPamC * 32 + kPamC * kPamKC) * sizeof(float);
    const size_t lds16 = ((size_t)16 * (W | 1) + kPamC * 16 + kPamC * kPamKC) * sizeof(float);
    if (lds32 <= 160 * 1024) return 32;
    if (lds16 <= 160 * 1024) return 16;
    return 0;
}

template <int MODE>
static int launch_pam(const PamArgs &a, int N, hipStream_t s) {
    static_assert(96 * (kPamJC + 1) <= kPamC * kPamKC, "V chunk must fit the K chunk region");
    if (a.C != kPamC) return CT_E_BADARG;
    const int tq = pam_tq(a.W);
    if (tq == 0) return CT_E_BADARG;   // W > 1983 (32 queries up to W = 959, 16 up to 1983): needs the streaming (online-softmax) variant
    const size_t lds = ((size_t)tq * (a.W | 1) + kPamC * tq + kPamC * kPamKC) * sizeof(float);
    return tq == 32 ? launch_pam_tq<MODE, 32>(a, N, s, lds) : launch_pam_tq<MODE, 16>(a, N, s, lds);
}

}  // namespace ct

extern "C" {

size_t ct_pam_workspace_bytes(int n, int h, int w) {
    if (n < 0 || h < 0 || w < 0) return 0;
    const int tq = ct::pam_tq(w);
    if (tq == 0) return 0;
    return (size_t)n * h * ((w + tq - 1) / tq) * w * sizeof(float);
}

int ct_pam_attend_f32(const float *q, const float *k, const float *v, const float *rgb, float *out_v, float *out_rgb,
                      float *att, int n, int c, int cv, int h, int w, void *stream) {
    if (!q || !k || !v || !rgb || !out_v || !out_rgb || n < 0 || c < 1 || cv < 1 || cv > 93 || h < 0 || w < 0)
        return CT_E_BADARG;
    if (n == 0 || h == 0 || w == 0) return CT_OK;
    ct::PamArgs a;
    a.q = q; a.k = k; a.v = v; a.rgb = rgb; a.out_v = out_v; a.out_rgb = out_rgb; a.colpart = nullptr; a.att = att;
    a.C = c; a.CV = cv; a.H = h; a.W = w;
    return ct::launch_pam<0>(a, n, (hipStream_t)stream);
}

int ct_pam_valid_f32(const float *q, const float *k, float *valid, float *colsum, float *att, int n, int c, int h, int w,
                     void *ws, size_t ws_bytes, void *stream) {
    if (!q || !k || !valid || n < 0 || c < 1 || h < 0 || w < 0) return CT_E_BADARG;
    if (n == 0 || h == 0 || w == 0) return CT_OK;
    if (!ws || ws_bytes < ct_pam_workspace_bytes(n, h, w)) return CT_E_WORKSPACE;
    ct::PamArgs a;
    a.q = q; a.k = k; a.v = nullptr; a.rgb = nullptr; a.out_v = nullptr; a.out_rgb = nullptr;
    a.colpart = reinterpret_cast<float *>(ws); a.att = att;
    a.C = c; a.CV = 0; a.H = h; a.W = w;
    int rc = ct::launch_pam<1>(a, n, (hipStream_t)stream);
    if (rc) return rc;
    const int tiles = (w + ct::pam_tq(w) - 1) / ct::pam_tq(w);
    hipLaunchKernelGGL(ct::pam_valid_kernel, dim3((w + 255) / 256, h, n), dim3(256), 0, (hipStream_t)stream,
                       (const float *)ws, tiles, h, w, valid, colsum);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
