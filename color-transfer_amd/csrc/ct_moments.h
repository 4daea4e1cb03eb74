// ct_moments.h -- what the Reinhard side (linear.hip) and the Monge-Kantorovich side (mk.hip) share: the workspace layout of
// the statistics sweeps, the argument checks of their entries, and the generic (non-table) moments sweep with its launcher.
//
// A sweep is a single coalesced HBM pass: a lane owns 4 whole HWC pixels (48 B of f32) per iteration, moments are reduced
// wave (__shfl_down) -> LDS -> one partial per workgroup -> a tiny finishing kernel, in a fixed order, so results are
// bitwise reproducible run to run (no float atomics).
//
// Moments use the shifted-data form with a common pivot K = value of pixel 0 of the image:
// S1 = sum(x-K), S2 = sum((x-K)(x-K)^T) are plainly additive across lanes/workgroups, and
// mean = K + S1/n, M2 = S2 - S1 S1^T / n is stable in float64 even for near-constant images.
#pragma once
#include "ct_reinhard.h"

namespace ct {

constexpr int kPartialStride = 12;  // doubles per workgroup partial (6 used for Lab, 9 for RGB cov)
constexpr int kPivotStride = 4;

struct WsLayout {
    double *partials;  // [n_images][kMaxBlocksPerImage][kPartialStride]
    double *pivots;    // [n_images][kPivotStride]
    double *stats;     // [n_images][CT_RGB_STATS_STRIDE] (only the fused entries use it)
};

static size_t ws_bytes_for(int n_images) {
    return (size_t)n_images * ((size_t)kMaxBlocksPerImage * kPartialStride + kPivotStride + CT_RGB_STATS_STRIDE) *
           sizeof(double);
}

static WsLayout ws_carve(void *ws, int n_images) {
    WsLayout l;
    l.partials = reinterpret_cast<double *>(ws);
    l.pivots = l.partials + (size_t)n_images * kMaxBlocksPerImage * kPartialStride;
    l.stats = l.pivots + (size_t)n_images * kPivotStride;
    return l;
}

template <typename T>
static int check_image_args(const T *p, int64_t n_pixels, int n_images) {
    if (n_pixels < 0 || n_images < 0) return CT_E_BADARG;
    if (n_images > 0 && n_pixels > 0 && p == nullptr) return CT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(p) % sizeof(T)) return CT_E_ALIGN;
    return CT_OK;
}

static int check_ws(const void *ws, size_t ws_bytes, int n_images) {
    if (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 15)) return CT_E_WORKSPACE;
    if (ws_bytes < ws_bytes_for(n_images)) return CT_E_WORKSPACE;
    return CT_OK;
}

// -------------------------------------------------------------------------------------------
// A1 / A3: first and second moments of Lab (LAB=true, 6 sums) or RGB (LAB=false, 9 sums)
// -------------------------------------------------------------------------------------------

// grid = (G, n_images). Images [0, n_first) live at base0, the rest at base1 (so that the
// targets and references of a batch of pairs are swept by ONE launch).
// No occupancy attribute: forcing 8 waves/SIMD spills and is slower, the kernels are VALU-bound and insensitive to the
// grid (measured r01).
template <typename T, bool LAB>
__global__ __launch_bounds__(kBlock) void moments_kernel(const T *__restrict__ base0, const T *__restrict__ base1,
                                                         int n_first, int64_t n_pixels, double *__restrict__ partials,
                                                         double *__restrict__ pivots) {
    constexpr int NV = LAB ? 6 : 9;
    __shared__ double lds[4 * NV];
    const int img = blockIdx.y;
    const T *p = (img < n_first) ? base0 + (size_t)img * n_pixels * 3 : base1 + (size_t)(img - n_first) * n_pixels * 3;
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15) == 0;

    double k[3] = {0.0, 0.0, 0.0};
    if (n_pixels > 0) to_space<LAB>((double)p[0], (double)p[1], (double)p[2], k[0], k[1], k[2]);

    double s[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) s[i] = 0.0;

    const int64_t n_chunks = n_pixels >> 2;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // register double-buffer: the next chunk's loads are in flight while this one is converted
    int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    Raw12<T> cur, nxt;
    if (c < n_chunks) load12_raw<T>(p + c * 12, vec, cur);
    for (; c < n_chunks; c += stride) {
        if (c + stride < n_chunks) load12_raw<T>(p + (c + stride) * 12, vec, nxt);
        double v[12];
        unpack12<T>(cur, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double x, y, z;
            to_space<LAB>(v[3 * q], v[3 * q + 1], v[3 * q + 2], x, y, z);
            accumulate<LAB>(s, k, x, y, z);
        }
        cur = nxt;
    }
    // ragged tail (n_pixels % 4 pixels): lanes 0..2 of workgroup 0
    if (blockIdx.x == 0) {
        const int64_t px = (n_chunks << 2) + threadIdx.x;
        if (threadIdx.x < 3 && px < n_pixels) {
            double x, y, z;
            to_space<LAB>((double)p[px * 3], (double)p[px * 3 + 1], (double)p[px * 3 + 2], x, y, z);
            accumulate<LAB>(s, k, x, y, z);
        }
    }
    block_sum<NV>(s, lds);
    if (threadIdx.x == 0) {
        double *dst = partials + ((size_t)img * kMaxBlocksPerImage + blockIdx.x) * kPartialStride;
#pragma unroll
        for (int i = 0; i < NV; ++i) dst[i] = s[i];
        if (blockIdx.x == 0) {
            pivots[img * kPivotStride + 0] = k[0];
            pivots[img * kPivotStride + 1] = k[1];
            pivots[img * kPivotStride + 2] = k[2];
        }
    }
}


// grid = n_images, one workgroup each: adds the G partials in a fixed order and writes the record.
template <bool LAB>
__global__ __launch_bounds__(kBlock) void moments_finalize_kernel(const double *__restrict__ partials,
                                                                  const double *__restrict__ pivots, int n_blocks,
                                                                  int64_t n_pixels, double *__restrict__ stats, double var_floor) {
    constexpr int NV = LAB ? 6 : 9;
    __shared__ double lds[4 * NV];
    const int img = blockIdx.x;
    double s[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) s[i] = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += kBlock) {
        const double *src = partials + ((size_t)img * kMaxBlocksPerImage + b) * kPartialStride;
#pragma unroll
        for (int i = 0; i < NV; ++i) s[i] += src[i];
    }
    block_sum<NV>(s, lds);
    if (threadIdx.x == 0) {
        const double n = (double)n_pixels;
        const double *k = pivots + img * kPivotStride;
        const double m0 = s[0] / n, m1 = s[1] / n, m2 = s[2] / n;  // mean of (x - K)
        if (LAB) {
            lab_record(s, k, n, stats + (size_t)img * CT_LAB_STATS_STRIDE, var_floor);
        } else {
            double *o = stats + (size_t)img * CT_RGB_STATS_STRIDE;
            o[0] = k[0] + m0; o[1] = k[1] + m1; o[2] = k[2] + m2;
            const double d = n - 1.0;  // np.cov default ddof = 1
            const double cxx = fma(-s[0], m0, s[3]) / d, cxy = fma(-s[0], m1, s[4]) / d, cxz = fma(-s[0], m2, s[5]) / d;
            const double cyy = fma(-s[1], m1, s[6]) / d, cyz = fma(-s[1], m2, s[7]) / d, czz = fma(-s[2], m2, s[8]) / d;
            o[3] = cxx; o[4] = cxy; o[5] = cxz;
            o[6] = cxy; o[7] = cyy; o[8] = cyz;
            o[9] = cxz; o[10] = cyz; o[11] = czz;
            o[12] = n; o[13] = 0.0; o[14] = 0.0; o[15] = 0.0;
        }
    }
}

// The generic sweep and its finishing kernel.  ev_start / ev_stop: optional events recorded immediately around the sweep
// (linear.hip's profile events; NULL = none).
template <typename T, bool LAB>
static int launch_moments(const T *base0, const T *base1, int n_first, int n_images, int64_t n_pixels, const WsLayout &l,
                          double *stats, hipStream_t s, hipEvent_t ev_start = nullptr, hipEvent_t ev_stop = nullptr) {
    if (n_images == 0) return CT_OK;
    const int G = blocks_per_image(n_pixels >> 2, n_images);
    if (ev_start) (void)hipEventRecord(ev_start, s);
    hipLaunchKernelGGL((moments_kernel<T, LAB>), dim3(G, n_images), dim3(kBlock), 0, s, base0, base1, n_first, n_pixels,
                       l.partials, l.pivots);
    CT_CHECK_LAUNCH();
    if (ev_stop) (void)hipEventRecord(ev_stop, s);
    hipLaunchKernelGGL((moments_finalize_kernel<LAB>), dim3(n_images), dim3(kBlock), 0, s, l.partials, l.pivots, G, n_pixels,
                       stats, 0.0);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // namespace ct
