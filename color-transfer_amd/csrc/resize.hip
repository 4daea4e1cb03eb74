// resize.hip -- bicubic resampling of float32 NCHW planes on gfx950: torch.nn.functional.interpolate(mode="bicubic",
// align_corners=False), with and without antialias, as the reference's demo notebook (cell 24) wraps DCMCS3DI in it.
//
// The rule without antialias (torch 2.10, UpSampleKernel.cpp / UpSample.h):
//   s = scale * (o + 0.5) - 0.5,  i = min(floor(s), in - 1),  t = clamp(s - i, 0, 1)
//   taps i-1 .. i+2, each clamped to [0, in-1]; cubic convolution weights with A = -0.75; rows of x-sums weighted in y;
//   nothing clamps the result (it overshoots [0, 1]).
// The rule with antialias (_upsample_bicubic2d_aa; separable, columns first, then rows):
//   center = scale * (o + 0.5),  support = 2 * max(scale, 1),  taps [trunc(center - support + 0.5), trunc(center + support + 0.5))
//   cut (not clamped) to the plane, weight cubic((j - center + 0.5) / max(scale, 1)) with A = -0.5, normalised by their sum.
// `scale` is the SOURCE step per output pixel (1 / scale_factor or in / out): a double argument, and every coordinate, every
// weight and every normalisation here is float64 -- torch's float32 kernel evaluates s in float32, which costs it 1.5e-4 on
// noise at 1080p x 0.75.  Without antialias the 16 taps are accumulated in float64 as well and rounded once
// (v_fma_f64 runs at the float32 rate on this part), so the result is the float64 one rounded to float32; the antialias passes
// round their weights to float32 and accumulate with fmaf.
//
// Streaming: the source plane is small next to the cache and its taps overlap between neighbours, so HBM sees one read of the
// input and the output write.  Where the output width is a multiple of 4 and the base sits on 16 bytes, a lane owns 4
// consecutive output columns and stores them as one dwordx4; any other width or base takes the same rule one element per lane.
// Every tap index is clamped or cut to the plane before it is used: no read leaves `in`, no write leaves `out`.
#include "ct_common.h"

namespace ct {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kAaMaxTaps = 128;      // antialias taps per output pixel and axis: ceil(2 * scale) * 2 + 1 (a 31-fold reduction)

// the two pieces of the cubic convolution kernel, |x| <= 1 and 1 < |x| < 2 (UpSample.h: cubic_convolution1 / 2)
__device__ __forceinline__ double cubic1(double x, double a) { return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0; }
__device__ __forceinline__ double cubic2(double x, double a) { return ((a * x - 5.0 * a) * x + 8.0 * a) * x - 4.0 * a; }

// output index o -> the four clamped taps and their weights (A = -0.75)
__device__ __forceinline__ void cubic_taps(int o, double scale, int in_size, int (&idx)[4], double (&wt)[4]) {
    const double a = -0.75;
    const double s = scale * ((double)o + 0.5) - 0.5;
    const double f = fmin(fmax(floor(s), -2.0), (double)(in_size - 1));      // s >= -0.5 for any scale > 0; bounded before the cast
    const int i = (int)f;
    const double t = fmin(fmax(s - f, 0.0), 1.0);
    wt[0] = cubic2(t + 1.0, a);
    wt[1] = cubic1(t, a);
    wt[2] = cubic1(1.0 - t, a);
    wt[3] = cubic2(2.0 - t, a);
#pragma unroll
    for (int k = 0; k < 4; ++k) idx[k] = min(max(i - 1 + k, 0), in_size - 1);
}

// A workgroup is 64 lanes of output columns (VEC columns each) by 4 waves of output rows; blockIdx.y strides over the rows of
// all planes.  VEC == 4 needs wo % 4 == 0 and a 16-byte aligned `out`.
template <int VEC>
__global__ __launch_bounds__(kBlock) void bicubic_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t rows_out,
                                                         int h, int w, int ho, int wo, double scale_h, double scale_w) {
    const int cx = blockIdx.x * kWave + (threadIdx.x & (kWave - 1));
    if (cx * VEC >= wo) return;
    int ix[VEC][4];
    double wx[VEC][4];
#pragma unroll
    for (int v = 0; v < VEC; ++v) cubic_taps(cx * VEC + v, scale_w, w, ix[v], wx[v]);
    for (int64_t r = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6); r < rows_out; r += (int64_t)gridDim.y * 4) {
        const int64_t p = r / ho;
        const int oy = (int)(r - p * ho);
        int iy[4];
        double wy[4];
        cubic_taps(oy, scale_h, h, iy, wy);
        const float *plane = in + p * h * w;
        double acc[VEC];
#pragma unroll
        for (int v = 0; v < VEC; ++v) acc[v] = 0.0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float *row = plane + (int64_t)iy[k] * w;
#pragma unroll
            for (int v = 0; v < VEC; ++v) {
                double s = wx[v][0] * (double)row[ix[v][0]];
                s = fma(wx[v][1], (double)row[ix[v][1]], s);
                s = fma(wx[v][2], (double)row[ix[v][2]], s);
                s = fma(wx[v][3], (double)row[ix[v][3]], s);
                acc[v] = fma(wy[k], s, acc[v]);
            }
        }
        float *dst = out + r * wo + (int64_t)cx * VEC;
        if constexpr (VEC == 4) {
            f32x4 o;
            o.x = (float)acc[0]; o.y = (float)acc[1]; o.z = (float)acc[2]; o.w = (float)acc[3];
            *reinterpret_cast<f32x4 *>(dst) = o;
        } else {
            dst[0] = (float)acc[0];
        }
    }
}

// ---- antialias ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double aa_filter(double x) {
    const double a = -0.5;
    x = fabs(x);
    if (x < 1.0) return cubic1(x, a);
    if (x < 2.0) return cubic2(x, a);
    return 0.0;
}

// _compute_indices_min_size_weights_aa: first tap and tap count of output index o (the casts truncate towards zero there; the
// bounds are applied before the cast here, which gives the same integers and keeps any scale inside int range)
__device__ __forceinline__ void aa_span(int o, double scale, double support, int in_size, int kmax, int &first, int &count, double &center) {
    center = scale * ((double)o + 0.5);
    first = (int)fmin(fmax(center - support + 0.5, 0.0), (double)in_size);
    const int last = (int)fmin(fmax(center + support + 0.5, 0.0), (double)in_size);
    count = min(max(last - first, 0), kmax);
}

__device__ __forceinline__ double aa_weight(int j, int first, double center, double invscale) {
    return aa_filter(((double)(j + first) - center + 0.5) * invscale);
}

// columns: in [rows][w] -> tmp [rows][wo].  A workgroup owns 64 output columns: wave 0 builds their taps and normalised weights
// in LDS once ([kmax][64] floats, lane-major: no bank conflicts), then the 4 waves stride over the rows.
__global__ __launch_bounds__(kBlock) void aa_columns_kernel(const float *__restrict__ in, float *__restrict__ tmp, int64_t rows, int w,
                                                            int wo, double scale, double support, double invscale, int kmax) {
    extern __shared__ float lds[];
    float *wt = lds;                                              // [kmax][64]
    int *first_s = reinterpret_cast<int *>(lds + kmax * kWave);   // [64]
    int *count_s = first_s + kWave;                               // [64]
    const int lane = threadIdx.x & (kWave - 1);
    const int ox = blockIdx.x * kWave + lane;
    if (threadIdx.x < kWave) {
        int first = 0, count = 0;
        double center = 0.0;
        if (ox < wo) aa_span(ox, scale, support, w, kmax, first, count, center);
        double total = 0.0;
        for (int j = 0; j < count; ++j) total += aa_weight(j, first, center, invscale);
        const double norm = total != 0.0 ? 1.0 / total : 1.0;
        for (int j = 0; j < count; ++j) wt[j * kWave + lane] = (float)(aa_weight(j, first, center, invscale) * norm);
        first_s[lane] = first;
        count_s[lane] = count;
    }
    __syncthreads();
    if (ox >= wo) return;
    const int first = first_s[lane], count = count_s[lane];       // first + count <= w
    for (int64_t r = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.y * 4) {
        const float *src = in + r * w + first;
        float acc = 0.0f;
        for (int j = 0; j < count; ++j) acc = fmaf(wt[j * kWave + lane], src[j], acc);
        tmp[r * wo + ox] = acc;
    }
}

// rows: tmp [planes][h][wo] -> out [planes][ho][wo].  blockIdx.y strides over the output rows (one set of weights per row, built
// by the first `count` lanes), blockIdx.z over the planes; a lane owns VEC consecutive columns.  VEC == 4 needs wo % 4 == 0 and
// 16-byte aligned tmp and out.
template <int VEC>
__global__ __launch_bounds__(kBlock) void aa_rows_kernel(const float *__restrict__ tmp, float *__restrict__ out, int64_t planes, int h,
                                                         int ho, int wo, double scale, double support, double invscale, int kmax) {
    __shared__ double raw[kAaMaxTaps];
    __shared__ float wt[kAaMaxTaps];
    const int cx = blockIdx.x * kBlock + threadIdx.x;
    const int tid = threadIdx.x;
    for (int oy = blockIdx.y; oy < ho; oy += gridDim.y) {         // uniform trip count: the barriers below are reached by all
        int first, count;
        double center;
        aa_span(oy, scale, support, h, kmax, first, count, center);
        __syncthreads();                                           // the previous row's readers are done with wt
        if (tid < count) raw[tid] = aa_weight(tid, first, center, invscale);
        __syncthreads();
        if (tid < count) {
            double total = 0.0;
            for (int j = 0; j < count; ++j) total += raw[j];
            wt[tid] = (float)(raw[tid] * (total != 0.0 ? 1.0 / total : 1.0));
        }
        __syncthreads();
        if (cx * VEC >= wo) continue;
        for (int64_t p = blockIdx.z; p < planes; p += gridDim.z) {
            const float *src = tmp + (p * h + first) * wo + (int64_t)cx * VEC;
            float *dst = out + (p * ho + oy) * wo + (int64_t)cx * VEC;
            if constexpr (VEC == 4) {
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int j = 0; j < count; ++j) {
                    const f32x4 a = *reinterpret_cast<const f32x4 *>(src + (int64_t)j * wo);
                    const float c = wt[j];
                    acc.x = fmaf(c, a.x, acc.x); acc.y = fmaf(c, a.y, acc.y); acc.z = fmaf(c, a.z, acc.z); acc.w = fmaf(c, a.w, acc.w);
                }
                *reinterpret_cast<f32x4 *>(dst) = acc;
            } else {
                float acc = 0.0f;
                for (int j = 0; j < count; ++j) acc = fmaf(wt[j], src[(int64_t)j * wo], acc);
                dst[0] = acc;
            }
        }
    }
}

// torch's filter support and tap bound for one axis; false when the reduction is beyond kAaMaxTaps
static bool aa_axis(double scale, double &support, double &invscale, int &kmax) {
    support = scale >= 1.0 ? 2.0 * scale : 2.0;
    invscale = scale >= 1.0 ? 1.0 / scale : 1.0;
    if (!(support <= kAaMaxTaps)) return false;
    kmax = (int)ceil(support) * 2 + 1;
    return kmax <= kAaMaxTaps;
}

static unsigned stride_grid(int64_t items, unsigned other) {
    int64_t cap = target_blocks() / (other > 0 ? other : 1);
    if (cap < 8) cap = 8;
    if (cap > 65535) cap = 65535;
    return (unsigned)(items < 1 ? 1 : items < cap ? items : cap);
}

}  // namespace ct

extern "C" {

size_t ct_bicubic_resize_workspace_bytes(int64_t planes, int h, int wo, int antialias) {
    if (!antialias || planes < 1 || h < 1 || wo < 1) return 0;
    return (size_t)planes * (size_t)h * (size_t)wo * sizeof(float);
}

int ct_bicubic_resize_f32(const float *in, float *out, int64_t planes, int h, int w, int ho, int wo, double scale_h, double scale_w,
                          int antialias, void *ws, size_t ws_bytes, void *stream) {
    if (!in || !out || planes < 1 || h < 1 || w < 1 || ho < 1 || wo < 1) return CT_E_BADARG;
    if (!(scale_h > 0.0) || !(scale_w > 0.0) || !(scale_h <= 1e9) || !(scale_w <= 1e9)) return CT_E_BADARG;   // NaN fails the first
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out)) % sizeof(float)) return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const bool vec = wo % 4 == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    if (!antialias) {
        const int64_t rows_out = planes * ho;
        const unsigned gx = (unsigned)(((vec ? wo / 4 : wo) + ct::kWave - 1) / ct::kWave);
        const dim3 grid(gx, ct::stride_grid((rows_out + 3) / 4, 1));      // no per-workgroup set-up to amortise: one step per row group
        if (vec)
            hipLaunchKernelGGL(ct::bicubic_kernel<4>, grid, dim3(ct::kBlock), 0, s, in, out, rows_out, h, w, ho, wo, scale_h, scale_w);
        else
            hipLaunchKernelGGL(ct::bicubic_kernel<1>, grid, dim3(ct::kBlock), 0, s, in, out, rows_out, h, w, ho, wo, scale_h, scale_w);
        CT_CHECK_LAUNCH();
        return CT_OK;
    }
    double sup_h, inv_h, sup_w, inv_w;
    int k_h, k_w;
    if (!ct::aa_axis(scale_h, sup_h, inv_h, k_h) || !ct::aa_axis(scale_w, sup_w, inv_w, k_w)) return CT_E_BADARG;
    if (!ws || reinterpret_cast<uintptr_t>(ws) % sizeof(float) || ws_bytes < ct_bicubic_resize_workspace_bytes(planes, h, wo, 1))
        return CT_E_WORKSPACE;
    float *tmp = reinterpret_cast<float *>(ws);
    {
        const int64_t rows = planes * h;
        const unsigned gx = (unsigned)((wo + ct::kWave - 1) / ct::kWave);
        const size_t lds = (size_t)k_w * ct::kWave * sizeof(float) + 2 * ct::kWave * sizeof(int);       // <= 33 KiB
        hipLaunchKernelGGL(ct::aa_columns_kernel, dim3(gx, ct::stride_grid((rows + 3) / 4, gx)), dim3(ct::kBlock), lds, s, in, tmp, rows, w,
                           wo, scale_w, sup_w, inv_w, k_w);
        CT_CHECK_LAUNCH();
    }
    {
        const bool vec2 = vec && (reinterpret_cast<uintptr_t>(tmp) & 15) == 0;
        const unsigned gx = (unsigned)(((vec2 ? wo / 4 : wo) + ct::kBlock - 1) / ct::kBlock);
        const unsigned gy = (unsigned)(ho < 65535 ? ho : 65535);
        const dim3 grid(gx, gy, ct::stride_grid(planes, gx * gy));
        if (vec2)
            hipLaunchKernelGGL(ct::aa_rows_kernel<4>, grid, dim3(ct::kBlock), 0, s, tmp, out, planes, h, ho, wo, scale_h, sup_h, inv_h, k_h);
        else
            hipLaunchKernelGGL(ct::aa_rows_kernel<1>, grid, dim3(ct::kBlock), 0, s, tmp, out, planes, h, ho, wo, scale_h, sup_h, inv_h, k_h);
        CT_CHECK_LAUNCH();
    }
    return CT_OK;
}

}  // extern "C"
