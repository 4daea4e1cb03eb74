// linear_u8.hip -- Monge-Kantorovich / Xiao on uint8 frames (gfx950): bytes in, bytes (or float32) out.
//   A3  np.mean + np.cov of k / 255        -> moments_u8_kernel + moments_u8_finish_kernel   (exact integer moments)
//   A5  (k / 255 - mu_t) @ A + mu_r        -> affine_u8_kernel                               (float32 and / or uint8 out, + PSNR)
//   a3  the fused MK entry                 -> the two above around ct_mk_coef_f64 (mk.hip)
//
// The first and second moments of a uint8 image are integers: per image the three sums of k and the six sums of k_i k_j are
// formed as unsigned 64-bit integers, so they do not depend on the order of summation, on the grid or on the batch.  The
// finishing thread forms N * sum(k_i k_j) - sum(k_i) * sum(k_j) exactly in 128-bit integers and rounds three times: the
// conversion to double, the division by N (N - 1) (exact in double for every supported N) and the division by 255^2.
// A constant frame has covariance exactly 0.
//
// A lane owns 16 whole pixels = 48 bytes = three 16-byte loads.  Frame b of a batch starts at b * 3 * n_pixels bytes, off the
// 16-byte grid for most sizes: the first h < 16 pixels of a frame (3 h = -base mod 16) and the last (n_pixels - h) % 16 go
// through a per-pixel path of the same arithmetic, the runs of 16 between them through the vector body.
// Plain stream-ordered launches only; partial sums travel through the workspace.
#include "ct_bytes.h"
#include "ct_linear_u8.h"
#include "ct_metrics.h"
#include "ct_moments.h"
#include "ct_quant.h"
#include "ct_u8_frames.h"

namespace ct {

typedef unsigned long long u64;

// N (N - 1) <= 2^53: the divisor of the covariance is an exact double
constexpr int64_t kMaxPixelsU8 = 94906265;

// NV 64-bit integers per thread -> their block sums in thread 0 (any order gives the same integers)
template <int NV>
__device__ __forceinline__ void block_sum_u64(u64 (&v)[NV], u64 *lds /* [4][NV] */) {
    wave_sum(v);
    const int lane = threadIdx.x & (kWave - 1), wid = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) lds[wid * NV + i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i) v[i] = lds[i] + lds[NV + i] + lds[2 * NV + i] + lds[3 * NV + i];
    }
}

// -------------------------------------------------------------------------------------------
// A3: sum k (3) and sum k_i k_j (6) per image.  grid = (G, n_images); images [0, n_first) at base0, the rest at base1.
// A 32-bit partial covers ONE run of 16 pixels (at most 16 * 255^2 = 1 040 400) and is added to the thread's 64-bit sums
// after every run: no 32-bit sum can overflow, whatever the frame holds.
// -------------------------------------------------------------------------------------------
__device__ __forceinline__ void add_pixel(unsigned int (&t)[9], unsigned int r, unsigned int g, unsigned int b) {
    t[0] += r; t[1] += g; t[2] += b;
    t[3] += r * r; t[4] += r * g; t[5] += r * b;
    t[6] += g * g; t[7] += g * b; t[8] += b * b;
}

__global__ __launch_bounds__(kBlock) void moments_u8_kernel(const uint8_t *__restrict__ base0, const uint8_t *__restrict__ base1,
                                                            int n_first, int64_t n_pixels, u64 *__restrict__ partials) {
    __shared__ u64 lds[4 * 9];
    const int img = blockIdx.y;
    const uint8_t *p = (img < n_first) ? base0 + (size_t)img * n_pixels * 3 : base1 + (size_t)(img - n_first) * n_pixels * 3;
    const int h = head_pixels(p, n_pixels);
    const int64_t n_chunks = (n_pixels - h) >> 4;
    const uint8_t *body = p + 3 * h;
    u64 s[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = 0;
    for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * kBlock) {
        unsigned int w[12], t[9];
        load48(body + c * 48, w);
#pragma unroll
        for (int i = 0; i < 9; ++i) t[i] = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) add_pixel(t, byte_of(w, 3 * k), byte_of(w, 3 * k + 1), byte_of(w, 3 * k + 2));
#pragma unroll
        for (int i = 0; i < 9; ++i) s[i] += t[i];
    }
    // the h pixels before the runs and the < 16 after them: one pixel per lane of workgroup 0
    if (blockIdx.x == 0) {
        const int tail = (int)(n_pixels - h - (n_chunks << 4));
        if ((int)threadIdx.x < h + tail) {
            const int64_t px = (int)threadIdx.x < h ? (int64_t)threadIdx.x : (n_chunks << 4) + threadIdx.x;
            unsigned int t[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) t[i] = 0;
            add_pixel(t, p[px * 3], p[px * 3 + 1], p[px * 3 + 2]);
#pragma unroll
            for (int i = 0; i < 9; ++i) s[i] += t[i];
        }
    }
    block_sum_u64<9>(s, lds);
    if (threadIdx.x == 0) {
        u64 *dst = partials + ((size_t)img * kMaxBlocksPerImage + blockIdx.x) * kPartialStride;
#pragma unroll
        for (int i = 0; i < 9; ++i) dst[i] = s[i];
    }
}

// a signed 128-bit integer -> the nearest double (ties to even): the top 64 bits with everything below them folded into the
// lowest one (it lies below the rounding position of the 53-bit significand), converted once, scaled by a power of two
__device__ inline double i128_to_double(__int128 v) {
    const bool neg = v < 0;
    const unsigned __int128 m = neg ? -(unsigned __int128)v : (unsigned __int128)v;
    const u64 hi = (u64)(m >> 64), lo = (u64)m;
    double d;
    if (hi == 0) {
        d = (double)lo;
    } else {
        const int sh = 64 - __clzll((long long)hi);          // 1 .. 64
        u64 top = sh == 64 ? hi : (hi << (64 - sh)) | (lo >> sh);
        const bool sticky = sh == 64 ? lo != 0 : (lo << (64 - sh)) != 0;
        top |= sticky ? 1ull : 0ull;
        d = ldexp((double)top, sh);
    }
    return neg ? -d : d;
}

// grid = n_images, one workgroup each: adds the G partials and writes the record of the image whose values are k / 255
__global__ __launch_bounds__(kBlock) void moments_u8_finish_kernel(const u64 *__restrict__ partials, int n_blocks, int64_t n_pixels,
                                                                   double *__restrict__ stats) {
    __shared__ u64 lds[4 * 9];
    const int img = blockIdx.x;
    u64 s[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = 0;
    for (int b = threadIdx.x; b < n_blocks; b += kBlock) {
        const u64 *src = partials + ((size_t)img * kMaxBlocksPerImage + b) * kPartialStride;
#pragma unroll
        for (int i = 0; i < 9; ++i) s[i] += src[i];
    }
    block_sum_u64<9>(s, lds);
    if (threadIdx.x == 0) {
        const u64 N = (u64)n_pixels;
        const double n = (double)N, nn1 = (double)(N * (N - (N > 0 ? 1 : 0)));      // N (N - 1) <= 2^53: exact
        double *o = stats + (size_t)img * CT_RGB_STATS_STRIDE;
#pragma unroll
        for (int i = 0; i < 3; ++i) o[i] = (double)s[i] / (255.0 * n);               // sum k <= 255 N < 2^53: one rounding
        auto cov = [&](int i, int j, int k) {                                       // k: where sum k_i k_j sits in s
            const __int128 num = (__int128)N * (__int128)s[k] - (__int128)s[i] * (__int128)s[j];
            return i128_to_double(num) / nn1 / 65025.0;
        };
        const double cxx = cov(0, 0, 3), cxy = cov(0, 1, 4), cxz = cov(0, 2, 5);
        const double cyy = cov(1, 1, 6), cyz = cov(1, 2, 7), czz = cov(2, 2, 8);
        o[3] = cxx; o[4] = cxy; o[5] = cxz;
        o[6] = cxy; o[7] = cyy; o[8] = cyz;
        o[9] = cxz; o[10] = cyz; o[11] = czz;
        o[12] = n; o[13] = 0.0; o[14] = 0.0; o[15] = 0.0;
    }
}

// -------------------------------------------------------------------------------------------
// A5: out = (k / 255 - mu_t) @ A + mu_r: x = (double)k / 255.0 from a 256-entry table, then the px() arithmetic of mk.hip's
// affine3x3_kernel (the same fma order, float64, one rounding to float32).  out_f32 and out_u8 are each optional; the bytes
// are ct_quant.h's rule applied to that float32 value.  With gt the sweep also adds (clamp(out, 0, 1) - gt / 255)^2 in float64,
// gt / 255 by float32 division (a second table), per thread in pixel order, then block_sum's fixed tree: one partial per
// workgroup in sq[img][kMaxBlocksPerImage].  A NaN result stays NaN in that sum (torch.clamp keeps it too).
// in / out_u8 carry no __restrict__: every pixel is read and then written by the same lane.
// -------------------------------------------------------------------------------------------
template <bool F32>   // F32: out_f32 is written (and out_u8 may be); else out_u8 alone
__global__ __launch_bounds__(kBlock) void affine_u8_kernel(const uint8_t *in, const double *__restrict__ coef, float *__restrict__ out_f32,
                                                           uint8_t *out_u8, const uint8_t *__restrict__ gt, double *__restrict__ sq,
                                                           int64_t n_pixels) {
    __shared__ double tab[256];
    __shared__ float tabf[256];
    __shared__ double red[4];
    __shared__ __attribute__((aligned(16))) float xpose[F32 ? 4 * 3072 : 4];   // per wave: the tile of the coalesced float32 store
    tab[threadIdx.x] = (double)threadIdx.x / 255.0;           // kBlock == 256: one entry per thread
    tabf[threadIdx.x] = (float)threadIdx.x / 255.0f;          // IEEE division: the reference's .float() / 255
    __syncthreads();

    const int img = blockIdx.y;
    const size_t off = (size_t)img * n_pixels * 3;
    const uint8_t *p = in + off;
    float *of = F32 ? out_f32 + off : nullptr;
    uint8_t *o8 = out_u8 ? out_u8 + off : nullptr;
    const uint8_t *g = gt ? gt + off : nullptr;
    const double *cf = coef + (size_t)img * 16;
    double A[9], mt[3], mr[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = cf[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { mt[i] = cf[9 + i]; mr[i] = cf[12 + i]; }

    auto px = [&](unsigned int kr, unsigned int kg, unsigned int kb, float &o0, float &o1, float &o2) {
        const double d0 = tab[kr] - mt[0], d1 = tab[kg] - mt[1], d2 = tab[kb] - mt[2];
        // same order as a row-vector @ matrix product: sum over i of d_i A[i][j], then + mu_r
        o0 = (float)(fma(d2, A[6], fma(d1, A[3], d0 * A[0])) + mr[0]);
        o1 = (float)(fma(d2, A[7], fma(d1, A[4], d0 * A[1])) + mr[1]);
        o2 = (float)(fma(d2, A[8], fma(d1, A[5], d0 * A[2])) + mr[2]);
    };
    double acc[1] = {0.0};
    auto sqerr = [&](float v, unsigned int kgt) { acc[0] += sq_err(v, [&] { return tabf[kgt]; }); };

    const int h = head_pixels(p, n_pixels);
    const int64_t n_chunks = (n_pixels - h) >> 4;
    const int64_t b0 = 3 * (int64_t)h;                            // first element of the runs of 16 pixels
    const bool vf = F32 && (reinterpret_cast<uintptr_t>(of + b0) & 15) == 0;
    const bool v8 = o8 && (reinterpret_cast<uintptr_t>(o8 + b0) & 15) == 0;
    const bool vg = g && (reinterpret_cast<uintptr_t>(g + b0) & 15) == 0;
    const int lane = threadIdx.x & (kWave - 1);
    float *lw = xpose + (F32 ? (threadIdx.x >> 6) * 3072 : 0);
    for (int64_t c0 = (int64_t)blockIdx.x * kBlock; c0 < n_chunks; c0 += (int64_t)gridDim.x * kBlock) {
        const int64_t c = c0 + threadIdx.x, wave_c0 = c0 + (threadIdx.x & ~63);
        if (c >= n_chunks) continue;                              // such a wave is not full: it meets no wave barrier below
        // a lane's 48 floats are 192 contiguous bytes: stored directly, every store instruction touches 64 cache lines.  A full
        // wave (wave-uniform) lays its 3072 floats down in a per-wave 12 KiB LDS buffer instead and moves them out as twelve
        // fully coalesced 16-byte stores
        const bool coalesce = F32 && vf && wave_c0 + 64 <= n_chunks;
        const int64_t e0 = b0 + c * 48;
        unsigned int w[12], gw[12], ow[12];
        load48(p + e0, w);
        if (g) {
            if (vg) load48(g + e0, gw);
            else load48_bytes(g + e0, gw);
        }
#pragma unroll
        for (int qd = 0; qd < 4; ++qd) {                          // four pixels = twelve values = three 16-byte vectors of float32
            float v[12];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int e = 12 * qd + 3 * q;
                px(byte_of(w, e), byte_of(w, e + 1), byte_of(w, e + 2), v[3 * q], v[3 * q + 1], v[3 * q + 2]);
            }
            if (F32) {
                if (coalesce) store12<float>(lw + lane * 48 + 12 * qd, true, v);
                else store12<float>(of + e0 + 12 * qd, vf, v);
            }
            if (o8) {
#pragma unroll
                for (int j = 0; j < 3; ++j) ow[3 * qd + j] = pack4(quant_u8(v[4 * j]), quant_u8(v[4 * j + 1]), quant_u8(v[4 * j + 2]), quant_u8(v[4 * j + 3]));
            }
            if (g) {
#pragma unroll
                for (int j = 0; j < 12; ++j) sqerr(v[j], byte_of(gw, 12 * qd + j));
            }
        }
        if (coalesce) {
            __builtin_amdgcn_wave_barrier();
            const float4 *l4 = reinterpret_cast<const float4 *>(lw);
            float4 *go = reinterpret_cast<float4 *>(of + b0 + wave_c0 * 48);
#pragma unroll
            for (int i = 0; i < 12; ++i) go[i * 64 + lane] = l4[i * 64 + lane];
            __builtin_amdgcn_wave_barrier();
        }
        if (o8) {
            if (v8) {
                uint4 *q = reinterpret_cast<uint4 *>(o8 + e0);
                q[0] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
                q[1] = make_uint4(ow[4], ow[5], ow[6], ow[7]);
                q[2] = make_uint4(ow[8], ow[9], ow[10], ow[11]);
            } else {
#pragma unroll
                for (int j = 0; j < 48; ++j) o8[e0 + j] = (uint8_t)byte_of(ow, j);
            }
        }
    }
    // the h pixels before the runs and the < 16 after them: one pixel per lane of workgroup 0
    if (blockIdx.x == 0) {
        const int tail = (int)(n_pixels - h - (n_chunks << 4));
        if ((int)threadIdx.x < h + tail) {
            const int64_t e = 3 * ((int)threadIdx.x < h ? (int64_t)threadIdx.x : (n_chunks << 4) + threadIdx.x);
            float v[3];
            px(p[e], p[e + 1], p[e + 2], v[0], v[1], v[2]);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                if (F32) of[e + j] = v[j];
                if (o8) o8[e + j] = (uint8_t)quant_u8(v[j]);
                if (g) sqerr(v[j], g[e + j]);
            }
        }
    }
    if (g) {                                                      // uniform over the grid
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) sq[(size_t)img * kMaxBlocksPerImage + blockIdx.x] = acc[0];
    }
}

// -------------------------------------------------------------------------------------------
// host-side launchers
// -------------------------------------------------------------------------------------------
static int launch_moments_u8(const uint8_t *base0, const uint8_t *base1, int n_first, int n_images, int64_t n_pixels, u64 *partials,
                             double *stats, hipStream_t s) {
    if (n_images == 0) return CT_OK;
    const int G = blocks_per_image(n_pixels >> 4, n_images);
    hipLaunchKernelGGL(moments_u8_kernel, dim3(G, n_images), dim3(kBlock), 0, s, base0, base1, n_first, n_pixels, partials);
    CT_CHECK_LAUNCH();
    hipLaunchKernelGGL(moments_u8_finish_kernel, dim3(n_images), dim3(kBlock), 0, s, (const u64 *)partials, G, n_pixels, stats);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

// gt != NULL: sq receives *sq_blocks partial sums per frame
static int launch_affine_u8(const uint8_t *in, const double *coef, float *out_f32, uint8_t *out_u8, const uint8_t *gt, double *sq,
                            int *sq_blocks, int64_t n_pixels, int batch, hipStream_t s) {
    const int G = blocks_per_image(n_pixels >> 4, batch);
    if (sq_blocks) *sq_blocks = G;
    if (out_f32) hipLaunchKernelGGL(affine_u8_kernel<true>, dim3(G, batch), dim3(kBlock), 0, s, in, coef, out_f32, out_u8, gt, sq, n_pixels);
    else hipLaunchKernelGGL(affine_u8_kernel<false>, dim3(G, batch), dim3(kBlock), 0, s, in, coef, out_f32, out_u8, gt, sq, n_pixels);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

static int affine_u8_impl(const uint8_t *in, const double *coef, float *out_f32, uint8_t *out_u8, int64_t n_pixels, int batch, void *stream) {
    int rc = check_image_args(in, n_pixels, batch);
    if (rc) return rc;
    if ((rc = out_f32 ? check_image_args(out_f32, n_pixels, batch) : check_image_args(out_u8, n_pixels, batch))) return rc;
    if (batch > 0 && coef == nullptr) return CT_E_BADARG;
    if (batch == 0 || n_pixels == 0) return CT_OK;
    return launch_affine_u8(in, coef, out_f32, out_u8, nullptr, nullptr, nullptr, n_pixels, batch, (hipStream_t)stream);
}

// the workspace of ct_mk_u8: the integer partials and the records of 2 * batch images (ct_moments.h's layout, the partials read
// as 64-bit integers), then the coefficient records and the squared-error partials of the batch
struct WsMkU8 {
    WsLayout l;
    double *coef;   // [batch][16]
    double *sq;     // [batch][kMaxBlocksPerImage]
};

size_t ws_bytes_mk_u8(int batch) {
    if (batch < 0) return 0;
    return ws_bytes_for(2 * batch) + (size_t)batch * (16 + kMaxBlocksPerImage) * sizeof(double);
}

static WsMkU8 ws_carve_mk_u8(void *ws, int batch) {
    WsMkU8 w;
    w.l = ws_carve(ws, 2 * batch);
    w.coef = reinterpret_cast<double *>(reinterpret_cast<char *>(ws) + ws_bytes_for(2 * batch));
    w.sq = w.coef + (size_t)batch * 16;
    return w;
}

}  // namespace ct

// -------------------------------------------------------------------------------------------
// C ABI (include/ct_hip.h)
// -------------------------------------------------------------------------------------------
extern "C" {

int ct_rgb_meancov_u8(const uint8_t *rgb, int64_t n_pixels, int n_images, double *stats, void *ws, size_t ws_bytes, void *stream) {
    int rc = ct::check_image_args(rgb, n_pixels, n_images);
    if (rc) return rc;
    if (n_pixels > ct::kMaxPixelsU8) return CT_E_BADARG;
    if (n_images > 0 && stats == nullptr) return CT_E_BADARG;
    if ((rc = ct::check_ws(ws, ws_bytes, n_images))) return rc;
    return ct::launch_moments_u8(rgb, rgb, n_images, n_images, n_pixels, reinterpret_cast<ct::u64 *>(ct::ws_carve(ws, n_images).partials),
                                 stats, (hipStream_t)stream);
}

int ct_affine3x3_u8_f32(const uint8_t *in, const double *coef, float *out, int64_t n_pixels, int batch, void *stream) {
    return ct::affine_u8_impl(in, coef, out, nullptr, n_pixels, batch, stream);
}
int ct_affine3x3_u8_u8(const uint8_t *in, const double *coef, uint8_t *out, int64_t n_pixels, int batch, void *stream) {
    return ct::affine_u8_impl(in, coef, nullptr, out, n_pixels, batch, stream);
}

int ct_mk_u8(const uint8_t *target, const uint8_t *reference, const uint8_t *gt, float *out_f32, uint8_t *out_u8, double *psnr_out,
             int64_t n_pixels, int batch, int decomposition, void *ws, size_t ws_bytes, void *stream) {
    int rc = ct::check_image_args(target, n_pixels, batch);
    if (rc) return rc;
    if ((rc = ct::check_image_args(reference, n_pixels, batch))) return rc;
    if ((rc = ct::check_u8_outputs(nullptr, nullptr, out_f32, out_u8, nullptr))) return rc;
    if (n_pixels > ct::kMaxPixelsU8 || decomposition < 0 || decomposition > 2) return CT_E_BADARG;
    if ((rc = ct::check_u8_outputs(batch > 0 ? gt : nullptr, nullptr, out_f32, out_u8, psnr_out))) return rc;   // the metric's rule comes last
    if (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < ct::ws_bytes_mk_u8(batch)) return CT_E_WORKSPACE;
    if (batch == 0 || n_pixels == 0) return CT_OK;
    hipStream_t s = (hipStream_t)stream;
    const ct::WsMkU8 w = ct::ws_carve_mk_u8(ws, batch);
    // records [0, batch) = targets, [batch, 2 batch) = references
    rc = ct::launch_moments_u8(target, reference, batch, 2 * batch, n_pixels, reinterpret_cast<ct::u64 *>(w.l.partials), w.l.stats, s);
    if (rc) return rc;
    if ((rc = ct_mk_coef_f64(w.l.stats, w.l.stats + (size_t)batch * CT_RGB_STATS_STRIDE, decomposition, batch, w.coef, stream))) return rc;
    int sq_blocks = 0;
    if ((rc = ct::launch_affine_u8(target, w.coef, out_f32, out_u8, gt, w.sq, &sq_blocks, n_pixels, batch, s))) return rc;
    if (gt == nullptr) return CT_OK;
    return ct::launch_psnr_finish(w.sq, sq_blocks, ct::kMaxBlocksPerImage, n_pixels * 3, batch, psnr_out, s);
}

}  // extern "C"
