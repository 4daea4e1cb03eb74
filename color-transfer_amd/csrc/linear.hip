// linear.hip -- the Reinhard transfer (global statistical colour transfer in Lab) on gfx950 (MI355X).
//
// Replaces the numpy/skimage sweeps of the reference's methods/linear.py:
//   A1  rgb2lab + np.mean/np.std          (linear.py:25-26,33-36)  -> lab_moments_lut_kernel / moments_kernel<T, true>
//   A2  affine in Lab + lab2rgb           (linear.py:38-40)        -> reinhard_apply_lut_kernel / reinhard_apply_kernel
// The Monge-Kantorovich side (A3-A5) is mk.hip; the generic moments sweep, the workspace layout and the argument checks both
// share are ct_moments.h; the per-frame PSNR of the fused entry is metrics.hip (ct_metrics.h); the persistent one-launch
// form is reinhard_persist.hip (ct_reinhard_persist.h).
//
// Both sweeps are single coalesced HBM passes, Lab never leaves registers, and every reduction has a fixed order, so
// results are bitwise reproducible run to run (no float atomics).
#include <atomic>

#include "ct_linear_u8.h"
#include "ct_metrics.h"
#include "ct_moments.h"
#include "ct_reinhard_persist.h"

namespace ct {

template <typename T, bool OUT_LAB>
__global__ __launch_bounds__(kBlock) void reinhard_apply_kernel(const T *__restrict__ target, const double *__restrict__ stats_t,
                                                         const double *__restrict__ stats_r, T *__restrict__ out,
                                                         int64_t n_pixels) {
    const int img = blockIdx.y;
    const T *p = target + (size_t)img * n_pixels * 3;
    T *o = out + (size_t)img * n_pixels * 3;
    const bool vec = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(o)) & 15) == 0;
    const ReinhardCoef c = reinhard_coef(stats_t + (size_t)img * CT_LAB_STATS_STRIDE,
                                         stats_r + (size_t)img * CT_LAB_STATS_STRIDE);
    const int64_t n_chunks = n_pixels >> 2;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int64_t ch = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    Raw12<T> cur, nxt;
    if (ch < n_chunks) load12_raw<T>(p + ch * 12, vec, cur);
    for (; ch < n_chunks; ch += stride) {
        if (ch + stride < n_chunks) load12_raw<T>(p + (ch + stride) * 12, vec, nxt);
        double v[12];
        T w[12];
        unpack12<T>(cur, v);
#pragma unroll
        for (int q = 0; q < 4; ++q)
            reinhard_pixel<T, OUT_LAB>(c, v[3 * q], v[3 * q + 1], v[3 * q + 2], w[3 * q], w[3 * q + 1], w[3 * q + 2]);
        store12<T>(o + ch * 12, vec, w);
        cur = nxt;
    }
    if (blockIdx.x == 0) {
        const int64_t px = (n_chunks << 2) + threadIdx.x;
        if (threadIdx.x < 3 && px < n_pixels) {
            T a, b, d;
            reinhard_pixel<T, OUT_LAB>(c, (double)p[px * 3], (double)p[px * 3 + 1], (double)p[px * 3 + 2], a, b, d);
            o[px * 3] = a; o[px * 3 + 1] = b; o[px * 3 + 2] = d;
        }
    }
}

// -------------------------------------------------------------------------------------------
// Table-driven variants of A1 / A2 for float32 images (ct_color_lut.h): the power functions are LDS look-ups.
//
// Work layout: a wave owns TILES of 256 consecutive pixels; lane l holds pixels l, l+64, l+128, l+192 of the tile, each
// fetched / stored with ONE 12-byte access (global_load/store_dwordx3): consecutive lanes touch consecutive bytes, so
// every wave instruction covers 768 contiguous bytes whatever the alignment of the image (measured,
// tools/ubench/stream_patterns.hip: a copy runs at 5.5 TB/s this way against 4.6 TB/s with three 16-byte accesses per lane
// at a 48-byte lane stride).  512-thread workgroups share one 32 KB (statistics) / 37 KB (apply) table image and are
// persistent: one round of resident workgroups sweeps all tiles.  A tile whose wave holds any value outside [0,1] (or a
// NaN) is computed with the exact float64 code of ct_color.h, pixel by pixel.
// -------------------------------------------------------------------------------------------
// minimum waves per SIMD the table kernels are compiled for (their register budget: 128 VGPRs)
constexpr int kLutMinWaves = 4;
// Both keep ONE register tile of prefetch: the next tile's loads are in flight while this one is computed, at one 12-register copy
// per tile.  Two tiles ahead, none at all, and two register sets in alternating roles (no copy, loop unrolled by two: 37.0 k
// pairs/s against 37.5 k, the unrolled loop's registers cost more than the copies) were measured and rejected, like the ablation
// and clock-diagnostic builds of these kernels; they can be read in this file at commit 2036944, DESIGN.md 4.1 has their results.

// A1, float32 arithmetic on the table path (see ct_color_lut.h: statistics only need unbiased per-pixel values): per lane
// float32 shifted sums over its ~40 pixels, converted once to float64 for the fixed-shape reduction tree.  The exact
// fallback (out-of-range tiles, the ragged last tile) accumulates in float64 beside it.
//
// A launch covers any part of the batch: grid row y stands for image img_lo + y (y < y_split) or img_hi + (y - y_split), and every
// index into the partials and pivots is the IMAGE's, so a chunk [p0, p1) of a batch of pairs (y_split = p1 - p0, img_lo = p0,
// img_hi = batch + p0) writes the rows the whole-batch launch (y_split = n_first, img_lo = 0, img_hi = n_first) writes for it.
// T_PLAIN: the rows below y_split (the targets of a pipelined chunk) are read with the default cache policy -- the apply
// sweep of the same chunk re-reads them within the reach of the Infinity Cache -- everything else non-temporal as ever.
template <bool T_PLAIN>
__global__ __launch_bounds__(kLutBlock, kLutMinWaves) void lab_moments_lut_kernel(const float *__restrict__ base0,
                                                                                  const float *__restrict__ base1, int n_first,
                                                                                  int64_t n_pixels, double *__restrict__ partials,
                                                                                  double *__restrict__ pivots, int y_split, int img_lo,
                                                                                  int img_hi) {
    __shared__ __attribute__((aligned(16))) unsigned char tab[lut::kLdsBytesFwd];
    __shared__ double red[kLutWaves * 6];
    __shared__ float piv[3];
    const int y = blockIdx.y;
    const int img = (y < y_split) ? img_lo + y : img_hi + (y - y_split);
    const float *p = (img < n_first) ? base0 + (size_t)img * n_pixels * 3 : base1 + (size_t)(img - n_first) * n_pixels * 3;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_full = n_pixels / kTilePixels;                   // full tiles; the ragged rest is swept by workgroup 0
    const int64_t stride = (int64_t)gridDim.x * kLutWaves;
    int64_t t = (int64_t)blockIdx.x * kLutWaves + (threadIdx.x >> 6);
    float cur[12], nxt[12];
    auto load = [&](const float *tile, float (&e)[12]) {
        if (T_PLAIN && y < y_split) load_tile_plain(tile, lane, e);
        else load_tile(tile, lane, e);
    };
    if (t < n_full) load(p + t * (kTilePixels * 3), cur);                     // in flight while the tables are copied
    float p0[3] = {0.f, 0.f, 0.f};
    if (threadIdx.x == 0 && n_pixels > 0) { p0[0] = p[0]; p0[1] = p[1]; p0[2] = p[2]; }
    lut::load_tables<kLutBlock, false>(tab);
    __syncthreads();
    // Pivot of the shifted sums: the values of pixel 0 of the image (any point inside the data's range keeps the variance
    // well conditioned), put on a 2^-10 grid: (a float32 difference, on a 2^-26 grid) - (a pivot with finer bits) would round
    // the SAME way for every pixel -- a bias of half an ulp (measured: 4e-9, i.e. 2e-6 in mean a*).  Out-of-range pixel 0: 0.5.
    if (threadIdx.x == 0) {
        float fy = 0.5f, dxy = 0.0f, dyz = 0.0f;
        if (max(max(__float_as_uint(p0[0]), __float_as_uint(p0[1])), __float_as_uint(p0[2])) <= lut::kOneBits) {
            lut::rgb_to_f_stats(tab, p0[0], p0[1], p0[2], fy, dxy, dyz);
        }
        piv[0] = rintf(fy * 1024.0f) * (1.0f / 1024.0f);
        piv[1] = rintf(dxy * 1024.0f) * (1.0f / 1024.0f);
        piv[2] = rintf(dyz * 1024.0f) * (1.0f / 1024.0f);
    }
    __syncthreads();
    const float kf[3] = {__uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(piv[0]))),
                         __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(piv[1]))),
                         __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(piv[2])))};
    const double kd[3] = {(double)kf[0], (double)kf[1], (double)kf[2]};
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    float sf[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto stats_tile = [&](float (&c)[12]) {
        if (__builtin_amdgcn_ballot_w64(max_bits12(c) > lut::kOneBits)) {
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                double x, y, z;
                to_space<true>((double)c[0], (double)c[1], (double)c[2], x, y, z);
                accumulate<true>(s, kd, x, y, z);
                rotate_pixels(c);
                asm volatile("" : "+v"(c[0]));     // keep the loop rolled
            }
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float fy, dxy, dyz;
                lut::rgb_to_f_stats_hw(tab, c[3 * q], c[3 * q + 1], c[3 * q + 2], fy, dxy, dyz);
                const float dx = fy - kf[0], dy = dxy - kf[1], dz = dyz - kf[2];
                sf[0] += dx; sf[1] += dy; sf[2] += dz;
                sf[3] = fmaf(dx, dx, sf[3]); sf[4] = fmaf(dy, dy, sf[4]); sf[5] = fmaf(dz, dz, sf[5]);
            }
        }
    };
    for (; t < n_full; t += stride) {
        if (t + stride < n_full) load(p + (t + stride) * (kTilePixels * 3), nxt);
        stats_tile(cur);
#pragma unroll
        for (int i = 0; i < 12; ++i) cur[i] = nxt[i];
    }
    if (blockIdx.x == 0) {                                           // ragged tail (n_pixels % 256), exact arithmetic
        const int64_t px = n_full * kTilePixels + threadIdx.x;
        if (threadIdx.x < kTilePixels && px < n_pixels) {
            double x, y, z;
            to_space<true>((double)p[px * 3], (double)p[px * 3 + 1], (double)p[px * 3 + 2], x, y, z);
            accumulate<true>(s, kd, x, y, z);
        }
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) s[i] += (double)sf[i];
    block_sum<6, kLutWaves>(s, red);
    if (threadIdx.x == 0) {
        double *dst = partials + ((size_t)img * kMaxBlocksPerImage + blockIdx.x) * kPartialStride;
#pragma unroll
        for (int i = 0; i < 6; ++i) dst[i] = s[i];
        if (blockIdx.x == 0) {
            pivots[img * kPivotStride + 0] = kd[0];
            pivots[img * kPivotStride + 1] = kd[1];
            pivots[img * kPivotStride + 2] = kd[2];
        }
    }
}

// A2 on the table path: float32 difference forms (ct_color_lut.h: a* = 500 (fx - fy) must be right per pixel).  Affine scales
// above kFastScale (the forward error grows with them), pixels outside [0,1] and pixels within rounding of a kink of Lab's f()
// take the exact float64 code, tile by tile.
template <bool OUT_LAB>
__global__ __launch_bounds__(kLutBlock, kLutMinWaves) void reinhard_apply_lut_kernel(const float *__restrict__ target,
                                                                                     const double *__restrict__ stats_t,
                                                                                     const double *__restrict__ stats_r,
                                                                                     float *__restrict__ out, int64_t n_pixels,
                                                                                     const double *__restrict__ partials,
                                                                                     const double *__restrict__ pivots, int n_partials,
                                                                                     int batch, double *__restrict__ stats_out,
                                                                                     const float *__restrict__ gt, double *__restrict__ sq_partials,
                                                                                     int img0) {
    // gt != NULL: the per-frame squared error of the result against a ground-truth frame (the PSNR of Runner.test_step,
    // methods/__init__.py:32) is accumulated on the way out -- the corrected frame is not read back from HBM for it
    // img0: the launch covers images img0 .. img0 + gridDim.y - 1 of the batch (a chunk of pairs; 0 = the whole batch); every
    // pointer and record keeps its whole-batch index
    __shared__ __attribute__((aligned(16))) unsigned char tab[OUT_LAB ? lut::kLdsBytesFwd : lut::kLdsBytesAll];
    __shared__ double fin[12 * 8 + 2 * CT_LAB_STATS_STRIDE];
    const int img = img0 + blockIdx.y;
    const float *p = target + (size_t)img * n_pixels * 3;
    float *o = out + (size_t)img * n_pixels * 3;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t n_full = n_pixels / kTilePixels;
    const int64_t stride = (int64_t)gridDim.x * kLutWaves;
    int64_t t = (int64_t)blockIdx.x * kLutWaves + (threadIdx.x >> 6);
    float cur[12], nxt[12];
    if (t < n_full) load_tile(p + t * (kTilePixels * 3), lane, cur);
    // Fused call (partials != NULL): the finishing step of the statistics sweep is done here, by every workgroup for its
    // own pair -- the partial sums of the target (image img) and the reference (image batch + img) are added in a fixed
    // order (8 interleaved chains per moment, then in chain order), identical in every workgroup -- instead of a
    // one-workgroup-per-image kernel of its own (5.5 us + a launch boundary per call).
    if (partials != nullptr && threadIdx.x < 96) {
        const int g = threadIdx.x >> 3, sub = threadIdx.x & 7;          // g = which * 6 + moment
        const int image = (g >= 6) ? batch + img : img;
        const double *src = partials + (size_t)image * kMaxBlocksPerImage * kPartialStride + (g % 6);
        double a = 0.0;
        for (int b = sub; b < n_partials; b += 8) a += src[(size_t)b * kPartialStride];
        fin[g * 8 + sub] = a;
    }
    lut::load_tables<kLutBlock, !OUT_LAB>(tab);
    const double *rec_t = stats_t + (size_t)img * CT_LAB_STATS_STRIDE, *rec_r = stats_r + (size_t)img * CT_LAB_STATS_STRIDE;
    if (partials != nullptr) {
        __syncthreads();
        if (threadIdx.x < 2) {
            const int image = threadIdx.x ? batch + img : img;
            double sum[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) {
                const double *f = fin + (threadIdx.x * 6 + m) * 8;
                sum[m] = ((((((f[0] + f[1]) + f[2]) + f[3]) + f[4]) + f[5]) + f[6]) + f[7];
            }
            double *rec = fin + 96 + threadIdx.x * CT_LAB_STATS_STRIDE;
            lab_record(sum, pivots + image * kPivotStride, (double)n_pixels, rec, kVarFloorF32);      // the fused call: float32 sweep
            if (blockIdx.x == 0 && stats_out != nullptr) {
#pragma unroll
                for (int m = 0; m < CT_LAB_STATS_STRIDE; ++m) stats_out[(size_t)image * CT_LAB_STATS_STRIDE + m] = rec[m];
            }
        }
        __syncthreads();
        rec_t = fin + 96;
        rec_r = fin + 96 + CT_LAB_STATS_STRIDE;
    }
    ReinhardCoef c = reinhard_coef(rec_t, rec_r);
    c.sL = uniform_f64(c.sL); c.sa = uniform_f64(c.sa); c.sb = uniform_f64(c.sb);
    c.cy = uniform_f64(c.cy); c.ca = uniform_f64(c.ca); c.cb = uniform_f64(c.cb);
    // the table path needs finite, moderate coefficients (every intermediate finite, the float32 error budget kept); anything
    // else -- a constant target gives inf / nan like the reference -- goes through the exact code
    const bool coef_bad = !reinhard_coef_fast(c);
    const float sLf = (float)c.sL, saf = (float)c.sa, sbf = (float)c.sb, cyf = (float)c.cy, caf = (float)c.ca, cbf = (float)c.cb;
    double sq = 0.0;
    __syncthreads();
    auto apply_one = [&](float (&cc)[12], int64_t tt) {
        float w[12];
        bool slow = coef_bad || __builtin_amdgcn_ballot_w64(max_bits12(cc) > lut::kOneBits);
        if (!slow) {
            bool near = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float fy, dxy, dyz;
                near |= lut::rgb_to_f(tab, cc[3 * q], cc[3 * q + 1], cc[3 * q + 2], fy, dxy, dyz);
                const float gy = fmaf(sLf, fy, cyf), dx = fmaf(saf, dxy, caf), dz = fmaf(sbf, dyz, cbf);
                if (OUT_LAB) {
                    w[3 * q] = fmaf(116.0f, gy, -16.0f); w[3 * q + 1] = 500.0f * dx; w[3 * q + 2] = 200.0f * dz;
                } else {
                    near |= lut::f_to_rgb_clip(tab, gy, dx, dz, w[3 * q], w[3 * q + 1], w[3 * q + 2]);
                }
            }
            slow = __builtin_amdgcn_ballot_w64(near) != 0;        // a pixel within rounding of a kink of f(): the whole tile again, exactly
        }
        if (slow) {
#pragma unroll 1
            for (int q = 0; q < 4; ++q) {
                rotate_pixels(w);                      // the result of pixel q lands in slot 3 and ends in slot q
                reinhard_pixel<float, OUT_LAB>(c, (double)cc[0], (double)cc[1], (double)cc[2], w[9], w[10], w[11]);
                rotate_pixels(cc);
                asm volatile("" : "+v"(cc[0]));       // keep the loop rolled
            }
        }
        store_tile(o + tt * (kTilePixels * 3), lane, w);
        if (gt != nullptr) {                           // requested after the store: asked for before the arithmetic, the tile spills
            float gv[12];
            load_tile(gt + ((size_t)img * n_pixels + (size_t)tt * kTilePixels) * 3, lane, gv);
            float e = 0.f;
#pragma unroll
            for (int i = 0; i < 12; ++i) { const float d = w[i] - gv[i]; e = fmaf(d, d, e); }
            sq += (double)e;
        }
    };
    for (; t < n_full; t += stride) {
        if (t + stride < n_full) load_tile(p + (t + stride) * (kTilePixels * 3), lane, nxt);
        apply_one(cur, t);
#pragma unroll
        for (int i = 0; i < 12; ++i) cur[i] = nxt[i];
    }
    if (blockIdx.x == 0) {                                           // ragged tail (n_pixels % 256), exact arithmetic
        const int64_t px = n_full * kTilePixels + threadIdx.x;
        if (threadIdx.x < kTilePixels && px < n_pixels) {
            float a, b, d;
            reinhard_pixel<float, OUT_LAB>(c, (double)p[px * 3], (double)p[px * 3 + 1], (double)p[px * 3 + 2], a, b, d);
            o[px * 3] = a; o[px * 3 + 1] = b; o[px * 3 + 2] = d;
            if (gt != nullptr) {
                const float *gp = gt + ((size_t)img * n_pixels + px) * 3;
                const double d0 = (double)a - gp[0], d1 = (double)b - gp[1], d2 = (double)d - gp[2];
                sq += (d0 * d0 + d1 * d1) + d2 * d2;
            }
        }
    }
    if (gt != nullptr) {                                             // uniform per launch
        double v[1] = {sq};
        __syncthreads();                                             // fin[] is free again
        block_sum<1, kLutWaves>(v, fin);
        if (threadIdx.x == 0) sq_partials[(size_t)img * kMaxBlocksPerImage + blockIdx.x] = v[0];
    }
}

// -------------------------------------------------------------------------------------------
// host-side launchers
// -------------------------------------------------------------------------------------------

// Optional HIP events bracketing the two streaming kernels of the Reinhard path (bench.py's roofline measurement):
// set with ct_profile_events(); NULL = off.  Recorded on the launch stream, so they time exactly one kernel.
static thread_local hipEvent_t g_prof_evt[4] = {nullptr, nullptr, nullptr, nullptr};     // per calling thread: the thread that set them launches the kernels they bracket

// Lab arithmetic of the float32 entries: 0 = table-driven (ct_color_lut.h, default), 1 = exact float64 (ct_color.h).
// float64 images always take the exact path.  Two levels: a process-wide default (ct_set_lab_mode / env CT_HIP_LAB; atomic) and a
// per-thread override (ct_set_lab_mode_thread; -1 = none), so that two host threads driving different streams with different
// modes do not race on one global -- every entry reads the mode once, through lab_mode(), on the calling thread.
static std::atomic<int> g_lab_mode_default{[] { const char *e = env_str("CT_HIP_LAB"); return (e && e[0] == 'e') ? 1 : 0; }()};
static thread_local int t_lab_mode = -1;
static inline int lab_mode() { return t_lab_mode >= 0 ? t_lab_mode : g_lab_mode_default.load(std::memory_order_relaxed); }

// The pipelined form of the fused float32 entries (reinhard_pipelined below; ct_set_reinhard_pipeline): pairs per chunk (-1 = the
// built-in plan, 0 = off, > 0 forced) and the target-load policy of a chunk's statistics sweep (0 = non-temporal, 1 = plain),
// packed into one word so that a reader never sees half of a setting.  Two levels like the Lab mode: a process-wide atomic
// default and a per-thread override (kPipeNoOverride = none); every entry reads it once, on the calling thread.
// The built-in plan is MEASURED (tools/bench_reinhard_pipeline.py): chunks of about kPlanChunkPixels (four 1080p
// pairs: 8 pairs of 720p, one of 2160p), an even number of them so that both lanes carry the same load, plain target loads.
// Frames below kPlanMinPixels and calls below kPlanMinCallPixels keep the two whole-batch launches: there the fork and the
// join cost as much as the overlap returns.
constexpr int64_t kPlanChunkPixels = 4 * 1920 * 1080;
constexpr int64_t kPlanMinPixels = 1280 * 720;
constexpr int64_t kPlanMinCallPixels = 14000000;
constexpr int kPlanTPolicy = 1;
constexpr int kPipeLanes = 2;
constexpr int kPipeMaxChunk = 1 << 14;
constexpr int kPipeNoOverride = -2;
static inline int pipe_pack(int chunk_pairs, int t_policy) { return (chunk_pairs + 2) | (t_policy << 16); }
static std::atomic<int> g_pipe_default{pipe_pack(-1, kPlanTPolicy)};
static thread_local int t_pipe_override = kPipeNoOverride;
static inline void pipe_setting(int *chunk_pairs, int *t_policy) {
    const int v = t_pipe_override != kPipeNoOverride ? t_pipe_override : g_pipe_default.load(std::memory_order_relaxed);
    *chunk_pairs = (v & 0xffff) - 2;
    *t_policy = v >> 16;
}
// pairs per chunk this call runs with (0 = the two whole-batch launches)
static inline int pipe_chunk_for(int chunk_pairs, int64_t n_pixels, int batch) {
    if (chunk_pairs >= 0) return chunk_pairs;
    const int64_t total = n_pixels * batch;
    if (n_pixels < kPlanMinPixels || total < kPlanMinCallPixels || batch < 2) return 0;
    int64_t half = (total + kPlanChunkPixels) / (2 * kPlanChunkPixels);          // chunks per lane, rounded to nearest
    if (half < 1) half = 1;
    const int n_chunks = (int)(kPipeLanes * half < batch ? kPipeLanes * half : batch);
    return (batch + n_chunks - 1) / n_chunks;
}

// The second lane of the pipelined form: ONE library-owned stream with its fork / join events, per device and per calling thread,
// created on first use and kept (the first lane is the caller's own stream).  Non-blocking, so it never synchronises with the
// legacy default stream behind the caller's back.  NULL when the caller's stream is being captured and the pool does not exist
// yet (nothing may be created inside a capture: that call stays unpipelined), or when the device refused a stream.
struct PipePool {
    hipStream_t st = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    int state = 0;                                  // 0 not tried, 1 ready, -1 failed
};
static thread_local PipePool t_pipe_pool[kMaxDevices];
static PipePool *pipe_pool(hipStream_t s) {
    PipePool &p = t_pipe_pool[current_device()];
    if (p.state == 0) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) { (void)hipGetLastError(); return nullptr; }
        const bool ok = hipStreamCreateWithFlags(&p.st, hipStreamNonBlocking) == hipSuccess &&
                        hipEventCreateWithFlags(&p.fork, hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&p.join, hipEventDisableTiming) == hipSuccess;
        if (!ok) {
            (void)hipGetLastError();
            if (p.join) (void)hipEventDestroy(p.join);
            if (p.fork) (void)hipEventDestroy(p.fork);
            if (p.st) (void)hipStreamDestroy(p.st);
        }
        p.state = ok ? 1 : -1;
    }
    return p.state == 1 ? &p : nullptr;
}

// Workgroups of a table kernel: ONE round of persistent workgroups -- as many as are resident at once (occupancy query,
// cached per kernel), each sweeping enough chunks to amortise its 32-37 KB table copy.  CT_HIP_LUT_BLOCKS overrides the
// total (tuning).
template <typename K>
static int resident_blocks(K kernel) {
    int dev = 0, per_cu = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kLutBlock, 0) != hipSuccess || per_cu < 1) per_cu = 2;
    (void)hipGetLastError();
    return per_cu * cus;
}
static int lut_blocks_per_image(int resident, int64_t n_tiles, int n_images) {
    static int forced = env_int("CT_HIP_LUT_BLOCKS", 0);
    const int total = forced > 0 ? forced : resident;
    int64_t want = (n_tiles + kLutWaves - 1) / kLutWaves;
    int64_t cap = total / (n_images > 0 ? n_images : 1);
    if (cap < 4) cap = 4;
    if (cap > kMaxBlocksPerImage) cap = kMaxBlocksPerImage;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    return (int)want;
}

// The Lab statistics sweep: float32 images in table mode take lab_moments_lut_kernel, everything else the generic sweep.
// deferred_partials (table mode only): the caller's next kernel finishes the statistics itself (fused Reinhard); receives the
// number of partial sums per image, or stays 0 when this launch took a path that finishes here.
template <typename T>
static int launch_lab_moments(const T *base0, const T *base1, int n_first, int n_images, int64_t n_pixels, const WsLayout &l,
                              double *stats, hipStream_t s, int *deferred_partials = nullptr) {
    if (n_images == 0) return CT_OK;
    if constexpr (sizeof(T) == 4) {
        static const int resident = resident_blocks(lab_moments_lut_kernel<false>);
        if (lab_mode() == 0) {
            const int G = lut_blocks_per_image(resident, n_pixels / kTilePixels, n_images);
            if (g_prof_evt[0]) (void)hipEventRecord(g_prof_evt[0], s);
            hipLaunchKernelGGL(lab_moments_lut_kernel<false>, dim3(G, n_images), dim3(kLutBlock), 0, s, base0, base1, n_first, n_pixels,
                               l.partials, l.pivots, n_first, 0, n_first);
            CT_CHECK_LAUNCH();
            if (g_prof_evt[1]) (void)hipEventRecord(g_prof_evt[1], s);
            if (deferred_partials != nullptr && n_pixels > 0) {
                *deferred_partials = G;
                return CT_OK;
            }
            hipLaunchKernelGGL((moments_finalize_kernel<true>), dim3(n_images), dim3(kBlock), 0, s, l.partials, l.pivots, G, n_pixels,
                               stats, kVarFloorF32);
            CT_CHECK_LAUNCH();
            return CT_OK;
        }
    }
    return launch_moments<T, true>(base0, base1, n_first, n_images, n_pixels, l, stats, s, g_prof_evt[0], g_prof_evt[1]);
}

// sq_blocks: receives the number of squared-error partials per image when the table kernel ran (only it takes gt)
template <typename T, bool OUT_LAB>
static int launch_reinhard_apply(const T *target, const double *st, const double *sr, T *out, int64_t n_pixels,
                                 int batch, hipStream_t s, const WsLayout *deferred = nullptr, int n_partials = 0,
                                 double *stats_out = nullptr, const float *gt = nullptr, double *sq_partials = nullptr,
                                 int *sq_blocks = nullptr) {
    if (batch == 0 || n_pixels == 0) return CT_OK;
    constexpr bool kLut = sizeof(T) == 4;
    const bool use_lut = kLut && lab_mode() == 0;
    int G = blocks_per_image(n_pixels >> 2, batch);
    if constexpr (kLut) {
        static const int resident = resident_blocks(reinhard_apply_lut_kernel<OUT_LAB>);
        if (use_lut) G = lut_blocks_per_image(resident, n_pixels / kTilePixels, batch);
    }
    if (g_prof_evt[2]) (void)hipEventRecord(g_prof_evt[2], s);
    if constexpr (kLut) {
        if (use_lut)
            hipLaunchKernelGGL((reinhard_apply_lut_kernel<OUT_LAB>), dim3(G, batch), dim3(kLutBlock), 0, s, target, st, sr, out,
                               n_pixels, (const double *)(deferred ? deferred->partials : nullptr),
                               (const double *)(deferred ? deferred->pivots : nullptr), n_partials, batch, stats_out, gt, sq_partials, 0);
        if (use_lut && sq_blocks) *sq_blocks = G;
    }
    if (!use_lut)
        hipLaunchKernelGGL((reinhard_apply_kernel<T, OUT_LAB>), dim3(G, batch), dim3(kBlock), 0, s, target, st, sr, out,
                           n_pixels);
    CT_CHECK_LAUNCH();
    if (g_prof_evt[3]) (void)hipEventRecord(g_prof_evt[3], s);
    return CT_OK;
}

template <typename T>
static int lab_stats_impl(const T *rgb, int64_t n_pixels, int n_images, double *stats, void *ws, size_t ws_bytes,
                          void *stream) {
    int rc = check_image_args(rgb, n_pixels, n_images);
    if (rc) return rc;
    if (n_images > 0 && stats == nullptr) return CT_E_BADARG;
    if ((rc = check_ws(ws, ws_bytes, n_images))) return rc;
    return launch_lab_moments<T>(rgb, rgb, n_images, n_images, n_pixels, ws_carve(ws, n_images), stats, (hipStream_t)stream);
}

// The two sweeps as the separate entries run them: ct_lab_stats_f32 on the targets, then on the references (each finished by
// moments_finalize_kernel), then ct_reinhard_apply_f32 -- bit for bit the result of those three calls.  For the one case in which
// the fused float32 entries may not take the persistent launch that is otherwise theirs (CT_HIP_REINHARD_PERSIST=1): an output
// that overlaps an input, which include/ct_hip.h allows them (out == target) and rp::launch refuses.  Table arithmetic only.
static int reinhard_separate_sweeps(const float *target, const float *reference, const float *gt, float *out, int64_t n_pixels, int batch,
                                    double *stats, const WsLayout &l, double *sq, int *sq_blocks, hipStream_t s) {
    int rc = launch_lab_moments<float>(target, target, batch, batch, n_pixels, l, stats, s);
    if (rc) return rc;
    double *stats_r = stats + (size_t)batch * CT_LAB_STATS_STRIDE;
    if ((rc = launch_lab_moments<float>(reference, reference, batch, batch, n_pixels, l, stats_r, s))) return rc;    // same stream: the partial sums are free again
    return launch_reinhard_apply<float, false>(target, stats, stats_r, out, n_pixels, batch, s, nullptr, 0, nullptr, gt, sq, sq_blocks);
}

// a1 for float64 frames: always the two exact sweeps; stats records [0,batch) = targets, [batch,2batch) = references
static int reinhard_f64_impl(const double *target, const double *reference, double *out, int64_t n_pixels, int batch,
                             double *stats_out, void *ws, size_t ws_bytes, void *stream) {
    int rc = check_image_args(target, n_pixels, batch);
    if (rc) return rc;
    if ((rc = check_image_args(reference, n_pixels, batch))) return rc;
    if ((rc = check_image_args(out, n_pixels, batch))) return rc;
    if ((rc = check_ws(ws, ws_bytes, 2 * batch))) return rc;
    if (batch == 0) return CT_OK;
    const WsLayout l = ws_carve(ws, 2 * batch);
    double *stats = stats_out ? stats_out : l.stats;
    rc = launch_lab_moments<double>(target, reference, batch, 2 * batch, n_pixels, l, stats, (hipStream_t)stream);
    if (rc) return rc;
    return launch_reinhard_apply<double, false>(target, stats, stats + (size_t)batch * CT_LAB_STATS_STRIDE, out, n_pixels, batch,
                                                (hipStream_t)stream);
}

// Workspace of the fused entry with the PSNR: the Reinhard layout followed by batch x kMaxBlocksPerImage doubles.
static size_t ws_bytes_reinhard_psnr(int batch) { return ws_bytes_for(2 * batch) + (size_t)batch * kMaxBlocksPerImage * sizeof(double); }

// The two table sweeps over chunks of `chunk` pairs on two lanes: chunk k runs statistics(k) -> apply(k) on the caller's stream (even
// k) or on the library's stream (odd k), which is forked from the caller's stream with an event before the first chunk and
// joined back into it with an event after the last -- no kernel waits for another, only stream order.  Every chunk launch is sized
// for 1 / kPipeLanes of the chip, so the kernels of the two lanes are resident SIDE BY SIDE: one lane's ramp (32-37 KB of tables
// per workgroup, the prologue barriers) and drain run under the other lane's streaming, and a statistics sweep (arithmetic and
// streaming in balance) shares the CUs with an apply sweep (HBM bound) whenever the lanes are out of phase.  Measured against
// the alternatives: whole-chip grids only overlap a tail with a ramp, and two library streams beside an idle
// caller's stream pay a second fork and join (slower than the whole-batch launches).
// The per-image workgroup counts are those of a FULL chunk, for the ragged last chunk too: one count of squared-error partials per
// image for the PSNR finish, and a static tile -> workgroup map.  Chunks write disjoint rows of the workspace and the order in
// which the lanes happen to run enters no sum: results are bitwise reproducible run to run.  The PSNR finish stays with the
// caller (once, over all images, on `s`).  Capturable: the fork / join events make the second lane part of a capture of `s`.
static int reinhard_pipelined(const float *target, const float *reference, const float *gt, float *out, int64_t n_pixels, int batch,
                              double *stats, const WsLayout &l, double *sq, int *sq_blocks, int chunk, bool t_plain, PipePool &pp,
                              hipStream_t s) {
    static const int res_stats = resident_blocks(lab_moments_lut_kernel<false>);
    static const int res_apply = resident_blocks(reinhard_apply_lut_kernel<false>);
    if (chunk > batch) chunk = batch;
    const int64_t tiles = n_pixels / kTilePixels;
    const int Gs = lut_blocks_per_image(res_stats / kPipeLanes, tiles, 2 * chunk);
    const int Ga = lut_blocks_per_image(res_apply / kPipeLanes, tiles, chunk);
    hipError_t e = hipEventRecord(pp.fork, s);
    if (e != hipSuccess) return (int)e;             // nothing forked yet
    e = hipStreamWaitEvent(pp.st, pp.fork, 0);
    int k = 0;
    for (int p0 = 0; p0 < batch && e == hipSuccess; p0 += chunk, ++k) {
        const int cp = batch - p0 < chunk ? batch - p0 : chunk;
        hipStream_t q = (k & 1) ? pp.st : s;
        if (t_plain)
            hipLaunchKernelGGL(lab_moments_lut_kernel<true>, dim3(Gs, 2 * cp), dim3(kLutBlock), 0, q, target, reference, batch, n_pixels,
                               l.partials, l.pivots, cp, p0, batch + p0);
        else
            hipLaunchKernelGGL(lab_moments_lut_kernel<false>, dim3(Gs, 2 * cp), dim3(kLutBlock), 0, q, target, reference, batch, n_pixels,
                               l.partials, l.pivots, cp, p0, batch + p0);
        if ((e = hipGetLastError()) != hipSuccess) break;
        hipLaunchKernelGGL((reinhard_apply_lut_kernel<false>), dim3(Ga, cp), dim3(kLutBlock), 0, q, target, (const double *)stats,
                           (const double *)(stats + (size_t)batch * CT_LAB_STATS_STRIDE), out, n_pixels, (const double *)l.partials,
                           (const double *)l.pivots, Gs, batch, stats, gt, sq, p0);
        e = hipGetLastError();
    }
    // join even after an error: a capture of `s` must not be left with a forked stream
    hipError_t j = hipEventRecord(pp.join, pp.st);
    if (j == hipSuccess) j = hipStreamWaitEvent(s, pp.join, 0);
    if (e == hipSuccess) e = j;
    if (gt != nullptr) *sq_blocks = Ga;
    return (int)e;
}

// a1 for float32 frames, the body of ct_reinhard_f32 (psnr = false; gt, psnr_out NULL) and of ct_reinhard_psnr_f32: the latter is
// color_transfer_between_images for `batch` pairs fused with the per-frame PSNR of Runner.test_step (methods/__init__.py:30-32,37),
// PSNR(result, gt) per frame.  Past the argument checks gt != NULL means "with the PSNR".  Table path: the squared error is
// accumulated by the apply sweep while it writes the result (one extra plane read, the result is never read back); exact
// path: a sweep of its own over (out, gt).
static int reinhard_f32_impl(bool psnr, const float *target, const float *reference, const float *gt, float *out, double *psnr_out,
                             int64_t n_pixels, int batch, double *stats_out, void *ws, size_t ws_bytes, void *stream) {
    int rc = check_image_args(target, n_pixels, batch);
    if (rc) return rc;
    if ((rc = check_image_args(reference, n_pixels, batch))) return rc;
    if (psnr && (rc = check_image_args(gt, n_pixels, batch))) return rc;
    if ((rc = check_image_args(out, n_pixels, batch))) return rc;
    if (psnr && batch > 0 && psnr_out == nullptr) return CT_E_BADARG;
    if ((rc = check_ws(ws, ws_bytes, 2 * batch))) return rc;
    if (psnr && ws_bytes < ws_bytes_reinhard_psnr(batch)) return CT_E_WORKSPACE;
    // an empty frame: the PSNR entry launches nothing, the plain one still runs its statistics launches
    if (batch == 0 || (psnr && n_pixels == 0)) return CT_OK;
    hipStream_t s = (hipStream_t)stream;
    const WsLayout l = ws_carve(ws, 2 * batch);
    double *stats = stats_out ? stats_out : l.stats;
    double *sq = psnr ? reinterpret_cast<double *>(reinterpret_cast<char *>(ws) + ws_bytes_for(2 * batch)) : nullptr;
    int sq_blocks = 0;
    // frames whose 1 / CUs share fits one CU's LDS: one persistent launch (reinhard_persist.hip) instead of the two sweeps
    if (lab_mode() == 0 && n_pixels > 0 && rp::eligible(n_pixels, false) && ws_bytes >= rp::ws_bytes(n_pixels, batch)) {
        if (!rp::overlaps(out, target, reference, gt, n_pixels, batch, sizeof(float))) {
            if (g_prof_evt[0]) (void)hipEventRecord(g_prof_evt[0], s);
            if (g_prof_evt[1]) (void)hipEventRecord(g_prof_evt[1], s);
            return rp::launch<float>(target, reference, gt, out, psnr_out, n_pixels, batch, stats_out, ws, ws_bytes, s, g_prof_evt[2], g_prof_evt[3]);
        }
        rc = reinhard_separate_sweeps(target, reference, gt, out, n_pixels, batch, stats, l, sq, &sq_blocks, s);      // e.g. out == target
    } else {
        // Table arithmetic, no profile events armed (they bracket undisturbed whole-batch launches), `out` clear of every input
        // (out == target exactly is fine: a chunk's apply sweep writes only its own targets): the sweeps may run chunk by chunk
        int chunk_pairs, t_policy;
        pipe_setting(&chunk_pairs, &t_policy);
        const int chunk = pipe_chunk_for(chunk_pairs, n_pixels, batch);
        PipePool *pp = nullptr;
        if (chunk > 0 && lab_mode() == 0 && n_pixels > 0 && !g_prof_evt[0] && !g_prof_evt[1] && !g_prof_evt[2] && !g_prof_evt[3] &&
            !rp::overlaps(out, out == target ? nullptr : target, reference, gt, n_pixels, batch, sizeof(float)))
            pp = pipe_pool(s);
        if (pp != nullptr) {
            rc = reinhard_pipelined(target, reference, gt, out, n_pixels, batch, stats, l, sq, &sq_blocks, chunk, t_policy == 1, *pp, s);
        } else {
            // one sweep over all 2*batch images; stats records [0,batch) = targets, [batch,2batch) = references
            int deferred = 0;      // > 0: table path, the apply kernel finishes the statistics in its prologue (and writes stats_out)
            rc = launch_lab_moments<float>(target, reference, batch, 2 * batch, n_pixels, l, stats, s, &deferred);
            if (rc) return rc;
            rc = launch_reinhard_apply<float, false>(target, stats, stats + (size_t)batch * CT_LAB_STATS_STRIDE, out, n_pixels, batch, s,
                                                     deferred > 0 ? &l : nullptr, deferred, stats, deferred > 0 ? gt : nullptr, sq, &sq_blocks);
        }
    }
    if (rc || gt == nullptr) return rc;
    if (sq_blocks == 0) {                       // exact path: a sweep of its own over (out, gt)
        if ((rc = launch_sqerr_partials(out, gt, n_pixels * 3, batch, sq, &sq_blocks, s))) return rc;
    }
    return launch_psnr_finish(sq, sq_blocks, kMaxBlocksPerImage, n_pixels * 3, batch, psnr_out, s);
}

// the persistent launch by name (any frame size it supports; the automatic dispatch above only takes frames that fill every wave)
template <typename T>
static int reinhard_persist_entry(const T *target, const T *reference, const T *gt, float *out, double *psnr_out, int64_t n_pixels, int batch,
                                  double *stats_out, void *ws, size_t ws_bytes, void *stream) {
    int rc = check_image_args(target, n_pixels, batch);
    if (rc) return rc;
    if ((rc = check_image_args(reference, n_pixels, batch))) return rc;
    if ((rc = check_image_args(out, n_pixels, batch))) return rc;
    if (gt != nullptr && psnr_out == nullptr) return CT_E_BADARG;
    if (batch == 0) return CT_OK;
    if (!rp::eligible(n_pixels, true)) return CT_E_BADARG;
    return rp::launch<T>(target, reference, gt, out, psnr_out, n_pixels, batch, stats_out, ws, ws_bytes, (hipStream_t)stream,
                             g_prof_evt[2], g_prof_evt[3]);
}

}  // namespace ct

// -------------------------------------------------------------------------------------------
// C ABI (include/ct_hip.h)
// -------------------------------------------------------------------------------------------
extern "C" {

int ct_set_lab_mode(int mode) {
    if (mode != CT_LAB_TABLE && mode != CT_LAB_EXACT) return CT_E_BADARG;
    ct::g_lab_mode_default.store(mode, std::memory_order_relaxed);
    return CT_OK;
}
int ct_get_lab_mode(void) { return ct::lab_mode(); }
int ct_set_lab_mode_thread(int mode) {
    if (mode != -1 && mode != CT_LAB_TABLE && mode != CT_LAB_EXACT) return CT_E_BADARG;
    ct::t_lab_mode = mode;
    return CT_OK;
}

static bool pipe_args_ok(int chunk_pairs, int t_policy) {
    return chunk_pairs >= -1 && chunk_pairs <= ct::kPipeMaxChunk && t_policy >= -1 && t_policy <= CT_PIPE_T_PLAIN;
}
int ct_set_reinhard_pipeline(int chunk_pairs, int t_policy) {
    if (!pipe_args_ok(chunk_pairs, t_policy)) return CT_E_BADARG;
    ct::g_pipe_default.store(ct::pipe_pack(chunk_pairs, t_policy < 0 ? ct::kPlanTPolicy : t_policy), std::memory_order_relaxed);
    return CT_OK;
}
int ct_set_reinhard_pipeline_thread(int chunk_pairs, int t_policy) {
    if (chunk_pairs == ct::kPipeNoOverride) { ct::t_pipe_override = ct::kPipeNoOverride; return CT_OK; }
    if (!pipe_args_ok(chunk_pairs, t_policy)) return CT_E_BADARG;
    ct::t_pipe_override = ct::pipe_pack(chunk_pairs, t_policy < 0 ? ct::kPlanTPolicy : t_policy);
    return CT_OK;
}
int ct_get_reinhard_pipeline(int *chunk_pairs, int *t_policy) {
    int c, p;
    ct::pipe_setting(&c, &p);
    if (chunk_pairs) *chunk_pairs = c;
    if (t_policy) *t_policy = p;
    return CT_OK;
}
int ct_reinhard_pipeline_chunk(int64_t n_pixels, int batch) {
    int c, p;
    ct::pipe_setting(&c, &p);
    return ct::pipe_chunk_for(c, n_pixels, batch);
}

void ct_profile_events(void *moments_start, void *moments_stop, void *apply_start, void *apply_stop) {
    ct::g_prof_evt[0] = (hipEvent_t)moments_start;
    ct::g_prof_evt[1] = (hipEvent_t)moments_stop;
    ct::g_prof_evt[2] = (hipEvent_t)apply_start;
    ct::g_prof_evt[3] = (hipEvent_t)apply_stop;
}

size_t ct_workspace_bytes(int kind, int64_t n_pixels, int n_images) {
    if (n_images < 0) return 0;
    switch (kind) {
        case CT_WS_LAB_STATS:
        case CT_WS_RGB_MEANCOV: return ct::ws_bytes_for(n_images);
        case CT_WS_REINHARD: { const size_t a = ct::ws_bytes_for(2 * n_images), b = ct::rp::ws_bytes(n_pixels, n_images); return a > b ? a : b; }
        case CT_WS_REINHARD_PSNR: { const size_t a = ct::ws_bytes_reinhard_psnr(n_images), b = ct::rp::ws_bytes(n_pixels, n_images); return a > b ? a : b; }
        case CT_WS_REINHARD_PERSIST: return ct::rp::ws_bytes(n_pixels, n_images);
        case CT_WS_MK_U8: return ct::ws_bytes_mk_u8(n_images);
        default: return 0;
    }
}

int ct_lab_stats_f32(const float *rgb, int64_t n_pixels, int n_images, double *stats, void *ws, size_t ws_bytes,
                     void *stream) {
    return ct::lab_stats_impl<float>(rgb, n_pixels, n_images, stats, ws, ws_bytes, stream);
}
int ct_lab_stats_f64(const double *rgb, int64_t n_pixels, int n_images, double *stats, void *ws, size_t ws_bytes,
                     void *stream) {
    return ct::lab_stats_impl<double>(rgb, n_pixels, n_images, stats, ws, ws_bytes, stream);
}

int ct_reinhard_apply_f32(const float *target, const double *stats_t, const double *stats_r, float *out,
                          int64_t n_pixels, int batch, void *stream) {
    int rc = ct::check_image_args(target, n_pixels, batch);
    if (rc) return rc;
    if ((rc = ct::check_image_args(out, n_pixels, batch))) return rc;
    if (batch > 0 && (!stats_t || !stats_r)) return CT_E_BADARG;
    return ct::launch_reinhard_apply<float, false>(target, stats_t, stats_r, out, n_pixels, batch, (hipStream_t)stream);
}
int ct_reinhard_apply_f64(const double *target, const double *stats_t, const double *stats_r, double *out,
                          int64_t n_pixels, int batch, void *stream) {
    int rc = ct::check_image_args(target, n_pixels, batch);
    if (rc) return rc;
    if ((rc = ct::check_image_args(out, n_pixels, batch))) return rc;
    if (batch > 0 && (!stats_t || !stats_r)) return CT_E_BADARG;
    return ct::launch_reinhard_apply<double, false>(target, stats_t, stats_r, out, n_pixels, batch,
                                                    (hipStream_t)stream);
}
int ct_reinhard_lab_f32(const float *target, const double *stats_t, const double *stats_r, float *out_lab,
                        int64_t n_pixels, int batch, void *stream) {
    int rc = ct::check_image_args(target, n_pixels, batch);
    if (rc) return rc;
    if ((rc = ct::check_image_args(out_lab, n_pixels, batch))) return rc;
    if (batch > 0 && (!stats_t || !stats_r)) return CT_E_BADARG;
    return ct::launch_reinhard_apply<float, true>(target, stats_t, stats_r, out_lab, n_pixels, batch,
                                                  (hipStream_t)stream);
}

int ct_reinhard_f32(const float *target, const float *reference, float *out, int64_t n_pixels, int batch,
                    double *stats_out, void *ws, size_t ws_bytes, void *stream) {
    return ct::reinhard_f32_impl(false, target, reference, nullptr, out, nullptr, n_pixels, batch, stats_out, ws, ws_bytes, stream);
}
int ct_reinhard_f64(const double *target, const double *reference, double *out, int64_t n_pixels, int batch,
                    double *stats_out, void *ws, size_t ws_bytes, void *stream) {
    return ct::reinhard_f64_impl(target, reference, out, n_pixels, batch, stats_out, ws, ws_bytes, stream);
}
int ct_reinhard_psnr_f32(const float *target, const float *reference, const float *gt, float *out, double *psnr_out, int64_t n_pixels,
                         int batch, double *stats_out, void *ws, size_t ws_bytes, void *stream) {
    return ct::reinhard_f32_impl(true, target, reference, gt, out, psnr_out, n_pixels, batch, stats_out, ws, ws_bytes, stream);
}

int ct_reinhard_persist_supported(int64_t n_pixels) { return ct::rp::eligible(n_pixels, true) ? 1 : 0; }
int ct_reinhard_takes_persist(int64_t n_pixels) { return (ct::lab_mode() == 0 && ct::rp::eligible(n_pixels, false)) ? 1 : 0; }
int ct_reinhard_persist_f32(const float *target, const float *reference, const float *gt, float *out, double *psnr_out, int64_t n_pixels,
                            int batch, double *stats_out, void *ws, size_t ws_bytes, void *stream) {
    return ct::reinhard_persist_entry<float>(target, reference, gt, out, psnr_out, n_pixels, batch, stats_out, ws, ws_bytes, stream);
}
int ct_reinhard_psnr_u8(const uint8_t *target, const uint8_t *reference, const uint8_t *gt, float *out, double *psnr_out, int64_t n_pixels,
                        int batch, double *stats_out, void *ws, size_t ws_bytes, void *stream) {
    return ct::reinhard_persist_entry<uint8_t>(target, reference, gt, out, psnr_out, n_pixels, batch, stats_out, ws, ws_bytes, stream);
}

}  // extern "C"
