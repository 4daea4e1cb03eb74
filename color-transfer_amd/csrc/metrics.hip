// metrics.hip -- per-frame quality metrics of Runner.test_step (reference methods/__init__.py:29-40) on gfx950:
//   SSIM  = piq.ssim(result, gt) with piq's defaults (11x11 Gaussian, sigma 1.5, k1 0.01, k2 0.03, data_range 1,
//           average-pool downsampling by max(1, round(min(H, W) / 256)), "valid" windows, mean over channels and positions)
//   iCID  = utils/icid.py:28-152 (perceptual intent, all seven maps, bilinear downsampling by the same factor, kornia's
//           rgb_to_lab, torchvision's 11x11 sigma-2 gaussian_blur with reflect padding); ct_frame_icid_opt_*: its other two
//           intents, omit_maps67 and downsampling = False (the maps at the frame's own size) as well
// piq, kornia and torchvision are third-party and absent offline: their arithmetic is restated from their published
// sources (oracle/metrics.py says where) -- "parity unpinned" for those calls; SSIM's core is anchored on scikit-image's
// structural_similarity, iCID's own lines on a run of the reference's utils/icid.py (tests/golden/make_golden_*).
//
//   PSNR  = a float64 squared-error sweep and its finish (at the end of this file; linear.hip's fused Reinhard + PSNR entry
//           launches the same two kernels through ct_metrics.h)
//
// SSIM and iCID are ONE fused pass per frame: a workgroup owns a 32x32 (SSIM) / 32x16 (iCID) tile of the metric map, brings the
// down-sampled inputs (plus a 5-pixel halo) into LDS straight from the full-resolution NCHW planes, runs the separable
// 11-tap Gaussian (rows into LDS, then columns) for all 5 / 11 moment maps at once, evaluates the per-pixel formula and
// reduces it to one float64 partial sum; a finishing kernel adds the partials in a fixed order (deterministic).  float32
// arithmetic, float64 sums; unlike the reference's torch code the second moments are taken about a pivot pixel of the tile, so
// that flat and saturated frames stay on the float64 value (the reference's float32 run leaves it by 3e-4 there: DESIGN.md 4.6).
//
// Both tile kernels are templates on the frame sources of ct_frame_src.h: planar float32 (ct_frame_*_f32), or what a group of uint8
// frames holds -- the transfer's unclamped float32 HWC result, clamped as it is read, and the uint8 HWC ground truth through a
// (float)k / 255.0f table in LDS (ct_frame_*_hwc_u8).  One body: the second form is bitwise the first on the converted tensors
// (DESIGN.md 4.20).
#include "ct_color.h"
#include "ct_common.h"
#include "ct_frame_src.h"
#include "ct_metrics.h"

namespace ct {

constexpr int kTaps = 11, kHalo = kTaps - 1;

__device__ __forceinline__ void gauss_weights(float *w /* LDS [11] */, float sigma) {
    if (threadIdx.x < kTaps) {
        float s = 0.f;
        for (int k = 0; k < kTaps; ++k) { const float x = (float)(k - 5) / sigma; s += expf(-0.5f * x * x); }
        const float x = (float)((int)threadIdx.x - 5) / sigma;
        w[threadIdx.x] = expf(-0.5f * x * x) / s;
    }
}

__device__ __forceinline__ double block_reduce_1(double v, double *lds /* [4] */) {
    double a[1] = {v};
    block_sum<1>(a, lds);
    return a[0];
}

// -------------------------------------------------------------------------------------------------------------------
// SSIM.  SA / SB: the frame sources of a (result) and b (ground truth), ct_frame_src.h.  Planar sources: grid = (tiles_x,
// tiles_y, batch * 3), a workgroup owns one plane's tile.  HWC sources: grid = (tiles_x, tiles_y, batch), a workgroup takes its
// tile's three channels from ONE pass over the pixels (12 B + 3 B contiguous per pixel) and runs the rest channel by channel
// through the one hb buffer; its partial of channel c lands in the slot the planar workgroup of plane img * 3 + c writes, with
// the same thread -> pixel assignment and block_sum: the same bits, and metric_finish_kernel serves both.
// Pooled size Hp x Wp = (H / f, W / f).  Dynamic LDS: sx, sy [NC][42][42], hb [5][42][32] floats (ssim_lds_bytes).
// -------------------------------------------------------------------------------------------------------------------
constexpr int kSsTW = 32, kSsTH = 32;
constexpr size_t ssim_lds_bytes(int nc) { return ((size_t)2 * nc * (kSsTH + kHalo) * (kSsTW + kHalo) + (size_t)5 * (kSsTH + kHalo) * kSsTW) * sizeof(float); }

template <class SA, class SB>
__global__ __launch_bounds__(kBlock) void ssim_tile_kernel(const typename SA::elem *__restrict__ a, const typename SB::elem *__restrict__ b, int H, int W,
                                                           int f, int Hp, int Wp, double *__restrict__ partials) {
    static_assert(SA::kHwc == SB::kHwc, "both frames planar or both HWC");
    constexpr int NC = SA::kHwc ? 3 : 1;               // channels per workgroup
    extern __shared__ __attribute__((aligned(16))) float ss_smem[];
    typedef float TileRow[kSsTW + kHalo];
    typedef float HbRow[kSsTW];
    TileRow(*sx)[kSsTH + kHalo] = reinterpret_cast<TileRow(*)[kSsTH + kHalo]>(ss_smem);
    TileRow(*sy)[kSsTH + kHalo] = sx + NC;
    HbRow(*hb)[kSsTH + kHalo] = reinterpret_cast<HbRow(*)[kSsTH + kHalo]>(sy + NC);
    __shared__ float w[kTaps];
    __shared__ float tab[SA::kTable || SB::kTable ? 256 : 1];
    __shared__ double red[4];
    const int img = SA::kHwc ? (int)blockIdx.z : (int)blockIdx.z / 3, c0 = SA::kHwc ? 0 : (int)blockIdx.z % 3;
    const int ox = blockIdx.x * kSsTW, oy = blockIdx.y * kSsTH;
    const int Ho = Hp - kHalo, Wo = Wp - kHalo;
    gauss_weights(w, 1.5f);
    if constexpr (SA::kTable || SB::kTable) {
        fill_u8_table_f32(tab);
        __syncthreads();
    }
    const SA pa(a, img, H, W, tab);
    const SB pb(b, img, H, W, tab);
    const float inv = 1.0f / (float)(f * f);
    // moments about a pivot of the tile (a frame pixel near its middle): variances and the covariance do not depend on it, and
    // E[x^2] - mu^2 no longer cancels from O(1) on a flat or saturated frame, where the float32 rounding of the sums over
    // c2 = 9e-4 put SSIM 2.6e-4 above 1.  Tile entries past the frame stay 0 and feed masked outputs only.
    const size_t pivot = (size_t)((oy + min(kSsTH / 2 + 5, Hp - 1 - oy)) * f) * W + (size_t)((ox + min(kSsTW / 2 + 5, Wp - 1 - ox)) * f);
    float pvx[NC], pvy[NC];
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) { pvx[ch] = pa.at(c0 + ch, pivot); pvy[ch] = pb.at(c0 + ch, pivot); }
    for (int i = threadIdx.x; i < (kSsTH + kHalo) * (kSsTW + kHalo); i += kBlock) {
        const int r = i / (kSsTW + kHalo), c = i % (kSsTW + kHalo);
        const int py = oy + r, px = ox + c;
        float vx[NC], vy[NC];
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) vx[ch] = vy[ch] = 0.f;
        if (py < Hp && px < Wp) {
            for (int dy = 0; dy < f; ++dy)
                for (int dx = 0; dx < f; ++dx) {
                    const size_t o = (size_t)(py * f + dy) * W + (px * f + dx);
                    if constexpr (NC == 3) {
                        float ta[3], tb[3];
                        pa.at3(o, ta); pb.at3(o, tb);
#pragma unroll
                        for (int ch = 0; ch < 3; ++ch) { vx[ch] += ta[ch]; vy[ch] += tb[ch]; }
                    } else {
                        vx[0] += pa.at(c0, o); vy[0] += pb.at(c0, o);
                    }
                }
#pragma unroll
            for (int ch = 0; ch < NC; ++ch) { vx[ch] = vx[ch] * inv - pvx[ch]; vy[ch] = vy[ch] * inv - pvy[ch]; }  // F.avg_pool2d(kernel_size = f), about the pivot
        }
#pragma unroll
        for (int ch = 0; ch < NC; ++ch) { sx[ch][r][c] = vx[ch]; sy[ch][r][c] = vy[ch]; }
    }
    __syncthreads();
    // channel by channel through hb: block_sum's barrier stands between a channel's column pass and the next one's row pass
#pragma unroll
    for (int ch = 0; ch < NC; ++ch) {
        for (int i = threadIdx.x; i < (kSsTH + kHalo) * kSsTW; i += kBlock) {
            const int r = i / kSsTW, c = i % kSsTW;
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
                const float x = sx[ch][r][c + k], y = sy[ch][r][c + k], g = w[k];
                m[0] = fmaf(g, x, m[0]); m[1] = fmaf(g, y, m[1]); m[2] = fmaf(g, x * x, m[2]); m[3] = fmaf(g, y * y, m[3]); m[4] = fmaf(g, x * y, m[4]);
            }
#pragma unroll
            for (int q = 0; q < 5; ++q) hb[q][r][c] = m[q];
        }
        __syncthreads();
        double acc = 0.0;
        for (int i = threadIdx.x; i < kSsTH * kSsTW; i += kBlock) {
            const int r = i / kSsTW, c = i % kSsTW;
            if (oy + r < Ho && ox + c < Wo) {
                float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < kTaps; ++k) {
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] = fmaf(w[k], hb[q][r + k][c], m[q]);
                }
                const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
                const float mx = m[0] + pvx[ch], my = m[1] + pvy[ch];        // the window means; m[] are about the pivots
                const float mxx = mx * mx, myy = my * my, mxy = mx * my;
                const float sxx = m[2] - m[0] * m[0], syy = m[3] - m[1] * m[1], sxy = m[4] - m[0] * m[1];
                const float cs = (2.0f * sxy + c2) / (sxx + syy + c2);
                acc += (double)((2.0f * mxy + c1) / (mxx + myy + c1) * cs);
            }
        }
        acc = block_reduce_1(acc, red);
        if (threadIdx.x == 0) partials[((size_t)(img * 3 + c0 + ch) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = acc;
    }
}

// -------------------------------------------------------------------------------------------------------------------
// iCID.  grid = (tiles_x, tiles_y, batch); down-sampled size h x w; maps live on the whole h x w grid (reflect padding).
// SA / SB: the frame sources (ct_frame_src.h); a pixel's three channels come from one at3() per bilinear tap.
// -------------------------------------------------------------------------------------------------------------------
constexpr int kIcTW = 32, kIcTH = 16;

// F.interpolate(scale_factor = 1/f, mode = "bilinear", align_corners = False) of the three channels of a frame at output pixel (y, x)
template <class S> __device__ __forceinline__ void bilinear_down3(const S &p, int H, int W, int f, int y, int x, float (&v)[3]) {
    if (f == 1) { p.at3((size_t)y * W + x, v); return; }
    const float sy = fmaxf(((float)y + 0.5f) * (float)f - 0.5f, 0.f), sx = fmaxf(((float)x + 0.5f) * (float)f - 0.5f, 0.f);
    const int y0 = (int)sy, x0 = (int)sx;
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float wy = sy - (float)y0, wx = sx - (float)x0;
    float v00[3], v01[3], v10[3], v11[3];
    p.at3((size_t)y0 * W + x0, v00); p.at3((size_t)y0 * W + x1, v01); p.at3((size_t)y1 * W + x0, v10); p.at3((size_t)y1 * W + x1, v11);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (1.f - wy) * ((1.f - wx) * v00[c] + wx * v01[c]) + wy * ((1.f - wx) * v10[c] + wx * v11[c]);
}

// INTENT (CT_ICID_*): the weights of utils/icid.py:42-47 -- float32 constants, as torch.tensor([...]) makes them; the hue-preserving
// intent raises the weight of map 5 (hue difference) to 0.02, the chromatic intent that of map 4 (chroma difference) as well.
// OMIT (omit_maps67): maps 6 and 7 get exponent 0 and torch.pow(x, 0) is 1 for any x, NaN included, so they are exactly dropped: the
// blurred C1^2, C2^2 and C1 C2 that only they read are not taken (8 of the 11 moment planes remain).  <CT_ICID_PERCEPTUAL, false> is
// what ct_frame_icid_f32 / ct_frame_icid_hwc_u8 have always launched.
template <class SA, class SB, int INTENT, bool OMIT>
__global__ __launch_bounds__(kBlock) void icid_tile_kernel(const typename SA::elem *__restrict__ a, const typename SB::elem *__restrict__ b, int H, int W,
                                                           int f, int h, int w_, double *__restrict__ partials) {
    constexpr int NP = OMIT ? 8 : 11;                   // moment planes: muL1 muC1 muL2 muC2 L1^2 L2^2 [C1^2 C2^2] sqrt(H) L1L2 [C1C2]
    constexpr int iH = OMIT ? 6 : 8, iL12 = OMIT ? 7 : 9;
    constexpr float wC = INTENT == CT_ICID_CHROMATIC ? 0.02f : 0.002f;          // weights[3], chroma difference
    constexpr float wH = INTENT == CT_ICID_PERCEPTUAL ? 0.002f : 0.02f;         // weights[4], hue difference
    // base planes: L1, C1, L2, C2, sqrt(H) of utils/icid.py:69-111
    __shared__ float base[5][kIcTH + kHalo][kIcTW + kHalo];
    __shared__ float hb[NP][kIcTH + kHalo][kIcTW];
    __shared__ float w[kTaps];
    __shared__ float tab[SA::kTable || SB::kTable ? 256 : 1];
    __shared__ double red[4];
    const int img = blockIdx.z;
    const int ox = blockIdx.x * kIcTW, oy = blockIdx.y * kIcTH;
    gauss_weights(w, 2.0f);
    if constexpr (SA::kTable || SB::kTable) {
        fill_u8_table_f32(tab);
        __syncthreads();
    }
    const SA pa(a, img, H, W, tab);
    const SB pb(b, img, H, W, tab);
    for (int i = threadIdx.x; i < (kIcTH + kHalo) * (kIcTW + kHalo); i += kBlock) {
        const int r = i / (kIcTW + kHalo), c = i % (kIcTW + kHalo);
        const int y = reflect(oy + r - 5, h), x = reflect(ox + c - 5, w_);
        float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (y >= 0 && y < h && x >= 0 && x < w_) {       // tiles past the image edge: unused entries
            float L1, A1, B1, L2, A2, B2, ra[3], rb[3];
            bilinear_down3(pa, H, W, f, y, x, ra);
            bilinear_down3(pb, H, W, f, y, x, rb);
            rgb_to_lab_f32(ra[0], ra[1], ra[2], L1, A1, B1);
            rgb_to_lab_f32(rb[0], rb[1], rb[2], L2, A2, B2);
            const float C1 = sqrtf(A1 * A1 + B1 * B1), C2 = sqrtf(A2 * A2 + B2 * B2);
            const float dA = A1 - A2, dB = B1 - B2, dC = C1 - C2;
            const float Hd = dA * dA + dB * dB - dC * dC;
            v[0] = L1; v[1] = C1; v[2] = L2; v[3] = C2; v[4] = sqrtf(Hd < 0.f ? 0.f : Hd);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) base[q][r][c] = v[q];
    }
    __syncthreads();
    // L and C moments about pivots of the tile (a map pixel near its middle): with L near 100 the sums of L^2 carry a float32
    // rounding of 1e-3 against the maps' constant 10, which on a saturated frame put |sL12| above sL1 sL2 and iCID below 0
    const int pr = 5 + min(kIcTH / 2, h - 1 - oy), pc = 5 + min(kIcTW / 2, w_ - 1 - ox);
    const float p0 = base[0][pr][pc], p1 = base[1][pr][pc], p2 = base[2][pr][pc], p3 = base[3][pr][pc];
    for (int i = threadIdx.x; i < (kIcTH + kHalo) * kIcTW; i += kBlock) {
        const int r = i / kIcTW, c = i % kIcTW;
        float m[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) m[q] = 0.f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const float g = w[k], L1 = base[0][r][c + k] - p0, C1 = base[1][r][c + k] - p1, L2 = base[2][r][c + k] - p2,
                        C2 = base[3][r][c + k] - p3;
            m[0] = fmaf(g, L1, m[0]); m[1] = fmaf(g, C1, m[1]); m[2] = fmaf(g, L2, m[2]); m[3] = fmaf(g, C2, m[3]);
            m[4] = fmaf(g, L1 * L1, m[4]); m[5] = fmaf(g, L2 * L2, m[5]);
            if constexpr (!OMIT) { m[6] = fmaf(g, C1 * C1, m[6]); m[7] = fmaf(g, C2 * C2, m[7]); }
            m[iH] = fmaf(g, base[4][r][c + k], m[iH]); m[iL12] = fmaf(g, L1 * L2, m[iL12]);
            if constexpr (!OMIT) m[10] = fmaf(g, C1 * C2, m[10]);
        }
#pragma unroll
        for (int q = 0; q < NP; ++q) hb[q][r][c] = m[q];
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = threadIdx.x; i < kIcTH * kIcTW; i += kBlock) {
        const int r = i / kIcTW, c = i % kIcTW;
        if (oy + r < h && ox + c < w_) {
            float m[NP];
#pragma unroll
            for (int q = 0; q < NP; ++q) m[q] = 0.f;
#pragma unroll
            for (int k = 0; k < kTaps; ++k) {
#pragma unroll
                for (int q = 0; q < NP; ++q) m[q] = fmaf(w[k], hb[q][r + k][c], m[q]);
            }
            const float muL1 = m[0], muC1 = m[1], muL2 = m[2], muC2 = m[3];      // about the pivots, like the second moments
            const float sL1q = fmaxf(m[4] - muL1 * muL1, 0.f), sL2q = fmaxf(m[5] - muL2 * muL2, 0.f);
            const float sL1 = sqrtf(sL1q), sL2 = sqrtf(sL2q);
            const float dL = (muL1 - muL2) + (p0 - p2), dC = (muC1 - muC2) + (p1 - p3);
            const float dLq = dL * dL, dCq = dC * dC, dHq = m[iH] * m[iH];
            const float sL12 = m[iL12] - muL1 * muL2;
            // weights (0.002, 10, 10, wC, wH, 10, 10) -- 0.002 and 0.002 for the perceptual intent --, exponents (1, 1, 3, 1, 1, 1, 1)
            const float m1 = 1.f / (0.002f * dLq + 1.f);
            const float m2 = (10.f + 2.f * sL1 * sL2) / (10.f + sL1q + sL2q);
            const float m3 = (10.f + fabsf(sL12)) / (10.f + sL1 * sL2);
            const float m4 = 1.f / (wC * dCq + 1.f);
            const float m5 = 1.f / (wH * dHq + 1.f);
            if constexpr (OMIT) {
                acc += (double)(m1 * m2 * (m3 * m3 * m3) * m4 * m5);
            } else {
                const float sC1q = fmaxf(m[6] - muC1 * muC1, 0.f), sC2q = fmaxf(m[7] - muC2 * muC2, 0.f);
                const float sC1 = sqrtf(sC1q), sC2 = sqrtf(sC2q);
                const float sC12 = m[10] - muC1 * muC2;
                const float m6 = (10.f + 2.f * sC1 * sC2) / (10.f + sC1 * sC1 + sC2 * sC2);
                const float m7 = (10.f + fabsf(sC12)) / (10.f + sC1 * sC2);
                acc += (double)(m1 * m2 * (m3 * m3 * m3) * m4 * m5 * m6 * m7);
            }
        }
    }
    acc = block_reduce_1(acc, red);
    if (threadIdx.x == 0) partials[((size_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = acc;
}

// out[i] = scale * (sum of the `n` partials of item i, per_item of them contiguous) / count + bias, added in a fixed order
__global__ __launch_bounds__(kBlock) void metric_finish_kernel(const double *__restrict__ partials, int per_item, double count, double scale,
                                                               double bias, double *__restrict__ out) {
    __shared__ double red[4];
    double s = 0.0;
    for (int i = threadIdx.x; i < per_item; i += kBlock) s += partials[(size_t)blockIdx.x * per_item + i];
    s = block_reduce_1(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = scale * (s / count) + bias;
}

static int metric_factor(int height, int width) {          // max(1, round(min(H, W) / 256)) with Python's round-half-even
    const int m = height < width ? height : width;
    const double q = (double)m / 256.0;
    double r = __builtin_floor(q + 0.5);
    if (q + 0.5 == r && ((long long)r % 2)) r -= 1.0;      // exact .5 -> even
    return r < 1.0 ? 1 : (int)r;
}

// -------------------------------------------------------------------------------------------
// Per-frame PSNR (the metric Runner.test_step logs, methods/__init__.py:32,37; piq.psnr semantics: inputs
// clamped by the caller, data_range 1, mean squared error over all elements of a frame, 10 log10(1/mse)).
// Deterministic: float64 partial sums per workgroup, fixed-order finish.  grid = (G, batch).
// -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sqerr_partial_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                               int64_t n, double *__restrict__ partials) {
    __shared__ double lds[4];
    const float *pa = a + (size_t)blockIdx.y * n, *pb = b + (size_t)blockIdx.y * n;
    double s[1] = {0.0};
    const bool vec = ((reinterpret_cast<uintptr_t>(pa) | reinterpret_cast<uintptr_t>(pb)) & 15) == 0;
    const int64_t n4 = vec ? (n >> 2) : 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n4; i += (int64_t)gridDim.x * kBlock) {
        const float4 x = reinterpret_cast<const float4 *>(pa)[i], y = reinterpret_cast<const float4 *>(pb)[i];
        const double d0 = (double)x.x - y.x, d1 = (double)x.y - y.y, d2 = (double)x.z - y.z, d3 = (double)x.w - y.w;
        s[0] += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
    for (int64_t i = (n4 << 2) + (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const double d = (double)pa[i] - pb[i];
        s[0] += d * d;
    }
    block_sum<1>(s, lds);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * kMaxBlocksPerImage + blockIdx.x] = s[0];
}

__global__ __launch_bounds__(kBlock) void psnr_finish_kernel(const double *__restrict__ partials, int n_blocks, int stride, int64_t n,
                                                             double *__restrict__ out) {
    __shared__ double lds[4];
    double s[1] = {0.0};
    for (int i = threadIdx.x; i < n_blocks; i += kBlock) s[0] += partials[(size_t)blockIdx.x * stride + i];
    block_sum<1>(s, lds);
    if (threadIdx.x == 0) {
        const double mse = s[0] / (double)n;
        out[blockIdx.x * 2] = mse;
        out[blockIdx.x * 2 + 1] = 10.0 * log10(1.0 / (mse > 1e-300 ? mse : 1e-300));
    }
}

int launch_sqerr_partials(const float *a, const float *b, int64_t n, int batch, double *partials, int *n_blocks, hipStream_t s) {
    const int G = blocks_per_image(n >> 2, batch);
    *n_blocks = G;
    hipLaunchKernelGGL(sqerr_partial_kernel, dim3(G, batch), dim3(kBlock), 0, s, a, b, n, partials);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int launch_psnr_finish(const double *partials, int n_blocks, int stride, int64_t n, int batch, double *out, hipStream_t s) {
    hipLaunchKernelGGL(psnr_finish_kernel, dim3(batch), dim3(kBlock), 0, s, partials, n_blocks, stride, n, out);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

static size_t metric_workspace_bytes(int height, int width, int batch) {
    if (height < 1 || width < 1 || batch < 0) return 0;
    const int f = metric_factor(height, width);
    const size_t t_ssim = (size_t)((width / f + kSsTW - 1) / kSsTW) * ((height / f + kSsTH - 1) / kSsTH) * 3;
    const size_t t_icid = (size_t)((width / f + kIcTW - 1) / kIcTW) * ((height / f + kIcTH - 1) / kIcTH);
    return (t_ssim > t_icid ? t_ssim : t_icid) * (size_t)batch * sizeof(double) + 64;
}

// the SSIM / iCID entries of one pair of frame sources: checks, the tile launch, the finishing launch
template <class SA, class SB>
static int frame_ssim(const typename SA::elem *a, const typename SB::elem *b, int height, int width, int batch, double *out, void *ws, size_t ws_bytes,
                      void *stream) {
    if (!a || !b || !out || height < 1 || width < 1 || batch < 0) return CT_E_BADARG;
    if (batch == 0) return CT_OK;
    const int f = metric_factor(height, width);
    const int Hp = height / f, Wp = width / f;
    if (Hp < kTaps || Wp < kTaps) return CT_E_BADARG;                          // piq asserts the kernel fits the image
    if (!ws || ws_bytes < metric_workspace_bytes(height, width, batch)) return CT_E_WORKSPACE;
    const int Ho = Hp - kHalo, Wo = Wp - kHalo;
    const int tx = (Wo + kSsTW - 1) / kSsTW, ty = (Ho + kSsTH - 1) / kSsTH;
    constexpr size_t lds = ssim_lds_bytes(SA::kHwc ? 3 : 1);
    auto kern = ssim_tile_kernel<SA, SB>;
    static DynLdsAttr attr;             // per instantiation, per device (the HWC form takes 69 KB)
    {
        const hipError_t e = attr.ensure(reinterpret_cast<const void *>(kern), lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kern, dim3(tx, ty, SA::kHwc ? batch : batch * 3), dim3(kBlock), lds, (hipStream_t)stream, a, b, height, width, f, Hp, Wp,
                       (double *)ws);
    CT_CHECK_LAUNCH();
    hipLaunchKernelGGL(metric_finish_kernel, dim3(batch), dim3(kBlock), 0, (hipStream_t)stream, (const double *)ws, tx * ty * 3, (double)Ho * Wo * 3.0,
                       1.0, 0.0, out);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

// iCID's map grid: the frame itself (downsampling off, or f == 1), else what F.interpolate(scale_factor = 1 / f) makes of it
static void icid_grid(int height, int width, int downsampling, int *f, int *h, int *w) {
    *f = downsampling ? metric_factor(height, width) : 1;
    *h = (int)__builtin_floor((double)height * (1.0 / *f));
    *w = (int)__builtin_floor((double)width * (1.0 / *f));
}

// one partial per tile of the map grid that `downsampling` selects; with it on, never more than metric_workspace_bytes
static size_t icid_workspace_bytes(int height, int width, int batch, int downsampling) {
    if (height < 1 || width < 1 || batch < 0) return 0;
    int f, h, w;
    icid_grid(height, width, downsampling, &f, &h, &w);
    return (size_t)((w + kIcTW - 1) / kIcTW) * ((h + kIcTH - 1) / kIcTH) * (size_t)batch * sizeof(double) + 64;
}

// options: the ct_frame_icid_opt_* entries, which size their workspace by ct_icid_workspace_bytes; the entries without options pass
// (CT_ICID_PERCEPTUAL, 0, 1) and keep ct_metric_workspace_bytes
template <class SA, class SB>
static int frame_icid(const typename SA::elem *a, const typename SB::elem *b, int height, int width, int batch, int intent, int omit_maps67,
                      int downsampling, bool options, double *out, void *ws, size_t ws_bytes, void *stream) {
    if (!a || !b || !out || height < 1 || width < 1 || batch < 0) return CT_E_BADARG;
    if (intent < CT_ICID_PERCEPTUAL || intent > CT_ICID_CHROMATIC) return CT_E_BADARG;
    if (batch == 0) return CT_OK;
    int f, h, w;
    icid_grid(height, width, downsampling, &f, &h, &w);
    if (h < 6 || w < 6) return CT_E_BADARG;                                    // reflect padding of 5 needs more than 5 pixels
    const size_t need = options ? icid_workspace_bytes(height, width, batch, downsampling) : metric_workspace_bytes(height, width, batch);
    if (!ws || ws_bytes < need) return CT_E_WORKSPACE;
    typedef void (*Kernel)(const typename SA::elem *, const typename SB::elem *, int, int, int, int, int, double *);
    static const Kernel kernels[3][2] = {
        {icid_tile_kernel<SA, SB, CT_ICID_PERCEPTUAL, false>, icid_tile_kernel<SA, SB, CT_ICID_PERCEPTUAL, true>},
        {icid_tile_kernel<SA, SB, CT_ICID_HUE_PRESERVING, false>, icid_tile_kernel<SA, SB, CT_ICID_HUE_PRESERVING, true>},
        {icid_tile_kernel<SA, SB, CT_ICID_CHROMATIC, false>, icid_tile_kernel<SA, SB, CT_ICID_CHROMATIC, true>}};
    const dim3 grid((w + kIcTW - 1) / kIcTW, (h + kIcTH - 1) / kIcTH, batch);
    hipLaunchKernelGGL(kernels[intent][omit_maps67 ? 1 : 0], grid, dim3(kBlock), 0, (hipStream_t)stream, a, b, height, width, f, h, w, (double *)ws);
    CT_CHECK_LAUNCH();
    hipLaunchKernelGGL(metric_finish_kernel, dim3(batch), dim3(kBlock), 0, (hipStream_t)stream, (const double *)ws, (int)(grid.x * grid.y), (double)h * w,
                       -1.0, 1.0, out);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // namespace ct

extern "C" {

size_t ct_metric_workspace_bytes(int height, int width, int batch) { return ct::metric_workspace_bytes(height, width, batch); }

int ct_frame_ssim_f32(const float *a, const float *b, int height, int width, int batch, double *out, void *ws, size_t ws_bytes, void *stream) {
    return ct::frame_ssim<ct::PlanarF32, ct::PlanarF32>(a, b, height, width, batch, out, ws, ws_bytes, stream);
}

int ct_frame_icid_f32(const float *a, const float *b, int height, int width, int batch, double *out, void *ws, size_t ws_bytes, void *stream) {
    return ct::frame_icid<ct::PlanarF32, ct::PlanarF32>(a, b, height, width, batch, CT_ICID_PERCEPTUAL, 0, 1, false, out, ws, ws_bytes, stream);
}

size_t ct_icid_workspace_bytes(int height, int width, int batch, int downsampling) { return ct::icid_workspace_bytes(height, width, batch, downsampling); }

int ct_frame_icid_opt_f32(const float *a, const float *b, int height, int width, int batch, int intent, int omit_maps67, int downsampling, double *out,
                          void *ws, size_t ws_bytes, void *stream) {
    return ct::frame_icid<ct::PlanarF32, ct::PlanarF32>(a, b, height, width, batch, intent, omit_maps67, downsampling, true, out, ws, ws_bytes, stream);
}

// the same metrics read from a frame group's own buffers: the result as float32 HWC (clamped as it is read), the ground truth as bytes
int ct_frame_ssim_hwc_u8(const float *result_hwc, const uint8_t *gt_hwc, int height, int width, int batch, double *out, void *ws, size_t ws_bytes,
                         void *stream) {
    return ct::frame_ssim<ct::ResultHwcF32, ct::GtHwcU8>(result_hwc, gt_hwc, height, width, batch, out, ws, ws_bytes, stream);
}

int ct_frame_icid_hwc_u8(const float *result_hwc, const uint8_t *gt_hwc, int height, int width, int batch, double *out, void *ws, size_t ws_bytes,
                         void *stream) {
    return ct::frame_icid<ct::ResultHwcF32, ct::GtHwcU8>(result_hwc, gt_hwc, height, width, batch, CT_ICID_PERCEPTUAL, 0, 1, false, out, ws, ws_bytes,
                                                         stream);
}

int ct_frame_icid_opt_hwc_u8(const float *result_hwc, const uint8_t *gt_hwc, int height, int width, int batch, int intent, int omit_maps67,
                             int downsampling, double *out, void *ws, size_t ws_bytes, void *stream) {
    return ct::frame_icid<ct::ResultHwcF32, ct::GtHwcU8>(result_hwc, gt_hwc, height, width, batch, intent, omit_maps67, downsampling, true, out, ws,
                                                         ws_bytes, stream);
}

int ct_frame_psnr_f32(const float *a, const float *b, int64_t n_elems, int batch, double *out, void *ws, size_t ws_bytes, void *stream) {
    if (!a || !b || !out || n_elems < 1 || batch < 0) return CT_E_BADARG;
    if (!ws || ws_bytes < (size_t)batch * ct::kMaxBlocksPerImage * sizeof(double)) return CT_E_WORKSPACE;
    if (batch == 0) return CT_OK;
    int G = 0;
    const int rc = ct::launch_sqerr_partials(a, b, n_elems, batch, (double *)ws, &G, (hipStream_t)stream);
    if (rc) return rc;
    return ct::launch_psnr_finish((const double *)ws, G, ct::kMaxBlocksPerImage, n_elems, batch, out, (hipStream_t)stream);
}

}  // extern "C"
