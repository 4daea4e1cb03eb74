// ct_ssim_map.h -- the per-channel SSIM map of kornia.metrics.ssim (window 11, sigma 1.5, reflect padding of 5; restated, see
// errmaps.hip) on one 64 x 32 tile: what the rgbssim view (errmaps.hip) and the SSIM loss (losses.hip) share, so that both see the
// same floats.  A kernel stages x and y with stage_plane, synchronises, runs ssim_rows, synchronises, and takes its thread's
// eight values from ssim_columns; sx / sy may be staged again after the second barrier, hb after the one that follows ssim_columns.
#pragma once
#include "ct_common.h"

namespace ct {
namespace em {

typedef float vf4 __attribute__((ext_vector_type(4)));

constexpr int kTW = 64, kTH = 32, kRad = 5, kTaps = 2 * kRad + 1;
constexpr int kLeft = 8;                                    // staged columns left of the tile: kRad rounded up to 16 bytes
constexpr int kSW = kTW + 2 * kLeft, kSH = kTH + 2 * kRad;  // 80 x 42 staged pixels
constexpr int kStrip = 8;                                   // output rows per thread in the column pass: kBlock = kTW * kTH / kStrip
constexpr int kSsimLds = (2 * kSH * kSW + 5 * kSH * kTW + 8) * (int)sizeof(float);
static_assert(kTW * kTH / kStrip == kBlock && kTW == kWave, "a wave owns one 8-row strip of the tile's 64 columns");
static_assert(kSsimLds <= 80 * 1024, "two workgroups per CU");

struct Taps {
    float v[kTaps];                                         // exp(-k^2 / (2 * 1.5^2)), k = -5 .. 5, normalised: made in float64 on the host
};

// rows oy - 5 .. oy + 36, columns ox - 8 .. ox + 71 of one plane; what no output of the frame needs (beyond 5 pixels outside the
// frame, where the reflected index would leave it again) is zero and is never read for a stored value
__device__ __forceinline__ void stage_plane(const float *__restrict__ p, float *__restrict__ s, int H, int W, int oy, int ox, bool vec) {
    for (int i = threadIdx.x; i < kSH * (kSW / 4); i += kBlock) {
        const int r = i / (kSW / 4), q = i - r * (kSW / 4);
        const int gy = oy + r - kRad, gx0 = ox - kLeft + 4 * q;
        vf4 v = (vf4)(0.0f);
        if (gy >= -kRad && gy < H + kRad) {
            const float *row = p + (int64_t)reflect(gy, H) * W;
            if (vec && gx0 >= 0 && gx0 + 3 < W) {
                v = *reinterpret_cast<const vf4 *>(row + gx0);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int gx = gx0 + e;
                    if (gx >= -kRad && gx < W + kRad) v[e] = row[reflect(gx, W)];
                }
            }
        }
        *reinterpret_cast<vf4 *>(s + r * kSW + 4 * q) = v;
    }
}

// the horizontal 11-tap pass over the staged tile: the five moments of 42 rows x 64 columns into hb
__device__ __forceinline__ void ssim_rows(const float *__restrict__ sx, const float *__restrict__ sy, float *__restrict__ hb, const Taps &taps) {
    for (int i = threadIdx.x; i < kSH * kTW; i += kBlock) {
        const int r = i / kTW, c = i - r * kTW;
        const float *px = sx + r * kSW + c + (kLeft - kRad), *py = sy + r * kSW + c + (kLeft - kRad);
        float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < kTaps; ++k) {
            const float a = px[k], d = py[k], g = taps.v[k];
            m[0] = fmaf(g, a, m[0]); m[1] = fmaf(g, d, m[1]); m[2] = fmaf(g, a * a, m[2]); m[3] = fmaf(g, d * d, m[3]); m[4] = fmaf(g, a * d, m[4]);
        }
#pragma unroll
        for (int q = 0; q < 5; ++q) hb[(q * kSH + r) * kTW + c] = m[q];
    }
}

// the vertical pass and the SSIM formula for rows r0 .. r0 + 7 of column col of the tile
__device__ __forceinline__ void ssim_columns(const float *__restrict__ hb, const Taps &taps, int r0, int col, float (&ssim)[kStrip]) {
    const float c1 = 0.01f * 0.01f, c2 = 0.03f * 0.03f;
    float acc[kStrip][5];
#pragma unroll
    for (int j = 0; j < kStrip; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[j][q] = 0.f;
#pragma unroll
    for (int k = 0; k < kStrip + 2 * kRad; ++k) {
        float v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = hb[(q * kSH + r0 + k) * kTW + col];
#pragma unroll
        for (int j = 0; j < kStrip; ++j) {
            if (k - j >= 0 && k - j < kTaps) {
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[j][q] = fmaf(taps.v[k - j], v[q], acc[j][q]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kStrip; ++j) {
        const float mu1 = acc[j][0], mu2 = acc[j][1];
        const float mu11 = mu1 * mu1, mu22 = mu2 * mu2, mu12 = mu1 * mu2;
        const float s11 = acc[j][2] - mu11, s22 = acc[j][3] - mu22, s12 = acc[j][4] - mu12;
        const float num = (2.0f * mu12 + c1) * (2.0f * s12 + c2);
        const float den = (mu11 + mu22 + c1) * (s11 + s22 + c2);
        ssim[j] = num / (den + 1e-12f);
    }
}

// the taps, made in float64 on the host and rounded once
static inline Taps ssim_taps() {
    Taps taps;
    double g[kTaps], sum = 0.0;
    for (int k = 0; k < kTaps; ++k) { g[k] = __builtin_exp(-(double)((k - kRad) * (k - kRad)) / (2.0 * 1.5 * 1.5)); sum += g[k]; }
    for (int k = 0; k < kTaps; ++k) taps.v[k] = (float)(g[k] / sum);
    return taps;
}

}  // namespace em
}  // namespace ct
