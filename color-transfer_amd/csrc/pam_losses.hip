// pam_losses.hip -- the three parallax-attention losses the reference's step logs (methods/dcmcs3di.py:68-92 through
// pasmnet/losses.py: loss_pam_photometric, loss_pam_cycle, loss_pam_smoothness) as per-image float64 sums over MATERIALISED
// attention maps [n][h][w][w] (what ct_pam_attend_f32 / ct_pam_valid_f32 write), on gfx950.
//
//   ct_pam_cycle_l1_f32   sum_h sum_i mask[h][i] sum_k |(A_h . B_h)[i][k] - delta_ik|: the w x w x w product of every image row on
//                         the exact-f32 MFMA (v_mfma_f32_32x32x2_f32), 64 x 64 output tile per workgroup, K staged through LDS in
//                         chunks of 32; the accumulator tile goes through |c - delta| * m in registers, the product is never stored.
//   ct_pam_map_sweep_f32  one pass over one map: vertical and diagonal smoothness sums, the warp-and-compare (photometric) sum, the
//                         identity sum.  A wave owns one query row i of one image and marches down a segment of kSweepSeg image
//                         rows with the previous row in registers (the vertical term), so the map comes from memory once (plus one
//                         row per segment and wave); the diagonal neighbour att[h][i+1][j+1] is a second, shifted load of a row
//                         that the next wave is reading at the same time (cache, not memory).
//   ct_masked_l1_f32      the reference's masked_l1_loss on tensors that are already there: sum |x - y| * mask and sum mask.
//
// Every term is formed in float32 as the reference's torch code forms it (the product as a float32 fma chain, |x - y| * mask as two
// float32 operations) and widened to float64 before it is added.  A workgroup leaves float64 partial sums, a finishing kernel adds an
// image's partials in a fixed order and counts the mask: deterministic, no atomics.  Counts that are zero stay zero: the division
// (and its 0 / 0 = NaN, as in the reference) is the caller's.
#include "ct_common.h"
#include "ct_split16.h"      // f32x16

namespace ct {
namespace pl {

constexpr int kCyTile = 64, kCyK = 32;
constexpr int kCyLdA = 36;            // A chunk [64 rows][32 k] + 4: 16-byte rows, conflict-free 16-byte operand reads
constexpr int kCyLdB = 66;            // B chunk [32 k][64 columns] + 2: the two k-halves of a wave read banks 32 apart
constexpr int kSweepSeg = 8;          // image rows per sweep workgroup
constexpr int kSweepMaxW = 1024;      // 16 columns per lane
constexpr int kMl1Blocks = 64;        // workgroups per image of ct_masked_l1_f32

// grid (tiles * tiles, h, n); partials [n][h][tiles * tiles].  Within a chunk of 32 the MFMA step s contracts k = s and k = 16 + s
// (a fixed order; the sum does not care, the rounding is that of a float32 fma chain either way).
__global__ __launch_bounds__(kBlock) void pam_cycle_tile_kernel(const float *__restrict__ A, const float *__restrict__ B,
                                                                const float *__restrict__ mask, int H, int W, int tiles,
                                                                double *__restrict__ partials) {
    __shared__ __attribute__((aligned(16))) float sA[kCyTile * kCyLdA];
    __shared__ float sB[kCyK * kCyLdB];
    __shared__ double red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = ((int)blockIdx.x / tiles) * kCyTile, n0 = ((int)blockIdx.x % tiles) * kCyTile;
    const size_t row = (size_t)blockIdx.z * H + blockIdx.y;                 // (image, image row)
    const float *a = A + row * W * W, *b = B + row * W * W;
    const int ak = tid & 31, am = tid >> 5;                                  // A rows am + 8 j, column k0 + ak
    const int bn = tid & 63, bk = tid >> 6;                                  // B rows k0 + bk + 4 j, column n0 + bn
    float ra[8], rb[8];
    // ragged tiles: zeros, so that padded rows / columns of the product are exactly zero
    auto fetch = [&](int k0) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int m = m0 + am + 8 * j, k = k0 + ak;
            ra[j] = (m < W && k < W) ? a[(size_t)m * W + k] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = k0 + bk + 4 * j, n = n0 + bn;
            rb[j] = (k < W && n < W) ? b[(size_t)k * W + n] : 0.f;
        }
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32, l31 = lane & 31, kh = lane >> 5;
    fetch(0);
    for (int k0 = 0; k0 < W; k0 += kCyK) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sA[(am + 8 * j) * kCyLdA + ak] = ra[j];
            sB[(bk + 4 * j) * kCyLdB + bn] = rb[j];
        }
        __syncthreads();
        if (k0 + kCyK < W) fetch(k0 + kCyK);                                 // the next chunk is in flight under the MFMAs
        float4 av[4];
        float bv[16];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) av[s4] = *reinterpret_cast<const float4 *>(&sA[(wm + l31) * kCyLdA + 16 * kh + 4 * s4]);
#pragma unroll
        for (int s = 0; s < 16; ++s) bv[s] = sB[(16 * kh + s) * kCyLdB + wn + l31];
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s4].x, bv[4 * s4], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s4].y, bv[4 * s4 + 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s4].z, bv[4 * s4 + 2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s4].w, bv[4 * s4 + 3], acc, 0, 0, 0);
        }
        __syncthreads();                                                     // the chunk is consumed
    }
    // the lane holds column l31 of the wave's tile, rows (r & 3) + 8 (r >> 2) + 4 kh.  Only rows and columns inside the map count:
    // a padded diagonal element would otherwise add |0 - 1|
    double s[1] = {0.0};
    const int col = n0 + wn + l31;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = m0 + wm + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (i < W && col < W) s[0] += (double)(fabsf(acc[r] - (i == col ? 1.f : 0.f)) * mask[row * W + i]);
    }
    block_sum<1>(s, red);
    if (tid == 0) partials[row * tiles * tiles + blockIdx.x] = s[0];
}

// grid (ceil(w / 4), ceil(h / kSweepSeg), n); partials [n][segments][ceil(w / 4)][4] = vertical, diagonal, photometric, identity.
// A wave owns query row i; a lane owns columns lane + 64 t.
template <int T>
__global__ __launch_bounds__(kBlock) void pam_sweep_kernel(const float *__restrict__ att, const float *__restrict__ src,
                                                           const float *__restrict__ dst, const float *__restrict__ mask, int H, int W,
                                                           double *__restrict__ partials) {
    __shared__ double red[4 * 4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = (int)blockIdx.x * 4 + wave, img = blockIdx.z;
    const int h0 = (int)blockIdx.y * kSweepSeg, h1 = min(h0 + kSweepSeg, H);
    const int hl = min(h1, H - 1);                                           // the row after the segment closes its last vertical pair
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < W) {                                                             // wave-uniform
        float cur[T], prev[T];
        {
            const float *p = att + (((size_t)img * H + h0) * W + i) * W;
#pragma unroll
            for (int t = 0; t < T; ++t) { const int j = lane + 64 * t; cur[t] = j < W ? p[j] : 0.f; prev[t] = 0.f; }
        }
        for (int h = h0; h <= hl; ++h) {
            const float *p = att + (((size_t)img * H + h) * W + i) * W;
            float nx[T];
#pragma unroll
            for (int t = 0; t < T; ++t) { const int j = lane + 64 * t; nx[t] = (h < hl && j < W) ? p[(size_t)W * W + j] : 0.f; }
            if (h > h0) {
#pragma unroll
                for (int t = 0; t < T; ++t)
                    if (lane + 64 * t < W) acc[0] += (double)fabsf(prev[t] - cur[t]);
            }
            if (h < h1) {
                if (i + 1 < W) {
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const int j = lane + 64 * t;
                        if (j + 1 < W) acc[1] += (double)fabsf(cur[t] - p[W + j + 1]);
                    }
                }
                if (mask) {
                    const float m = mask[((size_t)img * H + h) * W + i];
#pragma unroll
                    for (int t = 0; t < T; ++t) {
                        const int j = lane + 64 * t;
                        if (j < W) acc[3] += (double)(fabsf(cur[t] - (j == i ? 1.f : 0.f)) * m);
                    }
                    if (src) {
                        // warp[c] = sum_j att[i][j] src[c][h][j]: float32 products chained per lane, the 64 lane sums added in float64
                        float pc[3] = {0.f, 0.f, 0.f};
#pragma unroll
                        for (int t = 0; t < T; ++t) {
                            const int j = lane + 64 * t;
                            if (j < W) {
#pragma unroll
                                for (int c = 0; c < 3; ++c) pc[c] = fmaf(cur[t], src[(((size_t)img * 3 + c) * H + h) * W + j], pc[c]);
                            }
                        }
                        double pd[3] = {(double)pc[0], (double)pc[1], (double)pc[2]};
#pragma unroll
                        for (int off = kWave / 2; off > 0; off >>= 1) {
#pragma unroll
                            for (int c = 0; c < 3; ++c) pd[c] += __shfl_down(pd[c], off, kWave);
                        }
                        if (lane == 0) {
#pragma unroll
                            for (int c = 0; c < 3; ++c)
                                acc[2] += (double)(fabsf(dst[(((size_t)img * 3 + c) * H + h) * W + i] - (float)pd[c]) * m);
                        }
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < T; ++t) { prev[t] = cur[t]; cur[t] = nx[t]; }
        }
    }
    block_sum<4>(acc, red);
    if (threadIdx.x == 0) {
        double *p = partials + (((size_t)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 4;
        p[0] = acc[0]; p[1] = acc[1]; p[2] = acc[2]; p[3] = acc[3];
    }
}

// x, y [n][a][p][b], mask [n][p]; grid (kMl1Blocks, n); partials [n][kMl1Blocks]
__global__ __launch_bounds__(kBlock) void masked_l1_kernel(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ mask,
                                                           int64_t a, int64_t p, int64_t b, double *__restrict__ partials) {
    __shared__ double red[4];
    const int64_t total = a * p * b;
    const float *xi = x + (size_t)blockIdx.y * total, *yi = y + (size_t)blockIdx.y * total, *mi = mask + (size_t)blockIdx.y * p;
    double s[1] = {0.0};
    for (int64_t idx = (int64_t)blockIdx.x * kBlock + threadIdx.x; idx < total; idx += (int64_t)kMl1Blocks * kBlock)
        s[0] += (double)(fabsf(xi[idx] - yi[idx]) * mi[(idx / b) % p]);
    block_sum<1>(s, red);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * kMl1Blocks + blockIdx.x] = s[0];
}

// out[image][q] = the image's per_image partials of quantity q < NV, added in a fixed order; out[image][NV] = sum of its mask_len
// mask values (0 without a mask); grid = n
template <int NV>
__global__ __launch_bounds__(kBlock) void pam_losses_finish_kernel(const double *__restrict__ partials, int64_t per_image,
                                                                   const float *__restrict__ mask, int64_t mask_len, double *__restrict__ out) {
    __shared__ double red[4 * (NV + 1)];
    const double *p = partials + (size_t)blockIdx.x * per_image * NV;
    double s[NV + 1];
#pragma unroll
    for (int q = 0; q <= NV; ++q) s[q] = 0.0;
    for (int64_t k = threadIdx.x; k < per_image; k += kBlock) {
#pragma unroll
        for (int q = 0; q < NV; ++q) s[q] += p[k * NV + q];
    }
    if (mask)
        for (int64_t k = threadIdx.x; k < mask_len; k += kBlock) s[NV] += (double)mask[(size_t)blockIdx.x * mask_len + k];
    block_sum<NV + 1>(s, red);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q <= NV; ++q) out[(size_t)blockIdx.x * (NV + 1) + q] = s[q];
    }
}

inline size_t cycle_partials(int n, int h, int w) {
    const size_t tiles = (size_t)(w + kCyTile - 1) / kCyTile;
    return (size_t)n * h * tiles * tiles;
}
inline size_t sweep_partials(int n, int h, int w) {
    return (size_t)n * ((h + kSweepSeg - 1) / kSweepSeg) * ((w + 3) / 4) * 4;
}
inline bool off(const void *p, size_t align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

}  // namespace pl
}  // namespace ct

extern "C" {

size_t ct_pam_losses_workspace_bytes(int n, int h, int w) {
    using namespace ct::pl;
    if (n < 1 || h < 1 || w < 1) return 0;
    size_t need = cycle_partials(n, h, w);
    if (sweep_partials(n, h, w) > need) need = sweep_partials(n, h, w);
    if ((size_t)n * kMl1Blocks > need) need = (size_t)n * kMl1Blocks;
    return need * sizeof(double);
}

int ct_pam_cycle_l1_f32(const float *att_a, const float *att_b, const float *mask, double *out, void *ws, size_t ws_bytes, int n, int h,
                        int w, void *stream) {
    using namespace ct::pl;
    if (!att_a || !att_b || !mask || !out || n < 1 || n > 65535 || h < 1 || h > 65535 || w < 1) return CT_E_BADARG;
    const int64_t tiles = (w + kCyTile - 1) / kCyTile;
    if (tiles * tiles > 0x7fffffffLL) return CT_E_BADARG;
    if (!ws || ws_bytes < cycle_partials(n, h, w) * sizeof(double) || off(ws, sizeof(double))) return CT_E_WORKSPACE;
    if (off(att_a, sizeof(float)) || off(att_b, sizeof(float)) || off(mask, sizeof(float)) || off(out, sizeof(double))) return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pam_cycle_tile_kernel, dim3((unsigned)(tiles * tiles), h, n), dim3(ct::kBlock), 0, s, att_a, att_b, mask, h, w, (int)tiles,
                       reinterpret_cast<double *>(ws));
    CT_CHECK_LAUNCH();
    hipLaunchKernelGGL(pam_losses_finish_kernel<1>, dim3(n), dim3(ct::kBlock), 0, s, reinterpret_cast<const double *>(ws),
                       (int64_t)h * tiles * tiles, mask, (int64_t)h * w, out);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_pam_map_sweep_f32(const float *att, const float *src, const float *dst, const float *mask, double *out, void *ws, size_t ws_bytes,
                         int n, int h, int w, void *stream) {
    using namespace ct::pl;
    if (!att || !out || n < 1 || n > 65535 || h < 1 || w < 1 || w > kSweepMaxW) return CT_E_BADARG;
    if ((src == nullptr) != (dst == nullptr) || (src && !mask)) return CT_E_BADARG;      // the photometric term needs all three
    const dim3 grid((w + 3) / 4, (h + kSweepSeg - 1) / kSweepSeg, n);
    if (grid.y > 65535u) return CT_E_BADARG;
    if (!ws || ws_bytes < sweep_partials(n, h, w) * sizeof(double) || off(ws, sizeof(double))) return CT_E_WORKSPACE;
    if (off(att, sizeof(float)) || off(src, sizeof(float)) || off(dst, sizeof(float)) || off(mask, sizeof(float)) || off(out, sizeof(double)))
        return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    double *part = reinterpret_cast<double *>(ws);
    const int t = (w + 63) / 64;
    if (t <= 1) hipLaunchKernelGGL(pam_sweep_kernel<1>, grid, dim3(ct::kBlock), 0, s, att, src, dst, mask, h, w, part);
    else if (t <= 2) hipLaunchKernelGGL(pam_sweep_kernel<2>, grid, dim3(ct::kBlock), 0, s, att, src, dst, mask, h, w, part);
    else if (t <= 4) hipLaunchKernelGGL(pam_sweep_kernel<4>, grid, dim3(ct::kBlock), 0, s, att, src, dst, mask, h, w, part);
    else if (t <= 8) hipLaunchKernelGGL(pam_sweep_kernel<8>, grid, dim3(ct::kBlock), 0, s, att, src, dst, mask, h, w, part);
    else hipLaunchKernelGGL(pam_sweep_kernel<16>, grid, dim3(ct::kBlock), 0, s, att, src, dst, mask, h, w, part);
    CT_CHECK_LAUNCH();
    hipLaunchKernelGGL(pam_losses_finish_kernel<4>, dim3(n), dim3(ct::kBlock), 0, s, reinterpret_cast<const double *>(ws),
                       (int64_t)grid.x * grid.y, mask, (int64_t)h * w, out);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_masked_l1_f32(const float *x, const float *y, const float *mask, double *out, void *ws, size_t ws_bytes, int n, int64_t a, int64_t p,
                     int64_t b, void *stream) {
    using namespace ct::pl;
    if (!x || !y || !mask || !out || n < 1 || n > 65535 || a < 1 || p < 1 || b < 1) return CT_E_BADARG;
    if (a > (int64_t)1 << 40 || p > (int64_t)1 << 40 || b > (int64_t)1 << 40 || a * p > (int64_t)1 << 40 || a * p * b > (int64_t)1 << 40)
        return CT_E_BADARG;
    if (!ws || ws_bytes < (size_t)n * kMl1Blocks * sizeof(double) || off(ws, sizeof(double))) return CT_E_WORKSPACE;
    if (off(x, sizeof(float)) || off(y, sizeof(float)) || off(mask, sizeof(float)) || off(out, sizeof(double))) return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(masked_l1_kernel, dim3(kMl1Blocks, n), dim3(ct::kBlock), 0, s, x, y, mask, a, p, b, reinterpret_cast<double *>(ws));
    CT_CHECK_LAUNCH();
    hipLaunchKernelGGL(pam_losses_finish_kernel<1>, dim3(n), dim3(ct::kBlock), 0, s, reinterpret_cast<const double *>(ws), (int64_t)kMl1Blocks, mask,
                       p, out);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
