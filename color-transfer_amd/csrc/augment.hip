// augment.hip -- a batch of training / validation samples of the reference's ArtificialTrainValDataset (utils/data.py:25-84) on
// gfx950: the random crop of a stereo pair, the flip that swaps the views, the vertical flip, and apply_uniform_distortions --
// torchvision's adjust_brightness / contrast / saturation / hue / gamma / sharpness in a random order -- on the uint8 crop.  The
// random draws are the host's (utils/data.py here); this file applies them.
//
// The five colour adjustments are distort.hip's device functions (ct_distort.h).  adjust_sharpness is restated from torchvision's
// published _functional_tensor.py (adjust_sharpness, _blurred_degenerate_image, _cast_squeeze_out) -- "parity unpinned", like the
// others.  Its degenerate image is round(conv2d(img, k)) with k = 1/13 and 5/13 at the centre, in float32: the exact sum is a
// whole number of thirteenths, so it is never closer than 0.5 / 13 to a tie, two thousand times the float32 error of any order
// of the nine additions.  The rounding therefore does not depend on that order, and none is imitated here.
//
// A chain is not six pointwise passes.  Contrast in position k blends with the mean grey of the WHOLE crop after operations
// 0 .. k - 1, and sharpness in position k reads the eight neighbours after operations 0 .. k - 1.  Both are served by one device
// function, chain_tile: "the crop after the first k operations" at this thread's pixel of a 32 x 8 tile.  With a sharpness
// among those k operations the workgroup first evaluates the operations before it on the tile plus a one-pixel halo, into LDS
// (340 pixels for 256: the halo is recomputed, never exchanged between workgroups), then blurs, blends and goes on pointwise.
//   grey sums   one launch per contrast of the longest chain (the dataset's chains have one): chain_tile up to that contrast, the
//               integer grey values added by one atomic per workgroup -- exact, so the order does not matter
//   apply       one launch, the sample index on the grid's z axis: chain_tile over the whole chain, then the four outputs
// No cooperative launch, no flag between workgroups: a kernel boundary is the only synchronisation.
#include "ct_common.h"
#include "ct_distort.h"

namespace ct {
namespace aug {

constexpr int kTW = 32, kTH = 8;                            // a workgroup's tile of the crop: one pixel per thread
constexpr int kHW = kTW + 2, kHH = kTH + 2;                 // with the one-pixel halo of the 3 x 3 blur
constexpr int kOps = CT_AUGMENT_MAX_OPS;
static_assert(kTW * kTH == kBlock, "one pixel per thread");

// one sample's crop of its source pair, the flips folded into the index: gt / ref are the planes the sample's NEW gt / reference
// come from (exchanged when the views are swapped).  What indexes memory is clamped: the host entry has checked the host copy
// of the table, the kernels read the device copy.
struct View {
    const uint8_t *gt, *ref;
    int64_t plane;
    int W, top, left, ch, cw;
    bool mirror, vflip;
    __device__ __forceinline__ int64_t at(int y, int x) const {
        return (int64_t)(top + (vflip ? ch - 1 - y : y)) * W + left + (mirror ? cw - 1 - x : x);
    }
};

__device__ __forceinline__ View make_view(const uint8_t *gt, const uint8_t *ref, const ct_augment_sample &sp, int H, int W, int ch, int cw) {
    const int64_t plane = (int64_t)H * W;
    const uint8_t *g = gt + (int64_t)blockIdx.z * 3 * plane, *r = ref + (int64_t)blockIdx.z * 3 * plane;
    const bool swap = sp.swap_hflip != 0;
    View v;
    v.gt = swap ? r : g; v.ref = swap ? g : r;
    v.plane = plane; v.W = W; v.ch = ch; v.cw = cw;
    v.top = min(max(sp.top, 0), H - ch); v.left = min(max(sp.left, 0), W - cw);
    v.mirror = swap; v.vflip = sp.vflip != 0;
    return v;
}

// operations k0 .. k1 - 1 of the chain on one pixel; a sharpness among them is skipped (the caller has dealt with it, or the crop is
// too small for it to act)
__device__ __forceinline__ void pointwise(const ct_augment_sample &sp, const unsigned long long *__restrict__ sums, int64_t npix, int k0, int k1,
                                          float &r, float &g, float &b) {
    for (int k = k0; k < k1; ++k) {
        const int kind = sp.kind[k];
        const float mean = kind == kDistContrast ? gray_mean(sums[k], npix) : 0.f;
        distort_pixel(kind, (float)sp.param[k], (float)sp.one_minus[k], mean, r, g, b);
    }
}

// The crop after operations 0 .. k_end - 1 at pixel (y, x) = this thread's pixel of the workgroup's tile (inside: it lies in the
// crop).  sharp: the position of the chain's sharpness, -1 without one or when the crop is too small for it to act.  Every thread
// of the workgroup calls this with the same sp, k_end and sharp (a barrier inside); halo: LDS [3][kHH * kHW].
__device__ __forceinline__ void chain_tile(const ct_augment_sample &sp, const View &v, const unsigned long long *__restrict__ sums, int k_end, int sharp,
                                           uint8_t *__restrict__ halo, int y, int x, bool inside, float &r, float &g, float &b) {
    const int64_t npix = (int64_t)v.ch * v.cw;
    r = g = b = 0.f;
    if (sharp < 0 || sharp >= k_end) {
        if (inside) {
            const int64_t o = v.at(y, x);
            r = (float)v.gt[o]; g = (float)v.gt[v.plane + o]; b = (float)v.gt[2 * v.plane + o];
            pointwise(sp, sums, npix, 0, k_end, r, g, b);
        }
        return;
    }
    const int y0 = (int)blockIdx.y * kTH - 1, x0 = (int)blockIdx.x * kTW - 1;
    for (int i = threadIdx.x; i < kHH * kHW; i += kBlock) {
        const int hy = y0 + i / kHW, hx = x0 + i % kHW;
        if (hy >= 0 && hy < v.ch && hx >= 0 && hx < v.cw) {  // what lies outside the crop is never read: border pixels are not blurred
            const int64_t o = v.at(hy, hx);
            float pr = (float)v.gt[o], pg = (float)v.gt[v.plane + o], pb = (float)v.gt[2 * v.plane + o];
            pointwise(sp, sums, npix, 0, sharp, pr, pg, pb);
            halo[i] = (uint8_t)pr; halo[kHH * kHW + i] = (uint8_t)pg; halo[2 * kHH * kHW + i] = (uint8_t)pb;
        }
    }
    __syncthreads();
    if (!inside) return;
    const int c = ((int)threadIdx.x / kTW + 1) * kHW + (int)threadIdx.x % kTW + 1;
    const bool interior = y > 0 && y < v.ch - 1 && x > 0 && x < v.cw - 1;
    const float ratio = (float)sp.param[sharp], one_minus = (float)sp.one_minus[sharp];
    const float w1 = 1.0f / 13.0f, w5 = 5.0f / 13.0f;      // ones(3, 3); [1, 1] = 5; /= sum -- in float32
    float px[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const uint8_t *h = halo + q * kHH * kHW + c;
        const float centre = (float)h[0];
        float degenerate = centre;
        if (interior) {
            const int ring = (h[-kHW - 1] + h[-kHW] + h[-kHW + 1]) + (h[-1] + h[1]) + (h[kHW - 1] + h[kHW] + h[kHW + 1]);
            degenerate = rintf(w1 * (float)ring + w5 * centre);   // torch.round: ties to even (no tie occurs, see the head of this file)
        }
        px[q] = blend_u8(centre, degenerate, ratio, one_minus);
    }
    r = px[0]; g = px[1]; b = px[2];
    pointwise(sp, sums, npix, sharp + 1, k_end, r, g, b);
}

__device__ __forceinline__ int clamped_ops(const ct_augment_sample &sp) { return min(max(sp.n_ops, 0), kOps); }

__device__ __forceinline__ int sharpness_position(const ct_augment_sample &sp, int n_ops, int ch, int cw) {
    if (ch <= 2 || cw <= 2) return -1;                      // adjust_sharpness returns its input
    for (int k = 0; k < n_ops; ++k)
        if (sp.kind[k] == kDistSharpness) return k;
    return -1;
}

// grid (tiles_x, tiles_y, n).  level: which contrast of a chain this launch serves (0 = its first); sums [n][kOps], indexed by the
// contrast's position in the chain; the sums of earlier contrasts are complete (earlier launches).
__global__ __launch_bounds__(kBlock) void augment_gray_sum_kernel(const uint8_t *__restrict__ gt, const uint8_t *__restrict__ ref,
                                                                  const ct_augment_sample *__restrict__ table, int H, int W, int ch, int cw, int level,
                                                                  unsigned long long *__restrict__ sums) {
    __shared__ uint8_t halo[3 * kHH * kHW];
    __shared__ unsigned long long red[4];
    const ct_augment_sample &sp = table[blockIdx.z];
    const int n_ops = clamped_ops(sp);
    int pos = -1, seen = 0;
    for (int k = 0; k < n_ops; ++k)
        if (sp.kind[k] == kDistContrast && seen++ == level) { pos = k; break; }
    if (pos < 0) return;                                    // the whole workgroup: this chain has no such contrast
    const View v = make_view(gt, ref, sp, H, W, ch, cw);
    const int y = (int)blockIdx.y * kTH + (int)threadIdx.x / kTW, x = (int)blockIdx.x * kTW + (int)threadIdx.x % kTW;
    const bool inside = y < ch && x < cw;
    float r, g, b;
    chain_tile(sp, v, sums + (size_t)blockIdx.z * kOps, pos, sharpness_position(sp, n_ops, ch, cw), halo, y, x, inside, r, g, b);
    unsigned long long s = inside ? (unsigned long long)gray_u8(r, g, b) : 0ull;
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(sums + (size_t)blockIdx.z * kOps + pos, red[0] + red[1] + red[2] + red[3]);   // integer: order independent, exact
}

// grid (tiles_x, tiles_y, n); outputs [n][3][ch][cw]
__global__ __launch_bounds__(kBlock) void augment_apply_kernel(const uint8_t *__restrict__ gt, const uint8_t *__restrict__ ref,
                                                               const ct_augment_sample *__restrict__ table, int H, int W, int ch, int cw,
                                                               const unsigned long long *__restrict__ sums, float *__restrict__ out_gt,
                                                               float *__restrict__ out_ref, float *__restrict__ out_target, uint8_t *__restrict__ out_u8) {
    __shared__ uint8_t halo[3 * kHH * kHW];
    const ct_augment_sample &sp = table[blockIdx.z];
    const int n_ops = clamped_ops(sp);
    const View v = make_view(gt, ref, sp, H, W, ch, cw);
    const int y = (int)blockIdx.y * kTH + (int)threadIdx.x / kTW, x = (int)blockIdx.x * kTW + (int)threadIdx.x % kTW;
    const bool inside = y < ch && x < cw;
    float r, g, b;
    chain_tile(sp, v, sums + (size_t)blockIdx.z * kOps, n_ops, sharpness_position(sp, n_ops, ch, cw), halo, y, x, inside, r, g, b);
    if (!inside) return;
    const int64_t cplane = (int64_t)ch * cw, o = (int64_t)blockIdx.z * 3 * cplane + (int64_t)y * cw + x, src = v.at(y, x);
    const float t[3] = {r, g, b};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        out_gt[o + q * cplane] = (float)v.gt[src + q * v.plane] / 255.f;
        out_ref[o + q * cplane] = (float)v.ref[src + q * v.plane] / 255.f;
        out_target[o + q * cplane] = t[q] / 255.f;
        if (out_u8) out_u8[o + q * cplane] = (uint8_t)t[q];
    }
}

}  // namespace aug
}  // namespace ct

extern "C" {

size_t ct_augment_workspace_bytes(int n) { return n < 1 ? 0 : (size_t)n * ct::aug::kOps * sizeof(unsigned long long); }

int ct_augment_u8(const uint8_t *gt, const uint8_t *ref, int n, int height, int width, const ct_augment_sample *samples,
                  const ct_augment_sample *samples_dev, int crop_h, int crop_w, float *out_gt, float *out_ref, float *out_target,
                  uint8_t *out_target_u8, void *ws, size_t ws_bytes, void *stream) {
    using namespace ct::aug;
    if (!gt || !ref || !samples || !samples_dev || !out_gt || !out_ref || !out_target) return CT_E_BADARG;
    if (n < 1 || n > 65535 || height < 1 || width < 1 || crop_h < 1 || crop_w < 1 || crop_h > height || crop_w > width) return CT_E_BADARG;
    int levels = 0;                                          // contrasts in the chain that has the most
    for (int i = 0; i < n; ++i) {
        const ct_augment_sample &sp = samples[i];
        if (sp.top < 0 || sp.left < 0 || sp.top > height - crop_h || sp.left > width - crop_w) return CT_E_BADARG;
        if ((sp.swap_hflip != 0 && sp.swap_hflip != 1) || (sp.vflip != 0 && sp.vflip != 1) || sp.n_ops < 0 || sp.n_ops > kOps) return CT_E_BADARG;
        int contrasts = 0, sharps = 0;
        for (int k = 0; k < sp.n_ops; ++k) {
            const int kind = sp.kind[k];
            const double p = sp.param[k];
            if (kind < 0 || kind > ct::kDistSharpness) return CT_E_BADARG;
            if (kind == ct::kDistHue && !(p >= -0.5 && p <= 0.5)) return CT_E_BADARG;          // torchvision raises ValueError
            if (kind != ct::kDistIdentity && kind != ct::kDistHue && !(p >= 0.0)) return CT_E_BADARG;
            contrasts += kind == ct::kDistContrast;
            sharps += kind == ct::kDistSharpness;
        }
        if (sharps > 1) return CT_E_BADARG;                  // one halo: the neighbours of neighbours are not recomputed
        if (contrasts > levels) levels = contrasts;
    }
    const dim3 grid((crop_w + kTW - 1) / kTW, (crop_h + kTH - 1) / kTH, n);
    if (grid.y > 65535u) return CT_E_BADARG;
    if (!ws || ws_bytes < ct_augment_workspace_bytes(n) || (reinterpret_cast<uintptr_t>(ws) & 7)) return CT_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(out_gt) | reinterpret_cast<uintptr_t>(out_ref) | reinterpret_cast<uintptr_t>(out_target)) % sizeof(float) ||
        (reinterpret_cast<uintptr_t>(samples_dev) & 7))
        return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *sums = reinterpret_cast<unsigned long long *>(ws);
    if (levels) {
        const int zr = ct::zero_async(ws, ct_augment_workspace_bytes(n), s);
        if (zr) return zr;
    }
    for (int level = 0; level < levels; ++level) {
        hipLaunchKernelGGL(augment_gray_sum_kernel, grid, dim3(ct::kBlock), 0, s, gt, ref, samples_dev, height, width, crop_h, crop_w, level, sums);
        CT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(augment_apply_kernel, grid, dim3(ct::kBlock), 0, s, gt, ref, samples_dev, height, width, crop_h, crop_w,
                       (const unsigned long long *)sums, out_gt, out_ref, out_target, out_target_u8);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
