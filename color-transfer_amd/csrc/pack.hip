// pack.hip -- corrected float32 frames -> interleaved uint8 frames on gfx950: the last step of `utils.cli predict`, what the
// reference does on the host with skimage.util.img_as_ubyte(x.clip(0, 1)) before it writes PNGs (utils/postprocess.py:138-144).
//
// The rule, to the bit:  q = rint(clamp(x, 0, 1) * 255)
//   - ONE float32 multiplication by 255.0f (the Makefile's -ffp-contract=off keeps it out of an fma; no reciprocal),
//   - round to nearest, ties to even (v_rndne_f32),
//   - NaN, -inf and negatives -> 0;  +inf and values above 1 -> 255.
// skimage is third-party and absent offline: this restates its float32 branch (np.multiply(image, 255, dtype=float32), np.rint,
// np.clip) -- "parity unpinned"; the numpy restatement in tests/test_predict_gpu.py is the oracle.
//
// A pure streaming kernel: no LDS, no reuse, 4 bytes read and 1 byte written per element (1080p: 24 883 200 B in, 6 220 800 B
// out).  Each lane turns 16-byte non-temporal loads (the input is never read again) into 16-byte stores:
//   HWC  [n][H][W][3] -> same order: a flat run of elements; four consecutive dwordx4 loads feed one dwordx4 of 16 bytes;
//   CHW  [n][3][H][W] -> [n][H][W][3]: 16 pixels per lane, 4 dwordx4 loads from each of the three planes feed 3 x 16 B.
// What does not sit on the 16-byte grid (a total that is no multiple of 16, H*W % 4 != 0 in CHW, an odd base) goes through the
// element-wise tail / fallback of the same rule.
#include "ct_common.h"
#include "ct_quant.h"     // quant_u8, pack4: the rule itself

namespace ct {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// in / out 16-byte aligned: n_chunks runs of 16 elements, then (block 0) the n_tail < 16 elements after them
__global__ __launch_bounds__(kBlock) void pack_hwc_kernel(const float *__restrict__ in, int64_t n_chunks, int n_tail, uint8_t *__restrict__ out) {
    const f32x4 *src = reinterpret_cast<const f32x4 *>(in);
    u32x4 *dst = reinterpret_cast<u32x4 *>(out);
    for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * kBlock) {
        const f32x4 a = __builtin_nontemporal_load(src + 4 * c), b = __builtin_nontemporal_load(src + 4 * c + 1);
        const f32x4 d = __builtin_nontemporal_load(src + 4 * c + 2), e = __builtin_nontemporal_load(src + 4 * c + 3);
        u32x4 o;
        o.x = pack4(quant_u8(a.x), quant_u8(a.y), quant_u8(a.z), quant_u8(a.w));
        o.y = pack4(quant_u8(b.x), quant_u8(b.y), quant_u8(b.z), quant_u8(b.w));
        o.z = pack4(quant_u8(d.x), quant_u8(d.y), quant_u8(d.z), quant_u8(d.w));
        o.w = pack4(quant_u8(e.x), quant_u8(e.y), quant_u8(e.z), quant_u8(e.w));
        dst[c] = o;
    }
    if (blockIdx.x == 0 && (int)threadIdx.x < n_tail) {
        const int64_t i = n_chunks * 16 + threadIdx.x;
        out[i] = (uint8_t)quant_u8(in[i]);
    }
}

// any element-aligned base: one element per lane and step (HWC fallback)
__global__ __launch_bounds__(kBlock) void pack_hwc_scalar_kernel(const float *__restrict__ in, int64_t n_elems, uint8_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_elems; i += (int64_t)gridDim.x * kBlock)
        out[i] = (uint8_t)quant_u8(in[i]);
}

// blockIdx.y strides over the images.  An image whose three planes and whose output all start on 16 bytes takes the vector body
// for its whole runs of 16 pixels and the per-pixel path for the rest; any other image takes the per-pixel path throughout.
__global__ __launch_bounds__(kBlock) void pack_chw_kernel(const float *__restrict__ in, int n, int64_t plane, uint8_t *__restrict__ out) {
    for (int b = blockIdx.y; b < n; b += gridDim.y) {
        const float *p0 = in + (int64_t)b * 3 * plane, *p1 = p0 + plane, *p2 = p1 + plane;
        uint8_t *o = out + (int64_t)b * 3 * plane;
        const bool vec = ((reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2) |
                           reinterpret_cast<uintptr_t>(o)) & 15) == 0;                    // uniform over the workgroup
        const int64_t n_chunks = vec ? plane / 16 : 0;
        for (int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x; c < n_chunks; c += (int64_t)gridDim.x * kBlock) {
            unsigned int q[3][16];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const f32x4 *src = reinterpret_cast<const f32x4 *>((ch == 0 ? p0 : ch == 1 ? p1 : p2) + 16 * c);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const f32x4 a = __builtin_nontemporal_load(src + j);
                    q[ch][4 * j] = quant_u8(a.x); q[ch][4 * j + 1] = quant_u8(a.y);
                    q[ch][4 * j + 2] = quant_u8(a.z); q[ch][4 * j + 3] = quant_u8(a.w);
                }
            }
            u32x4 *dst = reinterpret_cast<u32x4 *>(o + 48 * c);
#pragma unroll
            for (int v = 0; v < 3; ++v) {                   // byte k of the 48 = channel k % 3 of pixel k / 3
                unsigned int w[4];
#pragma unroll
                for (int d = 0; d < 4; ++d) {
                    const int k = 16 * v + 4 * d;
                    w[d] = pack4(q[k % 3][k / 3], q[(k + 1) % 3][(k + 1) / 3], q[(k + 2) % 3][(k + 2) / 3], q[(k + 3) % 3][(k + 3) / 3]);
                }
                u32x4 t;
                t.x = w[0]; t.y = w[1]; t.z = w[2]; t.w = w[3];
                dst[v] = t;
            }
        }
        for (int64_t p = n_chunks * 16 + (int64_t)blockIdx.x * kBlock + threadIdx.x; p < plane; p += (int64_t)gridDim.x * kBlock) {
            o[3 * p] = (uint8_t)quant_u8(p0[p]);
            o[3 * p + 1] = (uint8_t)quant_u8(p1[p]);
            o[3 * p + 2] = (uint8_t)quant_u8(p2[p]);
        }
    }
}

}  // namespace ct

extern "C" {

int ct_pack_u8_f32(const float *in, int layout, int n, int height, int width, uint8_t *out_hwc, void *stream) {
    if (!in || !out_hwc || n < 1 || height < 1 || width < 1 || (layout != CT_PACK_HWC && layout != CT_PACK_CHW)) return CT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(in) % sizeof(float)) return CT_E_ALIGN;
    hipStream_t s = (hipStream_t)stream;
    const int64_t plane = (int64_t)height * width;
    if (layout == CT_PACK_HWC) {
        const int64_t n_elems = plane * 3 * n;
        const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out_hwc)) & 15) == 0;
        const int64_t n_chunks = vec ? n_elems / 16 : n_elems;          // lane-steps of work: runs of 16 elements, or elements
        int64_t blocks = (n_chunks + ct::kBlock - 1) / ct::kBlock;        // one batch is one flat run: the whole target grid, grid-stride the rest
        if (blocks > ct::target_blocks()) blocks = ct::target_blocks();
        if (blocks < 1) blocks = 1;                                      // fewer than 16 elements: the tail alone
        if (vec)
            hipLaunchKernelGGL(ct::pack_hwc_kernel, dim3((unsigned)blocks), dim3(ct::kBlock), 0, s, in, n_chunks, (int)(n_elems % 16), out_hwc);
        else
            hipLaunchKernelGGL(ct::pack_hwc_scalar_kernel, dim3((unsigned)blocks), dim3(ct::kBlock), 0, s, in, n_elems, out_hwc);
    } else {
        const int gy = n < 65535 ? n : 65535;
        // sized by the runs of 16 pixels; the per-pixel path of an off-grid image strides over the same grid
        hipLaunchKernelGGL(ct::pack_chw_kernel, dim3(ct::blocks_per_image((plane + 15) / 16, gy), gy), dim3(ct::kBlock), 0, s, in, n, plane, out_hwc);
    }
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
