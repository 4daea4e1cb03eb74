// yuv.hip -- 8-bit Y'CbCr 4:2:0 (packed I420 frames: Y plane, Cb plane, Cr plane) <-> interleaved RGB bytes on gfx950: what a
// video decoder hands over and what an encoder takes, 1.5 bytes per pixel on the host link instead of 3.
//
// The rule is an exact one (ct_yuv.h): every output byte is the correctly rounded value, ties to even, of a rational expression
// of the input bytes, evaluated in integers.  swscale / cv2 parity is unpinned (neither is present offline); the int64 numpy
// restatement in tests/yuv_common.py is the oracle and the bytes are equal to it.
//
// Two streaming kernels, no LDS, every input byte read once plus the chroma halo (decode: the chroma rows above and below and one
// column either side; encode with left siting: one pixel column to the left).  A lane owns TWO luma rows x 16 columns = one
// chroma row x 8 columns, so consecutive lanes of a wave cover 1 KiB of each luma row:
//   decode  2 x 16 B of Y, 3 rows x (8 B + 2 halo bytes) of Cb and of Cr  ->  2 x 48 B of RGB (3 x 16-byte stores per row)
//   encode  2 x 48 B of RGB (3 x 16-byte loads per row)                   ->  2 x 16 B of Y, 8 B of Cb, 8 B of Cr
// The planes of a frame start at H W and H W + ch cw, frames at multiples of the caller's stride, rows at multiples of W: none of
// these need be on the 16-byte grid.  Each run of a lane therefore decides by its own address (and by being a whole run) whether
// it moves as one vector or byte by byte; with W % 16 == 0 and aligned bases everything is a vector.
// Offsets inside a frame are 32-bit (H W 3 < 2^31 is required), frame bases 64-bit.
#include "ct_yuv.h"

namespace ct {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

#define CT_BYTE(w, k) (((w)[(k) >> 2] >> (8 * ((k) & 3))) & 255u)

// NW words = 4 NW bytes from p[0 .. valid): one vector when the run is whole and on its own grid, else byte by byte, the last
// valid byte repeated beyond the end (the edge clamp of a chroma row; luma bytes beyond the end are never used)
template <int NW>
__host__ __device__ __forceinline__ void load_run(const uint8_t *__restrict__ p, int valid, unsigned int (&w)[NW]) {
    typedef unsigned int vec_t __attribute__((ext_vector_type(NW)));
    if (valid >= 4 * NW && (reinterpret_cast<uintptr_t>(p) & (4 * NW - 1)) == 0) {
        const vec_t v = *reinterpret_cast<const vec_t *>(p);
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = v[i];
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = 0u;
#pragma unroll
        for (int k = 0; k < 4 * NW; ++k) w[k >> 2] |= (unsigned int)p[k < valid ? k : valid - 1] << (8 * (k & 3));
    }
}

// the first `valid` of 4 NW bytes to p
template <int NW>
__host__ __device__ __forceinline__ void store_run(uint8_t *__restrict__ p, int valid, const unsigned int (&w)[NW]) {
    typedef unsigned int vec_t __attribute__((ext_vector_type(NW)));
    if (valid >= 4 * NW && (reinterpret_cast<uintptr_t>(p) & (4 * NW - 1)) == 0) {
        vec_t v;
#pragma unroll
        for (int i = 0; i < NW; ++i) v[i] = w[i];
        *reinterpret_cast<vec_t *>(p) = v;
    } else {
#pragma unroll
        for (int k = 0; k < 4 * NW; ++k)
            if (k < valid) p[k] = (uint8_t)CT_BYTE(w, k);
    }
}

// ten chroma samples of one plane row around the lane's eight: columns cx0 - 1 .. cx0 + 8, clamped to the row
__host__ __device__ __forceinline__ void load_chroma_row(const uint8_t *__restrict__ row, int cx0, int cw, int (&c)[10]) {
    unsigned int w[2];
    load_run<2>(row + cx0, cw - cx0, w);
    c[0] = row[cx0 > 0 ? cx0 - 1 : 0];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k + 1] = (int)CT_BYTE(w, k);
    c[9] = row[cx0 + 8 < cw ? cx0 + 8 : cw - 1];
}

// one chroma plane at the lane's 2 x 16 luma positions, in sixteenths: the horizontal pass on the three plane rows (quarters),
// then 3 : 1 between the lane's own chroma row and the one above (upper luma row) / below (lower luma row)
__host__ __device__ __forceinline__ void chroma16(const uint8_t *__restrict__ plane, int i, int ch, int cx0, int cw, const YuvRule &p,
                                         int (&c16)[2][16]) {
    int h[3][16];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        int ri = i + r - 1;
        ri = ri < 0 ? 0 : ri > ch - 1 ? ch - 1 : ri;
        int c[10];
        load_chroma_row(plane + ri * cw, cx0, cw, c);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            h[r][2 * j] = p.we0 * c[j] + p.we1 * c[j + 1];
            h[r][2 * j + 1] = p.wo1 * c[j + 1] + p.wo2 * c[j + 2];
        }
    }
#pragma unroll
    for (int x = 0; x < 16; ++x) {
        c16[0][x] = 3 * h[1][x] + h[0][x];
        c16[1][x] = 3 * h[1][x] + h[2][x];
    }
}

// one lane's work: item = (frame * ch + chroma row) * ng + column group, ng = ceil(W / 16)
__host__ __device__ __forceinline__ void yuv420_to_rgb_item(const uint8_t *__restrict__ yuv, long long stride, int item, int H, int W,
                                                            const YuvRule &p, uint8_t *__restrict__ out) {
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1, ng = (W + 15) >> 4;
    {
        const int g = item % ng, t = item / ng, i = t % ch, f = t / ch;
        const uint8_t *frame = yuv + (long long)f * stride;
        const int x0 = 16 * g, cx0 = 8 * g, nx = W - x0;               // nx >= 1 columns of this run exist
        int cb[2][16], cr[2][16];
        chroma16(frame + H * W, i, ch, cx0, cw, p, cb);
        chroma16(frame + H * W + ch * cw, i, ch, cx0, cw, p, cr);
        uint8_t *o = out + (long long)f * H * W * 3;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * i + r;
            if (y >= H) break;
            unsigned int yw[4];
            load_run<4>(frame + y * W + x0, nx, yw);
            unsigned int ow[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) ow[k] = 0u;
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const long long yd = (int)CT_BYTE(yw, x) - p.yoff, cbd = cb[r][x] - 2048, crd = cr[r][x] - 2048;
                const unsigned int R = yuv_unit_to_u8(p.ay_rb * yd + p.a_r * crd, p.den_rb, p.inv_rb);
                const unsigned int G = yuv_unit_to_u8(p.ay_g * yd + p.g_b * cbd + p.g_r * crd, p.den_g, p.inv_g);
                const unsigned int B = yuv_unit_to_u8(p.ay_rb * yd + p.a_b * cbd, p.den_rb, p.inv_rb);
                ow[(3 * x) >> 2] |= R << (8 * ((3 * x) & 3));
                ow[(3 * x + 1) >> 2] |= G << (8 * ((3 * x + 1) & 3));
                ow[(3 * x + 2) >> 2] |= B << (8 * ((3 * x + 2) & 3));
            }
            uint8_t *orow = o + (y * W + x0) * 3;
            if (nx >= 16 && (reinterpret_cast<uintptr_t>(orow) & 15) == 0) {
                u32x4 *dst = reinterpret_cast<u32x4 *>(orow);
#pragma unroll
                for (int v = 0; v < 3; ++v) {
                    u32x4 q;
                    q.x = ow[4 * v]; q.y = ow[4 * v + 1]; q.z = ow[4 * v + 2]; q.w = ow[4 * v + 3];
                    dst[v] = q;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 48; ++k)
                    if (k < 3 * nx) orow[k] = (uint8_t)CT_BYTE(ow, k);
            }
        }
    }
}

// items = n * ch * ng lanes of work, grid-stride
__global__ __launch_bounds__(kBlock) void yuv420_to_rgb_kernel(const uint8_t *__restrict__ yuv, long long stride, int items, int H,
                                                               int W, YuvRule p, uint8_t *__restrict__ out) {
    for (int item = blockIdx.x * kBlock + threadIdx.x; item < items; item += gridDim.x * kBlock)
        yuv420_to_rgb_item(yuv, stride, item, H, W, p, out);
}

// sixteen RGB pixels of one row from column x0 (the last column repeated beyond the row's end) as 12 words
__host__ __device__ __forceinline__ void load_rgb_run(const uint8_t *__restrict__ row, int x0, int W, unsigned int (&w)[12]) {
    const uint8_t *p = row + 3 * x0;
    if (x0 + 16 <= W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
        const u32x4 *src = reinterpret_cast<const u32x4 *>(p);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            const u32x4 q = __builtin_nontemporal_load(src + v);
            w[4 * v] = q.x; w[4 * v + 1] = q.y; w[4 * v + 2] = q.z; w[4 * v + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 12; ++k) w[k] = 0u;
#pragma unroll
        for (int k = 0; k < 48; ++k) {
            const int x = x0 + k / 3 < W ? x0 + k / 3 : W - 1;
            w[k >> 2] |= (unsigned int)row[3 * x + k % 3] << (8 * (k & 3));
        }
    }
}

__host__ __device__ __forceinline__ void rgb_to_yuv420_item(const uint8_t *__restrict__ rgb, int item, int H, int W, const YuvRule &p,
                                                            uint8_t *__restrict__ yuv, long long stride) {
    const int ch = (H + 1) >> 1, cw = (W + 1) >> 1, ng = (W + 15) >> 4;
    {
        const int g = item % ng, t = item / ng, i = t % ch, f = t / ch;
        const uint8_t *in = rgb + (long long)f * H * W * 3;
        uint8_t *frame = yuv + (long long)f * stride;
        const int x0 = 16 * g, cx0 = 8 * g, nx = W - x0;
        unsigned int px[2][12];
        int halo[2][3];                                                  // column x0 - 1 (clamped): left siting only
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * i + r < H ? 2 * i + r : H - 1;             // an odd height repeats its last row under the chroma
            const uint8_t *row = in + y * W * 3;
            load_rgb_run(row, x0, W, px[r]);
            if (p.left) {
                const uint8_t *hp = row + 3 * (x0 > 0 ? x0 - 1 : 0);
                halo[r][0] = hp[0]; halo[r][1] = hp[1]; halo[r][2] = hp[2];
            } else {
                halo[r][0] = halo[r][1] = halo[r][2] = 0;
            }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int y = 2 * i + r;
            if (y >= H) break;
            unsigned int yw[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int x = 0; x < 16; ++x) {
                const int R = (int)CT_BYTE(px[r], 3 * x), G = (int)CT_BYTE(px[r], 3 * x + 1), B = (int)CT_BYTE(px[r], 3 * x + 2);
                const int q = p.yoff + rint_div<int>(p.ys * (p.kr * R + p.kg * G + p.kb * B), p.den_y, p.inv_y);
                yw[x >> 2] |= (unsigned int)clampi(q, p.ymin, p.ymax) << (8 * (x & 3));
            }
            store_run<4>(frame + y * W + x0, nx, yw);
        }
        unsigned int cbw[2] = {0u, 0u}, crw[2] = {0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                int a = 0;
#pragma unroll
                for (int r = 0; r < 2; ++r) {
                    const int mid = (int)CT_BYTE(px[r], 6 * j + c), nxt = (int)CT_BYTE(px[r], 6 * j + 3 + c);
                    const int prv = j == 0 ? halo[r][c] : (int)CT_BYTE(px[r], 6 * j - 3 + c);
                    a += p.left ? prv + 2 * mid + nxt : mid + nxt;
                }
                s[c] = a;
            }
            const int L = p.kr * s[0] + p.kg * s[1] + p.kb * s[2];
            const int qb = 128 + rint_div<long long>((long long)p.cs * (p.d * s[2] - L), p.den_cb, p.inv_cb);
            const int qr = 128 + rint_div<long long>((long long)p.cs * (p.d * s[0] - L), p.den_cr, p.inv_cr);
            cbw[j >> 2] |= (unsigned int)clampi(qb, p.cmin, p.cmax) << (8 * (j & 3));
            crw[j >> 2] |= (unsigned int)clampi(qr, p.cmin, p.cmax) << (8 * (j & 3));
        }
        const int nc = cw - cx0;
        store_run<2>(frame + H * W + i * cw + cx0, nc, cbw);
        store_run<2>(frame + H * W + ch * cw + i * cw + cx0, nc, crw);
    }
}

__global__ __launch_bounds__(kBlock) void rgb_to_yuv420_kernel(const uint8_t *__restrict__ rgb, int items, int H, int W, YuvRule p,
                                                               uint8_t *__restrict__ yuv, long long stride) {
    for (int item = blockIdx.x * kBlock + threadIdx.x; item < items; item += gridDim.x * kBlock)
        rgb_to_yuv420_item(rgb, item, H, W, p, yuv, stride);
}

// shared argument check: the rule, the lane count and the packed frame size
static int yuv_geometry(int n, int height, int width, long long stride, int matrix, int range, int siting, YuvRule &p, int &items) {
    if (n < 1 || height < 1 || width < 1 || !yuv_rule(matrix, range, siting, p)) return CT_E_BADARG;
    const long long hw = (long long)height * width;
    if (hw * 3 >= (1ll << 31)) return CT_E_BADARG;                       // 32-bit offsets inside a frame
    const long long ch = (height + 1) / 2, cw = (width + 1) / 2;
    if (stride < hw + 2 * ch * cw) return CT_E_BADARG;
    const long long it = (long long)n * ch * ((width + 15) / 16);
    if (it >= (1ll << 31) - 2 * (long long)kTargetBlocks * kBlock) return CT_E_BADARG;        // the grid-stride counter is an int
    items = (int)it;
    return CT_OK;
}

static unsigned yuv_blocks(int items) {
    const int b = (items + kBlock - 1) / kBlock, cap = target_blocks() < 2 * kTargetBlocks ? target_blocks() : 2 * kTargetBlocks;
    return (unsigned)(b > cap ? cap : b);
}

}  // namespace ct

extern "C" {

int ct_yuv420_to_rgb_u8(const uint8_t *yuv, int64_t frame_stride, int n, int height, int width, int matrix, int range, int siting,
                        uint8_t *out_rgb, void *stream) {
    ct::YuvRule p;
    int items = 0;
    if (!yuv || !out_rgb) return CT_E_BADARG;
    const int rc = ct::yuv_geometry(n, height, width, frame_stride, matrix, range, siting, p, items);
    if (rc != CT_OK) return rc;
    hipLaunchKernelGGL(ct::yuv420_to_rgb_kernel, dim3(ct::yuv_blocks(items)), dim3(ct::kBlock), 0, (hipStream_t)stream, yuv,
                       (long long)frame_stride, items, height, width, p, out_rgb);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_rgb_to_yuv420_u8(const uint8_t *rgb, int n, int height, int width, int matrix, int range, int siting, uint8_t *out_yuv,
                        int64_t frame_stride, void *stream) {
    ct::YuvRule p;
    int items = 0;
    if (!rgb || !out_yuv) return CT_E_BADARG;
    const int rc = ct::yuv_geometry(n, height, width, frame_stride, matrix, range, siting, p, items);
    if (rc != CT_OK) return rc;
    hipLaunchKernelGGL(ct::rgb_to_yuv420_kernel, dim3(ct::yuv_blocks(items)), dim3(ct::kBlock), 0, (hipStream_t)stream, rgb, items,
                       height, width, p, out_yuv, (long long)frame_stride);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
