// warp.hip -- perspective warp of interleaved uint8 frames on gfx950: the frame loop of the reference's dataset postprocessing
// (utils/postprocess.py:97 cv2.flip(left, 1); :127-129 the crop to bbox; :131-132 cv2.warpPerspective(img, H, (w, h)) with the
// defaults INTER_LINEAR and a constant 0 border; :134-136 the second crop).  Bytes in, bytes out, no float image.
//
// The rule is OpenCV's fixed-point bilinear path (modules/imgproc/src/imgwarp.cpp, warpPerspective + remapBilinear, up to 4.10;
// INTER_BITS = 5, INTER_TAB_SIZE = 32) restated -- "parity unpinned": cv2 is absent offline, requirements.txt pins no version, and
// OpenCV 4.11 replaced this path with a float one.  M is the destination -> source matrix (cv2's M after its own invert; the
// inversion is the caller's).  For destination pixel (row r, column c), with cv2's block grid
//     bh0 = min(16, crop_h), bw0 = min(1024 / bh0, crop_w), x0 = (c / bw0) * bw0, x1 = c - x0,
// in float64 with one rounding per operation (no fma: the Makefile's -ffp-contract=off), left to right:
//     X0 = M0*x0 + M1*r + M2;  Y0 = M3*x0 + M4*r + M5;  W0 = M6*x0 + M7*r + M8
//     W  = W0 + M6*x1;  W = (W != 0) ? 32 / W : 0
//     fX = max(-2^31, min(2^31 - 1, (X0 + M0*x1) * W));  fY likewise with M3;  X = (int)rint(fX) (ties to even), Y likewise
//     sx = sat16(X >> 5), sy = sat16(Y >> 5), a = X & 31, b = Y & 31
//     out = ((32-a)(32-b) p[sy][sx] + a(32-b) p[sy][sx+1] + (32-a)b p[sy+1][sx] + ab p[sy+1][sx+1] + 512) >> 10      per channel
// (cv2's 15-bit weight table holds a*b*32 exactly, so its (sum + 2^14) >> 15 is this).  p is the CROP of the -- possibly mirrored --
// raw frame: a tap outside the crop is 0 even where the raw frame has pixels.
//
// One workgroup per 64 x 16 tile of the output window (cv2's block when crop_h >= 16), four pixels of a row per thread.
//   staged taps (path = CT_WARP_STAGED; measured slower than the global taps at 1080p, so not the default): threads 0..3 map the tile's corners; where W keeps one sign over the tile the source of the tile lies
//     in the corners' bounding box.  Its rows (plus the second tap and a one-pixel margin) are copied into LDS with 16-byte loads,
//     as they lie in memory: the mirror is folded into the tap's address, not into the copy.  A tap that is inside the crop but not
//     in the box (none, unless the margin is ever too small) is read from memory, so the box is a cache, never a rule.
//   global taps (default, CT_WARP_AUTO / CT_WARP_GLOBAL): every tap from memory, through the caches.  Under CT_WARP_STAGED also
//     a tile whose box does not fit kWarpSrcBytes or in which W changes sign or vanishes, and every tile when the raw frames are
//     off the 16-byte grid (base or row pitch).
//   both give the same bytes: the arithmetic above is one function.
// Output: the tile's bytes go through LDS; of every row, the 16-byte runs that lie on the grid leave as vector stores whatever
// the alignment of out and of its row pitch (a second crop leaves any width), the up to 15 bytes at either end one by one.
// Taps are bounds-checked AFTER the integer conversion (the clamp makes the conversion itself defined for any matrix, NaN
// included), so no matrix can produce an address outside the crop.
#include "ct_common.h"

namespace ct {

constexpr int kWarpTileW = 64, kWarpTileH = 16;
constexpr int kWarpRowBytes = kWarpTileW * 3;    // a row of the tile's output image in LDS
constexpr int kWarpSrcBytes = 16384;             // LDS for the staged source box: 16 KB + 3 KB of output -> 8 workgroups per CU
typedef unsigned int wu32x4 __attribute__((ext_vector_type(4)));

struct WarpGeom {
    int src_h, src_w, crop_y, crop_w, crop_h, out_x, out_y, out_w, out_h, bw0;
    int col0, col_step;          // raw column of crop column sx: col0 + col_step * sx (the mirror: src_w - 1 - crop_x - sx)
};

// the fixed-point source coordinate of destination pixel (r, c); returns W before the inversion (the corners want its sign)
__device__ __forceinline__ double warp_xy(const double (&m)[9], int bw0, int c, int r, int &X, int &Y) {
    const int x0 = (c / bw0) * bw0;
    const double dx0 = (double)x0, dx1 = (double)(c - x0), dr = (double)r;
    const double X0 = m[0] * dx0 + m[1] * dr + m[2];
    const double Y0 = m[3] * dx0 + m[4] * dr + m[5];
    const double W0 = m[6] * dx0 + m[7] * dr + m[8];
    const double Wd = W0 + m[6] * dx1;
    const double W = (Wd != 0.0) ? 32.0 / Wd : 0.0;
    // fmin / fmax return the other operand for a NaN: the conversion below is in range for every input
    const double fX = fmax(-2147483648.0, fmin(2147483647.0, (X0 + m[0] * dx1) * W));
    const double fY = fmax(-2147483648.0, fmin(2147483647.0, (Y0 + m[3] * dx1) * W));
    X = (int)rint(fX);
    Y = (int)rint(fY);
    return Wd;
}

__device__ __forceinline__ int sat16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// the staged source box of a tile: rows ry0 .. ry0 + rows - 1 of the raw frame, bytes b0 .. b0 + span - 1 of each (rows == 0: none)
struct WarpBox {
    int ry0, rows, b0, span;
};

// one tap of the crop: 0 outside it, else the three bytes at (sy, sx) -- from the staged box when they are there
template <bool LDS>
__device__ __forceinline__ void warp_tap(const uint8_t *__restrict__ frame, const uint8_t *__restrict__ staged, const WarpGeom &g, const WarpBox &box,
                                         int sy, int sx, int (&p)[3]) {
    p[0] = p[1] = p[2] = 0;
    if ((unsigned)sx >= (unsigned)g.crop_w || (unsigned)sy >= (unsigned)g.crop_h) return;
    const int rr = g.crop_y + sy;
    const int rc = g.col0 + g.col_step * sx;
    if constexpr (LDS) {
        const int row = rr - box.ry0, off = 3 * rc - box.b0;
        if ((unsigned)row < (unsigned)box.rows && off >= 0 && off + 3 <= box.span) {
            const uint8_t *q = staged + row * box.span + off;
            p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
            return;
        }
    }
    const uint8_t *q = frame + ((int64_t)rr * g.src_w + rc) * 3;
    p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void warp_perspective_kernel(const uint8_t *__restrict__ raw, int n, WarpGeom g, const double *__restrict__ maps,
                                                                  int shared, uint8_t *__restrict__ out) {
    __shared__ wu32x4 src_lds[LDS ? kWarpSrcBytes / 16 : 1];
    __shared__ wu32x4 out_lds[kWarpTileH * kWarpRowBytes / 16 + 1];                         // + 16 bytes of slack for the funnel's fifth dword
    __shared__ int corner[4][3];
    const int t = threadIdx.x;
    const int tile_c = blockIdx.x * kWarpTileW, tile_r = blockIdx.y * kWarpTileH;          // within the window
    const int tile_w = min(kWarpTileW, g.out_w - tile_c), tile_h = min(kWarpTileH, g.out_h - tile_r);
    const int64_t src_pitch = (int64_t)g.src_w * 3, out_pitch = (int64_t)g.out_w * 3;
    const int prow = t >> 4, pcol = (t & 15) * 4;                                            // this thread's four pixels of the tile
    for (int f = blockIdx.z; f < n; f += gridDim.z) {
        const uint8_t *frame = raw + (int64_t)f * g.src_h * src_pitch;
        double m[9];
        const double *mp = maps + (shared ? 0 : (int64_t)f * 9);
#pragma unroll
        for (int k = 0; k < 9; ++k) m[k] = mp[k];
        WarpBox box = {0, 0, 0, 0};
        if constexpr (LDS) {
            if (t < 4) {
                int X, Y;
                const double Wd = warp_xy(m, g.bw0, g.out_x + tile_c + ((t & 1) ? tile_w - 1 : 0), g.out_y + tile_r + ((t & 2) ? tile_h - 1 : 0), X, Y);
                corner[t][0] = X >> 5;
                corner[t][1] = Y >> 5;
                corner[t][2] = (Wd > 0.0 && Wd < __builtin_inf()) ? 1 : ((Wd < 0.0 && Wd > -__builtin_inf()) ? -1 : 0);
            }
            __syncthreads();
            int sx_lo = corner[0][0], sx_hi = sx_lo, sy_lo = corner[0][1], sy_hi = sy_lo;
            bool ok = corner[0][2] != 0;
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                sx_lo = min(sx_lo, corner[k][0]); sx_hi = max(sx_hi, corner[k][0]);
                sy_lo = min(sy_lo, corner[k][1]); sy_hi = max(sy_hi, corner[k][1]);
                ok = ok && corner[k][2] == corner[0][2];
            }
            // the second tap and one pixel of margin (the corners bound the tile up to the 1/32 rounding), cut to the crop
            sx_lo = max(sx_lo - 1, 0); sx_hi = min(sx_hi + 2, g.crop_w - 1);
            sy_lo = max(sy_lo - 1, 0); sy_hi = min(sy_hi + 2, g.crop_h - 1);
            ok = ok && sx_lo <= sx_hi && sy_lo <= sy_hi;
            if (ok) {
                const int rc_a = g.col0 + g.col_step * sx_lo, rc_b = g.col0 + g.col_step * sx_hi;
                const int rc_lo = min(rc_a, rc_b), rc_hi = max(rc_a, rc_b);
                const int b0 = (3 * rc_lo) & ~15, b1 = (3 * rc_hi + 3 + 15) & ~15;      // b1 <= the row pitch: it is a multiple of 16 here
                const int rows = sy_hi - sy_lo + 1;
                if ((int64_t)rows * (b1 - b0) <= kWarpSrcBytes) box = {g.crop_y + sy_lo, rows, b0, b1 - b0};
            }
            const int per_row = box.span / 16, total = box.rows * per_row;
            for (int i = t; i < total; i += kBlock) {
                const int row = i / per_row, cc = i - row * per_row;
                src_lds[i] = *reinterpret_cast<const wu32x4 *>(frame + (int64_t)(box.ry0 + row) * src_pitch + box.b0 + 16 * cc);
            }
            __syncthreads();
        }
        const uint8_t *staged = reinterpret_cast<const uint8_t *>(src_lds);
        unsigned int px[4] = {0u, 0u, 0u, 0u};                                               // r | g << 8 | b << 16 of the four pixels
        if (prow < tile_h) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (pcol + j >= tile_w) break;
                int X, Y;
                (void)warp_xy(m, g.bw0, g.out_x + tile_c + pcol + j, g.out_y + tile_r + prow, X, Y);
                const int sx = sat16(X >> 5), sy = sat16(Y >> 5), a = X & 31, b = Y & 31;
                int p00[3], p01[3], p10[3], p11[3];
                warp_tap<LDS>(frame, staged, g, box, sy, sx, p00);
                warp_tap<LDS>(frame, staged, g, box, sy, sx + 1, p01);
                warp_tap<LDS>(frame, staged, g, box, sy + 1, sx, p10);
                warp_tap<LDS>(frame, staged, g, box, sy + 1, sx + 1, p11);
                const int w00 = (32 - a) * (32 - b), w01 = a * (32 - b), w10 = (32 - a) * b, w11 = a * b;
                unsigned int v = 0;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch)
                    v |= (unsigned int)((w00 * p00[ch] + w01 * p01[ch] + w10 * p10[ch] + w11 * p11[ch] + 512) >> 10) << (8 * ch);
                px[j] = v;
            }
        }
        uint8_t *o = out + ((int64_t)f * g.out_h + tile_r) * out_pitch + (int64_t)tile_c * 3;    // the tile's first byte
        // 12 bytes of a thread -> three dwords of the tile's [16][192 B] image
        unsigned int *img = reinterpret_cast<unsigned int *>(out_lds);
        img[prow * (kWarpRowBytes / 4) + (t & 15) * 3] = px[0] | px[1] << 24;
        img[prow * (kWarpRowBytes / 4) + (t & 15) * 3 + 1] = px[1] >> 8 | px[2] << 16;
        img[prow * (kWarpRowBytes / 4) + (t & 15) * 3 + 2] = px[2] >> 16 | px[3] << 8;
        __syncthreads();
        // A row of the tile is tile_w * 3 contiguous bytes at ANY address.  Its 16-byte runs that lie on the grid leave as vector
        // stores, each put together from five dwords of the image by the row's phase against the grid (a byte funnel; phase 0 when
        // out and its pitch are on the grid); the up to 15 bytes before and after them leave one by one.  13 lanes per row: at
        // most 12 runs, and one lane for the edges.
        const int row = t / 13, k = t - row * 13;
        if (row < tile_h) {
            uint8_t *dst = o + row * out_pitch;
            const int len = tile_w * 3;
            const int head = min(len, (int)((16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15));
            const int runs = (len - head) / 16;
            if (k < runs) {
                const int off = row * kWarpRowBytes + head + 16 * k;
                const int sh = 8 * (off & 3);
                unsigned int d[5];
#pragma unroll
                for (int j = 0; j < 5; ++j) d[j] = img[(off >> 2) + j];                     // d[4]: the slack dword after the last row
                wu32x4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (unsigned int)((((uint64_t)d[j + 1] << 32) | d[j]) >> sh);
                *reinterpret_cast<wu32x4 *>(dst + head + 16 * k) = v;
            } else if (k == 12) {
                const uint8_t *src = reinterpret_cast<const uint8_t *>(out_lds) + row * kWarpRowBytes;
                for (int i = 0; i < head; ++i) dst[i] = src[i];
                for (int i = head + 16 * runs; i < len; ++i) dst[i] = src[i];
            }
        }
        __syncthreads();                                     // corner / src_lds / out_lds are written again for the next frame
    }
}

}  // namespace ct

extern "C" {

int ct_warp_perspective_u8(const uint8_t *raw, int n, int src_h, int src_w, int flip_x, int crop_x, int crop_y, int crop_w, int crop_h,
                           const double *maps, int shared, int out_x, int out_y, int out_w, int out_h, uint8_t *out, int path, void *stream) {
    if (!raw || !maps || !out || n < 1 || src_h < 1 || src_w < 1 || crop_w < 1 || crop_h < 1 || out_w < 1 || out_h < 1) return CT_E_BADARG;
    if (crop_w > 32767 || crop_h > 32767 || (path != CT_WARP_AUTO && path != CT_WARP_STAGED && path != CT_WARP_GLOBAL)) return CT_E_BADARG;
    if (crop_x < 0 || crop_y < 0 || (int64_t)crop_x + crop_w > src_w || (int64_t)crop_y + crop_h > src_h) return CT_E_BADARG;
    if (out_x < 0 || out_y < 0 || (int64_t)out_x + out_w > crop_w || (int64_t)out_y + out_h > crop_h) return CT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(maps) % sizeof(double)) return CT_E_ALIGN;
    const int bh0 = crop_h < 16 ? crop_h : 16;
    const int bw0 = 1024 / bh0 < crop_w ? 1024 / bh0 : crop_w;
    const ct::WarpGeom g = {src_h, src_w, crop_y, crop_w, crop_h, out_x, out_y, out_w, out_h, bw0, flip_x ? src_w - 1 - crop_x : crop_x, flip_x ? -1 : 1};
    // 16-byte loads of source rows: the base and the row pitch (hence every frame) on the grid
    // CT_WARP_AUTO takes the global taps: at 1080p they measured 183 us against 230 us for 16 frames
    const bool staged = path == CT_WARP_STAGED &&reinterpret_cast<uintptr_t>(raw) % 16 == 0 && ((int64_t)src_w * 3) % 16 == 0;
    const dim3 grid((out_w + ct::kWarpTileW - 1) / ct::kWarpTileW, (out_h + ct::kWarpTileH - 1) / ct::kWarpTileH, n < 65535 ? n : 65535);
    hipStream_t s = (hipStream_t)stream;
    if (staged)
        hipLaunchKernelGGL(ct::warp_perspective_kernel<true>, grid, dim3(ct::kBlock), 0, s, raw, n, g, maps, shared != 0, out);
    else
        hipLaunchKernelGGL(ct::warp_perspective_kernel<false>, grid, dim3(ct::kBlock), 0, s, raw, n, g, maps, shared != 0, out);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
