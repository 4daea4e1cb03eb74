// regrain.hip -- the "regrain" post-process of automated_color_grading (reference methods/iterative.py:62-138) on gfx950.
//
//   _regrain  (iterative.py:62-78)   multigrid recursion: both images are halved with skimage.transform.resize down to
//                                    ~20 pixels, the coarse solution is resized back up and relaxed on every level
//   _solve    (iterative.py:81-117)  nbit Jacobi sweeps of a 5-point gradient-preserving relaxation (psi / phi weights
//                                    from the gradients of the ORIGINAL image)
//   skimage.transform.resize (third party, scikit-image 0.18.3 _warps.py:resize/warp + scipy.ndimage.gaussian_filter):
//       down: Gaussian anti-aliasing, sigma = (factor - 1) / 2 per axis, radius int(4 sigma + 0.5), 'mirror' boundary,
//             axis 0 then axis 1; then bilinear sampling at factor * (i + 0.5) - 0.5 with 'reflect' boundary
//       up:   the bilinear sampling alone
//
// All arithmetic is float64 (the reference's `img_arr_col` is the float64 IDT output; a float32 target is promoted here
// where the reference resizes it in float32 -- a 1e-7-level difference, see tests).  HWC layout, one thread per pixel;
// the relaxation runs k = 8 sweeps per launch on LDS-resident tiles with a recomputed halo (rg_sweepk_kernel: 31 sweep launches
// for a 1080p frame instead of 244, bitwise the same result); the resizes are plain streaming kernels.
//
// Every kernel has a frame axis: blockIdx.y is the frame, every buffer holds its frames back to back (frame stride = the pixel
// count of the level), so a group of k frames of one size takes the launches of one frame.  ct_regrain_f64 is the batch-1 call.
//
// ct_regrain_u8 / ct_acg_u8 (uint8 target in; float64, float32 and / or bytes out, + PSNR): level 0's img_in is the target itself,
// so the kernels that read it there (weights, the level-0 sweeps, the first down-resize) are instantiated for uint8_t: a byte is
// looked up in the 256-entry float64 table of the image it stands for (ct_bytes.h: fill_u8_table, ld_u8) and then takes the float64
// statements as they stand -- bitwise the float64 entry on that image.  The LAST level-0 launch (<., true>) writes the requested
// outputs and the squared-error partials of the metric (ct_u8_frames.h: U8Sinks, through rg_emit) instead of the float64 iterate.
#include "ct_bytes.h"
#include "ct_common.h"
#include "ct_metrics.h"
#include "ct_quant.h"
#include "ct_u8_frames.h"

namespace ct {

constexpr int kRgMaxLevels = 8;

// element e (over the whole batch) of the result, to the sinks of the LAST level-0 launch
__device__ __forceinline__ void rg_emit(const U8Sinks &sk, size_t e, double y, double &acc) {
    if (sk.f64) sk.f64[e] = y;
    const float v = (float)y;
    if (sk.f32) sk.f32[e] = v;
    if (sk.u8) sk.u8[e] = (uint8_t)quant_u8(v);
    if (sk.gt) acc += sq_err(v, [&] { return (float)sk.gt[e] / 255.0f; });
}

// uniform over the grid (sk.gt is): one partial per workgroup, sk.sq [batch][gridDim.x of this launch]
__device__ __forceinline__ void rg_publish(const U8Sinks &sk, double (&acc)[1], double *red) {
    if (sk.gt) {
        block_sum<1>(acc, red);
        if (threadIdx.x == 0) sk.sq[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = acc[0];
    }
}

__device__ __forceinline__ int mirror_idx(int i, int n) {          // scipy.ndimage 'mirror': d c b | a b c d | c b a
    if (n == 1) return 0;
    i = i < 0 ? -i : i;
    const int p = 2 * (n - 1);
    i %= p;
    return i >= n ? p - i : i;
}

// skimage _warp_fast coord_map(dim, coord, 'R')
__device__ __forceinline__ int reflect_idx(int coord, int dim) {
    const int cmax = dim - 1;
    if (dim == 1) return 0;
    if (coord < 0) {
        const int n = -coord;
        return ((n / cmax) % 2 != 0) ? cmax - (n % cmax) : n % cmax;
    }
    if (coord > cmax) return ((coord / cmax) % 2 != 0) ? cmax - (coord % cmax) : coord % cmax;
    return coord;
}

// one axis of scipy.ndimage.gaussian_filter on an [H][W][3] image: out = sum_k w[k] in[mirror(i + k - r)]
template <typename T>
__global__ __launch_bounds__(kBlock) void rg_gauss_kernel(const T *__restrict__ in_, double *__restrict__ out_, int H, int W, int axis,
                                                         int radius, const double w0, const double w1, const double w2, int input_f32) {
    __shared__ double tab[IsU8<T>::v ? 256 : 1];
    if constexpr (IsU8<T>::v) {
        fill_u8_table(tab, input_f32, true);
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const size_t f0 = (size_t)blockIdx.y * H * W * 3;                // this frame
    const T *__restrict__ in = in_ + f0;
    double *__restrict__ out = out_ + f0;
    const int r = (int)(i / W), c = (int)(i % W);
    const double wk[3] = {w0, w1, w2};                      // symmetric kernel: w[|k|], radius <= 2
    double acc[3] = {0.0, 0.0, 0.0};
    for (int k = -radius; k <= radius; ++k) {
        const int rr = axis == 0 ? mirror_idx(r + k, H) : r, cc = axis == 1 ? mirror_idx(c + k, W) : c;
        const size_t p = ((size_t)rr * W + cc) * 3;
        const double g = wk[k < 0 ? -k : k];
        acc[0] += g * ld_u8(in, p, tab); acc[1] += g * ld_u8(in, p + 1, tab); acc[2] += g * ld_u8(in, p + 2, tab);
    }
    double *o = out + (size_t)i * 3;
    o[0] = acc[0]; o[1] = acc[1]; o[2] = acc[2];
}

// skimage warp(order=1, mode='reflect') of an [Hi][Wi][3] image to [Ho][Wo][3]: source = factor * (i + 0.5) - 0.5
template <typename T>
__global__ __launch_bounds__(kBlock) void rg_bilinear_kernel(const T *__restrict__ in_, double *__restrict__ out_, int Hi, int Wi, int Ho,
                                                            int Wo, double fr, double fc, int input_f32) {
    __shared__ double tab[IsU8<T>::v ? 256 : 1];
    if constexpr (IsU8<T>::v) {
        fill_u8_table(tab, input_f32, true);
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)Ho * Wo) return;
    const T *__restrict__ in = in_ + (size_t)blockIdx.y * Hi * Wi * 3;
    double *__restrict__ out = out_ + (size_t)blockIdx.y * Ho * Wo * 3;
    const int r = (int)(i / Wo), c = (int)(i % Wo);
    const double sr = fr * ((double)r + 0.5) - 0.5, sc = fc * ((double)c + 0.5) - 0.5;
    const int minr = (int)floor(sr), minc = (int)floor(sc), maxr = (int)ceil(sr), maxc = (int)ceil(sc);
    const double dr = sr - (double)minr, dc = sc - (double)minc;
    const int r0 = reflect_idx(minr, Hi), r1 = reflect_idx(maxr, Hi), c0 = reflect_idx(minc, Wi), c1 = reflect_idx(maxc, Wi);
    const size_t p00 = ((size_t)r0 * Wi + c0) * 3, p01 = ((size_t)r0 * Wi + c1) * 3;
    const size_t p10 = ((size_t)r1 * Wi + c0) * 3, p11 = ((size_t)r1 * Wi + c1) * 3;
    double *o = out + (size_t)i * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double top = (1.0 - dc) * ld_u8(in, p00 + ch, tab) + dc * ld_u8(in, p01 + ch, tab);
        const double bottom = (1.0 - dc) * ld_u8(in, p10 + ch, tab) + dc * ld_u8(in, p11 + ch, tab);
        o[ch] = (1.0 - dr) * top + dr * bottom;
    }
}


// iterative.py:91-98: gradient magnitude of the original image -> psi, phi  (wt[i] = {psi, phi})
template <typename T>
__global__ __launch_bounds__(kBlock) void rg_weights_kernel(const T *__restrict__ in_, double2 *__restrict__ wt_, int H, int W, double phi_scale,
                                                           int input_f32) {
    __shared__ double tab[IsU8<T>::v ? 256 : 1];
    if constexpr (IsU8<T>::v) {
        fill_u8_table(tab, input_f32, true);
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const T *__restrict__ in = in_ + (size_t)blockIdx.y * H * W * 3;
    double2 *__restrict__ wt = wt_ + (size_t)blockIdx.y * H * W;
    const int r = (int)(i / W), c = (int)(i % W);
    const size_t pr = ((size_t)r * W + min(c + 1, W - 1)) * 3, pl = ((size_t)r * W + max(c - 1, 0)) * 3;
    const size_t pd = ((size_t)min(r + 1, H - 1) * W + c) * 3, pu = ((size_t)max(r - 1, 0) * W + c) * 3;
    double s = 0.0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const double dx = ld_u8(in, pr + ch, tab) - ld_u8(in, pl + ch, tab), dy = ld_u8(in, pd + ch, tab) - ld_u8(in, pu + ch, tab);
        s += dx * dx + dy * dy;
    }
    const double delta = sqrt(s);
    double psi = 256.0 * delta / 5.0;
    psi = psi > 1.0 ? 1.0 : psi;
    wt[i] = make_double2(psi, phi_scale / (1.0 + 10.0 * delta));
}

// one sweep of iterative.py:106-115 (Jacobi: everything on the right-hand side is the previous iterate)
// LAST: the outputs and the metric partials (rg_emit) instead of `next`
template <typename T, bool LAST>
__global__ __launch_bounds__(kBlock) void rg_sweep_kernel(const double *__restrict__ prev_, const T *__restrict__ in_, const double *__restrict__ col_,
                                                         const double2 *__restrict__ wt_, double *__restrict__ next_, int H, int W, int input_f32,
                                                         U8Sinks sk) {
    __shared__ double tab[IsU8<T>::v ? 256 : 1];
    __shared__ double red[LAST ? 4 : 1];
    if constexpr (IsU8<T>::v) {
        fill_u8_table(tab, input_f32, true);
        __syncthreads();
    }
    const size_t f0 = (size_t)blockIdx.y * H * W;                   // this frame, in pixels
    const double *__restrict__ prev = prev_ + f0 * 3, *__restrict__ col = col_ + f0 * 3;
    const T *__restrict__ in = in_ + f0 * 3;
    const double2 *__restrict__ wt = wt_ + f0;
    double *__restrict__ next = LAST ? nullptr : next_ + f0 * 3;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double acc[1] = {0.0};
    if (i < (int64_t)H * W) {
        const int r = (int)(i / W), c = (int)(i % W);
        const size_t iR = (size_t)r * W + min(c + 1, W - 1), iL = (size_t)r * W + max(c - 1, 0);
        const size_t iD = (size_t)min(r + 1, H - 1) * W + c, iU = (size_t)max(r - 1, 0) * W + c;
        const double2 w0 = wt[i];
        const double psi = w0.x, phi = w0.y;
        const double phi1 = (wt[iR].y + phi) / 2, phi2 = (wt[iD].y + phi) / 2, phi3 = (wt[iL].y + phi) / 2, phi4 = (wt[iU].y + phi) / 2;
        const double den = psi + phi1 + phi2 + phi3 + phi4;
        const double eps = 1e-6, rho = 1 / 5.0;
        // (num / (den + eps)) * (1 - rho) of the reference as num * scale: the quotient does not depend on the channel or the sweep
        // (one float64 division per pixel instead of three per sweep; the last bit may differ from the reference's order, the
        // relaxation is contractive: 1e-15 on the result, tests/test_regrain.py asserts 1e-9)
        const double scale = (1 - rho) / (den + eps);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const double x = ld_u8(in, i * 3 + ch, tab);
            const double num = psi * col[i * 3 + ch] + phi1 * (prev[iR * 3 + ch] - ld_u8(in, iR * 3 + ch, tab) + x) +
                               phi2 * (prev[iD * 3 + ch] - ld_u8(in, iD * 3 + ch, tab) + x) + phi3 * (prev[iL * 3 + ch] - ld_u8(in, iL * 3 + ch, tab) + x) +
                               phi4 * (prev[iU * 3 + ch] - ld_u8(in, iU * 3 + ch, tab) + x);
            const double y = num * scale + rho * prev[i * 3 + ch];
            if constexpr (LAST) rg_emit(sk, (f0 + i) * 3 + ch, y, acc[0]);
            else next[i * 3 + ch] = y;
        }
    }
    if constexpr (LAST) rg_publish(sk, acc, red);
}

// K sweeps of rg_sweep_kernel in ONE launch (temporal blocking with a recomputed halo): a workgroup owns a th x tw tile of
// the level, loads it with a halo of k pixels and runs k Jacobi sweeps on the WHOLE region, synchronising with
// barriers instead of launch boundaries.  Region pixels whose neighbours lie outside the region use the nearest region pixel
// instead: that garbage travels inward one pixel per sweep and after k sweeps has eaten exactly the halo; the tile itself is
// what rg_sweep_kernel would have produced, operation for operation (the per-pixel arithmetic below is the same code).
// Neighbours outside the IMAGE are the pixel itself in both kernels (min / max clamping, iterative.py:100-104).
// A 1080p frame: 244 sweep launches become 31 (nbits 4, 16, 32, 64, 64, 64 with k = 8).
constexpr int kRgKMax = 8;
constexpr int kRgMaxRegion = 1536;                      // (16 + 2 k) x (32 + 2 k) at k = 8
constexpr int kRgPxPerThread = kRgMaxRegion / kBlock;   // 6

// LDS holds ONE quantity per pixel and channel, d = iterate - in (what a neighbour needs: the formula reads prev[k] - in[k]),
// twice for the ping-pong; everything else a pixel needs in every sweep lives in the registers of the thread that owns it:
// in, the current iterate, psi * col, the four neighbour weights and the hoisted scale.
template <typename T, bool LAST>
__global__ __launch_bounds__(kBlock) void rg_sweepk_kernel(const double *__restrict__ prev_, const T *__restrict__ in_, const double *__restrict__ col_,
                                                          const double2 *__restrict__ wt_, double *__restrict__ next_, int H, int W, int th, int tw,
                                                          int k, int tiles_x, int input_f32, U8Sinks sk) {
    extern __shared__ double lds[];
    __shared__ double tab[IsU8<T>::v ? 256 : 1];
    __shared__ double red[LAST ? 4 : 1];
    if constexpr (IsU8<T>::v) {
        fill_u8_table(tab, input_f32, true);
        __syncthreads();
    }
    const size_t f0 = (size_t)blockIdx.y * H * W;                   // this frame, in pixels
    const double *__restrict__ prev = prev_ + f0 * 3, *__restrict__ col = col_ + f0 * 3;
    const T *__restrict__ in = in_ + f0 * 3;
    const double2 *__restrict__ wt = wt_ + f0;
    double *__restrict__ next = LAST ? nullptr : next_ + f0 * 3;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int y0 = ty * th, x0 = tx * tw;
    // region = tile + halo, clipped to the image
    const int ry0 = max(y0 - k, 0), ry1 = min(y0 + th + k, H), rx0 = max(x0 - k, 0), rx1 = min(x0 + tw + k, W);
    const int rh = ry1 - ry0, rw = rx1 - rx0, rn = rh * rw;
    double *dA = lds, *dB = lds + 3 * kRgMaxRegion, *phiL = lds + 6 * kRgMaxRegion;
    double inr[kRgPxPerThread][3], cur[kRgPxPerThread][3], pc[kRgPxPerThread][3], ph[kRgPxPerThread][4], sc[kRgPxPerThread];
    int nb[kRgPxPerThread][4];
#pragma unroll
    for (int j = 0; j < kRgPxPerThread; ++j) {
        const int p = threadIdx.x + j * kBlock;
        if (p < rn) {
            const int r = p / rw, c = p - r * rw;
            const size_t g = (size_t)(ry0 + r) * W + (rx0 + c);
            const double2 w0 = wt[g];
            ph[j][0] = w0.x;                                   // psi for now
            phiL[p] = w0.y;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                inr[j][ch] = ld_u8(in, g * 3 + ch, tab); cur[j][ch] = prev[g * 3 + ch]; pc[j][ch] = col[g * 3 + ch];
                dA[p * 3 + ch] = cur[j][ch] - inr[j][ch];
            }
            // image clamping == region clamping wherever the region edge is an image edge; elsewhere: halo garbage
            nb[j][0] = r * rw + min(c + 1, rw - 1); nb[j][1] = min(r + 1, rh - 1) * rw + c;
            nb[j][2] = r * rw + max(c - 1, 0);      nb[j][3] = max(r - 1, 0) * rw + c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kRgPxPerThread; ++j) {
        const int p = threadIdx.x + j * kBlock;
        if (p < rn) {
            const double psi = ph[j][0], phi = phiL[p];
            const double phi1 = (phiL[nb[j][0]] + phi) / 2, phi2 = (phiL[nb[j][1]] + phi) / 2, phi3 = (phiL[nb[j][2]] + phi) / 2,
                         phi4 = (phiL[nb[j][3]] + phi) / 2;
            const double den = psi + phi1 + phi2 + phi3 + phi4;
            const double eps = 1e-6, rho = 1 / 5.0;
            sc[j] = (1 - rho) / (den + eps);
            ph[j][0] = phi1; ph[j][1] = phi2; ph[j][2] = phi3; ph[j][3] = phi4;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) pc[j][ch] = psi * pc[j][ch];
        }
    }
    double *dc = dA, *dn = dB;
    for (int sweep = 0; sweep < k; ++sweep) {
#pragma unroll
        for (int j = 0; j < kRgPxPerThread; ++j) {
            const int p = threadIdx.x + j * kBlock;
            if (p < rn) {
                const double rho = 1 / 5.0;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const double x = inr[j][ch];
                    const double num = pc[j][ch] + ph[j][0] * (dc[nb[j][0] * 3 + ch] + x) + ph[j][1] * (dc[nb[j][1] * 3 + ch] + x) +
                                       ph[j][2] * (dc[nb[j][2] * 3 + ch] + x) + ph[j][3] * (dc[nb[j][3] * 3 + ch] + x);
                    cur[j][ch] = num * sc[j] + rho * cur[j][ch];
                    dn[p * 3 + ch] = cur[j][ch] - x;
                }
            }
        }
        __syncthreads();
        double *t = dc; dc = dn; dn = t;
    }
    // the tile (the part of the region that lies k pixels away from every non-image edge of it)
    double acc[1] = {0.0};
#pragma unroll
    for (int j = 0; j < kRgPxPerThread; ++j) {
        const int p = threadIdx.x + j * kBlock;
        if (p < rn) {
            const int r = p / rw, c = p - r * rw, gy = ry0 + r, gx = rx0 + c;
            if (gy >= y0 && gy < min(y0 + th, H) && gx >= x0 && gx < min(x0 + tw, W)) {
                const size_t g = (size_t)gy * W + gx;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    if constexpr (LAST) rg_emit(sk, (f0 + g) * 3 + ch, cur[j][ch], acc[0]);
                    else next[g * 3 + ch] = cur[j][ch];
                }
            }
        }
    }
    if constexpr (LAST) rg_publish(sk, acc, red);
}

// the image itself as the result (nbits[0] == 0), or the bytes as the float64 start image of a one-level pyramid
template <typename T>
__global__ __launch_bounds__(kBlock) void rg_emit_kernel(const T *__restrict__ src, int64_t n_px, int input_f32, U8Sinks sk) {
    __shared__ double tab[IsU8<T>::v ? 256 : 1];
    __shared__ double red[4];
    if constexpr (IsU8<T>::v) {
        fill_u8_table(tab, input_f32, true);
        __syncthreads();
    }
    const size_t f0 = (size_t)blockIdx.y * n_px;
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    double acc[1] = {0.0};
    if (i < n_px) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) rg_emit(sk, (f0 + i) * 3 + ch, ld_u8(src, (f0 + i) * 3 + ch, tab), acc[0]);
    }
    rg_publish(sk, acc, red);
}

struct RgLevel { int h, w; };

static int rg_levels(int H, int W, int n_nbits, RgLevel *lv) {      // iterative.py:62-68: recurse while len(nbits) > 1 and h2 > 20 and w2 > 20
    int n = 0;
    lv[n++] = {H, W};
    while (n < n_nbits) {
        const int h2 = (lv[n - 1].h + 1) / 2, w2 = (lv[n - 1].w + 1) / 2;
        if (!(h2 > 20 && w2 > 20)) break;
        lv[n++] = {h2, w2};
    }
    return n;
}

static inline dim3 rg_grid(int64_t n, int batch) { return dim3((unsigned)((n + kBlock - 1) / kBlock), (unsigned)batch); }

// skimage.transform.resize(src [hi][wi][3] -> dst [ho][wo][3]) of `batch` frames; tmp: two [batch][hi][wi][3] buffers
// (down-scaling only).  T = uint8_t: the first launch reads the bytes, the rest float64.
template <typename T>
static int rg_resize(const T *src, int hi, int wi, double *dst, int ho, int wo, double *tmp0, double *tmp1, int batch, int input_f32, hipStream_t s) {
    const double fr = (double)hi / (double)ho, fc = (double)wi / (double)wo;
    int radius[2] = {0, 0};
    double wts[2][3] = {{1.0, 0.0, 0.0}, {1.0, 0.0, 0.0}};
    bool filtered[2] = {false, false};
    for (int axis = 0; axis < 2; ++axis) {
        const double f = axis == 0 ? fr : fc;
        const double sigma = f > 1.0 ? (f - 1.0) / 2.0 : 0.0;
        if (!(sigma > 1e-15)) continue;                               // scipy skips such axes
        radius[axis] = (int)(4.0 * sigma + 0.5);
        if (radius[axis] > 2) return CT_E_BADARG;                     // halving pyramids never get here
        double sum = 0.0;
        for (int k = -radius[axis]; k <= radius[axis]; ++k) sum += exp(-0.5 / (sigma * sigma) * (double)(k * k));
        for (int k = 0; k <= radius[axis]; ++k) wts[axis][k] = exp(-0.5 / (sigma * sigma) * (double)(k * k)) / sum;
        filtered[axis] = true;
    }
    // (a fused gaussian + gaussian + bilinear kernel was tried: bitwise the same, 0.7 ms SLOWER per 1080p frame -- its 100 strided
    // float64 gathers per output pixel coalesce badly; the three streaming launches stay)
    const double *cur = nullptr;                                      // nullptr: still the source itself
    double *bufs[2] = {tmp0, tmp1};
    int nb = 0;
    for (int axis = 0; axis < 2; ++axis) {
        if (!filtered[axis]) continue;
        if (cur == nullptr)
            hipLaunchKernelGGL((rg_gauss_kernel<T>), rg_grid((int64_t)hi * wi, batch), dim3(kBlock), 0, s, src, bufs[nb], hi, wi, axis, radius[axis],
                               wts[axis][0], wts[axis][1], wts[axis][2], input_f32);
        else
            hipLaunchKernelGGL((rg_gauss_kernel<double>), rg_grid((int64_t)hi * wi, batch), dim3(kBlock), 0, s, cur, bufs[nb], hi, wi, axis,
                               radius[axis], wts[axis][0], wts[axis][1], wts[axis][2], 0);
        CT_CHECK_LAUNCH();
        cur = bufs[nb];
        nb ^= 1;
    }
    if (cur == nullptr)
        hipLaunchKernelGGL((rg_bilinear_kernel<T>), rg_grid((int64_t)ho * wo, batch), dim3(kBlock), 0, s, src, dst, hi, wi, ho, wo, fr, fc, input_f32);
    else
        hipLaunchKernelGGL((rg_bilinear_kernel<double>), rg_grid((int64_t)ho * wo, batch), dim3(kBlock), 0, s, cur, dst, hi, wi, ho, wo, fr, fc, 0);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

// ---- workspace: two resize scratch images [batch][H][W][3]; per level {in, col} (the halved images; on level 0 they are the
// caller's, the float64 entry keeps the two unused level-0 slots of its published size), two iterates and {psi, phi}, every one
// [batch][h][w][.]; then the metric partials [batch][rg_parts] ------------------------------------------------------------------
static size_t rg_parts(int H, int W) {               // workgroups of any last launch: one pixel per thread, or the small tiles
    const size_t flat = ((size_t)H * W + kBlock - 1) / kBlock, tiles = (size_t)((H + 7) / 8) * ((W + 15) / 16);
    return flat > tiles ? flat : tiles;
}
static size_t rg_ws_doubles(int batch, int H, int W, int n_nbits, bool l0_copies) {
    RgLevel lv[kRgMaxLevels];
    const int n = rg_levels(H, W, n_nbits, lv);
    size_t per_frame = (size_t)H * W * 3 * 2;
    for (int l = 0; l < n; ++l) per_frame += (size_t)lv[l].h * lv[l].w * ((l > 0 || l0_copies ? 3 * 4 : 3 * 2) + 2);
    return (size_t)batch * (per_frame + rg_parts(H, W));
}
static bool rg_size_ok(int batch, int H, int W, int n_nbits) {
    return batch >= 1 && batch <= 65535 && H >= 1 && W >= 1 && (int64_t)H * W <= 0x7fffffff && n_nbits >= 1 && n_nbits <= kRgMaxLevels;
}

template <typename T, bool LAST> static hipError_t rg_sweepk_attr() {
    static DynLdsAttr attr;             // per device and instantiation
    return attr.ensure(reinterpret_cast<const void *>(rg_sweepk_kernel<T, LAST>), 7 * kRgMaxRegion * sizeof(double));
}

// nbits[l] sweeps on one level.  T: the element type of `in` (uint8_t on level 0 of the byte entries).  last: this is level 0, so
// the final launch is the LAST form and writes `sk`; *n_parts: its workgroups per frame.  *result: the level's solution (not on
// the last level).
template <typename T>
static int rg_relax(const double *start, const T *in, const double *col, double2 *wt, double *it_a, double *it_b, int h, int w, int level, int n_sweeps,
                    bool last, int batch, int input_f32, const U8Sinks &sk, const double **result, int *n_parts, hipStream_t s) {
    const int64_t px = (int64_t)h * w;
    const U8Sinks none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL((rg_weights_kernel<T>), rg_grid(px, batch), dim3(kBlock), 0, s, in, wt, h, w, 30.0 * exp2(-(double)level), input_f32);
    CT_CHECK_LAUNCH();
    const double *prev = start;
    static const int kblock = [] { const int v = env_int("CT_HIP_REGRAIN_K", kRgKMax); return v < 1 ? 1 : (v > kRgKMax ? kRgKMax : v); }();
    // small levels: small tiles (a launch lasts as long as its slowest workgroup: k sweeps of region / 256 pixels per thread)
    const int th = px > 200000 ? 16 : 8, tw = px > 200000 ? 32 : 16;
    const int tiles_x = (w + tw - 1) / tw, tiles_y = (h + th - 1) / th;
    const size_t lds = (size_t)7 * kRgMaxRegion * sizeof(double);
    for (int i = 0; i < n_sweeps;) {
        const int kk = n_sweeps - i < kblock ? n_sweeps - i : kblock;
        double *next = (prev == it_b) ? it_a : it_b;               // ping-pong
        if (last && i + kk == n_sweeps) {                           // the LAST sweep of level 0 lands in the caller's buffers
            if (kk == 1) {
                hipLaunchKernelGGL((rg_sweep_kernel<T, true>), rg_grid(px, batch), dim3(kBlock), 0, s, prev, in, col, wt, (double *)nullptr, h, w,
                                   input_f32, sk);
                *n_parts = (int)rg_grid(px, batch).x;
            } else {
                hipLaunchKernelGGL((rg_sweepk_kernel<T, true>), dim3(tiles_x * tiles_y, batch), dim3(kBlock), lds, s, prev, in, col, wt,
                                   (double *)nullptr, h, w, th, tw, kk, tiles_x, input_f32, sk);
                *n_parts = tiles_x * tiles_y;
            }
            CT_CHECK_LAUNCH();
            *result = nullptr;
            return CT_OK;
        }
        if (kk == 1) {
            hipLaunchKernelGGL((rg_sweep_kernel<T, false>), rg_grid(px, batch), dim3(kBlock), 0, s, prev, in, col, wt, next, h, w, input_f32, none);
        } else {
            hipLaunchKernelGGL((rg_sweepk_kernel<T, false>), dim3(tiles_x * tiles_y, batch), dim3(kBlock), lds, s, prev, in, col, wt, next, h, w, th,
                               tw, kk, tiles_x, input_f32, none);
        }
        CT_CHECK_LAUNCH();
        prev = next;
        i += kk;
    }
    if (last) {                                                     // no sweep on the finest level: the start image is the result
        hipLaunchKernelGGL((rg_emit_kernel<double>), rg_grid(px, batch), dim3(kBlock), 0, s, prev, px, 0, sk);
        CT_CHECK_LAUNCH();
        *n_parts = (int)rg_grid(px, batch).x;
    }
    *result = prev;
    return CT_OK;
}

// The regrain of `batch` frames of one size; every argument has been checked.  T = double: ct_regrain_f64 (l0_copies: its
// published workspace layout).  T = uint8_t: img_in are the bytes of the target.  sk.sq is set here.
template <typename T>
static int rg_run(const T *img_in, const double *img_col, int batch, int height, int width, int input_f32, const int *nbits, int n_nbits,
                  bool l0_copies, U8Sinks sk, double *psnr_out, void *ws, hipStream_t s) {
    constexpr bool U8 = IsU8<T>::v;
    if (rg_sweepk_attr<double, false>() != hipSuccess || rg_sweepk_attr<T, false>() != hipSuccess || rg_sweepk_attr<T, true>() != hipSuccess)
        return CT_E_BADARG;
    RgLevel lv[kRgMaxLevels];
    const int n = rg_levels(height, width, n_nbits, lv);
    const size_t B = (size_t)batch;
    double *p = reinterpret_cast<double *>(ws);
    double *tmp0 = p; p += B * height * width * 3;
    double *tmp1 = p; p += B * height * width * 3;
    const double *in_l[kRgMaxLevels], *col_l[kRgMaxLevels];           // in_l[0] is img_in (of type T), not this array's entry
    double *it_a[kRgMaxLevels], *it_b[kRgMaxLevels];
    double2 *wt_l[kRgMaxLevels];
    in_l[0] = nullptr;
    col_l[0] = img_col;
    for (int l = 0; l < n; ++l) {
        const size_t px = B * lv[l].h * lv[l].w;
        double *a = nullptr, *b = nullptr;
        if (l > 0 || l0_copies) {
            a = p; p += px * 3;
            b = p; p += px * 3;
        }
        it_a[l] = p; p += px * 3;
        it_b[l] = p; p += px * 3;
        wt_l[l] = reinterpret_cast<double2 *>(p); p += px * 2;
        if (l > 0) {
            int rc = l == 1 ? rg_resize<T>(img_in, lv[0].h, lv[0].w, a, lv[1].h, lv[1].w, tmp0, tmp1, batch, input_f32, s)
                            : rg_resize<double>(in_l[l - 1], lv[l - 1].h, lv[l - 1].w, a, lv[l].h, lv[l].w, tmp0, tmp1, batch, 0, s);
            if (rc) return rc;
            if ((rc = rg_resize<double>(col_l[l - 1], lv[l - 1].h, lv[l - 1].w, b, lv[l].h, lv[l].w, tmp0, tmp1, batch, 0, s))) return rc;
            in_l[l] = a; col_l[l] = b;
        }
    }
    sk.sq = p;
    const U8Sinks none = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const double *coarse = nullptr;                                    // the solution of level l + 1
    int n_parts = 0;
    for (int l = n - 1; l >= 0; --l) {
        const int h = lv[l].h, w = lv[l].w;
        const double *start;
        if (coarse != nullptr) {
            const int rc = rg_resize<double>(coarse, lv[l + 1].h, lv[l + 1].w, it_a[l], h, w, tmp0, tmp1, batch, 0, s);
            if (rc) return rc;
            start = it_a[l];
        } else if (l > 0) {
            start = in_l[l];                                           // iterative.py:74: img_arr_out = img_arr_in
        } else if constexpr (U8) {                                     // a one-level pyramid: the bytes as the float64 start image
            U8Sinks as_f64 = none;
            as_f64.f64 = it_a[0];
            hipLaunchKernelGGL((rg_emit_kernel<uint8_t>), rg_grid((int64_t)h * w, batch), dim3(kBlock), 0, s, img_in, (int64_t)h * w, input_f32, as_f64);
            CT_CHECK_LAUNCH();
            start = it_a[0];
        } else {
            start = img_in;
        }
        const int rc = l == 0 ? rg_relax<T>(start, img_in, col_l[0], wt_l[0], it_a[0], it_b[0], h, w, 0, nbits[0], true, batch, input_f32, sk, &coarse,
                                            &n_parts, s)
                              : rg_relax<double>(start, in_l[l], col_l[l], wt_l[l], it_a[l], it_b[l], h, w, l, nbits[l], false, batch, 0, none, &coarse,
                                                 &n_parts, s);
        if (rc) return rc;
    }
    // the tiled sweep of a large frame has more workgroups than kMaxBlocksPerImage: the rows of sk.sq are n_parts apart
    if (sk.gt) return launch_psnr_finish(sk.sq, n_parts, n_parts, (int64_t)height * width * 3, batch, psnr_out, s);
    return CT_OK;
}

static bool rg_nbits_ok(const int *nbits, int n_nbits) {
    if (!nbits || n_nbits < 1 || n_nbits > kRgMaxLevels) return false;
    for (int i = 0; i < n_nbits; ++i)
        if (nbits[i] < 0) return false;
    return true;
}

}  // namespace ct

extern "C" {

size_t ct_regrain_workspace_bytes(int height, int width) {
    if (height < 1 || width < 1) return 0;
    ct::RgLevel lv[ct::kRgMaxLevels];
    const int n = ct::rg_levels(height, width, 6, lv);
    size_t doubles = (size_t)height * width * 3 * 2;                   // two resize scratch images at the finest size
    for (int l = 0; l < n; ++l) doubles += (size_t)lv[l].h * lv[l].w * (3 * 4 + 2);   // in, col, two iterates, {psi, phi}
    return doubles * sizeof(double) + 256;
}

// img_in, img_col, out: device [height][width][3] float64 (out may not alias the inputs); nbits: host array (the reference's
// default is {4, 16, 32, 64, 64, 64}); one frame per call: the batch-1 call of rg_run.
int ct_regrain_f64(const double *img_in, const double *img_col, double *out, int height, int width, const int *nbits, int n_nbits,
                   void *ws, size_t ws_bytes, void *stream) {
    using namespace ct;
    if (!img_in || !img_col || !out || !nbits || height < 1 || width < 1 || n_nbits < 1 || n_nbits > kRgMaxLevels) return CT_E_BADARG;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < ct_regrain_workspace_bytes(height, width)) return CT_E_WORKSPACE;
    if (!rg_size_ok(1, height, width, n_nbits) || !rg_nbits_ok(nbits, n_nbits)) return CT_E_BADARG;
    if (ws_bytes < (rg_ws_doubles(1, height, width, n_nbits, true) - rg_parts(height, width)) * sizeof(double)) return CT_E_WORKSPACE;   // more than 6 levels
    const U8Sinks sk = {out, nullptr, nullptr, nullptr, nullptr};
    return rg_run<double>(img_in, img_col, 1, height, width, 0, nbits, n_nbits, true, sk, nullptr, ws, (hipStream_t)stream);
}

size_t ct_regrain_u8_workspace_bytes(int batch, int height, int width, int n_nbits) {
    if (!ct::rg_size_ok(batch, height, width, n_nbits)) return 0;
    return (ct::rg_ws_doubles(batch, height, width, n_nbits, false) * sizeof(double) + 15) & ~(size_t)15;
}

int ct_regrain_u8(const uint8_t *img_in, const double *img_col, int batch, int height, int width, int input_f32, const int *nbits, int n_nbits,
                  double *out_f64, float *out_f32, uint8_t *out_u8, const uint8_t *gt, double *psnr_out, void *ws, size_t ws_bytes, void *stream) {
    using namespace ct;
    if (!img_in || !img_col || !rg_size_ok(batch, height, width, n_nbits) || !rg_nbits_ok(nbits, n_nbits)) return CT_E_BADARG;
    if (reinterpret_cast<uintptr_t>(img_col) & 7) return CT_E_ALIGN;
    const int rc = check_u8_outputs(gt, out_f64, out_f32, out_u8, psnr_out);
    if (rc) return rc;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < ct_regrain_u8_workspace_bytes(batch, height, width, n_nbits)) return CT_E_WORKSPACE;
    const U8Sinks sk = {out_f64, out_f32, out_u8, gt, nullptr};
    return rg_run<uint8_t>(img_in, img_col, batch, height, width, input_f32 ? 1 : 0, nbits, n_nbits, false, sk, psnr_out, ws, (hipStream_t)stream);
}

// workspace of ct_acg_u8: ct_idt_u8's (no state of its own), the float64 IDT result [batch][H][W][3], ct_regrain_u8's
static size_t acg_idt_bytes(int batch, int height, int width, int n_iter, int bins) {
    if (n_iter < 1) return 0;
    return (ct_idt_u8_workspace_bytes(batch, n_iter, bins, (int64_t)height * width, 0) + 15) & ~(size_t)15;
}
static size_t acg_state_bytes(int batch, int height, int width) { return ((size_t)batch * height * width * 3 * sizeof(double) + 15) & ~(size_t)15; }

size_t ct_acg_u8_workspace_bytes(int batch, int height, int width, int n_iter, int bins, int n_nbits) {
    const size_t rg = ct_regrain_u8_workspace_bytes(batch, height, width, n_nbits);
    if (rg == 0) return 0;
    const size_t idt = acg_idt_bytes(batch, height, width, n_iter, bins);
    if (idt == 0) return 0;
    return idt + acg_state_bytes(batch, height, width) + rg;
}

int ct_acg_u8(const uint8_t *target, const uint8_t *reference, int64_t n_r, const uint8_t *gt, int batch, int height, int width, const double *rot,
              const double *rinv, int n_iter, int bins, int input_f32, const int *nbits, int n_nbits, double *out_f64, float *out_f32,
              uint8_t *out_u8, double *psnr_out, void *ws, size_t ws_bytes, void *stream) {
    using namespace ct;
    if (!target || !reference || n_r < 1 || !rot || !rinv || n_iter < 1 || !rg_size_ok(batch, height, width, n_nbits) || !rg_nbits_ok(nbits, n_nbits))
        return CT_E_BADARG;
    const size_t need = ct_acg_u8_workspace_bytes(batch, height, width, n_iter, bins, n_nbits);
    if (need == 0) return CT_E_BADARG;                                 // bins
    const int rc = check_u8_outputs(gt, out_f64, out_f32, out_u8, psnr_out);
    if (rc) return rc;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < need) return CT_E_WORKSPACE;
    char *w = reinterpret_cast<char *>(ws);
    const size_t idt_bytes = acg_idt_bytes(batch, height, width, n_iter, bins);
    double *graded = reinterpret_cast<double *>(w + idt_bytes);
    const int f32 = input_f32 ? 1 : 0;
    const int ri = ct_idt_u8(target, (int64_t)height * width, reference, n_r, nullptr, batch, rot, rinv, n_iter, bins, f32, f32, graded, nullptr, nullptr,
                             nullptr, ws, idt_bytes, nullptr, stream);
    if (ri) return ri;
    const U8Sinks sk = {out_f64, out_f32, out_u8, gt, nullptr};
    return rg_run<uint8_t>(target, graded, batch, height, width, f32, nbits, n_nbits, false, sk, psnr_out, w + idt_bytes + acg_state_bytes(batch, height, width),
                           (hipStream_t)stream);
}

}  // extern "C"
