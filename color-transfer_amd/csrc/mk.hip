// mk.hip -- the Monge-Kantorovich / Xiao side of the reference's methods/linear.py on gfx950 (MI355X):
//   A3  np.mean + np.cov                  (linear.py:64-67,103-106)-> moments_kernel<T, false>   (ct_moments.h)
//   A4  the 3x3 algebra of the MK map     (linear.py:108-118)      -> mk_coef_kernel
//   A5  (x - mu_t) @ A + mu_r             (linear.py:80,122)       -> affine3x3_kernel
#include "ct_moments.h"

namespace ct {

// -------------------------------------------------------------------------------------------
// A5: out = (x - mu_t) @ A + mu_r, float64 arithmetic, unclipped
// -------------------------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ __launch_bounds__(kBlock) void affine3x3_kernel(const TI *__restrict__ in, const double *__restrict__ coef,
                                                           TO *__restrict__ out, int64_t n_pixels) {
    const int img = blockIdx.y;
    const TI *p = in + (size_t)img * n_pixels * 3;
    TO *o = out + (size_t)img * n_pixels * 3;
    const bool vin = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    const bool vout = (reinterpret_cast<uintptr_t>(o) & 15) == 0;
    const double *cf = coef + (size_t)img * 16;
    double A[9], mt[3], mr[3];
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = cf[i];
#pragma unroll
    for (int i = 0; i < 3; ++i) { mt[i] = cf[9 + i]; mr[i] = cf[12 + i]; }

    auto px = [&](double r, double g, double b, TO &o0, TO &o1, TO &o2) {
        const double d0 = r - mt[0], d1 = g - mt[1], d2 = b - mt[2];
        // same order as a row-vector @ matrix product: sum over i of d_i A[i][j], then + mu_r
        o0 = (TO)(fma(d2, A[6], fma(d1, A[3], d0 * A[0])) + mr[0]);
        o1 = (TO)(fma(d2, A[7], fma(d1, A[4], d0 * A[1])) + mr[1]);
        o2 = (TO)(fma(d2, A[8], fma(d1, A[5], d0 * A[2])) + mr[2]);
    };
    const int64_t n_chunks = n_pixels >> 2;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    constexpr bool kF32IO = sizeof(TI) == 4 && sizeof(TO) == 4;
    __shared__ float xpose[kF32IO ? kBlock * 12 : 1];   // per-wave 3 KiB transpose buffers (float I/O only)
    for (int64_t ch0 = (int64_t)blockIdx.x * kBlock; ch0 < n_chunks; ch0 += stride) {
        const int64_t ch = ch0 + threadIdx.x;
        const int64_t wave_c0 = ch0 + (threadIdx.x & ~63);
        const bool full_wave = wave_c0 + 64 <= n_chunks;          // wave-uniform
        if (kF32IO && vin && vout && full_wave) {
            // fully coalesced 16-byte global accesses (lane i <-> base + 16 i, three times per wave); the HWC de-interleave
            // into "4 whole pixels per lane" and back happens in a per-wave LDS buffer (conflict-free b128 accesses)
            const int lane = threadIdx.x & 63;
            float *lw = xpose + (threadIdx.x >> 6) * (64 * 12);
            const float4 *g = reinterpret_cast<const float4 *>(p + wave_c0 * 12);
            float4 *l4 = reinterpret_cast<float4 *>(lw);
            l4[lane] = g[lane]; l4[64 + lane] = g[64 + lane]; l4[128 + lane] = g[128 + lane];
            __builtin_amdgcn_wave_barrier();
            const float4 *r4 = reinterpret_cast<const float4 *>(lw + lane * 12);
            const float4 a0 = r4[0], a1 = r4[1], a2 = r4[2];
            const float vi[12] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w, a2.x, a2.y, a2.z, a2.w};
            TO w[12];
#pragma unroll
            for (int q = 0; q < 4; ++q) px((double)vi[3 * q], (double)vi[3 * q + 1], (double)vi[3 * q + 2], w[3 * q], w[3 * q + 1], w[3 * q + 2]);
            __builtin_amdgcn_wave_barrier();
            float4 *w4 = reinterpret_cast<float4 *>(lw + lane * 12);
            w4[0] = make_float4((float)w[0], (float)w[1], (float)w[2], (float)w[3]);
            w4[1] = make_float4((float)w[4], (float)w[5], (float)w[6], (float)w[7]);
            w4[2] = make_float4((float)w[8], (float)w[9], (float)w[10], (float)w[11]);
            __builtin_amdgcn_wave_barrier();
            float4 *go = reinterpret_cast<float4 *>(reinterpret_cast<float *>(o) + wave_c0 * 12);
            go[lane] = l4[lane]; go[64 + lane] = l4[64 + lane]; go[128 + lane] = l4[128 + lane];
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        if (ch >= n_chunks) continue;
        double v[12];
        TO w[12];
        load12<TI>(p + ch * 12, vin, v);
#pragma unroll
        for (int q = 0; q < 4; ++q) px(v[3 * q], v[3 * q + 1], v[3 * q + 2], w[3 * q], w[3 * q + 1], w[3 * q + 2]);
        store12<TO>(o + ch * 12, vout, w);
    }
    if (blockIdx.x == 0) {
        const int64_t q = (n_chunks << 2) + threadIdx.x;
        if (threadIdx.x < 3 && q < n_pixels) {
            TO a, b, d;
            px((double)p[q * 3], (double)p[q * 3 + 1], (double)p[q * 3 + 2], a, b, d);
            o[q * 3] = a; o[q * 3 + 1] = b; o[q * 3 + 2] = d;
        }
    }
}

// -------------------------------------------------------------------------------------------
// A4 (sync-free variant): the 3x3 algebra of monge_kantorovitch_color_transfer on the device
// (methods/linear.py:108-118).  One thread per pair, float64.  The matrix square root of a symmetric
// positive (semi)definite 3x3 is V diag(sqrt(lambda)) V^T from a cyclic Jacobi eigen-decomposition;
// it is unique, so no LAPACK sign convention is involved (Xiao's SVD-based T is NOT sign invariant
// and stays on the host).  mode: 0 = "MK", 1 = "sqrt", 2 = "cholesky".
// coef[b] = { T (row-major, out = (x - mu_t) @ T + mu_r), mu_t, mu_r, 0 }.
// -------------------------------------------------------------------------------------------
struct M3 { double a[3][3]; };

__device__ inline M3 m3_mul(const M3 &x, const M3 &y) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.a[i][j] = fma(x.a[i][2], y.a[2][j], fma(x.a[i][1], y.a[1][j], x.a[i][0] * y.a[0][j]));
    return r;
}

__device__ inline void m3_eig_sym(M3 s, M3 &v, double (&lam)[3]) {   // s = v diag(lam) v^T, cyclic Jacobi
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) v.a[i][j] = (i == j) ? 1.0 : 0.0;
    const double tiny = 1e-32 * (fabs(s.a[0][0]) + fabs(s.a[1][1]) + fabs(s.a[2][2]));
    for (int sweep = 0; sweep < 12; ++sweep) {
        const double off = fabs(s.a[0][1]) + fabs(s.a[0][2]) + fabs(s.a[1][2]);
        if (off <= tiny) break;          // quadratic convergence: 4-5 sweeps for a 3x3
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = s.a[p][q];
                // the usual Jacobi threshold: an entry below the rounding of its two diagonal neighbours stays (it moves
                // the eigenvalues by less than an ulp).  Rotating it away turns v by an arbitrary angle where two
                // eigenvalues agree to rounding (c I plus noise) and costs f(s) several ulp; it also covers apq == 0.
                if (fabs(apq) <= 0x1p-52 * (sqrt(fabs(s.a[p][p])) * sqrt(fabs(s.a[q][q])))) continue;
                rotated = true;
                const double theta = (s.a[q][q] - s.a[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                for (int k = 0; k < 3; ++k) {   // columns p, q of s
                    const double skp = s.a[k][p], skq = s.a[k][q];
                    s.a[k][p] = c * skp - sn * skq;
                    s.a[k][q] = sn * skp + c * skq;
                }
                for (int k = 0; k < 3; ++k) {   // rows p, q of s
                    const double spk = s.a[p][k], sqk = s.a[q][k];
                    s.a[p][k] = c * spk - sn * sqk;
                    s.a[q][k] = sn * spk + c * sqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = v.a[k][p], vkq = v.a[k][q];
                    v.a[k][p] = c * vkp - sn * vkq;
                    v.a[k][q] = sn * vkp + c * vkq;
                }
            }
        if (!rotated) break;
    }
    for (int i = 0; i < 3; ++i) lam[i] = s.a[i][i];
}

__device__ inline M3 m3_from_eig(const M3 &v, const double (&lam)[3], int fn) {   // v f(diag(lam)) v^T
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) {
                const double f = fn == 0 ? sqrt(lam[k]) : 1.0 / sqrt(lam[k]);
                acc = fma(v.a[i][k] * f, v.a[j][k], acc);
            }
            r.a[i][j] = acc;
        }
    return r;
}

__device__ inline M3 m3_fun_sym(const M3 &s, int fn) {   // fn 0: sqrt, 1: inverse sqrt  (of a symmetric PSD matrix)
    M3 v;
    double lam[3];
    m3_eig_sym(s, v, lam);
    return m3_from_eig(v, lam, fn);
}

// lower L with L L^T = s.  semidefinite: a pivot that is exactly zero leaves its column zero (the factor of a PSD matrix; an
// all-zero reference covariance then maps every pixel to mu_r, like the other two forms) instead of dividing 0 by 0; the
// target's factor is inverted, so there a zero pivot stays the NaN it is.
__device__ inline M3 m3_chol(const M3 &s, bool semidefinite) {
    M3 l;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) l.a[i][j] = 0.0;
    auto over = [&](double x, double d) { return semidefinite && d == 0.0 ? 0.0 : x / d; };
    l.a[0][0] = sqrt(s.a[0][0]);
    l.a[1][0] = over(s.a[1][0], l.a[0][0]);
    l.a[2][0] = over(s.a[2][0], l.a[0][0]);
    l.a[1][1] = sqrt(s.a[1][1] - l.a[1][0] * l.a[1][0]);
    l.a[2][1] = over(s.a[2][1] - l.a[2][0] * l.a[1][0], l.a[1][1]);
    l.a[2][2] = sqrt(s.a[2][2] - l.a[2][0] * l.a[2][0] - l.a[2][1] * l.a[2][1]);
    return l;
}

__device__ inline M3 m3_inv_lower(const M3 &l) {
    M3 r;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) r.a[i][j] = 0.0;
    r.a[0][0] = 1.0 / l.a[0][0];
    r.a[1][1] = 1.0 / l.a[1][1];
    r.a[2][2] = 1.0 / l.a[2][2];
    r.a[1][0] = -l.a[1][0] * r.a[0][0] * r.a[1][1];
    r.a[2][1] = -l.a[2][1] * r.a[1][1] * r.a[2][2];
    r.a[2][0] = -(l.a[2][0] * r.a[0][0] + l.a[2][1] * r.a[1][0]) * r.a[2][2];
    return r;
}

__global__ void mk_coef_kernel(const double *__restrict__ stats_t, const double *__restrict__ stats_r, int mode, int batch,
                               double *__restrict__ coef) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    const double *st = stats_t + (size_t)b * CT_RGB_STATS_STRIDE, *sr = stats_r + (size_t)b * CT_RGB_STATS_STRIDE;
    M3 ct_, cr;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { ct_.a[i][j] = st[3 + 3 * i + j]; cr.a[i][j] = sr[3 + 3 * i + j]; }
    M3 T;
    if (mode == 0) {            // A = sqrtm(St); T = A^-1 sqrtm(A Sr A) A^-1          (linear.py:116-118)
        M3 vt;
        double lt[3];
        m3_eig_sym(ct_, vt, lt);
        const M3 A = m3_from_eig(vt, lt, 0), Ai = m3_from_eig(vt, lt, 1);
        M3 mid = m3_mul(m3_mul(A, cr), A);
        for (int i = 0; i < 3; ++i)   // symmetrise the rounding residue before the eigen-decomposition
            for (int j = i + 1; j < 3; ++j) { const double h = 0.5 * (mid.a[i][j] + mid.a[j][i]); mid.a[i][j] = h; mid.a[j][i] = h; }
        T = m3_mul(m3_mul(Ai, m3_fun_sym(mid, 0)), Ai);
    } else if (mode == 1) {     // T = sqrtm(Sr) sqrtm(St)^-1                         (linear.py:112-115)
        T = m3_mul(m3_fun_sym(cr, 0), m3_fun_sym(ct_, 1));
    } else {                    // T = chol(Sr) chol(St)^-1                           (linear.py:108-111)
        T = m3_mul(m3_chol(cr, true), m3_inv_lower(m3_chol(ct_, false)));
    }
    double *o = coef + (size_t)b * 16;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) o[3 * i + j] = T.a[i][j];
    for (int i = 0; i < 3; ++i) { o[9 + i] = st[i]; o[12 + i] = sr[i]; }
    o[15] = 0.0;
}

// -------------------------------------------------------------------------------------------
// host-side launchers
// -------------------------------------------------------------------------------------------
template <typename T>
static int rgb_meancov_impl(const T *rgb, int64_t n_pixels, int n_images, double *stats, void *ws, size_t ws_bytes,
                            void *stream) {
    int rc = check_image_args(rgb, n_pixels, n_images);
    if (rc) return rc;
    if (n_images > 0 && stats == nullptr) return CT_E_BADARG;
    if ((rc = check_ws(ws, ws_bytes, n_images))) return rc;
    return launch_moments<T, false>(rgb, rgb, n_images, n_images, n_pixels, ws_carve(ws, n_images), stats,
                                    (hipStream_t)stream);
}

template <typename TI, typename TO>
static int affine_impl(const TI *in, const double *coef, TO *out, int64_t n_pixels, int batch, void *stream) {
    int rc = check_image_args(in, n_pixels, batch);
    if (rc) return rc;
    if ((rc = check_image_args(out, n_pixels, batch))) return rc;
    if (batch > 0 && coef == nullptr) return CT_E_BADARG;
    if (batch == 0 || n_pixels == 0) return CT_OK;
    const int G = blocks_per_image(n_pixels >> 2, batch);
    hipLaunchKernelGGL((affine3x3_kernel<TI, TO>), dim3(G, batch), dim3(kBlock), 0, (hipStream_t)stream, in, coef,
                       out, n_pixels);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

// a3 fused: moments of all 2*batch images in one sweep, finishing kernel, 3x3 algebra, affine apply -- no host sync
template <typename T, typename TO>
static int mk_impl(const T *target, const T *reference, TO *out, int64_t n_pixels, int batch, int decomposition, void *ws,
                   size_t ws_bytes, void *stream) {
    int rc = check_image_args(target, n_pixels, batch);
    if (rc) return rc;
    if ((rc = check_image_args(reference, n_pixels, batch))) return rc;
    if ((rc = check_image_args(out, n_pixels, batch))) return rc;
    if (decomposition < 0 || decomposition > 2) return CT_E_BADARG;
    if ((rc = check_ws(ws, ws_bytes, 2 * batch))) return rc;
    if (batch == 0 || n_pixels == 0) return CT_OK;
    const WsLayout l = ws_carve(ws, 2 * batch);
    hipStream_t s = (hipStream_t)stream;
    rc = launch_moments<T, false>(target, reference, batch, 2 * batch, n_pixels, l, l.stats, s);
    if (rc) return rc;
    // coefficient records live behind the stats records (the workspace reserves CT_RGB_STATS_STRIDE doubles per image)
    double *coef = l.partials;   // the partial sums are dead once the finishing kernel has run
    hipLaunchKernelGGL(mk_coef_kernel, dim3((batch + 63) / 64), dim3(64), 0, s, (const double *)l.stats,
                       (const double *)(l.stats + (size_t)batch * CT_RGB_STATS_STRIDE), decomposition, batch, coef);
    CT_CHECK_LAUNCH();
    return affine_impl<T, TO>(target, coef, out, n_pixels, batch, stream);
}

}  // namespace ct

// -------------------------------------------------------------------------------------------
// C ABI (include/ct_hip.h)
// -------------------------------------------------------------------------------------------
extern "C" {

int ct_rgb_meancov_f32(const float *rgb, int64_t n_pixels, int n_images, double *stats, void *ws, size_t ws_bytes,
                       void *stream) {
    return ct::rgb_meancov_impl<float>(rgb, n_pixels, n_images, stats, ws, ws_bytes, stream);
}
int ct_rgb_meancov_f64(const double *rgb, int64_t n_pixels, int n_images, double *stats, void *ws, size_t ws_bytes,
                       void *stream) {
    return ct::rgb_meancov_impl<double>(rgb, n_pixels, n_images, stats, ws, ws_bytes, stream);
}

int ct_mk_f32_f32(const float *target, const float *reference, float *out, int64_t n_pixels, int batch, int decomposition, void *ws,
                  size_t ws_bytes, void *stream) {
    return ct::mk_impl<float, float>(target, reference, out, n_pixels, batch, decomposition, ws, ws_bytes, stream);
}
int ct_mk_f32_f64(const float *target, const float *reference, double *out, int64_t n_pixels, int batch, int decomposition, void *ws,
                  size_t ws_bytes, void *stream) {
    return ct::mk_impl<float, double>(target, reference, out, n_pixels, batch, decomposition, ws, ws_bytes, stream);
}
int ct_mk_f64_f64(const double *target, const double *reference, double *out, int64_t n_pixels, int batch, int decomposition, void *ws,
                  size_t ws_bytes, void *stream) {
    return ct::mk_impl<double, double>(target, reference, out, n_pixels, batch, decomposition, ws, ws_bytes, stream);
}

int ct_mk_coef_f64(const double *stats_t, const double *stats_r, int decomposition, int batch, double *coef, void *stream) {
    if (!stats_t || !stats_r || !coef || batch < 0 || decomposition < 0 || decomposition > 2) return CT_E_BADARG;
    if (batch == 0) return CT_OK;
    hipLaunchKernelGGL(ct::mk_coef_kernel, dim3((batch + 63) / 64), dim3(64), 0, (hipStream_t)stream, stats_t, stats_r, decomposition,
                       batch, coef);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_affine3x3_f32_f64(const float *in, const double *coef, double *out, int64_t n_pixels, int batch, void *stream) {
    return ct::affine_impl<float, double>(in, coef, out, n_pixels, batch, stream);
}
int ct_affine3x3_f64_f64(const double *in, const double *coef, double *out, int64_t n_pixels, int batch,
                         void *stream) {
    return ct::affine_impl<double, double>(in, coef, out, n_pixels, batch, stream);
}
int ct_affine3x3_f32_f32(const float *in, const double *coef, float *out, int64_t n_pixels, int batch, void *stream) {
    return ct::affine_impl<float, float>(in, coef, out, n_pixels, batch, stream);
}

}  // extern "C"
