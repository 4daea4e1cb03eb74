// ct_yuv.h -- the exact integer form of the 8-bit Y'CbCr 4:2:0 <-> RGB rule of csrc/yuv.hip.
//
// Both directions are the correctly rounded value (ties to even) of an exact rational expression.  With Kr = kr / D, Kb = kb / D,
// Kg = kg / D (BT.601: 299, 114, 587 over 1000; BT.709: 2126, 722, 7152 over 10000), Yd = Y - Yoff and Cd = C16 - 2048 (C16 = the
// interpolated chroma in sixteenths) the decode is
//   R' = (8 Cs D Yd + (D - kr) Ys Crd) / (8 Ys Cs D)                         B' likewise with kb and Cbd
//   G' = (8 Cs D kg Yd - kb (D - kb) Ys Cbd - kr (D - kr) Ys Crd) / (8 Ys Cs D kg)
// and the encode, on the footprint sums S = sum(w * byte) of total weight Wt (1 for luma),
//   Y  = Yoff + rint(Ys L / (255 D Wt)),  L = kr Sr + kg Sg + kb Sb
//   Cb = 128 + rint(Cs (D Sb - L) / (510 Wt (D - kb))),  Cr likewise with Sr and kr.
// Every numerator stays below 2^55 (the largest, 510 * 8 * 219 * 224 * 10000 * 7152, is 1.4e16).
#pragma once
#include "ct_common.h"

namespace ct {

struct YuvRule {
    // decode: numerators over den_rb (R, B) and den_g (G)
    long long ay_rb, a_r, a_b, den_rb;
    long long ay_g, g_b, g_r, den_g;
    float inv_rb, inv_g;               // 1 / den as float32: the quotient's first guess
    int yoff;
    int we0, we1, wo1, wo2;            // horizontal chroma weights in quarters: even luma column (j - 1, j), odd (j, j + 1)
    // encode
    int kr, kg, kb, d, ys, cs;
    int ymin, ymax, cmin, cmax;
    int den_y;                         // 255 D
    float inv_y;
    long long den_cb, den_cr;          // 510 Wt (D - kb), 510 Wt (D - kr)
    float inv_cb, inv_cr;
    int left;                          // siting: 0 = centre (2x2 box), 1 = left ((1,2,1)/4 x two rows)
};

// false: an unknown enum
inline bool yuv_rule(int matrix, int range, int siting, YuvRule &p) {
    if ((matrix != CT_YUV_BT601 && matrix != CT_YUV_BT709) || (range != CT_YUV_LIMITED && range != CT_YUV_FULL) ||
        (siting != CT_YUV_SITING_CENTER && siting != CT_YUV_SITING_LEFT))
        return false;
    const long long d = matrix == CT_YUV_BT601 ? 1000 : 10000;
    const long long kr = matrix == CT_YUV_BT601 ? 299 : 2126, kb = matrix == CT_YUV_BT601 ? 114 : 722, kg = d - kr - kb;
    const long long ys = range == CT_YUV_LIMITED ? 219 : 255, cs = range == CT_YUV_LIMITED ? 224 : 255;
    p.yoff = range == CT_YUV_LIMITED ? 16 : 0;
    p.ay_rb = 8 * cs * d;        p.a_r = (d - kr) * ys;         p.a_b = (d - kb) * ys;         p.den_rb = 8 * ys * cs * d;
    p.ay_g = 8 * cs * d * kg;    p.g_b = -kb * (d - kb) * ys;   p.g_r = -kr * (d - kr) * ys;   p.den_g = 8 * ys * cs * d * kg;
    p.inv_rb = (float)(1.0 / (double)p.den_rb);
    p.inv_g = (float)(1.0 / (double)p.den_g);
    const bool left = siting == CT_YUV_SITING_LEFT;
    p.we0 = left ? 0 : 1; p.we1 = left ? 4 : 3; p.wo1 = left ? 2 : 3; p.wo2 = left ? 2 : 1;
    p.kr = (int)kr; p.kg = (int)kg; p.kb = (int)kb; p.d = (int)d; p.ys = (int)ys; p.cs = (int)cs;
    p.ymin = p.yoff; p.ymax = range == CT_YUV_LIMITED ? 235 : 255;
    p.cmin = p.yoff; p.cmax = range == CT_YUV_LIMITED ? 240 : 255;
    p.den_y = (int)(255 * d);
    p.inv_y = (float)(1.0 / (double)p.den_y);
    const long long wt = left ? 8 : 4;
    p.den_cb = 510 * wt * (d - kb); p.den_cr = 510 * wt * (d - kr);
    p.inv_cb = (float)(1.0 / (double)p.den_cb);
    p.inv_cr = (float)(1.0 / (double)p.den_cr);
    p.left = left ? 1 : 0;
    return true;
}

// rint(n / den), ties to even, exactly: a float32 guess (|q| <= 256 here, so it is off by less than 1e-4 and at most one step
// from the answer), then the sign of the exact remainder decides.  den > 0; 2 |n| + 2 * 257 den must fit T.
template <typename T>
__host__ __device__ __forceinline__ int rint_div(T n, T den, float inv) {
    int q = (int)rintf((float)n * inv);
    const T r = 2 * n - 2 * (T)q * den;
    if (r > den) ++q;
    else if (r < -den) --q;
    else if (r == den) q += q & 1;
    else if (r == -den) q -= q & 1;
    return q;
}

__host__ __device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

// one decoded channel: rint(255 clamp(n / den, 0, 1))
__host__ __device__ __forceinline__ unsigned int yuv_unit_to_u8(long long n, long long den, float inv) {
    n = n < 0 ? 0 : n > den ? den : n;
    return (unsigned int)rint_div<long long>(255 * n, den, inv);
}

}  // namespace ct
