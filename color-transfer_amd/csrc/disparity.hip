// disparity.hip -- the disparity of a parallax attention (pasmnet/utils.py:55-105, regress_disp): the expected matching column
// disp_ini[i] = i - sum_j att[i][j] j, then the occluded pixels (valid == 0) filled along their image row.
//
// The reference fills with two loops of 1x3 partial convolutions that run until no pixel changes anywhere in the batch.  Along a
// row that is exactly this scan: an invalid pixel k steps right of the last valid pixel p left of it holds disp_ini[p] divided k
// times by the float32 (1 + 1e-4) (filter [1,1,0]); a pixel left of the row's first valid pixel f holds disp_ini[f] divided
// (f - x) times (filter [0,1,1]); a row without a valid pixel is 0.  Each division is the correctly rounded float32 one, in the
// reference's order, so the fill is bitwise the reference's whenever disp_ini is.
//
//   disp_fill_kernel   : one wave per image row.  The mask becomes a bit row in LDS (ballots); the lane that owns the first pixel
//                        of a hole walks that hole alone (one lane per hole, not per pixel: W divisions per row at worst), reading
//                        the mask 32 pixels at a time from the bit row and disp_ini only at the hole's source pixel.
//   regress_index_kernel: one wave per query row of a materialised att [B,H,W,W]: 16-byte loads, a fixed summation order.
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ct_common.h"
#include "ct_attention16.h"

namespace ct {

static constexpr int kDispMaxW = 32768;          // the bit row of one image row: 4 KB of LDS

// (1 + 1e-4) as the reference's float32 tensor arithmetic forms it (utils.py:91,100: valid_mask_1 + 1e-4 with valid_mask_1 = 1)
__device__ __forceinline__ float fill_div(float x) {
    const float d = 1.0f + 1e-4f;
    return x / d;
}

// din, out: [rows][w] (may be the same buffer: only valid pixels are read, only invalid ones rewritten with other values);
// valid: [rows][w], 0 / 1.  blockDim 64, one block per row, dynamic LDS: 4 * nwords bytes with nwords = 2 * ceil(w / 64).
__global__ __launch_bounds__(64) void disp_fill_kernel(const float *din, const float *__restrict__ valid, float *out, int w) {
    extern __shared__ unsigned int bits[];
    const int lane = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * w;
    const float *vr = valid + base;
    const float *dr = din + base;
    float *orow = out + base;
    int first = -1;                               // first valid pixel of the row (wave-uniform)
    for (int c0 = 0; c0 < w; c0 += 64) {
        const int x = c0 + lane;
        const unsigned long long b = __ballot(x < w && vr[x] > 0.5f);
        if (lane == 0) { bits[c0 >> 5] = (unsigned int)b; bits[(c0 >> 5) + 1] = (unsigned int)(b >> 32); }
        if (first < 0 && b != 0ull) first = c0 + __builtin_ctzll(b);
    }
    __syncthreads();
    auto bit = [&](int x) -> unsigned int { return (bits[x >> 5] >> (x & 31)) & 1u; };
    for (int c0 = 0; c0 < w; c0 += 64) {
        const int x = c0 + lane;
        if (x >= w) break;
        if (bit(x)) {
            orow[x] = dr[x];
        } else if (first < 0) {
            orow[x] = 0.0f;                       // no valid pixel in the row: both loops leave it 0
        } else if (x == 0) {
            // the hole at the start of the row (second loop, filter [0,1,1]): right to left from the first valid pixel
            float val = dr[first];
            for (int y = first - 1; y >= 0; --y) {
                val = fill_div(val);
                orow[y] = val;
            }
        } else if (bit(x - 1)) {
            // a hole right of a valid pixel (first loop, filter [1,1,0]): left to right until the next valid pixel or the row's end;
            // the bit row says how far the hole runs 32 pixels at a time (bits past w are 0)
            float val = dr[x - 1];
            int y = x;
            while (y < w) {
                const unsigned int word = bits[y >> 5] >> (y & 31);
                int run = word ? __builtin_ctz(word) : 32 - (y & 31);
                if (run > w - y) run = w - y;
                for (int t = 0; t < run; ++t) {
                    val = fill_div(val);
                    orow[y + t] = val;
                }
                y += run;
                if (word) break;                  // the next valid pixel
            }
        }
    }
}

// disp[q] = (q % w) - sum_j att[q][j] j for the query rows q of att [rows * w][w]; one wave per query row, four per block.  Lane l
// sums its elements in index order, then a fixed butterfly over the lanes: deterministic.
__global__ __launch_bounds__(256) void regress_index_kernel(const float *__restrict__ att, float *__restrict__ disp, long long nq, int w) {
    const int lane = threadIdx.x & 63;
    const long long qrow = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (qrow >= nq) return;
    const float *a = att + (size_t)qrow * w;
    // scalar head up to 16-byte alignment, float4 body, scalar tail
    const int head = min(w, (int)((4 - ((reinterpret_cast<uintptr_t>(a) >> 2) & 3)) & 3));
    const int nb4 = (w - head) >> 2;
    float acc = 0.f;
    if (lane < head) acc = a[lane] * (float)lane;
    const float4 *a4 = reinterpret_cast<const float4 *>(a + head);
    int j4 = lane;
    for (; j4 + 192 < nb4; j4 += 256) {           // four independent 16-byte loads in flight per lane
        const float4 t0 = a4[j4], t1 = a4[j4 + 64], t2 = a4[j4 + 128], t3 = a4[j4 + 192];
        const float4 t[4] = {t0, t1, t2, t3};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float j = (float)(head + 4 * (j4 + 64 * u));
            acc = fmaf(t[u].x, j, acc);
            acc = fmaf(t[u].y, j + 1.0f, acc);
            acc = fmaf(t[u].z, j + 2.0f, acc);
            acc = fmaf(t[u].w, j + 3.0f, acc);
        }
    }
    for (; j4 < nb4; j4 += 64) {
        const float4 t = a4[j4];
        const float j = (float)(head + 4 * j4);
        acc = fmaf(t.x, j, acc);
        acc = fmaf(t.y, j + 1.0f, acc);
        acc = fmaf(t.z, j + 2.0f, acc);
        acc = fmaf(t.w, j + 3.0f, acc);
    }
    const int tail0 = head + 4 * nb4;
    if (tail0 + lane < w) acc = fmaf(a[tail0 + lane], (float)(tail0 + lane), acc);
    acc = wave_all_sum(acc);
    if (lane == 0) disp[qrow] = (float)(int)(qrow % w) - acc;
}

static int disp_fill_launch(const float *din, const float *valid, float *out, long long rows, int w, hipStream_t s) {
    const int nwords = 2 * ((w + 63) / 64);
    hipLaunchKernelGGL(disp_fill_kernel, dim3((unsigned)rows), dim3(64), nwords * 4, s, din, valid, out, w);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

// sizes shared by the two fill entries: n images of h rows of w pixels
static int disp_sizes(int n, int h, int w) {
    if (n < 0 || h < 0 || w < 0) return CT_E_BADARG;
    if (w > kDispMaxW || (long long)n * h > 0x7fffffffLL) return CT_E_BADARG;
    return CT_OK;
}

}  // namespace ct

// ---- C ABI (include/ct_hip.h) ---------------------------------------------------------------------------------------------
extern "C" {

int ct_attention_rows64_disp_f32(const float *q, const float *k, const float *v, float *out, float *disp_ini, int batch, int len,
                                 float scale, void *stream) {
    if (batch < 0 || len < 1) return CT_E_BADARG;
    if (batch == 0) return CT_OK;
    if (!q || !k || !disp_ini || (v && !out)) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k)) & 15) return CT_E_ALIGN;
    if (v && (reinterpret_cast<uintptr_t>(v) | reinterpret_cast<uintptr_t>(out)) & 15) return CT_E_ALIGN;
    if (ct::attention16_enabled()) {
        ct::attention16_rows64_disp(q, k, v, out, disp_ini, batch, len, scale, (hipStream_t)stream);
        CT_CHECK_LAUNCH();
        return CT_OK;
    }
    // CT_HIP_ATT16=0: `out` from the three-piece bf16 kernel, exactly as ct_attention_rows64_f32 writes it; the index from the
    // index-only pass of the two-piece kernel
    if (v) {
        const int rc = ct_attention_rows64_f32(q, k, v, out, nullptr, batch, len, scale, stream);
        if (rc != CT_OK) return rc;
    }
    ct::attention16_rows64_disp(q, k, nullptr, nullptr, disp_ini, batch, len, scale, (hipStream_t)stream);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_pam_disp_fill_f32(const float *disp_ini, const float *valid, float *disp, int n, int h, int w, void *stream) {
    const int rc = ct::disp_sizes(n, h, w);
    if (rc != CT_OK) return rc;
    if ((long long)n * h * w == 0) return CT_OK;
    if (!disp_ini || !valid || !disp) return CT_E_BADARG;
    return ct::disp_fill_launch(disp_ini, valid, disp, (long long)n * h, w, (hipStream_t)stream);
}

int ct_pam_regress_disp_f32(const float *att, const float *valid, float *disp, int n, int h, int w, void *stream) {
    const int rc = ct::disp_sizes(n, h, w);
    if (rc != CT_OK) return rc;
    if ((long long)n * h * w == 0) return CT_OK;
    if (!att || !valid || !disp) return CT_E_BADARG;
    const long long nq = (long long)n * h * w;
    if ((nq + 3) / 4 > 0x7fffffffLL) return CT_E_BADARG;
    hipLaunchKernelGGL(ct::regress_index_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, (hipStream_t)stream, att, disp, nq, w);
    CT_CHECK_LAUNCH();
    // in place: the fill reads disp_ini only at valid pixels and rewrites only invalid ones
    return ct::disp_fill_launch(disp, valid, disp, (long long)n * h, w, (hipStream_t)stream);
}

}  // extern "C"
