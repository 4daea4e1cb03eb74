// png_decode.hip -- the compressed half of a PNG file, read: ct_png_inflate_u8 turns zlib streams into filtered rows and
// ct_png_unfilter_u8 those into planar uint8 frames.  The container (signature, chunks, CRC-32, IHDR) is host work: utils/png.py.
//
// Inflate.  ONE wave (a workgroup of 64 lanes) per stream.  Huffman decoding is serial in the bits, so all lanes walk the same
// bits through csrc/ct_inflate.h (wave-uniform: it costs what one lane would) and share what is not serial:
//   (a) the input: a 1 KB stage in LDS, refilled 64 bytes per instruction (byte loads: a stream starts at any byte, and nothing
//       outside [start, end) is read; beyond the end the stage holds zeros);
//   (b) match copies: out[p + i] = out[p - D + (i mod D)] for i < L, 64 bytes per step, which is also right for D < L;
//   (c) the output: the last 32 KB live in LDS as a ring (the deflate window), every full 4 KB of it goes out coalesced (dwords
//       where the slot lies on 4 bytes, bytes otherwise) with its part of the Adler-32 sums.
// Matches read the RING, never the global memory this wave has just stored to: the order of a store and a later load of the same
// bytes by another lane would need a wait for the store and a cache write-back / invalidate in between; LDS needs neither.
// LDS operations of one wave are executed in the order they were issued, so a ds_write of lane 0 (a literal, a table entry) is seen
// by the next ds_read of any lane of the wave; wave_sync() keeps the compiler from reordering across it and emits no instruction.
// A match writes ring cells p .. p + L - 1, which alias positions 32 KB back: at most 4095 + 258 bytes are not yet written out,
// all within the last 32 KB, and a source at D = 32768 shares its cell with its destination (read, then written, by one lane).
// LDS: 32768 ring + 1024 stage + 3.8 KB tables = 37.5 KB per workgroup: four per CU (160 KB).
//
// Unfilter.  One wave per stream.  Average and Paeth are serial along x and depend on the row above, so a band of 64 rows runs on
// its anti-diagonal: lane k takes row y0 + k one pixel behind lane k - 1 and gets the pixel above from it with one __shfl_up of the
// packed pixel (the one above-left is last step's).  Sub and Up ride the same wavefront.  The last row of a band is handed to the
// next band in LDS (lane 63 writes pixel x at step x + 63, lane 0 of the next band reads it at step x: in-order LDS again, no
// global store-then-load).  32 KB of LDS for rows up to CT_PNG_MAX_WIDTH pixels.
#include "ct_common.h"
#include "ct_inflate.h"
#include "ct_png.h"        // paeth

namespace ct {

constexpr int kInfRing = 32768, kInfStage = 1024, kInfFlush = 4096;
constexpr unsigned int kInfAdlerMod = 65521u;

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct InflateStageSource {
    const uint8_t *__restrict__ src;                        // the stream's first byte
    long long len;
    uint8_t *stage;                                         // LDS [kInfStage + 4]
    long long base;                                         // the stage holds bytes base .. base + kInfStage - 1; -1: nothing yet
    unsigned int lane;
    __device__ __forceinline__ uint32_t word(long long pos) {
        if (base < 0 || pos < base || pos + 4 > base + kInfStage) {         // wave-uniform
            wave_sync();
            base = pos;
            for (int k = (int)lane; k < kInfStage; k += kWave) {
                const long long at = pos + k;
                stage[k] = at < len ? src[at] : (uint8_t)0;
            }
            wave_sync();
        }
        const uint8_t *p = stage + (int)(pos - base);
        return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    }
};

struct InflateRingSink {
    uint8_t *ring;                                          // LDS [kInfRing], 4-byte aligned
    uint8_t *__restrict__ dst;                              // the slot's first byte
    uint32_t capacity, p, flushed;                          // p: bytes produced; flushed: bytes written out, a multiple of kInfFlush
    unsigned int lane;
    bool dwords;                                            // the slot lies on 4 bytes
    unsigned long long sum, wsum;                           // this lane's part of sum d_i and of sum d_i ((capacity - i) mod 65521)
    uint32_t value;                                         // what adler() returned, for the status record

    __device__ __forceinline__ bool writer() const { return lane == 0; }
    __device__ __forceinline__ void sync() const { wave_sync(); }

    // bytes flushed .. flushed + n - 1 (n <= kInfFlush, all produced, flushed + n <= capacity) leave the ring
    __device__ __forceinline__ void flush(uint32_t n) {
        wave_sync();
        for (uint32_t k = 4u * lane; k < n; k += 4u * kWave) {
            const uint32_t at = flushed + k;
            const uint32_t w = *reinterpret_cast<const uint32_t *>(ring + (at & (kInfRing - 1)));
            const uint32_t m = n - k < 4u ? n - k : 4u;
            for (uint32_t j = 0; j < m; ++j) {
                const uint32_t d = (w >> (8u * j)) & 255u;
                sum += d;
                wsum += (unsigned long long)d * ((capacity - (at + j)) % kInfAdlerMod);
            }
            if (dwords && m == 4u) *reinterpret_cast<uint32_t *>(dst + at) = w;
            else
                for (uint32_t j = 0; j < m; ++j) dst[at + j] = (uint8_t)(w >> (8u * j));
        }
        flushed += n;
    }
    __device__ __forceinline__ void literal(uint8_t b) {
        if (lane == 0) ring[p & (kInfRing - 1)] = b;
        ++p;
        if (p - flushed >= (uint32_t)kInfFlush) flush(kInfFlush);
    }
    __device__ __forceinline__ void match(uint32_t length, uint32_t distance) {
        wave_sync();
        for (uint32_t i = lane; i < length; i += kWave) {
            const uint32_t s = distance >= length ? i : i % distance;
            const uint8_t v = ring[(p - distance + s) & (kInfRing - 1)];
            ring[(p + i) & (kInfRing - 1)] = v;
        }
        p += length;
        if (p - flushed >= (uint32_t)kInfFlush) flush(kInfFlush);
    }
    // after the last block, with p == capacity: the rest goes out and the sums become the Adler-32
    __device__ __forceinline__ uint32_t adler() {
        while (p - flushed > 0u) flush(p - flushed < (uint32_t)kInfFlush ? p - flushed : (uint32_t)kInfFlush);
        unsigned long long a = sum, b = wsum % kInfAdlerMod;
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, kWave);
            b += __shfl_xor(b, off, kWave);
        }
        const uint32_t s1 = (uint32_t)((1ull + a) % kInfAdlerMod);
        const uint32_t s2 = (uint32_t)((capacity % kInfAdlerMod + b) % kInfAdlerMod);
        return value = (s2 << 16) | s1;
    }
};

__global__ __launch_bounds__(kWave) void png_inflate_kernel(const uint8_t *__restrict__ src, const long long *__restrict__ src_offsets,
                                                            uint8_t *__restrict__ dst, const long long *__restrict__ dst_offsets,
                                                            int *__restrict__ status, unsigned int *__restrict__ adler_out) {
    __shared__ __attribute__((aligned(16))) uint8_t ring[kInfRing];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kInfStage + 16];
    __shared__ InflateTables tables;
    const unsigned int lane = threadIdx.x;
    const long long i = blockIdx.x;
    const long long s0 = src_offsets[i], s1 = src_offsets[i + 1], d0 = dst_offsets[i], d1 = dst_offsets[i + 1];
    int rc;
    uint32_t adler = 0u;
    if (s0 < 0 || s1 < s0 || d0 < 0 || d1 < d0) rc = CT_INFLATE_INPUT_EXHAUSTED;       // offsets that are none
    else if (d1 - d0 > 0x7fffffffll) rc = CT_INFLATE_OUTPUT_TOO_LARGE;
    else {
        InflateStageSource source{src + s0, s1 - s0, stage, -1ll, lane};
        InflateRingSink sink{ring, dst + d0, (uint32_t)(d1 - d0), 0u, 0u, lane, (reinterpret_cast<uintptr_t>(dst + d0) & 3u) == 0u, 0ull, 0ull, 0u};
        rc = inflate(source, s1 - s0, sink, sink.capacity, tables);
        adler = sink.value;
    }
    if (lane == 0) {
        status[i] = rc;
        adler_out[i] = adler;
    }
}

// ---- unfilter -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned int unfilter_byte(unsigned int x, unsigned int a, unsigned int b, unsigned int c, int type) {
    const unsigned int pred = type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : type == 4 ? paeth(a, b, c) : 0u;
    return (x + pred) & 255u;
}

__global__ __launch_bounds__(kWave) void png_unfilter_kernel(const uint8_t *__restrict__ filtered, const long long *__restrict__ offsets,
                                                             const int *__restrict__ dims, uint8_t *__restrict__ dst,
                                                             const long long *__restrict__ dst_offsets, int *__restrict__ status) {
    __shared__ unsigned int above[CT_PNG_MAX_WIDTH];        // the last row of the band before, packed r | g << 8 | b << 16
    const int lane = (int)threadIdx.x;
    const long long i = blockIdx.x;
    if (status[i] != CT_INFLATE_OK) return;                 // wave-uniform: the stream did not inflate
    const int h = dims[2 * i], w = dims[2 * i + 1];
    const long long f0 = offsets[i], f1 = offsets[i + 1], d0 = dst_offsets[i], d1 = dst_offsets[i + 1];
    if (h < 1 || w < 1 || w > CT_PNG_MAX_WIDTH || f0 < 0 || d0 < 0 || f1 - f0 != (long long)h * (1ll + 3ll * w) || d1 - d0 != 3ll * h * w) {
        if (lane == 0) status[i] = CT_INFLATE_DIMS;
        return;
    }
    const long long row_bytes = 1ll + 3ll * w, plane = (long long)h * w;
    const uint8_t *__restrict__ in = filtered + f0;
    uint8_t *__restrict__ out = dst + d0;
    bool bad = false;
    for (int y0 = 0; y0 < h; y0 += kWave) {
        const int rows = min(kWave, h - y0);
        const int y = y0 + lane;
        const bool have_row = lane < rows;
        const uint8_t *__restrict__ row = in + (long long)(have_row ? y : y0) * row_bytes;
        int type = have_row ? (int)row[0] : 0;
        if (type > 4) { bad = true; type = 0; }
        const bool hand_over = rows == kWave && y0 + kWave < h;     // lane 63's row is the next band's row above
        unsigned int left = 0u, up_left = 0u, mine = 0u;            // mine: this lane's pixel of the step before
        wave_sync();
        for (int t = 0; t < w + rows - 1; ++t) {
            const int x = t - lane;
            const bool on = have_row && x >= 0 && x < w;
            unsigned int up = __shfl_up(mine, 1, kWave);            // the pixel above: what lane k - 1 made one step ago
            if (lane == 0) up = (y0 > 0 && on) ? above[x] : 0u;
            if (on) {
                const uint8_t *__restrict__ px = row + 1 + 3ll * x;
                unsigned int v = 0u;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const unsigned int sh = 8u * c;
                    const unsigned int r = unfilter_byte(px[c], (left >> sh) & 255u, (up >> sh) & 255u, (up_left >> sh) & 255u, type);
                    out[c * plane + (long long)y * w + x] = (uint8_t)r;
                    v |= r << sh;
                }
                if (hand_over && lane == kWave - 1) above[x] = v;
                left = v;
                up_left = up;
                mine = v;
            }
        }
        wave_sync();
    }
    if (__any(bad) && lane == 0) status[i] = CT_INFLATE_FILTER;
}

}  // namespace ct

extern "C" {

int ct_png_inflate_u8(const uint8_t *src, const long long *src_offsets, int n, uint8_t *dst, const long long *dst_offsets, int *status,
                      unsigned int *adler_out, void *stream) {
    if (!src || !src_offsets || !dst || !dst_offsets || !status || !adler_out || n < 1) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(src_offsets) | reinterpret_cast<uintptr_t>(dst_offsets)) % sizeof(long long)) return CT_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(status) | reinterpret_cast<uintptr_t>(adler_out)) % sizeof(int)) return CT_E_ALIGN;
    hipLaunchKernelGGL(ct::png_inflate_kernel, dim3((unsigned)n), dim3(ct::kWave), 0, (hipStream_t)stream, src, src_offsets, dst, dst_offsets, status,
                       adler_out);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

int ct_png_unfilter_u8(const uint8_t *filtered, const long long *offsets, const int *dims, int n, uint8_t *dst, const long long *dst_offsets,
                       int *status, void *stream) {
    if (!filtered || !offsets || !dims || !dst || !dst_offsets || !status || n < 1) return CT_E_BADARG;
    if ((reinterpret_cast<uintptr_t>(offsets) | reinterpret_cast<uintptr_t>(dst_offsets)) % sizeof(long long)) return CT_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(status) | reinterpret_cast<uintptr_t>(dims)) % sizeof(int)) return CT_E_ALIGN;
    hipLaunchKernelGGL(ct::png_unfilter_kernel, dim3((unsigned)n), dim3(ct::kWave), 0, (hipStream_t)stream, filtered, offsets, dims, dst, dst_offsets,
                       status);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
