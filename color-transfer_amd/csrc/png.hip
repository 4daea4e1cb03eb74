// png.hip -- the compressed half of a PNG file on gfx950: ct_png_deflate_u8 turns uint8 HWC frames into deflate streams (PNG row
// filters, RFC 1951 dynamic-Huffman blocks of literals only, RFC 1950 Adler-32 parts).  The container (signature, IHDR, the zlib
// header, CRC-32) is host work: utils/png.py.
//
// A frame is cut into chunks of rows_per_chunk rows; ONE workgroup of 256 threads encodes a chunk and depends on nothing but the
// frame's own bytes (the row above a chunk's first row is read raw from the input), so the bytes of a frame do not depend on the
// batch, its position in it or the grid.  Three passes over the chunk's rows, which stay in L2 (92 KB at 1080p x 16 rows):
//   1. one WAVE per row: the five filters' sums of absolute values (bytes taken as signed), the smallest wins (the lowest type on a
//      tie); then the row again with that filter: histogram (LDS atomics on 16 bank-staggered copies, so that the one hot symbol
//      of a smooth frame meets 4-way instead of 64-way conflicts) and the two Adler-32 sums;
//   2. code lengths: the 257 counts ranked by 257 x 257 comparisons (all threads), the minimum-redundancy lengths limited to 15 bits
//      by ONE thread (ct_png.h: ~3 short loops over <= 257 LDS words), canonical codes by all threads;
//   3. the bit stream, tile by tile (2048 symbols): a thread codes 8 consecutive symbols into <= 120 bits of registers, a block scan
//      of the bit counts gives its position, LDS atomic ORs assemble the tile (<= 3.8 KB), whole dwords go out with aligned vector
//      stores and the last partial dword is carried into the next tile.  A slot that does not start on 4 bytes is handled by
//      shifting the whole stream by its misalignment: every store but the first and last few bytes is an aligned dword.
// Nothing of a chunk is staged whole: LDS per workgroup is 27 KB whatever the frame's width (5 workgroups per CU), and the third
// pass recomputes the filter instead of keeping 92 KB of filtered bytes, which would leave one workgroup per CU.
//
// Stream of a chunk (Huffman form), LSB first as RFC 1951 packs it:
//   3 bits   BFINAL = 0, BTYPE = 2
//   14 bits  HLIT = 0 (257 literal / length codes), HDIST = 0 (one distance code), HCLEN = 15 (19 code-length code lengths)
//   57 bits  the code-length code: 0 bits for 16, 17, 18 and 4 bits for each of 0 .. 15 -- a complete fixed code, symbol L is L
//   1032 b   258 code lengths of 4 bits each, no repeat symbols; the last one, the distance code, is 0 = "no distances"
//   payload  one code per filtered byte, then end-of-block
//   3 bits   BFINAL = 0, BTYPE = 0, padding to the next byte, then 00 00 FF FF: the empty stored block of Z_SYNC_FLUSH
// kPngHeaderBits = 1106.  When that is not smaller than stored blocks (5 bytes of header per <= 65 535 bytes, already byte
// aligned: no empty block after them), the chunk is stored; so a chunk never exceeds filtered + 5 ceil(filtered / 65535) bytes.
#include "ct_common.h"
#include "ct_png.h"

namespace ct {

constexpr int kPngSyms = 257;                               // 256 literals + end-of-block
constexpr int kPngHistCopies = 16;
constexpr int kPngMaxRows = 1024;                           // rows per chunk: one filter-type byte each in LDS
constexpr int kPngMaxWidth = 1 << 20;                       // keeps a row's sum of absolute values inside 32 bits
constexpr int kPngPerThread = 8;
constexpr int kPngTile = kBlock * kPngPerThread;
constexpr int kPngBufWords = kPngTile * kPngMaxBits / 32 + 4;       // a tile's bits + the carried partial dword + the trailer
constexpr int kPngHeaderBits = 17 + 19 * 3 + 258 * 4;
constexpr unsigned int kAdlerMod = 65521u;
constexpr unsigned int kStoredMax = 65535u;

// the neighbours of byte `col` of a row of 3-byte pixels: left, up, up-left; zero outside the frame (prev == nullptr: row 0)
__device__ __forceinline__ void neighbours(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev, unsigned int col, unsigned int &a,
                                           unsigned int &b, unsigned int &c) {
    a = col >= 3 ? cur[col - 3] : 0u;
    b = prev ? prev[col] : 0u;
    c = (prev && col >= 3) ? prev[col - 3] : 0u;
}

__device__ __forceinline__ unsigned int filtered(const uint8_t *__restrict__ cur, const uint8_t *__restrict__ prev, unsigned int col, int type) {
    const unsigned int x = cur[col];
    if (type == 0) return x;
    unsigned int a, b, c;
    neighbours(cur, prev, col, a, b, c);
    const unsigned int pred = type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth(a, b, c);
    return (x - pred) & 255u;
}

__device__ __forceinline__ unsigned int abs_signed(unsigned int v) { return v < 128u ? v : 256u - v; }

// v (any width up to 64 bits) ORed into the LDS bit buffer at bit q
__device__ __forceinline__ void or_bits(unsigned int *buf, unsigned int q, unsigned long long v) {
    if (!v) return;
    const unsigned int w = q >> 5, sh = q & 31u;
    const unsigned int lo = (unsigned int)v, hi = (unsigned int)(v >> 32);
    const unsigned int w0 = lo << sh;
    const unsigned int w1 = sh ? (lo >> (32 - sh)) | (hi << sh) : hi;
    const unsigned int w2 = sh ? hi >> (32 - sh) : 0u;
    if (w0) atomicOr(buf + w, w0);
    if (w1) atomicOr(buf + w + 1, w1);
    if (w2) atomicOr(buf + w + 2, w2);
}

// frames [n][h][w][3]; slot (frame, chunk) of `streams` at (frame * chunks + chunk) * cap; sizes [n][chunks]; adler [n][chunks][2]
__global__ __launch_bounds__(kBlock) void png_deflate_kernel(const uint8_t *__restrict__ frames, int h, int w, int rpc, int chunks, long long cap,
                                                             uint8_t *__restrict__ streams, int *__restrict__ sizes, unsigned int *__restrict__ adler) {
    __shared__ unsigned int hist[kPngHistCopies * kPngSyms];
    __shared__ unsigned int freq[kPngSyms];
    __shared__ uint32_t sorted_count[kPngSyms];             // ascending counts of the used symbols, then their code lengths
    __shared__ unsigned int sorted_sym[kPngSyms];
    __shared__ unsigned int len_of[kPngSyms];
    __shared__ unsigned int code_of[kPngSyms];              // bit-reversed code | length << 16
    __shared__ uint32_t count[kPngMaxBits + 1], first_code[kPngMaxBits + 1];
    __shared__ unsigned int buf[kPngBufWords];
    __shared__ unsigned long long sums[3];                  // sum of the filtered bytes, the weighted sum of Adler's s2, payload bits
    __shared__ unsigned int wave_bits[kBlock / kWave];
    __shared__ unsigned int n_used;
    __shared__ uint8_t ftype[kPngMaxRows];

    const unsigned int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid >> 6;
    const long long slot_index = blockIdx.x;
    const int frame = (int)(slot_index / chunks), chunk = (int)(slot_index - (long long)frame * chunks);
    const int row0 = chunk * rpc;
    const int rows = min(rpc, h - row0);
    const unsigned int rb = 3u * (unsigned int)w, sl = rb + 1u;             // a row's bytes, and with its filter-type byte
    const unsigned int total = (unsigned int)rows * sl;                     // < 2^31: checked by the entry
    const uint8_t *__restrict__ image = frames + (long long)frame * h * rb;

    for (unsigned int i = tid; i < kPngHistCopies * kPngSyms; i += kBlock) hist[i] = 0u;
    for (unsigned int i = tid; i < kPngSyms; i += kBlock) len_of[i] = 0u;
    if (tid < 3) sums[tid] = 0ull;
    if (tid == 0) n_used = 0u;
    __syncthreads();

    // ---- pass 1: filter choice, histogram, Adler sums; one wave per row ---------------------------------------------------------
    unsigned int *my_hist = hist + (tid & (kPngHistCopies - 1)) * kPngSyms;
    unsigned long long sum_d = 0ull, sum_wd = 0ull;
    for (int r = (int)wid; r < rows; r += kBlock / kWave) {
        const uint8_t *cur = image + (long long)(row0 + r) * rb;
        const uint8_t *prev = row0 + r > 0 ? cur - rb : nullptr;
        unsigned int s0 = 0u, s1 = 0u, s2 = 0u, s3 = 0u, s4 = 0u;
        for (unsigned int col = lane; col < rb; col += kWave) {
            const unsigned int x = cur[col];
            unsigned int a, b, c;
            neighbours(cur, prev, col, a, b, c);
            s0 += abs_signed(x);
            s1 += abs_signed((x - a) & 255u);
            s2 += abs_signed((x - b) & 255u);
            s3 += abs_signed((x - ((a + b) >> 1)) & 255u);
            s4 += abs_signed((x - paeth(a, b, c)) & 255u);
        }
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1) {
            s0 += __shfl_xor(s0, off, kWave);
            s1 += __shfl_xor(s1, off, kWave);
            s2 += __shfl_xor(s2, off, kWave);
            s3 += __shfl_xor(s3, off, kWave);
            s4 += __shfl_xor(s4, off, kWave);
        }
        int type = 0;
        unsigned int best = s0;
        if (s1 < best) { best = s1; type = 1; }
        if (s2 < best) { best = s2; type = 2; }
        if (s3 < best) { best = s3; type = 3; }
        if (s4 < best) { best = s4; type = 4; }
        if (lane == 0) ftype[r] = (uint8_t)type;
        const unsigned int base = (unsigned int)r * sl;
        for (unsigned int sc = lane; sc < sl; sc += kWave) {
            const unsigned int v = sc == 0 ? (unsigned int)type : filtered(cur, prev, sc - 1, type);
            atomicAdd(my_hist + v, 1u);
            sum_d += v;
            sum_wd += (unsigned long long)v * ((total - (base + sc)) % kAdlerMod);
        }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
        sum_d += __shfl_xor(sum_d, off, kWave);
        sum_wd += __shfl_xor(sum_wd, off, kWave);
    }
    if (lane == 0) {
        atomicAdd(&sums[0], sum_d);
        atomicAdd(&sums[1], sum_wd % kAdlerMod);
    }
    __syncthreads();

    // ---- pass 2: code lengths and codes ------------------------------------------------------------------------------------------
    for (unsigned int s = tid; s < kPngSyms; s += kBlock) {
        unsigned int f = 0u;
        if (s == 256u) f = 1u;
        else
            for (int k = 0; k < kPngHistCopies; ++k) f += hist[k * kPngSyms + s];
        freq[s] = f;
    }
    __syncthreads();
    for (unsigned int s = tid; s < kPngSyms; s += kBlock) {
        const unsigned int f = freq[s];
        if (f) {
            unsigned int rank = 0u;
            for (unsigned int j = 0; j < kPngSyms; ++j) {
                const unsigned int fj = freq[j];
                rank += (fj != 0u && (fj < f || (fj == f && j < s))) ? 1u : 0u;
            }
            sorted_count[rank] = f;
            sorted_sym[rank] = s;
            atomicAdd(&n_used, 1u);
        }
    }
    __syncthreads();
    const unsigned int used = n_used;                       // >= 2: a filter-type byte and end-of-block
    if (tid == 0) png_code_lengths(sorted_count, (int)used, count, first_code);
    __syncthreads();
    for (unsigned int i = tid; i < used; i += kBlock) len_of[sorted_sym[i]] = sorted_count[i];
    __syncthreads();
    for (unsigned int s = tid; s < kPngSyms; s += kBlock) {
        const unsigned int len = len_of[s];
        unsigned int packed = 0u;
        if (len) {
            unsigned int code = first_code[len];
            for (unsigned int j = 0; j < s; ++j) code += len_of[j] == len ? 1u : 0u;
            packed = (__brev(code) >> (32 - len)) | (len << 16);
            atomicAdd(&sums[2], (unsigned long long)freq[s] * len);
        }
        code_of[s] = packed;
    }
    __syncthreads();

    const unsigned long long huff_bits = (unsigned long long)kPngHeaderBits + sums[2] + 3ull;
    const unsigned long long huff_bytes = (huff_bits + 7ull) / 8ull + 4ull;
    const unsigned int n_stored = (total + kStoredMax - 1u) / kStoredMax;
    const unsigned long long stored_bytes = (unsigned long long)total + 5ull * n_stored;
    uint8_t *slot = streams + slot_index * cap;
    if (tid == 0) {
        adler[2 * slot_index] = (unsigned int)((1ull + sums[0]) % kAdlerMod);
        adler[2 * slot_index + 1] = (unsigned int)((total % kAdlerMod + sums[1]) % kAdlerMod);
    }

    // ---- pass 3, stored form: byte-aligned, every position known -------------------------------------------------------------------
    if (huff_bytes >= stored_bytes) {                       // uniform over the workgroup
        for (unsigned int b = tid; b < n_stored; b += kBlock) {
            const unsigned int len = min(kStoredMax, total - b * kStoredMax);
            uint8_t *p = slot + (unsigned long long)b * (kStoredMax + 5u);
            p[0] = 0;                                       // BFINAL = 0, BTYPE = 0, padding
            p[1] = (uint8_t)len;
            p[2] = (uint8_t)(len >> 8);
            p[3] = (uint8_t)~len;
            p[4] = (uint8_t)(~len >> 8);
        }
        for (unsigned int s = tid; s < total; s += kBlock) {
            const unsigned int r = s / sl, sc = s - r * sl;
            const uint8_t *cur = image + (long long)(row0 + (int)r) * rb;
            const uint8_t *prev = row0 + (int)r > 0 ? cur - rb : nullptr;
            const int type = ftype[r];
            slot[(unsigned long long)s + 5ull * (s / kStoredMax + 1u)] = (uint8_t)(sc == 0 ? (unsigned int)type : filtered(cur, prev, sc - 1, type));
        }
        if (tid == 0) sizes[slot_index] = (int)stored_bytes;
        return;
    }

    // ---- pass 3, Huffman form ----------------------------------------------------------------------------------------------------
    // The stream is addressed in bits from `vbase`, the slot's address rounded down to 4 bytes: it starts at bit 8 * mis.  buf holds
    // the stream's dwords from word_base on; `limit` (the end of the slot) bounds every store whatever the arithmetic above did.
    const unsigned int mis = (unsigned int)(reinterpret_cast<uintptr_t>(slot) & 3u);
    uint8_t *vbase = slot - mis;
    const unsigned long long limit = (unsigned long long)mis + (unsigned long long)cap;
    unsigned long long pos = 8ull * mis;                    // the next free bit
    unsigned long long word_base = 0ull;
    for (unsigned int i = tid; i < kPngBufWords; i += kBlock) buf[i] = 0u;
    __syncthreads();

    // whole dwords below new_pos go out, the partial one moves to buf[0]
    auto advance = [&](unsigned long long new_pos) {
        __syncthreads();                                    // every OR of this step has landed
        const unsigned int n_words = (unsigned int)((new_pos >> 5) - word_base);
        for (unsigned int i = tid; i < n_words; i += kBlock) {
            const unsigned long long byte = (word_base + i) * 4ull;
            const unsigned int v = buf[i];
            if (byte >= mis) {
                if (byte + 4ull <= limit) *reinterpret_cast<unsigned int *>(vbase + byte) = v;
            } else {                                        // the slot's first dword when it starts inside one
                for (unsigned int k = mis; k < 4u; ++k)
                    if (byte + k < limit) vbase[byte + k] = (uint8_t)(v >> (8u * k));
            }
        }
        const unsigned int carry = buf[n_words];
        __syncthreads();
        for (unsigned int i = tid; i < kPngBufWords; i += kBlock) buf[i] = i == 0 ? carry : 0u;
        __syncthreads();
        word_base += n_words;
        pos = new_pos;
    };

    // block header and the 258 code lengths
    {
        const unsigned int q = (unsigned int)pos;
        if (tid == 0) or_bits(buf, q, 4ull | (15ull << 13));                // BTYPE = 2 at bit 1, HCLEN = 15 at bit 13
        if (tid < 16) or_bits(buf, q + 26u + 3u * tid, 4ull);               // code-length code lengths of the symbols 0 .. 15, in RFC order
        for (unsigned int s = tid; s < kPngSyms; s += kBlock) or_bits(buf, q + 74u + 4u * s, __brev(len_of[s]) >> 28);
    }
    advance(pos + kPngHeaderBits);

    const unsigned int n_tokens = total + 1u;               // the filtered bytes and end-of-block
    for (unsigned int tile = 0; tile < n_tokens; tile += kPngTile) {
        unsigned long long lo = 0ull, hi = 0ull;
        unsigned int nbits = 0u;
        const unsigned int t0 = tile + tid * kPngPerThread;
        if (t0 < n_tokens) {
            unsigned int r = t0 / sl, sc = t0 - r * sl;
#pragma unroll
            for (int k = 0; k < kPngPerThread; ++k) {
                const unsigned int t = t0 + k;
                if (t < n_tokens) {
                    unsigned int sym = 256u;
                    if (t < total) {
                        const uint8_t *cur = image + (long long)(row0 + (int)r) * rb;
                        const uint8_t *prev = row0 + (int)r > 0 ? cur - rb : nullptr;
                        const int type = ftype[r];
                        sym = sc == 0 ? (unsigned int)type : filtered(cur, prev, sc - 1, type);
                    }
                    const unsigned int packed = code_of[sym];
                    const unsigned long long code = packed & 0xffffu;
                    const unsigned int len = packed >> 16;
                    if (nbits < 64u) {
                        lo |= code << nbits;
                        if (nbits + len > 64u) hi |= code >> (64u - nbits);
                    } else {
                        hi |= code << (nbits - 64u);
                    }
                    nbits += len;
                    if (++sc == sl) { sc = 0u; ++r; }
                }
            }
        }
        // block scan of nbits
        unsigned int incl = nbits;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const unsigned int up = __shfl_up(incl, off, kWave);
            if ((int)lane >= off) incl += up;
        }
        if (lane == kWave - 1) wave_bits[wid] = incl;
        __syncthreads();
        unsigned int before = 0u, tile_bits = 0u;
#pragma unroll
        for (unsigned int k = 0; k < kBlock / kWave; ++k) {
            const unsigned int wb = wave_bits[k];
            if (k < wid) before += wb;
            tile_bits += wb;
        }
        const unsigned int q = (unsigned int)(pos - word_base * 32ull) + before + incl - nbits;
        or_bits(buf, q, lo);
        or_bits(buf, q + 64u, hi);
        advance(pos + tile_bits);                           // its first barrier also separates the reads of wave_bits from the next tile's writes
    }

    // the empty stored block: 3 zero bits, zero padding to a byte, 00 00 FF FF
    pos = (pos + 3ull + 7ull) & ~7ull;
    if (tid == 0) or_bits(buf, (unsigned int)(pos - word_base * 32ull), 0xffff0000ull);
    pos += 32ull;
    __syncthreads();
    const unsigned long long end_byte = pos >> 3;
    for (unsigned long long byte = word_base * 4ull + tid; byte < end_byte; byte += kBlock) {
        const unsigned int i = (unsigned int)(byte - word_base * 4ull);
        if (byte >= mis && byte < limit) vbase[byte] = (uint8_t)(buf[i >> 2] >> (8u * (i & 3u)));
    }
    if (tid == 0) sizes[slot_index] = (int)(end_byte - mis);
}

}  // namespace ct

extern "C" {

long long ct_png_slot_capacity(int h, int w, int rows_per_chunk) {
    if (h < 1 || w < 1 || w > ct::kPngMaxWidth || rows_per_chunk < 1 || rows_per_chunk > ct::kPngMaxRows) return 0;
    const long long rows = rows_per_chunk < h ? rows_per_chunk : h;
    const long long filtered = rows * (3ll * w + 1);
    const long long cap = filtered + 5 * ((filtered + 65534) / 65535) + 5;
    return cap <= 0x7fffffffll ? cap : 0;
}

int ct_png_deflate_u8(const uint8_t *frames, int n, int h, int w, int rows_per_chunk, uint8_t *streams, long long capacity, int *sizes,
                      unsigned int *adler, void *stream) {
    if (!frames || !streams || !sizes || !adler || n < 1 || h < 1 || w < 1 || rows_per_chunk < 1) return CT_E_BADARG;
    const long long need = ct_png_slot_capacity(h, w, rows_per_chunk);
    if (need == 0) return CT_E_BADARG;                      // rows_per_chunk above 1024, a row above 2^20 pixels or a chunk of 2 GB
    if (capacity < need || capacity > 0x7fffffffll) return CT_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(sizes) | reinterpret_cast<uintptr_t>(adler)) % sizeof(int)) return CT_E_ALIGN;
    const int rpc = rows_per_chunk < h ? rows_per_chunk : h;
    const long long chunks = ((long long)h + rpc - 1) / rpc;
    if ((long long)n * chunks > 0x7fffffffll) return CT_E_BADARG;
    hipLaunchKernelGGL(ct::png_deflate_kernel, dim3((unsigned)(n * chunks)), dim3(ct::kBlock), 0, (hipStream_t)stream, frames, h, w, rpc, (int)chunks,
                       capacity, streams, sizes, adler);
    CT_CHECK_LAUNCH();
    return CT_OK;
}

}  // extern "C"
