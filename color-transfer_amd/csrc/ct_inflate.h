// ct_inflate.h -- the serial part of csrc/png_decode.hip: a zlib stream (RFC 1950 around RFC 1951) walked symbol by symbol.  Plain
// C++ on plain arrays, like ct_png.h: the kernel hands it LDS and a wave-cooperative source and sink, a host program hands it
// memory, so that it compiles and is checked on the CPU (tests/test_png_decode_host.py runs it under the sanitizers over every
// truncation and every single-bit flip of three streams).
//
// inflate<Source, Sink>(src, len, sink, capacity, tables) returns a CT_INFLATE_* status (include/ct_hip.h).
//   Source: word(pos) -> the four bytes at pos .. pos + 3 of the stream, little endian, ZERO where pos + k >= len.  It is the only
//           way the core reads the input, so nothing outside [src, src + len) is read whatever the bytes say.
//   Sink:   literal(byte), match(length, distance) -- called only with produced + length <= capacity and distance <= produced, so
//           nothing outside the slot is written; writer() -- true where stores into the tables are to be made (the host: always;
//           the kernel: lane 0, all lanes walk the same bits); sync() -- orders those stores before the loads of the other lanes;
//           adler() -- the Adler-32 of what was produced, asked for once after the last block.
// Bounds.  Every loop either consumes at least one bit per iteration and stops once more bits have been consumed than the stream
// has (CT_INFLATE_INPUT_EXHAUSTED; beyond the end the source delivers zeros), or runs over a constant (15 code lengths, 19 / 320
// symbols, the table sizes), or produces at least one byte per iteration and stops at the capacity.
// What zlib refuses is refused here: over-subscribed lengths, incomplete ones unless the literal / length or the distance code is
// ONE code of one bit (inftrees.c's exception; the code-length code gets none), a block without an end-of-block code, HLIT above
// 286 or HDIST above 30, the symbols 286 / 287 and the distances 30 / 31, a distance beyond the start of the output.
#pragma once
#include <stdint.h>

#include "../../include/ct_hip.h"

#if defined(__HIPCC__)
#define CT_INF_HD __host__ __device__ __forceinline__
#else
#define CT_INF_HD inline
#endif

namespace ct {

constexpr int kInfLitBits = 10;                             // primary look-up: literal / length codes up to 10 bits in one step
constexpr int kInfDistBits = 8;                             // and distance codes (and the code-length code, at most 7) up to 8
constexpr int kInfMaxBits = 15;
constexpr int kInfLitSyms = 288, kInfDistSyms = 32, kInfClSyms = 19;

// One decoding table: count[l] codes of l bits, their symbols in canonical order, and the primary look-up `tab`, indexed by the
// next `bits` bits of the stream: symbol | length << 9, or 0 where the code is longer than `bits` (or no code at all).
struct InflateTables {
    uint16_t lit_tab[1 << kInfLitBits];
    uint16_t dist_tab[1 << kInfDistBits];                   // also the code-length code's while a dynamic header is read
    uint16_t lit_sym[kInfLitSyms], dist_sym[kInfDistSyms];
    uint16_t lit_count[kInfMaxBits + 1], dist_count[kInfMaxBits + 1];
    uint16_t next[kInfMaxBits + 2];                         // scratch of build: offsets, then next codes
    uint8_t lens[kInfLitSyms + kInfDistSyms];
    uint8_t cl_lens[kInfClSyms + 1];
};

enum { kInfCodes = 0, kInfLens = 1, kInfDists = 2 };

template <typename Source>
struct InflateBits {
    Source &src;
    long long len, pos;                                     // pos: the next byte to fetch; it may pass len (zeros come back)
    uint64_t hold;
    int nbits;
    CT_INF_HD InflateBits(Source &s, long long n) : src(s), len(n), pos(0), hold(0), nbits(0) {}
    CT_INF_HD void ensure() {                               // at least 33 bits afterwards
        if (nbits <= 32) {
            hold |= (uint64_t)src.word(pos) << nbits;
            pos += 4;
            nbits += 32;
        }
    }
    CT_INF_HD uint32_t peek(int n) const { return (uint32_t)hold & ((1u << n) - 1u); }
    CT_INF_HD void drop(int n) { hold >>= n; nbits -= n; }
    CT_INF_HD uint32_t take(int n) { const uint32_t v = peek(n); drop(n); return v; }
    CT_INF_HD bool over() const { return 8 * pos - nbits > 8 * len; }      // more bits consumed than the stream has
};

// lens[0 .. n) -> count, sym, tab.  Wave-uniform: every lane reads the same values and comes to the same status.
template <typename Sink>
CT_INF_HD int inflate_build(Sink &sink, const uint8_t *lens, int n, uint16_t *count, uint16_t *sym, uint16_t *tab, int bits, int kind,
                            uint16_t *next) {
    if (sink.writer()) {
        for (int l = 0; l <= kInfMaxBits; ++l) count[l] = 0;
        for (int i = 0; i < n; ++i) ++count[lens[i] & 15];
    }
    sink.sync();
    int left = 1, longest = 0;
    for (int l = 1; l <= kInfMaxBits; ++l) {
        const int c = count[l];
        left = 2 * left - c;
        if (left < 0) return CT_INFLATE_OVERSUBSCRIBED;
        if (c) longest = l;
    }
    if (longest == 0) {                                     // no code at all: fine for distances (a block of literals), else incomplete
        if (kind != kInfDists) return CT_INFLATE_INCOMPLETE;
    } else if (left > 0 && (kind == kInfCodes || longest != 1)) {
        return CT_INFLATE_INCOMPLETE;
    }
    if (sink.writer()) {
        next[1] = 0;
        for (int l = 1; l <= kInfMaxBits; ++l) next[l + 1] = (uint16_t)(next[l] + count[l]);
        for (int i = 0; i < n; ++i)
            if (lens[i]) sym[next[lens[i] & 15]++] = (uint16_t)i;
        uint32_t code = 0;                                  // RFC 1951 3.2.2: the first code of each length (count[0] holds the unused symbols: not a length)
        for (int l = 1; l <= kInfMaxBits; ++l) {
            code = (code + (l == 1 ? 0u : (uint32_t)count[l - 1])) << 1;
            next[l] = (uint16_t)code;
        }
        for (int i = 0; i < (1 << bits); ++i) tab[i] = 0;
        for (int i = 0; i < n; ++i) {
            const int l = lens[i] & 15;
            if (!l) continue;
            const uint32_t c = next[l]++;
            if (l > bits) continue;
            uint32_t rev = 0;
            for (int k = 0; k < l; ++k) rev |= ((c >> k) & 1u) << (l - 1 - k);
            for (uint32_t j = rev; j < (1u << bits); j += 1u << l) tab[j] = (uint16_t)(i | (l << 9));
        }
    }
    sink.sync();
    return CT_INFLATE_OK;
}

// the next symbol, or -1 where the coming bits are no code; the caller has called ensure() (>= 33 bits held, zeros past the end)
template <typename Source>
CT_INF_HD int inflate_symbol(InflateBits<Source> &r, const uint16_t *count, const uint16_t *sym, const uint16_t *tab, int bits) {
    const uint32_t e = tab[r.peek(bits)];
    if (e) {
        r.drop((int)(e >> 9));
        return (int)(e & 511u);
    }
    int code = 0, first = 0, index = 0;                     // the canonical walk, one bit per length
    for (int l = 1; l <= kInfMaxBits; ++l) {
        code |= (int)((r.hold >> (l - 1)) & 1u);
        const int c = count[l];
        if (code - c < first) {
            r.drop(l);
            return sym[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

template <typename Source, typename Sink>
CT_INF_HD int inflate(Source &source, long long len, Sink &sink, uint32_t capacity, InflateTables &t) {
    InflateBits<Source> r(source, len);
    r.ensure();
    {
        const uint32_t cmf = r.take(8), flg = r.take(8);
        if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
        if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 32u) || ((cmf << 8) | flg) % 31u) return CT_INFLATE_BAD_HEADER;
    }
    uint32_t produced = 0;
    bool fixed_built = false;
    for (;;) {                                              // a block: at least 3 bits
        r.ensure();
        const uint32_t last = r.take(1), type = r.take(2);
        if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
        if (type == 3u) return CT_INFLATE_BLOCK_TYPE;
        if (type == 0u) {
            r.drop(r.nbits & 7);
            r.ensure();
            const uint32_t n = r.take(16), inv = r.take(16);
            if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
            if (n != (inv ^ 0xffffu)) return CT_INFLATE_STORED_LEN;
            for (uint32_t i = 0; i < n; ++i) {
                r.ensure();
                const uint32_t b = r.take(8);
                if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
                if (produced >= capacity) return CT_INFLATE_OUTPUT_TOO_LARGE;
                sink.literal((uint8_t)b);
                ++produced;
            }
        } else {
            if (type == 1u) {
                if (!fixed_built) {
                    if (sink.writer()) {
                        for (int i = 0; i < kInfLitSyms; ++i) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
                        for (int i = 0; i < kInfDistSyms; ++i) t.lens[kInfLitSyms + i] = 5;
                    }
                    sink.sync();
                    inflate_build(sink, t.lens, kInfLitSyms, t.lit_count, t.lit_sym, t.lit_tab, kInfLitBits, kInfLens, t.next);
                    inflate_build(sink, t.lens + kInfLitSyms, kInfDistSyms, t.dist_count, t.dist_sym, t.dist_tab, kInfDistBits, kInfDists, t.next);
                    fixed_built = true;
                }
            } else {
                fixed_built = false;
                r.ensure();
                const int nlen = (int)r.take(5) + 257, ndist = (int)r.take(5) + 1, ncode = (int)r.take(4) + 4;
                if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
                if (nlen > 286 || ndist > 30) return CT_INFLATE_INVALID_SYMBOL;
                for (int i = 0; i < kInfClSyms; ++i) {
                    uint32_t v = 0;
                    if (i < ncode) {
                        r.ensure();
                        v = r.take(3);
                    }
                    // RFC 1951 3.2.7, the order they are sent in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
                    const int k = i - 4;
                    const int s = i < 3 ? 16 + i : i == 3 ? 0 : (k & 1) ? 7 - (k >> 1) : 8 + (k >> 1);
                    if (sink.writer()) t.cl_lens[s] = (uint8_t)v;
                }
                if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
                sink.sync();
                int rc = inflate_build(sink, t.cl_lens, kInfClSyms, t.dist_count, t.dist_sym, t.dist_tab, kInfDistBits, kInfCodes, t.next);
                if (rc) return rc;
                const int total = nlen + ndist;
                int i = 0, prev = 0;
                while (i < total) {                         // a symbol each: at least one bit
                    r.ensure();
                    const int s = inflate_symbol(r, t.dist_count, t.dist_sym, t.dist_tab, kInfDistBits);
                    if (s < 0) return CT_INFLATE_INVALID_SYMBOL;
                    int rep = 1, v = s;
                    if (s == 16) {
                        if (i == 0) return CT_INFLATE_REPEAT;
                        rep = 3 + (int)r.take(2);
                        v = prev;
                    } else if (s == 17) {
                        rep = 3 + (int)r.take(3);
                        v = 0;
                    } else if (s == 18) {
                        rep = 11 + (int)r.take(7);
                        v = 0;
                    }
                    if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
                    if (i + rep > total) return CT_INFLATE_REPEAT;
                    if (sink.writer())
                        for (int k = 0; k < rep; ++k) t.lens[i + k] = (uint8_t)v;
                    i += rep;
                    prev = v;
                }
                sink.sync();
                if (t.lens[256] == 0) return CT_INFLATE_INCOMPLETE;         // a block that could never end
                rc = inflate_build(sink, t.lens, nlen, t.lit_count, t.lit_sym, t.lit_tab, kInfLitBits, kInfLens, t.next);
                if (rc) return rc;
                rc = inflate_build(sink, t.lens + nlen, ndist, t.dist_count, t.dist_sym, t.dist_tab, kInfDistBits, kInfDists, t.next);
                if (rc) return rc;
            }
            for (;;) {                                      // a symbol each: at least one bit
                r.ensure();
                const int s = inflate_symbol(r, t.lit_count, t.lit_sym, t.lit_tab, kInfLitBits);
                if (s < 0) return r.over() ? CT_INFLATE_INPUT_EXHAUSTED : CT_INFLATE_INVALID_SYMBOL;
                if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
                if (s < 256) {
                    if (produced >= capacity) return CT_INFLATE_OUTPUT_TOO_LARGE;
                    sink.literal((uint8_t)s);
                    ++produced;
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return CT_INFLATE_INVALID_SYMBOL;
                const int ls = s - 257;                     // RFC 1951 3.2.5, as arithmetic: 3 .. 10, then four codes per extra bit, 258
                uint32_t length;
                if (ls < 8) length = 3u + (uint32_t)ls;
                else if (ls == 28) length = 258u;
                else {
                    const int e = (ls >> 2) - 1;
                    length = 3u + ((4u + (uint32_t)(ls & 3)) << e) + r.take(e);
                }
                r.ensure();
                const int ds = inflate_symbol(r, t.dist_count, t.dist_sym, t.dist_tab, kInfDistBits);
                if (ds < 0 || ds > 29) return r.over() ? CT_INFLATE_INPUT_EXHAUSTED : CT_INFLATE_INVALID_SYMBOL;
                uint32_t distance;
                if (ds < 4) distance = 1u + (uint32_t)ds;
                else {
                    const int e = (ds >> 1) - 1;            // 1 .. 13 extra bits, two codes each
                    distance = 1u + ((2u + (uint32_t)(ds & 1)) << e) + r.take(e);
                }
                if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
                if (distance > produced) return CT_INFLATE_DISTANCE;
                if (length > capacity - produced) return CT_INFLATE_OUTPUT_TOO_LARGE;
                sink.match(length, distance);
                produced += length;
            }
        }
        if (last) break;
    }
    if (produced < capacity) return CT_INFLATE_OUTPUT_TOO_SMALL;
    r.drop(r.nbits & 7);
    r.ensure();
    const uint32_t lo = r.take(16), be = lo | (r.take(16) << 16);
    if (r.over()) return CT_INFLATE_INPUT_EXHAUSTED;
    const uint32_t want = (be >> 24) | ((be >> 8) & 0xff00u) | ((be << 8) & 0xff0000u) | (be << 24);
    return sink.adler() == want ? CT_INFLATE_OK : CT_INFLATE_ADLER;
}

// ---- the host's source and sink: plain arrays -----------------------------------------------------------------------------------
struct InflateArraySource {
    const uint8_t *p;
    long long len;
    CT_INF_HD uint32_t word(long long pos) const {
        uint32_t v = 0;
        for (int k = 0; k < 4; ++k)
            if (pos + k < len) v |= (uint32_t)p[pos + k] << (8 * k);
        return v;
    }
};

struct InflateArraySink {
    uint8_t *out;
    uint32_t n;
    CT_INF_HD bool writer() const { return true; }
    CT_INF_HD void sync() const {}
    CT_INF_HD void literal(uint8_t b) { out[n++] = b; }
    CT_INF_HD void match(uint32_t length, uint32_t distance) {
        for (uint32_t i = 0; i < length; ++i, ++n) out[n] = out[n - distance];
    }
    CT_INF_HD uint32_t adler() const {
        uint32_t s1 = 1, s2 = 0;
        for (uint32_t i = 0; i < n; ++i) {
            s1 = (s1 + out[i]) % 65521u;
            s2 = (s2 + s1) % 65521u;
        }
        return (s2 << 16) | s1;
    }
};

}  // namespace ct
