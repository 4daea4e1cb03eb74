// ct_png.h -- what csrc/png.hip and csrc/png_decode.hip share, and the serial part of the encoder: the Paeth predictor, and Huffman
// code lengths of at most 15 bits from sorted symbol counts.  Plain C++ on plain arrays (the kernel hands it LDS, a host program hands it memory), so that it can be compiled and checked on the CPU.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#if defined(__HIPCC__)
#define CT_PNG_HD __host__ __device__ __forceinline__
#else
#define CT_PNG_HD inline
#endif

namespace ct {

constexpr int kPngMaxBits = 15;                             // RFC 1951: no literal / length code is longer

// PNG filter type 4 (a: left, b: above, c: above left), of the encoder's filter choice and the decoder's unfilter
CT_PNG_HD unsigned int paeth(unsigned int a, unsigned int b, unsigned int c) {
    const int p = (int)a + (int)b - (int)c;
    const int pa = abs(p - (int)a), pb = abs(p - (int)b), pc = abs(p - (int)c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);         // ties: a, then b, then c
}

// a[0 .. n): the counts of the n >= 2 used symbols in ascending order.  On return a[i] is the code length of the i-th of them
// (the rarest symbol first: lengths descend), count[l] the number of codes of l bits (l = 0 .. 15, count[0] = 0) and
// first_code[l] the canonical code of the first symbol of l bits (RFC 1951 3.2.2).
//   1. The in-place minimum-redundancy construction of Moffat and Katajainen (1995): three passes over the sorted array -- pair
//      the two cheapest of {unused leaves, finished internal nodes} and leave a parent index behind; turn parent indices into
//      internal depths from the root down; hand every depth's free slots to the leaves that remain.  Sums stay below 2^32: the
//      caller's chunk holds fewer than 2^31 bytes.
//   2. Depths above 15 are cut to 15, which oversubscribes the code; then, until the Kraft sum is exactly 1 again, one 15-bit code
//      is dropped and the deepest shorter code is pushed one level down to share its slot with it (each step returns 2^-15).  The
//      lengths go back to the symbols longest to rarest.  This is the widely used heuristic of the public-domain deflate
//      encoders, not the optimal package-merge: it costs a fraction of a per cent on skewed histograms and nothing on others.
CT_PNG_HD void png_code_lengths(uint32_t *a, int n, uint32_t *count, uint32_t *first_code) {
    for (int l = 0; l <= kPngMaxBits; ++l) count[l] = 0;
    {
        a[0] += a[1];
        int root = 0, leaf = 2;
        for (int next = 1; next < n - 1; ++next) {
            if (leaf >= n || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = (uint32_t)next; } else a[next] = a[leaf++];
            if (leaf >= n || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = (uint32_t)next; } else a[next] += a[leaf++];
        }
        a[n - 2] = 0;
        for (int next = n - 3; next >= 0; --next) a[next] = a[a[next]] + 1;
        int avail = 1, used = 0, depth = 0, next = n - 1;
        root = n - 2;
        while (avail > 0) {
            while (root >= 0 && (int)a[root] == depth) { ++used; --root; }
            while (avail > used) { a[next--] = (uint32_t)depth; --avail; }
            avail = 2 * used;
            ++depth;
            used = 0;
        }
    }
    for (int i = 0; i < n; ++i) ++count[a[i] < (uint32_t)kPngMaxBits ? a[i] : kPngMaxBits];
    uint32_t kraft = 0;                                     // in units of 2^-15
    for (int l = 1; l <= kPngMaxBits; ++l) kraft += count[l] << (kPngMaxBits - l);
    while (kraft > (1u << kPngMaxBits)) {
        --count[kPngMaxBits];
        for (int l = kPngMaxBits - 1; l > 0; --l)
            if (count[l]) { --count[l]; count[l + 1] += 2; break; }
        --kraft;
    }
    int i = 0;
    for (int l = kPngMaxBits; l > 0; --l)
        for (uint32_t k = 0; k < count[l]; ++k) a[i++] = (uint32_t)l;
    uint32_t code = 0;
    first_code[0] = 0;
    for (int l = 1; l <= kPngMaxBits; ++l) {
        code = (code + count[l - 1]) << 1;
        first_code[l] = code;
    }
}

}  // namespace ct
