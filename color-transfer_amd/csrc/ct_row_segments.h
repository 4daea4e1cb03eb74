// ct_row_segments.h -- how the strip kernels (conv_ws.hip, conv_wino.hip, conv_wino4.hip) cut an image into row segments.
// Integers only, no HIP types: tests/test_row_segments.py compiles it into a plain host program.
#pragma once

namespace ct {

struct RowSegments {
    int n_seg, seg;   // segments per image, rows per segment (the last one may be shorter)
};

// The split with the fewest row steps of the busiest workgroup.  A band is one row segment of one image (and output group);
// XCD p of the eight owns the bands p, p + 8, .. and its 32 workgroups sweep them strip after strip, so the busiest workgroup
// runs ceil(bands_per_xcd * n_strips / 32) items of steps_of_segment(seg) steps each (the caller's count: rows + halo).
// Segments have at least 16 rows; even_rows rounds them up to even (the Winograd kernels step two rows at a time).
template <typename Steps>
inline RowSegments pick_row_segments(int H, long long imgs, int n_strips, bool even_rows, Steps steps_of_segment) {
    RowSegments r = {1, H};
    long long best = -1;
    for (int ns = 1; ns <= (H + 15) / 16; ++ns) {
        int sg = (H + ns - 1) / ns;
        if (even_rows) sg += sg & 1;
        const int ns_eff = (H + sg - 1) / sg;
        const long long bands_per_xcd = (imgs * ns_eff + 7) / 8;
        const long long rounds = (bands_per_xcd * n_strips + 31) / 32;
        const long long cost = rounds * steps_of_segment(sg);
        if (best < 0 || cost < best) { best = cost; r.n_seg = ns_eff; r.seg = sg; }
    }
    return r;
}

}  // namespace ct
