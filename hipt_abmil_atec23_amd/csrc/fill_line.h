// The integer geometry of the contour fill (fill.hip) as closed forms of the row: which columns of row y an edge's
// 8-connected line covers, and where its edge-table entry crosses the row.  Plain C++ (no HIP type), so that a host program can
// include this file and compare the closed forms with the loops they replace (tests/test_seg_mask_host.py does).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define HIPT_FILL_HD __host__ __device__ __forceinline__
#else
#define HIPT_FILL_HD inline
#endif

// The line iterator walks D + 1 points, D = max(|dx|, |dy|), d = min: it starts with err = D - 2 d and at step k = 1 .. D first
// steps the minor axis and adds 2 D if err < 0, then subtracts 2 d and steps the major axis.  Before the test of step k,
// err = D - 2 d k + 2 D m(k - 1), m(k) the minor steps taken so far; as d <= D the minor axis steps at most once per k, and
// induction gives m(k) = ceil((2 d k - D) / (2 D)) = floor((2 d k + D - 1) / (2 D)), m(0) = 0, m(D) = d.  Inverted: m(k) >= m
// (m >= 1) iff k > (2 D m - D) / (2 d), so minor position m is held for k in [floor((2 D m - D) / (2 d)) + 1, floor((2 D (m + 1) -
// D) / (2 d))], from 0 for m = 0 and up to D for m = d.
//
// Columns [*ca, *cb] of the line from (x0, y0) to (x1, y1) on row y; false when the line does not touch the row.  The walk goes
// left to right (the end points are swapped when x1 < x0); x is the major axis on a tie.  |coordinates| <= 2^21: the products fit
// int64 with room.
HIPT_FILL_HD bool hipt_fill_line_run(int x0, int y0, int x1, int y1, int y, int* ca, int* cb) {
    if (x1 < x0) {
        int t = x0; x0 = x1; x1 = t;
        t = y0; y0 = y1; y1 = t;
    }
    const int dx = x1 - x0, dy = y1 - y0, ady = dy < 0 ? -dy : dy;
    const int s = y - y0, m = s < 0 ? -s : s;           // steps along y from the start, if the row lies on the line's side
    if (m > ady || (m != 0 && (s < 0) != (dy < 0))) return false;
    if (dx >= ady) {                                    // x is the major axis: row y holds a run of columns
        const int64_t D = dx, d = ady;
        const int64_t lo = m == 0 ? 0 : (2 * D * m - D) / (2 * d) + 1;
        const int64_t hi = m == ady ? D : (2 * D * (m + 1) - D) / (2 * d);
        *ca = x0 + (int)lo;
        *cb = x0 + (int)hi;
    } else {                                            // y is the major axis: one pixel per row
        const int64_t D = ady, d = dx;
        *ca = *cb = x0 + (int)((2 * d * m + D - 1) / (2 * D));
    }
    return true;
}

// The edge table's entry of the edge between (xa, ya) and (xb, yb), ya != yb: active on the rows min(ya, yb) <= y < max(ya, yb);
// there x_fix = (x_top << 16) + (y - y_top) * slope with slope = ((x_bottom - x_top) << 16) / (y_bottom - y_top), truncated toward
// zero, and the column is (x_fix + 32768) >> 16 (floor).  false when the row is not active.
HIPT_FILL_HD bool hipt_fill_crossing(int xa, int ya, int xb, int yb, int y, int* col) {
    if (ya > yb) {
        int t = xa; xa = xb; xb = t;
        t = ya; ya = yb; yb = t;
    }
    if (y < ya || y >= yb) return false;
    const int64_t slope = ((int64_t)(xb - xa) * 65536) / (yb - ya);
    const int64_t xf = (int64_t)xa * 65536 + (int64_t)(y - ya) * slope;
    *col = (int)((xf + 32768) >> 16);
    return true;
}
