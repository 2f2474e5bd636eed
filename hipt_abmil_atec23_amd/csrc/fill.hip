// The tissue mask of WholeSlideImage.get_seg_mask (wsi_core/WholeSlideImage.py:741-757): contours filled one after
// the other as cv2.drawContours(..., thickness=-1) fills them -- every edge's 8-connected line plus an even-odd scan fill from a
// 16.16 fixed-point edge table -- in ONE launch, without a workspace and without atomics on global memory.
//
// The shape of tiling.hip turned by ninety degrees: a workgroup owns FL_ROWS canvas rows (one per wave) and up to FL_COLS columns of
// them, and walks the collections in draw order.  A collection is what one drawContours call fills: one contour (value 1), or all
// holes of one contour (value 0).  For a collection whose y range meets the band every lane takes edges (both vertices straight from
// global memory, scaled where they are loaded); for each row of the band the edge touches it
//   - marks the columns of the line's pixels on that row in an LDS bit set (a closed form of the row: fill_line.h), and
//   - if the edge's table entry is active on the row, adds 1 to the row's LDS counter at the column it crosses (closed form too); a
//     crossing left of the workgroup's columns goes to the row's carry counter, one right of them nowhere.
// Then each wave makes one pass over its row, 64 columns at a time: a column is covered when the number of crossings at or left of
// it is odd, or one lies on it, or a line pixel does.  (The scan fill pairs the crossings in sorted order and fills both ends: a
// pair [a, b] is exactly the columns with an odd count at or left of them, plus b.)  Covered columns take the collection's value in
// the row's state bits; counters and line bits are cleared on the way.  Integer adds and ORs commute: the result does not depend on
// the order in which lanes arrive.  After the last collection the state bits are written out as bytes, zeros included.
//
// The counters are 32 bits wide and a collection has at most HIPT_FILL_MAX_POINTS edges, so none can wrap.  Every scaled coordinate
// is clamped to +-HIPT_FILL_COORD_BOUND where it is loaded: the host refuses a call whose declared coordinate bound would exceed
// that, and a caller that declares less than it hands over still gets no access out of bounds (every LDS and global index below is
// derived from a column already tested against the workgroup's columns, and a row of the band below h).
// No floating point but the scaling's one float64 product per coordinate; no inline assembly; vector stores only.
#include "common.h"
#include "fill_line.h"

namespace {

constexpr int FL_THREADS = 256;
constexpr int FL_ROWS = FL_THREADS / 64;          // rows per workgroup: one per wave in the covering pass
constexpr int FL_COLS = HIPT_FILL_MAX_COLS;       // columns per pass
constexpr int FL_WORDS = FL_COLS / 32;
constexpr int FL_COLL = HIPT_FILL_COLLECTION_INTS;
static_assert(FL_COLS % 64 == 0, "the covering pass takes 64 columns at a time");
static_assert(FL_ROWS * (FL_COLS * 4 + FL_WORDS * 4 + FL_COLS / 8 + 4) <= 64 * 1024, "static LDS");

// double(p) * scale converted toward zero, offset added; clamped to the envelope (NaN and infinities included)
__device__ __forceinline__ int fl_scale(int p, double s, int off) {
    double v = (double)p * s;
    v = fmin(fmax(v, -2.0 * HIPT_FILL_COORD_BOUND), 2.0 * HIPT_FILL_COORD_BOUND);
    const int c = (int)v + off;
    return min(max(c, -HIPT_FILL_COORD_BOUND), HIPT_FILL_COORD_BOUND);
}

__device__ __forceinline__ long long fl_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(FL_THREADS) void fl_fill_kernel(const int* __restrict__ points, long long P, const long long* __restrict__ poly_off,
                                                             int n_polys, const int* __restrict__ colls, int n_colls, double sx, double sy,
                                                             int offx, int offy, int h, int w, int cols, uint8_t* __restrict__ out) {
    __shared__ unsigned s_cnt[FL_ROWS][FL_COLS];            // crossings per column, this collection
    __shared__ unsigned s_line[FL_ROWS][FL_WORDS];          // line pixels, this collection
    __shared__ unsigned long long s_state[FL_ROWS][FL_COLS / 64];
    __shared__ unsigned s_carry[FL_ROWS];                   // crossings left of the first column

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int y_first = (int)blockIdx.x * FL_ROWS, y_last = min(y_first + FL_ROWS, h) - 1;
    const int c_first = (int)blockIdx.y * cols, c_end = min(c_first + cols, w);   // columns [c_first, c_end)
    const int nblk = (c_end - c_first + 63) >> 6;

    for (int i = tid; i < FL_ROWS * FL_COLS; i += FL_THREADS) (&s_cnt[0][0])[i] = 0;
    for (int i = tid; i < FL_ROWS * FL_WORDS; i += FL_THREADS) (&s_line[0][0])[i] = 0;
    for (int i = tid; i < FL_ROWS * (FL_COLS / 64); i += FL_THREADS) (&s_state[0][0])[i] = 0;
    if (tid < FL_ROWS) s_carry[tid] = 0;
    __syncthreads();

    for (int c = 0; c < n_colls; ++c) {
        const int* d = colls + (size_t)c * FL_COLL;
        const int pb = min(max(d[0], 0), n_polys), pe = min(max(d[1], pb), n_polys);
        const int value = d[2];
        if (d[4] < y_first || d[3] > y_last || pb >= pe) continue;   // (uniform: the whole workgroup skips)

        for (int p = pb; p < pe; ++p) {
            const long long vb = fl_clamp(poly_off[p], 0, P), ve = fl_clamp(poly_off[p + 1], vb, P);
            const long long n = ve - vb;       // vertices = edges, the closing edge included; n = 1: the edge (v0, v0)
            for (long long i = tid; i < n; i += FL_THREADS) {
                const long long j = i == 0 ? n - 1 : i - 1;
                const int2 a = *(const int2*)(points + 2 * (vb + j)), b = *(const int2*)(points + 2 * (vb + i));
                const int ax = fl_scale(a.x, sx, offx), ay = fl_scale(a.y, sy, offy);
                const int bx = fl_scale(b.x, sx, offx), by = fl_scale(b.y, sy, offy);
                const int r0 = max(min(ay, by), y_first), r1 = min(max(ay, by), y_last);
                for (int y = r0; y <= r1; ++y) {
                    const int r = y - y_first;
                    int ca, cb, col;
                    if (hipt_fill_line_run(ax, ay, bx, by, y, &ca, &cb)) {
                        ca = max(ca, c_first) - c_first;
                        cb = min(cb, c_end - 1) - c_first;
                        for (int wd = ca >> 5; wd <= (cb >> 5) && ca <= cb; ++wd) {
                            const int lo = max(ca - (wd << 5), 0), hi = min(cb - (wd << 5), 31);
                            atomicOr(&s_line[r][wd], (0xffffffffu >> (31 - hi)) & (0xffffffffu << lo));
                        }
                    }
                    if (hipt_fill_crossing(ax, ay, bx, by, y, &col)) {
                        if (col < c_first) atomicAdd(&s_carry[r], 1u);
                        else if (col < c_end) atomicAdd(&s_cnt[r][col - c_first], 1u);
                    }
                }
            }
        }
        __syncthreads();

        // the covering pass: wave `wave` owns row y_first + wave (a row beyond h received nothing and writes nothing)
        if (y_first + wave <= y_last) {
            unsigned long long carry = (s_carry[wave] & 1u) ? ~0ull : 0ull;
            for (int b = 0; b < nblk; ++b) {
                const unsigned cnt = s_cnt[wave][(b << 6) + lane];
                unsigned long long par = __ballot(cnt & 1u);
                const unsigned long long on = __ballot(cnt != 0u);
                par ^= par << 1;  par ^= par << 2;  par ^= par << 4;   // bit x = parity of the counts of columns 0 .. x of the block
                par ^= par << 8;  par ^= par << 16; par ^= par << 32;
                par ^= carry;
                carry = (par >> 63) ? ~0ull : 0ull;
                const unsigned long long line = (unsigned long long)s_line[wave][2 * b] | ((unsigned long long)s_line[wave][2 * b + 1] << 32);
                const unsigned long long cover = par | on | line;
                if (cnt != 0u) s_cnt[wave][(b << 6) + lane] = 0;
                if (lane == 0) {
                    const unsigned long long s = s_state[wave][b];
                    s_state[wave][b] = value ? (s | cover) : (s & ~cover);
                    s_line[wave][2 * b] = 0;
                    s_line[wave][2 * b + 1] = 0;
                }
            }
            if (lane == 0) s_carry[wave] = 0;
        }
        __syncthreads();
    }

    if (y_first + wave <= y_last) {
        uint8_t* row = out + (size_t)(y_first + wave) * (size_t)w + (size_t)c_first;
        for (int b = 0; b < nblk; ++b) {
            const unsigned long long s = s_state[wave][b];
            const int x = (b << 6) + lane;
            if (x < c_end - c_first) row[x] = (uint8_t)((s >> lane) & 1ull);
        }
    }
}

}  // namespace

extern "C" int hipt_fill_contours(const int32_t* points, int64_t n_points, const int64_t* poly_off, int n_polys, const int32_t* collections,
                                  int n_collections, double scale_x, double scale_y, int off_x, int off_y, int coord_bound, int h, int w,
                                  int max_cols, uint8_t* mask, void* stream) {
    HIPT_CHECK_ARG(n_points >= 0 && n_polys >= 0 && n_collections >= 0, "fill_contours: n_points=%lld, n_polys=%d, n_collections=%d",
                   (long long)n_points, n_polys, n_collections);
    HIPT_CHECK_ARG(h >= 1 && w >= 1, "fill_contours: a canvas of %d x %d", h, w);
    HIPT_CHECK_ARG(coord_bound >= 0, "fill_contours: coord_bound=%d (the largest |coordinate| among the points)", coord_bound);
    HIPT_CHECK_ARG(scale_x == scale_x && scale_y == scale_y, "fill_contours: the scale is NaN");
    HIPT_CHECK_ARG(max_cols == 0 || (max_cols >= 64 && max_cols <= HIPT_FILL_MAX_COLS && max_cols % 64 == 0),
                   "fill_contours: max_cols=%d is neither 0 nor a multiple of 64 in 64 .. %d", max_cols, HIPT_FILL_MAX_COLS);
    HIPT_CHECK_ARG(mask && poly_off && (points || n_points == 0) && (collections || n_collections == 0),
                   "fill_contours: points / poly_off / collections / mask missing");
    HIPT_CHECK_ARG(((uintptr_t)points & 7) == 0 && ((uintptr_t)poly_off & 7) == 0 && ((uintptr_t)collections & 3) == 0,
                   "fill_contours: points and poly_off need 8-byte alignment, collections 4-byte");
    const double reach = (double)coord_bound * fmax(fabs(scale_x), fabs(scale_y)) + fmax(fabs((double)off_x), fabs((double)off_y));
    if (h > HIPT_FILL_MAX_DIM || w > HIPT_FILL_MAX_DIM || n_points > HIPT_FILL_MAX_POINTS || !(reach <= (double)HIPT_FILL_COORD_BOUND)) {
        hipt_set_error("fill_contours: a canvas of %d x %d, %lld points, coordinates up to %d scaled by (%g, %g) and moved by (%d, %d): outside "
                       "the envelope (h, w <= %d; at most %d points; scaled and moved coordinates within +-%d); nothing was launched",
                       h, w, (long long)n_points, coord_bound, scale_x, scale_y, off_x, off_y, HIPT_FILL_MAX_DIM, HIPT_FILL_MAX_POINTS,
                       HIPT_FILL_COORD_BOUND);
        return HIPT_E_UNSUPPORTED;
    }
    const int cols = max_cols ? max_cols : HIPT_FILL_MAX_COLS;
    const dim3 grid((unsigned)((h + FL_ROWS - 1) / FL_ROWS), (unsigned)((w + cols - 1) / cols));
    hipLaunchKernelGGL(fl_fill_kernel, grid, dim3(FL_THREADS), 0, (hipStream_t)stream, (const int*)points, (long long)n_points,
                       (const long long*)poly_off, n_polys, (const int*)collections, n_collections, scale_x, scale_y, off_x, off_y, h, w, cols,
                       mask);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
