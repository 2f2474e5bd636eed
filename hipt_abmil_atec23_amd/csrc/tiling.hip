// Patch coordinates from tissue contours (wsi_core/WholeSlideImage.py:357-372, 415-506 process_contour / isInContours / isInHoles;
// wsi_core/util_classes.py:53-111 isInContourV1 / V2 / V3_Easy / V3_Hard): which grid positions of a slide become
// patches.  The reference asks cv2.pointPolygonTest up to four times per candidate against the contour and once per hole, one
// Python call per candidate; here a workgroup owns TL_TILE consecutive candidates of ONE contour, one per thread, derives their
// corners from the grid (no candidate array exists) and streams the contour's edges ONCE past all of a candidate's test points,
// then each hole's edges past its hole point.
//
// Integer geometry in DOUBLED coordinates (the hole point pt + ps / 2 may be a half integer): with every doubled coordinate inside
// +-2^30 a difference fits int32 and the edge function
//     d = (p.y - a.y) * (b.x - a.x) - (p.x - a.x) * (b.y - a.y)
// is two 32 x 32 -> 64 bit products: exact.  An edge (a, b) matters to p only when min(a.y, b.y) <= p.y <= max(a.y, b.y); a
// contour is a pixel chain of short edges, so that is rare and d is computed behind that test alone.  There
//     exactly one of a.y <= p.y, b.y <= p.y (the half-open rule)  ->  d == 0: p is on the edge; else the edge's point at height p.y
//                                                                     lies right of p when (d > 0) == (b.y > a.y): parity flips;
//     both or neither                                             ->  p is on the edge when d == 0 and p.x is within [a.x, b.x]
//                                                                     (a horizontal edge at p.y, or p.y touching the upper end).
// Parity and the on-boundary flag are one bit per test point; they start at zero for every polygon (a uniform step: all threads
// of a workgroup walk the same polygon).  Every lane reads the SAME edge at the same time: the vertices of a chunk of
// TL_CHUNK edges are doubled and staged in LDS once per workgroup and read back as broadcasts, one 64-bit read per edge (the edge's
// first vertex is carried over from the previous trip).
// No floating point, no atomics on global memory, no workspace, no inline assembly.
#include "common.h"

namespace {

constexpr int TL_THREADS = HIPT_TILING_TILE;     // one candidate (or point) per thread
constexpr int TL_CHUNK = HIPT_TILING_EDGE_CHUNK; // edges staged per LDS chunk (TL_CHUNK + 1 vertices)
constexpr int TL_DESC = HIPT_TILING_CONTOUR_INTS;
static_assert(TL_THREADS == 256 && TL_CHUNK % TL_THREADS == 0, "whole staging trips");

// vertices [vb, ve) of polygon p, 0 <= p < P, clamped into [0, V] whatever poly_off holds
__device__ __forceinline__ void tl_range(const int* __restrict__ poly_off, int p, int V, int& vb, int& ve) {
    vb = min(max(poly_off[p], 0), V);
    ve = min(max(poly_off[p + 1], vb), V);
}

// Streams the closed polygon verts[vb, ve) past the NP doubled points of this thread: bit k of `par` flips with every edge that
// crosses point k's ray, bit k of `bnd` is set when point k lies on an edge.  Called by every thread of the workgroup with the
// same (vb, ve); it holds barriers.
template <int NP>
__device__ __forceinline__ void tl_walk(const int* __restrict__ verts, int vb, int ve, int2* sv, const int (&px)[NP], const int (&py)[NP],
                                        unsigned& par, unsigned& bnd) {
    const int n = ve - vb;   // vertices = edges (the closing edge included); n = 1: the degenerate edge (v0, v0)
    for (int e0 = 0; e0 < n; e0 += TL_CHUNK) {
        const int m = min(TL_CHUNK, n - e0);   // edges of this chunk: edge k joins staged vertices k and k + 1
        __syncthreads();                       // the previous chunk's (or polygon's) readers are done
        for (int i = threadIdx.x; i <= m; i += TL_THREADS) {
            int idx = e0 + i;
            if (idx >= n) idx -= n;            // (only idx == n: the closing edge's end is vertex 0)
            const size_t g = 2 * ((size_t)vb + idx);
            sv[i] = make_int2((int)((unsigned)verts[g] << 1), (int)((unsigned)verts[g + 1] << 1));
        }
        __syncthreads();
        int2 a = sv[0];
        for (int k = 0; k < m; ++k) {
            const int2 b = sv[k + 1];          // the same address in every lane: a broadcast
            const int ylo = min(a.y, b.y), yhi = max(a.y, b.y);
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                if (py[q] >= ylo && py[q] <= yhi) {
                    const long long d = (long long)(py[q] - a.y) * (long long)(b.x - a.x) - (long long)(px[q] - a.x) * (long long)(b.y - a.y);
                    if ((a.y <= py[q]) != (b.y <= py[q])) {
                        if (d == 0) bnd |= 1u << q;
                        else if ((d > 0) == (b.y > a.y)) par ^= 1u << q;
                    } else if (d == 0 && px[q] >= min(a.x, b.x) && px[q] <= max(a.x, b.x)) {
                        bnd |= 1u << q;
                    }
                }
            }
            a = b;
        }
    }
}

// The primitive: one point per thread.  The workgroup walks, in ascending order, every polygon one of its points names; a thread
// keeps the bits of its own polygon's walk.
__global__ __launch_bounds__(TL_THREADS) void tl_point_kernel(const int* __restrict__ verts, int V, const int* __restrict__ poly_off, int P,
                                                              const int* __restrict__ points2, const int* __restrict__ poly_id, int Q,
                                                              int8_t* __restrict__ out) {
    __shared__ int2 sv[TL_CHUNK + 1];
    __shared__ int s_next;
    const long long i = (long long)blockIdx.x * TL_THREADS + threadIdx.x;
    const bool active = i < Q;
    int id = active ? poly_id[i] : -1;
    if (id >= P) id = -1;
    int px[1] = {0}, py[1] = {0};
    if (active) {
        px[0] = points2[2 * i];
        py[0] = points2[2 * i + 1];
    }
    int result = -1, cur = -1;
    for (;;) {
        if (threadIdx.x == 0) s_next = 0x7fffffff;
        __syncthreads();
        if (id > cur) atomicMin(&s_next, id);   // (LDS)
        __syncthreads();
        const int p = s_next;
        __syncthreads();                        // everyone has read it before the next trip resets it
        if (p == 0x7fffffff) break;             // (uniform)
        int vb, ve;
        tl_range(poly_off, p, V, vb, ve);
        unsigned par = 0, bnd = 0;
        tl_walk<1>(verts, vb, ve, sv, px, py, par, bnd);
        if (id == p) result = bnd ? 0 : (par ? 1 : -1);
        cur = p;
    }
    if (active) out[i] = (int8_t)result;
}

// One tile of TL_THREADS candidates of one contour.  NP = 1: one point against the contour (pt + off); NP = 4: centre -+ shift.
template <int NP>
__global__ __launch_bounds__(TL_THREADS) void tl_tile_kernel(const int* __restrict__ verts, int V, const int* __restrict__ poly_off, int P,
                                                             const int* __restrict__ contours, int C, const int* __restrict__ units,
                                                             int off, int shift, int need_all, int ps, uint8_t* __restrict__ keep,
                                                             long long keep_len) {
    __shared__ int2 sv[TL_CHUNK + 1];
    const int c = units[2 * (size_t)blockIdx.x], first = units[2 * (size_t)blockIdx.x + 1];
    if ((unsigned)c >= (unsigned)C || first < 0) return;   // (uniform, as every return below)
    const int* d = contours + (size_t)c * TL_DESC;
    const int pb = max(d[0], 0), pe = min(d[1], P);
    const int nx = d[6], ny = d[7];
    if (pb >= pe || nx < 1 || ny < 1) return;
    const long long n = (long long)nx * ny;
    if (n > 0x7fffffffLL || first >= n) return;
    const long long i = (long long)first + threadIdx.x;
    const bool active = i < n;
    const int ii = active ? (int)i : first;
    const unsigned ix = (unsigned)(ii / ny), iy = (unsigned)(ii % ny);
    // (unsigned arithmetic: the same bits as int where the caller kept the coordinate bound, no undefined overflow where not)
    const unsigned ptx = (unsigned)d[2] + ix * (unsigned)d[4], pty = (unsigned)d[3] + iy * (unsigned)d[5];

    int px[NP], py[NP];
    const unsigned cx = ptx + (unsigned)off, cy = pty + (unsigned)off;
    if constexpr (NP == 1) {
        px[0] = (int)(cx << 1);
        py[0] = (int)(cy << 1);
    } else {
        const unsigned s = (unsigned)shift;   // the reference's order: (-,-), (+,+), (+,-), (-,+)
        px[0] = (int)((cx - s) << 1);  py[0] = (int)((cy - s) << 1);
        px[1] = (int)((cx + s) << 1);  py[1] = (int)((cy + s) << 1);
        px[2] = (int)((cx + s) << 1);  py[2] = (int)((cy - s) << 1);
        px[3] = (int)((cx - s) << 1);  py[3] = (int)((cy + s) << 1);
    }
    int vb, ve;
    tl_range(poly_off, pb, V, vb, ve);
    unsigned par = 0, bnd = 0;
    tl_walk<NP>(verts, vb, ve, sv, px, py, par, bnd);
    constexpr unsigned FULL = (1u << NP) - 1;
    const unsigned in = (par | bnd) & FULL;
    bool pass = need_all ? in == FULL : in != 0;

    // the holes: a candidate that passed is dropped when pt + ps / 2 (true division) is STRICTLY inside one
    if (pe - pb > 1 && __syncthreads_or(pass && active)) {
        const int hx[1] = {(int)((ptx << 1) + (unsigned)ps)}, hy[1] = {(int)((pty << 1) + (unsigned)ps)};
        for (int p = pb + 1; p < pe; ++p) {
            tl_range(poly_off, p, V, vb, ve);
            unsigned hp = 0, hb = 0;
            tl_walk<1>(verts, vb, ve, sv, hx, hy, hp, hb);
            if (hp && !hb) pass = false;
        }
    }
    if (active) {
        const long long o = (long long)d[8] + i;
        if (o >= 0 && o < keep_len) keep[o] = pass ? 1 : 0;
    }
}

bool tl_aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" int hipt_point_polygon_test(const int32_t* verts, int V, const int32_t* poly_off, int P, const int32_t* points2,
                                       const int32_t* poly_id, int Q, int8_t* out, void* stream) {
    HIPT_CHECK_ARG(V >= 0 && P >= 0 && Q >= 0, "point_polygon_test: V=%d, P=%d, Q=%d", V, P, Q);
    if (Q == 0) return HIPT_OK;
    HIPT_CHECK_ARG(poly_off && points2 && poly_id && out && (verts || V == 0), "point_polygon_test: verts / poly_off / points2 / poly_id / out missing");
    HIPT_CHECK_ARG(tl_aligned4(verts) && tl_aligned4(poly_off) && tl_aligned4(points2) && tl_aligned4(poly_id),
                   "point_polygon_test: the int32 arrays need 4-byte alignment");
    const unsigned grid = (unsigned)(((long long)Q + TL_THREADS - 1) / TL_THREADS);
    hipLaunchKernelGGL(tl_point_kernel, dim3(grid), dim3(TL_THREADS), 0, (hipStream_t)stream, verts, V, poly_off, P, points2, poly_id, Q, out);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

extern "C" int hipt_tile_contours(const int32_t* verts, int V, const int32_t* poly_off, int P, const int32_t* contours, int C,
                                  const int32_t* units, int U, int mode, int ref_patch_size, int shift, uint8_t* keep, int64_t keep_len,
                                  void* stream) {
    HIPT_CHECK_ARG(V >= 0 && P >= 0 && C >= 0 && U >= 0 && keep_len >= 0, "tile_contours: V=%d, P=%d, C=%d, U=%d, keep_len=%lld", V, P, C, U,
                   (long long)keep_len);
    HIPT_CHECK_ARG(mode >= HIPT_TILE_BASIC && mode <= HIPT_TILE_FOUR_PT_HARD, "tile_contours: mode %d is none of HIPT_TILE_BASIC .. HIPT_TILE_FOUR_PT_HARD",
                   mode);
    const int lim = HIPT_TILING_COORD_BOUND / 4;
    if (ref_patch_size < 1 || ref_patch_size >= lim || shift < 0 || shift >= lim) {
        hipt_set_error("tile_contours: ref_patch_size=%d, shift=%d outside the envelope (1 <= ref_patch_size, 0 <= shift, both < %d); "
                       "nothing was launched", ref_patch_size, shift, lim);
        return HIPT_E_UNSUPPORTED;
    }
    if (U == 0) return HIPT_OK;
    HIPT_CHECK_ARG(poly_off && contours && units && keep && (verts || V == 0), "tile_contours: verts / poly_off / contours / units / keep missing");
    HIPT_CHECK_ARG(tl_aligned4(verts) && tl_aligned4(poly_off) && tl_aligned4(contours) && tl_aligned4(units),
                   "tile_contours: the int32 arrays need 4-byte alignment");
    const int off = mode == HIPT_TILE_BASIC ? 0 : ref_patch_size / 2;
    const bool four = mode >= HIPT_TILE_FOUR_PT && shift > 0;
    const int need_all = mode == HIPT_TILE_FOUR_PT_HARD;
    auto k = four ? tl_tile_kernel<4> : tl_tile_kernel<1>;
    hipLaunchKernelGGL(k, dim3((unsigned)U), dim3(TL_THREADS), 0, (hipStream_t)stream, verts, V, poly_off, P, contours, C, units, off, shift,
                       need_all, ref_patch_size, keep, (long long)keep_len);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
