// cv2.findContours(mask, RETR_CCOMP, CHAIN_APPROX_NONE) on the device: Suzuki-Abe border following (8-connected foreground,
// 4-connected background) without a sequential walk; DESIGN.md 29, include/hipt_abmil.h.  All of it works on the PADDED plane
// [h + 2, w + 2] (a one-pixel frame of zeros), pixels and labels are indices into it, directions are OpenCV's chain codes
// (0 = east, then counter-clockwise on screen: NE, N, NW, W, SW, S, SE).
//   label    ct_init / ct_merge / ct_flatten: one union-find over the plane, foreground 8-connected and background 4-connected in the
//            same array (a pixel is one or the other).  A node only ever points at a smaller index of its own component and only
//            roots are linked (atomicMin on global memory, retried with what it returns), so every root ends as its component's
//            MINIMUM index whatever the schedule: the raster-first pixel.  A foreground root is the start of an outer border, a
//            background root other than the frame's (index 0) is the first pixel of a hole, whose border starts one pixel west.
//   compact  ct_scan / ct_compact: border pixels (foreground with a background 4-neighbour) and roots, numbered in raster order by a
//            block count, one scan of the counts and a block-local scan (no atomics: the numbering is the same in every run).
//   link     ct_links: a state is (border pixel, code of the direction to the PREVIOUS point).  Its successor is the first foreground
//            neighbour counter-clockwise after that direction; its predecessor the first clockwise, both read off the 3 x 3
//            neighbourhoods, every state at once.  A border is a cycle of states; the state (start, direction of the border's last
//            point) is its head, and the cycle is cut there: the head points at itself with weight 0, every other state at its
//            predecessor with weight 1.  A state whose successor is found without passing a background pixel lies on no border (it
//            circles three mutually adjacent pixels; every state that looks into the interior is one) and points at itself.
//   rank     ct_rank: pointer doubling over (pointer, weight) pairs, ping-pong between two arrays; a pass that changes nothing ends
//            the ranking (a flag on the device: the later launches return at once), so ceil(log2(longest border)) + 2 passes do the
//            work.  Then a state's pointer is its border's head and its weight its distance from the start.
//   table    ct_table: per border, in raster order of the roots: start, kind, length (the rank of the head's predecessor, plus one) and
//            the start of the outer border it lies on.  The caller reads this back, orders the borders and hands back the offsets;
//   emit     ct_emit scatters points[offset[border] + rank] = (x, y).
// Integers only; the only atomics are the union-find's atomicMin, whose outcome (the minimum) does not depend on arrival order, and
// relaxed loads / stores of flags.  No kernel walks a border.  No allocation and no host synchronisation in here: the ONE read-back
// between hipt_contours_trace and hipt_contours_emit is the caller's, which is why the pair cannot be captured into a graph.
#include "common.h"
#include "workspace.h"

namespace {

constexpr int CT_THREADS = 256;
constexpr int CT_SCAN_THREADS = 1024;
constexpr int CT_MAX_GRID = 4096;          // grid-stride kernels: enough workgroups to fill the device, however few states there are
constexpr int CT_HDR_INTS = 64, CT_ACT = 8;   // hdr[0] border pixels, hdr[1] borders; hdr[CT_ACT + k]: pass k has work
constexpr long long CT_MAX_PLANE = HIPT_CONTOURS_MAX_PLANE;
constexpr int CT_MAX_BPIX = HIPT_CONTOURS_MAX_BORDER_PIXELS, CT_MAX_BORDERS = HIPT_CONTOURS_MAX_BORDERS;

struct Geom {
    int H, W, PW, n;        // n = (H + 2) * (W + 2) <= 2^27
    int cap_b, cap_c;       // room for border pixels / borders
    int passes;             // launches of ct_rank: ceil(log2(8 cap_b)) + 2
};

__host__ __device__ inline int ct_min(int a, int b) { return a < b ? a : b; }

Geom make_geom(int h, int w) {
    Geom g = {};
    g.H = h, g.W = w, g.PW = w + 2;
    g.n = (int)((long long)(h + 2) * (long long)(w + 2));
    const long long hw = (long long)h * (long long)w;
    g.cap_b = (int)(hw < CT_MAX_BPIX ? hw : CT_MAX_BPIX);
    g.cap_c = (int)(hw < CT_MAX_BORDERS ? hw : CT_MAX_BORDERS);
    int bits = 0;
    while ((1LL << bits) < 8LL * g.cap_b) ++bits;
    g.passes = bits + 2;
    return g;
}

bool plane_ok(int h, int w) { return h >= 1 && w >= 1 && (long long)(h + 2) * (long long)(w + 2) <= CT_MAX_PLANE; }

// offset of chain code c in the padded plane
__device__ __forceinline__ int ct_off(int c, int PW) {
    // dx = {1, 1, 0, -1, -1, -1, 0, 1}, dy = {0, -1, -1, -1, 0, 1, 1, 1}
    const int x = (c == 0 || c == 1 || c == 7) ? 1 : ((c >= 3 && c <= 5) ? -1 : 0);
    const int y = (c >= 1 && c <= 3) ? -1 : ((c >= 5) ? 1 : 0);
    return y * PW + x;
}

// bit c: the neighbour of p in direction c is foreground.  p is a foreground pixel, so all eight lie inside the padded plane.
__device__ __forceinline__ uint32_t ct_nbmask(const uint8_t* __restrict__ cls, int p, int PW) {
    const uint8_t *u = cls + p - PW, *m = cls + p, *d = cls + p + PW;
    return (uint32_t)(m[1] != 0) | ((uint32_t)(u[1] != 0) << 1) | ((uint32_t)(u[0] != 0) << 2) | ((uint32_t)(u[-1] != 0) << 3) |
           ((uint32_t)(m[-1] != 0) << 4) | ((uint32_t)(d[-1] != 0) << 5) | ((uint32_t)(d[0] != 0) << 6) | ((uint32_t)(d[1] != 0) << 7);
}

// the first set direction clockwise on screen after s: s - 1, s - 2, .., s; -1 where the pixel has no foreground neighbour
__device__ __forceinline__ int ct_first_cw(uint32_t mask, int s) {
#pragma unroll
    for (int k = 1; k <= 8; ++k) {
        const int d = (s - k) & 7;
        if ((mask >> d) & 1u) return d;
    }
    return -1;
}

// ---- labels ----------------------------------------------------------------------------------------------------------------------
// The class plane (1 foreground, 0 background and frame) and the first labels: the start of the pixel's run of equal class within its
// wave's 64 consecutive indices of the padded plane.  Runs may wrap from a row's last pixel to the next row's first: both are frame.
__global__ __launch_bounds__(CT_THREADS) void ct_init(const uint8_t* __restrict__ mask, const Geom g, uint8_t* __restrict__ cls,
                                                      int* __restrict__ L) {
    const int i = (int)(blockIdx.x * (unsigned)CT_THREADS + threadIdx.x);
    const bool inb = i < g.n;
    int c = 0;
    if (inb) {
        const int y = i / g.PW, x = i - y * g.PW;
        if (x >= 1 && x <= g.W && y >= 1 && y <= g.H) c = mask[(size_t)(y - 1) * (size_t)g.W + (size_t)(x - 1)] != 0 ? 1 : 0;
    }
    const unsigned long long fg = __ballot(c);
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned long long bnd = (fg ^ (fg << 1)) | 1ull;              // bit l: lane l begins a run
    const unsigned long long below = bnd & (~0ull >> (63 - lane));       // .. among lanes 0 .. lane
    const int first = 63 - __clzll((long long)below);
    if (inb) {
        cls[i] = (uint8_t)c;
        L[i] = i - lane + first;
    }
}

__device__ __forceinline__ int ct_ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int ct_find(const int* L, int a) {
    for (;;) {
        const int p = ct_ld(L + a);   // always < a, or a itself at a root: the walk ends
        if (p == a) return a;
        a = p;
    }
}

// Join the components of a and b.  A load may be stale (another XCD's atomic); it is still an older parent of the same node, so the
// walk ends at a node of the right component, and the atomicMin's return value, which is never stale, tells whether that node was
// still a root.  If it was not, the link it had (to `old`) may just have been replaced: `old` is joined with b in its stead.
__device__ void ct_unite(int* L, int a, int b) {
    for (;;) {
        a = ct_find(L, a);
        b = ct_find(L, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(L + a, b);
        if (old == a) return;
        a = old;   // < a: the pair strictly decreases, so this ends
    }
}

// Every adjacency the first labels do not already hold: the wave boundary along the row, the pixel above, and for foreground the two
// diagonals above where no shared 4-neighbour joins them anyway.
__global__ __launch_bounds__(CT_THREADS) void ct_merge(const uint8_t* __restrict__ cls, const Geom g, int* L) {
    const int i = (int)(blockIdx.x * (unsigned)CT_THREADS + threadIdx.x);
    if (i >= g.n) return;
    const int PW = g.PW;
    const int c = cls[i];
    if ((i & 63) == 0 && i > 0 && cls[i - 1] == c) ct_unite(L, i, i - 1);
    if (i < PW) return;   // the first row has nothing above it
    const int cn = cls[i - PW];
    if (c) {   // 1 <= x <= W and y >= 1: the three pixels above and the one to the left exist
        const int cw = cls[i - 1], cnw = cls[i - PW - 1], cne = cls[i - PW + 1];
        if (cn) {
            if (!(cw && cnw)) ct_unite(L, i, i - PW);   // (W, NW and N all foreground: W joins NW, NW and N share a run)
        } else {
            if (cnw && !cw) ct_unite(L, i, i - PW - 1);
            if (cne) ct_unite(L, i, i - PW + 1);
        }
    } else if (!cn) {
        const bool held = i - PW - 1 >= 0 && cls[i - 1] == 0 && cls[i - PW - 1] == 0;
        if (!held) ct_unite(L, i, i - PW);
    }
}

__device__ __forceinline__ bool ct_is_border(const uint8_t* __restrict__ cls, int i, int PW) {
    return !(cls[i - 1] && cls[i + 1] && cls[i - PW] && cls[i + PW]);
}

// L[i] = the root; and the workgroup's numbers of border pixels and of borders (roots other than the frame's)
__global__ __launch_bounds__(CT_THREADS) void ct_flatten(const uint8_t* __restrict__ cls, const Geom g, int* L, uint2* __restrict__ bcnt) {
    const int i = (int)(blockIdx.x * (unsigned)CT_THREADS + threadIdx.x);
    int isb = 0, isr = 0;
    if (i < g.n) {
        int r = i;
        for (;;) {   // plain loads: nothing is linked any more, a node holds an older parent or already its root
            const int p = L[r];
            if (p == r) break;
            r = p;
        }
        L[i] = r;
        isr = r == i && i != 0;
        isb = cls[i] && ct_is_border(cls, i, g.PW);
    }
    const int nb = __syncthreads_count(isb), nr = __syncthreads_count(isr);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = make_uint2((unsigned)nb, (unsigned)nr);
}

// exclusive scan of the per-workgroup counts, in place, by ONE workgroup; the totals and the ranking's flags go to the header
__global__ __launch_bounds__(CT_SCAN_THREADS) void ct_scan(uint2* bcnt, int nblk, int* __restrict__ hdr, int* __restrict__ table) {
    __shared__ uint2 wsum[CT_SCAN_THREADS / 64];
    __shared__ uint2 carry;
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = make_uint2(0u, 0u);
    if (tid < CT_HDR_INTS) hdr[tid] = tid == CT_ACT ? 1 : 0;
    __syncthreads();
    for (int base = 0; base < nblk; base += CT_SCAN_THREADS) {
        const int idx = base + tid;
        const uint2 v = idx < nblk ? bcnt[idx] : make_uint2(0u, 0u);
        uint2 inc = v;  // (wave_incl_scan of common.h on a pair, written out: two calls compile to different code)
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned ax = __shfl_up(inc.x, o, 64), ay = __shfl_up(inc.y, o, 64);
            if (lane >= o) inc.x += ax, inc.y += ay;
        }
        if (lane == 63) wsum[wv] = inc;
        __syncthreads();
        uint2 pre = carry;
        for (int j = 0; j < wv; ++j) pre.x += wsum[j].x, pre.y += wsum[j].y;
        if (idx < nblk) bcnt[idx] = make_uint2(pre.x + inc.x - v.x, pre.y + inc.y - v.y);
        __syncthreads();
        if (tid == CT_SCAN_THREADS - 1) carry = make_uint2(pre.x + inc.x, pre.y + inc.y);
        __syncthreads();
    }
    if (tid == 0) {
        hdr[0] = (int)carry.x, hdr[1] = (int)carry.y;
        table[0] = (int)carry.x, table[1] = (int)carry.y, table[2] = 0, table[3] = 0;
    }
}

// Slots in raster order.  slot[i]: a border pixel's slot; a hole root's border number; -1 otherwise, and where the room ran out.
__global__ __launch_bounds__(CT_THREADS) void ct_compact(const uint8_t* __restrict__ cls, const int* __restrict__ L, const Geom g,
                                                         const uint2* __restrict__ bcnt, int* __restrict__ slot, int* __restrict__ bpix,
                                                         int* __restrict__ obid, int* __restrict__ table) {
    __shared__ uint2 wsum[CT_THREADS / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int i = (int)(blockIdx.x * (unsigned)CT_THREADS + threadIdx.x);
    const bool inb = i < g.n;
    int isb = 0, isr = 0, c = 0;
    if (inb) {
        c = cls[i];
        isr = L[i] == i && i != 0;
        isb = c && ct_is_border(cls, i, g.PW);
    }
    const unsigned long long mb = __ballot(isb), mr = __ballot(isr), lt = (1ull << lane) - 1ull;
    if (lane == 0) wsum[wv] = make_uint2((unsigned)__popcll(mb), (unsigned)__popcll(mr));
    __syncthreads();
    uint2 pre = bcnt[blockIdx.x];
    for (int j = 0; j < wv; ++j) pre.x += wsum[j].x, pre.y += wsum[j].y;
    if (!inb) return;
    int s = isb ? (int)(pre.x + (unsigned)__popcll(mb & lt)) : -1;
    int r = isr ? (int)(pre.y + (unsigned)__popcll(mr & lt)) : -1;
    if (s >= g.cap_b) s = -1;
    if (r >= g.cap_c) r = -1;
    if (s >= 0) {
        bpix[s] = i;
        obid[s] = isr ? r : -1;
    }
    slot[i] = c ? s : r;
    if (r >= 0) {
        const int PW = g.PW, W = g.W;
        const int start = c ? i : i - 1;   // a hole's border starts west of its first pixel: foreground, or i were not the first
        const int sy = start / PW, sx = start - sy * PW;
        int* row = table + 4 * (size_t)(r + 1);
        row[0] = (sy - 1) * W + (sx - 1);
        row[1] = c ? 0 : 1;
        row[2] = 0;
        int parent = -1;
        if (!c) {
            const int pl = L[start], py = pl / PW, px = pl - py * PW;
            parent = (py - 1) * W + (px - 1);
        }
        row[3] = parent;
    }
}

// ---- states ----------------------------------------------------------------------------------------------------------------------
// the state before (p, d) on its cycle: at the previous point q, the first foreground neighbour clockwise from the direction of p
__device__ __forceinline__ int ct_pred_state(const uint8_t* __restrict__ cls, const int* __restrict__ slot, int p, int d, int PW) {
    const int q = p + ct_off(d, PW);
    const int sq = slot[q];
    if (sq < 0) return -1;   // q is no border pixel (or the room ran out)
    return sq * 8 + ct_first_cw(ct_nbmask(cls, q, PW), (d + 4) & 7);   // (bit (d + 4) & 7 is p itself: never -1)
}

__global__ __launch_bounds__(CT_THREADS) void ct_links(const uint8_t* __restrict__ cls, const int* __restrict__ L, const int* __restrict__ slot,
                                                       const int* __restrict__ bpix, const int* __restrict__ obid, const int* __restrict__ hdr,
                                                       const Geom g, uint2* __restrict__ st, int* __restrict__ hb) {
    const int nb = ct_min(hdr[0], g.cap_b), PW = g.PW;
    for (int s = (int)(blockIdx.x * (unsigned)CT_THREADS + threadIdx.x); s < nb; s += (int)(gridDim.x * (unsigned)CT_THREADS)) {
        const int p = bpix[s];
        const uint32_t m = ct_nbmask(cls, p, PW);
        int d_out = -1, r_out = obid[s], d_hole = -1, r_hole = -1;
        if (r_out >= 0) d_out = ct_first_cw(m, 4);                 // the start of an outer border: search from the west neighbour
        if (cls[p + 1] == 0 && L[p + 1] == p + 1) {                // .. of a hole border: from the east neighbour, the hole's first pixel
            r_hole = slot[p + 1];
            if (r_hole >= 0) d_hole = ct_first_cw(m, 0);
        }
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int me = s * 8 + d;
            uint2 v = make_uint2((unsigned)me, 0u);
            int head = -1;
            // (a foreground neighbour in the next direction too: the successor is found without passing a background pixel, and so is
            // its own, and the third step is back here -- three mutually adjacent pixels, a cycle that bounds nothing: left out)
            if (((m >> d) & 1u) && !((m >> ((d + 1) & 7)) & 1u)) {
                if (d == d_out) {
                    head = r_out;
                } else if (d == d_hole) {
                    head = r_hole;
                } else {
                    const int pr = ct_pred_state(cls, slot, p, d, PW);
                    if (pr >= 0) v = make_uint2((unsigned)pr, 1u);
                }
            }
            st[me] = v;
            hb[me] = head;
        }
    }
}

// one doubling pass, src -> dst; does nothing unless pass k - 1 changed a pointer
__global__ __launch_bounds__(CT_THREADS) void ct_rank(const uint2* __restrict__ src, uint2* __restrict__ dst, int* hdr, int k, const Geom g) {
    if (hdr[CT_ACT + k] == 0) return;
    const int ns = 8 * ct_min(hdr[0], g.cap_b);
    bool changed = false;
    for (int s = (int)(blockIdx.x * (unsigned)CT_THREADS + threadIdx.x); s < ns; s += (int)(gridDim.x * (unsigned)CT_THREADS)) {
        uint2 v = src[s];
        if (v.x != (unsigned)s) {
            const uint2 t = src[v.x];
            changed |= t.x != v.x;
            v = make_uint2(t.x, v.y + t.y);   // (unsigned: a cycle that was never cut wraps harmlessly and is dropped)
        }
        dst[s] = v;
    }
    if (changed) __hip_atomic_store(hdr + CT_ACT + k + 1, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the number of passes that ran: the ranks lie in buffer (that number & 1)
__device__ __forceinline__ int ct_passes_run(const int* __restrict__ hdr, int passes) {
    int k = 0;
    while (k < passes && hdr[CT_ACT + k] != 0) ++k;
    return k;
}

__global__ __launch_bounds__(CT_THREADS) void ct_table(const uint8_t* __restrict__ cls, const int* __restrict__ slot, const int* __restrict__ hdr,
                                                       const Geom g, const uint2* __restrict__ st0, const uint2* __restrict__ st1,
                                                       int* __restrict__ table) {
    const int nc = ct_min(hdr[1], g.cap_c), PW = g.PW;
    const int run = ct_passes_run(hdr, g.passes);
    const uint2* fin = (run & 1) ? st1 : st0;
    if (blockIdx.x == 0 && threadIdx.x == 0) table[2] = run, table[3] = hdr[CT_ACT + g.passes] != 0 ? 1 : 0;
    for (int r = (int)(blockIdx.x * (unsigned)CT_THREADS + threadIdx.x); r < nc; r += (int)(gridDim.x * (unsigned)CT_THREADS)) {
        int* row = table + 4 * (size_t)(r + 1);
        const int su = row[0], sy = su / g.W, sx = su - sy * g.W;
        const int p = (sy + 1) * PW + sx + 1;
        const int d0 = ct_first_cw(ct_nbmask(cls, p, PW), row[1] ? 0 : 4);
        int len = 1;   // an isolated pixel
        if (d0 >= 0) {
            const int sp = slot[p], tail = ct_pred_state(cls, slot, p, d0, PW);
            len = -1;   // (stays where the room ran out, or the tail did not reach its head: the caller refuses)
            if (sp >= 0 && tail >= 0) {
                const uint2 t = fin[tail];
                if (t.x == (unsigned)(sp * 8 + d0)) len = (int)t.y + 1;
            }
        }
        row[2] = len;
    }
}

__global__ __launch_bounds__(CT_THREADS) void ct_emit(const int* __restrict__ hdr, const Geom g, const uint2* __restrict__ st0,
                                                      const uint2* __restrict__ st1, const int* __restrict__ hb, const int* __restrict__ bpix,
                                                      const int* __restrict__ table, const int* __restrict__ offsets, int n_borders, int n_points,
                                                      int2* __restrict__ points) {
    const int ns = 8 * ct_min(hdr[0], g.cap_b), nc = ct_min(ct_min(hdr[1], g.cap_c), n_borders), PW = g.PW;
    const uint2* fin = (ct_passes_run(hdr, g.passes) & 1) ? st1 : st0;
    const int stride = (int)(gridDim.x * (unsigned)CT_THREADS);
    for (int s = (int)(blockIdx.x * (unsigned)CT_THREADS + threadIdx.x); s < ns; s += stride) {
        const uint2 v = fin[s];
        if (v.x >= (unsigned)ns) continue;
        const int r = hb[v.x];
        if (r < 0 || r >= nc) continue;
        const int len = table[4 * (size_t)(r + 1) + 2], o = offsets[r];
        if (v.y >= (unsigned)len || o < 0 || o > n_points - len) continue;
        const int p = bpix[s >> 3], y = p / PW, x = p - y * PW;
        points[o + (int)v.y] = make_int2(x - 1, y - 1);
    }
    for (int r = (int)(blockIdx.x * (unsigned)CT_THREADS + threadIdx.x); r < nc; r += stride) {   // the one-point borders have no state
        const int* row = table + 4 * (size_t)(r + 1);
        const int o = offsets[r];
        if (row[2] != 1 || o < 0 || o >= n_points) continue;
        const int y = row[0] / g.W;
        points[o] = make_int2(row[0] - y * g.W, y);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct CtScratch {
    int* hdr;
    uint8_t* cls;
    int *L, *slot;
    uint2* bcnt;
    int *bpix, *obid;
    uint2 *st0, *st1;
    int* hb;
};

// the ONE layout, for both entry points: hipt_contours_emit reads what hipt_contours_trace left
CtScratch carve_contours(Carver& c, const Geom& g) {
    CtScratch s = {};
    const size_t n = (size_t)g.n, nblk = (n + CT_THREADS - 1) / CT_THREADS, nb = (size_t)g.cap_b;
    s.hdr = c.take<int>(CT_HDR_INTS);
    s.cls = c.take<uint8_t>(n);
    s.L = c.take<int>(n);
    s.slot = c.take<int>(n);
    s.bcnt = c.take<uint2>(nblk);
    s.bpix = c.take<int>(nb);
    s.obid = c.take<int>(nb);
    s.st0 = c.take<uint2>(8 * nb);
    s.st1 = c.take<uint2>(8 * nb);
    s.hb = c.take<int>(8 * nb);
    return s;
}

unsigned stride_grid(long long items) {
    const long long b = (items + CT_THREADS - 1) / CT_THREADS;
    return (unsigned)(b < 1 ? 1 : (b > CT_MAX_GRID ? CT_MAX_GRID : b));
}

}  // namespace

extern "C" size_t hipt_contours_workspace_bytes(int h, int w) {
    if (!plane_ok(h, w)) return 0;
    const Geom g = make_geom(h, w);
    return dry_run([&](Carver& c) { carve_contours(c, g); });
}

extern "C" int hipt_contours_trace(const uint8_t* mask, int h, int w, int32_t* table, void* ws, size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(h >= 1 && w >= 1, "contours: plane of %d x %d", h, w);
    if (!plane_ok(h, w)) {
        hipt_set_error("contours: plane of %d x %d: (h + 2) (w + 2) must not exceed 2^27; nothing was launched", h, w);
        return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_ARG(mask && table, "contours: mask / table missing");
    HIPT_CHECK_ARG(((uintptr_t)table & 15) == 0, "contours: table needs 16-byte alignment");
    const Geom g = make_geom(h, w);
    static_assert(CT_ACT + 32 + 1 <= CT_HDR_INTS, "the header holds a flag per pass");
    Carver c(ws, ws_bytes);
    const CtScratch s = carve_contours(c, g);
    if (int rc = check_workspace(c, "hipt_contours_trace")) return rc;
    HIPT_CHECK_ARG(ws != nullptr, "contours: the workspace is missing");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = (unsigned)(((long long)g.n + CT_THREADS - 1) / CT_THREADS);
    const dim3 block(CT_THREADS);
    hipLaunchKernelGGL(ct_init, dim3(nblk), block, 0, st, mask, g, s.cls, s.L);
    HIPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_merge, dim3(nblk), block, 0, st, s.cls, g, s.L);
    HIPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_flatten, dim3(nblk), block, 0, st, s.cls, g, s.L, s.bcnt);
    HIPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_scan, dim3(1), dim3(CT_SCAN_THREADS), 0, st, s.bcnt, (int)nblk, s.hdr, table);
    HIPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_compact, dim3(nblk), block, 0, st, s.cls, s.L, g, s.bcnt, s.slot, s.bpix, s.obid, table);
    HIPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(ct_links, dim3(stride_grid(g.cap_b)), block, 0, st, s.cls, s.L, s.slot, s.bpix, s.obid, s.hdr, g, s.st0, s.hb);
    HIPT_CHECK_LAUNCH();
    const unsigned sgrid = stride_grid(8LL * g.cap_b);
    for (int k = 0; k < g.passes; ++k) {
        hipLaunchKernelGGL(ct_rank, dim3(sgrid), block, 0, st, (k & 1) ? s.st1 : s.st0, (k & 1) ? s.st0 : s.st1, s.hdr, k, g);
        HIPT_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(ct_table, dim3(stride_grid(g.cap_c)), block, 0, st, s.cls, s.slot, s.hdr, g, s.st0, s.st1, table);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

extern "C" int hipt_contours_emit(int h, int w, const int32_t* table, const int32_t* offsets, int n_borders, int n_points, int32_t* points,
                                  const void* ws, size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(h >= 1 && w >= 1, "contours: plane of %d x %d", h, w);
    if (!plane_ok(h, w)) {
        hipt_set_error("contours: plane of %d x %d: (h + 2) (w + 2) must not exceed 2^27; nothing was launched", h, w);
        return HIPT_E_UNSUPPORTED;
    }
    const Geom g = make_geom(h, w);
    HIPT_CHECK_ARG(n_borders >= 1 && n_borders <= g.cap_c && n_points >= n_borders && n_points <= 8LL * g.cap_b + n_borders,
                   "contours: %d borders / %d points", n_borders, n_points);
    HIPT_CHECK_ARG(table && offsets && points, "contours: table / offsets / points missing");
    HIPT_CHECK_ARG(((uintptr_t)points & 7) == 0 && ((uintptr_t)offsets & 3) == 0 && ((uintptr_t)table & 15) == 0,
                   "contours: points need 8-byte, offsets 4-byte, table 16-byte alignment");
    Carver c((void*)ws, ws_bytes);
    const CtScratch s = carve_contours(c, g);
    if (int rc = check_workspace(c, "hipt_contours_emit")) return rc;
    HIPT_CHECK_ARG(ws != nullptr, "contours: the workspace is missing");
    const long long items = 8LL * g.cap_b > n_borders ? 8LL * g.cap_b : n_borders;
    hipLaunchKernelGGL(ct_emit, dim3(stride_grid(items)), dim3(CT_THREADS), 0, (hipStream_t)stream, s.hdr, g, s.st0, s.st1, s.hb, s.bpix, table,
                       offsets, n_borders, n_points, (int2*)points);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
