// Pillow's Image.resize of 8-bit RGB images (interleaved uint8 [n, H, W, 3]); DESIGN.md 23, include/hipt_abmil.h.
//
// Pillow resizes in two separable passes, horizontal first, and stores the intermediate image as uint8.  Behind the host-side table
// of 22-bit fixed-point weights (resize.py: resize_table) a pass is integer: out = clip((2^21 + sum_x src[xmin + x] * k[x]) >> 22) in
// int32.  ONE kernel does all of it: a workgroup owns a tile of tw x th output pixels and
//   1. copies the input rows the tile's vertical taps need, RC rows at a time and only the columns the tile's horizontal taps need,
//      into LDS as 16-byte vectors (3-byte pixels do not align to lanes; the row's misalignment is an offset into the LDS row);
//   2. runs the horizontal pass out of those raw rows into an LDS image of uint8 -- the bytes Pillow's intermediate image would hold;
//   3. runs the vertical pass out of that image and stores whole 32-bit words, single bytes only where a tile row's first or last
//      word is shared with a neighbour.
// An axis whose length does not change is skipped as Pillow skips it: step 2 (or 3) is then a copy.  The FUSED route is one launch
// with both passes; the GENERAL route is one launch per changing axis with the intermediate image in the caller's workspace, for
// geometries whose fused tile does not fit the LDS.  No floating point, no atomics, no allocation, no synchronisation with the host.
//
// The tables live on the device, so the launcher cannot read them.  The LDS sizes come from the geometry alone: xmin advances by at
// most ceil(d * scale) over d outputs and xmax <= ksize, so a tile of t outputs reads at most ceil((t - 1) * scale) + 1 + ksize inputs.
// Whatever a table holds, the kernel clamps every bound to the image and to the tile's staged window: no access leaves src, dst,
// the tables or the LDS.
#include <math.h>

#include "common.h"
#include "workspace.h"

namespace {

constexpr int RZ_THREADS = 256;
constexpr int RZ_LDS_MAX = 64 * 1024;   // the static launch limit: no per-device opt-in
constexpr int RZ_HALF = 1 << 21, RZ_SHIFT = 22;

struct ResizeArgs {
    const uint8_t* src;   // [n, H, W, 3]
    uint8_t* dst;         // [n, OH, OW, 3]
    const int32_t *kx, *bx, *ky, *by;   // kx [OW, ksx], bx [OW, 2]; ky [OH, ksy], by [OH, 2]; NULL for a skipped axis
    int n, H, W, OH, OW, ksx, ksy;
    int TW, TH, RC;       // tile of output pixels, raw input rows per chunk
    int tiles_x, tiles_y;
    int span_px;          // input pixels a tile's raw row holds at most
    int rows_cap;         // input rows a tile's intermediate image holds at most
    int raw_stride;       // bytes, a multiple of 16: >= 15 + span_px * 3
    int inter_stride;     // bytes, a multiple of 4: >= TW * 3
    long long src_bytes;  // n * H * W * 3
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint32_t clip8(int acc) { return (uint32_t)clampi(acc >> RZ_SHIFT, 0, 255); }

__global__ __launch_bounds__(RZ_THREADS) void resize_kernel(const ResizeArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const bool do_h = A.kx != nullptr, do_v = A.ky != nullptr;
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    const int tx = b % A.tiles_x;
    b /= A.tiles_x;
    const int ty = b % A.tiles_y;
    const int img = b / A.tiles_y;
    const int ox0 = tx * A.TW, oy0 = ty * A.TH;
    const int tw = min(A.TW, A.OW - ox0), th = min(A.TH, A.OH - oy0);

    // LDS: the tile's weights (int32), the raw chunk (16-byte aligned rows), the intermediate image
    int32_t* kxs = (int32_t*)smem;
    int32_t* kys = kxs + (do_h ? A.TW * A.ksx : 0);
    size_t at = ((size_t)((do_h ? A.TW * A.ksx : 0) + (do_v ? A.TH * A.ksy : 0)) * 4 + 15) & ~(size_t)15;
    uint8_t* raw = smem + at;
    uint8_t* inter = raw + (size_t)A.RC * A.raw_stride;

    // the tile's window of input columns [c0, c1) and rows [r0, r0 + nrows)
    int c0 = ox0, c1 = ox0 + tw;
    if (do_h) {
        c0 = clampi(A.bx[2 * ox0], 0, A.W);
        const int last = ox0 + tw - 1;
        const int lmin = clampi(A.bx[2 * last], 0, A.W);
        c1 = lmin + clampi(A.bx[2 * last + 1], 0, A.W - lmin);
        c1 = clampi(c1, c0, min(A.W, c0 + A.span_px));
    }
    int r0 = oy0, nrows = th;
    if (do_v) {
        r0 = clampi(A.by[2 * oy0], 0, A.H);
        const int last = oy0 + th - 1;
        const int lmin = clampi(A.by[2 * last], 0, A.H);
        const int r1 = lmin + clampi(A.by[2 * last + 1], 0, A.H - lmin);
        nrows = clampi(r1 - r0, 0, min(A.H - r0, A.rows_cap));
    }
    if (do_h)
        for (int i = tid; i < tw * A.ksx; i += RZ_THREADS) kxs[i] = A.kx[(size_t)ox0 * A.ksx + i];
    if (do_v)
        for (int i = tid; i < th * A.ksy; i += RZ_THREADS) kys[i] = A.ky[(size_t)oy0 * A.ksy + i];

    const int win_bytes = (c1 - c0) * 3;
    const int NV = A.raw_stride >> 4;
    for (int rs = 0; rs < nrows; rs += A.RC) {
        const int rc = min(A.RC, nrows - rs);
        __syncthreads();   // the previous chunk's readers are done with `raw` (first round: nothing yet)
        // 1. raw rows: 16-byte vectors from the aligned address at or below the window's first byte
        for (int i = tid; i < rc * NV; i += RZ_THREADS) {
            const int rr = i / NV, v = i - rr * NV;
            const long long g = (((long long)img * A.H + (r0 + rs + rr)) * A.W + c0) * 3;
            const int off = (int)(g & 15);
            if (v * 16 >= off + win_bytes) continue;
            const long long ga = (g & ~15LL) + 16LL * v;
            u32x4 q;
            if (ga + 16 <= A.src_bytes) {
                q = *(const u32x4*)(A.src + ga);
            } else {   // the last bytes of the last image: byte by byte, nothing past the end
                uint32_t w[4] = {0, 0, 0, 0};
                for (int k = 0; k < 16; ++k)
                    if (ga + k < A.src_bytes) w[k >> 2] |= (uint32_t)A.src[ga + k] << (8 * (k & 3));
                q[0] = w[0];
                q[1] = w[1];
                q[2] = w[2];
                q[3] = w[3];
            }
            *(u32x4*)(raw + (size_t)rr * A.raw_stride + 16 * v) = q;
        }
        __syncthreads();
        // 2. horizontal pass (or copy) into the intermediate rows rs .. rs + rc - 1
        if (do_h) {
            for (int i = tid; i < rc * tw; i += RZ_THREADS) {
                const int rr = i / tw, xl = i - rr * tw;
                const long long g = (((long long)img * A.H + (r0 + rs + rr)) * A.W + c0) * 3;
                const uint8_t* row = raw + (size_t)rr * A.raw_stride + (int)(g & 15);
                const int xmin = clampi(A.bx[2 * (ox0 + xl)], c0, c1);
                const int xmax = clampi(A.bx[2 * (ox0 + xl) + 1], 0, min(A.ksx, c1 - xmin));
                const int32_t* kk = kxs + xl * A.ksx;
                const uint8_t* p = row + (xmin - c0) * 3;
                int a0 = RZ_HALF, a1 = RZ_HALF, a2 = RZ_HALF;
                for (int x = 0; x < xmax; ++x) {
                    const int kv = kk[x];
                    a0 += (int)p[3 * x] * kv;
                    a1 += (int)p[3 * x + 1] * kv;
                    a2 += (int)p[3 * x + 2] * kv;
                }
                uint8_t* o = inter + (size_t)(rs + rr) * A.inter_stride + xl * 3;
                o[0] = (uint8_t)clip8(a0);
                o[1] = (uint8_t)clip8(a1);
                o[2] = (uint8_t)clip8(a2);
            }
        } else {
            for (int i = tid; i < rc * win_bytes; i += RZ_THREADS) {
                const int rr = i / win_bytes, j = i - rr * win_bytes;
                const long long g = (((long long)img * A.H + (r0 + rs + rr)) * A.W + c0) * 3;
                inter[(size_t)(rs + rr) * A.inter_stride + j] = raw[(size_t)rr * A.raw_stride + (int)(g & 15) + j];
            }
        }
    }
    __syncthreads();
    // 3. vertical pass (or copy) out of the intermediate image: one 32-bit word of an output row per item
    const int len = tw * 3;
    const int slots_max = (A.TW * 3 + 6) >> 2;
    for (int i = tid; i < th * slots_max; i += RZ_THREADS) {
        const int yl = i / slots_max, s = i - yl * slots_max;
        const long long d0 = (((long long)img * A.OH + (oy0 + yl)) * A.OW + ox0) * 3;   // the tile row's first byte in dst
        const int head = (int)(d0 & 3);
        const int j0 = 4 * s - head;   // the tile-row byte of this word's byte 0
        if (j0 >= len) continue;
        int ymin = yl, ymax = 1;
        if (do_v) {
            const int lo = clampi(A.by[2 * (oy0 + yl)], r0, r0 + nrows);
            ymax = clampi(A.by[2 * (oy0 + yl) + 1], 0, min(A.ksy, r0 + nrows - lo));
            ymin = lo - r0;
        } else if (yl >= nrows) {
            continue;
        }
        uint32_t word = 0;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = j0 + k;
            v[k] = 0;
            if (j < 0 || j >= len) continue;
            const uint8_t* col = inter + (size_t)ymin * A.inter_stride + j;
            if (do_v) {
                const int32_t* kk = kys + yl * A.ksy;
                int acc = RZ_HALF;
                for (int y = 0; y < ymax; ++y) acc += (int)col[(size_t)y * A.inter_stride] * kk[y];
                v[k] = clip8(acc);
            } else {
                v[k] = col[0];
            }
            word |= v[k] << (8 * k);
        }
        uint8_t* o = A.dst + d0 + j0;
        if (j0 >= 0 && j0 + 4 <= len) {
            *(uint32_t*)o = word;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (j0 + k >= 0 && j0 + k < len) o[k] = (uint8_t)v[k];
        }
    }
}

// The tile shapes tried, best first: output columns, output rows, raw rows per chunk.  The fused route takes one of the first
// RZ_FUSED_SHAPES; a single pass takes any.
struct TileShape {
    int tw, th, rc;
};
constexpr TileShape RZ_SHAPES[] = {{64, 32, 16}, {64, 16, 16}, {32, 16, 8}, {32, 8, 8}, {16, 8, 4}, {8, 8, 4}, {8, 4, 2}, {4, 4, 1}};
constexpr int RZ_FUSED_SHAPES = 4;
constexpr int RZ_NSHAPES = (int)(sizeof(RZ_SHAPES) / sizeof(RZ_SHAPES[0]));

// inputs a run of t outputs reads at most (see the head of the file), capped at the axis
int span_of(int t, int in_len, int out_len, int ksize) {
    const double scale = (double)in_len / (double)out_len;
    const double s = ceil((double)(t - 1) * scale) + 1.0 + (double)ksize;
    return s < (double)in_len ? (int)s : in_len;
}

// fills the tile fields of A for one launch (H x W -> OH x OW as A holds them); the LDS bytes, or 0 when no shape up to `nshapes` fits
size_t plan(ResizeArgs& A, int nshapes) {
    const bool do_h = A.kx != nullptr, do_v = A.ky != nullptr;
    for (int i = 0; i < nshapes; ++i) {
        const TileShape& t = RZ_SHAPES[i];
        const int span = do_h ? span_of(t.tw, A.W, A.OW, A.ksx) : t.tw;
        const int rows = do_v ? span_of(t.th, A.H, A.OH, A.ksy) : t.th;
        const size_t raw_stride = ((size_t)span * 3 + 15 + 15) & ~(size_t)15;
        const size_t inter_stride = ((size_t)t.tw * 3 + 3) & ~(size_t)3;
        const size_t tables = (((size_t)(do_h ? t.tw * A.ksx : 0) + (size_t)(do_v ? t.th * A.ksy : 0)) * 4 + 15) & ~(size_t)15;
        const size_t lds = tables + (size_t)t.rc * raw_stride + (size_t)rows * inter_stride;
        if (lds > (size_t)RZ_LDS_MAX) continue;
        A.TW = t.tw;
        A.TH = t.th;
        A.RC = t.rc;
        A.span_px = span;
        A.rows_cap = rows;
        A.raw_stride = (int)raw_stride;
        A.inter_stride = (int)inter_stride;
        A.tiles_x = (A.OW + t.tw - 1) / t.tw;
        A.tiles_y = (A.OH + t.th - 1) / t.th;
        return lds;
    }
    return 0;
}

int launch(ResizeArgs& A, int nshapes, const char* what, hipStream_t st) {
    const size_t lds = plan(A, nshapes);
    if (lds == 0) {
        hipt_set_error("resize: %s of %d x %d -> %d x %d with %d / %d taps: no tile fits the LDS; nothing was launched", what, A.H, A.W, A.OH,
                       A.OW, A.ksx, A.ksy);
        return HIPT_E_UNSUPPORTED;
    }
    const long long blocks = (long long)A.n * A.tiles_y * A.tiles_x;
    if (blocks >= (1LL << 31)) {
        hipt_set_error("resize: %lld tiles in one launch", blocks);
        return HIPT_E_UNSUPPORTED;
    }
    A.src_bytes = (long long)A.n * A.H * A.W * 3;
    hipLaunchKernelGGL(resize_kernel, dim3((unsigned)blocks), dim3(RZ_THREADS), lds, st, A);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

bool geometry_ok(int n, int in_h, int in_w, int out_h, int out_w) {
    const int lim = 1 << 24;
    return n >= 1 && in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1 && in_h < lim && in_w < lim && out_h < lim && out_w < lim &&
           (double)n * (in_h > out_h ? in_h : out_h) * (in_w > out_w ? in_w : out_w) * 3.0 < 1099511627776.0 /* 2^40 */;
}

// the general route's intermediate image [n, in_h, out_w, 3]: needed when both axes change
uint8_t* carve_resize(Carver& c, int n, int in_h, int in_w, int out_h, int out_w, int route) {
    if (route == HIPT_RESIZE_FUSED || in_h == out_h || in_w == out_w) return nullptr;
    return c.take<uint8_t>((size_t)n * in_h * out_w * 3);
}

}  // namespace

extern "C" size_t hipt_resize_workspace_bytes(int n, int in_h, int in_w, int out_h, int out_w, int route) {
    if (!geometry_ok(n, in_h, in_w, out_h, out_w) || route < HIPT_RESIZE_AUTO || route > HIPT_RESIZE_FUSED) return 0;
    return dry_run([&](Carver& c) { carve_resize(c, n, in_h, in_w, out_h, out_w, route); });
}

extern "C" int hipt_resize_u8(const uint8_t* src, int n, int in_h, int in_w, int out_h, int out_w, const int32_t* kx, const int32_t* bx,
                              int ksize_x, const int32_t* ky, const int32_t* by, int ksize_y, uint8_t* dst, void* ws, size_t ws_bytes, int route,
                              void* stream) {
    HIPT_CHECK_ARG(route >= HIPT_RESIZE_AUTO && route <= HIPT_RESIZE_FUSED, "resize: route %d", route);
    HIPT_CHECK_ARG(n >= 1 && in_h >= 1 && in_w >= 1 && out_h >= 1 && out_w >= 1, "resize: %d images of %d x %d -> %d x %d", n, in_h, in_w,
                   out_h, out_w);
    const bool do_h = in_w != out_w, do_v = in_h != out_h;
    if (!geometry_ok(n, in_h, in_w, out_h, out_w) || (do_h && ksize_x > HIPT_RESIZE_MAX_KSIZE) || (do_v && ksize_y > HIPT_RESIZE_MAX_KSIZE)) {
        hipt_set_error("resize: %d images of %d x %d -> %d x %d with %d / %d taps outside the envelope (sides below 2^24, n * H * W * 3 below "
                       "2^40, at most %d taps); nothing was launched", n, in_h, in_w, out_h, out_w, ksize_x, ksize_y, HIPT_RESIZE_MAX_KSIZE);
        return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_ARG(src && dst && src != dst, "resize: src / dst missing, or the same");
    HIPT_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 3) == 0, "resize: src needs 16-byte, dst 4-byte alignment");
    HIPT_CHECK_ARG(!do_h || (kx && bx && ksize_x >= 1), "resize: the width changes: kx / bx / ksize_x missing");
    HIPT_CHECK_ARG(!do_v || (ky && by && ksize_y >= 1), "resize: the height changes: ky / by / ksize_y missing");
    HIPT_CHECK_ARG((((uintptr_t)kx | (uintptr_t)bx | (uintptr_t)ky | (uintptr_t)by) & 3) == 0, "resize: the tables need 4-byte alignment");
    ResizeArgs A = {};
    A.n = n;
    if (route == HIPT_RESIZE_FUSED && !(do_h && do_v)) {
        hipt_set_error("resize: the fused route takes calls that change both axes (%d x %d -> %d x %d); nothing was launched", in_h, in_w, out_h,
                       out_w);
        return HIPT_E_UNSUPPORTED;
    }
    if (!(do_h && do_v)) {   // one pass, or the copy of equal sizes: a single launch, no workspace
        A.src = src, A.dst = dst, A.H = in_h, A.W = in_w, A.OH = out_h, A.OW = out_w;
        A.kx = do_h ? kx : nullptr, A.bx = do_h ? bx : nullptr, A.ksx = do_h ? ksize_x : 0;
        A.ky = do_v ? ky : nullptr, A.by = do_v ? by : nullptr, A.ksy = do_v ? ksize_y : 0;
        return launch(A, RZ_NSHAPES, "one pass", (hipStream_t)stream);
    }
    A.src = src, A.dst = dst, A.H = in_h, A.W = in_w, A.OH = out_h, A.OW = out_w;
    A.kx = kx, A.bx = bx, A.ksx = ksize_x, A.ky = ky, A.by = by, A.ksy = ksize_y;
    if (route != HIPT_RESIZE_GENERAL) {
        ResizeArgs F = A;
        if (plan(F, RZ_FUSED_SHAPES) != 0 || route == HIPT_RESIZE_FUSED) return launch(A, RZ_FUSED_SHAPES, "the fused route", (hipStream_t)stream);
    }
    // general route: horizontal pass into the workspace, vertical pass out of it.  Both plans are made before the first launch.
    Carver c(ws, ws_bytes);
    uint8_t* mid = carve_resize(c, n, in_h, in_w, out_h, out_w, HIPT_RESIZE_GENERAL);
    if (int rc = check_workspace(c, "hipt_resize_u8")) return rc;
    HIPT_CHECK_ARG(mid != nullptr, "resize: the general route needs its workspace");
    ResizeArgs P1 = {}, P2 = {};
    P1.n = P2.n = n;
    P1.src = src, P1.dst = mid, P1.H = in_h, P1.W = in_w, P1.OH = in_h, P1.OW = out_w, P1.kx = kx, P1.bx = bx, P1.ksx = ksize_x;
    P2.src = mid, P2.dst = dst, P2.H = in_h, P2.W = out_w, P2.OH = out_h, P2.OW = out_w, P2.ky = ky, P2.by = by, P2.ksy = ksize_y;
    ResizeArgs T1 = P1, T2 = P2;
    if (plan(T1, RZ_NSHAPES) == 0 || plan(T2, RZ_NSHAPES) == 0) {
        hipt_set_error("resize: %d x %d -> %d x %d with %d / %d taps: no tile fits the LDS; nothing was launched", in_h, in_w, out_h, out_w,
                       ksize_x, ksize_y);
        return HIPT_E_UNSUPPORTED;
    }
    if (int rc = launch(P1, RZ_NSHAPES, "the horizontal pass", (hipStream_t)stream)) return rc;
    return launch(P2, RZ_NSHAPES, "the vertical pass", (hipStream_t)stream);
}
