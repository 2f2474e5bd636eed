// Attention heat-map rasteriser (wsi_core/WholeSlideImage.py:576-684 with blur=False): N equally sized patches with
// one value each become overlay[h, w] = (sum of the covering patches' values, IN ASCENDING PATCH INDEX, in float64) / (their
// number), and that overlay, through a colour table, a mask and the canvas, becomes the uint8 image.
//
// Pixels GATHER; nothing is scattered and there is no floating-point atomic anywhere:
//   1. bin     every patch adds 1 to the counter of each HM_TW x HM_TH canvas tile it touches (integer atomics);
//   2. scan    exclusive prefix sum of the tile counters: 1024-tile segments, then the segment totals;
//   3. fill    every patch appends its index to the list of each tile it touches (integer atomic cursor: arrival order);
//   4. sort    one wave per tile puts the tile's list into ascending patch index (bitonic network, in LDS while the list fits
//              HM_SORT_LDS entries, in place in global memory beyond that), which makes the lists -- and so every sum -- a
//              function of the input alone;
//   5. pixel   one workgroup per tile, one thread per pixel: the tile's list is walked in chunks of HM_CHUNK candidates staged
//              through LDS (clipped rectangle, value, paint flag); every thread tests its pixel against each candidate and adds in
//              list order.  Mask, paint decision, colour lookup and blend follow in the same thread; the image bytes of the tile go
//              through LDS and leave as aligned 32-bit stores, each image byte written once.
// -ffp-contract=off (Makefile): the blend's two products and their sum are rounded one by one.  No inline assembly.
#include "common.h"
#include "kernels.h"
#include "workspace.h"

namespace {

constexpr int HM_TW = HIPT_HEATMAP_TILE_W, HM_TH = HIPT_HEATMAP_TILE_H;   // canvas tile of one workgroup
constexpr int HM_THREADS = HM_TW * HM_TH;                                  // one thread per pixel
constexpr int HM_CHUNK = 256;        // candidates staged per LDS chunk (one per thread)
constexpr int HM_SORT_THREADS = 64;  // one wave per tile list
constexpr int HM_SORT_LDS = 1024;    // longest list sorted in LDS
constexpr int HM_SCAN = 1024;        // tiles per scan segment
static_assert(HM_THREADS == 256 && HM_CHUNK == HM_THREADS, "one staged candidate per thread");
static_assert(HM_TW * 3 + 3 <= HM_TW * 4, "a tile row's bytes plus the misalignment fit one 32-bit word per lane");

struct HmGeo {
    int ntx, nty, nt, nb;   // tiles across / down / in all, scan segments
    long long cap;          // entries the lists can hold: N * (tiles one patch can touch)
};

bool hm_geo(int N, int pw, int ph, int w, int h, HmGeo* g) {
    if (N < 0 || pw < 1 || ph < 1 || w < 1 || h < 1 || w > HIPT_HEATMAP_MAX_DIM || h > HIPT_HEATMAP_MAX_DIM) return false;
    g->ntx = (w + HM_TW - 1) / HM_TW;
    g->nty = (h + HM_TH - 1) / HM_TH;
    const long long nt = (long long)g->ntx * g->nty;
    if (nt > ((long long)1 << 30)) return false;
    g->nt = (int)nt;
    g->nb = (g->nt + HM_SCAN - 1) / HM_SCAN;
    // a clipped run of at most pw pixels touches at most ceil(pw / T) + 1 tiles, and never more than there are
    const long long cx = (long long)(pw - 1) / HM_TW + 2, cy = (long long)(ph - 1) / HM_TH + 2;
    const long long per = (cx < g->ntx ? cx : g->ntx) * (cy < g->nty ? cy : g->nty);
    g->cap = (long long)N * per;
    return g->cap <= 0x7fffffffLL;
}

struct HmWs {
    int *cnt, *cur, *offs, *boff, *entries;
};

// the workspace's five arrays in order.  cnt and cur stay adjacent: hm_run zeroes the two with one memset that ends at offs.
void hm_carve(Carver& c, const HmGeo& g, HmWs& ws) {
    ws.cnt = c.take<int>(g.nt);
    ws.cur = c.take<int>(g.nt);
    ws.offs = c.take<int>(g.nt);
    ws.boff = c.take<int>(g.nb);
    ws.entries = c.take<int>((size_t)g.cap);
}

// the part of patch (x, y) that lies on the canvas, as [x0, x1) x [y0, y1); empty when x1 <= x0 or y1 <= y0
__device__ __forceinline__ int4 hm_clip(int x, int y, int pw, int ph, int w, int h) {
    const long long xe = (long long)x + pw, ye = (long long)y + ph;
    int4 r;
    r.x = min(max(x, 0), w);
    r.y = (int)min(max(xe, 0LL), (long long)w);
    r.z = min(max(y, 0), h);
    r.w = (int)min(max(ye, 0LL), (long long)h);
    return r;
}

// steps 1 and 3: FILL = false counts, FILL = true appends (list start = offs + boff of the tile's segment)
template <bool FILL>
__global__ __launch_bounds__(256) void hm_bin_kernel(const int* __restrict__ xy, int N, int pw, int ph, int w, int h, int ntx,
                                                     int* __restrict__ counter, const int* __restrict__ offs,
                                                     const int* __restrict__ boff, int* __restrict__ entries, long long cap) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int4 r = hm_clip(xy[2 * (size_t)i], xy[2 * (size_t)i + 1], pw, ph, w, h);
    if (r.y <= r.x || r.w <= r.z) return;
    const int tx0 = r.x / HM_TW, tx1 = (r.y - 1) / HM_TW, ty0 = r.z / HM_TH, ty1 = (r.w - 1) / HM_TH;
    for (int ty = ty0; ty <= ty1; ++ty)
        for (int tx = tx0; tx <= tx1; ++tx) {
            const int tile = ty * ntx + tx;
            const int pos = atomicAdd(&counter[tile], 1);
            if (FILL) {
                const long long e = (long long)offs[tile] + boff[tile / HM_SCAN] + pos;
                if (e < cap) entries[e] = i;   // (always: cap is the bound of hm_geo)
            }
        }
}

// step 2a: exclusive scan inside each segment of HM_SCAN tiles, the segment's total to bsum
__global__ __launch_bounds__(HM_SCAN) void hm_scan_local_kernel(const int* __restrict__ cnt, int nt, int* __restrict__ offs,
                                                                int* __restrict__ bsum) {
    __shared__ int wsum[HM_SCAN / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int i = blockIdx.x * HM_SCAN + t;
    const int v = i < nt ? cnt[i] : 0;
    const int incl = wave_incl_scan(v, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int base = 0;
    for (int k = 0; k < wave; ++k) base += wsum[k];
    if (i < nt) offs[i] = base + incl - v;
    if (t == HM_SCAN - 1) bsum[blockIdx.x] = base + incl;
}

// step 2b: exclusive scan of the segment totals, in place, by one workgroup
__global__ __launch_bounds__(HM_SCAN) void hm_scan_blocks_kernel(int* __restrict__ bsum, int nb) {
    __shared__ int wsum[HM_SCAN / 64];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int carry = 0;
    for (int b0 = 0; b0 < nb; b0 += HM_SCAN) {
        const int i = b0 + t;
        const int v = i < nb ? bsum[i] : 0;
        const int incl = wave_incl_scan(v, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        int base = carry, total = 0;
        for (int k = 0; k < HM_SCAN / 64; ++k) {
            if (k < wave) base += wsum[k];
            total += wsum[k];
        }
        if (i < nb) bsum[i] = base + incl - v;
        carry += total;
        __syncthreads();
    }
}

// step 4: ascending order of one tile's list.  The network compares in one direction only (first step of a merge: l against
// its mirror in the block; then halving strides), so a list of any length is sorted as the head of a power-of-two array whose
// missing tail holds +infinity: a comparison whose upper index is past the end is skipped.
__global__ __launch_bounds__(HM_SORT_THREADS) void hm_sort_kernel(const int* __restrict__ cnt, const int* __restrict__ offs,
                                                                  const int* __restrict__ boff, int* __restrict__ entries) {
    __shared__ int lds[HM_SORT_LDS];
    const int tile = blockIdx.x, t = threadIdx.x;
    const int len = cnt[tile];
    if (len < 2) return;
    int* list = entries + offs[tile] + boff[tile / HM_SCAN];
    const bool in_lds = len <= HM_SORT_LDS;
    int* a = in_lds ? lds : list;
    if (in_lds) {
        for (int i = t; i < len; i += HM_SORT_THREADS) lds[i] = list[i];
    }
    __syncthreads();
    int P = 2;
    while (P < len) P <<= 1;
    for (int k = 2; k <= P; k <<= 1) {
        for (int j = k >> 1; j >= 1; j >>= 1) {
            for (int q = t; q < (P >> 1); q += HM_SORT_THREADS) {
                int l, r;
                if (j == (k >> 1)) {
                    const int blk = q / j, off = q - blk * j;
                    l = blk * k + off;
                    r = blk * k + k - 1 - off;
                } else {
                    const int blk = q / j, off = q - blk * j;
                    l = blk * 2 * j + off;
                    r = l + j;
                }
                if (r < len) {
                    const int va = a[l], vb = a[r];
                    if (va > vb) {
                        a[l] = vb;
                        a[r] = va;
                    }
                }
            }
            __syncthreads();
        }
    }
    if (in_lds) {
        for (int i = t; i < len; i += HM_SORT_THREADS) list[i] = lds[i];
    }
}

struct HmPixelArgs {
    const int* xy;
    const double* v;
    const uint8_t* paint;   // NULL: every patch may paint
    int N, pw, ph, w, h, ntx, binarize;
    const int *cnt, *offs, *boff, *entries;   // cnt NULL: no patches at all
    const uint8_t* mask;     // NULL: no mask
    const uint8_t* canvas;   // NULL: white
    const uint8_t* lut;      // [258, 3]; needed with img
    float a, b;              // blend weights of the painted image and of the canvas
    int blend;
    uint8_t* img;            // the outputs: each may be NULL
    double* overlay;
    int* count;
    uint8_t* painted;
};

// step 5
__global__ __launch_bounds__(HM_THREADS) void hm_pixel_kernel(const HmPixelArgs A) {
    __shared__ int4 rect[HM_CHUNK];
    __shared__ double val[HM_CHUNK];
    __shared__ uint8_t pnt[HM_CHUNK];
    __shared__ __attribute__((aligned(4))) uint8_t stage[HM_TH][HM_TW * 4];   // a row's 3 * HM_TW image bytes

    const int tile = blockIdx.x, t = threadIdx.x;
    const int tyi = tile / A.ntx, txi = tile - tyi * A.ntx;
    const int px0 = txi * HM_TW, py0 = tyi * HM_TH;
    const int col = t % HM_TW, row = t / HM_TW;
    const int px = px0 + col, py = py0 + row;
    const bool inside = px < A.w && py < A.h;

    const int len = A.cnt ? A.cnt[tile] : 0;
    const int* list = len ? A.entries + A.offs[tile] + A.boff[tile / HM_SCAN] : nullptr;
    double sum = 0.0;
    int c = 0, any = 0;
    for (int base = 0; base < len; base += HM_CHUNK) {
        const int m = min(HM_CHUNK, len - base);
        if (t < m) {
            const int i = list[base + t];
            int4 r = make_int4(0, 0, 0, 0);
            double vi = 0.0;
            uint8_t p = 0;
            if ((unsigned)i < (unsigned)A.N) {   // (always: the lists hold patch indices)
                r = hm_clip(A.xy[2 * (size_t)i], A.xy[2 * (size_t)i + 1], A.pw, A.ph, A.w, A.h);
                vi = A.v[i];
                p = A.paint ? (A.paint[i] != 0) : 1;
            }
            rect[t] = r;
            val[t] = vi;
            pnt[t] = p;
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const int4 r = rect[k];   // the same address in every lane: a broadcast
            if (px >= r.x && px < r.y && py >= r.z && py < r.w) {
                sum += val[k];
                ++c;
                any |= pnt[k];
            }
        }
        __syncthreads();
    }

    double ov = 0.0;
    if (c) {
        ov = sum / (double)c;
        if (A.binarize) ov = rint(ov);   // np.around: half to even
    }
    if (inside) {
        const size_t p = (size_t)py * A.w + px;
        if (A.overlay) A.overlay[p] = ov;
        if (A.count) A.count[p] = c;
        if (A.painted) A.painted[p] = (uint8_t)any;
    }
    if (!A.img) return;   // (uniform)

    if (inside) {
        const size_t p = (size_t)py * A.w + px;
        uint8_t base[3] = {255, 255, 255}, out[3];
        if (A.canvas) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) base[ch] = A.canvas[p * 3 + ch];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[ch] = base[ch];
        if (any && (!A.mask || A.mask[p])) {
            const double tt = ov * 256.0;
            int idx;
            if (!(tt >= 0.0)) idx = 256;         // under (a NaN, which the host refuses, lands here too)
            else if (tt == 256.0) idx = 255;
            else if (tt > 256.0) idx = 257;      // over
            else idx = (int)tt;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[ch] = A.lut[idx * 3 + ch];
        }
        if (A.blend) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) out[ch] = blend_u8(out[ch], base[ch], A.a, A.b);
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) stage[row][col * 3 + ch] = out[ch];
    }
    __syncthreads();

    // write-out: lane `col` of row `row` owns the aligned 32-bit word number `col` of that row's byte run [g0, g0 + L)
    const int cols = min(HM_TW, A.w - px0);
    if (py < A.h) {
        const int L = cols * 3;
        const size_t g0 = ((size_t)py * A.w + px0) * 3;
        const int mis = (int)(g0 & 3);
        const int s0 = col * 4 - mis;   // offset in the run of this word's first byte
        if (s0 < L && s0 + 4 > 0) {
            uint8_t* dst = A.img + g0 + s0;   // (s0 may be negative: g0 + s0 is the aligned word's address)
            if (s0 >= 0 && s0 + 4 <= L) {
                const uint32_t word = (uint32_t)stage[row][s0] | ((uint32_t)stage[row][s0 + 1] << 8) |
                                      ((uint32_t)stage[row][s0 + 2] << 16) | ((uint32_t)stage[row][s0 + 3] << 24);
                *(uint32_t*)dst = word;
            } else {
                for (int k = 0; k < 4; ++k)
                    if (s0 + k >= 0 && s0 + k < L) dst[k] = stage[row][s0 + k];
            }
        }
    }
}

int hm_run(const int32_t* xy, const double* v, const uint8_t* paint, int N, int pw, int ph, int w, int h, int binarize,
           const uint8_t* mask, const uint8_t* canvas, const uint8_t* lut, double alpha, uint8_t* img, double* overlay, int32_t* count,
           uint8_t* painted, void* workspace, size_t ws_bytes, hipStream_t st, const char* what) {
    HmGeo g;
    if (!hm_geo(N, pw, ph, w, h, &g)) {
        hipt_set_error("%s: N=%d, patch %d x %d, canvas %d x %d outside the envelope (N >= 0, sizes >= 1, canvas side <= %d, "
                       "N * tiles-per-patch < 2^31); nothing was launched", what, N, pw, ph, w, h, HIPT_HEATMAP_MAX_DIM);
        return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_ARG(N == 0 || (xy && v), "%s: xy / v missing", what);
    HIPT_CHECK_ARG(((uintptr_t)xy & 3) == 0 && ((uintptr_t)v & 7) == 0 && ((uintptr_t)overlay & 7) == 0 && ((uintptr_t)count & 3) == 0 &&
                       ((uintptr_t)img & 3) == 0,
                   "%s: xy / count / img need 4-byte, v / overlay 8-byte alignment", what);
    HIPT_CHECK_ARG(!img || lut, "%s: an image needs the colour table", what);
    HmWs ws = {};
    if (N > 0) {
        Carver c(workspace, workspace ? ws_bytes : 0);  // (no buffer holds no bytes: a null workspace is refused like a short one)
        hm_carve(c, g, ws);
        if (int rc = check_workspace(c, what)) return rc;
        if (hipMemsetAsync(ws.cnt, 0, (size_t)((char*)ws.offs - (char*)ws.cnt), st) != hipSuccess) {   // cnt and cur
            hipt_set_error("%s: hipMemsetAsync failed", what);
            return HIPT_E_LAUNCH;
        }
        const dim3 pgrid((unsigned)((N + 255) / 256));
        hipLaunchKernelGGL(hm_bin_kernel<false>, pgrid, dim3(256), 0, st, xy, N, pw, ph, w, h, g.ntx, ws.cnt, (const int*)nullptr,
                           (const int*)nullptr, (int*)nullptr, g.cap);
        HIPT_CHECK_LAUNCH();
        hipLaunchKernelGGL(hm_scan_local_kernel, dim3((unsigned)g.nb), dim3(HM_SCAN), 0, st, (const int*)ws.cnt, g.nt, ws.offs, ws.boff);
        HIPT_CHECK_LAUNCH();
        hipLaunchKernelGGL(hm_scan_blocks_kernel, dim3(1), dim3(HM_SCAN), 0, st, ws.boff, g.nb);
        HIPT_CHECK_LAUNCH();
        hipLaunchKernelGGL(hm_bin_kernel<true>, pgrid, dim3(256), 0, st, xy, N, pw, ph, w, h, g.ntx, ws.cur, (const int*)ws.offs,
                           (const int*)ws.boff, ws.entries, g.cap);
        HIPT_CHECK_LAUNCH();
        hipLaunchKernelGGL(hm_sort_kernel, dim3((unsigned)g.nt), dim3(HM_SORT_THREADS), 0, st, (const int*)ws.cnt, (const int*)ws.offs,
                           (const int*)ws.boff, ws.entries);
        HIPT_CHECK_LAUNCH();
    }
    HmPixelArgs A;
    A.xy = xy;
    A.v = v;
    A.paint = paint;
    A.N = N;
    A.pw = pw;
    A.ph = ph;
    A.w = w;
    A.h = h;
    A.ntx = g.ntx;
    A.binarize = binarize != 0;
    A.cnt = N > 0 ? ws.cnt : nullptr;
    A.offs = ws.offs;
    A.boff = ws.boff;
    A.entries = ws.entries;
    A.mask = mask;
    A.canvas = canvas;
    A.lut = lut;
    A.a = (float)alpha;
    A.b = (float)(1.0 - alpha);
    A.blend = alpha < 1.0;
    A.img = img;
    A.overlay = overlay;
    A.count = count;
    A.painted = painted;
    hipLaunchKernelGGL(hm_pixel_kernel, dim3((unsigned)g.nt), dim3(HM_THREADS), 0, st, A);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

}  // namespace

extern "C" size_t hipt_heatmap_workspace_bytes(int N, int pw, int ph, int w, int h) {
    HmGeo g;
    if (N <= 0 || !hm_geo(N, pw, ph, w, h, &g)) return 0;
    return dry_run([&](Carver& c) { HmWs ws; hm_carve(c, g, ws); });
}

extern "C" int hipt_heatmap_overlay(const int32_t* xy, const double* v, const uint8_t* paint, int N, int pw, int ph, int w, int h,
                                    int binarize, double* overlay, int32_t* count, uint8_t* painted, void* workspace, size_t ws_bytes,
                                    void* stream) {
    HIPT_CHECK_ARG(overlay || count || painted, "heatmap_overlay: no output asked for");
    return hm_run(xy, v, paint, N, pw, ph, w, h, binarize, nullptr, nullptr, nullptr, 1.0, nullptr, overlay, count, painted, workspace,
                  ws_bytes, (hipStream_t)stream, "heatmap_overlay");
}

extern "C" int hipt_heatmap_render(const int32_t* xy, const double* v, const uint8_t* paint, int N, int pw, int ph, int w, int h,
                                   int binarize, const uint8_t* mask, const uint8_t* canvas, const uint8_t* lut, double alpha, uint8_t* img,
                                   double* overlay, void* workspace, size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(img && lut, "heatmap_render: img / lut missing");
    HIPT_CHECK_ARG(alpha == alpha, "heatmap_render: alpha is NaN");
    HIPT_CHECK_ARG(canvas != img, "heatmap_render: the canvas cannot be the output image");
    return hm_run(xy, v, paint, N, pw, ph, w, h, binarize, mask, canvas, lut, alpha, img, overlay, nullptr, nullptr, workspace, ws_bytes,
                  (hipStream_t)stream, "heatmap_render");
}
