// The pixel stages of WholeSlideImage.segmentTissue (wsi_core/WholeSlideImage.py:111-203) up to the binary mask; DESIGN.md 26,
// include/hipt_abmil.h.  cv2's calls are restated from OpenCV's published implementation, all in 8-bit integers:
//   saturation  cvtColor(RGB2HSV)[:, :, 1]:  v = max(r, g, b), d = v - min(r, g, b), S = (d * sdiv[v] + 2048) >> 12,
//               sdiv[0] = 0, sdiv[v] = rint(255 * 4096 / v)
//   median      medianBlur(S, k): the exact median of the k x k window, indices clamped (replicated border), k odd, 1 .. 15
//   Otsu        a 256-bin histogram of the median plane, then OpenCV's float64 scan, by ONE thread, in OpenCV's order
//   threshold   med > t ? maxval : 0
//   closing     morphologyEx(MORPH_CLOSE, ones((c, c))): dilate, then erode, anchor c / 2, separable (rows, then columns);
//               outside the image counts 0 for the dilation and 255 for the erosion
// Three kernels.  seg_median_kernel reads the source ONCE: a workgroup forms the saturation of its 64 x 32 tile plus halo in LDS
// (the plane goes to memory only when asked for), takes every output's median by an 8-step bitwise select over the LDS window --
// the median is the largest v with #{x < v} <= k k / 2 -- and adds its part of the histogram (LDS atomics, then one global integer
// atomic per non-empty bin).  seg_otsu_kernel is the scan.  seg_morph_kernel is one pass of a c x 1 or 1 x c window out of an LDS
// tile; the first pass thresholds what it loads, the passes ping-pong between two workspace planes and the last one writes the
// mask.  Integer atomics only (their order cannot show), no allocation, no synchronisation with the host.
#include <float.h>

#include "common.h"
#include "workspace.h"

namespace {

constexpr int SG_THREADS = 256;
constexpr int SG_MAX_K = HIPT_SEGMENT_MAX_MEDIAN, SG_MAX_CLOSE = HIPT_SEGMENT_MAX_CLOSE;
// median tile: 64 x 32 outputs, 4 adjacent outputs per item; LDS rows of 80 bytes hold 64 + 14 columns (the dword reads of the
// last item end at byte 80)
constexpr int MD_TW = 64, MD_TH = 32, MD_STRIDE = 80, MD_ROWS = MD_TH + SG_MAX_K - 1;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sdiv[v] = rint(255 * 4096 / v), half to even, in integers: the quotient's fraction is a multiple of 1 / v, v <= 255, so the float64
// quotient is never close enough to a half to round the other way
__device__ __forceinline__ uint32_t sdiv_of(uint32_t v) {
    if (v == 0) return 0;
    const uint32_t n = 255u << 12, q = n / v, r = n - q * v;
    return 2 * r > v ? q + 1 : (2 * r == v ? q + (q & 1) : q);
}

// four bytes to p: one 32-bit store where the address allows it and all four are inside the row
__device__ __forceinline__ void store4_u8(uint8_t* p, const uint32_t v[4], int valid) {
    if (valid == 4 && ((uintptr_t)p & 3) == 0) {
        *(uint32_t*)p = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < valid) p[j] = (uint8_t)v[j];
    }
}

// channels = 3 / 4: src is the interleaved image and the tile holds its saturation; channels = 1: src is a plane, taken as it is.
// sat, med, hist: NULL = not wanted.
template <int K>
__global__ __launch_bounds__(SG_THREADS) void seg_median_kernel(const uint8_t* __restrict__ src, int H, int W, int channels,
                                                                uint8_t* __restrict__ sat, uint8_t* __restrict__ med,
                                                                int32_t* __restrict__ hist, int tiles_x) {
    __shared__ __attribute__((aligned(16))) uint8_t tile[MD_ROWS * MD_STRIDE];
    __shared__ uint32_t sdiv[256];
    __shared__ int32_t lhist[256];
    constexpr int R = K / 2, RANK = (K * K) / 2, NDW = (K + 3 + 3) / 4;
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)tiles_x) * MD_TW, y0 = (int)(blockIdx.x / (unsigned)tiles_x) * MD_TH;
    sdiv[tid] = sdiv_of((uint32_t)tid);
    lhist[tid] = 0;
    __syncthreads();
    // 1. the tile plus halo, indices clamped to the image
    constexpr int LW = MD_TW + K - 1, LH = MD_TH + K - 1;
    const bool word_px = channels == 4 && ((uintptr_t)src & 3) == 0;
    for (int i = tid; i < LW * LH; i += SG_THREADS) {
        const int ly = i / LW, lx = i - ly * LW;
        const int gy = clampi(y0 - R + ly, 0, H - 1), gx = clampi(x0 - R + lx, 0, W - 1);
        const size_t px = (size_t)gy * (size_t)W + (size_t)gx;
        uint32_t s;
        if (channels == 1) {
            s = src[px];
        } else {
            uint32_t r, g, b;
            if (word_px) {
                const uint32_t q = *(const uint32_t*)(src + 4 * px);
                r = q & 255u, g = (q >> 8) & 255u, b = (q >> 16) & 255u;
            } else {
                const uint8_t* p = src + (size_t)channels * px;
                r = p[0], g = p[1], b = p[2];
            }
            const uint32_t v = max(r, max(g, b)), d = v - min(r, min(g, b));
            s = (d * sdiv[v] + 2048u) >> 12;
        }
        tile[ly * MD_STRIDE + lx] = (uint8_t)s;
    }
    __syncthreads();
    // 2. four adjacent outputs per item
    for (int it = tid; it < (MD_TW / 4) * MD_TH; it += SG_THREADS) {
        const int yl = it / (MD_TW / 4), xl = (it - yl * (MD_TW / 4)) * 4;
        const int gy = y0 + yl, gx = x0 + xl;
        if (gy >= H || gx >= W) continue;
        const int valid = min(4, W - gx);
        const size_t o = (size_t)gy * (size_t)W + (size_t)gx;
        if (sat != nullptr) {
            uint32_t c[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) c[j] = tile[(yl + R) * MD_STRIDE + xl + R + j];
            store4_u8(sat + o, c, valid);
        }
        if (med == nullptr && hist == nullptr) continue;
        uint32_t cand[4] = {0, 0, 0, 0};
        if (K == 1) {
#pragma unroll
            for (int j = 0; j < 4; ++j) cand[j] = tile[yl * MD_STRIDE + xl + j];
        } else {
#pragma unroll 1
            for (int bit = 7; bit >= 0; --bit) {
                uint32_t t[4], cnt[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) t[j] = cand[j] | (1u << bit), cnt[j] = 0;
#pragma unroll 1
                for (int wy = 0; wy < K; ++wy) {
                    const uint32_t* row = (const uint32_t*)(tile + (yl + wy) * MD_STRIDE + xl);   // xl and the stride are multiples of 4
                    uint32_t w[NDW];
#pragma unroll
                    for (int q = 0; q < NDW; ++q) w[q] = row[q];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < K; ++i) cnt[j] += ((w[(j + i) >> 2] >> (8 * ((j + i) & 3))) & 255u) < t[j] ? 1u : 0u;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (cnt[j] <= (uint32_t)RANK) cand[j] = t[j];
            }
        }
        if (med != nullptr) store4_u8(med + o, cand, valid);
        if (hist != nullptr) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < valid) atomicAdd(&lhist[cand[j]], 1);
        }
    }
    if (hist != nullptr) {
        __syncthreads();
        if (lhist[tid] != 0) atomicAdd(&hist[tid], lhist[tid]);
    }
}

__global__ void seg_zero_kernel(int32_t* hist) { hist[threadIdx.x] = 0; }

// OpenCV's getThreshVal_Otsu_8u scan over the finished histogram, by thread 0, every operation rounded on its own (the file is built
// with -ffp-contract=off).  use_otsu = 0 only records the fixed threshold.
__global__ void seg_otsu_kernel(const int32_t* __restrict__ hist, double npix, int use_otsu, int fixed, int32_t* __restrict__ thresh) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (!use_otsu) {
        *thresh = fixed;
        return;
    }
    const double scale = 1.0 / npix;
    long long s = 0;
    for (int i = 0; i < 256; ++i) s += (long long)i * (long long)hist[i];
    const double mu = (double)s * scale;
    double mu1 = 0.0, q1 = 0.0, max_sigma = 0.0;
    int best = 0;
    const double eps = (double)FLT_EPSILON;
    for (int i = 0; i < 256; ++i) {
        const double p = (double)hist[i] * scale;
        mu1 *= q1;
        q1 += p;
        const double q2 = 1.0 - q1;
        if (fmin(q1, q2) < eps || fmax(q1, q2) > 1.0 - eps) continue;
        mu1 = (mu1 + (double)i * p) / q1;
        const double mu2 = (mu - q1 * mu1) / q2;
        const double d = mu1 - mu2;
        const double sigma = q1 * q2 * d * d;
        if (sigma > max_sigma) {
            max_sigma = sigma;
            best = i;
        }
    }
    *thresh = best;
}

struct MorphArgs {
    const uint8_t* src;
    uint8_t* dst;
    int H, W;
    int cw, ch;           // the window: c x 1 or 1 x c
    int TW, TH, stride;   // outputs per tile; LDS row bytes: a multiple of 4, >= TW + cw - 1
    int tiles_x;
    int do_thresh, tval, maxval;   // the first pass: what is loaded is src > t ? maxval : 0
    const int32_t* tptr;           // t on the device (Otsu), or NULL: tval
};

// One pass of a grey-scale dilation (ERODE = false: max, outside = 0) or erosion (min, outside = 255): output (y, x) is taken over
// the inputs (y - ay + i, x - ax + j), i < ch, j < cw, with the anchor c / 2 on the window's axis and 0 on the other.
template <bool ERODE>
__global__ __launch_bounds__(SG_THREADS) void seg_morph_kernel(const MorphArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mtile[];
    constexpr uint32_t BORDER = ERODE ? 255u : 0u;
    auto op = [](uint32_t a, uint32_t b) { return ERODE ? min(a, b) : max(a, b); };
    const int tid = threadIdx.x;
    const int x0 = (int)(blockIdx.x % (unsigned)A.tiles_x) * A.TW, y0 = (int)(blockIdx.x / (unsigned)A.tiles_x) * A.TH;
    const int ax = A.cw / 2, ay = A.ch / 2;   // (1 / 2 = 0 on the axis without a window)
    const int rows = A.TH + A.ch - 1;
    const int t = A.do_thresh ? (A.tptr != nullptr ? *A.tptr : A.tval) : 0;
    for (int i = tid; i < rows * A.stride; i += SG_THREADS) {
        const int ly = i / A.stride, lx = i - ly * A.stride;
        const int gy = y0 - ay + ly, gx = x0 - ax + lx;
        uint32_t v = BORDER;
        if (gy >= 0 && gy < A.H && gx >= 0 && gx < A.W) {
            v = A.src[(size_t)gy * (size_t)A.W + (size_t)gx];
            if (A.do_thresh) v = (int)v > t ? (uint32_t)A.maxval : 0u;
        }
        mtile[i] = (uint8_t)v;
    }
    __syncthreads();
    const int groups = A.TW >> 2;
    for (int it = tid; it < groups * A.TH; it += SG_THREADS) {
        const int yl = it / groups, xl = (it - yl * groups) * 4;
        const int gy = y0 + yl, gx = x0 + xl;
        if (gy >= A.H || gx >= A.W) continue;
        uint32_t acc[4];
        if (A.cw == 1) {   // columns: one dword per window row
            uint32_t a0 = BORDER, a1 = BORDER, a2 = BORDER, a3 = BORDER;
            for (int wy = 0; wy < A.ch; ++wy) {
                const uint32_t w = *(const uint32_t*)(mtile + (yl + wy) * A.stride + xl);
                a0 = op(a0, w & 255u), a1 = op(a1, (w >> 8) & 255u), a2 = op(a2, (w >> 16) & 255u), a3 = op(a3, w >> 24);
            }
            acc[0] = a0, acc[1] = a1, acc[2] = a2, acc[3] = a3;
        } else {   // rows: output j takes bytes [j, j + cw); bytes [3, cw) belong to all four
            const uint8_t* row = mtile + yl * A.stride + xl;
            uint32_t common = BORDER;
            for (int i = 3; i < A.cw; ++i) common = op(common, row[i]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t a = common;
                for (int i = j; i < min(3, j + A.cw); ++i) a = op(a, row[i]);
                for (int i = max(A.cw, 3); i < j + A.cw; ++i) a = op(a, row[i]);
                acc[j] = a;
            }
        }
        store4_u8(A.dst + (size_t)gy * (size_t)A.W + (size_t)gx, acc, min(4, A.W - gx));
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------
struct SegScratch {
    int32_t *hist, *thresh;
    uint8_t *med, *p0, *p1;
};

// the ONE layout: histogram, threshold, the median plane, and the closing's two planes when there is a closing
SegScratch carve_segment(Carver& c, int h, int w, int close) {
    SegScratch s = {};
    const size_t n = (size_t)h * (size_t)w;
    s.hist = c.take<int32_t>(256);
    s.thresh = c.take<int32_t>(1);
    s.med = c.take<uint8_t>(n);
    if (close > 0) {
        s.p0 = c.take<uint8_t>(n);
        s.p1 = c.take<uint8_t>(n);
    }
    return s;
}

bool plane_ok(int h, int w) { return h >= 1 && w >= 1 && (long long)h * (long long)w < (1LL << 31); }

int launch_median(const uint8_t* src, int h, int w, int channels, int k, uint8_t* sat, uint8_t* med, int32_t* hist, hipStream_t st) {
    const int tiles_x = (w + MD_TW - 1) / MD_TW, tiles_y = (h + MD_TH - 1) / MD_TH;
    const dim3 grid((unsigned)((long long)tiles_x * tiles_y)), block(SG_THREADS);
    switch (k) {
#define SG_CASE(K) \
    case K: hipLaunchKernelGGL(seg_median_kernel<K>, grid, block, 0, st, src, h, w, channels, sat, med, hist, tiles_x); break
        SG_CASE(1);
        SG_CASE(3);
        SG_CASE(5);
        SG_CASE(7);
        SG_CASE(9);
        SG_CASE(11);
        SG_CASE(13);
        SG_CASE(15);
#undef SG_CASE
        default: hipt_set_error("segment: median window %d", k); return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

// one pass; c on the row axis (horizontal = true) or the column axis
int launch_morph(const uint8_t* src, uint8_t* dst, int h, int w, int c, bool horizontal, bool erode, int do_thresh, int tval, int maxval,
                 const int32_t* tptr, hipStream_t st) {
    MorphArgs A = {};
    A.src = src, A.dst = dst, A.H = h, A.W = w;
    A.cw = horizontal ? c : 1, A.ch = horizontal ? 1 : c;
    A.TW = horizontal ? 256 : 64, A.TH = horizontal ? 8 : 64;
    A.stride = (A.TW + A.cw - 1 + 3) & ~3;
    A.tiles_x = (w + A.TW - 1) / A.TW;
    A.do_thresh = do_thresh, A.tval = tval, A.maxval = maxval, A.tptr = tptr;
    const long long blocks = (long long)A.tiles_x * ((h + A.TH - 1) / A.TH);
    const size_t lds = (size_t)(A.TH + A.ch - 1) * A.stride;   // at most 191 * 64 or 8 * 384 bytes
    if (erode)
        hipLaunchKernelGGL(seg_morph_kernel<true>, dim3((unsigned)blocks), dim3(SG_THREADS), lds, st, A);
    else
        hipLaunchKernelGGL(seg_morph_kernel<false>, dim3((unsigned)blocks), dim3(SG_THREADS), lds, st, A);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

// threshold (where asked) + closing of `src` into `dst` through the two planes; close = 0: the threshold alone (or a copy)
int run_close(const uint8_t* src, uint8_t* dst, int h, int w, int close, int do_thresh, int tval, int maxval, const int32_t* tptr,
              uint8_t* p0, uint8_t* p1, hipStream_t st) {
    if (close == 0) return launch_morph(src, dst, h, w, 1, true, false, do_thresh, tval, maxval, tptr, st);
    if (int rc = launch_morph(src, p0, h, w, close, true, false, do_thresh, tval, maxval, tptr, st)) return rc;
    if (int rc = launch_morph(p0, p1, h, w, close, false, false, 0, 0, 0, nullptr, st)) return rc;
    if (int rc = launch_morph(p1, p0, h, w, close, true, true, 0, 0, 0, nullptr, st)) return rc;
    return launch_morph(p0, dst, h, w, close, false, true, 0, 0, 0, nullptr, st);
}

int check_median(int mthresh) {
    HIPT_CHECK_ARG(mthresh >= 1, "segment: median window %d", mthresh);
    if (mthresh % 2 == 0 || mthresh > SG_MAX_K) {
        hipt_set_error("segment: median window %d: the kernels take odd windows up to %d; nothing was launched", mthresh, SG_MAX_K);
        return HIPT_E_UNSUPPORTED;
    }
    return HIPT_OK;
}

int check_close(int close) {
    HIPT_CHECK_ARG(close >= 0, "segment: closing window %d", close);
    if (close > SG_MAX_CLOSE) {
        hipt_set_error("segment: closing window %d: the kernels take up to %d; nothing was launched", close, SG_MAX_CLOSE);
        return HIPT_E_UNSUPPORTED;
    }
    return HIPT_OK;
}

}  // namespace

extern "C" size_t hipt_segment_workspace_bytes(int h, int w, int close) {
    if (!plane_ok(h, w) || close < 0 || close > SG_MAX_CLOSE) return 0;
    return dry_run([&](Carver& c) { carve_segment(c, h, w, close); });
}

extern "C" int hipt_segment_saturation(const uint8_t* src, int h, int w, int channels, uint8_t* sat, void* stream) {
    HIPT_CHECK_ARG(plane_ok(h, w), "segment: image of %d x %d (h w must be below 2^31)", h, w);
    HIPT_CHECK_ARG(channels == 3 || channels == 4, "segment: %d channels (3 or 4)", channels);
    HIPT_CHECK_ARG(src && sat && src != sat, "segment: src / sat missing, or the same");
    return launch_median(src, h, w, channels, 1, sat, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int hipt_segment_median(const uint8_t* src, int h, int w, int ksize, uint8_t* dst, void* stream) {
    HIPT_CHECK_ARG(plane_ok(h, w), "segment: plane of %d x %d (h w must be below 2^31)", h, w);
    HIPT_CHECK_ARG(src && dst && src != dst, "segment: src / dst missing, or the same");
    if (int rc = check_median(ksize)) return rc;
    return launch_median(src, h, w, 1, ksize, nullptr, dst, nullptr, (hipStream_t)stream);
}

extern "C" int hipt_segment_otsu(const uint8_t* src, int h, int w, int32_t* hist, int32_t* thresh, void* stream) {
    HIPT_CHECK_ARG(plane_ok(h, w), "segment: plane of %d x %d (h w must be below 2^31)", h, w);
    HIPT_CHECK_ARG(src && hist && thresh, "segment: src / hist / thresh missing");
    HIPT_CHECK_ARG((((uintptr_t)hist | (uintptr_t)thresh) & 3) == 0, "segment: hist / thresh need 4-byte alignment");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(seg_zero_kernel, dim3(1), dim3(256), 0, st, hist);
    HIPT_CHECK_LAUNCH();
    if (int rc = launch_median(src, h, w, 1, 1, nullptr, nullptr, hist, st)) return rc;
    hipLaunchKernelGGL(seg_otsu_kernel, dim3(1), dim3(64), 0, st, hist, (double)h * (double)w, 1, 0, thresh);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

extern "C" int hipt_segment_close(const uint8_t* src, int h, int w, int close, uint8_t* dst, void* ws, size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(plane_ok(h, w), "segment: plane of %d x %d (h w must be below 2^31)", h, w);
    HIPT_CHECK_ARG(src && dst && src != dst, "segment: src / dst missing, or the same");
    if (int rc = check_close(close)) return rc;
    Carver c(ws, ws_bytes);
    const SegScratch s = carve_segment(c, h, w, close);
    if (int rc = check_workspace(c, "hipt_segment_close")) return rc;
    HIPT_CHECK_ARG(ws != nullptr, "segment: the workspace is missing");
    return run_close(src, dst, h, w, close, 0, 0, 0, nullptr, s.p0, s.p1, (hipStream_t)stream);
}

extern "C" int hipt_segment_mask(const uint8_t* src, int h, int w, int channels, int sthresh, int sthresh_up, int mthresh, int close,
                                 int use_otsu, uint8_t* mask, uint8_t* sat, uint8_t* med, int32_t* thresh, void* ws, size_t ws_bytes,
                                 void* stream) {
    HIPT_CHECK_ARG(plane_ok(h, w), "segment: image of %d x %d (h w must be below 2^31)", h, w);
    HIPT_CHECK_ARG(channels == 3 || channels == 4, "segment: %d channels (3 or 4)", channels);
    HIPT_CHECK_ARG(sthresh >= 0 && sthresh <= 255 && sthresh_up >= 0 && sthresh_up <= 255, "segment: sthresh %d / sthresh_up %d outside 0 .. 255",
                   sthresh, sthresh_up);
    HIPT_CHECK_ARG(src && mask && mask != src && mask != sat && mask != med && (sat == nullptr || sat != med),
                   "segment: src / mask missing, or two of the buffers are the same");
    HIPT_CHECK_ARG(((uintptr_t)thresh & 3) == 0, "segment: thresh needs 4-byte alignment");
    if (int rc = check_median(mthresh)) return rc;
    if (int rc = check_close(close)) return rc;
    Carver c(ws, ws_bytes);
    const SegScratch s = carve_segment(c, h, w, close);
    if (int rc = check_workspace(c, "hipt_segment_mask")) return rc;
    HIPT_CHECK_ARG(ws != nullptr, "segment: the workspace is missing");
    hipStream_t st = (hipStream_t)stream;
    uint8_t* m = med != nullptr ? med : s.med;
    int32_t* t = thresh != nullptr ? thresh : s.thresh;
    if (use_otsu) {
        hipLaunchKernelGGL(seg_zero_kernel, dim3(1), dim3(256), 0, st, s.hist);
        HIPT_CHECK_LAUNCH();
    }
    if (int rc = launch_median(src, h, w, channels, mthresh, sat, m, use_otsu ? s.hist : nullptr, st)) return rc;
    if (use_otsu || thresh != nullptr) {
        hipLaunchKernelGGL(seg_otsu_kernel, dim3(1), dim3(64), 0, st, s.hist, (double)h * (double)w, use_otsu ? 1 : 0, sthresh, t);
        HIPT_CHECK_LAUNCH();
    }
    return run_close(m, mask, h, w, close, 1, sthresh, sthresh_up, use_otsu ? t : nullptr, s.p0, s.p1, st);
}
