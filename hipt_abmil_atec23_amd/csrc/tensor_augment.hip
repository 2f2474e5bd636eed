// Tensor-space region augmentation (extract_features_fp.py:63-82, --use_transforms all / spatial): uint8 RGB regions in,
// normalised float32 planar regions out, one parameter record per region (include/hipt_abmil.h: hipt_tensor_augment_params;
// DESIGN.md 28 states the arithmetic).  The reference's Compose puts ToTensor first, so every step is torchvision's TENSOR
// code in float32: u8 / 255, flips, the affine as a normalised grid read through grid_sample(nearest, zeros,
// align_corners=False), ColorJitter's float blends and float HSV round trip, Normalize.
//
// A thread owns 4 consecutive output pixels in the region's row-major order (one 16-byte store per plane; a wave writes 1 KiB
// per plane and instruction); a 256-thread workgroup covers chunks of 1024 pixels.  The reads are a gather: they fall where
// the affine puts them.  Contrast blends against the mean grey of the whole region as it is at that step, so a call whose
// records hold a contrast op takes two passes: pass A runs the chain up to the contrast op and leaves one float64 partial sum
// per workgroup in the workspace; pass B sums a region's partials in a fixed tree, recomputes the chain from the uint8 source
// and finishes it.  No float intermediate is stored, no atomics: the same bits from run to run and for any batch.
//
// torch rounds every operation on its own: this file is compiled without FMA contraction.
#include "common.h"
#include "workspace.h"

#pragma clang fp contract(off)

namespace {

constexpr int TA_PX = 4;                        // output pixels per thread
constexpr int TA_THREADS = 256;
constexpr int TA_CHUNK = TA_PX * TA_THREADS;    // pixels per workgroup and step
constexpr int TA_MAX_PARTS = TA_THREADS;        // workgroups per region at most: pass B reads one partial per thread
enum { TA_SINGLE = 0, TA_SUM = 1, TA_FINISH = 2 };

typedef hipt_tensor_augment_params TaParams;

struct TaGeo {
    int rows, cols;
    int npix;     // rows * cols (<= 2^30)
    int chunks;   // ceil(npix / TA_CHUNK)
    int parts;    // workgroups per region = min(chunks, TA_MAX_PARTS)
};

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// torchvision rgb_to_grayscale on a float tensor
__device__ __forceinline__ float gray(float r, float g, float b) { return (0.2989f * r + 0.587f * g) + 0.114f * b; }

// torchvision _blend: (ratio * img1 + (1.0 - ratio) * img2).clamp(0, 1); 1.0 - ratio is exact in double, so its float32 value
// is the float32 difference
__device__ __forceinline__ float blend(float a, float b, float ratio) { return clamp01(ratio * a + (1.0f - ratio) * b); }

// torchvision adjust_hue on a float tensor: _rgb2hsv, h = (h + hue) % 1.0, _hsv2rgb
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float hue) {
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eq = maxc == minc;
    const float cr = maxc - minc;
    const float s = __fdiv_rn(cr, eq ? 1.0f : maxc);
    const float div = eq ? 1.0f : cr;
    const float rc = __fdiv_rn(maxc - r, div), gc = __fdiv_rn(maxc - g, div), bc = __fdiv_rn(maxc - b, div);
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = (2.0f + rc) - bc;
    else h = (4.0f + gc) - rc;
    h = __fdiv_rn(h, 6.0f) + 1.0f;
    h = h - truncf(h);                     // fmod(h, 1.0) of a positive h: exact
    h = h + hue;
    h = h - truncf(h);                     // torch's remainder: fmod, then + 1.0 where the sign differs from the divisor's
    if (h < 0.0f) h = h + 1.0f;
    const float h6 = h * 6.0f;
    const float fl = floorf(h6);
    const float f = h6 - fl;
    const int i = ((int)fl) % 6;           // (h may round up to 1.0: sector 6 is sector 0)
    const float v = maxc;
    const float p = clamp01(v * (1.0f - s));
    const float q = clamp01(v * (1.0f - s * f));
    const float t = clamp01(v * (1.0f - s * (1.0f - f)));
    switch (i) {
        case 0: r = v; g = t; b = p; break;
        case 1: r = q; g = v; b = p; break;
        case 2: r = p; g = v; b = t; break;
        case 3: r = p; g = q; b = v; break;
        case 4: r = t; g = p; b = v; break;
        default: r = v; g = p; b = q; break;
    }
}

// index of the contrast op in the record's order, or -1
__device__ __forceinline__ int contrast_at(const TaParams& p) {
    for (int k = 0; k < p.n_ops && k < 4; ++k)
        if (p.ops[k] == HIPT_AUG_CONTRAST) return k;
    return -1;
}

// the record's colour ops k0 .. k1-1 on one pixel; contrast blends against `mean`
__device__ __forceinline__ void colour(float& r, float& g, float& b, const TaParams& p, int k0, int k1, float mean) {
    for (int k = k0; k < k1; ++k) {
        const int op = p.ops[k];
        if (op == HIPT_AUG_BRIGHTNESS) {
            const float f = p.factor[0];
            r = blend(r, 0.0f, f); g = blend(g, 0.0f, f); b = blend(b, 0.0f, f);
        } else if (op == HIPT_AUG_CONTRAST) {
            const float f = p.factor[1];
            r = blend(r, mean, f); g = blend(g, mean, f); b = blend(b, mean, f);
        } else if (op == HIPT_AUG_SATURATION) {
            const float f = p.factor[2], l = gray(r, g, b);
            r = blend(r, l, f); g = blend(g, l, f); b = blend(b, l, f);
        } else if (op == HIPT_AUG_HUE) {
            hue_shift(r, g, b, p.hue);
        }
    }
}

// ToTensor of the source pixel that output pixel (x, y) reads: flips first (they act on the source), then the affine's grid
// (torchvision _gen_affine_grid) and grid_sample(nearest, zeros, align_corners=False).  rt: theta / [0.5 cols, 0.5 rows].
// Nothing is loaded unless the source index has passed the in-range test of ITS region.
template <bool IL>
__device__ __forceinline__ void fetch(const uint8_t* __restrict__ src, const TaGeo& G, const TaParams& p, const float (&rt)[6], int x, int y,
                                      float& r, float& g, float& b) {
    int xi = x, yi = y;
    bool in = true;
    if (p.flags & HIPT_AUG_AFFINE) {
        const float bx = (float)x + (0.5f - 0.5f * (float)G.cols), by = (float)y + (0.5f - 0.5f * (float)G.rows);  // linspace: exact
        const float gx = (bx * rt[0] + by * rt[1]) + rt[2], gy = (bx * rt[3] + by * rt[4]) + rt[5];
        const float fx = rintf(((gx + 1.0f) * (float)G.cols - 1.0f) * 0.5f), fy = rintf(((gy + 1.0f) * (float)G.rows - 1.0f) * 0.5f);
        in = fx >= 0.0f && fx <= (float)(G.cols - 1) && fy >= 0.0f && fy <= (float)(G.rows - 1);   // (a NaN is out of range)
        xi = in ? (int)fx : 0;
        yi = in ? (int)fy : 0;
    }
    r = g = b = 0.0f;
    if (in) {
        const int sx = (p.flags & HIPT_AUG_HFLIP) ? G.cols - 1 - xi : xi, sy = (p.flags & HIPT_AUG_VFLIP) ? G.rows - 1 - yi : yi;
        const int o = sy * G.cols + sx;   // 0 .. npix - 1
        uint8_t ur, ug, ub;
        if (IL) {
            const uint8_t* q = src + (size_t)o * 3;
            ur = q[0]; ug = q[1]; ub = q[2];
        } else {
            ur = src[o]; ug = src[(size_t)o + G.npix]; ub = src[(size_t)o + 2 * (size_t)G.npix];
        }
        r = __fdiv_rn((float)ur, 255.0f); g = __fdiv_rn((float)ug, 255.0f); b = __fdiv_rn((float)ub, 255.0f);
    }
}

// the sum of a workgroup's values, the same in every thread; a fixed tree: the same bits whatever runs beside it
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll  // (wave_sum of common.h, written out: on a double the call compiles to different code)
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

// MODE TA_SINGLE: the whole chain in one pass (the caller states that no record holds a contrast op; a record that does gets NaN)
//      TA_SUM:    pass A -- the chain up to the contrast op, grey summed into partials[region][workgroup]
//      TA_FINISH: pass B -- the mean from the partials, then the whole chain
// grid: n * G.parts workgroups; workgroup g of a region takes its chunks g, g + parts, ...
template <bool IL, int MODE>
__global__ __launch_bounds__(TA_THREADS) void ta_kernel(const uint8_t* __restrict__ src, TaGeo G, const TaParams* __restrict__ prm,
                                                        double* __restrict__ partials, float* __restrict__ dst, int vec) {
    __shared__ double lds[TA_THREADS / 64];
    const int r = blockIdx.x / G.parts, g = blockIdx.x - r * G.parts;
    const TaParams& p = prm[r];
    const int n_ops = min(max(p.n_ops, 0), 4);
    const int cpos = contrast_at(p);
    if (MODE == TA_SUM && cpos < 0) return;   // (uniform over the workgroup)
    float mean = 0.0f;
    if (MODE == TA_FINISH && cpos >= 0) {
        const double part = (int)threadIdx.x < G.parts ? partials[(size_t)r * G.parts + threadIdx.x] : 0.0;
        mean = (float)(block_sum(part, lds) / (double)G.npix);
    }
    const bool poison = MODE == TA_SINGLE && cpos >= 0;
    const float hw = 0.5f * (float)G.cols, hh = 0.5f * (float)G.rows;
    const float rt[6] = {__fdiv_rn(p.theta[0], hw), __fdiv_rn(p.theta[1], hw), __fdiv_rn(p.theta[2], hw),
                         __fdiv_rn(p.theta[3], hh), __fdiv_rn(p.theta[4], hh), __fdiv_rn(p.theta[5], hh)};
    const uint8_t* s = src + (size_t)r * 3 * G.npix;
    float* d = dst + (size_t)r * 3 * G.npix;
    double acc = 0.0;
    for (int chunk = g; chunk < G.chunks; chunk += G.parts) {
        const int i0 = chunk * TA_CHUNK + (int)threadIdx.x * TA_PX;
        if (i0 >= G.npix) continue;
        int y = i0 / G.cols, x = i0 - y * G.cols;
        float R[TA_PX], Gc[TA_PX], B[TA_PX];
#pragma unroll
        for (int j = 0; j < TA_PX; ++j) {
            R[j] = Gc[j] = B[j] = 0.0f;
            if (i0 + j < G.npix) {
                fetch<IL>(s, G, p, rt, x, y, R[j], Gc[j], B[j]);
                if (MODE == TA_SUM) {
                    colour(R[j], Gc[j], B[j], p, 0, cpos, 0.0f);
                    acc += (double)gray(R[j], Gc[j], B[j]);
                } else {
                    colour(R[j], Gc[j], B[j], p, 0, n_ops, mean);
                    R[j] = __fdiv_rn(R[j] - p.mean[0], p.std[0]);
                    Gc[j] = __fdiv_rn(Gc[j] - p.mean[1], p.std[1]);
                    B[j] = __fdiv_rn(B[j] - p.mean[2], p.std[2]);
                    if (poison) R[j] = Gc[j] = B[j] = __builtin_nanf("");
                }
            }
            if (++x == G.cols) { x = 0; ++y; }
        }
        if (MODE == TA_SUM) continue;
        if (vec) {   // npix % 4 == 0 and a 16-byte aligned dst: all four pixels exist and every plane's store is aligned
            *(f32x4*)(d + i0) = f32x4{R[0], R[1], R[2], R[3]};
            *(f32x4*)(d + (size_t)G.npix + i0) = f32x4{Gc[0], Gc[1], Gc[2], Gc[3]};
            *(f32x4*)(d + 2 * (size_t)G.npix + i0) = f32x4{B[0], B[1], B[2], B[3]};
        } else {
#pragma unroll
            for (int j = 0; j < TA_PX; ++j)
                if (i0 + j < G.npix) {
                    d[i0 + j] = R[j]; d[(size_t)G.npix + i0 + j] = Gc[j]; d[2 * (size_t)G.npix + i0 + j] = B[j];
                }
        }
    }
    if (MODE == TA_SUM) {
        const double t = block_sum(acc, lds);
        if (threadIdx.x == 0) partials[(size_t)r * G.parts + g] = t;
    }
}

TaGeo geometry(int rows, int cols) {
    TaGeo G;
    G.rows = rows; G.cols = cols;
    G.npix = rows * cols;
    G.chunks = (G.npix + TA_CHUNK - 1) / TA_CHUNK;
    G.parts = G.chunks < TA_MAX_PARTS ? G.chunks : TA_MAX_PARTS;
    return G;
}

bool in_envelope(int n, int rows, int cols) {
    return n >= 1 && rows >= 1 && cols >= 1 && (int64_t)rows * cols <= ((int64_t)1 << 30) &&
           (int64_t)n * geometry(rows, cols).parts < ((int64_t)1 << 31);
}

// the workspace: one float64 partial per workgroup of pass A
double* carve_tensor_augment(Carver& c, int n, const TaGeo& G) { return c.take<double>((size_t)n * G.parts); }

template <int MODE>
void launch(bool il, const uint8_t* src, const TaGeo& G, int n, const TaParams* prm, double* partials, float* dst, int vec, hipStream_t st) {
    const dim3 grid((unsigned)(n * G.parts)), block(TA_THREADS);
    if (il) hipLaunchKernelGGL((ta_kernel<true, MODE>), grid, block, 0, st, src, G, prm, partials, dst, vec);
    else hipLaunchKernelGGL((ta_kernel<false, MODE>), grid, block, 0, st, src, G, prm, partials, dst, vec);
}

}  // namespace

extern "C" size_t hipt_augment_tensor_workspace_bytes(int n, int rows, int cols) {
    if (!in_envelope(n, rows, cols)) return 0;
    const TaGeo G = geometry(rows, cols);
    return dry_run([&](Carver& c) { carve_tensor_augment(c, n, G); });
}

extern "C" int hipt_augment_tensor(const uint8_t* src, int interleaved, int n, int rows, int cols, const hipt_tensor_augment_params* params,
                                   float* dst, void* ws, size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(src && dst && params, "augment_tensor: src / params / dst missing");
    HIPT_CHECK_ARG(n >= 1 && rows >= 1 && cols >= 1, "augment_tensor: %d regions of %d x %d", n, rows, cols);
    HIPT_CHECK_ARG(in_envelope(n, rows, cols), "augment_tensor: %d regions of %d x %d: too many / too large (rows * cols <= 2^30)", n, rows, cols);
    HIPT_CHECK_ARG((((uintptr_t)dst | (uintptr_t)params) & 3) == 0, "augment_tensor: params / dst need 4-byte alignment");
    const size_t px = (size_t)n * 3 * rows * cols;
    HIPT_CHECK_ARG((const uint8_t*)dst + px * 4 <= src || src + px <= (const uint8_t*)dst, "augment_tensor: src and dst overlap");
    const TaGeo G = geometry(rows, cols);
    const int vec = (G.npix % TA_PX) == 0 && ((uintptr_t)dst & 15) == 0;
    hipStream_t st = (hipStream_t)stream;
    if (ws == nullptr && ws_bytes == 0) {   // the caller's statement that no record holds a contrast op: one launch
        launch<TA_SINGLE>(interleaved != 0, src, G, n, params, nullptr, dst, vec, st);
        HIPT_CHECK_LAUNCH();
        return HIPT_OK;
    }
    Carver c(ws, ws_bytes);
    double* partials = carve_tensor_augment(c, n, G);
    if (int rc = check_workspace(c, "augment_tensor")) return rc;
    HIPT_CHECK_ARG(ws != nullptr, "augment_tensor: workspace missing");
    launch<TA_SUM>(interleaved != 0, src, G, n, params, partials, dst, vec, st);
    HIPT_CHECK_LAUNCH();
    launch<TA_FINISH>(interleaved != 0, src, G, n, params, partials, dst, vec, st);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
