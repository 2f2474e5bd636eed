// Region augmentation (extract_features_fp.py:89-136, --use_transforms HIPT_*): uint8 RGB regions in, uint8 out, one
// parameter record per region (include/hipt_abmil.h: hipt_augment_params; DESIGN.md 10 states the arithmetic).
//
// A thread owns 16 consecutive output pixels of one row; a 256-thread workgroup covers a 128 x 32 output tile, so the source
// of a tile rotated by up to 90 degrees is still a compact 32 x 128 patch.  The per-pixel chain is: source coordinate
// (flips, then Pillow's 16.16 fixed-point AFFINE / its exact-scale path, NEAREST, fill 0) -> ColorJitter ops in the
// record's order.  Contrast blends against the mean luminance of the whole region as it is at that step, so pass 1 runs the
// chain up to the contrast op and sums L exactly (uint64, one atomic per workgroup: deterministic); pass 2 recomputes the
// chain and finishes it.  Regions without a contrast op leave pass 1 at once.
//
// Pillow's and torchvision's arithmetic is reproduced operation for operation (float32 blends, the float / double mix of
// Pillow's HSV conversions), so this file is compiled without FMA contraction.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int AUG_PX = 16;                 // output pixels per thread (one 16-byte vector per plane)
constexpr int AUG_TX = 8, AUG_TY = 32;     // threads per workgroup along cols / rows: a 128 x 32 tile
constexpr int AUG_TILE_W = AUG_TX * AUG_PX;

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow's RGB -> L: (19595 R + 38470 G + 7471 B + 0x8000) >> 16
__device__ __forceinline__ int lum(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Image.blend(degenerate, img, alpha) (float alpha): d + alpha * (p - d) in float32, clipped, truncated
__device__ __forceinline__ int blend(int d, int p, float alpha) {
    const float t = __fadd_rn((float)d, __fmul_rn(alpha, (float)(p - d)));
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// float32 division, correctly rounded by construction (the double quotient of two floats rounds to the float quotient)
__device__ __forceinline__ float fdiv(float a, float b) { return (float)((double)a / (double)b); }

// torchvision adjust_hue on a PIL image: RGB -> HSV (Pillow rgb2hsv), H += shift mod 256, HSV -> RGB (Pillow hsv2rgb)
__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int shift) {
    const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = mx;
    if (mx != mn) {
        const float cr = (float)(mx - mn);
        const float s = fdiv(cr, (float)mx);
        const float rc = fdiv((float)(mx - r), cr), gc = fdiv((float)(mx - g), cr), bc = fdiv((float)(mx - b), cr);
        float h;
        if (r == mx) h = bc - gc;
        else if (g == mx) h = (float)((2.0 + (double)rc) - (double)bc);
        else h = (float)((4.0 + (double)gc) - (double)rc);
        h = (float)fmod((double)h / 6.0 + 1.0, 1.0);
        uh = clip8((int)((double)h * 255.0));
        us = clip8((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        r = g = b = uv;
        return;
    }
    const double hh = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(hh);
    const float f = (float)(hh - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const double vv = (double)(float)uv;
    const int p = clip8((int)round(vv * (1.0 - (double)fs)));
    const int q = clip8((int)round(vv * (1.0 - (double)(fs * f))));
    const int t = clip8((int)round(vv * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

// the record's colour ops in order on 16 pixels; PRE: stop at the contrast op (pass 1), else contrast blends against `mean`.
// (ops outside, pixels inside: the pixel loop unrolls and the pixel arrays stay in registers)
template <bool PRE>
__device__ __forceinline__ void colour(int (&R)[AUG_PX], int (&G)[AUG_PX], int (&B)[AUG_PX], const hipt_augment_params& p, int mean) {
    for (int k = 0; k < p.n_ops; ++k) {
        const int op = p.ops[k];
        if (op == HIPT_AUG_BRIGHTNESS) {
            const float f = p.factor[0];
#pragma unroll
            for (int j = 0; j < AUG_PX; ++j) { R[j] = blend(0, R[j], f); G[j] = blend(0, G[j], f); B[j] = blend(0, B[j], f); }
        } else if (op == HIPT_AUG_CONTRAST) {
            if (PRE) return;
            const float f = p.factor[1];
#pragma unroll
            for (int j = 0; j < AUG_PX; ++j) { R[j] = blend(mean, R[j], f); G[j] = blend(mean, G[j], f); B[j] = blend(mean, B[j], f); }
        } else if (op == HIPT_AUG_SATURATION) {
            const float f = p.factor[2];
#pragma unroll
            for (int j = 0; j < AUG_PX; ++j) {
                const int l = lum(R[j], G[j], B[j]);
                R[j] = blend(l, R[j], f); G[j] = blend(l, G[j], f); B[j] = blend(l, B[j], f);
            }
        } else if (op == HIPT_AUG_HUE) {
#pragma unroll
            for (int j = 0; j < AUG_PX; ++j) hue_shift(R[j], G[j], B[j], p.hue_shift);
        }
    }
}

__device__ __forceinline__ bool has_contrast(const hipt_augment_params& p) {
    for (int k = 0; k < p.n_ops; ++k)
        if (p.ops[k] == HIPT_AUG_CONTRAST) return true;
    return false;
}

__device__ __forceinline__ bool scale_path(const hipt_augment_params& p) {
    return (p.flags & HIPT_AUG_AFFINE) && p.affine[1] == 0.0 && p.affine[3] == 0.0;  // Pillow: ImagingScaleAffine
}

__device__ __forceinline__ int fix16(double v) { return (int)floor(v * 65536.0 + 0.5); }  // Geometry.c FIX()

struct Geo {
    int rows, cols;
    int64_t plane;       // rows * cols
};

// the 48 loaded bytes -> 16 pixels (pixel j of the output = loaded pixel 15 - j under HFlip); all indices compile-time
template <bool IL, bool HF>
__device__ __forceinline__ void unpack16(const u32x4 (&w)[3], int (&R)[AUG_PX], int (&Gc)[AUG_PX], int (&B)[AUG_PX]) {
#pragma unroll
    for (int j = 0; j < AUG_PX; ++j) {
        const int jj = HF ? AUG_PX - 1 - j : j;
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int byte = IL ? 3 * jj + c : c * AUG_PX + jj;
            v[c] = (w[byte >> 4][(byte >> 2) & 3] >> (8 * (byte & 3))) & 255;
        }
        R[j] = v[0]; Gc[j] = v[1]; B[j] = v[2];
    }
}

// the source pixels of the 16 output pixels of row y from x0 (fill pixels are 0)
template <bool IL>
__device__ __forceinline__ void fetch(const uint8_t* src, const Geo& G, const hipt_augment_params& p, const int* xt, const int* yt,
                                      int x0, int y, int (&R)[AUG_PX], int (&Gc)[AUG_PX], int (&B)[AUG_PX]) {
    const bool hf = p.flags & HIPT_AUG_HFLIP, vf = p.flags & HIPT_AUG_VFLIP;
    if (!(p.flags & (HIPT_AUG_AFFINE | HIPT_AUG_BLUR)) && (G.cols % AUG_PX) == 0) {
        // flips only: the 16 source pixels are 16 consecutive ones (reversed under HFlip): three 16-byte loads
        const int sy = vf ? G.rows - 1 - y : y;
        const int sx = hf ? G.cols - AUG_PX - x0 : x0;
        u32x4 w[3];
        if (IL) {
            const u32x4* q = (const u32x4*)(src + ((int64_t)sy * G.cols + sx) * 3);
            w[0] = q[0]; w[1] = q[1]; w[2] = q[2];
        } else {
            const int64_t o = (int64_t)sy * G.cols + sx;
#pragma unroll
            for (int c = 0; c < 3; ++c) w[c] = *(const u32x4*)(src + o + c * G.plane);
        }
        if (hf) unpack16<IL, true>(w, R, Gc, B);
        else unpack16<IL, false>(w, R, Gc, B);
        return;
    }
    int xo = 0, yo = 0, a0 = 0, a1 = 0, a3 = 0, a4 = 0;
    const bool aff = p.flags & HIPT_AUG_AFFINE, scale = aff && scale_path(p);
    if (aff && !scale) {
        a0 = fix16(p.affine[0]); a1 = fix16(p.affine[1]); a3 = fix16(p.affine[3]); a4 = fix16(p.affine[4]);
        xo = fix16(p.affine[2] + p.affine[1] * 0.5 + p.affine[0] * 0.5);
        yo = fix16(p.affine[5] + p.affine[4] * 0.5 + p.affine[3] * 0.5);
    }
#pragma unroll
    for (int j = 0; j < AUG_PX; ++j) {
        const int x = min(x0 + j, G.cols - 1);  // (columns past the edge are computed but never stored or counted)
        int xi = x, yi = y;
        bool in = true;
        if (scale) {
            xi = xt[x]; yi = yt[y];
            in = xi >= 0 && yi >= 0;
        } else if (aff) {
            // Pillow steps xx by a0 per column and by a1 per row from xo in int: the same sums, formed directly
            const int xx = (int)((uint32_t)xo + (uint32_t)y * (uint32_t)a1 + (uint32_t)x * (uint32_t)a0);
            const int yy = (int)((uint32_t)yo + (uint32_t)y * (uint32_t)a4 + (uint32_t)x * (uint32_t)a3);
            xi = xx >> 16; yi = yy >> 16;
            in = xi >= 0 && xi < G.cols && yi >= 0 && yi < G.rows;
        }
        int vr = 0, vg = 0, vb = 0;  // (one assignment per array element: the arrays stay in registers)
        if (in) {
            const int sx = hf ? G.cols - 1 - xi : xi, sy = vf ? G.rows - 1 - yi : yi;
            const int64_t o = (int64_t)sy * G.cols + sx;
            if (IL) {
                const uint8_t* q = src + o * 3;
                vr = q[0]; vg = q[1]; vb = q[2];
            } else {
                vr = src[o]; vg = src[o + G.plane]; vb = src[o + 2 * G.plane];
            }
        }
        R[j] = vr; Gc[j] = vg; B[j] = vb;
    }
}

// GaussianBlur(kernel_size=(1,3)): vertical 3 taps over reflect-padded rows, float32, rounded half to even
template <bool IL>
__device__ __forceinline__ void blur(const uint8_t* src, const Geo& G, const hipt_augment_params& p, int x0, int y,
                                     int (&R)[AUG_PX], int (&Gc)[AUG_PX], int (&B)[AUG_PX]) {
    // (reflect padding needs 2 rows -- the caller refuses fewer; clamped so that a 1-row region cannot read outside)
    const int ya = y == 0 ? min(1, G.rows - 1) : y - 1, yb = y == G.rows - 1 ? max(G.rows - 2, 0) : y + 1;
    const float w0 = p.blur_w[0], w1 = p.blur_w[1], w2 = p.blur_w[2];
#pragma unroll
    for (int j = 0; j < AUG_PX; ++j) {
        const int x = min(x0 + j, G.cols - 1);
        int v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int64_t cs = IL ? c : c * G.plane, es = IL ? 3 : 1;
            const float s0 = src[((int64_t)ya * G.cols + x) * es + cs], s1 = src[((int64_t)y * G.cols + x) * es + cs],
                        s2 = src[((int64_t)yb * G.cols + x) * es + cs];
            const float acc = __fadd_rn(__fadd_rn(__fmul_rn(w0, s0), __fmul_rn(w1, s1)), __fmul_rn(w2, s2));
            v[c] = clip8((int)rintf(acc));
        }
        R[j] = v[0]; Gc[j] = v[1]; B[j] = v[2];
    }
}

__device__ __forceinline__ const int* tables(const void* ws, int n, int rows, int cols, int r) {
    return (const int*)((const char*)ws + (size_t)n * 8) + (size_t)r * (rows + cols);
}

// one workgroup per region: zero its luminance sum; for a record on Pillow's exact-scale path (a1 == a3 == 0), tabulate the
// source column of every output column and the source row of every output row (-1 = fill) by Pillow's own double recurrence
__global__ __launch_bounds__(64) void aug_prep_kernel(const hipt_augment_params* __restrict__ prm, int n, int rows, int cols,
                                                      void* __restrict__ ws) {
    const int r = blockIdx.x;
    const hipt_augment_params& p = prm[r];
    if (threadIdx.x == 0) ((uint64_t*)ws)[r] = 0;
    if (!scale_path(p)) return;
    int* xt = (int*)tables(ws, n, rows, cols, r);
    int* yt = xt + cols;
    if (threadIdx.x == 0) {
        double xo = p.affine[2] + p.affine[0] * 0.5;
        for (int x = 0; x < cols; ++x) {
            const int xin = xo < 0.0 ? -1 : (int)xo;
            xt[x] = xin < cols ? xin : -1;
            xo += p.affine[0];
        }
    } else if (threadIdx.x == 32) {
        double yo = p.affine[5] + p.affine[4] * 0.5;
        for (int y = 0; y < rows; ++y) {
            const int yin = yo < 0.0 ? -1 : (int)yo;
            yt[y] = yin < rows ? yin : -1;
            yo += p.affine[4];
        }
    }
}

// pass 1: sum of L over the region at the contrast step (regions without a contrast op return at once)
template <bool IL>
__global__ __launch_bounds__(256) void aug_sum_kernel(const uint8_t* __restrict__ src, int n, int rows, int cols,
                                                      const hipt_augment_params* __restrict__ prm, void* __restrict__ ws) {
    const int r = blockIdx.z;
    const hipt_augment_params& p = prm[r];
    if (!has_contrast(p)) return;
    const Geo G{rows, cols, (int64_t)rows * cols};
    const int x0 = (blockIdx.x * AUG_TX + (threadIdx.x % AUG_TX)) * AUG_PX, y = blockIdx.y * AUG_TY + threadIdx.x / AUG_TX;
    const int* xt = tables(ws, n, rows, cols, r);
    uint32_t s = 0;
    if (x0 < cols && y < rows) {
        int R[AUG_PX], Gc[AUG_PX], B[AUG_PX];
        fetch<IL>(src + (size_t)r * 3 * G.plane, G, p, xt, xt + cols, x0, y, R, Gc, B);
        colour<true>(R, Gc, B, p, 0);
#pragma unroll
        for (int j = 0; j < AUG_PX; ++j)
            if (x0 + j < cols) s += lum(R[j], Gc[j], B[j]);
    }
    // <= 256 threads x 16 pixels x 255: a workgroup's sum fits 32 bits; one 64-bit atomic per workgroup
#pragma unroll  // (wave_sum of common.h, written out: the call compiles to different code here)
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ uint32_t part[256 / 64];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = (unsigned long long)part[0] + part[1] + part[2] + part[3];
        if (t) atomicAdd((unsigned long long*)ws + r, t);
    }
}

// pass 2: the whole chain, 16 pixels per thread, written with 16-byte stores where the row allows it
template <bool IL>
__global__ __launch_bounds__(256) void aug_apply_kernel(const uint8_t* __restrict__ src, int n, int rows, int cols,
                                                        const hipt_augment_params* __restrict__ prm, const void* __restrict__ ws,
                                                        uint8_t* __restrict__ dst) {
    const int r = blockIdx.z;
    const hipt_augment_params& p = prm[r];
    const Geo G{rows, cols, (int64_t)rows * cols};
    const int x0 = (blockIdx.x * AUG_TX + (threadIdx.x % AUG_TX)) * AUG_PX, y = blockIdx.y * AUG_TY + threadIdx.x / AUG_TX;
    if (x0 >= cols || y >= rows) return;
    const uint8_t* s = src + (size_t)r * 3 * G.plane;
    uint8_t* d = dst + (size_t)r * 3 * G.plane;
    int R[AUG_PX], Gc[AUG_PX], B[AUG_PX];
    if (p.flags & HIPT_AUG_BLUR) {
        blur<IL>(s, G, p, x0, y, R, Gc, B);
    } else {
        const int* xt = tables(ws, n, rows, cols, r);
        fetch<IL>(s, G, p, xt, xt + cols, x0, y, R, Gc, B);
        if (p.n_ops) {
            // Pillow ImageStat: mean = sum / count in double; ImageEnhance.Contrast: int(mean + 0.5)
            const int mean = has_contrast(p) ? (int)((double)((const uint64_t*)ws)[r] / (double)G.plane + 0.5) : 0;
            colour<false>(R, Gc, B, p, mean);
        }
    }
    if ((cols % AUG_PX) == 0) {
        u32x4 w[3];
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            uint32_t v = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int byte = q * 4 + e, j = IL ? byte / 3 : byte % AUG_PX, c = IL ? byte % 3 : byte / AUG_PX;
                v |= (uint32_t)(c == 0 ? R[j] : (c == 1 ? Gc[j] : B[j])) << (8 * e);
            }
            w[q >> 2][q & 3] = v;
        }
        if (IL) {
            u32x4* o = (u32x4*)(d + ((int64_t)y * cols + x0) * 3);
            o[0] = w[0]; o[1] = w[1]; o[2] = w[2];
        } else {
            const int64_t o = (int64_t)y * cols + x0;
#pragma unroll
            for (int c = 0; c < 3; ++c) *(u32x4*)(d + o + c * G.plane) = w[c];
        }
    } else {
#pragma unroll
        for (int j = 0; j < AUG_PX; ++j) {
            const int64_t o = (int64_t)y * cols + x0 + j;
            if (x0 + j >= cols) {
            } else if (IL) {
                d[o * 3] = (uint8_t)R[j]; d[o * 3 + 1] = (uint8_t)Gc[j]; d[o * 3 + 2] = (uint8_t)B[j];
            } else {
                d[o] = (uint8_t)R[j]; d[o + G.plane] = (uint8_t)Gc[j]; d[o + 2 * G.plane] = (uint8_t)B[j];
            }
        }
    }
}

}  // namespace

extern "C" size_t hipt_augment_workspace_bytes(int n, int rows, int cols) {
    if (n <= 0 || rows <= 0 || cols <= 0) return 0;
    return (size_t)n * 8 + (size_t)n * (size_t)(rows + cols) * 4;
}

extern "C" int hipt_augment_regions(const uint8_t* src, int interleaved, int n, int rows, int cols, const hipt_augment_params* params,
                                    uint8_t* dst, void* workspace, size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(src && dst && params && workspace && n > 0 && rows > 0 && cols > 0, "augment_regions: null / empty argument");
    HIPT_CHECK_ARG(n <= 65535 && (int64_t)rows * cols <= ((int64_t)1 << 30), "augment_regions: %d regions of %d x %d: too many / too large",
                   n, rows, cols);
    HIPT_CHECK_ARG(((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0 && ((uintptr_t)workspace % 8) == 0 &&
                       ((uintptr_t)params % 8) == 0,
                   "augment_regions: src / dst need 16-byte, params / workspace 8-byte alignment");
    const size_t bytes = (size_t)n * 3 * rows * cols;
    HIPT_CHECK_ARG((const uint8_t*)dst + bytes <= src || src + bytes <= (const uint8_t*)dst, "augment_regions: src and dst overlap");
    if (ws_bytes < hipt_augment_workspace_bytes(n, rows, cols)) {
        hipt_set_error("augment_regions: workspace %zu B too small (need %zu)", ws_bytes, hipt_augment_workspace_bytes(n, rows, cols));
        return HIPT_E_WORKSPACE;
    }
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)((cols + AUG_TILE_W - 1) / AUG_TILE_W), (unsigned)((rows + AUG_TY - 1) / AUG_TY), (unsigned)n);
    hipLaunchKernelGGL(aug_prep_kernel, dim3(n), dim3(64), 0, st, params, n, rows, cols, workspace);
    HIPT_CHECK_LAUNCH();
    const dim3 block(AUG_TX * AUG_TY);
    if (interleaved) hipLaunchKernelGGL(aug_sum_kernel<true>, grid, block, 0, st, src, n, rows, cols, params, workspace);
    else hipLaunchKernelGGL(aug_sum_kernel<false>, grid, block, 0, st, src, n, rows, cols, params, workspace);
    HIPT_CHECK_LAUNCH();
    if (interleaved) hipLaunchKernelGGL(aug_apply_kernel<true>, grid, block, 0, st, src, n, rows, cols, params, (const void*)workspace, dst);
    else hipLaunchKernelGGL(aug_apply_kernel<false>, grid, block, 0, st, src, n, rows, cols, params, (const void*)workspace, dst);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
