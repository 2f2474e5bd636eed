// Hierarchical region attention heat-maps (HIPT_4K/hipt_heatmap_utils.py:347-485 create_hierarchical_heatmaps_indiv and its method
// form HIPT_4K/hipt_4k.py:167-303): the [CLS] attention maps of ViT-256 and ViT-4K of a region and of its shifted
// copies become, per head and per pair of heads, a picture blended with the region.
//
// The reference upscales every map (nearest neighbour, factor f), ranks the upscaled values (rankdata * 100 / len), shifts and adds
// the layers by slicing, and colours.  Upscaling repeats every value f * f times, so the rank of a value among the upscaled ones is a
// closed form of two integer counts over the L original values; the upscaled maps never exist here:
//   1. hier_ranks_kernel   one workgroup per vector, the vector in LDS, brute-force counts: no sort, no atomic, no workspace;
//   2. hier_render_kernel  a lane owns four consecutive pixels of a row.  It gathers the percentiles of the tokens that cover them in
//                          each layer, forms the nh + nh scores once and writes every requested picture from them: 12 bytes a
//                          picture, as three whole 32-bit words, lane after lane on consecutive addresses.  The ViT-256 scores wait
//                          in LDS while the loop over the ViT-4K heads pairs them.
// The four-pixel look-up, paint, store and the thresholded picture's rule are heat_paint.h's, shared with patch_heatmap.hip.
// All arithmetic is integer, float64 in the order written, or the float32 blend of common.h.
// -ffp-contract=off (Makefile): every float64 operation and the blend's two products and their sum are rounded one by one.
// No inline assembly, no atomics; every store is a vector store.
#include "heat_paint.h"   // the four-pixel look-up, blend, store and the thresholded picture's rule

namespace {

constexpr int HR_THREADS = 256;                    // ranking: threads per vector
constexpr int HR_MAX_L = HIPT_HIER_MAX_L;
constexpr int HH_THREADS = 128;                    // rendering: lanes (groups of four pixels) per workgroup
constexpr int HH_MAX_HEADS = HIPT_HIER_MAX_HEADS;
constexpr int HH_MAX_LUT = HIPT_HIER_MAX_LUT;
static_assert(HR_MAX_L % 4 == 0, "the counting loop reads four values at a time");
static_assert(HH_MAX_LUT * 4 + HH_MAX_HEADS * HH_PX * 8 * HH_THREADS <= 64 * 1024, "the render kernel's LDS fits the default limit");

// pct[v, i] = (less * f^2 + 0.5 * (eq * f^2 + 1)) * 100 / (L * f^2): scipy.stats.rankdata(u) * 100 / len(u) of the vector u that
// repeats every x[v, :] value f^2 times, at the copies of x[v, i]; less = #{x < x_i}, eq = #{x == x_i} in float32 (x_i counts itself)
__global__ __launch_bounds__(HR_THREADS) void hier_ranks_kernel(const float* __restrict__ x, int L, double f2, double len,
                                                               double* __restrict__ pct) {
    __shared__ __attribute__((aligned(16))) float v[HR_MAX_L];
    const int t = threadIdx.x;
    const size_t row = (size_t)blockIdx.x * L;
    const int L4 = (L + 3) & ~3;
    for (int i = t; i < L4; i += HR_THREADS) v[i] = i < L ? x[row + i] : __builtin_nanf("");   // (a NaN compares false both ways)
    __syncthreads();
    for (int i = t; i < L; i += HR_THREADS) {
        const float q = v[i];
        int less = 0, eq = 0;
        for (int j = 0; j < L4; j += 4) {
            const f32x4 r = *(const f32x4*)&v[j];   // the same address in every lane: a broadcast
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                less += r[u] < q;
                eq += r[u] == q;
            }
        }
        const double below = (double)less * f2;
        const double tie = 0.5 * ((double)eq * f2 + 1.0);
        const double rank = below + tie;
        const double p = rank * 100.0;
        pct[row + i] = p / len;
    }
}

struct HierArgs {
    const double* pct4k;    // [4, nh, n]
    const double* pct256;   // [2, nh, n, 256]
    int nh, n, h_256;       // heads, patches, patches across
    int lb, lt;             // log2 of the pixels per patch (b) and per token (t)
    int Hs, Ws;
    int off[4];             // layer offsets in output pixels (off[0] = 0)
    const uint8_t* base;    // [Hs, Ws, 3]
    const uint8_t* lut;     // [lut_n, 3]
    int lut_n;
    int idx_hi, idx_thr;    // table entries of 0.95 and of the threshold
    float a, b;             // blend weights of the colour and of the base image
    double w256;            // weight of the 256 level in the blended score
    double thr;
    uint8_t *hm4k, *hm256, *hm_blend, *hm_thr;   // each may be NULL
    signed char slot[HH_MAX_HEADS * HH_MAX_HEADS];   // picture of hm_blend for the pair (j, i) at [j * HH_MAX_HEADS + i], or -1
};

__global__ __launch_bounds__(HH_THREADS) void hier_render_kernel(const HierArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* lut = (uint32_t*)smem;                                      // [lut_n] packed r | g << 8 | b << 16
    double* s256_lds = (double*)(smem + (((size_t)A.lut_n * 4 + 15) & ~(size_t)15));   // [nh][HH_PX][HH_THREADS]
    const int t = threadIdx.x;
    hh_stage_lut(lut, A.lut, A.lut_n, t, HH_THREADS);
    __syncthreads();   // (the only barrier: lanes past the image leave after it)

    const int gpr = A.Ws / HH_PX;   // groups per row (Ws % 4 == 0: a group never straddles rows)
    const long long g = (long long)blockIdx.x * HH_THREADS + t;
    if (g >= (long long)A.Hs * gpr) return;
    const int y = (int)(g / gpr), x0 = (int)(g - (long long)y * gpr) * HH_PX;
    const size_t pix = (size_t)y * A.Ws + x0;
    const size_t pic = (size_t)A.Hs * A.Ws * 3;   // bytes of one picture
    const int bmask = (1 << A.lb) - 1;

    uint8_t base[12];
    hh_load(A.base + pix * 3, base);

    // where every layer reads: the patch (the ViT-4K token) and the ViT-256 token of it, or -1 where the layer is absent
    int patch[4][HH_PX], token[2][HH_PX];
    double ov4[HH_PX], ov256[HH_PX];   // 100 * the number of present layers, of all four and of the first two
#pragma unroll
    for (int k = 0; k < HH_PX; ++k) {
        int c4 = 0, c256 = 0;
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            const int yy = y - A.off[l], xx = x0 + k - A.off[l];
            const bool present = yy >= 0 && xx >= 0;
            const int p = (yy >> A.lb) * A.h_256 + (xx >> A.lb);
            patch[l][k] = present ? p : -1;
            c4 += present;
            if (l < 2) {
                token[l][k] = present ? p * 256 + (((yy & bmask) >> A.lt) << 4) + ((xx & bmask) >> A.lt) : -1;
                c256 += present;
            }
        }
        ov4[k] = 100.0 * (double)c4;
        ov256[k] = 100.0 * (double)c256;
    }

    // the 256 level: score256 = (u1 + u2) / ov256, its pictures, and the scores parked in LDS for the pairs
    const size_t n = (size_t)A.n;
    for (int i = 0; i < A.nh; ++i) {
        double s[HH_PX];
        int entry[HH_PX];
#pragma unroll
        for (int k = 0; k < HH_PX; ++k) {
            double sum = A.pct256[((size_t)i * n) * 256 + token[0][k]];   // (layer 1 has offset 0: always present)
            if (token[1][k] >= 0) sum += A.pct256[(((size_t)A.nh + i) * n) * 256 + token[1][k]];
            s[k] = sum / ov256[k];
            entry[k] = hh_entry(s[k], A.lut_n);
            s256_lds[((size_t)i * HH_PX + k) * HH_THREADS + t] = s[k];
        }
        if (A.hm256) hh_paint(A.hm256 + (size_t)i * pic + pix * 3, lut, entry, base, A.a, A.b);
        if (A.hm_thr) hh_paint_threshold(A.hm_thr + (size_t)i * pic + pix * 3, lut, s, A.thr, A.idx_hi, A.idx_thr, base, A.a, A.b);
    }

    if (!A.hm4k && !A.hm_blend) return;
    double ovw[HH_PX], den[HH_PX];   // overlay256 = w256 * ov256, and overlay4k + overlay256
#pragma unroll
    for (int k = 0; k < HH_PX; ++k) {
        ovw[k] = A.w256 * ov256[k];
        den[k] = ov4[k] + ovw[k];
    }
    // the 4K level: score4k = (v1 + v2 + v3 + v4) / ov4 (an absent layer is the reference's + 0.0), its picture, and the pairs
    for (int j = 0; j < A.nh; ++j) {
        double s4[HH_PX];
        int entry[HH_PX];
#pragma unroll
        for (int k = 0; k < HH_PX; ++k) {
            double sum = A.pct4k[(size_t)j * n + patch[0][k]];
#pragma unroll
            for (int l = 1; l < 4; ++l)
                if (patch[l][k] >= 0) sum += A.pct4k[((size_t)l * A.nh + j) * n + patch[l][k]];
            s4[k] = sum / ov4[k];
            entry[k] = hh_entry(s4[k], A.lut_n);
        }
        if (A.hm4k) hh_paint(A.hm4k + (size_t)j * pic + pix * 3, lut, entry, base, A.a, A.b);
        if (!A.hm_blend) continue;
        for (int i = 0; i < A.nh; ++i) {
            const int slot = A.slot[j * HH_MAX_HEADS + i];
            if (slot < 0) continue;   // (uniform)
#pragma unroll
            for (int k = 0; k < HH_PX; ++k) {
                const double s256 = s256_lds[((size_t)i * HH_PX + k) * HH_THREADS + t];
                const double p4 = s4[k] * ov4[k];
                const double p256 = s256 * ovw[k];
                const double num = p4 + p256;
                entry[k] = hh_entry(num / den[k], A.lut_n);
            }
            hh_paint(A.hm_blend + (size_t)slot * pic + pix * 3, lut, entry, base, A.a, A.b);
        }
    }
}

int log2_exact(int v) {
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

}  // namespace

extern "C" int hipt_hier_ranks(const float* x, int V, int L, int f, double* pct, void* stream) {
    if (L < 1 || L > HR_MAX_L || f < 1 || f > HIPT_HIER_MAX_UPSCALE) {
        hipt_set_error("hier_ranks: L=%d, f=%d outside the envelope (1 <= L <= %d, 1 <= f <= %d); nothing was launched", L, f, HR_MAX_L,
                       HIPT_HIER_MAX_UPSCALE);
        return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_ARG(V >= 0, "hier_ranks: V=%d", V);
    if (V == 0) return HIPT_OK;
    HIPT_CHECK_ARG(x && pct, "hier_ranks: x / pct missing");
    HIPT_CHECK_ARG(((uintptr_t)x & 3) == 0 && ((uintptr_t)pct & 7) == 0, "hier_ranks: x needs 4-byte, pct 8-byte alignment");
    const double f2 = (double)f * (double)f;
    hipLaunchKernelGGL(hier_ranks_kernel, dim3((unsigned)V), dim3(HR_THREADS), 0, (hipStream_t)stream, x, L, f2, (double)L * f2, pct);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

extern "C" int hipt_hier_render(const double* pct4k, const double* pct256, int nh, int w_256, int h_256, int scale, int off2, int off3,
                                int off4, const uint8_t* base, const uint8_t* lut, int lut_n, double alpha, double w256, const int32_t* pairs,
                                int npairs, int use_threshold, double threshold, uint8_t* hm4k, uint8_t* hm256, uint8_t* hm_blend,
                                uint8_t* hm256_thr, void* stream) {
    const bool scale_ok = scale == 1 || scale == 2 || scale == 4 || scale == 8 || scale == 16;
    if (!scale_ok || nh < 1 || nh > HH_MAX_HEADS || w_256 < 1 || h_256 < 1 || (long long)w_256 * h_256 > HR_MAX_L || lut_n < 2 ||
        lut_n > HH_MAX_LUT) {
        hipt_set_error("hier_render: scale=%d, nh=%d, grid %d x %d, table of %d outside the envelope (scale 1 / 2 / 4 / 8 / 16, 1 <= nh <= %d, "
                       "1 <= w_256 * h_256 <= %d, 2 <= N <= %d); nothing was launched", scale, nh, w_256, h_256, lut_n, HH_MAX_HEADS, HR_MAX_L,
                       HH_MAX_LUT);
        return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_ARG(hm4k || hm256 || hm_blend || hm256_thr, "hier_render: no output asked for");
    HIPT_CHECK_ARG(pct4k && pct256 && base && lut, "hier_render: pct4k / pct256 / base / lut missing");
    HIPT_CHECK_ARG(off2 >= 0 && off3 >= 0 && off4 >= 0, "hier_render: negative offsets %d, %d, %d", off2, off3, off4);
    HIPT_CHECK_ARG(alpha == alpha && w256 == w256 && w256 > 0.0, "hier_render: alpha is NaN, or w256 is not positive");
    HIPT_CHECK_ARG(!use_threshold || threshold == threshold, "hier_render: threshold is NaN");
    HIPT_CHECK_ARG(!hm256_thr || use_threshold, "hier_render: the threshold picture needs a threshold");
    HIPT_CHECK_ARG(((uintptr_t)pct4k & 7) == 0 && ((uintptr_t)pct256 & 7) == 0, "hier_render: pct4k / pct256 need 8-byte alignment");
    HIPT_CHECK_ARG((((uintptr_t)base | (uintptr_t)hm4k | (uintptr_t)hm256 | (uintptr_t)hm_blend | (uintptr_t)hm256_thr) & 3) == 0,
                   "hier_render: base and the pictures need 4-byte alignment");
    HIPT_CHECK_ARG(base != hm4k && base != hm256 && base != hm_blend && base != hm256_thr, "hier_render: the base image cannot be an output");
    HierArgs A;
    for (int k = 0; k < HH_MAX_HEADS * HH_MAX_HEADS; ++k) A.slot[k] = -1;
    if (hm_blend) {
        if (!pairs) {   // every pair, j major
            for (int j = 0; j < nh; ++j)
                for (int i = 0; i < nh; ++i) A.slot[j * HH_MAX_HEADS + i] = (signed char)(j * nh + i);
        } else {
            HIPT_CHECK_ARG(npairs >= 1 && npairs <= nh * nh, "hier_render: %d pairs (1 .. nh * nh, each once)", npairs);
            for (int k = 0; k < npairs; ++k) {
                const int j = pairs[2 * k], i = pairs[2 * k + 1];
                HIPT_CHECK_ARG(j >= 0 && j < nh && i >= 0 && i < nh, "hier_render: pair %d is (%d, %d), heads are 0 .. %d", k, j, i, nh - 1);
                HIPT_CHECK_ARG(A.slot[j * HH_MAX_HEADS + i] < 0, "hier_render: pair (%d, %d) is listed twice", j, i);
                A.slot[j * HH_MAX_HEADS + i] = (signed char)k;
            }
        }
    }
    const int b = 256 / scale, t = 16 / scale;
    A.pct4k = pct4k;
    A.pct256 = pct256;
    A.nh = nh;
    A.n = w_256 * h_256;
    A.h_256 = h_256;
    A.lb = log2_exact(b);
    A.lt = log2_exact(t);
    A.Hs = w_256 * b;
    A.Ws = h_256 * b;
    A.off[0] = 0;
    A.off[1] = off2;
    A.off[2] = off3;
    A.off[3] = off4;
    A.base = base;
    A.lut = lut;
    A.lut_n = lut_n;
    hh_threshold_entries(lut_n, use_threshold, threshold, &A.idx_hi, &A.idx_thr);
    A.a = (float)alpha;
    A.b = (float)(1.0 - alpha);
    A.w256 = w256;
    A.thr = use_threshold ? threshold : 2.0;
    A.hm4k = hm4k;
    A.hm256 = hm256;
    A.hm_blend = hm_blend;
    A.hm_thr = hm256_thr;
    const long long groups = (long long)A.Hs * (A.Ws / HH_PX);
    const size_t lds = (((size_t)lut_n * 4 + 15) & ~(size_t)15) + (size_t)nh * HH_PX * HH_THREADS * sizeof(double);
    hipLaunchKernelGGL(hier_render_kernel, dim3((unsigned)((groups + HH_THREADS - 1) / HH_THREADS)), dim3(HH_THREADS), lds,
                       (hipStream_t)stream, A);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
