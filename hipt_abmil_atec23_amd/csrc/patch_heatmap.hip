// Patch-level ViT-256 attention heat-maps (HIPT_4K/attention_visualization_utils.py:293-421 create_patch_heatmaps_indiv / _concat;
// DESIGN.md 24): the [CLS] attention of a 256 x 256 patch and of its copy shifted by 16 pixels becomes, per head, a picture blended
// with the patch and, with a threshold, the thresholded picture -- for a batch of patches in one launch.
//
// The reference upscales each 16 x 16 map by 16, ranks the 65 536 values, shifts layer 2 by `offset` by slicing, adds and colours:
// twelve full-size numpy passes a patch.  The ranks come from hipt_hier_ranks (f = 16) at the maps' own size; here
//   patch_render_kernel   a workgroup owns a band of PH_ROWS rows of one patch.  It stages the colour table and the patch's
//                         2 * nh * 256 ranks in LDS; a lane owns four consecutive pixels of a row, reads them once, forms the score
//                         of each head once and writes both pictures from it, 12 bytes a picture as three whole words, lane after
//                         lane on consecutive addresses (heat_paint.h).  With cols > 0 head i goes to tile (i / cols, i % cols) of a
//                         mosaic and the unused tiles of the last row are written 0: the concatenated form costs no second pass.
// All arithmetic is integer, float64 in the reference's order, or the float32 blend of common.h.
// -ffp-contract=off (Makefile).  No inline assembly, no atomics, no workspace; every store is a vector store.
#include "heat_paint.h"

namespace {

constexpr int PH_THREADS = 256;
constexpr int PH_SIDE = 256;                     // pixels along a patch
constexpr int PH_TOKENS = 256;                   // a 16 x 16 grid of tokens of 16 x 16 pixels
constexpr int PH_ROWS = 32;                      // rows per workgroup
constexpr int PH_BANDS = PH_SIDE / PH_ROWS;
constexpr int PH_GPR = PH_SIDE / HH_PX;          // groups of four pixels per row
constexpr int PH_MAX_HEADS = HIPT_HIER_MAX_HEADS;
constexpr int PH_MAX_LUT = HIPT_HIER_MAX_LUT;
static_assert(PH_ROWS * PH_GPR % PH_THREADS == 0, "every lane makes the same number of rounds");
static_assert(PH_MAX_LUT * 4 + 2 * PH_MAX_HEADS * PH_TOKENS * 8 <= 64 * 1024, "the colour table and a patch's ranks fit the default LDS limit");

struct PatchArgs {
    const double* pct;        // [P, 2, nh, 256]
    const uint8_t* patches;   // [P, 256, 256, 3]
    const uint8_t* lut;       // [lut_n, 3]
    int nh, lut_n, offset;
    int cols, tiles;          // mosaic: tiles across and in all (cols == 0: tiles == nh, one picture a head)
    int idx_hi, idx_thr;      // table entries of 0.95 and of the threshold
    float a, b;               // blend weights of the colour and of the patch
    double thr;
    uint8_t *hm, *hm_thr;     // each may be NULL
};

__global__ __launch_bounds__(PH_THREADS) void patch_render_kernel(const PatchArgs A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* lut = (uint32_t*)smem;                                                 // [lut_n] packed r | g << 8 | b << 16
    double* rk = (double*)(smem + (((size_t)A.lut_n * 4 + 15) & ~(size_t)15));       // [2][nh][256]
    const int t = threadIdx.x;
    const size_t p = blockIdx.x / PH_BANDS;
    const int band = blockIdx.x % PH_BANDS;
    hh_stage_lut(lut, A.lut, A.lut_n, t, PH_THREADS);
    const int nrk = 2 * A.nh * PH_TOKENS;
    const double* src = A.pct + p * (size_t)nrk;
    for (int e = t; e < nrk; e += PH_THREADS) rk[e] = src[e];
    __syncthreads();   // (the only barrier)

    // where a tile of an output begins: one picture a head, or the tile of a mosaic of `cols` tiles across
    const int across = A.cols > 0 ? A.cols : 1;
    const size_t row_bytes = (size_t)across * PH_SIDE * 3;                            // a row of the output image
    const size_t tile_bytes = (size_t)PH_SIDE * PH_SIDE * 3;
    const size_t out_p = p * (size_t)A.tiles * tile_bytes;                            // this patch's pictures / mosaic

    for (int g = t; g < PH_ROWS * PH_GPR; g += PH_THREADS) {
        const int y = band * PH_ROWS + g / PH_GPR, x0 = (g % PH_GPR) * HH_PX;
        uint8_t base[12];
        hh_load(A.patches + ((p * PH_SIDE + y) * PH_SIDE + x0) * 3, base);
        // layer 1's token, and layer 2's (the map shifted by offset down and right), or -1 where layer 2 is absent
        const int tok1 = (y >> 4) * 16 + (x0 >> 4);   // (x0 % 4 == 0: the four pixels share it)
        int tok2[HH_PX];
        double ov[HH_PX];
#pragma unroll
        for (int k = 0; k < HH_PX; ++k) {
            const int yy = y - A.offset, xx = x0 + k - A.offset;
            const bool present = yy >= 0 && xx >= 0;
            tok2[k] = present ? (yy >> 4) * 16 + (xx >> 4) : -1;
            ov[k] = present ? 200.0 : 100.0;
        }
        const size_t in_tile = (size_t)y * row_bytes + (size_t)x0 * 3;
        for (int i = 0; i < A.tiles; ++i) {
            const size_t at = out_p + (A.cols > 0 ? (size_t)(i / A.cols) * PH_SIDE * row_bytes + (size_t)(i % A.cols) * PH_SIDE * 3
                                                  : (size_t)i * tile_bytes) + in_tile;
            if (i >= A.nh) {   // an unused tile of the mosaic's last row (uniform)
                const uint8_t zero[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                if (A.hm) hh_store(A.hm + at, zero);
                if (A.hm_thr) hh_store(A.hm_thr + at, zero);
                continue;
            }
            const double s1 = rk[i * PH_TOKENS + tok1];
            double s[HH_PX];
            int entry[HH_PX];
#pragma unroll
            for (int k = 0; k < HH_PX; ++k) {
                double sum = s1;   // (an absent layer 2 is the reference's + 0.0)
                if (tok2[k] >= 0) sum += rk[(A.nh + i) * PH_TOKENS + tok2[k]];
                s[k] = sum / ov[k];
                entry[k] = hh_entry(s[k], A.lut_n);
            }
            if (A.hm) hh_paint(A.hm + at, lut, entry, base, A.a, A.b);
            if (A.hm_thr) hh_paint_threshold(A.hm_thr + at, lut, s, A.thr, A.idx_hi, A.idx_thr, base, A.a, A.b);
        }
    }
}

}  // namespace

extern "C" int hipt_patch_render(const double* pct, const uint8_t* patches, int P, int nh, const uint8_t* lut, int lut_n, int offset,
                                 double alpha, int use_threshold, double threshold, int cols, uint8_t* hm, uint8_t* hm_thr, void* stream) {
    if (nh < 1 || nh > PH_MAX_HEADS || lut_n < 2 || lut_n > PH_MAX_LUT || P > HIPT_PATCH_MAX_P) {
        hipt_set_error("patch_render: P=%d, nh=%d, table of %d outside the envelope (P <= %d, 1 <= nh <= %d, 2 <= N <= %d); nothing was "
                       "launched", P, nh, lut_n, HIPT_PATCH_MAX_P, PH_MAX_HEADS, PH_MAX_LUT);
        return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_ARG(P >= 0, "patch_render: P=%d", P);
    HIPT_CHECK_ARG(offset >= 0 && offset <= PH_SIDE, "patch_render: offset %d (0 .. %d)", offset, PH_SIDE);
    HIPT_CHECK_ARG(cols >= 0 && cols <= PH_MAX_HEADS, "patch_render: cols %d (0: one picture a head; 1 .. %d: a mosaic)", cols, PH_MAX_HEADS);
    HIPT_CHECK_ARG(alpha == alpha, "patch_render: alpha is NaN");
    HIPT_CHECK_ARG(!use_threshold || threshold == threshold, "patch_render: threshold is NaN");
    HIPT_CHECK_ARG(hm || hm_thr, "patch_render: no output asked for");
    HIPT_CHECK_ARG(!hm_thr || use_threshold, "patch_render: the threshold picture needs a threshold");
    if (P == 0) return HIPT_OK;
    HIPT_CHECK_ARG(pct && patches && lut, "patch_render: pct / patches / lut missing");
    HIPT_CHECK_ARG(((uintptr_t)pct & 7) == 0, "patch_render: pct needs 8-byte alignment");
    HIPT_CHECK_ARG((((uintptr_t)patches | (uintptr_t)hm | (uintptr_t)hm_thr) & 3) == 0, "patch_render: patches and the pictures need 4-byte alignment");
    HIPT_CHECK_ARG(patches != hm && patches != hm_thr && (hm != hm_thr), "patch_render: the patches cannot be an output, nor the outputs one buffer");
    PatchArgs A;
    A.pct = pct;
    A.patches = patches;
    A.lut = lut;
    A.nh = nh;
    A.lut_n = lut_n;
    A.offset = offset;
    A.cols = cols;
    A.tiles = cols > 0 ? (nh + cols - 1) / cols * cols : nh;
    hh_threshold_entries(lut_n, use_threshold, threshold, &A.idx_hi, &A.idx_thr);
    A.a = (float)alpha;
    A.b = (float)(1.0 - alpha);
    A.thr = use_threshold ? threshold : 2.0;
    A.hm = hm;
    A.hm_thr = hm_thr;
    const size_t lds = (((size_t)lut_n * 4 + 15) & ~(size_t)15) + (size_t)2 * nh * PH_TOKENS * sizeof(double);
    hipLaunchKernelGGL(patch_render_kernel, dim3((unsigned)P * PH_BANDS), dim3(PH_THREADS), lds, (hipStream_t)stream, A);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
