// What the single-bag kernel (abmil.hip) and the ragged multi-bag kernel (abmil_bags.hip) of the fused CLAM_SB / ABMIL row tile share:
// tile height, LDS budget and carve of one [T, S1, S2] instantiation, lane geometry, the swizzled h1 image,
// tile_max and store_partial, bag_head (the tail of both combine kernels) and the one table of supported
// widths (visit_width); and, of the multi-bag tile passes (abmil_bags.hip, abmil_bags_mb8.hip, abmil_narrow.hip, abmil_wide.hip,
// abmil_wide_mb.hip), the unit record, the grid, the one launcher (launch_tile_pass) and the wide pair's geometry (WG).  The GEMM
// phases, the gate and the pooling are still written out in every tile kernel, the sibling pairs abmil_wide / abmil_wide_mb and
// abmil_bags_mb / abmil_bags_mb8 included: a tile's statements behind a function boundary -- lifted phase by phase, or the whole unit
// loop as one body that each kernel calls -- compile to other device code.  The gate's sigmoid_f / tanh_f and the shuffle reductions (wave_*, quad_sum)
// are common.h's: the training step (clam_train.hip) recomputes the gate with the same two functions.
#pragma once
#include <cstdlib>

#include "common.h"
#include "launch.h"

namespace abmil_tile {

constexpr int TM = 128;  // rows per tile

template <typename T, int S1, int S2> struct AG {
    static constexpr int KB = Tr<T>::KB;
    static constexpr int NSLAB = S1 / KB;             // 128-byte slabs of the h1 image
    static constexpr int NJ1 = S1 / 32;               // n-frags per wave, phase 1 (2 column waves)
    static constexpr int NJ2 = (2 * S2) / 32;         // n-frags per wave, phase 2
    static constexpr int STAGE = (TM + S1) * 128;
    static constexpr int H1_BYTES = NSLAB * TM * 128;
    static constexpr int WAB_BYTES = NSLAB * 2 * S2 * 128;
    static constexpr int AREA = (2 * STAGE > H1_BYTES + WAB_BYTES) ? 2 * STAGE : H1_BYTES + WAB_BYTES;
    static constexpr int LDS = AREA + TM * 4 * 3 + 64;  // + A_raw[128], partial[2][128], scalars
    static_assert(S1 % KB == 0 && S1 % 32 == 0 && S1 <= 128, "fused ABMIL: S1 in {32(bf16: 64),64,128}");
    static_assert((2 * S2) % 32 == 0 && 2 * S2 <= 128, "fused ABMIL: S2 in {16,32,64}");
    // the carve of the kernel's dynamic LDS `s`
    static __device__ __forceinline__ char* h1s(char* s) { return s; }  // h1 image: aliases the stage ring of phase 1 (used after it)
    static __device__ __forceinline__ char* wabs(char* s) { return s + H1_BYTES; }
    static __device__ __forceinline__ float* as(char* s) { return (float*)(s + AREA); }  // A_raw of the tile
    static __device__ __forceinline__ float* ps(char* s) { return as(s) + TM; }          // [2][TM] per-column-wave partial gate sums
    static __device__ __forceinline__ float* sc(char* s) { return ps(s) + 2 * TM; }      // scalars
    // h1 once more, UNROUNDED (fp32 image), behind everything else: only where the launch adds TM * S1 * 4 bytes
    static __device__ __forceinline__ char* h32(char* s) { return s + LDS; }
    // the carve of the K-branch multi-bag kernel (abmil_bags.hip, KMAX = 4 branches): the same AREA, then A_raw[4][128],
    // partial[4][2][128], scalars, and the fp32 h1 image behind them
    static constexpr int KMAX = 4;
    static constexpr int LDS_MB = AREA + TM * 4 * 3 * KMAX + 64;
    static __device__ __forceinline__ float* as_mb(char* s) { return (float*)(s + AREA); }   // [KMAX][TM] A_raw of the tile
    static __device__ __forceinline__ float* ps_mb(char* s) { return as_mb(s) + KMAX * TM; } // [KMAX][2][TM] per-column-wave partial gate sums
    static __device__ __forceinline__ float* sc_mb(char* s) { return ps_mb(s) + 2 * KMAX * TM; }  // [KMAX][2] wave maxima
    static __device__ __forceinline__ char* h32_mb(char* s) { return s + LDS_MB; }
};

// Geometry of the WIDE tile passes (abmil_wide.hip, abmil_wide_mb.hip): a 128-row unit walked as sub-tiles of R rows, the phase-1 ring,
// the h1 image and the ring of the gate passes.  Each kernel's geometry derives from it and adds its own LDS carve behind AREA.
template <typename T, int S1, int S2> struct WG {
    static constexpr int KB = Tr<T>::KB;
    static constexpr int R = 128 / (int)sizeof(T);     // rows of a sub-tile
    static constexpr int NSUB = TM / R;                // sub-tiles of a unit
    static constexpr int NI = R / 16;                  // row fragments, all in every wave
    static constexpr int NJ1 = S1 / 64;                // column fragments per wave, phase 1
    static constexpr int NSLAB = S1 / KB;              // 128-byte slabs of the h1 image
    static constexpr int NXQ = R / 32;                 // LDS-DMA instructions per wave for the X rows of one K-slab
    static constexpr int NWQ = S1 / 32;                // ... for the W1 rows
    static constexpr int STAGE = (R + S1) * 128;
    static constexpr int H1_BYTES = NSLAB * R * 128;   // = S1 * 128
    static constexpr int NP = 2 * S2 < 256 ? 2 * S2 : 256;  // packed gate rows per pass
    static constexpr int NPASS = (2 * S2) / NP;
    static constexpr int NJ2 = NP / 64;                // gate column fragments per wave
    static constexpr int NGQ = NP / 32;                // LDS-DMA instructions per wave for one [Wa; Wb] slab of a pass
    static constexpr int GSTAGE = NP * 128;
    static constexpr int AREA = 2 * STAGE > H1_BYTES + 2 * GSTAGE ? 2 * STAGE : H1_BYTES + 2 * GSTAGE;
    static_assert(S1 % 64 == 0 && S1 % KB == 0, "wide ABMIL: S1 a multiple of 64");
    static_assert((2 * S2) % NP == 0 && NP % 64 == 0, "wide ABMIL: 2 * S2 a multiple of the pass width");
};

// lane geometry of the 256-thread tile kernels, built once per kernel
struct Lanes {
    int tid, lane, wave, wm, wn, g, li;
    int drow;     // LDS-DMA: row within an 8-row instruction block
    int foff[2];  // byte offset of this lane's operand fragment inside a 16-row block of a swizzled image, per K half
    __device__ __forceinline__ Lanes() {
        tid = threadIdx.x, lane = tid & 63;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        wm = wave >> 1, wn = wave & 1;
        g = lane >> 4, li = lane & 15;
        drow = lane >> 3;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) foff[ks] = li * 128 + (((g + 4 * ks) ^ ((lane >> 1) & 7)) << 4);
    }
};

// byte offset of element (row, col) inside the slab-major, swizzled A-operand image of a ROWS-row tile's h1 (the wide passes: a sub-tile)
template <typename T, int ROWS = TM> __device__ __forceinline__ int h1_off(int row, int col) {
    constexpr int KB = Tr<T>::KB, EPC = Tr<T>::EPC;
    const int slab = col / KB, c = (col % KB) / EPC, sub = (col % EPC) * (int)sizeof(T);
    return slab * (ROWS * 128) + row * 128 + ((c ^ ((row >> 1) & 7)) << 4) + sub;
}

// The tile's largest score, in every thread (finite: a tile has >= 1 valid row).  Its barrier also publishes As to the pooling.
__device__ __forceinline__ float tile_max(const Lanes& L, float* Sc, float a_mine) {
    const float mt = wave_max(a_mine);
    if (L.lane == 0 && L.wave < 2) Sc[L.wave] = mt;
    __syncthreads();
    return fmaxf(Sc[0], Sc[1]);
}


// one partial (max, sum, acc[S1]) at pw: wave w holds the c-frags 2w and 2w+1 of acc
template <int S1>
__device__ __forceinline__ void store_partial(const Lanes& L, float* __restrict__ pw, float mx, float sum, const f32x4 (&acc)[2]) {
    if (L.tid == 0) {
        pw[0] = mx;
        pw[1] = sum;
    }
    if (L.li == 0) {
#pragma unroll
        for (int cf = 0; cf < 2; ++cf)
            if ((L.wave * 2 + cf) * 16 < S1)
#pragma unroll
                for (int e = 0; e < 4; ++e) pw[2 + (L.wave * 2 + cf) * 16 + 4 * L.g + e] = acc[cf][e];
    }
}

// Tail of both combine kernels (1024 threads): bag classifier on Ms[S1] (LDS, written by the caller before a barrier), softmax,
// argmax (model_clam.py:180-183).  Ls: C floats of LDS.
__device__ __forceinline__ void bag_head(const float* Ms, float* Ls, int S1, const float* __restrict__ wcls,
                                         const float* __restrict__ bcls, int C, float* __restrict__ logits,
                                         float* __restrict__ Y_prob, int64_t* __restrict__ Y_hat) {
    const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
    for (int k = wv; k < C; k += 16) {
        float a = 0.f;
        for (int c = ln; c < S1; c += 64) a += Ms[c] * wcls[(int64_t)k * S1 + c];
        a = wave_sum(a);
        if (ln == 0) Ls[k] = a + bcls[k];
    }
    __syncthreads();
    if (tid == 0) {
        float lm = -INFINITY;
        int arg = 0;
        for (int k = 0; k < C; ++k)
            if (Ls[k] > lm) {
                lm = Ls[k];
                arg = k;
            }
        float se = 0.f;
        for (int k = 0; k < C; ++k) se += expf(Ls[k] - lm);
        for (int k = 0; k < C; ++k) {
            logits[k] = Ls[k];
            Y_prob[k] = expf(Ls[k] - lm) / se;
        }
        Y_hat[0] = arg;
    }
}

// THE supported [T, S1, S2] set: f(Width<T, S1, S2>{}) for the instantiation of (dtype, s1, s2); false (f not called) if there is none.
template <typename T_, int S1_, int S2_> struct Width { using T = T_; static constexpr int S1 = S1_, S2 = S2_; };
template <typename F> bool visit_width(int dtype, int s1, int s2, F&& f) {
#define HIPT_ABMIL_W(TT, A, B) if (s1 == A && s2 == B) return f(Width<TT, A, B>{}), true;
    if (dtype == HIPT_BF16) {
        HIPT_ABMIL_W(bf16_t, 128, 64) HIPT_ABMIL_W(bf16_t, 128, 32) HIPT_ABMIL_W(bf16_t, 128, 16)
        HIPT_ABMIL_W(bf16_t, 64, 64) HIPT_ABMIL_W(bf16_t, 64, 32) HIPT_ABMIL_W(bf16_t, 64, 16)
    } else {
        HIPT_ABMIL_W(float, 128, 64) HIPT_ABMIL_W(float, 128, 32) HIPT_ABMIL_W(float, 128, 16)
        HIPT_ABMIL_W(float, 64, 64) HIPT_ABMIL_W(float, 64, 32) HIPT_ABMIL_W(float, 64, 16)
        HIPT_ABMIL_W(float, 32, 64) HIPT_ABMIL_W(float, 32, 32) HIPT_ABMIL_W(float, 32, 16)
    }
#undef HIPT_ABMIL_W
    return false;
}

// The NARROW set of the ragged multi-bag tile kernel of abmil_narrow.hip (hipt_smallest [., 8, 4], hipt_smaller [., 16, 8], [., 32, 8],
// [., 32, 16]), each in both dtypes: a table of its own, so that visit_width keeps answering as it does.  fp32 (32, 16) is in both.
template <typename F> bool visit_narrow(int dtype, int s1, int s2, F&& f) {
#define HIPT_ABMIL_N(TT, A, B) if (s1 == A && s2 == B) return f(Width<TT, A, B>{}), true;
    if (dtype == HIPT_BF16) {
        HIPT_ABMIL_N(bf16_t, 8, 4) HIPT_ABMIL_N(bf16_t, 16, 8) HIPT_ABMIL_N(bf16_t, 32, 8) HIPT_ABMIL_N(bf16_t, 32, 16)
    } else if (dtype == HIPT_F32) {
        HIPT_ABMIL_N(float, 8, 4) HIPT_ABMIL_N(float, 16, 8) HIPT_ABMIL_N(float, 32, 8) HIPT_ABMIL_N(float, 32, 16)
    }
#undef HIPT_ABMIL_N
    return false;
}

// The WIDE set of the ragged multi-bag tile kernel of abmil_wide.hip (small_resnet18 / tiny [., 256, 64], small [., 512, 256], big
// [., 512, 384]), each in both dtypes: again a table of its own.
template <typename F> bool visit_wide(int dtype, int s1, int s2, F&& f) {
#define HIPT_ABMIL_WD(TT, A, B) if (s1 == A && s2 == B) return f(Width<TT, A, B>{}), true;
    if (dtype == HIPT_BF16) {
        HIPT_ABMIL_WD(bf16_t, 256, 64) HIPT_ABMIL_WD(bf16_t, 512, 256) HIPT_ABMIL_WD(bf16_t, 512, 384)
    } else if (dtype == HIPT_F32) {
        HIPT_ABMIL_WD(float, 256, 64) HIPT_ABMIL_WD(float, 512, 256) HIPT_ABMIL_WD(float, 512, 384)
    }
#undef HIPT_ABMIL_WD
    return false;
}

// ---- the multi-bag tile passes (abmil_bags.hip, abmil_narrow.hip, abmil_wide.hip) ----
// A work unit: rows [m0, min(m0 + TM, end)) of the concatenated matrix; m0 < 0: no unit (the table is sized from an upper bound)
struct BagUnit { int64_t m0, end; };

// Workgroups of a tile pass over max_units units: two per CU fit (launch bounds), four waves of units keep the tail short.
// HIPT_BAGS_MAX_WG (1..) lowers the cap for A/B runs and tests: the results do not depend on it.
inline int tile_pass_grid(int max_units) {
    int cap = 2048;
    if (const char* e = getenv("HIPT_BAGS_MAX_WG")) {
        const int v = atoi(e);
        if (v >= 1 && v < cap) cap = v;
    }
    return max_units < cap ? max_units : cap;
}

// The launch of every tile pass: the grid over max_units, this kernel instantiation's per-device setup (the dynamic-LDS opt-in, under
// the family name the error texts carry), 256 threads.  `args` are the kernel's arguments.
template <auto Kernel, typename... Args>
int launch_tile_pass(int lds, const char* family, int max_units, hipStream_t st, Args... args) {
    static DeviceSetup setup;  // one per kernel instantiation
    if (int rc = setup({(const void*)Kernel}, lds, family)) return rc;
    hipLaunchKernelGGL(Kernel, dim3(tile_pass_grid(max_units)), dim3(256), lds, st, args...);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

}  // namespace abmil_tile
