// CLAM_MB over MANY bags in one call with 5 .. 8 attention branches (ovarian_5class and wider tasks): the tile pass of abmil_bags.hip's
// abmil_bags_mb_kernel (K <= 4) for K <= 8, a kernel of its own so that the K <= 4 instantiations keep their device code (DESIGN.md
// sections 17 and 34).  The unit table (bags_units_kernel), the 128-row units that never span two bags, BagUnit, tile_pass_grid and the
// combine (abmil_bags_mb_combine_kernel, general in K) are abmil_bags.hip's as they stand.
//   once per unit   phase 1 (bag_tile @ W1^T through the two-stage LDS-DMA ring), the ReLU image (bf16: + the fp32 h1 image of the
//                   pooling), the [Wa; Wb] image and the gate GEMM: abmil_bags_mb_kernel's statements;
//   gate epilogue   tanh * sigmoid once per gate unit; the branches are walked in GROUPS OF FOUR, each group with the K <= 4 kernel's
//                   statement sequence on the gate products t0, t1 of the current column fragment, which stay in registers across the
//                   groups (the second group costs its gate[4][4] rows and nothing else);
//   pooling         branch after branch on the matrix pipe against the fp32 h1, as in the K <= 4 kernel.
// Every branch's arithmetic is the K <= 4 kernel's for a branch, operation for operation: the j order of the weighted sum, quad_sum,
// Ps[k][0] + Ps[k][1] + bc[k], the mb / cf order of the pooling MFMAs.  Hence branch k of a K-branch call has the bits of the same branch
// in a call of the K <= 4 kernel on a model made of a subset of the branches (tests/test_gpu_clam_mb_many.py holds this).
// No atomics, no tickets, no state between calls: the call can be captured in a graph.
// Shared with abmil_bags.hip as code (abmil_tile.h): AG, Lanes, h1_off, store_partial and the launcher.  Still a written-out copy of
// abmil_bags_mb_kernel's text: everything "once per unit" above and the pooling.  Either kernel's text behind a function boundary
// compiles to other device code, so one body for the pair was not kept (DESIGN.md sections 16 item 2 and 34).
#include "abmil_tile.h"
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace {
using namespace abmil_tile;

// The carve of this kernel's dynamic LDS: AG's AREA (stage ring / h1 image + [Wa; Wb] image), then A_raw[8][128], partial[8][2][128],
// the 8 x 2 wave maxima, and in bf16 the fp32 h1 image behind them.  [., 128, 64]: 143 424 B in both dtypes (fp32: AREA 131 072;
// bf16: AREA 65 536 + the 65 536 B fp32 h1 image), one workgroup per CU.
template <typename T, int S1, int S2> struct AG8 {
    using G = AG<T, S1, S2>;
    static constexpr int KMAX = 8, KGRP = 4;  // branches; branches per group of the gate epilogue (= the K <= 4 kernel's register row)
    static constexpr int LDS = G::AREA + TM * 4 * 3 * KMAX + 64;
    static constexpr int LDS_ALL = LDS + (sizeof(T) == 2 ? TM * S1 * 4 : 0);
    static_assert(KMAX * 2 * 4 <= 64, "the scalars hold KMAX x 2 wave maxima");
    static_assert(LDS_ALL <= 160 * 1024, "the carve fits the CU's LDS");
    // workgroups per CU that the carve admits (the CU has 160 KiB): one at S1 = 128, where the kernel may then use the whole register file
    static constexpr int WG_PER_CU = 2 * LDS_ALL <= 160 * 1024 ? 2 : 1;
    static __device__ __forceinline__ float* as(char* s) { return (float*)(s + G::AREA); }  // [KMAX][TM] A_raw of the tile
    static __device__ __forceinline__ float* ps(char* s) { return as(s) + KMAX * TM; }      // [KMAX][2][TM] per-column-wave partial gate sums
    static __device__ __forceinline__ float* sc(char* s) { return ps(s) + 2 * KMAX * TM; }  // [KMAX][2] wave maxima
    static __device__ __forceinline__ char* h32(char* s) { return s + LDS; }
};

template <typename T, int S1, int S2>
__global__ __launch_bounds__(256, (AG8<T, S1, S2>::WG_PER_CU)) void abmil_bags_mb8_kernel(const T* __restrict__ bag,
                                                                const BagUnit* __restrict__ units,
                                                                int max_units, int S0, const T* __restrict__ w1,
                                                                const float* __restrict__ b1, const T* __restrict__ wab,
                                                                const float* __restrict__ bab, const float* __restrict__ wc,
                                                                const float* __restrict__ bc, int K, int64_t a_stride,
                                                                float* __restrict__ A_raw, float* __restrict__ partials,
                                                                int attention_only) {
    using G = AG<T, S1, S2>;
    using G8 = AG8<T, S1, S2>;
    constexpr int EPC = Tr<T>::EPC, KMAX = G8::KMAX, KGRP = G8::KGRP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* H1s = G::h1s(smem);
    char* Wabs = G::wabs(smem);
    float *As = G8::as(smem), *Ps = G8::ps(smem), *Sc = G8::sc(smem);
    constexpr bool POOL32 = sizeof(T) == 2;
    char* Hp = POOL32 ? G8::h32(smem) : H1s;

    const Lanes L;
    const int tid = L.tid, lane = L.lane, wave = L.wave, wm = L.wm, wn = L.wn, g = L.g, li = L.li, drow = L.drow;
    const int* foff = L.foff;
    const int nk = S0 / G::KB;

    for (int unit = blockIdx.x; unit < max_units; unit += gridDim.x) {
        const BagUnit un = units[unit];
        const int64_t m0 = un.m0, mend = un.end;
        if (m0 < 0) break;  // uniform; the surplus entries are the table's tail
        // ---------------- phase 1: h1pre = bag_tile @ W1^T ----------------
        const T* xsrc[4];
        int xch[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = (wave * 4 + q) * 8 + drow;
            int64_t m = m0 + r;
            m = m < mend ? m : mend - 1;  // rows past the bag's end re-read its last row; masked below
            xsrc[q] = bag + m * S0;
            xch[q] = (lane & 7) ^ ((r >> 1) & 7);
        }
        auto stage = [&](int s, int kt) {
            char* sa = smem + s * G::STAGE;
#pragma unroll
            for (int q = 0; q < 4; ++q) glds16(xsrc[q] + (kt * 8 + xch[q]) * EPC, sa + (wave * 4 + q) * 1024);
#pragma unroll
            for (int q = 0; q < S1 / 32; ++q) {
                const int r = (wave * (S1 / 32) + q) * 8 + drow;
                glds16(w1 + (int64_t)r * S0 + (kt * 8 + ((lane & 7) ^ ((r >> 1) & 7))) * EPC,
                       sa + TM * 128 + (wave * (S1 / 32) + q) * 1024);
            }
        };
        f32x4 acc1[4][G::NJ1];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < G::NJ1; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        __syncthreads();  // previous unit's readers of the aliased area are done
        stage(0, 0);
        wait_vm0();
        __syncthreads();
        int cur = 0;
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
            const char* sa = smem + cur * G::STAGE + wm * 64 * 128;
            const char* sw = smem + cur * G::STAGE + TM * 128 + wn * (S1 / 2) * 128;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 af[4], wf[G::NJ1];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *(const u32x4*)(sa + i * 16 * 128 + foff[ks]);
#pragma unroll
                for (int j = 0; j < G::NJ1; ++j) wf[j] = *(const u32x4*)(sw + j * 16 * 128 + foff[ks]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < G::NJ1; ++j) Tr<T>::mma16(acc1[i][j], wf[j], af[i]);
            }
            wait_vm0();
            __syncthreads();
            cur ^= 1;
        }
        // ---------------- [Wa;Wb] image by LDS-DMA (rows interleaved a,a,b,b) ----------------
#pragma unroll
        for (int sl = 0; sl < G::NSLAB; ++sl)
#pragma unroll
            for (int q = 0; q < (2 * S2) / 32; ++q) {
                const int blk = wave * ((2 * S2) / 32) + q;
                const int r = blk * 8 + drow;
                const int srow = ((r & 3) >> 1) * S2 + (r >> 2) * 2 + (r & 1);
                glds16(wab + (int64_t)srow * S1 + (sl * 8 + ((lane & 7) ^ ((r >> 1) & 7))) * EPC,
                       Wabs + sl * (2 * S2 * 128) + blk * 1024);
            }
        // ---------------- h1 = ReLU(acc1 + b1) -> LDS image ----------------
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = wm * 64 + i * 16 + li;
#pragma unroll
            for (int j = 0; j < G::NJ1; ++j) {
                const int col = wn * (S1 / 2) + j * 16 + 4 * g;
                f32x4 v = acc1[i][j] + *(const f32x4*)(b1 + col);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                store4<T>((T*)(H1s + h1_off<T>(row, col)), v);
                if constexpr (POOL32)
                    if (!attention_only) store4<float>((float*)(Hp + h1_off<float>(row, col)), v);
            }
        }
        wait_vm0();
        __syncthreads();
        // ---------------- phase 2: ab = h1 @ [Wa;Wb]^T, gate once, K weighted sums ----------------
        f32x4 acc2[4][G::NJ2];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < G::NJ2; ++j) acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int sl = 0; sl < G::NSLAB; ++sl) {
            const char* sa = H1s + sl * (TM * 128) + wm * 64 * 128;
            const char* sw = Wabs + sl * (2 * S2 * 128) + wn * S2 * 128;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 af[4], wf[G::NJ2];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *(const u32x4*)(sa + i * 16 * 128 + foff[ks]);
#pragma unroll
                for (int j = 0; j < G::NJ2; ++j) wf[j] = *(const u32x4*)(sw + j * 16 * 128 + foff[ks]);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < G::NJ2; ++j) Tr<T>::mma16(acc2[i][j], wf[j], af[i]);
            }
        }
        {
            float gate[KMAX / KGRP][KGRP][4];
#pragma unroll
            for (int q = 0; q < KMAX / KGRP; ++q)
#pragma unroll
                for (int k = 0; k < KGRP; ++k)
#pragma unroll
                    for (int i = 0; i < 4; ++i) gate[q][k][i] = 0.f;
#pragma unroll
            for (int j = 0; j < G::NJ2; ++j) {
                const int r0 = wn * S2 + j * 16 + 4 * g;  // packed row of element 0
                const int j0 = (r0 >> 2) * 2;             // gate unit of elements 0 (a) and 2 (b); j0+1 for 1 and 3
                const float ba0 = bab[j0], ba1 = bab[j0 + 1], bb0 = bab[S2 + j0], bb1 = bab[S2 + j0 + 1];
                float t0[4], t1[4];  // the gate products of this column fragment: formed once, used by both groups
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 v = acc2[i][j];
                    t0[i] = tanh_f(v[0] + ba0) * sigmoid_f(v[2] + bb0);
                    t1[i] = tanh_f(v[1] + ba1) * sigmoid_f(v[3] + bb1);
                }
#pragma unroll
                for (int q = 0; q < KMAX / KGRP; ++q) {
                    float c0[KGRP], c1[KGRP];
#pragma unroll
                    for (int k = 0; k < KGRP; ++k) {
                        c0[k] = q * KGRP + k < K ? wc[(q * KGRP + k) * S2 + j0] : 0.f;
                        c1[k] = q * KGRP + k < K ? wc[(q * KGRP + k) * S2 + j0 + 1] : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i)
#pragma unroll
                        for (int k = 0; k < KGRP; ++k) gate[q][k][i] += t0[i] * c0[k] + t1[i] * c1[k];
                }
            }
#pragma unroll
            for (int q = 0; q < KMAX / KGRP; ++q)
#pragma unroll
                for (int k = 0; k < KGRP; ++k)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = quad_sum(gate[q][k][i]);
                        if (g == 0) Ps[((q * KGRP + k) * 2 + wn) * TM + wm * 64 + i * 16 + li] = v;
                    }
        }
        __syncthreads();
        float a_mine[KMAX];  // threads 0..127 own one row each
#pragma unroll
        for (int k = 0; k < KMAX; ++k) a_mine[k] = -INFINITY;
        if (tid < TM) {
            const int64_t m = m0 + tid;
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) {
                    if (m < mend) {
                        a_mine[k] = Ps[(k * 2) * TM + tid] + Ps[(k * 2 + 1) * TM + tid] + bc[k];
                        A_raw[(int64_t)k * a_stride + m] = a_mine[k];
                    }
                    As[k * TM + tid] = a_mine[k];
                }
        }
        if (attention_only) continue;  // uniform
        // ---------------- the K tile maxima (finite: a tile has >= 1 valid row); the barrier also publishes As ----------------
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
            const float mt = wave_max(a_mine[k]);
            if (lane == 0 && wave < 2) Sc[k * 2 + wave] = mt;
        }
        __syncthreads();
        // ---------------- pooling of THIS tile, branch after branch: softmax numerator + p^T h1 (fp32 weights, fp32 h1) ----------------
        for (int k = 0; k < K; ++k) {
            const float m_new = fmaxf(Sc[k * 2], Sc[k * 2 + 1]);
            const float* Ak = As + k * TM;
            float lsum = 0.f;
            f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int mb = 0; mb < TM; mb += 16) {
                u32x4 pf;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = expf(Ak[mb + 4 * g + e] - m_new);
                    lsum += p;
                    pf[e] = __builtin_bit_cast(uint32_t, p);
                }
#pragma unroll
                for (int cf = 0; cf < 2; ++cf) {
                    const int col = (wave * 2 + cf) * 16 + li;
                    if ((wave * 2 + cf) * 16 < S1) {
                        u32x4 hf;
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            hf[e] = *(const uint32_t*)(Hp + h1_off<float>(mb + 4 * g + e, col));
                        Tr<float>::mma16(o[cf], hf, pf);
                    }
                }
            }
            lsum = quad_sum(lsum);
            store_partial<S1>(L, partials + ((int64_t)unit * K + k) * (2 + S1), m_new, lsum, o);
        }
    }
}

template <typename T, int S1, int S2>
int launch_bags_mb8(const hipt_clam_weights* w, const void* bags, const void* units, int max_units, int attention_only,
                    int64_t a_stride, float* A_raw, float* partials, hipStream_t st) {
    constexpr int LDS = AG8<T, S1, S2>::LDS_ALL;  // bf16: with the fp32 h1 image of the pooling (<= 143 424 B of the CU's 163 840)
    return launch_tile_pass<abmil_bags_mb8_kernel<T, S1, S2>>(LDS, "abmil_bags_mb8", max_units, st, (const T*)bags, (const BagUnit*)units,
                                                              max_units, w->s0, (const T*)w->w1, w->b1, (const T*)w->wab, w->bab, w->wc,
                                                              w->bc, w->n_att, a_stride, A_raw, partials, attention_only);
}

}  // namespace

int hipt_clam_bags_mb8_tiles_launch(const hipt_clam_weights* w, const void* bags, const void* units, int max_units,
                                    int attention_only, int64_t a_stride, float* A_raw, float* partials, hipStream_t st) {
    if (w->n_att < 5 || w->n_att > AG8<float, 128, 64>::KMAX) {
        hipt_set_error("clam mb many bags: %d branches (5..%d)", w->n_att, AG8<float, 128, 64>::KMAX);
        return HIPT_E_UNSUPPORTED;
    }
    int rc = HIPT_E_UNSUPPORTED;
    const bool found = visit_width(w->dtype, w->s1, w->s2, [&](auto wd) {
        using W = decltype(wd);
        rc = launch_bags_mb8<typename W::T, W::S1, W::S2>(w, bags, units, max_units, attention_only, a_stride, A_raw, partials, st);
    });
    if (!found) hipt_set_error("clam mb many bags: unsupported widths");
    return rc;
}
