// The tile pass of the ragged multi-bag CLAM_MB forward for the WIDE gated heads: abmil_wide.hip's sub-tile walk carrying K = w->n_att
// (2 .. 4) score vectors and K poolings instead of one.  (S1, S2) in {(256, 64), (512, 256), (512, 384)} (abmil_tile.h: visit_wide); the
// unit table is abmil_bags.hip's and the partials are laid out as hipt_clam_bags_mb_tiles_launch writes them -- K records
// (max, sum, acc[S1]) per unit, branch k of unit u at partials[(u * K + k) * (2 + S1)] -- so hipt_clam_bags_mb_combine_launch serves it.
// W1 and [Wa; Wb] are shared by the branches.  Per sub-tile of R = 128 / sizeof(T) rows, ONCE whatever K is: phase 1 through the
// two-stage LDS-DMA ring, h1 = ReLU(acc + b1) left unrounded in the accumulators with its T-rounded operand image in LDS, the whole gate
// GEMM in passes of NP = min(2 * S2, 256) packed rows through the second ring, and tanh * sigmoid of every gate unit.  PER BRANCH k:
//   score    the gate unit times wc[k][j], summed pass after pass in registers, then the two lane-group shuffles, then the four waves in
//            wave order through LDS, + bc[k]; A_raw[k * a_stride + m] for the real rows;
//   pooling  sub-tile max, p = exp(A - m) (rows past the bag's end carry -inf: exactly 0), sum_r p_r h1[r][c] from the accumulators (row
//            fragments in order, then the fixed 16-lane shuffle tree), folded into branch k's running record (m, l, o[S1]) in sub-tile
//            order (online softmax).
// The K running records do not fit in registers beside the accumulators (the one-branch kernel's o_run alone is S1 / 16 registers), so
// they live in LDS: o[K][S1] floats, each element read and written by ONE thread only (lane li = 0 of the column's owner) -- no barrier
// guards them --, and (m, l) once per wave (every lane of a wave reads, then writes, the same numbers).
// Rounding model, per branch that of abmil_wide.hip: bf16 bag, W1, Wa, Wb; h1 rounded to bf16 as the gate GEMM's operand only; the gate,
// the K scores and the K poolings fp32 on unrounded h1.  fp32: nothing is rounded.
// A unit's result does not depend on the workgroup that ran it: no atomics, no tickets, nothing kept in the workspace.
// Shared with abmil_wide.hip as code (abmil_tile.h): the geometry WG, h1_off<T, R> and the launcher.  Still a written-out copy of that
// file's text: the unit loop up to acc2 (row addresses and stage, the phase-1 ring, stage_g, the ReLU / h1 image, the gate GEMM passes).
// One body for both kernels changed the device code of all 12 instantiations and was put back (DESIGN.md sections 16 item 2 and 33).
#include "abmil_tile.h"
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace {
using namespace abmil_tile;

constexpr int KMAX = 4;  // attention branches a workgroup's LDS holds running records for

// abmil_tile.h's wide geometry, and behind its AREA the K-fold carve: A_raw[KMAX][R], gate sums [KMAX][4][R], running acc [KMAX][S1],
// running (m, l) [4 waves][KMAX][2]
template <typename T, int S1, int S2> struct WGk : WG<T, S1, S2> {
    using G = WG<T, S1, S2>;
    static constexpr int LDS = G::AREA + KMAX * (G::R + 4 * G::R) * 4 + KMAX * S1 * 4 + 4 * KMAX * 2 * 4;
    static_assert(KMAX * G::R <= 256, "wide ABMIL MB: one thread per (branch, row)");
    static_assert(LDS <= 160 * 1024, "wide ABMIL MB: LDS");
};

template <typename T, int S1, int S2>
__global__ __launch_bounds__(256) void abmil_wide_mb_kernel(const T* __restrict__ bag, const BagUnit* __restrict__ units, int max_units,
                                                            int S0, const T* __restrict__ w1, const float* __restrict__ b1,
                                                            const T* __restrict__ wab, const float* __restrict__ bab,
                                                            const float* __restrict__ wc, const float* __restrict__ bc, int K,
                                                            int64_t a_stride, float* __restrict__ A_raw, float* __restrict__ partials,
                                                            int attention_only) {
    using G = WGk<T, S1, S2>;
    constexpr int EPC = Tr<T>::EPC, R = G::R, NI = G::NI, NJ1 = G::NJ1, NJ2 = G::NJ2, NP = G::NP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* H1s = smem;                         // h1 operand image: aliases the ring of phase 1 (used after it)
    char* Gs = smem + G::H1_BYTES;            // [2][NP][128 B] ring of the [Wa; Wb] slabs
    float* As = (float*)(smem + G::AREA);     // [KMAX][R] A_raw of the sub-tile, branch by branch
    float* Ps = As + KMAX * R;                // [KMAX][4][R] gate sums of the four column waves
    float* Os = Ps + KMAX * 4 * R;            // [KMAX][S1] running acc of the unit: element (k, c) belongs to ONE thread
    float* Ml = Os + KMAX * S1;               // [4][KMAX][2] running (m, l) of the unit, a copy per wave

    const Lanes L;
    const int tid = L.tid, lane = L.lane, wave = L.wave, g = L.g, li = L.li, drow = L.drow;
    const int* foff = L.foff;
    const int nk = S0 / G::KB;
    float* Mw = Ml + wave * (KMAX * 2);
    float* Ow = Os + wave * (S1 / 4) + 4 * g;  // + k * S1 + j * 16: this lane group's four columns of fragment j (lane li = 0 owns them)

    for (int unit = blockIdx.x; unit < max_units; unit += gridDim.x) {
        const BagUnit un = units[unit];
        const int64_t m0 = un.m0, mend = un.end;
        if (m0 < 0) break;  // uniform; the surplus entries are the table's tail
        // the unit's K running records: (-inf, 0, zeros).  Written and read by the same threads throughout: no barrier
        if (!attention_only) {
            for (int k = 0; k < K; ++k) {
                if (lane == 0) {
                    Mw[k * 2] = -INFINITY;
                    Mw[k * 2 + 1] = 0.f;
                }
                if (li == 0) {
#pragma unroll
                    for (int j = 0; j < NJ1; ++j) *(f32x4*)(Ow + k * S1 + j * 16) = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
        }

        for (int sub = 0; sub < G::NSUB; ++sub) {
            const int64_t ms0 = m0 + sub * R;
            if (ms0 >= mend) break;  // uniform: the first sub-tile of a unit always has a row
            // ---------------- phase 1: h1pre = bag_subtile @ W1^T ----------------
            // the S1 / 8 row addresses of W1 are built HERE, per sub-tile, from a row index the compiler cannot see through: hoisted out of the
            // unit loop they stay live across the gate and the pooling (S1 / 16 registers), which the S1 = 512 bf16 instantiations pay in scratch
            int drow_s = drow;
            asm volatile("" : "+v"(drow_s));
            const T* xsrc[G::NXQ];
            int xch[G::NXQ];
#pragma unroll
            for (int q = 0; q < G::NXQ; ++q) {
                const int r = (wave * G::NXQ + q) * 8 + drow;
                int64_t m = ms0 + r;
                m = m < mend ? m : mend - 1;  // rows past the bag's end re-read its last row; masked below
                xsrc[q] = bag + m * S0;
                xch[q] = (lane & 7) ^ ((r >> 1) & 7);
            }
            auto stage = [&](int s, int kt) {
                char* sa = smem + s * G::STAGE;
#pragma unroll
                for (int q = 0; q < G::NXQ; ++q) glds16(xsrc[q] + (kt * 8 + xch[q]) * EPC, sa + (wave * G::NXQ + q) * 1024);
#pragma unroll
                for (int q = 0; q < G::NWQ; ++q) {  // S1 rows of W1: S1 / 8 instructions over 4 waves
                    const int r = (wave * G::NWQ + q) * 8 + drow_s;
                    glds16(w1 + (int64_t)r * S0 + (kt * 8 + ((lane & 7) ^ ((r >> 1) & 7))) * EPC,
                           sa + R * 128 + (wave * G::NWQ + q) * 1024);
                }
            };
            f32x4 acc1[NI][NJ1];
#pragma unroll
            for (int i = 0; i < NI; ++i)
#pragma unroll
                for (int j = 0; j < NJ1; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

            __syncthreads();  // previous sub-tile's readers of the aliased area, As and Ps are done
            stage(0, 0);
            wait_vm0();
            __syncthreads();
            int cur = 0;
            for (int kt = 0; kt < nk; ++kt) {
                if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
                const char* sa = smem + cur * G::STAGE;
                const char* sw = smem + cur * G::STAGE + R * 128 + wave * (S1 / 4) * 128;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    u32x4 af[NI], wf[NJ1];
#pragma unroll
                    for (int i = 0; i < NI; ++i) af[i] = *(const u32x4*)(sa + i * 16 * 128 + foff[ks]);
#pragma unroll
                    for (int j = 0; j < NJ1; ++j) wf[j] = *(const u32x4*)(sw + j * 16 * 128 + foff[ks]);
#pragma unroll
                    for (int i = 0; i < NI; ++i)
#pragma unroll
                        for (int j = 0; j < NJ1; ++j) Tr<T>::mma16(acc1[i][j], wf[j], af[i]);
                }
                wait_vm0();
                __syncthreads();
                cur ^= 1;
            }
            // ---------------- the gate's ring: slab `it` = (pass, K-slab) of [Wa; Wb], rows interleaved a,a,b,b ----------------
            // packed row pr: quad = pr>>2, pos = pr&3 -> source row (pos>>1)*S2 + quad*2 + (pos&1)
            auto stage_g = [&](int s, int it) {
                const int p = it / G::NSLAB, sl = it % G::NSLAB;
#pragma unroll
                for (int q = 0; q < G::NGQ; ++q) {
                    const int blk = wave * G::NGQ + q;
                    const int r = blk * 8 + drow, pr = p * NP + r;
                    const int srow = ((pr & 3) >> 1) * S2 + (pr >> 2) * 2 + (pr & 1);
                    glds16(wab + (int64_t)srow * S1 + (sl * 8 + ((lane & 7) ^ ((r >> 1) & 7))) * EPC, Gs + s * G::GSTAGE + blk * 1024);
                }
            };
            stage_g(0, 0);  // behind the h1 image: the ring of phase 1 has no reader left (the loop's last barrier)
            // ---------------- h1 = ReLU(acc1 + b1): fp32 in place, rounded to T -> LDS operand image ----------------
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                const int row = i * 16 + li;
#pragma unroll
                for (int j = 0; j < NJ1; ++j) {
                    const int col = wave * (S1 / 4) + j * 16 + 4 * g;
                    f32x4 v = acc1[i][j] + *(const f32x4*)(b1 + col);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
                    acc1[i][j] = v;
                    store4<T>((T*)(H1s + h1_off<T, R>(row, col)), v);
                }
            }
            wait_vm0();
            __syncthreads();
            // ---------------- gate: ab = h1 @ [Wa;Wb]^T pass by pass; tanh * sigmoid once per gate unit, times wc[k] into K scores ----------------
            float gate[KMAX][NI];
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
#pragma unroll
                for (int i = 0; i < NI; ++i) gate[k][i] = 0.f;
            cur = 0;
#pragma unroll 1
            for (int p = 0; p < G::NPASS; ++p) {
                f32x4 acc2[NI][NJ2];
#pragma unroll
                for (int i = 0; i < NI; ++i)
#pragma unroll
                    for (int j = 0; j < NJ2; ++j) acc2[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
                for (int sl = 0; sl < G::NSLAB; ++sl) {
                    const int it = p * G::NSLAB + sl;
                    if (it + 1 < G::NPASS * G::NSLAB) stage_g(cur ^ 1, it + 1);
                    const char* sa = H1s + sl * (R * 128);
                    const char* sw = Gs + cur * G::GSTAGE + wave * (NP / 4) * 128;
#pragma unroll
                    for (int ks = 0; ks < 2; ++ks) {
                        u32x4 af[NI], wf[NJ2];
#pragma unroll
                        for (int i = 0; i < NI; ++i) af[i] = *(const u32x4*)(sa + i * 16 * 128 + foff[ks]);
#pragma unroll
                        for (int j = 0; j < NJ2; ++j) wf[j] = *(const u32x4*)(sw + j * 16 * 128 + foff[ks]);
#pragma unroll
                        for (int i = 0; i < NI; ++i)
#pragma unroll
                            for (int j = 0; j < NJ2; ++j) Tr<T>::mma16(acc2[i][j], wf[j], af[i]);
                    }
                    wait_vm0();
                    __syncthreads();
                    cur ^= 1;
                }
#pragma unroll
                for (int j = 0; j < NJ2; ++j) {
                    const int r0 = p * NP + wave * (NP / 4) + j * 16 + 4 * g;  // packed row of element 0
                    const int j0 = (r0 >> 2) * 2;                              // gate unit of elements 0 (a) and 2 (b); j0+1 for 1 and 3
                    const float ba0 = bab[j0], ba1 = bab[j0 + 1], bb0 = bab[S2 + j0], bb1 = bab[S2 + j0 + 1];
                    float c0[KMAX], c1[KMAX];  // rows k >= K carry a zero weight and are never stored
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) {
                        c0[k] = k < K ? wc[k * S2 + j0] : 0.f;
                        c1[k] = k < K ? wc[k * S2 + j0 + 1] : 0.f;
                    }
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        const f32x4 v = acc2[i][j];
                        const float t0 = tanh_f(v[0] + ba0) * sigmoid_f(v[2] + bb0);
                        const float t1 = tanh_f(v[1] + ba1) * sigmoid_f(v[3] + bb1);
#pragma unroll
                        for (int k = 0; k < KMAX; ++k) gate[k][i] += t0 * c0[k] + t1 * c1[k];
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (k < K) {  // uniform
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        float v = gate[k][i];
                        v += __shfl_xor(v, 16, 64);
                        v += __shfl_xor(v, 32, 64);
                        if (g == 0) Ps[(k * 4 + wave) * R + i * 16 + li] = v;
                    }
                }
            __syncthreads();
            if (tid < K * R) {  // thread (k, r) owns branch k of row r of the sub-tile
                const int k = tid / R, r = tid % R;
                const int64_t m = ms0 + r;
                const float* Pk = Ps + k * 4 * R + r;
                float a = -INFINITY;
                if (m < mend) {
                    a = ((Pk[0] + Pk[R]) + Pk[2 * R]) + Pk[3 * R] + bc[k];
                    A_raw[(int64_t)k * a_stride + m] = a;
                }
                As[k * R + r] = a;
            }
            if (attention_only) continue;  // uniform
            __syncthreads();
            // ---------------- pooling of THIS sub-tile from the accumulators, branch after branch, folded into the branch's record ----------------
#pragma unroll 1
            for (int k = 0; k < K; ++k) {
                const float* Ak = As + k * R;
                const float m_s = wave_max(Ak[lane & (R - 1)]);  // finite: the sub-tile has a row; the same bits in every wave
                float p[NI], l_s = 0.f;
#pragma unroll
                for (int i = 0; i < NI; ++i) {
                    p[i] = expf(Ak[i * 16 + li] - m_s);  // rows past the end carry -inf -> exactly 0
                    l_s += p[i];
                }
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) l_s += __shfl_xor(l_s, o, 64);
                const float m_run = Mw[k * 2], l_run = Mw[k * 2 + 1];
                const float m_new = fmaxf(m_run, m_s);
                const float f_run = expf(m_run - m_new), f_s = expf(m_s - m_new);  // first sub-tile: exp(-inf) = 0 against zeros
                if (lane == 0) {
                    Mw[k * 2] = m_new;
                    Mw[k * 2 + 1] = l_run * f_run + l_s * f_s;
                }
#pragma unroll
                for (int j = 0; j < NJ1; ++j) {
                    f32x4 o_s;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float s = 0.f;
#pragma unroll
                        for (int i = 0; i < NI; ++i) s = fmaf(p[i], acc1[i][j][e], s);
#pragma unroll
                        for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o, 64);
                        o_s[e] = s;
                    }
                    if (li == 0) {
                        f32x4* po = (f32x4*)(Ow + k * S1 + j * 16);
                        const f32x4 o_run = *po;
#pragma unroll
                        for (int e = 0; e < 4; ++e) o_s[e] = o_run[e] * f_run + o_s[e] * f_s;
                        *po = o_s;
                    }
                }
            }
        }
        if (attention_only) continue;  // uniform
        // ---------------- the unit's K partials: (max, sum, acc[S1]) each ----------------
        for (int k = 0; k < K; ++k) {
            float* pw = partials + ((int64_t)unit * K + k) * (2 + S1);
            if (tid == 0) {
                pw[0] = Mw[k * 2];
                pw[1] = Mw[k * 2 + 1];
            }
            if (li == 0) {
#pragma unroll
                for (int j = 0; j < NJ1; ++j) {
                    const f32x4 o = *(const f32x4*)(Ow + k * S1 + j * 16);
#pragma unroll
                    for (int e = 0; e < 4; ++e) pw[2 + wave * (S1 / 4) + j * 16 + 4 * g + e] = o[e];
                }
            }
        }
    }
}

template <typename T, int S1, int S2>
int launch_wide_mb(const hipt_clam_weights* w, const void* bags, const void* units, int max_units, int attention_only, int64_t a_stride,
                   float* A_raw, float* partials, hipStream_t st) {
    return launch_tile_pass<abmil_wide_mb_kernel<T, S1, S2>>(WGk<T, S1, S2>::LDS, "abmil_wide_mb", max_units, st, (const T*)bags,
                                                             (const BagUnit*)units, max_units, w->s0, (const T*)w->w1, w->b1,
                                                             (const T*)w->wab, w->bab, w->wc, w->bc, w->n_att, a_stride, A_raw,
                                                             partials, attention_only);
}

}  // namespace

int hipt_clam_wide_mb_tiles_launch(const hipt_clam_weights* w, const void* bags, const void* units, int max_units, int attention_only,
                                   int64_t a_stride, float* A_raw, float* partials, hipStream_t st) {
    if (w->n_att < 2 || w->n_att > KMAX) {
        hipt_set_error("clam mb wide bags: %d branches (2..%d)", w->n_att, KMAX);
        return HIPT_E_UNSUPPORTED;
    }
    int rc = HIPT_E_UNSUPPORTED;
    const bool found = visit_wide(w->dtype, w->s1, w->s2, [&](auto wd) {
        using W = decltype(wd);
        rc = launch_wide_mb<typename W::T, W::S1, W::S2>(w, bags, units, max_units, attention_only, a_stride, A_raw, partials, st);
    });
    if (!found) hipt_set_error("clam mb wide bags: unsupported widths");
    return rc;
}
