// The tile pass of the ragged multi-bag CLAM_SB forward (abmil_bags.hip) for the WIDE gated heads: (S1, S2) in {(256, 64), (512, 256),
// (512, 384)} (small_resnet18 [512, 256, 64], tiny [1024, 256, 64], small [1024, 512, 256], big [1024, 512, 384]; abmil_tile.h:
// visit_wide).  The unit table and the partial record (max, sum, acc[S1]) are abmil_bags.hip's, unchanged; only this kernel is new.
// A 128-row unit is walked as SUB-TILES of R = 128 / sizeof(T) rows (64 in bf16, 32 in fp32) in row order; R is chosen so that the
// operand image of h1 is S1 * 128 bytes in both dtypes (64 KiB at S1 = 512).  Per sub-tile:
//   phase 1  h1pre = X W1^T on the matrix pipe.  Wave w owns ALL R rows (R / 16 row fragments) and the columns w * S1/4 .. (S1 / 64
//            column fragments): a row operand is read once per wave and K half, a W1 operand by one wave only.  X and the W1 K-slab go
//            through the LDS-DMA ring of abmil_tile.h's geometry (8-row x 128-byte instructions, swizzled chunks), two stages.
//   h1       ReLU(acc + b1) STAYS in the accumulators, unrounded, until the pooling; a copy rounded to T goes to LDS as the gate
//            GEMM's operand image (slab-major, swizzled; it aliases the ring of phase 1).
//   gate     ab = h1 [Wa; Wb]^T on the matrix pipe, in passes of NP = min(2 * S2, 256) packed gate rows (a, a, b, b interleaved as in
//            abmil_bags_kernel): the [Wa; Wb] K-slabs of a pass stream through a second two-stage LDS-DMA ring behind the h1 image.
//            After a pass, tanh * sigmoid * wc of its NP / 2 gate units is added to the row's score in registers, pass after pass;
//            then the 4 lane groups and the 4 waves are added in a fixed order.
//   pooling  sub-tile max, p = exp(A - m) (rows past the bag's end: exactly 0), sum_r p_r h1[r][c] straight from the accumulators:
//            the row fragments in order in the thread, then the 16 row lanes by one fixed shuffle tree.  The sub-tile's
//            (m, sum, acc) is folded into the unit's running record in sub-tile order (online softmax).
// Rounding model: in bf16 mode the bag, W1, Wa and Wb are bf16 and h1 is rounded to bf16 as the gate GEMM's operand only; ab, the
// gate and the pooling are fp32 and the pooling reads unrounded h1 -- the model of the generic per-bag path for these widths.
// A unit's result does not depend on the workgroup that ran it: no atomics, no tickets, nothing kept in the workspace.
#include "abmil_tile.h"
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace {
using namespace abmil_tile;

// abmil_tile.h's wide geometry, and behind its AREA this kernel's carve: A_raw[R], gate sums [4][R]
template <typename T, int S1, int S2> struct WGm : WG<T, S1, S2> {
    using G = WG<T, S1, S2>;
    static constexpr int LDS = G::AREA + (G::R + 4 * G::R) * 4;
    static_assert(LDS <= 160 * 1024, "wide ABMIL: LDS");
};

template <typename T, int S1, int S2>
__global__ __launch_bounds__(256) void abmil_wide_kernel(const T* __restrict__ bag, const BagUnit* __restrict__ units, int max_units,
                                                         int S0, const T* __restrict__ w1, const float* __restrict__ b1,
                                                         const T* __restrict__ wab, const float* __restrict__ bab,
                                                         const float* __restrict__ wc, const float* __restrict__ bc,
                                                         float* __restrict__ A_raw, float* __restrict__ partials, int attention_only) {
    using G = WGm<T, S1, S2>;
    constexpr int EPC = Tr<T>::EPC, R = G::R, NI = G::NI, NJ1 = G::NJ1, NJ2 = G::NJ2, NP = G::NP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* H1s = smem;                         // h1 operand image: aliases the ring of phase 1 (used after it)
    char* Gs = smem + G::H1_BYTES;            // [2][NP][128 B] ring of the [Wa; Wb] slabs
    float* As = (float*)(smem + G::AREA);     // [R] A_raw of the sub-tile
    float* Ps = As + R;                       // [4][R] gate sums of the four column waves

    const Lanes L;
    const int tid = L.tid, lane = L.lane, wave = L.wave, g = L.g, li = L.li, drow = L.drow;
    const int* foff = L.foff;
    const int nk = S0 / G::KB;
    const float bc0 = bc[0];

    for (int unit = blockIdx.x; unit < max_units; unit += gridDim.x) {
        const BagUnit un = units[unit];
        const int64_t m0 = un.m0, mend = un.end;
        if (m0 < 0) break;  // uniform; the surplus entries are the table's tail
        // the unit's running record: every lane of a wave carries (m_run, l_run); o_run is the wave's S1 / 4 columns
        float m_run = -INFINITY, l_run = 0.f;
        f32x4 o_run[NJ1];
#pragma unroll
        for (int j = 0; j < NJ1; ++j) o_run[j] = f32x4{0.f, 0.f, 0.f, 0.f};

        for (int sub = 0; sub < G::NSUB; ++sub) {
            const int64_t ms0 = m0 + sub * R;
            if (ms0 >= mend) break;  // uniform: the first sub-tile of a unit always has a row
            // ---------------- phase 1: h1pre = bag_subtile @ W1^T ----------------
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
                    const int r = (wave * G::NWQ + q) * 8 + drow;
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
            // ---------------- gate: ab = h1 @ [Wa;Wb]^T pass by pass, tanh * sigmoid * wc into the row's score ----------------
            float gate[NI];
#pragma unroll
            for (int i = 0; i < NI; ++i) gate[i] = 0.f;
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
                    const float c0 = wc[j0], c1 = wc[j0 + 1];
#pragma unroll
                    for (int i = 0; i < NI; ++i) {
                        const f32x4 v = acc2[i][j];
                        gate[i] += tanh_f(v[0] + ba0) * sigmoid_f(v[2] + bb0) * c0 + tanh_f(v[1] + ba1) * sigmoid_f(v[3] + bb1) * c1;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                float v = gate[i];
                v += __shfl_xor(v, 16, 64);  // (quad_sum of common.h, written out: the call compiles to different code here)
                v += __shfl_xor(v, 32, 64);
                if (g == 0) Ps[wave * R + i * 16 + li] = v;
            }
            __syncthreads();
            if (tid < R) {  // thread r owns row r of the sub-tile
                const int64_t m = ms0 + tid;
                float a = -INFINITY;
                if (m < mend) {
                    a = ((Ps[tid] + Ps[R + tid]) + Ps[2 * R + tid]) + Ps[3 * R + tid] + bc0;
                    A_raw[m] = a;
                }
                As[tid] = a;
            }
            if (attention_only) continue;  // uniform
            __syncthreads();
            // ---------------- pooling of THIS sub-tile from the accumulators, folded into the unit's record ----------------
            const float m_s = wave_max(As[lane & (R - 1)]);  // finite: the sub-tile has a row; the same bits in every wave
            float p[NI], l_s = 0.f;
#pragma unroll
            for (int i = 0; i < NI; ++i) {
                p[i] = expf(As[i * 16 + li] - m_s);  // rows past the end carry -inf -> exactly 0
                l_s += p[i];
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) l_s += __shfl_xor(l_s, o, 64);
            const float m_new = fmaxf(m_run, m_s);
            const float f_run = expf(m_run - m_new), f_s = expf(m_s - m_new);  // first sub-tile: exp(-inf) = 0 against zeros
            l_run = l_run * f_run + l_s * f_s;
#pragma unroll
            for (int j = 0; j < NJ1; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float o_s = 0.f;
#pragma unroll
                    for (int i = 0; i < NI; ++i) o_s = fmaf(p[i], acc1[i][j][e], o_s);
#pragma unroll
                    for (int o = 1; o < 16; o <<= 1) o_s += __shfl_xor(o_s, o, 64);
                    o_run[j][e] = o_run[j][e] * f_run + o_s * f_s;
                }
            m_run = m_new;
        }
        if (attention_only) continue;  // uniform
        // ---------------- the unit's partial: (max, sum, acc[S1]) ----------------
        float* pw = partials + (int64_t)unit * (2 + S1);
        if (tid == 0) {
            pw[0] = m_run;
            pw[1] = l_run;
        }
        if (li == 0) {
#pragma unroll
            for (int j = 0; j < NJ1; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) pw[2 + wave * (S1 / 4) + j * 16 + 4 * g + e] = o_run[j][e];
        }
    }
}

template <typename T, int S1, int S2>
int launch_wide(const hipt_clam_weights* w, const void* bags, const void* units, int max_units, int attention_only, float* A_raw,
                float* partials, hipStream_t st) {
    return launch_tile_pass<abmil_wide_kernel<T, S1, S2>>(WGm<T, S1, S2>::LDS, "abmil_wide", max_units, st, (const T*)bags,
                                                          (const BagUnit*)units, max_units, w->s0, (const T*)w->w1, w->b1,
                                                          (const T*)w->wab, w->bab, w->wc, w->bc, A_raw, partials, attention_only);
}

}  // namespace

bool hipt_clam_wide_supported(const hipt_clam_weights* w) {
    const int kb = w->dtype == HIPT_F32 ? 32 : 64;
    return w->s0 > 0 && w->s0 % kb == 0 && visit_wide(w->dtype, w->s1, w->s2, [](auto) {});
}

int hipt_clam_wide_tiles_launch(const hipt_clam_weights* w, const void* bags, const void* units, int max_units, int attention_only,
                                int64_t /*a_stride: one branch*/, float* A_raw, float* partials, hipStream_t st) {
    int rc = HIPT_E_UNSUPPORTED;
    const bool found = visit_wide(w->dtype, w->s1, w->s2, [&](auto wd) {
        using W = decltype(wd);
        rc = launch_wide<typename W::T, W::S1, W::S2>(w, bags, units, max_units, attention_only, A_raw, partials, st);
    });
    if (!found) hipt_set_error("clam wide bags: unsupported widths");
    return rc;
}
