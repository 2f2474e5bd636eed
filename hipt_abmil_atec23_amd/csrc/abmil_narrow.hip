// The tile pass of the ragged multi-bag CLAM_SB forward (abmil_bags.hip) for the NARROW gated heads: S1 <= 32, S2 <= 16
// (hipt_smaller [192,16,8], hipt_smallest [192,8,4], [.,32,8], [.,32,16]; abmil_tile.h: visit_narrow).  The unit table, the partial
// record (max, sum, acc[S1]) and the combine are abmil_bags.hip's, unchanged; only this kernel is new.
//   phase 1  h1pre = X W1^T on the matrix pipe.  Wave w owns rows 32w .. 32w+31 of the tile (two 16-row fragments) and ALL
//            max(S1, 16) / 16 column fragments: no column waves, no gate partials between waves.  X and the W1 K-slab go through the
//            LDS-DMA ring of abmil_tile.h's geometry (8-row x 128-byte instructions, swizzled chunks), as in abmil_bags_kernel.
//   gate     a [32 x 32] GEMM at most: not worth the matrix pipe.  h1 = ReLU(h1pre + b1) goes to LDS UNROUNDED (fp32, [128][S1 + 1]);
//            thread (row, half) forms a and b of its half of the S2 gate units against an fp32 image of [Wa; Wb] in LDS, in a
//            fixed order, and the two halves are added in order.
//   pooling  tile_max, p = exp(A - m), sum_r p_r h1[r][c] on the vector ALU against the same fp32 image: thread (c, part) adds rows
//            part, part + NP, ... in order, then the NP parts are added in order.
// Rounding model: in bf16 mode the bag, W1, Wa and Wb are bf16; nothing else is rounded (h1, the gate, the pooling are fp32), which is
// the model of the generic per-bag path for these widths.
// S1 = 8 fills half a 16-row operand fragment: rows 8..15 of the W1 operand are zeros made in registers, b1 / wab / the partial are
// read and written for S1 columns only.  A unit's result does not depend on the workgroup that ran it: no atomics, no tickets.
#include "abmil_tile.h"
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace {
using namespace abmil_tile;

template <typename T, int S1, int S2> struct NG {
    static constexpr int KB = Tr<T>::KB;
    static constexpr int S1P = S1 < 16 ? 16 : S1;    // W1 rows of the operand image (whole 16-row fragments)
    static constexpr int NC = S1P / 16;              // column fragments, all in every wave
    static constexpr int NW = S1 / 8;                // 8-row LDS-DMA instructions of one W1 K-slab (one per wave, waves 0 .. NW-1)
    static constexpr int STAGE = (TM + S1P) * 128;
    static constexpr int HS = S1 + 1;                // row stride of the fp32 h1 image (floats): odd, conflict-free column walks
    static constexpr int NP = 256 / S1;              // row parts of the pooling
    static constexpr int RING = 2 * STAGE;
    static constexpr int H_BYTES = TM * HS * 4;
    static constexpr int W_FLOATS = 2 * S2 * S1 + 2 * S2 + S2;  // [Wa; Wb] | [ba; bb] | wc
    // floats behind the ring and h1: weights | A_raw[128] | gate halves [2][128] | p[128] | pooled parts [NP][S1] = 256 | scalars[16]
    static constexpr int LDS = RING + H_BYTES + (W_FLOATS + TM * 4 + 256 + 16) * 4;
    static_assert(S1 == 8 || S1 == 16 || S1 == 32, "narrow ABMIL: S1 in {8,16,32}");
    static_assert(S2 % 2 == 0 && S2 >= 2 && S2 <= 16, "narrow ABMIL: S2 in {4,8,16}");
    static_assert(NW <= 4 && NP * S1 == 256, "narrow ABMIL: 256 threads");
};

template <typename T, int S1, int S2>
__global__ __launch_bounds__(256, 2) void abmil_narrow_kernel(const T* __restrict__ bag, const BagUnit* __restrict__ units,
                                                              int max_units, int S0, const T* __restrict__ w1,
                                                              const float* __restrict__ b1, const T* __restrict__ wab,
                                                              const float* __restrict__ bab, const float* __restrict__ wc,
                                                              const float* __restrict__ bc, float* __restrict__ A_raw,
                                                              float* __restrict__ partials, int attention_only) {
    using G = NG<T, S1, S2>;
    constexpr int EPC = Tr<T>::EPC, HS = G::HS, NP = G::NP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* Hs = (float*)(smem + G::RING);      // [TM][HS] h1, fp32
    float* Wf = Hs + TM * HS;                  // [2*S2][S1] fp32 image of [Wa; Wb]
    float* Bf = Wf + 2 * S2 * S1;              // [2*S2] ba | bb
    float* Cf = Bf + 2 * S2;                   // [S2] wc
    float* As = Cf + S2;                       // [TM] A_raw of the tile
    float* Ps = As + TM;                       // [2][TM] gate sums of the two unit halves
    float* Pe = Ps + 2 * TM;                   // [TM] softmax numerators
    float* Cs = Pe + TM;                       // [NP][S1] pooled row parts
    float* Sc = Cs + 256;                      // scalars

    const Lanes L;
    const int tid = L.tid, lane = L.lane, wave = L.wave, g = L.g, li = L.li, drow = L.drow;
    const int* foff = L.foff;
    const int nk = S0 / G::KB;

    // the gate's weights, once per workgroup: exactly 2*S2*S1 elements of wab, 2*S2 of bab, S2 of wc
    for (int i = tid; i < 2 * S2 * S1; i += 256) Wf[i] = Tr<T>::to_f(wab[i]);
    if (tid < 2 * S2) Bf[tid] = bab[tid];
    if (tid < S2) Cf[tid] = wc[tid];
    const float bc0 = bc[0];

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
        const int wr = wave * 8 + drow;  // W1 row of this lane's LDS-DMA instruction (waves 0 .. NW-1: wr < S1)
        const T* wsrc = w1 + (int64_t)(wr < S1 ? wr : 0) * S0;
        const int wch = (lane & 7) ^ ((wr >> 1) & 7);
        auto stage = [&](int s, int kt) {
            char* sa = smem + s * G::STAGE;
#pragma unroll
            for (int q = 0; q < 4; ++q) glds16(xsrc[q] + (kt * 8 + xch[q]) * EPC, sa + (wave * 4 + q) * 1024);
            if (wave < G::NW) glds16(wsrc + (kt * 8 + wch) * EPC, sa + TM * 128 + wave * 1024);  // uniform
        };
        f32x4 acc1[2][G::NC];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < G::NC; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        __syncthreads();  // previous unit's readers of the ring, h1 and the exchange buffers are done; the weights are published
        stage(0, 0);
        wait_vm0();
        __syncthreads();
        int cur = 0;
        for (int kt = 0; kt < nk; ++kt) {
            if (kt + 1 < nk) stage(cur ^ 1, kt + 1);
            const char* sa = smem + cur * G::STAGE + wave * 32 * 128;
            const char* sw = smem + cur * G::STAGE + TM * 128;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                u32x4 af[2], wf[G::NC];
#pragma unroll
                for (int i = 0; i < 2; ++i) af[i] = *(const u32x4*)(sa + i * 16 * 128 + foff[ks]);
#pragma unroll
                for (int j = 0; j < G::NC; ++j) {
                    wf[j] = *(const u32x4*)(sw + j * 16 * 128 + foff[ks]);
                    // S1 = 8: rows 8..15 of the operand are not W1 (nothing was staged there): zeros, made here
                    if (S1 < 16 && li >= S1) wf[j] = u32x4{0u, 0u, 0u, 0u};
                }
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < G::NC; ++j) Tr<T>::mma16(acc1[i][j], wf[j], af[i]);
            }
            wait_vm0();
            __syncthreads();
            cur ^= 1;
        }
        // ---------------- h1 = ReLU(acc1 + b1), unrounded, -> LDS [row][col] (columns < S1 only) ----------------
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = wave * 32 + i * 16 + li;
#pragma unroll
            for (int j = 0; j < G::NC; ++j) {
                const int col = j * 16 + 4 * g;
                if (col < S1) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) Hs[row * HS + col + e] = fmaxf(acc1[i][j][e] + b1[col + e], 0.f);
                }
            }
        }
        __syncthreads();
        // ---------------- gate: thread (row, half) over the units half * S2/2 .. ; a, b, tanh * sigmoid * wc in a fixed order ----------------
        {
            const int row = tid & (TM - 1), half = wave >> 1;  // half is wave-uniform
            float h[S1];
#pragma unroll
            for (int c = 0; c < S1; ++c) h[c] = Hs[row * HS + c];
            float gate = 0.f;
#pragma unroll
            for (int jj = 0; jj < S2 / 2; ++jj) {
                const int j = half * (S2 / 2) + jj;
                const float* wa = Wf + j * S1;
                const float* wb = Wf + (S2 + j) * S1;
                float a = 0.f, b = 0.f;
#pragma unroll
                for (int c = 0; c < S1; ++c) {
                    a = fmaf(h[c], wa[c], a);
                    b = fmaf(h[c], wb[c], b);
                }
                gate += tanh_f(a + Bf[j]) * sigmoid_f(b + Bf[S2 + j]) * Cf[j];
            }
            Ps[half * TM + row] = gate;
        }
        __syncthreads();
        float a_mine = -INFINITY;  // threads 0..127 own one row each
        if (tid < TM) {
            const int64_t m = m0 + tid;
            if (m < mend) {
                a_mine = Ps[tid] + Ps[TM + tid] + bc0;
                A_raw[m] = a_mine;
            }
            As[tid] = a_mine;
        }
        if (attention_only) continue;  // uniform
        // ---------------- pooling of THIS tile: softmax numerator against the tile's own maximum, sum_r p_r h1[r][c] ----------------
        const float m_new = tile_max(L, Sc, a_mine);
        if (tid < TM) Pe[tid] = expf(a_mine - m_new);  // invalid rows carry -inf -> p = 0
        __syncthreads();
        {
            const int c = tid % S1, part = tid / S1;
            float o = 0.f;
#pragma unroll 4
            for (int r = part; r < TM; r += NP) o = fmaf(Pe[r], Hs[r * HS + c], o);
            Cs[part * S1 + c] = o;
        }
        float lsum = 0.f;
        if (wave == 0) lsum = wave_sum(Pe[lane] + Pe[lane + 64]);  // one fixed shuffle tree
        __syncthreads();
        // ---------------- the unit's partial: (max, sum, acc[S1]); S1 columns, no more ----------------
        float* pw = partials + (int64_t)unit * (2 + S1);
        if (tid == 0) {
            pw[0] = m_new;
            pw[1] = lsum;
        }
        if (tid < S1) {
            float o = 0.f;
#pragma unroll
            for (int p = 0; p < NP; ++p) o += Cs[p * S1 + tid];
            pw[2 + tid] = o;
        }
    }
}

template <typename T, int S1, int S2>
int launch_narrow(const hipt_clam_weights* w, const void* bags, const void* units, int max_units, int attention_only, float* A_raw,
                  float* partials, hipStream_t st) {
    return launch_tile_pass<abmil_narrow_kernel<T, S1, S2>>(NG<T, S1, S2>::LDS, "abmil_narrow", max_units, st, (const T*)bags,
                                                            (const BagUnit*)units, max_units, w->s0, (const T*)w->w1, w->b1,
                                                            (const T*)w->wab, w->bab, w->wc, w->bc, A_raw, partials, attention_only);
}

}  // namespace

bool hipt_clam_narrow_supported(const hipt_clam_weights* w) {
    const int kb = w->dtype == HIPT_F32 ? 32 : 64;
    return w->s0 > 0 && w->s0 % kb == 0 && visit_narrow(w->dtype, w->s1, w->s2, [](auto) {});
}

int hipt_clam_narrow_tiles_launch(const hipt_clam_weights* w, const void* bags, const void* units, int max_units,
                                  int attention_only, int64_t /*a_stride: one branch*/, float* A_raw, float* partials, hipStream_t st) {
    int rc = HIPT_E_UNSUPPORTED;
    const bool found = visit_narrow(w->dtype, w->s1, w->s2, [&](auto wd) {
        using W = decltype(wd);
        rc = launch_narrow<typename W::T, W::S1, W::S2>(w, bags, units, max_units, attention_only, A_raw, partials, st);
    });
    if (!found) hipt_set_error("clam narrow bags: unsupported widths");
    return rc;
}
