// Max-pooling MIL (models/model_mil.py: MIL_fc for two classes, MIL_fc_mc for more) over a run of ragged bags, in one pass over the rows:
//   h1 = ReLU(x W1^T + b1) [N, S1];  logits = h1 W2^T + b2 [N, C];  y_probs = softmax_C(logits);
//   MIL_fc:    the row with the largest y_probs[:, 1];         MIL_fc_mc: the first maximum of y_probs flattened to [N * C];
//   top_logits = logits[row], top_prob = y_probs[row], y_hat = first maximum of top_logits, top_features = h1[row].
// Three launches: abmil_bags.hip's unit table (a unit = 128 rows of ONE bag), the tile pass, one combine workgroup per bag.
// Tile pass, per unit, in SUB-TILES of R = 128 / sizeof(T) rows in row order (abmil_tile.h's wide geometry WG<T, S1, .>):
//   phase 1     abmil_wide.hip's, statement for statement: X and the W1 K-slabs through the two-stage LDS-DMA ring, wave w owns all R
//               rows and the columns w * S1/4 ..
//   h1          ReLU(acc + b1) stays in the accumulators, unrounded
//   classifier  logits[r][c] on the vector ALU straight from the accumulators, class after class: a lane adds its S1/16 columns in
//               ascending order with one fma each, then the 4 lane groups (xor 16, xor 32), then the four waves through
//               Ps[4][R][8] in wave order, then + b2[c]
//   softmax     thread r owns row r: row maximum, exp, the sum in class order, the quotient; y_probs[row][0..C) is stored for rows inside
//               the bag only
//   key         from the values just stored.  MIL_fc: y_probs[r][1].  MIL_fc_mc: the row's largest value, the lowest class among equals
//   record      (key, row of the concatenated matrix, class): the sub-tile's best by `key larger, or equal and row lower`, folded
//               into the unit's record with a strict >, sub-tile after sub-tile: the result of scanning the rows in order with a
//               strict >, so the lowest row wins a tie (torch.topk leaves the order of equal values open: this is the project's rule)
//   Rows past the bag's end: phase 1 re-reads the bag's last row for them; they carry the key -inf and the row INT64_MAX, are never
//   stored and never enter a record.  One record per unit goes to the workspace.
// Combine: thread t folds the records t, t + 256, .. of the bag in order, thread 0 the 256 results in order: the same rule.  The
// workgroup then runs THE SAME sub-tile routine on the selected row alone (a one-row sub-tile: every row slot re-reads it), so logits,
// probabilities and h1 have the bits the tile pass had for that row -- a row's numbers depend on that row and the weights only: one
// accumulator element is one dot product in a fixed K order -- and writes top_idx (bag-local), top_logits, top_prob, y_hat, top_features.
// Rounding model.  fp32: everything is fp32.  bf16: the bag and W1 are bf16, the MFMA accumulates in fp32, and everything from + b1 on
// (h1, W2, b2, logits, softmax, keys) is fp32.  The file is built with -ffp-contract=off and the dot product is written with fmaf:
// every operation is rounded as written, in both kernels.
// No atomics, no tickets, no state in the workspace; a unit's record does not depend on the workgroup that ran it.
#include "abmil_tile.h"
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace {
using namespace abmil_tile;

constexpr int CMAX = 8;  // classes

struct MilRecord {
    float key;
    int cls;
    int64_t row;  // of the concatenated matrix
};
static_assert(sizeof(MilRecord) == 16, "MilRecord");

__device__ __forceinline__ bool mil_better(float ka, int64_t ra, float kb, int64_t rb) { return ka > kb || (ka == kb && ra < rb); }

// the wide geometry without a gate (S2 plays no part in what is used here) and this kernel's carve behind the phase-1 ring
template <typename T, int S1> struct MG : WG<T, S1, 64> {
    using G = WG<T, S1, 64>;
    static constexpr int RING = 2 * G::STAGE;
    static constexpr int LDS = RING + 4 * G::R * CMAX * 4;  // + Ps[4][R][CMAX]
    static_assert(LDS <= 160 * 1024, "MIL: LDS");
    static_assert(G::R <= 64, "MIL: the rows of a sub-tile are owned by the threads of wave 0");
};

struct MilArgs {
    int S0, C, multi;
    const float *b1, *w2, *b2;
};

// One sub-tile: rows [ms0, min(ms0 + R, mend)) of `bag`.  acc1 is left holding h1 (fragment layout of phase 1); thread r < R gets row
// r's logits and probabilities in lg / pr (valid rows only) and the sub-tile's best record comes back in every lane of wave 0.
// y_probs: where to store the probabilities (row m at y_probs + m * C), or null.
template <typename T, int S1>
__device__ __forceinline__ void mil_subtile(char* smem, const Lanes& L, const T* __restrict__ bag, const T* __restrict__ w1,
                                            const MilArgs& a, int64_t ms0, int64_t mend, float* __restrict__ y_probs,
                                            f32x4 (&acc1)[MG<T, S1>::NI][MG<T, S1>::NJ1], float (&lg)[CMAX], float (&pr)[CMAX],
                                            MilRecord& best) {
    using G = MG<T, S1>;
    constexpr int EPC = Tr<T>::EPC, R = G::R, NI = G::NI, NJ1 = G::NJ1;
    float* Ps = (float*)(smem + G::RING);  // [4][R][CMAX] class sums of the four column waves
    const int tid = L.tid, lane = L.lane, wave = L.wave, g = L.g, li = L.li, drow = L.drow;
    const int* foff = L.foff;
    const int nk = a.S0 / G::KB, C = a.C;
    // ---------------- phase 1: h1pre = bag_subtile @ W1^T (abmil_wide.hip) ----------------
    const T* xsrc[G::NXQ];
    int xch[G::NXQ];
#pragma unroll
    for (int q = 0; q < G::NXQ; ++q) {
        const int r = (wave * G::NXQ + q) * 8 + drow;
        int64_t m = ms0 + r;
        m = m < mend ? m : mend - 1;  // rows past the bag's end re-read its last row; masked below
        xsrc[q] = bag + m * a.S0;
        xch[q] = (lane & 7) ^ ((r >> 1) & 7);
    }
    auto stage = [&](int s, int kt) {
        char* sa = smem + s * G::STAGE;
#pragma unroll
        for (int q = 0; q < G::NXQ; ++q) glds16(xsrc[q] + (kt * 8 + xch[q]) * EPC, sa + (wave * G::NXQ + q) * 1024);
#pragma unroll
        for (int q = 0; q < G::NWQ; ++q) {  // S1 rows of W1: S1 / 8 instructions over 4 waves
            const int r = (wave * G::NWQ + q) * 8 + drow;
            glds16(w1 + (int64_t)r * a.S0 + (kt * 8 + ((lane & 7) ^ ((r >> 1) & 7))) * EPC, sa + R * 128 + (wave * G::NWQ + q) * 1024);
        }
    };
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ1; ++j) acc1[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    __syncthreads();  // previous sub-tile's readers of the ring and of Ps are done
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
    // ---------------- h1 = ReLU(acc1 + b1): fp32, in place ----------------
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < NJ1; ++j) {
            const int col = wave * (S1 / 4) + j * 16 + 4 * g;
            f32x4 v = acc1[i][j] + *(const f32x4*)(a.b1 + col);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.f);
            acc1[i][j] = v;
        }
    // ---------------- classifier: class after class, this lane's columns in ascending order, lane groups, then the waves ----------------
#pragma unroll 1
    for (int c = 0; c < C; ++c) {
        f32x4 wv[NJ1];
#pragma unroll
        for (int j = 0; j < NJ1; ++j) wv[j] = *(const f32x4*)(a.w2 + (int64_t)c * S1 + wave * (S1 / 4) + j * 16 + 4 * g);
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < NJ1; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fmaf(acc1[i][j][e], wv[j][e], s);
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (g == 0) Ps[(wave * R + i * 16 + li) * CMAX + c] = s;
        }
    }
    __syncthreads();
    // ---------------- thread r owns row r: logits, softmax, key; wave 0 picks the sub-tile's best ----------------
    if (wave == 0) {  // uniform per wave (R <= 64)
        float key = -INFINITY;
        int kc = 0;
        int64_t row = INT64_MAX;
        const int64_t m = ms0 + lane;
        if (lane < R && m < mend) {
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float* p = Ps + lane * CMAX + c;
                    lg[c] = (((p[0] + p[R * CMAX]) + p[2 * R * CMAX]) + p[3 * R * CMAX]) + a.b2[c];
                    mx = fmaxf(mx, lg[c]);
                }
            float se = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    pr[c] = expf(lg[c] - mx);
                    se += pr[c];
                }
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    pr[c] = pr[c] / se;
                    if (y_probs) y_probs[m * C + c] = pr[c];
                }
            if (a.multi) {
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < C && pr[c] > key) {
                        key = pr[c];
                        kc = c;
                    }
            } else {
                key = pr[1];
                kc = 1;
            }
            if (!(key == key)) key = -INFINITY;  // a NaN never wins
            row = m;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float k2 = __shfl_xor(key, o, 64);
            const int c2 = __shfl_xor(kc, o, 64);
            const int64_t r2 = __shfl_xor(row, o, 64);
            if (mil_better(k2, r2, key, row)) {
                key = k2;
                kc = c2;
                row = r2;
            }
        }
        best.key = key;
        best.cls = kc;
        best.row = row;
    }
    (void)tid;
}

// ---------------- tiles: one record per unit ----------------
template <typename T, int S1>
__global__ __launch_bounds__(256) void mil_tile_kernel(const T* __restrict__ bag, const BagUnit* __restrict__ units, int max_units,
                                                       const T* __restrict__ w1, MilArgs a, float* __restrict__ y_probs,
                                                       MilRecord* __restrict__ records) {
    using G = MG<T, S1>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const Lanes L;
    for (int unit = blockIdx.x; unit < max_units; unit += gridDim.x) {
        const BagUnit un = units[unit];
        const int64_t m0 = un.m0, mend = un.end;
        if (m0 < 0) break;  // uniform; the surplus entries are the table's tail
        MilRecord run{-INFINITY, a.multi ? 0 : 1, m0};  // (a unit whose keys are all NaN names its first row)
        for (int sub = 0; sub < G::NSUB; ++sub) {
            const int64_t ms0 = m0 + sub * G::R;
            if (ms0 >= mend) break;  // uniform: the first sub-tile of a unit always has a row
            f32x4 acc1[G::NI][G::NJ1];
            float lg[CMAX], pr[CMAX];
            MilRecord best{-INFINITY, 0, INT64_MAX};
            mil_subtile<T, S1>(smem, L, bag, w1, a, ms0, mend, y_probs, acc1, lg, pr, best);
            if (best.key > run.key) run = best;  // strict: the earlier sub-tile keeps a tie (wave 0 only holds it)
        }
        if (L.tid == 0) records[unit] = run;
    }
}

// ---------------- combine: one workgroup per bag ----------------
template <typename T, int S1>
__global__ __launch_bounds__(256) void mil_combine_kernel(const T* __restrict__ bag, const int64_t* __restrict__ offsets,
                                                          const int* __restrict__ tile_start, int max_units, const T* __restrict__ w1,
                                                          MilArgs a, const MilRecord* __restrict__ records, int64_t* __restrict__ top_idx,
                                                          float* __restrict__ top_logits, float* __restrict__ top_prob,
                                                          int64_t* __restrict__ y_hat, float* __restrict__ top_features) {
    using G = MG<T, S1>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float fold_key[256];
    __shared__ int fold_cls[256];
    __shared__ int64_t fold_row[256];
    const Lanes L;
    const int b = blockIdx.x, tid = L.tid;
    const int ts = tile_start[b];
    const int te = tile_start[b + 1] < max_units ? tile_start[b + 1] : max_units;
    const int T_ = te - ts;
    if (T_ <= 0) return;  // uniform; only a bag the unit table refused
    float mkey = -INFINITY;
    int mcls = 0;
    int64_t mrow = INT64_MAX;
    for (int t = tid; t < T_; t += 256) {  // the thread's first record, then a strict >: its lowest row among equal keys
        const float k = records[ts + t].key;
        if (t == tid || k > mkey) {
            mkey = k;
            mcls = records[ts + t].cls;
            mrow = records[ts + t].row;
        }
    }
    fold_key[tid] = mkey;
    fold_cls[tid] = mcls;
    fold_row[tid] = mrow;
    __syncthreads();
    if (tid == 0) {
        const int n = T_ < 256 ? T_ : 256;
        int at = 0;
        // thread t's records lie between those of t - 1 and t + 1 only in their first round: compare by (key, row) to keep the lowest row
        for (int t = 1; t < n; ++t)
            if (mil_better(fold_key[t], fold_row[t], mkey, mrow)) {
                mkey = fold_key[t];
                mrow = fold_row[t];
                at = t;
            }
        fold_row[0] = mrow;
        fold_cls[0] = fold_cls[at];
    }
    __syncthreads();
    const int64_t sel_row = fold_row[0];
    const int64_t lo = offsets[b], hi = offsets[b + 1];
    if (sel_row < lo || sel_row >= hi) return;  // uniform; cannot happen with a table made from these offsets
    f32x4 acc1[G::NI][G::NJ1];
    float lg[CMAX], pr[CMAX];
    MilRecord best{-INFINITY, 0, INT64_MAX};
    mil_subtile<T, S1>(smem, L, bag, w1, a, sel_row, sel_row + 1, nullptr, acc1, lg, pr, best);
    const int C = a.C;
    if (tid == 0) {  // row 0 of the one-row sub-tile
        top_idx[b] = sel_row - lo;
        float lm = -INFINITY;
        int arg = 0;
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) {
                top_logits[(int64_t)b * C + c] = lg[c];
                top_prob[(int64_t)b * C + c] = pr[c];
                if (lg[c] > lm) {
                    lm = lg[c];
                    arg = c;
                }
            }
        y_hat[b] = arg;
    }
    if (top_features && L.li == 0) {  // row 0: fragment 0, lane row 0
#pragma unroll
        for (int j = 0; j < G::NJ1; ++j)
            *(f32x4*)(top_features + (int64_t)b * S1 + L.wave * (S1 / 4) + j * 16 + 4 * L.g) = acc1[0][j];
    }
}

template <typename F> bool visit_mil(int dtype, int s1, F&& f) {
#define HIPT_MIL_W(TT, A) if (s1 == A) return f(Width<TT, A, 0>{}), true;
    if (dtype == HIPT_BF16) {
        HIPT_MIL_W(bf16_t, 256) HIPT_MIL_W(bf16_t, 512)
    } else if (dtype == HIPT_F32) {
        HIPT_MIL_W(float, 256) HIPT_MIL_W(float, 512)
    }
#undef HIPT_MIL_W
    return false;
}

MilArgs mil_args(const hipt_mil_weights* w) { return MilArgs{w->s0, w->n_classes, w->multi_class ? 1 : 0, w->b1, w->w2, w->b2}; }

template <typename T, int S1>
int launch_mil(const hipt_mil_weights* w, const void* bags, const int64_t* offsets, int B, const void* units, const int* tile_start,
               int max_units, float* y_probs, void* records, int64_t* top_idx, float* top_logits, float* top_prob, int64_t* y_hat,
               float* top_features, hipStream_t st) {
    constexpr int LDS = MG<T, S1>::LDS;
    if (int rc = launch_tile_pass<mil_tile_kernel<T, S1>>(LDS, "mil_tile", max_units, st, (const T*)bags, (const BagUnit*)units, max_units,
                                                         (const T*)w->w1, mil_args(w), y_probs, (MilRecord*)records))
        return rc;
    static DeviceSetup setup;  // one per instantiation
    if (int rc = setup({(const void*)mil_combine_kernel<T, S1>}, LDS, "mil_combine")) return rc;
    hipLaunchKernelGGL((mil_combine_kernel<T, S1>), dim3(B), dim3(256), LDS, st, (const T*)bags, offsets, tile_start, max_units,
                       (const T*)w->w1, mil_args(w), (const MilRecord*)records, top_idx, top_logits, top_prob, y_hat, top_features);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

}  // namespace

size_t hipt_mil_record_bytes() { return sizeof(MilRecord); }

bool hipt_mil_supported(const hipt_mil_weights* w) {
    const int kb = w->dtype == HIPT_F32 ? 32 : 64;
    return w->s0 > 0 && w->s0 % kb == 0 && w->n_classes >= 2 && w->n_classes <= CMAX && (w->multi_class || w->n_classes == 2) &&
           visit_mil(w->dtype, w->s1, [](auto) {});
}

int hipt_mil_tiles_combine_launch(const hipt_mil_weights* w, const void* bags, const int64_t* offsets, int B, const void* units,
                                  const int* tile_start, int max_units, float* y_probs, void* records, int64_t* top_idx,
                                  float* top_logits, float* top_prob, int64_t* y_hat, float* top_features, hipStream_t st) {
    int rc = HIPT_E_UNSUPPORTED;
    const bool found = visit_mil(w->dtype, w->s1, [&](auto wd) {
        using W = decltype(wd);
        rc = launch_mil<typename W::T, W::S1>(w, bags, offsets, B, units, tile_start, max_units, y_probs, records, top_idx, top_logits,
                                              top_prob, y_hat, top_features, st);
    });
    if (!found) hipt_set_error("mil bags: unsupported width");
    return rc;
}
