// CLAM_SB / ABMIL over MANY bags in one call: a concatenated [total_rows, S0] matrix and B+1 row offsets (int64, on the device).
// The workloads are loops over slides (the reference's summary(), utils/eval_utils.py:115-179; validate_clam; the DRAS-MIL rounds) whose
// bags have tens to a few hundred rows: one or two workgroups of abmil.hip's kernel per slide plus a one-workgroup combine, launch
// after launch on a 256-CU chip.  Here the whole set is three plain launches on one stream:
//   units    one workgroup turns the offsets into the work-unit table: unit = one 128-row tile of ONE bag (a tile never spans two
//            bags), units of a bag consecutive and in row order, tile_start[b] = first unit of bag b;
//   tiles    abmil_fused_kernel's tile arithmetic, statement for statement on the geometry and LDS carve of abmil_tile.h (phase 1
//            GEMM by LDS-DMA ring, +b1, ReLU, gate GEMM, tanh * sigmoid * wc, the tile's softmax numerator and p^T h1 on the matrix
//            pipe), but WITHOUT running state from tile to tile: every unit writes A_raw of its rows and its own partial
//            (max, sum, acc[S1]) to partials[unit].  One difference, bf16 only: the pooling takes fp32 weights and an fp32 copy of h1
//            (the fp32 instantiation's code) instead of the bf16 image, which costs 4 * 128 * S1 bytes of LDS and brings M to the
//            accuracy of the per-bag streaming kernel;
//   combine  one workgroup per bag merges partials[tile_start[b] .. tile_start[b+1]) in a reduction whose shape depends on the
//            bag's tile count alone, then the bag classifier, softmax and argmax as abmil_combine_kernel.
// Hence a bag's outputs are bit for bit independent of the other bags of the call, of its position, of B and of the grid size
// (workgroups stride over the units; a unit's result does not depend on which workgroup ran it).  There are no atomics, no
// tickets, no waiting on another workgroup and no host synchronisation: the workspace carries no state between calls.
#include "abmil_tile.h"
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace {
using namespace abmil_tile;

// ---------------- units: offsets -> tile_start[B+1], units[max_units] ----------------
// One 1024-thread workgroup; thread t owns a contiguous run of ceil(B/1024) bags: count its tiles, exclusive scan over the threads
// (shuffles inside a wave, 16 wave totals through LDS), then write its bags' entries.  A bag whose offsets are not inside
// [0, total_rows] or not increasing gets no unit (the caller checks the offsets; this only keeps every later access in bounds).
__global__ __launch_bounds__(1024) void bags_units_kernel(const int64_t* __restrict__ offsets, int B, int64_t total_rows,
                                                          int max_units, int* __restrict__ tile_start,
                                                          BagUnit* __restrict__ units) {
    __shared__ int wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (B + 1023) / 1024;
    const int b0 = tid * per < B ? tid * per : B, b1 = b0 + per < B ? b0 + per : B;
    auto tiles_of = [&](int b) -> int {
        const int64_t lo = offsets[b], hi = offsets[b + 1];
        if (lo < 0 || hi <= lo || hi > total_rows) return 0;
        const int64_t t = (hi - lo + TM - 1) / TM;
        return t < (int64_t)max_units ? (int)t : max_units;
    };
    int cnt = 0;
    for (int b = b0; b < b1; ++b) {
        const int t = tiles_of(b);
        cnt = cnt + t < max_units ? cnt + t : max_units;  // saturate: no overflow whatever the offsets hold
    }
    int v = cnt;  // wave_incl_scan's ladder, but SATURATING at max_units (no overflow whatever the offsets hold): written out
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int n = __shfl_up(v, o, 64);
        if (lane >= o) v = v + n < max_units ? v + n : max_units;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (i < wave) base = base + wsum[i] < max_units ? base + wsum[i] : max_units;
        total = total + wsum[i] < max_units ? total + wsum[i] : max_units;
    }
    int ts = base + (v - cnt);
    ts = ts < max_units ? ts : max_units;
    for (int b = b0; b < b1; ++b) {
        const int t = tiles_of(b);
        tile_start[b] = ts;
        const int64_t lo = offsets[b], hi = offsets[b + 1];
        for (int i = 0; i < t && ts + i < max_units; ++i) units[ts + i] = BagUnit{lo + (int64_t)i * TM, hi};
        ts = ts + t < max_units ? ts + t : max_units;
    }
    if (tid == 0) tile_start[B] = total;
    for (int u = total + tid; u < max_units; u += 1024) units[u] = BagUnit{-1, -1};
}

// ---------------- tiles: abmil_fused_kernel's tile, one (bag, tile) unit at a time ----------------
template <typename T, int S1, int S2>
__global__ __launch_bounds__(256, 2) void abmil_bags_kernel(const T* __restrict__ bag, const BagUnit* __restrict__ units,
                                                            int max_units, int S0, const T* __restrict__ w1,
                                                            const float* __restrict__ b1, const T* __restrict__ wab,
                                                            const float* __restrict__ bab, const float* __restrict__ wc,
                                                            const float* __restrict__ bc, float* __restrict__ A_raw,
                                                            float* __restrict__ partials, int attention_only) {
    using G = AG<T, S1, S2>;
    constexpr int EPC = Tr<T>::EPC;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* H1s = G::h1s(smem);                     // aliases the stage ring (used after phase 1)
    char* Wabs = G::wabs(smem);
    float *As = G::as(smem), *Ps = G::ps(smem), *Sc = G::sc(smem);
    // bf16 only: h1 once more, UNROUNDED (fp32, the fp32 instantiation's image layout), behind everything else.  The gate GEMM reads the
    // bf16 image as in abmil_fused_kernel; the pooling reads this one, so that M carries no bf16 rounding of h1 or of the softmax weights
    // (the per-bag streaming kernel pools fp32 h1 too; a one-row bag's M is h1 itself).
    constexpr bool POOL32 = sizeof(T) == 2;
    char* Hp = POOL32 ? G::h32(smem) : H1s;

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
            for (int q = 0; q < S1 / 32; ++q) {  // S1 rows of W1: S1/8 instructions over 4 waves
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
        // packed row r: quad = r>>2, pos = r&3 -> source row (pos>>1)*S2 + quad*2 + (pos&1)
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
        // ---------------- phase 2: ab = h1 @ [Wa;Wb]^T, gate, reduce ----------------
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
            float gate[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < G::NJ2; ++j) {
                const int r0 = wn * S2 + j * 16 + 4 * g;  // packed row of element 0
                const int j0 = (r0 >> 2) * 2;             // gate unit of elements 0 (a) and 2 (b); j0+1 for 1 and 3
                const float ba0 = bab[j0], ba1 = bab[j0 + 1], bb0 = bab[S2 + j0], bb1 = bab[S2 + j0 + 1];
                const float c0 = wc[j0], c1 = wc[j0 + 1];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 v = acc2[i][j];
                    gate[i] += tanh_f(v[0] + ba0) * sigmoid_f(v[2] + bb0) * c0 +
                               tanh_f(v[1] + ba1) * sigmoid_f(v[3] + bb1) * c1;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float v = quad_sum(gate[i]);
                if (g == 0) Ps[wn * TM + wm * 64 + i * 16 + li] = v;
            }
        }
        __syncthreads();
        float a_mine = -INFINITY;  // threads 0..127 own one row each
        if (tid < TM) {
            const int64_t m = m0 + tid;
            if (m < mend) {
                a_mine = Ps[tid] + Ps[TM + tid] + bc[0];
                A_raw[m] = a_mine;
            }
            As[tid] = a_mine;
        }
        if (attention_only) continue;  // uniform
        // ---------------- pooling of THIS tile: softmax numerator against the tile's own maximum + p^T h1 ----------------
        const float m_new = tile_max(L, Sc, a_mine);
        // p for this lane's K slots (rows of the tile); invalid rows carry -inf -> p = 0
        float lsum = 0.f;
        f32x4 o[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
        // fp32 weights against fp32 h1 in both instantiations (four 16x16x4 MFMAs per fragment)
#pragma unroll
        for (int mb = 0; mb < TM; mb += 16) {
            u32x4 pf;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = expf(As[mb + 4 * g + e] - m_new);
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
        // lsum: lane (g, li) summed the rows of its K slots; the 4 groups partition the tile's rows and
        // all 16 li lanes of a group hold the same value -> total = sum over g = 2 shuffles
        lsum = quad_sum(lsum);
        // ---------------- the unit's partial: (max, sum, acc[S1]) ----------------
        store_partial<S1>(L, partials + (int64_t)unit * (2 + S1), m_new, lsum, o);
    }
}

// ---------------- combine: one workgroup per bag ----------------
// Merges the bag's T partials (ascending units = ascending tiles) and applies the bag classifier, softmax and argmax
// (model_clam.py:180-183) as abmil_combine_kernel does.  Thread (c, part) sums column c over tiles part, part + 8, ...; the 8 parts are
// then added in order: the shape of every sum is a function of T alone.  T is not capped (a 100 000-row bag has 782 tiles): the
// rescale factors exp(m_t - m*) are recomputed where they are used instead of being kept in LDS.
__global__ __launch_bounds__(1024) void abmil_bags_combine_kernel(const float* __restrict__ partials,
                                                                  const int* __restrict__ tile_start, int max_units, int S1,
                                                                  const float* __restrict__ wcls,
                                                                  const float* __restrict__ bcls, int C, float* __restrict__ M,
                                                                  float* __restrict__ logits, float* __restrict__ Y_prob,
                                                                  int64_t* __restrict__ Y_hat) {
    extern __shared__ float sm[];  // [8*S1] column partial sums | [S1] M | [C] logits
    float* Cs = sm;
    float* Ms = Cs + 8 * S1;
    float* Ls = Ms + S1;
    __shared__ float red[16];
    const int b = blockIdx.x;
    const int ts = tile_start[b];
    const int te = tile_start[b + 1] < max_units ? tile_start[b + 1] : max_units;
    const int T = te - ts;
    if (T <= 0) return;  // uniform; only a bag the unit table refused (offsets the caller did not check)
    const int tid = threadIdx.x, stride = 2 + S1, wv = tid >> 6, ln = tid & 63;
    const float* P = partials + (int64_t)ts * stride;
    M += (int64_t)b * S1;
    logits += (int64_t)b * C;
    Y_prob += (int64_t)b * C;
    float mx = -INFINITY;
    for (int t = tid; t < T; t += 1024) mx = fmaxf(mx, P[(int64_t)t * stride]);
    mx = wave_max(mx);
    if (ln == 0) red[wv] = mx;
    __syncthreads();
    mx = red[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mx = fmaxf(mx, red[i]);
    __syncthreads();
    float ls = 0.f;
    for (int t = tid; t < T; t += 1024) ls += P[(int64_t)t * stride + 1] * expf(P[(int64_t)t * stride] - mx);
    ls = wave_sum(ls);
    if (ln == 0) red[wv] = ls;
    __syncthreads();
    float L = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) L += red[i];
    // column sums: 128 columns x 8 parts = 1024 threads at a time (S1 <= 128: one round; the wide heads of abmil_wide.hip: 2 or 4)
    for (int c = tid & 127; c < S1; c += 128) {
        const int part = tid >> 7;
        float a = 0.f;
        for (int t = part; t < T; t += 8) a += P[(int64_t)t * stride + 2 + c] * expf(P[(int64_t)t * stride] - mx);
        Cs[part * S1 + c] = a;
    }
    __syncthreads();
    for (int c = tid; c < S1; c += 1024) {
        float a = 0.f;
#pragma unroll
        for (int part = 0; part < 8; ++part) a += Cs[part * S1 + c];
        a /= L;
        Ms[c] = a;
        M[c] = a;
    }
    __syncthreads();
    bag_head(Ms, Ls, S1, wcls, bcls, C, logits, Y_prob, Y_hat + b);
}

// ---------------- tiles, K attention branches (CLAM_MB): a second kernel next to abmil_bags_kernel ----------------
// W1 and [Wa; Wb] are shared by the branches, so phase 1, the ReLU image and the gate GEMM are abmil_bags_kernel's, statement for
// statement, once per tile.  The gate epilogue computes tanh * sigmoid once per gate unit and multiplies it by wc[k][j] for each branch
// (KMAX register rows; rows k >= K carry a zero weight and are never stored).  A_raw is [K, a_stride] (a_stride = total_rows):
// branch k of row m at A_raw[k * a_stride + m].  The pooling then runs branch after branch on the matrix pipe against the fp32 h1
// (the fp32 instantiation's own image, the extra fp32 image in bf16: abmil_bags_kernel's POOL32 path), and the unit writes K partials
// (max, sum, acc[S1]) at partials[(unit * K + k) * (2 + S1)].  The single-branch kernel above is left as it is: its instantiations
// keep their code.
template <typename T, int S1, int S2>
__global__ __launch_bounds__(256, 2) void abmil_bags_mb_kernel(const T* __restrict__ bag, const BagUnit* __restrict__ units,
                                                               int max_units, int S0, const T* __restrict__ w1,
                                                               const float* __restrict__ b1, const T* __restrict__ wab,
                                                               const float* __restrict__ bab, const float* __restrict__ wc,
                                                               const float* __restrict__ bc, int K, int64_t a_stride,
                                                               float* __restrict__ A_raw, float* __restrict__ partials,
                                                               int attention_only) {
    using G = AG<T, S1, S2>;
    constexpr int EPC = Tr<T>::EPC, KMAX = G::KMAX;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* H1s = G::h1s(smem);
    char* Wabs = G::wabs(smem);
    float *As = G::as_mb(smem), *Ps = G::ps_mb(smem), *Sc = G::sc_mb(smem);
    constexpr bool POOL32 = sizeof(T) == 2;
    char* Hp = POOL32 ? G::h32_mb(smem) : H1s;

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
            float gate[KMAX][4];
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) gate[k][i] = 0.f;
#pragma unroll
            for (int j = 0; j < G::NJ2; ++j) {
                const int r0 = wn * S2 + j * 16 + 4 * g;  // packed row of element 0
                const int j0 = (r0 >> 2) * 2;             // gate unit of elements 0 (a) and 2 (b); j0+1 for 1 and 3
                const float ba0 = bab[j0], ba1 = bab[j0 + 1], bb0 = bab[S2 + j0], bb1 = bab[S2 + j0 + 1];
                float c0[KMAX], c1[KMAX];
#pragma unroll
                for (int k = 0; k < KMAX; ++k) {
                    c0[k] = k < K ? wc[k * S2 + j0] : 0.f;
                    c1[k] = k < K ? wc[k * S2 + j0 + 1] : 0.f;
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const f32x4 v = acc2[i][j];
                    const float t0 = tanh_f(v[0] + ba0) * sigmoid_f(v[2] + bb0);
                    const float t1 = tanh_f(v[1] + ba1) * sigmoid_f(v[3] + bb1);
#pragma unroll
                    for (int k = 0; k < KMAX; ++k) gate[k][i] += t0 * c0[k] + t1 * c1[k];
                }
            }
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float v = quad_sum(gate[k][i]);
                    if (g == 0) Ps[(k * 2 + wn) * TM + wm * 64 + i * 16 + li] = v;
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

// ---------------- combine, K branches: one workgroup per bag ----------------
// Branch after branch the reduction of abmil_bags_combine_kernel (parts t, t + 8, ..., then the 8 parts in order) on the branch's
// partials, M[b, k, :], logits[b, k] = wcls[k] . M[b, k] + bcls[k] (model_clam.py:248-250; the dot product as bag_head forms it for a
// one-class classifier), then softmax and first-maximum argmax over the K logits.
__global__ __launch_bounds__(1024) void abmil_bags_mb_combine_kernel(const float* __restrict__ partials,
                                                                     const int* __restrict__ tile_start, int max_units, int S1,
                                                                     const float* __restrict__ wcls,
                                                                     const float* __restrict__ bcls, int K, float* __restrict__ M,
                                                                     float* __restrict__ logits, float* __restrict__ Y_prob,
                                                                     int64_t* __restrict__ Y_hat) {
    extern __shared__ float sm[];  // [8*S1] column partial sums | [S1] M of the branch | [K] logits
    float* Cs = sm;
    float* Ms = Cs + 8 * S1;
    float* Ls = Ms + S1;
    __shared__ float red[16];
    const int b = blockIdx.x;
    const int ts = tile_start[b];
    const int te = tile_start[b + 1] < max_units ? tile_start[b + 1] : max_units;
    const int T = te - ts;
    if (T <= 0) return;  // uniform; only a bag the unit table refused
    const int tid = threadIdx.x, stride = 2 + S1, wv = tid >> 6, ln = tid & 63;
    const int64_t tstride = (int64_t)K * stride;  // from a tile's partial of branch k to the next tile's
    for (int k = 0; k < K; ++k) {
        const float* P = partials + ((int64_t)ts * K + k) * stride;
        float* Mk = M + ((int64_t)b * K + k) * S1;
        float mx = -INFINITY;
        for (int t = tid; t < T; t += 1024) mx = fmaxf(mx, P[t * tstride]);
        mx = wave_max(mx);
        if (ln == 0) red[wv] = mx;
        __syncthreads();
        mx = red[0];
#pragma unroll
        for (int i = 1; i < 16; ++i) mx = fmaxf(mx, red[i]);
        __syncthreads();
        float ls = 0.f;
        for (int t = tid; t < T; t += 1024) ls += P[t * tstride + 1] * expf(P[t * tstride] - mx);
        ls = wave_sum(ls);
        if (ln == 0) red[wv] = ls;
        __syncthreads();
        float L = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) L += red[i];
        // 128 columns x 8 parts = 1024 threads at a time (S1 <= 128: one round; the wide heads of abmil_wide_mb.hip: 2 or 4)
        for (int c = tid & 127; c < S1; c += 128) {
            const int part = tid >> 7;
            float a = 0.f;
            for (int t = part; t < T; t += 8) a += P[t * tstride + 2 + c] * expf(P[t * tstride] - mx);
            Cs[part * S1 + c] = a;
        }
        __syncthreads();
        for (int c = tid; c < S1; c += 1024) {
            float a = 0.f;
#pragma unroll
            for (int part = 0; part < 8; ++part) a += Cs[part * S1 + c];
            a /= L;
            Ms[c] = a;
            Mk[c] = a;
        }
        __syncthreads();
        if (wv == 0) {
            float a = 0.f;
            for (int c = ln; c < S1; c += 64) a += Ms[c] * wcls[(int64_t)k * S1 + c];
            a = wave_sum(a);
            if (ln == 0) Ls[k] = a + bcls[k];
        }
        __syncthreads();  // red, Cs and Ms are free for the next branch; Ls[k] is published
    }
    if (tid == 0) {
        float lm = -INFINITY;
        int arg = 0;
        for (int k = 0; k < K; ++k)
            if (Ls[k] > lm) {
                lm = Ls[k];
                arg = k;
            }
        float se = 0.f;
        for (int k = 0; k < K; ++k) se += expf(Ls[k] - lm);
        for (int k = 0; k < K; ++k) {
            logits[(int64_t)b * K + k] = Ls[k];
            Y_prob[(int64_t)b * K + k] = expf(Ls[k] - lm) / se;
        }
        Y_hat[b] = arg;
    }
}

template <typename T, int S1, int S2>
int launch_bags(const hipt_clam_weights* w, const void* bags, const void* units, int max_units, int attention_only, float* A_raw,
                float* partials, hipStream_t st) {
    using G = AG<T, S1, S2>;
    constexpr int LDS = G::LDS + (sizeof(T) == 2 ? TM * S1 * 4 : 0);  // bf16: + the fp32 h1 image of the pooling (<= 130 KiB of the CU's 160)
    return launch_tile_pass<abmil_bags_kernel<T, S1, S2>>(LDS, "abmil_bags", max_units, st, (const T*)bags, (const BagUnit*)units,
                                                          max_units, w->s0, (const T*)w->w1, w->b1, (const T*)w->wab, w->bab, w->wc,
                                                          w->bc, A_raw, partials, attention_only);
}

template <typename T, int S1, int S2>
int launch_bags_mb(const hipt_clam_weights* w, const void* bags, const void* units, int max_units, int attention_only,
                   int64_t a_stride, float* A_raw, float* partials, hipStream_t st) {
    using G = AG<T, S1, S2>;
    constexpr int LDS = G::LDS_MB + (sizeof(T) == 2 ? TM * S1 * 4 : 0);  // bf16: + the fp32 h1 image of the pooling (<= 135 KiB of the CU's 160)
    return launch_tile_pass<abmil_bags_mb_kernel<T, S1, S2>>(LDS, "abmil_bags_mb", max_units, st, (const T*)bags, (const BagUnit*)units,
                                                             max_units, w->s0, (const T*)w->w1, w->b1, (const T*)w->wab, w->bab, w->wc,
                                                             w->bc, w->n_att, a_stride, A_raw, partials, attention_only);
}

}  // namespace

int hipt_clam_bags_mb_tiles_launch(const hipt_clam_weights* w, const void* bags, const void* units, int max_units,
                                   int attention_only, int64_t a_stride, float* A_raw, float* partials, hipStream_t st) {
    if (w->n_att < 2 || w->n_att > AG<float, 128, 64>::KMAX) {
        hipt_set_error("clam mb bags: %d branches (2..%d)", w->n_att, AG<float, 128, 64>::KMAX);
        return HIPT_E_UNSUPPORTED;
    }
    int rc = HIPT_E_UNSUPPORTED;
    const bool found = visit_width(w->dtype, w->s1, w->s2, [&](auto wd) {
        using W = decltype(wd);
        rc = launch_bags_mb<typename W::T, W::S1, W::S2>(w, bags, units, max_units, attention_only, a_stride, A_raw, partials, st);
    });
    if (!found) hipt_set_error("clam mb bags: unsupported widths");
    return rc;
}

int hipt_clam_bags_mb_combine_launch(const float* partials, const int* tile_start, int max_units, int B,
                                     const hipt_clam_weights* w, float* M, float* logits, float* Y_prob, int64_t* Y_hat,
                                     hipStream_t st) {
    const size_t lds = (9 * (size_t)w->s1 + w->n_att) * sizeof(float);
    hipLaunchKernelGGL(abmil_bags_mb_combine_kernel, dim3(B), dim3(1024), lds, st, partials, tile_start, max_units, w->s1,
                       w->wcls, w->bcls, w->n_att, M, logits, Y_prob, Y_hat);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

size_t hipt_clam_bags_unit_bytes() { return sizeof(BagUnit); }

int hipt_clam_bags_units_launch(const int64_t* offsets, int B, int64_t total_rows, int max_units, int* tile_start, void* units,
                                hipStream_t st) {
    hipLaunchKernelGGL(bags_units_kernel, dim3(1), dim3(1024), 0, st, offsets, B, total_rows, max_units, tile_start,
                       (BagUnit*)units);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

int hipt_clam_bags_tiles_launch(const hipt_clam_weights* w, const void* bags, const void* units, int max_units,
                                int attention_only, int64_t /*a_stride: one branch*/, float* A_raw, float* partials, hipStream_t st) {
    int rc = HIPT_E_UNSUPPORTED;
    const bool found = visit_width(w->dtype, w->s1, w->s2, [&](auto wd) {
        using W = decltype(wd);
        rc = launch_bags<typename W::T, W::S1, W::S2>(w, bags, units, max_units, attention_only, A_raw, partials, st);
    });
    if (!found) hipt_set_error("clam bags: unsupported widths");
    return rc;
}

int hipt_clam_bags_combine_launch(const float* partials, const int* tile_start, int max_units, int B,
                                  const hipt_clam_weights* w, float* M, float* logits, float* Y_prob, int64_t* Y_hat,
                                  hipStream_t st) {
    const size_t lds = (9 * (size_t)w->s1 + w->n_classes) * sizeof(float);
    hipLaunchKernelGGL(abmil_bags_combine_kernel, dim3(B), dim3(1024), lds, st, partials, tile_start, max_units, w->s1, w->wcls,
                       w->bcls, w->n_classes, M, logits, Y_prob, Y_hat);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
