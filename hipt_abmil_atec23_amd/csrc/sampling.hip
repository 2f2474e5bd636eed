// DRAS-MIL attention-guided sampling (eval.py --sampling; utils/eval_utils.py:182-565 summary_sampling, helpers in
// utils/sampling_utils.py:11-187): the two device pieces of one sampling round.
//
//   hipt_knn              brute-force k nearest neighbours of S rows of the point set itself, replacing
//                         NearestNeighbors(algorithm='ball_tree').fit(X) + kneighbors(X[sample_idxs]) (eval_utils.py:285,390-391,413).
//                         Order: ascending (squared distance, index).  spatial: int32 [N,2] coordinates, 64-bit integer
//                         squared distances (exact); textural: fp32 [N,D], the fp32 sum of squared differences.
//   hipt_sampling_update  update_sampling_weights(normalise=False, repeats_allowed=False) of one round (sampling_utils.py:66-187)
//                         on float64 weights, plus their sum in a fixed order.
//
// Selection.  A key is (d, i): d the squared distance as an unsigned 64-bit number (the integer itself, or the bit pattern of
// the non-negative fp32 sum, which orders like the float), i the point index.  A wave keeps a query's best keys as a sorted
// list, one entry per lane; a batch of 64 candidates (one per lane) is first compared with the list's k-th entry, and the few
// that beat it are inserted one at a time (ballot -> position, shift up by one lane).  Stage 1: a workgroup owns one segment
// of the points and up to 128 queries, its lists live in LDS, and it leaves the k best keys per (query, segment) in the
// workspace.  Stage 2: one wave per query merges its segments' lists the same way.  Every key is produced by exactly one thread
// in a fixed operation order and the result of the selection does not depend on the order of arrival, so the output is
// bitwise repeatable.  No inline assembly anywhere in this file.
#include "common.h"
#include "kernels.h"
#include "launch.h"
#include "workspace.h"

namespace {

typedef unsigned long long u64;

constexpr int KNN_TP = 64;        // points per tile = one candidate per lane
constexpr int KNN_TQ = 128;       // queries per workgroup
constexpr int KNN_KS = 32;        // feature slab (floats) of the textural kernel
constexpr int KNN_LDW = KNN_KS + 4;   // padded LDS row: 16 rows of 36 floats start in 16 different 4-bank groups
constexpr int KNN_DTW = KNN_TP + 1;
constexpr int KNN_MAX_K = 64;
constexpr u64 KEY_INF = ~0ull;
constexpr int IDX_INF = 0x7fffffff;

__device__ __forceinline__ bool key_lt(u64 d1, int i1, u64 d2, int i2) { return d1 < d2 || (d1 == d2 && i1 < i2); }

// Insert the lanes' candidates (cd, ci) that beat the list's entry k-1 into the wave's sorted list (ld, li; lane = rank).
// Entries of rank >= k are not maintained (they only ever hold keys that were once inside the best k, or the sentinel).
__device__ __forceinline__ void wave_insert(u64& ld, int& li, u64 cd, int ci, int k, int lane) {
    u64 td = __shfl(ld, k - 1);
    int ti = __shfl(li, k - 1);
    u64 m = __ballot(key_lt(cd, ci, td, ti));
    while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const u64 bd = __shfl(cd, src);
        const int bi = __shfl(ci, src);
        td = __shfl(ld, k - 1);
        ti = __shfl(li, k - 1);
        if (!key_lt(bd, bi, td, ti)) continue;   // the list tightened since the ballot (wave-uniform)
        const int pos = __popcll(__ballot(!key_lt(bd, bi, ld, li)));   // entries <= candidate: a prefix of the sorted list
        const u64 ud = __shfl_up(ld, 1);
        const int ui = __shfl_up(li, 1);
        if (lane > pos) {
            ld = ud;
            li = ui;
        } else if (lane == pos) {
            ld = bd;
            li = bi;
        }
    }
}

// One query's list in LDS (k entries) against one batch of candidates: nothing is loaded unless a candidate beats entry k-1.
__device__ __forceinline__ void lds_list_update(u64* ld_s, int* li_s, u64 cd, int ci, int k, int lane) {
    const u64 td = ld_s[k - 1];
    const int ti = li_s[k - 1];
    if (!__ballot(key_lt(cd, ci, td, ti))) return;
    u64 ld = lane < k ? ld_s[lane] : KEY_INF;
    int li = lane < k ? li_s[lane] : IDX_INF;
    wave_insert(ld, li, cd, ci, k, lane);
    if (lane < k) {
        ld_s[lane] = ld;
        li_s[lane] = li;
    }
}

__device__ __forceinline__ int clamp_row(long long r, int N) { return r < 0 ? 0 : (r >= N ? N - 1 : (int)r); }

struct KnnGeo {
    int N, S, k, G, tiles_per_seg;
};

__device__ __forceinline__ void lists_init(u64* ld_s, int* li_s, int n) {
    for (int e = threadIdx.x; e < n; e += blockDim.x) {
        ld_s[e] = KEY_INF;
        li_s[e] = IDX_INF;
    }
}

__device__ __forceinline__ void lists_store(const u64* ld_s, const int* li_s, const KnnGeo g, int q0, u64* cand_d, int* cand_i) {
    const int nq = min(KNN_TQ, g.S - q0);
    for (int e = threadIdx.x; e < nq * g.k; e += blockDim.x) {
        const int q = e / g.k, j = e - q * g.k;
        const size_t o = ((size_t)(q0 + q) * g.G + blockIdx.x) * g.k + j;
        cand_d[o] = ld_s[e];
        cand_i[o] = li_s[e];
    }
}

// ---- spatial: int32 coordinates, exact 64-bit squared distances ---------------------------------------------------------
__global__ __launch_bounds__(256) void knn_spatial_kernel(const int* __restrict__ C, const int64_t* __restrict__ qidx, KnnGeo g,
                                                          u64* __restrict__ cand_d, int* __restrict__ cand_i) {
    extern __shared__ __align__(16) unsigned char smem[];
    u64* ld_s = (u64*)smem;                           // [TQ][k]
    int* li_s = (int*)(ld_s + KNN_TQ * g.k);          // [TQ][k]
    int* qx_s = li_s + KNN_TQ * g.k;                  // [TQ]
    int* qy_s = qx_s + KNN_TQ;
    const int q0 = blockIdx.y * KNN_TQ, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    lists_init(ld_s, li_s, KNN_TQ * g.k);
    if (threadIdx.x < KNN_TQ) {
        const int q = q0 + threadIdx.x;
        const int r = q < g.S ? clamp_row(qidx[q], g.N) : 0;
        qx_s[threadIdx.x] = C[2 * r];
        qy_s[threadIdx.x] = C[2 * r + 1];
    }
    __syncthreads();
    const int t0 = blockIdx.x * g.tiles_per_seg;
    const int nq = min(KNN_TQ, g.S - q0);
    for (int t = t0; t < t0 + g.tiles_per_seg; ++t) {
        const int p = t * KNN_TP + lane;
        if (t * KNN_TP >= g.N) break;
        const bool live = p < g.N;
        const long long px = live ? C[2 * p] : 0, py = live ? C[2 * p + 1] : 0;
        for (int q = wave; q < nq; q += 4) {   // a wave owns its queries' lists: no barrier in this loop
            const long long dx = px - qx_s[q], dy = py - qy_s[q];
            const u64 cd = live ? (u64)(dx * dx + dy * dy) : KEY_INF;
            lds_list_update(ld_s + q * g.k, li_s + q * g.k, cd, live ? p : IDX_INF, g.k, lane);
        }
    }
    __syncthreads();
    lists_store(ld_s, li_s, g, q0, cand_d, cand_i);
}

// ---- textural: fp32 features, d = sum over the D features of (q - x)^2 in fp32, features in ascending order ---------------
// 256 threads = 16 point groups x 16 query groups; a thread owns points tp + 16a (a < 4) and queries tq + 16b (b < 8).
__global__ __launch_bounds__(256) void knn_textural_kernel(const float* __restrict__ X, const int64_t* __restrict__ qidx, int D, KnnGeo g,
                                                           u64* __restrict__ cand_d, int* __restrict__ cand_i) {
    extern __shared__ __align__(16) unsigned char smem[];
    u64* ld_s = (u64*)smem;                           // [TQ][k]
    int* li_s = (int*)(ld_s + KNN_TQ * g.k);          // [TQ][k]
    int* qrow_s = li_s + KNN_TQ * g.k;                // [TQ] row of X, -1 = no query
    float* xs = (float*)(qrow_s + KNN_TQ);            // [TP][LDW]   | both slabs are dead while
    float* qs = xs + KNN_TP * KNN_LDW;                // [TQ][LDW]   | dt (the distance tile [TQ][DTW]) is alive
    float* dt = xs;
    const int q0 = blockIdx.y * KNN_TQ, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tp = threadIdx.x & 15, tq = threadIdx.x >> 4;
    lists_init(ld_s, li_s, KNN_TQ * g.k);
    if (threadIdx.x < KNN_TQ) {
        const int q = q0 + threadIdx.x;
        qrow_s[threadIdx.x] = q < g.S ? clamp_row(qidx[q], g.N) : -1;
    }
    __syncthreads();
    const int nq = min(KNN_TQ, g.S - q0);
    const int nslab = (D + KNN_KS - 1) / KNN_KS;
    const int t0 = blockIdx.x * g.tiles_per_seg;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int t = t0; t < t0 + g.tiles_per_seg; ++t) {
        const int p0 = t * KNN_TP;
        if (p0 >= g.N) break;
        float acc[8][4];
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a) acc[b][a] = 0.f;
        float4 rx[2], rq[4];
        auto fetch = [&](int slab) __attribute__((always_inline)) {   // global -> registers: slab `slab` of the tile's 64 points and of the 128 query rows
            const int k0 = slab * KNN_KS;
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int id = threadIdx.x + 256 * r, row = id >> 3, c = k0 + (id & 7) * 4;
                rx[r] = (p0 + row < g.N && c < D) ? *(const float4*)(X + (size_t)(p0 + row) * D + c) : zero4;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int id = threadIdx.x + 256 * r, row = id >> 3, c = k0 + (id & 7) * 4;
                const int qr = qrow_s[row];
                rq[r] = (qr >= 0 && c < D) ? *(const float4*)(X + (size_t)qr * D + c) : zero4;
            }
        };
        fetch(0);
        for (int slab = 0; slab < nslab; ++slab) {
#pragma unroll
            for (int r = 0; r < 2; ++r) {
                const int id = threadIdx.x + 256 * r;
                *(float4*)(xs + (id >> 3) * KNN_LDW + (id & 7) * 4) = rx[r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int id = threadIdx.x + 256 * r;
                *(float4*)(qs + (id >> 3) * KNN_LDW + (id & 7) * 4) = rq[r];
            }
            __syncthreads();
            if (slab + 1 < nslab) fetch(slab + 1);   // in flight under the arithmetic below
#pragma unroll 2
            for (int c = 0; c < KNN_KS; c += 4) {
                float4 xv[4];
#pragma unroll
                for (int a = 0; a < 4; ++a) xv[a] = *(const float4*)(xs + (tp + 16 * a) * KNN_LDW + c);
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const float4 qv = *(const float4*)(qs + (tq + 16 * b) * KNN_LDW + c);
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        float d = qv.x - xv[a].x;
                        acc[b][a] = fmaf(d, d, acc[b][a]);
                        d = qv.y - xv[a].y;
                        acc[b][a] = fmaf(d, d, acc[b][a]);
                        d = qv.z - xv[a].z;
                        acc[b][a] = fmaf(d, d, acc[b][a]);
                        d = qv.w - xv[a].w;
                        acc[b][a] = fmaf(d, d, acc[b][a]);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int b = 0; b < 8; ++b)
#pragma unroll
            for (int a = 0; a < 4; ++a) dt[(tq + 16 * b) * KNN_DTW + tp + 16 * a] = acc[b][a];
        __syncthreads();
        const int p = p0 + lane;
        const bool live = p < g.N;
        for (int q = wave; q < nq; q += 4) {
            const u64 cd = live ? (u64)__float_as_uint(dt[q * KNN_DTW + lane]) : KEY_INF;
            lds_list_update(ld_s + q * g.k, li_s + q * g.k, cd, live ? p : IDX_INF, g.k, lane);
        }
        __syncthreads();
    }
    lists_store(ld_s, li_s, g, q0, cand_d, cand_i);
}

// ---- stage 2: one wave per query merges its G segment lists ---------------------------------------------------------------
template <bool SPATIAL>
__global__ __launch_bounds__(64) void knn_merge_kernel(const u64* __restrict__ cand_d, const int* __restrict__ cand_i, KnnGeo g,
                                                       int64_t* __restrict__ ids, void* __restrict__ dist) {
    const int q = blockIdx.x, lane = threadIdx.x;
    u64 ld = KEY_INF;
    int li = IDX_INF;
    const size_t base = (size_t)q * g.G * g.k;
    const int n = g.G * g.k;
    for (int e0 = 0; e0 < n; e0 += 64) {
        const int e = e0 + lane;
        const u64 cd = e < n ? cand_d[base + e] : KEY_INF;
        const int ci = e < n ? cand_i[base + e] : IDX_INF;
        wave_insert(ld, li, cd, ci, g.k, lane);
    }
    if (lane < g.k) {
        ids[(size_t)q * g.k + lane] = li;
        if (SPATIAL) ((double*)dist)[(size_t)q * g.k + lane] = sqrt((double)ld);
        else ((float*)dist)[(size_t)q * g.k + lane] = sqrtf(__uint_as_float((unsigned)ld));
    }
}

size_t lists_bytes(int k) { return (size_t)KNN_TQ * k * 12; }
size_t spatial_lds(int k) { return lists_bytes(k) + KNN_TQ * 8; }
size_t textural_lds(int k) {
    const size_t slabs = (size_t)(KNN_TP + KNN_TQ) * KNN_LDW * 4, tile = (size_t)KNN_TQ * KNN_DTW * 4;
    return lists_bytes(k) + KNN_TQ * 4 + (slabs > tile ? slabs : tile);
}

KnnGeo knn_geo(int N, int S, int k) {
    KnnGeo g;
    g.N = N;
    g.S = S;
    g.k = k;
    const int tiles = (N + KNN_TP - 1) / KNN_TP;
    const int qtiles = (S + KNN_TQ - 1) / KNN_TQ;
    int G = 65536 / (qtiles * KNN_TQ);   // segments: enough workgroups to fill the chip, a bounded candidate buffer
    if (G < 4) G = 4;
    if (G > tiles) G = tiles;
    g.tiles_per_seg = (tiles + G - 1) / G;
    g.G = (tiles + g.tiles_per_seg - 1) / g.tiles_per_seg;
    return g;
}

// ---- sampling-weight update -------------------------------------------------------------------------------------------------
constexpr unsigned SAMPLED = 0xffffffffu;   // above the bit pattern of every finite positive float

struct UpdWs {
    unsigned* bits;   // [N] max mode: bit pattern of the largest contributing score; SAMPLED = in all_sampled (every mode)
    int* first;       // [N] average: flat position i * neighbors + c of the first contribution
    int* cnt;         // [N] average: number of contributions
    double* newd;     // [N] average: the folded value
    double* partial;  // [256]
};

__global__ __launch_bounds__(256) void upd_scatter_kernel(UpdWs ws, int N, const float* __restrict__ scores, int S, const int64_t* __restrict__ ids,
                                                          int k_stride, int neighbors, const int64_t* __restrict__ all_sampled, int T, int mode) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (mode != HIPT_SAMPLING_NEWEST && e < S * neighbors) {
        const int i = e / neighbors, c = e - i * neighbors;
        const int64_t j = ids[(size_t)i * k_stride + c];
        if (j >= 0 && j < N) {
            if (mode == HIPT_SAMPLING_MAX) {
                const float s = scores[i];
                if (s > 0.f) atomicMax(ws.bits + j, __float_as_uint(s));   // integer max of non-negative floats: exact in any order
            } else {
                atomicMin(ws.first + j, e);
                atomicAdd(ws.cnt + j, 1);
            }
        }
    }
    if (e < T) {
        const int64_t j = all_sampled[e];
        if (j >= 0 && j < N) atomicMax(ws.bits + j, SAMPLED);
    }
}

// average: the thread of a target's FIRST contribution folds all of that target's contributions in ascending (i, c):
// new = new > 0 ? (new + s) / 2 : s  (sampling_utils.py:77-83), walking the ids forward until it has met cnt of them.
__global__ __launch_bounds__(256) void upd_fold_kernel(UpdWs ws, int N, const float* __restrict__ scores, int S, const int64_t* __restrict__ ids,
                                                       int k_stride, int neighbors) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= S * neighbors) return;
    int i = e / neighbors, c = e - i * neighbors;
    const int64_t j = ids[(size_t)i * k_stride + c];
    if (j < 0 || j >= N || ws.first[j] != e) return;
    double v = (double)scores[i];
    int left = ws.cnt[j] - 1;
    while (left > 0) {
        if (++c == neighbors) {
            c = 0;
            if (++i == S) break;
        }
        if (ids[(size_t)i * k_stride + c] == j) {
            const double s = (double)scores[i];
            v = v > 0.0 ? (v + s) / 2 : s;
            --left;
        }
    }
    ws.newd[j] = v;
}

__device__ __forceinline__ double block_sum(double v, double* red) {   // fixed tree: the same bits on every run
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void upd_apply_kernel(UpdWs ws, double* __restrict__ w, int N, int per_block, double power, int mode) {
    __shared__ double red[256];
    const int lo = blockIdx.x * per_block, hi = min(N, lo + per_block);
    double acc = 0.0;
    for (int j = lo + threadIdx.x; j < hi; j += 256) {
        const unsigned b = ws.bits[j];
        double x = w[j];
        if (b == SAMPLED) {
            x = 0.0;                                               // repeats_allowed=False (:179-181), after the update
        } else if (mode == HIPT_SAMPLING_MAX) {
            const double p = b ? pow((double)__uint_as_float(b), power) : 0.0;
            if (p > x) x = p;                                      // :165-172
        } else if (mode == HIPT_SAMPLING_AVERAGE) {
            const double v = ws.newd[j];
            if (v > 0.0) {
                const double p = pow(v, power);
                if (p > 0.0) x = p;                                // :84-88, an overwrite
            }
        }
        w[j] = x;
        acc += x;
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) ws.partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void upd_sum_kernel(const double* __restrict__ partial, int n, double* __restrict__ out) {
    __shared__ double red[256];
    const double s = block_sum((int)threadIdx.x < n ? partial[threadIdx.x] : 0.0, red);
    if (threadIdx.x == 0) *out = s;
}

// the candidate lists of the S x G (query, segment) pairs, k entries each: keys | point ids
struct KnnWs { u64* cand_d; int* cand_i; };
void carve_knn(Carver& c, const KnnGeo& g, KnnWs& ws) {
    const size_t n = (size_t)g.S * g.G * g.k;
    ws.cand_d = c.take<u64>(n);
    ws.cand_i = c.take<int>(n);
}

// bits and cnt are taken one after the other on purpose: AVERAGE mode zeroes the two with ONE memset of 2 * al256(4 N) bytes
// starting at bits (hipt_sampling_update), so nothing may ever be carved between them.
void carve_update(Carver& c, int N, UpdWs& ws) {
    ws.bits = c.take<unsigned>(N);
    ws.cnt = c.take<int>(N);
    ws.first = c.take<int>(N);
    ws.newd = c.take<double>(N);
    ws.partial = c.take<double>(256);
}

}  // namespace

extern "C" size_t hipt_knn_workspace_bytes(int N, int S, int k) {
    if (N <= 0 || S <= 0 || k <= 0 || k > KNN_MAX_K || k > N) return 0;
    return dry_run([&](Carver& c) { KnnWs ws; carve_knn(c, knn_geo(N, S, k), ws); });
}

extern "C" int hipt_knn(const void* X, int kind, int N, int D, const int64_t* q_idx, int S, int k, int64_t* ids, void* dist,
                        void* workspace, size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(X && q_idx && ids && dist && workspace, "knn: null argument");
    HIPT_CHECK_ARG(kind == HIPT_KNN_SPATIAL || kind == HIPT_KNN_TEXTURAL, "knn: kind %d is neither spatial nor textural", kind);
    HIPT_CHECK_ARG(N > 0 && N <= (1 << 20) && S > 0 && S <= 4096, "knn: N=%d (1..2^20) / S=%d (1..4096) outside the envelope", N, S);
    HIPT_CHECK_ARG(k > 0 && k <= KNN_MAX_K, "knn: k=%d outside 1..%d", k, KNN_MAX_K);
    if (k > N) {
        hipt_set_error("knn: expected n_neighbors <= n_samples, but n_samples = %d, n_neighbors = %d", N, k);
        return HIPT_E_BADARG;
    }
    if (kind == HIPT_KNN_SPATIAL) HIPT_CHECK_ARG(D == 2 && ((uintptr_t)X % 8) == 0, "knn: spatial points are int32 [N, 2], 8-byte aligned (D=%d)", D);
    else HIPT_CHECK_ARG(D > 0 && D <= 2048 && D % 4 == 0 && ((uintptr_t)X % 16) == 0, "knn: textural D=%d must be a multiple of 4 up to 2048, X 16-byte aligned", D);
    const KnnGeo g = knn_geo(N, S, k);
    Carver c(workspace, ws_bytes);
    KnnWs ws;
    carve_knn(c, g, ws);
    if (int rc = check_workspace(c, "knn")) return rc;
    hipStream_t st = (hipStream_t)stream;
    // (one opt-in for both kernels, the larger of their two needs: the attribute is a ceiling, each launch asks for its own size)
    static DeviceSetup setup;
    const size_t lds_max = spatial_lds(KNN_MAX_K) > textural_lds(KNN_MAX_K) ? spatial_lds(KNN_MAX_K) : textural_lds(KNN_MAX_K);
    if (int rc = setup({(const void*)knn_spatial_kernel, (const void*)knn_textural_kernel}, (int)lds_max, "knn kernels")) return rc;
    const dim3 grid((unsigned)g.G, (unsigned)((S + KNN_TQ - 1) / KNN_TQ));
    if (kind == HIPT_KNN_SPATIAL) {
        hipLaunchKernelGGL(knn_spatial_kernel, grid, dim3(256), spatial_lds(k), st, (const int*)X, q_idx, g, ws.cand_d, ws.cand_i);
        HIPT_CHECK_LAUNCH();
        hipLaunchKernelGGL(knn_merge_kernel<true>, dim3(S), dim3(64), 0, st, (const u64*)ws.cand_d, (const int*)ws.cand_i, g, ids, dist);
    } else {
        hipLaunchKernelGGL(knn_textural_kernel, grid, dim3(256), textural_lds(k), st, (const float*)X, q_idx, D, g, ws.cand_d, ws.cand_i);
        HIPT_CHECK_LAUNCH();
        hipLaunchKernelGGL(knn_merge_kernel<false>, dim3(S), dim3(64), 0, st, (const u64*)ws.cand_d, (const int*)ws.cand_i, g, ids, dist);
    }
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

extern "C" size_t hipt_sampling_update_workspace_bytes(int N) {
    if (N <= 0) return 0;
    return dry_run([&](Carver& c) { UpdWs ws; carve_update(c, N, ws); });
}

extern "C" int hipt_sampling_update(double* weights, int N, const float* scores, int S, const int64_t* ids, int k_stride, int neighbors,
                                    const int64_t* all_sampled, int T, double power, int mode, double* sum_out, void* workspace,
                                    size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(weights && sum_out && workspace && N > 0 && N <= (1 << 24), "sampling_update: null argument / N=%d outside 1..2^24", N);
    HIPT_CHECK_ARG(mode == HIPT_SAMPLING_MAX || mode == HIPT_SAMPLING_NEWEST || mode == HIPT_SAMPLING_AVERAGE, "sampling_update: unknown mode %d", mode);
    HIPT_CHECK_ARG(S >= 0 && neighbors >= 0 && k_stride >= neighbors && (int64_t)S * neighbors <= (1 << 24),
                   "sampling_update: S=%d neighbors=%d k_stride=%d: prefix wider than the rows, or more than 2^24 entries", S, neighbors, k_stride);
    HIPT_CHECK_ARG(S * neighbors == 0 || (scores && ids), "sampling_update: scores / ids missing");
    HIPT_CHECK_ARG(T >= 0 && (T == 0 || all_sampled), "sampling_update: all_sampled missing");
    HIPT_CHECK_ARG(power > 0.0, "sampling_update: power must be positive");
    Carver c(workspace, ws_bytes);
    UpdWs ws;
    carve_update(c, N, ws);
    if (int rc = check_workspace(c, "sampling_update")) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool avg = mode == HIPT_SAMPLING_AVERAGE;
    if (hipMemsetAsync(ws.bits, 0, avg ? 2 * al256((size_t)N * 4) : (size_t)N * 4, st) != hipSuccess ||
        (avg && (hipMemsetAsync(ws.first, 0x7f, (size_t)N * 4, st) != hipSuccess || hipMemsetAsync(ws.newd, 0, (size_t)N * 8, st) != hipSuccess))) {
        hipt_set_error("sampling_update: hipMemsetAsync failed");
        return HIPT_E_LAUNCH;
    }
    const int entries = S * neighbors;
    const int work = entries > T ? entries : T;
    if (work > 0) {
        hipLaunchKernelGGL(upd_scatter_kernel, dim3((work + 255) / 256), dim3(256), 0, st, ws, N, scores, S, ids, k_stride, neighbors, all_sampled, T, mode);
        HIPT_CHECK_LAUNCH();
    }
    if (avg && entries > 0) {
        hipLaunchKernelGGL(upd_fold_kernel, dim3((entries + 255) / 256), dim3(256), 0, st, ws, N, scores, S, ids, k_stride, neighbors);
        HIPT_CHECK_LAUNCH();
    }
    int per_block = (N + 255) / 256;
    per_block = (per_block + 255) / 256 * 256;
    const int blocks = (N + per_block - 1) / per_block;
    hipLaunchKernelGGL(upd_apply_kernel, dim3(blocks), dim3(256), 0, st, ws, weights, N, per_block, power, mode);
    HIPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(upd_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)ws.partial, blocks, sum_out);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
