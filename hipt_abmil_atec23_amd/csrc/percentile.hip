// Heat-map score ranks (wsi_core/wsi_utils.py:124-127 to_percentiles; vis_utils/heatmap_utils.py:22-24 score2percentile):
// for every query q[i] two integer counts over the reference, less = #{ref < q} and leq = #{ref <= q}, and from them the percentile
// in float64 with the reference's own order of operations.
//
// Brute force, as the kNN of sampling.hip: no sort, no atomic, no ticket, no workspace.  One wave is one workgroup and owns
// PCT_QW = 64 * PCT_Q queries, PCT_Q per lane in registers (query k of lane l is number l + 64 k of the workgroup: coalesced).
// The reference streams past them in tiles of PCT_T values through LDS; every lane reads the SAME address (a broadcast, two values
// per 128-bit read), so a pair costs two float64 compares and two add-with-carry and nothing else.  The next tile's values travel
// from global memory into registers while the current one is being counted.  The tail of the last tile is padded with NaN, which
// compares false both ways: the inner loop has no bound check.  A query's counts are sums over the whole reference, so they depend
// on nothing but q[i] and ref.
// -ffp-contract=off (Makefile): the float64 product, quotient and product of the percentile are rounded one by one.
#include "common.h"

namespace {

constexpr int PCT_THREADS = 64;                    // one wave
constexpr int PCT_Q = HIPT_PCT_QUERIES_PER_WG / PCT_THREADS;   // queries per lane
constexpr int PCT_QW = HIPT_PCT_QUERIES_PER_WG;    // queries per workgroup
constexpr int PCT_T = HIPT_PCT_REF_TILE;           // reference values per LDS tile
constexpr int PCT_L = PCT_T / PCT_THREADS;         // tile values each lane carries from global memory to LDS
constexpr int PCT_UNROLL = 8;                      // reference values per trip of the counting loop
static_assert(PCT_Q * PCT_THREADS == PCT_QW && PCT_L * PCT_THREADS == PCT_T && PCT_T % PCT_UNROLL == 0, "whole lanes, whole trips");

__global__ __launch_bounds__(PCT_THREADS) void pct_counts_kernel(const double* __restrict__ q, long long nq,
                                                                 const double* __restrict__ ref, long long nref, int mode, double scale,
                                                                 int* __restrict__ less, int* __restrict__ leq, double* __restrict__ pct) {
    __shared__ __attribute__((aligned(16))) double tile[PCT_T];
    const int lane = threadIdx.x;
    const long long q0 = (long long)blockIdx.x * PCT_QW + lane;

    double qv[PCT_Q];
    int lt[PCT_Q], le[PCT_Q];
#pragma unroll
    for (int k = 0; k < PCT_Q; ++k) {
        const long long i = q0 + (long long)k * PCT_THREADS;
        qv[k] = i < nq ? q[i] : 0.0;
        lt[k] = 0;
        le[k] = 0;
    }

    const double pad = __builtin_nan("");
    double nxt[PCT_L];
#pragma unroll
    for (int s = 0; s < PCT_L; ++s) {
        const long long j = (long long)s * PCT_THREADS + lane;
        nxt[s] = j < nref ? ref[j] : pad;
    }
    for (long long base = 0; base < nref; base += PCT_T) {
#pragma unroll
        for (int s = 0; s < PCT_L; ++s) tile[s * PCT_THREADS + lane] = nxt[s];
        __syncthreads();
        const long long nb = base + PCT_T;
        if (nb < nref) {   // (uniform) the loads of the next tile are in flight under the counting below
#pragma unroll
            for (int s = 0; s < PCT_L; ++s) {
                const long long j = nb + (long long)s * PCT_THREADS + lane;
                nxt[s] = j < nref ? ref[j] : pad;
            }
        }
        const long long left = nref - base;
        const int m = left < PCT_T ? (int)((left + PCT_UNROLL - 1) / PCT_UNROLL) * PCT_UNROLL : PCT_T;   // (the rest of the trip is NaN)
        for (int j = 0; j < m; j += PCT_UNROLL) {
#pragma unroll
            for (int u = 0; u < PCT_UNROLL; ++u) {
                const double r = tile[j + u];   // the same address in every lane: a broadcast
#pragma unroll
                for (int k = 0; k < PCT_Q; ++k) {
                    lt[k] += r < qv[k];
                    le[k] += r <= qv[k];
                }
            }
        }
        __syncthreads();
    }

    const double n = (double)nref;
#pragma unroll
    for (int k = 0; k < PCT_Q; ++k) {
        const long long i = q0 + (long long)k * PCT_THREADS;
        if (i >= nq) continue;
        if (less) less[i] = lt[k];
        if (leq) leq[i] = le[k];
        if (pct) {
            const long long both = (long long)lt[k] + le[k];
            double p;
            if (mode == HIPT_PCT_RANKDATA) {
                const double rank = 0.5 * (double)(both + 1);   // the mean of the 1-based positions less + 1 .. leq
                p = rank / n;
                p = p * 100.0;
            } else {
                p = (double)(both + (lt[k] < le[k] ? 1 : 0)) * scale;   // scale = 50.0 / nref, one division on the host
            }
            pct[i] = p;
        }
    }
}

}  // namespace

extern "C" int hipt_score_counts(const double* q, int64_t nq, const double* ref, int64_t nref, int mode, int32_t* less, int32_t* leq,
                                 double* pct, void* stream) {
    HIPT_CHECK_ARG(nq >= 0 && nref >= 0, "score_counts: nq=%lld, nref=%lld", (long long)nq, (long long)nref);
    HIPT_CHECK_ARG(mode == HIPT_PCT_RANKDATA || mode == HIPT_PCT_OF_SCORE, "score_counts: mode %d is neither HIPT_PCT_RANKDATA nor HIPT_PCT_OF_SCORE",
                   mode);
    if (nq == 0 || nref == 0) return HIPT_OK;
    const long long groups = ((long long)nq + PCT_QW - 1) / PCT_QW;
    if (nref > 0x7fffffffLL || groups > 0x7fffffffLL) {
        hipt_set_error("score_counts: nref=%lld (counts are int32: nref < 2^31) or nq=%lld (at most %lld queries a call) outside the "
                       "envelope; nothing was launched", (long long)nref, (long long)nq, 0x7fffffffLL * PCT_QW);
        return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_ARG(q && ref, "score_counts: q / ref missing");
    HIPT_CHECK_ARG(less || leq || pct, "score_counts: no output asked for");
    HIPT_CHECK_ARG(((uintptr_t)q & 7) == 0 && ((uintptr_t)ref & 7) == 0 && ((uintptr_t)pct & 7) == 0 && ((uintptr_t)less & 3) == 0 &&
                       ((uintptr_t)leq & 3) == 0,
                   "score_counts: q / ref / pct need 8-byte, less / leq 4-byte alignment");
    const double scale = 50.0 / (double)nref;
    hipLaunchKernelGGL(pct_counts_kernel, dim3((unsigned)groups), dim3(PCT_THREADS), 0, (hipStream_t)stream, q, (long long)nq, ref,
                       (long long)nref, mode, scale, less, leq, pct);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
