// Bootstrapped evaluation metrics (bootstrapping.py:78-102): AUC, F1, accuracy and balanced accuracy of B resamples of n
// pooled predictions, one workgroup per replicate.
//
// A replicate is a multiset of the n samples, given as n drawn indices.  Everything up to the last divisions is integer:
//   1. histogram of the drawn indices into LDS counts cnt[n] (integer LDS atomics: the order of arrival cannot matter);
//   2. the K x K confusion counts conf[y][y_hat] += cnt[j];
//   3. per scored class c (class 1 alone for K = 2, every class one-vs-rest for K > 2) the samples are walked in the order of
//      that class's score (order[c][p], prepared on the host): an exclusive prefix sum E of the negatives' counts over the
//      positions, then  num_c = sum over positive positions p of cnt * (E[lo(p)] + E[hi(p)])  where [lo, hi) is the position
//      range of p's tie group: E[lo] negatives score strictly lower, E[hi] - E[lo] tie, so the sum is
//      2 #{pos > neg} + #{pos = neg}, in 64-bit integers;
//   4. thread 0 divides: auc_c = num_c / (2 P_c N_c), f1_c = 2tp / (2tp + fp + fn), accuracy = trace / n,
//      recall_c = tp_c / (tp_c + fn_c), and the means over the classes in ascending class order.
// Scores never reach the device, so ties are exactly the host's float64 equalities.  A replicate's result depends on its n
// indices only: not on its position in the call, the chunking of the call or the launch geometry.  No inline assembly.
#include "common.h"
#include "kernels.h"

namespace {

constexpr int BS_THREADS = 256;
constexpr int BS_WAVES = BS_THREADS / 64;
constexpr int BS_MAX_K = HIPT_BOOTSTRAP_MAX_CLASSES;

// dynamic LDS: cnt int[n] | E int[n + 1] | lab uint8[n] (y | y_hat << 4)
__global__ __launch_bounds__(BS_THREADS) void bootstrap_kernel(const int* __restrict__ Y, const int* __restrict__ Yh,
                                                               const int* __restrict__ order, const int* __restrict__ tie, int n, int K,
                                                               const int* __restrict__ idx, double* __restrict__ out, int* __restrict__ flags) {
    extern __shared__ int smem[];
    int* cnt = smem;
    int* E = smem + n;
    unsigned char* lab = (unsigned char*)(E + n + 1);
    __shared__ int conf[BS_MAX_K * BS_MAX_K];
    __shared__ int wsum[BS_WAVES];
    __shared__ long long wnum[BS_WAVES];
    __shared__ long long num[BS_MAX_K];
    __shared__ int bad;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int C = K == 2 ? 1 : K;   // scored classes
    bool mybad = false;   // an index or label outside its range: never followed, reported through the flag word
    for (int i = t; i < n; i += BS_THREADS) {
        cnt[i] = 0;
        int y = Y[i], yh = Yh[i];
        if ((unsigned)y >= (unsigned)K || (unsigned)yh >= (unsigned)K) {   // a label outside 0..K-1 would index past conf
            mybad = true;
            y = yh = 0;
        }
        lab[i] = (unsigned char)(y | (yh << 4));
    }
    if (t < BS_MAX_K * BS_MAX_K) conf[t] = 0;
    if (t == 0) {
        bad = 0;
        E[0] = 0;
    }
    __syncthreads();

    // 1. histogram of this replicate's draws
    const int* row = idx + (size_t)blockIdx.x * n;
    for (int i = t; i < n; i += BS_THREADS) {
        const int j = row[i];
        if ((unsigned)j < (unsigned)n) atomicAdd(&cnt[j], 1);
        else mybad = true;
    }
    __syncthreads();

    // 2. confusion counts
    for (int i = t; i < n; i += BS_THREADS) {
        const int c = cnt[i];
        if (c) atomicAdd(&conf[(lab[i] & 15) * K + (lab[i] >> 4)], c);
    }

    // 3. one scan per scored class; thread t owns the positions [p0, p1)
    const int per = (n + BS_THREADS - 1) / BS_THREADS;
    const int p0 = min(n, t * per), p1 = min(n, p0 + per);
    for (int c = 0; c < C; ++c) {
        const int label = K == 2 ? 1 : c;
        const int* ord = order + (size_t)c * n;
        const int* tg = tie + (size_t)c * n;
        int s = 0;
        for (int p = p0; p < p1; ++p) {
            int j = ord[p];
            if ((unsigned)j >= (unsigned)n) {
                mybad = true;
                j = n - 1;
            }
            s += (lab[j] & 15) == label ? 0 : cnt[j];
        }
        const int incl = wave_incl_scan(s, lane);
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();   // also: E and wnum of the previous class have been read
        int run = incl - s;
        for (int w = 0; w < wave; ++w) run += wsum[w];
        for (int p = p0; p < p1; ++p) {
            const int j = min((unsigned)ord[p], (unsigned)(n - 1));
            run += (lab[j] & 15) == label ? 0 : cnt[j];
            E[p + 1] = run;   // negatives at positions <= p
        }
        __syncthreads();
        long long acc = 0;
        for (int p = p0; p < p1; ++p) {
            const int j = min((unsigned)ord[p], (unsigned)(n - 1));
            const int w = cnt[j];
            if (w && (lab[j] & 15) == label) {
                const unsigned g = (unsigned)tg[p];
                const int lo = min((int)(g & 0xffffu), n), hi = min((int)(g >> 16), n);
                acc += (long long)w * (long long)(E[lo] + E[hi]);
            }
        }
#pragma unroll  // (wave_sum of common.h, written out: on a 64-bit value the call compiles to different code)
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) wnum[wave] = acc;
        __syncthreads();
        if (t == 0) {
            long long a = 0;
            for (int w = 0; w < BS_WAVES; ++w) a += wnum[w];
            num[c] = a;
        }
    }
    if (mybad) bad = 1;
    __syncthreads();

    // 4. the float64 epilogue: every operand below is an integer that float64 holds exactly
    if (t == 0) {
        bool degenerate = false;
        int trace = 0, present = 0;
        double auc = 0.0, f1 = 0.0, rec = 0.0;
        for (int c = 0; c < K; ++c) {
            int rowsum = 0, colsum = 0;
            for (int k = 0; k < K; ++k) {
                rowsum += conf[c * K + k];
                colsum += conf[k * K + c];
            }
            const int tp = conf[c * K + c];
            trace += tp;
            if (rowsum > 0) {
                rec += (double)tp / (double)rowsum;
                ++present;
            }
            const bool scored = K == 2 ? c == 1 : true;
            if (scored) {
                const int den = rowsum + colsum;   // 2tp + fp + fn
                f1 += den > 0 ? (double)(2 * tp) / (double)den : 0.0;
                const long long P = rowsum, Nn = n - rowsum;
                if (P == 0 || Nn == 0) degenerate = true;
                else auc += (double)num[K == 2 ? 0 : c] / (double)(2 * P * Nn);
            }
        }
        double* o = out + (size_t)blockIdx.x * 4;
        o[0] = degenerate ? __builtin_nan("") : auc / (double)C;
        o[1] = f1 / (double)C;
        o[2] = (double)trace / (double)n;
        o[3] = present > 0 ? rec / (double)present : 0.0;
        const int f = (degenerate ? HIPT_BOOTSTRAP_DEGENERATE : 0) | (bad ? HIPT_BOOTSTRAP_BAD_INPUT : 0);
        if (f) atomicOr(flags, f);
    }
}

}  // namespace

size_t hipt_bootstrap_lds_bytes(int n) { return ((size_t)n * 4 + ((size_t)n + 1) * 4 + (size_t)n + 15) & ~(size_t)15; }

int hipt_launch_bootstrap(const int* Y, const int* Yh, const int* order, const int* tie, int n, int K, const int* idx, int B, double* out,
                          int* flags, hipStream_t st) {
    hipLaunchKernelGGL(bootstrap_kernel, dim3((unsigned)B), dim3(BS_THREADS), hipt_bootstrap_lds_bytes(n), st, Y, Yh, order, tie, n, K, idx,
                       out, flags);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

extern "C" int hipt_bootstrap_metrics(const int32_t* Y, const int32_t* Y_hat, const int32_t* order, const int32_t* tie, int n, int K,
                                      const int32_t* idx, int B, double* out, int32_t* flags, void* stream) {
    HIPT_CHECK_ARG(Y && Y_hat && order && tie && idx && out && flags, "bootstrap_metrics: null argument");
    HIPT_CHECK_ARG(n >= 1 && K >= 2 && B >= 1, "bootstrap_metrics: n=%d (>= 1), K=%d (>= 2), B=%d (>= 1)", n, K, B);
    if (n > HIPT_BOOTSTRAP_MAX_N || K > HIPT_BOOTSTRAP_MAX_CLASSES || B > HIPT_BOOTSTRAP_MAX_REPLICATES) {
        hipt_set_error("bootstrap_metrics: n=%d / K=%d / B=%d beyond the limits %d / %d / %d (nothing was launched)", n, K, B,
                       HIPT_BOOTSTRAP_MAX_N, HIPT_BOOTSTRAP_MAX_CLASSES, HIPT_BOOTSTRAP_MAX_REPLICATES);
        return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_ARG(((uintptr_t)out & 7) == 0, "bootstrap_metrics: out must be 8-byte aligned");
    return hipt_launch_bootstrap(Y, Y_hat, order, tie, n, K, idx, B, out, flags, (hipStream_t)stream);
}
