// Macenko stain normalisation of 8-bit RGB images (extract_features_fp.py:41-60, --use_transforms macenko: torchstain's
// MacenkoNormalizer(backend='torch') per item); DESIGN.md 25, include/hipt_abmil.h.
//
// A call takes R images of h x w pixels, planar [R, 3, h, w] or interleaved [R, h, w, 3].  Nothing per pixel is ever stored: the
// optical density of a byte comes from a 256-entry table in LDS, and phi / C are recomputed from the bytes in every pass by the ONE
// function each has below (px_phi, px_conc), so that all passes of a select see the same bits.  The file is built with
// -ffp-contract=off and the keys are written in explicit __fmul_rn / __fmaf_rn on top of that.
//
//   lut      the table -log((v + 1) / Io), v = 0..255, float32, into the workspace (every pass of `fit` loads these 1024 bytes);
//            it also zeroes the histograms
//   cov      per workgroup: n and the sums of OD and OD OD^T over its tissue pixels, in float64 -> one slab of 10 doubles
//   finish1  one thread per image: the slabs added in slab order, the unbiased covariance, Jacobi (float64), the plane E, the ranks
//   select   three histogram passes (11 + 11 + 10 bits of the order-preserving integer image of the float32 key) for TWO order
//            statistics at once: phi at the ranks of alpha and 100 - alpha over the tissue pixels, then C[0] and C[1] at the rank of
//            99 over all pixels.  Integer counts only: LDS histogram (a wave whose lanes all hit one bin adds once), then one global
//            integer atomic per non-empty bin and workgroup.  Integer sums do not depend on their order.
//   scan     one workgroup per image after each pass: the bin that holds the rank, the rank within it, the histogram zeroed for
//            the next pass.  After the third pass the key is complete; its thread 0 then finishes: the stain vectors HE and the
//            2 x 3 matrix P = (HE^T HE)^-1 HE^T after phi, maxC / the status / the outputs after C.
//   apply    C = P OD, out = Io exp(-(HERef (C maxCRef / maxC))), clipped at 255 and truncated; fallback images copied through.
// -0.0 and +0.0 are EQUAL keys: a zero key is +0.0 before its integer image is taken (ordered_key).
// A workgroup's pixels, the slab count and the order of every float64 sum depend on h * w alone: an image's HE, maxC, status and
// bytes do not depend on R, on its place in the batch or on its neighbours.  No allocation, no host synchronisation.
#include <math.h>

#include "common.h"
#include "workspace.h"

namespace {

constexpr int MK_THREADS = 256;
constexpr int MK_PX = 16;                          // pixels per thread and trip: three 16-byte loads in either layout
constexpr int MK_WG_PX = MK_THREADS * MK_PX;       // 4096
constexpr int MK_MAX_WG = 1024;                    // workgroups per image at most (then each strides over the image)
constexpr int MK_BINS = 2048;                      // 11 bits; the last pass uses 1024 of them
constexpr int MK_SLAB = 10;                        // n, sum OD[3], sum OD OD^T [6: 00 01 02 11 12 22]
constexpr float MK_HEREF[6] = {0.5626f, 0.2159f, 0.7201f, 0.8012f, 0.4062f, 0.5581f};
constexpr float MK_MAXCREF[2] = {1.9705f, 1.0308f};

// per image, in the workspace; the first 16 words are what `aux` receives
struct MkState {
    float E[6];       // e1[3], e2[3]: the eigenvectors of the middle and the largest eigenvalue
    float phi[2];     // minPhi, maxPhi
    float P[6];       // row j = (HE^T HE)^-1 HE^T [j, :]
    int n;            // tissue pixels
    int status;
    float HE[6];      // [3, 2]
    float maxC[2];
    uint32_t prefix[2];
    int krem[2];
    int pad[4];
};
static_assert(sizeof(MkState) == 128, "MkState is 32 words");

struct MkGeom {
    const uint8_t* src;
    long long npix;   // h * w
    int nwg;          // workgroups per image
    int vec;          // npix % 16 == 0 and every base 16-byte aligned: whole 16-byte vectors, no bound checks
};

__device__ __forceinline__ float od_entry(int v, float Io) { return -logf(__fdiv_rn((float)(v + 1), Io)); }

__device__ __forceinline__ float dot3(const float* a, float x, float y, float z) {
    return __fmaf_rn(a[2], z, __fmaf_rn(a[1], y, __fmul_rn(a[0], x)));
}
// THE keys: every pass, the apply kernel and the key dump go through these two
__device__ __forceinline__ float px_phi(const float* E, float r, float g, float b) { return atan2f(dot3(E + 3, r, g, b), dot3(E, r, g, b)); }
__device__ __forceinline__ float px_conc(const float* P, int j, float r, float g, float b) { return dot3(P + 3 * j, r, g, b); }

// order-preserving integer image of a float32; -0.0 and +0.0 give the same key
__device__ __forceinline__ uint32_t ordered_key(float x) {
    if (x == 0.0f) x = 0.0f;
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// 16 pixels from pixel p0 of one image as 12 words; byte (pixel j, channel c) is byte 3 j + c (interleaved) or 16 c + j (planar)
template <bool IL> __device__ __forceinline__ void load_px(const uint8_t* img, long long npix, long long p0, bool vec, uint32_t w[12]) {
    if (vec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const u32x4 q = IL ? ((const u32x4*)(img + p0 * 3))[c] : *(const u32x4*)(img + (long long)c * npix + p0);
            w[4 * c] = q[0], w[4 * c + 1] = q[1], w[4 * c + 2] = q[2], w[4 * c + 3] = q[3];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i] = 0;
#pragma unroll
        for (int k = 0; k < 48; ++k) {
            const int j = IL ? k / 3 : k & 15, c = IL ? k % 3 : k >> 4;
            if (p0 + j < npix) w[k >> 2] |= (uint32_t)img[IL ? (p0 + j) * 3 + c : (long long)c * npix + p0 + j] << (8 * (k & 3));
        }
    }
}
template <bool IL> __device__ __forceinline__ int px_byte(const uint32_t w[12], int j, int c) {
    const int k = IL ? 3 * j + c : 16 * c + j;
    return (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
}

__device__ __forceinline__ void load_lut(float* lut_s, const float* lut) {
    for (int i = threadIdx.x; i < 256; i += MK_THREADS) lut_s[i] = lut[i];
}

// the table, and every histogram zeroed (workgroup r: image r's): the workspace carries nothing from call to call
__global__ void mk_lut_kernel(float* lut, float Io, int* hist) {
    if (blockIdx.x == 0) lut[threadIdx.x] = od_entry(threadIdx.x, Io);
    for (int i = threadIdx.x; i < 2 * MK_BINS; i += 256) hist[(long long)blockIdx.x * 2 * MK_BINS + i] = 0;
}

// ---- covariance sums -----------------------------------------------------------------------------------------------------------
template <bool IL> __global__ __launch_bounds__(MK_THREADS) void mk_cov_kernel(const MkGeom G, const float* __restrict__ lut, float beta,
                                                                              double* __restrict__ slabs) {
    __shared__ float lut_s[256];
    __shared__ double red[MK_THREADS / 64][MK_SLAB];
    const int img = blockIdx.x / G.nwg, wg = blockIdx.x - img * G.nwg;
    const uint8_t* base = G.src + (long long)img * G.npix * 3;
    load_lut(lut_s, lut);
    __syncthreads();
    double s[MK_SLAB];
#pragma unroll
    for (int i = 0; i < MK_SLAB; ++i) s[i] = 0.0;
    const long long nchunks = (G.npix + MK_PX - 1) / MK_PX;
    for (long long c0 = (long long)wg * MK_THREADS; c0 < nchunks; c0 += (long long)G.nwg * MK_THREADS) {
        const long long ch = c0 + threadIdx.x;
        if (ch >= nchunks) continue;
        const long long p0 = ch * MK_PX;
        uint32_t w[12];
        load_px<IL>(base, G.npix, p0, G.vec != 0, w);
#pragma unroll
        for (int j = 0; j < MK_PX; ++j) {
            const float r = lut_s[px_byte<IL>(w, j, 0)], g = lut_s[px_byte<IL>(w, j, 1)], b = lut_s[px_byte<IL>(w, j, 2)];
            if (p0 + j < G.npix && !(r < beta) && !(g < beta) && !(b < beta)) {
                const double x = r, y = g, z = b;
                s[0] += 1.0;
                s[1] += x, s[2] += y, s[3] += z;
                s[4] += x * x, s[5] += x * y, s[6] += x * z, s[7] += y * y, s[8] += y * z, s[9] += z * z;
            }
        }
    }
    // a fixed tree: lanes of a wave, then the four waves in order
#pragma unroll
    for (int i = 0; i < MK_SLAB; ++i) {
#pragma unroll  // (wave_sum of common.h, written out: on a double the call compiles to different code)
        for (int o = 32; o > 0; o >>= 1) s[i] += __shfl_xor(s[i], o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < MK_SLAB; ++i) red[threadIdx.x >> 6][i] = s[i];
    }
    __syncthreads();
    if (threadIdx.x < MK_SLAB) {
        double t = red[0][threadIdx.x];
        for (int wv = 1; wv < MK_THREADS / 64; ++wv) t += red[wv][threadIdx.x];
        slabs[(long long)blockIdx.x * MK_SLAB + threadIdx.x] = t;
    }
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }
__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }

// cyclic Jacobi of a symmetric 3 x 3 matrix: eigenvalues in d, eigenvectors in the columns of V
__device__ void jacobi3(double A[3][3], double d[3], double V[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; ++sweep) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        const double dia = A[0][0] * A[0][0] + A[1][1] * A[1][1] + A[2][2] * A[2][2];
        if (!(off > 1e-34 * dia)) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {   // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {   // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 3; ++i) d[i] = A[i][i];
}

// percentile's rank: k = 1 + round_half_even(0.01 * q * (len - 1)), the products taken left to right in float64
__device__ __forceinline__ int rank_of(double q, long long len) { return 1 + (int)rint((0.01 * q) * (double)(len - 1)); }

__global__ void mk_finish1_kernel(MkState* __restrict__ st, const double* __restrict__ slabs, int R, int nwg, double alpha) {
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= R) return;
    double s[MK_SLAB];
    for (int i = 0; i < MK_SLAB; ++i) s[i] = 0.0;
    for (int wg = 0; wg < nwg; ++wg)
        for (int i = 0; i < MK_SLAB; ++i) s[i] += slabs[((long long)img * nwg + wg) * MK_SLAB + i];
    MkState S = {};
    const long long n = (long long)s[0];
    S.n = (int)n;
    S.status = 1;
    if (n >= 2) {
        const double inv = 1.0 / (double)(n - 1), dn = (double)n;
        double A[3][3];
        const int ix[3][3] = {{4, 5, 6}, {5, 7, 8}, {6, 8, 9}};
        bool ok = true;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                A[i][j] = (s[ix[i][j]] - s[1 + i] * s[1 + j] / dn) * inv;
                ok = ok && finite_d(A[i][j]);
            }
        if (ok) {
            double d[3], V[3][3];
            jacobi3(A, d, V);
            int lo = 0, hi = 0;
            for (int i = 1; i < 3; ++i) {
                if (d[i] < d[lo]) lo = i;
                if (d[i] >= d[hi]) hi = i;
            }
            if (lo == hi) lo = 0, hi = 2;   // three equal eigenvalues
            const int col[2] = {3 - lo - hi, hi};
            for (int e = 0; e < 2; ++e) {
                int big = 0;
                for (int i = 1; i < 3; ++i)
                    if (fabs(V[i][col[e]]) > fabs(V[big][col[e]])) big = i;
                const double sg = V[big][col[e]] < 0.0 ? -1.0 : 1.0;
                for (int i = 0; i < 3; ++i) S.E[3 * e + i] = (float)(sg * V[i][col[e]]);
            }
            S.status = 0;
            S.krem[0] = rank_of(alpha, n);
            S.krem[1] = rank_of(100.0 - alpha, n);
        }
    }
    st[img] = S;
}

// P = (HE^T HE)^-1 HE^T of a float32 HE [3, 2], in float64, rounded once
__device__ __forceinline__ void pinv_of(const float* HE, float* P) {
    double a = 0.0, b = 0.0, d = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double h0 = HE[2 * c], h1 = HE[2 * c + 1];
        a += h0 * h0, b += h0 * h1, d += h1 * h1;
    }
    const double det = a * d - b * b;
    for (int c = 0; c < 3; ++c) {
        const double h0 = HE[2 * c], h1 = HE[2 * c + 1];
        P[c] = (float)((d * h0 - b * h1) / det);
        P[3 + c] = (float)((a * h1 - b * h0) / det);
    }
}

// ---- select --------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void wave_hist_add(int* h, uint32_t bin, bool part) {
    const unsigned long long m = __ballot(part);
    if (m == 0) return;
    const int first = __ffsll((long long)m) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)bin, first, 64);
    if (__ballot(part && bin == b0) == m) {   // one bin for the whole wave (flat areas): one add
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&h[b0], __popcll(m));
    } else if (part) {
        atomicAdd(&h[bin], 1);
    }
}

// STAGE 0: phi over the tissue pixels (both ranks share the key); STAGE 1: C[0] and C[1] over all pixels
template <bool IL, int STAGE> __global__ __launch_bounds__(MK_THREADS) void mk_select_kernel(const MkGeom G, const float* __restrict__ lut,
                                                                                            float beta, const MkState* __restrict__ st,
                                                                                            int* __restrict__ hist, int pass) {
    __shared__ float lut_s[256];
    __shared__ int h[2 * MK_BINS];
    __shared__ float coef[6];
    const int img = blockIdx.x / G.nwg, wg = blockIdx.x - img * G.nwg;
    if (st[img].status != 0) return;   // (the whole workgroup)
    const uint8_t* base = G.src + (long long)img * G.npix * 3;
    load_lut(lut_s, lut);
    for (int i = threadIdx.x; i < 2 * MK_BINS; i += MK_THREADS) h[i] = 0;
    if (threadIdx.x < 6) coef[threadIdx.x] = STAGE == 0 ? st[img].E[threadIdx.x] : st[img].P[threadIdx.x];
    const uint32_t pre0 = st[img].prefix[0], pre1 = st[img].prefix[1];
    __syncthreads();
    const int shift = pass == 0 ? 21 : (pass == 1 ? 10 : 0);
    const int up = pass == 1 ? 21 : 10;   // (pass 0 compares nothing)
    const uint32_t mask = pass == 2 ? 1023u : 2047u;
    const bool shared_bins = STAGE == 0 && pass == 0;   // both ranks count the same keys: counted once, flushed twice
    const long long nchunks = (G.npix + MK_PX - 1) / MK_PX;
    for (long long c0 = (long long)wg * MK_THREADS; c0 < nchunks; c0 += (long long)G.nwg * MK_THREADS) {
        const long long ch = c0 + threadIdx.x;
        const bool live = ch < nchunks;
        const long long p0 = (live ? ch : 0) * MK_PX;
        uint32_t w[12];
        load_px<IL>(base, G.npix, p0, G.vec != 0, w);
#pragma unroll
        for (int j = 0; j < MK_PX; ++j) {
            const float r = lut_s[px_byte<IL>(w, j, 0)], g = lut_s[px_byte<IL>(w, j, 1)], b = lut_s[px_byte<IL>(w, j, 2)];
            bool in = live && p0 + j < G.npix;
            uint32_t k0, k1;
            if (STAGE == 0) {
                in = in && !(r < beta) && !(g < beta) && !(b < beta);
                k0 = k1 = ordered_key(px_phi(coef, r, g, b));
            } else {
                k0 = ordered_key(px_conc(coef, 0, r, g, b));
                k1 = ordered_key(px_conc(coef, 1, r, g, b));
            }
            wave_hist_add(h, (k0 >> shift) & mask, in && (pass == 0 || (k0 >> up) == pre0));
            if (!shared_bins) wave_hist_add(h + MK_BINS, (k1 >> shift) & mask, in && (pass == 0 || (k1 >> up) == pre1));
        }
    }
    __syncthreads();
    int* out = hist + (long long)img * 2 * MK_BINS;
    for (int i = threadIdx.x; i < 2 * MK_BINS; i += MK_THREADS) {
        const int v = shared_bins ? h[i & (MK_BINS - 1)] : h[i];
        if (v) atomicAdd(&out[i], v);
    }
}

// After pass `pass` of stage `stage`: narrows both selects of an image, zeroes its histogram; after the last pass finishes the stage.
__global__ __launch_bounds__(MK_THREADS) void mk_scan_kernel(MkState* st, int* hist, int stage, int pass, long long npix,
                                                            float* __restrict__ HE_out, float* __restrict__ maxC_out,
                                                            int32_t* __restrict__ status_out, float* __restrict__ aux) {
    __shared__ int part[2][MK_THREADS];
    const int img = blockIdx.x, tid = threadIdx.x;
    MkState* S = st + img;
    int* h = hist + (long long)img * 2 * MK_BINS;
    constexpr int PER = MK_BINS / MK_THREADS;   // 8
    const bool run = S->status == 0;
    if (run) {
        for (int s = 0; s < 2; ++s) {
            int sum = 0;
            for (int j = 0; j < PER; ++j) sum += h[s * MK_BINS + tid * PER + j];
            part[s][tid] = sum;
        }
    }
    __syncthreads();
    if (run && tid < 2) {
        const int s = tid, k = S->krem[s];
        int cum = 0, t = 0, bin = -1;
        for (; t < MK_THREADS; ++t) {
            if (cum + part[s][t] >= k) break;
            cum += part[s][t];
        }
        if (t < MK_THREADS && k >= 1)
            for (int j = 0; j < PER; ++j) {
                const int c = h[s * MK_BINS + t * PER + j];
                if (cum + c >= k) {
                    bin = t * PER + j;
                    break;
                }
                cum += c;
            }
        if (bin < 0) {
            S->status = 1;   // the rank is in no bin: the passes did not see the same keys.  No second try.
        } else {
            S->prefix[s] = pass == 0 ? (uint32_t)bin : ((S->prefix[s] << (pass == 1 ? 11 : 10)) | (uint32_t)bin);
            S->krem[s] = k - cum;
        }
    }
    __syncthreads();
    if (run)
        for (int i = tid; i < 2 * MK_BINS; i += MK_THREADS) h[i] = 0;
    if (pass != 2 || tid != 0) return;
    if (stage == 0) {
        if (S->status != 0) return;
        const float p0 = key_value(S->prefix[0]), p1 = key_value(S->prefix[1]);
        S->phi[0] = p0, S->phi[1] = p1;
        double vmin[3], vmax[3];
        const double c0 = cos((double)p0), s0 = sin((double)p0), c1 = cos((double)p1), s1 = sin((double)p1);
        for (int c = 0; c < 3; ++c) {
            vmin[c] = (double)S->E[c] * c0 + (double)S->E[3 + c] * s0;
            vmax[c] = (double)S->E[c] * c1 + (double)S->E[3 + c] * s1;
        }
        const bool min_first = vmin[0] > vmax[0];
        bool ok = true;
        for (int c = 0; c < 3; ++c) {
            S->HE[2 * c] = (float)(min_first ? vmin[c] : vmax[c]);
            S->HE[2 * c + 1] = (float)(min_first ? vmax[c] : vmin[c]);
            ok = ok && finite_f(S->HE[2 * c]) && finite_f(S->HE[2 * c + 1]);
        }
        if (!ok) {
            S->status = 1;
            return;
        }
        pinv_of(S->HE, S->P);
        S->prefix[0] = S->prefix[1] = 0;
        S->krem[0] = S->krem[1] = rank_of(99.0, npix);
        return;
    }
    if (S->status == 0) {
        for (int j = 0; j < 2; ++j) {
            S->maxC[j] = key_value(S->prefix[j]);
            if (!finite_f(S->maxC[j]) || !(S->maxC[j] > 0.0f)) S->status = 1;
        }
    }
    const bool ok = S->status == 0;
    for (int i = 0; i < 6; ++i) HE_out[(long long)img * 6 + i] = ok ? S->HE[i] : 0.0f;
    for (int j = 0; j < 2; ++j) maxC_out[(long long)img * 2 + j] = ok ? S->maxC[j] : 0.0f;
    status_out[img] = S->status;
    if (aux)
        for (int i = 0; i < 16; ++i) aux[(long long)img * 16 + i] = ((const float*)S)[i];
}

// ---- apply ---------------------------------------------------------------------------------------------------------------------
template <bool IL> __global__ __launch_bounds__(MK_THREADS) void mk_apply_kernel(const MkGeom G, float Io, const float* __restrict__ HE,
                                                                                const float* __restrict__ maxC,
                                                                                const int32_t* __restrict__ status,
                                                                                const float* __restrict__ ref_HE,
                                                                                const float* __restrict__ ref_maxC, void* __restrict__ dst,
                                                                                int dst_f32) {
    __shared__ float lut_s[256];
    __shared__ float P[6], M[6], sc[2];
    const int img = blockIdx.x / G.nwg, wg = blockIdx.x - img * G.nwg;
    const uint8_t* base = G.src + (long long)img * G.npix * 3;
    const bool through = status != nullptr && status[img] != 0;
    lut_s[threadIdx.x] = od_entry(threadIdx.x, Io);
    if (threadIdx.x == 0) pinv_of(HE + (long long)img * 6, P);
    if (threadIdx.x >= 64 && threadIdx.x < 70) M[threadIdx.x - 64] = ref_HE ? ref_HE[threadIdx.x - 64] : MK_HEREF[threadIdx.x - 64];
    if (threadIdx.x >= 128 && threadIdx.x < 130) {
        const int j = threadIdx.x - 128;
        sc[j] = __fdiv_rn(ref_maxC ? ref_maxC[j] : MK_MAXCREF[j], maxC[(long long)img * 2 + j]);
    }
    __syncthreads();
    const long long nchunks = (G.npix + MK_PX - 1) / MK_PX;
    for (long long c0 = (long long)wg * MK_THREADS; c0 < nchunks; c0 += (long long)G.nwg * MK_THREADS) {
        const long long ch = c0 + threadIdx.x;
        if (ch >= nchunks) continue;
        const long long p0 = ch * MK_PX;
        uint32_t w[12];
        load_px<IL>(base, G.npix, p0, G.vec != 0, w);
        uint32_t o[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) o[i] = w[i];
        if (!through) {
#pragma unroll
            for (int i = 0; i < 12; ++i) o[i] = 0;
#pragma unroll
            for (int j = 0; j < MK_PX; ++j) {
                const float r = lut_s[px_byte<IL>(w, j, 0)], g = lut_s[px_byte<IL>(w, j, 1)], b = lut_s[px_byte<IL>(w, j, 2)];
                const float a0 = __fmul_rn(px_conc(P, 0, r, g, b), sc[0]), a1 = __fmul_rn(px_conc(P, 1, r, g, b), sc[1]);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float e = __fmaf_rn(M[2 * c + 1], a1, __fmul_rn(M[2 * c], a0));
                    const float v = fminf(__fmul_rn(Io, expf(-e)), 255.0f);   // (a NaN becomes 255)
                    const int k = IL ? 3 * j + c : 16 * c + j;
                    o[k >> 2] |= (uint32_t)(int)v << (8 * (k & 3));
                }
            }
        }
        if (dst_f32) {   // planar float32 [R, 3, h, w] = byte / 255
            float* d = (float*)dst + (long long)img * 3 * G.npix;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float f[MK_PX];
#pragma unroll
                for (int j = 0; j < MK_PX; ++j) f[j] = __fdiv_rn((float)px_byte<IL>(o, j, c), 255.0f);
                float* q = d + (long long)c * G.npix + p0;
                if (G.vec) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        f32x4 t;
                        t[0] = f[4 * v], t[1] = f[4 * v + 1], t[2] = f[4 * v + 2], t[3] = f[4 * v + 3];
                        ((f32x4*)q)[v] = t;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < MK_PX; ++j)
                        if (p0 + j < G.npix) q[j] = f[j];
                }
            }
        } else {   // uint8, the input's layout
            uint8_t* d = (uint8_t*)dst + (long long)img * 3 * G.npix;
            if (G.vec) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    u32x4 t;
                    t[0] = o[4 * c], t[1] = o[4 * c + 1], t[2] = o[4 * c + 2], t[3] = o[4 * c + 3];
                    if (IL)
                        ((u32x4*)(d + p0 * 3))[c] = t;
                    else
                        *(u32x4*)(d + (long long)c * G.npix + p0) = t;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 48; ++k) {
                    const int j = IL ? k / 3 : k & 15, c = IL ? k % 3 : k >> 4;
                    if (p0 + j < G.npix) d[IL ? (p0 + j) * 3 + c : (long long)c * G.npix + p0 + j] = (uint8_t)((o[k >> 2] >> (8 * (k & 3))) & 255u);
                }
            }
        }
    }
}

// the keys of every pixel of (small) images, by the functions the passes use: phi, C[0], C[1] as float32 [R, 3, npix], tissue [R, npix]
template <bool IL> __global__ __launch_bounds__(MK_THREADS) void mk_keys_kernel(const MkGeom G, float Io, float beta, const float* __restrict__ aux,
                                                                               float* __restrict__ keys, uint8_t* __restrict__ tissue) {
    __shared__ float lut_s[256];
    __shared__ float E[6], P[6];
    const int img = blockIdx.x / G.nwg, wg = blockIdx.x - img * G.nwg;
    const uint8_t* base = G.src + (long long)img * G.npix * 3;
    lut_s[threadIdx.x] = od_entry(threadIdx.x, Io);
    if (threadIdx.x < 6) E[threadIdx.x] = aux[(long long)img * 16 + threadIdx.x], P[threadIdx.x] = aux[(long long)img * 16 + 8 + threadIdx.x];
    __syncthreads();
    const long long nchunks = (G.npix + MK_PX - 1) / MK_PX;
    for (long long c0 = (long long)wg * MK_THREADS; c0 < nchunks; c0 += (long long)G.nwg * MK_THREADS) {
        const long long ch = c0 + threadIdx.x;
        if (ch >= nchunks) continue;
        const long long p0 = ch * MK_PX;
        uint32_t w[12];
        load_px<IL>(base, G.npix, p0, false, w);
#pragma unroll
        for (int j = 0; j < MK_PX; ++j) {
            if (p0 + j >= G.npix) continue;
            const float r = lut_s[px_byte<IL>(w, j, 0)], g = lut_s[px_byte<IL>(w, j, 1)], b = lut_s[px_byte<IL>(w, j, 2)];
            float* k = keys + (long long)img * 3 * G.npix + p0 + j;
            k[0] = px_phi(E, r, g, b);
            k[G.npix] = px_conc(P, 0, r, g, b);
            k[2 * G.npix] = px_conc(P, 1, r, g, b);
            tissue[(long long)img * G.npix + p0 + j] = (!(r < beta) && !(g < beta) && !(b < beta)) ? 1 : 0;
        }
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
int wg_per_image(long long npix) {
    const long long n = (npix + MK_WG_PX - 1) / MK_WG_PX;
    return (int)(n < MK_MAX_WG ? n : MK_MAX_WG);
}

struct MkScratch {
    float* lut;
    MkState* st;
    double* slabs;
    int* hist;
    float *HE, *maxC;
    int32_t* status;
};

MkScratch carve_macenko(Carver& c, int R, long long npix) {
    MkScratch s;
    s.lut = c.take<float>(256);
    s.st = c.take<MkState>((size_t)R);
    s.slabs = c.take<double>((size_t)R * wg_per_image(npix) * MK_SLAB);
    s.hist = c.take<int>((size_t)R * 2 * MK_BINS);
    s.HE = c.take<float>((size_t)R * 6);      // where `normalize` keeps what the caller does not ask for
    s.maxC = c.take<float>((size_t)R * 2);
    s.status = c.take<int32_t>((size_t)R);
    return s;
}

bool finite_host(double v) { return v == v && v - v == 0.0; }

// the refusals every entry point shares; 0 when the geometry can run
int check_geometry(const char* who, const void* src, int R, int h, int w, double Io) {
    HIPT_CHECK_ARG(R >= 1 && h >= 1 && w >= 1, "%s: %d images of %d x %d", who, R, h, w);
    const long long npix = (long long)h * w;
    if (npix >= (1LL << 31) || (long long)R * wg_per_image(npix) >= (1LL << 31)) {
        hipt_set_error("%s: %d images of %d x %d outside the envelope (h * w below 2^31, R * workgroups below 2^31); nothing was launched", who, R,
                       h, w);
        return HIPT_E_UNSUPPORTED;
    }
    HIPT_CHECK_ARG(finite_host(Io) && Io > 0.0, "%s: Io = %g is not positive", who, Io);
    HIPT_CHECK_ARG(src != nullptr, "%s: src missing", who);
    return HIPT_OK;
}

int check_fit_params(const char* who, double alpha, double beta) {
    HIPT_CHECK_ARG(finite_host(alpha) && alpha > 0.0 && alpha < 50.0, "%s: alpha = %g is outside (0, 50)", who, alpha);
    HIPT_CHECK_ARG(finite_host(beta) && beta >= 0.0, "%s: beta = %g is negative", who, beta);
    return HIPT_OK;
}

MkGeom geometry(const uint8_t* src, int h, int w, const void* other) {
    MkGeom G;
    G.src = src;
    G.npix = (long long)h * w;
    G.nwg = wg_per_image(G.npix);
    G.vec = (G.npix % MK_PX == 0 && (((uintptr_t)src | (uintptr_t)other) & 15) == 0) ? 1 : 0;
    return G;
}

int fit_launches(const MkGeom& G, int interleaved, int R, float Io, double alpha, float beta, const MkScratch& s, float* HE, float* maxC,
                 int32_t* status, float* aux, hipStream_t stream) {
    const dim3 grid((unsigned)((long long)R * G.nwg)), block(MK_THREADS);
    hipLaunchKernelGGL(mk_lut_kernel, dim3((unsigned)R), dim3(256), 0, stream, s.lut, Io, s.hist);
    HIPT_CHECK_LAUNCH();
    if (interleaved)
        hipLaunchKernelGGL(mk_cov_kernel<true>, grid, block, 0, stream, G, s.lut, beta, s.slabs);
    else
        hipLaunchKernelGGL(mk_cov_kernel<false>, grid, block, 0, stream, G, s.lut, beta, s.slabs);
    HIPT_CHECK_LAUNCH();
    hipLaunchKernelGGL(mk_finish1_kernel, dim3((unsigned)((R + 63) / 64)), dim3(64), 0, stream, s.st, s.slabs, R, G.nwg, alpha);
    HIPT_CHECK_LAUNCH();
    for (int stage = 0; stage < 2; ++stage)
        for (int pass = 0; pass < 3; ++pass) {
            if (stage == 0 && interleaved)
                hipLaunchKernelGGL((mk_select_kernel<true, 0>), grid, block, 0, stream, G, s.lut, beta, s.st, s.hist, pass);
            else if (stage == 0)
                hipLaunchKernelGGL((mk_select_kernel<false, 0>), grid, block, 0, stream, G, s.lut, beta, s.st, s.hist, pass);
            else if (interleaved)
                hipLaunchKernelGGL((mk_select_kernel<true, 1>), grid, block, 0, stream, G, s.lut, beta, s.st, s.hist, pass);
            else
                hipLaunchKernelGGL((mk_select_kernel<false, 1>), grid, block, 0, stream, G, s.lut, beta, s.st, s.hist, pass);
            HIPT_CHECK_LAUNCH();
            hipLaunchKernelGGL(mk_scan_kernel, dim3((unsigned)R), block, 0, stream, s.st, s.hist, stage, pass, G.npix, HE, maxC, status, aux);
            HIPT_CHECK_LAUNCH();
        }
    return HIPT_OK;
}

int apply_launch(const MkGeom& G, int interleaved, int R, float Io, const float* HE, const float* maxC, const int32_t* status,
                 const float* ref_HE, const float* ref_maxC, void* dst, int dst_f32, hipStream_t stream) {
    const dim3 grid((unsigned)((long long)R * G.nwg)), block(MK_THREADS);
    if (interleaved)
        hipLaunchKernelGGL(mk_apply_kernel<true>, grid, block, 0, stream, G, Io, HE, maxC, status, ref_HE, ref_maxC, dst, dst_f32);
    else
        hipLaunchKernelGGL(mk_apply_kernel<false>, grid, block, 0, stream, G, Io, HE, maxC, status, ref_HE, ref_maxC, dst, dst_f32);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

}  // namespace

extern "C" size_t hipt_macenko_workspace_bytes(int R, int h, int w) {
    if (R < 1 || h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) return 0;
    return dry_run([&](Carver& c) { carve_macenko(c, R, (long long)h * w); });
}

extern "C" int hipt_macenko_fit(const uint8_t* src, int interleaved, int R, int h, int w, double Io, double alpha, double beta, float* HE,
                                float* maxC, int32_t* status, float* aux, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_geometry("macenko_fit", src, R, h, w, Io)) return rc;
    if (int rc = check_fit_params("macenko_fit", alpha, beta)) return rc;
    HIPT_CHECK_ARG(HE && maxC && status, "macenko_fit: HE / maxC / status missing");
    HIPT_CHECK_ARG((((uintptr_t)HE | (uintptr_t)maxC | (uintptr_t)status | (uintptr_t)aux) & 3) == 0,
                   "macenko_fit: HE / maxC / status / aux need 4-byte alignment");
    Carver c(ws, ws_bytes);
    const MkScratch s = carve_macenko(c, R, (long long)h * w);
    if (int rc = check_workspace(c, "macenko_fit")) return rc;
    HIPT_CHECK_ARG(ws != nullptr, "macenko_fit: workspace missing");
    return fit_launches(geometry(src, h, w, nullptr), interleaved != 0, R, (float)Io, alpha, (float)beta, s, HE, maxC, status, aux,
                        (hipStream_t)stream);
}

extern "C" int hipt_macenko_apply(const uint8_t* src, int interleaved, int R, int h, int w, double Io, const float* HE, const float* maxC,
                                  const int32_t* status, const float* ref_HE, const float* ref_maxC, void* dst, int dst_f32, void* stream) {
    if (int rc = check_geometry("macenko_apply", src, R, h, w, Io)) return rc;
    HIPT_CHECK_ARG(HE && maxC && dst, "macenko_apply: HE / maxC / dst missing");
    HIPT_CHECK_ARG((const void*)src != dst, "macenko_apply: dst is src");
    HIPT_CHECK_ARG((((uintptr_t)HE | (uintptr_t)maxC | (uintptr_t)status | (uintptr_t)ref_HE | (uintptr_t)ref_maxC) & 3) == 0 &&
                       (!dst_f32 || ((uintptr_t)dst & 3) == 0),
                   "macenko_apply: HE / maxC / status / the target / a float32 dst need 4-byte alignment");
    return apply_launch(geometry(src, h, w, dst), interleaved != 0, R, (float)Io, HE, maxC, status, ref_HE, ref_maxC, dst, dst_f32 != 0,
                        (hipStream_t)stream);
}

extern "C" int hipt_macenko_normalize(const uint8_t* src, int interleaved, int R, int h, int w, double Io, double alpha, double beta,
                                      const float* ref_HE, const float* ref_maxC, void* dst, int dst_f32, float* HE, float* maxC,
                                      int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    if (int rc = check_geometry("macenko_normalize", src, R, h, w, Io)) return rc;
    if (int rc = check_fit_params("macenko_normalize", alpha, beta)) return rc;
    HIPT_CHECK_ARG(dst != nullptr && (const void*)src != dst, "macenko_normalize: dst missing, or src");
    HIPT_CHECK_ARG((((uintptr_t)HE | (uintptr_t)maxC | (uintptr_t)status | (uintptr_t)ref_HE | (uintptr_t)ref_maxC) & 3) == 0 &&
                       (!dst_f32 || ((uintptr_t)dst & 3) == 0),
                   "macenko_normalize: HE / maxC / status / the target / a float32 dst need 4-byte alignment");
    Carver c(ws, ws_bytes);
    const MkScratch s = carve_macenko(c, R, (long long)h * w);
    if (int rc = check_workspace(c, "macenko_normalize")) return rc;
    HIPT_CHECK_ARG(ws != nullptr, "macenko_normalize: workspace missing");
    float* he = HE ? HE : s.HE;
    float* mc = maxC ? maxC : s.maxC;
    int32_t* stt = status ? status : s.status;
    if (int rc = fit_launches(geometry(src, h, w, nullptr), interleaved != 0, R, (float)Io, alpha, (float)beta, s, he, mc, stt, nullptr,
                              (hipStream_t)stream))
        return rc;
    return apply_launch(geometry(src, h, w, dst), interleaved != 0, R, (float)Io, he, mc, stt, ref_HE, ref_maxC, dst, dst_f32 != 0,
                        (hipStream_t)stream);
}

extern "C" int hipt_macenko_keys(const uint8_t* src, int interleaved, int R, int h, int w, double Io, double beta, const float* aux,
                                 float* keys, uint8_t* tissue, void* stream) {
    if (int rc = check_geometry("macenko_keys", src, R, h, w, Io)) return rc;
    HIPT_CHECK_ARG(finite_host(beta) && beta >= 0.0, "macenko_keys: beta = %g is negative", beta);
    HIPT_CHECK_ARG(aux && keys && tissue, "macenko_keys: aux / keys / tissue missing");
    HIPT_CHECK_ARG((((uintptr_t)aux | (uintptr_t)keys) & 3) == 0, "macenko_keys: aux / keys need 4-byte alignment");
    const MkGeom G = geometry(src, h, w, nullptr);
    const dim3 grid((unsigned)((long long)R * G.nwg)), block(MK_THREADS);
    if (interleaved)
        hipLaunchKernelGGL(mk_keys_kernel<true>, grid, block, 0, (hipStream_t)stream, G, (float)Io, (float)beta, aux, keys, tissue);
    else
        hipLaunchKernelGGL(mk_keys_kernel<false>, grid, block, 0, (hipStream_t)stream, G, (float)Io, (float)beta, aux, keys, tissue);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
