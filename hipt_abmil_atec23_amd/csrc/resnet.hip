// ResNet-50 baseline feature extractor (reference models/resnet_custom.py:ResNet_Baseline): stem conv 7x7/2 + BN + ReLU,
// maxpool 3x3/2, layer1..layer3 of Bottleneck_Baseline, global average pool -> [n, 1024] fp32.
//
// Activations are NHWC in the compute dtype T (fp32 or bf16); eval-mode BatchNorm is folded into the conv weights and a
// fp32 bias at pack time.  Every convolution is ONE implicit-GEMM kernel: M = output pixels, N = Cout, K = kh*kw*Cin in
// (ky, kx, ci) order, so that for Cin % KB == 0 (every conv but the stem) one 128-byte K slab of a row lies inside ONE
// filter tap and is a contiguous 128-byte run of the input pixel's channels (or zeros for a padding tap).  The stem
// (Cin = 3, K = 147) takes the element-gather form of the same loader, K zero-padded to the slab.
//
// Tile: BM (128; 64 on the small maps of the BasicBlock network below) output pixels x BN (128 or 64) output channels per
// 256-thread workgroup (4 waves as 2(M) x 2(N)).  Operands are
// staged global -> registers -> LDS (two buffers, one barrier per slab), with the same 16-byte-chunk XOR swizzle as
// gemm.hip; weights are the MFMA A operand so each lane ends with 4 consecutive output channels of one pixel (8/16-byte
// stores).  The epilogue is bias, optional residual add, optional ReLU, store.  No split-K and no atomics: every output
// row is computed by the same instruction sequence whatever the batch, so features do not depend on the batch.
// There are no hand-counted waits in this file (plain C++ loads and stores; the compiler places every s_waitcnt).
#include "common.h"
#include "workspace.h"

namespace {

constexpr int RN_BM = 128;
constexpr int RN_THREADS = 256;

struct ConvArgs {
    const void* x;      // [n, h, w, cin] T
    const void* wt;     // [cout, kp] T (BN folded, K zero-padded to kp)
    const float* bias;  // [cout]
    const void* resid;  // [M, cout] T or null
    void* out;          // [M, cout] T
    int n, h, w, cin, oh, ow, cout, kh, kw, stride, pad, K, kp, M, relu;
};

// BM: output pixels per tile, 128 or 64 (the ResNet-18 driver's small maps).  A 64-row tile stages half as many
// A rows per slab and gives each wave 32 rows instead of 64; the K loop, the swizzle and the column fragments are the same, so one
// output element is accumulated by the same MFMA sequence under either height.
template <typename T, int BN, bool GATHER, int BM = RN_BM>
__global__ __launch_bounds__(RN_THREADS) void rn_conv_kernel(const ConvArgs p) {
    constexpr int EPC = Tr<T>::EPC, KB = Tr<T>::KB;
    constexpr int AQ = BM / 32;       // pixel-row chunks per thread per slab
    constexpr int MFR = BM / 32;      // 16-row fragments per wave (a wave owns BM / 2 rows)
    constexpr int WQ = BN / 32;       // weight chunks per thread per slab
    constexpr int NFR = BN / 32;      // 16-column fragments per wave (a wave owns BN / 2 columns)
    constexpr int A_BYTES = BM * 128, STAGE = A_BYTES + BN * 128;
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 15, g = lane >> 4;
    const int tiles_n = p.cout / BN;
    const int tile = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (tile / tiles_n) * BM, n0 = (tile % tiles_n) * BN;

    // ---- staging slots: row (tid >> 3) + 32 q, 16-byte chunk (tid & 7) ----
    const int c = tid & 7;
    const int ohw = p.oh * p.ow;
    int iy0[AQ], ix0[AQ];
    int64_t pix0[AQ];  // element offset of image b's pixel (0, 0)
    bool mok[AQ];
#pragma unroll
    for (int q = 0; q < AQ; ++q) {
        const int m = m0 + (tid >> 3) + 32 * q;
        mok[q] = m < p.M;
        const int mm = mok[q] ? m : 0;
        const int b = mm / ohw, r = mm - b * ohw, oy = r / p.ow, ox = r - oy * p.ow;
        iy0[q] = oy * p.stride - p.pad;
        ix0[q] = ox * p.stride - p.pad;
        pix0[q] = (int64_t)b * p.h * p.w * p.cin;
    }
    const T* X = (const T*)p.x;
    const T* wrow[WQ];
#pragma unroll
    for (int q = 0; q < WQ; ++q) wrow[q] = (const T*)p.wt + (int64_t)(n0 + (tid >> 3) + 32 * q) * p.kp + c * EPC;

    u32x4 ra[AQ], rw[WQ];
    auto load = [&](int kt) {
        const int k0 = kt * KB;
        if constexpr (GATHER) {
#pragma unroll
            for (int q = 0; q < AQ; ++q) {
                T v[EPC];
#pragma unroll
                for (int e = 0; e < EPC; ++e) {
                    const int k = k0 + c * EPC + e;
                    const int tap = k / p.cin, ci = k - tap * p.cin, ky = tap / p.kw, kx = tap - ky * p.kw;
                    const int iy = iy0[q] + ky, ix = ix0[q] + kx;
                    const bool ok = mok[q] && k < p.K && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w;
                    v[e] = ok ? X[pix0[q] + ((int64_t)iy * p.w + ix) * p.cin + ci] : Tr<T>::from_f(0.0f);
                }
                ra[q] = *(const u32x4*)v;
            }
        } else {
            const int tap = k0 / p.cin, ci0 = k0 - tap * p.cin, ky = tap / p.kw, kx = tap - ky * p.kw;
#pragma unroll
            for (int q = 0; q < AQ; ++q) {
                const int iy = iy0[q] + ky, ix = ix0[q] + kx;
                const bool ok = mok[q] && iy >= 0 && iy < p.h && ix >= 0 && ix < p.w;
                ra[q] = ok ? *(const u32x4*)(X + pix0[q] + ((int64_t)iy * p.w + ix) * p.cin + ci0 + c * EPC) : u32x4{0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int q = 0; q < WQ; ++q) rw[q] = *(const u32x4*)(wrow[q] + k0);
    };
    auto store = [&](int s) {
        char* sa = smem + s * STAGE;
#pragma unroll
        for (int q = 0; q < AQ; ++q) {
            const int r = (tid >> 3) + 32 * q;
            *(u32x4*)(sa + r * 128 + ((c ^ ((r >> 1) & 7)) << 4)) = ra[q];
        }
#pragma unroll
        for (int q = 0; q < WQ; ++q) {
            const int r = (tid >> 3) + 32 * q;
            *(u32x4*)(sa + A_BYTES + r * 128 + ((c ^ ((r >> 1) & 7)) << 4)) = rw[q];
        }
    };

    int foff[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) foff[ks] = li * 128 + (((g + 4 * ks) ^ ((li >> 1) & 7)) << 4);

    f32x4 acc[MFR][NFR];
#pragma unroll
    for (int i = 0; i < MFR; ++i)
#pragma unroll
        for (int j = 0; j < NFR; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.kp / KB;
    load(0);
    store(0);
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) load(kt + 1);
        const char* sa = smem + (kt & 1) * STAGE + wm * (BM / 2) * 128;
        const char* sw = smem + (kt & 1) * STAGE + A_BYTES + wn * (BN / 2) * 128;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            u32x4 wf[NFR], af[MFR];
#pragma unroll
            for (int j = 0; j < NFR; ++j) wf[j] = *(const u32x4*)(sw + j * 16 * 128 + foff[ks]);
#pragma unroll
            for (int i = 0; i < MFR; ++i) af[i] = *(const u32x4*)(sa + i * 16 * 128 + foff[ks]);
#pragma unroll
            for (int i = 0; i < MFR; ++i)
#pragma unroll
                for (int j = 0; j < NFR; ++j) Tr<T>::mma16(acc[i][j], wf[j], af[i]);
        }
        if (kt + 1 < nk) store((kt + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue: lane holds C[pixel m0 + wm*BM/2 + 16 i + li][channel n0 + wn*BN/2 + 16 j + 4 g + 0..3] ----
    const T* R = (const T*)p.resid;
    T* O = (T*)p.out;
#pragma unroll
    for (int i = 0; i < MFR; ++i) {
        const int m = m0 + wm * (BM / 2) + i * 16 + li;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < NFR; ++j) {
            const int n = n0 + wn * (BN / 2) + j * 16 + 4 * g;
            f32x4 v = acc[i][j] + *(const f32x4*)(p.bias + n);
            const int64_t o = (int64_t)m * p.cout + n;
            if (R) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] += Tr<T>::to_f(R[o + e]);
            }
            if (p.relu) {
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = fmaxf(v[e], 0.0f);
            }
            store4<T>(O + o, v);
        }
    }
}

// BN fold + repack of one conv: w [cout, cin, kh, kw] fp32 -> [cout, kp] T in (ky, kx, ci) order, zero beyond K; bias fp32.
template <typename T>
__global__ void rn_pack_kernel(hipt_conv_bn c, int K, int kp, T* wout, float* bout) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)c.cout * kp) return;
    const int n = (int)(i / kp), k = (int)(i - (int64_t)n * kp);
    const double scale = (double)c.bn_weight[n] / sqrt((double)c.bn_var[n] + (double)c.bn_eps);
    float v = 0.0f;
    if (k < K) {
        const int tap = k / c.cin, ci = k - tap * c.cin, ky = tap / c.kw, kx = tap - ky * c.kw;
        v = (float)((double)c.weight[(((int64_t)n * c.cin + ci) * c.kh + ky) * c.kw + kx] * scale);
    }
    wout[i] = Tr<T>::from_f(v);
    if (k == 0) bout[n] = (float)((double)c.bn_bias[n] - (double)c.bn_mean[n] * scale);
}

// input -> NHWC T.  KIND 0: fp32 planar, already normalised (copied / rounded as is); 1: uint8 planar; 2: uint8 [n,h,w,3].
// uint8: ToTensor + Normalize, (float(x) / 255 - mean_c) / std_c, each operation rounded on its own (file built with
// -ffp-contract=off, IEEE division), which is what torch computes for the same bytes.
// The layout is a template parameter on purpose: with a runtime `kind` switched per channel, hipcc (ROCm 7.2, gfx950) lowered
// the interleaved case of channels 1 and 2 to a ubyte load from an address register the path never set (an illegal access).
// One straight-line kernel per layout leaves no such control flow.
struct NormArgs {
    float mean[3], std[3];
};
template <typename T, int KIND>
__global__ void rn_input_kernel(const void* x, int64_t npx, int64_t plane, NormArgs nm, T* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const int64_t b = i / plane, r = i - b * plane;
    float v[3];
    if constexpr (KIND == HIPT_RESNET_IN_F32) {
        const float* s = (const float*)x + b * 3 * plane + r;
        v[0] = s[0], v[1] = s[plane], v[2] = s[2 * plane];
    } else {
        uint8_t u[3];
        if constexpr (KIND == HIPT_RESNET_IN_U8) {
            const uint8_t* s = (const uint8_t*)x + b * 3 * plane + r;
            u[0] = s[0], u[1] = s[plane], u[2] = s[2 * plane];
        } else {
            const uint8_t* s = (const uint8_t*)x + i * 3;
            u[0] = s[0], u[1] = s[1], u[2] = s[2];
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            float f = (float)u[ch] / 255.0f;
            f = f - nm.mean[ch];
            v[ch] = f / nm.std[ch];
        }
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) out[i * 3 + ch] = Tr<T>::from_f(v[ch]);
}

template <typename T>
int launch_input(const void* x, int kind, int64_t npx, int64_t plane, const NormArgs& nm, T* out, hipStream_t st) {
    const unsigned blocks = (unsigned)((npx + 255) / 256);
    if (kind == HIPT_RESNET_IN_F32)
        hipLaunchKernelGGL((rn_input_kernel<T, HIPT_RESNET_IN_F32>), dim3(blocks), dim3(256), 0, st, x, npx, plane, nm, out);
    else if (kind == HIPT_RESNET_IN_U8)
        hipLaunchKernelGGL((rn_input_kernel<T, HIPT_RESNET_IN_U8>), dim3(blocks), dim3(256), 0, st, x, npx, plane, nm, out);
    else
        hipLaunchKernelGGL((rn_input_kernel<T, HIPT_RESNET_IN_U8_HWC>), dim3(blocks), dim3(256), 0, st, x, npx, plane, nm, out);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

// MaxPool2d(3, 2, 1) on NHWC: one thread per (output pixel, 16-byte channel chunk).  Padding taps never win (-inf).
template <typename T>
__global__ void rn_maxpool_kernel(const T* x, int n, int h, int w, int C, int oh, int ow, T* out) {
    constexpr int EPC = Tr<T>::EPC;
    const int cpp = C / EPC;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * oh * ow * cpp) return;
    const int cc = (int)(i % cpp);
    const int64_t px = i / cpp;
    const int ox = (int)(px % ow), oy = (int)((px / ow) % oh), b = (int)(px / ((int64_t)ow * oh));
    float m[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) m[e] = -INFINITY;
    for (int dy = 0; dy < 3; ++dy) {
        const int iy = oy * 2 - 1 + dy;
        if (iy < 0 || iy >= h) continue;
        for (int dx = 0; dx < 3; ++dx) {
            const int ix = ox * 2 - 1 + dx;
            if (ix < 0 || ix >= w) continue;
            const u32x4 raw = *(const u32x4*)(x + (((int64_t)b * h + iy) * w + ix) * C + cc * EPC);
            T v[EPC];
            *(u32x4*)v = raw;
#pragma unroll
            for (int e = 0; e < EPC; ++e) m[e] = fmaxf(m[e], Tr<T>::to_f(v[e]));
        }
    }
    T o[EPC];
#pragma unroll
    for (int e = 0; e < EPC; ++e) o[e] = Tr<T>::from_f(m[e]);
    *(u32x4*)(out + px * C + cc * EPC) = *(const u32x4*)o;
}

// AdaptiveAvgPool2d(1): out[b, c] = (sum over the hw pixels in pixel order, fp32) / hw.  One thread per (b, c).
template <typename T>
__global__ void rn_avgpool_kernel(const T* x, int n, int hw, int C, float* out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)n * C) return;
    const int64_t b = i / C, ch = i - b * C;
    const T* p = x + b * hw * C + ch;
    float s = 0.0f;
    for (int k = 0; k < hw; ++k) s += Tr<T>::to_f(p[(int64_t)k * C]);
    out[i] = s / (float)hw;
}

inline int esize(int dtype) { return dtype == HIPT_BF16 ? 2 : 4; }
inline int kslab(int dtype) { return dtype == HIPT_BF16 ? 64 : 32; }
inline int conv_out(int x, int k, int s, int pad) { return (x + 2 * pad - k) / s + 1; }

int conv_kp(int cin, int kh, int kw, int dtype) {
    const int K = cin * kh * kw, kb = kslab(dtype);
    return (K + kb - 1) / kb * kb;
}

template <typename T, int BN, int BM>
int launch_conv_bn(const ConvArgs& a, hipStream_t st) {
    const int tiles = ((a.M + BM - 1) / BM) * (a.cout / BN);
    if (a.cin % Tr<T>::KB == 0)
        hipLaunchKernelGGL((rn_conv_kernel<T, BN, false, BM>), dim3(tiles), dim3(RN_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((rn_conv_kernel<T, BN, true, BM>), dim3(tiles), dim3(RN_THREADS), 0, st, a);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

template <typename T, int BM>
int launch_conv(const ConvArgs& a, hipStream_t st) {
    return a.cout % 128 == 0 ? launch_conv_bn<T, 128, BM>(a, st) : launch_conv_bn<T, 64, BM>(a, st);
}

// The tile height of the ResNet-18 driver and of hipt_conv2d_ex(tile_rows = 0): a pure function of (M, cout), so a conv's launch
// shape never depends on anything but its own shape.  64 rows where 128-row tiles leave compute units idle (fewer workgroups
// than the MI355X's 256 CUs) and halving the tile adds at least one workgroup; 128 rows everywhere else.
// The 256 is a constant of this gfx950-only library, not a device query, and the rule was measured on 256 x 256 patches at
// batch 32 and 256 only: another CU count or patch size wants its own A/B.
constexpr int RN_CUS = 256;
int tile_rows_rule(int64_t M, int cout) {
    const int64_t tn = cout / (cout % 128 == 0 ? 128 : 64);
    const int64_t t128 = (M + 127) / 128, t64 = (M + 63) / 64;
    return (t128 * tn < RN_CUS && t64 > t128) ? 64 : 128;
}

// shape checks of one conv; fills the derived fields
int conv_setup(ConvArgs& a, int dtype) {
    HIPT_CHECK_ARG(dtype == HIPT_F32 || dtype == HIPT_BF16, "conv2d: bad dtype %d", dtype);
    HIPT_CHECK_ARG(a.n > 0 && a.h > 0 && a.w > 0 && a.cin > 0 && a.cout > 0 && a.kh > 0 && a.kw > 0 && a.stride > 0 && a.pad >= 0,
                   "conv2d: empty or negative shape");
    HIPT_CHECK_ARG(a.cout % 64 == 0, "conv2d: cout=%d must be a multiple of 64", a.cout);
    HIPT_CHECK_ARG(a.cin % kslab(dtype) == 0 || a.cin * a.kh * a.kw <= 1024,
                   "conv2d: cin=%d is neither a multiple of %d nor a small (K <= 1024) gathered input", a.cin, kslab(dtype));
    a.oh = conv_out(a.h, a.kh, a.stride, a.pad);
    a.ow = conv_out(a.w, a.kw, a.stride, a.pad);
    HIPT_CHECK_ARG(a.oh > 0 && a.ow > 0, "conv2d: empty output");
    const int64_t M = (int64_t)a.n * a.oh * a.ow;
    HIPT_CHECK_ARG(M < ((int64_t)1 << 31) / 2 && (int64_t)a.n * a.h * a.w * a.cin < ((int64_t)1 << 40), "conv2d: problem too large");
    a.M = (int)M;
    a.K = a.cin * a.kh * a.kw;
    a.kp = conv_kp(a.cin, a.kh, a.kw, dtype);
    HIPT_CHECK_ARG(a.x && a.wt && a.bias && a.out, "conv2d: null pointer");
    HIPT_CHECK_ARG(((uintptr_t)a.x % 16) == 0 && ((uintptr_t)a.wt % 16) == 0 && ((uintptr_t)a.out % 16) == 0 &&
                       ((uintptr_t)a.bias % 16) == 0 && ((uintptr_t)a.resid % 16) == 0,
                   "conv2d: pointers must be 16-byte aligned");
    return HIPT_OK;
}

// rows: RN_BM (every ResNet-50 launch), 64, or 0 for tile_rows_rule
int run_conv(ConvArgs& a, int dtype, hipStream_t st, int rows = RN_BM) {
    const int rc = conv_setup(a, dtype);
    if (rc != HIPT_OK) return rc;
    if (rows == 0) rows = tile_rows_rule(a.M, a.cout);
    if (rows == 64) return dtype == HIPT_BF16 ? launch_conv<bf16_t, 64>(a, st) : launch_conv<float, 64>(a, st);
    return dtype == HIPT_BF16 ? launch_conv<bf16_t, RN_BM>(a, st) : launch_conv<float, RN_BM>(a, st);
}

int run_maxpool(const void* x, int n, int h, int w, int C, void* out, int dtype, hipStream_t st) {
    const int oh = conv_out(h, 3, 2, 1), ow = conv_out(w, 3, 2, 1);
    const int64_t tot = (int64_t)n * oh * ow * (C / (16 / esize(dtype)));
    const unsigned blocks = (unsigned)((tot + 255) / 256);
    if (dtype == HIPT_BF16)
        hipLaunchKernelGGL(rn_maxpool_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)x, n, h, w, C, oh, ow, (bf16_t*)out);
    else
        hipLaunchKernelGGL(rn_maxpool_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)x, n, h, w, C, oh, ow, (float*)out);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

int run_avgpool(const void* x, int n, int hw, int C, float* out, int dtype, hipStream_t st) {
    const unsigned blocks = (unsigned)(((int64_t)n * C + 255) / 256);
    if (dtype == HIPT_BF16)
        hipLaunchKernelGGL(rn_avgpool_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)x, n, hw, C, out);
    else
        hipLaunchKernelGGL(rn_avgpool_kernel<float>, dim3(blocks), dim3(256), 0, st, (const float*)x, n, hw, C, out);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

// ---- the network ------------------------------------------------------------------------------------------------------
// Both networks (bottleneck: hipt_resnet_weights, BasicBlock: hipt_resnet_basic_weights) are ONE description, built per call in
// fixed-size arrays: the conv records in the order of the caller's convs[] (the reference's state dict: stem, then block by block)
// and the steps in launch order, each naming its activation buffers by index.  The packed image, the workspace sizes, the
// pointers and the launches all come from it; a further network (ResNet-34, -101, ...) is a builder of a few lines.
// Head and tail are fixed: input -> NHWC in T, stem conv T -> A, maxpool A -> B, the blocks, average pool of the last block output.
struct NetConv {
    int cin, cout, k, stride, pad;
};
struct Step {
    int conv, src, dst, resid, relu;  // conv record and buffers by index; resid < 0: none
};
constexpr int RN_MAX_CONVS = 1 + 3 * 4 * 64;  // 3 layers of 64 four-conv bottlenecks, or 4 layers of 64 three-conv BasicBlocks
constexpr int RN_MAX_BUFS = 5;
// A, B: block input / output, swapped block by block; T: block interior, first the NHWC copy of the input.  The buffers after
// these are the block shape's own (bottleneck: T2, D; BasicBlock: D).
enum { BUF_A, BUF_B, BUF_T };
constexpr Step RN_STEM = {0, BUF_T, BUF_A, -1, 1};

struct Net {
    const char* name;  // the prefix of this network's messages
    int dtype;
    int rows;          // tile height of every conv launch: RN_BM, or 0 for tile_rows_rule
    int grain;         // envelope: H and W multiples of this, at least 32
    int n_bufs, n_convs, n_steps;
    int cur, width;    // buffer and channels of the newest block output
    NetConv conv[RN_MAX_CONVS];
    Step step[RN_MAX_CONVS];
};

void net_init(Net& net, const char* name, int dtype, int rows, int grain, int n_bufs) {
    net.name = name, net.dtype = dtype, net.rows = rows, net.grain = grain, net.n_bufs = n_bufs;
    net.n_convs = 1, net.n_steps = 0, net.cur = BUF_B, net.width = 64;
    net.conv[0] = {3, 64, 7, 2, 3};
}
int add_conv(Net& net, NetConv c) {
    net.conv[net.n_convs] = c;
    return net.n_convs++;
}
void add_step(Net& net, Step s) { net.step[net.n_steps++] = s; }

// Bottleneck_Baseline, stride on conv2.  Records: conv1, conv2, conv3, downsample; launches: conv1, conv2, downsample, conv3.
void add_bottleneck(Net& net, int planes, int s) {
    const int in = net.width, out = planes * 4, cur = net.cur, nxt = cur ^ 1, T2 = 3, D = 4;
    const bool ds = s != 1 || in != out;  // _make_layer's rule
    const int c1 = add_conv(net, {in, planes, 1, 1, 0}), c2 = add_conv(net, {planes, planes, 3, s, 1});
    const int c3 = add_conv(net, {planes, out, 1, 1, 0});
    add_step(net, {c1, cur, BUF_T, -1, 1});
    add_step(net, {c2, BUF_T, T2, -1, 1});
    if (ds) add_step(net, {add_conv(net, {in, out, 1, s, 0}), cur, D, -1, 0});
    add_step(net, {c3, T2, nxt, ds ? D : cur, 1});
    net.cur = nxt, net.width = out;
}

// torchvision's BasicBlock, stride on conv1.  Records: conv1, conv2, downsample; launches: conv1, downsample, conv2.
void add_basic(Net& net, int planes, int s) {
    const int in = net.width, cur = net.cur, nxt = cur ^ 1, D = 3;
    const bool ds = s != 1 || in != planes;  // _make_layer's rule
    const int c1 = add_conv(net, {in, planes, 3, s, 1}), c2 = add_conv(net, {planes, planes, 3, 1, 1});
    add_step(net, {c1, cur, BUF_T, -1, 1});
    if (ds) add_step(net, {add_conv(net, {in, planes, 1, s, 0}), cur, D, -1, 0});
    add_step(net, {c2, BUF_T, nxt, ds ? D : cur, 1});
    net.cur = nxt, net.width = planes;
}

// layer L: layers[L] blocks of 64 << L planes; its first block halves the map, except in the first layer (behind the maxpool)
void add_layers(Net& net, const int* layers, int nl, void (*add_block)(Net&, int, int)) {
    for (int L = 0; L < nl; ++L)
        for (int b = 0; b < layers[L]; ++b) add_block(net, 64 << L, (L && b == 0) ? 2 : 1);
}

// the caller's conv records against the ones the layer counts imply
int check_convs(const hipt_conv_bn* convs, int n_convs, const Net& net) {
    HIPT_CHECK_ARG(n_convs == net.n_convs && convs != nullptr, "resnet: %d convs given, the layer counts need %d", n_convs, net.n_convs);
    for (int i = 0; i < net.n_convs; ++i) {
        const hipt_conv_bn& c = convs[i];
        const NetConv& e = net.conv[i];
        HIPT_CHECK_ARG(c.cin == e.cin && c.cout == e.cout && c.kh == e.k && c.kw == e.k,
                       "resnet: conv %d is %dx%dx%dx%d, expected %dx%dx%dx%d", i, c.cout, c.cin, c.kh, c.kw, e.cout, e.cin, e.k, e.k);
        HIPT_CHECK_ARG(c.weight && c.bn_weight && c.bn_bias && c.bn_mean && c.bn_var, "resnet: conv %d has a null tensor", i);
    }
    return HIPT_OK;
}

// the caller's struct, checked, as a description: 128-row tiles on every conv, H and W multiples of 16
int check_weights(const hipt_resnet_weights* w, Net& net) {
    HIPT_CHECK_ARG(w != nullptr, "resnet: null weights");
    HIPT_CHECK_ARG(w->dtype == HIPT_F32 || w->dtype == HIPT_BF16, "resnet: bad dtype %d", w->dtype);
    for (int L = 0; L < 3; ++L)
        HIPT_CHECK_ARG(w->layers[L] >= 1 && w->layers[L] <= 64, "resnet: layers[%d]=%d outside [1, 64]", L, w->layers[L]);
    net_init(net, "resnet", w->dtype, RN_BM, 16, 5);
    add_layers(net, w->layers, 3, add_bottleneck);
    return check_convs(w->convs, w->n_convs, net);
}

// the BasicBlock network (torchvision's ResNet-18 / -34 family).  layers[]: blocks of layer1..layer4; trailing zeros leave the later
// layers out (the output is the last built layer's width).  Tile height as the struct says: the rule (0) or 128 rows on every conv,
// both give the same bits.  H and W multiples of 32.
int check_basic_weights(const hipt_resnet_basic_weights* w, Net& net) {
    HIPT_CHECK_ARG(w != nullptr, "resnet_basic: null weights");
    HIPT_CHECK_ARG(w->dtype == HIPT_F32 || w->dtype == HIPT_BF16, "resnet_basic: bad dtype %d", w->dtype);
    HIPT_CHECK_ARG(w->tile_rows == 0 || w->tile_rows == RN_BM, "resnet_basic: tile_rows=%d is neither 0 (the rule) nor 128", w->tile_rows);
    int nl = 0;
    while (nl < 4 && w->layers[nl] > 0) ++nl;
    HIPT_CHECK_ARG(nl >= 1, "resnet_basic: layers[0]=%d, at least one block is needed", w->layers[0]);
    for (int L = 0; L < 4; ++L)
        HIPT_CHECK_ARG(L < nl ? w->layers[L] <= 64 : w->layers[L] == 0, "resnet_basic: layers[%d]=%d (1..64 blocks, then zeros only)", L,
                       w->layers[L]);
    net_init(net, "resnet_basic", w->dtype, w->tile_rows, 32, 4);
    add_layers(net, w->layers, nl, add_basic);
    return check_convs(w->convs, w->n_convs, net);
}

int check_shape(const Net& net, int n, int h, int w) {
    HIPT_CHECK_ARG(n >= 1 && h > 0 && w > 0, "%s: empty input n=%d h=%d w=%d", net.name, n, h, w);
    if (h % net.grain || w % net.grain || h < 32 || w < 32) {
        hipt_set_error("%s: %d x %d input outside the envelope (height and width multiples of %d, at least 32)", net.name, h, w, net.grain);
        return HIPT_E_UNSUPPORTED;
    }
    if ((int64_t)n * (h / 2) * (w / 2) >= ((int64_t)1 << 30)) {
        hipt_set_error("%s: batch of %d images of %d x %d too large for one call", net.name, n, h, w);
        return HIPT_E_UNSUPPORTED;
    }
    return HIPT_OK;
}

// the packed weight image: per conv, in the order of the caller's convs[], its packed weight | its folded fp32 bias
struct ConvImg { const void* w; const float* bias; };
void carve_packed(Carver& c, const Net& net, ConvImg* out) {
    for (int i = 0; i < net.n_convs; ++i) {
        const NetConv& e = net.conv[i];
        out[i].w = c.take((size_t)e.cout * conv_kp(e.cin, e.k, e.k, net.dtype) * esize(net.dtype));
        out[i].bias = c.take<float>(e.cout);
    }
}

// One walk over the head and the steps for n images of h x w: the map every step reads, and the bytes of every buffer.
// The workspace rule: a buffer is as large as the largest tensor the walk puts into it; a block's output counts for A and B
// alike (which of the two it lands in follows from the number of blocks before it; the size must not); no buffer is empty
// (D of a BasicBlock network of layer1 alone is never written).
struct NetPlan {
    size_t sz[RN_MAX_BUFS];
    int h[RN_MAX_CONVS], w[RN_MAX_CONVS];  // the map step i reads
    int sh, sw, oh, ow;                    // the stem's output map, the last block's
};
NetPlan plan(const Net& net, int n, int h, int w) {
    NetPlan pl;
    const size_t es = esize(net.dtype);
    int bh[RN_MAX_BUFS], bw[RN_MAX_BUFS];  // the map each buffer holds
    for (int b = 0; b < net.n_bufs; ++b) pl.sz[b] = 0;
    auto hold = [&](int b, int hh, int ww, int c) {  // buffer b now holds [n, hh, ww, c]
        bh[b] = hh, bw[b] = ww;
        const size_t bytes = (size_t)n * hh * ww * c * es;
        pl.sz[b] = pl.sz[b] > bytes ? pl.sz[b] : bytes;
        return bytes;
    };
    auto conv = [&](const Step& s) {
        const NetConv& c = net.conv[s.conv];
        return hold(s.dst, conv_out(bh[s.src], c.k, c.stride, c.pad), conv_out(bw[s.src], c.k, c.stride, c.pad), c.cout);
    };
    hold(BUF_T, h, w, net.conv[0].cin);
    conv(RN_STEM);
    pl.sh = bh[BUF_A], pl.sw = bw[BUF_A];
    hold(BUF_B, conv_out(pl.sh, 3, 2, 1), conv_out(pl.sw, 3, 2, 1), net.conv[0].cout);
    for (int i = 0; i < net.n_steps; ++i) {
        const Step& s = net.step[i];
        pl.h[i] = bh[s.src], pl.w[i] = bw[s.src];
        const size_t bytes = conv(s);
        if (s.dst <= BUF_B && pl.sz[s.dst ^ 1] < bytes) pl.sz[s.dst ^ 1] = bytes;  // A and B alike
    }
    pl.oh = bh[net.cur], pl.ow = bw[net.cur];
    for (int b = 0; b < net.n_bufs; ++b) pl.sz[b] = al256(pl.sz[b] ? pl.sz[b] : 1);  // no buffer is empty
    return pl;
}

void carve_net(Carver& c, const Net& net, const NetPlan& pl, char** buf) {
    for (int b = 0; b < net.n_bufs; ++b) buf[b] = (char*)c.take(pl.sz[b]);
}

// ---- the four entry points of a network, on its description ---------------------------------------------------------------
size_t net_packed_bytes(const Net& net) {
    ConvImg img[RN_MAX_CONVS];
    return dry_run([&](Carver& c) { carve_packed(c, net, img); });
}

int net_pack_weights(const Net& net, const hipt_conv_bn* convs, void* packed, void* stream) {
    HIPT_CHECK_ARG(packed && ((uintptr_t)packed % 256) == 0, "%s_pack_weights: packed image must be 256-byte aligned", net.name);
    ConvImg img[RN_MAX_CONVS];
    Carver c(packed);
    carve_packed(c, net, img);
    for (int i = 0; i < net.n_convs; ++i)
        if (int r = hipt_conv_bn_pack(&convs[i], net.dtype, (void*)img[i].w, (float*)img[i].bias, stream)) return r;
    return HIPT_OK;
}

size_t net_workspace_bytes(const Net& net, int n, int h, int w) {
    char* buf[RN_MAX_BUFS];
    return dry_run([&](Carver& c) { carve_net(c, net, plan(net, n, h, w), buf); });
}

int net_forward(const Net& net, const void* packed, const void* x, int input_kind, const float* norm, int n, int h, int w, float* out,
                void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_shape(net, n, h, w);
    if (rc != HIPT_OK) return rc;
    HIPT_CHECK_ARG(input_kind == HIPT_RESNET_IN_F32 || input_kind == HIPT_RESNET_IN_U8 || input_kind == HIPT_RESNET_IN_U8_HWC,
                   "%s: bad input kind %d", net.name, input_kind);
    HIPT_CHECK_ARG(packed && x && out && workspace && ((uintptr_t)packed % 256) == 0 && ((uintptr_t)workspace % 256) == 0 &&
                       ((uintptr_t)out % 16) == 0,
                   "%s: null pointer, or packed / workspace not 256-byte aligned", net.name);
    const int dt = net.dtype;
    hipStream_t st = (hipStream_t)stream;
    const NetPlan pl = plan(net, n, h, w);
    char* buf[RN_MAX_BUFS];
    Carver ws(workspace, ws_bytes);
    carve_net(ws, net, pl, buf);
    char who[32];
    snprintf(who, sizeof who, "%s_forward", net.name);
    if ((rc = check_workspace(ws, who)) != HIPT_OK) return rc;
    ConvImg img[RN_MAX_CONVS];
    Carver pk((void*)packed);
    carve_packed(pk, net, img);

    NormArgs nm = {{0.485f, 0.456f, 0.406f}, {0.229f, 0.224f, 0.225f}};
    if (norm)
        for (int c = 0; c < 3; ++c) nm.mean[c] = norm[c], nm.std[c] = norm[3 + c];
    const int64_t npx = (int64_t)n * h * w;
    rc = dt == HIPT_BF16 ? launch_input<bf16_t>(x, input_kind, npx, (int64_t)h * w, nm, (bf16_t*)buf[BUF_T], st)
                         : launch_input<float>(x, input_kind, npx, (int64_t)h * w, nm, (float*)buf[BUF_T], st);
    if (rc != HIPT_OK) return rc;
    auto conv = [&](const Step& s, int hh, int ww) -> int {
        const NetConv& c = net.conv[s.conv];
        ConvArgs a = {};
        a.x = buf[s.src], a.wt = img[s.conv].w, a.bias = img[s.conv].bias, a.resid = s.resid < 0 ? nullptr : buf[s.resid], a.out = buf[s.dst];
        a.n = n, a.h = hh, a.w = ww, a.cin = c.cin, a.cout = c.cout, a.kh = c.k, a.kw = c.k, a.stride = c.stride, a.pad = c.pad;
        a.relu = s.relu;
        return run_conv(a, dt, st, net.rows);
    };
    if ((rc = conv(RN_STEM, h, w)) != HIPT_OK) return rc;
    if ((rc = run_maxpool(buf[BUF_A], n, pl.sh, pl.sw, net.conv[0].cout, buf[BUF_B], dt, st)) != HIPT_OK) return rc;
    for (int i = 0; i < net.n_steps; ++i)
        if ((rc = conv(net.step[i], pl.h[i], pl.w[i])) != HIPT_OK) return rc;
    return run_avgpool(buf[net.cur], n, pl.oh * pl.ow, net.width, out, dt, st);
}

}  // namespace

extern "C" {

size_t hipt_conv_bn_packed_bytes(const hipt_conv_bn* c, int dtype) {
    if (!c || c->cout <= 0 || c->cin <= 0 || c->kh <= 0 || c->kw <= 0 || (dtype != HIPT_F32 && dtype != HIPT_BF16)) return 0;
    return (size_t)c->cout * conv_kp(c->cin, c->kh, c->kw, dtype) * esize(dtype);
}

int hipt_conv_bn_pack(const hipt_conv_bn* c, int dtype, void* w_out, float* bias_out, void* stream) {
    HIPT_CHECK_ARG(hipt_conv_bn_packed_bytes(c, dtype) > 0, "conv_bn_pack: bad conv shape or dtype");
    HIPT_CHECK_ARG(c->weight && c->bn_weight && c->bn_bias && c->bn_mean && c->bn_var && w_out && bias_out,
                   "conv_bn_pack: null pointer");
    const int K = c->cin * c->kh * c->kw, kp = conv_kp(c->cin, c->kh, c->kw, dtype);
    const int64_t tot = (int64_t)c->cout * kp;
    const unsigned blocks = (unsigned)((tot + 255) / 256);
    hipStream_t st = (hipStream_t)stream;
    if (dtype == HIPT_BF16)
        hipLaunchKernelGGL(rn_pack_kernel<bf16_t>, dim3(blocks), dim3(256), 0, st, *c, K, kp, (bf16_t*)w_out, bias_out);
    else
        hipLaunchKernelGGL(rn_pack_kernel<float>, dim3(blocks), dim3(256), 0, st, *c, K, kp, (float*)w_out, bias_out);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

int hipt_conv_tile_rows(int64_t m, int cout) {
    return (m > 0 && cout > 0 && cout % 64 == 0) ? tile_rows_rule(m, cout) : 0;
}

int hipt_conv2d_ex(const void* x, int n, int h, int w, int cin, const void* w_packed, const float* bias, int cout, int kh, int kw,
                   int stride, int pad, const void* resid, int relu, void* out, int dtype, int tile_rows, void* stream) {
    HIPT_CHECK_ARG(tile_rows == 0 || tile_rows == 64 || tile_rows == RN_BM, "conv2d_ex: tile_rows=%d is not 0, 64 or 128", tile_rows);
    ConvArgs a = {};
    a.x = x, a.wt = w_packed, a.bias = bias, a.resid = resid, a.out = out;
    a.n = n, a.h = h, a.w = w, a.cin = cin, a.cout = cout, a.kh = kh, a.kw = kw, a.stride = stride, a.pad = pad, a.relu = relu ? 1 : 0;
    return run_conv(a, dtype, (hipStream_t)stream, tile_rows);
}

// 128-row tiles, as every launch of the bottleneck network
int hipt_conv2d(const void* x, int n, int h, int w, int cin, const void* w_packed, const float* bias, int cout, int kh, int kw,
                int stride, int pad, const void* resid, int relu, void* out, int dtype, void* stream) {
    return hipt_conv2d_ex(x, n, h, w, cin, w_packed, bias, cout, kh, kw, stride, pad, resid, relu, out, dtype, RN_BM, stream);
}

int hipt_resnet_maxpool(const void* x, int n, int h, int w, int c, void* out, int dtype, void* stream) {
    HIPT_CHECK_ARG(x && out && n > 0 && h > 0 && w > 0 && c > 0 && (dtype == HIPT_F32 || dtype == HIPT_BF16), "resnet_maxpool: bad argument");
    HIPT_CHECK_ARG(c % (16 / esize(dtype)) == 0 && ((uintptr_t)x % 16) == 0 && ((uintptr_t)out % 16) == 0,
                   "resnet_maxpool: channels must fill 16-byte chunks, pointers 16-byte aligned");
    return run_maxpool(x, n, h, w, c, out, dtype, (hipStream_t)stream);
}

int hipt_resnet_avgpool(const void* x, int n, int hw, int c, float* out, int dtype, void* stream) {
    HIPT_CHECK_ARG(x && out && n > 0 && hw > 0 && c > 0 && (dtype == HIPT_F32 || dtype == HIPT_BF16), "resnet_avgpool: bad argument");
    return run_avgpool(x, n, hw, c, out, dtype, (hipStream_t)stream);
}

size_t hipt_resnet_packed_bytes(const hipt_resnet_weights* w) {
    Net net;
    return check_weights(w, net) == HIPT_OK ? net_packed_bytes(net) : 0;
}

int hipt_resnet_pack_weights(const hipt_resnet_weights* w, void* packed, void* stream) {
    Net net;
    const int rc = check_weights(w, net);
    return rc != HIPT_OK ? rc : net_pack_weights(net, w->convs, packed, stream);
}

size_t hipt_resnet_workspace_bytes(const hipt_resnet_weights* w, int n, int h, int wd) {
    Net net;
    return check_weights(w, net) == HIPT_OK && n >= 1 && h >= 1 && wd >= 1 ? net_workspace_bytes(net, n, h, wd) : 0;
}

int hipt_resnet_forward(const hipt_resnet_weights* w, const void* packed, const void* x, int input_kind, const float* norm,
                        int n, int h, int wd, float* out, void* workspace, size_t ws_bytes, void* stream) {
    Net net;
    const int rc = check_weights(w, net);
    return rc != HIPT_OK ? rc : net_forward(net, packed, x, input_kind, norm, n, h, wd, out, workspace, ws_bytes, stream);
}

size_t hipt_resnet_basic_packed_bytes(const hipt_resnet_basic_weights* w) {
    Net net;
    return check_basic_weights(w, net) == HIPT_OK ? net_packed_bytes(net) : 0;
}

int hipt_resnet_basic_pack_weights(const hipt_resnet_basic_weights* w, void* packed, void* stream) {
    Net net;
    const int rc = check_basic_weights(w, net);
    return rc != HIPT_OK ? rc : net_pack_weights(net, w->convs, packed, stream);
}

size_t hipt_resnet_basic_workspace_bytes(const hipt_resnet_basic_weights* w, int n, int h, int wd) {
    Net net;  // what the forward refuses has no size
    return check_basic_weights(w, net) == HIPT_OK && check_shape(net, n, h, wd) == HIPT_OK ? net_workspace_bytes(net, n, h, wd) : 0;
}

int hipt_resnet_basic_forward(const hipt_resnet_basic_weights* w, const void* packed, const void* x, int input_kind, const float* norm,
                              int n, int h, int wd, float* out, void* workspace, size_t ws_bytes, void* stream) {
    Net net;
    const int rc = check_basic_weights(w, net);
    return rc != HIPT_OK ? rc : net_forward(net, packed, x, input_kind, norm, n, h, wd, out, workspace, ws_bytes, stream);
}

}  // extern "C"
