// Shared device helpers for the gfx950 kernels (wave64, MFMA 16x16, LDS tiles of 128-byte rows): vector types and the per-type MFMA
// traits, bf16 packing and stores, the shuffle reductions and the wave scan (wave_*, quad_*, half_*), the gate's sigmoid_f / tanh_f,
// LDS-DMA and the "invisible" LDS accesses, wait_vm<N>, blend_u8, xcd_remap; then the host-side error and environment helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hipt_abmil.h"

typedef __bf16 bf16_t;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

#define LDS_AS __attribute__((address_space(3)))

// ---- per-type traits: a "chunk" is 16 bytes = one lane's MFMA operand fragment -----------
// One LDS tile row is 128 bytes = 8 chunks: 64 bf16 or 32 fp32 along K.
// mma16(acc, a, b): acc[16x16] += A'[16 x kc] * B'[16 x kc]^T where lane l supplies row (l & 15)
// of A' in `a` and row (l & 15) of B' in `b`, both for K-slot group (l >> 4).
//   bf16: one v_mfma_f32_16x16x32_bf16 (group g carries k = 8g..8g+7).
//   fp32: four v_mfma_f32_16x16x4_f32; step j uses element j of both fragments, i.e. group g
//         carries k = 4g+j.  Any K permutation is legal as long as A and B agree.
// Result layout (both): acc[i] = C[row 4*(l>>4)+i of A'-rows][col (l&15) of B'-rows].
template <typename T> struct Tr;

template <> struct Tr<float> {
    static constexpr int EPC = 4;    // elements per 16-byte chunk
    static constexpr int KB = 32;    // elements per 128-byte LDS row
    static constexpr int DT = HIPT_F32;
    static __device__ __forceinline__ void mma16(f32x4& acc, const u32x4& a, const u32x4& b) {
        // NB: bit-cast the whole vector, not a[j]: __builtin_bit_cast on a vector-element lvalue
        // reads element 0 (observed with ROCm 7.2 clang)
        const f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[j], bf[j], acc, 0, 0, 0);
    }
    static __device__ __forceinline__ float to_f(float v) { return v; }
    static __device__ __forceinline__ float from_f(float v) { return v; }
};

template <> struct Tr<bf16_t> {
    static constexpr int EPC = 8;
    static constexpr int KB = 64;
    static constexpr int DT = HIPT_BF16;
    static __device__ __forceinline__ void mma16(f32x4& acc, const u32x4& a, const u32x4& b) {
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                      __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    }
    static __device__ __forceinline__ float to_f(bf16_t v) { return (float)v; }
    static __device__ __forceinline__ bf16_t from_f(float v) { return (bf16_t)v; }
};

__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    bf16x2 p;
    p[0] = (bf16_t)lo;
    p[1] = (bf16_t)hi;
    return __builtin_bit_cast(uint32_t, p);
}

// store 4 consecutive outputs (columns n..n+3 of one row) as T
template <typename T> __device__ __forceinline__ void store4(T* p, const f32x4& v);
template <> __device__ __forceinline__ void store4<float>(float* p, const f32x4& v) { *(f32x4*)p = v; }
template <> __device__ __forceinline__ void store4<bf16_t>(bf16_t* p, const f32x4& v) {
    u32x2 o;
    o[0] = pack_bf16x2(v[0], v[1]);
    o[1] = pack_bf16x2(v[2], v[3]);
    *(u32x2*)p = o;
}

__device__ __forceinline__ float gelu_erf(float x) {  // nn.GELU() default (exact erf)
    return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
}

// ---- wave-level reductions and scans ------------------------------------------------
// THE one definition of each: the order of the xor steps is part of a kernel's bits (fp32 sums), so a kernel that needs another
// order writes it out locally and says why.  All return the result in every participating lane.  A few sites keep the steps written
// out because the call compiled to other code there (each says so); the 64-bit wave_sum sites are all among them.
// wave_sum / wave_max: all 64 lanes, xor 32, 16, 8, 4, 2, 1.
template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
// quad_sum / quad_max: across the four 16-lane groups (the lanes that share lane & 15: one row of an MFMA fragment), xor 16 then 32.
// (fp contract off in the sums: the pragma holds per function body, so a caller's own does not reach in here)
__device__ __forceinline__ float quad_sum(float v) {
#pragma clang fp contract(off)
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}
__device__ __forceinline__ float quad_max(float v) {
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    v = fmaxf(v, __shfl_xor(v, 32, 64));
    return v;
}
// half_sum / half_max: across the two 32-lane halves (32x32 MFMA fragments), xor 32.
__device__ __forceinline__ float half_sum(float v) {
#pragma clang fp contract(off)
    return v + __shfl_xor(v, 32, 64);
}
__device__ __forceinline__ float half_max(float v) { return fmaxf(v, __shfl_xor(v, 32, 64)); }
// inclusive scan over the lanes of a wave (lane = threadIdx & 63): lane l gets v_0 + .. + v_l.  T: int, unsigned.
template <typename T> __device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}

// The gate's two transcendental functions (CLAM / ABMIL forward and the training step's recomputation: the gradients are held
// against the forward's bits, so both use THESE).
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) {
    // 1 - 2/(e^{2x}+1): exact limits at +-inf, abs error ~1e-7 elsewhere
    return 1.0f - 2.0f / (expf(2.0f * x) + 1.0f);
}

// async global -> LDS, 16 bytes per lane; LDS destination = wave-uniform base + lane*16
__device__ __forceinline__ void glds16(const void* gsrc, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gsrc,
                                     (LDS_AS void*)lds_wave_base, 16, 0, 0);
}
// ---- "invisible" LDS accesses -----------------------------------------------------------------------
// While LDS-DMA (global_load_lds) is in flight, hipcc cannot prove that a C++-level LDS access does not
// alias the DMA destination and inserts s_waitcnt vmcnt(0) in front of it — draining the whole DMA ring.
// Inside ring loops every LDS access therefore goes through these helpers (the compiler sees no LDS op);
// each carries its own lgkmcnt(0), so they are for the non-hot accesses (biases, tiny exchange buffers).
__device__ __forceinline__ uint32_t lds_addr(const void* p) { return (uint32_t)(uintptr_t)(LDS_AS const char*)p; }
__device__ __forceinline__ f32x4 lds_ld128(uint32_t a) {
    f32x4 v;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
    return v;
}
__device__ __forceinline__ float lds_ld32(uint32_t a) {
    float v;
    asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
    return v;
}
__device__ __forceinline__ u32x2 lds_ld_tr64(uint32_t a) {  // ds_read_b64_tr_b16: EXEC must be all ones
    u32x2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(a) : "memory");
    return v;
}
__device__ __forceinline__ void lds_st32(uint32_t a, float v) { asm volatile("ds_write_b32 %0, %1" ::"v"(a), "v"(v) : "memory"); }
__device__ __forceinline__ void lds_st64(uint32_t a, u32x2 v) { asm volatile("ds_write_b64 %0, %1" ::"v"(a), "v"(v) : "memory"); }

// wait until at most N of this wave's vector-memory operations (loads, LDS-DMA, stores) are still in flight
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_vm0() { wait_vm<0>(); }

// The heat-maps' blend with the slide (heatmap.hip, hier_heatmap.hip): sat_u8(rint(float32(img) * a + float32(canvas) * b)),
// a = float32(alpha), b = float32(1 - alpha) -- cv2.addWeighted's formula.  Both files are built with -ffp-contract=off: the two
// products and their sum are rounded one by one.
__device__ __forceinline__ uint8_t blend_u8(uint8_t img, uint8_t canvas, float a, float b) {
    const float p = (float)img * a;
    const float q = (float)canvas * b;
    const float s = rintf(p + q);   // half to even
    return (uint8_t)fminf(fmaxf(s, 0.0f), 255.0f);
}

// XCD-aware bijective remap of a linear block id: blocks b and b+8 share an XCD (and its L2),
// so give each XCD a contiguous range of logical tiles (cdna guide T1, bijective form).
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = bid & 7, j = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
}

// host side -------------------------------------------------------------------------------
void hipt_set_error(const char* fmt, ...);

// The library reads EIGHT environment switches, all for debugging / A-B runs (README.md):
//   HIPT_GENERIC=1        every operator takes its generic kernel (no streaming / packed-weight kernels)
//   HIPT_NO_IMG=1         no activation images / head-major qkv between the streaming kernels
//   HIPT_NO_PRUNE=1       the last ViT-256 block runs in full instead of for the [CLS] rows only
//   HIPT_NO_FUSED_ATTN=1  LayerNorm-chained blocks run QKV GEMM + attention as two kernels instead of the fused one
//   HIPT_NO_PROJ_FOLD=1   the attention block's output projection runs as its own kernel instead of at the head of the fused MLP's tiles
//   HIPT_NO_CLS_ABSORB=1  the [CLS]-pruned last block projects K and V for every token (the fused kernel's CLSONLY form) instead of absorbing them
//   HIPT_NO_EMBED_LN=1    the patch embedding writes row-major tokens only; the first block applies its own LayerNorm-1 (LN-in-GEMM + two-kernel attention)
//   HIPT_BAGS_MAX_WG=n    the multi-bag CLAM tile pass launches at most n workgroups (abmil_bags.hip; the results do not depend on it)
// read per call (cheap: host side, a handful of calls per forward), so a test may flip them inside one process.
#include <stdlib.h>
inline bool hipt_env_on(const char* name) {
    const char* v = getenv(name);
    return v != nullptr && v[0] != '\0' && v[0] != '0';
}
inline bool hipt_generic_only() { return hipt_env_on("HIPT_GENERIC"); }

// In-kernel time stamps and the host code that reads them back (launch.h: StampBuffer) exist only in diagnostic builds
// (make DEBUG_STAMPS=1 -> libhipt_abmil_dbg.so).
#ifdef HIPT_DEBUG_STAMPS
#define HIPT_STAMPS_ON(ptr) ((ptr) != nullptr)
#else
#define HIPT_STAMPS_ON(ptr) false
#endif
#define HIPT_CHECK_ARG(cond, ...)                \
    do {                                         \
        if (!(cond)) {                           \
            hipt_set_error(__VA_ARGS__);         \
            return HIPT_E_BADARG;                \
        }                                        \
    } while (0)
#define HIPT_CHECK_LAUNCH()                                                        \
    do {                                                                           \
        hipError_t e__ = hipGetLastError();                                        \
        if (e__ != hipSuccess) {                                                   \
            hipt_set_error("%s:%d: %s", __FILE__, __LINE__, hipGetErrorString(e__)); \
            return HIPT_E_LAUNCH;                                                  \
        }                                                                          \
    } while (0)
