// Building blocks of the software-pipelined streaming kernels (seqgemm_pipe.hip, mlp16.hip, embed32.hip, qkv_attention.hip,
// abmil32.hip): compile-time loops, inline-asm LDS reads with counted waits; and LayerNorm into MFMA operand fragments, for them
// (ln_rows_lds) and for the LDS-ring kernels seqgemm.hip and mlp.hip (ln_rows) -- the one place either is defined.
#pragma once
#include <type_traits>

#include "common.h"

template <int I, int N, class F> __device__ __forceinline__ void sfor(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        sfor<I + 1, N>(f);
    }
}

#define DSR128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
#define DSR64(dst, addr, off) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off))
// four / eight LDS reads AND their wait in ONE statement: the outputs are valid when the statement ends, so the
// compiler may do what it likes with them (the split form -- reads, then a counted wait -- is only safe where
// nothing makes hipcc copy or re-use the destinations in between: tools/audit_asm_reads.py checks the .s)
#define DSR128X4_WAIT(d0, d1, d2, d3, addr, o0, o1, o2, o3)                                                      \
    asm volatile("ds_read_b128 %0, %4 offset:%5\n\tds_read_b128 %1, %4 offset:%6\n\tds_read_b128 %2, %4 offset:%7\n\t" \
                 "ds_read_b128 %3, %4 offset:%8\n\ts_waitcnt lgkmcnt(0)"                                           \
                 : "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3)                                                     \
                 : "v"(addr), "n"(o0), "n"(o1), "n"(o2), "n"(o3))
#define LGKM(n)                                                 \
    asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n) : "memory"); \
    __builtin_amdgcn_sched_barrier(0)

// ---- LayerNorm into MFMA operand fragments ---------------------------------------------------------------------------
// One row is held by the 4 lanes (lane>>4 = g = 0..3) that share lane&15: a lane owns the 16-byte chunks g + 4c, c < NCH (8 elements
// each, v[c][0] | v[c][1]).  Two-pass statistics (mean, centred variance) as torch; the result is packed as bf16 operand chunks.
// Every multiply-add is written out (fp contract off, in EVERY function below: the pragma holds per function body): left to hipcc,
// the unrolled instances get DIFFERENT contractions (mul+add here, fma there), i.e. a row's result would depend on which fragment
// of a tile it lands in -- the outputs must not depend on how rows are batched.
// The row length divides differently in the two forms and STAYS so: ln_rows takes a run-time K and divides (s / (float)K, correctly
// rounded), ln_rows_lds takes a compile-time D and multiplies by the rounded reciprocal (s * (1.0f / D)).  1 / 384 is not a binary fraction,
// so the product is rounded twice and differs from the quotient in the last bit for some sums: rewriting either form as the other
// changes the bits of every kernel behind it (and what each has been checked against), for no gain.
template <int NCH> __device__ __forceinline__ float ln_row_sum(const f32x4 (&v)[NCH][2]) {
#pragma clang fp contract(off)
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) s += v[c][0][e] + v[c][1][e];
    return quad_sum(s);
}
template <int NCH> __device__ __forceinline__ float ln_row_sqsum(const f32x4 (&v)[NCH][2], float mean) {
#pragma clang fp contract(off)
    float q = 0.f;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float a = v[c][0][e] - mean, b = v[c][1][e] - mean;
            q = __builtin_fmaf(a, a, q);
            q = __builtin_fmaf(b, b, q);
        }
    return quad_sum(q);
}
// one chunk: ((v - mean) * rstd) * gamma + beta, rounded to bf16
__device__ __forceinline__ u32x4 ln_chunk(const f32x4 (&v)[2], float mean, float rstd, const f32x4& g0, const f32x4& g1,
                                          const f32x4& b0, const f32x4& b1) {
#pragma clang fp contract(off)
    f32x4 y0, y1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        y0[e] = __builtin_fmaf((v[0][e] - mean) * rstd, g0[e], b0[e]);
        y1[e] = __builtin_fmaf((v[1][e] - mean) * rstd, g1[e], b1[e]);
    }
    u32x4 o;
    o[0] = pack_bf16x2(y0[0], y0[1]);
    o[1] = pack_bf16x2(y0[2], y0[3]);
    o[2] = pack_bf16x2(y1[0], y1[1]);
    o[3] = pack_bf16x2(y1[2], y1[3]);
    return o;
}

// gamma / beta in memory the compiler may read (global, or LDS outside a DMA ring): seqgemm.hip, mlp.hip.  g = lane >> 4.
template <int NCH>
__device__ __forceinline__ void ln_rows(f32x4 (&v)[NCH][2], const float* gam, const float* bet, int K, float eps, int g,
                                        u32x4 (&out)[NCH]) {
#pragma clang fp contract(off)
    const float mean = ln_row_sum<NCH>(v) / (float)K;
    const float rstd = 1.0f / sqrtf(ln_row_sqsum<NCH>(v, mean) / (float)K + eps);
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        const int k0 = (g + 4 * c) * 8;
        const f32x4 g0 = *(const f32x4*)(gam + k0), g1 = *(const f32x4*)(gam + k0 + 4);
        const f32x4 b0 = *(const f32x4*)(bet + k0), b1 = *(const f32x4*)(bet + k0 + 4);
        out[c] = ln_chunk(v[c], mean, rstd, g0, g1, b0, b1);
    }
}

// gamma / beta from LDS through asm reads with immediate offsets off ONE address register: written as C++ loads, hipcc hoists the
// 48 per-chunk addresses out of the tile loop and spills every one of them.
// gaddr = LDS byte address of gamma + 32 g;  beta sits D floats behind gamma.
template <int D, int NCH>
__device__ __forceinline__ void ln_rows_lds(f32x4 (&v)[NCH][2], uint32_t gaddr, float eps, u32x4 (&out)[NCH]) {
#pragma clang fp contract(off)
    const float mean = ln_row_sum<NCH>(v) * (1.0f / D);
    const float rstd = 1.0f / sqrtf(ln_row_sqsum<NCH>(v, mean) * (1.0f / D) + eps);
    sfor<0, NCH>([&](auto C_) __attribute__((always_inline)) {
        constexpr int c = decltype(C_)::value;
        f32x4 g0, g1, b0, b1;
        const uint32_t ga = gaddr;
        DSR128X4_WAIT(g0, g1, b0, b1, ga, c * 128, c * 128 + 16, c * 128 + D * 4, c * 128 + D * 4 + 16);
        out[c] = ln_chunk(v[c], mean, rstd, g0, g1, b0, b1);
    });
}
