// Geometry and scalar helpers of the fused CLAM_SB / ABMIL row tile, shared by the single-bag kernel (abmil.hip) and the ragged
// multi-bag kernel (abmil_bags.hip): the tile height, the LDS budget of one [T, S1, S2] instantiation, the swizzled h1 image and the
// gate's two transcendental functions.  Declarations only move here: both files compile them exactly as abmil.hip did on its own.
#pragma once
#include "common.h"

namespace abmil_tile {

constexpr int TM = 128;  // rows per tile

__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float tanh_f(float x) {
    // 1 - 2/(e^{2x}+1): exact limits at +-inf, abs error ~1e-7 elsewhere
    return 1.0f - 2.0f / (expf(2.0f * x) + 1.0f);
}

template <typename T, int S1, int S2> struct AG {
    static constexpr int KB = Tr<T>::KB;
    static constexpr int NSLAB = S1 / KB;             // 128-byte slabs of the h1 image
    static constexpr int NJ1 = S1 / 32;               // n-frags per wave, phase 1 (2 column waves)
    static constexpr int NJ2 = (2 * S2) / 32;         // n-frags per wave, phase 2
    static constexpr int STAGE = (TM + S1) * 128;
    static constexpr int H1_BYTES = NSLAB * TM * 128;
    static constexpr int WAB_BYTES = NSLAB * 2 * S2 * 128;
    static constexpr int AREA = (2 * STAGE > H1_BYTES + WAB_BYTES) ? 2 * STAGE : H1_BYTES + WAB_BYTES;
    static constexpr int LDS = AREA + TM * 4 * 3 + 64;  // + A_raw[128], partial[2][128], scalars
    static_assert(S1 % KB == 0 && S1 % 32 == 0 && S1 <= 128, "fused ABMIL: S1 in {32(bf16: 64),64,128}");
    static_assert((2 * S2) % 32 == 0 && 2 * S2 <= 128, "fused ABMIL: S2 in {16,32,64}");
};

// byte offset of element (row, col) inside the slab-major, swizzled A-operand image of h1
template <typename T> __device__ __forceinline__ int h1_off(int row, int col) {
    constexpr int KB = Tr<T>::KB, EPC = Tr<T>::EPC;
    const int slab = col / KB, c = (col % KB) / EPC, sub = (col % EPC) * (int)sizeof(T);
    return slab * (TM * 128) + row * 128 + ((c ^ ((row >> 1) & 7)) << 4) + sub;
}

}  // namespace abmil_tile
