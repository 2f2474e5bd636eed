// What the attention heat-map renderers share (hier_heatmap.hip, patch_heatmap.hip): a lane owns four consecutive
// pixels of a row -- 12 bytes, three whole 32-bit words -- and turns their scores into table entries, colours, the float32 blend of
// common.h and one 12-byte vector store.  The thresholded picture's rule lives here once.
// Both files are built with -ffp-contract=off (Makefile).  No inline assembly, no atomics; every store is a vector store.
#pragma once
#include "common.h"

constexpr int HH_PX = 4;   // pixels per lane

struct Words3 {
    uint32_t w[3];
};

// 12 bytes (four pixels) as three aligned words
__device__ __forceinline__ void hh_store(uint8_t* dst, const uint8_t (&o)[12]) {
    Words3 w;
#pragma unroll
    for (int k = 0; k < 3; ++k)
        w.w[k] = (uint32_t)o[4 * k] | ((uint32_t)o[4 * k + 1] << 8) | ((uint32_t)o[4 * k + 2] << 16) | ((uint32_t)o[4 * k + 3] << 24);
    *(Words3*)dst = w;
}

__device__ __forceinline__ void hh_load(const uint8_t* src, uint8_t (&o)[12]) {
    const Words3 w = *(const Words3*)src;
#pragma unroll
    for (int k = 0; k < 12; ++k) o[k] = (uint8_t)(w.w[k >> 2] >> (8 * (k & 3)));
}

// the colour table uint8 [lut_n, 3] into LDS, packed r | g << 8 | b << 16 (the caller's barrier follows)
__device__ __forceinline__ void hh_stage_lut(uint32_t* lut, const uint8_t* src, int lut_n, int t, int threads) {
    for (int e = t; e < lut_n; e += threads) lut[e] = (uint32_t)src[3 * e] | ((uint32_t)src[3 * e + 1] << 8) | ((uint32_t)src[3 * e + 2] << 16);
}

__device__ __forceinline__ int hh_entry(double score, int lut_n) {   // matplotlib's look-up of a value in [0, 1]
    const int e = (int)(score * (double)lut_n);
    return min(max(e, 0), lut_n - 1);
}

// one picture's four pixels: table entries -> colours -> blend with the base -> store
__device__ __forceinline__ void hh_paint(uint8_t* dst, const uint32_t* lut, const int (&entry)[HH_PX], const uint8_t (&base)[12], float a,
                                         float b) {
    uint8_t o[12];
#pragma unroll
    for (int k = 0; k < HH_PX; ++k) {
        const uint32_t c = lut[entry[k]];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[3 * k + ch] = blend_u8((uint8_t)(c >> (8 * ch)), base[3 * k + ch], a, b);
    }
    hh_store(dst, o);
}

// The thresholded picture's four pixels.  The reference: mask = score; mask[mask < thr] = 0; mask[mask > thr] = 0.95;
// hm = blend(cmap(mask), base); hm[mask == 0] = 0; inv = base; inv[mask == 0.95] = 0; picture = hm + inv (uint8).
// idx_hi, idx_thr: the table entries of 0.95 and of the threshold (hh_threshold_entries).
__device__ __forceinline__ void hh_paint_threshold(uint8_t* dst, const uint32_t* lut, const double (&s)[HH_PX], double thr, int idx_hi,
                                                   int idx_thr, const uint8_t (&base)[12], float a, float b) {
    uint8_t o[12];
#pragma unroll
    for (int k = 0; k < HH_PX; ++k) {
        const bool above = s[k] > thr || (s[k] == thr && thr == 0.95);   // (a score equal to a threshold of 0.95 IS the 0.95 mark)
        const bool equal = s[k] == thr && !above;
        const uint32_t c = lut[above ? idx_hi : idx_thr];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const uint8_t bl = blend_u8((uint8_t)(c >> (8 * ch)), base[3 * k + ch], a, b);
            // below: the base image; above: the blend; equal: neither half of the reference's sum is blanked -- a uint8 sum, which wraps
            o[3 * k + ch] = above ? bl : (equal ? (uint8_t)(bl + base[3 * k + ch]) : base[3 * k + ch]);
        }
    }
    hh_store(dst, o);
}

// host side: the two table entries hh_paint_threshold needs
inline void hh_threshold_entries(int lut_n, int use_threshold, double threshold, int* idx_hi, int* idx_thr) {
    *idx_hi = (int)(0.95 * (double)lut_n);
    *idx_thr = 0;
    if (use_threshold && threshold >= 0.0 && threshold <= 1.0) {   // (no score lies outside [0, 1]: nothing equals another threshold)
        const int e = (int)(threshold * (double)lut_n);
        *idx_thr = e < lut_n - 1 ? e : lut_n - 1;
    }
}
