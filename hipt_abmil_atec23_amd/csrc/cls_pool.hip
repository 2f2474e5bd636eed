// The [CLS]-pruned last ViT-256 block with the K / V projection absorbed (capi.hip, run_last_block_cls).
//
// Only token 0 of a patch asks a question in that block, so for head h, with q_h the [CLS] query (bias included) and xn_j the
// LayerNorm-1 rows of the patch (j = 0..256):
//     score_j = scale * q_h . (Wk_h xn_j + bk_h) = scale * (xn_j . u_h) + const,      u_h = Wk_h^T q_h          (384 values)
//     p       = softmax_j(scale * xn_j . u_h)                                         (the constant cancels: bk is not needed)
//     o_h     = sum_j p_j (Wv_h xn_j + bv_h)     = Wv_h z_h + bv_h,                   z_h = sum_j p_j xn_j      (384 values)
// u and o are two GEMMs over nseq rows (capi.hip, on the zero-padded per-head matrices packed below); cls_pool_kernel is what
// is left of the attention: ONE pass over the bf16 xn image with six score columns and six pooled rows per patch -- no K, no V.
//
// cls_pool_kernel.  Persistent workgroups of four waves, one patch per work unit (an eighth of the patches per XCD, round robin over
// its workgroups, as in qkv_attention.hip: a patch's bits do not depend on the grid or on the call's other patches).  The 257 rows
// of a patch are 17 blocks of 16 tokens (the last holds row 256 alone); wave w owns blocks 4w .. 4w+3, wave 0 block 16 as well.
// Per block:
//   load     the 16 rows as twelve 16-byte pieces per lane straight out of the activation image (kernels.h): lane 16g + i holds
//            row i, columns 32c + 8g .. + 7 -- the 16x16x32 MFMA operand as it is (`nt`: every row is read once); the next
//            block's pieces -- of the workgroup's next patch behind a patch's last block -- are requested before this block's
//            products, so every row is loaded exactly once.
//   scores   S[token][head] = X u^T: 12 + 12 MFMAs (u as a hi + lo bf16 pair, rows 6..15 of the head operand zero); the lane ends
//            with tokens 4g .. 4g+3 of head i -- the k order of the 16x16x16 B operand.
//   softmax  fp32, running max / sum per head (online over the wave's blocks); p rounded to bf16 as the MFMA operand, and the
//            sum taken over the rounded values.
//   pool     Z^T[column][head] += X^T P^T: the rows go through a per-wave LDS buffer ([16 tokens][800 B]) and come back token-minor
//            by ds_read_b64_tr_b16 as the A operand, 24 MFMAs of 16x16x16.  Row pitch 800 B = 32 (mod 256): the eight rows a
//            32-lane half reads land on eight distinct 32-byte bank windows.
// The four waves' (max, sum, Z) partials are merged through LDS in fixed wave order (as the fused kernel merges its [CLS]
// partials), normalised and written as bf16 z[nseq, 6, 384].  No hand-counted waits: every wait is the compiler's.
#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace {

constexpr int CP_D = 384, CP_H = 6, CP_NTOK = 257, CP_HD = CP_H * CP_D;  // 2304
constexpr int CP_WAVES = 4, CP_THREADS = CP_WAVES * 64;
constexpr int XPITCH = 800;                   // bytes per token row of a wave's transpose buffer
constexpr int XBYTES = 16 * XPITCH;           // 12 800: also holds the wave's fp32 partial [6][384] (9 216 B) at the merge
constexpr int UPITCH = 784;                   // bytes per head row of the u images (768 + 16: ds_read_b128 rows on distinct banks)
constexpr int UBYTES = CP_H * UPITCH;         // 4 704 per image (hi, lo)
constexpr int OFF_U = CP_WAVES * XBYTES;      // 51 200
constexpr int OFF_ST = OFF_U + 2 * UBYTES;    // 60 608: (max, sum) per wave and head
constexpr int CP_LDS = OFF_ST + CP_WAVES * 16 * 2 * 4;  // 61 120 B: two workgroups per CU
static_assert(CP_LDS <= 64 * 1024, "static LDS");
static_assert(CP_H * CP_D * 4 <= XBYTES, "the merge partial fits the transpose buffer");

struct ClsPoolParams {
    const bf16_t* xn;  // bf16 activation image [nseq * 257, 384]
    const float* u;    // [nseq, 6, 384] fp32
    bf16_t* z;         // [nseq, 6, 384] bf16
    int nseq;
    float scale;
    int px;      // patches per XCD: XCD x (workgroup id % 8: ids that differ by 8 share an XCD) owns patches [x px, (x + 1) px) -- the fused
    int nslots;  // attention kernel's split (qkv_attention.hip); its workgroups (slot = id / 8) take them round robin: slot, slot + nslots, ..
};

typedef LDS_AS s16x4* lds_s16x4_ptr;

__global__ __launch_bounds__(CP_THREADS, 2) void cls_pool_kernel(const ClsPoolParams p) {
    __shared__ __attribute__((aligned(16))) char smem[CP_LDS];
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, g = lane >> 4;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* const xw = smem + w * XBYTES;
    const int nblk = w == 0 ? 5 : 4;
    const bool head = li < CP_H;
    const int uoff = (head ? li : 0) * UPITCH + 16 * g;
    const int troff = (4 * g + (li >> 2)) * XPITCH + (li & 3) * 8;  // row 4g + q, columns 4p .. 4p+3 of a 16-column tile (+ 32 n)
    float* const st = (float*)(smem + OFF_ST);

    // image address of this lane's row of block kb of patch b: token 16 kb + li, clamped to the patch (block 16: row 256 for every lane)
    auto row_ptr = [&](int b, int kb) {
        int t = 16 * kb + li;
        t = t < CP_NTOK ? t : CP_NTOK - 1;
        const size_t R = (size_t)b * CP_NTOK + t;
        return (const u32x4*)(p.xn + (R >> 4) * (16 * CP_D) + (16 * g + (int)(R & 15)) * 8);
    };
    auto blk_of = [&](int i) { return i < 4 ? 4 * w + i : 16; };

    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int b0 = xcd * p.px + slot;
    const int bend = (xcd + 1) * p.px < p.nseq ? (xcd + 1) * p.px : p.nseq;
    u32x4 x[12], xnext[12];
    if (b0 < bend) {  // the first block of the first patch; every later block is requested one block ahead, across patches too
        const u32x4* src = row_ptr(b0, blk_of(0));
#pragma unroll
        for (int c = 0; c < 12; ++c) x[c] = __builtin_nontemporal_load(src + c * 64);  // + c * 512 elements
    }
    for (int b = b0; b < bend; b += p.nslots) {
        // ---- u of this patch as a hi + lo bf16 pair ----
        // (no barrier in front: the last readers of the u images -- the previous patch's scores -- passed that patch's merge barrier,
        //  and the buffers the merge reads are written again only behind the barrier below)
        for (int i = tid; i < CP_HD / 4; i += CP_THREADS) {
            const f32x4 v = *(const f32x4*)(p.u + (size_t)b * CP_HD + 4 * i);
            const int h = i / (CP_D / 4), c4 = i % (CP_D / 4);
            u32x2 hi, lo;
            float r[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) r[e] = v[e] - (float)(bf16_t)v[e];
            hi[0] = pack_bf16x2(v[0], v[1]), hi[1] = pack_bf16x2(v[2], v[3]);
            lo[0] = pack_bf16x2(r[0], r[1]), lo[1] = pack_bf16x2(r[2], r[3]);
            *(u32x2*)(smem + OFF_U + h * UPITCH + c4 * 8) = hi;
            *(u32x2*)(smem + OFF_U + UBYTES + h * UPITCH + c4 * 8) = lo;
        }
        __syncthreads();

        float m = -INFINITY, l = 0.f;
        f32x4 acc[24];
#pragma unroll
        for (int n = 0; n < 24; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < nblk; ++i) {
            const int kb = blk_of(i);
            const bool more = i + 1 < nblk;
            if (more || b + p.nslots < bend) {  // the next block of this patch, or the first one of this workgroup's next patch
                const u32x4* src = more ? row_ptr(b, blk_of(i + 1)) : row_ptr(b + p.nslots, blk_of(0));
#pragma unroll
                for (int c = 0; c < 12; ++c) xnext[c] = __builtin_nontemporal_load(src + c * 64);
            }
            // ---- scores: s[r] = token 4g + r of the block, head li ----
            f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 12; ++c) {
                u32x4 uh = *(const u32x4*)(smem + OFF_U + uoff + 64 * c);
                u32x4 ul = *(const u32x4*)(smem + OFF_U + UBYTES + uoff + 64 * c);
                if (!head) uh = u32x4{0u, 0u, 0u, 0u}, ul = u32x4{0u, 0u, 0u, 0u};
                Tr<bf16_t>::mma16(s, x[c], uh);
                Tr<bf16_t>::mma16(s, x[c], ul);
            }
            float bm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                s[r] = 16 * kb + 4 * g + r < CP_NTOK ? s[r] * p.scale : -INFINITY;
                bm = fmaxf(bm, s[r]);
            }
            bm = quad_max(bm);
            const float mn = fmaxf(m, bm);  // (finite: every block holds a valid token)
            const float alpha = __expf(m - mn);
            bf16x4 pb;
            float ps = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pb[r] = (bf16_t)__expf(s[r] - mn);
                ps += (float)pb[r];
            }
            ps = quad_sum(ps);
            l = l * alpha + ps;
            m = mn;
#pragma unroll
            for (int n = 0; n < 24; ++n) acc[n] *= alpha;
            // ---- pool: the rows through the wave's LDS buffer, back token-minor ----
#pragma unroll
            for (int c = 0; c < 12; ++c) *(u32x4*)(xw + li * XPITCH + 64 * c + 16 * g) = x[c];
            __builtin_amdgcn_wave_barrier();
            const s16x4 pbs = __builtin_bit_cast(s16x4, pb);
#pragma unroll
            for (int n = 0; n < 24; ++n) {
                const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_ptr)(xw + troff + 32 * n));
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, pbs, acc[n], 0, 0, 0);  // acc[n][r] = Z^T[column 16n + 4g + r][head li]
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int c = 0; c < 12; ++c) x[c] = xnext[c];
        }

        // ---- merge the waves' partials in wave order ----
        if (head) {
#pragma unroll
            for (int n = 0; n < 24; ++n) *(f32x4*)(xw + (li * CP_D + 16 * n + 4 * g) * 4) = acc[n];
            if (g == 0) st[w * 32 + li * 2] = m, st[w * 32 + li * 2 + 1] = l;
        }
        __syncthreads();
        for (int i = tid; i < CP_HD / 4; i += CP_THREADS) {
            const int h = i / (CP_D / 4);
            float M = st[h * 2];
#pragma unroll
            for (int v = 1; v < CP_WAVES; ++v) M = fmaxf(M, st[v * 32 + h * 2]);
            float L = 0.f;
            f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int v = 0; v < CP_WAVES; ++v) {
                const float e = __expf(st[v * 32 + h * 2] - M);
                L += st[v * 32 + h * 2 + 1] * e;
                z += *(const f32x4*)(smem + v * XBYTES + 16 * i) * e;
            }
            z *= 1.0f / L;
            store4<bf16_t>(p.z + (size_t)b * CP_HD + 4 * i, z);
        }
    }
}

// The weights of the two GEMMs around the kernel, from the K and V thirds of qkv_w [1152, 384] (bf16 values moved, none changed):
//   Wu [2304, 384]: row 384 h + c, column k = Wk[k][c] for k in head h (64 h .. 64 h + 63), else 0   -> u = q Wu^T
//   Wo [384, 2304]: row n, column 384 h + c = Wv[n][c] for n in head h, else 0                       -> o = z Wo^T + bv
// The zeros make each one launch of the row GEMM instead of six per-head ones; a zero product adds nothing to a sum.
__global__ void cls_absorb_pack_kernel(const bf16_t* __restrict__ qkv_w, bf16_t* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 2 * CP_HD * CP_D) return;
    const bf16_t zero = (bf16_t)0.0f;
    if (i < CP_HD * CP_D) {
        const int row = i / CP_D, k = i % CP_D, h = row / CP_D, c = row % CP_D;
        out[i] = k / 64 == h ? qkv_w[(size_t)(CP_D + k) * CP_D + c] : zero;
    } else {
        const int j = i - CP_HD * CP_D, n = j / CP_HD, col = j % CP_HD, h = col / CP_D, c = col % CP_D;
        out[i] = n / 64 == h ? qkv_w[(size_t)(2 * CP_D + n) * CP_D + c] : zero;
    }
}

}  // namespace

bool hipt_cls_pool_supported(int dtype, int D, int heads, int ntok) { return dtype == HIPT_BF16 && D == CP_D && heads == CP_H && ntok == CP_NTOK; }

size_t hipt_cls_absorb_packed_bytes() { return (size_t)2 * CP_HD * CP_D * sizeof(bf16_t); }

int hipt_cls_absorb_pack_launch(const void* qkv_w, void* packed, hipStream_t st) {
    const int n = 2 * CP_HD * CP_D;
    hipLaunchKernelGGL(cls_absorb_pack_kernel, dim3((n + 255) / 256), dim3(256), 0, st, (const bf16_t*)qkv_w, (bf16_t*)packed);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}

int hipt_cls_pool_launch(const void* xn_img, const float* u, void* z, int nseq, float scale, hipStream_t st) {
    HIPT_CHECK_ARG(nseq > 0 && ((int64_t)nseq * CP_NTOK) % 16 == 0, "cls_pool: nseq * 257 = %lld rows are not whole 16-row fragments", (long long)nseq * CP_NTOK);
    HIPT_CHECK_ARG(((uintptr_t)xn_img % 16) == 0 && ((uintptr_t)u % 16) == 0 && ((uintptr_t)z % 8) == 0, "cls_pool: unaligned operands");
    static DeviceSetup setup;  // (no LDS opt-in: the CU count only)
    int ncu;
    if (int rc = setup({}, 0, "cls_pool", &ncu)) return rc;
    ClsPoolParams p;
    p.xn = (const bf16_t*)xn_img; p.u = u; p.z = (bf16_t*)z; p.nseq = nseq; p.scale = scale;
    // two workgroups per CU; an eighth of the patches per XCD, as in the fused attention kernel (a patch's bits do not depend on the split)
    p.px = (nseq + 7) / 8;
    const int per_xcd = 2 * ncu / 8 > 0 ? 2 * ncu / 8 : 1;
    p.nslots = p.px < per_xcd ? p.px : per_xcd;
    hipLaunchKernelGGL(cls_pool_kernel, dim3(8 * p.nslots), dim3(CP_THREADS), 0, st, p);
    HIPT_CHECK_LAUNCH();
    return HIPT_OK;
}
