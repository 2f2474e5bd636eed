// extern "C" ViT and CLAM entry points of libhipt_abmil.so (include/hipt_abmil.h): argument validation, scratch
// carving and the launch sequences.  Host code only: nothing here synchronises or allocates, so a
// caller may capture any call into a hipGraph.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "kernels.h"
#include "workspace.h"

static thread_local char g_err[512] = "";

void hipt_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

namespace {

inline int esz(int dtype) { return dtype == HIPT_F32 ? 4 : 2; }
inline hipStream_t S(void* s) { return (hipStream_t)s; }

// ---- optional per-kernel timing (bench.py's roofline leg): HIP events around every launch -----
enum { PC_EMBED, PC_LN, PC_QKV, PC_ATTN, PC_PROJ, PC_FC1, PC_FC2, PC_MLP, PC_ABMIL, PC_COMBINE, PC_OTHER, PC_VIT4K, PC_LASTCLS, PC_QKVATT, PC_CLSROWS, PC_N };
const char* const kProfNames[PC_N] = {"embed_gemm", "layernorm", "qkv_gemm", "attention", "proj_gemm",
                                      "fc1_gemm",   "fc2_gemm",  "mlp_fused",   "abmil_fused", "abmil_combine", "other",
                                      "vit4k_blocks", "last_block_cls", "qkv_attention_fused", "qkv_cls_rows"};
constexpr int kProfMax = 8192;
struct Prof {
    bool on = false, created = false;
    hipEvent_t ev[kProfMax][2];
    int cat[kProfMax];
    int n = 0;
} g_prof;

inline void prof_begin(int cat, hipStream_t st) {
    if (g_prof.on && g_prof.n < kProfMax) {
        g_prof.cat[g_prof.n] = cat;
        (void)hipEventRecord(g_prof.ev[g_prof.n][0], st);
    }
}
inline void prof_end(hipStream_t st) {
    if (g_prof.on && g_prof.n < kProfMax) {
        (void)hipEventRecord(g_prof.ev[g_prof.n][1], st);
        ++g_prof.n;
    }
}
#define PROF(cat, expr)        \
    do {                       \
        prof_begin(cat, st);   \
        rc = (expr);           \
        prof_end(st);          \
        if (rc) return rc;     \
    } while (0)

int check_vit(const hipt_vit_weights* w) {
    HIPT_CHECK_ARG(w != nullptr && w->blocks != nullptr, "vit: null weights");
    HIPT_CHECK_ARG(w->dtype == HIPT_F32 || w->dtype == HIPT_BF16, "vit: bad dtype %d", w->dtype);
    HIPT_CHECK_ARG(w->dim > 0 && w->dim % 64 == 0, "vit: dim=%d must be a multiple of 64", w->dim);
    HIPT_CHECK_ARG(w->heads > 0 && w->dim % w->heads == 0, "vit: dim %d not divisible by heads %d", w->dim, w->heads);
    const int dh = w->dim / w->heads;
    HIPT_CHECK_ARG(dh == 32 || dh == 64, "vit: head dim %d not in {32,64}", dh);
    HIPT_CHECK_ARG(w->hidden % 64 == 0, "vit: hidden=%d must be a multiple of 64", w->hidden);
    HIPT_CHECK_ARG(w->ln_eps > 0.f && w->ln_eps < 1.f, "vit: ln_eps=%g looks uninitialised", (double)w->ln_eps);
    if (w->ntok < 1 || w->ntok > 288) {
        hipt_set_error("vit: ntok=%d outside the on-chip attention envelope [1, 288]", w->ntok);
        return HIPT_E_UNSUPPORTED;
    }
    return HIPT_OK;
}

// Attention.scale (vision_transformer.py:112): qk_scale when the module was built with one, else head_dim ** -0.5
inline float attn_scale(const hipt_vit_weights* w) { return w->attn_scale > 0.f ? w->attn_scale : 1.0f / sqrtf((float)(w->dim / w->heads)); }

// ---- the scratch of a run of ViT blocks ---------------------------------------------------------------------------------------
// The tile queues of the streaming kernels, one 64-byte line each.  `aux`: the proj GEMM, or the [CLS]-row Q GEMM of the pruned block.
struct TileQueues { int mlp[16], qkv[16], aux[16]; };
struct BlockScratch {
    void *xn, *qkv, *att, *hid;  // [rows, D] | [rows, 3 D] | [rows, D] | [rows, hidden] in the compute dtype
    // borrowed from the hidden slot by the streaming routes, which never materialise the hidden tensor:
    TileQueues* queues;
    float* xc;      // [nseq, D] fp32: the compact [CLS] residual rows of the pruned last block
    void* cls_xn;   // [nseq, D] bf16: the gathered LayerNorm-1 rows of the [CLS] tokens
    void* cls_qkv;  // [nseq, 3 D] bf16 (+ 1 KiB the fused kernel's row DMA may read past the end): q | k | v of the [CLS] rows
    // borrowed from the qkv slot by the K/V-absorbed last block, behind the [nseq, D] attention rows it leaves at s.qkv itself:
    void* u;        // [nseq, heads, D] fp32
    void* z;        // [nseq, heads, D] bf16
    bool fits_xc, fits_cls_xn;  // queues + xc (+ cls_xn) lie inside the hidden slot
};

// The borrowing is legal because every route that uses a borrowed buffer runs shapes whose slot holds it:
//  - queues (192 B): the streaming routes run more than 1 088 rows of hidden >= 128 bf16 elements;
//  - cls_qkv, u, z: the fused / absorbed kernels exist for bf16, D = 384, 6 heads, 257 tokens only.  Per sequence the hidden slot is
//    257 * hidden * 2 B >= 65 792 B (hidden % 128 == 0) against 1 536 (xc) + 768 (cls_xn) + 2 304 (cls_qkv) = 4 608 B, plus under 3 KiB
//    of fixed cost (queues, the 1 KiB slack, alignment); the qkv slot is 257 * 2 304 B against 768 + 9 216 + 4 608 B;
//  - xc and cls_xn: the pruned last block takes any token count up to 320, and a model of a handful of tokens per sequence with a
//    narrow MLP does NOT leave room (hidden = 128, 3 tokens: 768 B a sequence).  fits_xc / fits_cls_xn say so and the one user,
//    vit256_range_impl, refuses such a call.
BlockScratch carve_blocks(Carver& c, const hipt_vit_weights* w, int nseq) {
    const size_t rows = (size_t)nseq * w->ntok, e = esz(w->dtype), D = w->dim, n = nseq;
    BlockScratch s;
    s.xn = c.take(rows * D * e);
    s.qkv = c.take(rows * 3 * D * e);
    s.att = c.take(rows * D * e);
    s.hid = c.take(rows * w->hidden * e);
    Carver h(s.hid, rows * w->hidden * e);
    s.queues = (TileQueues*)h.take(sizeof(TileQueues));
    s.xc = (float*)h.take(n * D * 4);
    s.fits_xc = h.ok();
    s.cls_xn = h.take(n * D * 2);
    s.fits_cls_xn = h.ok();
    s.cls_qkv = h.take(n * 3 * D * 2 + 1024);
    Carver k(s.qkv, rows * 3 * D * e);
    k.take(n * D * 2);
    s.u = k.take(n * w->heads * D * 4);
    s.z = k.take(n * w->heads * D * 2);
    return s;
}

// ---- one builder per parameter struct: a call site sets only the fields in which it differs -----------------------------------
GemmParams gemm_params(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, void* out, int64_t ldc, int M, int N, int K) {
    GemmParams p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.lda = lda; p.W = W; p.ldw = ldw; p.bias = bias; p.out = out; p.ldc = ldc; p.M = M; p.N = N; p.K = K;
    return p;
}
inline int linear(const GemmParams& p, int dtype, int flags, hipStream_t st) { return hipt_gemm_launch(p, dtype, ALOAD_PLAIN, flags, st); }

// The QKV projection of block `blk` over M rows of the residual stream x, LayerNorm-1 in the load (launch with ln = true), into s.qkv.
// qkv_from_xn(): the rows are bf16 operands another kernel already normalised instead (launch with ln = false).
SeqGemmParams qkv_params(const hipt_vit_weights* w, int blk, int M, const float* x, const BlockScratch& s) {
    const hipt_block_weights& b = w->blocks[blk];
    const int D = w->dim;
    SeqGemmParams q;
    memset(&q, 0, sizeof(q));
    q.M = M; q.K = D; q.ln_eps = w->ln_eps;
    q.A = x; q.lda = D; q.ln_w = b.ln1_w; q.ln_b = b.ln1_b; q.W = b.qkv_w; q.wpk = b.qkv_pk; q.N = 3 * D; q.bias = b.qkv_b;
    q.out = s.qkv; q.ldc = 3 * D; q.out_ntok = w->ntok;
    q.counter = s.queues->qkv;
    return q;
}
inline void qkv_from_xn(SeqGemmParams& q, const void* xn) { q.A = xn, q.ln_w = q.ln_b = nullptr; }

// The fused MLP of block `blk` over M rows of x, the attention branch's output y1 in s.xn
MlpParams mlp_params(const hipt_vit_weights* w, int blk, int M, float* x, const BlockScratch& s) {
    const hipt_block_weights& b = w->blocks[blk];
    MlpParams m;
    memset(&m, 0, sizeof(m));
    m.x = x; m.y1 = s.xn; m.bproj = b.proj_b; m.ln_w = b.ln2_w; m.ln_b = b.ln2_b; m.ln_eps = w->ln_eps;
    m.w1 = b.fc1_w; m.b1 = b.fc1_b; m.w2 = b.fc2_w; m.b2 = b.fc2_b; m.wpk = b.mlp_pk; m.wpk_fmt = b.mlp_pk_fmt; m.M = M; m.D = w->dim; m.hidden = w->hidden;
    m.counter = s.queues->mlp;
    return m;
}
// ... which also leaves LayerNorm-1 of block `next` of the rows it finishes in xn_out
inline void mlp_emit_xn(MlpParams& m, const hipt_block_weights& next, void* xn_out) { m.ln_next_w = next.ln1_w, m.ln_next_b = next.ln1_b, m.xn_out = xn_out; }

// Linears over ONE row per sequence (the [CLS] rows: M = nseq).  Up to 1 088 rows the small-M GEMM (gemm.hip: a wave per 16 x 32 output
// tile, reading the rows out of the activation image itself when a_row_step > 0), above that a gather launch (image rows only) + the
// tiled GEMM -- and BOTH walk k in the same ascending 32-element steps (GemmParams::asc), so that a sequence's bits do not depend
// on how many sequences share the call (feature_store.extract_slide gathers loader batches on that promise).
// a_row_step > 0: A is a bf16 activation image, GEMM row r its row r * a_row_step; `gather` = [M, K] scratch for the gathered rows.
int rows_linear(GemmParams p, int dtype, int flags, hipStream_t st, int a_row_step = 0, void* gather = nullptr) {
    p.asc = 1;
    if (a_row_step > 0) {
        if (!hipt_generic_only() && hipt_gemm_arows_supported(p.M, p.K, dtype, ALOAD_PLAIN, 0)) {
            p.a_row_step = a_row_step;
        } else {
            int rc = hipt_gather_cls_bf16_launch(p.A, gather, p.M, a_row_step, p.K, st, 1);
            if (rc) return rc;
            p.A = gather;
        }
    }
    return linear(p, dtype, flags, st);
}

// ---- the route of a call: decided once, here, from the model, the call's size and the environment switches --------------------
// at most four 272-row sequences: what gemm.hip's small-M kernel takes (HIPT_GENERIC keeps its meaning: the generic kernels either way)
static bool small_call(const hipt_vit_weights* w, int nseq) { return (int64_t)nseq * w->ntok <= 1088; }

// do blocks [b0, b1) of a call of nseq sequences run LayerNorm-chained on the streaming kernels?  (only those have the LayerNorm
// epilogue / prologue: every block of the range needs its packed weight images)
static bool blocks_chain(const hipt_vit_weights* w, int nseq, int b0, int b1) {
    const int D = w->dim, dt = w->dtype;
    bool chain = hipt_seqgemm_supported(dt, D) && hipt_mlp_supported(dt, D, w->hidden) && !small_call(w, nseq) && !hipt_generic_only() &&
                 hipt_mlp16_supported(dt, D, w->hidden) && hipt_seqgemm_pipe_supported(dt, D, 3 * D, false, 0);
    for (int i = b0; i < b1 && chain; ++i) chain = w->blocks[i].qkv_pk && w->blocks[i].proj_pk && w->blocks[i].mlp_pk && (w->blocks[i].mlp_pk_fmt == 2 || w->blocks[i].mlp_pk_fmt == 3);
    return chain;
}

// Last block when only the [CLS] row is consumed afterwards (ViT.forward returns norm(x)[:, 0], vision_transformer.py:248-253):
// K and V are needed for every token, everything after that only for token 0 of each sequence (run_last_block_cls)
static bool can_prune_last(const hipt_vit_weights* w) {
    return w->dtype == HIPT_BF16 && w->dim == 384 && w->dim / w->heads == 64 && w->ntok <= 320 && hipt_seqgemm_supported(w->dtype, w->dim) &&
           hipt_mlp_supported(w->dtype, w->dim, w->hidden) && !hipt_env_on("HIPT_NO_PRUNE");
}

// what the caller of run_blocks can accept
enum {
    RT_EMIT_LAST = 1,    // it runs block b1 itself and takes LayerNorm-1 of that block from the MLP of block b1 - 1 (bf16, s.att), when there is one
    RT_CLS_ONLY = 2,     // it owns x and consumes the [CLS] rows of the whole ViT only: the last block may be pruned, x may be an activation image
    RT_PX_EMBED = 4,     // its embedding is embed32.hip, which can write activation images + LayerNorm-1 of block 0
    RT_FORCE_SMALL = 8,  // the small-call kernels for ANY number of rows (hipt_vit4k_forward)
};
struct VitRoute {
    int b0, b1;        // the blocks run_blocks runs (prune: b1 = depth - 1, run_last_block_cls runs the last one)
    bool emit_last;    // RT_EMIT_LAST, or prune
    // A call of a few hundred rows (ONE 256 x 256 patch: 257; the second-level ViT of one region: 257) is latency, not throughput: the
    // A-stationary kernels would put it on two 192-row tiles, the fused MLP on seventeen 16-row tiles that each stream the whole weight
    // image (55 us a block).  Such calls take the per-operator path, whose Linears run on the small-M GEMM (gemm.hip: a wave per
    // 16 x 32 output tile, 51-204 workgroups): seven launches of a few microseconds per block.
    bool small, force_small;
    bool seq;          // bf16, D in {192, 384}: the A-stationary QKV / proj GEMMs and the fused MLP
    bool chain;        // the MLP of block i applies LayerNorm-1 of block i + 1 to the rows it finishes (bf16 operands in s.att)
    bool img;          // chained blocks exchange y1 / xn / x as activation images (kernels.h): whole 16-row fragments, no probability output
    bool hm;           // with them, q | k | v leave the QKV GEMM head-major (the attention kernel's K / V staging reads consecutive bytes)
    bool prune;        // the last block runs for the [CLS] rows only
    bool pre;          // the embedding leaves x as the fp32 activation image and LayerNorm-1 of block 0 as the bf16 image s.att (embed32.hip, LNOUT)
    bool fuse_ok, fold_ok, absorb_ok;  // the model-wide part of block_route()
    // running state of the call
    bool have_xn = false;  // s.att holds LayerNorm-1 of the next block to run
    bool x_img = false;    // x (and s.att with it) is an activation image
};

VitRoute vit_route(const hipt_vit_weights* w, int nseq, int b0, int b1, bool want_probs, int accept) {
    const int D = w->dim, dt = w->dtype;
    const int64_t M = (int64_t)nseq * w->ntok;
    VitRoute r;
    r.force_small = (accept & RT_FORCE_SMALL) != 0;
    r.small = small_call(w, nseq) || r.force_small;
    r.prune = (accept & RT_CLS_ONLY) && can_prune_last(w) && !small_call(w, nseq);
    r.b0 = b0;
    r.b1 = r.prune ? w->depth - 1 : b1;
    r.emit_last = r.prune || (accept & RT_EMIT_LAST);
    r.seq = hipt_seqgemm_supported(dt, D) && hipt_mlp_supported(dt, D, w->hidden) && !r.small;
    r.chain = !r.force_small && blocks_chain(w, nseq, r.b0, r.b1);
    r.img = r.chain && r.prune && !want_probs && M % 16 == 0 && !hipt_env_on("HIPT_NO_IMG") && hipt_attention64_supported(dt, D / w->heads, w->ntok, false);
    r.hm = r.img && M * 3 * D * 2 < ((int64_t)1 << 32) - 65536;
    r.pre = r.img && (accept & RT_PX_EMBED) && r.b0 < r.b1 && !hipt_env_on("HIPT_NO_EMBED_LN");
    r.fuse_ok = hipt_qkv_attn_supported(dt, D, w->heads, w->ntok) && !hipt_env_on("HIPT_NO_FUSED_ATTN");
    r.fold_ok = r.chain && !hipt_env_on("HIPT_NO_PROJ_FOLD");
    r.absorb_ok = hipt_cls_pool_supported(dt, D, w->heads, w->ntok) && !hipt_env_on("HIPT_NO_CLS_ABSORB");
    return r;
}

struct BlockRoute {
    // LayerNorm-chained block with activation images: the QKV projection runs inside the attention kernel (qkv_attention.hip),
    // q | k | v never reach HBM.  The [CLS] rows (257 = 8 x 32 + 1) get their q | k | v from a side GEMM over nseq rows.
    bool fuse;
    // MLP image format 3: the output projection runs at the head of the fused MLP's tiles (mlp16.hip, FOLD) -- no proj launch, no y1
    bool fold;
    // (pruned last block) K / V projection absorbed (cls_pool.hip): with one query per (patch, head) the scores are xn . u, u_h = Wk_h^T q_h, and
    // the output is Wv_h z_h + bv_h, z_h the softmax-pooled xn rows.  The two per-head products run as row GEMMs on the zero-padded
    // matrices behind the block's fused-attention image (b.cls_absorb).
    bool absorb;
};
BlockRoute block_route(const VitRoute& r, const hipt_block_weights& b, bool last_probs) {
    BlockRoute k;
    k.fuse = r.have_xn && r.x_img && b.qkv_att_pk && r.fuse_ok && !last_probs;
    k.fold = r.fold_ok && b.mlp_pk_fmt == 3 && !last_probs;
    k.absorb = k.fuse && b.cls_absorb == HIPT_CLS_ABSORB_TAIL && r.absorb_ok;
    return k;
}

// the side GEMM of the fused attention kernels: q | k | v (N = 3 D) or q alone (N = D) of the [CLS] rows, whose LayerNorm-1 rows are
// row r * a_row_step of the image s.att (a_row_step > 0) or the gathered rows s.cls_xn
int cls_rows_qkv(const hipt_vit_weights* w, const hipt_block_weights& b, int nseq, int N, const BlockScratch& s, int a_row_step, hipStream_t st) {
    const int D = w->dim;
    return rows_linear(gemm_params(a_row_step > 0 ? s.att : s.cls_xn, D, b.qkv_w, D, b.qkv_b, s.cls_qkv, N, nseq, N, D), w->dtype, 0, st, a_row_step, s.cls_xn);
}

// Blocks [r.b0, r.b1) over the nseq sequences of x; probs != null: the attention map of block b1 - 1, after which that block stops.
int run_blocks(const hipt_vit_weights* w, float* x, int nseq, float* probs, const BlockScratch& s, VitRoute& r, hipStream_t st) {
    const int D = w->dim, M = nseq * w->ntok, dt = w->dtype, dh = D / w->heads;
    const float scale = attn_scale(w);
    int rc;
    // timing categories: the kernels of the small second-level ViT (D = 192, a few hundred rows) are booked together,
    // so that the per-kernel categories hold only the ViT-256 launches the roofline is computed on
    const bool big = D >= 384;
    const int cQKV = big ? PC_QKV : PC_VIT4K, cATTN = big ? PC_ATTN : PC_VIT4K, cPROJ = big ? PC_PROJ : PC_VIT4K, cMLP = big ? PC_MLP : PC_VIT4K;
    r.have_xn = r.x_img = r.pre;
    // the tile queues of the streaming kernels reset themselves at the end of a launch:
    // zeroed once here instead of before each of the ~44 launches (5 us each on the stream: 3 % of a one-region forward)
    const int qz = r.chain && hipMemsetAsync(s.queues, 0, sizeof(TileQueues), st) == hipSuccess ? 1 : 0;
    for (int i = r.b0; i < r.b1; ++i) {
        const hipt_block_weights& b = w->blocks[i];
        const bool last_probs = probs != nullptr && i == r.b1 - 1;
        if (r.seq) {
            // bf16, D in {192,384}: A-stationary kernels.  QKV with LayerNorm-1 fused into the activation
            // load; proj leaves the attention-branch output y1 in bf16 (s.xn); the fused MLP kernel folds
            // y1 in, does LN2 + fc1 + GELU + fc2 with the hidden tensor on chip and updates x in place.
            const BlockRoute k = block_route(r, b, last_probs);
            SeqGemmParams q = qkv_params(w, i, M, x, s);
            q.counter_zeroed = qz;
            // Where the attention output goes.  Fused kernel: the (unused) qkv slot.  Two kernels: s.att -- except under the fold, where the
            // MLP kernel reads the attention rows as y1 AND writes the next block's LayerNorm-1 rows to s.att in the same launch: the y1 slot
            // s.xn is free then (no proj launch writes it), so the two never share a buffer.  (The kernel itself would tolerate the alias -- a
            // workgroup loads all attention rows of its tile before it stores any, tiles own disjoint rows: mlp16.hip, "in place" -- but
            // nothing in a launch sequence should rest on that.)
            void* att_two = k.fold ? s.xn : s.att;
            const void* att_out = k.fuse ? s.qkv : att_two;
            if (k.fuse) {
                // (nseq rows are a handful of the streaming kernel's 192-row tiles -- 11 CUs for 2 048 patches; the generic GEMM tiles N as well.
                //  Up to 1 088 sequences the small-M GEMM reads the [CLS] rows out of the image itself: one launch, not two)
                PROF(PC_CLSROWS, cls_rows_qkv(w, b, nseq, 3 * D, s, w->ntok, st));
                PROF(PC_QKVATT, hipt_qkv_attn_launch(s.att, b.qkv_att_pk, b.qkv_b, s.cls_qkv, s.qkv, nseq, scale, st));
            } else {
                if (r.have_xn) qkv_from_xn(q, s.att);  // LayerNorm-1 already applied by the previous block's MLP epilogue
                q.img = (r.have_xn && r.img ? 1 : 0) | (r.hm ? 4 : 0);
                PROF(cQKV, hipt_seqgemm_launch(q, !r.have_xn, 0, st));
                // (with activation images the attention output is one too: proj then reads its operands 1 KiB at a time)
                PROF(cATTN, hipt_attention_launch(s.qkv, att_two, last_probs ? probs : nullptr, nseq, w->ntok, w->heads, dh, scale, dt, st, r.img ? 1 : 0, r.hm ? 1 : 0));
            }
            if (last_probs) break;
            if (!k.fold) {
                qkv_from_xn(q, att_out);
                q.W = b.proj_w; q.wpk = b.proj_pk; q.N = D; q.bias = b.proj_b; q.out = s.xn; q.ldc = D;
                q.counter = s.queues->aux;
                q.img = r.img ? 3 : 0;  // A = the attention output image, out = y1 image
                PROF(cPROJ, hipt_seqgemm_launch(q, false, 0, st));
            }
            MlpParams m = mlp_params(w, i, M, x, s);
            if (k.fold) m.y1 = att_out;
            m.fold = k.fold ? 1 : 0;
            m.counter_zeroed = qz;
            r.have_xn = r.chain && (i + 1 < r.b1 || r.emit_last) && i + 1 < w->depth;
            if (r.have_xn) mlp_emit_xn(m, w->blocks[i + 1], s.att);
            if (r.img) {
                m.img = r.x_img ? 3 : 1;
                r.x_img = true;
            }
            PROF(cMLP, hipt_mlp_launch(m, st));
            continue;
        }
        // (small calls: both LayerNorms run in the prologue of the GEMM that consumes them -- five launches a block instead of seven)
        // (the kernel loads gamma / beta 16 bytes at a time: parameters that are views into a flat buffer off that grid keep the
        //  separate LayerNorm launch, which has no alignment requirement)
        const bool ln_al = (((uintptr_t)b.ln1_w | (uintptr_t)b.ln1_b | (uintptr_t)b.ln2_w | (uintptr_t)b.ln2_b) & 15) == 0;
        const bool ln_in_gemm = r.small && ln_al && !hipt_generic_only() && hipt_gemm_ln_supported(M, D, ALOAD_PLAIN, 0, r.force_small);
        // a Linear of this path: one M tile per sequence, a residual update of x under HIPT_EPI_RESID
        auto lin = [&](int cat, GemmParams g, int flags) -> int {
            g.rpt = w->ntok;
            g.small_any = r.force_small ? 1 : 0;
            if (flags & HIPT_EPI_RESID) g.resid = x;
            PROF(cat, linear(g, dt, flags, st));
            return HIPT_OK;
        };
        // the same over LayerNorm(x; lw, lb): in the GEMM's prologue (g.A = x), or by a launch of its own into s.xn
        auto ln_lin = [&](int cat, const float* lw, const float* lb, GemmParams g, int flags) -> int {
            if (ln_in_gemm) {
                g.ln_w = lw; g.ln_b = lb; g.ln_eps = w->ln_eps;
            } else {
                PROF(PC_LN, hipt_layernorm_launch(x, D, lw, lb, s.xn, dt, D, M, D, w->ln_eps, st));
                g.A = s.xn;
            }
            return lin(cat, g, flags);
        };
        const int H = w->hidden;
        if ((rc = ln_lin(PC_QKV, b.ln1_w, b.ln1_b, gemm_params(x, D, b.qkv_w, D, b.qkv_b, s.qkv, 3 * D, M, 3 * D, D), 0))) return rc;
        PROF(PC_ATTN, hipt_attention_launch(s.qkv, s.att, last_probs ? probs : nullptr, nseq, w->ntok, w->heads, dh, scale, dt, st));
        if (last_probs) break;  // Block.forward(return_attention=True) returns before the residual (:148-149)
        if ((rc = lin(PC_PROJ, gemm_params(s.att, D, b.proj_w, D, b.proj_b, x, D, M, D, D), HIPT_EPI_RESID | HIPT_EPI_OUT_F32))) return rc;
        if ((rc = ln_lin(PC_FC1, b.ln2_w, b.ln2_b, gemm_params(x, D, b.fc1_w, D, b.fc1_b, s.hid, H, M, H, D), HIPT_EPI_GELU))) return rc;
        if ((rc = lin(PC_FC2, gemm_params(s.hid, H, b.fc2_w, H, b.fc2_b, x, D, M, D, H), HIPT_EPI_RESID | HIPT_EPI_OUT_F32))) return rc;
    }
    return HIPT_OK;
}

// Last block when only the [CLS] row is consumed afterwards (VitRoute::prune): the attention of one query per (sequence, head), then
// proj / residual / MLP on nseq rows instead of nseq * ntok (allowed, and the pruned FLOP figure is the one the
// roofline uses).  Leaves the final residual rows compact in s.xc [nseq, D].
// (its [CLS]-row launches are booked apart: the per-kernel categories then hold full-size launches only)
static int run_last_block_cls(const hipt_vit_weights* w, float* x, int nseq, const BlockScratch& s, const VitRoute& r, hipStream_t st) {
    const int D = w->dim, M = nseq * w->ntok, dt = w->dtype, last = w->depth - 1;
    const hipt_block_weights& b = w->blocks[last];
    const float scale = attn_scale(w);
    const BlockRoute k = block_route(r, b, false);
    int rc;
    const void* att_rows = s.att;  // [nseq, D] bf16: the attention output of the [CLS] tokens
    if (k.fuse) {
        // The fused kernel's [CLS]-only form: K and V of every token are computed per (patch, head) and consumed in place by the one
        // query of the patch; q | k | v of the [CLS] rows themselves from the side GEMM, as in the other blocks.  Output: the
        // attention rows of the [CLS] tokens, compact, in the (unused) qkv slot.
        PROF(PC_LASTCLS, hipt_gather_cls_bf16_launch(s.att, s.cls_xn, nseq, w->ntok, D, st, 1));
        if (k.absorb) {
            // Q rows, u, ONE streaming pass over the xn image, o.  The same kernels whatever the call's size or company: rows_linear is
            // row independent bit for bit, a patch is one work unit.
            const int HD = w->heads * D;
            const char* wu = (const char*)b.qkv_att_pk + hipt_qkv_attn_packed_bytes();
            const char* wo = wu + (size_t)HD * D * 2;
            PROF(PC_LASTCLS, cls_rows_qkv(w, b, nseq, D, s, 0, st));
            PROF(PC_LASTCLS, rows_linear(gemm_params(s.cls_qkv, D, wu, D, nullptr, s.u, HD, nseq, HD, D), dt, HIPT_EPI_OUT_F32, st));
            PROF(PC_LASTCLS, hipt_cls_pool_launch(s.att, (const float*)s.u, s.z, nseq, scale, st));
            PROF(PC_LASTCLS, rows_linear(gemm_params(s.z, HD, wo, HD, b.qkv_b + 2 * D, s.qkv, D, nseq, D, HD), dt, 0, st));
        } else {
            PROF(PC_LASTCLS, cls_rows_qkv(w, b, nseq, 3 * D, s, 0, st));
            PROF(PC_LASTCLS, hipt_qkv_attn_cls_launch(s.att, b.qkv_att_pk, b.qkv_b, s.cls_qkv, s.qkv, nseq, scale, st));
        }
        att_rows = s.qkv;
    } else {
        SeqGemmParams q = qkv_params(w, last, M, x, s);
        if (r.have_xn) {  // LayerNorm-1 already applied by the previous block's MLP epilogue (bf16 operands in s.att)
            // Only token 0 of a sequence asks a question in this block: K and V for every row (columns 384.. of the QKV Linear: the
            // weight image of an N tile is the 98 304 bytes of its rows, so the tail of the image IS the [K; V] matrix), Q for the
            // [CLS] rows alone -- their operands gathered into the free hidden slot, a [nseq, 384] GEMM scattered to rows s * ntok
            PROF(PC_LASTCLS, hipt_gather_cls_bf16_launch(s.att, s.cls_xn, nseq, w->ntok, D, st, r.x_img ? 1 : 0));
            const size_t wq = (size_t)D * D * 2;
            qkv_from_xn(q, s.att);
            q.img = r.x_img ? 1 : 0;  // (x and the operands s.att change layout together)
            q.W = (const char*)b.qkv_w + wq; q.wpk = b.qkv_pk ? (const char*)b.qkv_pk + wq : nullptr; q.N = 2 * D; q.bias = b.qkv_b + D;
            q.out = (bf16_t*)s.qkv + D;
            PROF(PC_LASTCLS, hipt_seqgemm_launch(q, false, 0, st));
            q.img = 0;
            q.M = nseq; q.A = s.cls_xn; q.W = b.qkv_w; q.wpk = b.qkv_pk; q.N = D; q.bias = b.qkv_b; q.out = s.qkv; q.ldc = w->ntok * 3 * D;
            q.counter = s.queues->aux;
            PROF(PC_LASTCLS, hipt_seqgemm_launch(q, false, 0, st));
        } else {
            PROF(PC_QKV, hipt_seqgemm_launch(q, true, 0, st));
        }
        PROF(PC_LASTCLS, hipt_attn_cls_launch(s.qkv, s.att, nullptr, nseq, w->ntok, w->heads, D / w->heads, scale, st));
    }
    PROF(PC_OTHER, hipt_gather_cls_launch(x, s.xc, nseq, (int64_t)w->ntok * D, D, st, r.x_img ? 1 : 0));
    // (nseq rows: the generic GEMM tiles N as well -- see the side GEMM of the fused blocks)
    PROF(PC_LASTCLS, rows_linear(gemm_params(att_rows, D, b.proj_w, D, b.proj_b, s.xn, D, nseq, D, D), dt, 0, st));
    PROF(PC_LASTCLS, hipt_mlp_launch(mlp_params(w, last, nseq, s.xc, s), st));
    return HIPT_OK;
}

int64_t image_elems(const hipt_image_layout* lay, int nseq_total) {
    const int per = lay->grid_w * lay->grid_h;
    return (int64_t)((nseq_total + per - 1) / per) * lay->batch_stride;
}

// input image kinds: fp32 [.., 3, W, H], or uint8 in the same layout / interleaved [.., W, H, 3] (normalised on device)
enum { IMG_F32 = 0, IMG_U8_CHW = 1, IMG_U8_HWC = 2 };

// the image tensor in the compute dtype: bf16 mode holds a bf16 image, fp32 mode an fp32 one for uint8 input, and none where fp32
// input is used where it lies
size_t image_compute_bytes(const hipt_vit_weights* w, const hipt_image_layout* lay, int nseq, int kind) {
    const size_t n = (size_t)image_elems(lay, nseq);
    return w->dtype == HIPT_BF16 ? al256(n * 2) : kind != IMG_F32 ? al256(n * 4) : 0;
}

// tokens of sequences [seq0, seq0+nseq) from an image tensor already in the compute dtype
int embed256(const hipt_vit_weights* w, const void* img, const hipt_image_layout* lay, int seq0, int nseq, float* x,
             hipStream_t st) {
    HIPT_CHECK_ARG(lay->patch_h % 16 == 0 && lay->patch_w % 16 == 0, "vit256: patch %dx%d not a multiple of 16", lay->patch_h,
                   lay->patch_w);
    const int nty = lay->patch_h / 16, ntx = lay->patch_w / 16;
    HIPT_CHECK_ARG(nty * ntx + 1 == w->ntok, "vit256: image gives %d tokens, weights expect %d", nty * ntx + 1, w->ntok);
    HIPT_CHECK_ARG(w->embed_k == 768, "vit256: embed_k must be 768 (3x16x16)");
    GemmParams p = gemm_params(img, 0, w->embed_w, w->embed_k, w->embed_b, x, w->dim, nseq * nty * ntx, w->dim, w->embed_k);
    p.pos = w->pos;
    p.rows_per_seq = p.rpt = nty * ntx;
    p.im = *lay; p.im_nty = nty; p.im_ntx = ntx; p.im_seq0 = seq0;
    int rc;
    PROF(PC_EMBED, hipt_gemm_launch(p, w->dtype, ALOAD_IM2COL, HIPT_EPI_OUT_F32 | EPI_ROWMAP, st));
    PROF(PC_OTHER, hipt_cls_init_launch(x, w->cls, w->pos, nseq, w->ntok, w->dim, st));
    return HIPT_OK;
}

// may the embedding read fp32 pixels itself (embed32.hip)?  `slot` bytes are available for its packed weight + tile queue
static bool embed_fused_ok(const hipt_vit_weights* w, const void* images, const hipt_image_layout* lay, size_t slot, int kind = IMG_F32) {
    // (uint8: 8-byte pixel runs; interleaved tensors are whole [n, W, H, 3] images: batch_stride = 3 * chan_stride)
    if (kind != IMG_F32 && (lay->row_stride % 8 != 0 || lay->chan_stride % 8 != 0 || lay->batch_stride != 3 * lay->chan_stride))
        return false;
    return lay->patch_w % 16 == 0 && lay->patch_h % 16 == 0 &&
           hipt_embed32_supported(w->dtype, w->dim, w->embed_k, lay->patch_h / 16, lay->patch_w / 16) &&
           w->ntok == (lay->patch_h / 16) * (lay->patch_w / 16) + 1 && slot >= hipt_embed32_packed_bytes() + 256 && ((uintptr_t)images % 16) == 0 &&
           lay->row_stride % 4 == 0 && lay->chan_stride % 4 == 0 && lay->batch_stride % 4 == 0;
}

// the same from the fp32 / uint8 image itself (embed32.hip): `wpk` = the packed Conv2d weight with the kernel's tile queue behind it
// xn_img != null: x leaves as the fp32 activation image and LayerNorm-1 of the first block as the bf16 image xn_img (VitRoute::pre)
int embed256_px(const hipt_vit_weights* w, const void* img, int kind, const hipt_image_layout* lay, int seq0, int nseq, float* x, const void* wpk,
                void* xn_img, hipStream_t st) {
    EmbedParams p;
    memset(&p, 0, sizeof(p));
    p.img = img; p.kind = kind; p.im = *lay; p.nty = lay->patch_h / 16; p.ntx = lay->patch_w / 16; p.seq0 = seq0; p.nseq = nseq;
    p.wpk = wpk; p.bias = w->embed_b; p.pos = w->pos; p.x = x; p.ntok = w->ntok;
    p.counter = (int*)((char*)wpk + hipt_embed32_packed_bytes());
    if (xn_img) {
        p.xn_out = xn_img; p.ln_w = w->blocks[0].ln1_w; p.ln_b = w->blocks[0].ln1_b; p.ln_eps = w->ln_eps;
    }
    int rc;
    PROF(PC_EMBED, hipt_embed32_launch(p, st));
    if (xn_img)
        PROF(PC_OTHER, hipt_cls_init_img_launch(x, xn_img, w->cls, w->pos, p.ln_w, p.ln_b, p.ln_eps, nseq, w->ntok, w->dim, st));
    else
        PROF(PC_OTHER, hipt_cls_init_launch(x, w->cls, w->pos, nseq, w->ntok, w->dim, st));
    return HIPT_OK;
}

int embed4k(const hipt_vit_weights* w, const void* tokens, int nseq, float* x, hipStream_t st, int small_any = 0) {
    const int K = w->embed_k;
    GemmParams p = gemm_params(tokens, K, w->embed_w, K, w->embed_b, x, w->dim, nseq * (w->ntok - 1), w->dim, K);
    p.small_any = small_any;
    p.pos = w->pos;
    p.rows_per_seq = p.rpt = w->ntok - 1;
    int rc = HIPT_OK;
    if (p.M > 0) PROF(PC_EMBED, hipt_gemm_launch(p, w->dtype, ALOAD_PLAIN, HIPT_EPI_GELU | HIPT_EPI_OUT_F32 | EPI_ROWMAP, st));
    PROF(PC_OTHER, hipt_cls_init_launch(x, w->cls, w->pos, nseq, w->ntok, w->dim, st));
    return HIPT_OK;
}

// ---- the workspaces of the forwards ---------------------------------------------------------------------------------------------
// ViT-4K forward: the residual stream (with_x) | block scratch | the bf16 copy of the input tokens (the only extra of the prepare_tokens calls)
struct Vit4kWs { float* x; BlockScratch s; void* tok; };
Vit4kWs carve_vit4k(Carver& c, const hipt_vit_weights* w, int nseq, bool with_x) {
    Vit4kWs k;
    k.x = with_x ? (float*)c.take((size_t)nseq * w->ntok * w->dim * 4) : nullptr;
    k.s = carve_blocks(c, w, nseq);
    k.tok = c.take((size_t)nseq * w->ntok * w->embed_k * 2);
    return k;
}

// ViT-256 over a range of sequences, `chunk` at a time (<= 0: 2 048): the residual stream of one chunk + its block scratch
struct RangeWs { int chunk; float* x; BlockScratch s; };
int default_chunk(int nseq) { return nseq < 2048 ? nseq : 2048; }
RangeWs carve_range(Carver& c, const hipt_vit_weights* w, int nseq, int chunk) {
    RangeWs g;
    if (chunk <= 0) chunk = default_chunk(nseq);
    g.chunk = chunk < nseq ? chunk : nseq;
    g.x = (float*)c.take((size_t)g.chunk * w->ntok * w->dim * 4);
    g.s = carve_blocks(c, w, g.chunk);
    return g;
}

// ... behind it one slot of `nslot` bytes: the image in the compute dtype, or the pixel-reading embedding's packed weight + tile queue
struct Vit256Ws { void *range, *slot; size_t nrange, nslot; };
Vit256Ws carve_vit256(Carver& c, const hipt_vit_weights* w, int nseq, int chunk, size_t nslot) {
    Vit256Ws v;
    v.nrange = dry_run([&](Carver& d) { carve_range(d, w, nseq, chunk); });
    v.nslot = al256(nslot);
    v.range = c.take(v.nrange);
    v.slot = c.take(v.nslot);
    return v;
}
inline size_t embed_px_slot_bytes() { return hipt_embed32_packed_bytes() + 256; }

static hipt_image_layout region_layout(int W, int H) {
    hipt_image_layout lay;
    lay.grid_w = W / 256;
    lay.grid_h = H / 256;
    lay.patch_h = lay.patch_w = 256;
    lay.row_stride = H;
    lay.chan_stride = (int64_t)W * H;
    lay.batch_stride = 3 * lay.chan_stride;
    return lay;
}

// HIPT_4K over nreg regions of w_256 x h_256 patches: the [CLS] grid of the first level | ViT-256 forward | ViT-4K forward
struct Hipt4kWs { float* cls; void *ws256, *ws4k; size_t n256, n4k; };
Hipt4kWs carve_hipt4k(Carver& c, const hipt_vit_weights* w256, const hipt_vit_weights* w4k, int nreg, int w_256, int h_256, int chunk, int kind) {
    const hipt_image_layout lay = region_layout(w_256 * 256, h_256 * 256);
    const int nseq = nreg * w_256 * h_256;
    Hipt4kWs h;
    h.n256 = dry_run([&](Carver& d) { carve_vit256(d, w256, nseq, chunk, image_compute_bytes(w256, &lay, nseq, kind)); });
    h.n4k = dry_run([&](Carver& d) { carve_vit4k(d, w4k, nreg, true); });
    h.cls = (float*)c.take((size_t)nseq * w256->dim * 4);
    h.ws256 = c.take(h.n256);
    h.ws4k = c.take(h.n4k);
    return h;
}

}  // namespace

extern "C" {

int hipt_abi_version(void) { return HIPT_ABI_VERSION; }

int hipt_profile_enable(int on) {
    if (on && !g_prof.created) {
        for (int i = 0; i < kProfMax; ++i)
            for (int j = 0; j < 2; ++j)
                if (hipEventCreate(&g_prof.ev[i][j]) != hipSuccess) {
                    hipt_set_error("profile: hipEventCreate failed");
                    return HIPT_E_LAUNCH;
                }
        g_prof.created = true;
    }
    g_prof.on = on != 0;
    g_prof.n = 0;
    return HIPT_OK;
}
int hipt_profile_categories(void) { return PC_N; }
const char* hipt_profile_category_name(int i) { return (i >= 0 && i < PC_N) ? kProfNames[i] : ""; }
int hipt_profile_read(float* ms, int* counts) {
    for (int i = 0; i < PC_N; ++i) {
        ms[i] = 0.f;
        counts[i] = 0;
    }
    for (int i = 0; i < g_prof.n; ++i) {
        if (hipEventSynchronize(g_prof.ev[i][1]) != hipSuccess) {
            hipt_set_error("profile: hipEventSynchronize failed");
            return HIPT_E_LAUNCH;
        }
        float t = 0.f;
        (void)hipEventElapsedTime(&t, g_prof.ev[i][0], g_prof.ev[i][1]);
        ms[g_prof.cat[i]] += t;
        counts[g_prof.cat[i]] += 1;
    }
    const int dropped = g_prof.n >= kProfMax;
    g_prof.n = 0;
    return dropped ? HIPT_E_WORKSPACE : HIPT_OK;
}
const char* hipt_last_error(void) { return g_err; }

int hipt_layernorm(const float* x, int64_t x_stride, const float* w, const float* b, void* out, int out_dtype,
                   int64_t out_stride, int rows, int D, float eps, void* stream) {
    return hipt_layernorm_launch(x, x_stride, w, b, out, out_dtype, out_stride, rows, D, eps, S(stream));
}

int hipt_linear(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias, const float* resid, void* out,
                int64_t ldc, int M, int N, int K, int dtype, int flags, void* stream) {
    HIPT_CHECK_ARG((flags & ~(HIPT_EPI_GELU | HIPT_EPI_RESID | HIPT_EPI_OUT_F32 | HIPT_EPI_RELU)) == 0, "linear: bad flags %d",
                   flags);
    HIPT_CHECK_ARG(!(flags & HIPT_EPI_RESID) || resid != nullptr, "linear: RESID without a residual pointer");
    GemmParams p = gemm_params(A, lda, W, ldw, bias, out, ldc, M, N, K);
    p.resid = resid;
    return linear(p, dtype, flags, S(stream));
}

int hipt_attention(const void* qkv, void* out, float* probs, int B, int ntok, int heads, int dh, float scale, int dtype,
                   void* stream) {
    return hipt_attention_launch(qkv, out, probs, B, ntok, heads, dh, scale, dtype, S(stream));
}

size_t hipt_vit_workspace_bytes(const hipt_vit_weights* w, int nseq) {
    return dry_run([&](Carver& c) { carve_vit4k(c, w, nseq, false); });
}

size_t hipt_vit256_forward_workspace_bytes(const hipt_vit_weights* w, const hipt_image_layout* lay, int nseq, int chunk) {
    return dry_run([&](Carver& c) { carve_vit256(c, w, nseq, chunk, image_compute_bytes(w, lay, nseq, IMG_F32)); });
}

size_t hipt_vit4k_forward_workspace_bytes(const hipt_vit_weights* w, int nseq) {
    return dry_run([&](Carver& c) { carve_vit4k(c, w, nseq, true); });
}

int hipt_vit256_prepare_tokens(const hipt_vit_weights* w, const float* images, const hipt_image_layout* lay, int seq0,
                               int nseq, float* x, void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(images && lay && x && nseq > 0 && seq0 >= 0, "vit256_prepare_tokens: null/empty argument");
    const void* img = images;
    if (w->dtype == HIPT_BF16) {
        const int64_t n = image_elems(lay, seq0 + nseq);
        Carver c(workspace, ws_bytes);
        c.take((size_t)n * 2);
        if ((rc = check_workspace(c, "vit256_prepare_tokens"))) return rc;
        if (embed_fused_ok(w, images, lay, ws_bytes)) {
            if ((rc = hipt_embed32_pack_launch(w->embed_w, workspace, S(stream)))) return rc;
            return embed256_px(w, images, IMG_F32, lay, seq0, nseq, x, workspace, nullptr, S(stream));
        }
        if ((rc = hipt_f32_to_bf16_launch(images, workspace, n, S(stream)))) return rc;
        img = workspace;
    }
    return embed256(w, img, lay, seq0, nseq, x, S(stream));
}

int hipt_vit4k_prepare_tokens(const hipt_vit_weights* w, const float* tokens_in, int nseq, float* x, void* workspace,
                              size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(x && nseq > 0 && (tokens_in || w->ntok == 1), "vit4k_prepare_tokens: null/empty argument");
    const void* tok = tokens_in;
    const int64_t n = (int64_t)nseq * (w->ntok - 1) * w->embed_k;
    if (w->dtype == HIPT_BF16 && n > 0) {
        Carver c(workspace, ws_bytes);
        c.take((size_t)n * 2);
        if ((rc = check_workspace(c, "vit4k_prepare_tokens"))) return rc;
        if ((rc = hipt_f32_to_bf16_launch(tokens_in, workspace, n, S(stream)))) return rc;
        tok = workspace;
    }
    return embed4k(w, tok, nseq, x, S(stream));
}

int hipt_vit_blocks(const hipt_vit_weights* w, float* x, int nseq, int blk_begin, int blk_end, float* probs, void* workspace,
                    size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(x && nseq > 0 && blk_begin >= 0 && blk_end <= w->depth && blk_begin <= blk_end, "vit_blocks: bad range [%d,%d)",
                   blk_begin, blk_end);
    Carver c(workspace, ws_bytes);
    BlockScratch s = carve_blocks(c, w, nseq);
    if ((rc = check_workspace(c, "vit_blocks"))) return rc;
    VitRoute r = vit_route(w, nseq, blk_begin, blk_end, probs != nullptr, 0);
    return run_blocks(w, x, nseq, probs, s, r, S(stream));
}

// the [CLS] row of the last block's attention map, probs_cls[nseq, heads, ntok], without the
// [nseq, heads, ntok, ntok] tensor (heat-maps read attention[:, :, 0, 1:], hipt_4k.py:143-158).  x = prepared tokens
// (modified: it ends as the input of the last block).  Every dtype / head dim check_vit admits.
int hipt_vit_cls_attention(const hipt_vit_weights* w, float* x, int nseq, float* probs_cls, void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(x && probs_cls && nseq > 0, "vit_cls_attention: null/empty argument");
    const int D = w->dim, dh = D / w->heads, M = nseq * w->ntok, last = w->depth - 1;
    Carver c(workspace, ws_bytes);
    BlockScratch s = carve_blocks(c, w, nseq);
    if ((rc = check_workspace(c, "vit_cls_attention"))) return rc;
    hipStream_t st = S(stream);
    // ViT-256 hot case: the A-stationary QKV GEMM (LayerNorm-1 from the chained MLP before it where there is one) + the one-query kernel
    const bool hot = w->dtype == HIPT_BF16 && dh == 64 && hipt_seqgemm_supported(w->dtype, D);
    VitRoute r = vit_route(w, nseq, 0, last, false, hot ? RT_EMIT_LAST : 0);
    if ((rc = run_blocks(w, x, nseq, nullptr, s, r, st))) return rc;
    if (hot) {
        SeqGemmParams q = qkv_params(w, last, M, x, s);
        if (r.have_xn) qkv_from_xn(q, s.att);
        if ((rc = hipt_seqgemm_launch(q, !r.have_xn, 0, st))) return rc;
        return hipt_attn_cls_launch(s.qkv, nullptr, probs_cls, nseq, w->ntok, w->heads, dh, attn_scale(w), st);
    }
    // every other configuration (fp32; head dim 32 = ViT-4K): LayerNorm-1 + the QKV projection of the last block and the
    // probabilities of the [CLS] query from the one-query kernel
    const hipt_block_weights& b = w->blocks[last];
    GemmParams g = gemm_params(s.xn, D, b.qkv_w, D, b.qkv_b, s.qkv, 3 * D, M, 3 * D, D);
    g.rpt = w->ntok;
    if ((rc = hipt_layernorm_launch(x, D, b.ln1_w, b.ln1_b, s.xn, w->dtype, D, M, D, w->ln_eps, st))) return rc;
    if ((rc = linear(g, w->dtype, 0, st))) return rc;
    return hipt_attn_cls_probs_launch(s.qkv, probs_cls, nseq, w->ntok, w->heads, dh, attn_scale(w), w->dtype, st);
}

int hipt_vit_attention_unit(const hipt_vit_weights* w, int block, const void* xn_img, int nseq, void* out_img, int fused, void* workspace,
                            size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(xn_img && out_img && xn_img != out_img && nseq > 0 && block >= 0 && block < w->depth, "vit_attention_unit: bad argument");
    const int D = w->dim, M = nseq * w->ntok;
    if (!hipt_qkv_attn_supported(w->dtype, D, w->heads, w->ntok) || M % 16 != 0) {
        hipt_set_error("vit_attention_unit: bf16, D = 384, 6 heads, 257 tokens and nseq * 257 %% 16 == 0 only");
        return HIPT_E_UNSUPPORTED;
    }
    Carver c(workspace, workspace ? ws_bytes : 0);  // (a null workspace is refused like a short one)
    BlockScratch s = carve_vit4k(c, w, nseq, false).s;  // hipt_vit_workspace_bytes' layout: the size the header asks for is the size checked
    if ((rc = check_workspace(c, "vit_attention_unit"))) return rc;
    hipStream_t st = S(stream);
    const hipt_block_weights& b = w->blocks[block];
    SeqGemmParams q = qkv_params(w, block, M, nullptr, s);
    qkv_from_xn(q, xn_img);
    HIPT_CHECK_ARG(b.qkv_pk != nullptr, "vit_attention_unit: blocks[%d].qkv_pk is NULL", block);
    // (the launches are booked in the forward's categories: a test reads the route it got from the counts)
    if (fused) {
        HIPT_CHECK_ARG(b.qkv_att_pk != nullptr, "vit_attention_unit: blocks[%d].qkv_att_pk is NULL", block);
        PROF(PC_CLSROWS, hipt_gather_cls_bf16_launch(xn_img, s.cls_xn, nseq, w->ntok, D, st, 1));
        q.M = nseq; q.A = s.cls_xn; q.out = s.cls_qkv;
        PROF(PC_CLSROWS, hipt_seqgemm_launch(q, false, 0, st));
        PROF(PC_QKVATT, hipt_qkv_attn_launch(xn_img, b.qkv_att_pk, b.qkv_b, s.cls_qkv, out_img, nseq, attn_scale(w), st));
        return HIPT_OK;
    }
    const bool hm = (int64_t)M * 3 * D * 2 < ((int64_t)1 << 32) - 65536;
    q.img = 1 | (hm ? 4 : 0);
    PROF(PC_QKV, hipt_seqgemm_launch(q, false, 0, st));
    PROF(PC_ATTN, hipt_attention_launch(s.qkv, out_img, nullptr, nseq, w->ntok, w->heads, D / w->heads, attn_scale(w), w->dtype, st, 1, hm ? 1 : 0));
    return HIPT_OK;
}

int hipt_vit_mlp_unit(const hipt_vit_weights* w, int block, float* x_img, const void* att_img, int nseq, void* xn_out_img, void* workspace,
                      size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(x_img && att_img && nseq > 0 && block >= 0 && block < w->depth, "vit_mlp_unit: bad argument");
    const int D = w->dim, M = nseq * w->ntok;
    const hipt_block_weights& b = w->blocks[block];
    if (!hipt_mlp16_supported(w->dtype, D, w->hidden) || M % 16 != 0 || !b.mlp_pk || b.mlp_pk_fmt != 3) {
        hipt_set_error("vit_mlp_unit: bf16, D = 384, hidden %% 128 == 0, nseq * ntok %% 16 == 0 and blocks[%d].mlp_pk in format 3 only", block);
        return HIPT_E_UNSUPPORTED;
    }
    Carver c(workspace, workspace ? ws_bytes : 0);  // (no buffer holds no bytes: a null workspace is refused like a short one)
    BlockScratch s = {};
    s.queues = c.take<TileQueues>(1);  // (the one queue it needs: the first line of the 256 bytes)
    if ((rc = check_workspace(c, "vit_mlp_unit"))) return rc;
    MlpParams m = mlp_params(w, block, M, x_img, s);
    m.y1 = att_img;
    m.fold = 1;
    m.img = 3;
    if (xn_out_img) mlp_emit_xn(m, w->blocks[block + 1 < w->depth ? block + 1 : block], xn_out_img);
    hipStream_t st = S(stream);
    PROF(PC_MLP, hipt_mlp_launch(m, st));
    return HIPT_OK;
}

int hipt_vit_cls_block_unit(const hipt_vit_weights* w, const void* xn_img, const float* x_img, int nseq, float* xc_out, void* att_out, void* workspace,
                            size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(xn_img && x_img && xc_out && nseq > 0, "vit_cls_block_unit: null/empty argument");
    const int D = w->dim;
    const int64_t M = (int64_t)nseq * w->ntok;
    // the route of a whole forward of this size whose embedding wrote images (vit256_range_impl), in the state run_blocks leaves it in
    // behind the last chained block: x an fp32 image, s.att LayerNorm-1 of the last block as a bf16 image
    VitRoute r = vit_route(w, nseq, 0, w->depth, false, RT_CLS_ONLY | RT_PX_EMBED);
    if (!hipt_qkv_attn_supported(w->dtype, D, w->heads, w->ntok) || M % 16 != 0 || !r.prune || !r.chain || !r.img) {
        hipt_set_error("vit_cls_block_unit: bf16, D = 384, 6 heads, 257 tokens, nseq * 257 %% 16 == 0 and a forward that prunes its last block "
                       "on activation images only");
        return HIPT_E_UNSUPPORTED;
    }
    r.have_xn = r.x_img = true;
    Carver c(workspace, workspace ? ws_bytes : 0);  // (a null workspace is refused like a short one)
    BlockScratch s = carve_vit4k(c, w, nseq, false).s;  // hipt_vit_workspace_bytes' layout
    if ((rc = check_workspace(c, "vit_cls_block_unit"))) return rc;
    HIPT_CHECK_ARG(s.fits_cls_xn, "vit_cls_block_unit: hidden %d leaves no room for the [CLS] rows in the block scratch", w->hidden);
    hipStream_t st = S(stream);
    // The fused routes only read the LayerNorm-1 image: they run on the caller's.  The two-kernel route leaves its attention rows in
    // s.att, so it runs on a copy in the workspace slot.  x is read by the [CLS] residual gather alone.
    if (block_route(r, w->blocks[w->depth - 1], false).fuse)
        s.att = const_cast<void*>(xn_img);
    else if (hipMemcpyAsync(s.att, xn_img, (size_t)M * D * 2, hipMemcpyDeviceToDevice, st) != hipSuccess)
        return HIPT_E_LAUNCH;
    const void* rows = s.att == xn_img ? s.qkv : s.att;  // where run_last_block_cls leaves att_rows
    if ((rc = run_last_block_cls(w, const_cast<float*>(x_img), nseq, s, r, st))) return rc;
    if (hipMemcpyAsync(xc_out, s.xc, (size_t)nseq * D * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return HIPT_E_LAUNCH;
    if (att_out && hipMemcpyAsync(att_out, rows, (size_t)nseq * D * 2, hipMemcpyDeviceToDevice, st) != hipSuccess) return HIPT_E_LAUNCH;
    return HIPT_OK;
}

int hipt_vit_embed_unit(const hipt_vit_weights* w, const void* images, int input_kind, const hipt_image_layout* lay, int seq0, int nseq, float* x_out,
                        void* xn_out_img, void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(images && lay && x_out && nseq > 0 && seq0 >= 0 && input_kind >= IMG_F32 && input_kind <= IMG_U8_HWC && (!xn_out_img || w->depth > 0),
                   "vit_embed_unit: bad argument");
    // the forwards' own question (vit256_forward_impl, hipt_vit256_forward_range_px), asked of a slot that is large enough: a short
    // workspace is refused as a workspace below
    if (!embed_fused_ok(w, images, lay, embed_px_slot_bytes(), input_kind) || (xn_out_img && ((int64_t)nseq * w->ntok) % 16 != 0)) {
        hipt_set_error("vit_embed_unit: bf16, D = 384, 256 x 256 patches of 16 x 16-pixel tokens, 16-byte aligned pixel rows (uint8: strides %% 8 == 0, "
                       "batch_stride = 3 * chan_stride), nseq * ntok %% 16 == 0 for the image outputs, and not under HIPT_GENERIC only");
        return HIPT_E_UNSUPPORTED;
    }
    Carver c(workspace, workspace ? ws_bytes : 0);  // (a null workspace is refused like a short one)
    void* slot = c.take(embed_px_slot_bytes());     // the packed Conv2d weight with the kernel's tile queue behind it
    if ((rc = check_workspace(c, "vit_embed_unit"))) return rc;
    hipStream_t st = S(stream);
    if ((rc = hipt_embed32_pack_launch(w->embed_w, slot, st))) return rc;
    return embed256_px(w, images, input_kind, lay, seq0, nseq, x_out, slot, xn_out_img, st);
}

// Format of the fused MLP's weight image: 2 = csrc/mlp16.hip (16x16x32 MFMAs), 0 = this shape has no packed form.  (Format 1 was a
// 32x32x16 form, tools/experiments/mlp32_r4.hip, since retired -- DESIGN.md; an image packed as format 1 is refused by blocks_chain
// and its model falls back to the generic kernels.)
// 3 (what this version packs) = format 2 behind six units of the proj matrix: the attention block's output projection then runs at the
// head of the fused MLP's tiles (mlp16.hip, FOLD) and the chained blocks have no proj launch.  HIPT_NO_PROJ_FOLD=1 at LAUNCH time runs proj as its
// own kernel again from the same image (the MLP's own units lie behind the proj units); an image packed as format 2 by an older binding still runs.
int hipt_vit_mlp_pack_format(const hipt_vit_weights* w) { return w && hipt_mlp16_supported(w->dtype, w->dim, w->hidden) ? 3 : 0; }

size_t hipt_vit_packed_bytes(const hipt_vit_weights* w, int what) {
    if (!w || w->dtype != HIPT_BF16) return 0;
    const int D = w->dim;
    switch (what) {
        case HIPT_PACK_QKV: return hipt_seqgemm_pipe_supported(w->dtype, D, 3 * D, false, 0) ? (size_t)3 * D * D * 2 : 0;
        case HIPT_PACK_PROJ: return hipt_seqgemm_pipe_supported(w->dtype, D, D, false, 0) ? (size_t)D * D * 2 : 0;
        case HIPT_PACK_MLP: return hipt_vit_mlp_pack_format(w) != 0 ? hipt_mlp16_packed_bytes(D, w->hidden, hipt_vit_mlp_pack_format(w) == 3) : 0;
        case HIPT_PACK_QKV_ATT: return hipt_qkv_attn_supported(w->dtype, D, w->heads, w->ntok) ? hipt_qkv_attn_packed_bytes() : 0;
        case HIPT_PACK_CLS_ABSORB:
            return hipt_qkv_attn_supported(w->dtype, D, w->heads, w->ntok) && hipt_cls_pool_supported(w->dtype, D, w->heads, w->ntok) ? hipt_cls_absorb_packed_bytes() : 0;
        default: return 0;
    }
}

int hipt_vit_pack_weights(const hipt_vit_weights* w, int block, int what, void* out, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(block >= 0 && block < w->depth, "vit_pack_weights: block %d of %d", block, w->depth);
    HIPT_CHECK_ARG(out != nullptr, "vit_pack_weights: null output");
    if (hipt_vit_packed_bytes(w, what) == 0) {
        hipt_set_error("vit_pack_weights: matrix %d of this ViT (dtype %d, D=%d, hidden=%d) has no packed form", what, w->dtype, w->dim, w->hidden);
        return HIPT_E_UNSUPPORTED;
    }
    const hipt_block_weights& b = w->blocks[block];
    const int D = w->dim;
    hipStream_t st = S(stream);
    switch (what) {
        case HIPT_PACK_QKV: return hipt_seqgemm_pack_launch(b.qkv_w, 3 * D, D, out, st);
        case HIPT_PACK_PROJ: return hipt_seqgemm_pack_launch(b.proj_w, D, D, out, st);
        case HIPT_PACK_QKV_ATT: return hipt_qkv_attn_pack_launch(b.qkv_w, out, st);
        case HIPT_PACK_CLS_ABSORB: return hipt_cls_absorb_pack_launch(b.qkv_w, out, st);
        default:
            // the format the caller recorded beside the pointer (hipt_vit_mlp_pack_format): pack and launch read the same field
            if ((b.mlp_pk_fmt == 2 || b.mlp_pk_fmt == 3) && hipt_mlp16_supported(w->dtype, D, w->hidden))
                return hipt_mlp16_pack_launch(b.fc1_w, b.fc2_w, D, w->hidden, out, st, b.mlp_pk_fmt == 3 ? b.proj_w : nullptr);
            hipt_set_error("hipt_vit_pack_weights: blocks[%d].mlp_pk_fmt = %d is not a format this model has", block, b.mlp_pk_fmt);
            return HIPT_E_BADARG;
    }
}

int hipt_vit_head(const hipt_vit_weights* w, const float* x, int nseq, int cls_only, float* out, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    const int D = w->dim;
    if (cls_only)
        return hipt_layernorm_launch(x, (int64_t)w->ntok * D, w->norm_w, w->norm_b, out, HIPT_F32, D, nseq, D, w->ln_eps, S(stream));
    return hipt_layernorm_launch(x, D, w->norm_w, w->norm_b, out, HIPT_F32, D, nseq * w->ntok, D, w->ln_eps, S(stream));
}

// ViT-256 over the sequences [seq0, seq0 + nseq) of an image tensor that is ALREADY in the compute dtype, chunk by chunk:
// out[i] = [CLS] feature of sequence seq0 + i.
// (embed_pk != null: `img` is the fp32 / uint8 image and the embedding reads it directly -- embed32.hip)
static int vit256_range_impl(const hipt_vit_weights* w, const void* img, const hipt_image_layout* lay, int seq0, int nseq, int chunk, float* out,
                             void* workspace, size_t ws_bytes, hipStream_t st, const void* embed_pk = nullptr, int embed_kind = IMG_F32) {
    int rc;
    const int D = w->dim;
    Carver c(workspace, ws_bytes);
    const RangeWs g = carve_range(c, w, nseq, chunk);
    if ((rc = check_workspace(c, "vit256_forward"))) return rc;
    for (int s0 = 0; s0 < nseq; s0 += g.chunk) {
        const int n = nseq - s0 < g.chunk ? nseq - s0 : g.chunk;
        VitRoute r = vit_route(w, n, 0, w->depth, false, RT_CLS_ONLY | (embed_pk ? RT_PX_EMBED : 0));
        if (r.prune && !(r.chain ? g.s.fits_cls_xn : g.s.fits_xc)) {
            hipt_set_error("vit256_forward: %d tokens x hidden %d leave no room in the block scratch for the [CLS] rows of the pruned last block "
                           "(HIPT_NO_PRUNE=1 runs it in full)", w->ntok, w->hidden);
            return HIPT_E_WORKSPACE;
        }
        if (embed_pk)
            rc = embed256_px(w, img, embed_kind, lay, seq0 + s0, n, g.x, embed_pk, r.pre ? g.s.att : nullptr, st);
        else
            rc = embed256(w, img, lay, seq0 + s0, n, g.x, st);
        if (rc) return rc;
        if ((rc = run_blocks(w, g.x, n, nullptr, g.s, r, st))) return rc;
        if (r.prune && (rc = run_last_block_cls(w, g.x, n, g.s, r, st))) return rc;
        // the [CLS] rows: compact after the pruned block, row 0 of every sequence otherwise
        PROF(PC_LN, hipt_layernorm_launch(r.prune ? g.s.xc : g.x, r.prune ? D : (int64_t)w->ntok * D, w->norm_w, w->norm_b, out + (size_t)s0 * D,
                                          HIPT_F32, D, n, D, w->ln_eps, st));
    }
    return HIPT_OK;
}

// the input image tensor in the compute dtype: fp32 input in fp32 mode is used where it lies (returns `images`), everything
// else is converted / normalised into `dst`
static int image_to_compute(const hipt_vit_weights* w, const void* images, int kind, const hipt_image_layout* lay, int nseq, void* dst,
                            const void** img_out, hipStream_t st) {
    int rc;
    const int64_t n_img = image_elems(lay, nseq);
    if (kind != IMG_F32) {
        const int per = lay->grid_w * lay->grid_h;
        HIPT_CHECK_ARG(nseq % per == 0, "vit256_forward: uint8 input must hold whole regions");
        const int64_t plane = lay->batch_stride / 3;
        PROF(PC_OTHER, hipt_u8_normalize_launch(images, kind == IMG_U8_HWC, nseq / per, plane, dst, w->dtype, st));
        *img_out = dst;
    } else if (w->dtype == HIPT_BF16) {
        PROF(PC_OTHER, hipt_f32_to_bf16_launch((const float*)images, dst, n_img, st));
        *img_out = dst;
    } else {
        *img_out = images;
    }
    return HIPT_OK;
}

static int vit256_forward_impl(const hipt_vit_weights* w, const void* images, int kind, const hipt_image_layout* lay, int nseq, int chunk,
                               float* out, void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(images && lay && out && nseq > 0, "vit256_forward: null/empty argument");
    hipStream_t st = S(stream);
    Carver c(workspace, ws_bytes);
    const Vit256Ws v = carve_vit256(c, w, nseq, chunk, image_compute_bytes(w, lay, nseq, kind));
    if ((rc = check_workspace(c, "vit256_forward"))) return rc;
    const void* img = images;
    // fp32 pixels, bf16 model, 256 x 256 patches: the embedding kernel reads the image itself; the slot of the bf16 copy holds its
    // packed weight (made here: 0.6 MB, a few microseconds) and its tile queue instead
    // (uint8 RGB, planar or interleaved: the same kernel normalises in registers -- no device copy of the image at all)
    if (embed_fused_ok(w, images, lay, v.nslot, kind)) {
        if ((rc = hipt_embed32_pack_launch(w->embed_w, v.slot, st))) return rc;
        return vit256_range_impl(w, images, lay, 0, nseq, chunk, out, v.range, v.nrange, st, v.slot, kind);
    }
    if ((rc = image_to_compute(w, images, kind, lay, nseq, v.slot, &img, st))) return rc;
    return vit256_range_impl(w, img, lay, 0, nseq, chunk, out, v.range, v.nrange, st);
}

int hipt_vit256_forward(const hipt_vit_weights* w, const float* images, const hipt_image_layout* lay, int nseq, int chunk,
                        float* out, void* workspace, size_t ws_bytes, void* stream) {
    return vit256_forward_impl(w, images, IMG_F32, lay, nseq, chunk, out, workspace, ws_bytes, stream);
}

size_t hipt_image_compute_bytes(const hipt_vit_weights* w, const hipt_image_layout* lay, int nseq, int input_kind) {
    return w && lay && nseq > 0 ? image_compute_bytes(w, lay, nseq, input_kind) : 0;
}

int hipt_image_to_compute(const hipt_vit_weights* w, const void* images, int input_kind, const hipt_image_layout* lay, int nseq, void* dst,
                          void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(images && lay && nseq > 0 && input_kind >= IMG_F32 && input_kind <= IMG_U8_HWC, "image_to_compute: bad argument");
    HIPT_CHECK_ARG(dst != nullptr && ((uintptr_t)dst & 255) == 0, "image_to_compute: null / unaligned destination");
    const void* img = nullptr;
    return image_to_compute(w, images, input_kind, lay, nseq, dst, &img, S(stream));
}

size_t hipt_vit256_range_workspace_bytes(const hipt_vit_weights* w, int nseq, int chunk) {
    return w && nseq > 0 ? dry_run([&](Carver& c) { carve_range(c, w, nseq, chunk); }) : 0;
}

int hipt_vit256_forward_range(const hipt_vit_weights* w, const void* images_cd, const hipt_image_layout* lay, int seq0, int nseq, int chunk,
                              float* out, void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(images_cd && lay && out && nseq > 0 && seq0 >= 0, "vit256_forward_range: null/empty argument");
    return vit256_range_impl(w, images_cd, lay, seq0, nseq, chunk, out, workspace, ws_bytes, S(stream));
}

// the same over fp32 pixels where the embedding kernel reads them itself (embed32.hip): no image in the compute dtype is needed
size_t hipt_vit256_range_px_workspace_bytes(const hipt_vit_weights* w, const hipt_image_layout* lay, int nseq, int chunk) {
    if (!w || !lay || nseq <= 0 || lay->patch_h <= 0 || lay->patch_w <= 0) return 0;
    // (the pointer's alignment is checked at the call; any non-null 16-byte aligned value stands in for it here)
    if (!embed_fused_ok(w, (const void*)16, lay, embed_px_slot_bytes())) return 0;
    return dry_run([&](Carver& c) { carve_vit256(c, w, nseq, chunk, embed_px_slot_bytes()); });
}

int hipt_vit256_forward_range_px(const hipt_vit_weights* w, const float* images, const hipt_image_layout* lay, int seq0, int nseq, int chunk,
                                 float* out, void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(images && lay && out && nseq > 0 && seq0 >= 0, "vit256_forward_range_px: null/empty argument");
    if (!embed_fused_ok(w, images, lay, embed_px_slot_bytes())) {
        hipt_set_error("vit256_forward_range_px: this model / layout has no pixel-reading embedding (hipt_vit256_range_px_workspace_bytes returns 0)");
        return HIPT_E_UNSUPPORTED;
    }
    Carver c(workspace, ws_bytes);
    const Vit256Ws v = carve_vit256(c, w, nseq, chunk, embed_px_slot_bytes());
    if ((rc = check_workspace(c, "vit256_forward_range_px"))) return rc;
    if ((rc = hipt_embed32_pack_launch(w->embed_w, v.slot, S(stream)))) return rc;
    return vit256_range_impl(w, images, lay, seq0, nseq, chunk, out, v.range, v.nrange, S(stream), v.slot);
}

int hipt_vit4k_forward(const hipt_vit_weights* w, const float* tokens_in, int nseq, float* out, void* workspace,
                       size_t ws_bytes, void* stream) {
    int rc = check_vit(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(out && nseq > 0, "vit4k_forward: null/empty argument");
    hipStream_t st = S(stream);
    Carver c(workspace, ws_bytes);
    const Vit4kWs k = carve_vit4k(c, w, nseq, true);
    if ((rc = check_workspace(c, "vit4k_forward"))) return rc;
    const void* tok = tokens_in;
    const int64_t n = (int64_t)nseq * (w->ntok - 1) * w->embed_k;
    if (w->dtype == HIPT_BF16 && n > 0) {
        if ((rc = hipt_f32_to_bf16_launch(tokens_in, k.tok, n, st))) return rc;
        tok = k.tok;
    }
    // ALL the regions of a call go through the small-call kernels together (RT_FORCE_SMALL): one wave per 16 x 32 output tile, rows
    // independent bit for bit, the attention one workgroup per (region, head) -- which kernels a region's 257 rows meet, and the bits they
    // write, do not depend on how many regions share the call: one region alone, eight gathered by extract_slide and a ragged tail of three
    // agree exactly (tests).  Thirty launches per call whatever its size; the phi GEMM takes the small kernel too, for the same reason.
    if ((rc = embed4k(w, tok, nseq, k.x, st, 1))) return rc;
    VitRoute r = vit_route(w, nseq, 0, w->depth, false, RT_FORCE_SMALL);
    if ((rc = run_blocks(w, k.x, nseq, nullptr, k.s, r, st))) return rc;
    return hipt_layernorm_launch(k.x, (int64_t)w->ntok * w->dim, w->norm_w, w->norm_b, out, HIPT_F32, w->dim, nseq, w->dim, w->ln_eps, st);
}

size_t hipt_hipt4k_workspace_bytes(const hipt_vit_weights* w256, const hipt_vit_weights* w4k, int nreg, int w_256, int h_256,
                                   int chunk) {
    return dry_run([&](Carver& c) { carve_hipt4k(c, w256, w4k, nreg, w_256, h_256, chunk, IMG_F32); });
}

static int hipt4k_forward_impl(const hipt_vit_weights* w256, const hipt_vit_weights* w4k, const void* regions, int kind, int nreg, int W,
                               int H, int chunk, float* cls256_out, float* out, void* workspace, size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(w256 && w4k && regions && out && nreg > 0, "hipt4k_forward: null/empty argument");
    HIPT_CHECK_ARG(W > 0 && H > 0 && W % 256 == 0 && H % 256 == 0, "hipt4k_forward: region %dx%d must be cropped to multiples of 256",
                   W, H);
    const int per = (W / 256) * (H / 256), nseq = nreg * per;
    HIPT_CHECK_ARG(w4k->ntok == per + 1, "hipt4k_forward: ViT-4K weights prepared for %d tokens, region has %d", w4k->ntok, per + 1);
    HIPT_CHECK_ARG(w4k->embed_k == w256->dim, "hipt4k_forward: ViT-4K input width %d != ViT-256 width %d", w4k->embed_k, w256->dim);
    const hipt_image_layout lay = region_layout(W, H);
    Carver c(workspace, ws_bytes);
    const Hipt4kWs h = carve_hipt4k(c, w256, w4k, nreg, W / 256, H / 256, chunk, kind);
    int rc = check_workspace(c, "hipt4k_forward");
    if (rc) return rc;
    // cls256 [nreg * per, 384] token-major = nreg sequences of `per` tokens: exactly phi's input (hipt_4k.py:72-74)
    float* cls = cls256_out ? cls256_out : h.cls;
    rc = vit256_forward_impl(w256, regions, kind, &lay, nseq, chunk, cls, h.ws256, h.n256, stream);
    if (rc) return rc;
    return hipt_vit4k_forward(w4k, cls, nreg, out, h.ws4k, h.n4k, stream);
}

int hipt_hipt4k_forward(const hipt_vit_weights* w256, const hipt_vit_weights* w4k, const float* regions, int nreg, int W, int H,
                        int chunk, float* cls256_out, float* out, void* workspace, size_t ws_bytes, void* stream) {
    return hipt4k_forward_impl(w256, w4k, regions, IMG_F32, nreg, W, H, chunk, cls256_out, out, workspace, ws_bytes, stream);
}

size_t hipt_hipt4k_u8_workspace_bytes(const hipt_vit_weights* w256, const hipt_vit_weights* w4k, int nreg, int w_256, int h_256, int chunk) {
    if (!w256 || !w4k || nreg <= 0 || w_256 <= 0 || h_256 <= 0) return 0;
    return dry_run([&](Carver& c) { carve_hipt4k(c, w256, w4k, nreg, w_256, h_256, chunk, IMG_U8_CHW); });
}

int hipt_hipt4k_forward_u8(const hipt_vit_weights* w256, const hipt_vit_weights* w4k, const uint8_t* regions, int interleaved, int nreg,
                           int W, int H, int chunk, float* cls256_out, float* out, void* workspace, size_t ws_bytes, void* stream) {
    return hipt4k_forward_impl(w256, w4k, regions, interleaved ? IMG_U8_HWC : IMG_U8_CHW, nreg, W, H, chunk, cls256_out, out, workspace,
                               ws_bytes, stream);
}

int hipt_u8_normalize(const void* src, int interleaved, int64_t n_images, int64_t plane, void* dst, int dst_dtype, void* stream) {
    return hipt_u8_normalize_launch(src, interleaved, n_images, plane, dst, dst_dtype, S(stream));
}

// ------------------------------------------------------------------------------------------------
// CLAM_SB / ABMIL
// ------------------------------------------------------------------------------------------------
static int check_clam(const hipt_clam_weights* w) {
    HIPT_CHECK_ARG(w != nullptr, "clam: null weights");
    HIPT_CHECK_ARG(w->dtype == HIPT_F32 || w->dtype == HIPT_BF16, "clam: bad dtype %d", w->dtype);
    HIPT_CHECK_ARG(w->s1 > 0 && w->s2 > 0, "clam: bad widths [%d,%d,%d]", w->s0, w->s1, w->s2);
    return HIPT_OK;
}

// The ticket block is the FIRST 256 bytes of the workspace, whatever the model's widths, and nothing else ever writes there
// (one workspace may serve several CLAM modules of different widths / paths on a stream: the generic path's scratch must not
// run over the streaming kernels' arrival counter).
size_t hipt_clam_ticket_offset(const hipt_clam_weights* w, int N) { return 0; }

// ticket (hipt_clam_ticket_offset() = 0: zero before the first use, zero after every call) | partials | gmax, and for the generic path
// h1 fp32 | ab fp32 | h1 in the compute dtype
struct ClamWs { unsigned* ticket; float *partials, *gmax, *h1, *ab; void* h1T; };
static ClamWs carve_clam(Carver& c, const hipt_clam_weights* w, int N) {
    ClamWs k;
    k.ticket = (unsigned*)c.take(256);
    k.partials = (float*)c.take((size_t)1024 * (2 + w->s1) * 4);  // fused: <= 512 workgroups; generic pool: <= 1024 row blocks
    k.gmax = (float*)c.take(256);
    k.h1 = (float*)c.take((size_t)N * w->s1 * 4);
    k.ab = (float*)c.take((size_t)N * 2 * w->s2 * 4);
    k.h1T = c.take((size_t)N * w->s1 * 2);
    return k;
}

size_t hipt_clam_workspace_bytes(const hipt_clam_weights* w, int N) { return dry_run([&](Carver& c) { carve_clam(c, w, N); }); }

size_t hipt_clam_stream_packed_bytes(const hipt_clam_weights* w) { return w ? hipt_clam_stream_image_bytes(w) : 0; }

int hipt_clam_stream_pack(const hipt_clam_weights* w, void* out, void* stream) {
    HIPT_CHECK_ARG(w != nullptr, "clam_stream_pack: null weights");
    return hipt_clam_stream_pack_launch(w, out, S(stream));
}

static int gated_scores(const hipt_clam_weights* w, const void* x, int xdtype, int N, float* ab, void* xT, float* A,
                        hipStream_t st) {
    // ab = x @ [Wa;Wb]^T + [ba;bb]  (x: [N,S1] in xdtype), then the gate
    const int kb = w->dtype == HIPT_F32 ? 32 : 64, n2 = 2 * w->s2;
    int rc;
    if (w->s1 % kb == 0 && n2 % 4 == 0) {
        const void* a = x;
        if (xdtype != w->dtype) {  // fp32 h1 -> bf16 operand
            if ((rc = hipt_f32_to_bf16_launch((const float*)x, xT, (int64_t)N * w->s1, st))) return rc;
            a = xT;
        }
        rc = linear(gemm_params(a, w->s1, w->wab, w->s1, w->bab, ab, n2, N, n2, w->s1), w->dtype, HIPT_EPI_OUT_F32, st);
    } else {
        rc = hipt_small_ab_launch(x, xdtype, N, w->s1, n2, w->wab, w->dtype, w->bab, ab, st);
    }
    if (rc) return rc;
    return hipt_gate_launch(ab, n2, N, w->s2, w->wc, w->bc, A, st);
}

int hipt_clam_sb_forward(const hipt_clam_weights* w, const void* bag, int N, int attention_only, float* A_raw, float* M,
                         float* logits, float* Y_prob, int64_t* Y_hat, void* workspace, size_t ws_bytes, void* stream) {
    int rc = check_clam(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(bag && A_raw && N > 0, "clam_sb_forward: null/empty bag (N=%d)", N);
    HIPT_CHECK_ARG(attention_only || (M && logits && Y_prob && Y_hat), "clam_sb_forward: null output");
    HIPT_CHECK_ARG(((uintptr_t)bag & 15) == 0, "clam_sb_forward: bag must be 16-byte aligned");
    const int kb = w->dtype == HIPT_F32 ? 32 : 64;
    if (w->s0 % kb != 0 || w->s1 % 4 != 0) {
        hipt_set_error("clam_sb_forward: S0=%d must be a multiple of %d and S1=%d of 4", w->s0, kb, w->s1);
        return HIPT_E_UNSUPPORTED;
    }
    Carver c(workspace, ws_bytes);
    const ClamWs k = carve_clam(c, w, N);
    if ((rc = check_workspace(c, "clam_sb_forward"))) return rc;
    hipStream_t st = S(stream);
    int G = 0;
    if (hipt_clam_stream_supported(w)) {  // bf16 [S0,128,64]: weight-stationary streaming kernel
        PROF(PC_ABMIL, hipt_clam_stream_launch(w, bag, N, attention_only, A_raw, k.partials, &G, k.ticket, M, logits, Y_prob, Y_hat, st));
        if (!attention_only && G == 0) return HIPT_OK;
    } else if (hipt_clam_fused_supported(w)) {
        PROF(PC_ABMIL, hipt_clam_fused_launch(w, bag, N, attention_only, A_raw, k.partials, &G, st));
    } else {
        if ((rc = linear(gemm_params(bag, w->s0, w->w1, w->s0, w->b1, k.h1, w->s1, N, w->s1, w->s0), w->dtype, HIPT_EPI_RELU | HIPT_EPI_OUT_F32, st))) return rc;
        if ((rc = gated_scores(w, k.h1, HIPT_F32, N, k.ab, k.h1T, A_raw, st))) return rc;
        if (!attention_only && (rc = hipt_pool_launch(A_raw, k.h1, N, w->s1, k.gmax, k.partials, &G, st))) return rc;
    }
    if (attention_only) return HIPT_OK;
    PROF(PC_COMBINE, hipt_clam_combine_launch(k.partials, G, w, M, logits, Y_prob, Y_hat, st));
    return HIPT_OK;
}

// ---- B bags in one call (abmil_bags.hip, abmil_narrow.hip, abmil_wide.hip, abmil_wide_mb.hip, abmil_bags_mb8.hip): unit table | tile_start | one partial per unit and branch; no state ----
// The call exists in six forms -- the mid-width single-branch heads, the narrow heads, the wide heads, the K = n_att branches of CLAM_MB at the
// mid widths (2..4 branches; 5..8 branches) and at the wide ones -- which share every line of the host side but the four things a ClamBagsForm names.
int hipt_clam_bags_supported(const hipt_clam_weights* w) { return w && check_clam(w) == HIPT_OK && w->s0 > 0 && hipt_clam_fused_supported(w) ? 1 : 0; }
int hipt_clam_narrow_bags_supported(const hipt_clam_weights* w) { return w && check_clam(w) == HIPT_OK && hipt_clam_narrow_supported(w) ? 1 : 0; }
int hipt_clam_wide_bags_supported(const hipt_clam_weights* w) { return w && check_clam(w) == HIPT_OK && hipt_clam_wide_supported(w) ? 1 : 0; }
int hipt_clam_mb_bags_supported(const hipt_clam_weights* w) {
    return hipt_clam_bags_supported(w) && w->n_att >= 2 && w->n_att <= 4 && w->n_att == w->n_classes ? 1 : 0;
}
int hipt_clam_mb_wide_bags_supported(const hipt_clam_weights* w) {
    return hipt_clam_wide_bags_supported(w) && w->n_att >= 2 && w->n_att <= 4 && w->n_att == w->n_classes ? 1 : 0;
}
int hipt_clam_mb_many_bags_supported(const hipt_clam_weights* w) {
    return hipt_clam_bags_supported(w) && w->n_att >= 5 && w->n_att <= 8 && w->n_att == w->n_classes ? 1 : 0;
}

struct ClamBagsForm {
    const char* name;                                // of the entry point, as every message starts
    int (*supported)(const hipt_clam_weights*);
    int (*branches)(const hipt_clam_weights*);       // partials per unit
    decltype(&hipt_clam_bags_tiles_launch) tiles;
    decltype(&hipt_clam_bags_combine_launch) combine;
    const char* why_not;                             // format of the unsupported message: name, S0, S1, S2, n_att, n_classes
};
static int one_branch(const hipt_clam_weights*) { return 1; }
static int att_branches(const hipt_clam_weights* w) { return w->n_att; }
static const ClamBagsForm BAGS_SB = {"clam_sb_forward_bags", hipt_clam_bags_supported, one_branch, hipt_clam_bags_tiles_launch,
                                     hipt_clam_bags_combine_launch,
                                     "%s: no multi-bag form for [%d,%d,%d] in this dtype: call hipt_clam_sb_forward per bag"};
static const ClamBagsForm BAGS_NARROW = {"clam_sb_forward_bags_narrow", hipt_clam_narrow_bags_supported, one_branch,
                                         hipt_clam_narrow_tiles_launch, hipt_clam_bags_combine_launch,
                                         "%s: [%d,%d,%d] is not a narrow head: (S1, S2) in {(8,4), (16,8), (32,8), (32,16)}, S0 a "
                                         "multiple of 32 (fp32) / 64 (bf16)"};
static const ClamBagsForm BAGS_WIDE = {"clam_sb_forward_bags_wide", hipt_clam_wide_bags_supported, one_branch, hipt_clam_wide_tiles_launch,
                                       hipt_clam_bags_combine_launch,
                                       "%s: [%d,%d,%d] is not a wide head: (S1, S2) in {(256,64), (512,256), (512,384)}, S0 a multiple "
                                       "of 32 (fp32) / 64 (bf16)"};
static const ClamBagsForm BAGS_MB = {"clam_mb_forward_bags", hipt_clam_mb_bags_supported, att_branches, hipt_clam_bags_mb_tiles_launch,
                                     hipt_clam_bags_mb_combine_launch,
                                     "%s: no multi-bag form for [%d,%d,%d] with %d branches / %d classes in this dtype: call "
                                     "hipt_clam_mb_forward or hipt_clam_sb_forward per bag"};
static const ClamBagsForm BAGS_MB_WIDE = {"clam_mb_forward_bags_wide", hipt_clam_mb_wide_bags_supported, att_branches,
                                          hipt_clam_wide_mb_tiles_launch, hipt_clam_bags_mb_combine_launch,
                                          "%s: [%d,%d,%d] with %d branches / %d classes is not a wide K-branch head: (S1, S2) in {(256,64), "
                                          "(512,256), (512,384)}, S0 a multiple of 32 (fp32) / 64 (bf16), 2 <= branches <= 4, branches == "
                                          "classes"};
static const ClamBagsForm BAGS_MB_MANY = {"clam_mb_forward_bags_many", hipt_clam_mb_many_bags_supported, att_branches,
                                          hipt_clam_bags_mb8_tiles_launch, hipt_clam_bags_mb_combine_launch,
                                          "%s: [%d,%d,%d] with %d branches / %d classes is not a many-branch head: the widths of "
                                          "hipt_clam_sb_forward_bags, 5 <= branches <= 8, branches == classes (2..4 branches: "
                                          "hipt_clam_mb_forward_bags)"};

// units of a call: sum_b ceil(N_b / 128) <= total_rows / 128 + B, known without reading the offsets back
static int64_t clam_bags_max_units(int B, int64_t total_rows) { return (total_rows + 127) / 128 + B; }
struct ClamBagsWs { void* units; int* tile_start; float* partials; };
static ClamBagsWs carve_clam_bags(Carver& c, const hipt_clam_weights* w, int B, int64_t total_rows, int branches) {
    const size_t nu = (size_t)clam_bags_max_units(B, total_rows);
    ClamBagsWs k;
    k.units = c.take(nu * hipt_clam_bags_unit_bytes());
    k.tile_start = c.take<int>((size_t)B + 1);
    k.partials = c.take<float>(nu * (size_t)branches * (2 + (size_t)w->s1));  // one partial per unit and attention branch
    return k;
}

static size_t clam_bags_ws_bytes(const ClamBagsForm& f, const hipt_clam_weights* w, int B, int64_t total_rows) {
    if (!f.supported(w) || B < 1 || total_rows < B || clam_bags_max_units(B, total_rows) > INT32_MAX) return 0;
    return dry_run([&](Carver& c) { carve_clam_bags(c, w, B, total_rows, f.branches(w)); });
}

static int clam_bags_forward(const ClamBagsForm& f, const hipt_clam_weights* w, const void* bags, const int64_t* offsets_dev, int B,
                             int64_t total_rows, int attention_only, float* A_raw, float* M, float* logits, float* Y_prob,
                             int64_t* Y_hat, void* workspace, size_t ws_bytes, void* stream) {
    HIPT_CHECK_ARG(w != nullptr, "%s: null weights", f.name);
    int rc = check_clam(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(bags && offsets_dev && A_raw && workspace, "%s: null argument", f.name);
    HIPT_CHECK_ARG(attention_only || (M && logits && Y_prob && Y_hat), "%s: null output", f.name);
    HIPT_CHECK_ARG(((uintptr_t)bags & 15) == 0, "%s: bags must be 16-byte aligned", f.name);
    HIPT_CHECK_ARG(B >= 1 && total_rows >= B, "%s: B = %d bags need at least one row each (total_rows = %lld)", f.name, B,
                   (long long)total_rows);
    HIPT_CHECK_ARG(clam_bags_max_units(B, total_rows) <= INT32_MAX, "%s: %lld rows in %d bags exceed 2^31 tiles", f.name,
                   (long long)total_rows, B);
    if (!f.supported(w)) {
        hipt_set_error(f.why_not, f.name, w->s0, w->s1, w->s2, w->n_att, w->n_classes);  // (a format may leave trailing arguments unread)
        return HIPT_E_UNSUPPORTED;
    }
    Carver c(workspace, ws_bytes);
    const ClamBagsWs k = carve_clam_bags(c, w, B, total_rows, f.branches(w));
    if (check_workspace(c, f.name)) return HIPT_E_BADARG;  // these entry points' contract: a short buffer is a bad argument
    hipStream_t st = S(stream);
    const int nu = (int)clam_bags_max_units(B, total_rows);
    PROF(PC_OTHER, hipt_clam_bags_units_launch(offsets_dev, B, total_rows, nu, k.tile_start, k.units, st));
    PROF(PC_ABMIL, f.tiles(w, bags, k.units, nu, attention_only, total_rows, A_raw, k.partials, st));  // A_raw [branches, total_rows]
    if (attention_only) return HIPT_OK;
    PROF(PC_COMBINE, f.combine(k.partials, k.tile_start, nu, B, w, M, logits, Y_prob, Y_hat, st));
    return HIPT_OK;
}

#define HIPT_CLAM_BAGS_ENTRY(forward, ws_bytes_fn, form)                                                                                 \
    size_t ws_bytes_fn(const hipt_clam_weights* w, int B, int64_t total_rows) { return clam_bags_ws_bytes(form, w, B, total_rows); }     \
    int forward(const hipt_clam_weights* w, const void* bags, const int64_t* offsets_dev, int B, int64_t total_rows, int attention_only, \
                float* A_raw, float* M, float* logits, float* Y_prob, int64_t* Y_hat, void* workspace, size_t ws_bytes, void* stream) {  \
        return clam_bags_forward(form, w, bags, offsets_dev, B, total_rows, attention_only, A_raw, M, logits, Y_prob, Y_hat, workspace,  \
                                 ws_bytes, stream);                                                                                      \
    }
HIPT_CLAM_BAGS_ENTRY(hipt_clam_sb_forward_bags, hipt_clam_bags_workspace_bytes, BAGS_SB)
HIPT_CLAM_BAGS_ENTRY(hipt_clam_sb_forward_bags_narrow, hipt_clam_narrow_bags_workspace_bytes, BAGS_NARROW)
HIPT_CLAM_BAGS_ENTRY(hipt_clam_sb_forward_bags_wide, hipt_clam_wide_bags_workspace_bytes, BAGS_WIDE)
HIPT_CLAM_BAGS_ENTRY(hipt_clam_mb_forward_bags, hipt_clam_mb_bags_workspace_bytes, BAGS_MB)
HIPT_CLAM_BAGS_ENTRY(hipt_clam_mb_forward_bags_wide, hipt_clam_mb_wide_bags_workspace_bytes, BAGS_MB_WIDE)
HIPT_CLAM_BAGS_ENTRY(hipt_clam_mb_forward_bags_many, hipt_clam_mb_many_bags_workspace_bytes, BAGS_MB_MANY)
#undef HIPT_CLAM_BAGS_ENTRY

// ---- max-pooling MIL over B bags (mil.hip): the unit table of the calls above | tile_start | one record per unit; no state ----
int hipt_mil_bags_supported(const hipt_mil_weights* w) {
    return w && (w->dtype == HIPT_F32 || w->dtype == HIPT_BF16) && hipt_mil_supported(w) ? 1 : 0;
}
struct MilBagsWs { void* units; int* tile_start; void* records; };
static MilBagsWs carve_mil_bags(Carver& c, int B, int64_t total_rows) {
    const size_t nu = (size_t)clam_bags_max_units(B, total_rows);
    MilBagsWs k;
    k.units = c.take(nu * hipt_clam_bags_unit_bytes());
    k.tile_start = c.take<int>((size_t)B + 1);
    k.records = c.take(nu * hipt_mil_record_bytes());
    return k;
}

size_t hipt_mil_bags_workspace_bytes(const hipt_mil_weights* w, int B, int64_t total_rows) {
    if (!hipt_mil_bags_supported(w) || B < 1 || total_rows < B || clam_bags_max_units(B, total_rows) > INT32_MAX) return 0;
    return dry_run([&](Carver& c) { carve_mil_bags(c, B, total_rows); });
}

int hipt_mil_forward_bags(const hipt_mil_weights* w, const void* bags, const int64_t* offsets_dev, int B, int64_t total_rows,
                          float* y_probs, int64_t* top_idx, float* top_logits, float* top_prob, int64_t* y_hat, float* top_features,
                          void* workspace, size_t ws_bytes, void* stream) {
    const char* name = "mil_forward_bags";
    HIPT_CHECK_ARG(w != nullptr, "%s: null weights", name);
    HIPT_CHECK_ARG(w->dtype == HIPT_F32 || w->dtype == HIPT_BF16, "%s: bad dtype %d", name, w->dtype);
    HIPT_CHECK_ARG(w->w1 && w->b1 && w->w2 && w->b2, "%s: null weight pointer", name);
    HIPT_CHECK_ARG(bags && offsets_dev && y_probs && top_idx && top_logits && top_prob && y_hat && workspace, "%s: null argument", name);
    HIPT_CHECK_ARG(((uintptr_t)bags & 15) == 0 && ((uintptr_t)w->w1 & 15) == 0 && ((uintptr_t)w->w2 & 15) == 0 && ((uintptr_t)w->b1 & 15) == 0 &&
                       (top_features == nullptr || ((uintptr_t)top_features & 15) == 0),
                   "%s: bags, w1, b1, w2 and top_features must be 16-byte aligned", name);
    HIPT_CHECK_ARG(B >= 1 && total_rows >= B, "%s: B = %d bags need at least one row each (total_rows = %lld)", name, B, (long long)total_rows);
    HIPT_CHECK_ARG(clam_bags_max_units(B, total_rows) <= INT32_MAX, "%s: %lld rows in %d bags exceed 2^31 tiles", name, (long long)total_rows, B);
    if (!hipt_mil_bags_supported(w)) {
        hipt_set_error("%s: [%d,%d] with %d classes (multi_class = %d) is outside the envelope: S1 in {256, 512}, S0 a multiple of 32 (fp32) / "
                       "64 (bf16), 2 <= classes <= 8, two classes unless multi_class", name, w->s0, w->s1, w->n_classes, w->multi_class);
        return HIPT_E_UNSUPPORTED;
    }
    Carver c(workspace, ws_bytes);
    const MilBagsWs k = carve_mil_bags(c, B, total_rows);
    if (check_workspace(c, name)) return HIPT_E_BADARG;  // as the CLAM multi-bag calls: a short buffer is a bad argument
    hipStream_t st = S(stream);
    const int nu = (int)clam_bags_max_units(B, total_rows);
    int rc;
    PROF(PC_OTHER, hipt_clam_bags_units_launch(offsets_dev, B, total_rows, nu, k.tile_start, k.units, st));
    PROF(PC_ABMIL, hipt_mil_tiles_combine_launch(w, bags, offsets_dev, B, k.units, k.tile_start, nu, y_probs, k.records, top_idx, top_logits,
                                                 top_prob, y_hat, top_features, st));
    return HIPT_OK;
}

int hipt_clam_mb_supported(const hipt_clam_weights* w) { return w && check_clam(w) == HIPT_OK && hipt_clam_mb_stream_supported(w) ? 1 : 0; }

// ticket | partials of <= 128 workgroups x 4 branches | h1 as a bf16 image
struct ClamMbWs { unsigned* ticket; float* partials; void* h1; };
static ClamMbWs carve_clam_mb(Carver& c, int N) {
    ClamMbWs k;
    k.ticket = (unsigned*)c.take(256);
    k.partials = (float*)c.take((size_t)128 * 4 * (4 + 128) * 4);
    k.h1 = c.take(hipt_clam_mb_h1_bytes(N > 0 ? N : 1));
    return k;
}

size_t hipt_clam_mb_workspace_bytes(const hipt_clam_weights* w, int N) { return dry_run([&](Carver& c) { carve_clam_mb(c, N); }); }

int hipt_clam_mb_forward(const hipt_clam_weights* w, const void* bag, int N, int attention_only, float* A_raw, float* M, float* logits, void* workspace,
                         size_t ws_bytes, void* stream) {
    int rc = check_clam(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(bag && A_raw && N > 0, "clam_mb_forward: null/empty bag (N=%d)", N);
    HIPT_CHECK_ARG(attention_only || (M && logits), "clam_mb_forward: null output");
    HIPT_CHECK_ARG(((uintptr_t)bag & 15) == 0, "clam_mb_forward: bag must be 16-byte aligned");
    if (!hipt_clam_mb_stream_supported(w)) {
        hipt_set_error("clam_mb_forward: no one-pass form for this configuration (bf16 [384|192,128,64], 2..4 branches = classes, stream_pk, bound < 60): "
                       "call hipt_clam_sb_forward per branch");
        return HIPT_E_UNSUPPORTED;
    }
    Carver c(workspace, ws_bytes);
    const ClamMbWs k = carve_clam_mb(c, N);
    if ((rc = check_workspace(c, "clam_mb_forward"))) return rc;
    hipStream_t st = S(stream);
    // (the two launches are booked apart: 'abmil_fused' = the streaming pass, 'abmil_combine' = the pooling pass)
    PROF(PC_ABMIL, hipt_clam_mb_stream_launch(w, bag, N, 1, A_raw, k.h1, k.partials, k.ticket, M, logits, st));  // (passes = 1: the streaming pass)
    if (!attention_only) PROF(PC_COMBINE, hipt_clam_mb_stream_launch(w, bag, N, 2, A_raw, k.h1, k.partials, k.ticket, M, logits, st));  // (passes = 2: the pooling pass)
    return HIPT_OK;
}

int hipt_attn_net_gated(const hipt_clam_weights* w, const void* x, int N, float* A, void* workspace, size_t ws_bytes,
                        void* stream) {
    int rc = check_clam(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(x && A && N > 0, "attn_net_gated: null/empty input");
    Carver c(workspace, ws_bytes);
    float* ab = (float*)c.take((size_t)N * 2 * w->s2 * 4);
    if ((rc = check_workspace(c, "attn_net_gated"))) return rc;
    return gated_scores(w, x, w->dtype, N, ab, nullptr, A, S(stream));
}

int hipt_clam_gather_h1(const hipt_clam_weights* w, const void* bag, const int64_t* idx, int n_idx, float* out, void* stream) {
    int rc = check_clam(w);
    if (rc) return rc;
    HIPT_CHECK_ARG(bag && idx && out && n_idx > 0, "clam_gather_h1: null/empty argument");
    return hipt_gather_h1_launch(w, bag, idx, n_idx, out, S(stream));
}

}  // extern "C"
