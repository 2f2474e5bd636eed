/*
 * hipt_abmil.h — C ABI of libhipt_abmil.so (gfx950 / MI355X).
 *
 * The reference (scjjb/HIPT_ABMIL_ATEC23) is pure Python on torch.nn; it has no native
 * boundary of its own.  This header is the boundary the build introduces UNDER the
 * reference's Python call surface: each entry point replaces the
 * stock-PyTorch op sequence of one reference function, cited per declaration as
 * file:line relative to the reference checkout.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch-allocated); the
 *     library allocates nothing persistent and keeps no state between calls;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*; NULL =
 *     the default stream) and returns immediately: no host synchronisation, no
 *     allocation, so calls may be captured into a hipGraph;
 *   - return value: HIPT_OK (0), or a negative HIPT_E_* code; the library never throws
 *     or aborts.  hipt_last_error() returns a static message for the calling thread;
 *   - `dtype` selects the arithmetic type of the GEMM operands: HIPT_F32 (exact fp32 MFMA,
 *     the reference's numerics, parity 1e-4) or HIPT_BF16 (bf16 operands, fp32 accumulate).
 *     LayerNorm statistics, softmax, biases, the residual stream and all outputs are fp32
 *     in both modes;
 *   - matrices are row-major; Linear weights keep torch's [out_features, in_features] layout.
 */
#ifndef HIPT_ABMIL_H
#define HIPT_ABMIL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 5 (round 6): the HIPT_PACK_MLP image of format 3 is 2*D*hidden*2 + D*D*2 bytes (six proj units in front: ask
 * hipt_vit_packed_bytes, never compute the size) and packing it reads blocks[i].proj_w, which must be set first;
 * hipt_vit_mlp_unit added; formats 1 / HIPT_MLP32 are gone.
 * 6: hipt_bootstrap_metrics added (nothing else changed).  The heat-map entry points (hipt_heatmap_workspace_bytes, _overlay,
 * _render), hipt_vit_cls_block_unit, hipt_score_counts and the hierarchical heat-map pair (hipt_hier_ranks, hipt_hier_render) and the
 * tiling pair (hipt_point_polygon_test, hipt_tile_contours), the resize pair, hipt_patch_render, the hipt_macenko_* five, the hipt_segment_* six and the hipt_contours_* three were added later under the same
 * number: additive, nothing existing changed.  hipt_vit_embed_unit likewise. */
#define HIPT_ABI_VERSION 6

enum { HIPT_F32 = 0, HIPT_BF16 = 1 };

enum {
    HIPT_OK = 0,
    HIPT_E_BADARG = -1,      /* shape / dtype / alignment the kernels do not support */
    HIPT_E_WORKSPACE = -2,   /* workspace too small */
    HIPT_E_LAUNCH = -3,      /* hipLaunch / hip runtime error (see hipt_last_error) */
    HIPT_E_UNSUPPORTED = -4  /* valid request outside the implemented envelope */
};

int hipt_abi_version(void);
const char* hipt_last_error(void);

/* Optional per-kernel timing for benchmarking (not part of the reference surface): when enabled,
 * every kernel launch of the calls below is bracketed by HIP events on the caller's stream.
 * hipt_profile_read() synchronises on them, returns total milliseconds and launch counts per
 * category (hipt_profile_categories() entries, named by hipt_profile_category_name) and resets.
 * Returns HIPT_E_WORKSPACE if more launches were issued than the event pool (8192) holds. */
int hipt_profile_enable(int on);
int hipt_profile_categories(void);
const char* hipt_profile_category_name(int i);
int hipt_profile_read(float* ms, int* counts);

/* ------------------------------------------------------------------------------------
 * Transformer block weights: Block / Attention / Mlp
 * (HIPT_4K/vision_transformer.py:88-152, duplicated HIPT_4K/vision_transformer4k.py:94-158).
 * GEMM matrices are in `dtype`; LayerNorm affine terms and all biases are fp32.
 * ---------------------------------------------------------------------------------- */
typedef struct hipt_block_weights {
    const float* ln1_w;  const float* ln1_b;    /* blocks.i.norm1.{weight,bias}      [D]     */
    const void*  qkv_w;  const float* qkv_b;    /* blocks.i.attn.qkv.{weight,bias}   [3D,D]  */
    const void*  proj_w; const float* proj_b;   /* blocks.i.attn.proj.{weight,bias}  [D,D]   */
    const float* ln2_w;  const float* ln2_b;    /* blocks.i.norm2.{weight,bias}      [D]     */
    const void*  fc1_w;  const float* fc1_b;    /* blocks.i.mlp.fc1.{weight,bias}    [Dh,D]  */
    const void*  fc2_w;  const float* fc2_b;    /* blocks.i.mlp.fc2.{weight,bias}    [D,Dh]  */
    /* Optional (NULL = absent) pre-packed images of the bf16 GEMM matrices, written by hipt_vit_pack_weights from the
     * matrices above: the same values in the byte order of the streaming kernels' LDS ring, so that a 1 KiB DMA piece is
     * one run of consecutive bytes instead of eight 128-byte row segments (2.4x the L2->LDS rate on MI355X).  They
     * are a cache of qkv_w / proj_w / fc1_w+fc2_w: re-pack after the weights change. */
    const void*  qkv_pk;  const void* proj_pk;  const void* mlp_pk;
    /* The image format of mlp_pk: the value hipt_vit_mlp_pack_format returned when it was packed (3 = the streaming kernel's
     * fragment image on 16x16x32 MFMAs behind six units of proj_w: what this version packs; 2 = the same without the proj
     * units, still run; 0 = no packed form for this shape). */
    int32_t      mlp_pk_fmt;
    /* HIPT_CLS_ABSORB_TAIL (exactly that value): the qkv_att_pk image is FOLLOWED, in the same allocation, by the
     * HIPT_PACK_CLS_ABSORB image (hipt_vit_packed_bytes(.., HIPT_PACK_CLS_ABSORB) more bytes, written by
     * hipt_vit_pack_weights(.., HIPT_PACK_CLS_ABSORB, ..) at qkv_att_pk + hipt_vit_packed_bytes(.., HIPT_PACK_QKV_ATT)).  Read for the
     * LAST block only: its [CLS]-pruned form then runs without the K / V projection (the K and V thirds of qkv_w absorbed into two
     * [CLS]-row GEMMs around one pass over the tokens).  Any other value (the field was `reserved` before; zero-initialise the
     * struct): that block projects K and V for every token, as before, and nothing is read behind the qkv_att_pk image. */
    int32_t      cls_absorb;
    /* Optional: qkv_w once more, head by head in the operand order of the fused QKV + attention kernel (HIPT_PACK_QKV_ATT;
     * ViT-256 shape only: D = 384, 6 heads of 64, 257 tokens).  NULL: LayerNorm-chained blocks run the QKV GEMM and the
     * attention as two kernels with the q|k|v tensor in HBM between them. */
    const void*  qkv_att_pk;
} hipt_block_weights;

#define HIPT_PACK_QKV  0
#define HIPT_PACK_PROJ 1
#define HIPT_PACK_MLP  2   /* fc1 and fc2 in one image, in the format hipt_vit_mlp_pack_format names */
#define HIPT_PACK_QKV_ATT 3
#define HIPT_PACK_CLS_ABSORB 4   /* lives behind the last block's HIPT_PACK_QKV_ATT image: hipt_block_weights.cls_absorb */
#define HIPT_CLS_ABSORB_TAIL 0x4B564142   /* hipt_block_weights.cls_absorb: "the tail image is there" (a tag, so that a stale non-zero value is not taken for it) */

/* One ViT (ViT-256 `vit_small` or ViT-4K `vit4k_xs`, or any width the classes are built with).
 * `pos` is the ALREADY INTERPOLATED positional table for this token grid
 * (interpolate_pos_encoding, vision_transformer.py:213-233): input independent, computed once
 * on the host side with the reference's exact F.interpolate call and cached. */
typedef struct hipt_vit_weights {
    int32_t dtype;        /* HIPT_F32 | HIPT_BF16 (type of embed_w and of the block GEMM matrices) */
    int32_t dim;          /* D: 384 (ViT-256) / 192 (ViT-4K); multiple of 32                        */
    int32_t depth;        /* number of blocks                                                     */
    int32_t heads;        /* D / heads must be 32 or 64                                           */
    int32_t hidden;       /* MLP hidden width (4*D)                                               */
    int32_t ntok;         /* tokens per sequence incl. [CLS] (257); <= 288                        */
    int32_t embed_k;      /* K of the embedding GEMM: 3*16*16 = 768 (ViT-256) / 384 (ViT-4K phi)   */
    float   ln_eps;       /* eps of every LayerNorm (1e-6 for vit_small / vit4k_xs)                 */
    float   attn_scale;   /* Attention.scale = qk_scale or head_dim ** -0.5 (vision_transformer.py:112);
                             <= 0 selects head_dim ** -0.5                                          */
    int32_t reserved;
    const void*  embed_w; /* patch_embed.proj.weight viewed [D, 768]  /  phi.0.weight [D, 384]     */
    const float* embed_b; /* patch_embed.proj.bias / phi.0.bias                                   */
    const float* cls;     /* cls_token [D]                                                        */
    const float* pos;     /* interpolated pos_embed [ntok, D]                                     */
    const float* norm_w;  const float* norm_b;     /* final norm                                  */
    const hipt_block_weights* blocks;              /* HOST array of `depth` entries               */
} hipt_vit_weights;

/* Where the 16x16-pixel tokens of sequence b live inside the input image tensor
 * (PatchEmbed Conv2d k16 s16, vision_transformer.py:155-170, fused with the
 * unfold/rearrange patchify of hipt_4k.py:64-65):
 *   pixel(b, c, y, x) = img[ (b / (grid_w*grid_h)) * batch_stride + c * chan_stride
 *                            + (((b / grid_h) % grid_w) * patch_h + y) * row_stride
 *                            + (b % grid_h) * patch_w + x ]
 * A plain batch [B,3,w,h]: grid 1x1, patch_h=w, patch_w=h, row_stride=h, chan_stride=w*h,
 * batch_stride=3*w*h.  A region [1,3,W,H] cut into 256x256 patches: grid (W/256)x(H/256),
 * patch 256x256, row_stride=H, chan_stride=W*H. */
typedef struct hipt_image_layout {
    int32_t grid_w, grid_h;      /* patch grid per batch item (w_256, h_256)       */
    int32_t patch_h, patch_w;    /* pixels per patch along dim2 / dim3 (multiples of 16) */
    int64_t row_stride, chan_stride, batch_stride; /* in elements                  */
} hipt_image_layout;

/* ---- fine-grained operators (also the units the parity tests exercise) ---- */

/* nn.LayerNorm(D, eps) over rows (vision_transformer.py:138,142,195).  x fp32 rows of D with
 * stride x_stride; out rows in out_dtype with stride out_stride.  D % 64 == 0, D <= 2048. */
int hipt_layernorm(const float* x, int64_t x_stride, const float* w, const float* b,
                   void* out, int out_dtype, int64_t out_stride, int rows, int D, float eps,
                   void* stream);

/* out = epilogue(A[M,K] @ W[N,K]^T + bias)  — nn.Linear (vision_transformer.py:93-95,114,116).
 * flags: bit0 GELU(erf) after bias, bit1 add fp32 residual `resid` (ld = ldc), bit2 output fp32
 * (else `dtype`), bit4 ReLU after bias.  A and W are `dtype`; K % (HIPT_F32 ? 32 : 64) == 0,
 * N % 4 == 0, 16-byte aligned rows. */
enum { HIPT_EPI_GELU = 1, HIPT_EPI_RESID = 2, HIPT_EPI_OUT_F32 = 4, HIPT_EPI_RELU = 16 };
int hipt_linear(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                const float* resid, void* out, int64_t ldc, int M, int N, int K, int dtype,
                int flags, void* stream);

/* Attention core of Attention.forward (vision_transformer.py:119-128): for each (b, head)
 * softmax(q k^T * scale) v with q,k,v read in place from the qkv projection output
 * qkv[B, ntok, 3, heads, dh] (`dtype`); out[B, ntok, heads*dh] (`dtype`).  If `probs` is not
 * NULL the [B, heads, ntok, ntok] fp32 softmax probabilities are also written (the tensor
 * Block.forward(return_attention=True) returns, :148-149).  dh in {32, 64}; ntok <= 288. */
int hipt_attention(const void* qkv, void* out, float* probs, int B, int ntok, int heads, int dh,
                   float scale, int dtype, void* stream);

/* ---- ViT forward (VisionTransformer.forward :248-253 / VisionTransformer4K.forward :241-246) ---- */

/* Bytes of scratch hipt_vit*_prepare_tokens / hipt_vit_blocks need for `nseq` sequences processed at
 * once (hipt_vit256_prepare_tokens additionally needs the bf16 copy of the image tensor in
 * HIPT_BF16 mode: + 2 bytes per image element it addresses). */
size_t hipt_vit_workspace_bytes(const hipt_vit_weights* w, int nseq);

/* Pre-packed weight images (hipt_block_weights.*_pk).  hipt_vit_packed_bytes: size of the image of matrix `what`
 * (HIPT_PACK_*) of one block, 0 when this dtype / shape has no packed form (then leave the pointer NULL).
 * hipt_vit_pack_weights: write the image of block `block` into `out` (device memory of that size) from w->blocks[block]
 * (HIPT_PACK_MLP: in the format w->blocks[block].mlp_pk_fmt names -- set it first, from hipt_vit_mlp_pack_format).
 * Done once per set of weights by the module that owns them (vision_transformer.py:_PackedVit here). */
size_t hipt_vit_packed_bytes(const hipt_vit_weights* w, int what);
/* The fused-MLP image format hipt_vit_pack_weights(.., HIPT_PACK_MLP, ..) writes for this model, to be stored in
 * hipt_block_weights.mlp_pk_fmt beside the pointer: 3 = the streaming kernel's fragment image on 16x16x32 MFMAs with six
 * units of the block's proj matrix in front (the attention block's output projection then runs at the head of the fused MLP's
 * tiles: LayerNorm-chained blocks have no proj launch and no y1 tensor; hipt_vit_packed_bytes(HIPT_PACK_MLP) includes them),
 * 0 = this dtype / shape has no packed form (the generic kernel reads the row-major matrices).  An image packed as format 2
 * (the same without the proj units) by an older binding still runs, with proj as its own kernel.  (1 was the 32x32x16 form
 * of ABI versions before round 5: an image in that format is no longer run -- its model takes the generic kernels.)
 * The BYTES of an image are private to the library build that wrote them (since late round 6 the fused-MLP image holds W1 / 8 and
 * 8 * W2, exact power-of-two scalings its kernel undoes): pack with the library that will run the image, never carry one across builds. */
int hipt_vit_mlp_pack_format(const hipt_vit_weights* w);
int hipt_vit_pack_weights(const hipt_vit_weights* w, int block, int what, void* out, void* stream);
/* Scratch of the whole-forward calls below (residual stream + block scratch + bf16 input copy). */
size_t hipt_vit256_forward_workspace_bytes(const hipt_vit_weights* w, const hipt_image_layout* lay,
                                           int nseq, int chunk);
size_t hipt_vit4k_forward_workspace_bytes(const hipt_vit_weights* w, int nseq);

/* prepare_tokens for ViT-256 (vision_transformer.py:235-246): patchify + Conv2d(3,D,16,16) +
 * [CLS] + positional table.  images: fp32, addressed through `lay`; x: fp32 [nseq, ntok, D]. */
int hipt_vit256_prepare_tokens(const hipt_vit_weights* w, const float* images,
                               const hipt_image_layout* lay, int seq0, int nseq, float* x,
                               void* workspace, size_t ws_bytes, void* stream);

/* prepare_tokens for ViT-4K (vision_transformer4k.py:223-239): phi = Linear(384,D)+GELU, [CLS],
 * positional table.  tokens_in: fp32 [nseq, ntok-1, embed_k] token-major
 * (= x.flatten(2,3).transpose(1,2)); x: fp32 [nseq, ntok, D]. */
int hipt_vit4k_prepare_tokens(const hipt_vit_weights* w, const float* tokens_in, int nseq, float* x,
                              void* workspace, size_t ws_bytes, void* stream);

/* Run blocks [blk_begin, blk_end) in place on x (Block.forward :146-152).  If probs != NULL the
 * last block of the range stops after its attention and only writes the probabilities
 * (get_last_selfattention :255-262); x then holds the input of that block. */
int hipt_vit_blocks(const hipt_vit_weights* w, float* x, int nseq, int blk_begin, int blk_end,
                    float* probs, void* workspace, size_t ws_bytes, void* stream);

/* The attention unit of ONE LayerNorm-chained ViT-256 block as the streaming path runs it (Attention.forward before proj,
 * vision_transformer.py:121-128), exposed for the parity tests: xn_img = LayerNorm-1(x) and out_img = the attention output,
 * both bf16 "activation images" of [nseq * 257, 384] (16-row fragments in MFMA operand order: element (row 16 F + i,
 * column 32 c + 8 g + e) at F * 6144 + c * 512 + (16 g + i) * 8 + e).  fused != 0: the QKV projection runs inside the
 * attention kernel (needs blocks[block].qkv_att_pk); fused == 0: QKV GEMM + attention kernel with q | k | v in the workspace
 * (needs blocks[block].qkv_pk).  bf16 ViT-256 shape only (D = 384, 6 heads, 257 tokens), nseq * 257 a multiple of 16.
 * workspace >= hipt_vit_workspace_bytes(w, nseq); out_img must not alias xn_img. */
int hipt_vit_attention_unit(const hipt_vit_weights* w, int block, const void* xn_img, int nseq, void* out_img, int fused,
                            void* workspace, size_t ws_bytes, void* stream);

/* The other half of a LayerNorm-chained ViT-256 block as the streaming path runs it, for per-kernel benches and parity tests:
 * x <- x + proj(att) + b_proj;  x <- x + fc2(GELU(fc1(LayerNorm-2(x))))  (Block.forward, vision_transformer.py:146-152 with Mlp.forward
 * :98-104) in ONE launch of the fused proj + MLP kernel.  x_img: the fp32 residual stream [nseq * 257, 384] as an activation image,
 * updated in place; att_img: the attention output (before proj) as a bf16 activation image (hipt_vit_attention_unit's out_img);
 * xn_out_img: NULL, or where LayerNorm-1 of block + 1 (of `block` itself for the last one) of the updated rows goes as a bf16 image
 * (may alias att_img: a workgroup loads all attention rows of its tile before it writes them).  Needs blocks[block].mlp_pk in format 3
 * (bf16, D = 384, hidden % 128 == 0), nseq * 257 a multiple of 16; workspace >= 256 bytes (the kernel's tile queue). */
int hipt_vit_mlp_unit(const hipt_vit_weights* w, int block, float* x_img, const void* att_img, int nseq, void* xn_out_img,
                      void* workspace, size_t ws_bytes, void* stream);

/* The [CLS]-pruned LAST block of a bf16 ViT-256 forward as that forward runs it (the launch sequence behind its chained blocks:
 * [CLS]-row gather, Q rows, u = q Wu^T, the pooling kernel, o = z Wo^T + bv, proj rows, the fused MLP on nseq rows), exposed for the
 * parity tests.  xn_img: LayerNorm-1 of the last block's input as a bf16 activation image [nseq * 257, 384]; x_img: the fp32 residual
 * stream as an activation image (only its [CLS] rows are read).  Neither is written.  xc_out [nseq, 384] fp32, row-major: the final
 * residual rows of the [CLS] tokens, before the final norm (hipt_vit_head with ntok = 1 strides finishes them).  att_out: NULL, or
 * [nseq, 384] bf16 row-major: the attention rows before proj.  The route is the forward's own: HIPT_NO_CLS_ABSORB=1 takes the fused
 * kernel's [CLS]-only form, HIPT_NO_FUSED_ATTN=1 the K | V GEMM + the one-query attention kernel (on a copy of xn_img in the
 * workspace).  HIPT_E_UNSUPPORTED outside bf16 / D = 384 / 6 heads / 257 tokens / nseq * 257 % 16 == 0, or when a forward of this
 * size would not prune its last block on activation images (HIPT_NO_PRUNE, HIPT_NO_IMG, HIPT_GENERIC).
 * workspace >= hipt_vit_workspace_bytes(w, nseq), 256-byte aligned. */
int hipt_vit_cls_block_unit(const hipt_vit_weights* w, const void* xn_img, const float* x_img, int nseq, float* xc_out, void* att_out,
                            void* workspace, size_t ws_bytes, void* stream);

/* The pixel-reading patch embedding of a bf16 ViT-256 forward as that forward runs it (prepare_tokens, vision_transformer.py:235-246:
 * patchify + Conv2d(3, 384, 16, 16) + bias + pos, the [CLS] rows = cls + pos[0]), exposed for the parity tests: the Conv2d weight is
 * packed into the workspace, then the embedding kernel and the [CLS]-row kernel are launched exactly as the forwards launch them.
 * images: sequences [seq0, seq0 + nseq) addressed through `lay`; input_kind 0: fp32, 1: uint8 planar [.., 3, W, H], 2: uint8
 * interleaved [.., W, H, 3] (ToTensor + Normalize(0.5, 0.5) in registers; strides of `lay` in pixels of one channel, as for
 * hipt_image_to_compute).  The images are not written.
 * xn_out_img == NULL: x_out [nseq, 257, 384] fp32 row-major (what hipt_vit256_prepare_tokens returns).
 * xn_out_img != NULL: x_out is the fp32 activation image of the [nseq * 257, 384] rows and xn_out_img the bf16 activation image of
 * LayerNorm-1 of block 0 applied to them (what the first block of a whole forward receives); needs nseq * 257 % 16 == 0.
 * HIPT_E_UNSUPPORTED wherever the forwards would not take this kernel: outside bf16 / D = 384 / 256 x 256 patches / 257 tokens, images
 * not 16-byte aligned, strides not multiples of 4 (uint8: of 8, and batch_stride == 3 * chan_stride), under HIPT_GENERIC=1, and for the
 * image outputs when nseq * 257 is not a multiple of 16.  Nothing is launched then.
 * workspace >= 590 080 bytes (12 x 48 KiB of packed weight + 256 for the kernel's tile queue), 256-byte aligned; HIPT_E_WORKSPACE
 * otherwise.  It need not be cleared between calls. */
int hipt_vit_embed_unit(const hipt_vit_weights* w, const void* images, int input_kind, const hipt_image_layout* lay, int seq0, int nseq,
                        float* x_out, void* xn_out_img, void* workspace, size_t ws_bytes, void* stream);

/* [CLS] row of the last block's attention map: probs_cls[nseq, heads, ntok] fp32 =
 * get_last_selfattention(x)[:, :, 0, :] (vision_transformer.py:255-262 as consumed by the heat-maps,
 * HIPT_4K/hipt_4k.py:143-158) without materialising [nseq, heads, ntok, ntok].  x = prepared tokens, modified.
 * Both compute dtypes, head dim 32 (ViT-4K) and 64 (ViT-256).  workspace >= hipt_vit_workspace_bytes(). */
int hipt_vit_cls_attention(const hipt_vit_weights* w, float* x, int nseq, float* probs_cls,
                           void* workspace, size_t ws_bytes, void* stream);

/* Final LayerNorm; cls_only=1 -> out[nseq, D] = norm(x)[:,0] (:252-253), else out[nseq, ntok, D]
 * (get_intermediate_layers :264-272). */
int hipt_vit_head(const hipt_vit_weights* w, const float* x, int nseq, int cls_only, float* out,
                  void* stream);

/* Whole ViT-256 forward over nseq patches in chunks of `chunk` sequences (chunk <= 0: library
 * default) -> out[nseq, D] fp32. */
int hipt_vit256_forward(const hipt_vit_weights* w, const float* images, const hipt_image_layout* lay,
                        int nseq, int chunk, float* out, void* workspace, size_t ws_bytes, void* stream);

/* The same in two steps, for callers that spread the patches of ONE call over several HIP streams (a batch-of-one region on
 * two streams: each stream's kernels fill the CUs the other's leave idle in their ragged last round of tiles):
 *   hipt_image_to_compute  the input tensor in the compute dtype (input_kind 0: fp32 [..,3,W,H]; 1: uint8 [..,3,W,H]; 2: uint8
 *                          interleaved [..,W,H,3], both normalised (x / 255 - 0.5) / 0.5) into dst
 *                          (hipt_image_compute_bytes(); 0 = fp32 input in fp32 mode: use the input where it lies);
 *   hipt_vit256_forward_range  ViT-256 over sequences [seq0, seq0 + nseq) of that tensor -> out[nseq, D]
 *                          (workspace >= hipt_vit256_range_workspace_bytes(w, nseq, chunk)). */
size_t hipt_image_compute_bytes(const hipt_vit_weights* w, const hipt_image_layout* lay, int nseq, int input_kind);
int hipt_image_to_compute(const hipt_vit_weights* w, const void* images, int input_kind, const hipt_image_layout* lay,
                          int nseq, void* dst, void* stream);
size_t hipt_vit256_range_workspace_bytes(const hipt_vit_weights* w, int nseq, int chunk);
int hipt_vit256_forward_range(const hipt_vit_weights* w, const void* images_cd, const hipt_image_layout* lay,
                              int seq0, int nseq, int chunk, float* out, void* workspace, size_t ws_bytes, void* stream);
/* The same straight from fp32 pixels, for models / layouts whose patch embedding reads them itself (bf16 ViT-256 on 256 x 256
 * patches): no compute-dtype copy of the image.  hipt_vit256_range_px_workspace_bytes returns 0 where that is not available
 * (then: hipt_image_to_compute + hipt_vit256_forward_range).
 * Bits: the pixel-reading embedding hands the first block LayerNorm-ed operands itself (bf16, whole 16-row fragments), which the embedding over a
 * compute-dtype copy does not -- hipt_vit256_forward_range_px gives the bits of hipt_vit256_forward / hipt_hipt4k_forward on the same pixels,
 * hipt_vit256_forward_range agrees with them to the bf16 bar only.  Split a call with the _px form (uint8 input: hipt_u8_normalize to fp32 first). */
size_t hipt_vit256_range_px_workspace_bytes(const hipt_vit_weights* w, const hipt_image_layout* lay, int nseq, int chunk);
int hipt_vit256_forward_range_px(const hipt_vit_weights* w, const float* images, const hipt_image_layout* lay, int seq0, int nseq,
                                 int chunk, float* out, void* workspace, size_t ws_bytes, void* stream);

/* Whole ViT-4K forward -> out[nseq, D] fp32. */
int hipt_vit4k_forward(const hipt_vit_weights* w, const float* tokens_in, int nseq, float* out,
                       void* workspace, size_t ws_bytes, void* stream);

/* HIPT_4K.forward (HIPT_4K/hipt_4k.py:48-76) for `nreg` regions already cropped to multiples of 256:
 * regions fp32 [nreg,3,W,H] -> cls256[nreg*w_256*h_256, 384] (kept on device, no CPU hop) -> out[nreg,192].
 * The reference processes one region per call (batch_size 1, hipt_4k.py:73); nreg > 1 is the throughput
 * form: regions are independent, so their patches are simply stacked along the sequence axis.
 * cls256_out may be NULL.  workspace >= hipt_hipt4k_workspace_bytes(). */
size_t hipt_hipt4k_workspace_bytes(const hipt_vit_weights* w256, const hipt_vit_weights* w4k,
                                   int nreg, int w_256, int h_256, int chunk);
int hipt_hipt4k_forward(const hipt_vit_weights* w256, const hipt_vit_weights* w4k,
                        const float* regions, int nreg, int W, int H, int chunk, float* cls256_out, float* out,
                        void* workspace, size_t ws_bytes, void* stream);

/* uint8 input (replaces eval_transforms = ToTensor + Normalize(0.5, 0.5),
 * HIPT_4K/hipt_model_utils.py:113-118, and the float H2D copy of extract_features_fp.py:166): regions are
 * uint8 [nreg, 3, W, H] (interleaved = 0) or [nreg, W, H, 3] (interleaved = 1, the layout of a decoded RGB
 * tile); they are normalised on device, (x / 255 - 0.5) / 0.5 in fp32 exactly as torchvision, into the compute
 * dtype.  Same outputs as hipt_hipt4k_forward on the normalised float tensor, bit for bit.
 * workspace >= hipt_hipt4k_u8_workspace_bytes(). */
size_t hipt_hipt4k_u8_workspace_bytes(const hipt_vit_weights* w256, const hipt_vit_weights* w4k,
                                      int nreg, int w_256, int h_256, int chunk);
int hipt_hipt4k_forward_u8(const hipt_vit_weights* w256, const hipt_vit_weights* w4k,
                           const uint8_t* regions, int interleaved, int nreg, int W, int H, int chunk,
                           float* cls256_out, float* out, void* workspace, size_t ws_bytes, void* stream);

/* The normalisation alone: src uint8 [n_images, 3, plane] or [n_images, plane, 3] -> dst [n_images, 3, plane]
 * in dst_dtype (HIPT_F32 / HIPT_BF16); plane = W*H must be a multiple of 16. */
int hipt_u8_normalize(const void* src, int interleaved, int64_t n_images, int64_t plane, void* dst,
                      int dst_dtype, void* stream);

/* ------------------------------------------------------------------------------------
 * CLAM_SB / ABMIL gated-attention pooling (models/model_clam.py:41-64, 77-191)
 * ---------------------------------------------------------------------------------- */
typedef struct hipt_clam_weights {
    int32_t dtype;            /* type of w1 / wab (and of the bag)                              */
    int32_t s0, s1, s2;       /* size_dict entry [S0,S1,S2] (model_clam.py:81)                  */
    int32_t n_classes;        /* bag classifier outputs                                         */
    int32_t n_att;            /* attention branches K: 0 / 1 = one (CLAM_SB; the field was `reserved` up to ABI 4); K > 1 = CLAM_MB
                                 (hipt_clam_mb_forward): wc = [K,S2], bc = [K], wcls = the K Linear(S1,1) stacked [K,S1], bcls = [K],
                                 n_classes = K, logit_bound = the largest of the K bounds */
    const void*  w1;  const float* b1;     /* attention_net.0: Linear(S0,S1) (+ReLU)  [S1,S0]     */
    const void*  wab; const float* bab;    /* attention_a.0 / attention_b.0 stacked [2*S2,S1]:
                                              rows [0,S2) = a, rows [S2,2*S2) = b; bias likewise */
    const float* wc;  const float* bc;     /* attention_c Linear(S2,1): [S2], [1]               */
    const float* wcls; const float* bcls;  /* classifiers Linear(S1,C): [C,S1], [C]             */
    float        logit_bound; /* optional (0 = unknown): an upper bound of |A_raw - bc| = sum_j |wc_j| (tanh * sigmoid lies in
                                 (-1, 1)), computed in fp32 by the owner of the weights; lets the streaming kernels exponentiate against
                                 the fixed shift bc + bound instead of a running maximum when the bound is small enough */
    int32_t      reserved2;
    const void*  stream_pk;   /* optional (NULL = absent): the weights as the LDS image of the streaming kernel (MFMA operand fragments
                                 of W1 and [Wa;Wb], biases and wc in accumulator order), written by hipt_clam_stream_pack into
                                 hipt_clam_stream_packed_bytes(w) bytes of device memory; bf16 [384|192,128,64] only.  With it (and a
                                 logit_bound < 60) hipt_clam_sb_forward is ONE launch of the streaming kernel; without it the
                                 general kernels run */
} hipt_clam_weights;

/* The streaming kernel's weight image (hipt_clam_weights.stream_pk): size in bytes (0: this shape / type has none) and the
 * packing launch (reads w1, b1, wab, bab, wc; `out` 256-byte aligned device memory).  Pack once per set of weights. */
size_t hipt_clam_stream_packed_bytes(const hipt_clam_weights* w);
int hipt_clam_stream_pack(const hipt_clam_weights* w, void* out, void* stream);

/* Scratch of the calls below.  ONE piece of state lives in it: the 256-byte "ticket block" at byte offset
 * hipt_clam_ticket_offset() (= 0: the head of the workspace, whatever the widths; the arrival counter of the in-kernel
 * combine).  It must be ZERO before the first call that uses a given workspace (zero it once when allocating) and every
 * completed call leaves it zero again -- no memset per call, any dispatch order, graph-replayable; no path of the library
 * writes anything else there, so one workspace may serve modules of different widths.  Calls that may run concurrently
 * (different streams) need different workspaces. */
size_t hipt_clam_workspace_bytes(const hipt_clam_weights* w, int N);
size_t hipt_clam_ticket_offset(const hipt_clam_weights* w, int N);

/* CLAM_SB.forward (model_clam.py:147-191, eval path without instance_eval), one bag:
 *   h1 = ReLU(bag W1^T + b1); A_raw = (tanh(h1 Wa^T+ba) * sigmoid(h1 Wb^T+bb)) wc + bc;
 *   M = softmax_N(A_raw) h1; logits = M Wcls^T + bcls; Y_prob = softmax(logits);
 *   Y_hat = argmax(logits) (int64, first maximum, as torch.topk(logits,1)).
 * bag: [N,S0] in w->dtype.  Outputs fp32: A_raw[N], M[S1], logits[C], Y_prob[C]; Y_hat int64[1].
 * attention_only != 0 skips pooling (only A_raw is written; model_clam.py:151-152). */
int hipt_clam_sb_forward(const hipt_clam_weights* w, const void* bag, int N, int attention_only,
                         float* A_raw, float* M, float* logits, float* Y_prob, int64_t* Y_hat,
                         void* workspace, size_t ws_bytes, void* stream);

/* CLAM forward over B bags in ONE call (the loop over slides of utils/eval_utils.py:115-179 and validate_clam).  The call exists in five
 * forms -- the mid-width gated heads, the narrow ones, the wide ones, the K branches of CLAM_MB at the mid and at the wide widths -- each with its own
 * <form>_supported, <form>_workspace_bytes and forward entry point of one signature.  What holds for all five is stated here, once; each form below lists only what differs.
 * bags: the bags' rows concatenated, [total_rows, S0] in w->dtype, 16-byte aligned; offsets_dev: int64[B + 1] in DEVICE memory, offsets[0] = 0,
 * increasing, offsets[B] = total_rows: bag b is rows [offsets[b], offsets[b+1]).  Every bag has at least one row.  The CONTENTS of the offsets
 * are the caller's responsibility (check them on the host before the upload); a bag whose offsets break the rules is left unwritten.
 * Outputs fp32 and Y_hat int64[B], per bag exactly the quantities of the per-bag call.  attention_only != 0: only A_raw is written (M ..
 * Y_hat may be NULL).
 * Three plain launches on `stream` (unit table from the offsets, 128-row tiles that never span two bags, one combine workgroup per bag): no
 * atomics, no waiting between workgroups, no host synchronisation or copy -- graph-capturable, and the workspace holds NO state (no ticket
 * block, nothing to zero).  A bag's outputs are bit for bit independent of the other bags in the call, of its position and of B.
 * <form>_supported(w) != 0: the configuration has this form; otherwise HIPT_E_UNSUPPORTED and <form>_workspace_bytes = 0: loop over the
 * per-bag call.  HIPT_E_BADARG -- before anything is launched or written -- for a null pointer, a misaligned `bags`, B < 1, total_rows < B,
 * and for a workspace smaller than <form>_workspace_bytes(w, B, total_rows) or not 256-byte aligned.
 *
 * The wide heads, CLAM_SB.forward per bag (hipt_clam_sb_forward): fp32 S1 in {128, 64, 32}, bf16 S1 in {128, 64}; S2 in {64, 32, 16}; S0 a
 * multiple of 32 (fp32) / 64 (bf16).  A_raw[total_rows], M[B, S1], logits[B, C], Y_prob[B, C]. */
int hipt_clam_bags_supported(const hipt_clam_weights* w);
size_t hipt_clam_bags_workspace_bytes(const hipt_clam_weights* w, int B, int64_t total_rows);
int hipt_clam_sb_forward_bags(const hipt_clam_weights* w, const void* bags, const int64_t* offsets_dev, int B, int64_t total_rows,
                              int attention_only, float* A_raw, float* M, float* logits, float* Y_prob, int64_t* Y_hat,
                              void* workspace, size_t ws_bytes, void* stream);

/* The NARROW gated heads, which the wide form does not take: (S1, S2) in {(8, 4), (16, 8), (32, 8), (32, 16)} in fp32 and in bf16, S0 a
 * multiple of 32 (fp32) / 64 (bf16) -- the reference's hipt_smallest [192, 8, 4] and hipt_smaller [192, 16, 8] among them.  Outputs as the
 * wide form; the same unit table and per-bag combine, the tile pass is a kernel of its own.  Rounding in bf16: the bag, W1, Wa and Wb are
 * bf16; h1, the gate and the pooling are fp32 (the model of hipt_clam_sb_forward for these widths).  fp32 (32, 16) is taken by both forms;
 * their results agree within fp32 rounding, not bit for bit. */
int hipt_clam_narrow_bags_supported(const hipt_clam_weights* w);
size_t hipt_clam_narrow_bags_workspace_bytes(const hipt_clam_weights* w, int B, int64_t total_rows);
int hipt_clam_sb_forward_bags_narrow(const hipt_clam_weights* w, const void* bags, const int64_t* offsets_dev, int B, int64_t total_rows,
                                     int attention_only, float* A_raw, float* M, float* logits, float* Y_prob, int64_t* Y_hat,
                                     void* workspace, size_t ws_bytes, void* stream);

/* The heads WIDER than the first form's (the reference's tiny, small, big and small_resnet18): (S1, S2) in {(256, 64), (512, 256), (512, 384)}
 * in fp32 and in bf16, S0 a multiple of 32 (fp32) / 64 (bf16).  Outputs as the first form; the same unit table and per-bag combine, the tile
 * pass is a kernel of its own that walks a 128-row unit as sub-tiles of 64 (bf16) / 32 (fp32) rows in a fixed order.  Rounding in bf16: the
 * bag, W1, Wa and Wb are bf16; h1 is rounded to bf16 as the gate GEMM's operand only; ab, the gate and the pooling (on unrounded h1) are
 * fp32 (the model of hipt_clam_sb_forward for these widths). */
int hipt_clam_wide_bags_supported(const hipt_clam_weights* w);
size_t hipt_clam_wide_bags_workspace_bytes(const hipt_clam_weights* w, int B, int64_t total_rows);
int hipt_clam_sb_forward_bags_wide(const hipt_clam_weights* w, const void* bags, const int64_t* offsets_dev, int B, int64_t total_rows,
                                   int attention_only, float* A_raw, float* M, float* logits, float* Y_prob, int64_t* Y_hat,
                                   void* workspace, size_t ws_bytes, void* stream);

/* CLAM_MB.forward (model_clam.py:226-264): the K = w->n_att attention branches of a hipt_clam_weights stacked as hipt_clam_mb_forward takes
 * it (wc [K, S2], bc [K], wcls [K, S1], bcls [K], n_classes = K; stream_pk and logit_bound are not read).  Supported: hipt_clam_bags_supported(w)
 * and 2 <= n_att <= 4 and n_att == n_classes.  K partials per work unit in the workspace.
 * A_raw [K, total_rows] -- branch k of row m at A_raw[k * total_rows + m], so bag b is the [K, N_b] window of columns
 * [offsets[b], offsets[b+1]) with row stride total_rows --, M [B, K, S1], logits [B, K] (logits[b, k] = wcls[k] . M[b, k] + bcls[k],
 * :248-250), Y_prob [B, K] = softmax over the K logits, Y_hat int64 [B] = their first maximum. */
int hipt_clam_mb_bags_supported(const hipt_clam_weights* w);
size_t hipt_clam_mb_bags_workspace_bytes(const hipt_clam_weights* w, int B, int64_t total_rows);
int hipt_clam_mb_forward_bags(const hipt_clam_weights* w, const void* bags, const int64_t* offsets_dev, int B, int64_t total_rows,
                              int attention_only, float* A_raw, float* M, float* logits, float* Y_prob, int64_t* Y_hat,
                              void* workspace, size_t ws_bytes, void* stream);

/* The same K-branch call for the heads WIDER than that form's (tiny, small -- what CLAM_MB() is built with by default --, big,
 * small_resnet18).  Supported: hipt_clam_wide_bags_supported(w) -- (S1, S2) in {(256, 64), (512, 256), (512, 384)}, fp32 and bf16, S0 a
 * multiple of 32 (fp32) / 64 (bf16) -- and 2 <= n_att <= 4 and n_att == n_classes.  Inputs, outputs and the K partials per work unit as
 * hipt_clam_mb_forward_bags; the same unit table and per-bag combine; the tile pass is the wide form's sub-tile walk (64 rows in bf16,
 * 32 in fp32, in a fixed order) with phase 1, the gate GEMM and tanh * sigmoid done once per sub-tile and K scores, K poolings and K
 * running records behind them.  Rounding per branch as the wide form: in bf16 the bag, W1, Wa and Wb are bf16 and h1 is rounded to bf16 as
 * the gate GEMM's operand only; the gate, the scores and the poolings (on unrounded h1) are fp32. */
int hipt_clam_mb_wide_bags_supported(const hipt_clam_weights* w);
size_t hipt_clam_mb_wide_bags_workspace_bytes(const hipt_clam_weights* w, int B, int64_t total_rows);
int hipt_clam_mb_forward_bags_wide(const hipt_clam_weights* w, const void* bags, const int64_t* offsets_dev, int B, int64_t total_rows,
                                   int attention_only, float* A_raw, float* M, float* logits, float* Y_prob, int64_t* Y_hat,
                                   void* workspace, size_t ws_bytes, void* stream);

/* The same K-branch call for MANY branches: 5 <= K <= 8 (the reference's ovarian_5class and wider tasks) at the widths of
 * hipt_clam_mb_forward_bags.  Supported: hipt_clam_bags_supported(w) and 5 <= n_att <= 8 and n_att == n_classes.  Inputs, outputs and the K
 * partials per work unit as hipt_clam_mb_forward_bags; the same unit table and per-bag combine; the tile pass is a kernel of its own that
 * walks the branches in groups of four behind one gate GEMM.  Every branch is computed operation for operation as that form computes a
 * branch: branch k of a call has the bits of the same branch in a hipt_clam_mb_forward_bags call on weights made of a subset of the
 * branches (logits[b, k] and M[b, k] included; Y_prob and Y_hat depend on all K logits). */
int hipt_clam_mb_many_bags_supported(const hipt_clam_weights* w);
size_t hipt_clam_mb_many_bags_workspace_bytes(const hipt_clam_weights* w, int B, int64_t total_rows);
int hipt_clam_mb_forward_bags_many(const hipt_clam_weights* w, const void* bags, const int64_t* offsets_dev, int B, int64_t total_rows,
                                   int attention_only, float* A_raw, float* M, float* logits, float* Y_prob, int64_t* Y_hat,
                                   void* workspace, size_t ws_bytes, void* stream);

/* CLAM_MB.forward (model_clam.py:226-264), inference, with ONE pass over the bag for all K = w->n_att attention branches (2 <= K <= 4; W1 and
 * [Wa; Wb] are shared by the branches, only wc / bc / the classifier rows differ):  A_raw[K, N] = the K logits of every row;
 * M[K, S1] = softmax_N(A_raw[k]) h1;  logits[K]: logits[k] = wcls[k] . M[k] + bcls[k] (:248-250; Y_prob / Y_hat are K numbers: the caller's).
 * Two launches: the streaming kernel (MFMA projections, gate once per row, K logits, h1 left in HBM as bf16) and a pooling kernel.
 * hipt_clam_mb_supported(w) != 0: this configuration has the one-pass form (bf16 [384 | 192, 128, 64], stream_pk packed with n_att = K,
 * logit_bound < 60); otherwise call hipt_clam_sb_forward once per branch.  attention_only != 0: A_raw only.
 * workspace >= hipt_clam_mb_workspace_bytes(w, N), 256-byte aligned, its first 256 bytes zero before the first use (the ticket block). */
int hipt_clam_mb_supported(const hipt_clam_weights* w);
size_t hipt_clam_mb_workspace_bytes(const hipt_clam_weights* w, int N);
int hipt_clam_mb_forward(const hipt_clam_weights* w, const void* bag, int N, int attention_only, float* A_raw, float* M, float* logits,
                         void* workspace, size_t ws_bytes, void* stream);

/* Attn_Net_Gated.forward (model_clam.py:59-64) on its own: A[N] from x[N,L]
 * (w->s1 = L, w->s2 = D; w1/b1/wcls unused). */
int hipt_attn_net_gated(const hipt_clam_weights* w, const void* x, int N, float* A,
                        void* workspace, size_t ws_bytes, void* stream);

/* inst_eval support (model_clam.py:116-145): h1 rows for `n_idx` selected instances,
 * out[n_idx, S1] fp32 = ReLU(bag[idx] W1^T + b1). */
int hipt_clam_gather_h1(const hipt_clam_weights* w, const void* bag, const int64_t* idx, int n_idx,
                        float* out, void* stream);

/* ------------------------------------------------------------------------------------
 * Max-pooling MIL baseline (models/model_mil.py: MIL_fc, MIL_fc_mc; main.py --model_type mil)
 * ---------------------------------------------------------------------------------- */
typedef struct hipt_mil_weights {
    int32_t dtype;            /* type of w1 (and of the bags)                                                    */
    int32_t s0, s1;           /* size_dict entry [S0, S1] (model_mil.py:11)                                      */
    int32_t n_classes;        /* C: 2 for MIL_fc, 3 .. 8 for MIL_fc_mc                                           */
    int32_t multi_class;      /* 0: MIL_fc (the row with the largest y_probs[:, 1]); 1: MIL_fc_mc (the first maximum of y_probs
                                 flattened to [N * C])                                                           */
    int32_t reserved;
    const void*  w1; const float* b1;   /* Linear(S0, S1) (+ReLU)  [S1, S0], [S1]                                */
    const float* w2; const float* b2;   /* MIL_fc: the Linear(S1, 2); MIL_fc_mc: the C Linear(S1, 1) stacked.  [C, S1], [C], fp32 in
                                           both dtypes, w2 16-byte aligned                                       */
} hipt_mil_weights;

/* MIL_fc.forward / MIL_fc_mc.forward (model_mil.py:26-43, :68-93; top_k = 1) over B ragged bags in ONE call; one bag is B = 1.
 *   h1 = ReLU(x W1^T + b1); logits = h1 W2^T + b2; y_probs = softmax_C(logits), per row;
 *   the selected row of a bag: MIL_fc -- the largest y_probs[:, 1]; MIL_fc_mc -- the first maximum of y_probs flattened to [N * C].
 *   Equal keys: the LOWEST row wins, then the lowest class (torch.topk leaves the order of equal values open; argmax takes the first).
 * bags, offsets_dev, B, total_rows: as hipt_clam_sb_forward_bags; every bag has at least one row.
 * Outputs: y_probs fp32 [total_rows, C]; per bag top_idx int64 [B] (bag-local row), top_logits fp32 [B, C] = logits of that row, top_prob
 * fp32 [B, C] = its row of y_probs, bit for bit; y_hat int64 [B] = the first maximum of top_logits; top_features fp32 [B, S1] = the row of
 * h1 (NULL: not written).  Rows outside a bag are never written.
 * Rounding: fp32 -- everything fp32.  bf16 -- the bags and W1 are bf16, the products accumulate in fp32, everything from + b1 on is fp32.
 * Three plain launches on `stream` (abmil_bags' unit table, the tile pass, one combine workgroup per bag which recomputes the selected row):
 * no atomics, no host synchronisation, graph-capturable, no state in the workspace.  A bag's outputs are bit for bit independent of the
 * other bags of the call, of its position, of B and of the grid.
 * hipt_mil_bags_supported(w) != 0: S1 in {256, 512}, S0 a positive multiple of 32 (fp32) / 64 (bf16), 2 <= C <= 8, C == 2 unless multi_class,
 * fp32 or bf16; otherwise HIPT_E_UNSUPPORTED and hipt_mil_bags_workspace_bytes = 0.  HIPT_E_BADARG -- before anything is launched -- for
 * a null pointer, misaligned bags or w2, B < 1, total_rows < B (an empty bag), a short or misaligned workspace. */
int hipt_mil_bags_supported(const hipt_mil_weights* w);
size_t hipt_mil_bags_workspace_bytes(const hipt_mil_weights* w, int B, int64_t total_rows);
int hipt_mil_forward_bags(const hipt_mil_weights* w, const void* bags, const int64_t* offsets_dev, int B, int64_t total_rows,
                          float* y_probs, int64_t* top_idx, float* top_logits, float* top_prob, int64_t* y_hat, float* top_features,
                          void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * CLAM training step: differentiable forward + backward of CLAM_SB.forward / CLAM_MB.forward
 * (models/model_clam.py:147-191, 226-264) with the instance branch's top-k (inst_eval / inst_eval_out, :116-145), as
 * driven by utils/core_utils.py:300-348 (train_loop_clam) and :373-426 (train_loop; loss.backward() at :423).
 * fp32 throughout (the reference's training precision).  A forward is two launches, a backward two.
 * ---------------------------------------------------------------------------------- */
typedef struct hipt_clam_train_weights {
    int32_t s0, s1, s2;       /* size_dict entry; each a multiple of 4 (every entry of the reference's table is)  */
    int32_t n_att;            /* K attention branches: 1 (CLAM_SB) or n_classes (CLAM_MB); <= 8                   */
    int32_t n_classes;        /* C <= 8                                                                           */
    int32_t multi_branch;     /* 0: logits = wcls[C,S1] M[0] + bcls (CLAM_SB :181); 1: logits[c] = wcls[c] . M[c] + bcls[c] (CLAM_MB :248-250) */
    const float* w1;  const float* b1;     /* attention_net.0                     [S1,S0], [S1] */
    const float* wa;  const float* ba;     /* attention_a.0                       [S2,S1], [S2] */
    const float* wb;  const float* bb;     /* attention_b.0                       [S2,S1], [S2] */
    const float* wc;  const float* bc;     /* attention_c                         [K,S2],  [K]  */
    const float* wcls; const float* bcls;  /* classifiers (CLAM_MB: the C Linear(S1,1) stacked) [C,S1], [C] */
} hipt_clam_train_weights;

typedef struct hipt_clam_train_grads {     /* outputs of the backward, same shapes as the weights; dbag may be NULL */
    float* dw1; float* db1; float* dwa; float* dba; float* dwb; float* dbb; float* dwc; float* dbc;
    float* dwcls; float* dbcls;
    float* dbag;                           /* [N,S0] or NULL (bags normally do not require a gradient)            */
} hipt_clam_train_grads;

size_t hipt_clam_train_workspace_bytes(const hipt_clam_train_weights* w, int N);   /* scratch of the backward */
/* 1 when the training kernels take this size_dict entry with K = n_att attention branches and C = n_classes (widths multiples
 * of 4, K and C <= 8, the row tiles of forward AND backward within the 160 KiB of LDS; need_dbag: the bag requires a
 * gradient too), else 0: the caller then keeps the PyTorch-op sequence ('big' [1024,512,384] with a bag gradient does not fit). */
int hipt_clam_train_shape_supported(int s0, int s1, int s2, int n_att, int n_classes, int need_dbag);

/* Forward.  bag [N,S0] fp32.  m1 [N,S1], ma / mb [N,S2]: dropout masks already scaled (0 or 1/(1-p)), or NULL
 * (nn.Dropout after the ReLU, :86-87, and inside Attn_Net_Gated, :48-52; the caller draws them).
 * Saved for the backward (caller-allocated): h1 [N,S1] (after ReLU and dropout = the `h` the reference returns),
 * t = tanh(.) and s = sigmoid(.) [N,S2] before dropout, A_raw [K,N], stats [K,2] = (max, sum exp) of the softmax over N,
 * M [K,S1].  Results: logits [C], Y_prob [C], Y_hat int64 [1].
 * k_sample > 0: topk_ids int64 [K,2,k_sample] = per branch the ids of the k largest and of the k smallest attention
 * scores (torch.topk(A, k) / torch.topk(-A, k), :120-123; ties: lowest index first), and, when h1_sel != NULL,
 * h1_sel [K,2,k_sample,S1] = those rows of h1 (index_select).  k_sample > N is an error, as in torch.topk. */
int hipt_clam_train_forward(const hipt_clam_train_weights* w, const float* bag, int N,
                            const float* m1, const float* ma, const float* mb,
                            float* h1, float* t, float* s, float* A_raw, float* stats, float* M,
                            float* logits, float* Y_prob, int64_t* Y_hat,
                            int k_sample, int64_t* topk_ids, float* h1_sel, void* stream);

/* Backward.  Incoming gradients: dlogits [C]; optional (NULL = zero) dA_raw [K,N] and dM [K,S1] (the 'features' output);
 * optional instance-branch rows: n_sel row ids sel_ids [n_sel] with their gradients dh1_sel [n_sel,S1], added to dh1.
 * Everything else is what the forward saved.  Writes every member of g.  workspace >= hipt_clam_train_workspace_bytes(). */
int hipt_clam_train_backward(const hipt_clam_train_weights* w, const float* bag, int N,
                             const float* m1, const float* ma, const float* mb,
                             const float* h1, const float* t, const float* s, const float* A_raw,
                             const float* stats, const float* M,
                             const float* dlogits, const float* dA_raw, const float* dM,
                             const int64_t* sel_ids, const float* dh1_sel, int n_sel,
                             const hipt_clam_train_grads* g, void* workspace, size_t ws_bytes, void* stream);

/* torch.topk(A, k) and torch.topk(-A, k) of every row of A [rows, N] on the device (inst_eval, :120-123):
 * ids int64 [rows, 2, k], descending / ascending by value, ties -> lowest index first.  One total order on fp32: -0.0 == +0.0, and a NaN
 * (either sign bit) ranks above +inf in BOTH lists, as in torch.topk, NaNs among themselves lowest index first.  Every id lies in [0, N)
 * whatever the values. */
int hipt_topk_rows(const float* A, int rows, int N, int k, int64_t* ids, void* stream);

/* hipt_topk_rows over the bags of a multi-bag call (the instance branch of validate_clam, one launch per call instead of one per slide).
 * A: the scores of hipt_clam_sb_forward_bags (K = 1, row_stride = total_rows) or hipt_clam_mb_forward_bags (K branches, row_stride =
 * total_rows): branch r of bag b is the offsets[b+1] - offsets[b] numbers at A + r * row_stride + offsets[b]; offsets_dev: int64 [B + 1] in
 * device memory.  ids int64 [B, K, 2, k]: for every bag and branch what hipt_topk_rows returns on that row alone (bag-local ids, the k
 * largest then the k smallest, ties -> lowest index first).  global_ids (may be NULL) int64 [B, K, 2, k]: the same ids plus offsets[b],
 * i.e. rows of the concatenated matrix, ready for hipt_clam_gather_h1.  One workgroup per (bag, branch).  A bag with fewer than k rows is
 * the caller's error (check the offsets on the host): every access stays in bounds and its ids are -1. */
int hipt_topk_segments(const float* A, int64_t row_stride, const int64_t* offsets_dev, int B, int K, int k, int64_t* ids,
                       int64_t* global_ids, void* stream);

/* ------------------------------------------------------------------------------------
 * Region augmentation (extract_features_fp.py:89-136, --use_transforms HIPT_*): uint8 RGB in, uint8 out, one parameter
 * record per region drawn by the caller.  Reproduces torchvision's PIL path: HFlip / VFlip, RandomAffine (Pillow AFFINE,
 * NEAREST, fill 0), ColorJitter (Pillow ImageEnhance blends, HSV hue shift) and GaussianBlur((1,3)).
 * ---------------------------------------------------------------------------------- */
enum { HIPT_AUG_HFLIP = 1, HIPT_AUG_VFLIP = 2, HIPT_AUG_AFFINE = 4, HIPT_AUG_BLUR = 8 };
enum { HIPT_AUG_BRIGHTNESS = 0, HIPT_AUG_CONTRAST = 1, HIPT_AUG_SATURATION = 2, HIPT_AUG_HUE = 3 };

typedef struct hipt_augment_params {
    double  affine[6];   /* Pillow AFFINE data (output pixel -> input pixel, width = cols), read when flags & HIPT_AUG_AFFINE */
    float   factor[3];   /* blend factors of brightness, contrast, saturation                                              */
    float   blur_w[3];   /* vertical 3-tap weights (row above, row, row below), read when flags & HIPT_AUG_BLUR              */
    int32_t flags;       /* HIPT_AUG_*; flips apply first (to the source), then the affine; BLUR is alone (the rest ignored)  */
    int32_t hue_shift;   /* added to Pillow's HSV hue modulo 256                                                             */
    int32_t n_ops;       /* colour ops applied, 0..4                                                                         */
    int32_t ops[4];      /* HIPT_AUG_BRIGHTNESS.. in application order                                                       */
    int32_t reserved;
} hipt_augment_params;

/* workspace of hipt_augment_regions: a uint64 luminance sum and two sampling tables per region */
size_t hipt_augment_workspace_bytes(int n, int rows, int cols);
/* src / dst uint8 [n,3,rows,cols] (interleaved = 0) or [n,rows,cols,3] (interleaved = 1), any rows x cols; params: n DEVICE
 * records; src and dst must not overlap.  A record that is the identity copies the bytes. */
int hipt_augment_regions(const uint8_t* src, int interleaved, int n, int rows, int cols, const hipt_augment_params* params,
                         uint8_t* dst, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Tensor-space region augmentation (extract_features_fp.py:63-82, --use_transforms all / spatial): uint8 RGB in, normalised
 * float32 out, one parameter record per region drawn by the caller.  The reference's Compose puts ToTensor first, so this is
 * torchvision's TENSOR path in float32: x = u8 / 255; HFlip / VFlip; RandomAffine as a normalised grid read
 * through grid_sample(nearest, zeros, align_corners=False); ColorJitter's float blends and float HSV hue shift (mean grey of the
 * whole region for contrast); (x - mean) / std.  Added under ABI 6: additive; hipt_augment_params is untouched.
 * flags: HIPT_AUG_HFLIP / _VFLIP / _AFFINE (flips act on the source, then the affine; BLUR is not read); ops: HIPT_AUG_BRIGHTNESS..
 * ---------------------------------------------------------------------------------- */
typedef struct hipt_tensor_augment_params {
    float   theta[6];    /* inverse affine matrix about the image centre (output -> input, centred pixel units), read when AFFINE */
    float   factor[3];   /* blend ratios of brightness, contrast, saturation                                                     */
    float   hue;         /* added to the HSV hue in [0, 1), modulo 1                                                             */
    int32_t flags;       /* HIPT_AUG_HFLIP | HIPT_AUG_VFLIP | HIPT_AUG_AFFINE                                                     */
    int32_t n_ops;       /* colour ops applied, 0..4                                                                             */
    int32_t ops[4];      /* HIPT_AUG_BRIGHTNESS.. in application order                                                           */
    float   mean[3];     /* Normalize: (x - mean) / std per channel                                                              */
    float   std[3];
    int32_t reserved[2]; /* pads the record to 96 bytes                                                                          */
} hipt_tensor_augment_params;

/* workspace of hipt_augment_tensor: one float64 partial sum of grey per workgroup of the summing pass (0 outside the envelope) */
size_t hipt_augment_tensor_workspace_bytes(int n, int rows, int cols);
/* src uint8 [n,3,rows,cols] (interleaved = 0) or [n,rows,cols,3] (interleaved = 1); dst float32 planar [n,3,rows,cols]; params: n
 * DEVICE records.  ws: hipt_augment_tensor_workspace_bytes(n, rows, cols) bytes, 256-byte aligned: two launches (sum, then finish).
 * ws NULL with ws_bytes 0 is the caller's statement that no record holds HIPT_AUG_CONTRAST: one launch, and a record that breaks
 * the statement has its region written as NaN.  HIPT_E_BADARG before any launch for a missing pointer, n < 1, rows cols < 1 or
 * > 2^30, params / dst not 4-byte aligned, src and dst overlapping; HIPT_E_WORKSPACE for a short or misaligned ws.  A region's
 * output depends on its own bytes and record only and is the same from run to run (fixed-order float64 sums, no atomics). */
int hipt_augment_tensor(const uint8_t* src, int interleaved, int n, int rows, int cols, const hipt_tensor_augment_params* params,
                        float* dst, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * ResNet-50 baseline feature extractor (models/resnet_custom.py:ResNet_Baseline, resnet50_baseline; the default route of
 * extract_features_fp.py:187,210-211): stem conv 7x7/2 + BN + ReLU, maxpool 3x3/2, layer1..layer3 of Bottleneck_Baseline
 * (stride on conv2), AdaptiveAvgPool2d(1) -> [n, 1024] fp32.  Eval-mode BatchNorm only (running statistics), folded into
 * the conv weights at pack time.  Activations between layers are NHWC in the compute dtype.
 * ---------------------------------------------------------------------------------- */
enum { HIPT_RESNET_IN_F32 = 0, HIPT_RESNET_IN_U8 = 1, HIPT_RESNET_IN_U8_HWC = 2 };

/* One Conv2d(bias=False) + BatchNorm2d pair: device fp32 tensors of torch's layouts (weight [cout, cin, kh, kw]). */
typedef struct hipt_conv_bn {
    const float* weight;
    const float* bn_weight;
    const float* bn_bias;
    const float* bn_mean;   /* running_mean */
    const float* bn_var;    /* running_var  */
    int32_t cout, cin, kh, kw;
    float   bn_eps;
    int32_t reserved;
} hipt_conv_bn;

/* The network: `convs` is a HOST array of n_convs records in state-dict order -- conv1/bn1, then per block conv1/bn1,
 * conv2/bn2, conv3/bn3 and, in the first block of a layer whose shape changes, downsample.0/downsample.1.
 * layers[]: blocks of layer1..layer3 (ResNet_Baseline's layers[0..2]; layers[3] is never built by the reference). */
typedef struct hipt_resnet_weights {
    int32_t dtype;          /* HIPT_F32 / HIPT_BF16: GEMM operands and stored activations */
    int32_t layers[3];
    const hipt_conv_bn* convs;
    int32_t n_convs;
    int32_t reserved;
} hipt_resnet_weights;

/* Bytes of the packed image (every conv's BN-folded weight in the compute dtype plus its fp32 bias); 0 if w is invalid. */
size_t hipt_resnet_packed_bytes(const hipt_resnet_weights* w);
/* Fill `packed` (256-byte aligned, hipt_resnet_packed_bytes) from w's tensors; enqueued on stream. */
int hipt_resnet_pack_weights(const hipt_resnet_weights* w, void* packed, void* stream);
size_t hipt_resnet_workspace_bytes(const hipt_resnet_weights* w, int n, int h, int wd);
/* out[n, 1024] fp32 = ResNet_Baseline.forward(x) for n images of h x wd pixels (h, wd multiples of 16, >= 32; else
 * HIPT_E_UNSUPPORTED).  input_kind HIPT_RESNET_IN_F32: x fp32 [n, 3, h, wd], already normalised (the reference's input);
 * HIPT_RESNET_IN_U8 / _U8_HWC: raw RGB bytes [n, 3, h, wd] / [n, h, wd, 3], normalised on the device as ToTensor +
 * Normalize, (x / 255 - mean_c) / std_c in fp32 (bit-identical to feeding the fp32 tensor torch computes from the same
 * bytes).  norm: HOST array {mean[3], std[3]}, NULL = ImageNet (0.485, 0.456, 0.406) / (0.229, 0.224, 0.225).
 * packed and workspace 256-byte aligned.  Every output row depends on its own image only (no cross-image reduction). */
int hipt_resnet_forward(const hipt_resnet_weights* w, const void* packed, const void* x, int input_kind, const float* norm,
                        int n, int h, int wd, float* out, void* workspace, size_t ws_bytes, void* stream);

/* The units, for tests and composition.  hipt_conv_bn_pack: one conv's BN fold into w_out [cout, kp] (compute dtype,
 * (ky, kx, ci) order, K = cin*kh*kw zero-padded to kp = multiple of 64 (bf16) / 32 (fp32); hipt_conv_bn_packed_bytes
 * gives cout*kp*element size) and bias_out [cout] fp32. */
size_t hipt_conv_bn_packed_bytes(const hipt_conv_bn* c, int dtype);
int hipt_conv_bn_pack(const hipt_conv_bn* c, int dtype, void* w_out, float* bias_out, void* stream);
/* out[n, oh, ow, cout] = relu?(conv(x[n, h, w, cin], w_packed) + bias (+ resid[n, oh, ow, cout])), NHWC, all tensors in
 * dtype except the fp32 bias; cout a multiple of 64; cin a multiple of 64 (bf16) / 32 (fp32), or cin*kh*kw <= 1024
 * (gathered, the stem's Cin = 3).  Padding taps read zeros.  16-byte aligned pointers. */
int hipt_conv2d(const void* x, int n, int h, int w, int cin, const void* w_packed, const float* bias, int cout, int kh, int kw,
                int stride, int pad, const void* resid, int relu, void* out, int dtype, void* stream);
/* MaxPool2d(3, 2, 1) on NHWC x[n, h, w, c] -> out[n, (h+1)/2, (w+1)/2, c]; c a multiple of 8 (bf16) / 4 (fp32). */
int hipt_resnet_maxpool(const void* x, int n, int h, int w, int c, void* out, int dtype, void* stream);
/* AdaptiveAvgPool2d(1) on NHWC x[n, hw, c] -> out[n, c] fp32, each sum in pixel order. */
int hipt_resnet_avgpool(const void* x, int n, int hw, int c, float* out, int dtype, void* stream);
/* hipt_conv2d with the output-pixel tile height chosen by the caller: tile_rows 128 (what hipt_conv2d and the ResNet-50
 * network launch), 64, or 0 for hipt_conv_tile_rows(n*oh*ow, cout).  One output element is accumulated in the same K
 * order under either height: the results are bit-identical, only the workgroup count differs. */
int hipt_conv2d_ex(const void* x, int n, int h, int w, int cin, const void* w_packed, const float* bias, int cout, int kh, int kw,
                   int stride, int pad, const void* resid, int relu, void* out, int dtype, int tile_rows, void* stream);
/* The tile rule of the BasicBlock network, a pure function of a conv's output pixels m and channels: 64 where 128-row
 * tiles give fewer workgroups than the chip has compute units (256) and 64-row tiles give more, else 128; 0 for a bad
 * argument (m < 1, cout not a multiple of 64).  The 256 is the MI355X's CU count, compiled in; the rule was measured on
 * 256 x 256 patches at batch 32 and 256 only. */
int hipt_conv_tile_rows(int64_t m, int cout);

/* ------------------------------------------------------------------------------------
 * BasicBlock ResNet feature extractor (torchvision's resnet18, what models/resnet_custom.py:resnet18_baseline builds;
 * extract_features_fp.py --model_type resnet18): stem conv 7x7/2 + BN + ReLU, maxpool 3x3/2, layer1..layer4 of BasicBlocks
 * (two 3x3 convs, the stride on conv1, a 1x1 downsample in block 0 of layers 2..4), AdaptiveAvgPool2d(1) -> [n, 512] fp32
 * (the fc layer is the caller's).  Same contract as the ResNet-50 entry points above: input kinds, norm, 256-byte
 * alignment, error codes, nothing launched on a refusal.
 * `convs`: HOST array in state-dict order -- conv1/bn1, then per block conv1/bn1, conv2/bn2 and, where present,
 * downsample.0/downsample.1.  layers[]: blocks of layer1..layer4; trailing zeros leave the later layers out, and out is
 * [n, 64 * 2^(L-1)] for the last built layer L.  tile_rows: 0 (the rule below) or 128 (128-row tiles on every conv: the
 * other side of the rule's A/B; the results do not change, only the speed); anything else is HIPT_E_BADARG.
 * ---------------------------------------------------------------------------------- */
typedef struct hipt_resnet_basic_weights {
    int32_t dtype;          /* HIPT_F32 / HIPT_BF16: GEMM operands and stored activations */
    int32_t layers[4];
    const hipt_conv_bn* convs;
    int32_t n_convs;
    int32_t tile_rows;      /* 0: hipt_conv_tile_rows picks each conv's tile height; 128: 128-row tiles on every conv */
} hipt_resnet_basic_weights;

size_t hipt_resnet_basic_packed_bytes(const hipt_resnet_basic_weights* w);   /* 0 if w is invalid */
int hipt_resnet_basic_pack_weights(const hipt_resnet_basic_weights* w, void* packed, void* stream);
/* 0 if w is invalid or the shape is one the forward refuses (n < 1, h or wd not a multiple of 32) */
size_t hipt_resnet_basic_workspace_bytes(const hipt_resnet_basic_weights* w, int n, int h, int wd);
/* h, wd multiples of 32 (every map down to layer4's is even), else HIPT_E_UNSUPPORTED.  Every output row depends on its
 * own image only: no split-K, no atomics, and the tile height (which follows the batch) changes no bit. */
int hipt_resnet_basic_forward(const hipt_resnet_basic_weights* w, const void* packed, const void* x, int input_kind, const float* norm,
                              int n, int h, int wd, float* out, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * DRAS-MIL attention-guided sampling (eval.py --sampling: utils/eval_utils.py:182-565 summary_sampling, helpers in
 * utils/sampling_utils.py:11-187): the two device pieces of a sampling round.
 * ---------------------------------------------------------------------------------- */
enum { HIPT_KNN_SPATIAL = 0, HIPT_KNN_TEXTURAL = 1 };
enum { HIPT_SAMPLING_MAX = 0, HIPT_SAMPLING_NEWEST = 1, HIPT_SAMPLING_AVERAGE = 2 };

/* Brute-force k nearest neighbours of S rows of the point set itself: replaces NearestNeighbors(n_neighbors=k,
 * algorithm='ball_tree').fit(X) and .kneighbors(X[sample_idxs]) (eval_utils.py:285,390-391,413).  Queries are the rows
 * q_idx int64 [S] of X.  Results: ids int64 [S, k] and dist [S, k], every row in ascending (squared distance, index) order --
 * a defined order, which sklearn's is not: a query's first neighbour is itself unless an identical point has a lower index.
 *   HIPT_KNN_SPATIAL:  X int32 [N, 2] (patch coordinates, |value| <= 2^30), D = 2; squared distances are 64-bit integers,
 *                      so the lists are exact; dist is float64 [S, k] = sqrt of that integer converted to float64.
 *   HIPT_KNN_TEXTURAL: X fp32 [N, D], D a multiple of 4 up to 2048, 16-byte aligned; the squared distance is the fp32 sum
 *                      over the features, in ascending order, of the squared fp32 difference (never the |a|^2+|b|^2-2ab
 *                      expansion); dist is fp32 [S, k] = its square root.
 * Envelope: 1 <= k <= 64, k <= N (else HIPT_E_BADARG, as sklearn raises), S <= 4096, N <= 2^20.  X is read from memory once
 * per 128 queries.  workspace: 256-byte aligned, hipt_knn_workspace_bytes.  Results are bitwise repeatable. */
size_t hipt_knn_workspace_bytes(int N, int S, int k);
int hipt_knn(const void* X, int kind, int N, int D, const int64_t* q_idx, int S, int k, int64_t* ids, void* dist,
             void* workspace, size_t ws_bytes, void* stream);

/* update_sampling_weights(..., normalise=False, repeats_allowed=False) of one round (sampling_utils.py:66-187), in place on
 * weights float64 [N].  scores fp32 [S] >= 0 (the softmaxed attention of the round's sample); ids int64 [S, k_stride], of
 * which the first `neighbors` columns of every row are used; all_sampled int64 [T].  Row i contributes scores[i] to every
 * target j in its prefix (ids outside [0, N) are ignored):
 *   HIPT_SAMPLING_MAX      new[j] = max_i scores[i];  weights[j] = max(weights[j], new[j] ** power)          (:125-172)
 *   HIPT_SAMPLING_NEWEST   the reference assigns new[j] and never uses it (:174-177): the weights are left alone
 *   HIPT_SAMPLING_AVERAGE  new[j] = new[j] > 0 ? (new[j] + scores[i]) / 2 : scores[i], folded over the contributions in
 *                          ascending (i, column); weights[j] = new[j] ** power where that is > 0 (an overwrite) (:77-88)
 * then weights[all_sampled] = 0 (:179-181).  All arithmetic is float64; the fold order and hence the result do not depend on
 * scheduling.  sum_out float64 [1] receives the sum of the updated weights, added in a fixed order.  power > 0.
 * workspace: 256-byte aligned, hipt_sampling_update_workspace_bytes. */
size_t hipt_sampling_update_workspace_bytes(int N);
int hipt_sampling_update(double* weights, int N, const float* scores, int S, const int64_t* ids, int k_stride, int neighbors,
                         const int64_t* all_sampled, int T, double power, int mode, double* sum_out, void* workspace,
                         size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Bootstrapped evaluation metrics (bootstrapping.py:78-102): for each of B resamples (with replacement) of n pooled
 * predictions, roc_auc_score / f1_score / accuracy_score / balanced_accuracy_score as exact ratios of integer counts
 * (DESIGN.md 13).  One workgroup per replicate; the per-replicate state (index histogram, prefix sums, labels: 9 n + 4
 * bytes) lives in LDS, which sets the limits:
 * ---------------------------------------------------------------------------------- */
#define HIPT_BOOTSTRAP_MAX_N 4096        /* pooled predictions per replicate */
#define HIPT_BOOTSTRAP_MAX_CLASSES 8     /* K */
#define HIPT_BOOTSTRAP_MAX_REPLICATES (1 << 20)   /* B of one call (one workgroup each); call again for more */
enum { HIPT_BOOTSTRAP_DEGENERATE = 1, HIPT_BOOTSTRAP_BAD_INPUT = 2 };   /* bits of *flags */

/* Y, Y_hat int32 [n]: class ids in 0..K-1.  C = 1 scored class for K = 2 (class 1: p_1 against Y == 1, as roc_auc_score
 * does for binary targets) and C = K for K > 2 (one-vs-rest, macro).  Scores do not cross this boundary; the host sorts them:
 *   order int32 [C, n]: order[c][p] = the sample at position p when the samples are sorted ascending by class c's score;
 *   tie   int32 [C, n]: tie[c][p] = lo | hi << 16, where [lo, hi) is the range of positions whose score equals that of
 *                       position p (its tie group; two scores tie when their float64 values are equal).
 * idx int32 [B, n]: the drawn sample indices of B replicates, each in 0..n-1.
 * out float64 [B, 4]: AUC (mean over the C classes of (2 #{pos > neg} + #{pos = neg}) / (2 P N)), F1 (class 1 for K = 2,
 * else the mean over classes of 2tp / (2tp + fp + fn), 0 where that denominator is 0), accuracy (trace / n) and balanced
 * accuracy (mean of tp / (tp + fn) over the classes that occur).  All counting is integer, every quotient is one correctly
 * rounded float64 division and the class means add in ascending class order, so a replicate's four values depend on its n
 * indices alone -- not on B, its position in the call or the launch geometry.
 * flags int32 [1]: the CALLER zeroes it; the call ORs in HIPT_BOOTSTRAP_DEGENERATE if some replicate leaves a scored class
 * without a positive or without a negative member (its AUC is written as NaN; sklearn raises there), and
 * HIPT_BOOTSTRAP_BAD_INPUT if a label, an index or an order entry lies outside its range (such an entry is never followed;
 * the results of the call are then meaningless).  Beyond the limits above the call returns HIPT_E_UNSUPPORTED and launches
 * nothing.  No workspace. */
int hipt_bootstrap_metrics(const int32_t* Y, const int32_t* Y_hat, const int32_t* order, const int32_t* tie, int n, int K,
                           const int32_t* idx, int B, double* out, int32_t* flags, void* stream);

/* ------------------------------------------------------------------------------------
 * Attention heat-map rasteriser (wsi_core/WholeSlideImage.py:576-684, visHeatmap with blur=False).
 * N patches of one size pw x ph (canvas pixels) at xy[i] = (x, y), the patch's top-left canvas pixel, carry one value v[i]:
 *   overlay[p] = (sum of v[i] over the patches covering pixel p, added in ASCENDING i, in float64) / count[p],
 *                rounded half to even when `binarize`; 0 where count[p] = 0;
 *   count[p]   = the number of covering patches (int32; the reference wraps a uint16);
 *   painted[p] = 1 if some covering patch has paint[i] != 0 (paint NULL: every patch paints).
 * Patches are clipped at the canvas edge; one that lies wholly outside covers nothing.  Pixels gather from per-tile candidate
 * lists (tiles of HIPT_HEATMAP_TILE_W x HIPT_HEATMAP_TILE_H pixels, binned on the device and put into ascending patch index);
 * there is no floating-point atomic, so the results are a function of the inputs alone, bit for bit what the numpy loops give.
 * A patch touches at most (ceil(pw / TILE_W) + 1) * (ceil(ph / TILE_H) + 1) tiles, which bounds the workspace from
 * N, pw, ph, w, h.  Envelope: w, h <= HIPT_HEATMAP_MAX_DIM and N times that tile bound < 2^31, else HIPT_E_UNSUPPORTED with
 * nothing launched.  N = 0 is legal (no workspace needed: the size function returns 0).
 * ---------------------------------------------------------------------------------- */
#define HIPT_HEATMAP_TILE_W 32
#define HIPT_HEATMAP_TILE_H 8
#define HIPT_HEATMAP_MAX_DIM (1 << 20)     /* canvas side in pixels */
#define HIPT_HEATMAP_LUT_ENTRIES 258       /* 256 colours, then the under and the over colour */

/* workspace: 256-byte aligned; 0 for N = 0 or a request outside the envelope. */
size_t hipt_heatmap_workspace_bytes(int N, int pw, int ph, int w, int h);

/* xy int32 [N, 2], v float64 [N], paint uint8 [N] or NULL; overlay float64 [h, w], count int32 [h, w], painted uint8 [h, w]:
 * each output may be NULL, not all three. */
int hipt_heatmap_overlay(const int32_t* xy, const double* v, const uint8_t* paint, int N, int pw, int ph, int w, int h,
                         int binarize, double* overlay, int32_t* count, uint8_t* painted, void* workspace, size_t ws_bytes,
                         void* stream);

/* The image of the same overlay.  Per pixel p, with base = canvas[p] (canvas uint8 [h, w, 3], NULL = white):
 *   colour = painted[p] and (mask NULL or mask[p] != 0; mask uint8 [h, w]) ? lut[index(overlay[p])] : base, where for
 *            t = overlay * 256: t < 0 -> entry 256 (under), t == 256 -> entry 255, t > 256 -> entry 257 (over), else trunc(t);
 *   img[p]  = alpha < 1 ? sat_u8(rint(float32(colour) * float32(alpha) + float32(base) * float32(1 - alpha))) : colour,
 * each product and the sum rounded to float32 on its own (no contraction), rint half to even: cv2.addWeighted's formula.
 * lut uint8 [HIPT_HEATMAP_LUT_ENTRIES, 3]; img uint8 [h, w, 3], 4-byte aligned, not the canvas; overlay float64 [h, w] or NULL. */
int hipt_heatmap_render(const int32_t* xy, const double* v, const uint8_t* paint, int N, int pw, int ph, int w, int h,
                        int binarize, const uint8_t* mask, const uint8_t* canvas, const uint8_t* lut, double alpha, uint8_t* img,
                        double* overlay, void* workspace, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Heat-map score ranks (wsi_core/wsi_utils.py:124-127 to_percentiles, vis_utils/heatmap_utils.py:22-24 score2percentile;
 * DESIGN.md 19).  For each of nq queries, against nref reference values (all float64, device pointers):
 *   less[i] = #{j : ref[j] < q[i]},  leq[i] = #{j : ref[j] <= q[i]}      (int32; IEEE comparisons: -0.0 == +0.0, +-inf order)
 *   pct[i]  = (0.5 * (less + leq + 1)) / nref * 100                      mode HIPT_PCT_RANKDATA: with q = ref this is
 *                                                                        scipy.stats.rankdata(ref, 'average') / len(ref) * 100
 *           = (less + leq + (less < leq)) * (50.0 / nref)                mode HIPT_PCT_OF_SCORE: scipy.stats.percentileofscore(ref, q)
 * in float64, every operation rounded on its own in the order written, so the values are bit for bit scipy's.  less, leq and
 * pct may each be NULL (not all three).  The counts come from brute force over the reference -- no sort, no atomic, no
 * workspace -- so a query's three results depend on q[i] and ref alone: not on nq, its position in q or the launch geometry.
 * One wave owns HIPT_PCT_QUERIES_PER_WG queries and walks the reference in LDS tiles of HIPT_PCT_REF_TILE values.
 * NaN in q or ref is a caller error (a NaN compares false both ways; the Python layer refuses it).  nq = 0 or nref = 0 returns
 * HIPT_OK and touches nothing; nref >= 2^31 (the counts are int32) is HIPT_E_UNSUPPORTED with nothing launched.  q may be ref.
 * ---------------------------------------------------------------------------------- */
enum { HIPT_PCT_RANKDATA = 0, HIPT_PCT_OF_SCORE = 1 };
#define HIPT_PCT_REF_TILE 512
#define HIPT_PCT_QUERIES_PER_WG 128
int hipt_score_counts(const double* q, int64_t nq, const double* ref, int64_t nref, int mode, int32_t* less, int32_t* leq,
                      double* pct, void* stream);

/* ------------------------------------------------------------------------------------
 * Hierarchical region attention heat-maps (HIPT_4K/hipt_heatmap_utils.py:347-485, HIPT_4K/hipt_4k.py:167-303).
 *
 * hipt_hier_ranks: x float32 [V, L] (device), pct float64 [V, L].  The reference upscales a map by f (nearest neighbour: every
 * value f * f times) and takes scipy.stats.rankdata(u) * 100 / len(u) of the upscaled values u.  With less = #{k : x[v,k] < x[v,i]}
 * and eq = #{k : x[v,k] == x[v,i]} (float32 comparisons, x[v,i] counts itself, -0.0 == +0.0) that is, at every copy of x[v,i],
 *   pct[v,i] = (less * f^2 + 0.5 * (eq * f^2 + 1)) * 100 / (L * f^2)
 * in float64 with the operations in that order: bit for bit scipy's value.  One workgroup per vector, the vector in LDS, brute
 * force: no sort, no atomic, no workspace.  Envelope 1 <= L <= HIPT_HIER_MAX_L, 1 <= f <= HIPT_HIER_MAX_UPSCALE, else
 * HIPT_E_UNSUPPORTED with nothing launched; V = 0 returns HIPT_OK.  NaN in x is a caller error.
 *
 * hipt_hier_render: every picture of one region in one pass over its pixels.
 *   pct4k  float64 [4, nh, w_256 * h_256]      the ranks (f = 256 / scale) of the ViT-4K maps of the region and its three shifted copies
 *   pct256 float64 [2, nh, w_256 * h_256, 256] the ranks (f = 16 / scale) of the ViT-256 maps of the region and its first shifted copy
 *   scale in {1, 2, 4, 8, 16}: b = 256 / scale pixels per patch, t = 16 / scale per token; the pictures are Hs = w_256 * b rows of
 *   Ws = h_256 * b pixels (the reference's naming: tensor dimension 2 is "w").  Layer l (offsets 0, off2, off3, off4, output pixels)
 *   is present at (y, x) iff y >= off_l and x >= off_l; its value is the percentile of token ((y - off_l) % b) / t, ((x - off_l) % b) / t
 *   (row major in 16) of patch ((y - off_l) / b) * h_256 + (x - off_l) / b; for the 4K level the patch is the token.  In float64,
 *   every operation rounded on its own:
 *     overlay4k = 100 * present layers;  score4k  = (v1 + v2 + v3 + v4) / overlay4k     (present layers, left to right)
 *     ov        = 100 * present of the first two;  score256 = (u1 + u2) / ov
 *     overlay256 = w256 * ov;  score = (score4k * overlay4k + score256 * overlay256) / (overlay4k + overlay256)
 *   colour = lut[min(trunc(score * lut_n), lut_n - 1)] (matplotlib's look-up in [0, 1]); pixel = the blend of hipt_heatmap_render,
 *   sat_u8(rint(float32(colour) * float32(alpha) + float32(base) * float32(1 - alpha))).
 *   hm4k [nh, Hs, Ws, 3] shows score4k of head j; hm256 [nh, Hs, Ws, 3] score256 of head i; hm_blend [npairs, Hs, Ws, 3] the blended
 *   score of the pairs (j, i) = pairs[k] (a HOST array int32 [npairs, 2], read before the call returns, each pair at most once;
 *   NULL: all nh * nh pairs, j major, and npairs is ignored); hm256_thr [nh, Hs, Ws, 3] (needs use_threshold): base where
 *   score256 < threshold, the blend of entry trunc(0.95 * lut_n) where it is above, and the uint8 wrapping sum of base and the blend
 *   of the threshold's own entry where it is equal (a threshold of exactly 0.95 counts as above).  Each output may be NULL, not all.
 * base uint8 [Hs, Ws, 3], lut uint8 [lut_n, 3]; base and the pictures 4-byte aligned, base none of the pictures.
 * Envelope: 1 <= nh <= HIPT_HIER_MAX_HEADS, 1 <= w_256 * h_256 <= HIPT_HIER_MAX_L, 2 <= lut_n <= HIPT_HIER_MAX_LUT, scale as
 * above, else HIPT_E_UNSUPPORTED with nothing launched.  One launch on `stream`, no workspace, no atomics, no host read-back.
 * ---------------------------------------------------------------------------------- */
#define HIPT_HIER_MAX_L 4096
#define HIPT_HIER_MAX_UPSCALE 256
#define HIPT_HIER_MAX_HEADS 8
#define HIPT_HIER_MAX_LUT 4096
int hipt_hier_ranks(const float* x, int V, int L, int f, double* pct, void* stream);
int hipt_hier_render(const double* pct4k, const double* pct256, int nh, int w_256, int h_256, int scale, int off2, int off3, int off4,
                     const uint8_t* base, const uint8_t* lut, int lut_n, double alpha, double w256, const int32_t* pairs, int npairs,
                     int use_threshold, double threshold, uint8_t* hm4k, uint8_t* hm256, uint8_t* hm_blend, uint8_t* hm256_thr,
                     void* stream);

/* ------------------------------------------------------------------------------------
 * Patch-level ViT-256 attention heat-maps (HIPT_4K/attention_visualization_utils.py:293-421 create_patch_heatmaps_indiv / _concat;
 * DESIGN.md 24), for a batch of P patches of 256 x 256 pixels in one launch.
 *   pct     float64 [P, 2, nh, 256]   hipt_hier_ranks (f = 16) of the [CLS] attention over the 16 x 16 tokens of each patch (layer 1)
 *                                     and of its copy shifted by 16 pixels (layer 2)
 *   patches uint8 [P, 256, 256, 3], lut uint8 [lut_n, 3]
 * At pixel (y, x) of a patch, in float64 with every operation rounded on its own: u1 = pct[p, 0, i, (y / 16) * 16 + x / 16];
 * layer 2 is present iff y >= offset and x >= offset, u2 = pct[p, 1, i, ((y - offset) / 16) * 16 + (x - offset) / 16];
 *   score = (u1 + u2) / 200 where layer 2 is present, u1 / 100 elsewhere           (0 <= offset <= 256; at 256 nothing overlaps)
 * hm shows score: colour = lut[min(trunc(score * lut_n), lut_n - 1)], pixel = the blend of hipt_hier_render with the patch.
 * hm_thr (needs use_threshold) is hipt_hier_render's hm256_thr rule on score: the patch where score < threshold, the blend of entry
 * trunc(0.95 * lut_n) where it is above, the uint8 wrapping sum of the patch and the blend of the threshold's own entry where equal.
 * cols == 0: an output is [P, nh, 256, 256, 3].  cols > 0: it is a mosaic [P, ceil(nh / cols) * 256, cols * 256, 3] with head i at
 * tile (i / cols, i % cols); the unused tiles of the last row are written 0.  Either output may be NULL, not both; they are 4-byte
 * aligned like patches, distinct, and neither is patches.
 * Envelope: P <= HIPT_PATCH_MAX_P, 1 <= nh <= HIPT_HIER_MAX_HEADS, 2 <= lut_n <= HIPT_HIER_MAX_LUT, else HIPT_E_UNSUPPORTED with nothing
 * launched; 0 <= cols <= HIPT_HIER_MAX_HEADS; P = 0 returns HIPT_OK.  One launch on `stream`, no workspace, no atomics, no host read-back.
 * ---------------------------------------------------------------------------------- */
#define HIPT_PATCH_MAX_P 1048576
int hipt_patch_render(const double* pct, const uint8_t* patches, int P, int nh, const uint8_t* lut, int lut_n, int offset, double alpha,
                      int use_threshold, double threshold, int cols, uint8_t* hm, uint8_t* hm_thr, void* stream);

/* ----------------------------------------------------------------------------------
 * Patch coordinates from tissue contours (wsi_core/WholeSlideImage.py:357-372, 415-506; wsi_core/util_classes.py:53-111;
 * DESIGN.md 21).  Integer geometry only: no floating point, no workspace, no atomics, no state between calls, one launch a call.
 *
 * Polygons are packed: verts int32 [V, 2] (x, y), poly_off int32 [P + 1] with polygon p = vertices poly_off[p] .. poly_off[p+1] - 1
 * (closed: the edge last -> first is part of it).  Points travel DOUBLED (2 * coordinate), so a half integer is an integer here;
 * the kernels double the vertices themselves.  Every doubled coordinate, vertex or point, must lie strictly inside
 * +-HIPT_TILING_COORD_BOUND: every difference then fits int32 and the edge function is two 32 x 32 -> 64 bit products.  The arrays
 * live on the device, so this bound is the CALLER's to keep (the Python layer refuses what breaks it); whatever the arrays hold,
 * no access leaves verts[0, V), poly_off[0, P], the point / unit / contour arrays or the output.
 *
 * The test of a point p against a polygon (cv2.pointPolygonTest(poly, p, False)):
 *    0   p lies on a closed edge segment;
 *   +1   otherwise, an odd number of edges cross the ray from p towards +x, an edge (a, b) counting when exactly one of
 *        a.y <= p.y, b.y <= p.y holds and its point at height p.y lies right of p;
 *   -1   otherwise.  A polygon of no vertices is -1 everywhere; one of 1 or 2 vertices is 0 on it and -1 elsewhere.
 *
 * hipt_point_polygon_test: points2 int32 [Q, 2] doubled, poly_id int32 [Q] in [0, P), out int8 [Q].  A workgroup of 256 points walks
 * every polygon one of its points names, the edges in chunks of HIPT_TILING_EDGE_CHUNK through LDS: points grouped by polygon
 * cost one walk a workgroup.  A point whose poly_id is outside [0, P) gets -1.  Q = 0 returns HIPT_OK.
 *
 * hipt_tile_contours: the keep-flag of every candidate patch of every contour of a slide.
 *   contours int32 [C, HIPT_TILING_CONTOUR_INTS]: poly_begin, poly_end (polygon poly_begin is the contour, the others up to
 *            poly_end - 1 its holes), start_x, start_y, step_x, step_y, nx, ny, keep_off.  Candidate i of the contour, 0 <= i <
 *            nx * ny, is the patch whose top-left corner is pt = (start_x + (i / ny) * step_x, start_y + (i % ny) * step_y), and
 *            its flag is keep[keep_off + i];
 *   units    int32 [U, 2]: (contour, first candidate) of a tile of HIPT_TILING_TILE consecutive candidates, one workgroup each;
 *            the caller lists the tiles it wants flags for (all of them: ceil(nx * ny / HIPT_TILING_TILE) per contour);
 *   mode, ref_patch_size (ps), shift: the points tested against the contour and the rule
 *            HIPT_TILE_BASIC          pt                                               in when the test is >= 0
 *            HIPT_TILE_CENTER         pt + ps / 2 (integer division)                    in when >= 0
 *            HIPT_TILE_FOUR_PT        (pt + ps / 2) -+ shift in x and in y: four points  in when ANY is >= 0
 *            HIPT_TILE_FOUR_PT_HARD   the same four points                             in when ALL are >= 0
 *            (shift = 0: the single centre point in both four-point modes);
 *   keep uint8 [keep_len]: 1 when the candidate is in and pt + ps / 2 (TRUE division: doubled, 2 * pt + ps) lies strictly inside
 *            (test > 0) none of the holes, else 0.  keep[keep_off + i] is written for the candidates of the listed tiles alone.
 * A contour whose polygon range is empty or whose nx, ny are not positive gets no flag written.  1 <= ps, 0 <= shift, both below
 * HIPT_TILING_COORD_BOUND / 4, else HIPT_E_UNSUPPORTED with nothing launched; U = 0 returns HIPT_OK.
 * ---------------------------------------------------------------------------------- */
enum { HIPT_TILE_BASIC = 0, HIPT_TILE_CENTER = 1, HIPT_TILE_FOUR_PT = 2, HIPT_TILE_FOUR_PT_HARD = 3 };
#define HIPT_TILING_COORD_BOUND 1073741824
#define HIPT_TILING_EDGE_CHUNK 1024
#define HIPT_TILING_TILE 256
#define HIPT_TILING_CONTOUR_INTS 9
int hipt_point_polygon_test(const int32_t* verts, int V, const int32_t* poly_off, int P, const int32_t* points2, const int32_t* poly_id,
                            int Q, int8_t* out, void* stream);
int hipt_tile_contours(const int32_t* verts, int V, const int32_t* poly_off, int P, const int32_t* contours, int C, const int32_t* units,
                       int U, int mode, int ref_patch_size, int shift, uint8_t* keep, int64_t keep_len, void* stream);

/* ----------------------------------------------------------------------------------
 * Pillow's Image.resize of 8-bit RGB images (HIPT_4K/hipt_heatmap_utils.py:385, HIPT_4K/hipt_4k.py:204, datasets/dataset_h5.py:92,202,
 * wsi_core/WholeSlideImage.py:690-694).  Integer arithmetic only; the results are Pillow's bytes.
 *
 * src uint8 [n, in_h, in_w, 3] -> dst uint8 [n, out_h, out_w, 3], interleaved RGB, contiguous, n >= 1; every image of a call shares
 * the geometry and the tables.  Pillow (ImagingResample, reducing_gap = None, no box) resizes in two separable passes, horizontal
 * first, and stores the intermediate image as uint8.  A pass along an axis from I to O samples is, per output xx and channel,
 *     out = clip((2^21 + sum_{x < xmax} in[xmin + x] * k[xx * ksize + x]) >> 22, 0, 255)         (int32, arithmetic shift)
 * with (xmin, xmax) = b[2 xx], b[2 xx + 1].  k (int32 [O, ksize]) and b (int32 [O, 2]) are DEVICE arrays the caller computes once per
 * (I, O, filter) on the host in doubles (precompute_coeffs + normalize_coeffs_8bpc; hipt_abmil_atec23_amd/resize.py: resize_table):
 * kx, bx, ksize_x for the width, ky, by, ksize_y for the height.  An axis whose length does not change is skipped, as Pillow skips
 * it (its table pointers may be NULL and are ignored); with both unchanged dst becomes a copy of src.  The caller guarantees
 * 255 * sum_x |k[xx, x]| + 2^21 < 2^31 for every row (true of Pillow's filters); the kernel clamps every (xmin, xmax) it reads to the
 * image and to its staged window, so a wrong table gives wrong pixels and no access outside src, dst, the tables or the workspace.
 *
 * Routes.  HIPT_RESIZE_FUSED: one launch; a workgroup runs the horizontal pass over the input rows its output tile's vertical taps
 * need, keeps them in LDS as uint8 (clipped exactly as the stored intermediate image) and runs the vertical pass out of LDS: the
 * input is read once, no intermediate image reaches memory, no workspace.  It takes calls that change both axes and whose tile fits
 * 64 KiB of LDS, else HIPT_E_UNSUPPORTED with nothing launched.  HIPT_RESIZE_GENERAL: one launch per changing axis (two, one or --
 * equal sizes, the copy -- one); with two, the intermediate image [n, in_h, out_w, 3] is carved from ws.  HIPT_RESIZE_AUTO: fused
 * where it applies, else general.  hipt_resize_workspace_bytes: the bytes ws must hold for a route -- 0 for FUSED and for calls that
 * change at most one axis; for AUTO the general route's need, since the choice also depends on the tap counts (0 too when the
 * geometry is outside the envelope: the call itself says why).  ws: 256-byte aligned (NULL with ws_bytes = 0 where nothing is needed).
 * Envelope: every side below 2^24, n * max(in_h, out_h) * max(in_w, out_w) * 3 below 2^40, ksize_x, ksize_y <= HIPT_RESIZE_MAX_KSIZE,
 * else HIPT_E_UNSUPPORTED with nothing launched.  src 16-byte aligned (rows are read as 16-byte vectors), dst and the tables 4-byte;
 * src != dst.  No atomics, no allocation, no host synchronisation: the launches can be captured into a graph.
 * ---------------------------------------------------------------------------------- */
enum { HIPT_RESIZE_AUTO = 0, HIPT_RESIZE_GENERAL = 1, HIPT_RESIZE_FUSED = 2 };
#define HIPT_RESIZE_MAX_KSIZE 512
size_t hipt_resize_workspace_bytes(int n, int in_h, int in_w, int out_h, int out_w, int route);
int hipt_resize_u8(const uint8_t* src, int n, int in_h, int in_w, int out_h, int out_w, const int32_t* kx, const int32_t* bx, int ksize_x,
                   const int32_t* ky, const int32_t* by, int ksize_y, uint8_t* dst, void* ws, size_t ws_bytes, int route, void* stream);

/* ----------------------------------------------------------------------------------
 * Macenko stain normalisation of 8-bit RGB images (extract_features_fp.py:41-60, --use_transforms macenko: torchstain's
 * MacenkoNormalizer, torch backend).  Added under ABI 6: additive.
 *
 * src: R images of h x w pixels, uint8, planar [R, 3, h, w] (interleaved = 0) or interleaved [R, h, w, 3], contiguous.  Per image:
 *   OD = -log((I + 1) / Io) (float32, a 256-entry table); tissue = the pixels with no channel OD < beta, n of them;
 *   E = the eigenvectors (e1, e2) of the two largest eigenvalues, ascending, of the unbiased covariance of OD over the tissue (sums and
 *       Jacobi in float64), each with its largest-magnitude component made positive;
 *   phi = atan2(OD . e2, OD . e1) over the tissue; minPhi, maxPhi = its order statistics of rank 1 + round_half_even(0.01 q (n - 1)),
 *       q = alpha and 100 - alpha -- exact order statistics (three histogram passes over the order-preserving integer image of the
 *       float32 key, -0.0 equal to +0.0), never an interpolation;
 *   vMin = E [cos minPhi, sin minPhi], vMax likewise; HE [3, 2] = [vMin, vMax] if vMin[0] > vMax[0], else [vMax, vMin];
 *   C [2] = (HE^T HE)^-1 HE^T OD for ALL pixels; maxC[j] = the order statistic of C[j] at q = 99 over the h w pixels;
 *   out = trunc(min(Io exp(-(ref_HE (C ref_maxC / maxC))), 255)).
 * status[r] (int32): 0, or 1 = fallback: n < 2, a non-finite entry of the covariance, HE or maxC, maxC[j] <= 0, or a select that
 * ended on an empty bin.  HE and maxC of a fallback image are written as zeros; apply copies its pixels through unchanged.  Nothing is
 * read back to decide it.  An image's HE, maxC, status and output bytes do not depend on R, on its place in the batch or on the
 * other images, and are the same from run to run (float64 sums in a fixed order, integer atomics only).
 *
 * hipt_macenko_fit: HE float32 [R, 3, 2], maxC float32 [R, 2], status int32 [R]; aux (NULL, or float32 [R, 16]) receives per image
 *   e1[3], e2[3], minPhi, maxPhi, the 2 x 3 matrix (HE^T HE)^-1 HE^T, then n and status as int32 bit patterns.
 * hipt_macenko_apply: the last line above for given HE / maxC / status (status NULL: all 0) and a target ref_HE float32 [3, 2] /
 *   ref_maxC float32 [2] on the device (NULL: torchstain's constants).  dst: uint8 in src's layout (dst_f32 = 0), or float32 planar
 *   [R, 3, h, w] equal to uint8 / 255 (dst_f32 = 1): the tensor the reference's route hands its model.  No workspace.
 * hipt_macenko_normalize: fit, then apply, on `stream`; HE / maxC / status may be NULL (they then live in the workspace).
 * hipt_macenko_keys: the float32 keys of every pixel as the passes compute them, for tests: keys [R, 3, h w] = phi, C[0], C[1] from
 *   aux's E and matrix, tissue uint8 [R, h w].
 * ws: hipt_macenko_workspace_bytes(R, h, w) bytes (0 for a geometry outside the envelope), 256-byte aligned; it holds the table,
 * 128 bytes, 16 KiB of histograms and at most 1024 slabs of 10 doubles per image -- nothing per pixel -- and carries nothing from
 * call to call.  HIPT_E_BADARG before any launch for R < 1, h w < 1, Io <= 0, alpha outside (0, 50), beta < 0, a missing pointer,
 * dst == src; HIPT_E_UNSUPPORTED for h w >= 2^31; HIPT_E_WORKSPACE for a short or misaligned ws.  16-byte aligned src / dst and
 * h w % 16 == 0 take the 16-byte loads and stores; anything else is read and written byte by byte, with the same results.
 * No allocation, no host synchronisation, no float atomics: the launches can be captured into a graph.
 * ---------------------------------------------------------------------------------- */
size_t hipt_macenko_workspace_bytes(int R, int h, int w);
int hipt_macenko_fit(const uint8_t* src, int interleaved, int R, int h, int w, double Io, double alpha, double beta, float* HE, float* maxC,
                     int32_t* status, float* aux, void* ws, size_t ws_bytes, void* stream);
int hipt_macenko_apply(const uint8_t* src, int interleaved, int R, int h, int w, double Io, const float* HE, const float* maxC,
                       const int32_t* status, const float* ref_HE, const float* ref_maxC, void* dst, int dst_f32, void* stream);
int hipt_macenko_normalize(const uint8_t* src, int interleaved, int R, int h, int w, double Io, double alpha, double beta,
                           const float* ref_HE, const float* ref_maxC, void* dst, int dst_f32, float* HE, float* maxC, int32_t* status,
                           void* ws, size_t ws_bytes, void* stream);
int hipt_macenko_keys(const uint8_t* src, int interleaved, int R, int h, int w, double Io, double beta, const float* aux, float* keys,
                      uint8_t* tissue, void* stream);

/* ----------------------------------------------------------------------------------
 * Tissue segmentation mask: the pixel stages of WholeSlideImage.segmentTissue (wsi_core/WholeSlideImage.py:111-203) up to the binary
 * mask.  Added under ABI 6: additive.  Contour tracing (cv2.findContours) is hipt_contours_* below.
 *
 * src: one uint8 image [h, w, channels], interleaved, channels 3 (RGB) or 4 (RGBA; the fourth channel is ignored).  Every plane below
 * is uint8 [h, w], contiguous.  The definitions, restated from OpenCV's published implementation:
 *   saturation  v = max(r, g, b), d = v - min(r, g, b), S = (d * sdiv[v] + 2048) >> 12; sdiv[0] = 0, sdiv[v] = rint(255 * 4096 / v)
 *   median      the exact median of the mthresh x mthresh window, indices clamped to the image; mthresh odd, 1 (a copy) ..
 *               HIPT_SEGMENT_MAX_MEDIAN
 *   Otsu        256 integer counts of the median plane; then, in float64 and in this order: scale = 1 / (h w), mu = (sum i hist[i]) scale;
 *               for i = 0 .. 255: p = hist[i] scale; mu1 *= q1; q1 += p; q2 = 1 - q1; skip i if min(q1, q2) < FLT_EPSILON or
 *               max(q1, q2) > 1 - FLT_EPSILON; mu1 = (mu1 + i p) / q1; mu2 = (mu - q1 mu1) / q2; sigma = q1 q2 (mu1 - mu2)^2; the first i
 *               with a strictly larger sigma is the threshold (0 if there is none)
 *   threshold   mask = med > t ? sthresh_up : 0; t = sthresh, or with use_otsu the value above, which never leaves the device
 *   closing     dilate, then erode, with a close x close rectangle, anchor close / 2: both read offsets -(close / 2) .. close - 1 -
 *               close / 2 on each axis; outside the image counts 0 for the dilation and 255 for the erosion; close = 0: no closing;
 *               close <= HIPT_SEGMENT_MAX_CLOSE and may exceed the image's sides
 * hipt_segment_mask: all of it on `stream`.  sat, med (planes) and thresh (int32 [1], the threshold used) may be NULL.
 * Stage entries: hipt_segment_saturation (src image -> sat); hipt_segment_median (src plane -> dst, window ksize);
 * hipt_segment_otsu (src plane -> hist int32 [256], thresh int32 [1]); hipt_segment_close (src plane -> dst; grey-scale, any bytes).
 * ws: hipt_segment_workspace_bytes(h, w, close) bytes (0 outside the envelope), 256-byte aligned: the histogram, the threshold, the
 * median plane and, for close > 0, two planes; hipt_segment_close takes the same size.  Nothing is carried from call to call.
 * HIPT_E_BADARG before any launch for a missing pointer, two buffers that are the same, h w < 1 or >= 2^31, channels not 3 / 4,
 * sthresh / sthresh_up outside 0 .. 255, mthresh < 1, close < 0; HIPT_E_UNSUPPORTED for an even mthresh, mthresh >
 * HIPT_SEGMENT_MAX_MEDIAN, close > HIPT_SEGMENT_MAX_CLOSE; HIPT_E_WORKSPACE for a short or misaligned ws.
 * No allocation, no host synchronisation, integer atomics only: the launches can be captured into a graph.
 * ---------------------------------------------------------------------------------- */
#define HIPT_SEGMENT_MAX_MEDIAN 15
#define HIPT_SEGMENT_MAX_CLOSE 128
size_t hipt_segment_workspace_bytes(int h, int w, int close);
int hipt_segment_mask(const uint8_t* src, int h, int w, int channels, int sthresh, int sthresh_up, int mthresh, int close, int use_otsu,
                      uint8_t* mask, uint8_t* sat, uint8_t* med, int32_t* thresh, void* ws, size_t ws_bytes, void* stream);
int hipt_segment_saturation(const uint8_t* src, int h, int w, int channels, uint8_t* sat, void* stream);
int hipt_segment_median(const uint8_t* src, int h, int w, int ksize, uint8_t* dst, void* stream);
int hipt_segment_otsu(const uint8_t* src, int h, int w, int32_t* hist, int32_t* thresh, void* stream);
int hipt_segment_close(const uint8_t* src, int h, int w, int close, uint8_t* dst, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------
 * Contour tracing: cv2.findContours(mask, RETR_CCOMP, CHAIN_APPROX_NONE) of a uint8 plane.  Added under ABI 6: additive.
 *
 * mask: uint8 [h, w], contiguous; any non-zero byte is foreground; the plane counts as surrounded by a one-pixel frame of zeros.
 * Suzuki-Abe border following, foreground 8-connected, background 4-connected: one OUTER border per foreground component, from its
 * raster-first pixel; one HOLE border per background component that does not reach the frame, from the foreground pixel west of the
 * hole's raster-first pixel.  The first search runs clockwise on screen from the west (outer) or east (hole) neighbour and finds the
 * border's LAST point; every later one runs counter-clockwise from just after the previous point; a point is listed once per visit.
 *
 * Two calls with ONE read-back of the caller's between them (the library itself never synchronises), so the pair cannot be
 * captured into a graph:
 *   hipt_contours_trace  labels, links and ranks every border on `stream` and writes `table`, int32 [1 + min(h w,
 *                        HIPT_CONTOURS_MAX_BORDERS), 4], 16-byte aligned: row 0 = {border pixels B, borders C, ranking passes run,
 *                        1 if the ranking did not settle}; row 1 + r, r < C, in raster order of the borders' root pixels =
 *                        {start pixel y w + x, kind (0 outer, 1 hole), number of points, for a hole the start pixel of the outer
 *                        border it lies on, else -1}.  A length of -1, or B / C above the room named below, means the request went
 *                        beyond the envelope: the caller must not go on to hipt_contours_emit.
 *   hipt_contours_emit   offsets int32 [n_borders]: where border r's points begin in the caller's order; n_borders = C, n_points = the
 *                        sum of the lengths; writes points int32 [n_points, 2] = (x, y), 8-byte aligned.  `ws` is the workspace the
 *                        trace call left, untouched in between.
 * Envelope: (h + 2) (w + 2) <= HIPT_CONTOURS_MAX_PLANE (8192 x 8192 is inside), so every pixel index fits 27 bits and every state
 * index (8 per border pixel) 31; room for min(h w, HIPT_CONTOURS_MAX_BORDER_PIXELS) border pixels and min(h w,
 * HIPT_CONTOURS_MAX_BORDERS) borders, which no plane of up to 2^22 pixels can exceed.
 * ws: hipt_contours_workspace_bytes(h, w) bytes (0 outside the envelope), 256-byte aligned.
 * HIPT_E_BADARG before any launch for a missing pointer, a misaligned table / offsets / points, h or w < 1, counts outside the room;
 * HIPT_E_UNSUPPORTED for a plane beyond the envelope; HIPT_E_WORKSPACE for a short or misaligned ws.
 * Integers only; the only read-modify-write atomics are the labelling's atomicMin, whose result (a component's minimum index) does not
 * depend on arrival order: the same mask gives the same bytes in every run.  No kernel follows a border point by point.
 * ---------------------------------------------------------------------------------- */
#define HIPT_CONTOURS_MAX_PLANE 134217728
#define HIPT_CONTOURS_MAX_BORDER_PIXELS 16777216
#define HIPT_CONTOURS_MAX_BORDERS 4194304
size_t hipt_contours_workspace_bytes(int h, int w);
int hipt_contours_trace(const uint8_t* mask, int h, int w, int32_t* table, void* ws, size_t ws_bytes, void* stream);
int hipt_contours_emit(int h, int w, const int32_t* table, const int32_t* offsets, int n_borders, int n_points, int32_t* points,
                       const void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------
 * Contour fill: the tissue mask of WholeSlideImage.get_seg_mask (wsi_core/WholeSlideImage.py:741-757), a sequence of
 * cv2.drawContours(..., thickness=-1) calls.  Added under ABI 6: additive.
 *
 * points int32 [n_points, 2] = (x, y), 8-byte aligned; poly_off int64 [n_polys + 1]: polygon p is points[poly_off[p] : poly_off[p + 1]],
 * closed (the edge from its last point to its first is its first edge).  collections int32 [n_collections,
 * HIPT_FILL_COLLECTION_INTS], in DRAW ORDER, each what one drawContours call fills: {first polygon, one past the last polygon, value
 * (0 / 1), y_min, y_max}; y_min .. y_max bound the rows the collection's scaled and moved points lie on -- a workgroup skips a
 * collection whose range misses its rows, so a range that is too narrow gives a wrong mask (never an access out of bounds) and
 * INT32_MIN .. INT32_MAX is always right.  All three live on the device.
 * A coordinate becomes (int)((double)p * scale) + off, converted toward zero: the reference's (cont * scale).astype(int32) and offset.
 * Per collection, for every polygon edge: (a) the 8-connected line between its end points (integer Bresenham, D = max(|dx|, |dy|),
 * d = min, x the major axis on a tie, err = D - 2 d, each step: err < 0 ? minor step, err += 2 D; err -= 2 d; walked from the end point
 * with the smaller x); (b) unless horizontal, an edge-table entry on the rows y_top <= y < y_bottom with x_fix = (x_top << 16) +
 * (y - y_top) * (((x_bottom - x_top) << 16) / (y_bottom - y_top)), the division truncating toward zero; per row the entries are
 * paired in sorted order and the columns (x_fix + 32768) >> 16 of a pair, both included, are filled.  The union of (a) and (b),
 * clipped to the canvas, takes the collection's value; later collections overwrite earlier ones.
 * mask: uint8 [h, w], contiguous, FULLY written with 0 / 1 (also with no collection at all).
 * coord_bound: the caller's bound on |x|, |y| of the points.  Envelope: h, w <= HIPT_FILL_MAX_DIM; n_points <= HIPT_FILL_MAX_POINTS;
 * coord_bound * max(|scale|) + max(|off|) <= HIPT_FILL_COORD_BOUND -- HIPT_E_UNSUPPORTED otherwise, nothing is clipped silently.  (The
 * kernel clamps every scaled coordinate to the bound, so a caller that declares less than it hands over gets a wrong mask, not a
 * fault.)  The crossing counters are 32 bits wide: no number of crossings on one pixel can wrap them.
 * max_cols: columns per pass, 0 = HIPT_FILL_MAX_COLS, else a multiple of 64 up to it; a wider canvas is filled in column chunks, each
 * counting the crossings left of it.  The mask does not depend on max_cols.
 * HIPT_E_BADARG before the launch for a missing or misaligned pointer, h or w < 1, negative counts, a NaN scale, a bad max_cols.
 * One launch on `stream`; no workspace, no allocation, no host synchronisation, no atomics on global memory (integer adds and ORs in
 * LDS only, which commute): the same input gives the same bytes in every run, and the launch can be captured into a graph.
 * ---------------------------------------------------------------------------------- */
#define HIPT_FILL_MAX_DIM 65535
#define HIPT_FILL_MAX_POINTS 134217728
#define HIPT_FILL_COORD_BOUND 1048576
#define HIPT_FILL_MAX_COLS 3072
#define HIPT_FILL_COLLECTION_INTS 5
int hipt_fill_contours(const int32_t* points, int64_t n_points, const int64_t* poly_off, int n_polys, const int32_t* collections,
                       int n_collections, double scale_x, double scale_y, int off_x, int off_y, int coord_bound, int h, int w, int max_cols,
                       uint8_t* mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HIPT_ABMIL_H */
