/* orn.h -- C ABI of liborn.so: the MI355X-native (gfx950) Online-RepNeRV training hot path.
 *
 * The reference (maoqingyu1996/Boosting-Neural-Video-Representation-via-Online-Structural-
 * Reparameteration) is pure Python and exposes no FFI; the interface it *does* expose for this path is
 * the Python surface of model.py / utils.py / main_train.py.  Each entry point below names the
 * reference call site it replaces (file:line, relative to the reference root).  The Python mirror
 * in boosting-..._amd/ binds these with ctypes (see INTEGRATION.md for the stub a reference
 * maintainer would add).
 *
 * Conventions
 *   - Every tensor argument is a raw DEVICE pointer (torch.Tensor.data_ptr()).  fp32, NCHW,
 *     contiguous, weights [O,C,kh,kw] exactly as PyTorch stores them.  The caller allocates every
 *     input, output and workspace and keeps them alive until the stream has drained.  No ownership
 *     is transferred; the library allocates no device memory.
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *     all work is enqueued there, nothing synchronises, every call is hipGraph-capturable.
 *   - Return value: 0 = success; < 0 = argument / shape error (text via orn_last_error);
 *     > 0 = hipError_t of a failed launch.  Nothing throws across the ABI, nothing calls exit().
 *   - All reductions are fixed-order two-pass trees: results are run-to-run bit-identical.
 *   - `ws` arguments are scratch; the required size comes from the matching *_ws_bytes().
 *   - One process drives ONE device (the deployment model of this path: one rank per GPU).  Kernels that need more than 64 KB
 *     of LDS raise their limit with hipFuncSetAttribute the first time they are launched and remember that in a process-wide
 *     flag; the attribute is per device, so a process that switches devices after its first call must not use this library
 *     on the second device.  Entry points may be called from several host threads as long as they use the same device
 *     (setting the attribute twice is harmless); orn_last_error is per thread.
 */
#ifndef ORN_H_
#define ORN_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORN_VERSION 120          /* 0.1.2: + orn_loss_target_stats*, orn_engine_set_target_stats (round 3); + orn_engine_decode_frames;
                                  * + orn_msssim_frames*, orn_engine_eval_frames*; + ORN_LOSS_SSIM .. ORN_LOSS_FUSION12, orn_loss_spec,
                                  * orn_loss_ws_bytes_for; + ORN_MAX_BATCH, orn_engine_batch_ws_bytes, orn_engine_set_batch_ws,
                                  * orn_engine_train_steps_batch; + orn_engine_step_forward, orn_engine_step_backward (the split step);
                                  * + orn_frames_ingest_u8, orn_frames_pool_f32 (K11: frames of any size); + orn_stem_bwd_ws_bytes;
                                  * + ORN_BRANCH_ACB / _REPVGG / _ECB, orn_branch_ptrs, orn_branch_merge_fwd / _bwd_ws_bytes / _bwd, and, appended
                                  * to orn_engine_desc, branch_kind + branch[] (N7: the paper's comparison blocks through an online merge);
                                  * + orn_engine_set_stage_targets / _stage_target_stats / _stage_stats and, appended to orn_engine_desc, multi_res + lw +
                                  * side_head_w[] / side_head_b[] (N8: a head and a loss at every stage); + ORN_ACT_SWISH / ORN_ACT_GELU, the *_act entry points and, appended to
                                  * orn_engine_desc, act (--act gelu); + orn_stage_out, orn_engine_eval_stages_ws_bytes, orn_engine_eval_stages (N9: decode and
                                  * evaluate any stage of a multi-resolution fit) */
/* Every entry point below is exported with default visibility; the library is built with -fvisibility=hidden, so these (and
 * the probe-only ones of orn_debug.h) are its whole dynamic symbol table. */
#define ORN_API __attribute__((visibility("default")))
#define ORN_MAX_LAYERS 8
/* --act: the activation behind every block's PixelShuffle and inside the stem (model.py:24-45).  swish = z sigmoid(z); gelu = nn.GELU()
 * without the tanh approximation, 0.5 z erfc(-z / sqrt 2).  Entry points named *_act take one of these as their last `int act`
 * (ORN_E_ARG for any other value); the entry points without it are the swish form. */
#define ORN_ACT_SWISH 0
#define ORN_ACT_GELU 1

#define ORN_OK 0
#define ORN_E_ARG (-1)           /* bad pointer / size / unsupported shape */
#define ORN_E_WS (-2)            /* workspace too small */
#define ORN_E_STATE (-3)         /* engine used in the wrong state */

ORN_API int orn_version(void);
/* Copies the last error text of the calling thread into buf (NUL-terminated); returns its length. */
ORN_API int orn_last_error(char *buf, size_t n);

/* ---- A1  PositionalEncoding.forward                                   utils.py:121-129 ------
 * out[b, 2i] = sin(arg), out[b, 2i+1] = cos(arg), arg = fp32(fp32(pos[b]*fp32(lbase^i))*fp32(pi)).
 * lbase_pow[i] = (float)(lbase**i) is computed by the caller in double (Python `lbase ** i`). */
ORN_API int orn_pe_fwd(const float *pos, int B, const float *lbase_pow, int levels, float *out, void *stream);

/* ---- A2  MLP stem (Linear+SiLU, Linear+SiLU)                         model.py:174-188,612 ----
 * pre1/h1: [B,Hd], pre2/h2: [B,Nout] (h2 is the block input viewed [B,C,fc_h,fc_w]). */
ORN_API int orn_stem_fwd(const float *embed, const float *w0, const float *b0, const float *w1, const float *b1,
                 int B, int E, int Hd, int Nout, float *pre1, float *h1, float *pre2, float *h2,
                 void *stream);
/* dh2 [B,Nout] -> dw0,db0,dw1,db1 (overwritten).  ws: orn_stem_bwd_ws_bytes(B, Hd, Nout) bytes, 4-byte aligned:
 * B*(Nout + 2*Hd) floats and max(256, ceil(Nout/16)) rows of B*Hd partial sums (at B == 1 the second layer's kernel leaves one
 * row per 16 outputs: more than 256 rows from Nout = 4097 on). */
ORN_API size_t orn_stem_bwd_ws_bytes(int B, int Hd, int Nout);
ORN_API int orn_stem_bwd(const float *embed, const float *w1, const float *pre1, const float *h1, const float *pre2,
                 const float *dh2, int B, int E, int Hd, int Nout, float *dw0, float *db0, float *dw1,
                 float *db1, float *ws, void *stream);

/* The same two with the activation of --act (ORN_ACT_*) in place of SiLU. */
ORN_API int orn_stem_fwd_act(const float *embed, const float *w0, const float *b0, const float *w1, const float *b1,
                 int B, int E, int Hd, int Nout, float *pre1, float *h1, float *pre2, float *h2,
                 void *stream, int act);
ORN_API int orn_stem_bwd_act(const float *embed, const float *w1, const float *pre1, const float *h1, const float *pre2,
                 const float *dh2, int B, int E, int Hd, int Nout, float *dw0, float *db0, float *dw1,
                 float *db1, float *ws, void *stream, int act);

/* ---- A3  NeRVBlock.get_equivalent_kernel_bias (online ERB merge)     model.py:450-516 --------
 * T[O,C,3,3] (kept for the backward), wf[O,C,3,3], bf[O].  Bit-exact against oracle/merge_ref.c:
 * both contractions are single k-ordered fmaf chains. */
ORN_API int orn_erb_merge_fwd(const float *w3x3, const float *b3x3, const float *w3x1, const float *b3x1,
                      const float *w1x3, const float *b1x3, const float *w1, const float *w2,
                      const float *w3, int C, int O, float *T, float *wf, float *bf, void *stream);
ORN_API size_t orn_erb_merge_bwd_ws_bytes(int C, int O);
/* g = dL/dwf [O,C,3,3], dbf = dL/dbf [O] -> gradients of the 9 branch tensors (overwritten). */
ORN_API int orn_erb_merge_bwd(const float *g, const float *dbf, const float *w1, const float *w2, const float *w3,
                      const float *T, int C, int O, float *d3x3, float *db3x3, float *d3x1, float *db3x1,
                      float *d1x3, float *db1x3, float *dw1, float *dw2, float *dw3, void *ws,
                      size_t ws_bytes, void *stream);

/* ---- N7  ACB / RepVGG / ECB blocks trained through an online merge    model.py:345-393, 541-565 ----
 * The reference trains these blocks as three to five convolutions summed on the activations.  Each is linear in its weights, so it
 * is trained here the way ERB is: merged to one 3x3 kernel every step (wf [O,C,3,3], bf [O]), which feeds the one conv of the block,
 * and dL/dwf is sent back through the merge.  Taps are (kh, kw) in 0..2, k = 3*kh + kw, centre k = 4.  All arithmetic is fp32.
 *   ACB     wf = (w3x3 + pad_h(w1x3)) + pad_w(w3x1);  bf = (b3x3 + b1x3) + b3x1
 *   RepVGG  wf = w3x3, plus w1x1 at the centre tap;   bf = b3x3 + b1x1
 *   ECB     wf = w3x3 + T + sum_t (scale_t * mask_t) * k0_t, terms added in the order written, t = sbx, sby, lpl;
 *           T[o,c,k] = sum_m wB[o,m,k] * wA[m,c], one m-ordered fmaf chain from 0;  bf = ((b3x3 + bias_sbx) + bias_sby) + bias_lpl.
 *           b0_t enters bf with the factor sum_k scale_t * mask_t[k], which is exactly 0 in fp32 for the Sobel and Laplacian masks: it
 *           is left out.  mask_t is read from memory like any other tensor (a state-dict tensor that is never trained).
 * Backward, g = dL/dwf, dbf = dL/dbf (fixed-order sums, no atomics, run-to-run bit-identical):
 *   d3x3 = g, every branch bias gets dbf;  ACB: d3x1[o,c,kh] = g[o,c,kh,1], d1x3[o,c,kw] = g[o,c,1,kw];  RepVGG: d1x1[o,c] = g[o,c,1,1];
 *   ECB: dwB[o,m,k] = sum_c g[o,c,k] * wA[m,c];  dwA[m,c] = sum_{o,k} wB[o,m,k] * g[o,c,k] (partial sums over slabs of 32 output
 *        channels, then the slabs in order);  with q_t[o,c] = sum_k mask_t[o,k] * g[o,c,k]:  dk0_t = scale_t * q_t,
 *        dscale_t[o] = sum_c k0_t[o,c] * q_t[o,c], dbias_t = dbf;  db0_t = 0 and dmask_t = 0 are WRITTEN, so that an optimiser over
 *        the whole arena never reads a stale value.
 * orn_branch_ptrs holds device pointers: the parameters (forward; backward reads wA, wB, k0, scale, mask) or, as the `grads`
 * argument of the backward, where each gradient goes (tensors of the same shapes).  Only the members of the given kind are read.
 * grads->w3x3 == g and grads->b3x3 == dbf are allowed (no copy then: the engine's dwf already lies in the 3x3 branch's slot). */
#define ORN_BRANCH_ACB 2
#define ORN_BRANCH_REPVGG 3
#define ORN_BRANCH_ECB 4
typedef struct orn_branch_ptrs {
    float *w3x3, *b3x3;                 /* [O,C,3,3], [O]: every kind */
    float *w3x1, *b3x1, *w1x3, *b1x3;   /* ACB: [O,C,3,1], [O], [O,C,1,3], [O] */
    float *w1x1, *b1x1;                 /* RepVGG: [O,C,1,1], [O] */
    float *wA, *wB;                     /* ECB: rbr_1x1_3x3_branch_1x1 [2C,C,1,1], rbr_1x1_3x3_branch_3x3 [O,2C,3,3] */
    struct { float *k0, *b0, *scale, *bias, *mask; } sb[3];   /* ECB: rbr_conv1x1_{sbx,sby,lpl}_branch: [O,C,1,1], [O], [O,1,1,1], [O], [O,1,3,3] */
} orn_branch_ptrs;
ORN_API int orn_branch_merge_fwd(int kind, const orn_branch_ptrs *p, int C, int O, float *wf, float *bf, void *stream);
ORN_API size_t orn_branch_merge_bwd_ws_bytes(int kind, int C, int O);       /* 0 on bad arguments (and 256 for the kinds that need none) */
ORN_API int orn_branch_merge_bwd(int kind, const orn_branch_ptrs *p, const float *g, const float *dbf, int C, int O,
                                 const orn_branch_ptrs *grads, void *ws, size_t ws_bytes, void *stream);

/* ---- A4  NeRVBlock.forward: conv3x3(pad 1)+bias -> PixelShuffle(s) -> SiLU   model.py:539,567 --
 * x [B,C,H,W]; wf [O,C,3,3]; bf [O]; O = Cn*s*s.  z (pre-activation, post-shuffle) and
 * a = SiLU(z): [B,Cn,H*s,W*s].  z may be NULL for inference (decode). */
ORN_API int orn_conv3x3_ps_silu_fwd(const float *x, const float *wf, const float *bf, int B, int C, int O, int H,
                            int W, int s, float *z, float *a, void *stream);
ORN_API size_t orn_conv3x3_ps_silu_bwd_ws_bytes(int B, int C, int O, int H, int W);
/* da [B,Cn,Hs,Ws] -> dx [B,C,H,W] (NULL to skip), dwf [O,C,3,3], dbf [O] (overwritten). */
ORN_API int orn_conv3x3_ps_silu_bwd(const float *x, const float *wf, const float *z, const float *da, int B, int C,
                            int O, int H, int W, int s, float *dx, float *dwf, float *dbf, void *ws,
                            size_t ws_bytes, void *stream);

/* The same two with the activation of --act (ORN_ACT_*): a = act(z), dy = unshuffle(da * act'(z)).  Same workspace. */
ORN_API int orn_conv3x3_ps_silu_fwd_act(const float *x, const float *wf, const float *bf, int B, int C, int O, int H,
                            int W, int s, float *z, float *a, void *stream, int act);
ORN_API int orn_conv3x3_ps_silu_bwd_act(const float *x, const float *wf, const float *z, const float *da, int B, int C,
                            int O, int H, int W, int s, float *dx, float *dwf, float *dbf, void *ws,
                            size_t ws_bytes, void *stream, int act);

/* ---- A4 on the bf16 MFMA path (fp32 accumulate): same contract as the two calls above for B = 1,
 * C <= 96 (zero-padded to 96 in the staging), O % 32 == 0, O % (s*s) == 0 and (O/(s*s)) % 8 == 0.  Inputs/outputs stay fp32 NCHW; the channels-last bf16
 * staging (DESIGN.md "data layout") lives in `ws`, which the caller must zero-fill once before the
 * first use (the one-pixel borders are never written).  The engine uses the same kernels without the
 * layout conversions.  fwd: `a` may be NULL (the last block's form: z only), then `z` must not be. */
ORN_API size_t orn_conv3x3_ps_silu_bf16_ws_bytes(int C, int O, int H, int W, int s);
ORN_API int orn_conv3x3_ps_silu_fwd_bf16(const float *x, const float *wf, const float *bf, int C, int O, int H, int W,
                                 int s, float *z, float *a, void *ws, size_t ws_bytes, void *stream);
ORN_API int orn_conv3x3_ps_silu_bwd_bf16(const float *x, const float *wf, const float *z, const float *da, int C, int O,
                                 int H, int W, int s, float *dx, float *dwf, float *dbf, void *ws,
                                 size_t ws_bytes, void *stream);

/* The forward conv kernel on the engine's own channels-last bf16 buffers (DESIGN.md "data layout"):
 * xpad [H+2][W+2][C] zero-bordered, wb [9][O'][C], bias_p [O'] (o' = (i*s+j)*Cn + n), z [H*s][W*s][Cn],
 * apad [H*s+2][W*s+2][Cn] or NULL.  C == 96; O % 32 == 0 and Cn % 8 == 0 (O % 96 == 0 for the two-work-group form the large
 * layers take; other O run the first form).
 * SLACK: the raw entry points of this group tile N by 96 or 128 channels and compute a ragged last tile on whatever lies behind
 * the operand (results of the missing channels are dropped, never stored).  When O % 128 != 0 the caller must therefore keep
 * `wb` / `wd` READABLE for 96*C elements past their [9][O'][C] / [9][C][O'] extent and `dypad` for 128 elements past its
 * [H+2][W+2][O'] extent (any finite or non-finite contents; never written).  The engine and the fp32-layout hooks above pad
 * their own workspaces; a caller that allocates exact sizes at e.g. O = 864 risks a fault at a page boundary. */
ORN_API int orn_conv_nhwc_bf16_fwd(const void *xpad, const void *wb, const float *bias_p, int H, int W, int C, int O,
                           int s, void *z, void *apad, void *stream);
/* the same kernel built for IEEE half (precision 2 of the engine, the mode bench.py's headline runs in): buffers hold fp16 */
ORN_API int orn_conv_nhwc_f16_fwd(const void *xpad, const void *wb, const float *bias_p, int H, int W, int C, int O,
                          int s, void *z, void *apad, void *stream);

/* Same for the two backward kernels (dgrad fused with SiLU' + un-shuffle into the previous layer's dypad;
 * wgrad + dbias into PyTorch-layout dwf [O][96][3][3], dbf [O]) (the timing-only ablation switch of
 * tools/probes lives in orn_debug.h). */
ORN_API int orn_dgrad_nhwc_bf16(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev,
                        void *dyprev, int sp, void *stream);
ORN_API size_t orn_wgrad_nhwc_bf16_ws_bytes(int H, int W, int O);
ORN_API int orn_wgrad_nhwc_bf16(const void *xpad, const void *dypad, int H, int W, int C, int O, int s, float *slabs,
                        float *dwf, float *dbf, void *stream);
/* IEEE-half twins of the two backward kernels and of the fp32-layout block hooks (same arguments, half buffers, same
 * workspace sizes): every 16-bit kernel the engine's fp16 mode launches can be checked per op against the oracle. */
ORN_API int orn_dgrad_nhwc_f16(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev,
                       void *dyprev, int sp, void *stream);
ORN_API int orn_wgrad_nhwc_f16(const void *xpad, const void *dypad, int H, int W, int C, int O, int s, float *slabs,
                       float *dwf, float *dbf, void *stream);
ORN_API int orn_conv3x3_ps_silu_fwd_f16(const float *x, const float *wf, const float *bf, int C, int O, int H, int W, int s,
                                float *z, float *a, void *ws, size_t ws_bytes, void *stream);
ORN_API int orn_conv3x3_ps_silu_bwd_f16(const float *x, const float *wf, const float *z, const float *da, int C, int O, int H,
                                int W, int s, float *dx, float *dwf, float *dbf, void *ws, size_t ws_bytes, void *stream);

/* The four fp32-layout block hooks of the 16-bit path with the activation of --act (ORN_ACT_*).  Same workspace. */
ORN_API int orn_conv3x3_ps_silu_fwd_bf16_act(const float *x, const float *wf, const float *bf, int C, int O, int H, int W,
                                 int s, float *z, float *a, void *ws, size_t ws_bytes, void *stream, int act);
ORN_API int orn_conv3x3_ps_silu_bwd_bf16_act(const float *x, const float *wf, const float *z, const float *da, int C, int O,
                                 int H, int W, int s, float *dx, float *dwf, float *dbf, void *ws,
                                 size_t ws_bytes, void *stream, int act);
ORN_API int orn_conv3x3_ps_silu_fwd_f16_act(const float *x, const float *wf, const float *bf, int C, int O, int H, int W, int s,
                                float *z, float *a, void *ws, size_t ws_bytes, void *stream, int act);
ORN_API int orn_conv3x3_ps_silu_bwd_f16_act(const float *x, const float *wf, const float *z, const float *da, int C, int O, int H,
                                int W, int s, float *dx, float *dwf, float *dbf, void *ws, size_t ws_bytes, void *stream, int act);

/* ---- A5  head: 1x1 conv -> (tanh+1)/2 or sigmoid                      model.py:621-622 --------
 * a [B,C,H,W]; w [3,C,1,1]; b [3]; out [B,3,H,W]. */
ORN_API int orn_head_fwd(const float *a, const float *w, const float *b, int B, int C, int H, int W, int sigmoid,
                 float *out, void *stream);
ORN_API size_t orn_head_bwd_ws_bytes(int B, int C, int H, int W);
ORN_API int orn_head_bwd(const float *a, const float *w, const float *out, const float *dout, int B, int C, int H,
                 int W, int sigmoid, float *da, float *dw, float *db, void *ws, size_t ws_bytes,
                 void *stream);

/* ---- A7 + A10  loss_fn (every loss but the two FFT ones) and psnr_fn   utils.py:139-199 ---------
 * pred/target [B,Ch,H,W].  stats (device, 8 floats):
 *   [0] loss  [1] mean|p-t|  [2] mean (p-t)^2  [3] ssim for the SSIM kinds, ms_ssim for the MS-SSIM kinds, else 0
 *   [4] psnr = -10 log10(mse)
 * dpred = dLoss/dpred * loss_scale (NULL: forward only).
 * Every id resolves through one table (orn_loss_spec) to loss = w_l1 * L1 + w_l2 * MSE + w_struct * (1 - s) with s = ssim
 * (kind ORN_LOSS_KIND_SSIM) or ms_ssim (ORN_LOSS_KIND_MSSSIM); the weights are those of utils.py:142-172.  Fusion13 / Fusion15
 * (FFT terms) are not built and have no id: such an objective -- any objective -- trains through the split step below
 * (orn_engine_step_forward / orn_engine_step_backward), which takes dLoss/dpred from the caller.
 *   kind SSIM: one launch, the 16x64-tile kernel of Fusion6 (80 KB of LDS) with other gradient weights; an L2 term takes the
 *     place of the L1 term at compile time.  Fusion7 / Fusion8 (kind NONE) are the plain L1 / L2 kernel with both terms.
 *   kind MSSSIM (min(H, W) > 160 and B*Ch <= 64, else ORN_E_ARG): 5 + 1 + 5 launches.  The five level launches of orn_msssim on the
 *     step's planes (pooled planes and per-tile partials stay in ws); one coefficient launch (level means, their product, the value
 *     of stats[3] -- bit-equal to orn_msssim on the same pair -- and per plane and level dLoss/d(level mean) / map size); then levels
 *     4..0 backwards: per 16x64 tile the filtered maps are recomputed in LDS, the derivative maps of the CS map (levels 0..3) or the
 *     SSIM map (level 4) go through the adjoint 11-tap filter, and the 2x2 average pool's adjoint of the level above is added.  Level
 *     0 adds the L1 / L2 term and writes dpred.  No atomics, fixed-order sums. */
#define ORN_LOSS_L2 0
#define ORN_LOSS_L1 1
#define ORN_LOSS_FUSION6 2
#define ORN_LOSS_SSIM 3
#define ORN_LOSS_FUSION1 4
#define ORN_LOSS_FUSION2 5
#define ORN_LOSS_FUSION3 6
#define ORN_LOSS_FUSION4 7
#define ORN_LOSS_FUSION5 8
#define ORN_LOSS_FUSION7 9
#define ORN_LOSS_FUSION8 10
#define ORN_LOSS_FUSION9 11
#define ORN_LOSS_FUSION10 12
#define ORN_LOSS_FUSION11 13
#define ORN_LOSS_FUSION12 14
#define ORN_LOSS_COUNT 15
#define ORN_LOSS_KIND_NONE 0
#define ORN_LOSS_KIND_SSIM 1
#define ORN_LOSS_KIND_MSSSIM 2
/* weights3 (host) = {w_l1, w_l2, w_struct}, *kind = ORN_LOSS_KIND_*; ORN_E_ARG for an id that is not built. */
ORN_API int orn_loss_spec(int loss_type, float *weights3, int *kind);
/* orn_loss_ws_bytes: the workspace of ids 0..2 and of every kind but MSSSIM.  orn_loss_ws_bytes_for: the workspace of any id (the
 * same number for those; the MS-SSIM kinds add both pyramids, the level gradients and the coefficients); 0 for an unknown id and
 * for an MS-SSIM id with min(H, W) <= 160 or B*Ch > 64.  orn_loss_fwd_bwd checks ws_bytes against the latter. */
ORN_API size_t orn_loss_ws_bytes(int B, int Ch, int H, int W);
ORN_API size_t orn_loss_ws_bytes_for(int loss_type, int B, int Ch, int H, int W);
ORN_API int orn_loss_fwd_bwd(const float *pred, const float *target, int B, int Ch, int H, int W, int loss_type,
                     float loss_scale, float *stats, float *dpred, void *ws, size_t ws_bytes, void *stream);
/* SSIM kinds (SSIM, Fusion1-6, Fusion9), engine only: the TARGET side of the SSIM statistics (utils.py:160 -> pytorch_msssim ssim: the 11-tap Gaussian of
 * t and of t*t on the valid map) of `n` resident frames [n][Ch][H][W] -> out [n][2][Ch][H-10][W-10] (orn_loss_target_stats_bytes).
 * A video's frames never change during its fit, so the engine can be handed this table once (orn_engine_set_target_stats) and
 * its steps then filter three maps (p, p*p, p*t) instead of five; same taps and fmaf order as the in-step form: results are
 * bit-identical with and without it. */
ORN_API size_t orn_loss_target_stats_bytes(int n, int Ch, int H, int W);
ORN_API int orn_loss_target_stats(const float *frames, int n, int Ch, int H, int W, float *out, void *stream);

/* ---- N3  msssim_fn: pytorch_msssim.ms_ssim(pred, target, data_range=1, size_average=True)   utils.py:201-211
 * Logging metric of the reference's train/eval loops (main_train.py:254).  out: one device float, the mean over the B*Ch planes
 * (B*Ch <= 64).  min(H, W) must exceed 160.  Six launches, nothing uploaded, nothing synchronised: capturable after one eager
 * loss / MS-SSIM call of the process (see orn_msssim_frames).  orn_msssim_ws_bytes: 0 on bad arguments. */
ORN_API size_t orn_msssim_ws_bytes(int B, int Ch, int H, int W);
ORN_API int orn_msssim(const float *pred, const float *target, int B, int Ch, int H, int W, float *out, void *ws,
               size_t ws_bytes, void *stream);
/* The same metric for n frame pairs, one value per frame: out[k] = ms_ssim(pred[k:k+1], targets[rows[k]:rows[k]+1],
 * data_range=1), which is how utils.py:201-211 calls it per frame with batch 1 from the evaluation loops (main_train.py:377-438,
 * main_eval.py:795-815).  pred [n][Ch][H][W]; targets [*][Ch][H][W]; rows: DEVICE int32[n] read on the device, NULL = identity
 * (targets[k]).  One launch per pyramid level for a whole chunk of frames (the level kernel also writes the next level's 2x2
 * average pool) and one finalize launch: six launches per chunk, nothing uploaded, nothing synchronised, capturable (the first
 * loss / MS-SSIM call of a process uploads the 11 filter taps and must not be the captured one).  The workspace must hold at
 * least one frame (orn_msssim_frames_ws_bytes with n = 1; ORN_E_WS otherwise); n is worked through in chunks of as many frames
 * as ws_bytes holds, and the values do not depend on the chunk size.  orn_msssim is this call with one group of B*Ch planes.
 * Ch <= 64, min(H, W) must exceed 160, n == 0 is a no-op. */
ORN_API size_t orn_msssim_frames_ws_bytes(int n, int Ch, int H, int W);       /* bytes for a chunk of n frames; 0 on bad arguments */
ORN_API int orn_msssim_frames(const float *pred, const float *targets, const int32_t *rows, int n, int Ch, int H, int W,
                              float *out /* [n] */, void *ws, size_t ws_bytes, void *stream);

/* ---- K11  ToTensor + F.adaptive_avg_pool2d(data, (h, w))      main_train.py:200,239,420; main_eval.py:467,807 ----
 * The reference pools every target to the decoder's output size inside the step; a video's frames never change during its fit, so
 * this runs once per video.  ATen's CPU arithmetic, bit for bit: output (i, j) is the fp32 sum, row-major from 0, over rows
 * [floor(i*H/h), ceil((i+1)*H/h)) and the same in W / w, divided by the window height and then by the window width (two correctly
 * rounded divisions); h > H or w > W (upsampling) follows the same formula.  A byte's value is (float)b / 255.0f correctly rounded
 * (ToTensor), from a table.  h == H && w == W gives exactly ToTensor (uint8 entry) and an exact copy (fp32 entry).
 * One launch per 65535 frames, no workspace, no atomics, capturable; src and dst must not overlap unless they are equal at
 * identity size (fp32 entry).  Every side at most 32768; ORN_E_ARG when a single output pixel's source row does not fit the
 * kernel's staging buffer (more than about 2700 source columns per output column).  n == 0 is a no-op. */
ORN_API int orn_frames_ingest_u8(const uint8_t *src /* device [n][H][W][3], interleaved as PIL decodes it */,
                                 int n, int H, int W, float *dst /* device [n][3][h][w] planar */, int h, int w, void *stream);
ORN_API int orn_frames_pool_f32(const float *src /* device [n][3][H][W] */, int n, int H, int W,
                                float *dst /* device [n][3][h][w] */, int h, int w, void *stream);

/* ---- A9  optim.Adam.step over one flat arena                         main_train.py:196,250 ---
 * p,g,m,v: n floats each.  step = 1-based global step.  weight decay 0, amsgrad off.
 * Hyper-parameters are doubles (as Python holds them): 1-beta, lr/(1-beta1^t) and sqrt(1-beta2^t)
 * are formed in double and rounded to fp32 once, exactly as torch.optim.Adam does. */
ORN_API int orn_adam_step(float *p, const float *g, float *m, float *v, size_t n, double lr, double beta1,
                  double beta2, double eps, int step, void *stream);

/* ---- A11  the whole per-frame training step as one engine           main_train.py:229-254 ----
 * The engine owns no memory: the caller passes four parameter-shaped arenas (params, grads, adam m,
 * adam v) laid out by `param_off` and one workspace.  Tensors inside an arena keep the PyTorch
 * shapes, so state_dict tensors can be views of `params`. */
typedef struct orn_layer_desc {
    int32_t C, O, s, H, W;          /* conv in-ch, conv out-ch (= Cn*s*s), stride, input H, W */
    /* offsets in floats into the parameter arenas; -1 = tensor absent */
    int64_t w3x3, b3x3;             /* ERB 3x3 branch, or the single conv of vanilla / deploy */
    int64_t w3x1, b3x1, w1x3, b1x3; /* ERB only */
    int64_t w1, w2, w3;             /* ERB only: 1x1 -> 3x3 -> 1x1 */
} orn_layer_desc;

/* The offsets of a block of a kind of N7 that orn_layer_desc has no field for (same units; read only for that kind).  ACB uses
 * w3x1 / b3x1 / w1x3 / b1x3 of orn_layer_desc; ECB uses w1 / w2 for wA / wB, with w3 = -1. */
typedef struct orn_branch_desc {
    int64_t w1x1, b1x1;             /* RepVGG */
    struct { int64_t k0, b0, scale, bias, mask; } sb[3];    /* ECB: sbx, sby, lpl */
} orn_branch_desc;

typedef struct orn_engine_desc {
    int32_t n_layers;
    int32_t erb;                    /* 1: ERB online merge; 0: single 3x3 conv per block */
    int32_t embed_len, stem_dim, fc_h, fc_w, fc_dim;
    int32_t sigmoid;                /* head activation (model.py:622) */
    int32_t loss_type;              /* ORN_LOSS_* (an MS-SSIM kind needs an output with min(H, W) > 160) */
    int32_t precision;              /* 0: fp32 everywhere; 1: bf16, 2: IEEE fp16 activations + 16-bit MFMA convs (fp32 accumulate) */
    double beta1, beta2, eps;
    int64_t stem_w0, stem_b0, stem_w1, stem_b1, head_w, head_b;
    int64_t n_params;               /* arena length in floats */
    orn_layer_desc layer[ORN_MAX_LAYERS];
    /* appended (N7); all zero = the engine that `erb` describes */
    int32_t branch_kind;            /* 0: as `erb` says; ORN_BRANCH_ACB / _REPVGG / _ECB (with erb = 0): every block is of that kind -- a
                                     * single-conv block whose (wf, bf) are merged into the workspace every step, as ERB's are.  Serial
                                     * step, graph replay, batched and split step, decode; no pipelined form */
    int32_t reserved_;
    orn_branch_desc branch[ORN_MAX_LAYERS];
    /* appended (multi-resolution heads); all zero = the engine of before */
    int32_t multi_res;              /* 1: a head on every stage (model.py:597-625 without sin_res) and the objective of main_train.py:239-250,
                                     * sum_{i < n-1} lw * loss(out_i, target_i) + loss(out_{n-1}, target_{n-1}); see orn_engine_set_stage_targets */
    float lw;                       /* weight of the stages below the last (--lw) */
    int64_t side_head_w[ORN_MAX_LAYERS], side_head_b[ORN_MAX_LAYERS];   /* heads of stages 0 .. n_layers-2: [3,C_i,1,1], [3]; head_w / head_b stay the last stage's */
    /* appended (--act); all zero = the engine of before */
    int32_t act;                    /* ORN_ACT_*: the activation of the stem and of every block, in every form of the engine (ORN_E_ARG for an
                                     * unknown value).  The workspace does not depend on it */
    int32_t reserved2_;
} orn_engine_desc;

/* One entry of the per-step schedule (device array, uploaded per epoch by the caller). */
typedef struct orn_step_sched {
    int32_t frame;                  /* index into frames / embed table */
    int32_t step;                   /* 1-based global optimiser step (Adam bias correction) */
    float lr;                       /* adjust_lr() value for this step (utils.py:240-259) */
    float pad;
} orn_step_sched;

typedef struct orn_engine orn_engine;

ORN_API size_t orn_engine_ws_bytes(const orn_engine_desc *d);
ORN_API int orn_engine_create(const orn_engine_desc *d, float *params, float *grads, float *adam_m, float *adam_v,
                      void *ws, size_t ws_bytes, orn_engine **out);
ORN_API void orn_engine_destroy(orn_engine *e);
/* Forward only (decode): embed [E] device -> img [3,H,W] device. */
ORN_API int orn_engine_decode(orn_engine *e, const float *embed, float *img, void *stream);
/* ---- N2  decode a fitted video: pixels and PSNR                     main_eval.py:795-815, main_train.py:377-438 ----
 * Decode n frames back to back on `stream` (no sync, capturable).  The weight-only work of the forward (ERB merge, 16-bit
 * operand copies) runs once, for frame 0; a 16-bit engine ends each frame in one kernel that reads the last block's output and
 * writes what is asked for (no fp32 image in between, no copy).
 * rows: DEVICE int32[n], indices into `embeds` [*,E] and, when given, `targets` [*,3,H,W] (fp32 planar).
 * Outputs, each optional (NULL = not wanted), at least one of the three non-NULL:
 *   rgb8  uint8 [n][H][W][3]   interleaved; q = (uint8) clamp(x*255 + 0.5, 0, 255)  (torchvision save_image; three fp32 ops)
 *   img   float [n][3][H][W]   what orn_engine_decode writes, bit for bit
 *   stats float [n][4]         {mse, psnr} of the float image and {mse, psnr} of q/255, against targets[rows[k]]
 *                              (psnr = -10 log10(mse), utils.py:191); requires targets
 * The engine may have been created without grads / Adam arenas (a decode-only engine).  Not to be enqueued on two streams at once
 * (one workspace). */
ORN_API int orn_engine_decode_frames(orn_engine *e, const float *embeds, const int32_t *rows, int32_t n,
                                     const float *targets, uint8_t *rgb8, float *img, float *stats, void *stream);
/* ---- N2 + N3  evaluate a fitted video: pixels, PSNR and MS-SSIM per frame   main_eval.py:795-815, main_train.py:377-438,
 * utils.py:201-211 ----
 * orn_engine_decode_frames plus one column: msssim float [n], the batched MS-SSIM above of each decoded frame against
 * targets[rows[k]] (requires targets; min(H, W) of the decoder output must exceed 160).  Same loop (the weight-only work runs for
 * frame 0 only) and the same output stage: rgb8 / img / stats hold exactly the bytes orn_engine_decode_frames writes.  After every
 * chunk of decoded frames the six MS-SSIM launches run on the chunk's fp32 planes: the caller's img when given, else slots inside
 * ws that the output kernel fills.  ws: orn_engine_eval_frames_ws_bytes for a chunk of >= 1 frames (16-byte aligned; the chunk
 * used is the largest that fits, the values do not depend on it); the engine's own workspace is not used for any of it.
 * msssim == NULL: exactly orn_engine_decode_frames (ws is not read).  No sync, capturable, one stream at a time. */
ORN_API size_t orn_engine_eval_frames_ws_bytes(const orn_engine_desc *d, int chunk);       /* 0 on bad arguments */
ORN_API int orn_engine_eval_frames(orn_engine *e, const float *embeds, const int32_t *rows, int32_t n, const float *targets,
                                   uint8_t *rgb8, float *img, float *stats /* [n][4] */, float *msssim /* [n] */,
                                   void *ws, size_t ws_bytes, void *stream);
/* One optimiser step.  frames [n_frames,3,H,W], embeds [n_frames,E] (device); sched: device array,
 * `cursor` a device int32 the step reads and post-increments, so `n` back-to-back steps consume
 * sched[cursor..cursor+n).  stats_out: device [n_slots][8] ring written at slot (cursor % n_slots). */
ORN_API int orn_engine_train_step(orn_engine *e, const float *frames, const float *embeds,
                          const orn_step_sched *sched, int32_t *cursor, float *stats_out, int32_t n_slots,
                          void *stream);
/* ---- N6  a caller-supplied loss: the step split at the loss              utils.py:139-189 (loss_fn is ordinary Python) ----
 * orn_engine_train_step in two calls, with the loss left to the caller: any function of the engine's output whose value and
 * gradient the caller can compute on the device (torch ops on the same stream, no host synchronisation needed).
 * orn_engine_step_forward: the schedule advance for one step and the training forward, exactly as orn_engine_train_step runs them.
 *   *pred receives the engine's own fp32 planar image [3,H,W] (device; inside the engine's workspace; no copy).  The step is now
 *   OPEN: until orn_engine_step_backward has run, every other stepping, decoding and evaluation entry of this engine -- and a second
 *   orn_engine_step_forward -- returns ORN_E_STATE, since it would overwrite the activations the backward needs.
 * orn_engine_step_backward: needs an open step (ORN_E_STATE otherwise) and the stream of its forward half.
 *   dpred  device fp32 [3,H,W], planar and contiguous: dLoss/dpred of the UNSCALED loss (the engine applies its own loss scale in
 *          the head's backward, as in every other step).  It is read in place by the head's backward (no copy): alive and unchanged
 *          until the stream has passed the call.  NULL abandons the step: its flag is raised and the Adam launch runs, so the
 *          step is skipped and counted like any other skipped step (parameters and moments untouched, `skipped` + 1).
 *   loss   optional device float: becomes stats[0] of the step's record (NULL: 0).  A non-finite value skips the step.
 *   The record: {loss, L1, MSE, 0, PSNR, lr, frame, step}; L1, MSE and PSNR of pred against the step's frame, as for every built-in
 *   loss (per 16x64 tile in fp32, tiles in double, fixed order, no atomics).  A NaN or infinity anywhere in dpred skips the step.
 *   From the head's backward on it runs the launches of orn_engine_train_step (serial form: no side stream, no graph), so a
 *   caller that hands in what orn_loss_fwd_bwd computes gets the bits of a built-in step.
 * Neither call synchronises.  frames / embeds / sched / cursor / stats_out / n_slots as for orn_engine_train_step, the same in
 * both halves.  There is no batched, pipelined or graph form of the split step. */
ORN_API int orn_engine_step_forward(orn_engine *e, const float *frames, const float *embeds, const orn_step_sched *sched,
                            int32_t *cursor, int32_t n_slots, const float **pred, void *stream);
ORN_API int orn_engine_step_backward(orn_engine *e, const float *frames, const float *embeds, const float *dpred,
                             const float *loss, float *stats_out, int32_t n_slots, void *stream);
/* Optional 0/1 gradient mask in the arena layout (device, float, 16-byte aligned; null removes it): gradients are
 * multiplied by it before Adam.  The prune fine-tune of main_eval.py:213-531 -- torch.nn.utils.prune keeps
 * weight = weight_orig * mask, so pruned entries never receive a gradient -- and its frozen tensors. */
ORN_API int orn_engine_set_grad_mask(orn_engine *e, const float *mask);
/* Optional table of orn_loss_target_stats for the frame table the following steps are given (device, 16-byte aligned, caller-owned,
 * alive while set; null removes it).  Used by the SSIM kinds (SSIM, Fusion1-6, Fusion9); other loss types ignore it. */
ORN_API int orn_engine_set_target_stats(orn_engine *e, const float *stats);
/* ---- N8  multi-resolution heads: a head and a loss at every stage       model.py:597-625, main_train.py:239-250 ----
 * An engine created with multi_res = 1 trains every stage's head.  Stage i < n_layers - 1 (a SIDE stage) has the image
 * out_i = act(W_i a_i + b_i) [3][H_i][W_i] of its block's output a_i, the loss of `loss_type` against its own target, weighted by lw,
 * and the backward term  da_i += W_i^T du_i,  du_i = lw * dLoss_i/dout_i * act'(out_i),  which the side head's backward adds to the
 * gradient buffer that block i + 1's dgrad has already written (orn_side_head.hip; 16-bit layers: the stored half + the term in fp32,
 * rounded once).  The last stage, every conv, merge and Adam launch are those of a single-resolution engine; lw = 0 gives its bits.
 * Forms: orn_engine_train_step, orn_engine_train_steps (always the serial form here), _graph, _batch.  The split step
 * (orn_engine_step_forward) returns ORN_E_ARG: a caller's objective takes one image.  orn_engine_decode / _decode_frames / _eval_frames give the last stage alone; every stage's image
 * comes from orn_engine_eval_stages (N9), which runs the side heads' forward inside its output kernel.
 * A 16-bit engine keeps its first block apart from the second (no fused first pair), so that the block's output exists in a layout a
 * head can read.  A non-finite pre-activation of a side head, side loss or side-head gradient raises the step's flag like any other.
 * orn_engine_create refuses (ORN_E_ARG, the stage named) a descriptor whose loss does not take a stage's size: an SSIM kind needs
 * H_i, W_i > 10, an MS-SSIM kind min(H_i, W_i) > 160 (pytorch_msssim asserts there).
 *   set_stage_targets: the resident target table of side stage `stage`, fp32 [n][3][H_i][W_i] (device, 16-byte aligned, caller-owned,
 *     alive while set), indexed by the schedule's frame index like `frames`: adaptive_avg_pool2d of the SOURCE frames to that stage's
 *     size (orn_frames_ingest_u8 / orn_frames_pool_f32).  Every side stage needs one before a training step (ORN_E_STATE otherwise).
 *   set_stage_target_stats: orn_loss_target_stats of that table (SSIM kinds; optional; null removes it), as orn_engine_set_target_stats.
 *   set_stage_stats: optional device ring [n_slots][n_layers][2] = {unweighted loss_i, psnr_i} of every stage, the last included,
 *     written at the slot of the step's record; in a batched step at the frame's place in the batch (null removes it).
 * The [n_slots][8] record keeps its layout: its loss entry holds the weighted sum, ((lw l_0 + lw l_1) + ..) + l_last in fp32; L1, MSE,
 * s and PSNR stay the last stage's.  All three calls drop the graph cache. */
ORN_API int orn_engine_set_stage_targets(orn_engine *e, int32_t stage, const float *frames);
ORN_API int orn_engine_set_stage_target_stats(orn_engine *e, int32_t stage, const float *stats);
ORN_API int orn_engine_set_stage_stats(orn_engine *e, float *out, int32_t n_slots);
/* ---- N9  decode and evaluate any stage of a multi-resolution fit          main_train.py:378-438 (psnr_fn / msssim_fn over output_list) ----
 * A multi-resolution fit is a scalable bitstream: the image of stage i needs the blocks 0..i and that stage's head only.
 * orn_engine_eval_stages is orn_engine_eval_frames with one output record per stage, out[0 .. n_layers): per frame ONE forward that
 * runs up to `top`, the highest stage with any output asked for -- the blocks above it and the last head are not launched, and block
 * `top`'s conv fills no input buffer for the block above -- then one output launch per wanted stage.  The weight-only work of the
 * forward runs for frame 0 only, as in orn_engine_decode_frames.
 *   Side stage of a 16-bit block: one kernel (k_stage_out_nhwc, orn_decode_out.hip) reads the block's channels-last pre-activation,
 *     applies the stage's head with the per-pixel arithmetic of the training forward's side head (so the fp32 value is the image that
 *     step's loss saw, bit for bit, wherever the conv launcher picks the kernel form it picks in training; a conv that fills no
 *     next-block buffer may take another form on large images, and the values then differ by 16-bit rounding of the block's output)
 *     and writes what is asked for; no fp32 image goes through memory on the way to the bytes.
 *   Side stage of an fp32 block (every stage of an fp32 engine; the first block of a 16-bit multi-resolution engine): the training
 *     forward's fp32 side head into the engine's own stage image, then the planar output stage.
 *   The last stage ends in the output stage of orn_engine_decode_frames: its rgb8 / img / stats / msssim are the bytes
 *     orn_engine_eval_frames writes on the same engine.
 * Per stage, each output optional as in orn_engine_decode_frames (sizes H_i x W_i: the stage's): rgb8, img, stats [n][4], and msssim
 * [n] through the batched MS-SSIM at that stage's size after every chunk of frames, on the caller's img or on slots in ws (the values
 * do not depend on the chunk).  targets: the stage's own table, indexed by rows[k] like `embeds`.
 * ws: orn_engine_eval_stages_ws_bytes(d, mask of the stages with an msssim column, chunk >= 1) bytes, 16-byte aligned, read only when
 * an msssim column is asked for (the largest chunk that fits is used); 0 for a bad descriptor, chunk < 1, or a mask naming a stage
 * that does not exist or whose smaller side is <= 160.  The engine's own workspace keeps its size.
 * Refused before anything is enqueued: no stage wanted; stats / msssim without targets; msssim on a stage with a side <= 160
 * (ORN_E_ARG); a stage below the last on an engine created with multi_res = 0, which has no side heads and may run its first two
 * blocks fused (ORN_E_STATE); a workspace too small for one frame (ORN_E_WS); an open split step (ORN_E_STATE).
 * The engine may be decode-only (null grads / Adam arenas) with multi_res = 1.  No sync, capturable, one stream at a time.  It changes
 * no parameter, gradient or optimiser state. */
typedef struct orn_stage_out {          /* one per stage; all members NULL = stage not wanted */
    const float *targets;               /* [*][3][H_i][W_i] fp32, indexed by rows[k] (needed by stats / msssim) */
    uint8_t *rgb8;                      /* [n][H_i][W_i][3] */
    float *img;                         /* [n][3][H_i][W_i] */
    float *stats;                       /* [n][4], as orn_engine_decode_frames */
    float *msssim;                      /* [n]; min(H_i, W_i) must exceed 160 */
} orn_stage_out;
ORN_API size_t orn_engine_eval_stages_ws_bytes(const orn_engine_desc *d, uint32_t msssim_stages, int chunk);
ORN_API int orn_engine_eval_stages(orn_engine *e, const float *embeds, const int32_t *rows, int32_t n,
                                   const orn_stage_out *out /* [n_layers] */, void *ws, size_t ws_bytes, void *stream);
/* One eager training step with HIP events around the conv launches, on the launch stream; synchronises it.  ms_out (host,
 * 2*n_layers + 2 floats): [i] forward conv of layer i, [n_layers + i] dgrad launch of layer i (0: none), [2*n_layers] the
 * batched wgrad launch of the 16-bit layers, [2*n_layers + 1] its split-K reduction (0 in fp32 mode, where each layer's
 * backward is one multi-kernel call reported under its dgrad slot).  Measurement hook for bench.py's roofline leg -- no
 * reference counterpart. */
ORN_API int orn_engine_profile_step(orn_engine *e, const float *frames, const float *embeds, const orn_step_sched *sched,
                            int32_t *cursor, float *stats_out, int32_t n_slots, float *ms_out, void *stream);
/* n_steps optimiser steps enqueued on `stream` without a graph (main_train.py:229-254, the loop body n times).  Engines in a
 * 16-bit mode with at least two blocks on the fast path run them PIPELINED: the last block's weight gradient, its slab reduction,
 * merge backward, Adam update (with the head's) and next merge forward run on a second stream the engine owns, forked off at the end
 * of the backward and joined in front of that block's forward conv of the next step, so that this chain overlaps the latency-bound
 * launches of the step boundary.  Same arithmetic, same order of every sum: bit-identical to orn_engine_train_step, except for a
 * step that only the side branch's late detectors flag (a late-only skip, below: counted and reported by orn_engine_scale_state).
 * All work is joined back into `stream` before the call returns (stream order on `stream` covers it). */
ORN_API int orn_engine_train_steps(orn_engine *e, const float *frames, const float *embeds, const orn_step_sched *sched,
                           int32_t *cursor, float *stats_out, int32_t n_slots, int32_t n_steps, void *stream);
/* Capture one train step into a hipGraph on `stream` and replay it n times (same arguments as above). */
ORN_API int orn_engine_train_steps_graph(orn_engine *e, const float *frames, const float *embeds,
                                 const orn_step_sched *sched, int32_t *cursor, float *stats_out,
                                 int32_t n_slots, int32_t n_steps, void *stream);
/* ---- N5  -b / --batchSize: B frames per optimiser step                main_train.py:205-254, utils.py:139-199 ----
 * loss_fn on a stacked batch is the mean over its frames of the single-frame loss (L1 / MSE: means over all elements; ssim /
 * ms_ssim with size_average: means over B*Ch planes), so the batch gradient is the mean of the per-frame gradients.  A batched
 * step runs, on the caller's stream alone (serial form: no side stream, no graph):
 *   the batched advance (flags and scale once per optimiser step, one clean step credited, the frame table filled);
 *   frame 0: the single-frame step's launches up to its last directly written gradient (merge forward included);
 *   frames 1..B-1: the same with the forward's merge left out -- the parameters have not changed, so the merged kernels, their
 *     16-bit operand copies and the merge backward's half copies of frame 0 stay valid;
 *   behind each frame one accumulate launch over the slots the backward writes directly (ERB: every block's w3x3 / b3x3 slot,
 *     which holds dWf / dbf; the head's and the stem's tensors; vanilla: every slot), frames summed in fp32 in frame order,
 *     ((g0 + g1) + g2) + ...; frame 0 writes the accumulator (no zeroing pass), the last frame's launch writes
 *     G = (acc + g_last) * (1.0f / B), one rounded multiply, back into the gradient arena (B == 1: no launch, G is frame 0's);
 *   then ONE merge backward (ERB; it is linear in dWf), the batch record, ONE Adam launch.
 * No atomics: run-to-run bit-identical.  The loss scale is constant within a step; a non-finite value in any frame skips the whole
 * optimiser step (parameters and moments untouched, `skipped` + 1, one halving at the next advance, Adam's count excludes it).
 * Ring record of an optimiser step, slot (optimiser-step index % n_slots) with the index = cursor / batch at its start:
 * {loss, L1, MSE, s, PSNR, lr, frame, step}: loss, L1, MSE, s are the means over the frames, summed in double in frame order;
 * PSNR = -10 log10 of the batch-mean MSE (psnr_fn takes the MSE over the whole batch, utils.py:191); frame is the batch's first.
 * An optimiser step consumes `batch` consecutive schedule entries: the frames come from all of them, step and lr from the first.
 * batch == 1 gives the bits of orn_engine_train_step.
 * The batch workspace is caller-owned device memory (256-byte aligned, alive while set; null removes it): the accumulation arena
 * (arena layout), the frame table of the step in flight and [max_batch][8] per-frame stats.  The engine's own workspace is
 * unchanged by it.  ORN_E_ARG for a missing workspace, batch < 1 or batch > max_batch. */
#define ORN_MAX_BATCH 16
ORN_API size_t orn_engine_batch_ws_bytes(const orn_engine_desc *d, int max_batch);      /* 0 on bad arguments */
ORN_API int orn_engine_set_batch_ws(orn_engine *e, void *ws, size_t bytes, int max_batch);
ORN_API int orn_engine_train_steps_batch(orn_engine *e, const float *frames, const float *embeds, const orn_step_sched *sched,
                                 int32_t *cursor, float *stats_out, int32_t n_slots, int32_t n_steps, int32_t batch,
                                 void *stream);
/* Dynamic loss scale + non-finite guard (the reference trains in fp32 and has neither; torch.cuda.amp.GradScaler is the
 * model).  The 16-bit gradient tensors of precision 2 travel multiplied by a scale held in device memory (2^20 at creation;
 * 1 for the other precisions).  A step whose gradients (or loss) are not finite leaves parameters and Adam moments untouched
 * and halves the scale; 2000 clean steps double it again up to its initial value.  All of it happens on the device, inside
 * the captured step.  out8 (host): {scale, 1/scale, ceiling, flag, steps skipped, clean steps, halvings, late-only skips};
 * synchronises.  flag includes a late-only skip the scale has not yet backed off for.
 * Where this differs from GradScaler:
 *  - granularity: the flag is PER STEP (one scale-state entry per step of the unrolled graph: an overflowing step skips itself
 *    only, the clean steps before and behind it in the same graph launch update the parameters), but the scale changes only
 *    where the device-side schedule advances, once per graph launch (orn_engine_train_steps_graph replays groups of 4 steps;
 *    orn_engine_train_step advances every step): one halving per group however many of its steps overflowed;
 *  - Adam's step numbers of a group are fixed when it is launched: a step skipped INSIDE a group leaves the bias corrections of
 *    the at most 3 steps behind it one count ahead (the next group is exact again);
 *  - the merge backward of the 16-bit modes rounds the UN-scaled weight gradient times 2^14 to IEEE half, and carries
 *    dT = W3^T dWf in half at the same scale: |dWf| > 4 and |W3^T dWf| > 4 raise the same flag, and no loss scale cures that.
 *    Such a fit has diverged; main_train restores the start of the epoch and continues in a wider precision (bf16 keeps that
 *    operand format, fp32 does not have it);
 *  - Adam's step count, in the device schedule and in the checkpoint's optimizer entry, excludes skipped steps;
 *  - orn_engine_train_steps (pipelined form) advances the schedule every step, like orn_engine_train_step.  The skip decision of a
 *    step is taken by the Adam launch on the caller's stream, behind every detector that runs there (the loss, the hand-off into
 *    the fp32 part, the lower blocks' slab reduction and merge-backward half copies, the head's dW finish is on the side stream but
 *    the dy it sums is covered by the lower blocks' detectors: a non-finite dy of the last block reaches them through the dgrad chain), and
 *    the side stream's Adam launch (last block + head) follows that decision.  Two detectors of the side branch run BEHIND the
 *    decision: the last block's slab reduction (unreachable alone, by the argument above) and the fp16 copies of its merged-kernel
 *    gradient and of dT in its merge backward (|dWf| > 4, |W3^T dWf| > 4).  If one of them fires alone (a LATE-ONLY skip), only
 *    the side stream's update of that step is skipped: the lower blocks take it, the last block and the head do not, the parameters
 *    stay finite.  It is counted apart from the skipped steps (out8[7]), and the scale backs off for it at the next advance or, when the side branch's Adam launch runs
 *    behind that one, at the advance after it.  Adam's step numbers (device schedule, checkpoint) do not exclude it: the lower
 *    blocks did apply the step.  This is the one case in which the pipelined form differs from the serial forms, which skip and
 *    count the whole step. */
ORN_API int orn_engine_scale_state(orn_engine *e, float *out8);
/* Overrides the live scale (>= 1) and, if gs_max > 0, its ceiling: tests inject an overflowing step this way. */
ORN_API int orn_engine_set_grad_scale(orn_engine *e, float gs, float gs_max);
/* Merged (deploy) kernel/bias of layer i, valid after a decode / train step (model.py:395-448; ERB and the kinds of N7). */
ORN_API int orn_engine_fused_kernel(orn_engine *e, int layer, const float **wf, const float **bf);

#ifdef __cplusplus
}
#endif
#endif /* ORN_H_ */
