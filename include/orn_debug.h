/* orn_debug.h -- test and probe entry points of liborn.so.  NOT part of the drop-in boundary: nothing here has a reference
 * counterpart.  The ablation flags make results WRONG (they exist to time parts of a kernel in isolation, tools/probes); the
 * conv entry points compute correct results (tests/test_gpu_conv16_forms.py checks every kernel form through them), and so does
 * the merge backward's (tests/test_gpu_merge16.py), the fused first block's and the slab-summing stem backward's
 * (tests/test_gpu_stage0.py), the MS-SSIM level kernels' (tests/test_gpu_msssim_levels.py), the loss launcher's
 * (tests/test_gpu_fusion6.py), the side heads'
 * (tests/test_gpu_side_head.py), the last stage's 16-bit head's (tests/test_gpu_head16.py), the fp32 conv path's
 * (tests/test_gpu_conv32_forms.py) and the batched weight-gradient and slab-reduction launches' (tests/test_gpu_wgrad16_batch.py).
 * Where they are defined: the entries of the 16-bit fast path (conv, head, wgrad16, side_head, stage_out, decode_out, orn_debug_set) in
 * csrc/orn_debug.hip, built once, each body written once against the type-erased table the engine calls through and exported under its
 * bf16 / f16 names; every other entry in the once-built file of the kernels it reaches (orn_stage0.hip, orn_elementwise.hip,
 * orn_conv_f32.hip, orn_loss.hip, orn_loss_msssim.hip, orn_merge_h16.hip). */
#ifndef ORN_DEBUG_H_
#define ORN_DEBUG_H_
#include "orn.h"
#ifdef __cplusplus
extern "C" {
#endif
/* Timing-only ablation flags of the 16-bit conv / wgrad kernels; effective only in a library built with -DORN_CONV_ABLATE
 * (the product build compiles the switches out).  0 restores normal operation. */
ORN_API void orn_debug_set(int flags);
/* The 16-bit conv launchers exactly as the engine calls them, bf16 and IEEE-half builds; buffers and conventions as
 * orn_conv_nhwc_bf16_fwd / orn_dgrad_nhwc_bf16 in orn.h (same slack rules), plus the arguments the raw entry points fix:
 *   fwd:   xpad holds Cin (= 96) channels per pixel, zero above the c_real real ones; c_real <= 32 with apad != NULL takes the
 *          narrow form.
 *   dgrad: dx_f32 alone (zprev = dyprev = NULL): fp32 output slabs [Q][H][W][C], Q = O/96 when the image has fewer than 128
 *          pixel tiles of 8 x 32 and O > 96, else 1 (their sum is dx); c_real <= 32 on a split launch writes channels [0, 32)
 *          only.  zprev, dyprev and dx_f32 together (only where Q > 1): dx_f32 is the scratch of that split, which is
 *          then finished into dyprev.  zprev, dyprev alone: the fused epilogue. */
ORN_API int orn_debug_conv_fwd_bf16(const void *xpad, const void *wb, const float *bias_p, int H, int W, int Cin, int O, int s,
                                    void *z, void *apad, int c_real, void *stream);
ORN_API int orn_debug_conv_fwd_f16(const void *xpad, const void *wb, const float *bias_p, int H, int W, int Cin, int O, int s,
                                   void *z, void *apad, int c_real, void *stream);
ORN_API int orn_debug_conv_dgrad_bf16(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev,
                                      void *dyprev, int sp, float *dx_f32, int c_real, void *stream);
ORN_API int orn_debug_conv_dgrad_f16(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev,
                                     void *dyprev, int sp, float *dx_f32, int c_real, void *stream);
/* The merge backward of the 16-bit engine modes (ERB: dW3, dT, dW2, dW1 on half operand copies, then the slices) on n = 1..8
 * layers in one set, with the launchers and the call sequence of the engine; workspace and scale state of its own, allocated
 * and freed inside, `stream` synchronised.  Host arrays, per layer i:
 *   co[2i ..]:  C, O
 *   in[6i ..]:  G = dL/dWf [O][C][3][3], dbf [O], T [O][C][3][3], w1 [2C][C], w2 [O][2C][3][3], w3 [O][O]   (fp32, device)
 *   out[7i ..]: dW3 [O][O], dW2 [O][2C][3][3], dW1 [2C][C], d1x3 [O][C][3], d3x1 [O][C][3], db1x3 [O], db3x1 [O]  (fp32, device)
 * *flag: the flag word of the scale state after the call (1: a half copy of G or of dT was not finite).  Returns 0 or an
 * error code. */
ORN_API int orn_debug_merge_h16_bwd(int n, const int *co, const float *const *in, float *const *out, int *flag, void *stream);
/* The output stage of orn_engine_decode_frames in its fp32-engine form, on a caller's planar image img [3][H][W] (device): bytes
 * rgb8 [H][W][3], a copy img_out, stats[4] = {mse, psnr, mse of bytes / 255, its psnr} against target [3][H][W]; each output
 * optional.  ws (device, 4-byte aligned, the size the _ws_bytes call returns) is needed for stats only.  tests/test_gpu_decode.py pins the
 * quantisation at the half-way points k + 0.5 through it. */
ORN_API size_t orn_debug_decode_out_ws_bytes(void);
ORN_API int orn_debug_decode_out_f32(const float *img, int H, int W, const float *target, uint8_t *rgb8, float *img_out,
                                     float *stats, void *ws, size_t ws_bytes, void *stream);
/* The output stage of a SIDE stage of orn_engine_eval_stages (include/orn.h N9; k_stage_out_nhwc, orn_decode_out.hip) on a caller's
 * channels-last pre-activation z [H][W][C] (bf16 / IEEE half, 2-byte aligned; 16-byte loads where C % 8 == 0 and z is 16-byte
 * aligned) and head w [3][C], b [3]; 1 <= C <= 512, H*W <= 2^30; sigmoid: 0 = (tanh + 1) / 2.  Outputs and workspace as
 * orn_debug_decode_out_f32: rgb8 [H][W][3], img [3][H][W] -- bit-identical to orn_debug_side_head_fwd_* on the same inputs --,
 * stats[4] against target [3][H][W]; the ticket word (float index 2 * 8192 of ws) is zero again after the launch.  ORN_E_ARG, with
 * nothing enqueued, for a bad argument.  The _act twins take ORN_ACT_* last.  tests/test_gpu_stage_out.py. */
ORN_API int orn_debug_stage_out_bf16(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, const float *target,
                                     uint8_t *rgb8, float *img, float *stats, void *ws, size_t ws_bytes, void *stream);
ORN_API int orn_debug_stage_out_f16(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, const float *target,
                                    uint8_t *rgb8, float *img, float *stats, void *ws, size_t ws_bytes, void *stream);
ORN_API int orn_debug_stage_out_bf16_act(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, const float *target,
                                         uint8_t *rgb8, float *img, float *stats, void *ws, size_t ws_bytes, void *stream, int act);
ORN_API int orn_debug_stage_out_f16_act(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, const float *target,
                                        uint8_t *rgb8, float *img, float *stats, void *ws, size_t ws_bytes, void *stream, int act);
/* The fused fp32 first block of a 16-bit engine (orn_stage0.hip) through the launchers the engine calls, with no rider and no
 * pack work-groups; tests/test_gpu_stage0.py pins both kernels elementwise through them.  x [C][H][W], wf [O][C][3][3], bf [O]
 * (fp32, device); Cn = O / s^2 post-shuffle channels.
 *   supported: 1 when the fused block takes the shape (1 <= C <= 64, O % s^2 == 0, W >= 4, H*W a multiple of 16 and <= 256, LDS);
 *          every other entry returns ORN_E_ARG ("stage0: unsupported ...") for a shape it declines, and launches nothing.
 *   slabs: work-groups of the backward = dx partial slabs, s^2 * ceil(Cn / 16) (0 for arguments without a meaning).
 *   fwd:   z [s^2][H*W][Cn] fp32, element ((i*s + j)*H*W + h*W + w)*Cn + n = pre-activation of conv channel n*s^2 + i*s + j at
 *          (h, w); every element is written; NULL: not kept (the decode form, same xpad_next bits).  xpad_next: 16-bit
 *          [H*s + 2][W*s + 2][Cp] channels-last (precision 1: bf16, 2: IEEE half), Cp >= Cn; written: channels [0, Cn) of the
 *          interior, SiLU of the shuffled pre-activation rounded to nearest even.  NOT written: the one-pixel ring and channels
 *          [Cn, Cp) (the engine zeroes them once).
 *   bwd:   z as the forward left it; dxn [nslab][H*s][W*s][Cp] fp32, the next block's dgrad slabs (no ring): their sum times
 *          inv_gs is the gradient with respect to the block's output; channels [Cn, Cp) are never read.  slabs: scratch and
 *          output, orn_debug_stage0_slabs(O, s) x [C][H*W] floats, 16-byte aligned, every element overwritten; their sum is dx.
 *          dx [C][H][W]: that sum (a fixed-order reduction launch); NULL: the slabs are left to the caller, as the engine leaves
 *          them to the stem backward.  dwf [O][C][3][3], dbf [O]: overwritten, every element. */
ORN_API int orn_debug_stage0_supported(int C, int O, int H, int W, int s);
ORN_API int orn_debug_stage0_slabs(int O, int s);
ORN_API int orn_debug_stage0_fwd(const float *x, const float *wf, const float *bf, int C, int O, int H, int W, int s, float *z,
                                 void *xpad_next, int Cp, int precision, void *stream);
ORN_API int orn_debug_stage0_bwd(const float *x, const float *wf, const float *z, const float *dxn, int nslab, int Cp, float inv_gs,
                                 int C, int O, int H, int W, int s, float *slabs, float *dx, float *dwf, float *dbf, void *stream);
/* The B == 1 stem backward as the 16-bit engine runs it behind the fused first block (two launches, no deferred jobs): dh2_slabs
 * [nslab][Nout] are partial rows of dL/dh2 that the first kernel sums itself (64 lanes stride over the slabs, fixed order);
 * other arguments and outputs as orn_stem_bwd at B = 1.  ws: orn_stem_bwd_ws_bytes(1, Hd, Nout) bytes (ORN_E_WS below that);
 * written: dpre1 [Hd] at float offset Nout and ceil(Nout / 16) rows of Hd partials at Nout + 2*Hd, nothing else. */
ORN_API int orn_debug_stem_bwd_slabs(const float *embed, const float *w1, const float *pre1, const float *h1, const float *pre2,
                                     const float *dh2_slabs, int nslab, int E, int Hd, int Nout, float *dw0, float *db0, float *dw1,
                                     float *db1, float *ws, size_t ws_bytes, void *stream);
/* The MS-SSIM losses (Fusion10 / 11 / 12; orn_loss.hip, orn_loss_msssim.hip) one launch at a time, at any plane size H, W >= 11 --
 * orn_loss_fwd_bwd itself takes nothing below 161 px, so levels 1..4 only ever see what pooling leaves.  The kernel argument of
 * every launch is built by the function the product launcher builds it with (tile counts, pooled size and padding, the float4
 * condition, the grid); tests/test_gpu_msssim_levels.py pins the kernels elementwise to fp64 through these.  Every entry returns
 * ORN_E_ARG with a message for arguments it declines (a null pointer, planes outside 1..65535, H or W below 11, H*W above 2^26, a
 * form outside 0..3) and launches nothing then.  All pointers are device pointers; planes are fp32 [planes][H][W].
 *   gauss_taps: the 11 filter taps every SSIM / MS-SSIM kernel uses (host array; no GPU is touched): fp32 exp, fp32 sum in index
 *          order, fp32 divide.
 *   level_fwd_tiles / level_bwd_tiles: work-groups per plane of the launch below (16x64 tiles of the valid map (H-10) x (W-10) /
 *          of the image); 0 for H or W below 11.
 *   level_fwd: one k_msssim_level launch.  part [planes][tiles][2] = {sum of the SSIM map, sum of the CS map} over the tile's part
 *          of the valid map; every element is written.  nx, ny (both or neither): the 2x2 average pool of x and y,
 *          [planes][Ho][Wo], Ho = (H + 2 (H % 2)) / 2 (avg_pool2d(2, padding = size % 2), count_include_pad); every element is
 *          written, by exactly one work-group.
 *   level_bwd: one k_msssim_level_bwd launch.  form 0: the SSIM map's derivatives (level 4 of the chain); 1: the CS map's (levels
 *          3..1); 2: the CS map's at level 0, with the pixel term; 3: level 0 without the gradient.
 *          g [planes][H][W] = k[plane] * d(sum of the map over the valid region)/dx + the pool's adjoint of gnext
 *          (0.25 * gnext[(y + H % 2) / 2][(x + W % 2) / 2]; gnext [planes][Ho][Wo], NULL: none) + (form 2) g_l1 * sign(x - y) +
 *          g_l2 * (x - y); every element is written.  Forms 2 and 3 also write part_l1 [planes][tiles][2] = {sum |x - y|,
 *          sum (x - y)^2} per image tile; form 3 writes nothing else and reads neither k nor gnext (k, gnext, g may be NULL).
 *          frame_idx (forms 2 and 3, optional): y is taken at y + *frame_idx * frame_stride floats; the float4 load path needs
 *          W % 4 == 0, 16-byte aligned x and y and, with a frame index, frame_stride % 4 == 0.
 *   loss_msssim_layout: where orn_loss_fwd_bwd(loss_type = an MS-SSIM id, B, Ch, H, W) keeps its intermediates, as float offsets
 *          from the start of its workspace; out[44] (host).  Per level l = 0..4, out[8 l + ..]: 0, 1 the level's H, W; 2, 3 the
 *          pooled pred / target planes [B*Ch][H_l][W_l] (-1 at level 0: the caller's arrays); 4 the forward's tile partials
 *          [B*Ch][nblk][2]; 5 nblk; 6 the level's gradient planes (-1 at level 0: dpred); 7 the level's coefficients k[l] [B*Ch].
 *          out[40]: the MS-SSIM value; out[41], out[42]: the level-0 {|d|, d^2} partials and their tiles per plane; out[43]: the
 *          workspace in floats (orn_loss_ws_bytes_for / 4). */
ORN_API void orn_debug_gauss_taps(float *g11);
ORN_API int orn_debug_msssim_level_fwd_tiles(int H, int W);
ORN_API int orn_debug_msssim_level_bwd_tiles(int H, int W);
ORN_API int orn_debug_msssim_level_fwd(const float *x, const float *y, int planes, int H, int W, float *part, float *nx, float *ny,
                                       void *stream);
ORN_API int orn_debug_msssim_level_bwd(int form, const float *x, const float *y, const float *k, const float *gnext,
                                       const int *frame_idx, size_t frame_stride, int planes, int H, int W, float g_l1, float g_l2,
                                       float *g, float *part_l1, void *stream);
ORN_API int orn_debug_loss_msssim_layout(int loss_type, int B, int Ch, int H, int W, int64_t *out);
/* The loss launcher of every step (orn_launch_loss: k_fusion6 / k_loss_grad + the finalize launch) with all the arguments the engine
 * gives it, where orn_loss_fwd_bwd fixes frame_idx = NULL and tstats = NULL; tests/test_gpu_fusion6.py pins both kernels elementwise
 * to fp64 through it.  The launcher itself picks the kernel form and decides the float4 load path (W % 4 == 0, 16-byte aligned pred
 * and frames and, with a frame index, frame_stride % 4 == 0).
 *   loss_launch: pred, dpred [B][Ch][H][W]; the target is frames + *frame_idx * frame_stride floats (frame_idx: device, NULL: frames
 *          itself).  tstats (NULL: none): orn_loss_target_stats of the same table, SSIM kinds only, B == 1 (one frame's maps hold
 *          Ch planes).  dpred NULL: no gradient, the same partials and stats.  stats[8], ws, ws_bytes as orn_loss_fwd_bwd.  Refused
 *          with ORN_E_ARG and nothing launched: a null pointer, a size below 1, more than 65535 planes, an unknown or an MS-SSIM
 *          loss_type, tstats with a loss that has no SSIM term; ORN_E_WS: a workspace below orn_loss_ws_bytes_for.
 *   loss_layout: what the launch leaves in ws.  out[4] (host) = tiles_w, tiles_h (16x64 tiles of the image), the float offset of
 *          part_l1, the workspace in floats: part_ssim [B*Ch][tiles] at offset 0 (SSIM kinds), part_l1 [B*Ch][tiles][2] = {sum |d|,
 *          sum d^2}. */
ORN_API int orn_debug_loss_launch(const float *pred, const float *frames, const int *frame_idx, size_t frame_stride, int B, int Ch,
                                  int H, int W, int loss_type, float loss_scale, const float *tstats, float *stats, float *dpred,
                                  void *ws, size_t ws_bytes, void *stream);
ORN_API int orn_debug_loss_layout(int B, int Ch, int H, int W, int64_t *out);
/* The side heads of a multi-resolution generator (model.py:597-625 without sin_res; orn_side_head.hip, fp32: orn_side_head_f32.hip): the head of a stage below
 * the last one, whose backward ADDS to a gradient buffer the block above has already written.  tests/test_gpu_side_head.py pins
 * them elementwise to fp64.  w [3][C], b [3], out / dout [3][H][W] planar fp32; 1 <= C <= 512, H*W <= 2^30; sigmoid: 0 = (tanh + 1) / 2.
 *   fwd (16 bit): z [H][W][C] channels-last pre-activation (bf16 / IEEE half); out = act(W SiLU(z) + b), every element written.
 *          Per-pixel arithmetic and, with C % 32 == 0, summation order of the last stage's 16-bit head.
 *   fwd_f32: a [C][H][W] activation (fp32 NCHW); out = act(W a + b), one c-ordered fmaf chain per output, expf / tanhf.
 *   bwd (16 bit): du = dout * lw * gs * act'(out).  dypad: the block's gradient buffer, [H/sp + 2][W/sp + 2][C sp^2] channels-last,
 *          pixel (h, w) channel c at ((h/sp + 1) (W/sp + 2) + w/sp + 1) C sp^2 + ((h % sp) sp + w % sp) C + c (H % sp == W % sp == 0).
 *          Every interior element becomes round16(fp32(old) + (W^T du)[c] * SiLU'(z)): one rounding; the one-pixel ring is neither
 *          read nor written.  16-byte accesses when C % 8 == 0 and z, dypad are 16-byte aligned, element-wise otherwise.
 *          dw [3][C] = sum_pixels du SiLU(z) / gs, db [3] = sum du / gs: overwritten, fixed summation order.
 *   bwd_f32: a [C][H][W] activation, da [C][H][W] the gradient with respect to it: da += W^T du with du = dout * lw * act'(out);
 *          dw = sum du a, db = sum du.
 *   ws: orn_debug_side_head_bwd_ws_bytes(C, H, W) bytes (0 for sizes outside the ranges above), 4-byte aligned; ORN_E_WS below that. */
ORN_API size_t orn_debug_side_head_bwd_ws_bytes(int C, int H, int W);
ORN_API int orn_debug_side_head_fwd_bf16(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                         void *stream);
ORN_API int orn_debug_side_head_fwd_f16(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                        void *stream);
ORN_API int orn_debug_side_head_fwd_f32(const float *a, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                        void *stream);
ORN_API int orn_debug_side_head_bwd_bf16(const void *z, const float *w, const float *out, const float *dout, int C, int H, int W,
                                         int sigmoid, int sp, float lw, float gs, void *dypad, float *dw, float *db, void *ws,
                                         size_t ws_bytes, void *stream);
ORN_API int orn_debug_side_head_bwd_f16(const void *z, const float *w, const float *out, const float *dout, int C, int H, int W,
                                        int sigmoid, int sp, float lw, float gs, void *dypad, float *dw, float *db, void *ws,
                                        size_t ws_bytes, void *stream);
ORN_API int orn_debug_side_head_bwd_f32(const float *a, const float *w, const float *out, const float *dout, int C, int H, int W,
                                        int sigmoid, float lw, float *da, float *dw, float *db, void *ws, size_t ws_bytes, void *stream);
/* The fp32 block path (orn_conv_f32.hip) and the fp32 engine's fused head backward (k_head_bwd_fused_f32, orn_elementwise.hip):
 * which kernel form the launchers pick for a shape, and the forms no public entry reaches.  tests/test_conv32_plan_host.py pins
 * the selection, tests/test_gpu_conv32_forms.py every form elementwise to fp64.  x [B][C][H][W], wf [O][C][3][3], bf [O],
 * z / a [B][O/s^2][H s][W s] (fp32 NCHW, device).  Every entry returns ORN_E_ARG with a message for arguments it declines (a null
 * pointer, a size below 1, O not a multiple of s^2) and launches nothing then.
 *   conv_f32_plan: no GPU is touched.  out[18] (host), from the selection functions the launchers themselves call, for the block
 *          (B, C, O, H, W):
 *            forward (orn_conv3x3_ps_silu_fwd)  0: 1 = 2-row tiles (fewer than 256 work-groups on 8-row tiles), 0 = 8-row tiles;
 *                   1: work-groups of the launch.
 *            dgrad = conv(dy, Wd) with C_in = O, O_out = C (orn_conv3x3_ps_silu_bwd)  2: 2-row tiles; 3: nsplit, the partial
 *                   slabs the input channels are split over (1: none); 4: input channels per split; 5: 1 = a launch on 64-channel
 *                   tiles happens; 6: 1 = the launch of the last 32 output channels on a 32-channel tile happens (8-row tiles,
 *                   O_out % 64 == 32, unsplit); 7: reduction of the slabs, 0 = none, 1 = k_reduce_rows, 2 = k_reduce_rows_tall;
 *                   8: work-groups of all its conv launches.
 *            wgrad  9: form, 1 = k_wgrad_f32, 2 = k_wgrad_f32_v2 (O % 128 == 0 and C % 32 == 0); 10: S, the split-K slabs;
 *                   11: K tiles (4 x 32 pixels, form 2: 1 x 32); 12: work items (S x o tiles x n tiles); 13: reduction of the
 *                   slabs, 1 or 2 as above.
 *            conv dbias  14: rows of partials k_silu_bwd_unshuffle writes (B x chunks of 2048 pixels); 15: their reduction;
 *                   16: rows the fused head backward writes instead (B == 1: work-groups of 512 pixels); 17: their reduction.
 *   conv_fwd_f32: orn_conv3x3_ps_silu_fwd with either output optional: z == NULL or a == NULL (not both); a == NULL is the engine's
 *          z-only form of the last block.
 *   head_fwd_z: orn_head_fwd on the pre-activation: out = act(W SiLU(z) + b), SiLU formed in the kernel; z [B][C][H][W], C <= 512.
 *   conv_bwd_f32_head: orn_conv3x3_ps_silu_bwd at B = 1, s = 2 with the head's backward fused in front, as the fp32 engine runs
 *          its last block: instead of da it takes the head's w [3][O/4], out and dout [3][2H][2W]; du = dout * act'(out),
 *          dy = unshuffle((W^T du) * SiLU'(z)).  dx (optional) [C][H][W], dwf, dbf as orn_conv3x3_ps_silu_bwd; head_dw [3][O/4] =
 *          sum du SiLU(z), head_db [3] = sum du: overwritten, fixed summation order.  preflip != 0: the dgrad's flipped kernel is
 *          made first by the engine's all-layers launch (orn_launch_flip_transpose_all, one layer) in a region of ws of its own and
 *          handed over ready-made; same bits as preflip == 0.  O % 4 == 0, O / 4 <= 512.  ws: 4-byte aligned,
 *          orn_debug_conv_bwd_f32_head_ws_bytes(C, O, H, W) bytes (0 for sizes without a meaning); ORN_E_WS below that. */
ORN_API int orn_debug_conv_f32_plan(int B, int C, int O, int H, int W, int32_t *out);
ORN_API int orn_debug_conv_fwd_f32(const float *x, const float *wf, const float *bf, int B, int C, int O, int H, int W, int s,
                                   float *z, float *a, void *stream);
ORN_API int orn_debug_head_fwd_z(const float *z, const float *w, const float *b, int B, int C, int H, int W, int sigmoid, float *out,
                                 void *stream);
ORN_API size_t orn_debug_conv_bwd_f32_head_ws_bytes(int C, int O, int H, int W);
ORN_API int orn_debug_conv_bwd_f32_head(const float *x, const float *wf, const float *z, const float *head_w, const float *head_out,
                                        const float *head_dout, int C, int O, int H, int W, int sigmoid, int preflip, float *dx,
                                        float *dwf, float *dbf, float *head_dw, float *head_db, void *ws, size_t ws_bytes,
                                        void *stream);
/* The last stage's 16-bit head (k_head_fwd_nhwc_bf16, k_head_bwd_nhwc_bf16<C / 32>, orn_ops_bf16.hip) and the reduction of its dW / db
 * partials (head_finish_body, orn_wgrad_bf16.hip), through the launchers the engine calls; tests/test_gpu_head16.py pins them
 * elementwise to fp64.  w [3][C], b [3], out / dout / target [3][H][W] planar fp32; sigmoid: 0 = (tanh + 1) / 2.
 *   bwd_blocks: work-groups of the backward = rows of partials it leaves (64 pixels each, at most 512: above 512 x 64 pixels a lane
 *          walks several pixels); bwd_ws_bytes: its workspace, (512 + 1) x (3 C + 3) floats.  No GPU is touched; 0 for sizes without a
 *          meaning (H or W below 1; C outside {32, 64, 96, 128}).
 *   fwd:   z [H][W][C] channels-last pre-activation (bf16 / IEEE half), C % 32 == 0, 32 <= C <= 256; out = act(W SiLU(z) + b), every
 *          element written.  Above 8192 x 64 pixels a lane walks several pixels.
 *   bwd:   du = dout * gs * act'(out).  dypad [H/sp + 2][W/sp + 2][C sp^2] channels-last (layout: the side head's, above); every interior
 *          element is OVERWRITTEN with round16((W^T du)[c] * SiLU'(z)), the one-pixel ring is neither read nor written.  dw [3][C] =
 *          sum_pixels du SiLU(z) / gs, db [3] = sum du / gs: overwritten, fixed summation order.
 *          flag == NULL, the per-op form: gs travels by value and the reduction is a launch of its own (k_head_bf16_finish).
 *          flag != NULL, the engine's form: gs and 1 / gs are read from a scale state of the entry's own (allocated and freed inside,
 *          `stream` synchronised), the reduction rides on a batched weight-gradient launch without jobs; *flag: the state's flag word
 *          after the call (1: dw or db was not finite).  Same bits in both forms.
 *          target != NULL, the rider: orn_loss_fwd_bwd's launches on (out, target) with loss_scale = gs come first and WRITE dout; the
 *          loss's last stage then runs as one more work-group of the head backward and leaves stats[8] (device) as orn_loss_fwd_bwd does.
 *   ws:    4-byte aligned, orn_debug_head16_bwd_ws_bytes(C) bytes.  With a target: 16-byte aligned,
 *          orn_debug_head16_bwd_rider_ws_bytes(C, H, W, loss_type) bytes (0 where the loss takes no such image) -- the head's part,
 *          rounded up to a multiple of 256 bytes, then the loss's orn_loss_ws_bytes_for(loss_type, 1, 3, H, W) bytes.
 *   Refused with ORN_E_ARG and nothing launched: a null pointer, C outside {32, 64, 96, 128}, H or W not a multiple of sp, gs <= 0;
 *   ORN_E_WS: a workspace below the size. */
ORN_API int orn_debug_head16_bwd_blocks(int H, int W);
ORN_API size_t orn_debug_head16_bwd_ws_bytes(int C);
ORN_API size_t orn_debug_head16_bwd_rider_ws_bytes(int C, int H, int W, int loss_type);
ORN_API int orn_debug_head_fwd_bf16(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                    void *stream);
ORN_API int orn_debug_head_fwd_f16(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                   void *stream);
ORN_API int orn_debug_head_bwd_bf16(const void *z, const float *w, const float *out, float *dout, int C, int H, int W, int sigmoid,
                                    int sp, float gs, void *dypad, float *dw, float *db, void *ws, size_t ws_bytes, int *flag,
                                    const float *target, int loss_type, float *stats, void *stream);
ORN_API int orn_debug_head_bwd_f16(const void *z, const float *w, const float *out, float *dout, int C, int H, int W, int sigmoid,
                                   int sp, float gs, void *dypad, float *dw, float *db, void *ws, size_t ws_bytes, int *flag,
                                   const float *target, int loss_type, float *stats, void *stream);
/* ---- the activation of --act (ORN_ACT_SWISH / ORN_ACT_GELU, include/orn.h) ----
 * act_eval: f[i] = act(z[i]), df[i] = act'(z[i]) for n <= 2^30 device floats, through the device functions the kernels call: exact == 0
 *          the pair of the 16-bit kernels (OrnAct<act>::f / df), exact != 0 the pair of the fp32 path (f_exact / df_exact);
 *          tests/test_gpu_act_eval.py sweeps them against fp64.
 * Every other *_act entry below is the entry of the same name without the suffix (above), same arguments and conventions, with the
 * activation as one more trailing `int act`; the un-suffixed entries are these with ORN_ACT_SWISH.  An unknown act: ORN_E_ARG with a
 * text, checked before anything else, nothing launched. */
ORN_API int orn_debug_act_eval(int act, int exact, const float *z, size_t n, float *f, float *df, void *stream);
ORN_API int orn_debug_conv_fwd_bf16_act(const void *xpad, const void *wb, const float *bias_p, int H, int W, int Cin, int O, int s,
                                        void *z, void *apad, int c_real, void *stream, int act);
ORN_API int orn_debug_conv_fwd_f16_act(const void *xpad, const void *wb, const float *bias_p, int H, int W, int Cin, int O, int s,
                                       void *z, void *apad, int c_real, void *stream, int act);
ORN_API int orn_debug_conv_dgrad_bf16_act(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev,
                                          void *dyprev, int sp, float *dx_f32, int c_real, void *stream, int act);
ORN_API int orn_debug_conv_dgrad_f16_act(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev,
                                         void *dyprev, int sp, float *dx_f32, int c_real, void *stream, int act);
ORN_API int orn_debug_head_fwd_bf16_act(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                        void *stream, int act);
ORN_API int orn_debug_head_fwd_f16_act(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                       void *stream, int act);
ORN_API int orn_debug_head_bwd_bf16_act(const void *z, const float *w, const float *out, float *dout, int C, int H, int W, int sigmoid,
                                        int sp, float gs, void *dypad, float *dw, float *db, void *ws, size_t ws_bytes, int *flag,
                                        const float *target, int loss_type, float *stats, void *stream, int act);
ORN_API int orn_debug_head_bwd_f16_act(const void *z, const float *w, const float *out, float *dout, int C, int H, int W, int sigmoid,
                                       int sp, float gs, void *dypad, float *dw, float *db, void *ws, size_t ws_bytes, int *flag,
                                       const float *target, int loss_type, float *stats, void *stream, int act);
ORN_API int orn_debug_side_head_fwd_bf16_act(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                             void *stream, int act);
ORN_API int orn_debug_side_head_fwd_f16_act(const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                            void *stream, int act);
ORN_API int orn_debug_side_head_bwd_bf16_act(const void *z, const float *w, const float *out, const float *dout, int C, int H, int W,
                                             int sigmoid, int sp, float lw, float gs, void *dypad, float *dw, float *db, void *ws,
                                             size_t ws_bytes, void *stream, int act);
ORN_API int orn_debug_side_head_bwd_f16_act(const void *z, const float *w, const float *out, const float *dout, int C, int H, int W,
                                            int sigmoid, int sp, float lw, float gs, void *dypad, float *dw, float *db, void *ws,
                                            size_t ws_bytes, void *stream, int act);
ORN_API int orn_debug_stage0_fwd_act(const float *x, const float *wf, const float *bf, int C, int O, int H, int W, int s, float *z,
                                     void *xpad_next, int Cp, int precision, void *stream, int act);
ORN_API int orn_debug_stage0_bwd_act(const float *x, const float *wf, const float *z, const float *dxn, int nslab, int Cp, float inv_gs,
                                     int C, int O, int H, int W, int s, float *slabs, float *dx, float *dwf, float *dbf, void *stream,
                                     int act);
ORN_API int orn_debug_stem_bwd_slabs_act(const float *embed, const float *w1, const float *pre1, const float *h1, const float *pre2,
                                         const float *dh2_slabs, int nslab, int E, int Hd, int Nout, float *dw0, float *db0, float *dw1,
                                         float *db1, float *ws, size_t ws_bytes, void *stream, int act);
ORN_API int orn_debug_conv_fwd_f32_act(const float *x, const float *wf, const float *bf, int B, int C, int O, int H, int W, int s,
                                       float *z, float *a, void *stream, int act);
ORN_API int orn_debug_head_fwd_z_act(const float *z, const float *w, const float *b, int B, int C, int H, int W, int sigmoid, float *out,
                                     void *stream, int act);
ORN_API int orn_debug_conv_bwd_f32_head_act(const float *x, const float *wf, const float *z, const float *head_w, const float *head_out,
                                            const float *head_dout, int C, int O, int H, int W, int sigmoid, int preflip, float *dx,
                                            float *dwf, float *dbf, float *head_dw, float *head_db, void *ws, size_t ws_bytes,
                                            void *stream, int act);
/* ---- the two weight-gradient launches of every 16-bit step (k_wgrad_nhwc_bf16_all, k_wgrad_bf16_reduce_all; orn_wgrad_bf16.hip) ----
 * wgrad16_step: exactly what the engine's fast_weight_grads / side_branch_backward enqueue, through the OrnHalfOps members they call
 * (wgrad_batch, then wgrad_reduce_all), on the caller's buffers; tests/test_gpu_wgrad16_batch.py pins both launches elementwise to fp64.
 *   jobs:  n in 0..ORN_MAX_LAYERS problems, launched and reduced in the order given.  xpad [H+2][W+2][96], dypad [H+2][W+2][O] (+ 128
 *          elements of slack) as orn_wgrad_nhwc_bf16; smax: the caller's slab cap (OrnWgradJob::smax, handed to the reduction too; below 8:
 *          none); slabs: at least orn_debug_wgrad16_ws_floats(H, W, O) floats, of which the first S * (9 * O * 96 + O) are written,
 *          S = orn_debug_wgrad16_split(H, W, O, smax); dwf [O][C][3][3], dbf [O]: overwritten, every element, un-scaled by 1 / gs.
 *   head:  (NULL: none) the head's dW / db finish as trailing work-groups of the first launch: partial [blocks][3 C + 3] as the head
 *          backward leaves them, dw [3][C], db [3] = their column sums / gs.
 *   stem:  (NULL: none) the B == 1 stem backward in its deferred form, arguments as orn_debug_stem_bwd_slabs_act: its first kernel
 *          trails the first launch (behind the head's work-groups), its last kernel is one more y slice of the second.  A non-finite
 *          row of either kernel raises the flag of the scale state.
 *   gs > 0: the scale the 16-bit gradients carry.  use_state == 0: 1 / gs travels by value, no scale state (flag may be NULL).
 *          use_state != 0, the engine's form: a scale state of the entry's own (allocated and freed inside, `stream` synchronised) holds
 *          gs and 1 / gs; *flag: its flag word after the call (1: a dwf, dbf, head dw / db or stem element was not finite).  Same bits.
 *   side:  1: the launch keeps the default wave priority, as on the engine's side stream.  act: of the stem job.
 *   Refused with ORN_E_ARG and nothing launched: a null pointer where one is needed, n outside 0..ORN_MAX_LAYERS, H, W or s below 1, the
 *   launcher's own "wgrad_bf16: unsupported" conditions (C outside 1..96, O % 32 != 0, O % s^2 != 0), head blocks or C below 1, stem sizes
 *   below 1, gs <= 0, an unknown act; ORN_E_WS: a stem workspace below orn_stem_bwd_ws_bytes(1, Hd, Nout).
 * wgrad16_split / wgrad16_ws_floats: orn_wgrad_bf16_split and orn_wgrad_bf16_ws_floats themselves (no GPU is touched);
 * tests/test_wgrad16_split_host.py keeps S * (9 * O * 96 + O) <= ws_floats for every cap. */
typedef struct orn_debug_wgrad16_job {
    const void *xpad, *dypad;
    int32_t H, W, C, O, s, smax;
    float *slabs, *dwf, *dbf;
} orn_debug_wgrad16_job;
typedef struct orn_debug_wgrad16_head {
    const float *partial;
    int32_t blocks, C;
    float *dw, *db;
} orn_debug_wgrad16_head;
typedef struct orn_debug_wgrad16_stem {
    const float *embed, *w1, *pre1, *h1, *pre2, *dh2_slabs;
    int32_t nslab, E, Hd, Nout;
    float *dw0, *db0, *dw1, *db1, *ws;
    size_t ws_bytes;
} orn_debug_wgrad16_stem;
ORN_API int orn_debug_wgrad16_split(int H, int W, int O, int smax);
ORN_API size_t orn_debug_wgrad16_ws_floats(int H, int W, int O);
ORN_API int orn_debug_wgrad16_step_bf16(int n, const orn_debug_wgrad16_job *jobs, const orn_debug_wgrad16_head *head,
                                        const orn_debug_wgrad16_stem *stem, float gs, int use_state, int side, int act, int *flag,
                                        void *stream);
ORN_API int orn_debug_wgrad16_step_f16(int n, const orn_debug_wgrad16_job *jobs, const orn_debug_wgrad16_head *head,
                                       const orn_debug_wgrad16_stem *stem, float gs, int use_state, int side, int act, int *flag,
                                       void *stream);
#ifdef ORN_CONV_STAMP
/* Diagnostic build -DORN_CONV_STAMP only: buffer of 128 uint64 per work-group that receives the conv kernel's phase stamps. */
ORN_API void orn_debug_set_stamps(void *buf);
#endif
#ifdef __cplusplus
}
#endif
#endif /* ORN_DEBUG_H_ */
