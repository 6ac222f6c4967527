// Internal (non-exported) launchers shared between the op files and the engine.
#pragma once
#include "orn_common.h"

// orn_elementwise.hip
int orn_launch_linear_silu(const float *x, const int *row_idx, size_t row_stride, const float *w, const float *b,
                           int B, int K, int N, float *pre, float *y, hipStream_t st, int act);
int orn_launch_stem_bwd(const float *embed, const int *row_idx, size_t row_stride, const float *w1, const float *pre1,
                        const float *h1, const float *pre2, const float *dh2, int B, int E, int Hd, int Nout,
                        float *dw0, float *db0, float *dw1, float *db1, float *ws, hipStream_t st, int dh2_nslab,
                        OrnStemW0Job *defer_w0,    // defer_w0 (B == 1): the last kernel is returned as a job instead of launched
                        OrnStemL2Job *defer_l2,    // defer_l2 (with defer_w0): so is the first one (it then has to run in an EARLIER launch than w0)
                        int act,             // ORN_ACT_*; a deferred job must be run by a launch instantiated for the same one
                        OrnScaleState *sc = nullptr);    // (B == 1) a non-finite row of the l2 block / of a deferred w0 job raises its flag
// dh2_nslab > 1 (B == 1): dh2 holds that many partial rows of Nout floats, summed in fixed order by the first kernel
size_t orn_stem_bwd_ws_floats(int B, int Hd, int Nout);
int orn_launch_head_fwd(const float *a, const float *w, const float *b, int B, int C, size_t HW, int sigmoid,
                        float *out, hipStream_t st, bool z_input,    // z_input: `a` holds the pre-activation, the activation is applied here
                        int act);
int orn_launch_head_bwd(const float *a, const float *w, const float *out, const float *dout, int B, int C, size_t HW,
                        int sigmoid, float *da, float *dw, float *db, float *ws, hipStream_t st);
int orn_launch_adam(float *p, const float *g, float *m, float *v, size_t n, double lr, int step, const OrnStepCur *sp,
                    double beta1, double beta2, double eps, float inv_gscale, hipStream_t st, const float *gmask = nullptr,
                    OrnScaleState *sc = nullptr,    // sc: skip the update while its flag is up
                    OrnScaleState *sc_master = nullptr,    // (engine: the entry that counts skipped steps; default sc itself)
                    OrnScaleState *mirror = nullptr,       // (engine, deferred last block) the skip decision is also stored into mirror->mirrored
                    bool count_skip = true,                // false: a skipped launch does not count (the step's other Adam launch does)
                    OrnScaleState *late = nullptr);        // (side branch) a skip of sc->flag alone, not mirrored, counts in late->late_skipped
// Batched step (orn_engine_train_steps_batch): the gradient slots the backward writes directly, as ranges of the arena (floats;
// 2 per block + the head's 2 + the stem's 4).  blk_end[r]: work-groups of ranges 0..r (ORN_ACCUM_CHUNK floats each).
#define ORN_ACCUM_MAX_RANGES (2 * ORN_MAX_LAYERS + 6)
#define ORN_ACCUM_CHUNK 2048
struct OrnAccumTable { int n; int blk_end[ORN_ACCUM_MAX_RANGES]; int64_t off[ORN_ACCUM_MAX_RANGES], len[ORN_ACCUM_MAX_RANGES]; };
// mode 0 (first frame): acc = g;  1: acc = acc + g;  2 (last frame): g = (acc + g) * inv_b, one rounded multiply
int orn_launch_grad_accum(const OrnAccumTable &t, float *g, float *acc, int mode, float inv_b, hipStream_t st);
// per-frame stats [B][8] (the loss finalize's records) -> the optimiser step's ring record at cur->slot, means in double
int orn_launch_batch_stats(const float *frame_stats, int B, const OrnStepCur *cur, float *ring, hipStream_t st);

// orn_stage0.hip: the fp32 block below the first 16-bit one (tiny stem image), forward / backward as one launch each
bool orn_stage0_supported(int C, int O, int H, int W, int s);
int orn_stage0_slabs(int O, int s);
struct OrnPrepLayer;      // (below) 16-bit operand copies of later blocks' kernels, written by rider work-groups of this launch
int orn_launch_stage0_fwd(const float *x, const float *wf, const float *bf, int C, int O, int H, int W, int s, float *z,
                          void *xpad_next, int Cp, int precision, hipStream_t st, int n_prep, const OrnPrepLayer *prep,
                          const void *pack, int pack_t_blocks,    // pack: the merge backward's T -> Th copies as further riders
                          int act);
int orn_launch_stage0_bwd(const float *x, const float *wf, const float *z, const float *dxn, int nslab, int Cp, float inv_gs, int C,
                          int O, int H, int W, int s, float *slabs, float *dx, float *dwf, float *dbf, hipStream_t st,
                          const OrnScaleState *sc,    // sc: 1/scale from the device state instead of inv_gs
                          int act);

// orn_merge.hip
int orn_launch_merge_fwd(const float *w3x3, const float *b3x3, const float *w3x1, const float *b3x1,
                         const float *w1x3, const float *b1x3, const float *w1, const float *w2, const float *w3,
                         int C, int O, float *T, float *wf, float *bf, hipStream_t st);
int orn_launch_merge_bwd(const float *g, const float *dbf, const float *w1, const float *w2, const float *w3,
                         const float *T, int C, int O, float *d3x3, float *db3x3, float *d3x1, float *db3x1,
                         float *d1x3, float *db1x3, float *dw1, float *dw2, float *dw3, float *ws, hipStream_t st);

// grouped merge (engine): all ERB layers per launch
struct OrnMergeLayer {
    int C, O;
    const float *w3x3, *w3x1, *w1x3, *w1, *w2, *w3;   // parameters
    const float *b3x3, *b1x3, *b3x1; float *bf;       // optional: bias merge folded into the S GEMM (null: separate launch)
    float *T, *wf;                                    // forward products
    float *w2t;                                       // optional: tap-major copy of w2, [9][O][2C] (orn_launch_w2_transpose); the T products then read 16-byte rows
    const float *g;                                   // dL/dWf (in the gradient arena)
    float *dT, *dw1p, *dw2, *dw3;                     // backward scratch / outputs
    float *dw2t;                                      // 16-bit modes: dW2 tap-major [9][O][2C], interleaved by the tail kernel
    // 16-bit fast layers (engine): the S GEMM's epilogue also writes the conv kernels' operand copies (half_kind 1 bf16 / 2 fp16)
    int half_kind, s2, Cp;
    void *wb, *wd;
    float *biasp;
};
size_t orn_merge_group_bytes();
// W2 [O][2C][3][3] -> w2t [9][O][2C] for every layer with a w2t buffer, one launch (first launch of the forward merge)
// (pack / par_blocks: the parameter-side half copies of the merge backward's operands ride behind the transposes)
int orn_launch_w2_transpose(int n_layers, const OrnMergeLayer *L, hipStream_t st, const void *pack = nullptr, int par_blocks = 0);
// problem tables of the grouped launches: 0 = T, 1 = S (forward); fp32_bwd: also 2 = {dW3, dT}, 3 = {dW2, dW1 partials}.
// tiles[q]: work-groups of table q's launch, to be handed to the launchers below (0: table not built)
int orn_merge_groups_build(void *dev_tables, int n_layers, const OrnMergeLayer *L, bool fp32_bwd, int tiles[4]);
int orn_launch_merge_group(const void *dev_tables, int which, int tiles, hipStream_t st);   // which = 2 / 3 (fp32 engine)
int orn_launch_merge_group_linear(const void *dev_tables, int which, int tiles, const OrnLinearJob &job, hipStream_t st,
                                  const void *pack, int pack_blocks,    // pack: trailing T -> Th pack jobs (orn_merge_h16_pack)
                                  int act);                           // act: of the linear job

// orn_merge_h16.hip: merge backward GEMMs of the 16-bit engine modes (packed half operands, fragments from global)
size_t orn_merge_h16_layer_halfs(int C, int O);
size_t orn_merge_h16_table_bytes();
size_t orn_merge_h16_host_bytes();
int orn_merge_h16_build(void *dev_tables, void *host, int n_layers, const OrnMergeLayer *L, void *const *bufs, OrnScaleState *sc);
int orn_launch_merge_h16_bwd(const void *dev_tables, const void *host, hipStream_t st, OrnScaleState *sc = nullptr);   // sc: the launching step's scale-state entry
const void *orn_merge_h16_pack(const void *host, int *par_blocks, int *t_blocks);
// the parameter-side (which = 1) or T -> Th (which = 2) pack jobs of the set as a launch of their own (instead of riders)
int orn_launch_merge_h16_pack_jobs(const void *host, int which, hipStream_t st);

// per-layer elementwise tail of the merge backward, all layers per launch (both precisions)
struct OrnMergeMisc {
    int C, O;
    const float *g, *dbf, *dw1p;                                      // backward inputs (dWf, dbf live in the grad arena)
    float *d3x1, *db3x1, *d1x3, *db1x3, *dw1;                         // backward outputs
    const float *dw2t; float *dw2;                                    // optional: dW2 [9][O][2C] -> [O][2C][3][3]
};
int orn_launch_merge_bwd_tail_all(int n, const OrnMergeMisc *L, hipStream_t st);

// orn_merge_lin.hip: online merge of the ACB / RepVGG / ECB blocks (include/orn.h, N7), all blocks of an engine per launch
struct OrnBranchLayer {
    int kind, C, O;                   // ORN_BRANCH_*
    orn_branch_ptrs p;                // parameters (read only)
    float *wf, *bf;                   // forward: the merged kernel and bias
    const float *g, *dbf;             // backward: dL/dwf, dL/dbf ...
    orn_branch_ptrs d;                // ... and where each gradient goes (d.w3x3 == g, d.b3x3 == dbf: no copy)
    float *dwAp;                      // ECB: orn_branch_merge_bwd_ws_floats floats, the slabs of dwA
};
size_t orn_branch_merge_bwd_ws_floats(int kind, int C, int O);
int orn_launch_branch_merge_fwd(int n, const OrnBranchLayer *L, hipStream_t st);
int orn_launch_branch_merge_bwd(int n, const OrnBranchLayer *L, hipStream_t st);    // ECB: two launches (the slabs of dwA are summed by the second)

// orn_conv_f32.hip
int orn_launch_conv3x3_f32(const float *x, const float *w, const float *bias, int B, int C, int O, int H, int W,
                           int s, int epi, float *z, float *out, hipStream_t st, float *split_ws, int act);
// head: fp32 engine only -- the last block's backward starts from the head's (out, dout) instead of da (orn_launch_head_bwd_fused_f32)
struct OrnHeadBwdFuse { const float *w, *out, *dout; int sigmoid; float *dw, *db, *hws; };
int orn_launch_conv_bwd_f32(const float *x, const float *wf, const float *z, const float *da, int B, int C, int O,
                            int H, int W, int s, float *dx, float *dwf, float *dbf, float *ws, hipStream_t st,
                            const OrnHeadBwdFuse *head, const float *wd_ready,    // wd_ready: the flipped / transposed kernel, already made
                            int act);
int orn_launch_flip_transpose_all(int n, const float *const *wf, float *const *wd, const int *O, const int *C, hipStream_t st);
int orn_head_bwd_fused_f32_blocks(int H, int W);
int orn_launch_head_bwd_fused_f32(const float *z, const float *w, const float *out, const float *dout, int Cn, int H, int W,
                                  int sigmoid, float *dy, float *dbp, float *dw, float *db, float *hws, hipStream_t st, int act);

// orn_side_head.hip, orn_side_head_f32.hip: the heads of the stages below the last one (multi-resolution engine; include/orn.h, N8).
// 16-bit entries (OrnHalfOps::side_head_fwd / _bwd): z is the block's channels-last pre-activation, dypad its padded un-shuffled gradient
// buffer, which the backward ADDS to; fp32 entries (orn_side_head_f32.hip): the NCHW activation and the gradient with respect to it.
// sc: the step's scale-state entry (the scale is read from it, a non-finite pre-activation / dw / db raises its flag).
// ws: orn_side_head_bwd_ws_floats floats.
#define SH_MAXC 512              // LDS copy of W [3][C] + b
#define SH_PPT 8                 // 16-bit backward: a work-group takes SH_PPT x 64 pixels (the larger of the two layouts' partial tables)
size_t orn_side_head_bwd_ws_floats(int C, int H, int W);
// column sums of either layout's partials [rows][3 C + 3] times inv -> dw, db.  sc (engine): non-finite sums raise its flag; scaled: the
// partials carry its scale (inv is then read from it)
int orn_launch_side_head_finish(const float *partial, int rows, int C, float inv, float *dw, float *db, hipStream_t st, OrnScaleState *sc,
                                bool scaled);
int orn_launch_side_head_fwd_f32(const float *a, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st,
                                 OrnScaleState *sc);
int orn_launch_side_head_bwd_f32(const float *a, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid,
                                 float lw, float *da, float *dw, float *db, float *ws, hipStream_t st, OrnScaleState *sc);

// orn_loss.hip
int orn_loss_init();
// The one table of loss ids (include/orn.h): loss = w_l1 * L1 + w_l2 * MSE + w_struct * (1 - s), weights of utils.py:142-172.
struct OrnLossSpec { double w_l1, w_l2, w_struct; int kind; };      // doubles: the gradient scales are formed in double
static inline const OrnLossSpec *orn_loss_spec_of(int loss_type)
{
    static const OrnLossSpec tab[ORN_LOSS_COUNT] = {
        /* L2       */ {0.0, 1.0, 0.0, ORN_LOSS_KIND_NONE},   /* L1       */ {1.0, 0.0, 0.0, ORN_LOSS_KIND_NONE},
        /* Fusion6  */ {0.7, 0.0, 0.3, ORN_LOSS_KIND_SSIM},   /* SSIM     */ {0.0, 0.0, 1.0, ORN_LOSS_KIND_SSIM},
        /* Fusion1  */ {0.0, 0.3, 0.7, ORN_LOSS_KIND_SSIM},   /* Fusion2  */ {0.3, 0.0, 0.7, ORN_LOSS_KIND_SSIM},
        /* Fusion3  */ {0.0, 0.5, 0.5, ORN_LOSS_KIND_SSIM},   /* Fusion4  */ {0.5, 0.0, 0.5, ORN_LOSS_KIND_SSIM},
        /* Fusion5  */ {0.0, 0.7, 0.3, ORN_LOSS_KIND_SSIM},   /* Fusion7  */ {0.3, 0.7, 0.0, ORN_LOSS_KIND_NONE},
        /* Fusion8  */ {0.5, 0.5, 0.0, ORN_LOSS_KIND_NONE},   /* Fusion9  */ {0.9, 0.0, 0.1, ORN_LOSS_KIND_SSIM},
        /* Fusion10 */ {0.7, 0.0, 0.3, ORN_LOSS_KIND_MSSSIM}, /* Fusion11 */ {0.9, 0.0, 0.1, ORN_LOSS_KIND_MSSSIM},
        /* Fusion12 */ {0.8, 0.0, 0.2, ORN_LOSS_KIND_MSSSIM}};
    return (loss_type >= 0 && loss_type < ORN_LOSS_COUNT) ? &tab[loss_type] : nullptr;
}
int orn_launch_loss(const float *pred, const float *target, const int *frame_idx, size_t frame_stride, int B, int Ch,
                    int H, int W, int loss_type, float loss_scale, float *stats, float *dpred, float *ws,
                    hipStream_t st, const OrnStepCur *cur = nullptr, float *ring = nullptr, OrnScaleState *sc = nullptr,
                    const float *tstats = nullptr,    // tstats: orn_loss_target_stats of the SAME frame table (SSIM kinds; indexed by *frame_idx)
                    OrnLossFinalJob *defer = nullptr);   // defer: the finalize stage is returned as a job instead of launched
// The loss stage of a split step (orn_engine_step_backward): the caller supplies dLoss/dpred and the loss value (device; optional).
// Two launches: per-tile {|d|, d^2} partials of pred - target[*frame_idx] + a NaN / inf scan of dpred into sc->flag, then a
// one-work-group finalize (stats and ring record {loss, L1, MSE, 0, PSNR, ...}; a non-finite loss raises the flag).  dpred null:
// the step is abandoned -- no scan, the flag goes up.  ws: orn_loss_ws_bytes(1, Ch, H, W) bytes.
int orn_launch_loss_ext(const float *pred, const float *target, const int *frame_idx, size_t frame_stride, int Ch, int H, int W,
                        const float *dpred, const float *loss, float *stats, float *ws, hipStream_t st, const OrnStepCur *cur,
                        float *ring, OrnScaleState *sc);
void orn_gauss_taps(float g[11]);        // pytorch_msssim _fspecial_gauss_1d(11, 1.5)
// The five level launches of the batched MS-SSIM on F groups of Ch planes (no finalize); the pooled planes of levels 1..4 and the
// per-tile partials stay in ws (orn_msssim_pyramid_floats) and are described by *out.
struct OrnMsPyramid {
    int Hs[5], Ws[5], nblk[5]; float nmap[5];
    float *pooled[5][2];         // [level 1..4][pred, target]: [F*Ch][Hs][Ws]
    float *part;                 // level l at part_off[l]: [F*Ch][nblk[l]][2] = {ssim, cs} tile sums
    size_t part_off[5];
};
static inline int orn_msssim_pooled(int n) { return (n + 2 * (n % 2)) / 2; }      // avg_pool2d(2, padding = n % 2)
static inline void orn_msssim_geom(int H, int W, int Hs[5], int Ws[5])
{
    Hs[0] = H; Ws[0] = W;
    for (int l = 1; l < 5; ++l) { Hs[l] = orn_msssim_pooled(Hs[l - 1]); Ws[l] = orn_msssim_pooled(Ws[l - 1]); }
}
// The same workspace as float offsets from its start (what OrnMsPyramid holds as pointers); total: its size.
struct OrnMsLayout {
    int Hs[5], Ws[5], nblk[5]; float nmap[5];
    size_t pooled[5][2], part, part_off[5], total;       // level l's partials at part + part_off[l]
};
void orn_msssim_layout(size_t planes, int H, int W, OrnMsLayout *out);
size_t orn_msssim_pyramid_floats(size_t planes, int H, int W);
int orn_launch_msssim_levels(const float *pred, const float *targets, const int32_t *rows, int F, int Ch, int H, int W, float *ws,
                             hipStream_t st, OrnMsPyramid *out);
// orn_loss_msssim.hip: the MS-SSIM losses (kind ORN_LOSS_KIND_MSSSIM).  ms_ws: orn_loss_msssim_ws_floats floats, 16-byte aligned.
// Writes dpred (null: forward only) and the level-0 {|d|, d^2} tile partials part_l1 (the 16x64 tiling of orn_launch_loss);
// *ms_val: where the coefficient launch leaves the MS-SSIM value for the finalize stage.
int orn_loss_msssim_init();
size_t orn_loss_msssim_ws_floats(size_t planes, int H, int W);
// float offsets inside ms_ws behind the pyramid: the gradient planes of levels 1..4 (grad[0] unused), the coefficient table
// [5][planes] (the value follows it)
void orn_loss_msssim_layout(size_t planes, int H, int W, size_t grad[5], size_t *coef);
int orn_launch_loss_msssim(const float *pred, const float *target, const int *frame_idx, size_t frame_stride, int planes, int H, int W,
                           float g_l1, float g_l2, float w_struct_scaled, float *dpred, float *part_l1, float *ms_ws, hipStream_t st,
                           const float **ms_val);
// Batched MS-SSIM (orn_msssim_frames): one chunk of F frames, pred [F][Ch][H][W] against targets[rows[k]] (rows null: targets[k]),
// out [F]; ws: orn_msssim_frames_ws_bytes(F, ...) bytes.  Six launches, no copy, no sync.  orn_msssim_frames_chunk: the most frames
// (<= n) whose workspace fits in ws_bytes, 0 if not even one.
int orn_msssim_frames_chunk(int n, int Ch, int H, int W, size_t ws_bytes);
int orn_launch_msssim_frames(const float *pred, const float *targets, const int32_t *rows, int F, int Ch, int H, int W, float *out,
                             float *ws, hipStream_t st);

// The 16-bit MFMA fast path (channels-last buffers, see the header of orn_conv_bf16.hip): orn_conv_fwd_bf16.hip, orn_conv_bf16.hip
// (dgrad), orn_conv2_bf16.hip (both, large images), orn_wgrad_bf16.hip, orn_side_head.hip, orn_decode_out.hip and orn_ops_bf16.hip,
// with orn_h16.h between them.  These files are built twice (bf16 and, with -DORN_FP16, IEEE half) and hold only code that names the
// element type h16: the typed kernels and their launchers.  Everything else reaches either build through the type-erased table that
// orn_ops_bf16.hip fills -- the engine, and the test entry points of include/orn_debug.h (orn_debug.hip); the fp32 kernels that serve
// the same stages are built once (orn_side_head_f32.hip, orn_decode_out_f32.hip).
// Limits of the launchers behind the table that argument checks outside these files repeat:
#define STAGE_OUT_MAXC SH_MAXC   // stage_out: LDS copy of W [3][C] + b, as the side heads
static inline bool orn_head_bwd_c_ok(int C) { return C == 32 || C == 64 || C == 96 || C == 128; }   // head_bwd: one instantiation per C / 32
struct OrnPrepLayer { const float *wf, *bf; int O, C, s; void *wb, *wd; float *biasp; int Cp; };   // Cp: channel stride (0: = C)
// deferred split-K reduction of a layer's wgrad slabs (wgrad called with dwf == nullptr leaves them in `slabs`)
struct OrnWgradReduce { const float *slabs; int H, W, C, O, s; float gscale; float *dwf, *dbf; OrnScaleState *sc; int smax; };   // sc (optional): 1/scale from the device state, non-finite results raise its flag
// deferred reduction of the 16-bit head backward's per-block partials (head_bwd called with dw == nullptr leaves them in ws)
struct OrnHeadFinish { const float *partial; int blocks, C; float gscale; float *dw, *db; OrnScaleState *sc; };
struct OrnWgradJob { const void *xpad, *dypad; int H, W, C, O, s; float *slabs; int smax; };   // wgrad into slabs, reduction deferred; smax > 0: at most that many split-K slabs (the reduction must be told the same)
// Decode output stage (orn_decode_out.hip): what one decoded frame leaves behind.  Every output is optional (null: not wanted).
//   rgb8 [H][W][3] bytes, q = (uint8) clamp(x*255 + 0.5, 0, 255); img [3][H][W] fp32; stats {mse, psnr} of x and of q/255 against
//   targets[*row] ([3][H][W] fp32 each).  ws: ORN_DECODE_WS_FLOATS floats, the last of them a ticket counter that is zero
//   between launches (per-block partial sums in front of it; the last block to arrive sums them in fixed order).
#define ORN_DECODE_MAX_BLOCKS 8192
#define ORN_DECODE_WS_FLOATS (2 * ORN_DECODE_MAX_BLOCKS + 64)
struct OrnDecodeOut { const float *targets; const int32_t *row; uint8_t *rgb8; float *img, *stats; float *ws; };
// fp32 engine: the same stage from the planar image the fp32 head wrote (orn_decode_out_f32.hip)
int orn_launch_decode_out_f32(const float *src, size_t HW, const OrnDecodeOut &o, hipStream_t st);
struct OrnHalfOps {
    int (*conv_fwd)(const void *xpad, const void *wb, const float *bias_p, int H, int W, int Cin, int O, int s, void *z, void *apad,
                    hipStream_t st, int c_real, int act);   // c_real <= Cin: input channels that are not zero padding; act: ORN_ACT_* (here and below)
    int (*conv_dgrad)(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev, void *dyprev, int sp,
                      float *dx_f32, hipStream_t st, int c_real, int act);   // c_real: output channels that are not zero padding
    size_t (*wgrad_ws_floats)(int H, int W, int O);
    int (*wgrad_split)(int H, int W, int O, int smax);   // slab count of a layer under the caller's cap (below 8: none)
    int (*wgrad_batch)(int n, const OrnWgradJob *J, hipStream_t st, const OrnHeadFinish *hf, const OrnStemL2Job *l2, int side, int act);   // side: launched on the engine's side stream (default wave priority)   // several layers' slabs in one launch (+ optional head finish, + the stem backward's first kernel)
    int (*wgrad_reduce_all)(int n, const OrnWgradReduce *L, hipStream_t st, const OrnStemW0Job *w0, int act);   // all layers' reductions in one launch (+ the stem backward's last kernel)
    int (*prep_all)(int n, const OrnPrepLayer *L, hipStream_t st);
    int (*to_nhwc)(const float *src, int C, int Cp, int H, int W, void *dst, hipStream_t st);
    int (*to_nchw_f32)(const float *src, int C, int Cp, int H, int W, int nslab, float scale, float *dst, hipStream_t st, const OrnScaleState *sc);
    int (*dgrad_f32_slabs)(int H, int W, int O);
    int (*head_fwd)(const void *z, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st, int act);
    size_t (*head_bwd_ws_floats)(int C);
    int (*head_bwd_blocks)(int H, int W);
    int (*head_bwd)(const void *z, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid, int sp,
                    float gs_up, void *dypad, float *dw, float *db, float *ws, hipStream_t st, const OrnScaleState *sc,
                    const OrnLossFinalJob *fin, int act);   // sc: gs from the device state; fin (optional): the loss's finalize stage as one more work-group
    // decode: head forward on z + the output stage above in one kernel (same per-pixel arithmetic as head_fwd)
    int (*decode_out)(const void *z, const float *w, const float *b, int C, size_t HW, int sigmoid, const OrnDecodeOut &o, hipStream_t st, int act);
    // multi-resolution engine: the head of a stage below the last (orn_side_head.hip, above)
    int (*side_head_fwd)(const void *z, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st, OrnScaleState *sc, int act);
    int (*side_head_bwd)(const void *z, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid, int sp, float lw,
                         float gs, void *dypad, float *dw, float *db, float *ws, hipStream_t st, OrnScaleState *sc, int act);
    // per-stage evaluation (orn_engine_eval_stages): a side stage's head on its block's z + the output stage in one kernel (same per-pixel
    // arithmetic as side_head_fwd)
    int (*stage_out)(const void *z, const float *w, const float *b, int C, size_t HW, int sigmoid, const OrnDecodeOut &o, hipStream_t st, int act);
};
const OrnHalfOps *orn_half_ops_bf16();
const OrnHalfOps *orn_half_ops_f16();
