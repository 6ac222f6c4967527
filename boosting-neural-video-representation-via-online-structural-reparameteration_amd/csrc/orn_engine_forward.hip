// The engine's forward (orn_engine.h) and the entries that run nothing else: decode, multi-frame decode, evaluation.
#include "orn_engine.h"

// Multi-resolution heads, stage i < n_layers - 1, forward: the image of the block's output (16-bit layers: from the channels-last
// pre-activation; fp32 layers: from the NCHW activation), then the engine's loss on (image, the stage's target of the step's
// frame) with its own finalize launch: stats {loss_i, .., psnr_i}, dLoss_i/dout_i un-weighted and un-scaled (lw and the loss scale
// enter in the head's backward), a non-finite loss raises the step's flag.
static int side_forward(orn_engine *e, int i, const int *frame_idx, hipStream_t st, OrnScaleState *sc)
{
    const orn_engine_desc &d = e->d;
    const orn_engine::SideStage &s = e->stage[i];
    const float *w = e->params + d.side_head_w[i], *b = e->params + d.side_head_b[i];
    const size_t HW = (size_t)s.H * s.W;
    if (i >= e->ff)
        ORN_TRY(e->ops->side_head_fwd(e->L[i].zb, w, b, s.C, HW, d.sigmoid, s.img, st, sc, d.act));
    else
        ORN_TRY(orn_launch_side_head_fwd_f32(e->L[i].a, w, b, s.C, HW, d.sigmoid, s.img, st, sc));
    return orn_launch_loss(s.img, s.targets, frame_idx, 3 * HW, 1, 3, s.H, s.W, d.loss_type, 1.0f, s.stats, s.dimg, s.loss_ws, st, nullptr, nullptr, sc,
                           orn_loss_spec_of(d.loss_type)->kind == ORN_LOSS_KIND_SSIM ? s.tstats : nullptr, nullptr);
}

int forward(orn_engine *e, const float *embeds, const int *row_idx, bool keep_z, hipStream_t st, int top, int set, bool head, OrnScaleState *side_sc)
{
    const bool merge = set != MERGE_NONE;
    const orn_engine_desc &d = e->d;
    const int Nout = d.fc_h * d.fc_w * d.fc_dim;
    float *P = e->params;
    const OrnLinearJob lin1 = {embeds, row_idx, (size_t)d.embed_len, P + d.stem_w0, P + d.stem_b0, 1, d.embed_len, d.stem_dim, e->pre1, e->h1};
    const OrnLinearJob lin2 = {e->h1, nullptr, 0, P + d.stem_w1, P + d.stem_b1, 1, d.stem_dim, Nout, e->pre2, e->h2};
    const float *x = e->h2;
    const int nl = d.n_layers, ff = e->ff;
    assert(top >= 0 && top < nl);
    const void *pack_t = nullptr;
    int pack_t_blocks = 0;
    if (d.erb && merge) {
        // online re-parameterisation of every layer (model.py:534): weights only, so all layers up front -- two grouped
        // launches (T, then S with the bias merge b3x3 + (b1x3 + b3x1) in its first tile column), each carrying one of
        // the stem's two linear layers as extra work-groups
        // half operand copies for the merge BACKWARD (training step, 16-bit modes) as riders: the parameter-side ones behind
        // the W2 transposes, T -> Th behind the first block's launch (or, without it, behind the S products)
        const orn_engine::MergeSet &ms = e->mset[set];
        int pk_par = 0, pk_t = 0;
        const void *pk = (keep_z && ms.mh_host) ? orn_merge_h16_pack(ms.mh_host, &pk_par, &pk_t) : nullptr;
        ORN_TRY(orn_launch_w2_transpose(ms.n, ms.ml, st, pk, pk_par));
        ORN_TRY(orn_launch_merge_group_linear(ms.tables, 0, ms.tiles[0], lin1, st, nullptr, 0, d.act));
        ORN_TRY(orn_launch_merge_group_linear(ms.tables, 1, ms.tiles[1], lin2, st, e->stage0 ? nullptr : pk, e->stage0 ? 0 : pk_t, d.act));
        pack_t = e->stage0 ? pk : nullptr; pack_t_blocks = e->stage0 ? pk_t : 0;
    } else {
        ORN_TRY(orn_launch_linear_silu(lin1.x, lin1.row_idx, lin1.row_stride, lin1.w, lin1.bias, 1, lin1.K, lin1.N, lin1.pre, lin1.y, st, d.act));
        ORN_TRY(orn_launch_linear_silu(lin2.x, nullptr, 0, lin2.w, lin2.bias, 1, lin2.K, lin2.N, lin2.pre, lin2.y, st, d.act));
    }
    if (e->nbr && merge) ORN_TRY(orn_launch_branch_merge_fwd(e->nbr, e->bl, st));      // ACB / RepVGG / ECB: (wf, bf) of every block, one launch
    if (ff < nl && !d.erb && merge) {      // 16-bit operand copies of every fast layer's kernel, one launch (ERB: written by the merge's S launch)
        OrnPrepLayer pl[ORN_MAX_LAYERS];
        const int np = (set == 1 ? nl - 1 : nl) - ff;       // (pipelined step: the side branch prepares the last block's)
        for (int i = ff; i < ff + np; ++i) pl[i - ff] = prep_layer(e, i);
        ORN_TRY(e->ops->prep_all(np, pl, st));
    }
    for (int i = 0; i <= top; ++i) {       // (top < nl - 1, orn_engine_eval_stages: the blocks above it and the last head are not launched)
        const orn_layer_desc &l = d.layer[i];
        LayerBuf &b = e->L[i];
        if (i < ff) {
            if (e->prof) (void)hipEventRecord(e->prof_ev[2 * i], st);
            if (e->stage0) { // conv + PixelShuffle + SiLU straight into layer 1's 16-bit input (b.z in the fused pair's own layout)
                // ERB: the 16-bit operand copies of the later blocks' merged kernels ride on this launch (orn_prep_rider.h)
                OrnPrepLayer pl[ORN_MAX_LAYERS];
                int np = 0;
                if (d.erb && merge)
                    for (int j = ff; j < (set == 1 ? nl - 1 : nl); ++j) pl[np++] = prep_layer(e, j);
                ORN_TRY(orn_launch_stage0_fwd(x, b.wf, b.bf, l.C, l.O, l.H, l.W, l.s, keep_z ? b.z : nullptr, e->L[1].xpad, ORN_FAST_C,
                                              d.precision, st, np, pl, pack_t, pack_t_blocks, d.act));
            }
            else
            {
                // fp32 engine, training step, last block: nothing but the head reads its activation, and the head's backward is fused with
                // this block's (it reads z): store z only and let the head's forward form SiLU(z) (354 MB less written at 720p)
                const bool z_only = keep_z && i == nl - 1 && f32_head_on_z(e);
                ORN_TRY(orn_launch_conv3x3_f32(x, b.wf, b.bf, 1, l.C, l.O, l.H, l.W, l.s, 1, keep_z ? b.z : nullptr, z_only ? nullptr : b.a, st, nullptr,
                                               d.act));
            }
            if (e->prof) (void)hipEventRecord(e->prof_ev[2 * i + 1], st);
            x = b.a;
        } else {
            if (i == ff && !e->stage0) ORN_TRY(e->ops->to_nhwc(x, l.C, ORN_FAST_C, l.H, l.W, b.xpad, st));
            if (e->prof) (void)hipEventRecord(e->prof_ev[2 * i], st);
            const bool last = (i + 1 == nl);
            const bool fill_next = i < top;            // the next block's input: the last block and an early exit's top have none to fill
            // pipelined step: the side branch of the previous step still reads the last block's input buffer (its weight gradient)
            // until ev_wgrad, and writes that block's merged kernel (and the head's parameters) until ev_join
            if (e->side_busy && i + 3 == nl && e->side_below) ORN_HIP(hipStreamWaitEvent(st, e->ev_below, 0));   // (this conv overwrites the input of the block below the last)
            if (e->side_busy && i + 2 == nl) ORN_HIP(hipStreamWaitEvent(st, e->ev_wgrad, 0));
            if (e->side_busy && last) { ORN_HIP(hipStreamWaitEvent(st, e->ev_join, 0)); e->side_busy = false; }
            ORN_TRY(e->ops->conv_fwd(b.xpad, b.wb, b.biasp, l.H, l.W, ORN_FAST_C, l.O, l.s, b.zb, fill_next ? e->L[i + 1].xpad : nullptr, st, l.C, d.act));
            if (e->prof) (void)hipEventRecord(e->prof_ev[2 * i + 1], st);
        }
        if (side_sc && i + 1 < nl) ORN_TRY(side_forward(e, i, row_idx, st, side_sc));
    }
    if (top + 1 < nl) return 0;
    if (ff < nl) {
        if (head)
            ORN_TRY(e->ops->head_fwd(e->L[nl - 1].zb, P + d.head_w, P + d.head_b, e->Cn_last, (size_t)e->Hout * e->Wout, d.sigmoid, e->img, st,
                                     d.act));
    } else
    {
        const bool z_only = keep_z && f32_head_on_z(e);
        ORN_TRY(orn_launch_head_fwd(z_only ? e->L[nl - 1].z : x, P + d.head_w, P + d.head_b, 1, e->Cn_last, (size_t)e->Hout * e->Wout, d.sigmoid, e->img,
                                    st, z_only, d.act));
    }
    return 0;
}

extern "C" int orn_engine_decode(orn_engine *e, const float *embed, float *img, void *stream)
{
    ORN_REQUIRE(e && embed && img, "engine_decode: null pointer");
    ORN_REQUIRE_CLOSED(e, "engine_decode");
    hipStream_t st = (hipStream_t)stream;
    ORN_TRY(forward(e, embed, nullptr, false, st, e->d.n_layers - 1));
    hipError_t rc = hipMemcpyAsync(img, e->img, (size_t)3 * e->Hout * e->Wout * 4, hipMemcpyDeviceToDevice, st);
    if (rc != hipSuccess) { orn_set_error("engine_decode: copy failed: %s", hipGetErrorString(rc)); return (int)rc; }
    return 0;
}

// n frames back to back: frame 0 runs the full forward (the parameters may have changed since the last call), the others reuse
// its merged kernels and operand copies (MERGE_NONE); each ends in the decode output stage (orn_decode_out.hip) instead of
// head + copy (+ the caller's torch ops for bytes and PSNR).  main_eval.py:795-815, main_train.py:377-438.
// msssim (orn_engine_eval_frames): after every `chunk` decoded frames, the batched MS-SSIM launches (orn_loss.hip) on the chunk's
// fp32 planes -- the caller's img, or slots at the head of `ws` that the output kernel fills through its img output.
static int decode_frames(orn_engine *e, const float *embeds, const int32_t *rows, int32_t n, const float *targets, uint8_t *rgb8,
                         float *img, float *stats, float *msssim, float *ws, int chunk, hipStream_t st)
{
    assert(!e->side_busy);          // orn_engine_train_steps joins its side branch before it returns
    const orn_engine_desc &d = e->d;
    const size_t HW = (size_t)e->Hout * e->Wout;
    const bool fast = e->ff < d.n_layers;
    float *ms_ws = msssim ? ws + orn_align((size_t)chunk * 3 * HW * 4) / 4 : nullptr;
    if (stats && n > 0) ORN_HIP(hipMemsetAsync(e->dec_ws + 2 * ORN_DECODE_MAX_BLOCKS, 0, 64 * 4, st));      // the ticket starts at zero
    for (int32_t k = 0; k < n; ++k) {
        ORN_TRY(forward(e, embeds, rows + k, false, st, d.n_layers - 1, k == 0 ? 0 : MERGE_NONE, false));
        float *planes = img ? img + (size_t)k * HW * 3 : (msssim ? ws + (size_t)(k % chunk) * HW * 3 : nullptr);
        const OrnDecodeOut o = {targets, rows + k, rgb8 ? rgb8 + (size_t)k * HW * 3 : nullptr, planes,
                                stats ? stats + (size_t)k * 4 : nullptr, e->dec_ws};
        if (fast)
            ORN_TRY(e->ops->decode_out(e->L[d.n_layers - 1].zb, e->params + d.head_w, e->params + d.head_b, e->Cn_last, HW, d.sigmoid, o, st,
                                       d.act));
        else
            ORN_TRY(orn_launch_decode_out_f32(e->img, HW, o, st));
        if (msssim && ((k + 1) % chunk == 0 || k + 1 == n)) {
            const int32_t k0 = k / chunk * chunk;
            ORN_TRY(orn_launch_msssim_frames(img ? img + (size_t)k0 * HW * 3 : ws, targets, rows + k0, k + 1 - k0, 3, e->Hout, e->Wout,
                                             msssim + k0, ms_ws, st));
        }
    }
    return 0;
}

extern "C" int orn_engine_decode_frames(orn_engine *e, const float *embeds, const int32_t *rows, int32_t n, const float *targets,
                                        uint8_t *rgb8, float *img, float *stats, void *stream)
{
    ORN_REQUIRE(e && embeds, "engine_decode_frames: null engine / embeds");
    ORN_REQUIRE_CLOSED(e, "engine_decode_frames");
    ORN_REQUIRE(n >= 0 && (rows || n == 0), "engine_decode_frames: n=%d frames need a device array of n row indices", n);
    ORN_REQUIRE(rgb8 || img || stats, "engine_decode_frames: no output asked for (rgb8, img and stats are all null)");
    ORN_REQUIRE(!stats || targets, "engine_decode_frames: stats need targets");
    return decode_frames(e, embeds, rows, n, targets, rgb8, img, stats, nullptr, nullptr, 0, (hipStream_t)stream);
}

// `chunk` fp32 image slots [3][H][W], then the MS-SSIM workspace of a chunk of that many frames
extern "C" size_t orn_engine_eval_frames_ws_bytes(const orn_engine_desc *d, int chunk)
{
    if (chunk <= 0 || check_desc(d) != 0) return 0;
    const StageGeo g = stage_geometry(d);
    const int H = g.H[d->n_layers - 1], W = g.W[d->n_layers - 1];       // image size
    const size_t ms = orn_msssim_frames_ws_bytes(chunk, 3, H, W);
    return ms ? orn_align((size_t)chunk * 3 * H * W * 4) + ms : 0;
}

extern "C" int orn_engine_eval_frames(orn_engine *e, const float *embeds, const int32_t *rows, int32_t n, const float *targets,
                                      uint8_t *rgb8, float *img, float *stats, float *msssim, void *ws, size_t ws_bytes, void *stream)
{
    if (!msssim) return orn_engine_decode_frames(e, embeds, rows, n, targets, rgb8, img, stats, stream);
    ORN_REQUIRE(e && embeds, "engine_eval_frames: null engine / embeds");
    ORN_REQUIRE_CLOSED(e, "engine_eval_frames");
    ORN_REQUIRE(n >= 0 && (rows || n == 0), "engine_eval_frames: n=%d frames need a device array of n row indices", n);
    ORN_REQUIRE(targets, "engine_eval_frames: msssim needs targets");
    ORN_REQUIRE((e->Hout < e->Wout ? e->Hout : e->Wout) > 160, "engine_eval_frames: msssim: image side must exceed 160 (got %dx%d)", e->Hout, e->Wout);
    if (n == 0) return 0;
    ORN_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "engine_eval_frames: msssim needs a 16-byte aligned workspace");
    int chunk = n < 65535 / 3 ? n : 65535 / 3;
    while (chunk > 0 && orn_engine_eval_frames_ws_bytes(&e->d, chunk) > ws_bytes) --chunk;
    if (chunk < 1) { orn_set_error("engine_eval_frames: workspace %zu < %zu", ws_bytes, orn_engine_eval_frames_ws_bytes(&e->d, 1)); return ORN_E_WS; }
    return decode_frames(e, embeds, rows, n, targets, rgb8, img, stats, msssim, (float *)ws, chunk, (hipStream_t)stream);
}

// ---- N9  every stage of a multi-resolution fit: one forward per frame up to the highest stage asked for ----
// The caller's workspace, in floats: per stage with an MS-SSIM column `chunk` image slots [3][H_i][W_i], then ONE MS-SSIM workspace,
// the largest any of those stages needs for a chunk (their launches follow each other on one stream).  It starts with 64 unused
// floats, so that a valid request never sizes to 0, the error value.
struct StagesWs { size_t slot[ORN_MAX_LAYERS], ms, total; };
static size_t stages_ws_layout(const orn_engine_desc *d, uint32_t msssim_stages, int chunk, StagesWs *out)
{
    if (chunk <= 0 || chunk > 65535 / 3 || (d->n_layers < 32 && (msssim_stages >> d->n_layers) != 0)) return 0;
    const StageGeo g = stage_geometry(d);
    StagesWs L = {};
    size_t off = 64, ms_max = 0;
    for (int i = 0; i < d->n_layers; ++i) {
        if (!((msssim_stages >> i) & 1u)) continue;
        if ((g.H[i] < g.W[i] ? g.H[i] : g.W[i]) <= 160) return 0;
        const size_t ms = orn_msssim_frames_ws_bytes(chunk, 3, g.H[i], g.W[i]);
        if (!ms) return 0;
        L.slot[i] = off;
        off += al((size_t)chunk * 3 * g.H[i] * g.W[i]);
        if (ms > ms_max) ms_max = ms;
    }
    L.ms = off;
    off += al(ms_max / 4);
    L.total = off * 4;
    if (out) *out = L;
    return L.total;
}

extern "C" size_t orn_engine_eval_stages_ws_bytes(const orn_engine_desc *d, uint32_t msssim_stages, int chunk)
{
    if (check_desc(d) != 0) return 0;
    return stages_ws_layout(d, msssim_stages, chunk, nullptr);
}

extern "C" int orn_engine_eval_stages(orn_engine *e, const float *embeds, const int32_t *rows, int32_t n, const orn_stage_out *out, void *ws,
                                      size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(e && embeds && out, "engine_eval_stages: null engine / embeds / out");
    ORN_REQUIRE_CLOSED(e, "engine_eval_stages");
    ORN_REQUIRE(n >= 0 && (rows || n == 0), "engine_eval_stages: n=%d frames need a device array of n row indices", n);
    const orn_engine_desc &d = e->d;
    const int nl = d.n_layers;
    const StageGeo g = stage_geometry(&d);
    int top = -1;
    uint32_t ms_mask = 0;
    bool any_stats = false;
    for (int i = 0; i < nl; ++i) {
        const orn_stage_out &s = out[i];
        if (!(s.rgb8 || s.img || s.stats || s.msssim)) continue;       // (a target table alone asks for nothing)
        ORN_REQUIRE(!(s.stats || s.msssim) || s.targets, "engine_eval_stages: stage %d: stats and msssim need targets", i);
        if (s.msssim) {
            ORN_REQUIRE((g.H[i] < g.W[i] ? g.H[i] : g.W[i]) > 160, "engine_eval_stages: stage %d: msssim: image side must exceed 160 (got %dx%d)", i,
                        g.H[i], g.W[i]);
            ms_mask |= 1u << i;
        }
        any_stats = any_stats || s.stats;
        top = i;
    }
    ORN_REQUIRE(top >= 0, "engine_eval_stages: no stage wanted (every member of every out[i] is null)");
    if (!d.multi_res)
        for (int i = 0; i + 1 < nl; ++i)
            if (out[i].rgb8 || out[i].img || out[i].stats || out[i].msssim) {
                orn_set_error("engine_eval_stages: stage %d is below the last, and the engine was created with multi_res = 0 (no side heads; its first two "
                              "blocks may be fused)", i);
                return ORN_E_STATE;
            }
    if (n == 0) return 0;
    int chunk = 0;
    StagesWs L = {};
    if (ms_mask) {
        ORN_REQUIRE(ws && (uintptr_t)ws % 16 == 0, "engine_eval_stages: msssim needs a 16-byte aligned workspace");
        chunk = n < 65535 / 3 ? n : 65535 / 3;
        while (chunk > 0 && stages_ws_layout(&d, ms_mask, chunk, &L) > ws_bytes) --chunk;
        if (chunk < 1) { orn_set_error("engine_eval_stages: workspace %zu < %zu", ws_bytes, stages_ws_layout(&d, ms_mask, 1, nullptr)); return ORN_E_WS; }
    }
    assert(!e->side_busy);          // orn_engine_train_steps joins its side branch before it returns
    hipStream_t st = (hipStream_t)stream;
    float *wsf = (float *)ws;
    // the ticket starts at zero; every output launch of every stage leaves it there for the next one on this stream
    if (any_stats) ORN_HIP(hipMemsetAsync(e->dec_ws + 2 * ORN_DECODE_MAX_BLOCKS, 0, 64 * 4, st));
    for (int32_t k = 0; k < n; ++k) {
        ORN_TRY(forward(e, embeds, rows + k, false, st, top, k == 0 ? 0 : MERGE_NONE, false));
        for (int i = 0; i <= top; ++i) {
            const orn_stage_out &s = out[i];
            if (!(s.rgb8 || s.img || s.stats || s.msssim)) continue;
            const size_t HW = (size_t)g.H[i] * g.W[i];
            float *planes = s.img ? s.img + (size_t)k * HW * 3 : (s.msssim ? wsf + L.slot[i] + (size_t)(k % chunk) * HW * 3 : nullptr);
            const OrnDecodeOut o = {s.targets, rows + k, s.rgb8 ? s.rgb8 + (size_t)k * HW * 3 : nullptr, planes,
                                    s.stats ? s.stats + (size_t)k * 4 : nullptr, e->dec_ws};
            if (i + 1 == nl) {               // the last stage: the output stage of orn_engine_decode_frames
                if (e->ff < nl)
                    ORN_TRY(e->ops->decode_out(e->L[i].zb, e->params + d.head_w, e->params + d.head_b, e->Cn_last, HW, d.sigmoid, o, st, d.act));
                else
                    ORN_TRY(orn_launch_decode_out_f32(e->img, HW, o, st));
            } else if (i >= e->ff) {         // a 16-bit block's side stage: head + output stage in one kernel
                ORN_TRY(e->ops->stage_out(e->L[i].zb, e->params + d.side_head_w[i], e->params + d.side_head_b[i], g.C[i], HW, d.sigmoid, o, st, d.act));
            } else {                         // an fp32 block's side stage: the training forward's head, then the planar output stage
                ORN_TRY(orn_launch_side_head_fwd_f32(e->L[i].a, e->params + d.side_head_w[i], e->params + d.side_head_b[i], g.C[i], HW, d.sigmoid,
                                                     e->stage[i].img, st, nullptr));
                ORN_TRY(orn_launch_decode_out_f32(e->stage[i].img, HW, o, st));
            }
        }
        if (ms_mask && ((k + 1) % chunk == 0 || k + 1 == n)) {
            const int32_t k0 = k / chunk * chunk;
            for (int i = 0; i <= top; ++i) {
                const orn_stage_out &s = out[i];
                if (!s.msssim) continue;
                const size_t HW = (size_t)g.H[i] * g.W[i];
                ORN_TRY(orn_launch_msssim_frames(s.img ? s.img + (size_t)k0 * HW * 3 : wsf + L.slot[i], s.targets, rows + k0, k + 1 - k0, 3, g.H[i],
                                                 g.W[i], s.msssim + k0, wsf + L.ms, st));
            }
        }
    }
    return 0;
}
