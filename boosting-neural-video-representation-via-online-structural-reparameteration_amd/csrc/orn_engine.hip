// The engine's description and memory (orn_engine.h): the descriptor check, the stage geometry, the workspace carve, creation and
// destruction, and every setter.  The forward is orn_engine_forward.hip, the step orn_engine_step.hip.
#include "orn_engine.h"
#include <new>
#include <cstdlib>

// the five events of the pipelined step (struct orn_engine, `side`)
static hipEvent_t orn_engine::*const SIDE_EVENTS[] = {&orn_engine::ev_fork, &orn_engine::ev_adam, &orn_engine::ev_wgrad, &orn_engine::ev_join,
                                                      &orn_engine::ev_below};

// Split-K slabs of the LAST block's weight gradient on an engine that can run the pipelined step: fewer, longer work-groups (one
// per CU, or little more) leave room on every CU for the launches that run beside it.  Measured on the 720p step (tools/probes, round 4):
// 40 / 32 / 24 slabs = 1.050 / 1.015..1.024 / 1.019..1.023 ms per pipelined step in the final form of the branch (32 and 24
// are equal within the noise of a box, 24 moves less data).  The serial forms of the step use the same count, so that all forms of
// the step give bit-identical results.  (The block below the last keeps the default rule: 32 / 40 / 16 slabs for it were measured, none faster.)
static constexpr int ORN_LAST_SMAX = 24;

void drop_graphs(orn_engine *e)
{
    if (e->graph_exec) { (void)hipGraphExecDestroy(e->graph_exec); e->graph_exec = nullptr; }
    if (e->graph) { (void)hipGraphDestroy(e->graph); e->graph = nullptr; }
    if (e->graph_exec_u) { (void)hipGraphExecDestroy(e->graph_exec_u); e->graph_exec_u = nullptr; }
    if (e->graph_u) { (void)hipGraphDestroy(e->graph_u); e->graph_u = nullptr; }
}

extern "C" size_t orn_conv3x3_ps_silu_bwd_ws_bytes(int B, int C, int O, int H, int W);
extern "C" size_t orn_erb_merge_bwd_ws_bytes(int C, int O);
extern "C" size_t orn_head_bwd_ws_bytes(int B, int C, int H, int W);
extern "C" size_t orn_loss_ws_bytes_for(int loss_type, int B, int Ch, int H, int W);

StageGeo stage_geometry(const orn_engine_desc *d)
{
    StageGeo g = {};
    int H = d->fc_h, W = d->fc_w;
    for (int i = 0; i < d->n_layers && d->layer[i].s >= 1; ++i) {
        const orn_layer_desc &l = d->layer[i];
        H *= l.s; W *= l.s;
        g.C[i] = (int)(l.O / ((long long)l.s * l.s)); g.H[i] = H; g.W[i] = W;
    }
    return g;
}

int check_desc(const orn_engine_desc *d)
{
    ORN_REQUIRE(d, "engine: null desc");
    ORN_REQUIRE(d->n_layers >= 1 && d->n_layers <= ORN_MAX_LAYERS, "engine: n_layers=%d out of range", d->n_layers);
    ORN_REQUIRE(d->precision >= 0 && d->precision <= 2, "engine: precision %d not built", d->precision);
    ORN_REQUIRE(orn_act_known(d->act), "engine: act = %d is not ORN_ACT_SWISH (0) or ORN_ACT_GELU (1)", d->act);
    ORN_REQUIRE(d->branch_kind == 0 || ((d->branch_kind == ORN_BRANCH_ACB || d->branch_kind == ORN_BRANCH_REPVGG || d->branch_kind == ORN_BRANCH_ECB) && !d->erb),
                "engine: branch_kind %d (with erb = %d) is not 0 or ORN_BRANCH_ACB / _REPVGG / _ECB with erb = 0", d->branch_kind, d->erb);
    ORN_REQUIRE(d->embed_len > 0 && d->stem_dim > 0 && d->fc_h > 0 && d->fc_w > 0 && d->fc_dim > 0, "engine: bad stem geometry");
    const StageGeo g = stage_geometry(d);
    int C = d->fc_dim, H = d->fc_h, W = d->fc_w;
    for (int i = 0; i < d->n_layers; ++i) {
        const orn_layer_desc &l = d->layer[i];
        ORN_REQUIRE(l.C == C && l.H == H && l.W == W,
                    "engine: layer %d geometry (C=%d,H=%d,W=%d) does not chain (expected %d,%d,%d)", i, l.C, l.H, l.W, C, H, W);
        ORN_REQUIRE(l.s >= 1 && l.O > 0 && l.O % (l.s * l.s) == 0, "engine: layer %d: O=%d not divisible by s^2", i, l.O);
        ORN_REQUIRE(l.w3x3 >= 0 && l.b3x3 >= 0, "engine: layer %d: missing 3x3 weight/bias", i);
        if (d->erb)
            ORN_REQUIRE(l.w3x1 >= 0 && l.b3x1 >= 0 && l.w1x3 >= 0 && l.b1x3 >= 0 && l.w1 >= 0 && l.w2 >= 0 && l.w3 >= 0,
                        "engine: layer %d: missing ERB branch tensors", i);
        const orn_branch_desc &x = d->branch[i];
        if (d->branch_kind == ORN_BRANCH_ACB)
            ORN_REQUIRE(l.w3x1 >= 0 && l.b3x1 >= 0 && l.w1x3 >= 0 && l.b1x3 >= 0, "engine: layer %d: missing ACB branch tensors", i);
        if (d->branch_kind == ORN_BRANCH_REPVGG)
            ORN_REQUIRE(x.w1x1 >= 0 && x.b1x1 >= 0, "engine: layer %d: missing RepVGG branch tensors", i);
        if (d->branch_kind == ORN_BRANCH_ECB) {
            ORN_REQUIRE(l.w1 >= 0 && l.w2 >= 0, "engine: layer %d: missing ECB branch tensors (w1 = wA, w2 = wB)", i);
            for (int t = 0; t < 3; ++t)
                ORN_REQUIRE(x.sb[t].k0 >= 0 && x.sb[t].b0 >= 0 && x.sb[t].scale >= 0 && x.sb[t].bias >= 0 && x.sb[t].mask >= 0,
                            "engine: layer %d: missing ECB branch tensors (1x1 -> mask branch %d)", i, t);
        }
        C = g.C[i]; H = g.H[i]; W = g.W[i];
    }
    ORN_REQUIRE(d->n_params > 0 && d->n_params % 4 == 0, "engine: n_params must be a positive multiple of 4");
    const OrnLossSpec *sp = orn_loss_spec_of(d->loss_type);
    ORN_REQUIRE(sp, "engine: bad loss_type %d", d->loss_type);
    if (sp->kind == ORN_LOSS_KIND_MSSSIM)       // pytorch_msssim's own limit (H, W: the decoder's output by now)
        ORN_REQUIRE((H < W ? H : W) > 160, "engine: the MS-SSIM losses need an output side above 160 (got %dx%d)", H, W);
    ORN_REQUIRE(d->multi_res == 0 || d->multi_res == 1, "engine: multi_res = %d is not 0 or 1", d->multi_res);
    if (d->multi_res) {
        // a head and a loss of this type on every stage: the loss must take every stage's size, as the reference's does
        ORN_REQUIRE(fabsf(d->lw) <= 3.0e38f, "engine: lw is not finite");
        for (int i = 0; i + 1 < d->n_layers; ++i) {
            H = g.H[i]; W = g.W[i];
            ORN_REQUIRE(d->side_head_w[i] >= 0 && d->side_head_b[i] >= 0, "engine: stage %d: missing head tensors (side_head_w / side_head_b)", i);
            const int64_t Ci = g.C[i];
            ORN_REQUIRE(d->side_head_w[i] + 3 * Ci <= d->n_params && d->side_head_b[i] + 3 <= d->n_params,
                        "engine: stage %d: head tensors lie outside the arena of %lld floats", i, (long long)d->n_params);
            ORN_REQUIRE(Ci <= 512, "engine: stage %d: a side head takes at most 512 channels (got %lld)", i, (long long)Ci);
            if (sp->kind == ORN_LOSS_KIND_SSIM)
                ORN_REQUIRE(H > 10 && W > 10, "engine: stage %d (%dx%d): the SSIM losses need an 11x11 window to fit (H, W > 10)", i, H, W);
            if (sp->kind == ORN_LOSS_KIND_MSSSIM)
                ORN_REQUIRE((H < W ? H : W) > 160, "engine: stage %d (%dx%d): the MS-SSIM losses need a side above 160", i, H, W);
        }
    }
    return 0;
}

static bool layer_is_fast(const orn_layer_desc &l)
{
    // O % 96: whole 32-channel MFMA blocks forward (a last N tile of 96 is ragged) and whole 96-channel K chunks in the dgrad
    return l.C == ORN_FAST_C && l.O % 96 == 0 && l.O % (l.s * l.s) == 0;
}

// First layer from which every layer (and the head) can run on the bf16 MFMA path.
static int first_fast_layer(const orn_engine_desc *d)
{
    if (d->precision == 0) return d->n_layers;
    const orn_layer_desc &last = d->layer[d->n_layers - 1];
    const int cn = last.O / (last.s * last.s);
    if (!(cn == 32 || cn == 64 || cn == 96 || cn == 128)) return d->n_layers;
    int ff = d->n_layers;
    while (ff > 0 && layer_is_fast(d->layer[ff - 1])) --ff;
    // one narrower layer below them may join, zero-padded to 96 input channels (its fp32 NCHW input is converted
    // anyway): 3.7x the FLOPs of C=26 on a 16x faster pipe, and none of the fp32 path's small launches
    if (ff > 0 && ff < d->n_layers) {
        const orn_layer_desc &l = d->layer[ff - 1];
        if (l.C < ORN_FAST_C && l.O % 96 == 0 && l.O % (l.s * l.s) == 0) --ff;
    }
    return ff;
}

// Computes the workspace layout (in floats); if e != null also fills its pointers.
static size_t layout(const orn_engine_desc *d, orn_engine *e)
{
    size_t off = 0;
    const int ff = first_fast_layer(d);
    const StageGeo g = stage_geometry(d);
    float *dxn = nullptr;
    float *base = e ? e->ws : nullptr;
    auto take = [&](size_t floats) { float *p = base ? base + off : nullptr; off += al(floats); return p; };
    const int Nout = d->fc_h * d->fc_w * d->fc_dim;
    float *pre1 = take(d->stem_dim), *h1 = take(d->stem_dim), *pre2 = take(Nout), *h2 = take(Nout), *dh2 = take(Nout);
    size_t scratch = orn_stem_bwd_ws_floats(1, d->stem_dim, Nout);
    LayerBuf L[ORN_MAX_LAYERS] = {};
    for (int i = 0; i < d->n_layers; ++i) {
        const orn_layer_desc &l = d->layer[i];
        const size_t wsz = (size_t)l.O * l.C * 9;
        if (d->erb) {
            L[i].T = take(wsz); L[i].wf = take(wsz); L[i].bf = take(l.O);
            L[i].w2t = (2 * l.C * 9 * 4 * 4 <= 64 * 1024) ? take((size_t)9 * l.O * 2 * l.C) : nullptr;
            L[i].dT = take(wsz); L[i].dw1p = take((size_t)9 * 2 * l.C * l.C);
            if (d->precision != 0) {
                L[i].mh16 = take((orn_merge_h16_layer_halfs(l.C, l.O) + 1) / 2);
                L[i].dw2t = take((size_t)9 * l.O * 2 * l.C);
            }
        }
        if (d->branch_kind) {
            L[i].wf = take(wsz); L[i].bf = take(l.O);
            L[i].dwap = take(orn_branch_merge_bwd_ws_floats(d->branch_kind, l.C, l.O));
        }
        const size_t asz = (size_t)g.C[i] * g.H[i] * g.W[i];
        size_t s1;
        if (i < ff) {
            L[i].z = take(asz); L[i].a = take(asz); L[i].da = take(asz);
            L[i].wd32 = take(wsz);
            s1 = orn_conv3x3_ps_silu_bwd_ws_bytes(1, l.C, l.O, l.H, l.W) / 4;
            const size_t s0 = al(orn_stem_bwd_ws_floats(1, d->stem_dim, Nout)) + (size_t)orn_stage0_slabs(l.O, l.s) * l.C * l.H * l.W;   // fused first block
            if (s0 > s1) s1 = s0;
        } else {
            // halfs are carved as floats (2 per float)
            const size_t wpz = (size_t)l.O * ORN_FAST_C * 9 + 96 * ORN_FAST_C;      // + the rows a ragged last N tile reads past the end
            L[i].xpad = (uint16_t *)take(((size_t)(l.H + 2) * (l.W + 2) * ORN_FAST_C + 1) / 2);
            L[i].zb = (uint16_t *)take((asz + 1) / 2);
            L[i].dypad = (uint16_t *)take(((size_t)(l.H + 2) * (l.W + 2) * l.O + 128 + 1) / 2);   // + a ragged wgrad tile's over-read
            L[i].wb = (uint16_t *)take((wpz + 1) / 2);
            L[i].wd = (uint16_t *)take((wpz + 1) / 2);
            L[i].biasp = take(l.O);
            L[i].wslab = take(orn_half_ops_bf16()->wgrad_ws_floats(l.H, l.W, l.O));
            const OrnHalfOps *ops = orn_half_ops_bf16();     // sizes do not depend on the element type
            if (i == ff) dxn = take((size_t)l.H * l.W * ORN_FAST_C * ops->dgrad_f32_slabs(l.H, l.W, l.O));
            s1 = al(ops->wgrad_ws_floats(l.H, l.W, l.O));
            const size_t sd = (size_t)l.H * l.W * ORN_FAST_C * ops->dgrad_f32_slabs(l.H, l.W, l.O);
            if (ops->dgrad_f32_slabs(l.H, l.W, l.O) > 1 && sd > s1) s1 = sd;
        }
        if (d->erb) { const size_t s2 = orn_erb_merge_bwd_ws_bytes(l.C, l.O) / 4; if (s2 > s1) s1 = s2; }
        if (s1 > scratch) scratch = s1;
    }
    const int Cn = g.C[d->n_layers - 1], H = g.H[d->n_layers - 1], W = g.W[d->n_layers - 1];      // the decoder's output
    const size_t isz = (size_t)3 * H * W;
    float *img = take(isz), *dimg = take(isz), *stats = take(8);
    float *loss_ws = take(orn_loss_ws_bytes_for(d->loss_type, 1, 3, H, W) / 4);    // ids 0..2: orn_loss_ws_bytes, to the byte
    const size_t s3 = (ff < d->n_layers) ? orn_half_ops_bf16()->head_bwd_ws_floats(Cn) : orn_head_bwd_ws_bytes(1, Cn, H, W) / 4;
    if (s3 > scratch) scratch = s3;
    float *scr = take(scratch);
    // (fp32 engine: partials of the fused head backward of the last block, stride 2 only)
    const orn_layer_desc &ll = d->layer[d->n_layers - 1];
    float *head_ws = (ff < d->n_layers) ? take(orn_half_ops_bf16()->head_bwd_ws_floats(Cn))
                   : (ll.s == 2 ? take((size_t)(orn_head_bwd_fused_f32_blocks(ll.H, ll.W) + 1) * (3 * Cn + 3)) : nullptr);
    float *cur = take((sizeof(OrnStepCur) * ORN_GRAPH_UNROLL + 3) / 4 + 16);    // one cursor state per step of the unrolled graph
    float *scs = take(sizeof(OrnScaleState) * ORN_SCALE_SLOTS / 4);     // one entry per step of the unrolled graph (entry 0 = master)
    float *mtab[3], *mhtab[3];
    for (int k = 0; k < 3; ++k) {
        mtab[k] = d->erb ? take(orn_merge_group_bytes() / 4) : nullptr;
        mhtab[k] = (d->erb && d->precision != 0) ? take(orn_merge_h16_table_bytes() / 4) : nullptr;
    }
    float *cur_side = take((sizeof(OrnStepCur) + 3) / 4 + 16);
    float *sc_side = take(sizeof(OrnScaleState) / 4 + 16);
    float *dec_ws = take(ORN_DECODE_WS_FLOATS);
    // multi-resolution heads: behind everything else, so that a single-resolution engine's carve is the one it has always had
    orn_engine::SideStage stg[ORN_MAX_LAYERS] = {};
    for (int i = 0; d->multi_res && i + 1 < d->n_layers; ++i) {
        orn_engine::SideStage &s = stg[i];
        s.C = g.C[i]; s.H = g.H[i]; s.W = g.W[i];
        const size_t isz_i = (size_t)3 * s.H * s.W;
        s.img = take(isz_i); s.dimg = take(isz_i); s.stats = take(8);
        s.loss_ws = take(orn_loss_ws_bytes_for(d->loss_type, 1, 3, s.H, s.W) / 4);
        s.head_ws = take(orn_side_head_bwd_ws_floats(s.C, s.H, s.W));
    }
    if (e) {
        for (int i = 0; i < ORN_MAX_LAYERS; ++i) {       // (the target tables are the caller's: kept)
            stg[i].targets = e->stage[i].targets; stg[i].tstats = e->stage[i].tstats;
            e->stage[i] = stg[i];
        }
        e->pre1 = pre1; e->h1 = h1; e->pre2 = pre2; e->h2 = h2; e->dh2 = dh2;
        e->img = img; e->dimg = dimg; e->stats = stats; e->loss_ws = loss_ws; e->scratch = scr; e->head_ws = head_ws;
        e->cur = (OrnStepCur *)cur;
        e->sc = (OrnScaleState *)scs;
        for (int i = 0; i < d->n_layers; ++i) e->L[i] = L[i];
        e->Hout = H; e->Wout = W; e->Cn_last = Cn;
        e->ff = ff; e->dxn = dxn;
        e->stem_ws = al(orn_stem_bwd_ws_floats(1, d->stem_dim, Nout));
        const orn_layer_desc &l0 = d->layer[0];
        // (multi-resolution heads: stage 0's head reads the block's fp32 activation and adds to its fp32 gradient, which the fused
        // pair never materialises -- the two blocks stay apart there)
        e->stage0 = d->precision != 0 && ff == 1 && d->n_layers > 1 && orn_stage0_supported(l0.C, l0.O, l0.H, l0.W, l0.s) && !d->multi_res;
        for (int k = 0; k < 3; ++k) { e->mset[k].tables = mtab[k]; e->mset[k].mh_tables = mhtab[k]; }
        e->cur_side = (OrnStepCur *)cur_side;
        e->sc_side = (OrnScaleState *)sc_side;
        e->dec_ws = dec_ws;
    }
    return off * 4;
}

extern "C" size_t orn_engine_ws_bytes(const orn_engine_desc *d)
{
    if (check_desc(d) != 0) return 0;
    return layout(d, nullptr);
}

// ---- orn_engine_create, step by step (each may fail: the caller then destroys the partly built engine) ----
static void accum_add(OrnAccumTable &t, int64_t off, int64_t len)      // appends the range [off, off + len) of the arena
{
    const int blocks = (t.n ? t.blk_end[t.n - 1] : 0) + orn_cdiv((long)len, ORN_ACCUM_CHUNK);
    t.off[t.n] = off; t.len[t.n] = len;
    t.blk_end[t.n++] = blocks;
}

// 1. batched step: the gradient slots the backward writes directly (ERB: dWf / dbf in the 3x3 branch's slots; the other
// branches' gradients come from the merge backward, which runs once per optimiser step on the summed dWf)
static void fill_accum_tables(orn_engine *e)
{
    const orn_engine_desc *d = &e->d;
    for (int i = 0; i < d->n_layers; ++i) {
        accum_add(e->acc_tab, d->layer[i].w3x3, (int64_t)d->layer[i].O * d->layer[i].C * 9);
        accum_add(e->acc_tab, d->layer[i].b3x3, d->layer[i].O);
    }
    const int64_t Nout = (int64_t)d->fc_h * d->fc_w * d->fc_dim;
    accum_add(e->acc_tab, d->head_w, (int64_t)3 * e->Cn_last); accum_add(e->acc_tab, d->head_b, 3);
    accum_add(e->acc_tab, d->stem_w0, (int64_t)d->stem_dim * d->embed_len); accum_add(e->acc_tab, d->stem_b0, d->stem_dim);
    accum_add(e->acc_tab, d->stem_w1, Nout * d->stem_dim); accum_add(e->acc_tab, d->stem_b1, Nout);
    // (multi-resolution heads) the side heads' slots: a table of their own, so that the first keeps the launch it has always had
    for (int i = 0; d->multi_res && i + 1 < d->n_layers; ++i) {
        accum_add(e->side_tab, d->side_head_w[i], (int64_t)3 * e->stage[i].C);
        accum_add(e->side_tab, d->side_head_b[i], 3);
    }
}

// 2. the one-pixel borders of the channels-last buffers must be (and stay) zero; the scale state starts at the initial scale
static int init_workspace(orn_engine *e, size_t bytes)
{
    hipError_t rc = hipMemset(e->ws, 0, bytes);
    if (rc == hipSuccess) rc = hipDeviceSynchronize();
    if (rc != hipSuccess) { orn_set_error("engine_create: hipMemset failed: %s", hipGetErrorString(rc)); return (int)rc; }
    OrnScaleState s0[ORN_SCALE_SLOTS] = {};
    for (int r = 0; r < ORN_SCALE_SLOTS; ++r) { s0[r].gs = e->gs; s0[r].inv_gs = 1.0f / e->gs; s0[r].gs_max = e->gs; }
    rc = hipMemcpy(e->sc, s0, sizeof(s0), hipMemcpyHostToDevice);
    if (rc == hipSuccess) rc = hipMemcpy(e->sc_side, s0, sizeof(OrnScaleState), hipMemcpyHostToDevice);
    if (rc != hipSuccess) { orn_set_error("engine_create: scale state upload failed: %s", hipGetErrorString(rc)); return (int)rc; }
    return 0;
}

// 3. Can this engine run the pipelined step?  16-bit mode with the last block AND the block below it on the fast path (the
// hand-off points are their buffers), gradients present, and an arena in which the last block's tensors and the head's lie
// behind everything else (one Adam launch per stream).
static int setup_pipeline(orn_engine *e)
{
    const orn_engine_desc *d = &e->d;
    const int nl = d->n_layers;
    const orn_layer_desc &ll = d->layer[nl - 1];
    bool ok = d->precision != 0 && e->ff < nl - 1 && e->grads && e->m && e->v && !d->branch_kind     // (no pipelined form of the ACB / RepVGG / ECB merge,
              && !d->multi_res;                                                                      //  nor of the multi-resolution heads)
    if (ok) {
        const int64_t lo_all[9] = {ll.w3x3, ll.b3x3, ll.w3x1, ll.b3x1, ll.w1x3, ll.b1x3, ll.w1, ll.w2, ll.w3};
        int64_t lo = d->n_params;
        for (int k = 0; k < (d->erb ? 9 : 2); ++k) if (lo_all[k] >= 0 && lo_all[k] < lo) lo = lo_all[k];
        ok = d->head_w >= lo && d->head_b >= lo && d->stem_w0 < lo && d->stem_b0 < lo && d->stem_w1 < lo && d->stem_b1 < lo && lo % 64 == 0;
        for (int i = 0; i < nl - 1 && ok; ++i) {
            const orn_layer_desc &l = d->layer[i];
            const int64_t o[9] = {l.w3x3, l.b3x3, l.w3x1, l.b3x1, l.w1x3, l.b1x3, l.w1, l.w2, l.w3};
            for (int k = 0; k < (d->erb ? 9 : 2); ++k) ok = ok && o[k] < lo;
        }
        e->side_lo = (size_t)lo;
    }
    if (ok) {
        // (A high-priority side stream returns ~2 us per step -- the branch's small launches queue less behind the 8-wave forward
        // launches of the middle blocks -- but while such a queue exists, even idle, every OTHER stream of the process loses: the
        // fp32 engine's step, run next to an idle fp16 engine, went 6.66 -> 8.25 ms.  Default priority.)
        hipError_t rc = hipStreamCreateWithFlags(&e->side, hipStreamNonBlocking);
        // hipEventDisableSystemFence: these events order streams of ONE device; what the flag gives up is visibility to the host and
        // to other devices at the record (hip_runtime_api.h), which the caller's own synchronisation of its stream provides.  The
        // record is then a lighter packet: ~4 us per step (3 records / waits on the caller's stream) against the default events.
        for (auto ev : SIDE_EVENTS)
            if (rc == hipSuccess) rc = hipEventCreateWithFlags(&(e->*ev), hipEventDisableTiming | hipEventDisableSystemFence);
        if (rc != hipSuccess) { orn_set_error("engine_create: side stream: %s", hipGetErrorString(rc)); return (int)rc; }
    }
    e->pipe_ok = ok;
    e->last_smax = ok ? ORN_LAST_SMAX : 0;
    // Where the side branch forks off the backward.  Measured on the 720p step with the last block alone on the branch, one box
    // (tools/probes/mode_ab.sh; serial 1.079 ms): fork behind the head's backward 1.038, behind the dgrad of layer 4 (the last block)
    // 1.058, 3 1.024, 2 1.032, 1 1.035, 0 1.067, behind the lower blocks' weight gradients and their reduction 1.050 ms -- the last
    // block's own dgrad and the launch behind it are full-chip MFMA launches that the side branch's weight gradient only thrashes;
    // behind them the caller's stream runs under-filled launches, and the earlier the branch starts the earlier it is back for the
    // next forward.
    // With a fast block between the last one and the first fast layer, the side stream also takes the weight gradient of the block
    // below the last one (ahead of the last block's), and then forks one launch earlier, behind the last block's dgrad (whose output is
    // that wgrad's dy): that wgrad (216 work-groups at 720p) runs beside the block's own dgrad launch (230 work-groups on 512 slots), and
    // the lower blocks' batched wgrad on the caller's stream shrinks to a third (95 -> 40 us at 720p).  Same box: 1.037 -> 1.021 ms per
    // step.  With exactly two blocks on the fast path the branch keeps the last block alone and forks behind the slab reduction.
    e->side_below = ok && nl - 2 > e->ff;
    e->fork_behind_dgrad = e->side_below;
    return 0;
}

// the arena offsets of a block as pointers into `base`: the parameters, or (grads) where their gradients go
static orn_branch_ptrs branch_ptrs(const orn_engine_desc *d, int i, float *base)
{
    const orn_layer_desc &l = d->layer[i];
    const orn_branch_desc &x = d->branch[i];
    orn_branch_ptrs p = {};
    p.w3x3 = base + l.w3x3; p.b3x3 = base + l.b3x3;
    if (d->branch_kind == ORN_BRANCH_ACB) { p.w3x1 = base + l.w3x1; p.b3x1 = base + l.b3x1; p.w1x3 = base + l.w1x3; p.b1x3 = base + l.b1x3; }
    if (d->branch_kind == ORN_BRANCH_REPVGG) { p.w1x1 = base + x.w1x1; p.b1x1 = base + x.b1x1; }
    if (d->branch_kind == ORN_BRANCH_ECB) {
        p.wA = base + l.w1; p.wB = base + l.w2;
        for (int t = 0; t < 3; ++t) {
            p.sb[t].k0 = base + x.sb[t].k0; p.sb[t].b0 = base + x.sb[t].b0; p.sb[t].scale = base + x.sb[t].scale;
            p.sb[t].bias = base + x.sb[t].bias; p.sb[t].mask = base + x.sb[t].mask;
        }
    }
    return p;
}

// layer i of an ERB engine as the merge launchers see it
static void fill_merge_layer(const orn_engine *e, int i, OrnMergeLayer &m, bool half_in_S)
{
    const orn_engine_desc *d = &e->d;
    float *params = e->params, *grads = e->grads;
    const orn_layer_desc &l = d->layer[i];
    m.C = l.C; m.O = l.O;
    m.w3x3 = params + l.w3x3; m.w3x1 = params + l.w3x1; m.w1x3 = params + l.w1x3;
    m.w1 = params + l.w1; m.w2 = params + l.w2; m.w3 = params + l.w3;
    m.T = e->L[i].T; m.wf = e->L[i].wf; m.w2t = e->L[i].w2t;
    m.b3x3 = params + l.b3x3; m.b1x3 = params + l.b1x3; m.b3x1 = params + l.b3x1; m.bf = e->L[i].bf;
    m.g = grads ? grads + l.w3x3 : nullptr;
    m.dT = e->L[i].dT; m.dw1p = e->L[i].dw1p;
    m.dw2 = grads ? grads + l.w2 : nullptr; m.dw3 = grads ? grads + l.w3 : nullptr;
    m.dw2t = e->L[i].dw2t;
    m.half_kind = 0; m.s2 = l.s * l.s; m.Cp = ORN_FAST_C; m.wb = m.wd = nullptr; m.biasp = nullptr;
    // the merged kernel's 16-bit operand copies: rider work-groups of the first block's launch (forward()) when that
    // launch exists, else (and always on the side stream) the epilogue of the merge's S product
    if (i >= e->ff && half_in_S) {
        m.half_kind = d->precision; m.wb = e->L[i].wb; m.wd = e->L[i].wd; m.biasp = e->L[i].biasp;
    }
}

// 4. the blocks as their merge sees them: the branch layers (ACB / RepVGG / ECB), the parameters as (wf, bf) (vanilla / deploy), or
// the merge sets (ERB)
static int build_blocks(orn_engine *e)
{
    const orn_engine_desc *d = &e->d;
    if (d->branch_kind) {
        for (int i = 0; i < d->n_layers; ++i) {
            OrnBranchLayer &b = e->bl[i];
            b = OrnBranchLayer{};
            b.kind = d->branch_kind; b.C = d->layer[i].C; b.O = d->layer[i].O;
            b.p = branch_ptrs(d, i, e->params);
            b.wf = e->L[i].wf; b.bf = e->L[i].bf;
            if (e->grads) {        // dWf / dbf land in the 3x3 branch's gradient slots: d3x3 = g, db3x3 = dbf without a copy
                b.d = branch_ptrs(d, i, e->grads);
                b.g = b.d.w3x3; b.dbf = b.d.b3x3;
            }
            b.dwAp = e->L[i].dwap;
            e->L[i].T = nullptr;
        }
        e->nbr = d->n_layers;
        return 0;
    }
    if (!d->erb) {
        for (int i = 0; i < d->n_layers; ++i) {
            e->L[i].T = nullptr;
            e->L[i].wf = e->params + d->layer[i].w3x3;
            e->L[i].bf = e->params + d->layer[i].b3x3;
        }
        return 0;
    }
    // set 0: every layer; set 1: all but the last block (caller's stream of the pipelined step); set 2: the last block (side stream)
    const int nl = d->n_layers;
    for (int k = 0; k < (e->pipe_ok ? 3 : 1); ++k) {
        orn_engine::MergeSet &ms = e->mset[k];
        const int i0 = k == 2 ? nl - 1 : 0, i1 = k == 1 ? nl - 1 : nl;
        ms.n = 0;
        void *bufs[ORN_MAX_LAYERS];
        for (int i = i0; i < i1; ++i) {
            fill_merge_layer(e, i, ms.ml[ms.n], k == 2 || !e->stage0);
            bufs[ms.n] = e->L[i].mh16;
            ms.layer[ms.n++] = i;
        }
        ORN_TRY(orn_merge_groups_build(ms.tables, ms.n, ms.ml, d->precision == 0, ms.tiles));
        if (d->precision != 0) {
            ms.mh_host = malloc(orn_merge_h16_host_bytes());
            ORN_TRY(ms.mh_host ? orn_merge_h16_build(ms.mh_tables, ms.mh_host, ms.n, ms.ml, bufs, k == 2 ? e->sc_side : e->sc) : ORN_E_ARG);
        }
    }
    return 0;
}

extern "C" int orn_engine_create(const orn_engine_desc *d, float *params, float *grads, float *adam_m, float *adam_v,
                                 void *ws, size_t ws_bytes, orn_engine **out)
{
    ORN_TRY(check_desc(d));
    ORN_REQUIRE(params && out && ws, "engine_create: null pointer");
    ORN_REQUIRE(((uintptr_t)params | (uintptr_t)grads | (uintptr_t)adam_m | (uintptr_t)adam_v | (uintptr_t)ws) % 256 == 0,
                "engine_create: arenas and workspace must be 256-byte aligned");
    const size_t need = layout(d, nullptr);
    if (ws_bytes < need) {
        orn_set_error("engine_create: workspace %zu < %zu", ws_bytes, need);
        return ORN_E_WS;
    }
    ORN_TRY(orn_loss_init());
    orn_engine *e = new (std::nothrow) orn_engine();      // value-initialised: what is not set below is zero / null / false
    ORN_REQUIRE(e, "engine_create: out of host memory");
    e->d = *d;
    e->params = params; e->grads = grads; e->m = adam_m; e->v = adam_v;
    e->ws = (float *)ws;
    e->ops = (d->precision == 2) ? orn_half_ops_f16() : orn_half_ops_bf16();
    e->gs = (d->precision == 2) ? 1048576.0f : 1.0f;
    layout(d, e);
    fill_accum_tables(e);
    int rc = init_workspace(e, need);
    if (rc == 0) rc = setup_pipeline(e);
    if (rc == 0) rc = build_blocks(e);
    if (rc != 0) { orn_engine_destroy(e); return rc; }      // (destroy takes a partly built engine)
    *out = e;
    return 0;
}

extern "C" void orn_engine_destroy(orn_engine *e)
{
    if (!e) return;
    drop_graphs(e);
    for (int i = 0; i < 4 * ORN_MAX_LAYERS + 4; ++i)
        if (e->prof_ev[i]) (void)hipEventDestroy(e->prof_ev[i]);
    if (e->side) { (void)hipStreamSynchronize(e->side); (void)hipStreamDestroy(e->side); }
    for (auto ev : SIDE_EVENTS) if (e->*ev) (void)hipEventDestroy(e->*ev);
    for (int k = 0; k < 3; ++k) free(e->mset[k].mh_host);
    delete e;
}

// Optional 0/1 mask multiplied into the gradients before Adam (null: none).  Changes what a captured step does, so
// the graph cache is dropped.  main_eval.py:213-531 (prune fine-tune): pruned weights keep a zero gradient.
extern "C" int orn_engine_set_grad_mask(orn_engine *e, const float *mask)
{
    ORN_REQUIRE(e, "engine_set_grad_mask: null engine");
    ORN_REQUIRE((uintptr_t)mask % 16 == 0, "engine_set_grad_mask: mask must be 16-byte aligned");
    e->gmask = mask;
    drop_graphs(e);
    return 0;
}

// orn_loss_target_stats of the frame table the next steps will be given (null removes it).  Changes what a captured step
// does, so the graph cache is dropped.
extern "C" int orn_engine_set_target_stats(orn_engine *e, const float *stats)
{
    ORN_REQUIRE(e, "engine_set_target_stats: null engine");
    ORN_REQUIRE((uintptr_t)stats % 16 == 0, "engine_set_target_stats: stats must be 16-byte aligned");
    e->tstats = stats;
    drop_graphs(e);
    return 0;
}

// ---- multi-resolution heads: the side stages' tables and the per-stage ring (include/orn.h, N8).  Each changes what a captured step
// reads or writes, so the graph cache is dropped.
static int side_stage_arg(orn_engine *e, int32_t stage, const void *p, const char *name)
{
    if (!e) { orn_set_error("%s: null engine", name); return ORN_E_ARG; }
    if (!e->d.multi_res) { orn_set_error("%s: the engine was created with multi_res = 0", name); return ORN_E_STATE; }
    ORN_REQUIRE(stage >= 0 && stage + 1 < e->d.n_layers, "%s: stage %d outside [0, %d) (the last stage's table is `frames`)", name, stage, e->d.n_layers - 1);
    ORN_REQUIRE((uintptr_t)p % 16 == 0, "%s: the table must be 16-byte aligned", name);
    return 0;
}

extern "C" int orn_engine_set_stage_targets(orn_engine *e, int32_t stage, const float *frames)
{
    ORN_TRY(side_stage_arg(e, stage, frames, "engine_set_stage_targets"));
    e->stage[stage].targets = frames;
    drop_graphs(e);
    return 0;
}

extern "C" int orn_engine_set_stage_target_stats(orn_engine *e, int32_t stage, const float *stats)
{
    ORN_TRY(side_stage_arg(e, stage, stats, "engine_set_stage_target_stats"));
    e->stage[stage].tstats = stats;
    drop_graphs(e);
    return 0;
}

extern "C" int orn_engine_set_stage_stats(orn_engine *e, float *out, int32_t n_slots)
{
    ORN_REQUIRE(e, "engine_set_stage_stats: null engine");
    if (!e->d.multi_res) { orn_set_error("engine_set_stage_stats: the engine was created with multi_res = 0"); return ORN_E_STATE; }
    ORN_REQUIRE(!out || n_slots >= 1, "engine_set_stage_stats: n_slots = %d", n_slots);
    e->stage_ring = out;
    e->stage_slots = out ? n_slots : 0;
    drop_graphs(e);
    return 0;
}

// ---- batched step (-b B): B frames per optimiser step, gradients summed on the device (include/orn.h, N5) ----
// batch workspace, in floats: the accumulation arena (arena layout, so a range has one offset in both), the frame table, the
// per-frame stats
static size_t batch_ws_layout(const orn_engine_desc *d, int max_batch, size_t *cur_off, size_t *stats_off)
{
    size_t off = al((size_t)d->n_params);
    if (cur_off) *cur_off = off;
    off += al((sizeof(OrnStepCur) * (size_t)max_batch + 3) / 4);
    if (stats_off) *stats_off = off;
    off += al((size_t)8 * max_batch);
    return off * 4;
}

extern "C" size_t orn_engine_batch_ws_bytes(const orn_engine_desc *d, int max_batch)
{
    if (max_batch < 1 || max_batch > ORN_MAX_BATCH || check_desc(d) != 0) return 0;
    return batch_ws_layout(d, max_batch, nullptr, nullptr);
}

extern "C" int orn_engine_set_batch_ws(orn_engine *e, void *ws, size_t bytes, int max_batch)
{
    ORN_REQUIRE(e, "engine_set_batch_ws: null engine");
    if (!ws) { e->b_acc = nullptr; e->b_cur = nullptr; e->b_stats = nullptr; e->b_max = 0; return 0; }
    ORN_REQUIRE(max_batch >= 1 && max_batch <= ORN_MAX_BATCH, "engine_set_batch_ws: max_batch=%d outside [1, %d]", max_batch, ORN_MAX_BATCH);
    ORN_REQUIRE((uintptr_t)ws % 256 == 0, "engine_set_batch_ws: workspace must be 256-byte aligned");
    for (const OrnAccumTable *tp : {&e->acc_tab, &e->side_tab}) {
        const OrnAccumTable &t = *tp;
        for (int r = 0; r < t.n; ++r)       // (the accumulate launches write exactly these ranges of both arenas)
            ORN_REQUIRE(t.off[r] >= 0 && t.len[r] > 0 && t.off[r] + t.len[r] <= e->d.n_params,
                        "engine_set_batch_ws: gradient range %d [%lld, +%lld) lies outside the arena", r, (long long)t.off[r], (long long)t.len[r]);
    }
    size_t cur_off, stats_off;
    const size_t need = batch_ws_layout(&e->d, max_batch, &cur_off, &stats_off);
    if (bytes < need) { orn_set_error("engine_set_batch_ws: workspace %zu < %zu", bytes, need); return ORN_E_WS; }
    e->b_acc = (float *)ws;
    e->b_cur = (OrnStepCur *)((float *)ws + cur_off);
    e->b_stats = (float *)ws + stats_off;
    e->b_max = max_batch;
    return 0;
}

// Loss-scale state: out8 = {gs, 1/gs, gs_max, flag, skipped, good, backoffs, late-only skips} (host floats; synchronises the device).
extern "C" int orn_engine_scale_state(orn_engine *e, float *out8)
{
    ORN_REQUIRE(e && out8, "engine_scale_state: null pointer");
    OrnScaleState sa[ORN_SCALE_SLOTS];
    hipError_t rc = hipDeviceSynchronize();
    if (rc == hipSuccess) rc = hipMemcpy(sa, e->sc, sizeof(sa), hipMemcpyDeviceToHost);
    if (rc != hipSuccess) { orn_set_error("engine_scale_state: %s", hipGetErrorString(rc)); return (int)rc; }
    const OrnScaleState &s = sa[0];
    int any = 0;                                      // flag: a step since the last advance met a non-finite value
    for (int r = 0; r < ORN_SCALE_SLOTS; ++r) any |= sa[r].flag;
    any |= s.late_skipped != s.late_seen ? 1 : 0;    // a late-only skip the next advance has still to fold into the scale
    out8[0] = s.gs; out8[1] = s.inv_gs; out8[2] = s.gs_max; out8[3] = (float)any; out8[4] = (float)s.skipped;
    out8[5] = (float)s.good; out8[6] = (float)s.backoffs; out8[7] = (float)s.late_skipped;
    return 0;
}

// Overrides the live gradient scale (tests: a scale far too large makes the 16-bit gradients overflow; tuning).  gs_max > 0
// also replaces the ceiling the scale may grow back to.
extern "C" int orn_engine_set_grad_scale(orn_engine *e, float gs, float gs_max)
{
    ORN_REQUIRE(e && gs >= 1.0f, "engine_set_grad_scale: scale must be >= 1");
    OrnScaleState sa[ORN_SCALE_SLOTS];
    hipError_t rc = hipDeviceSynchronize();
    if (rc == hipSuccess) rc = hipMemcpy(sa, e->sc, sizeof(sa), hipMemcpyDeviceToHost);
    for (int r = 0; r < ORN_SCALE_SLOTS; ++r) {
        sa[r].gs = gs; sa[r].inv_gs = 1.0f / gs;
        if (gs_max > 0.f) sa[r].gs_max = gs_max;
    }
    sa[0].good = 0;
    if (rc == hipSuccess) rc = hipMemcpy(e->sc, sa, sizeof(sa), hipMemcpyHostToDevice);
    if (rc != hipSuccess) { orn_set_error("engine_set_grad_scale: %s", hipGetErrorString(rc)); return (int)rc; }
    return 0;
}

extern "C" int orn_engine_fused_kernel(orn_engine *e, int layer, const float **wf, const float **bf)
{
    ORN_REQUIRE(e && wf && bf && layer >= 0 && layer < e->d.n_layers, "engine_fused_kernel: bad arguments");
    *wf = e->L[layer].wf;
    *bf = e->L[layer].bf;
    return 0;
}
