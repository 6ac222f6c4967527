// Every form of the engine's training step (orn_engine.h): the schedule advance, the two halves of a step around the loss, the side
// branch of the pipelined form, and the entries -- single, pipelined, batched, split, profiling, graph.
#include "orn_engine.h"
#include <climits>

// ------------------------------------------------------------------------------------------------
// Loss-scale bookkeeping of an advance (one thread): folds the flags of the steps that have just run into the scale and notes that
// `launched` optimiser steps follow.  Returns the optimiser steps skipped so far.
__device__ static int32_t advance_scale(OrnScaleState *sc, int launched)
{
    // the steps of the group that has just run: any overflow halves the scale (once per advance); clean groups are credited
    // now that they HAVE run, and ORN_SCALE_GROWTH_INTERVAL clean steps double the scale again, up to its initial value
    int nflag = 0;
    for (int r = 0; r < ORN_SCALE_SLOTS; ++r)
        if (sc[r].flag) { nflag += 1; sc[r].flag = 0; }
    // late-only skips of the pipelined step (the side branch's Adam launch counts them, possibly after this advance has run:
    // then the next one backs off).  A counter and not a flag: a flag would be read by the next step's Adam, which is clean
    const int32_t late = __atomic_load_n(&sc->late_skipped, __ATOMIC_RELAXED);
    if (late != sc->late_seen) { nflag += 1; sc->late_seen = late; }
    float gs = sc->gs;
    if (nflag) {
        gs = fmaxf(gs * 0.5f, 1.0f);
        sc->good = 0; sc->backoffs += 1;
    } else {
        sc->good += sc->launched;
        if (sc->good >= ORN_SCALE_GROWTH_INTERVAL && gs < sc->gs_max) { gs *= 2.0f; sc->good = 0; }
    }
    sc->launched = launched;
    for (int r = 0; r < ORN_SCALE_SLOTS; ++r) { sc[r].gs = gs; sc[r].inv_gs = 1.0f / gs; }
    return sc->skipped;
}

// The state of a step that takes step count and lr from schedule entry s, and `frame`
__device__ static OrnStepCur advance_cur(const orn_step_sched &s, int32_t frame, int32_t skipped, double beta1, double beta2, int32_t slot)
{
    OrnStepCur c;
    c.frame = frame;
    c.step = max(s.step - skipped, 1);              // torch: a skipped optimizer.step() does not advance Adam's step count
    c.lr = s.lr;
    // torch.optim.Adam: bias corrections in double, rounded to fp32 once
    const double bc1 = 1.0 - pow(beta1, (double)c.step), bc2 = 1.0 - pow(beta2, (double)c.step);
    c.step_size = (float)((double)s.lr / bc1);
    c.sqrt_bc2 = (float)sqrt(bc2);
    c.slot = slot;
    c.pad[0] = c.pad[1] = 0;
    return c;
}

// `count` consecutive steps at once (thread j -> cur[j]): the unrolled graph advances once for all its steps
__global__ void k_advance(const orn_step_sched *__restrict__ sched, int32_t *cursor, int32_t n_slots, double beta1,
                          double beta2, OrnStepCur *cur_all, int count, OrnScaleState *sc)
{
    const int32_t c0 = *cursor;
    __shared__ int32_t skipped;
    if (threadIdx.x == 0) skipped = advance_scale(sc, count);
    __syncthreads();
    if (blockIdx.x == 0 && (int)threadIdx.x < count) {
        const int32_t c = c0 + threadIdx.x;
        const orn_step_sched s = sched[c];
        cur_all[threadIdx.x] = advance_cur(s, s.frame, skipped, beta1, beta2, n_slots > 0 ? c % n_slots : 0);
        if (threadIdx.x == 0) *cursor = c0 + count;
    }
}

// The batched form of the advance (orn_engine_train_steps_batch): ONE optimiser step that consumes `batch` schedule entries.  Flags
// and scale are processed once, as k_advance does for a group of one step (one clean step credited per optimiser step, however
// many frames it had).  step (less the skipped steps) and lr come from the first entry, the frames from all of them:
//   cur0   the optimiser step's state: Adam's scalars, the first frame, the ring slot (optimiser-step index % n_slots)
//   bcur   the frame table: the same state per frame j, with frame = sched[c0 + j].frame and slot = j (where the loss's finalize
//          stage leaves that frame's stats)
__global__ void k_advance_batch(const orn_step_sched *__restrict__ sched, int32_t *cursor, int32_t n_slots, double beta1, double beta2,
                                OrnStepCur *cur0, OrnStepCur *bcur, int batch, OrnScaleState *sc)
{
    const int32_t c0 = *cursor;
    __shared__ int32_t skipped;
    if (threadIdx.x == 0) skipped = advance_scale(sc, 1);      // (late-only skips: left by pipelined calls before this one)
    __syncthreads();
    if ((int)threadIdx.x < batch) {
        const int j = threadIdx.x;
        OrnStepCur c = advance_cur(sched[c0], sched[c0 + j].frame, skipped, beta1, beta2, j);
        bcur[j] = c;
        if (j == 0) {
            c.slot = n_slots > 0 ? (c0 / batch) % n_slots : 0;
            *cur0 = c;
            *cursor = c0 + batch;
        }
    }
}

// Backward of side stage i (orn_engine_forward.hip, side_forward), to run behind block i + 1's dgrad and in front of block i's own
// backward: adds W_i^T du_i to the gradient block i + 1 left for block i's output and writes the head's own gradients (un-scaled)
// into the arena.
static int side_backward(orn_engine *e, int i, hipStream_t st, OrnScaleState *sc)
{
    const orn_engine_desc &d = e->d;
    const orn_engine::SideStage &s = e->stage[i];
    const float *w = e->params + d.side_head_w[i];
    float *dw = e->grads + d.side_head_w[i], *db = e->grads + d.side_head_b[i];
    if (i >= e->ff)
        return e->ops->side_head_bwd(e->L[i].zb, w, s.img, s.dimg, s.C, s.H, s.W, d.sigmoid, d.layer[i].s, d.lw, e->gs, e->L[i].dypad, dw, db,
                                     s.head_ws, st, sc, d.act);
    return orn_launch_side_head_bwd_f32(e->L[i].a, w, s.img, s.dimg, s.C, s.H, s.W, d.sigmoid, d.lw, e->L[i].da, dw, db, s.head_ws, st, sc);
}

static OrnMergeMisc merge_misc(const orn_engine *e, int i)
{
    const orn_layer_desc &l = e->d.layer[i];
    float *G = e->grads;
    OrnMergeMisc m = {};
    m.C = l.C; m.O = l.O;
    m.g = G + l.w3x3; m.dbf = G + l.b3x3; m.dw1p = e->L[i].dw1p;
    m.d3x1 = G + l.w3x1; m.db3x1 = G + l.b3x1; m.d1x3 = G + l.w1x3; m.db1x3 = G + l.b1x3;
    m.dw1 = G + l.w1;
    if (e->d.precision != 0) { m.dw2t = e->L[i].dw2t; m.dw2 = G + l.w2; }
    return m;
}

// The side branch of a pipelined step, first half (enqueued at the fork point, fork_behind_dgrad): the weight gradient of the block below the
// last one (side_below), then the last block's weight gradient (+ the head's dW / db finish), its slab reduction, its merge backward.
static int side_branch_backward(orn_engine *e, hipStream_t st)
{
    const orn_engine_desc &d = e->d;
    const int nl = d.n_layers;
    float *G = e->grads;
    hipStream_t sd = e->side;
    OrnScaleState *sc = e->sc_side;                     // this step's scale, copied by the loss's finalize stage; the branch's detections
    ORN_HIP(hipEventRecord(e->ev_fork, st));
    ORN_HIP(hipStreamWaitEvent(sd, e->ev_fork, 0));
    if (e->side_below) {      // (its dy is the output of the dgrad launch this branch forks behind; its slabs are reduced on the caller's stream)
        const OrnWgradJob wb = wgrad_job(e, nl - 2);
        ORN_TRY(e->ops->wgrad_batch(1, &wb, sd, nullptr, nullptr, 1, d.act));
        ORN_HIP(hipEventRecord(e->ev_below, sd));
    }
    const OrnWgradJob wj = wgrad_job(e, nl - 1);
    const OrnHeadFinish hf = {e->head_ws, e->ops->head_bwd_blocks(e->Hout, e->Wout), e->Cn_last, 1.0f / e->gs, G + d.head_w, G + d.head_b, sc};
    ORN_TRY(e->ops->wgrad_batch(1, &wj, sd, &hf, nullptr, 1, d.act));
    ORN_HIP(hipEventRecord(e->ev_wgrad, sd));           // the last block's input buffer is free again
    const OrnWgradReduce wr = wgrad_reduce(e, nl - 1, sc);
    ORN_TRY(e->ops->wgrad_reduce_all(1, &wr, sd, nullptr, d.act));
    if (d.erb) {
        const orn_engine::MergeSet &ms = e->mset[2];
        ORN_TRY(orn_launch_merge_h16_bwd(ms.mh_tables, ms.mh_host, sd, sc));
        const OrnMergeMisc mm = merge_misc(e, nl - 1);
        ORN_TRY(orn_launch_merge_bwd_tail_all(1, &mm, sd));
    }
    return 0;
}

// Second half (enqueued behind the caller's Adam launch, whose skip decision it follows; a detection of the branch's own skips it too, as
// a late-only skip, counted in sc[0].late_skipped and folded into the scale by the next advance or the one after): Adam over the last block's and the head's
// parameters, then the last block's merge forward (or, without ERB, its 16-bit operand copies) for the NEXT step.
// more: another step follows in this call (the last step of a call skips the merge forward: the next call's first step merges every
// block itself, the parameters may have been touched in between)
static int side_branch_update(orn_engine *e, bool more)
{
    const orn_engine_desc &d = e->d;
    const int nl = d.n_layers;
    hipStream_t sd = e->side;
    const size_t lo = e->side_lo;
    ORN_HIP(hipStreamWaitEvent(sd, e->ev_adam, 0));
    ORN_TRY(orn_launch_adam(e->params + lo, e->grads + lo, e->m + lo, e->v + lo, (size_t)d.n_params - lo, 0.0, 1, e->cur_side, d.beta1, d.beta2,
                            d.eps, 1.0f, sd, e->gmask ? e->gmask + lo : nullptr, e->sc_side, nullptr, nullptr, false, e->sc));
    const void *packs = nullptr;        // (16-bit ERB) the branch's pack jobs, launched behind the join event
    if (more && d.erb) {
        const orn_engine::MergeSet &ms = e->mset[2];
        const OrnLinearJob none = {};
        ORN_TRY(orn_launch_w2_transpose(ms.n, ms.ml, sd));
        ORN_TRY(orn_launch_merge_group_linear(ms.tables, 0, ms.tiles[0], none, sd, nullptr, 0, d.act));
        ORN_TRY(orn_launch_merge_group_linear(ms.tables, 1, ms.tiles[1], none, sd, nullptr, 0, d.act));   // the S epilogue writes the 16-bit operand copies
        packs = ms.mh_host;
    } else if (more) {
        const OrnPrepLayer pl = prep_layer(e, nl - 1);
        ORN_TRY(e->ops->prep_all(1, &pl, sd));
    }
    ORN_HIP(hipEventRecord(e->ev_join, sd));
    if (packs) {
        // The pack jobs that ride on these launches in the serial step (half copies for the NEXT merge backward of this block: needed
        // a whole step later) are launches of their own BEHIND the join event here: the branch's S launch runs while the 8-wave forward
        // conv of the block below holds all but a few CUs, and 160 rider work-groups in front of its 84 tiles cost it those (as riders:
        // +3..10 us per step).
        ORN_TRY(orn_launch_merge_h16_pack_jobs(packs, 1, sd));
        ORN_TRY(orn_launch_merge_h16_pack_jobs(packs, 2, sd));
    }
    e->side_busy = true;
    return 0;
}

// Weight gradients of every fast layer the caller's stream keeps: nothing on the dgrad chain needs them, so they run behind it as ONE
// launch (the small layers' 72 / 216 / 360 work-groups pack behind the last block's 504 instead of leaving CUs idle one launch
// at a time: -37 us per 720p step), followed by ONE launch that reduces every layer's split-K slabs (-27 us).  The stem backward's
// deferred kernels (needed by Adam only) ride on the two launches.
static int fast_weight_grads(orn_engine *e, hipStream_t st, bool pipe, OrnScaleState *sc, const OrnStemL2Job *l2job, const OrnStemW0Job *w0job)
{
    const orn_engine_desc &d = e->d;
    const int nl = d.n_layers, ff = e->ff;
    OrnWgradJob wj[ORN_MAX_LAYERS];
    int nj = 0;
    const int n_main = pipe ? nl - 1 : nl;      // (pipelined step: the last block's is the side branch's)
    for (int i = n_main - 1; i >= ff; --i) {    // largest first
        if (pipe && i == nl - 2 && e->side_below) continue;      // (the side stream's)
        wj[nj++] = wgrad_job(e, i);
    }
    const OrnHeadFinish hf = {e->head_ws, e->ops->head_bwd_blocks(e->Hout, e->Wout), e->Cn_last, 1.0f / e->gs, e->grads + d.head_w, e->grads + d.head_b, sc};
    if (e->prof) (void)hipEventRecord(e->prof_ev[4 * ORN_MAX_LAYERS], st);
    ORN_TRY(e->ops->wgrad_batch(nj, wj, st, pipe ? nullptr : &hf, l2job, 0, d.act));
    if (e->prof) (void)hipEventRecord(e->prof_ev[4 * ORN_MAX_LAYERS + 1], st);
    OrnWgradReduce wr[ORN_MAX_LAYERS];
    for (int i = ff; i < n_main; ++i) wr[i - ff] = wgrad_reduce(e, i, sc);
    if (e->prof) (void)hipEventRecord(e->prof_ev[4 * ORN_MAX_LAYERS + 2], st);
    if (pipe && e->side_below) ORN_HIP(hipStreamWaitEvent(st, e->ev_below, 0));
    ORN_TRY(e->ops->wgrad_reduce_all(n_main - ff, wr, st, w0job, d.act));
    if (e->prof) (void)hipEventRecord(e->prof_ev[4 * ORN_MAX_LAYERS + 3], st);
    return 0;
}

// (ERB) merge backward of every layer of a set (closed forms): dW3 & dT, then dW2 & dW1, then the slices
static int merge_backward(orn_engine *e, const orn_engine::MergeSet &ms, hipStream_t st, OrnScaleState *sc)
{
    if (e->d.precision != 0) {
        ORN_TRY(orn_launch_merge_h16_bwd(ms.mh_tables, ms.mh_host, st, sc));
    } else {
        ORN_TRY(orn_launch_merge_group(ms.tables, 2, ms.tiles[2], st));
        ORN_TRY(orn_launch_merge_group(ms.tables, 3, ms.tiles[3], st));
    }
    OrnMergeMisc mm[ORN_MAX_LAYERS];
    for (int k = 0; k < ms.n; ++k) mm[k] = merge_misc(e, ms.layer[k]);
    ORN_TRY(orn_launch_merge_bwd_tail_all(ms.n, mm, st));
    return 0;
}

// A step in two halves, split at the loss: step_front produces e->img (schedule advance + training forward), step_back consumes
// dLoss/dimg and the loss's finalize job (head -> dgrad chain -> stem -> weight gradients -> merge backward -> Adam).  train_step runs
// a built-in loss between them; the split entries (orn_engine_step_forward / _backward) leave that place to the caller.
static int step_front(orn_engine *e, const float *embeds, const orn_step_sched *sched, int32_t *cursor, int32_t n_slots, hipStream_t st,
                      const StepOpts &o)
{
    const orn_engine_desc &d = e->d;
    if (o.advance > 0) {
        hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, st, sched, cursor, n_slots, d.beta1, d.beta2, e->cur, o.advance, e->sc /* all entries */);
        ORN_LAUNCH_CHECK("advance");
    }
    const int *fidx = &step_cur(e, o)->frame;
    return forward(e, embeds, fidx, true, st, d.n_layers - 1, (o.batch > 0 && o.bframe > 0) ? (int)MERGE_NONE : (o.pipe && e->side_busy) ? 1 : 0, true,
                   d.multi_res ? e->sc + o.cur : nullptr);
}

// Multi-resolution heads, end of a step (one thread): the per-stage ring's entry {loss_i, psnr_i} of every stage, and the weighted
// sum in the loss entry of the step's record, ((lw l_0 + lw l_1) + ..) + l_last as Python's sum() forms it (main_train.py:243-244).
// ring: where the last stage's finalize left the record {l_last, L1, MSE, s, PSNR, ..} at cur->slot (null: none kept).
struct StageRecord {
    int n_side;
    const float *stats[ORN_MAX_LAYERS];     // the side stages' loss stats
    float lw;
    const OrnStepCur *cur;
    float *ring, *stage_ring;
};
__global__ void k_stage_record(StageRecord r)
{
    if (threadIdx.x != 0 || !r.ring) return;
    float *rec = r.ring + (size_t)r.cur->slot * 8;
    const float last = rec[0];
    float sum = 0.f;
    for (int i = 0; i < r.n_side; ++i) sum = __fadd_rn(sum, __fmul_rn(r.lw, r.stats[i][0]));      // (two roundings, as torch: never an fma)
    rec[0] = sum + last;
    if (r.stage_ring) {
        float *s = r.stage_ring + (size_t)r.cur->slot * (r.n_side + 1) * 2;
        for (int i = 0; i < r.n_side; ++i) { s[2 * i] = r.stats[i][0]; s[2 * i + 1] = r.stats[i][4]; }
        s[2 * r.n_side] = last; s[2 * r.n_side + 1] = rec[4];
    }
}

// dimg: dLoss/d(e->img), fp32 planar (the engine's own buffer, or the caller's in a split step); fin: the loss's finalize stage for a
// 16-bit engine's head backward to carry (n_l1 == 0: none)
static int step_back(orn_engine *e, const float *embeds, const float *dimg, OrnLossFinalJob &fin, float *stats_out, hipStream_t st,
                     const StepOpts &o)
{
    const orn_engine_desc &d = e->d;
    const bool pipe = o.pipe;
    float *P = e->params, *G = e->grads;
    const int Nout = d.fc_h * d.fc_w * d.fc_dim;
    const size_t HWo = (size_t)e->Hout * e->Wout;
    const bool batched = o.batch > 0;
    OrnStepCur *cur = step_cur(e, o);
    OrnScaleState *const sc = e->sc + o.cur;            // this step's entry: its own flag, the shared scale
    const int *fidx = &cur->frame;
    const int nl = d.n_layers, ff = e->ff;
    if (pipe) { fin.cur_copy = e->cur_side; fin.sc_copy = e->sc_side; }     // (the previous step's side branch was joined in forward())
    if (ff < nl)
        ORN_TRY(e->ops->head_bwd(e->L[nl - 1].zb, P + d.head_w, e->img, dimg, e->Cn_last, e->Hout, e->Wout, d.sigmoid,
                                 d.layer[nl - 1].s, e->gs, e->L[nl - 1].dypad, nullptr, nullptr, e->head_ws, st, sc, &fin, d.act));   // dW / db: finished with the wgrad batch
    const bool head_fused32 = f32_head_on_z(e);
    const OrnHeadBwdFuse hfuse = {P + d.head_w, e->img, dimg, d.sigmoid, G + d.head_w, G + d.head_b, e->head_ws};
    if (ff >= nl && !head_fused32)
        ORN_TRY(orn_launch_head_bwd(e->L[nl - 1].a, P + d.head_w, e->img, dimg, 1, e->Cn_last, HWo, d.sigmoid, e->L[nl - 1].da,
                                    G + d.head_w, G + d.head_b, e->scratch, st));
    if (ff >= nl) {
        // fp32 engine: every layer's dgrad kernel (flipped taps, transposed) in one launch instead of one per layer
        const float *wfs[ORN_MAX_LAYERS]; float *wds[ORN_MAX_LAYERS]; int Os[ORN_MAX_LAYERS], Cs[ORN_MAX_LAYERS];
        for (int i = 0; i < nl; ++i) { wfs[i] = e->L[i].wf; wds[i] = e->L[i].wd32; Os[i] = d.layer[i].O; Cs[i] = d.layer[i].C; }
        ORN_TRY(orn_launch_flip_transpose_all(nl, wfs, wds, Os, Cs, st));
    }
    for (int i = nl - 1; i >= 0; --i) {
        const orn_layer_desc &l = d.layer[i];
        LayerBuf &b = e->L[i];
        const float *x = (i == 0) ? e->h2 : e->L[i - 1].a;
        float *dx = (i == 0) ? e->dh2 : e->L[i - 1].da;
        // dWf / dbf land directly in the 3x3 branch's gradient slots (dW3x3 = dWf, db3x3 = dbf)
        if (e->prof) (void)hipEventRecord(e->prof_ev[2 * ORN_MAX_LAYERS + 2 * i], st);
        if (i >= ff) {
            // (the wgrads of all fast layers run as one multi-problem launch after the dgrad chain, see below)
            if (i > ff) {
                // few pixel tiles: input-chunk split through fp32 partial slabs in the scratch, finished into dypad
                float *part = e->ops->dgrad_f32_slabs(l.H, l.W, l.O) > 1 ? e->scratch : nullptr;
                ORN_TRY(e->ops->conv_dgrad(b.dypad, b.wd, l.H, l.W, l.O, l.C, e->L[i - 1].zb, e->L[i - 1].dypad, d.layer[i - 1].s,
                                           part, st, l.C, d.act));
            } else {
                ORN_TRY(e->ops->conv_dgrad(b.dypad, b.wd, l.H, l.W, l.O, ORN_FAST_C, nullptr, nullptr, 1, e->dxn, st, l.C, d.act));
                if (!e->stage0)
                ORN_TRY(e->ops->to_nchw_f32(e->dxn, l.C, ORN_FAST_C, l.H, l.W, e->ops->dgrad_f32_slabs(l.H, l.W, l.O), 1.0f / e->gs, dx,
                                            st, sc));
            }
        } else if (e->stage0) {
            const orn_layer_desc &l1 = d.layer[1];
            ORN_TRY(orn_launch_stage0_bwd(x, b.wf, b.z, e->dxn, e->ops->dgrad_f32_slabs(l1.H, l1.W, l1.O), ORN_FAST_C, 1.0f / e->gs, l.C, l.O,
                                          l.H, l.W, l.s, e->scratch + e->stem_ws, nullptr, G + l.w3x3, G + l.b3x3, st, sc, d.act));
        } else
        ORN_TRY(orn_launch_conv_bwd_f32(x, b.wf, b.z, b.da, 1, l.C, l.O, l.H, l.W, l.s, dx, G + l.w3x3, G + l.b3x3, e->scratch, st,
                                        (i == nl - 1 && head_fused32) ? &hfuse : nullptr, ff >= nl ? b.wd32 : nullptr, d.act));
        if (e->prof) (void)hipEventRecord(e->prof_ev[2 * ORN_MAX_LAYERS + 2 * i + 1], st);
        if (pipe && e->fork_behind_dgrad && i == nl - 1) ORN_TRY(side_branch_backward(e, st));     // fork: behind the last block's dgrad
        // multi-resolution heads: block i - 1's gradient buffer holds what this block sent down; its stage's head adds its own term
        if (d.multi_res && i >= 1) ORN_TRY(side_backward(e, i - 1, st, sc));
    }
    // stem backward; with a wgrad batch behind it, its last kernel (needed by Adam only) rides along that launch
    OrnStemW0Job w0job;
    OrnStemL2Job l2job;
    const bool defer_w0 = ff < nl;
    ORN_TRY(orn_launch_stem_bwd(embeds, fidx, d.embed_len, P + d.stem_w1, e->pre1, e->h1, e->pre2,
                                e->stage0 ? e->scratch + e->stem_ws : e->dh2, 1, d.embed_len, d.stem_dim, Nout, G + d.stem_w0,
                                G + d.stem_b0, G + d.stem_w1, G + d.stem_b1, e->scratch, st,
                                e->stage0 ? orn_stage0_slabs(d.layer[0].O, d.layer[0].s) : 1, defer_w0 ? &w0job : nullptr, defer_w0 ? &l2job : nullptr,
                                d.act, defer_w0 ? sc : nullptr));      // (the riders flag a non-finite stem gradient like the wgrad reduction beside them)
    if (ff < nl) ORN_TRY(fast_weight_grads(e, st, pipe, sc, &l2job, &w0job));
    if (pipe && !e->fork_behind_dgrad) ORN_TRY(side_branch_backward(e, st));     // fork: behind the lower blocks' slab reduction
    if (d.multi_res) {      // (behind the head's backward, which carries a 16-bit engine's loss finalize: the step's -- or, batched, the frame's -- record exists)
        StageRecord r = {};
        r.n_side = nl - 1;
        for (int i = 0; i < nl - 1; ++i) r.stats[i] = e->stage[i].stats;
        r.lw = d.lw; r.cur = cur; r.ring = batched ? e->b_stats : stats_out; r.stage_ring = e->stage_ring;
        hipLaunchKernelGGL(k_stage_record, dim3(1), dim3(64), 0, st, r);
        ORN_LAUNCH_CHECK("stage_record");
    }
    if (batched) {
        // every directly written gradient slot holds this frame's gradient: fold it into the batch's sum (B == 1: it is the sum)
        if (o.batch > 1)
            ORN_TRY(orn_launch_grad_accum(e->acc_tab, G, e->b_acc, o.bframe == 0 ? 0 : (o.bframe + 1 < o.batch ? 1 : 2), 1.0f / (float)o.batch, st));
        if (o.batch > 1 && e->side_tab.n)
            ORN_TRY(orn_launch_grad_accum(e->side_tab, G, e->b_acc, o.bframe == 0 ? 0 : (o.bframe + 1 < o.batch ? 1 : 2), 1.0f / (float)o.batch, st));
        if (o.bframe + 1 < o.batch) return 0;
        cur = e->cur;                                   // the optimiser step's own state (k_advance_batch)
        if (stats_out) ORN_TRY(orn_launch_batch_stats(e->b_stats, o.batch, cur, stats_out, st));
    }
    if (d.erb) ORN_TRY(merge_backward(e, e->mset[pipe ? 1 : 0], st, sc));
    if (e->nbr) ORN_TRY(orn_launch_branch_merge_bwd(e->nbr, e->bl, st));     // ACB / RepVGG / ECB: dWf / dbf (3x3 slots) -> the other branches' slots
    if (pipe) {
        // this stream's Adam launch covers everything below the last block; its skip decision is mirrored for the side branch's launch
        // (into sc_side->mirrored: a word of its own, apart from the flag the side branch's detectors raise meanwhile)
        ORN_TRY(orn_launch_adam(P, G, e->m, e->v, e->side_lo, 0.0, 1, cur, d.beta1, d.beta2, d.eps, 1.0f, st, e->gmask, sc, e->sc, e->sc_side));
        ORN_HIP(hipEventRecord(e->ev_adam, st));
        return side_branch_update(e, o.more);
    }
    ORN_TRY(orn_launch_adam(P, G, e->m, e->v, (size_t)d.n_params, 0.0, 1, cur, d.beta1, d.beta2, d.eps, 1.0f, st, e->gmask, sc, e->sc));
    return 0;
}

// forward -> loss -> backward -> Adam: both halves around the engine's own loss
static int train_step(orn_engine *e, const float *frames, const float *embeds, const orn_step_sched *sched,
                      int32_t *cursor, float *stats_out, int32_t n_slots, hipStream_t st, const StepOpts &o = StepOpts())
{
    const orn_engine_desc &d = e->d;
    ORN_TRY(step_front(e, embeds, sched, cursor, n_slots, st, o));
    const OrnStepCur *cur = step_cur(e, o);
    OrnLossFinalJob fin = {};
    ORN_TRY(orn_launch_loss(e->img, frames, &cur->frame, (size_t)3 * e->Hout * e->Wout, 1, 3, e->Hout, e->Wout, d.loss_type, 1.0f, e->stats, e->dimg,
                            e->loss_ws, st, cur, o.batch > 0 ? e->b_stats : stats_out, e->sc + o.cur,
                            orn_loss_spec_of(d.loss_type)->kind == ORN_LOSS_KIND_SSIM ? e->tstats : nullptr,
                            e->ff < d.n_layers ? &fin : nullptr));     // 16-bit engine: the finalize stage rides on the head's backward launch
    return step_back(e, embeds, e->dimg, fin, stats_out, st, o);
}

// Every side stage has its target table, and the per-stage ring (if any) has the slots this call's records go to
static int side_ready(const orn_engine *e, int32_t slots_needed, const char *name)
{
    if (!e->d.multi_res) return 0;
    for (int i = 0; i + 1 < e->d.n_layers; ++i)
        if (!e->stage[i].targets) {
            orn_set_error("%s: stage %d has no target table (orn_engine_set_stage_targets)", name, i);
            return ORN_E_STATE;
        }
    ORN_REQUIRE(!e->stage_ring || e->stage_slots >= slots_needed, "%s: the per-stage ring has %d slots, %d needed", name, e->stage_slots, slots_needed);
    return 0;
}

// What every training entry checks first, in this order.  args: the entry's own pointers and counts are good (else `complaint`);
// ring_slots: slots of the per-stage ring its records need (NO_SIDE: an entry without a multi-resolution form, which says so itself)
enum { NO_SIDE = INT_MIN };
static int entry_check(const orn_engine *e, bool args, const char *name, const char *complaint, int32_t ring_slots)
{
    ORN_REQUIRE(e && args, "%s: %s", name, complaint);
    ORN_REQUIRE(e->grads && e->m && e->v, "%s: engine was created without grads / Adam arenas", name);
    ORN_REQUIRE_CLOSED(e, name);
    return ring_slots == NO_SIDE ? 0 : side_ready(e, ring_slots, name);
}

extern "C" int orn_engine_train_step(orn_engine *e, const float *frames, const float *embeds,
                                     const orn_step_sched *sched, int32_t *cursor, float *stats_out, int32_t n_slots,
                                     void *stream)
{
    ORN_TRY(entry_check(e, frames && embeds && sched && cursor, "engine_train_step", "null pointer", n_slots > 0 ? n_slots : 1));
    return train_step(e, frames, embeds, sched, cursor, stats_out, n_slots, (hipStream_t)stream);
}

// ---- the split step: the caller's own loss between the two halves (include/orn.h) ----
extern "C" int orn_engine_step_forward(orn_engine *e, const float *frames, const float *embeds, const orn_step_sched *sched,
                                       int32_t *cursor, int32_t n_slots, const float **pred, void *stream)
{
    ORN_TRY(entry_check(e, frames && embeds && sched && cursor && pred, "engine_step_forward", "null pointer", NO_SIDE));
    ORN_REQUIRE(!e->d.multi_res, "engine_step_forward: a multi-resolution engine has no split step (a caller's objective takes one image)");
    assert(!e->side_busy);          // orn_engine_train_steps joins its side branch before it returns
    ORN_TRY(step_front(e, embeds, sched, cursor, n_slots, (hipStream_t)stream, StepOpts()));
    *pred = e->img;
    e->open = true;
    e->open_st = (hipStream_t)stream;
    return 0;
}

extern "C" int orn_engine_step_backward(orn_engine *e, const float *frames, const float *embeds, const float *dpred,
                                        const float *loss, float *stats_out, int32_t n_slots, void *stream)
{
    ORN_REQUIRE(e && frames && embeds, "engine_step_backward: null pointer");
    (void)n_slots;                  // (the ring slot was fixed by the forward half's advance)
    if (!e->open) {
        orn_set_error("engine_step_backward: no open step (orn_engine_step_forward first)");
        return ORN_E_STATE;
    }
    hipStream_t st = (hipStream_t)stream;
    ORN_REQUIRE(st == e->open_st, "engine_step_backward: not the stream of the step's forward half");
    ORN_REQUIRE((uintptr_t)dpred % 4 == 0 && (uintptr_t)loss % 4 == 0, "engine_step_backward: dpred / loss must be float-aligned");
    e->open = false;
    const orn_engine_desc &d = e->d;
    const OrnStepCur *cur = e->cur;
    ORN_TRY(orn_launch_loss_ext(e->img, frames, &cur->frame, (size_t)3 * e->Hout * e->Wout, 3, e->Hout, e->Wout, dpred, loss, e->stats,
                                e->loss_ws, st, cur, stats_out, e->sc));
    if (!dpred)                     // abandoned: the flag is up, so this launch changes nothing and counts the skipped step
        return orn_launch_adam(e->params, e->grads, e->m, e->v, (size_t)d.n_params, 0.0, 1, cur, d.beta1, d.beta2, d.eps, 1.0f, st, e->gmask,
                               e->sc, e->sc);
    OrnLossFinalJob none = {};      // (16-bit engines: nothing rides on the head's backward launch)
    return step_back(e, embeds, dpred, none, stats_out, st, StepOpts());
}

// n_steps steps enqueued on `stream` (no graph): where the engine can (struct orn_engine, `side`) in the pipelined form, the
// last block's weight-gradient chain of step k running on the engine's own second stream beside the boundary of steps k / k + 1.
// Everything is joined back into `stream` before the call returns, so the caller's stream order covers all of it.
extern "C" int orn_engine_train_steps(orn_engine *e, const float *frames, const float *embeds, const orn_step_sched *sched,
                                      int32_t *cursor, float *stats_out, int32_t n_slots, int32_t n_steps, void *stream)
{
    ORN_TRY(entry_check(e, frames && embeds && sched && cursor && n_steps >= 0, "engine_train_steps", "bad arguments", n_slots > 0 ? n_slots : 1));
    hipStream_t st = (hipStream_t)stream;
    int rc = 0;
    StepOpts o;
    o.pipe = e->pipe_ok;
    for (int k = 0; k < n_steps && rc == 0; ++k) {
        o.more = k + 1 < n_steps;
        rc = train_step(e, frames, embeds, sched, cursor, stats_out, n_slots, st, o);
    }
    if (e->side_busy) {
        const hipError_t hrc = hipStreamWaitEvent(st, e->ev_join, 0);
        e->side_busy = false;
        if (hrc != hipSuccess && rc == 0) { orn_set_error("engine_train_steps: join: %s", hipGetErrorString(hrc)); rc = (int)hrc; }
    }
    return rc;
}

// n_steps optimiser steps of `batch` frames each, serial form, on the caller's stream: per step the batched advance, then the
// frames one behind the other (train_step, StepOpts::batch).
extern "C" int orn_engine_train_steps_batch(orn_engine *e, const float *frames, const float *embeds, const orn_step_sched *sched,
                                            int32_t *cursor, float *stats_out, int32_t n_slots, int32_t n_steps, int32_t batch, void *stream)
{
    ORN_TRY(entry_check(e, frames && embeds && sched && cursor && n_steps >= 0, "engine_train_steps_batch", "bad arguments", batch));
    ORN_REQUIRE(e->b_acc, "engine_train_steps_batch: no batch workspace (orn_engine_set_batch_ws)");
    ORN_REQUIRE(batch >= 1 && batch <= e->b_max, "engine_train_steps_batch: batch=%d outside [1, %d] (max_batch of the workspace)", batch, e->b_max);
    assert(!e->side_busy);          // orn_engine_train_steps joins its side branch before it returns
    hipStream_t st = (hipStream_t)stream;
    StepOpts o;
    o.advance = 0;
    o.batch = batch;
    for (int k = 0; k < n_steps; ++k) {
        hipLaunchKernelGGL(k_advance_batch, dim3(1), dim3(64), 0, st, sched, cursor, n_slots, e->d.beta1, e->d.beta2, e->cur, e->b_cur, (int)batch,
                           e->sc /* all entries */);
        ORN_LAUNCH_CHECK("advance_batch");
        for (o.bframe = 0; o.bframe < batch; ++o.bframe)
            ORN_TRY(train_step(e, frames, embeds, sched, cursor, stats_out, n_slots, st, o));
    }
    return 0;
}

// One EAGER training step with HIP events around every layer's forward conv launch, on the launch stream:
// ms_out[i] = duration of layer i's forward conv kernel inside a real step (bench.py's roofline leg).  Synchronises.
extern "C" int orn_engine_profile_step(orn_engine *e, const float *frames, const float *embeds, const orn_step_sched *sched,
                                       int32_t *cursor, float *stats_out, int32_t n_slots, float *ms_out, void *stream)
{
    ORN_TRY(entry_check(e, frames && embeds && sched && cursor && ms_out, "engine_profile_step", "null pointer", n_slots > 0 ? n_slots : 1));
    hipStream_t st = (hipStream_t)stream;
    const int nl = e->d.n_layers;
    for (int i = 0; i < 4 * ORN_MAX_LAYERS + 4; ++i)
        if (!e->prof_ev[i]) {
            hipError_t rc = hipEventCreate(&e->prof_ev[i]);
            if (rc != hipSuccess) { orn_set_error("engine_profile_step: hipEventCreate: %s", hipGetErrorString(rc)); return (int)rc; }
        }
    e->prof = true;
    const int trc = train_step(e, frames, embeds, sched, cursor, stats_out, n_slots, st);
    e->prof = false;
    if (trc != 0) return trc;
    hipError_t rc = hipStreamSynchronize(st);
    if (rc != hipSuccess) { orn_set_error("engine_profile_step: sync: %s", hipGetErrorString(rc)); return (int)rc; }
    auto span = [&](int a, float *out) -> int {
        float ms = 0.f;
        hipError_t r = hipEventElapsedTime(&ms, e->prof_ev[a], e->prof_ev[a + 1]);
        if (r != hipSuccess) { orn_set_error("engine_profile_step: elapsed: %s", hipGetErrorString(r)); return (int)r; }
        *out = ms;
        return 0;
    };
    const bool fast = e->ff < nl;
    for (int i = 0; i < nl; ++i) {
        ORN_TRY(span(2 * i, &ms_out[i]));
        ORN_TRY(span(2 * ORN_MAX_LAYERS + 2 * i, &ms_out[nl + i]));
    }
    ms_out[2 * nl] = ms_out[2 * nl + 1] = 0.f;
    if (fast) {
        ORN_TRY(span(4 * ORN_MAX_LAYERS, &ms_out[2 * nl]));
        ORN_TRY(span(4 * ORN_MAX_LAYERS + 2, &ms_out[2 * nl + 1]));
    }
    return 0;
}

extern "C" int orn_engine_train_steps_graph(orn_engine *e, const float *frames, const float *embeds,
                                            const orn_step_sched *sched, int32_t *cursor, float *stats_out,
                                            int32_t n_slots, int32_t n_steps, void *stream)
{
    ORN_TRY(entry_check(e, frames && embeds && sched && cursor && n_steps >= 0, "engine_train_steps_graph", "bad arguments", n_slots > 0 ? n_slots : 1));
    hipStream_t st = (hipStream_t)stream;
    const bool same = e->graph_exec && e->g_frames == frames && e->g_embeds == embeds && e->g_sched == sched &&
                      e->g_cursor == cursor && e->g_stats == stats_out && e->g_slots == n_slots && e->g_stream == st;
    if (!same) {
        drop_graphs(e);
        for (int pass = 0; pass < 2; ++pass) {
            const int reps = pass == 0 ? 1 : ORN_GRAPH_UNROLL;
            hipGraph_t *g = pass == 0 ? &e->graph : &e->graph_u;
            hipGraphExec_t *ge = pass == 0 ? &e->graph_exec : &e->graph_exec_u;
            hipError_t rc = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
            if (rc != hipSuccess) { orn_set_error("graph: BeginCapture failed: %s", hipGetErrorString(rc)); return (int)rc; }
            int trc = 0;
            for (int r = 0; r < reps && trc == 0; ++r) {
                StepOpts o;
                o.advance = r == 0 ? reps : 0;      // the first step of the graph advances the schedule for all of them
                o.cur = r;
                trc = train_step(e, frames, embeds, sched, cursor, stats_out, n_slots, st, o);
            }
            rc = hipStreamEndCapture(st, g);
            if (trc != 0) { if (*g) { (void)hipGraphDestroy(*g); *g = nullptr; } return trc; }
            if (rc != hipSuccess) { orn_set_error("graph: EndCapture failed: %s", hipGetErrorString(rc)); return (int)rc; }
            rc = hipGraphInstantiate(ge, *g, nullptr, nullptr, 0);
            if (rc != hipSuccess) { orn_set_error("graph: Instantiate failed: %s", hipGetErrorString(rc)); return (int)rc; }
        }
        e->g_frames = frames; e->g_embeds = embeds; e->g_sched = sched; e->g_cursor = cursor; e->g_stats = stats_out;
        e->g_slots = n_slots; e->g_stream = st;
    }
    int left = n_steps;
    // The host needs longer to launch the unrolled graph than the single-step one, and on an idle stream that launch is exposed (the
    // device waits for it): a call that will launch several graphs starts with ONE single step, and the unrolled launches queue up
    // behind it while it runs.  (20-step timed region after a synchronise: see DESIGN 6.)
    if (left > ORN_GRAPH_UNROLL) {
        hipError_t rc = hipGraphLaunch(e->graph_exec, st);
        if (rc != hipSuccess) { orn_set_error("graph: Launch failed: %s", hipGetErrorString(rc)); return (int)rc; }
        left -= 1;
    }
    while (left > 0) {
        const bool big = left >= ORN_GRAPH_UNROLL;
        hipError_t rc = hipGraphLaunch(big ? e->graph_exec_u : e->graph_exec, st);
        if (rc != hipSuccess) { orn_set_error("graph: Launch failed: %s", hipGetErrorString(rc)); return (int)rc; }
        left -= big ? ORN_GRAPH_UNROLL : 1;
    }
    return 0;
}
