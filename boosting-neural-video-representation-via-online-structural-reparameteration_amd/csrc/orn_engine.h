// A11  The per-frame training step of main_train.py:229-254 as one native engine:
//   stem -> N x {online ERB merge, conv3x3+PixelShuffle+SiLU} -> head -> loss (+PSNR) -> backward
//   -> Adam, every launch on the caller's stream, capturable as one hipGraph.
// The engine owns no device memory: four parameter-shaped arenas + one workspace come from the
// caller (PyTorch is only the allocator).
// This header (private to the library) holds the engine's state and what its three files share: orn_engine.hip (description, workspace
// carve, creation, setters), orn_engine_forward.hip (forward, decode, evaluation) and orn_engine_step.hip (every form of the step).
#pragma once
#include "orn_internal.h"
#include <cassert>

struct LayerBuf {
    float *T, *wf, *bf;   // merge products (ERB) -- wf/bf alias the params for vanilla/deploy
    float *w2t;           // tap-major copy of W2 (ERB): the T products read contiguous rows
    float *dT, *dw1p;     // merge backward scratch (ERB)
    float *dwap;          // merge backward scratch of an ECB block: the slabs of dwA (orn_merge_lin.hip)
    float *wd32;          // fp32 layers: flipped / transposed merged kernel for the dgrad (made for all layers in one launch)
    void *mh16;           // half operand copies of the merge backward (16-bit modes, orn_merge_h16.hip)
    float *dw2t;          // dW2 tap-major [9][O][2C] (16-bit modes)
    float *z, *a;         // block output (pre-activation, activation)          [fp32 layers]
    float *da;            // gradient wrt the block output                       [fp32 layers]
    // bf16 fast path (precision 1, layers >= ff): channels-last bf16, see orn_conv_bf16.hip
    uint16_t *xpad;       // conv input, zero-bordered [H+2][W+2][C]   (16-bit elements: bf16 or fp16)
    uint16_t *zb;         // pre-activation [Hs][Ws][Cn]
    uint16_t *dypad;      // gradient wrt conv output, zero-bordered [H+2][W+2][O']
    uint16_t *wb, *wd;    // merged kernel in 16 bit: forward / dgrad operand layouts
    float *biasp;         // bias in o' order
    float *wslab;         // split-K slabs of this layer's wgrad (reduced for all layers at the end of the backward)
};

// Created value-initialised (orn_engine_create): every member starts as zero / null / false.
struct orn_engine {
    orn_engine_desc d;
    float *params, *grads, *m, *v;
    const float *gmask;              // optional 0/1 gradient mask (prune fine-tune), same layout as the arenas
    const float *tstats;             // optional orn_loss_target_stats of the resident video (Fusion6)
    float *ws;
    // workspace carve
    float *pre1, *h1, *pre2, *h2, *dh2;
    float *img, *dimg, *stats;
    float *loss_ws;
    float *dec_ws;                   // orn_engine_decode_frames: per-block partial sums of the PSNR + the ticket (OrnDecodeOut)
    float *scratch;                  // shared scratch for the backward kernels
    float *head_ws;                  // 16-bit head backward: per-block partials (live until the deferred finish)
    OrnStepCur *cur;                 // state of the step in flight (device)
    LayerBuf L[ORN_MAX_LAYERS];
    int Hout, Wout, Cn_last;
    const OrnHalfOps *ops;           // 16-bit fast-path kernels (bf16 or fp16 build)
    float gs;                        // INITIAL gradient scale of the 16-bit gradient tensors (1 for bf16, 2^20 for fp16)
    OrnScaleState *sc;               // device: the live scale + non-finite flag (dynamic loss scaling, skipped steps)
    // (ERB) the grouped merge launches work on a SET of layers: all of them (a serial step, decode), or -- in the pipelined
    // form of the step, below -- all but the last block on the caller's stream and the last block alone on the side stream
    struct MergeSet {
        int n;                          // layers in the set (0: set not built)
        OrnMergeLayer ml[ORN_MAX_LAYERS];   // the layers as the merge launchers see them
        int layer[ORN_MAX_LAYERS];      // their indices in the engine
        void *tables;                   // device-resident grouped-GEMM problem tables
        int tiles[4];                   // work-groups of each table's launch, as orn_merge_groups_build counted them
        void *mh_tables, *mh_host;      // 16-bit modes: tables of the packed-operand merge backward (device / host)
    } mset[3];
    // (ACB / RepVGG / ECB, d.branch_kind) the blocks as the launchers of orn_merge_lin.hip see them: such a block is a single-conv block
    // whose (wf, bf) live in the workspace, merged by one launch in front of the forward and sent back by one behind the weight gradients
    int nbr;                         // 0: not such an engine
    OrnBranchLayer bl[ORN_MAX_LAYERS];
    int ff;                          // first layer on the bf16 fast path (== n_layers: none)
    float *dxn;                      // fp32 NHWC dgrad output of layer ff (converted to NCHW for the fp32 part)
    size_t stem_ws;                  // floats of `scratch` the stem backward uses (the fused first block's dx slabs sit behind them)
    bool stage0;                     // layer 0 is the only fp32 block and fits orn_stage0.hip: fused forward / backward
    // graph cache: one captured train step, and ORN_GRAPH_UNROLL steps back to back (the schedule is device-side, so
    // a longer graph is the same nodes repeated; it amortises the ~8 us gap between graph launches)
    hipGraph_t graph, graph_u;
    hipGraphExec_t graph_exec, graph_exec_u;
    const void *g_frames, *g_embeds, *g_sched, *g_cursor, *g_stats;
    int g_slots;
    hipStream_t g_stream;
    // Pipelined form of the step (orn_engine_train_steps; 16-bit engines with >= 2 blocks on the fast path): the LAST block's
    // weight gradient, slab reduction, merge backward, Adam update and next merge forward run on a second stream (`side`),
    // forked off the caller's stream inside the backward (fork_behind_dgrad, below) and joined in front of the
    // last block's forward conv of the NEXT step.  That chain -- one full-chip MFMA launch and a tail of small ones -- then runs beside the latency-bound
    // launches of the step boundary (merge backward / Adam / merge forward of the lower blocks, stem, first blocks) instead of
    // in front of them.  Same arithmetic as the serial step (bit-identical results); what it needs:
    //   ev_fork   main -> side: dy / x of the last block, the head's partials and the step's copied schedule state are final
    //   ev_adam   main -> side: the step's skip decision has been taken (the side's Adam launch follows it)
    //   ev_wgrad  side -> main: the last block's input buffer may be overwritten (by the forward conv of the block below it)
    //   ev_below  side -> main: the weight gradient of the block BELOW the last one, which the side stream computes first (beside that
    //                           block's own dgrad launch on the caller's stream: 230 work-groups on 512 slots at 720p, and a wgrad
    //                           of 216), is complete: its slabs may be reduced, its input buffer overwritten
    //   ev_join   side -> main: the last block's merged kernel (and the head's parameters) of the next step are ready
    // cur_side / sc_side: this step's schedule entry and loss scale, copied by the loss's finalize stage (the main stream advances
    // to the next step while the side branch still reads them); sc_side->mirrored holds the caller's-stream Adam's skip decision,
    // sc_side->flag what the side branch's own detectors raise, two of them behind that decision (include/orn.h, the loss-scale
    // comment): the side branch's Adam launch skips on either and counts a skip of the flag alone in sc[0].late_skipped.
    hipStream_t side;
    hipEvent_t ev_fork, ev_adam, ev_wgrad, ev_join, ev_below;
    OrnStepCur *cur_side;
    OrnScaleState *sc_side;
    size_t side_lo;                  // parameters [side_lo, n_params) belong to the side branch's Adam launch (last block + head)
    bool pipe_ok;                    // this engine can run the pipelined form
    // The shape of the pipelined step, decided once in orn_engine_create (the measurements behind each choice are there)
    bool side_below;                 // the side branch also takes the weight gradient of the block BELOW the last one (ahead of the last block's)
    bool fork_behind_dgrad;          // the side branch forks behind the last block's dgrad; else behind the lower blocks' slab reduction
    int last_smax;                   // split-K slab cap of the last block's weight gradient, in every form of the step (0: the default rule)
    bool side_busy;                  // a side branch is in flight (joined by the next step's forward or at the end of the call)
    // Batched step (orn_engine_train_steps_batch): the directly written gradient slots as ranges of the arena (built at creation),
    // and the caller's batch workspace (orn_engine_set_batch_ws; null: none): accumulation arena, the frame table of the step in
    // flight (one schedule state per frame, filled by k_advance_batch; slot = the frame's place in the batch) and the per-frame
    // stats the loss's finalize stage writes through that slot
    OrnAccumTable acc_tab;
    float *b_acc;
    OrnStepCur *b_cur;
    float *b_stats;
    int b_max;
    // Split step (orn_engine_step_forward / orn_engine_step_backward): the forward half has run on open_st and its activations wait
    // for the backward half; every other entry that would overwrite them is refused meanwhile (ORN_E_STATE)
    bool open;
    hipStream_t open_st;
    // Multi-resolution heads (d.multi_res; include/orn.h, N8): what stage i < n_layers - 1 keeps -- its image, dLoss_i/dout_i, the
    // loss's stats and workspace, the head backward's partials (workspace carve), and the caller's target tables
    struct SideStage {
        int C, H, W;                 // the stage's output: channels of block i's output, image size
        float *img, *dimg, *stats, *loss_ws, *head_ws;
        const float *targets, *tstats;
    } stage[ORN_MAX_LAYERS];
    float *stage_ring;               // optional [stage_slots][n_layers][2] = {loss_i, psnr_i} (orn_engine_set_stage_stats)
    int stage_slots;
    OrnAccumTable side_tab;          // batched step: the side heads' gradient slots (a second accumulate launch)
    // orn_engine_profile_step: HIP events around every forward conv launch of an eager step
    bool prof;
    hipEvent_t prof_ev[4 * ORN_MAX_LAYERS + 4];      // pairs: forward conv of layer i, dgrad launch of layer i, wgrad batch, its reduction
};

#define ORN_GRAPH_UNROLL 4
static_assert(ORN_SCALE_SLOTS >= ORN_GRAPH_UNROLL, "one scale-state entry per step of the unrolled graph");
#define ORN_FAST_C 96          // input channels per pixel of every 16-bit channels-last buffer

// While a split step is open the engine's activations belong to its backward: every other stepping, decoding and evaluation
// entry is refused until orn_engine_step_backward has closed it.
#define ORN_REQUIRE_CLOSED(e, name)                                                                                               \
    do {                                                                                                                          \
        if ((e)->open) {                                                                                                          \
            orn_set_error("%s: a split step is open (orn_engine_step_forward); orn_engine_step_backward closes it", name);       \
            return ORN_E_STATE;                                                                                                   \
        }                                                                                                                         \
    } while (0)

static inline size_t al(size_t floats) { return orn_align(floats * 4) / 4; }

// fp32 engine: the last block's backward starts from the head's (out, dout) and reads z (k_head_bwd_fused_f32), so its training
// forward needs no stored activation either
static inline bool f32_head_on_z(const orn_engine *e)
{
    const orn_engine_desc &d = e->d;
    return e->ff >= d.n_layers && e->head_ws && d.layer[d.n_layers - 1].s == 2;
}

// The per-layer descriptors of the fast path's batched launches.  The slab cap of a layer's weight gradient comes from slab_cap()
// alone, so a wgrad job and the reduction of its slabs cannot disagree (a mismatch would be a silent change of the summation order).
static inline int slab_cap(const orn_engine *e, int i) { return i == e->d.n_layers - 1 ? e->last_smax : 0; }

static inline OrnPrepLayer prep_layer(const orn_engine *e, int i)
{
    const orn_layer_desc &l = e->d.layer[i];
    return OrnPrepLayer{e->L[i].wf, e->L[i].bf, l.O, l.C, l.s, e->L[i].wb, e->L[i].wd, e->L[i].biasp, ORN_FAST_C};
}

static inline OrnWgradJob wgrad_job(const orn_engine *e, int i)
{
    const orn_layer_desc &l = e->d.layer[i];
    return OrnWgradJob{e->L[i].xpad, e->L[i].dypad, l.H, l.W, l.C, l.O, l.s, e->L[i].wslab, slab_cap(e, i)};
}

static inline OrnWgradReduce wgrad_reduce(const orn_engine *e, int i, OrnScaleState *sc)
{
    const orn_layer_desc &l = e->d.layer[i];
    return OrnWgradReduce{e->L[i].wslab, l.H, l.W, l.C, l.O, l.s, 1.0f / e->gs, e->grads + l.w3x3, e->grads + l.b3x3, sc, slab_cap(e, i)};
}

struct StepOpts {
    int advance = 1;        // advance the device-side schedule by this many steps first (states e->cur[0 .. advance)); 0: not at all
    int cur = 0;            // the step itself runs on e->cur[cur]
    bool pipe = false;      // the pipelined form (struct orn_engine, `side`): the last block's weight-gradient chain leaves this step on the side stream
    bool more = false;      // (pipelined form) another step follows in this call
    // batched step (orn_engine_train_steps_batch; with advance = 0, the batched advance has run): this call is frame `bframe` of an
    // optimiser step of `batch` frames.  It reads its frame from the frame table, leaves its stats there, and ends in the accumulate
    // launch; frames 1.. skip the merge forward; the last frame goes on to the one merge backward, the ring record and Adam.
    int batch = 0, bframe = 0;
};
static inline OrnStepCur *step_cur(const orn_engine *e, const StepOpts &o) { return o.batch > 0 ? e->b_cur + o.bframe : e->cur + o.cur; }

// ---- what crosses the engine's files (C++ linkage: none of it reaches the dynamic symbol table) ----
// orn_engine.hip.  StageGeo: (C, H, W) of every stage's output -- block i's channels and image size -- of a descriptor that check_desc
// has passed; of one it has not, the stages below the first layer with a bad stride are right (all that check_desc reads).
struct StageGeo { int C[ORN_MAX_LAYERS], H[ORN_MAX_LAYERS], W[ORN_MAX_LAYERS]; };
StageGeo stage_geometry(const orn_engine_desc *d);
int check_desc(const orn_engine_desc *d);
void drop_graphs(orn_engine *e);      // the graph cache is dropped whenever what a captured step does (or is given) changes
// orn_engine_forward.hip
// set: which layers this forward merges (0 all; 1: all but the last block, whose merged kernel the side branch of the previous
// pipelined step leaves behind -- the forward then waits for that branch where it touches the last block's buffers;
// MERGE_NONE: nothing -- the parameters have not changed since the previous forward (frames 1.. of orn_engine_decode_frames), so
// every wf / bf / wb / biasp is used as that forward left it: no W2 transpose, no merge launch, no operand copies, no riders)
// head: false leaves the A5 head of a 16-bit engine to the caller (the decode output kernel reads the last block's z)
// side_sc (training forward of a multi-resolution engine): the step's scale-state entry -- behind every block below the last, its
// stage's head and loss run (side_forward)
enum { MERGE_NONE = -1 };
// top: the last block that runs (n_layers - 1: the whole forward).  Below that (orn_engine_eval_stages) the forward ends behind block
// `top`'s conv, which fills no input buffer for the block above it; neither those blocks nor the last head are launched.
int forward(orn_engine *e, const float *embeds, const int *row_idx, bool keep_z, hipStream_t st, int top, int set = 0, bool head = true,
            OrnScaleState *side_sc = nullptr);
