// Test and probe entry points (include/orn_debug.h) of the code that lives in the twice-built files of the 16-bit fast path and in
// the two fp32 files beside them (orn_side_head_f32.hip, orn_decode_out_f32.hip).  No element type is named here and the file is built
// once: every body is written once against the type-erased table the engine calls through (OrnHalfOps, orn_internal.h) and exported
// under its bf16 / f16 names, with and without the trailing activation, by one-line forwards.  A body checks "unknown activation"
// first and everything else before its first launch or allocation.  Entries that sit beside file-static kernels and argument
// builders of once-built files (stage0, stem, act_eval, head_fwd_z, conv_f32_*, msssim / loss, the 16-bit merge backward) stay there.
#include "orn_internal.h"

// The four exported names of one body debug_<name>(ops, <params>, act): params_ / args_ are its parameter and argument lists in parentheses.
#define LIST(...) __VA_ARGS__
#define TWINS(name_, params_, args_)                                                                                                        \
    extern "C" int orn_debug_##name_##_bf16_act(LIST params_, int act) { return debug_##name_(orn_half_ops_bf16(), LIST args_, act); }      \
    extern "C" int orn_debug_##name_##_f16_act(LIST params_, int act) { return debug_##name_(orn_half_ops_f16(), LIST args_, act); }        \
    extern "C" int orn_debug_##name_##_bf16(LIST params_) { return debug_##name_(orn_half_ops_bf16(), LIST args_, ORN_ACT_SWISH); }         \
    extern "C" int orn_debug_##name_##_f16(LIST params_) { return debug_##name_(orn_half_ops_f16(), LIST args_, ORN_ACT_SWISH); }

// The engine's form of a scale: a state entry on the device, of the entry point's own.  own_scale_create fills one with gs;
// own_scale_finish synchronises the stream, hands its flag word out (where everything went well) and frees it.
static int own_scale_create(const char *who, float gs, OrnScaleState *&sc)
{
    OrnScaleState s0 = {};
    s0.gs = s0.gs_max = gs;
    s0.inv_gs = 1.0f / gs;
    ORN_HIP(hipMalloc(&sc, sizeof(s0)));
    const hipError_t e = hipMemcpy(sc, &s0, sizeof(s0), hipMemcpyHostToDevice);
    if (e != hipSuccess) { orn_set_error("%s: %s", who, hipGetErrorString(e)); (void)hipFree(sc); return (int)e; }
    return 0;
}
static int own_scale_finish(const char *who, OrnScaleState *sc, hipStream_t st, int rc, int *flag)
{
    OrnScaleState s0 = {};
    hipError_t e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(&s0, sc, sizeof(s0), hipMemcpyDeviceToHost);
    if (rc == 0 && e != hipSuccess) { orn_set_error("%s: %s", who, hipGetErrorString(e)); rc = (int)e; }
    if (rc == 0) *flag = s0.flag;
    (void)hipFree(sc);
    return rc;
}

// Timing-only ablation flags and the stamp buffer of the conv / wgrad kernels: probe-only switches that reach both builds.
namespace orn_bf16 { void set_debug(int flags); void set_stamps(void *buf); }
namespace orn_f16 { void set_debug(int flags); void set_stamps(void *buf); }
extern "C" void orn_debug_set(int flags) { orn_bf16::set_debug(flags); orn_f16::set_debug(flags); }
#ifdef ORN_CONV_STAMP
extern "C" void orn_debug_set_stamps(void *buf) { orn_bf16::set_stamps(buf); orn_f16::set_stamps(buf); }
#endif

// ---- the two conv launchers with the engine's full argument lists, so that a test reaches every kernel form they select (the narrow
// c_real forms, the split dgrad + finish, the fp32 hand-off) with the engine's buffers ----
static int debug_conv_fwd(const OrnHalfOps *ops, const void *xpad, const void *wb, const float *bias_p, int H, int W, int Cin, int O, int s,
                          void *z, void *apad, int c_real, void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "debug_conv_fwd: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    return ops->conv_fwd(xpad, wb, bias_p, H, W, Cin, O, s, z, apad, (hipStream_t)stream, c_real, act);
}
TWINS(conv_fwd, (const void *xpad, const void *wb, const float *bias_p, int H, int W, int Cin, int O, int s, void *z, void *apad, int c_real,
                 void *stream),
      (xpad, wb, bias_p, H, W, Cin, O, s, z, apad, c_real, stream))

static int debug_conv_dgrad(const OrnHalfOps *ops, const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev,
                            void *dyprev, int sp, float *dx_f32, int c_real, void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "debug_conv_dgrad: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    return ops->conv_dgrad(dypad, wd, H, W, O, C, zprev, dyprev, sp, dx_f32, (hipStream_t)stream, c_real, act);
}
TWINS(conv_dgrad, (const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev, void *dyprev, int sp, float *dx_f32,
                   int c_real, void *stream),
      (dypad, wd, H, W, O, C, zprev, dyprev, sp, dx_f32, c_real, stream))

// ---- the last stage's head: its launchers and the two forms of the dW / db finish, as the per-op path and the engine call them.  The
// sizes are the launchers' own functions (they do not depend on the element type) ----
extern "C" int orn_debug_head16_bwd_blocks(int H, int W) { return (H >= 1 && W >= 1) ? orn_half_ops_bf16()->head_bwd_blocks(H, W) : 0; }
extern "C" size_t orn_debug_head16_bwd_ws_bytes(int C)
{
    return orn_head_bwd_c_ok(C) ? orn_half_ops_bf16()->head_bwd_ws_floats(C) * sizeof(float) : 0;
}
extern "C" size_t orn_debug_head16_bwd_rider_ws_bytes(int C, int H, int W, int loss_type)
{
    const size_t head = orn_debug_head16_bwd_ws_bytes(C), loss = orn_loss_ws_bytes_for(loss_type, 1, 3, H, W);
    return head && loss ? orn_align(head) + loss : 0;
}

static int debug_head_fwd(const OrnHalfOps *ops, const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                          void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "head_fwd: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    ORN_REQUIRE(z && w && b && out, "head_fwd: null pointer");
    ORN_REQUIRE(C >= 32 && H >= 1 && W >= 1, "head_fwd: bad sizes C=%d %dx%d", C, H, W);
    return ops->head_fwd(z, w, b, C, (size_t)H * W, sigmoid, out, (hipStream_t)stream, act);
}
TWINS(head_fwd, (const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out, void *stream),
      (z, w, b, C, H, W, sigmoid, out, stream))

static int debug_head_bwd(const OrnHalfOps *ops, const void *z, const float *w, const float *out, float *dout, int C, int H, int W, int sigmoid,
                          int sp, float gs, void *dypad, float *dw, float *db, void *ws, size_t ws_bytes, int *flag, const float *target,
                          int loss_type, float *stats, void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "head_bwd: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    ORN_REQUIRE(z && w && out && dout && dypad && dw && db && ws && (!target || stats), "head_bwd: null pointer");
    const size_t head_bytes = orn_debug_head16_bwd_ws_bytes(C);
    ORN_REQUIRE(head_bytes, "head_bwd: unsupported C=%d", C);
    ORN_REQUIRE(H >= 1 && W >= 1 && sp >= 1 && H % sp == 0 && W % sp == 0, "head_bwd: %dx%d not divisible by the stride %d", H, W, sp);
    ORN_REQUIRE(gs > 0.f, "head_bwd: gradient scale %g", (double)gs);
    const size_t need = target ? orn_debug_head16_bwd_rider_ws_bytes(C, H, W, loss_type) : head_bytes;
    ORN_REQUIRE(need, "head_bwd: loss_type %d does not take a %dx%d image", loss_type, H, W);
    ORN_REQUIRE(!target || (uintptr_t)ws % 16 == 0, "head_bwd: the rider needs a 16-byte aligned workspace");
    if (ws_bytes < need) { orn_set_error("head_bwd: workspace %zu < %zu", ws_bytes, need); return ORN_E_WS; }
    hipStream_t st = (hipStream_t)stream;
    OrnScaleState *sc = nullptr;
    if (flag) ORN_TRY(own_scale_create("head_bwd", gs, sc));      // the engine's form: the scale lives in a state entry on the device
    int rc = 0;
    OrnLossFinalJob fj = {};
    if (target)                                         // the loss writes dout and leaves its finalize stage to the head backward
        rc = orn_launch_loss(out, target, nullptr, 0, 1, 3, H, W, loss_type, gs, stats, dout, (float *)((char *)ws + orn_align(head_bytes)), st,
                             nullptr, nullptr, sc, nullptr, &fj);
    if (rc == 0)
        rc = ops->head_bwd(z, w, out, dout, C, H, W, sigmoid, sp, gs, dypad, flag ? nullptr : dw, flag ? nullptr : db, (float *)ws, st, sc,
                           target ? &fj : nullptr, act);
    if (rc == 0 && flag) {
        const OrnHeadFinish hf = {(const float *)ws, ops->head_bwd_blocks(H, W), C, 1.0f / gs, dw, db, sc};
        rc = ops->wgrad_batch(0, nullptr, st, &hf, nullptr, 0, act);     // (no stem job on it: nothing evaluates the activation)
    }
    return flag ? own_scale_finish("head_bwd", sc, st, rc, flag) : rc;
}
TWINS(head_bwd, (const void *z, const float *w, const float *out, float *dout, int C, int H, int W, int sigmoid, int sp, float gs, void *dypad,
                 float *dw, float *db, void *ws, size_t ws_bytes, int *flag, const float *target, int loss_type, float *stats, void *stream),
      (z, w, out, dout, C, H, W, sigmoid, sp, gs, dypad, dw, db, ws, ws_bytes, flag, target, loss_type, stats, stream))

// ---- the two weight-gradient launches of a step through the table members the engine calls, in the order and with the argument structs
// of fast_weight_grads / side_branch_backward (orn_engine_step.hip); the slab rule's two host functions ----
extern "C" int orn_debug_wgrad16_split(int H, int W, int O, int smax) { return orn_half_ops_bf16()->wgrad_split(H, W, O, smax); }
extern "C" size_t orn_debug_wgrad16_ws_floats(int H, int W, int O) { return orn_half_ops_bf16()->wgrad_ws_floats(H, W, O); }

static int debug_wgrad16_step(const OrnHalfOps *ops, int n, const orn_debug_wgrad16_job *jobs, const orn_debug_wgrad16_head *head,
                              const orn_debug_wgrad16_stem *stem, float gs, int use_state, int side, int act, int *flag, void *stream)
{
    ORN_REQUIRE(orn_act_known(act), "debug_wgrad16_step: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    ORN_REQUIRE(n >= 0 && n <= ORN_MAX_LAYERS, "debug_wgrad16_step: %d jobs (0..%d)", n, ORN_MAX_LAYERS);
    ORN_REQUIRE((n == 0 || jobs) && (!use_state || flag), "debug_wgrad16_step: null pointer");
    ORN_REQUIRE(gs > 0.f, "debug_wgrad16_step: gradient scale %g", (double)gs);
    for (int i = 0; i < n; ++i) {
        const orn_debug_wgrad16_job &j = jobs[i];
        ORN_REQUIRE(j.xpad && j.dypad && j.slabs && j.dwf && j.dbf, "debug_wgrad16_step: null pointer in job %d", i);
        ORN_REQUIRE(j.H >= 1 && j.W >= 1 && j.s >= 1, "debug_wgrad16_step: job %d: bad sizes %dx%d s=%d", i, j.H, j.W, j.s);
        ORN_REQUIRE(j.C >= 1 && j.C <= 96 && j.O >= 32 && j.O % 32 == 0 && j.O % (j.s * j.s) == 0, "wgrad_bf16: unsupported C=%d O=%d", j.C, j.O);
    }
    if (head) {
        ORN_REQUIRE(head->partial && head->dw && head->db, "debug_wgrad16_step: null pointer in the head finish");
        ORN_REQUIRE(head->blocks >= 1 && head->C >= 1, "debug_wgrad16_step: head finish of %d blocks, C=%d", head->blocks, head->C);
    }
    if (stem) {
        const orn_debug_wgrad16_stem &t = *stem;
        ORN_REQUIRE(t.embed && t.w1 && t.pre1 && t.h1 && t.pre2 && t.dh2_slabs && t.dw0 && t.db0 && t.dw1 && t.db1 && t.ws,
                    "debug_wgrad16_step: null pointer in the stem job");
        ORN_REQUIRE(t.nslab >= 1 && t.E > 0 && t.Hd > 0 && t.Nout > 0, "debug_wgrad16_step: bad stem sizes");
        if (t.ws_bytes < orn_stem_bwd_ws_bytes(1, t.Hd, t.Nout) || (uintptr_t)t.ws % 4 != 0) {
            orn_set_error("debug_wgrad16_step: stem workspace of %zu bytes, needs orn_stem_bwd_ws_bytes = %zu, 4-byte aligned", t.ws_bytes,
                          orn_stem_bwd_ws_bytes(1, t.Hd, t.Nout));
            return ORN_E_WS;
        }
    }
    hipStream_t st = (hipStream_t)stream;
    OrnScaleState *sc = nullptr;
    if (use_state) ORN_TRY(own_scale_create("debug_wgrad16_step", gs, sc));      // the engine's form: the scale lives in a state entry on the device
    int rc = 0;
    OrnStemW0Job w0job;
    OrnStemL2Job l2job;
    if (stem)                                           // deferred: both kernels come back as jobs, nothing is launched here
        rc = orn_launch_stem_bwd(stem->embed, nullptr, 0, stem->w1, stem->pre1, stem->h1, stem->pre2, stem->dh2_slabs, 1, stem->E, stem->Hd,
                                 stem->Nout, stem->dw0, stem->db0, stem->dw1, stem->db1, stem->ws, st, stem->nslab, &w0job, &l2job, act, sc);
    OrnWgradJob wj[ORN_MAX_LAYERS];
    OrnWgradReduce wr[ORN_MAX_LAYERS];
    for (int i = 0; i < n; ++i) {
        const orn_debug_wgrad16_job &j = jobs[i];
        wj[i] = OrnWgradJob{j.xpad, j.dypad, j.H, j.W, j.C, j.O, j.s, j.slabs, j.smax};
        wr[i] = OrnWgradReduce{j.slabs, j.H, j.W, j.C, j.O, j.s, 1.0f / gs, j.dwf, j.dbf, sc, j.smax};
    }
    OrnHeadFinish hf = {};
    if (head) hf = OrnHeadFinish{head->partial, head->blocks, head->C, 1.0f / gs, head->dw, head->db, sc};
    if (rc == 0) rc = ops->wgrad_batch(n, wj, st, head ? &hf : nullptr, stem ? &l2job : nullptr, side ? 1 : 0, act);
    if (rc == 0) rc = ops->wgrad_reduce_all(n, wr, st, stem ? &w0job : nullptr, act);
    return use_state ? own_scale_finish("debug_wgrad16_step", sc, st, rc, flag) : rc;
}
extern "C" int orn_debug_wgrad16_step_bf16(int n, const orn_debug_wgrad16_job *jobs, const orn_debug_wgrad16_head *head,
                                           const orn_debug_wgrad16_stem *stem, float gs, int use_state, int side, int act, int *flag, void *stream)
{
    return debug_wgrad16_step(orn_half_ops_bf16(), n, jobs, head, stem, gs, use_state, side, act, flag, stream);
}
extern "C" int orn_debug_wgrad16_step_f16(int n, const orn_debug_wgrad16_job *jobs, const orn_debug_wgrad16_head *head,
                                          const orn_debug_wgrad16_stem *stem, float gs, int use_state, int side, int act, int *flag, void *stream)
{
    return debug_wgrad16_step(orn_half_ops_f16(), n, jobs, head, stem, gs, use_state, side, act, flag, stream);
}

// ---- the side heads (orn_side_head.hip, orn_side_head_f32.hip) ----
extern "C" size_t orn_debug_side_head_bwd_ws_bytes(int C, int H, int W) { return orn_side_head_bwd_ws_floats(C, H, W) * sizeof(float); }

static int debug_side_head_fwd(const OrnHalfOps *ops, const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                               void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "side_head_fwd: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    ORN_REQUIRE(z && w && b && out && H >= 1 && W >= 1, "side_head_fwd: bad arguments");
    return ops->side_head_fwd(z, w, b, C, (size_t)H * W, sigmoid, out, (hipStream_t)stream, nullptr, act);
}
TWINS(side_head_fwd, (const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out, void *stream),
      (z, w, b, C, H, W, sigmoid, out, stream))

static int debug_side_head_bwd(const OrnHalfOps *ops, const void *z, const float *w, const float *out, const float *dout, int C, int H, int W,
                               int sigmoid, int sp, float lw, float gs, void *dypad, float *dw, float *db, void *ws, size_t ws_bytes,
                               void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "side_head_bwd: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    ORN_REQUIRE(z && w && out && dout && dypad && dw && db && ws, "side_head_bwd: null pointer");
    const size_t need = orn_debug_side_head_bwd_ws_bytes(C, H, W);
    ORN_REQUIRE(need, "side_head_bwd: bad sizes C=%d %dx%d", C, H, W);
    if (ws_bytes < need) { orn_set_error("side_head_bwd: workspace %zu < %zu", ws_bytes, need); return ORN_E_WS; }
    return ops->side_head_bwd(z, w, out, dout, C, H, W, sigmoid, sp, lw, gs, dypad, dw, db, (float *)ws, (hipStream_t)stream, nullptr, act);
}
TWINS(side_head_bwd, (const void *z, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid, int sp, float lw,
                      float gs, void *dypad, float *dw, float *db, void *ws, size_t ws_bytes, void *stream),
      (z, w, out, dout, C, H, W, sigmoid, sp, lw, gs, dypad, dw, db, ws, ws_bytes, stream))

extern "C" int orn_debug_side_head_fwd_f32(const float *a, const float *w, const float *b, int C, int H, int W, int sigmoid, float *out,
                                           void *stream)
{
    ORN_REQUIRE(a && w && b && out && H >= 1 && W >= 1, "side_head_fwd_f32: bad arguments");
    return orn_launch_side_head_fwd_f32(a, w, b, C, (size_t)H * W, sigmoid, out, (hipStream_t)stream, nullptr);
}
extern "C" int orn_debug_side_head_bwd_f32(const float *a, const float *w, const float *out, const float *dout, int C, int H, int W,
                                           int sigmoid, float lw, float *da, float *dw, float *db, void *ws, size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(a && w && out && dout && da && dw && db && ws, "side_head_bwd_f32: null pointer");
    const size_t need = orn_debug_side_head_bwd_ws_bytes(C, H, W);
    ORN_REQUIRE(need, "side_head_bwd_f32: bad sizes C=%d %dx%d", C, H, W);
    if (ws_bytes < need) { orn_set_error("side_head_bwd_f32: workspace %zu < %zu", ws_bytes, need); return ORN_E_WS; }
    return orn_launch_side_head_bwd_f32(a, w, out, dout, C, H, W, sigmoid, lw, da, dw, db, (float *)ws, (hipStream_t)stream, nullptr);
}

// ---- the decode output stage on a caller's image (fp32 engines: the planar kernel) or a caller's z (a side stage's output kernel).
// Every argument is checked before anything is enqueued ----
extern "C" size_t orn_debug_decode_out_ws_bytes(void) { return (size_t)ORN_DECODE_WS_FLOATS * 4; }

// with stats: the row index (0: `target` is the one frame) lives in the workspace, behind the ticket
static int debug_decode_ws(OrnDecodeOut &o, hipStream_t st)
{
    if (!o.stats) return 0;
    ORN_HIP(hipMemsetAsync(o.ws + 2 * ORN_DECODE_MAX_BLOCKS, 0, 64 * 4, st));
    o.row = reinterpret_cast<const int32_t *>(o.ws + 2 * ORN_DECODE_MAX_BLOCKS + 1);
    return 0;
}

extern "C" int orn_debug_decode_out_f32(const float *img, int H, int W, const float *target, uint8_t *rgb8, float *img_out, float *stats,
                                        void *ws, size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(img && H > 0 && W > 0 && (rgb8 || img_out || stats), "debug_decode_out_f32: bad arguments");
    ORN_REQUIRE(!stats || (target && ws && ws_bytes >= orn_debug_decode_out_ws_bytes() && (uintptr_t)ws % 4 == 0),
                "debug_decode_out_f32: stats need a target and a workspace of orn_debug_decode_out_ws_bytes");
    hipStream_t st = (hipStream_t)stream;
    OrnDecodeOut o = {target, nullptr, rgb8, img_out, stats, (float *)ws};
    ORN_TRY(debug_decode_ws(o, st));
    return orn_launch_decode_out_f32(img, (size_t)H * W, o, st);
}

static int debug_stage_out(const OrnHalfOps *ops, const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid,
                           const float *target, uint8_t *rgb8, float *img, float *stats, void *ws, size_t ws_bytes, void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "debug_stage_out: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    ORN_REQUIRE(z && w && b && H > 0 && W > 0 && (rgb8 || img || stats), "debug_stage_out: bad arguments");
    ORN_REQUIRE(C >= 1 && C <= STAGE_OUT_MAXC, "debug_stage_out: C=%d outside [1, %d]", C, STAGE_OUT_MAXC);
    ORN_REQUIRE((size_t)H * W <= ((size_t)1 << 30), "debug_stage_out: bad image size %dx%d", H, W);
    ORN_REQUIRE(!stats || (target && ws && ws_bytes >= orn_debug_decode_out_ws_bytes() && (uintptr_t)ws % 4 == 0),
                "debug_stage_out: stats need a target and a workspace of orn_debug_decode_out_ws_bytes");
    hipStream_t st = (hipStream_t)stream;
    OrnDecodeOut o = {target, nullptr, rgb8, img, stats, (float *)ws};
    ORN_TRY(debug_decode_ws(o, st));
    return ops->stage_out(z, w, b, C, (size_t)H * W, sigmoid, o, st, act);
}
TWINS(stage_out, (const void *z, const float *w, const float *b, int C, int H, int W, int sigmoid, const float *target, uint8_t *rgb8, float *img,
                  float *stats, void *ws, size_t ws_bytes, void *stream),
      (z, w, b, C, H, W, sigmoid, target, rgb8, img, stats, ws, ws_bytes, stream))
