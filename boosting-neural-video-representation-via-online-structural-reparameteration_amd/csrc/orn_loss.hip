// A7 + A10  loss_fn (utils.py:139-189) fused with its gradient and with psnr_fn (utils.py:191-199), and N3 msssim_fn.  Every loss id
// resolves through orn_loss_spec_of to w_l1 * L1 + w_l2 * MSE + w_struct * (1 - s); one 16x64 tiling of the image for all kinds:
//   k_fusion6   : s = ssim, one pass per tile through the tile machine of orn_ssim_tile.h: SSIM map, its derivative maps, their adjoint
//                 filter, the pixel term -> dL/dpred and the tile partials {ssim}, {|d|, d^2}.  TC_FILL makes the target's own
//                 filtered maps once per video, TC_READ reads them in the step
//   k_loss_grad : no structural term (L1, L2, Fusion7 / 8);  k_loss_ext: the split step, whose loss and gradient the caller computed
//   k_msssim_level, k_msssim_frames_finalize: MS-SSIM, as a metric and as the forward of the MS-SSIM losses (orn_loss_msssim.hip)
// each followed by a fixed-order finalize.  SSIM and MS-SSIM follow pytorch_msssim 0.2.1's published algorithm (the package is not in
// the reference tree: parity unpinned, see oracle/cpu_ref.py).
#include "orn_ssim_tile.h"

#define SS_TH 16             // k_loss_grad, k_loss_ext and k_msssim_level (k_fusion6 too: the static_assert in orn_launch_loss)
#define SS_TW 64
#define SS_PH (SS_TH + 10)
#define SS_PW (SS_TW + 10)
#define SS_PWP 76            // padded row stride (floats): 16-byte aligned rows for float4 LDS reads

struct LossP {
    const float *pred, *target;
    const int *frame_idx;      // optional device index selecting the target frame
    size_t frame_stride;
    int planes, H, W, Hv, Wv;  // planes = B*Ch
    float *part_ssim;          // [n_blocks]
    float *part_l1;            // [n_blocks][2]
    float *dpred;              // may be null
    int loss_type;
    int vec4;                  // orn_loss_vec4: the fused Fusion6 kernel loads float4
    // Fusion6, optional: the TARGET's own filtered maps G*t and G*t^2 on the valid map, [frame][2][planes][Hv][Wv], computed
    // once per video by k_fusion6<.., TC_FILL> with the arithmetic of the in-kernel form (same taps, same fmaf order: the
    // step's results do not change by a bit).  The target never changes during a fit, and 288 GB of HBM hold 2.9 GB of
    // them for a 132-frame 720p video: the step then filters three maps (p, p^2, pt) instead of five.
    float *tstats;
    size_t tstats_stride;      // floats per frame
    float g_l1, g_l2, g_ssim;  // gradient scales (already include loss_scale and 1/n)
    int tiles_w, tiles_h;
};

// Fusion6 in ONE pass per image tile (round 3; rounds 1-2 ran k_ssim_stats + k_loss_grad with the three dS maps making a round trip
// through HBM): the tile machine of orn_ssim_tile.h with the SSIM map.  HBM traffic: p, t read (aprons from L2), dL/dpred written.
enum { TC_NONE = 0, TC_READ = 1, TC_FILL = 2 };
// L2T: the pixel term of the gradient is g_l2 * d (Fusion1 / 3 / 5: MSE + SSIM) instead of g_l1 * sign(d)
template <bool GRAD, int TC, bool L2T = false>
__global__ void __launch_bounds__(256) k_fusion6(LossP q)
{
    extern __shared__ __attribute__((aligned(16))) float f6s[];
    float *Xp = f6s, *Xt = f6s + ST_PH * ST_PWP;
    float *Hm = f6s + 2 * ST_PH * ST_PWP;
    float *Dm = f6s;                       // written after the last read of Xp / Xt
    float *Hh = Hm;                        // written after the last read of Hm
    float *sred = f6s + 2 * ST_PH * ST_PWP + 5 * ST_PH * ST_DWP;
    const int t = threadIdx.x;
    const int plane = blockIdx.y;
    const int tw = blockIdx.x % q.tiles_w, th = blockIdx.x / q.tiles_w;
    const int y0 = th * ST_TH, x0 = tw * ST_TW;
    const size_t HW = (size_t)q.H * q.W;
    const size_t fr = TC == TC_FILL ? (size_t)blockIdx.z : (q.frame_idx ? (size_t)(*q.frame_idx) : 0);
    const float *tp = q.target + fr * q.frame_stride + (size_t)plane * HW;
    const float *pp = TC == TC_FILL ? tp : q.pred + (size_t)plane * HW;       // (TC_FILL: only the target's two maps are formed)
    float *ts_mu = nullptr, *ts_tt = nullptr;
    if (TC != TC_NONE) {
        ts_mu = q.tstats + fr * q.tstats_stride + (size_t)plane * q.Hv * q.Wv;
        ts_tt = ts_mu + (size_t)q.planes * q.Hv * q.Wv;
    }
    // the cached target statistics of this thread's nine map positions (column filter mapping below) are requested first: two
    // barriers lie between here and their use.  (Loaded where they are used, they cost more than the two filters they save:
    // with two work-groups per CU nothing covers a round trip to HBM in the middle of a phase.)
    constexpr bool P_MAPS = TC != TC_FILL, T_MAPS = TC != TC_READ;       // which of the five maps this mode forms
    const int vrg = t / ST_DWP, vj = t - vrg * ST_DWP, vr4 = vrg == 2 ? 17 : vrg * ST_RPT;
    float c_mu[ST_RPT], c_tt[ST_RPT];
    if (TC == TC_READ && t < 3 * ST_DWP) {
#pragma unroll
        for (int o = 0; o < ST_RPT; ++o) {
            const int vy = min(max(y0 - 10 + vr4 + o, 0), q.Hv - 1), vx = min(max(x0 - 10 + vj, 0), q.Wv - 1);
            c_mu[o] = ts_mu[(size_t)vy * q.Wv + vx];
            c_tt[o] = ts_tt[(size_t)vy * q.Wv + vx];
        }
    }
    st_load_patch(Xp, Xt, pp, tp, y0, x0, q.H, q.W, q.vec4, t);
    __syncthreads();
    st_row_filter<P_MAPS, T_MAPS>(Xp, Xt, Hm, t);
    __syncthreads();
    // ---- column filter + SSIM map + dS maps; item = (column j, 9 rows from r4) as for the prefetch above
    float ssum = 0.f;
    if (t < 3 * ST_DWP) {
        const int rg = vrg, j = vj, r4 = vr4;
        float v[5][ST_RPT];
#pragma unroll
        for (int m = 0; m < 5; ++m)
            if ((m == 1 || m == 3) ? T_MAPS : P_MAPS) st_col_filter(Hm, m, r4, j, v[m]);
#pragma unroll
        for (int o = 0; o < ST_RPT; ++o) {
            const int i = r4 + o;
            const int vy = y0 - 10 + i, vx = x0 - 10 + j;
            float dm = 0.f, dq = 0.f, dr = 0.f;
            if (TC == TC_FILL) {                        // the owned part of the two target maps, once
                if (vy >= 0 && vy < q.Hv && vx >= 0 && vx < q.Wv && i >= 10 && j >= 10 && j < ST_TW + 10 && (rg < 2 || o > 0)) {
                    ts_mu[(size_t)vy * q.Wv + vx] = v[1][o];
                    ts_tt[(size_t)vy * q.Wv + vx] = v[3][o];
                }
                continue;
            }
            if (vy >= 0 && vy < q.Hv && vx >= 0 && vx < q.Wv && j < ST_TW + 10) {
                const float S = st_deriv<true>(v[0][o], TC == TC_READ ? c_mu[o] : v[1][o], v[2][o], TC == TC_READ ? c_tt[o] : v[3][o], v[4][o], dm, dq, dr);
                if (i >= 10 && j >= 10 && (rg < 2 || o > 0)) ssum += S;      // this tile's own part of the map, once
            }
            st_store_deriv(Dm, i, j, dm, dq, dr);
        }
    }
    if (TC == TC_FILL) return;
    // this thread's four output pixels (last phase) are requested before the two adjoint passes
    const int fc = t & (ST_TW - 1), fr4 = (t >> 6) * 4;
    float fp[4], ft[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const size_t oo = (size_t)min(y0 + fr4 + o, q.H - 1) * q.W + min(x0 + fc, q.W - 1);
        fp[o] = pp[oo]; ft[o] = tp[oo];
    }
    __syncthreads();
    float sabs = 0.f, ssq = 0.f;
    if (GRAD) {
        st_adj_row(Dm, Hh, t);
        __syncthreads();
    }
    // ---- adjoint column filter + pixel term: thread = (column c, 4 rows)
    {
        const int c = fc, r4 = fr4;
        float am[4] = {0, 0, 0, 0}, aq[4] = {0, 0, 0, 0}, ar[4] = {0, 0, 0, 0};
        if (GRAD) st_adj_col(Hh, r4, c, am, aq, ar);
        const int gx = x0 + c;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int gy = y0 + r4 + o;
            if (gy >= q.H || gx >= q.W) continue;
            const size_t oo = (size_t)gy * q.W + gx;
            const float p = fp[o], tg = ft[o], d = p - tg;
            sabs += fabsf(d);
            ssq = fmaf(d, d, ssq);
            if (GRAD) {
                float g = L2T ? q.g_l2 * d : q.g_l1 * ((d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f));
                g -= q.g_ssim * (am[o] + 2.f * p * aq[o] + tg * ar[o]);
                q.dpred[(size_t)plane * HW + oo] = g;
            }
        }
    }
    const float ts = orn_block_sum(ssum, sred);
    const float ta = orn_block_sum(sabs, sred);
    const float tq = orn_block_sum(ssq, sred);
    if (t == 0) {
        const size_t bi = (size_t)plane * gridDim.x + blockIdx.x;
        q.part_ssim[bi] = ts;
        q.part_l1[2 * bi] = ta;
        q.part_l1[2 * bi + 1] = tq;
    }
}

// L1 / L2 losses (no SSIM term), and LT == ORN_LOSS_FUSION7: both terms (Fusion7 / Fusion8).  LT / GRAD are compile-time: the per-pixel loop carries no loss-type or null-pointer branches
template <int LT, bool GRAD>
__global__ void __launch_bounds__(256) k_loss_grad(LossP q)
{
    __shared__ float sred[16];
    const int t = threadIdx.x;
    const int plane = blockIdx.y;
    const int tw = blockIdx.x % q.tiles_w, th = blockIdx.x / q.tiles_w;
    const int y0 = th * SS_TH, x0 = tw * SS_TW;
    const size_t HW = (size_t)q.H * q.W;
    const float *pp = q.pred + (size_t)plane * HW;
    const float *tp = q.target + (q.frame_idx ? (size_t)(*q.frame_idx) * q.frame_stride : 0) + (size_t)plane * HW;
    float sabs = 0.f, ssq = 0.f;
    for (int idx = t; idx < SS_TH * SS_TW; idx += 256) {
        const int r = idx / SS_TW, c = idx - r * SS_TW;
        const int gy = y0 + r, gx = x0 + c;
        if (gy >= q.H || gx >= q.W) continue;
        const size_t o = (size_t)gy * q.W + gx;
        const float p = pp[o], tg = tp[o], d = p - tg;
        sabs += fabsf(d);
        ssq = fmaf(d, d, ssq);
        if (GRAD) {
            float g;
            if (LT == ORN_LOSS_L2) g = q.g_l2 * d;
            else if (LT == ORN_LOSS_FUSION7) g = fmaf(q.g_l2, d, q.g_l1 * ((d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f)));
            else g = q.g_l1 * ((d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f));
            q.dpred[(size_t)plane * HW + o] = g;
        }
    }
    const float ta = orn_block_sum(sabs, sred);
    const float tq = orn_block_sum(ssq, sred);
    if (t == 0) {
        const size_t bi = (size_t)plane * gridDim.x + blockIdx.x;
        q.part_l1[2 * bi] = ta;
        q.part_l1[2 * bi + 1] = tq;
    }
}

// One block; fixed-order strided partial sums in double, then a fixed tree (orn_common.h: orn_loss_finalize_block).
__global__ void __launch_bounds__(256) k_loss_finalize(OrnLossFinalJob j)
{
    __shared__ double sd[3 * 256];
    orn_loss_finalize_block(j, sd);
}

// The loss of a SPLIT step (orn_engine_step_forward / orn_engine_step_backward): the caller computed the loss and dLoss/dpred itself.
// What is left for the device: the {|d|, d^2} tile partials of pred - target that every built-in loss leaves in part_l1 (L1, MSE, PSNR
// of the step's record), and a scan of the caller's gradient for NaN / inf (the step's flag: Adam then skips the step).  One 16x64
// tile per work-group as in k_loss_grad; VEC4 (W % 4 == 0, 16-byte aligned planes): one float4 of each tensor per thread.
struct LossExtP {
    const float *pred, *target, *dpred;      // dpred null: no scan (an abandoned step)
    const int *frame_idx;
    size_t frame_stride;
    int H, W, tiles_w;
    float *part_l1;                          // [n_blocks][2]
    OrnScaleState *sc;
};

template <bool VEC4>
__global__ void __launch_bounds__(256) k_loss_ext(LossExtP q)
{
    __shared__ float sred[16];
    const int t = threadIdx.x;
    const int plane = blockIdx.y;
    const int tw = blockIdx.x % q.tiles_w, th = blockIdx.x / q.tiles_w;
    const int y0 = th * SS_TH, x0 = tw * SS_TW;
    const size_t HW = (size_t)q.H * q.W;
    const float *pp = q.pred + (size_t)plane * HW;
    const float *tp = q.target + (q.frame_idx ? (size_t)(*q.frame_idx) * q.frame_stride : 0) + (size_t)plane * HW;
    const float *gp = q.dpred ? q.dpred + (size_t)plane * HW : nullptr;
    float sabs = 0.f, ssq = 0.f;
    bool bad = false;
    if (VEC4) {
        const int r = t / (SS_TW / 4), c = (t - r * (SS_TW / 4)) * 4;
        const int gy = y0 + r, gx = x0 + c;
        if (gy < q.H && gx < q.W) {                        // W % 4 == 0: the whole float4 lies inside the row
            const size_t o = (size_t)gy * q.W + gx;
            const float4 p = *reinterpret_cast<const float4 *>(pp + o), tg = *reinterpret_cast<const float4 *>(tp + o);
            const float d[4] = {p.x - tg.x, p.y - tg.y, p.z - tg.z, p.w - tg.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) { sabs += fabsf(d[k]); ssq = fmaf(d[k], d[k], ssq); }
            if (gp) {
                const float4 g = *reinterpret_cast<const float4 *>(gp + o);
                bad = !(fabsf(g.x) <= 3.0e38f) || !(fabsf(g.y) <= 3.0e38f) || !(fabsf(g.z) <= 3.0e38f) || !(fabsf(g.w) <= 3.0e38f);
            }
        }
    } else {
        for (int idx = t; idx < SS_TH * SS_TW; idx += 256) {
            const int r = idx / SS_TW, c = idx - r * SS_TW;
            const int gy = y0 + r, gx = x0 + c;
            if (gy >= q.H || gx >= q.W) continue;
            const size_t o = (size_t)gy * q.W + gx;
            const float d = pp[o] - tp[o];
            sabs += fabsf(d);
            ssq = fmaf(d, d, ssq);
            if (gp) bad = bad || !(fabsf(gp[o]) <= 3.0e38f);
        }
    }
    if (bad) orn_flag_nonfinite(q.sc, __builtin_inff());
    const float ta = orn_block_sum(sabs, sred);
    const float tq = orn_block_sum(ssq, sred);
    if (t == 0) {
        const size_t bi = (size_t)plane * gridDim.x + blockIdx.x;
        q.part_l1[2 * bi] = ta;
        q.part_l1[2 * bi + 1] = tq;
    }
}

// Finalize stage of the split step, one work-group: the partials summed as orn_loss_finalize_block sums them (strided per thread
// in double, then the fixed tree), the step's stats and ring record, and the checks of what the caller handed in.
struct LossExtFinal {
    const float *part_l1; int n_l1; double n_elem;
    const float *loss;             // the caller's loss value (device; null: the record holds 0)
    int abandon;                   // the caller gave the step up: its flag goes up whatever the values
    float *stats; const OrnStepCur *cur; float *ring; OrnScaleState *sc;
};

__global__ void __launch_bounds__(256) k_loss_ext_finalize(LossExtFinal j)
{
    __shared__ double sd[2 * 256];
    const int t = threadIdx.x, nt = blockDim.x;
    double a = 0.0, b = 0.0;
    for (int i = t; i < j.n_l1; i += nt) { a += (double)j.part_l1[2 * i]; b += (double)j.part_l1[2 * i + 1]; }
    sd[t] = a; sd[nt + t] = b;
    __syncthreads();
    for (int s = nt >> 1; s > 0; s >>= 1) {
        if (t < s) { sd[t] += sd[t + s]; sd[nt + t] += sd[nt + t + s]; }
        __syncthreads();
    }
    if (t == 0) {
        const float l1 = (float)(sd[0] / j.n_elem);
        const float mse = (float)(sd[nt] / j.n_elem);
        const float loss = j.loss ? *j.loss : 0.f;
        orn_flag_nonfinite(j.sc, loss);                // the caller's loss is NaN / inf: no update from this step
        orn_flag_nonfinite(j.sc, mse);                 // so is the forward pass itself
        if (j.abandon && j.sc) j.sc->flag = 1;
        const float psnr = -10.0f * log10f(mse);
        j.stats[0] = loss; j.stats[1] = l1; j.stats[2] = mse; j.stats[3] = 0.f; j.stats[4] = psnr;
        j.stats[5] = 0.f; j.stats[6] = 0.f; j.stats[7] = 0.f;
        if (j.ring) {
            float *r = j.ring + (size_t)j.cur->slot * 8;
            r[0] = loss; r[1] = l1; r[2] = mse; r[3] = 0.f; r[4] = psnr;
            r[5] = j.cur->lr; r[6] = (float)j.cur->frame; r[7] = (float)j.cur->step;
        }
    }
}

// pytorch_msssim _fspecial_gauss_1d(11, 1.5): fp32 exp, fp32 normalise
void orn_gauss_taps(float g[11])
{
    float s = 0.f;
    for (int i = 0; i < 11; ++i) {
        const float c = (float)(i - 5);
        g[i] = expf(-(c * c) / (2.0f * 1.5f * 1.5f));
        s += g[i];
    }
    for (int i = 0; i < 11; ++i) g[i] /= s;
}

struct LossGeom { int planes, Hv, Wv, tw, th; size_t nmap, off_pl, total; };

// one tiling (16 x 64 pixels of the image) for every loss type; per-tile partial sums: SSIM [n], {|d|, d^2} [n][2]
static LossGeom loss_geom(int B, int Ch, int H, int W)
{
    LossGeom g;
    g.planes = B * Ch;
    g.Hv = H > 10 ? H - 10 : 0;
    g.Wv = W > 10 ? W - 10 : 0;
    g.tw = orn_cdiv(W, SS_TW); g.th = orn_cdiv(H, SS_TH);
    g.nmap = (size_t)g.planes * g.Hv * g.Wv;
    g.off_pl = orn_align((size_t)g.planes * g.tw * g.th * 4 + 4) / 4;
    g.total = g.off_pl + orn_align((size_t)g.planes * g.tw * g.th * 8 + 8) / 4;
    return g;
}

extern "C" size_t orn_loss_ws_bytes(int B, int Ch, int H, int W) { return loss_geom(B, Ch, H, W).total * 4; }

extern "C" int orn_loss_spec(int loss_type, float *weights3, int *kind)
{
    const OrnLossSpec *sp = orn_loss_spec_of(loss_type);
    ORN_REQUIRE(sp, "loss: loss_type %d is not built", loss_type);
    if (weights3) { weights3[0] = (float)sp->w_l1; weights3[1] = (float)sp->w_l2; weights3[2] = (float)sp->w_struct; }
    if (kind) *kind = sp->kind;
    return 0;
}

// the MS-SSIM kinds append their own region (orn_loss_msssim.hip) behind the tile partials every loss type has
extern "C" size_t orn_loss_ws_bytes_for(int loss_type, int B, int Ch, int H, int W)
{
    const OrnLossSpec *sp = orn_loss_spec_of(loss_type);
    if (!sp || B <= 0 || Ch <= 0 || H <= 0 || W <= 0) return 0;
    size_t f = loss_geom(B, Ch, H, W).total;
    if (sp->kind == ORN_LOSS_KIND_MSSSIM) {
        if ((H < W ? H : W) <= 160 || (long)B * Ch > 64) return 0;
        f += orn_loss_msssim_ws_floats((size_t)B * Ch, H, W);
    }
    return f * 4;
}

// Must be called once outside any graph capture (orn_ssim_tile_init).
int orn_loss_init()
{
    ORN_TRY(orn_ssim_tile_init({(const void *)k_fusion6<true, TC_NONE>, (const void *)k_fusion6<false, TC_NONE>, (const void *)k_fusion6<true, TC_READ>,
                                (const void *)k_fusion6<false, TC_READ>, (const void *)k_fusion6<false, TC_FILL>,
                                (const void *)k_fusion6<true, TC_NONE, true>, (const void *)k_fusion6<true, TC_READ, true>}));
    return orn_loss_msssim_init();
}

int orn_launch_loss(const float *pred, const float *target, const int *frame_idx, size_t frame_stride, int B, int Ch,
                    int H, int W, int loss_type, float loss_scale, float *stats, float *dpred, float *ws,
                    hipStream_t st, const OrnStepCur *cur, float *ring, OrnScaleState *sc, const float *tstats, OrnLossFinalJob *defer)
{
    const OrnLossSpec *sp = orn_loss_spec_of(loss_type);
    ORN_REQUIRE(sp, "loss: unsupported loss_type %d", loss_type);
    ORN_TRY(orn_loss_init());
    static_assert(SS_TH == ST_TH && SS_TW == ST_TW, "one tiling for all loss kernels");
    const LossGeom g = loss_geom(B, Ch, H, W);
    const bool ssim = sp->kind == ORN_LOSS_KIND_SSIM, msssim = sp->kind == ORN_LOSS_KIND_MSSSIM;
    if (ssim) ORN_REQUIRE(g.Hv > 0 && g.Wv > 0, "loss: SSIM needs H,W > 10 (got %dx%d)", H, W);
    if (msssim) {
        ORN_REQUIRE((H < W ? H : W) > 160, "loss: the MS-SSIM losses need an image side above 160 (got %dx%d)", H, W);
        ORN_REQUIRE(g.planes <= 64, "loss: the MS-SSIM losses take at most 64 planes (got %d)", g.planes);
        ORN_REQUIRE(!frame_idx || frame_stride == (size_t)Ch * H * W, "loss: MS-SSIM: frames must be contiguous");
    }
    LossP q;
    q.pred = pred; q.target = target; q.frame_idx = frame_idx; q.frame_stride = frame_stride;
    q.planes = g.planes; q.H = H; q.W = W; q.Hv = g.Hv; q.Wv = g.Wv;
    q.part_ssim = ws; q.part_l1 = ws + g.off_pl;
    q.dpred = dpred; q.loss_type = loss_type;
    q.tstats = const_cast<float *>(tstats); q.tstats_stride = 2 * g.nmap;
    q.vec4 = orn_loss_vec4(W, (uintptr_t)pred | (uintptr_t)target, frame_stride, frame_idx) ? 1 : 0;
    const double n = (double)g.planes * H * W;
    // (ids 0..2: the values they have always had -- 0.7 * loss_scale / n, 2.0 * loss_scale / n, 0.3 * loss_scale / nmap)
    q.g_l1 = (float)(sp->w_l1 * loss_scale / n);
    q.g_l2 = (float)(2.0 * sp->w_l2 * loss_scale / n);
    q.g_ssim = g.nmap ? (float)(sp->w_struct * loss_scale / (double)g.nmap) : 0.f;
    q.tiles_w = g.tw; q.tiles_h = g.th;
    const int n_tiles = g.planes * g.tw * g.th;
    const float *ms_val = nullptr;
    if (msssim) {
        ORN_TRY(orn_launch_loss_msssim(pred, target, frame_idx, frame_stride, g.planes, H, W, q.g_l1, q.g_l2, (float)(sp->w_struct * loss_scale),
                                       dpred, q.part_l1, ws + g.total, st, &ms_val));
    } else {
        const dim3 gr(g.tw * g.th, g.planes), bl(256);
        const bool gd = q.dpred != nullptr;
        const bool l2t = sp->w_l2 != 0.0;      // SSIM kinds: an L2 pixel term in place of the L1 one (no loss has both)
        if (ssim) {
            if (tstats) {
                if (!gd) hipLaunchKernelGGL((k_fusion6<false, TC_READ>), gr, bl, ST_LDS_FLOATS * 4, st, q);
                else if (l2t) hipLaunchKernelGGL((k_fusion6<true, TC_READ, true>), gr, bl, ST_LDS_FLOATS * 4, st, q);
                else hipLaunchKernelGGL((k_fusion6<true, TC_READ>), gr, bl, ST_LDS_FLOATS * 4, st, q);
            }
            else if (!gd) hipLaunchKernelGGL((k_fusion6<false, TC_NONE>), gr, bl, ST_LDS_FLOATS * 4, st, q);
            else if (l2t) hipLaunchKernelGGL((k_fusion6<true, TC_NONE, true>), gr, bl, ST_LDS_FLOATS * 4, st, q);
            else hipLaunchKernelGGL((k_fusion6<true, TC_NONE>), gr, bl, ST_LDS_FLOATS * 4, st, q);
        }
        else if (loss_type == ORN_LOSS_L2) { if (gd) hipLaunchKernelGGL((k_loss_grad<ORN_LOSS_L2, true>), gr, bl, 0, st, q); else hipLaunchKernelGGL((k_loss_grad<ORN_LOSS_L2, false>), gr, bl, 0, st, q); }
        else if (loss_type == ORN_LOSS_L1) { if (gd) hipLaunchKernelGGL((k_loss_grad<ORN_LOSS_L1, true>), gr, bl, 0, st, q); else hipLaunchKernelGGL((k_loss_grad<ORN_LOSS_L1, false>), gr, bl, 0, st, q); }
        else { if (gd) hipLaunchKernelGGL((k_loss_grad<ORN_LOSS_FUSION7, true>), gr, bl, 0, st, q); else hipLaunchKernelGGL((k_loss_grad<ORN_LOSS_L1, false>), gr, bl, 0, st, q); }
        ORN_LAUNCH_CHECK("loss");
    }
    OrnLossFinalJob fj = {q.part_ssim, ssim ? n_tiles : 0, q.part_l1, n_tiles, n, (double)g.nmap, loss_type,
                          loss_scale, stats, cur, ring, sc};
    fj.w_l1 = (float)sp->w_l1; fj.w_l2 = (float)sp->w_l2; fj.w_struct = (float)sp->w_struct; fj.ms_val = ms_val;
    if (defer) { *defer = fj; return 0; }              // the caller runs it as a rider of a later launch
    hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(256), 0, st, fj);
    ORN_LAUNCH_CHECK("loss_finalize");
    return 0;
}

// The loss stage of a split step (k_loss_ext + its finalize launch).  ws: orn_loss_ws_bytes floats, the part_l1 region of the layout
// every loss type shares.  dpred null: the step is abandoned (no scan, the flag goes up).
int orn_launch_loss_ext(const float *pred, const float *target, const int *frame_idx, size_t frame_stride, int Ch, int H, int W,
                        const float *dpred, const float *loss, float *stats, float *ws, hipStream_t st, const OrnStepCur *cur,
                        float *ring, OrnScaleState *sc)
{
    const LossGeom g = loss_geom(1, Ch, H, W);
    LossExtP q;
    q.pred = pred; q.target = target; q.dpred = dpred; q.frame_idx = frame_idx; q.frame_stride = frame_stride;
    q.H = H; q.W = W; q.tiles_w = g.tw;
    q.part_l1 = ws + g.off_pl;
    q.sc = sc;
    const bool vec4 = orn_loss_vec4(W, (uintptr_t)pred | (uintptr_t)target | (uintptr_t)dpred, frame_stride, frame_idx);
    const dim3 gr(g.tw * g.th, g.planes), bl(256);
    if (vec4) hipLaunchKernelGGL(k_loss_ext<true>, gr, bl, 0, st, q);
    else hipLaunchKernelGGL(k_loss_ext<false>, gr, bl, 0, st, q);
    ORN_LAUNCH_CHECK("loss_ext");
    const LossExtFinal fj = {q.part_l1, g.planes * g.tw * g.th, (double)g.planes * H * W, loss, dpred ? 0 : 1, stats, cur, ring, sc};
    hipLaunchKernelGGL(k_loss_ext_finalize, dim3(1), dim3(256), 0, st, fj);
    ORN_LAUNCH_CHECK("loss_ext_finalize");
    return 0;
}

// The target side of Fusion6's SSIM statistics for `n` frames (LossP::tstats): out [n][2][Ch][H-10][W-10].
extern "C" size_t orn_loss_target_stats_bytes(int n, int Ch, int H, int W)
{
    if (n <= 0 || Ch <= 0 || H <= 10 || W <= 10) return 0;
    return (size_t)n * 2 * Ch * (H - 10) * (W - 10) * sizeof(float);
}

extern "C" int orn_loss_target_stats(const float *frames, int n, int Ch, int H, int W, float *out, void *stream)
{
    ORN_REQUIRE(frames && out && n > 0 && Ch > 0 && H > 10 && W > 10 && n <= 65535, "loss_target_stats: bad arguments");
    ORN_TRY(orn_loss_init());
    const LossGeom g = loss_geom(1, Ch, H, W);
    LossP q = {};
    q.pred = frames; q.target = frames; q.frame_idx = nullptr; q.frame_stride = (size_t)Ch * H * W;
    q.planes = g.planes; q.H = H; q.W = W; q.Hv = g.Hv; q.Wv = g.Wv;
    q.tstats = out; q.tstats_stride = 2 * g.nmap;
    q.loss_type = ORN_LOSS_FUSION6;
    q.vec4 = orn_loss_vec4(W, (uintptr_t)frames, q.frame_stride, nullptr) ? 1 : 0;      // (frames of Ch * H * W floats: W % 4 == 0 covers the stride)
    q.tiles_w = g.tw; q.tiles_h = g.th;
    hipLaunchKernelGGL((k_fusion6<false, TC_FILL>), dim3(g.tw * g.th, g.planes, n), dim3(256), ST_LDS_FLOATS * 4, (hipStream_t)stream, q);
    ORN_LAUNCH_CHECK("loss_target_stats");
    return 0;
}

extern "C" int orn_loss_fwd_bwd(const float *pred, const float *target, int B, int Ch, int H, int W, int loss_type,
                                float loss_scale, float *stats, float *dpred, void *ws, size_t ws_bytes,
                                void *stream)
{
    ORN_REQUIRE(pred && target && stats && ws, "loss_fwd_bwd: null pointer");
    ORN_REQUIRE(B > 0 && Ch > 0 && H > 0 && W > 0, "loss_fwd_bwd: bad sizes");
    const OrnLossSpec *sp = orn_loss_spec_of(loss_type);
    ORN_REQUIRE(sp, "loss_fwd_bwd: unsupported loss_type %d", loss_type);
    if (sp->kind == ORN_LOSS_KIND_MSSSIM) {
        ORN_REQUIRE((H < W ? H : W) > 160, "loss_fwd_bwd: the MS-SSIM losses need an image side above 160 (got %dx%d)", H, W);
        ORN_REQUIRE((long)B * Ch <= 64, "loss_fwd_bwd: the MS-SSIM losses take at most 64 planes (got %ld)", (long)B * Ch);
        ORN_REQUIRE((uintptr_t)ws % 16 == 0, "loss_fwd_bwd: the MS-SSIM losses need a 16-byte aligned workspace");
    }
    const size_t need = orn_loss_ws_bytes_for(loss_type, B, Ch, H, W);
    if (ws_bytes < need) {
        orn_set_error("loss_fwd_bwd: workspace %zu < %zu", ws_bytes, need);
        return ORN_E_WS;
    }
    return orn_launch_loss(pred, target, nullptr, 0, B, Ch, H, W, loss_type, loss_scale, stats, dpred, (float *)ws,
                           (hipStream_t)stream, nullptr, nullptr);
}

// ================================================================================================
// N3  msssim_fn (utils.py:201-211): pytorch_msssim.ms_ssim, 5 scales, weights (0.0448, 0.2856, 0.3001, 0.2363,
// 0.1333), avg_pool2d(2) between scales (parity unpinned like SSIM: the package is not in the reference tree).
// Logging metric only -- kept off the timed training path.
// One implementation serves both entry points of include/orn.h: orn_msssim_frames (one value per frame for n frame pairs; the
// `msssim` column of orn_engine_eval_frames) and orn_msssim (the mean over B*Ch planes: one group of B*Ch planes).
// Per chunk of F groups of Ch planes: ONE launch per pyramid level over F x Ch planes, then ONE finalize launch.
// Nothing is uploaded and nothing synchronises: the five levels' geometry is a kernel argument.
//   k_msssim_level, per 16x64 tile of one plane: loads the tile with its 10-pixel apron of pred and target into LDS, runs the
//   11-tap Gaussian as separable fmaf chains (rows, then columns) over x, y, x^2, y^2 and xy, and sums ssim_map and cs_map over the
//   tile's part of the VALID map (H-10 x W-10) into one pair of per-tile partials.  From the patch it already holds it also writes
//   the 2x2 average-pooled pred and target (avg_pool2d, padding = size % 2, count_include_pad: in-bounds taps added in (dy, dx)
//   order, then * 0.25f) of the region it OWNS into the next level's buffers.
//   Ownership: pooled pixel (yo, xo) belongs to the tile that holds its first in-bounds input row max(2*yo - ph, 0) and column
//   max(2*xo - pw, 0); the second row / column then lies at most one past the tile's 16 x 64 pixels, inside its 10-pixel apron.
//   The last tile row / column own everything up to the image edge: the tiles cover the VALID map, so what is left of the image
//   behind them is at most the apron.
// Summation order (the contract: the values do not depend on n, the chunk size or the entry point): per tile orn_block_sum of the
// threads' float sums; per plane and level the tile partials walked in tile order in double; per group the planes' weighted
// products summed in plane order in double, then divided by Ch.
// ================================================================================================
struct OrnMsLevel {
    const float *x, *y;          // pred planes [F][Ch][H][W]; target planes likewise, or (level 0) the frame table rows index
    const int32_t *rows;         // level 0: frame k's target is y[rows[k]]; nullptr: y[k]
    int Ch, H, W, tiles_w, tiles_h;
    float *part;                 // [F*Ch][tiles][2]
    float *nx, *ny;              // next level's planes [F*Ch][Ho][Wo]; nullptr at the last level
    int Ho, Wo, ph, pw;          // avg_pool2d(2, padding = size % 2)
};
struct OrnMsGeom { int nblk[5]; float nmap[5]; };

__global__ void __launch_bounds__(256) k_msssim_level(OrnMsLevel q)
{
    __shared__ __attribute__((aligned(16))) float Ps[SS_PH][SS_PWP];
    __shared__ __attribute__((aligned(16))) float Ts[SS_PH][SS_PWP];
    __shared__ float Hs[5][SS_PH][SS_TW];
    __shared__ float sred[16];
    const int t = threadIdx.x, plane = blockIdx.y;
    const int H = q.H, W = q.W;
    const int tw = blockIdx.x % q.tiles_w, th = blockIdx.x / q.tiles_w;
    const int y0 = th * SS_TH, x0 = tw * SS_TW;
    const int Hv = H - 10, Wv = W - 10;
    const int frame = plane / q.Ch;
    const size_t tplane = q.rows ? (size_t)q.rows[frame] * q.Ch + (plane - frame * q.Ch) : (size_t)plane;
    const float *pp = q.x + (size_t)plane * H * W, *tp = q.y + tplane * H * W;
    for (int idx = t; idx < SS_PH * SS_PWP; idx += 256) {
        const int r = idx / SS_PWP, c = idx - r * SS_PWP;
        const int gy = y0 + r, gx = x0 + c;
        const bool ok = c < SS_PW && gy < H && gx < W;
        Ps[r][c] = ok ? pp[(size_t)gy * W + gx] : 0.f;
        Ts[r][c] = ok ? tp[(size_t)gy * W + gx] : 0.f;
    }
    __syncthreads();
    if (q.nx) {
        // pooled rows [yo0, yo1) x columns [xo0, xo1): the ones whose first in-bounds input row / column this tile holds
        const int yo0 = th == 0 ? 0 : y0 / 2 + q.ph, yo1 = th == q.tiles_h - 1 ? q.Ho : (y0 + SS_TH) / 2 + q.ph;
        const int xo0 = tw == 0 ? 0 : x0 / 2 + q.pw, xo1 = tw == q.tiles_w - 1 ? q.Wo : (x0 + SS_TW) / 2 + q.pw;
        const int nxo = xo1 - xo0, cnt = (yo1 - yo0) * nxo;
        float *ox = q.nx + (size_t)plane * q.Ho * q.Wo, *oy = q.ny + (size_t)plane * q.Ho * q.Wo;
        for (int idx = t; idx < cnt; idx += 256) {
            const int yo = yo0 + idx / nxo, xo = xo0 + idx % nxo;
            float sx = 0.f, sy = 0.f;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int yy = yo * 2 + dy - q.ph, xx = xo * 2 + dx - q.pw;
                    if (yy >= 0 && yy < H && xx >= 0 && xx < W) { sx += Ps[yy - y0][xx - x0]; sy += Ts[yy - y0][xx - x0]; }
                }
            ox[(size_t)yo * q.Wo + xo] = sx * 0.25f;
            oy[(size_t)yo * q.Wo + xo] = sy * 0.25f;
        }
    }
    for (int idx = t; idx < SS_PH * SS_TW; idx += 256) {
        const int r = idx / SS_TW, c = idx - r * SS_TW;
        float sp = 0.f, st = 0.f, spp = 0.f, stt = 0.f, spt = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float g = c_gauss[k], a = Ps[r][c + k], b = Ts[r][c + k];
            sp = fmaf(g, a, sp); st = fmaf(g, b, st);
            spp = fmaf(g, a * a, spp); stt = fmaf(g, b * b, stt); spt = fmaf(g, a * b, spt);
        }
        Hs[0][r][c] = sp; Hs[1][r][c] = st; Hs[2][r][c] = spp; Hs[3][r][c] = stt; Hs[4][r][c] = spt;
    }
    __syncthreads();
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    float ss = 0.f, cs = 0.f;
    for (int idx = t; idx < SS_TH * SS_TW; idx += 256) {
        const int r = idx / SS_TW, c = idx - r * SS_TW;
        if (y0 + r >= Hv || x0 + c >= Wv) continue;
        float m = 0.f, mu = 0.f, qq = 0.f, tt = 0.f, rr = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) {
            const float g = c_gauss[k];
            m = fmaf(g, Hs[0][r + k][c], m); mu = fmaf(g, Hs[1][r + k][c], mu);
            qq = fmaf(g, Hs[2][r + k][c], qq); tt = fmaf(g, Hs[3][r + k][c], tt); rr = fmaf(g, Hs[4][r + k][c], rr);
        }
        const float csm = (2.f * (rr - m * mu) + C2) / ((qq - m * m) + (tt - mu * mu) + C2);
        cs += csm;
        ss += ((2.f * m * mu + C1) / (m * m + mu * mu + C1)) * csm;
    }
    const float a = orn_block_sum(ss, sred);
    const float b = orn_block_sum(cs, sred);
    if (t == 0) {
        const size_t bi = (size_t)plane * gridDim.x + blockIdx.x;
        q.part[2 * bi] = a;
        q.part[2 * bi + 1] = b;
    }
}

// One thread per (frame, plane): level means -> relu -> weighted product, then per frame the mean over its planes in plane order.
// 256 / Ch frames per work-group.
__global__ void __launch_bounds__(256) k_msssim_frames_finalize(const float *__restrict__ part, OrnMsGeom g, int F, int Ch, float *__restrict__ out)
{
    __shared__ double acc[256];
    const int fpb = 256 / Ch, fl = threadIdx.x / Ch, pc = threadIdx.x - fl * Ch;
    const int frame = blockIdx.x * fpb + fl, planes = F * Ch;
    const bool live = fl < fpb && frame < F;
    double val = 0.0;
    if (live) {
        const size_t pl = (size_t)frame * Ch + pc;
        size_t off = 0;
        double prod = 1.0;
        for (int lv = 0; lv < 5; ++lv) {
            const double v = orn_msssim_level_mean(part + off, pl, g.nblk[lv], g.nmap[lv], lv);
            off += (size_t)2 * planes * g.nblk[lv];
            prod *= pow(v > 0.0 ? v : 0.0, (double)c_ms_weights[lv]);
        }
        val = prod;
    }
    acc[threadIdx.x] = val;
    __syncthreads();
    if (live && pc == 0) {
        double s = 0.0;
        for (int i = 0; i < Ch; ++i) s += acc[fl * Ch + i];
        out[frame] = (float)(s / Ch);
    }
}

// One level's geometry in the kernel's argument: sizes, the 16x64 tiling of the VALID map, the pooled size and padding (pool: the
// level writes the next one's planes).  orn_msssim_layout, the level launches and orn_debug_msssim_level_fwd all come through here.
static OrnMsLevel ms_level_geom(int H, int W, bool pool)
{
    OrnMsLevel q = {};
    q.H = H; q.W = W;
    q.tiles_w = orn_cdiv(W - 10, SS_TW); q.tiles_h = orn_cdiv(H - 10, SS_TH);
    if (pool) { q.Ho = orn_msssim_pooled(H); q.Wo = orn_msssim_pooled(W); q.ph = H % 2; q.pw = W % 2; }
    return q;
}

// One chunk's workspace in floats: pooled pred / target planes of levels 1..4, then every level's per-tile partials
void orn_msssim_layout(size_t planes, int H, int W, OrnMsLayout *out)
{
    OrnMsLayout &ly = *out;
    orn_msssim_geom(H, W, ly.Hs, ly.Ws);
    size_t f = 0, nb = 0;
    ly.pooled[0][0] = ly.pooled[0][1] = 0;
    for (int l = 1; l < 5; ++l)
        for (int k = 0; k < 2; ++k) {
            ly.pooled[l][k] = f;
            f += orn_align(planes * ly.Hs[l] * ly.Ws[l] * 4) / 4;
        }
    ly.part = f;
    for (int l = 0; l < 5; ++l) {
        const OrnMsLevel q = ms_level_geom(ly.Hs[l], ly.Ws[l], l < 4);
        ly.nblk[l] = q.tiles_w * q.tiles_h;
        ly.nmap[l] = (float)(ly.Hs[l] - 10) * (float)(ly.Ws[l] - 10);
        ly.part_off[l] = 2 * planes * nb;
        nb += (size_t)ly.nblk[l];
    }
    ly.total = f + orn_align(2 * planes * nb * 4) / 4;
}

extern "C" size_t orn_msssim_frames_ws_bytes(int n, int Ch, int H, int W)
{
    if (n <= 0 || Ch <= 0 || Ch > 64 || (H < W ? H : W) <= 160) return 0;
    OrnMsLayout ly;
    orn_msssim_layout((size_t)n * Ch, H, W, &ly);
    return ly.total * 4;
}

// The most frames one chunk may hold in ws_bytes (0: not even one); F * Ch is a grid dimension.
int orn_msssim_frames_chunk(int n, int Ch, int H, int W, size_t ws_bytes)
{
    int F = n < 65535 / Ch ? n : 65535 / Ch;
    while (F > 0 && orn_msssim_frames_ws_bytes(F, Ch, H, W) > ws_bytes) --F;
    return F;
}

size_t orn_msssim_pyramid_floats(size_t planes, int H, int W)
{
    OrnMsLayout ly;
    orn_msssim_layout(planes, H, W, &ly);
    return ly.total;
}

// The five level launches of one chunk (F frames whose workspace fits: the callers check); *out describes what they left in ws.
int orn_launch_msssim_levels(const float *pred, const float *targets, const int32_t *rows, int F, int Ch, int H, int W, float *ws,
                             hipStream_t st, OrnMsPyramid *out)
{
    OrnMsPyramid &py = *out;
    const size_t planes = (size_t)F * Ch;
    OrnMsLayout ly;
    orn_msssim_layout(planes, H, W, &ly);
    for (int l = 0; l < 5; ++l) {
        py.Hs[l] = ly.Hs[l]; py.Ws[l] = ly.Ws[l]; py.nblk[l] = ly.nblk[l]; py.nmap[l] = ly.nmap[l]; py.part_off[l] = ly.part_off[l];
        for (int k = 0; k < 2; ++k) py.pooled[l][k] = l ? ws + ly.pooled[l][k] : nullptr;
    }
    py.part = ws + ly.part;
    const float *x = pred, *y = targets;
    for (int l = 0; l < 5; ++l) {
        OrnMsLevel q = ms_level_geom(py.Hs[l], py.Ws[l], l < 4);
        q.x = x; q.y = y; q.rows = l ? nullptr : rows; q.Ch = Ch;
        q.part = py.part + py.part_off[l];
        if (l < 4) { q.nx = py.pooled[l + 1][0]; q.ny = py.pooled[l + 1][1]; }
        hipLaunchKernelGGL(k_msssim_level, dim3(py.nblk[l], (unsigned)planes), dim3(256), 0, st, q);
        ORN_LAUNCH_CHECK("msssim_level");
        x = q.nx; y = q.ny;
    }
    return 0;
}

// One chunk: F frames whose workspace fits (the callers check).  Six launches.
int orn_launch_msssim_frames(const float *pred, const float *targets, const int32_t *rows, int F, int Ch, int H, int W, float *out,
                             float *ws, hipStream_t st)
{
    OrnMsPyramid py;
    ORN_TRY(orn_launch_msssim_levels(pred, targets, rows, F, Ch, H, W, ws, st, &py));
    OrnMsGeom g;
    for (int l = 0; l < 5; ++l) { g.nblk[l] = py.nblk[l]; g.nmap[l] = py.nmap[l]; }
    const int fpb = 256 / Ch;
    hipLaunchKernelGGL(k_msssim_frames_finalize, dim3(orn_cdiv(F, fpb)), dim3(256), 0, st, py.part, g, F, Ch, out);
    ORN_LAUNCH_CHECK("msssim_frames_finalize");
    return 0;
}

// out[k] = ms_ssim(pred[k:k+1], targets[rows[k]] (rows NULL: targets[k]), data_range=1), k < n, in chunks of as many frames as ws holds.
extern "C" int orn_msssim_frames(const float *pred, const float *targets, const int32_t *rows, int n, int Ch, int H, int W, float *out,
                                 void *ws, size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(n >= 0 && Ch > 0 && Ch <= 64, "msssim_frames: bad frame / plane count");
    ORN_REQUIRE((H < W ? H : W) > 160, "msssim_frames: image side must exceed 160 (got %dx%d)", H, W);
    if (n == 0) return 0;
    ORN_REQUIRE(pred && targets && out && ws, "msssim_frames: null pointer");
    const int chunk = orn_msssim_frames_chunk(n, Ch, H, W, ws_bytes);
    if (chunk < 1) { orn_set_error("msssim_frames: workspace too small"); return ORN_E_WS; }
    ORN_TRY(orn_loss_init());
    for (int k = 0; k < n; k += chunk) {
        const int F = n - k < chunk ? n - k : chunk;
        const size_t at = (size_t)k * Ch * H * W;
        ORN_TRY(orn_launch_msssim_frames(pred + at, rows ? targets : targets + at, rows ? rows + k : nullptr, F, Ch, H, W, out + k,
                                         (float *)ws, (hipStream_t)stream));
    }
    return 0;
}

extern "C" size_t orn_msssim_ws_bytes(int B, int Ch, int H, int W)
{
    return B > 0 && Ch > 0 ? orn_msssim_frames_ws_bytes(1, B * Ch, H, W) : 0;
}

// out[0] = ms_ssim(pred, target, data_range=1, size_average=True): one group of B*Ch planes.  Needs min(H, W) > 160
// (pytorch_msssim's own limit).
extern "C" int orn_msssim(const float *pred, const float *target, int B, int Ch, int H, int W, float *out, void *ws,
                          size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(pred && target && out && ws, "msssim: null pointer");
    ORN_REQUIRE(B > 0 && Ch > 0 && B * Ch <= 64, "msssim: bad plane count");
    ORN_REQUIRE((H < W ? H : W) > 160, "msssim: image side must exceed 160 (got %dx%d)", H, W);
    if (ws_bytes < orn_msssim_ws_bytes(B, Ch, H, W)) { orn_set_error("msssim: workspace too small"); return ORN_E_WS; }
    ORN_TRY(orn_loss_init());
    return orn_launch_msssim_frames(pred, target, nullptr, 1, B * Ch, H, W, out, (float *)ws, (hipStream_t)stream);
}

// ---- test entry points (include/orn_debug.h) ----
extern "C" void orn_debug_gauss_taps(float *g11) { orn_gauss_taps(g11); }

extern "C" int orn_debug_msssim_level_fwd_tiles(int H, int W)
{
    if (H < 11 || W < 11) return 0;
    const OrnMsLevel q = ms_level_geom(H, W, false);
    return q.tiles_w * q.tiles_h;
}

extern "C" int orn_debug_msssim_level_fwd(const float *x, const float *y, int planes, int H, int W, float *part, float *nx, float *ny,
                                          void *stream)
{
    ORN_REQUIRE(x && y && part, "debug_msssim_level_fwd: null pointer");
    ORN_REQUIRE((nx != nullptr) == (ny != nullptr), "debug_msssim_level_fwd: nx and ny go together");
    ORN_REQUIRE(planes >= 1 && planes <= 65535, "debug_msssim_level_fwd: bad plane count %d", planes);
    ORN_REQUIRE(H >= 11 && W >= 11 && (long)H * W <= (1L << 26), "debug_msssim_level_fwd: unsupported size %dx%d", H, W);
    ORN_TRY(orn_loss_init());
    OrnMsLevel q = ms_level_geom(H, W, nx != nullptr);
    q.x = x; q.y = y; q.rows = nullptr; q.Ch = planes;
    q.part = part; q.nx = nx; q.ny = ny;
    hipLaunchKernelGGL(k_msssim_level, dim3(q.tiles_w * q.tiles_h, (unsigned)planes), dim3(256), 0, (hipStream_t)stream, q);
    ORN_LAUNCH_CHECK("msssim_level");
    return 0;
}

// orn_launch_loss itself with every argument the engine gives it: the frame table, the device frame index and the cached target maps
extern "C" int orn_debug_loss_launch(const float *pred, const float *frames, const int *frame_idx, size_t frame_stride, int B, int Ch,
                                     int H, int W, int loss_type, float loss_scale, const float *tstats, float *stats, float *dpred,
                                     void *ws, size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(pred && frames && stats && ws, "debug_loss_launch: null pointer");
    ORN_REQUIRE(B > 0 && Ch > 0 && H > 0 && W > 0 && (long)B * Ch <= 65535, "debug_loss_launch: bad sizes");
    const OrnLossSpec *sp = orn_loss_spec_of(loss_type);
    ORN_REQUIRE(sp, "debug_loss_launch: unsupported loss_type %d", loss_type);
    ORN_REQUIRE(sp->kind != ORN_LOSS_KIND_MSSSIM, "debug_loss_launch: loss_type %d is an MS-SSIM loss", loss_type);
    ORN_REQUIRE(!tstats || sp->kind == ORN_LOSS_KIND_SSIM, "debug_loss_launch: only the SSIM kinds read target statistics");
    const size_t need = orn_loss_ws_bytes_for(loss_type, B, Ch, H, W);
    if (ws_bytes < need) {
        orn_set_error("debug_loss_launch: workspace %zu < %zu", ws_bytes, need);
        return ORN_E_WS;
    }
    return orn_launch_loss(pred, frames, frame_idx, frame_stride, B, Ch, H, W, loss_type, loss_scale, stats, dpred, (float *)ws,
                           (hipStream_t)stream, nullptr, nullptr, nullptr, tstats);
}

extern "C" int orn_debug_loss_layout(int B, int Ch, int H, int W, int64_t *out)
{
    ORN_REQUIRE(out, "debug_loss_layout: null pointer");
    ORN_REQUIRE(B > 0 && Ch > 0 && H > 0 && W > 0, "debug_loss_layout: bad sizes");
    const LossGeom g = loss_geom(B, Ch, H, W);
    out[0] = g.tw; out[1] = g.th; out[2] = (int64_t)g.off_pl; out[3] = (int64_t)g.total;
    return 0;
}

extern "C" int orn_debug_loss_msssim_layout(int loss_type, int B, int Ch, int H, int W, int64_t *out)
{
    const OrnLossSpec *sp = orn_loss_spec_of(loss_type);
    ORN_REQUIRE(out, "debug_loss_msssim_layout: null pointer");
    ORN_REQUIRE(sp && sp->kind == ORN_LOSS_KIND_MSSSIM, "debug_loss_msssim_layout: loss_type %d is not an MS-SSIM loss", loss_type);
    ORN_REQUIRE(B > 0 && Ch > 0 && (long)B * Ch <= 64 && (H < W ? H : W) > 160, "debug_loss_msssim_layout: unsupported shape");
    const LossGeom g = loss_geom(B, Ch, H, W);
    const size_t planes = (size_t)g.planes, ms = g.total;      // orn_launch_loss: ms_ws = ws + g.total
    OrnMsLayout ly;
    orn_msssim_layout(planes, H, W, &ly);
    size_t grad[5], coef;
    orn_loss_msssim_layout(planes, H, W, grad, &coef);
    for (int l = 0; l < 5; ++l) {
        int64_t *o = out + 8 * l;
        o[0] = ly.Hs[l]; o[1] = ly.Ws[l];
        o[2] = l ? (int64_t)(ms + ly.pooled[l][0]) : -1; o[3] = l ? (int64_t)(ms + ly.pooled[l][1]) : -1;
        o[4] = (int64_t)(ms + ly.part + ly.part_off[l]); o[5] = ly.nblk[l];
        o[6] = l ? (int64_t)(ms + grad[l]) : -1;
        o[7] = (int64_t)(ms + coef + (size_t)l * planes);
    }
    out[40] = (int64_t)(ms + coef + 5 * planes);
    out[41] = (int64_t)g.off_pl; out[42] = (int64_t)g.tw * g.th;
    out[43] = (int64_t)(orn_loss_ws_bytes_for(loss_type, B, Ch, H, W) / 4);
    return 0;
}
