// The MS-SSIM losses of loss_fn (utils.py:167-172: Fusion10 / 11 / 12 = a * L1 + b * (1 - ms_ssim)) with their gradient.
//   forward : the five k_msssim_level launches of orn_loss.hip on the step's planes (one group of B*Ch planes); the pooled pred /
//             target planes of levels 1..4 and the per-tile {ssim, cs} partials stay in the workspace
//   k_msssim_coef      : per plane the five level means v_l (orn_msssim_level_mean, which k_msssim_frames_finalize calls too: the
//                        value equals orn_msssim's on the same pair), P = prod relu(v_l)^w_l, the MS-SSIM value, and
//                        k[l][plane] = -w_struct * loss_scale * w_l * P / v_l / planes / nmap_l (0 where v_l <= 0)
//   k_msssim_level_bwd : levels 4, 3, 2, 1, 0.  g_l = k[l] * (G^T dm + 2 x G^T dq + y G^T dr) + avg-pool adjoint of g_{l+1}, where
//                        dm / dq / dr are the derivatives of level l's map (CS at 0..3, SSIM at 4) with respect to the filtered
//                        G*x, G*x^2, G*xy.  A work-group owns a 16x64 tile of g_l and recomputes the five filtered maps on the tile
//                        plus a 20-pixel apron in LDS through the functions of orn_ssim_tile.h, as k_fusion6 (orn_loss.hip) does for
//                        one level with the SSIM map.  Level 0 adds the L1 / L2 term, writes dpred and the {|d|, d^2} tile partials.
// No atomics, fixed-order sums: run-to-run bit-identical.  Levels shrink to 45x80 at 720p and 11x12 at the smallest legal size:
// every load is bounds-checked against the level's own H x W and everything outside is zero, as the valid filter's adjoint needs.
#include "orn_ssim_tile.h"

struct MsBwdP {
    const float *x, *y;            // this level's pred / target planes [planes][H][W]
    const int *frame_idx;          // level 0, optional: the target is y + *frame_idx * frame_stride
    size_t frame_stride;
    int H, W, Hv, Wv, tiles_w;
    int vec4;                      // orn_loss_vec4
    const float *k;                // [planes] this level's coefficients
    const float *gnext;            // level l+1's gradient [planes][Ho][Wo]; null at level 4
    int Ho, Wo, ph, pw;
    float *g;                      // level l's gradient [planes][H][W] (level 0: dpred; null with GRAD false)
    float g_l1, g_l2;              // level 0: pixel-term scales
    float *part_l1;                // level 0: [planes * tiles][2]
};

enum { MS_CS = 0, MS_SSIM = 1 };
// KIND: which map's derivatives; LAST: level 0; GRAD false (level 0 only): the {|d|, d^2} partials alone
template <int KIND, bool LAST, bool GRAD>
__global__ void __launch_bounds__(256) k_msssim_level_bwd(MsBwdP q)
{
    extern __shared__ __attribute__((aligned(16))) float mls[];
    float *Xp = mls, *Xt = mls + ST_PH * ST_PWP;
    float *Hm = mls + 2 * ST_PH * ST_PWP;
    float *Dm = mls;                       // written after the last read of Xp / Xt
    float *Hh = Hm;                        // written after the last read of Hm
    float *sred = mls + 2 * ST_PH * ST_PWP + 5 * ST_PH * ST_DWP;
    const int t = threadIdx.x;
    const int plane = blockIdx.y;
    const int tw = blockIdx.x % q.tiles_w, th = blockIdx.x / q.tiles_w;
    const int y0 = th * ST_TH, x0 = tw * ST_TW;
    const size_t HW = (size_t)q.H * q.W;
    const float *tp = q.y + (q.frame_idx ? (size_t)(*q.frame_idx) * q.frame_stride : 0) + (size_t)plane * HW;
    const float *pp = q.x + (size_t)plane * HW;
    if (GRAD) {
        st_load_patch(Xp, Xt, pp, tp, y0, x0, q.H, q.W, q.vec4, t);
        __syncthreads();
        st_row_filter<true, true>(Xp, Xt, Hm, t);
        __syncthreads();
        // ---- column filter + derivative maps; item = (column j, 9 rows from r4)
        if (t < 3 * ST_DWP) {
            const int rg = t / ST_DWP, j = t - rg * ST_DWP, r4 = rg == 2 ? 17 : rg * ST_RPT;
            float v[5][ST_RPT];
#pragma unroll
            for (int m = 0; m < 5; ++m) st_col_filter(Hm, m, r4, j, v[m]);
#pragma unroll
            for (int o = 0; o < ST_RPT; ++o) {
                const int i = r4 + o;
                const int vy = y0 - 10 + i, vx = x0 - 10 + j;
                float dm = 0.f, dq = 0.f, dr = 0.f;
                if (vy >= 0 && vy < q.Hv && vx >= 0 && vx < q.Wv && j < ST_TW + 10)
                    st_deriv<KIND == MS_SSIM>(v[0][o], v[1][o], v[2][o], v[3][o], v[4][o], dm, dq, dr);
                st_store_deriv(Dm, i, j, dm, dq, dr);
            }
        }
    }
    // this thread's four output pixels (last phase) are requested before the two adjoint passes
    const int fc = t & (ST_TW - 1), fr4 = (t >> 6) * 4;
    float fp[4], ft[4], gn[4];
    const float kl = GRAD ? q.k[plane] : 0.f;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int cy = min(y0 + fr4 + o, q.H - 1), cx = min(x0 + fc, q.W - 1);
        const size_t oo = (size_t)cy * q.W + cx;
        fp[o] = pp[oo]; ft[o] = tp[oo];
        // adjoint of avg_pool2d(2, padding = size % 2, count_include_pad): every pixel feeds exactly one pooled pixel, weight 1/4
        gn[o] = (GRAD && q.gnext) ? q.gnext[(size_t)plane * q.Ho * q.Wo + (size_t)((cy + q.ph) >> 1) * q.Wo + ((cx + q.pw) >> 1)] : 0.f;
    }
    float am[4] = {0, 0, 0, 0}, aq[4] = {0, 0, 0, 0}, ar[4] = {0, 0, 0, 0};
    if (GRAD) {
        __syncthreads();
        st_adj_row(Dm, Hh, t);
        __syncthreads();
        st_adj_col(Hh, fr4, fc, am, aq, ar);
    }
    float sabs = 0.f, ssq = 0.f;
    const int gx = x0 + fc;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = y0 + fr4 + o;
        if (gy >= q.H || gx >= q.W) continue;
        const size_t oo = (size_t)gy * q.W + gx;
        const float p = fp[o], tg = ft[o], d = p - tg;
        if (LAST) { sabs += fabsf(d); ssq = fmaf(d, d, ssq); }
        if (GRAD) {
            float g = fmaf(kl, am[o] + 2.f * p * aq[o] + tg * ar[o], 0.25f * gn[o]);
            if (LAST) g += fmaf(q.g_l2, d, q.g_l1 * ((d > 0.f) ? 1.f : ((d < 0.f) ? -1.f : 0.f)));
            q.g[(size_t)plane * HW + oo] = g;
        }
    }
    if (LAST) {
        const float ta = orn_block_sum(sabs, sred);
        const float tq = orn_block_sum(ssq, sred);
        if (t == 0) {
            const size_t bi = (size_t)plane * gridDim.x + blockIdx.x;
            q.part_l1[2 * bi] = ta;
            q.part_l1[2 * bi + 1] = tq;
        }
    }
}

// One work-group, one thread per plane (planes <= 64).  The level means and their product as k_msssim_frames_finalize forms them
// (orn_loss.hip): orn_msssim_level_mean, pow in double, the planes summed in plane order.
struct MsCoefP {
    const float *part; size_t part_off[5]; int nblk[5]; float nmap[5];
    int planes; float w_scaled;      // w_struct * loss_scale
    float *k;                        // [5][planes]
    float *val;                      // the MS-SSIM value (mean over the planes)
};
__global__ void __launch_bounds__(64) k_msssim_coef(MsCoefP q)
{
    __shared__ double acc[64];
    const int pl = threadIdx.x;
    const bool live = pl < q.planes;
    double prod = 1.0, v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0, v4 = 0.0;
    if (live) {
#pragma unroll
        for (int lv = 0; lv < 5; ++lv) {
            const double v = orn_msssim_level_mean(q.part + q.part_off[lv], (size_t)pl, q.nblk[lv], q.nmap[lv], lv);
            prod *= pow(v > 0.0 ? v : 0.0, (double)c_ms_weights[lv]);
            if (lv == 0) v0 = v; else if (lv == 1) v1 = v; else if (lv == 2) v2 = v; else if (lv == 3) v3 = v; else v4 = v;
        }
    }
    acc[pl] = live ? prod : 0.0;
    __syncthreads();
    if (pl == 0) {
        double s = 0.0;
        for (int i = 0; i < q.planes; ++i) s += acc[i];
        *q.val = (float)(s / q.planes);
    }
    if (live) {
#pragma unroll
        for (int lv = 0; lv < 5; ++lv) {
            const double v = lv == 0 ? v0 : (lv == 1 ? v1 : (lv == 2 ? v2 : (lv == 3 ? v3 : v4)));
            const double c = -(double)q.w_scaled * (double)c_ms_weights[lv] * prod / v / (double)q.planes / (double)q.nmap[lv];
            q.k[(size_t)lv * q.planes + pl] = v > 0.0 ? (float)c : 0.f;
        }
    }
}

// Must be called once outside any graph capture (orn_ssim_tile_init).
int orn_loss_msssim_init()
{
    return orn_ssim_tile_init({(const void *)k_msssim_level_bwd<MS_SSIM, false, true>, (const void *)k_msssim_level_bwd<MS_CS, false, true>,
                               (const void *)k_msssim_level_bwd<MS_CS, true, true>, (const void *)k_msssim_level_bwd<MS_CS, true, false>});
}

// floats behind the pyramid of the forward: the gradient planes of levels 1..4, then the coefficients [5][planes] and the value
// (as float offsets from the start of the region)
static size_t ms_loss_floats(size_t planes, int H, int W, size_t grad[5], size_t *kbuf)
{
    int Hs[5], Ws[5];
    orn_msssim_geom(H, W, Hs, Ws);
    size_t f = orn_align(orn_msssim_pyramid_floats(planes, H, W) * 4) / 4;
    for (int l = 1; l < 5; ++l) {
        if (grad) grad[l] = f;
        f += orn_align(planes * Hs[l] * Ws[l] * 4) / 4;
    }
    if (kbuf) *kbuf = f;
    return f + orn_align((5 * planes + 1) * 4) / 4;
}

size_t orn_loss_msssim_ws_floats(size_t planes, int H, int W) { return ms_loss_floats(planes, H, W, nullptr, nullptr); }

void orn_loss_msssim_layout(size_t planes, int H, int W, size_t grad[5], size_t *coef)
{
    grad[0] = 0;
    ms_loss_floats(planes, H, W, grad, coef);
}

// One backward launch's geometry in the kernel's argument: the level's planes and sizes, the 16x64 tiling of the IMAGE (*grid), the
// float4 load path's condition and, where a level above feeds in (pool), its size and padding.  The caller adds k, gnext, g, the
// pixel-term scales and part_l1.  orn_launch_loss_msssim and orn_debug_msssim_level_bwd both come through here.
static MsBwdP ms_bwd_geom(const float *x, const float *y, const int *frame_idx, size_t frame_stride, int H, int W, bool pool, int planes,
                          dim3 *grid)
{
    MsBwdP q = {};
    q.x = x; q.y = y;
    q.frame_idx = frame_idx; q.frame_stride = frame_stride;
    q.H = H; q.W = W; q.Hv = H - 10; q.Wv = W - 10;
    q.tiles_w = orn_cdiv(W, ST_TW);
    q.vec4 = orn_loss_vec4(W, (uintptr_t)x | (uintptr_t)y, frame_stride, frame_idx) ? 1 : 0;
    if (pool) { q.Ho = orn_msssim_pooled(H); q.Wo = orn_msssim_pooled(W); q.ph = H % 2; q.pw = W % 2; }
    *grid = dim3(q.tiles_w * orn_cdiv(H, ST_TH), planes);
    return q;
}

// form: 0 SSIM map (level 4), 1 CS map (levels 3..1), 2 CS map at level 0 with the gradient, 3 level 0, the partials alone
static int ms_bwd_launch(int form, const MsBwdP &q, dim3 gr, hipStream_t st)
{
    const dim3 bl(256);
    const size_t lds = ST_LDS_FLOATS * 4;
    if (form == 0) hipLaunchKernelGGL((k_msssim_level_bwd<MS_SSIM, false, true>), gr, bl, lds, st, q);
    else if (form == 1) hipLaunchKernelGGL((k_msssim_level_bwd<MS_CS, false, true>), gr, bl, lds, st, q);
    else if (form == 2) hipLaunchKernelGGL((k_msssim_level_bwd<MS_CS, true, true>), gr, bl, lds, st, q);
    else hipLaunchKernelGGL((k_msssim_level_bwd<MS_CS, true, false>), gr, bl, lds, st, q);
    ORN_LAUNCH_CHECK("msssim_level_bwd");
    return 0;
}

// 5 + 1 + 5 launches (forward only: 5 + 1 + 1).  The callers have checked min(H, W) > 160, planes <= 64 and the workspace.
int orn_launch_loss_msssim(const float *pred, const float *target, const int *frame_idx, size_t frame_stride, int planes, int H, int W,
                           float g_l1, float g_l2, float w_struct_scaled, float *dpred, float *part_l1, float *ms_ws, hipStream_t st,
                           const float **ms_val)
{
    ORN_REQUIRE((uintptr_t)ms_ws % 16 == 0, "loss_msssim: workspace must be 16-byte aligned");
    OrnMsPyramid py;
    // one group of `planes` planes; with a frame index the group's target is row *frame_idx of the frame table
    ORN_TRY(orn_launch_msssim_levels(pred, target, frame_idx, 1, planes, H, W, ms_ws, st, &py));
    size_t goff[5] = {}, koff = 0;
    ms_loss_floats((size_t)planes, H, W, goff, &koff);
    float *grad[5] = {}, *kbuf = ms_ws + koff;
    for (int l = 1; l < 5; ++l) grad[l] = ms_ws + goff[l];
    MsCoefP c;
    c.part = py.part;
    for (int l = 0; l < 5; ++l) { c.part_off[l] = py.part_off[l]; c.nblk[l] = py.nblk[l]; c.nmap[l] = py.nmap[l]; }
    c.planes = planes; c.w_scaled = w_struct_scaled; c.k = kbuf; c.val = kbuf + 5 * (size_t)planes;
    hipLaunchKernelGGL(k_msssim_coef, dim3(1), dim3(64), 0, st, c);
    ORN_LAUNCH_CHECK("msssim_coef");
    *ms_val = c.val;
    for (int l = dpred ? 4 : 0; l >= 0; --l) {
        dim3 gr;
        MsBwdP q = ms_bwd_geom(l ? py.pooled[l][0] : pred, l ? py.pooled[l][1] : target, l ? nullptr : frame_idx, frame_stride,
                               py.Hs[l], py.Ws[l], l < 4, planes, &gr);
        q.k = kbuf + (size_t)l * planes;
        if (l < 4) q.gnext = grad[l + 1];
        q.g = l ? grad[l] : dpred;
        q.g_l1 = g_l1; q.g_l2 = g_l2; q.part_l1 = part_l1;
        ORN_TRY(ms_bwd_launch(l == 4 ? 0 : (l > 0 ? 1 : (dpred ? 2 : 3)), q, gr, st));
    }
    return 0;
}

extern "C" int orn_debug_msssim_level_bwd_tiles(int H, int W)
{
    if (H < 11 || W < 11) return 0;
    dim3 gr;
    ms_bwd_geom(nullptr, nullptr, nullptr, 0, H, W, false, 1, &gr);
    return (int)gr.x;
}

extern "C" int orn_debug_msssim_level_bwd(int form, const float *x, const float *y, const float *k, const float *gnext,
                                          const int *frame_idx, size_t frame_stride, int planes, int H, int W, float g_l1, float g_l2,
                                          float *g, float *part_l1, void *stream)
{
    ORN_REQUIRE(form >= 0 && form <= 3, "debug_msssim_level_bwd: form %d is not one of 0..3", form);
    ORN_REQUIRE(x && y, "debug_msssim_level_bwd: null pointer");
    ORN_REQUIRE(planes >= 1 && planes <= 65535, "debug_msssim_level_bwd: bad plane count %d", planes);
    ORN_REQUIRE(H >= 11 && W >= 11 && (long)H * W <= (1L << 26), "debug_msssim_level_bwd: unsupported size %dx%d", H, W);
    ORN_REQUIRE(form == 3 || (k && g), "debug_msssim_level_bwd: forms 0..2 need k and g");
    ORN_REQUIRE(form < 2 || part_l1, "debug_msssim_level_bwd: the level-0 forms need part_l1");
    ORN_REQUIRE(form >= 2 || !frame_idx, "debug_msssim_level_bwd: only the level-0 forms take a frame index");
    ORN_TRY(orn_loss_msssim_init());
    dim3 gr;
    MsBwdP q = ms_bwd_geom(x, y, frame_idx, frame_stride, H, W, gnext != nullptr, planes, &gr);
    q.k = k; q.gnext = gnext; q.g = g;
    q.g_l1 = g_l1; q.g_l2 = g_l2; q.part_l1 = form >= 2 ? part_l1 : nullptr;
    return ms_bwd_launch(form, q, gr, (hipStream_t)stream);
}
