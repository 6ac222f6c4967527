// A4 fast path, everything around the conv kernels: the 16-bit operand copies of the merged kernels (weight prep), the layout
// converters between fp32 NCHW and padded channels-last 16-bit, the bias gradient, the A5 head (model.py:621-622) forward /
// backward on the channels-last pre-activation of the last block, the type-erased operation table that everything outside the
// twice-built files calls through (OrnHalfOps, one per compiled element type: the engine and the test entry points of orn_debug.hip)
// and the typed per-op C ABI of include/orn.h.  Buffer layouts: orn_conv_bf16.hip.
// Compiled twice (orn_h16.h): bf16 and, with -DORN_FP16, IEEE half.
#include "orn_h16.h"

namespace HNS {

// ================================================================================================
// format helpers
// ================================================================================================
// Wf fp32 [O][C][3][3] -> Wb bf16 [9][O'][C] (o' = (o % s2)*Cn + o / s2), Wd bf16 [9][C][O'] with
// flipped taps (tap' = 8 - tap), bias' [O'].
__global__ void k_prep_weights_bf16(const float *__restrict__ wf, const float *__restrict__ bf, int O, int C, int Cn, int s2,
                                    h16 *__restrict__ wb, h16 *__restrict__ wd, float *__restrict__ bias_p)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (size_t)O) {
        const int o = (int)idx;
        bias_p[(o % s2) * Cn + o / s2] = bf[o];
    }
    if (idx >= (size_t)O * C * 9) return;
    const int tap = (int)(idx % 9);
    const size_t oc = idx / 9;
    const int c = (int)(oc % C), o = (int)(oc / C);
    const int op = (o % s2) * Cn + o / s2;
    const h16 v = (h16)wf[idx];
    wb[((size_t)tap * O + op) * C + c] = v;
    wd[((size_t)(8 - tap) * C + c) * O + op] = v;
}

struct PrepAll {
    int n;
    struct { const float *wf, *bf; int O, C, Cp, Cn, s2; h16 *wb, *wd; float *biasp; } l[ORN_MAX_LAYERS];   // Cp: channel stride
};

// PREP_EPT elements per thread (measured: 1 beats 4 here -- the scattered 2-byte writes, not the dispatcher, bound it)
#define PREP_EPT 1
__global__ void __launch_bounds__(256) k_prep_weights_bf16_all(PrepAll a)
{
    const auto &l = a.l[blockIdx.y];
    const size_t base = (size_t)blockIdx.x * (256 * PREP_EPT) + threadIdx.x;
    const size_t bidx = (size_t)blockIdx.x * 256 + threadIdx.x;     // the grid has >= O / 256 blocks (C * 9 >= PREP_EPT)
    if (bidx < (size_t)l.O) {
        const int o = (int)bidx;
        l.biasp[(o % l.s2) * l.Cn + o / l.s2] = l.bf[o];
    }
    const size_t n = (size_t)l.O * l.C * 9;
#pragma unroll
    for (int i = 0; i < PREP_EPT; ++i) {
        const size_t idx = base + (size_t)i * 256;
        if (idx >= n) return;
        const int tap = (int)(idx % 9);
        const size_t oc = idx / 9;
        const int c = (int)(oc % l.C), o = (int)(oc / l.C);
        const int op = (o % l.s2) * l.Cn + o / l.s2;
        const h16 v = (h16)l.wf[idx];
        l.wb[((size_t)tap * l.O + op) * l.Cp + c] = v;
        l.wd[((size_t)(8 - tap) * l.Cp + c) * l.O + op] = v;
    }
}

int orn_launch_prep_weights_bf16_all(int n, const OrnPrepLayer *L, hipStream_t st)
{
    if (n == 0) return 0;
    PrepAll a;
    a.n = n;
    size_t mx = 0;
    for (int i = 0; i < n; ++i) {
        a.l[i].wf = L[i].wf; a.l[i].bf = L[i].bf; a.l[i].O = L[i].O; a.l[i].C = L[i].C;
        a.l[i].Cp = L[i].Cp > 0 ? L[i].Cp : L[i].C;
        a.l[i].Cn = L[i].O / (L[i].s * L[i].s); a.l[i].s2 = L[i].s * L[i].s;
        a.l[i].wb = (h16 *)L[i].wb; a.l[i].wd = (h16 *)L[i].wd; a.l[i].biasp = L[i].biasp;
        const size_t w = (size_t)L[i].O * L[i].C * 9;
        if (w > mx) mx = w;
    }
    hipLaunchKernelGGL(k_prep_weights_bf16_all, dim3(orn_cdiv((long)mx, 256 * PREP_EPT), n), dim3(256), 0, st, a);
    ORN_LAUNCH_CHECK("prep_weights_bf16_all");
    return 0;
}

int orn_launch_prep_weights_bf16(const float *wf, const float *bf, int O, int C, int s, h16 *wb, h16 *wd, float *bias_p,
                                 hipStream_t st)
{
    hipLaunchKernelGGL(k_prep_weights_bf16, dim3(orn_cdiv((long)O * C * 9, 256)), dim3(256), 0, st, wf, bf, O, C, O / (s * s),
                       s * s, wb, wd, bias_p);
    ORN_LAUNCH_CHECK("prep_weights_bf16");
    return 0;
}

// fp32 NCHW [C][H][W] -> bf16 padded NHWC [H+2][W+2][Cp] interior, channels [0, C) (border and channels >= C stay zero).
// 64-pixel x C tile through LDS: coalesced along pixels on the read, along channels on the write.
#define TR_PX 16
#define TR_MAXC 128
__global__ void __launch_bounds__(256) k_nchw_to_nhwc_pad_bf16(const float *__restrict__ src, int C, int Cp, int H, int W,
                                                              h16 *__restrict__ dst)
{
    __shared__ float tile[TR_MAXC][TR_PX + 1];
    const size_t HW = (size_t)H * W;
    const size_t p0 = (size_t)blockIdx.x * TR_PX;
    for (int idx = threadIdx.x; idx < C * TR_PX; idx += 256) {
        const int c = idx / TR_PX, px = idx - c * TR_PX;
        tile[c][px] = (p0 + px < HW) ? src[(size_t)c * HW + p0 + px] : 0.f;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < C * TR_PX; idx += 256) {
        const int px = idx / C, c = idx - px * C;
        const size_t pix = p0 + px;
        if (pix < HW) {
            const int h = (int)(pix / W), w = (int)(pix - (size_t)h * W);
            dst[((size_t)(h + 1) * (W + 2) + (w + 1)) * Cp + c] = (h16)tile[c][px];
        }
    }
}

// fp32 NHWC slabs [nslab][H][W][Cp] -> fp32 NCHW [C][H][W], C <= Cp (sum over slabs in fixed order), tiled through LDS
__global__ void __launch_bounds__(256) k_nhwc_to_nchw_f32(const float *__restrict__ src, int C, int Cp, int H, int W, int nslab,
                                                         float scale, float *__restrict__ dst, const OrnScaleState *sc)
{
    if (sc) scale = sc->inv_gs;
    __shared__ float tile[TR_MAXC][TR_PX + 1];
    const size_t HW = (size_t)H * W, n = HW * Cp;
    const size_t p0 = (size_t)blockIdx.x * TR_PX;
    for (int idx = threadIdx.x; idx < C * TR_PX; idx += 256) {
        const int px = idx / C, c = idx - px * C;
        float v = 0.f;
        if (p0 + px < HW)
            for (int s = 0; s < nslab; ++s) v += src[(size_t)s * n + (p0 + px) * Cp + c];
        tile[c][px] = v * scale;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < C * TR_PX; idx += 256) {
        const int c = idx / TR_PX, px = idx - c * TR_PX;
        if (p0 + px < HW) dst[(size_t)c * HW + p0 + px] = tile[c][px];
    }
}

int orn_launch_nchw_to_nhwc_pad_bf16(const float *src, int C, int Cp, int H, int W, h16 *dst, hipStream_t st)
{
    ORN_REQUIRE(C <= TR_MAXC && C <= Cp, "nchw_to_nhwc: C=%d > %d or > stride %d", C, TR_MAXC, Cp);
    hipLaunchKernelGGL(k_nchw_to_nhwc_pad_bf16, dim3(orn_cdiv((long)H * W, TR_PX)), dim3(256), 0, st, src, C, Cp, H, W, dst);
    ORN_LAUNCH_CHECK("nchw_to_nhwc_pad_bf16");
    return 0;
}

int orn_launch_nhwc_to_nchw_f32(const float *src, int C, int Cp, int H, int W, int nslab, float scale, float *dst, hipStream_t st,
                                const OrnScaleState *sc = nullptr)
{
    ORN_REQUIRE(C <= TR_MAXC && C <= Cp, "nhwc_to_nchw: C=%d > %d or > stride %d", C, TR_MAXC, Cp);
    hipLaunchKernelGGL(k_nhwc_to_nchw_f32, dim3(orn_cdiv((long)H * W, TR_PX)), dim3(256), 0, st, src, C, Cp, H, W, nslab, scale, dst, sc);
    ORN_LAUNCH_CHECK("nhwc_to_nchw_f32");
    return 0;
}

// ================================================================================================
// A5 head on the channels-last bf16 pre-activation of the last block (model.py:621-622):
//   a = SiLU(z);  u = W a + b;  out = (tanh u + 1)/2 | sigmoid u           out: fp32 NCHW [3][H][W]
// 4 lanes per pixel (C/4 channels each, 16-byte loads), 16 pixels per wave: fully coalesced.
// ================================================================================================
template <int ACT>
__global__ void __launch_bounds__(256)
k_head_fwd_nhwc_bf16(const h16 *__restrict__ z, const float *__restrict__ w, const float *__restrict__ bias, int C, size_t HW,
                     int sigmoid, float *__restrict__ out)
{
    __shared__ float sw[3 * HB_MAXC + 3];
    for (int i = threadIdx.x; i < 3 * C; i += 256) sw[i] = w[i];
    if (threadIdx.x < 3) sw[3 * C + threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const int sub = threadIdx.x & 3;
    const int nq = C / 32;
    // software pipeline (nq <= 4, i.e. C <= 128): the next pixel's z is requested before this pixel's arithmetic
    const size_t pstep = (size_t)gridDim.x * 64;
    size_t pix = (size_t)blockIdx.x * 64 + (threadIdx.x >> 2);
    const bool piped = nq <= 4;
    h16x8 vn[4];
    if (piped && pix < HW) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < nq) vn[q] = *reinterpret_cast<const h16x8 *>(z + pix * C + (q * 4 + sub) * 8);
    }
    for (; pix < HW; pix += pstep) {
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
        h16x8 vc[4];
        if (piped) {
#pragma unroll
            for (int q = 0; q < 4; ++q) vc[q] = vn[q];
            const size_t pnx = pix + pstep;
            if (pnx < HW) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    if (q < nq) vn[q] = *reinterpret_cast<const h16x8 *>(z + pnx * C + (q * 4 + sub) * 8);
            }
        }
        auto proc = [&](const h16x8 v, int c0) { head_accum8<ACT>(v, c0, C, sw, a0, a1, a2); };
        if (piped) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nq) proc(vc[q], (q * 4 + sub) * 8);
        } else {
            for (int q = 0; q < nq; ++q) proc(*reinterpret_cast<const h16x8 *>(z + pix * C + (q * 4 + sub) * 8), (q * 4 + sub) * 8);
        }
        head_reduce4(a0, a1, a2);
        if (sub < 3) out[(size_t)sub * HW + pix] = head_act(a0, a1, a2, sub, C, sw, sigmoid);
    }
}

// Backward: du = dout * act'(out); dz = (W^T du) * SiLU'(z) -> previous-layer dypad layout (bf16);
// dW[k][c] += du[k]*SiLU(z[c]); db[k] += du[k].  partial[blk][3*C+3], reduced afterwards.
template <int NQ, int ACT>
__global__ void __launch_bounds__(256)
k_head_bwd_nhwc_bf16(const h16 *__restrict__ z, const float *__restrict__ w, const float *__restrict__ out,
                     const float *__restrict__ dout, int H, int W, int sigmoid, int sp, float gs_up, h16 *__restrict__ dypad,
                     float *__restrict__ partial, const OrnScaleState *sc, OrnLossFinalJob fin, int nblk)
{
    if ((int)blockIdx.x >= nblk) {                   // rider: the loss's finalize stage (needed by Adam only)
        __shared__ double fsd[3 * 256];
        orn_loss_finalize_block(fin, fsd);
        return;
    }
    if (sc) gs_up = sc->gs;                          // engine: the scale lives in device memory (dynamic loss scaling)
    constexpr int C = NQ * 32;
    __shared__ float sw[3 * C];
    __shared__ float sred[4][4][NQ * 24 + 3];
    for (int i = threadIdx.x; i < 3 * C; i += 256) sw[i] = w[i];
    __syncthreads();
    const int sub = threadIdx.x & 3, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t HW = (size_t)H * W;
    float dwacc[NQ][8][3];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) { dwacc[q][e][0] = 0.f; dwacc[q][e][1] = 0.f; dwacc[q][e][2] = 0.f; }
    float dbacc[3] = {0.f, 0.f, 0.f};
    const int Wp = W / sp + 2, Cp = C * sp * sp;
    // software pipeline: the next pixel's operands (3 x 16 B of z, out / dout) are requested before this pixel's ~500
    // VALU instructions, so each iteration no longer starts with an exposed HBM round trip
    const size_t pstep = (size_t)nblk * 64;
    size_t pix = (size_t)blockIdx.x * 64 + (threadIdx.x >> 2);
    h16x8 vn[NQ];
    float on[3], gn[3];
    if (pix < HW) {
#pragma unroll
        for (int q = 0; q < NQ; ++q) vn[q] = *reinterpret_cast<const h16x8 *>(z + pix * C + (q * 4 + sub) * 8);
#pragma unroll
        for (int k = 0; k < 3; ++k) { on[k] = out[(size_t)k * HW + pix]; gn[k] = dout[(size_t)k * HW + pix]; }
    }
    for (; pix < HW; pix += pstep) {
        h16x8 vc[NQ];
        float du[3];
#pragma unroll
        for (int q = 0; q < NQ; ++q) vc[q] = vn[q];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float o = on[k], g = gn[k];
            du[k] = g * gs_up * (sigmoid ? o * (1.0f - o) : 2.0f * o * (1.0f - o));
            dbacc[k] += du[k];
        }
        const size_t pnx = pix + pstep;
        if (pnx < HW) {
#pragma unroll
            for (int q = 0; q < NQ; ++q) vn[q] = *reinterpret_cast<const h16x8 *>(z + pnx * C + (q * 4 + sub) * 8);
#pragma unroll
            for (int k = 0; k < 3; ++k) { on[k] = out[(size_t)k * HW + pnx]; gn[k] = dout[(size_t)k * HW + pnx]; }
        }
        const int h = (int)(pix / W), ww = (int)(pix - (size_t)h * W);
        const int ph = h / sp, pw = ww / sp;
        h16 *dst = dypad + ((size_t)(ph + 1) * Wp + (pw + 1)) * Cp + ((h - ph * sp) * sp + (ww - pw * sp)) * C;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c0 = (q * 4 + sub) * 8;
            const h16x8 v = vc[q];
            h16x8 o8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float zz = (float)v[e];
                float a;
                if constexpr (ACT == ORN_ACT_SWISH) {
                    const float sg = orn_sigmoid(zz);
                    a = zz * sg;
                    const float da = fmaf(sw[2 * C + c0 + e], du[2], fmaf(sw[C + c0 + e], du[1], sw[c0 + e] * du[0]));
                    o8[e] = (h16)(da * (sg * (1.0f + zz * (1.0f - sg))));
                } else {
                    a = OrnAct<ACT>::f(zz);
                    const float da = fmaf(sw[2 * C + c0 + e], du[2], fmaf(sw[C + c0 + e], du[1], sw[c0 + e] * du[0]));
                    o8[e] = (h16)(da * OrnAct<ACT>::df(zz));
                }
                dwacc[q][e][0] = fmaf(du[0], a, dwacc[q][e][0]);
                dwacc[q][e][1] = fmaf(du[1], a, dwacc[q][e][1]);
                dwacc[q][e][2] = fmaf(du[2], a, dwacc[q][e][2]);
            }
            *reinterpret_cast<h16x8 *>(dst + c0) = o8;
        }
    }
    // reduce over the 16 pixel slots of the wave (lanes with equal sub), fixed butterfly order
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e)
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float v = dwacc[q][e][k];
                v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
                if (lane < 4) sred[wave][sub][(q * 8 + e) * 3 + k] = v;
            }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float v = dbacc[k];
        v += __shfl_xor(v, 4, 64); v += __shfl_xor(v, 8, 64); v += __shfl_xor(v, 16, 64); v += __shfl_xor(v, 32, 64);
        if (lane < 4) sred[wave][sub][NQ * 24 + k] = v;
    }
    __syncthreads();
    float *pout = partial + (size_t)blockIdx.x * (3 * C + 3);
    for (int i = threadIdx.x; i < 3 * C; i += 256) {
        const int k = i / C, c = i - k * C;
        const int grp = c / 8, e = c - grp * 8, q = grp / 4, sb = grp - q * 4;
        const int ri = (q * 8 + e) * 3 + k;
        pout[i] = (sred[0][sb][ri] + sred[1][sb][ri]) + (sred[2][sb][ri] + sred[3][sb][ri]);
    }
    if (threadIdx.x < 3) {
        const int ri = NQ * 24 + threadIdx.x;
        // every sub lane accumulated the same du: take sub 0
        pout[3 * C + threadIdx.x] = (sred[0][0][ri] + sred[1][0][ri]) + (sred[2][0][ri] + sred[3][0][ri]);
    }
}

#define HB_BLOCKS 512

int orn_launch_head_fwd_bf16(const h16 *z, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st, int act)
{
    ORN_REQUIRE(orn_act_known(act), "head_bf16: unknown activation %d", act);
    ORN_REQUIRE(C % 32 == 0 && C <= HB_MAXC, "head_bf16: unsupported C=%d", C);
    int blocks = orn_cdiv((long)HW, 64);
    if (blocks > 8192) blocks = 8192;           // measured: 8192 beats 2048 by ~7 us at 720p
    ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL(k_head_fwd_nhwc_bf16<A>, dim3(blocks), dim3(256), 0, st, z, w, b, C, HW, sigmoid, out));
    ORN_LAUNCH_CHECK("head_fwd_bf16");
    return 0;
}

size_t orn_head_bwd_bf16_ws_floats(int C) { return (size_t)(HB_BLOCKS + 1) * (3 * C + 3); }
int orn_head_bwd_bf16_blocks(int H, int W) { const int b = orn_cdiv((long)H * W, 64); return b > HB_BLOCKS ? HB_BLOCKS : b; }

// gs_up: gradient scale carried by dypad (1 for bf16, 2^20 for fp16); dw/db are un-scaled here
int orn_launch_head_bwd_bf16(const h16 *z, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid,
                             int sp, float gs_up, h16 *dypad, float *dw, float *db, float *ws, hipStream_t st, const OrnScaleState *sc,
                             const OrnLossFinalJob *fin, int act)
{
    ORN_REQUIRE(orn_act_known(act), "head_bwd_bf16: unknown activation %d", act);
    ORN_REQUIRE(orn_head_bwd_c_ok(C), "head_bwd_bf16: unsupported C=%d", C);
    ORN_REQUIRE(H % sp == 0 && W % sp == 0, "head_bwd_bf16: H,W not divisible by stride");
    int blocks = orn_cdiv((long)H * W, 64);
    if (blocks > HB_BLOCKS) blocks = HB_BLOCKS;
    float *partial = ws;
    OrnLossFinalJob fj = {};
    if (fin) fj = *fin;
    const int nfin = (fin && fin->n_l1 > 0) ? 1 : 0;
    switch (C) {
    case 32: ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_head_bwd_nhwc_bf16<1, A>), dim3(blocks + nfin), dim3(256), 0, st, z, w, out, dout, H, W, sigmoid, sp, gs_up, dypad, partial, sc, fj, blocks)); break;
    case 64: ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_head_bwd_nhwc_bf16<2, A>), dim3(blocks + nfin), dim3(256), 0, st, z, w, out, dout, H, W, sigmoid, sp, gs_up, dypad, partial, sc, fj, blocks)); break;
    case 96: ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_head_bwd_nhwc_bf16<3, A>), dim3(blocks + nfin), dim3(256), 0, st, z, w, out, dout, H, W, sigmoid, sp, gs_up, dypad, partial, sc, fj, blocks)); break;
    default: ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_head_bwd_nhwc_bf16<4, A>), dim3(blocks + nfin), dim3(256), 0, st, z, w, out, dout, H, W, sigmoid, sp, gs_up, dypad, partial, sc, fj, blocks)); break;
    }
    ORN_LAUNCH_CHECK("head_bwd_bf16");
    if (!dw) return 0;                  // deferred: rides along orn_launch_wgrad_bf16_batch (OrnHeadFinish)
    return orn_launch_head_finish_bf16(partial, blocks, C, 1.0f / gs_up, dw, db, st);
}

// ---- type-erased operation table for the engine (one per compiled element type) -----------------------
static int a_conv_fwd(const void *xpad, const void *wb, const float *bias_p, int H, int W, int Cin, int O, int s, void *z, void *apad,
                      hipStream_t st, int c_real, int act)
{ return orn_launch_conv_bf16_fwd((const h16 *)xpad, (const h16 *)wb, bias_p, H, W, Cin, O, s, (h16 *)z, (h16 *)apad, st, c_real, act); }
static int a_conv_dgrad(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev, void *dyprev, int sp,
                        float *dx_f32, hipStream_t st, int c_real, int act)
{ return orn_launch_conv_bf16_dgrad((const h16 *)dypad, (const h16 *)wd, H, W, O, C, (const h16 *)zprev, (h16 *)dyprev, sp, dx_f32, st, c_real, act); }
static int a_to_nhwc(const float *src, int C, int Cp, int H, int W, void *dst, hipStream_t st)
{ return orn_launch_nchw_to_nhwc_pad_bf16(src, C, Cp, H, W, (h16 *)dst, st); }
static int a_to_nchw_f32(const float *src, int C, int Cp, int H, int W, int nslab, float scale, float *dst, hipStream_t st, const OrnScaleState *sc)
{ return orn_launch_nhwc_to_nchw_f32(src, C, Cp, H, W, nslab, scale, dst, st, sc); }
static int a_head_fwd(const void *z, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st, int act)
{ return orn_launch_head_fwd_bf16((const h16 *)z, w, b, C, HW, sigmoid, out, st, act); }
static int a_decode_out(const void *z, const float *w, const float *b, int C, size_t HW, int sigmoid, const OrnDecodeOut &o, hipStream_t st, int act)
{ return orn_launch_decode_out_h16((const h16 *)z, w, b, C, HW, sigmoid, o, st, act); }
static int a_head_bwd(const void *z, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid, int sp,
                      float gs_up, void *dypad, float *dw, float *db, float *ws, hipStream_t st, const OrnScaleState *sc, const OrnLossFinalJob *fin,
                      int act)
{ return orn_launch_head_bwd_bf16((const h16 *)z, w, out, dout, C, H, W, sigmoid, sp, gs_up, (h16 *)dypad, dw, db, ws, st, sc, fin, act); }
static int a_side_head_fwd(const void *z, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st, OrnScaleState *sc,
                           int act)
{ return orn_launch_side_head_fwd_h16((const h16 *)z, w, b, C, HW, sigmoid, out, st, sc, act); }
static int a_side_head_bwd(const void *z, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid, int sp, float lw,
                           float gs, void *dypad, float *dw, float *db, float *ws, hipStream_t st, OrnScaleState *sc, int act)
{ return orn_launch_side_head_bwd_h16((const h16 *)z, w, out, dout, C, H, W, sigmoid, sp, lw, gs, (h16 *)dypad, dw, db, ws, st, sc, act); }
static int a_stage_out(const void *z, const float *w, const float *b, int C, size_t HW, int sigmoid, const OrnDecodeOut &o, hipStream_t st, int act)
{ return orn_launch_stage_out_h16((const h16 *)z, w, b, C, HW, sigmoid, o, st, act); }

const OrnHalfOps ops = {a_conv_fwd, a_conv_dgrad, orn_wgrad_bf16_ws_floats, orn_wgrad_bf16_split, orn_launch_wgrad_bf16_batch, orn_launch_wgrad_reduce_all,
                        orn_launch_prep_weights_bf16_all, a_to_nhwc, a_to_nchw_f32, orn_dgrad_f32_slabs, a_head_fwd, orn_head_bwd_bf16_ws_floats,
                        orn_head_bwd_bf16_blocks, a_head_bwd, a_decode_out, a_side_head_fwd, a_side_head_bwd, a_stage_out};

// ================================================================================================
// per-op hooks of include/orn.h: the 16-bit block on PyTorch-layout fp32 tensors (conversions included).  Built in both element
// types: the bf16 build exports orn_*_bf16, the IEEE-half build the orn_*_f16 twins (same arguments, half buffers).  HOOK names
// them; the two _ws_bytes functions have no element type in them and exist once, in the bf16 build.
// ================================================================================================
#ifdef ORN_FP16
#define HOOK(bf16_, f16_) f16_
#else
#define HOOK(bf16_, f16_) bf16_
#endif
// bf16 NHWC [H][W][C] (optionally padded source) -> fp32 NCHW
__global__ void k_nhwc_bf16_to_nchw_f32(const h16 *__restrict__ src, int C, int H, int W, int pad, float *__restrict__ dst)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)C * H * W) return;
    const size_t HW = (size_t)H * W;
    const int c = (int)(idx / HW);
    const size_t pix = idx - (size_t)c * HW;
    const int h = (int)(pix / W), w = (int)(pix - (size_t)h * W);
    dst[idx] = (float)src[((size_t)(h + pad) * (W + 2 * pad) + (w + pad)) * C + c];
}

// fp32 NCHW z, da [Cn][Hs][Ws] -> z bf16 NHWC and dypad = unshuffle(da * SiLU'(z)) (o' order, padded)
template <int ACT>
__global__ void k_make_dy_bf16(const float *__restrict__ z, const float *__restrict__ da, int Cn, int H, int W, int s,
                               h16 *__restrict__ zb, h16 *__restrict__ dypad)
{
    const size_t n = (size_t)Cn * H * s * W * s;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const int Hs = H * s, Ws = W * s;
    const int c = (int)(idx % Cn);
    const size_t pix = idx / Cn;
    const int ow = (int)(pix % Ws), oh = (int)(pix / Ws);
    const size_t src = ((size_t)c * Hs + oh) * Ws + ow;
    const h16 zq = (h16)z[src];
    zb[pix * Cn + c] = zq;
    const int ph = oh / s, pw = ow / s, sub = (oh - ph * s) * s + (ow - pw * s);
    dypad[((size_t)(ph + 1) * (W + 2) + (pw + 1)) * ((size_t)Cn * s * s) + (size_t)sub * Cn + c] =
        (h16)(da[src] * OrnAct<ACT>::df((float)zq));
}

static inline size_t alh(size_t halfs) { return orn_align(halfs * 2) / 2; }

struct Bf16Ws {
    h16 *xpad, *wb, *wd, *zb, *apad, *dypad;
    float *biasp, *slabs, *dxn;
    size_t bytes;
};

// The per-op workspace layout, in one place: the slices of `ws` and their total size (ws == nullptr: the size alone, as layout()
// of orn_engine.hip).
static Bf16Ws carve_bf16(void *ws, int C, int O, int H, int W, int s)
{
    const size_t Hs = (size_t)H * s, Ws = (size_t)W * s, Cn = O / (s * s);
    size_t off = 0;
    auto take = [&](size_t bytes) { void *p = ws ? (unsigned char *)ws + off : nullptr; off += bytes; return p; };
    Bf16Ws r;
    r.xpad = (h16 *)take(alh((size_t)(H + 2) * (W + 2) * C) * 2);
    r.wb = (h16 *)take(alh((size_t)9 * O * C + 96 * C) * 2);                 // (+ the rows a ragged last N tile reads past the end)
    r.wd = (h16 *)take(alh((size_t)9 * O * C + 96 * C) * 2);
    r.biasp = (float *)take(orn_align((size_t)O * 4));
    r.zb = (h16 *)take(alh(Hs * Ws * Cn) * 2);
    r.apad = (h16 *)take(alh((Hs + 2) * (Ws + 2) * Cn) * 2);
    r.dypad = (h16 *)take(alh((size_t)(H + 2) * (W + 2) * O + 128) * 2);     // (+ what a ragged last wgrad tile reads past the end)
    r.slabs = (float *)take(orn_align(orn_wgrad_bf16_ws_floats(H, W, O) * 4));
    r.dxn = (float *)take(orn_align((size_t)H * W * C * 4 * 8));             // dx fp32 NHWC (up to 8 chunk slabs)
    r.bytes = off;
    return r;
}

#ifdef ORN_FP16
extern "C" size_t orn_conv3x3_ps_silu_bf16_ws_bytes(int C, int O, int H, int W, int s);     // element size is the same: one definition
#else
extern "C" size_t orn_conv3x3_ps_silu_bf16_ws_bytes(int C, int O, int H, int W, int s) { return carve_bf16(nullptr, C, O, H, W, s).bytes; }
#endif

// Same contract as orn_conv3x3_ps_silu_fwd (B = 1) but computed on the bf16 MFMA path.
// `ws` must be zero-filled by the caller before the first use (the padded borders are never written).
extern "C" int HOOK(orn_conv3x3_ps_silu_fwd_bf16_act, orn_conv3x3_ps_silu_fwd_f16_act)(const float *x, const float *wf, const float *bf, int C, int O, int H, int W,
                                            int s, float *z, float *a, void *ws, size_t ws_bytes, void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "conv3x3_ps_silu_fwd_bf16: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    ORN_REQUIRE(x && wf && bf && (z || a) && ws, "conv3x3_ps_silu_fwd_bf16: null pointer");   // a == NULL: the last block's form (z only)
    ORN_REQUIRE(C % CB_CK == 0 && O % 32 == 0 && O % (s * s) == 0, "conv3x3_ps_silu_fwd_bf16: unsupported C=%d O=%d s=%d", C, O, s);
    if (ws_bytes < orn_conv3x3_ps_silu_bf16_ws_bytes(C, O, H, W, s)) { orn_set_error("conv3x3_ps_silu_fwd_bf16: workspace too small"); return ORN_E_WS; }
    hipStream_t st = (hipStream_t)stream;
    const Bf16Ws b = carve_bf16(ws, C, O, H, W, s);
    const int Cn = O / (s * s), Hs = H * s, Ws = W * s;
    ORN_TRY(orn_launch_nchw_to_nhwc_pad_bf16(x, C, C, H, W, b.xpad, st));
    ORN_TRY(orn_launch_prep_weights_bf16(wf, bf, O, C, s, b.wb, b.wd, b.biasp, st));
    ORN_TRY(orn_launch_conv_bf16_fwd(b.xpad, b.wb, b.biasp, H, W, C, O, s, b.zb, a ? b.apad : nullptr, st, C, act));
    const long n = (long)Cn * Hs * Ws;
    if (z) hipLaunchKernelGGL(k_nhwc_bf16_to_nchw_f32, dim3(orn_cdiv(n, 256)), dim3(256), 0, st, b.zb, Cn, Hs, Ws, 0, z);
    if (a) hipLaunchKernelGGL(k_nhwc_bf16_to_nchw_f32, dim3(orn_cdiv(n, 256)), dim3(256), 0, st, b.apad, Cn, Hs, Ws, 1, a);
    ORN_LAUNCH_CHECK("nhwc_bf16_to_nchw_f32");
    return 0;
}
extern "C" int HOOK(orn_conv3x3_ps_silu_fwd_bf16, orn_conv3x3_ps_silu_fwd_f16)(const float *x, const float *wf, const float *bf, int C, int O, int H, int W,
                                            int s, float *z, float *a, void *ws, size_t ws_bytes, void *stream)
{
    return HOOK(orn_conv3x3_ps_silu_fwd_bf16_act, orn_conv3x3_ps_silu_fwd_f16_act)(x, wf, bf, C, O, H, W, s, z, a, ws, ws_bytes, stream, ORN_ACT_SWISH);
}

extern "C" int HOOK(orn_conv3x3_ps_silu_bwd_bf16_act, orn_conv3x3_ps_silu_bwd_f16_act)(const float *x, const float *wf, const float *z, const float *da, int C, int O,
                                            int H, int W, int s, float *dx, float *dwf, float *dbf, void *ws,
                                            size_t ws_bytes, void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "conv3x3_ps_silu_bwd_bf16: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    ORN_REQUIRE(x && wf && z && da && dwf && dbf && ws, "conv3x3_ps_silu_bwd_bf16: null pointer");
    ORN_REQUIRE(C == 96 && O % 96 == 0 && O % (s * s) == 0, "conv3x3_ps_silu_bwd_bf16: unsupported C=%d O=%d", C, O);
    if (ws_bytes < orn_conv3x3_ps_silu_bf16_ws_bytes(C, O, H, W, s)) { orn_set_error("conv3x3_ps_silu_bwd_bf16: workspace too small"); return ORN_E_WS; }
    hipStream_t st = (hipStream_t)stream;
    const Bf16Ws b = carve_bf16(ws, C, O, H, W, s);
    const int Cn = O / (s * s);
    ORN_TRY(orn_launch_nchw_to_nhwc_pad_bf16(x, C, C, H, W, b.xpad, st));
    ORN_TRY(orn_launch_prep_weights_bf16(wf, dbf /*scratch: overwritten below*/, O, C, s, b.wb, b.wd, b.biasp, st));
    const long n = (long)Cn * H * s * W * s;
    ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL(k_make_dy_bf16<A>, dim3(orn_cdiv(n, 256)), dim3(256), 0, st, z, da, Cn, H, W, s, b.zb, b.dypad));
    ORN_LAUNCH_CHECK("make_dy_bf16");
    ORN_TRY(orn_launch_wgrad_bf16(b.xpad, b.dypad, H, W, C, O, s, 1.0f, b.slabs, dwf, dbf, st));
    if (dx) {
        ORN_TRY(orn_launch_conv_bf16_dgrad(b.dypad, b.wd, H, W, O, C, nullptr, nullptr, 1, b.dxn, st, C, act));   // (fp32 slabs: no activation in it)
        ORN_TRY(orn_launch_nhwc_to_nchw_f32(b.dxn, C, C, H, W, orn_dgrad_f32_slabs(H, W, O), 1.0f, dx, st));
    }
    return 0;
}
extern "C" int HOOK(orn_conv3x3_ps_silu_bwd_bf16, orn_conv3x3_ps_silu_bwd_f16)(const float *x, const float *wf, const float *z, const float *da, int C, int O,
                                            int H, int W, int s, float *dx, float *dwf, float *dbf, void *ws,
                                            size_t ws_bytes, void *stream)
{
    return HOOK(orn_conv3x3_ps_silu_bwd_bf16_act, orn_conv3x3_ps_silu_bwd_f16_act)(x, wf, z, da, C, O, H, W, s, dx, dwf, dbf, ws, ws_bytes, stream,
                                                                                   ORN_ACT_SWISH);
}

// Raw channels-last entry points (the engine's own layouts; used by bench.py's roofline leg).
extern "C" int HOOK(orn_conv_nhwc_bf16_fwd, orn_conv_nhwc_f16_fwd)(const void *xpad, const void *wb, const float *bias_p, int H, int W, int C, int O,
                                      int s, void *z, void *apad, void *stream)
{
    ORN_REQUIRE(xpad && wb && z, "conv_nhwc_bf16_fwd: null pointer");
    return orn_launch_conv_bf16_fwd((const h16 *)xpad, (const h16 *)wb, bias_p, H, W, C, O, s, (h16 *)z, (h16 *)apad,
                                    (hipStream_t)stream, C, ORN_ACT_SWISH);      // the raw entry is the swish form (include/orn.h)
}

extern "C" int HOOK(orn_wgrad_nhwc_bf16, orn_wgrad_nhwc_f16)(const void *xpad, const void *dypad, int H, int W, int C, int O, int s, float *slabs,
                                   float *dwf, float *dbf, void *stream)
{
    return orn_launch_wgrad_bf16((const h16 *)xpad, (const h16 *)dypad, H, W, C, O, s, 1.0f, slabs, dwf, dbf, (hipStream_t)stream);
}
#ifndef ORN_FP16
extern "C" size_t orn_wgrad_nhwc_bf16_ws_bytes(int H, int W, int O) { return orn_wgrad_bf16_ws_floats(H, W, O) * 4; }
#endif
extern "C" int HOOK(orn_dgrad_nhwc_bf16, orn_dgrad_nhwc_f16)(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev,
                                   void *dyprev, int sp, void *stream)
{
    return orn_launch_conv_bf16_dgrad((const h16 *)dypad, (const h16 *)wd, H, W, O, C, (const h16 *)zprev, (h16 *)dyprev, sp,
                                      nullptr, (hipStream_t)stream, C, ORN_ACT_SWISH);      // the raw entry is the swish form (include/orn.h)
}

}  // namespace HNS

const OrnHalfOps *
#ifdef ORN_FP16
orn_half_ops_f16()
#else
orn_half_ops_bf16()
#endif
{
    return &HNS::ops;
}
