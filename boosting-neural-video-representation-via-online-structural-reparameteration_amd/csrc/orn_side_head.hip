// Side heads of the multi-resolution generator (model.py:597-625 without sin_res: head_layers[i] = Conv2d(ngf_i, 3, 1) on every
// stage, one image per stage; main_train.py:239-250: loss = sum_{i < n-1} lw * loss_fn(out_i, target_i) + loss_fn(out_{n-1}, ..)).
// A stage below the last one differs from the last in one point: the gradient buffer of its block already holds what the block
// above sent down (dgrad_{i+1}), so the head's backward ADDS its term instead of writing it:
//   da_i = dgrad_{i+1}(dz_{i+1}) + W_head_i^T du_i,   du_i = lw * dLoss_i/dout_i * act'(out_i)
// Two layouts, those a block's output is kept in:
//   16 bit (this file; compiled twice, orn_h16.h): z channels-last [H][W][C] (pre-activation), gradient target the block's dypad --
//     zero-bordered [H/sp + 2][W/sp + 2][C sp^2], un-shuffled, as k_head_bwd_nhwc_bf16 (orn_ops_bf16.hip) writes it.  Any C in 1..512:
//     16-byte loads and stores where C % 8 == 0 and the buffers are 16-byte aligned, element-wise otherwise (both forms add in the
//     same order).
//   fp32 (orn_side_head_f32.hip, built once): a NCHW [C][H][W] (activation), gradient target da NCHW (gradient with respect to the
//     activation: no SiLU' here).  The column sums that finish dW / db (k_side_head_finish) and the size of the partial table, which
//     both layouts share, live there too.
// In the engine a head whose pre-activation u = W a + b is not finite raises the step's flag: tanh and sigmoid would hide it.
// dW / db: per-work-group partial sums in fixed order, then one wave per column over the work-groups, no atomics: run-to-run
// bit-identical.
// Test entry points (include/orn_debug.h): orn_debug.hip, through OrnHalfOps (orn_ops_bf16.hip), as the engine reaches these launchers.
#include "orn_h16.h"

#define SH_CHUNK 128             // 16-bit backward: channels per work-group (blockIdx.y walks the chunks): dW sums live in registers

namespace HNS {

// 4 lanes per pixel; lane `sub` takes the 8-channel groups sub, sub + 4, ... (the last group may be short).  With C % 32 == 0 this is
// the summation order of k_head_fwd_nhwc_bf16.
template <bool VEC, int ACT>
__global__ void __launch_bounds__(256)
k_side_head_fwd_h16(const h16 *__restrict__ z, const float *__restrict__ w, const float *__restrict__ bias, int C, size_t HW, int sigmoid,
                    float *__restrict__ out, OrnScaleState *sc)
{
    __shared__ float sw[3 * SH_MAXC + 3];
    for (int i = threadIdx.x; i < 3 * C; i += 256) sw[i] = w[i];
    if (threadIdx.x < 3) sw[3 * C + threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const int sub = threadIdx.x & 3;
    const size_t pix = (size_t)blockIdx.x * 64 + (threadIdx.x >> 2);
    const bool valid = pix < HW;                      // (all four lanes of a pixel agree; every lane stays for the shuffles)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (valid) {
        const h16 *zp = z + pix * C;
        for (int c0 = sub * 8; c0 < C; c0 += 32) {
            if (VEC) {
                head_accum8<ACT>(*reinterpret_cast<const h16x8 *>(zp + c0), c0, C, sw, a0, a1, a2);
            } else {
                const int ne = C - c0 < 8 ? C - c0 : 8;
                for (int e = 0; e < ne; ++e) {
                    const float a = OrnAct<ACT>::f((float)zp[c0 + e]);
                    a0 = fmaf(sw[c0 + e], a, a0);
                    a1 = fmaf(sw[C + c0 + e], a, a1);
                    a2 = fmaf(sw[2 * C + c0 + e], a, a2);
                }
            }
        }
    }
    head_reduce4(a0, a1, a2);
    if (valid && sub < 3) {
        // (engine) a head that has left the finite range -- tanh and sigmoid would hide it: out = 0 or 1, du = 0 -- skips the step
        orn_flag_nonfinite(sc, (sub == 0 ? a0 : (sub == 1 ? a1 : a2)) + sw[3 * C + sub]);
        out[(size_t)sub * HW + pix] = head_act(a0, a1, a2, sub, C, sw, sigmoid);
    }
}

// Accumulating backward.  gs: the gradient scale dypad carries.  Work-group (x, y): pixels [x * 64 SH_PPT, + 64 SH_PPT),
// channels [y * SH_CHUNK, + SH_CHUNK); NQ = 8-channel groups per lane of that chunk.  partial [gridDim.x][3 C + 3]: dW[k][c] at
// k C + c, db[k] at 3 C + k (written by the work-groups of chunk 0).
template <int NQ, bool VEC, int ACT>
__global__ void __launch_bounds__(256)
k_side_head_bwd_h16(const h16 *__restrict__ z, const float *__restrict__ w, const float *__restrict__ out, const float *__restrict__ dout,
                    int C, int H, int W, int sigmoid, int sp, float lw, float gs, h16 *__restrict__ dypad, float *__restrict__ partial,
                    const OrnScaleState *sc)
{
    if (sc) gs = sc->gs;                             // engine: the scale lives in device memory (dynamic loss scaling)
    const float scale = lw * gs;
    __shared__ float sw[3 * SH_CHUNK];
    __shared__ float sred[4][4][NQ * 24 + 3];
    const int cbase = blockIdx.y * SH_CHUNK;
    const int cc = C - cbase < SH_CHUNK ? C - cbase : SH_CHUNK;       // channels of this chunk
    for (int i = threadIdx.x; i < 3 * cc; i += 256) {
        const int k = i / cc, c = i - k * cc;
        sw[k * SH_CHUNK + c] = w[k * C + cbase + c];
    }
    __syncthreads();
    const int sub = threadIdx.x & 3, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t HW = (size_t)H * W;
    float dwacc[NQ][8][3];
#pragma unroll
    for (int q = 0; q < NQ; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) { dwacc[q][e][0] = 0.f; dwacc[q][e][1] = 0.f; dwacc[q][e][2] = 0.f; }
    float dbacc[3] = {0.f, 0.f, 0.f};
    const int Wp = W / sp + 2;
    const size_t Cp = (size_t)C * sp * sp;
    for (int it = 0; it < SH_PPT; ++it) {
        const size_t pix = ((size_t)blockIdx.x * SH_PPT + it) * 64 + (threadIdx.x >> 2);
        if (pix >= HW) break;                                         // (pixels ascend with `it`; the shuffles come after the loop)
        float du[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float o = out[(size_t)k * HW + pix], g = dout[(size_t)k * HW + pix];
            du[k] = g * scale * (sigmoid ? o * (1.0f - o) : 2.0f * o * (1.0f - o));
            dbacc[k] += du[k];
        }
        const int h = (int)(pix / W), ww = (int)(pix - (size_t)h * W);
        const int ph = h / sp, pw = ww / sp;
        h16 *dst = dypad + ((size_t)(ph + 1) * Wp + (pw + 1)) * Cp + (size_t)((h - ph * sp) * sp + (ww - pw * sp)) * C + cbase;
        const h16 *zp = z + pix * C + cbase;
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int c0 = (q * 4 + sub) * 8;
            if (c0 >= cc) continue;
            const int ne = cc - c0 < 8 ? cc - c0 : 8;                 // (VEC: always 8)
            h16x8 v, d8;
            if (VEC) {
                v = *reinterpret_cast<const h16x8 *>(zp + c0);
                d8 = *reinterpret_cast<const h16x8 *>(dst + c0);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    v[e] = e < ne ? zp[c0 + e] : (h16)0.f;
                    d8[e] = e < ne ? dst[c0 + e] : (h16)0.f;
                }
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (!VEC && e >= ne) continue;
                const float zz = (float)v[e];
                float a;
                // the stored 16-bit value + this head's term, added in fp32 and rounded once
                if constexpr (ACT == ORN_ACT_SWISH) {
                    const float sg = orn_sigmoid(zz);
                    a = zz * sg;
                    const float da = fmaf(sw[2 * SH_CHUNK + c0 + e], du[2], fmaf(sw[SH_CHUNK + c0 + e], du[1], sw[c0 + e] * du[0]));
                    d8[e] = (h16)((float)d8[e] + da * (sg * (1.0f + zz * (1.0f - sg))));
                } else {
                    a = OrnAct<ACT>::f(zz);
                    const float da = fmaf(sw[2 * SH_CHUNK + c0 + e], du[2], fmaf(sw[SH_CHUNK + c0 + e], du[1], sw[c0 + e] * du[0]));
                    d8[e] = (h16)((float)d8[e] + da * OrnAct<ACT>::df(zz));
                }
                dwacc[q][e][0] = fmaf(du[0], a, dwacc[q][e][0]);
                dwacc[q][e][1] = fmaf(du[1], a, dwacc[q][e][1]);
                dwacc[q][e][2] = fmaf(du[2], a, dwacc[q][e][2]);
            }
            if (VEC) {
                *reinterpret_cast<h16x8 *>(dst + c0) = d8;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (e < ne) dst[c0 + e] = d8[e];
            }
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
    for (int i = threadIdx.x; i < 3 * cc; i += 256) {
        const int k = i / cc, c = i - k * cc;
        const int grp = c / 8, e = c - grp * 8, q = grp / 4, sb = grp - q * 4;
        const int ri = (q * 8 + e) * 3 + k;
        pout[k * C + cbase + c] = (sred[0][sb][ri] + sred[1][sb][ri]) + (sred[2][sb][ri] + sred[3][sb][ri]);
    }
    if (blockIdx.y == 0 && threadIdx.x < 3) {
        const int ri = NQ * 24 + threadIdx.x;
        // every sub lane accumulated the same du: take sub 0
        pout[3 * C + threadIdx.x] = (sred[0][0][ri] + sred[1][0][ri]) + (sred[2][0][ri] + sred[3][0][ri]);
    }
}

static int side_head_bwd_blocks_h16(int H, int W) { return orn_cdiv((long)H * W, 64 * SH_PPT); }

static bool side_head_vec(int C, const void *z, const void *dypad)
{
    return C % 8 == 0 && (uintptr_t)z % 16 == 0 && (uintptr_t)dypad % 16 == 0;
}

int orn_launch_side_head_fwd_h16(const h16 *z, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st,
                                 OrnScaleState *sc, int act)
{
    ORN_REQUIRE(orn_act_known(act), "side_head_fwd: unknown activation %d", act);
    ORN_REQUIRE(C >= 1 && C <= SH_MAXC, "side_head_fwd: C=%d outside [1, %d]", C, SH_MAXC);
    ORN_REQUIRE(HW >= 1 && HW <= ((size_t)1 << 30), "side_head_fwd: %zu pixels outside [1, 2^30]", HW);
    const dim3 grid(orn_cdiv((long)HW, 64));
    if (side_head_vec(C, z, nullptr))
        ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_side_head_fwd_h16<true, A>), grid, dim3(256), 0, st, z, w, b, C, HW, sigmoid, out, sc));
    else
        ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_side_head_fwd_h16<false, A>), grid, dim3(256), 0, st, z, w, b, C, HW, sigmoid, out, sc));
    ORN_LAUNCH_CHECK("side_head_fwd");
    return 0;
}

// gs: the gradient scale dypad carries (1 for bf16, the loss scale for fp16; sc, engine: the live scale of the device state instead, and
// non-finite dw / db raise its flag); dw / db are finished un-scaled (lw stays: it is part of the objective)
int orn_launch_side_head_bwd_h16(const h16 *z, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid,
                                 int sp, float lw, float gs, h16 *dypad, float *dw, float *db, float *ws, hipStream_t st, OrnScaleState *sc,
                                 int act)
{
    ORN_REQUIRE(orn_act_known(act), "side_head_bwd: unknown activation %d", act);
    ORN_REQUIRE(C >= 1 && C <= SH_MAXC, "side_head_bwd: C=%d outside [1, %d]", C, SH_MAXC);
    ORN_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W <= ((size_t)1 << 30), "side_head_bwd: bad image size %dx%d", H, W);
    ORN_REQUIRE(sp >= 1 && H % sp == 0 && W % sp == 0, "side_head_bwd: %dx%d not divisible by the stride %d", H, W, sp);
    ORN_REQUIRE(gs > 0.f, "side_head_bwd: gradient scale %g", (double)gs);
    const int blocks = side_head_bwd_blocks_h16(H, W);
    const int cmax = C < SH_CHUNK ? C : SH_CHUNK;
    const int nq = orn_cdiv(orn_cdiv(cmax, 8), 4);                    // 8-channel groups per lane of the widest chunk: 1..4
    const dim3 grid(blocks, orn_cdiv(C, SH_CHUNK));
    const bool vec = side_head_vec(C, z, dypad);
#define SH_LAUNCH(NQ_)                                                                                                                       \
    do {                                                                                                                                     \
        if (vec) ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_side_head_bwd_h16<NQ_, true, A>), grid, dim3(256), 0, st, z, w, out, dout, C, H, W, sigmoid, sp, lw, gs, dypad, ws, sc));  \
        else ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_side_head_bwd_h16<NQ_, false, A>), grid, dim3(256), 0, st, z, w, out, dout, C, H, W, sigmoid, sp, lw, gs, dypad, ws, sc));     \
    } while (0)
    switch (nq) {
    case 1: SH_LAUNCH(1); break;
    case 2: SH_LAUNCH(2); break;
    case 3: SH_LAUNCH(3); break;
    default: SH_LAUNCH(4); break;
    }
#undef SH_LAUNCH
    ORN_LAUNCH_CHECK("side_head_bwd");
    return orn_launch_side_head_finish(ws, blocks, C, 1.0f / gs, dw, db, st, sc, true);
}

}  // namespace HNS
