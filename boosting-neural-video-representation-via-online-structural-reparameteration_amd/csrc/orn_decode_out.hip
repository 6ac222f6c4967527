// Decode output stage (orn_engine_decode_frames, include/orn.h): the end of the network as pixels and PSNR instead of an fp32
// image -- what main_eval.py:795-815 / main_train.py:377-438 do per frame with torch ops (x*255 + 0.5, clamp, uint8, HWC; psnr_fn).
//   16-bit engines: ONE kernel reads the last block's channels-last pre-activation z [H*W][C] (the only large operand: 177 MB per
//     720p frame), applies SiLU + the 1x1 head + (tanh+1)/2 | sigmoid with the arithmetic of k_head_fwd_nhwc_bf16 (orn_h16.h:
//     head_accum8 / head_reduce4 / head_act, so the fp32 value is bit-identical to orn_engine_decode's), and per pixel optionally stores the
//     three fp32 planes, three interleaved bytes, and accumulates the squared error of the value and of its byte / 255 against the
//     target pixel.  LDS-free streaming apart from the head's weights: 16-byte loads, 4 lanes per pixel, 16 pixels per wave.
//   fp32 engines: the fp32 head writes its planar image as before; k_decode_out_planar (orn_decode_out_f32.hip, built once) does the
//     same output stage from it, with the quantisation and the error sums of orn_decode_out.h.
// Bytes: a wave's 16 (64) pixels are 48 (192) contiguous bytes; where that run starts on a 4-byte boundary and is complete the
// wave gathers whole dwords with lane shuffles and stores those, else every lane stores its own bytes.
// Error sums: per-lane fp32, a fixed-order tree per work-group, per-block partials, and the LAST work-group to arrive (an integer
// ticket) sums the partials in fixed order in double: no float atomics, run-to-run bit-identical.
//   side stages (orn_engine_eval_stages): k_stage_out_nhwc, the same stage behind the head of a block below the last (any C in 1..512).
// Compiled twice (orn_h16.h): the two typed kernels and their launchers, nothing else.  Test entry points (include/orn_debug.h):
// orn_debug.hip, through OrnHalfOps::stage_out.
#include "orn_h16.h"
#include "orn_decode_out.h"

namespace HNS {

template <int ACT>
__global__ void __launch_bounds__(256)
k_decode_out_nhwc(const h16 *__restrict__ z, const float *__restrict__ w, const float *__restrict__ bias, int C, size_t HW, int sigmoid,
                  OrnDecodeOut o)
{
    __shared__ float sw[3 * HB_MAXC + 3];
    __shared__ double sd[512];
    __shared__ float sf[16];
    for (int i = threadIdx.x; i < 3 * C; i += 256) sw[i] = w[i];
    if (threadIdx.x < 3) sw[3 * C + threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, sub = threadIdx.x & 3;
    const int nq = C / 32;                                      // <= 4 (launcher)
    const float *tgt = o.stats ? o.targets + (size_t)(*o.row) * 3 * HW : nullptr;
    float ef = 0.f, eq = 0.f;
    // wave-uniform loop over runs of 16 pixels (the byte gather below shuffles across the pixels of a wave); the next run's z is
    // requested before this run's arithmetic, as in k_head_fwd_nhwc_bf16
    const size_t pstep = (size_t)gridDim.x * 64;
    size_t wp = (size_t)blockIdx.x * 64 + (size_t)(threadIdx.x >> 6) * 16;
    h16x8 vn[4] = {};
    if (wp + (lane >> 2) < HW) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < nq) vn[q] = *reinterpret_cast<const h16x8 *>(z + (wp + (lane >> 2)) * C + (q * 4 + sub) * 8);
    }
    for (; wp < HW; wp += pstep) {
        const size_t pix = wp + (lane >> 2);
        const bool valid = pix < HW;
        h16x8 vc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) vc[q] = vn[q];
        const size_t pnx = pix + pstep;
        if (pnx < HW) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nq) vn[q] = *reinterpret_cast<const h16x8 *>(z + pnx * C + (q * 4 + sub) * 8);
        }
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (q < nq) head_accum8<ACT>(vc[q], (q * 4 + sub) * 8, C, sw, a0, a1, a2);
        head_reduce4(a0, a1, a2);
        const float v = sub < 3 ? head_act(a0, a1, a2, sub, C, sw, sigmoid) : 0.f;
        const unsigned qv = sub < 3 ? orn_quant8(v) : 0u;
        const bool mine = valid && sub < 3;
        if (mine && o.img) o.img[(size_t)sub * HW + pix] = v;
        if (mine && tgt) {
            const float tv = tgt[(size_t)sub * HW + pix];
            const float df = v - tv, dq = (float)qv / 255.0f - tv;
            ef += df * df;
            eq += dq * dq;
        }
        if (o.rgb8) {
            uint8_t *run = o.rgb8 + wp * 3;                     // this wave's 48 bytes: byte b = channel b % 3 of pixel b / 3
            const bool wide = wp + 16 <= HW && ((uintptr_t)run & 3) == 0;       // wave-uniform
            unsigned word = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b = (4 * lane + i) % 48;              // lanes >= 12 gather bytes nobody stores
                word |= (unsigned)__shfl((int)qv, (b / 3) * 4 + b % 3, 64) << (8 * i);
            }
            if (wide) {
                if (lane < 12) reinterpret_cast<unsigned *>(run)[lane] = word;
            } else if (mine)
                o.rgb8[pix * 3 + sub] = (uint8_t)qv;
        }
    }
    if (o.stats) orn_decode_stats_block(ef, eq, o, HW, sd, sf);
}

int orn_launch_decode_out_h16(const h16 *z, const float *w, const float *b, int C, size_t HW, int sigmoid, const OrnDecodeOut &o, hipStream_t st,
                              int act)
{
    ORN_REQUIRE(orn_act_known(act), "decode_out: unknown activation %d", act);
    ORN_REQUIRE(C % 32 == 0 && C <= 128, "decode_out: unsupported C=%d", C);
    ORN_REQUIRE(!o.stats || (o.targets && o.row && o.ws), "decode_out: stats need targets and a workspace");
    int blocks = orn_cdiv((long)HW, 64);
    if (blocks > ORN_DECODE_MAX_BLOCKS) blocks = ORN_DECODE_MAX_BLOCKS;     // (the head forward's own grid: 8192 beat 2048 there)
    ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL(k_decode_out_nhwc<A>, dim3(blocks), dim3(256), 0, st, z, w, b, C, HW, sigmoid, o));
    ORN_LAUNCH_CHECK("decode_out");
    return 0;
}

// The output stage of a SIDE stage (orn_engine_eval_stages, include/orn.h N9): the same outputs from the channels-last
// pre-activation zb [H*W][C] of a block below the last and that stage's head.  Per-pixel arithmetic of k_side_head_fwd_h16
// (orn_side_head.hip) -- 4 lanes per pixel, lane `sub` walks the 8-channel groups sub, sub + 4, .. (the last may be short), then
// head_reduce4 and head_act -- so the fp32 value is the one the training step formed its loss on, bit for bit.  Any C in
// 1..STAGE_OUT_MAXC: 16-byte loads (VEC) where C % 8 == 0 and z is 16-byte aligned, element-wise loads otherwise, both in the same
// order of every sum.  Side images are small and odd-sized and a batch's frame k starts at byte k H W 3: the per-lane byte stores
// and the short last run are ordinary paths here.  One streaming pass; the wave loop is uniform (the byte gather shuffles).
template <bool VEC, int ACT>
__global__ void __launch_bounds__(256)
k_stage_out_nhwc(const h16 *__restrict__ z, const float *__restrict__ w, const float *__restrict__ bias, int C, size_t HW, int sigmoid,
                 OrnDecodeOut o)
{
    __shared__ float sw[3 * STAGE_OUT_MAXC + 3];
    __shared__ double sd[512];
    __shared__ float sf[16];
    for (int i = threadIdx.x; i < 3 * C; i += 256) sw[i] = w[i];
    if (threadIdx.x < 3) sw[3 * C + threadIdx.x] = bias[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, sub = threadIdx.x & 3;
    const float *tgt = o.stats ? o.targets + (size_t)(*o.row) * 3 * HW : nullptr;
    float ef = 0.f, eq = 0.f;
    const size_t pstep = (size_t)gridDim.x * 64;
    for (size_t wp = (size_t)blockIdx.x * 64 + (size_t)(threadIdx.x >> 6) * 16; wp < HW; wp += pstep) {
        const size_t pix = wp + (lane >> 2);
        const bool valid = pix < HW;                  // (all four lanes of a pixel agree; every lane stays for the shuffles)
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
        const bool mine = valid && sub < 3;
        const float v = mine ? head_act(a0, a1, a2, sub, C, sw, sigmoid) : 0.f;
        const unsigned qv = mine ? orn_quant8(v) : 0u;
        if (mine && o.img) o.img[(size_t)sub * HW + pix] = v;
        if (mine && tgt) {
            const float tv = tgt[(size_t)sub * HW + pix];
            const float df = v - tv, dq = (float)qv / 255.0f - tv;
            ef += df * df;
            eq += dq * dq;
        }
        if (o.rgb8) {
            uint8_t *run = o.rgb8 + wp * 3;                     // this wave's 48 bytes, as in k_decode_out_nhwc
            const bool wide = wp + 16 <= HW && ((uintptr_t)run & 3) == 0;       // wave-uniform
            unsigned word = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b = (4 * lane + i) % 48;              // lanes >= 12 gather bytes nobody stores
                word |= (unsigned)__shfl((int)qv, (b / 3) * 4 + b % 3, 64) << (8 * i);
            }
            if (wide) {
                if (lane < 12) reinterpret_cast<unsigned *>(run)[lane] = word;
            } else if (mine)
                o.rgb8[pix * 3 + sub] = (uint8_t)qv;
        }
    }
    if (o.stats) orn_decode_stats_block(ef, eq, o, HW, sd, sf);
}

int orn_launch_stage_out_h16(const h16 *z, const float *w, const float *b, int C, size_t HW, int sigmoid, const OrnDecodeOut &o, hipStream_t st,
                             int act)
{
    ORN_REQUIRE(orn_act_known(act), "stage_out: unknown activation %d", act);
    ORN_REQUIRE(C >= 1 && C <= STAGE_OUT_MAXC, "stage_out: C=%d outside [1, %d]", C, STAGE_OUT_MAXC);
    ORN_REQUIRE(HW >= 1 && HW <= ((size_t)1 << 30), "stage_out: %zu pixels outside [1, 2^30]", HW);
    ORN_REQUIRE(!o.stats || (o.targets && o.row && o.ws), "stage_out: stats need targets and a workspace");
    int blocks = orn_cdiv((long)HW, 64);
    if (blocks > ORN_DECODE_MAX_BLOCKS) blocks = ORN_DECODE_MAX_BLOCKS;
    if (C % 8 == 0 && (uintptr_t)z % 16 == 0)
        ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_stage_out_nhwc<true, A>), dim3(blocks), dim3(256), 0, st, z, w, b, C, HW, sigmoid, o));
    else
        ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL((k_stage_out_nhwc<false, A>), dim3(blocks), dim3(256), 0, st, z, w, b, C, HW, sigmoid, o));
    ORN_LAUNCH_CHECK("stage_out");
    return 0;
}

}  // namespace HNS
