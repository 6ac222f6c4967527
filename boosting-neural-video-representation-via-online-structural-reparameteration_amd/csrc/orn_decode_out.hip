// Decode output stage (orn_engine_decode_frames, include/orn.h): the end of the network as pixels and PSNR instead of an fp32
// image -- what main_eval.py:795-815 / main_train.py:377-438 do per frame with torch ops (x*255 + 0.5, clamp, uint8, HWC; psnr_fn).
//   16-bit engines: ONE kernel reads the last block's channels-last pre-activation z [H*W][C] (the only large operand: 177 MB per
//     720p frame), applies SiLU + the 1x1 head + (tanh+1)/2 | sigmoid with the arithmetic of k_head_fwd_nhwc_bf16 (orn_h16.h:
//     head_accum8 / head_reduce4 / head_act, so the fp32 value is bit-identical to orn_engine_decode's), and per pixel optionally stores the
//     three fp32 planes, three interleaved bytes, and accumulates the squared error of the value and of its byte / 255 against the
//     target pixel.  LDS-free streaming apart from the head's weights: 16-byte loads, 4 lanes per pixel, 16 pixels per wave.
//   fp32 engines: the fp32 head writes its planar image as before; k_decode_out_planar does the same output stage from it.
// Bytes: a wave's 16 (64) pixels are 48 (192) contiguous bytes; where that run starts on a 4-byte boundary and is complete the
// wave gathers whole dwords with lane shuffles and stores those, else every lane stores its own bytes.
// Error sums: per-lane fp32, a fixed-order tree per work-group, per-block partials, and the LAST work-group to arrive (an integer
// ticket) sums the partials in fixed order in double: no float atomics, run-to-run bit-identical.
//   side stages (orn_engine_eval_stages): k_stage_out_nhwc, the same stage behind the head of a block below the last (any C in 1..512).
// Compiled twice (orn_h16.h); the planar kernel and its test hook belong to the bf16 build only.
#include "orn_h16.h"

// torchvision.utils.save_image's quantisation as torch computes it: three separate fp32 ops.  x*255 + 0.5 must NOT contract into
// an fma (hipcc's default): the fma rounds once, and near k + 0.5 that changes the byte.
__device__ __forceinline__ unsigned orn_quant8(float x)
{
    const float y = __fadd_rn(__fmul_rn(x, 255.0f), 0.5f);
    return (unsigned)fminf(fmaxf(y, 0.0f), 255.0f);
}

// ef / eq: this thread's sums of squared errors.  Every thread of the 256-thread work-group calls it (barriers inside).
// sd: 512 doubles of LDS, sf: 16 floats.
__device__ __forceinline__ void orn_decode_stats_block(float ef, float eq, const OrnDecodeOut &o, size_t HW, double *sd, float *sf)
{
    __shared__ int last;
    const int t = threadIdx.x;
    float *part = o.ws;
    unsigned *ticket = reinterpret_cast<unsigned *>(o.ws + 2 * ORN_DECODE_MAX_BLOCKS);
    const float bf = orn_block_sum(ef, sf);
    const float bq = orn_block_sum(eq, sf);
    if (t == 0) {
        part[2 * blockIdx.x] = bf;
        part[2 * blockIdx.x + 1] = bq;
        __threadfence();                                    // the partials are visible before the ticket is taken
        last = atomicAdd(ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    double a = 0.0, b = 0.0;
    for (int i = t; i < (int)gridDim.x; i += 256) {
        a += (double)__hip_atomic_load(part + 2 * i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        b += (double)__hip_atomic_load(part + 2 * i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    sd[t] = a; sd[256 + t] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { sd[t] += sd[t + s]; sd[256 + t] += sd[256 + t + s]; }
        __syncthreads();
    }
    if (t == 0) {
        const double n = 3.0 * (double)HW;
        const float mf = (float)(sd[0] / n), mq = (float)(sd[256] / n);
        o.stats[0] = mf; o.stats[1] = -10.0f * log10f(mf);      // psnr_fn, utils.py:191 (as orn_loss_finalize_block)
        o.stats[2] = mq; o.stats[3] = -10.0f * log10f(mq);
        *ticket = 0u;                                           // ready for the next launch
    }
}

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
#define STAGE_OUT_MAXC 512       // = SH_MAXC (orn_side_head.hip): LDS copy of W [3][C] + b
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

#ifndef ORN_FP16
// fp32 engines: the output stage from the planar image [3][HW] the fp32 head wrote.  One pixel per lane; a wave's 64 pixels are
// 192 contiguous bytes.
__global__ void __launch_bounds__(256) k_decode_out_planar(const float *__restrict__ src, size_t HW, OrnDecodeOut o)
{
    __shared__ double sd[512];
    __shared__ float sf[16];
    const int lane = threadIdx.x & 63;
    const float *tgt = o.stats ? o.targets + (size_t)(*o.row) * 3 * HW : nullptr;
    float ef = 0.f, eq = 0.f;
    const size_t pstep = (size_t)gridDim.x * 256;
    for (size_t wp = (size_t)blockIdx.x * 256 + (size_t)(threadIdx.x >> 6) * 64; wp < HW; wp += pstep) {
        const size_t pix = wp + lane;
        const bool valid = pix < HW;
        unsigned packed = 0;
        if (valid) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = src[(size_t)c * HW + pix];
                const unsigned qv = orn_quant8(v);
                packed |= qv << (8 * c);
                if (o.img) o.img[(size_t)c * HW + pix] = v;
                if (tgt) {
                    const float tv = tgt[(size_t)c * HW + pix];
                    const float df = v - tv, dq = (float)qv / 255.0f - tv;
                    ef += df * df;
                    eq += dq * dq;
                }
            }
        }
        if (o.rgb8) {
            uint8_t *run = o.rgb8 + wp * 3;
            const bool wide = wp + 64 <= HW && ((uintptr_t)run & 3) == 0;       // wave-uniform
            unsigned word = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int b = (4 * lane + i) % 192;             // lanes >= 48 gather bytes nobody stores
                const unsigned p = (unsigned)__shfl((int)packed, b / 3, 64);
                word |= ((p >> (8 * (b % 3))) & 255u) << (8 * i);
            }
            if (wide) {
                if (lane < 48) reinterpret_cast<unsigned *>(run)[lane] = word;
            } else if (valid) {
                o.rgb8[pix * 3] = (uint8_t)(packed & 255u);
                o.rgb8[pix * 3 + 1] = (uint8_t)((packed >> 8) & 255u);
                o.rgb8[pix * 3 + 2] = (uint8_t)((packed >> 16) & 255u);
            }
        }
    }
    if (o.stats) orn_decode_stats_block(ef, eq, o, HW, sd, sf);
}

int orn_launch_decode_out_f32(const float *src, size_t HW, const OrnDecodeOut &o, hipStream_t st)
{
    ORN_REQUIRE(!o.stats || (o.targets && o.row && o.ws), "decode_out: stats need targets and a workspace");
    int blocks = orn_cdiv((long)HW, 256);
    if (blocks > ORN_DECODE_MAX_BLOCKS) blocks = ORN_DECODE_MAX_BLOCKS;
    hipLaunchKernelGGL(k_decode_out_planar, dim3(blocks), dim3(256), 0, st, src, HW, o);
    ORN_LAUNCH_CHECK("decode_out_f32");
    return 0;
}

// test hook (include/orn_debug.h): the planar output stage on a caller's image
extern "C" size_t orn_debug_decode_out_ws_bytes(void) { return (size_t)ORN_DECODE_WS_FLOATS * 4; }
extern "C" int orn_debug_decode_out_f32(const float *img, int H, int W, const float *target, uint8_t *rgb8, float *img_out, float *stats,
                                        void *ws, size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(img && H > 0 && W > 0 && (rgb8 || img_out || stats), "debug_decode_out_f32: bad arguments");
    ORN_REQUIRE(!stats || (target && ws && ws_bytes >= orn_debug_decode_out_ws_bytes() && (uintptr_t)ws % 4 == 0),
                "debug_decode_out_f32: stats need a target and a workspace of orn_debug_decode_out_ws_bytes");
    hipStream_t st = (hipStream_t)stream;
    OrnDecodeOut o = {target, nullptr, rgb8, img_out, stats, (float *)ws};
    if (stats) {       // the row index (0: `target` is the one frame) lives in the workspace, behind the ticket
        ORN_HIP(hipMemsetAsync((float *)ws + 2 * ORN_DECODE_MAX_BLOCKS, 0, 64 * 4, st));
        o.row = reinterpret_cast<const int32_t *>((float *)ws + 2 * ORN_DECODE_MAX_BLOCKS + 1);
    }
    return orn_launch_decode_out_f32(img, (size_t)H * W, o, st);
}
#else
extern "C" size_t orn_debug_decode_out_ws_bytes(void);
#endif

// test hooks (include/orn_debug.h), one set per element type: the side stage's output kernel on a caller's z; the workspace
// convention of orn_debug_decode_out_f32.  Every argument is checked before anything is enqueued.
#ifdef ORN_FP16
#define HOOK(bf16_, f16_) f16_
#else
#define HOOK(bf16_, f16_) bf16_
#endif
extern "C" int HOOK(orn_debug_stage_out_bf16_act, orn_debug_stage_out_f16_act)(const void *z, const float *w, const float *b, int C, int H, int W,
                                                                               int sigmoid, const float *target, uint8_t *rgb8, float *img,
                                                                               float *stats, void *ws, size_t ws_bytes, void *stream, int act)
{
    ORN_REQUIRE(orn_act_known(act), "debug_stage_out: unknown activation %d (ORN_ACT_SWISH, ORN_ACT_GELU)", act);
    ORN_REQUIRE(z && w && b && H > 0 && W > 0 && (rgb8 || img || stats), "debug_stage_out: bad arguments");
    ORN_REQUIRE(C >= 1 && C <= STAGE_OUT_MAXC, "debug_stage_out: C=%d outside [1, %d]", C, STAGE_OUT_MAXC);
    ORN_REQUIRE((size_t)H * W <= ((size_t)1 << 30), "debug_stage_out: bad image size %dx%d", H, W);
    ORN_REQUIRE(!stats || (target && ws && ws_bytes >= orn_debug_decode_out_ws_bytes() && (uintptr_t)ws % 4 == 0),
                "debug_stage_out: stats need a target and a workspace of orn_debug_decode_out_ws_bytes");
    hipStream_t st = (hipStream_t)stream;
    OrnDecodeOut o = {target, nullptr, rgb8, img, stats, (float *)ws};
    if (stats) {       // the row index (0: `target` is the one frame) lives in the workspace, behind the ticket
        ORN_HIP(hipMemsetAsync((float *)ws + 2 * ORN_DECODE_MAX_BLOCKS, 0, 64 * 4, st));
        o.row = reinterpret_cast<const int32_t *>((float *)ws + 2 * ORN_DECODE_MAX_BLOCKS + 1);
    }
    return HNS::orn_launch_stage_out_h16((const h16 *)z, w, b, C, (size_t)H * W, sigmoid, o, st, act);
}
extern "C" int HOOK(orn_debug_stage_out_bf16, orn_debug_stage_out_f16)(const void *z, const float *w, const float *b, int C, int H, int W,
                                                                       int sigmoid, const float *target, uint8_t *rgb8, float *img, float *stats,
                                                                       void *ws, size_t ws_bytes, void *stream)
{
    return HOOK(orn_debug_stage_out_bf16_act, orn_debug_stage_out_f16_act)(z, w, b, C, H, W, sigmoid, target, rgb8, img, stats, ws, ws_bytes, stream,
                                                                           ORN_ACT_SWISH);
}
