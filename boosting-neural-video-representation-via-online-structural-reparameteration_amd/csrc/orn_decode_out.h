// What the decode output kernels share (orn_decode_out.hip, the 16-bit engines' kernels, built per element type; orn_decode_out_f32.hip,
// the planar kernel of the fp32 engines): the byte quantisation and the fixed-order error sums behind the ticket.
#pragma once
#include "orn_internal.h"

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
