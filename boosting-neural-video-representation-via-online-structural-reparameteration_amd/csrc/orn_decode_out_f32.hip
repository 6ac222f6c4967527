// Decode output stage of the fp32 engines (orn_engine_decode_frames, include/orn.h): the fp32 head writes its planar image as before,
// k_decode_out_planar turns it into bytes, an optional fp32 copy and the error sums -- the outputs, the byte gather and the ticket
// reduction of the 16-bit engines' kernels (orn_decode_out.hip; shared pieces: orn_decode_out.h).  No element type in it: built once.
#include "orn_decode_out.h"

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
