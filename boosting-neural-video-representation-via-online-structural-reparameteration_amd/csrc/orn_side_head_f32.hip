// Side heads of the multi-resolution generator, the part without an element type (the 16-bit kernels and the story: orn_side_head.hip):
// the fp32 layout's forward and accumulating backward -- a NCHW [C][H][W] (activation), gradient target da NCHW (gradient with respect
// to the activation: no SiLU' here) --, the column sums that finish dW / db from either layout's per-work-group partials, and the size
// of that partial table.  Built once.
#include "orn_internal.h"

#define SH_F32_PPT 8             // fp32 backward: 256 x SH_F32_PPT pixels per work-group

// column sums of the per-work-group partials [rows][n] -> dw [3 C], db [3], times `inv` (1 / the gradient scale the partials carry).
// One wave per column: lane l sums rows l, l + 64, ... in order, then the butterfly.
__global__ void __launch_bounds__(64) k_side_head_finish(const float *__restrict__ partial, int rows, int n, int C, float inv,
                                                        float *__restrict__ dw, float *__restrict__ db, OrnScaleState *sc, int scaled)
{
    if (sc && scaled) inv = sc->inv_gs;
    const int i = blockIdx.x;
    float s = 0.f;
    for (int r = threadIdx.x; r < rows; r += 64) s += partial[(size_t)r * n + i];
    s = orn_wave_sum(s) * inv;
    if (threadIdx.x == 0) {
        orn_flag_nonfinite(sc, s);
        if (i < 3 * C) dw[i] = s;
        else db[i - 3 * C] = s;
    }
}

// sc (engine): non-finite sums raise its flag; scaled: the partials carry its scale (inv is then read from it)
int orn_launch_side_head_finish(const float *partial, int rows, int C, float inv, float *dw, float *db, hipStream_t st, OrnScaleState *sc,
                                bool scaled)
{
    const int n = 3 * C + 3;
    hipLaunchKernelGGL(k_side_head_finish, dim3(n), dim3(64), 0, st, partial, rows, n, C, inv, dw, db, sc, scaled ? 1 : 0);
    ORN_LAUNCH_CHECK("side_head_finish");
    return 0;
}

// fp32 NCHW forward: k_head_fwd<1> (orn_elementwise.hip) plus the flag.  One thread per pixel, one k-ordered fmaf chain per output.
__global__ void __launch_bounds__(256)
k_side_head_fwd_f32(const float *__restrict__ a, const float *__restrict__ w, const float *__restrict__ bias, int C, size_t HW, int sigmoid,
                    float *__restrict__ out, OrnScaleState *sc)
{
    __shared__ float sw[3 * SH_MAXC + 3];
    for (int i = threadIdx.x; i < 3 * C + 3; i += 256) sw[i] = i < 3 * C ? w[i] : bias[i - 3 * C];
    __syncthreads();
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < C; ++c) {
        const float av = a[(size_t)c * HW + p];
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = fmaf(sw[k * C + c], av, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = acc[k] + sw[3 * C + k];
        orn_flag_nonfinite(sc, u);
        out[(size_t)k * HW + p] = sigmoid ? 1.0f / (1.0f + expf(-u)) : (tanhf(u) + 1.0f) * 0.5f;
    }
}

int orn_launch_side_head_fwd_f32(const float *a, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st,
                                 OrnScaleState *sc)
{
    ORN_REQUIRE(C >= 1 && C <= SH_MAXC, "side_head_fwd_f32: C=%d outside [1, %d]", C, SH_MAXC);
    ORN_REQUIRE(HW >= 1 && HW <= ((size_t)1 << 30), "side_head_fwd_f32: %zu pixels outside [1, 2^30]", HW);
    hipLaunchKernelGGL(k_side_head_fwd_f32, dim3(orn_cdiv((long)HW, 256)), dim3(256), 0, st, a, w, b, C, HW, sigmoid, out, sc);
    ORN_LAUNCH_CHECK("side_head_fwd_f32");
    return 0;
}

// fp32 NCHW.  k_head_bwd (orn_elementwise.hip) with two differences: du carries lw, and da is read, added to and written back.
__global__ void __launch_bounds__(256)
k_side_head_bwd_f32(const float *__restrict__ a, const float *__restrict__ w, const float *__restrict__ out, const float *__restrict__ dout,
                    int C, size_t HW, int sigmoid, float lw, float *__restrict__ da, float *__restrict__ partial)
{
    __shared__ float sw[3 * SH_MAXC];
    __shared__ float sred[4][3 * SH_MAXC + 3];
    for (int i = threadIdx.x; i < 3 * C; i += 256) sw[i] = w[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t p0 = (size_t)blockIdx.x * 256 * SH_F32_PPT;
    float du[3][SH_F32_PPT];
    size_t pp[SH_F32_PPT];
#pragma unroll
    for (int i = 0; i < SH_F32_PPT; ++i) {
        pp[i] = p0 + (size_t)i * 256 + threadIdx.x;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float d = 0.f;
            if (pp[i] < HW) {
                const float o = out[(size_t)k * HW + pp[i]], g = dout[(size_t)k * HW + pp[i]];
                d = g * lw * (sigmoid ? o * (1.0f - o) : 2.0f * o * (1.0f - o));
            }
            du[k][i] = d;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < SH_F32_PPT; ++i) s += du[k][i];
        s = orn_wave_sum(s);
        if (lane == 0) sred[wave][3 * C + k] = s;
    }
    for (int c = 0; c < C; ++c) {
        const float w0 = sw[c], w1 = sw[C + c], w2 = sw[2 * C + c];
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < SH_F32_PPT; ++i) {
            if (pp[i] < HW) {
                const size_t idx = (size_t)c * HW + pp[i];
                const float av = a[idx];
                s0 = fmaf(du[0][i], av, s0);
                s1 = fmaf(du[1][i], av, s1);
                s2 = fmaf(du[2][i], av, s2);
                da[idx] = da[idx] + fmaf(w2, du[2][i], fmaf(w1, du[1][i], w0 * du[0][i]));
            }
        }
        s0 = orn_wave_sum(s0);
        s1 = orn_wave_sum(s1);
        s2 = orn_wave_sum(s2);
        if (lane == 0) {
            sred[wave][c] = s0;
            sred[wave][C + c] = s1;
            sred[wave][2 * C + c] = s2;
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * C + 3; i += 256)
        partial[(size_t)blockIdx.x * (3 * C + 3) + i] = (sred[0][i] + sred[1][i]) + (sred[2][i] + sred[3][i]);
}

static int side_head_bwd_blocks_f32(int H, int W) { return orn_cdiv((long)H * W, 256 * SH_F32_PPT); }

int orn_launch_side_head_bwd_f32(const float *a, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid,
                                 float lw, float *da, float *dw, float *db, float *ws, hipStream_t st, OrnScaleState *sc)
{
    ORN_REQUIRE(C >= 1 && C <= SH_MAXC, "side_head_bwd_f32: C=%d outside [1, %d]", C, SH_MAXC);
    ORN_REQUIRE(H >= 1 && W >= 1 && (size_t)H * W <= ((size_t)1 << 30), "side_head_bwd_f32: bad image size %dx%d", H, W);
    const int blocks = side_head_bwd_blocks_f32(H, W);
    hipLaunchKernelGGL(k_side_head_bwd_f32, dim3(blocks), dim3(256), 0, st, a, w, out, dout, C, (size_t)H * W, sigmoid, lw, da, ws);
    ORN_LAUNCH_CHECK("side_head_bwd_f32");
    return orn_launch_side_head_finish(ws, blocks, C, 1.0f, dw, db, st, sc, false);
}

// the larger of the two layouts' partial tables
size_t orn_side_head_bwd_ws_floats(int C, int H, int W)
{
    if (C < 1 || C > SH_MAXC || H < 1 || W < 1 || (size_t)H * W > ((size_t)1 << 30)) return 0;
    return orn_align((size_t)orn_cdiv((long)H * W, 64 * SH_PPT) * (3 * (size_t)C + 3) * sizeof(float)) / sizeof(float);
}
