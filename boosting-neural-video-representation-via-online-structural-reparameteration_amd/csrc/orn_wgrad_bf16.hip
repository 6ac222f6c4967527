// A4 fast path, WGRAD of the NeRVBlock conv: dW[tap][o'][c] = sum_p dy[p][o'] * x[p + off(tap)][c] on v_mfma_f32_32x32x16
// (fp32 accumulate); buffer layouts in orn_conv_bf16.hip.  Work-group = 128 out channels x one kernel row (3 taps) x all 96
// in-channels, K = pixels split over S work-groups that each write an fp32 slab; both operands pixel-major in LDS and read
// with ds_read_b64_tr_b16 (the work-group body: orn_wgrad_body.h).  The engine runs every layer's wgrad as ONE launch
// (k_wgrad_nhwc_bf16_all) and every layer's split-K reduction as one more (k_wgrad_bf16_reduce_all); kernels that only Adam
// waits for ride on both as trailing work-groups (the head's dW/db reduction, two kernels of the stem backward).
// Compiled twice (orn_h16.h): bf16 and, with -DORN_FP16, IEEE half.
#include "orn_h16.h"

namespace HNS {

#include "orn_wgrad_body.h"     // WgradBP, wgrad_body
static int g_wgrad_dbg = 0;   // timing experiments only (tools/probes), see orn_debug_set
void set_debug_wgrad(int flags) { g_wgrad_dbg = flags; }

// ================================================================================================
// wgrad: dW[tap][o'][c] = sum_p dy[p][o'] * x[p + off(tap)][c]
// ================================================================================================
__global__ void __launch_bounds__(256, 2) k_wgrad_nhwc_bf16(WgradBP p) { wgrad_body(p, blockIdx.x); }

// Reduction of the 16-bit head backward (orn_ops_bf16.hip), here because it rides on the batched wgrad launch below:
// dw/db = gscale * sum over blocks of the head backward's per-block partials [blocks][3C+3]: one work-group per column, lane t sums rows t, t+256, .. in ascending order, fixed-order block tree after (deterministic).
__device__ __forceinline__ void head_finish_body(const float *__restrict__ partial, int blocks, int C, float gscale, float *__restrict__ dw,
                                                 float *__restrict__ db, int col, float *sred /* 256 floats of LDS */, OrnScaleState *sc = nullptr)
{
    if (sc) gscale = sc->inv_gs;
    const int n = 3 * C + 3, t = threadIdx.x;
    float acc = 0.f;
    for (int r = t; r < blocks; r += 256) acc += partial[(size_t)r * n + col];
    sred[t] = acc;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (t < w) sred[t] += sred[t + w];
        __syncthreads();
    }
    if (t == 0) {
        const float v = sred[0] * gscale;
        orn_flag_nonfinite(sc, v);
        if (col < 3 * C) dw[col] = v;
        else db[col - 3 * C] = v;
    }
}

// the same reduction as a launch of its own (head backward called with dw: the per-op path)
__global__ void __launch_bounds__(256) k_head_bf16_finish(const float *__restrict__ partial, int blocks, int C, float gscale,
                                                          float *__restrict__ dw, float *__restrict__ db)
{
    __shared__ float sred[256];
    head_finish_body(partial, blocks, C, gscale, dw, db, blockIdx.x, sred);
}

int orn_launch_head_finish_bf16(const float *partial, int blocks, int C, float gscale, float *dw, float *db, hipStream_t st)
{
    hipLaunchKernelGGL(k_head_bf16_finish, dim3(3 * C + 3), dim3(256), 0, st, partial, blocks, C, gscale, dw, db);
    ORN_LAUNCH_CHECK("head_bf16_finish");
    return 0;
}

// Several layers in one launch (problems in the order given, each on a multiple-of-8 block range so the XCD decode holds):
// the small layers' wgrads do not fill the chip one at a time (72 / 216 / 360 work-groups for 512 slots at 720p), and
// nothing but the deferred reduction consumes them.
// The head's dW/db reduction (needed by Adam only) rides along as trailing work-groups: one graph node less.
struct WgradBPAll { int n; int start[ORN_MAX_LAYERS + 1]; WgradBP p[ORN_MAX_LAYERS]; OrnHeadFinish hf; int hf_blocks; OrnStemL2Job l2; int side; };
// ACT: the activation of the stem job it may carry (the wgrad and the head finish evaluate none)
template <int ACT>
__global__ void __launch_bounds__(256, 2) k_wgrad_nhwc_bf16_all(WgradBPAll a)
{
    if (!a.side) ORN_PRIO_HIGH();         // (the side branch's launch keeps the default priority: orn_common.h)
    if ((int)blockIdx.x >= a.start[a.n] + a.hf_blocks) {        // stem backward, second linear layer: 16 output rows per work-group
        extern __shared__ __attribute__((aligned(16))) unsigned char smem_l2[];
        orn_stem_l2_block<ACT>(a.l2, (int)blockIdx.x - a.start[a.n] - a.hf_blocks, (int)threadIdx.x, reinterpret_cast<float *>(smem_l2));
        return;
    }
    if ((int)blockIdx.x >= a.start[a.n]) {
        extern __shared__ __attribute__((aligned(16))) unsigned char smem_hf[];
        head_finish_body(a.hf.partial, a.hf.blocks, a.hf.C, a.hf.gscale, a.hf.dw, a.hf.db, (int)blockIdx.x - a.start[a.n],
                         reinterpret_cast<float *>(smem_hf), a.hf.sc);
        return;
    }
    int k = 0;
    while (k + 1 < a.n && (int)blockIdx.x >= a.start[k + 1]) ++k;
    k = __builtin_amdgcn_readfirstlane(k);
    wgrad_body(a.p[k], (int)blockIdx.x - a.start[k]);
}

// dWf[o][c][i][j] = gscale * sum_s slabs[s][tap][o'(o)][c],  o' = (o % s2)*Cn + o / s2
// Cr <= 96 real input channels (a narrower first fast layer runs zero-padded to 96): only those are written
__device__ __forceinline__ void wgrad_reduce_body(const float *__restrict__ slabs, const float *__restrict__ bias_slabs, int S, int O, int Cn,
                                                  int s2, int Cr, float gscale, float *__restrict__ dwf, float *__restrict__ dbf,
                                                  OrnScaleState *sc = nullptr)
{
    // sc: the un-scaling factor comes from the device-side loss-scale state, and a non-finite result (an overflow of the
    // 16-bit gradient tensors shows up in the bias gradient = plain sum of dy at the latest) raises its flag
    if (sc) gscale = sc->inv_gs;
    const size_t n = (size_t)9 * O * 96;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (size_t)O && dbf) {
        float b = 0.f;
        for (int s = 0; s < S; ++s) b += bias_slabs[(size_t)s * O + idx];
        const int ij = (int)idx / Cn, nn = (int)idx - ij * Cn;
        dbf[nn * s2 + ij] = b * gscale;
        orn_flag_nonfinite(sc, b * gscale);
    }
    if (idx >= n) return;
    const int c = (int)(idx % 96);
    if (c >= Cr) return;
    // 8 independent partial sums keep 8 loads in flight (fixed order -> still deterministic)
    float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (; s + 8 <= S; s += 8) {
#pragma unroll
        for (int k = 0; k < 8; ++k) a8[k] += slabs[(size_t)(s + k) * n + idx];
    }
    for (; s < S; ++s) a8[0] += slabs[(size_t)s * n + idx];
    const float acc = ((a8[0] + a8[1]) + (a8[2] + a8[3])) + ((a8[4] + a8[5]) + (a8[6] + a8[7]));
    const size_t r = idx / 96;
    const int op = (int)(r % O), tap = (int)(r / O);
    const int ij = op / Cn, nn = op - ij * Cn;
    const int o = nn * s2 + ij;
    dwf[((size_t)o * Cr + c) * 9 + tap] = acc * gscale;
    orn_flag_nonfinite(sc, acc * gscale);
}

__global__ void k_wgrad_bf16_reduce(const float *__restrict__ slabs, const float *__restrict__ bias_slabs, int S, int O, int Cn,
                                    int s2, int Cr, float gscale, float *__restrict__ dwf, float *__restrict__ dbf)
{
    wgrad_reduce_body(slabs, bias_slabs, S, O, Cn, s2, Cr, gscale, dwf, dbf);
}

// Every fast layer's reduction in one launch at the end of the backward (blockIdx.y = layer): four graph nodes of 6-26 us
// that each started cold become one that keeps the whole chip streaming.
struct WgradReduceAll {
    struct { const float *slabs, *bias_slabs; int S, O, Cn, s2, Cr; float gscale; float *dwf, *dbf; OrnScaleState *sc; } l[ORN_MAX_LAYERS];
    int n; OrnStemW0Job w0;        // blockIdx.y == n: the stem backward's last kernel, two output rows per work-group (needed by Adam only)
};
template <int ACT>
__global__ void k_wgrad_bf16_reduce_all(WgradReduceAll a)
{
    if ((int)blockIdx.y == a.n) {
        __shared__ float sh_w0[4];
        if (2 * (int)blockIdx.x >= a.w0.N) return;
        const int half = threadIdx.x >> 7;
        orn_stem_w0_row<ACT>(a.w0, (int)blockIdx.x * 2 + half, threadIdx.x & 127, sh_w0 + 2 * half);
        return;
    }
    const auto &l = a.l[blockIdx.y];
    if ((size_t)blockIdx.x * blockDim.x >= (size_t)9 * l.O * 96) return;
    wgrad_reduce_body(l.slabs, l.bias_slabs, l.S, l.O, l.Cn, l.s2, l.Cr, l.gscale, l.dwf, l.dbf, l.sc);
}

int orn_wgrad_bf16_split(int H, int W, int O, int smax = 0)
{
    // S slabs of 9*O*96 floats are written and re-read: keep >= 8 K tiles per work-group so the slab traffic
    // stays small next to the layer's own data, up to one full wave of work-groups (2 per CU)
    const int n_ktiles = orn_cdiv(H, WB_TH) * orn_cdiv(W, WB_TW);
    const int per = 3 * orn_cdiv(O, WB_BO);
    int S = (512 / per) / 8 * 8;
    // measured in the 720p step: a full wave of work-groups (56 slabs) makes the slab write + re-read cost more than the idle
    // slots do -- L3 (900 K tiles): 40 slabs beat 56 by 17 us; L4 (3600 K tiles), since the DMA prefetch of the K loop works:
    // 32 / 40 / 48 / 56 slabs = 1.148 / 1.128 / 1.133 / 1.143 ms per step (reduction 30 / 35 / 38 / 45 us, wgrad 224 / 199 / 199 / 201)
    if (S > 40) S = 40;
    // layers under 2000 K tiles (720p L3: 900): 24 slabs -- the wgrad launch does not notice (all layers share it), the reduction
    // reads less: 40 / 32 / 24 = 35 / 32 / 30 us
    if (n_ktiles < 2000 && S > 24 && smax < 8) S = 24;     // (a caller's count replaces this rule)
    const int by_work = (n_ktiles / 8) / 8 * 8;
    if (S > by_work) S = by_work;
    if (smax >= 8 && S > smax) S = smax / 8 * 8;   // caller's cap (the engine's side branch runs the last block on fewer, longer work-groups)
    if (S < 8) S = 8;
    return S;
}

// (sized for the largest slab count any caller may ask for -- the engine chooses per layer: OrnWgradJob::smax)
size_t orn_wgrad_bf16_ws_floats(int H, int W, int O)
{
    const int S = orn_wgrad_bf16_split(H, W, O), Smax = orn_wgrad_bf16_split(H, W, O, 40);
    return (size_t)(S > Smax ? S : Smax) * (9 * (size_t)O * 96 + O);
}

// Both wgrad kernels are launched with WB_LDS_BYTES of dynamic LDS: their attribute is raised once per process, before the first
// launch of either (wgrad_fill, and the batch launch that carries riders only and fills no job).
static int wgrad_lds_setup()
{
    static bool attr_done = false;
    if (!attr_done) {
        const size_t smem = WB_LDS_BYTES;
        hipError_t e = hipFuncSetAttribute((const void *)k_wgrad_nhwc_bf16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_wgrad_nhwc_bf16_all<ORN_ACT_SWISH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_wgrad_nhwc_bf16_all<ORN_ACT_GELU>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) { orn_set_error("wgrad_bf16: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
        attr_done = true;
    }
    return 0;
}

// dwf [O][C][3][3] and dbf [O] (PyTorch channel order), both overwritten.  C <= 96 real channels; xpad always has 96
// channels per pixel (zeros above C).
static int wgrad_fill(WgradBP &p, const h16 *xpad, const h16 *dypad, int H, int W, int C, int O, int s, float *slabs, int smax = 0)
{
    // O % 32: a ragged last 128-channel tile reads up to 96 channels past a pixel's O; behind the last interior pixel (H, W) they
    // fall on dypad's border ring, so this kernel stays inside [H+2][W+2][O].  The 128 elements of slack orn.h asks for behind
    // dypad (the engine and the per-op hooks allocate them) serve the dgrad's reads; tests/test_gpu_conv16_forms.py fills them
    // with NaN.
    ORN_REQUIRE(C >= 1 && C <= 96 && O % 32 == 0 && O % (s * s) == 0, "wgrad_bf16: unsupported C=%d O=%d", C, O);
    p.dbg = g_wgrad_dbg;
    p.xpad = xpad; p.dypad = dypad; p.slabs = slabs; p.H = H; p.W = W; p.O = O;
    p.tiles_w = orn_cdiv(W, WB_TW);
    p.n_ktiles = p.tiles_w * orn_cdiv(H, WB_TH);
    p.S = orn_wgrad_bf16_split(H, W, O, smax);
    p.bias_slabs = slabs + (size_t)p.S * 9 * O * 96;
    p.n_otiles = orn_cdiv(O, WB_BO);
    return wgrad_lds_setup();
}

// slabs only (no reduction), several layers in one launch
int orn_launch_wgrad_bf16_batch(int n, const OrnWgradJob *J, hipStream_t st, const OrnHeadFinish *hf, const OrnStemL2Job *l2, int side, int act)
{
    if (n == 0 && !hf && !l2) return 0;
    ORN_REQUIRE(orn_act_known(act), "wgrad_batch: unknown activation %d", act);
    ORN_REQUIRE(n <= ORN_MAX_LAYERS, "wgrad_batch: %d layers", n);
    WgradBPAll a;
    a.n = n;
    a.side = side;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        ORN_TRY(wgrad_fill(a.p[i], (const h16 *)J[i].xpad, (const h16 *)J[i].dypad, J[i].H, J[i].W, J[i].C, J[i].O, J[i].s, J[i].slabs, J[i].smax));
        a.start[i] = total;
        total += 3 * a.p[i].n_otiles * a.p[i].S;        // S % 8 == 0: every start is a multiple of 8
    }
    a.start[n] = total;
    if (n == 0) ORN_TRY(wgrad_lds_setup());             // riders alone: no wgrad_fill has run for this launch
    a.hf = OrnHeadFinish{};
    a.hf_blocks = 0;
    if (hf) { a.hf = *hf; a.hf_blocks = 3 * hf->C + 3; total += a.hf_blocks; }
    a.l2 = OrnStemL2Job{};
    if (l2) { a.l2 = *l2; total += orn_cdiv(l2->N, ORN_STEM_ROWS); }
    ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL(k_wgrad_nhwc_bf16_all<A>, dim3(total), dim3(256), WB_LDS_BYTES, st, a));
    ORN_LAUNCH_CHECK("wgrad_nhwc_bf16_all");
    return 0;
}

// dwf [O][C][3][3] and dbf [O] (PyTorch channel order), both overwritten.  C <= 96 real channels; xpad always has 96
// channels per pixel (zeros above C).
int orn_launch_wgrad_bf16(const h16 *xpad, const h16 *dypad, int H, int W, int C, int O, int s, float gscale,
                          float *slabs, float *dwf, float *dbf, hipStream_t st)
{
    WgradBP p;
    ORN_TRY(wgrad_fill(p, xpad, dypad, H, W, C, O, s, slabs));
    hipLaunchKernelGGL(k_wgrad_nhwc_bf16, dim3(3 * p.n_otiles * p.S), dim3(256), WB_LDS_BYTES, st, p);
    ORN_LAUNCH_CHECK("wgrad_nhwc_bf16");
    if (!dwf) return 0;                 // deferred: orn_launch_wgrad_reduce_all
    const size_t n = (size_t)9 * O * 96;
    hipLaunchKernelGGL(k_wgrad_bf16_reduce, dim3(orn_cdiv((long)n, 256)), dim3(256), 0, st, slabs, p.bias_slabs, p.S, O,
                       O / (s * s), s * s, C, gscale, dwf, dbf);
    ORN_LAUNCH_CHECK("wgrad_bf16_reduce");
    return 0;
}

int orn_launch_wgrad_reduce_all(int n, const OrnWgradReduce *L, hipStream_t st, const OrnStemW0Job *w0, int act)
{
    if (n == 0 && !w0) return 0;
    ORN_REQUIRE(orn_act_known(act), "wgrad_reduce_all: unknown activation %d", act);
    ORN_REQUIRE(n <= ORN_MAX_LAYERS, "wgrad_reduce_all: %d layers", n);
    WgradReduceAll a;
    size_t mx = 0;
    for (int i = 0; i < n; ++i) {
        const int S = orn_wgrad_bf16_split(L[i].H, L[i].W, L[i].O, L[i].smax), s2 = L[i].s * L[i].s;
        a.l[i].slabs = L[i].slabs; a.l[i].bias_slabs = L[i].slabs + (size_t)S * 9 * L[i].O * 96;
        a.l[i].S = S; a.l[i].O = L[i].O; a.l[i].Cn = L[i].O / s2; a.l[i].s2 = s2; a.l[i].Cr = L[i].C; a.l[i].gscale = L[i].gscale;
        a.l[i].dwf = L[i].dwf; a.l[i].dbf = L[i].dbf; a.l[i].sc = L[i].sc;
        const size_t w = (size_t)9 * L[i].O * 96;
        if (w > mx) mx = w;
    }
    a.n = n;
    a.w0 = OrnStemW0Job{};
    if (w0) { a.w0 = *w0; const size_t need = (size_t)orn_cdiv(w0->N, 2) * 256; if (need > mx) mx = need; }
    ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL(k_wgrad_bf16_reduce_all<A>, dim3(orn_cdiv((long)mx, 256), n + (w0 ? 1 : 0)), dim3(256), 0, st, a));
    ORN_LAUNCH_CHECK("wgrad_bf16_reduce_all");
    return 0;
}

}  // namespace HNS
