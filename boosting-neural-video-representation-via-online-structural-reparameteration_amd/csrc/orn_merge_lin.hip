// N7  Online merge of the paper's comparison blocks -- ACB, RepVGG, ECB (model.py:345-393, 541-565) -- to one 3x3 kernel, and its
// backward (include/orn.h, N7, states the formulas and the order of every sum).  Each block is linear in its weights, so it trains
// the way ERB does: merge every step, run the block's one conv, send dL/dWf back through the merge.
//
// These are latency- and bandwidth-bound launches over at most O*C*9 = 0.75 M elements per block (2.2 M with ECB's wB), so they are
// built for few launches and plain coalesced traffic, not for FLOPs:
//   forward   ONE launch for all blocks of an engine: a work-group per output channel o, a thread per input channel c, the nine taps
//             of (o, c) in registers.  ECB's T[o,c,:] = sum_m wB[o,m,:] * wA[m,c] is formed in the same threads (nine m-ordered fmaf
//             chains): wB[o,m,:] is uniform in the work-group (scalar loads), wA[m,c] is a coalesced row.  No intermediate T in memory.
//   backward  ONE launch for all blocks with three kinds of work-group, all reading only g = dL/dWf and parameters:
//               row    per o: the slice / copy gradients, the bias fan-out, ECB's q_t, dk0_t, dscale_t (block tree over c), and the
//                      zeros of db0_t and dmask_t
//               dwB    per o: dwB[o,m,:] = sum_c g[o,c,:] * wA[m,c], a thread per m; wA passes through LDS in [m][32 c] tiles (read
//                      coalesced along c, used along m), g[o,c,:] is uniform (scalar loads)
//               dwA    per (slab of 32 output channels, 8 rows m): partial[slab][m][c] = sum_{o in slab} sum_k wB[o,m,k] * g[o,c,k],
//                      one fmaf chain in (o, k) order; a thread per c, four m per thread so that a loaded g serves four chains
//             and a second, small launch (ECB only) that adds the slabs of dwA in slab order.  No atomics anywhere.
#include "orn_internal.h"

#define BR_FWD_THREADS 128
#define BR_BWD_THREADS 256
#define BR_SLAB 32              // output channels per partial sum of dwA
#define BR_DWA_M 4              // rows m of dwA per thread
#define BR_TILE_C 32            // c per LDS tile of wA in the dwB work-groups

struct BrFwdLayer {
    int kind, C, O;
    const float *w3x3, *b3x3, *wa, *ba, *wb, *bb;     // ACB: a = 1x3, b = 3x1; RepVGG: a = 1x1; ECB: wa = wA, wb = wB
    const float *k0[3], *scale[3], *bias[3], *mask[3];
    float *wf, *bf;
};
struct BrFwdAll { int n; int blk_end[ORN_MAX_LAYERS]; BrFwdLayer l[ORN_MAX_LAYERS]; };

struct BrBwdLayer {
    int kind, C, O, nslab;
    const float *g, *dbf, *wA, *wB, *k0[3], *scale[3], *mask[3];
    float *d3x3, *db3x3, *da, *dba, *db, *dbb;        // ACB: a = 1x3, b = 3x1; RepVGG: a = 1x1
    float *dwA, *dwB, *dwAp;
    float *dk0[3], *db0[3], *dscale[3], *dbias[3], *dmask[3];
};
// work-groups of a layer: [row: O][dwB: O][dwA: nslab * ceil(2C / 8)] (the last two for ECB only); blk_end: running total
struct BrBwdAll { int n; int blk_end[ORN_MAX_LAYERS]; BrBwdLayer l[ORN_MAX_LAYERS]; };

__global__ void __launch_bounds__(BR_FWD_THREADS) k_branch_merge_fwd(BrFwdAll a)
{
    int li = 0;
    while (li + 1 < a.n && (int)blockIdx.x >= a.blk_end[li]) ++li;
    const BrFwdLayer &l = a.l[li];
    const int o = blockIdx.x - (li ? a.blk_end[li - 1] : 0);
    const int C = l.C, t = threadIdx.x;
    if (t == 0) {
        float b = l.b3x3[o];
        if (l.kind == ORN_BRANCH_ACB) b = __fadd_rn(__fadd_rn(b, l.ba[o]), l.bb[o]);
        else if (l.kind == ORN_BRANCH_REPVGG) b = __fadd_rn(b, l.ba[o]);
        else
            for (int s = 0; s < 3; ++s) b = __fadd_rn(b, l.bias[s][o]);
        l.bf[o] = b;
    }
    float sm[3][9];             // ECB: scale_t[o] * mask_t[o, k], uniform in the work-group
    if (l.kind == ORN_BRANCH_ECB) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const float sc = l.scale[s][o];
#pragma unroll
            for (int k = 0; k < 9; ++k) sm[s][k] = __fmul_rn(sc, l.mask[s][(size_t)o * 9 + k]);
        }
    }
    for (int c = t; c < C; c += BR_FWD_THREADS) {
        const size_t oc = (size_t)o * C + c;
        float v[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = l.w3x3[oc * 9 + k];
        if (l.kind == ORN_BRANCH_ACB) {
            // (w3x3 + pad_h(w1x3)) + pad_w(w3x1): the zeros of the padded kernels are added too, as the tensor expression adds them
            float p13[9] = {0.f, 0.f, 0.f, l.wa[oc * 3], l.wa[oc * 3 + 1], l.wa[oc * 3 + 2], 0.f, 0.f, 0.f};
            float p31[9] = {0.f, l.wb[oc * 3], 0.f, 0.f, l.wb[oc * 3 + 1], 0.f, 0.f, l.wb[oc * 3 + 2], 0.f};
#pragma unroll
            for (int k = 0; k < 9; ++k) v[k] = __fadd_rn(__fadd_rn(v[k], p13[k]), p31[k]);
        } else if (l.kind == ORN_BRANCH_REPVGG) {
            const float w11 = l.wa[oc];
#pragma unroll
            for (int k = 0; k < 9; ++k) v[k] = __fadd_rn(v[k], k == 4 ? w11 : 0.f);
        } else {
            float T[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const int K2 = 2 * C;
            const float *wBo = l.wb + (size_t)o * K2 * 9;
            for (int m = 0; m < K2; ++m) {
                const float am = l.wa[(size_t)m * C + c];
#pragma unroll
                for (int k = 0; k < 9; ++k) T[k] = fmaf(wBo[m * 9 + k], am, T[k]);
            }
            const float k0s[3] = {l.k0[0][oc], l.k0[1][oc], l.k0[2][oc]};
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                float x = __fadd_rn(v[k], T[k]);
#pragma unroll
                for (int s = 0; s < 3; ++s) x = __fadd_rn(x, __fmul_rn(sm[s][k], k0s[s]));
                v[k] = x;
            }
        }
#pragma unroll
        for (int k = 0; k < 9; ++k) l.wf[oc * 9 + k] = v[k];
    }
}

// ---- backward: the three kinds of work-group ---------------------------------------------------------------------------------
__device__ __forceinline__ void br_bwd_row(const BrBwdLayer &l, int o, float *red /* 16 floats */)
{
    const int C = l.C, t = threadIdx.x;
    const bool ecb = l.kind == ORN_BRANCH_ECB;
    float mk[3][9], sc[3] = {0.f, 0.f, 0.f}, ds[3] = {0.f, 0.f, 0.f};
    if (ecb) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            sc[s] = l.scale[s][o];
#pragma unroll
            for (int k = 0; k < 9; ++k) mk[s][k] = l.mask[s][(size_t)o * 9 + k];
        }
    }
    for (int c = t; c < C; c += BR_BWD_THREADS) {
        const size_t oc = (size_t)o * C + c;
        float v[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = l.g[oc * 9 + k];
        if (l.d3x3 != l.g) {
#pragma unroll
            for (int k = 0; k < 9; ++k) l.d3x3[oc * 9 + k] = v[k];
        }
        if (l.kind == ORN_BRANCH_ACB) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                l.da[oc * 3 + k] = v[3 + k];            // d1x3[o,c,kw] = g[o,c,1,kw]
                l.db[oc * 3 + k] = v[3 * k + 1];        // d3x1[o,c,kh] = g[o,c,kh,1]
            }
        } else if (l.kind == ORN_BRANCH_REPVGG) {
            l.da[oc] = v[4];
        } else {
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                float q = 0.f;
#pragma unroll
                for (int k = 0; k < 9; ++k) q = fmaf(mk[s][k], v[k], q);
                l.dk0[s][oc] = sc[s] * q;
                ds[s] = fmaf(l.k0[s][oc], q, ds[s]);
            }
        }
    }
    if (ecb) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const float tot = orn_block_sum(ds[s], red);     // (barriers inside: every thread of the work-group gets here)
            if (t == 0) l.dscale[s][o] = tot;
        }
        if (t < 27) l.dmask[t / 9][(size_t)o * 9 + t % 9] = 0.f;
    }
    if (t == 0) {
        const float d = l.dbf[o];
        if (l.db3x3 != l.dbf) l.db3x3[o] = d;
        if (l.kind == ORN_BRANCH_ACB) { l.dba[o] = d; l.dbb[o] = d; }
        else if (l.kind == ORN_BRANCH_REPVGG) l.dba[o] = d;
        else
            for (int s = 0; s < 3; ++s) { l.dbias[s][o] = d; l.db0[s][o] = 0.f; }
    }
}

// dwB[o,m,k] = sum_c g[o,c,k] * wA[m,c]: nine c-ordered fmaf chains per thread m
__device__ __forceinline__ void br_bwd_dwB(const BrBwdLayer &l, int o, float (*tile)[BR_TILE_C + 1])
{
    const int C = l.C, K2 = 2 * C, t = threadIdx.x;
    const float *go = l.g + (size_t)o * C * 9;
    for (int m0 = 0; m0 < K2; m0 += BR_BWD_THREADS) {
        const int rows = min(BR_BWD_THREADS, K2 - m0);
        float acc[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < C; c0 += BR_TILE_C) {
            const int cols = min(BR_TILE_C, C - c0);
            __syncthreads();
            for (int i = t; i < rows * BR_TILE_C; i += BR_BWD_THREADS) {
                const int r = i / BR_TILE_C, cc = i % BR_TILE_C;
                tile[r][cc] = cc < cols ? l.wA[(size_t)(m0 + r) * C + c0 + cc] : 0.f;
            }
            __syncthreads();
            if (t < rows)
                for (int cc = 0; cc < cols; ++cc) {
                    const float a = tile[t][cc];
#pragma unroll
                    for (int k = 0; k < 9; ++k) acc[k] = fmaf(go[(c0 + cc) * 9 + k], a, acc[k]);
                }
        }
        if (t < rows) {
#pragma unroll
            for (int k = 0; k < 9; ++k) l.dwB[((size_t)o * K2 + m0 + t) * 9 + k] = acc[k];
        }
    }
}

// partial[slab][m][c] of dwA for the 8 rows m of this work-group: threads 0..127 take rows mg*8 + 0..3, threads 128..255 rows + 4..7
__device__ __forceinline__ void br_bwd_dwA(const BrBwdLayer &l, int slab, int mg)
{
    const int C = l.C, K2 = 2 * C, t = threadIdx.x;
    const int half = __builtin_amdgcn_readfirstlane(t >> 7);        // uniform in a wave: the wB reads below stay scalar
    const int m0 = mg * 2 * BR_DWA_M + half * BR_DWA_M;
    const int o0 = slab * BR_SLAB, o1 = min(l.O, o0 + BR_SLAB);
    for (int c = t & 127; c < C; c += 128) {
        float acc[BR_DWA_M] = {0.f, 0.f, 0.f, 0.f};
        for (int o = o0; o < o1; ++o) {
            const float *gp = l.g + ((size_t)o * C + c) * 9;
            const float *wp = l.wB + ((size_t)o * K2 + m0) * 9;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float gv = gp[k];
#pragma unroll
                for (int j = 0; j < BR_DWA_M; ++j)
                    if (m0 + j < K2) acc[j] = fmaf(wp[j * 9 + k], gv, acc[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < BR_DWA_M; ++j)
            if (m0 + j < K2) l.dwAp[((size_t)slab * K2 + m0 + j) * C + c] = acc[j];
    }
}

__global__ void __launch_bounds__(BR_BWD_THREADS) k_branch_merge_bwd(BrBwdAll a)
{
    __shared__ float tile[BR_BWD_THREADS][BR_TILE_C + 1];
    int li = 0;
    while (li + 1 < a.n && (int)blockIdx.x >= a.blk_end[li]) ++li;
    const BrBwdLayer &l = a.l[li];
    int b = blockIdx.x - (li ? a.blk_end[li - 1] : 0);
    if (b < l.O) { br_bwd_row(l, b, &tile[0][0]); return; }
    b -= l.O;
    if (b < l.O) { br_bwd_dwB(l, b, tile); return; }
    b -= l.O;
    const int mgs = (2 * l.C + 2 * BR_DWA_M - 1) / (2 * BR_DWA_M);
    br_bwd_dwA(l, b / mgs, b % mgs);
}

// dwA[m,c] = the slabs' partial sums added in slab order
struct BrSumAll { int n; int blk_end[ORN_MAX_LAYERS]; struct { const float *part; float *out; int nslab; long len; } l[ORN_MAX_LAYERS]; };
__global__ void __launch_bounds__(256) k_branch_merge_bwd_sum(BrSumAll a)
{
    int li = 0;
    while (li + 1 < a.n && (int)blockIdx.x >= a.blk_end[li]) ++li;
    const long i = (long)(blockIdx.x - (li ? a.blk_end[li - 1] : 0)) * 256 + threadIdx.x;
    if (i >= a.l[li].len) return;
    float acc = 0.f;
    for (int s = 0; s < a.l[li].nslab; ++s) acc += a.l[li].part[(long)s * a.l[li].len + i];
    a.l[li].out[i] = acc;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------------
static bool br_kind_ok(int kind) { return kind == ORN_BRANCH_ACB || kind == ORN_BRANCH_REPVGG || kind == ORN_BRANCH_ECB; }

size_t orn_branch_merge_bwd_ws_floats(int kind, int C, int O)
{
    return kind == ORN_BRANCH_ECB ? (size_t)orn_cdiv(O, BR_SLAB) * 2 * C * C : 0;
}

int orn_launch_branch_merge_fwd(int n, const OrnBranchLayer *L, hipStream_t st)
{
    if (n <= 0) return 0;
    BrFwdAll a = {};
    a.n = n;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        const OrnBranchLayer &s = L[i];
        BrFwdLayer &d = a.l[i];
        d.kind = s.kind; d.C = s.C; d.O = s.O;
        d.w3x3 = s.p.w3x3; d.b3x3 = s.p.b3x3;
        if (s.kind == ORN_BRANCH_ACB) { d.wa = s.p.w1x3; d.ba = s.p.b1x3; d.wb = s.p.w3x1; d.bb = s.p.b3x1; }
        else if (s.kind == ORN_BRANCH_REPVGG) { d.wa = s.p.w1x1; d.ba = s.p.b1x1; }
        else {
            d.wa = s.p.wA; d.wb = s.p.wB;
            for (int t = 0; t < 3; ++t) { d.k0[t] = s.p.sb[t].k0; d.scale[t] = s.p.sb[t].scale; d.bias[t] = s.p.sb[t].bias; d.mask[t] = s.p.sb[t].mask; }
        }
        d.wf = s.wf; d.bf = s.bf;
        blocks += s.O;
        a.blk_end[i] = blocks;
    }
    hipLaunchKernelGGL(k_branch_merge_fwd, dim3(blocks), dim3(BR_FWD_THREADS), 0, st, a);
    ORN_LAUNCH_CHECK("branch_merge_fwd");
    return 0;
}

int orn_launch_branch_merge_bwd(int n, const OrnBranchLayer *L, hipStream_t st)
{
    if (n <= 0) return 0;
    BrBwdAll a = {};
    BrSumAll sm = {};
    a.n = n;
    int blocks = 0, sblocks = 0;
    for (int i = 0; i < n; ++i) {
        const OrnBranchLayer &s = L[i];
        BrBwdLayer &d = a.l[i];
        d.kind = s.kind; d.C = s.C; d.O = s.O; d.nslab = orn_cdiv(s.O, BR_SLAB);
        d.g = s.g; d.dbf = s.dbf;
        d.d3x3 = s.d.w3x3; d.db3x3 = s.d.b3x3;
        blocks += s.O;
        if (s.kind == ORN_BRANCH_ACB) { d.da = s.d.w1x3; d.dba = s.d.b1x3; d.db = s.d.w3x1; d.dbb = s.d.b3x1; }
        else if (s.kind == ORN_BRANCH_REPVGG) { d.da = s.d.w1x1; d.dba = s.d.b1x1; }
        else {
            d.wA = s.p.wA; d.wB = s.p.wB; d.dwA = s.d.wA; d.dwB = s.d.wB; d.dwAp = s.dwAp;
            for (int t = 0; t < 3; ++t) {
                d.k0[t] = s.p.sb[t].k0; d.scale[t] = s.p.sb[t].scale; d.mask[t] = s.p.sb[t].mask;
                d.dk0[t] = s.d.sb[t].k0; d.db0[t] = s.d.sb[t].b0; d.dscale[t] = s.d.sb[t].scale; d.dbias[t] = s.d.sb[t].bias;
                d.dmask[t] = s.d.sb[t].mask;
            }
            blocks += s.O + d.nslab * orn_cdiv(2 * s.C, 2 * BR_DWA_M);
            sm.l[sm.n].part = s.dwAp; sm.l[sm.n].out = s.d.wA; sm.l[sm.n].nslab = d.nslab; sm.l[sm.n].len = (long)2 * s.C * s.C;
            sblocks += orn_cdiv(sm.l[sm.n].len, 256);
            sm.blk_end[sm.n++] = sblocks;
        }
        a.blk_end[i] = blocks;
    }
    hipLaunchKernelGGL(k_branch_merge_bwd, dim3(blocks), dim3(BR_BWD_THREADS), 0, st, a);
    ORN_LAUNCH_CHECK("branch_merge_bwd");
    if (sm.n) {
        hipLaunchKernelGGL(k_branch_merge_bwd_sum, dim3(sblocks), dim3(256), 0, st, sm);
        ORN_LAUNCH_CHECK("branch_merge_bwd_sum");
    }
    return 0;
}

// ---- C ABI (per op) --------------------------------------------------------------------------------------------------------
static int br_check_ptrs(const char *what, int kind, const orn_branch_ptrs *p, bool grads)
{
    ORN_REQUIRE(p && p->w3x3 && p->b3x3, "%s: null 3x3 pointer", what);
    if (kind == ORN_BRANCH_ACB) ORN_REQUIRE(p->w3x1 && p->b3x1 && p->w1x3 && p->b1x3, "%s: null ACB pointer", what);
    if (kind == ORN_BRANCH_REPVGG) ORN_REQUIRE(p->w1x1 && p->b1x1, "%s: null RepVGG pointer", what);
    if (kind == ORN_BRANCH_ECB) {
        ORN_REQUIRE(p->wA && p->wB, "%s: null ECB pointer (wA / wB)", what);
        for (int t = 0; t < 3; ++t)
            ORN_REQUIRE(p->sb[t].k0 && p->sb[t].scale && p->sb[t].bias && p->sb[t].mask && (!grads || p->sb[t].b0),
                        "%s: null ECB pointer (branch %d)", what, t);
    }
    return 0;
}

extern "C" int orn_branch_merge_fwd(int kind, const orn_branch_ptrs *p, int C, int O, float *wf, float *bf, void *stream)
{
    ORN_REQUIRE(br_kind_ok(kind), "branch_merge_fwd: kind %d is not ORN_BRANCH_ACB / _REPVGG / _ECB", kind);
    ORN_REQUIRE(C > 0 && O > 0 && wf && bf, "branch_merge_fwd: bad sizes C=%d O=%d or null output", C, O);
    ORN_TRY(br_check_ptrs("branch_merge_fwd", kind, p, false));
    OrnBranchLayer l = {};
    l.kind = kind; l.C = C; l.O = O; l.p = *p; l.wf = wf; l.bf = bf;
    return orn_launch_branch_merge_fwd(1, &l, (hipStream_t)stream);
}

extern "C" size_t orn_branch_merge_bwd_ws_bytes(int kind, int C, int O)
{
    if (!br_kind_ok(kind) || C <= 0 || O <= 0) return 0;
    return orn_align(orn_branch_merge_bwd_ws_floats(kind, C, O) * sizeof(float) + 1);
}

extern "C" int orn_branch_merge_bwd(int kind, const orn_branch_ptrs *p, const float *g, const float *dbf, int C, int O,
                                    const orn_branch_ptrs *grads, void *ws, size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(br_kind_ok(kind), "branch_merge_bwd: kind %d is not ORN_BRANCH_ACB / _REPVGG / _ECB", kind);
    ORN_REQUIRE(C > 0 && O > 0 && g && dbf, "branch_merge_bwd: bad sizes C=%d O=%d or null gradient", C, O);
    ORN_TRY(br_check_ptrs("branch_merge_bwd", kind, grads, true));
    OrnBranchLayer l = {};
    l.kind = kind; l.C = C; l.O = O; l.g = g; l.dbf = dbf; l.d = *grads;
    if (kind == ORN_BRANCH_ECB) {
        ORN_TRY(br_check_ptrs("branch_merge_bwd", kind, p, false));
        l.p = *p;
        ORN_REQUIRE(ws && (uintptr_t)ws % 4 == 0, "branch_merge_bwd: ECB needs a float-aligned workspace");
        if (ws_bytes < orn_branch_merge_bwd_ws_bytes(kind, C, O)) {
            orn_set_error("branch_merge_bwd: workspace %zu < %zu", ws_bytes, orn_branch_merge_bwd_ws_bytes(kind, C, O));
            return ORN_E_WS;
        }
        l.dwAp = (float *)ws;
    }
    return orn_launch_branch_merge_bwd(1, &l, (hipStream_t)stream);
}
