// The tile machine of the SSIM gradient, shared by k_fusion6 (orn_loss.hip) and k_msssim_level_bwd (orn_loss_msssim.hip), with the
// Gaussian tap table of the loss kernels and the level means of MS-SSIM.  What the two kernels promise each other -- the LDS layout,
// the register blocking and the fmaf order of every filter -- holds because both call the functions below.
// A work-group of 256 threads owns a 16x64 tile of the gradient.  It needs the derivative maps on the tile + a 10-pixel apron (adjoint
// of the valid 11x11 filter), hence pred and target on the tile + a 20-pixel apron: the five filtered maps and the three derivative
// maps are RECOMPUTED on the apron (2.9x / 1.9x the arithmetic of the tile alone: the separable filters are cheap VALU work) and never
// leave LDS.  Register-blocked separable filtering: every thread produces 4 adjacent outputs from a 14-wide window (3x fewer LDS
// reads than one output per thread).  The passes below run in the order they stand in, a barrier between each two.
//   LDS (80 KB, two work-groups per CU):  X [2][36][88] p, t patch | Hm [5][36][76] row-filtered p, t, p^2, t^2, pt
//                                         D [3][26][76] dS/dm, dS/dq, dS/dr (over X) | Hh [3][26][64] row-adjoint of D (over Hm)
#pragma once
#include <initializer_list>
#include "orn_internal.h"

#define ST_TH 16
#define ST_TW 64
#define ST_PH (ST_TH + 20)
#define ST_PWP 88            // 84 columns used
#define ST_DH (ST_TH + 10)
#define ST_DWP 76            // 74 columns used
#define ST_RPT 9             // rows per thread of the column filter
#define ST_LDS_FLOATS (2 * ST_PH * ST_PWP + 5 * ST_PH * ST_DWP + 16)

// orn_gauss_taps.  The library is not linked as relocatable device code: every file that includes this header has its own copy
// (static), filled by its own orn_ssim_tile_init.
static __constant__ float c_gauss[11];
static __constant__ const float c_ms_weights[5] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};      // pytorch_msssim's level weights

// Uploads this file's tap table and lets `kerns` use the tile machine's dynamic LDS.  Must be called once outside any graph capture
// (hipMemcpyToSymbol is synchronous).
static int orn_ssim_tile_init(std::initializer_list<const void *> kerns)
{
    static bool done = false;
    if (done) return 0;
    float g[11];
    orn_gauss_taps(g);
    hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(c_gauss), g, sizeof(g));
    for (const void *k : kerns)
        if (e == hipSuccess) e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, ST_LDS_FLOATS * 4);
    if (e != hipSuccess) { orn_set_error("loss: init failed: %s", hipGetErrorString(e)); return (int)e; }
    done = true;
    return 0;
}

// The float4 load path of the loss kernels: rows of whole float4s, 16-byte aligned planes (planes: their addresses, or-ed), and a
// frame offset that keeps them so
static inline bool orn_loss_vec4(int W, uintptr_t planes, size_t frame_stride, const int *frame_idx)
{
    return W % 4 == 0 && planes % 16 == 0 && (frame_stride % 4 == 0 || !frame_idx);
}

// ---- patch rows y0-10 .. y0+25, columns x0-10 .. x0+73 (LDS column c <-> image column x0 - 10 + c); zero outside the image
__device__ __forceinline__ void st_load_patch(float *Xp, float *Xt, const float *pp, const float *tp, int y0, int x0, int H, int W, int vec4, int t)
{
    if (vec4) {           // rows are 16-byte aligned: float4 units from image column x0 - 12
        constexpr int NU = 22, NIT = (ST_PH * NU + 255) / 256;
        float4 ra[NIT], rb[NIT];
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = t + it * 256;
            const int r = idx / NU, u = idx - r * NU;
            const int gy = y0 - 10 + r, gx = x0 - 12 + 4 * u;
            ra[it] = make_float4(0.f, 0.f, 0.f, 0.f); rb[it] = ra[it];
            if (idx < ST_PH * NU && gy >= 0 && gy < H && gx >= 0 && gx < W) {
                ra[it] = *reinterpret_cast<const float4 *>(pp + (size_t)gy * W + gx);
                rb[it] = *reinterpret_cast<const float4 *>(tp + (size_t)gy * W + gx);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int idx = t + it * 256;
            const int r = idx / NU, u = idx - r * NU;
            if (idx < ST_PH * NU) {
                const int c = 4 * u - 2;
                if (u > 0) {
                    *reinterpret_cast<float2 *>(Xp + r * ST_PWP + c) = make_float2(ra[it].x, ra[it].y);
                    *reinterpret_cast<float2 *>(Xt + r * ST_PWP + c) = make_float2(rb[it].x, rb[it].y);
                }
                *reinterpret_cast<float2 *>(Xp + r * ST_PWP + c + 2) = make_float2(ra[it].z, ra[it].w);
                *reinterpret_cast<float2 *>(Xt + r * ST_PWP + c + 2) = make_float2(rb[it].z, rb[it].w);
            }
        }
    } else {
        constexpr int NL = (ST_PH * ST_PWP + 255) / 256;
#pragma unroll 1
        for (int it = 0; it < NL; ++it) {
            const int idx = t + it * 256;
            const int r = idx / ST_PWP, c = idx - r * ST_PWP;
            const int gy = y0 - 10 + r, gx = x0 - 10 + c;
            float a = 0.f, b = 0.f;
            if (idx < ST_PH * ST_PWP && gy >= 0 && gy < H && gx >= 0 && gx < W) { a = pp[(size_t)gy * W + gx]; b = tp[(size_t)gy * W + gx]; }
            if (idx < ST_PH * ST_PWP) { Xp[idx] = a; Xt[idx] = b; }
        }
    }
}

// ---- row filter: Hm[m][r][j] = sum_k g[k] X[r][j + k], j < 76 (74 used); item = (row r, 4 columns).  P_MAPS / T_MAPS: p, p^2, pt / t, t^2
template <bool P_MAPS, bool T_MAPS>
__device__ __forceinline__ void st_row_filter(const float *Xp, const float *Xt, float *Hm, int t)
{
    for (int idx = t; idx < ST_PH * (ST_DWP / 4); idx += 256) {
        const int r = idx / (ST_DWP / 4), c4 = (idx - r * (ST_DWP / 4)) * 4;
        float a[16], b[16];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float4 va = *reinterpret_cast<const float4 *>(Xp + r * ST_PWP + c4 + 4 * k);
            const float4 vb = *reinterpret_cast<const float4 *>(Xt + r * ST_PWP + c4 + 4 * k);
            a[4 * k] = va.x; a[4 * k + 1] = va.y; a[4 * k + 2] = va.z; a[4 * k + 3] = va.w;
            b[4 * k] = vb.x; b[4 * k + 1] = vb.y; b[4 * k + 2] = vb.z; b[4 * k + 3] = vb.w;
        }
        float sp[4] = {0, 0, 0, 0}, st[4] = {0, 0, 0, 0}, spp[4] = {0, 0, 0, 0}, stt[4] = {0, 0, 0, 0}, spt[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 14; ++k) {
            const float aa = a[k] * a[k], bb = b[k] * b[k], ab = a[k] * b[k];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                const int tap = k - o;
                if (tap >= 0 && tap < 11) {
                    const float g = c_gauss[tap];
                    if (P_MAPS) { sp[o] = fmaf(g, a[k], sp[o]); spp[o] = fmaf(g, aa, spp[o]); spt[o] = fmaf(g, ab, spt[o]); }
                    if (T_MAPS) { st[o] = fmaf(g, b[k], st[o]); stt[o] = fmaf(g, bb, stt[o]); }
                }
            }
        }
        float *h = Hm + r * ST_DWP + c4;
        if (P_MAPS) {
            *reinterpret_cast<float4 *>(h) = make_float4(sp[0], sp[1], sp[2], sp[3]);
            *reinterpret_cast<float4 *>(h + 2 * ST_PH * ST_DWP) = make_float4(spp[0], spp[1], spp[2], spp[3]);
            *reinterpret_cast<float4 *>(h + 4 * ST_PH * ST_DWP) = make_float4(spt[0], spt[1], spt[2], spt[3]);
        }
        if (T_MAPS) {
            *reinterpret_cast<float4 *>(h + ST_PH * ST_DWP) = make_float4(st[0], st[1], st[2], st[3]);
            *reinterpret_cast<float4 *>(h + 3 * ST_PH * ST_DWP) = make_float4(stt[0], stt[1], stt[2], stt[3]);
        }
    }
}

// ---- column filter of map m on valid-map rows y0-10+i (i < 26), columns x0-10+j (j < 74): v[o] = the map at row r4 + o, column j.
// item = (column j, 9 rows from r4), threads t < 3 * ST_DWP: row group rg = t / ST_DWP, j = t - rg * ST_DWP, r4 = 9 * rg, but the
// third row group restarts at row 17 (rows 17..25: row 17 is computed twice, same value).  The callers loop over the maps the row
// filter formed: one call per map keeps 3 to 5 VGPRs less than a loop over the maps in here.
__device__ __forceinline__ void st_col_filter(const float *Hm, int m, int r4, int j, float (&v)[ST_RPT])
{
    float col[ST_RPT + 10];
#pragma unroll
    for (int k = 0; k < ST_RPT + 10; ++k) col[k] = Hm[(m * ST_PH + r4 + k) * ST_DWP + j];
#pragma unroll
    for (int o = 0; o < ST_RPT; ++o) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 11; ++k) acc = fmaf(c_gauss[k], col[o + k], acc);
        v[o] = acc;
    }
}

// ---- derivative maps of one valid-map pixel with respect to the filtered G*p (dm), G*p^2 (dq) and G*pt (dr), from the five filtered
// values m = G*p, mu = G*t, qq = G*p^2, tt = G*t^2, rr = G*pt: of the SSIM map, or of the CS map (MS-SSIM levels
// 0..3); returns the map's value.  Reciprocals as v_rcp_f32 + one Newton step (< 1 ulp) instead of IEEE divisions (~10 instructions each).
template <bool SSIM>
__device__ __forceinline__ float st_deriv(float m, float mu, float qq, float tt, float rr, float &dm, float &dq, float &dr)
{
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float sp = qq - m * m, st = tt - mu * mu, spt = rr - m * mu;
    const float A2 = 2.f * spt + C2, B2 = sp + st + C2;
    float i2 = __builtin_amdgcn_rcpf(B2);
    i2 = i2 * (2.0f - B2 * i2);
    if (!SSIM) {
        const float cs = A2 * i2;
        dm = (2.f * m * cs - 2.f * mu) * i2;
        dq = -cs * i2;
        dr = 2.f * i2;
        return cs;
    }
    // (m * m + mu * mu written out: the compiler contracts either product, and not the same one in every kernel it is inlined into)
    const float A1 = 2.f * m * mu + C1, B1 = fmaf(m, m, __fmul_rn(mu, mu)) + C1;
    float i1 = __builtin_amdgcn_rcpf(B1);
    i1 = i1 * (2.0f - B1 * i1);
    const float inv = i1 * i2;
    const float S = A1 * A2 * inv;
    dm = 2.f * mu * (A2 - A1) * inv - 2.f * m * S * i1 + 2.f * m * S * i2;
    dq = -S * i2;
    dr = 2.f * A1 * inv;
    return S;
}

// D[.][i][j]: over the patch, which is dead since the barrier behind the row filter
__device__ __forceinline__ void st_store_deriv(float *Dm, int i, int j, float dm, float dq, float dr)
{
    float *d = Dm + i * ST_DWP + j;
    d[0] = dm; d[ST_DH * ST_DWP] = dq; d[2 * ST_DH * ST_DWP] = dr;
}

// ---- adjoint row filter: Hh[m][i][c] = sum_k g[k] D[m][i][c + 10 - k]; item = (row i, 4 columns, map m)
__device__ __forceinline__ void st_adj_row(const float *Dm, float *Hh, int t)
{
#pragma unroll 2      // 416 items over 256 threads: both trips in flight, as the compiler unrolls the loop written out in a kernel
    for (int idx = t; idx < ST_DH * (ST_TW / 4); idx += 256) {
        const int r = idx / (ST_TW / 4), c4 = (idx - r * (ST_TW / 4)) * 4;
#pragma unroll
        for (int m = 0; m < 3; ++m) {
            float w[16];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float4 vv = *reinterpret_cast<const float4 *>(Dm + (m * ST_DH + r) * ST_DWP + c4 + 4 * k);
                w[4 * k] = vv.x; w[4 * k + 1] = vv.y; w[4 * k + 2] = vv.z; w[4 * k + 3] = vv.w;
            }
            float hv[4];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                float acc = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) acc = fmaf(c_gauss[k], w[o + 10 - k], acc);
                hv[o] = acc;
            }
            *reinterpret_cast<float4 *>(Hh + (m * ST_DH + r) * ST_TW + c4) = make_float4(hv[0], hv[1], hv[2], hv[3]);
        }
    }
}

// ---- adjoint column filter: thread = (column c, 4 rows from r4) of the tile; am, aq, ar = G^T dm, G^T dq, G^T dr
__device__ __forceinline__ void st_adj_col(const float *Hh, int r4, int c, float (&am)[4], float (&aq)[4], float (&ar)[4])
{
#pragma unroll
    for (int m = 0; m < 3; ++m) {
        float col[4 + 10];
#pragma unroll
        for (int k = 0; k < 4 + 10; ++k) col[k] = Hh[(m * ST_DH + r4 + k) * ST_TW + c];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) acc = fmaf(c_gauss[k], col[o + 10 - k], acc);
            if (m == 0) am[o] = acc; else if (m == 1) aq[o] = acc; else ar[o] = acc;
        }
    }
}

// The mean of one MS-SSIM level of plane `pl`: the level's {ssim, cs} tile partials (part [planes][nblk][2]) walked in tile order in
// double; cs at levels 0..3, ssim at level 4.  The MS-SSIM value of a plane is prod_lv relu(mean)^c_ms_weights[lv], formed in double.
__device__ __forceinline__ double orn_msssim_level_mean(const float *part, size_t pl, int nblk, float nmap, int lv)
{
    double ss = 0.0, cs = 0.0;
    for (int b = 0; b < nblk; ++b) {
        ss += (double)part[2 * (pl * nblk + b)];
        cs += (double)part[2 * (pl * nblk + b) + 1];
    }
    return (lv < 4 ? cs : ss) / (double)nmap;
}
