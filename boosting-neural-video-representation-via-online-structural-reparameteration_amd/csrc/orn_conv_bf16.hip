// A4 fast path: the NeRVBlock conv (model.py:539,567) and its backward on bf16 MFMA
// (v_mfma_f32_32x32x16_bf16, fp32 accumulate) for the layers that carry 99 % of the step's FLOPs
// (C_in % 96 == 0).  Activations live in HBM as channels-last bf16 with a one-pixel zero border:
//
//   xpad [H+2][W+2][C]      conv input  (= previous block's a = SiLU(z), border = conv zero padding)
//   z    [Hs][Ws][Cn]       pre-activation after PixelShuffle (kept for SiLU')
//   dypad[H+2][W+2][O']     gradient wrt the conv output, out-channel order o' = (i*s+j)*Cn + n so
//                           that PixelShuffle / unshuffle move whole Cn-channel rows
//   Wb   [9][O'][C]         merged kernel, bf16, tap-major, o' order        (forward B operand)
//   Wd   [9][C][O']         flipped taps, transposed                        (dgrad B operand)
//
// conv (fwd and dgrad share one kernel): work-group = 8x32 output pixels; the (8+2)x(32+2) input
// patch of a 96-channel chunk stays in LDS for all 9 taps (and all N tiles) -- each input byte is
// read 1.33x instead of 9x -- while [BN][96] weight tiles stream from L2 through a double-buffered
// LDS stage.  wgrad: work-group = 128 out channels x one kernel row (3 taps) x all 96 in-channels,
// K = pixels, both operands pixel-major in LDS and read with ds_read_b64_tr_b16.
// This file is compiled twice: as is (bf16, namespace orn_bf16) and with -DORN_FP16 (IEEE half, namespace
// orn_f16: 11-bit significand, same MFMA rate; gradients then travel scaled by 2^20, see the engine).
#include "orn_internal.h"
#include <type_traits>
#include <cstdlib>
#ifdef ORN_FP16
#define HNS orn_f16
typedef _Float16 h16;
#define MFMA_H16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0)
#else
#define HNS orn_bf16
typedef __bf16 h16;
#define MFMA_H16(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
#endif
typedef __attribute__((ext_vector_type(8))) h16 h16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
// The conv kernels (forward / dgrad) run on v_mfma_f32_16x16x32: at equal cycles per FLOP the chip holds a higher clock under
// this shape than under 32x32x16 (MI355X_MICROARCH.md, DVFS item 7; measured here: -7 % forward, -9 % dgrad kernel time).
// The wgrad keeps 32x32x16 (its transposed-read operand path is built around it and the same swap made it slower).
#ifdef ORN_FP16
#define MFMA16_H16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0)
#else
#define MFMA16_H16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0)
#endif
typedef __attribute__((ext_vector_type(4))) h16 h16x4;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;

// compile-time loop: f(std::integral_constant<int, I>{}) for I in [I0, N)
template <int I, int N, class F>
__device__ __forceinline__ void orn_sfor(F &&f)
{
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        orn_sfor<I + 1, N>(f);
    }
}

namespace HNS {

// The timing-ablation flags cost registers and branches in the hot loops: they are compiled in only with
// -DORN_CONV_ABLATE (tools/probes builds); product builds see a constant 0.
#ifdef ORN_CONV_ABLATE
#define PDBG(p_) ((p_).dbg)
#else
#define PDBG(p_) 0
#endif

#include "orn_wgrad_body.h"     // WgradBP, wgrad_body (also ridden by orn_conv2_bf16.hip's dgrad launch)
static int g_conv_dbg = 0;   // timing experiments only (tools/probes), see orn_debug_set
// Phase stamps (diagnostic build -DORN_CONV_STAMP; the product build compiles none of it): wave 0 of every work-group writes
// s_memtime at the N-tile phase boundaries into a buffer no other code reads.
#ifdef ORN_CONV_STAMP
static unsigned long long *g_conv_stamps = nullptr;
// stamps collect in 512 B of LDS behind the kernel's own images (a global store per stamp would sit in every vmcnt wait)
#define STAMP_LDS ((unsigned long long *)(smem + PATCH_LDS + NBUF * BS_BYTES + 0))
#define STAMP(i_) { if (p.stamps && t == 0) STAMP_LDS[i_] = __builtin_amdgcn_s_memtime(); }
#define STAMP_RT(i_) { if (p.stamps && t == 0) STAMP_LDS[i_] = __builtin_amdgcn_s_memrealtime(); }
#define STAMP_FLUSH() { if (p.stamps && t < 128) p.stamps[(size_t)(blockIdx.x + blockIdx.y * gridDim.x) * 128 + t] = STAMP_LDS[t]; }
// per-tap stamps of wave 0 (slots 16..) and of the wave that shares its SIMD (slots 64..): up to 4 N tiles / chunks x 9 taps
#define STAMP_TAP(seg_, tap_) { if (p.stamps && (seg_) < 4 && lane == 0 && (wave == 0 || wave == NWAVES / 2)) STAMP_LDS[(wave == 0 ? 16 : 64) + (seg_) * 9 + (tap_)] = __builtin_amdgcn_s_memtime(); }
// rendezvous of taps 3..5 of segment 0: arrival (k 0), after the vmcnt wait (1), after the barrier (2); wave 0 -> slots 100.., partner -> 112..
#define STAMP_BAR(seg_, tap_, k_) { if (p.stamps && (seg_) == 0 && (tap_) >= 3 && (tap_) <= 5 && lane == 0 && (wave == 0 || wave == NWAVES / 2)) STAMP_LDS[(wave == 0 ? 100 : 112) + ((tap_) - 3) * 3 + (k_)] = __builtin_amdgcn_s_memtime(); }
#else
#define STAMP(i_)
#define STAMP_RT(i_)
#define STAMP_FLUSH()
#define STAMP_TAP(seg_, tap_)
#define STAMP_BAR(seg_, tap_, k_)
#endif

#define CB_TH 8
#define CB_TW 32
#define CB_PH (CB_TH + 2)
#define CB_PW (CB_TW + 2)
#define CB_CK 96                 // channels per K chunk
#define CB_PIXB 208              // LDS bytes per patch pixel (192 data + 16 pad: conflict-free b128 reads)
#define CB_PATCH_BYTES (CB_PH * CB_PW * CB_PIXB)
#define CB_ROWB 208              // LDS bytes per weight-tile row

// EPI_B_FWD_LAST: the forward of the last block (no activation copy for a next layer): its own instantiation, so the
// largest launch of the step carries neither the second set of deferred-store registers nor the SiLU code
enum { EPI_B_FWD = 0, EPI_B_DGRAD = 1, EPI_B_DGRAD_F32 = 2, EPI_B_FWD_LAST = 3 };
#define EPI_IS_FWD(e_) ((e_) == EPI_B_FWD || (e_) == EPI_B_FWD_LAST)

typedef __attribute__((ext_vector_type(2))) h16 h16x2;
__device__ __forceinline__ unsigned pack_h16x2(float lo, float hi)
{
    h16x2 v;
    v[0] = (h16)lo;
    v[1] = (h16)hi;
    return __builtin_bit_cast(unsigned, v);
}
// v_permlane32_swap: lanes 32-63 of `a` <-> lanes 0-31 of `b` (guide T21).  After the call lanes < 32
// hold (own a, upper half's a) and lanes >= 32 hold (lower half's b, own b).
__device__ __forceinline__ void swap_halves(unsigned &a, unsigned &b)
{
    const auto r = __builtin_amdgcn_permlane32_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}
__device__ __forceinline__ void swap_halves_f(float &a, float &b)
{
    unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
    swap_halves(ua, ub);
    a = __builtin_bit_cast(float, ua);
    b = __builtin_bit_cast(float, ub);
}

// v_permlane16_swap: odd 16-lane rows of `a` <-> even rows of `b`.  Afterwards rows 0 / 2 hold (own a, the next row's a) and
// rows 1 / 3 hold (the previous row's b, own b) -- checked on hardware with tools/probes (row = lane >> 4).
__device__ __forceinline__ void swap_rows(unsigned &a, unsigned &b)
{
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    a = r[0];
    b = r[1];
}
__device__ __forceinline__ void swap_rows_f(float &a, float &b)
{
    unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
    swap_rows(ua, ub);
    a = __builtin_bit_cast(float, ua);
    b = __builtin_bit_cast(float, ub);
}

__device__ __forceinline__ int conv_div(int x, unsigned m) { return m ? (int)__umulhi((unsigned)x, m) : x; }

struct ConvBP {
    const h16 *xpad;     // [H+2][W+2][Cin]
    const h16 *w;        // [9][Nout][Cin]
    const float *bias;   // [Nout] (o' order) or null
    int H, W, Cin, Nout;
    int tiles_w, tiles_h, n_tiles_per_wg;
    int n_full;          // work-groups [0, n_full) own whole pixel tiles; the rest own one N tile each
    int qsplit;          // EPI_B_DGRAD_F32 on small images: blockIdx.y = input chunk, one fp32 partial slab per chunk
    // EPI_B_FWD
    h16 *z;              // [H*s][W*s][Cn]
    h16 *apad;           // [H*s+2][W*s+2][Cn] or null
    int s, Cn;
    unsigned z_bytes, apad_bytes;   // sizes of the two buffers (raw-buffer bounds)
    // EPI_B_DGRAD: out = dx * silu'(zprev) scattered into the previous layer's dypad
    const h16 *zprev;    // [H][W][Nout]
    h16 *dyprev;         // [H/sp+2][W/sp+2][Nout*sp*sp]
    int sp;
    // EPI_B_DGRAD_F32
    float *dx_f32;       // [H][W][Nout]
    // exact division by multiply-high for the epilogues' index math (a runtime integer division costs ~30 instructions,
    // and 16 of them per N tile per lane were a measurable part of the forward kernel): conv_div / conv_magic
    unsigned mCn, mS, mSp;
    int dbg;             // timing-only ablation flags (tools/probes): 1 no weight restage, 2 no patch stage, 4 no stores
    unsigned long long *stamps;   // -DORN_CONV_STAMP diagnostic builds only: 64 time stamps per work-group (tools/probes/conv_stamps.py)
};

// Fragment register sets: reads run CONV_NSET - 1 k-steps ahead of the MFMAs that consume them
#ifndef CONV_NSET_DGRAD
#define CONV_NSET_DGRAD 2
#endif
// Fragment reads of k-step (TAP, KS_) -- 32 input channels -- into register set SET.  v_mfma_f32_16x16x32 operands: lane l
// (l15 = l & 15, g4 = l >> 4) holds 8 consecutive k of row / column l15 starting at k = 8 * g4, i.e. the 16-byte chunk
// c = 4 * KS_ + g4 of that LDS row.  fa: 2 * MB pixel sub-blocks (16 pixels: the MFMA's B operand / D columns); fb: 2 * NB
// channel sub-blocks (16 output channels: A operand / D rows).  LDS rows are swizzled: chunk c of row R sits at position
// c ^ ((R >> 1) & 3) (conflict-free ds_read_b128 for this lane map; the DMA applies the same XOR on its source address).
// a_lane = LDS byte address of the patch pixel (row wm*MB, column l15, tap 0), pix_lane = that pixel's index,
// b_lane = this lane's weight-row address with its swizzled chunk offset for KS_ = 0 folded in.
template <int NSET, int MB, int NB, int ROWB, int BS_BYTES, bool ALLTAPS, int SET, int TAP, int KS_>
__device__ __forceinline__ void conv_read_step(h16x8 (&fa)[NSET][2 * MB], h16x8 (&fb)[NSET][2 * NB], unsigned a_lane, unsigned pix_lane,
                                               unsigned b_lane, int g4)
{
    constexpr int ti = TAP / 3, tj = TAP - ti * 3;
    constexpr int buf = ALLTAPS ? TAP : TAP % 3;
    constexpr int kimm = 64 * KS_;
#pragma unroll
    for (int i = 0; i < 2 * MB; ++i) {
        const unsigned pixoff = ((i >> 1) + ti) * CB_PW + 16 * (i & 1) + tj;
        const unsigned pix = pix_lane + pixoff;
        const unsigned addr = a_lane + pixoff * ROWB + 16 * (g4 ^ ((pix >> 1) & 3));
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fa[SET][i]) : "v"(addr), "n"(kimm) : "memory");
    }
    const unsigned baddr = b_lane + (buf >= 4 ? 4 * BS_BYTES : 0);
    constexpr int bimm = (buf >= 4 ? buf - 4 : buf) * BS_BYTES + kimm;
    static_assert(bimm + (2 * NB - 1) * 16 * ROWB < 65536, "ds_read offset field");
    static_assert(NB <= 3, "conv_read_step: add the fourth weight block");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[SET][0]) : "v"(baddr), "n"(bimm) : "memory");
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[SET][1]) : "v"(baddr), "n"(bimm + 16 * ROWB) : "memory");
    if constexpr (NB > 1) {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[SET][NB > 1 ? 2 : 0]) : "v"(baddr), "n"(bimm + 32 * ROWB) : "memory");
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[SET][NB > 1 ? 3 : 0]) : "v"(baddr), "n"(bimm + 48 * ROWB) : "memory");
    }
    if constexpr (NB > 2) {
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[SET][NB > 2 ? 4 : 0]) : "v"(baddr), "n"(bimm + 64 * ROWB) : "memory");
        asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[SET][NB > 2 ? 5 : 0]) : "v"(baddr), "n"(bimm + 80 * ROWB) : "memory");
    }
}

// The wait that retires register set SET (its reads were issued before the PEND newest ones) names every register of the
// set as read-write, so no MFMA that consumes them can be scheduled above it.
template <int NSET, int MB, int NB, int SET, int PEND>
__device__ __forceinline__ void conv_wait_set(h16x8 (&fa)[NSET][2 * MB], h16x8 (&fb)[NSET][2 * NB])
{
    if constexpr (MB == 2 && NB == 2)
        asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(fa[SET][0]), "+v"(fa[SET][1]), "+v"(fa[SET][MB > 1 ? 2 : 0]), "+v"(fa[SET][MB > 1 ? 3 : 0]),
                     "+v"(fb[SET][0]), "+v"(fb[SET][1]), "+v"(fb[SET][NB > 1 ? 2 : 0]), "+v"(fb[SET][NB > 1 ? 3 : 0]) : "n"(PEND));
    else if constexpr (MB == 1 && NB == 3)
        asm volatile("s_waitcnt lgkmcnt(%8)" : "+v"(fa[SET][0]), "+v"(fa[SET][1]), "+v"(fb[SET][0]), "+v"(fb[SET][1]), "+v"(fb[SET][NB > 1 ? 2 : 0]),
                     "+v"(fb[SET][NB > 1 ? 3 : 0]), "+v"(fb[SET][NB > 2 ? 4 : 0]), "+v"(fb[SET][NB > 2 ? 5 : 0]) : "n"(PEND));
    else if constexpr (MB == 1 && NB == 1)
        asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(fa[SET][0]), "+v"(fa[SET][1]), "+v"(fb[SET][0]), "+v"(fb[SET][1]) : "n"(PEND));
    else
        static_assert(MB == 2 && NB == 2, "conv_wait_set: add this wave tile");
}

// The (2 MB) x (2 NB) MFMAs of one k-step on register set SET.
template <int NSET, int MB, int NB, int SET>
__device__ __forceinline__ void conv_mfma_step(h16x8 (&fa)[NSET][2 * MB], h16x8 (&fb)[NSET][2 * NB], f32x4 (&acc)[2 * MB][2 * NB])
{
#ifdef ORN_V_JOUTER
#pragma unroll
    for (int j = 0; j < 2 * NB; ++j)
#pragma unroll
        for (int i = 0; i < 2 * MB; ++i) acc[i][j] = MFMA16_H16(fb[SET][j], fa[SET][i], acc[i][j]);
#else
#pragma unroll
    for (int i = 0; i < 2 * MB; ++i)
#pragma unroll
        for (int j = 0; j < 2 * NB; ++j) acc[i][j] = MFMA16_H16(fb[SET][j], fa[SET][i], acc[i][j]);
#endif
}

// CK = input channels per K chunk: 96 (the general form above), or 32 for a layer whose input has <= 32 real channels
// (the zero-padded narrow layer, forward only): its whole K = 9 x 32 fits LDS -- patch 22 KB + all nine [BN][32] weight
// tiles 72 KB -- so an N tile is ONE rendezvous and 72 back-to-back MFMAs per wave instead of nine rounds of barrier +
// counted wait + 24 MFMAs of which two thirds multiply zeros.  Rows are 64 B: 4 chunks, XOR swizzle (chunk ^ ((row >> 1) & 3)).
// ALLTAPS: all nine weight tiles of the (single) K chunk resident, one rendezvous per N tile -- the narrow form, and the
// chunk-split dgrad of a layer with <= 32 real OUTPUT channels (N tile 32: 9 x 6 KB next to the 64 KB patch).
template <int WAVES_M, int WAVES_N, int MB, int NB, int EPI, int CK = CB_CK, bool ALLTAPS = (CK != CB_CK)>
__global__ void __launch_bounds__(WAVES_M *WAVES_N * 64) k_conv_nhwc_bf16(ConvBP p)
{
    ORN_PRIO_HIGH();
    static_assert(!EPI_IS_FWD(EPI) && CK == CB_CK, "this file holds the dgrad kernels (forward: orn_conv_fwd_bf16.hip)");
    constexpr bool NARROW = false;
    constexpr int NCH = CK / 8;                        // 16-byte chunks per LDS row
    static_assert(!NARROW || ALLTAPS, "the narrow form keeps all taps resident");
    constexpr int NBUF = ALLTAPS ? 9 : 3;              // weight tiles resident at once
    constexpr int NT = WAVES_M * WAVES_N * 64;
    constexpr int BN = WAVES_N * NB * 32;
    static_assert(WAVES_M * MB == CB_TH, "M tile must be 8 rows of 32 pixels");
    // LDS images: UNPADDED 192-byte rows (12 x 16-byte chunks) filled by LDS-DMA (global_load_lds_dwordx4: 1 KiB per
    // wave-instruction, lane-linear destination, no VGPRs, no ds_write).  Conflict-free ds_read_b128 comes from a
    // rotation swizzle -- logical chunk c of row R sits at position (c + ((R >> 2) & 3)) % 12 -- applied on the DMA's
    // per-lane SOURCE address and on the fragment reads (both sides or neither: guide rule 21).
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NWAVES = WAVES_M * WAVES_N;
    constexpr int ROWB = CK * 2;
    constexpr int PATCH_INSTR = (CB_PH * CB_PW * ROWB + 1023) / 1024;   // 340 pixels x 192 B = 65,280 -> 64 wave-instructions
    constexpr int PATCH_LDS = PATCH_INSTR * 1024;
    constexpr int BS_BYTES = BN * ROWB;
    constexpr int B_INSTR = BS_BYTES / 1024;           // wave-instructions per weight tile
    // Weight tiles are fetched by the FIRST HALF of the waves only (one per SIMD: waves w and w + NWAVES/2 share one): an
    // LDS-DMA instruction parks its wave for ~100 cycles, and when both waves of a SIMD issue theirs right after the
    // rendezvous the matrix pipe idles for all of them (~300 cycles per tap, measured with phase stamps); with one loader
    // per SIMD its partner's MFMAs run meanwhile, and the loader catches up while the partner waits at the next rendezvous.
    constexpr int NLOAD = (ALLTAPS || NWAVES < 8) ? NWAVES : NWAVES / 2;
    constexpr int B_PER_WAVE = (B_INSTR + NLOAD - 1) / NLOAD;
    constexpr int P_PER_WAVE = (PATCH_INSTR + NWAVES - 1) / NWAVES;
    static_assert((NARROW || PATCH_INSTR % NWAVES == 0) && BS_BYTES % 1024 == 0, "tile geometry");
    unsigned char *patch = smem;
    unsigned char *bs0 = smem + PATCH_LDS;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    // work list: the first n_full work-groups take a pixel tile with all its N tiles; the pixel tiles of the
    // last partial round are cut into single-N-tile work-groups so the tail spreads over every CU
    int tile = blockIdx.x, nt0 = blockIdx.y * p.n_tiles_per_wg, nt_cnt = p.n_tiles_per_wg;
    if ((int)blockIdx.x >= p.n_full) {
        const int r = blockIdx.x - p.n_full;
        tile = p.n_full + r / p.n_tiles_per_wg;
        nt0 = r - (r / p.n_tiles_per_wg) * p.n_tiles_per_wg;
        nt_cnt = 1;
    }
    const int tw = tile % p.tiles_w, th = tile / p.tiles_w;
    const int h0 = th * CB_TH, w0 = tw * CB_TW;
    const int H = p.H, W = p.W, Cin = p.Cin;
    const int q_base = (EPI == EPI_B_DGRAD_F32 && p.qsplit) ? (int)blockIdx.y : 0;   // chunk split: this WG's chunk
    // chunks of the input channels walked by one work-group (the all-taps-resident form is launched chunk-split: one)
    constexpr bool MULTI_CHUNK = !ALLTAPS;
    const int Q = (!MULTI_CHUNK || (EPI == EPI_B_DGRAD_F32 && p.qsplit)) ? 1 : Cin / CB_CK;
    if (EPI == EPI_B_DGRAD_F32 && p.qsplit) nt0 = 0;
    const int n_tiles = Q * 9;                         // weight tiles per N tile

    const int uwave = __builtin_amdgcn_readfirstlane(wave);        // provably wave-uniform (LDS-DMA base -> M0)
    // per-lane SOURCE offsets (elements) of this wave's DMA instructions; rot() un-swizzles position -> logical chunk
    // (unsigned BYTE offsets from a wave-uniform base: the DMA then takes its scalar-base + 32-bit-offset form instead of a
    // 64-bit address pair per piece kept in VGPRs across the whole loop)
    unsigned b_goff[B_PER_WAVE], p_goff[P_PER_WAVE];
    bool p_ok[P_PER_WAVE];
#pragma unroll
    for (int k = 0; k < B_PER_WAVE; ++k) {
        const int m = (uwave + NLOAD * k) % B_INSTR;               // surplus instructions re-load a tile piece (harmless)
        const int L = m * 64 + lane, R = L / NCH, pos = L - R * NCH;
        const int c = pos ^ ((R >> 1) & 3);
        b_goff[k] = (unsigned)(R * Cin + c * 8) * 2u;
    }
#pragma unroll
    for (int k = 0; k < P_PER_WAVE; ++k) {
        const int m = uwave + NWAVES * k;
        const int L = m * 64 + lane, pix = L / NCH, pos = L - pix * NCH;
        const int c = pos ^ ((pix >> 1) & 3);
        const int pr = pix / CB_PW, pc = pix - pr * CB_PW;
        const int gh = h0 + pr, gw_ = w0 + pc;
        p_ok[k] = (pix < CB_PH * CB_PW) && gh < H + 2 && gw_ < W + 2;
        // out-of-image pixels read the (0,0) border pixel, which is all zeros
        p_goff[k] = (unsigned)(p_ok[k] ? ((gh * (W + 2) + gw_) * Cin + c * 8) : c * 8) * 2u;
    }
#define DMA16(gptr_, ldsoff_)                                                                                   \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gptr_),                   \
                                     (__attribute__((address_space(3))) void *)(smem + (ldsoff_)), 16, 0, 0)
#define DMA_B(buf_, nt_, q_, tap_)                                                                              \
    {                                                                                                           \
        if (NLOAD == NWAVES || uwave < NLOAD) {                                                                 \
            const h16 *wbase = p.w + ((size_t)((tap_) * p.Nout + (nt_) * BN) * Cin + ((q_) + q_base) * CK);     \
            _Pragma("unroll") for (int k = 0; k < B_PER_WAVE; ++k)                                              \
                DMA16((const char *)wbase + b_goff[k], PATCH_LDS + (buf_) * BS_BYTES + ((uwave + NLOAD * k) % B_INSTR) * 1024); \
        }                                                                                                       \
    }
#define DMA_PATCH(q_)                                                                                           \
    {                                                                                                           \
        _Pragma("unroll") for (int k = 0; k < P_PER_WAVE; ++k)                                                  \
            if (!NARROW || uwave + NWAVES * k < PATCH_INSTR)                                                    \
                DMA16((const char *)p.xpad + (p_goff[k] + (p_ok[k] ? (unsigned)(((q_) + q_base) * CK) * 2u : 0u)), (uwave + NWAVES * k) * 1024);  \
    }
#define WAIT_VM(n_) asm volatile("s_waitcnt vmcnt(" #n_ ")" ::: "memory")
#define WAIT_VMC(n_) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n_) : "memory")
#define BARRIER() __builtin_amdgcn_s_barrier()
    // Fragment reads are hand-placed (inline asm: hipcc sinks every builtin LDS read next to its consumer and waits
    // lgkmcnt(0) right behind it, which exposed one LDS round trip per k-step); see conv_read_step for the operand map.
    // All addresses are LDS byte offsets in a VGPR.
    const int l15 = lane & 15, g4 = lane >> 4;
    const unsigned lds0 = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char *)smem;
    const unsigned b_lane = lds0 + PATCH_LDS + (wn * NB * 32 + l15) * ROWB + 16 * (g4 ^ ((l15 >> 1) & 3));   // weight row + chunk of k-step 0
    const unsigned a_lane = lds0 + (wm * MB * CB_PW + l15) * ROWB;                                         // patch pixel of (row wm*MB, tap 0)

    STAMP_RT(0)
    constexpr int NSET = CONV_NSET_DGRAD, LEAD = NSET - 1;   // reads run LEAD k-steps ahead of their MFMAs
    h16x8 fa[NSET][2 * MB], fb[NSET][2 * NB];           // fragment register sets (carried across N tiles by the pipeline)
    for (int nti = 0; nti < nt_cnt; ++nti) {
        const int nt = nt0 + nti;
        STAMP(2 + nti * 4)
        // acc[pi][ci]: 16 x 16 tiles.  D rows = 16 output channels (A operand = weights), D cols = 16 pixels (B operand = input
        // patch): pixel sub-block pi = 2 * row + half, channel sub-block ci; lane (l15, g4) owns pixel l15 of the sub-block and the
        // 4 consecutive channels 4 * g4 + r of the 16.
        f32x4 acc[2 * MB][2 * NB];
#pragma unroll
        for (int i = 0; i < 2 * MB; ++i)
#pragma unroll
            for (int j = 0; j < 2 * NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

        // prologue (every N tile of the all-taps-resident forms; otherwise once per work-group: the weight-tile ring then
        // runs on ACROSS N tiles -- the last three taps of an N tile fetch the first three tiles of the next one, so an N
        // tile boundary costs a rendezvous, not a drained pipeline): the patch (chunk 0) and weight tiles 0, 1; tile 2 stays
        // in flight behind the first rendezvous.
        const bool has_next_nt = (nti + 1 < nt_cnt);
        if (ALLTAPS || nti == 0) {
            BARRIER();
            if ((nti == 0 || (MULTI_CHUNK && Q > 1)) && !(PDBG(p) & 2)) DMA_PATCH(0)
            DMA_B(0, nt, 0, 0)
            if (n_tiles > 1) DMA_B(1, nt, 0, 1)
            if (ALLTAPS) {                             // the whole K of this N tile: taps 2..8 too, then the only rendezvous
#pragma unroll
                for (int tp = 2; tp < 9; ++tp) DMA_B(tp, nt, 0, tp)
            }
            WAIT_VM(0);
            BARRIER();
            if (!ALLTAPS && n_tiles > 2) DMA_B(2, nt, 0, 2)
        }
        // One software pipeline over all k-steps (chunks of 96 input channels outside; nine taps x CK/16 k-slices inside,
        // unrolled at compile time so tap, kernel row / column, ring slot, register set and LDS offsets are constants): step s
        // issues the fragment reads of step s+LEAD into another register set, waits with a COUNTED lgkmcnt for its own
        // (issued LEAD steps earlier), then runs its MFMAs -- also across a tap boundary, so the rendezvous at the end of a tap
        // sits between MFMAs whose operands are already in registers or in flight.  (LEAD = 2 measured the same as 1 on the
        // 720p shapes: CONV_NSET_* keep the knob.)  Reading tile t+1 before rendezvous t is legal because every wave waits for
        // ALL its outstanding DMA pieces (tile t+2 included) before rendezvous t: tile t+1 was complete, and known to be, at
        // rendezvous t-1.  Ring: after rendezvous t the DMA of tile t+3 overwrites tile t.
        constexpr int KS = CK / 32, NR = 2 * (MB + NB), NSTEP = 9 * KS;
        static_assert(NSET == 2 && LEAD == 1, "two register sets, reads one k-step ahead");
#define READ_STEP(set_, tap_, ks_) conv_read_step<NSET, MB, NB, ROWB, BS_BYTES, ALLTAPS, set_, tap_, ks_>(fa, fb, a_lane, wm * MB * CB_PW + l15, b_lane, g4)
        STAMP(3 + nti * 4)
        if (ALLTAPS || nti == 0) READ_STEP(0, 0, 0);                       // later N tiles: issued by the previous N tile's last step
        for (int q = 0; q < Q; ++q) {
            const bool last_chunk = (q + 1 >= Q);
            const bool more_segs = !last_chunk || has_next_nt;             // another (N tile, chunk) segment follows in the stream
            const int qn = last_chunk ? 0 : q + 1, ntn = last_chunk ? nt + 1 : nt;
            // one segment = the 9 taps of one (N tile, chunk); its first k-step always finds its operands in set 0
            {
                constexpr int P0 = 0;
                orn_sfor<0, 9>([&](auto tap_c) __attribute__((always_inline)) {
                    constexpr int tap = decltype(tap_c)::value;
                    constexpr int buf = ALLTAPS ? tap : tap % 3;
                    orn_sfor<0, KS>([&](auto ks_c) __attribute__((always_inline)) {
                        constexpr int ks = decltype(ks_c)::value;
                        constexpr int g = tap * KS + ks, cur = (g + P0) % NSET, nxt = (g + LEAD + P0) % NSET;
                        constexpr int g2 = g + LEAD;                       // the step whose reads are issued now
                        if constexpr (g2 < NSTEP) {
                            READ_STEP(nxt, g2 / KS, g2 % KS);
                            conv_wait_set<NSET, MB, NB, cur, LEAD * NR>(fa, fb);
                        } else
                            conv_wait_set<NSET, MB, NB, cur, (NSTEP - 1 - g) * NR>(fa, fb);
                        // the rendezvous that ends a tap goes IN FRONT of the tap's last MFMAs (their operands are in registers):
                        // the matrix pipe works through them while the waves wake up, issue the next DMA and run on
                        if constexpr (ks == KS - 1) {
                            if (!ALLTAPS && ((tap < 8) || more_segs)) {
                                STAMP_BAR(nti * Q + q, tap, 0)
                                WAIT_VM(0);         // this wave's pieces of every tile in flight (tile tt+2) have landed
                                STAMP_BAR(nti * Q + q, tap, 1)
                                if (!(PDBG(p) & 8)) BARRIER();
                                STAMP_BAR(nti * Q + q, tap, 2)
                            }
                        }
                        conv_mfma_step<NSET, MB, NB, cur>(fa, fb, acc);
                    });
                    STAMP_TAP(nti * Q + q, tap)
                    if (!ALLTAPS && ((tap < 8) || more_segs)) {
                        if constexpr (tap == 8) {
                            if (MULTI_CHUNK && Q > 1) {   // next chunk: everyone is done with the old chunk's patch
                                if (!(PDBG(p) & 2)) DMA_PATCH(qn)
                                WAIT_VM(0);
                                BARRIER();
                            }
                        }
                        if (!(PDBG(p) & 1)) {       // tile tt + 3 into the buffer of tile tt (free now)
                            if constexpr (tap < 6) DMA_B(buf, nt, q, tap + 3)
                            else if (more_segs) DMA_B(buf, ntn, qn, tap - 6)
                        }
                        if constexpr (tap == 8) {
                            if (MULTI_CHUNK && Q > 1) READ_STEP(0, 0, 0);  // fresh pipeline on the new patch: set 0
                        }
                    }
                });
            }
        }
#undef READ_STEP
        STAMP(4 + nti * 4)

        // ---- epilogue --------------------------------------------------------------------------
        // Lane (l15, g4) holds, of every 16 x 16 tile, channels 4 * g4 + r (r = 0..3) of pixel l15.  v_permlane16_swap on the
        // tiles (2j, 2j+1) of one 32-channel block gives every lane 8 CONSECUTIVE channels of its pixel: 16-byte stores, and
        // the four lanes of a pixel cover 64 contiguous bytes.  Rows g4 = 0..3 end up with channels +0, +16, +8, +24 of the block.
        const int c8_lane = 16 * (g4 & 1) + 8 * (g4 >> 1);
#pragma unroll
        for (int pi = 0; pi < 2 * MB; ++pi) {
            const int gh = h0 + wm * MB + (pi >> 1), gw = w0 + 16 * (pi & 1) + l15;
            const bool ok = (gh < H) && (gw < W) && !(PDBG(p) & 4);
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                const int cb = nt * BN + (wn * NB + j) * 32;            // first output channel of the 32-channel block
                const int c8 = cb + c8_lane;                            // the 8 channels this lane stores
                const f32x4 ta = acc[pi][2 * j], tb = acc[pi][2 * j + 1];
                {
                    float v[8];
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float x0 = ta[e], x1 = tb[e];
                        swap_rows_f(x0, x1);
                        v[e] = x0; v[4 + e] = x1;
                    }
                    if (EPI == EPI_B_DGRAD) {
                        if (ok) {
                            const h16x8 zz = *reinterpret_cast<const h16x8 *>(p.zprev + ((size_t)gh * W + gw) * p.Nout + c8);
                            h16x8 o8;
#pragma unroll
                            for (int e = 0; e < 8; ++e) o8[e] = (h16)(v[e] * orn_silu_grad((float)zz[e]));
                            const int sp = p.sp, ph = conv_div(gh, p.mSp), pw = conv_div(gw, p.mSp);
                            const int sub = (gh - ph * sp) * sp + (gw - pw * sp);
                            *reinterpret_cast<h16x8 *>(p.dyprev + ((size_t)(ph + 1) * (W / sp + 2) + (pw + 1)) * (p.Nout * sp * sp) +
                                                       sub * p.Nout + c8) = o8;
                        }
                    } else if (ok) {
                        float *dst = p.dx_f32 + (size_t)q_base * H * W * p.Nout + ((size_t)gh * W + gw) * p.Nout + c8;
                        *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                        *reinterpret_cast<float4 *>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
                    }
                }
            }
        }
        STAMP(5 + nti * 4)
    }
    STAMP(2 + nt_cnt * 4)
    STAMP_RT(1)
    STAMP_FLUSH()
}

#undef DMA16
#undef DMA_B
#undef DMA_PATCH
#undef WAIT_VM
#undef BARRIER

template <int WAVES_M, int WAVES_N, int MB, int NB, int EPI, int CK = CB_CK, bool ALLTAPS = (CK != CB_CK)>
static int launch_conv_cfg(const ConvBP &p, int n_tiles_total, hipStream_t st)
{
    constexpr int BN = WAVES_N * NB * 32;
    constexpr int NT = WAVES_M * WAVES_N * 64;
    constexpr size_t LDS_IMG = (size_t)(CB_PH * CB_PW * CK * 2 + 1023) / 1024 * 1024 + (ALLTAPS ? 9 : 3) * (size_t)BN * CK * 2;
    size_t smem = LDS_IMG;
#ifdef ORN_CONV_STAMP
    smem += 1024;
#endif
    auto kern = k_conv_nhwc_bf16<WAVES_M, WAVES_N, MB, NB, EPI, CK, ALLTAPS>;
    static bool attr_done = false;
    if (!attr_done) {
        // opt in once for the largest request (bias copy up to 2048 channels)
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(LDS_IMG + 8192));
        if (e != hipSuccess) { orn_set_error("conv_bf16: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
        attr_done = true;
    }
    const int ptiles = p.tiles_w * p.tiles_h;
    ConvBP q = p;
    dim3 grid(ptiles, n_tiles_total / p.n_tiles_per_wg);
    if (p.qsplit) grid.y = p.Cin / CB_CK;
    q.n_full = ptiles;
    if (p.n_tiles_per_wg > 1 && p.n_tiles_per_wg == n_tiles_total && ptiles > 256) {
        // 256 CUs, one work-group each: whole rounds keep full tiles, the last partial round is cut up
        q.n_full = ptiles / 256 * 256;
        grid = dim3(q.n_full + (ptiles - q.n_full) * p.n_tiles_per_wg, 1);
    }
    hipLaunchKernelGGL(kern, grid, dim3(NT), smem, st, q);
    ORN_LAUNCH_CHECK("conv_nhwc_bf16");
    return 0;
}

void set_debug_fwd(int flags);
void set_debug(int flags) { g_conv_dbg = flags; set_debug_fwd(flags); }

// m with x / d == umulhi(x, m) for every 0 <= x < 2^16 and 2 <= d < 2^16 (m = ceil(2^32 / d): the error term
// x * (m*d - 2^32) < 2^16 * 2^16); d == 1 is encoded as m = 0 (conv_div returns x)
static unsigned conv_magic(int d)
{
    return d <= 1 ? 0u : (unsigned)(((1ull << 32) + (unsigned long long)d - 1) / (unsigned long long)d);
}

// dgrad: N = 96 in one tile (waves 8x1, wave tile 32 px x 96 ch).  The forward launcher lives with its kernel in
// orn_conv_fwd_bf16.hip (the other MFMA shape).
int orn_launch_dgrad2(const h16 *dypad, const h16 *wd, int H, int W, int O, const h16 *zprev, h16 *dyprev, int sp, hipStream_t st);   // orn_conv2_bf16.hip
static int wgrad_fill(WgradBP &p, const h16 *xpad, const h16 *dypad, int H, int W, int C, int O, int s, float *slabs, int smax = 0);
int orn_launch_conv_bf16_fwd(const h16 *xpad, const h16 *wb, const float *bias_p, int H, int W, int Cin, int O, int s,
                             h16 *z, h16 *apad, hipStream_t st, int c_real, OrnHeadFuse *head = nullptr);
void set_debug_fwd(int flags);
#ifdef ORN_CONV_STAMP
void set_stamps_fwd(void *buf);
#endif

// dx_f32 must hold orn_dgrad_f32_slabs(H, W, O) partial slabs of H*W*C floats; the NCHW convert sums them.
int orn_dgrad_f32_slabs(int H, int W, int O)
{
    return (orn_cdiv(W, CB_TW) * orn_cdiv(H, CB_TH) < 128 && O / CB_CK > 1) ? O / CB_CK : 1;
}

// Small images (too few pixel tiles to fill the chip): the dgrad runs split over the input chunks into fp32 partial
// slabs [Q][H][W][96]; this pass sums them (fixed order), applies SiLU'(z_prev) and scatters into the previous layer's
// dypad -- what the EPI_B_DGRAD epilogue does in one go on large images.
__global__ void __launch_bounds__(256) k_dgrad_finish(const float *__restrict__ slabs, int Q, const h16 *__restrict__ zprev, int H, int W,
                                                     int sp, h16 *__restrict__ dyprev)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;       // (pixel, 8-channel group)
    const size_t n = (size_t)H * W * 12;
    if (idx >= n) return;
    const size_t pix = idx / 12;
    const int c8 = (int)(idx - pix * 12) * 8;
    const int gh = (int)(pix / W), gw = (int)(pix - (size_t)gh * W);
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int q = 0; q < Q; ++q) {
        const float *src = slabs + ((size_t)q * H * W + pix) * 96 + c8;
        const float4 a = *reinterpret_cast<const float4 *>(src), b = *reinterpret_cast<const float4 *>(src + 4);
        v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
    }
    const h16x8 zz = *reinterpret_cast<const h16x8 *>(zprev + pix * 96 + c8);
    h16x8 o8;
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = (h16)(v[e] * orn_silu_grad((float)zz[e]));
    const int ph = gh / sp, pw = gw / sp, sub = (gh - ph * sp) * sp + (gw - pw * sp);
    *reinterpret_cast<h16x8 *>(dyprev + ((size_t)(ph + 1) * (W / sp + 2) + (pw + 1)) * (96 * sp * sp) + sub * 96 + c8) = o8;
}

// dx_f32 alone: fp32 output slabs (layer below is fp32).  zprev/dyprev alone: fused epilogue.  Both: dx_f32 is scratch for
// orn_dgrad_f32_slabs(H, W, O) partial slabs and the result is finished into dyprev (small images).
// c_real (fp32-output form only): output channels that are not zero padding; <= 32 of them on a chunk-split launch take the
// all-taps-resident N = 32 form and only channels [0, 32) of the slabs are written
int orn_launch_conv_bf16_dgrad(const h16 *dypad, const h16 *wd, int H, int W, int O, int C, const h16 *zprev,
                               h16 *dyprev, int sp, float *dx_f32, hipStream_t st, int c_real);
int orn_launch_conv_bf16_dgrad(const h16 *dypad, const h16 *wd, int H, int W, int O, int C, const h16 *zprev,
                               h16 *dyprev, int sp, float *dx_f32, hipStream_t st, int c_real)
{
    ORN_REQUIRE(O % CB_CK == 0 && C == 96, "conv_bf16_dgrad: unsupported O=%d C=%d", O, C);
    ConvBP p = {};
    p.dbg = g_conv_dbg;
#ifdef ORN_CONV_STAMP
    p.stamps = g_conv_stamps;
#endif
    p.xpad = dypad; p.w = wd; p.bias = nullptr; p.H = H; p.W = W; p.Cin = O; p.Nout = C;
    p.tiles_w = orn_cdiv(W, CB_TW); p.tiles_h = orn_cdiv(H, CB_TH);
    p.n_tiles_per_wg = 1;
    p.zprev = zprev; p.dyprev = dyprev; p.sp = sp; p.dx_f32 = dx_f32;
    ORN_REQUIRE(H < 65536 && W < 65536 && sp >= 1 && sp < 65536, "conv_bf16_dgrad: sizes exceed the epilogue's index math");
    p.mSp = conv_magic(sp);
    if (dx_f32) {
        p.qsplit = (p.tiles_w * p.tiles_h < 128 && O / CB_CK > 1) ? 1 : 0;   // few pixel tiles: one work-group per input chunk
        if (!zprev && p.qsplit && c_real > 0 && c_real <= 32) return launch_conv_cfg<8, 1, 1, 1, EPI_B_DGRAD_F32, CB_CK, true>(p, 1, st);
        if (!zprev) return launch_conv_cfg<8, 1, 1, 3, EPI_B_DGRAD_F32>(p, 1, st);
        ORN_REQUIRE(dyprev && sp >= 1 && H % sp == 0 && W % sp == 0 && p.qsplit, "conv_bf16_dgrad: bad split-epilogue arguments");
        p.zprev = nullptr; p.dyprev = nullptr;
        ORN_TRY((launch_conv_cfg<8, 1, 1, 3, EPI_B_DGRAD_F32>(p, 1, st)));
        hipLaunchKernelGGL(k_dgrad_finish, dim3(orn_cdiv((long)H * W * 12, 256)), dim3(256), 0, st, dx_f32, O / CB_CK, zprev, H, W, sp, dyprev);
        ORN_LAUNCH_CHECK("dgrad_finish");
        return 0;
    }
    ORN_REQUIRE(zprev && dyprev && sp >= 1 && H % sp == 0 && W % sp == 0, "conv_bf16_dgrad: bad epilogue arguments");
    static const bool form1 = orn_probe_env("ORN_DGRAD_FORM1") != nullptr;       // tools/probes: A/B against the one-work-group-per-CU form
    if (form1) return launch_conv_cfg<8, 1, 1, 3, EPI_B_DGRAD>(p, 1, st);
    // (Round 3 also built the block's own wgrad riding behind these dgrad tiles in one launch: the two combined launches took 17 us
    // less than the launches they replaced, the STEP 13 us more -- DESIGN 4.5; removed in round 4.)
    return orn_launch_dgrad2(dypad, wd, H, W, O, zprev, dyprev, sp, st);       // two work-groups per CU: orn_conv2_bf16.hip
}

// ================================================================================================
// wgrad: dW[tap][o'][c] = sum_p dy[p][o'] * x[p + off(tap)][c]
// ================================================================================================
__global__ void __launch_bounds__(256, 2) k_wgrad_nhwc_bf16(WgradBP p) { wgrad_body(p, blockIdx.x); }

// Several layers in one launch (problems in the order given, each on a multiple-of-8 block range so the XCD decode holds):
// the small layers' wgrads do not fill the chip one at a time (72 / 216 / 360 work-groups for 512 slots at 720p), and
// nothing but the deferred reduction consumes them.
// dw/db = gscale * sum over blocks of the head backward's per-block partials [blocks][3C+3]: one work-group per column, lane
// t sums rows t, t+256, .. in ascending order, fixed-order block tree after (deterministic).
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

// The head's dW/db reduction (needed by Adam only) rides along as trailing work-groups: one graph node less.
struct WgradBPAll { int n; int start[ORN_MAX_LAYERS + 1]; WgradBP p[ORN_MAX_LAYERS]; OrnHeadFinish hf; int hf_blocks; OrnStemL2Job l2; int side; };
__global__ void __launch_bounds__(256, 2) k_wgrad_nhwc_bf16_all(WgradBPAll a)
{
    if (!a.side) ORN_PRIO_HIGH();         // (the side branch's launch keeps the default priority: orn_common.h)
    if ((int)blockIdx.x >= a.start[a.n] + a.hf_blocks) {        // stem backward, second linear layer: 16 output rows per work-group
        extern __shared__ __attribute__((aligned(16))) unsigned char smem_l2[];
        orn_stem_l2_block(a.l2, (int)blockIdx.x - a.start[a.n] - a.hf_blocks, (int)threadIdx.x, reinterpret_cast<float *>(smem_l2));
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
__global__ void k_wgrad_bf16_reduce_all(WgradReduceAll a)
{
    if ((int)blockIdx.y == a.n) {
        __shared__ float sh_w0[4];
        if (2 * (int)blockIdx.x >= a.w0.N) return;
        const int half = threadIdx.x >> 7;
        orn_stem_w0_row(a.w0, (int)blockIdx.x * 2 + half, threadIdx.x & 127, sh_w0 + 2 * half);
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
    static const int s_env = orn_probe_env_int("ORN_WGRAD_SMAX", 0);      // tools/probes: split-K sweep
    if (s_env > 0 && S > s_env) S = s_env;
    // measured in the 720p step: a full wave of work-groups (56 slabs) makes the slab write + re-read cost more than the idle
    // slots do -- L3 (900 K tiles): 40 slabs beat 56 by 17 us; L4 (3600 K tiles), since the DMA prefetch of the K loop works:
    // 32 / 40 / 48 / 56 slabs = 1.148 / 1.128 / 1.133 / 1.143 ms per step (reduction 30 / 35 / 38 / 45 us, wgrad 224 / 199 / 199 / 201)
    if (S > 40) S = 40;
    // layers under 2000 K tiles (720p L3: 900): 24 slabs -- the wgrad launch does not notice (all layers share it), the reduction
    // reads less: 40 / 32 / 24 = 35 / 32 / 30 us
    static const int s_small = orn_probe_env_int("ORN_WGRAD_SMAX_SMALL", 24);   // tools/probes override
    if (n_ktiles < 2000 && S > s_small && smax < 8) S = s_small;     // (a caller's count replaces this rule)
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

// dwf [O][C][3][3] and dbf [O] (PyTorch channel order), both overwritten.  C <= 96 real channels; xpad always has 96
// channels per pixel (zeros above C).
static int wgrad_fill(WgradBP &p, const h16 *xpad, const h16 *dypad, int H, int W, int C, int O, int s, float *slabs, int smax)
{
    // O % 32: a ragged last 128-channel tile reads up to 96 channels past a pixel's O; behind the last interior pixel (H, W) they
    // fall on dypad's border ring, so this kernel stays inside [H+2][W+2][O].  The 128 elements of slack orn.h asks for behind
    // dypad (the engine and the per-op hooks allocate them) serve the dgrad's reads; tests/test_gpu_conv16_forms.py fills them
    // with NaN.
    ORN_REQUIRE(C >= 1 && C <= 96 && O % 32 == 0 && O % (s * s) == 0, "wgrad_bf16: unsupported C=%d O=%d", C, O);
    p.dbg = g_conv_dbg;
    p.xpad = xpad; p.dypad = dypad; p.slabs = slabs; p.H = H; p.W = W; p.O = O;
    p.tiles_w = orn_cdiv(W, WB_TW);
    p.n_ktiles = p.tiles_w * orn_cdiv(H, WB_TH);
    p.S = orn_wgrad_bf16_split(H, W, O, smax);
    p.bias_slabs = slabs + (size_t)p.S * 9 * O * 96;
    p.n_otiles = orn_cdiv(O, WB_BO);
    static bool attr_done = false;
    if (!attr_done) {
        const size_t smem = WB_LDS_BYTES;
        hipError_t e = hipFuncSetAttribute((const void *)k_wgrad_nhwc_bf16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_wgrad_nhwc_bf16_all, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
        if (e != hipSuccess) { orn_set_error("wgrad_bf16: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
        attr_done = true;
    }
    return 0;
}

// slabs only (no reduction), several layers in one launch
int orn_launch_wgrad_bf16_batch(int n, const OrnWgradJob *J, hipStream_t st, const OrnHeadFinish *hf, const OrnStemL2Job *l2, int side)
{
    if (n == 0 && !hf && !l2) return 0;
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
    a.hf = OrnHeadFinish{};
    a.hf_blocks = 0;
    if (hf) { a.hf = *hf; a.hf_blocks = 3 * hf->C + 3; total += a.hf_blocks; }
    a.l2 = OrnStemL2Job{};
    if (l2) { a.l2 = *l2; total += orn_cdiv(l2->N, ORN_STEM_ROWS); }
    hipLaunchKernelGGL(k_wgrad_nhwc_bf16_all, dim3(total), dim3(256), WB_LDS_BYTES, st, a);
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

int orn_launch_wgrad_reduce_all(int n, const OrnWgradReduce *L, hipStream_t st, const OrnStemW0Job *w0)
{
    if (n == 0 && !w0) return 0;
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
    hipLaunchKernelGGL(k_wgrad_bf16_reduce_all, dim3(orn_cdiv((long)mx, 256), n + (w0 ? 1 : 0)), dim3(256), 0, st, a);
    ORN_LAUNCH_CHECK("wgrad_bf16_reduce_all");
    return 0;
}

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

// dbias: partial[blk][o'] = sum over the block's pixel rows of dypad interior; then reduced + un-permuted
#define DB_MAXO 1536
__global__ void __launch_bounds__(256) k_dbias_nhwc_partial(const h16 *__restrict__ dypad, int H, int W, int O, int rows_per_blk,
                                                            float *__restrict__ partial)
{
    __shared__ float red[DB_MAXO];
    const int o8 = O / 8;                       // 16-byte groups per pixel
    const int nw = 256 / o8;                    // pixel lanes
    const int grp = threadIdx.x % o8, lw = threadIdx.x / o8;
    const int h_begin = blockIdx.x * rows_per_blk, h_end = min(H, h_begin + rows_per_blk);
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (lw < nw)
        for (int h = h_begin; h < h_end; ++h) {
            const h16 *row = dypad + ((size_t)(h + 1) * (W + 2) + 1) * O + grp * 8;
            for (int w = lw; w < W; w += nw) {
                const h16x8 v = *reinterpret_cast<const h16x8 *>(row + (size_t)w * O);
#pragma unroll
                for (int k = 0; k < 8; ++k) s[k] += (float)v[k];
            }
        }
    for (int i = threadIdx.x; i < O; i += 256) red[i] = 0.f;
    __syncthreads();
    for (int r = 0; r < nw; ++r) {              // fixed order: deterministic
        if (lw == r)
#pragma unroll
            for (int k = 0; k < 8; ++k) red[grp * 8 + k] += s[k];
        __syncthreads();
    }
    for (int i = threadIdx.x; i < O; i += 256) partial[(size_t)blockIdx.x * O + i] = red[i];
}

__global__ void k_dbias_finish(const float *__restrict__ partial, int nblk, int O, int Cn, int s2, float gscale,
                               float *__restrict__ dbf)
{
    const int op = blockIdx.x * blockDim.x + threadIdx.x;
    if (op >= O) return;
    float acc = 0.f;
    for (int b = 0; b < nblk; ++b) acc += partial[(size_t)b * O + op];
    const int ij = op / Cn, nn = op - ij * Cn;
    dbf[nn * s2 + ij] = acc * gscale;
}

size_t orn_dbias_bf16_ws_floats(int H, int O) { return (size_t)orn_cdiv(H, 2) * O; }

int orn_launch_dbias_bf16(const h16 *dypad, int H, int W, int O, int s, float gscale, float *partial, float *dbf, hipStream_t st)
{
    ORN_REQUIRE(O % 8 == 0 && O / 8 <= 256 && O <= DB_MAXO, "dbias_bf16: unsupported O=%d", O);
    const int rows_per_blk = 2, nblk = orn_cdiv(H, rows_per_blk);
    hipLaunchKernelGGL(k_dbias_nhwc_partial, dim3(nblk), dim3(256), 0, st, dypad, H, W, O, rows_per_blk, partial);
    ORN_LAUNCH_CHECK("dbias_partial");
    hipLaunchKernelGGL(k_dbias_finish, dim3(orn_cdiv(O, 128)), dim3(128), 0, st, partial, nblk, O, O / (s * s), s * s, gscale, dbf);
    ORN_LAUNCH_CHECK("dbias_finish");
    return 0;
}

// ================================================================================================
// A5 head on the channels-last bf16 pre-activation of the last block (model.py:621-622):
//   a = SiLU(z);  u = W a + b;  out = (tanh u + 1)/2 | sigmoid u           out: fp32 NCHW [3][H][W]
// 4 lanes per pixel (C/4 channels each, 16-byte loads), 16 pixels per wave: fully coalesced.
// ================================================================================================
#define HB_MAXC 256

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
        auto proc = [&](const h16x8 v, int c0) {
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = orn_silu((float)v[e]);
                a0 = fmaf(sw[c0 + e], a, a0);
                a1 = fmaf(sw[C + c0 + e], a, a1);
                a2 = fmaf(sw[2 * C + c0 + e], a, a2);
            }
        };
        if (piped) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (q < nq) proc(vc[q], (q * 4 + sub) * 8);
        } else {
            for (int q = 0; q < nq; ++q) proc(*reinterpret_cast<const h16x8 *>(z + pix * C + (q * 4 + sub) * 8), (q * 4 + sub) * 8);
        }
        a0 += __shfl_xor(a0, 1, 64); a1 += __shfl_xor(a1, 1, 64); a2 += __shfl_xor(a2, 1, 64);
        a0 += __shfl_xor(a0, 2, 64); a1 += __shfl_xor(a1, 2, 64); a2 += __shfl_xor(a2, 2, 64);
        if (sub < 3) {
            const float u = (sub == 0 ? a0 : (sub == 1 ? a1 : a2)) + sw[3 * C + sub];
            out[(size_t)sub * HW + pix] = sigmoid ? 1.0f / (1.0f + __expf(-u)) : (tanhf(u) + 1.0f) * 0.5f;
        }
    }
}

// Backward: du = dout * act'(out); dz = (W^T du) * SiLU'(z) -> previous-layer dypad layout (bf16);
// dW[k][c] += du[k]*SiLU(z[c]); db[k] += du[k].  partial[blk][3*C+3], reduced afterwards.
template <int NQ>
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
                const float sg = orn_sigmoid(zz);
                const float a = zz * sg;
                const float da = fmaf(sw[2 * C + c0 + e], du[2], fmaf(sw[C + c0 + e], du[1], sw[c0 + e] * du[0]));
                o8[e] = (h16)(da * (sg * (1.0f + zz * (1.0f - sg))));
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

__global__ void __launch_bounds__(256) k_head_bf16_finish(const float *__restrict__ partial, int blocks, int C, float gscale,
                                                          float *__restrict__ dw, float *__restrict__ db)
{
    __shared__ float sred[256];
    head_finish_body(partial, blocks, C, gscale, dw, db, blockIdx.x, sred);
}

#define HB_BLOCKS 512

int orn_launch_head_fwd_bf16(const h16 *z, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st)
{
    ORN_REQUIRE(C % 32 == 0 && C <= HB_MAXC, "head_bf16: unsupported C=%d", C);
    int blocks = orn_cdiv((long)HW, 64);
    if (blocks > 8192) blocks = 8192;           // measured: 8192 beats 2048 by ~7 us at 720p
    hipLaunchKernelGGL(k_head_fwd_nhwc_bf16, dim3(blocks), dim3(256), 0, st, z, w, b, C, HW, sigmoid, out);
    ORN_LAUNCH_CHECK("head_fwd_bf16");
    return 0;
}

size_t orn_head_bwd_bf16_ws_floats(int C) { return (size_t)(HB_BLOCKS + 1) * (3 * C + 3); }
int orn_head_bwd_bf16_blocks(int H, int W) { const int b = orn_cdiv((long)H * W, 64); return b > HB_BLOCKS ? HB_BLOCKS : b; }

// gs_up: gradient scale carried by dypad (1 for bf16, 2^20 for fp16); dw/db are un-scaled here
int orn_launch_head_bwd_bf16(const h16 *z, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid,
                             int sp, float gs_up, h16 *dypad, float *dw, float *db, float *ws, hipStream_t st, const OrnScaleState *sc = nullptr,
                             const OrnLossFinalJob *fin = nullptr)
{
    ORN_REQUIRE(C == 96 || C == 32 || C == 64 || C == 128, "head_bwd_bf16: unsupported C=%d", C);
    ORN_REQUIRE(H % sp == 0 && W % sp == 0, "head_bwd_bf16: H,W not divisible by stride");
    int blocks = orn_cdiv((long)H * W, 64);
    if (blocks > HB_BLOCKS) blocks = HB_BLOCKS;
    float *partial = ws, *red = ws + (size_t)HB_BLOCKS * (3 * C + 3);
    OrnLossFinalJob fj = {};
    if (fin) fj = *fin;
    const int nfin = (fin && fin->n_l1 > 0) ? 1 : 0;
    switch (C) {
    case 32: hipLaunchKernelGGL(k_head_bwd_nhwc_bf16<1>, dim3(blocks + nfin), dim3(256), 0, st, z, w, out, dout, H, W, sigmoid, sp, gs_up, dypad, partial, sc, fj, blocks); break;
    case 64: hipLaunchKernelGGL(k_head_bwd_nhwc_bf16<2>, dim3(blocks + nfin), dim3(256), 0, st, z, w, out, dout, H, W, sigmoid, sp, gs_up, dypad, partial, sc, fj, blocks); break;
    case 96: hipLaunchKernelGGL(k_head_bwd_nhwc_bf16<3>, dim3(blocks + nfin), dim3(256), 0, st, z, w, out, dout, H, W, sigmoid, sp, gs_up, dypad, partial, sc, fj, blocks); break;
    default: hipLaunchKernelGGL(k_head_bwd_nhwc_bf16<4>, dim3(blocks + nfin), dim3(256), 0, st, z, w, out, dout, H, W, sigmoid, sp, gs_up, dypad, partial, sc, fj, blocks); break;
    }
    ORN_LAUNCH_CHECK("head_bwd_bf16");
    if (!dw) return 0;                  // deferred: rides along orn_launch_wgrad_bf16_batch (OrnHeadFinish)
    const size_t n = 3 * (size_t)C + 3;
    (void)red;
    hipLaunchKernelGGL(k_head_bf16_finish, dim3((unsigned)n), dim3(256), 0, st, partial, blocks, C, 1.0f / gs_up, dw, db);
    ORN_LAUNCH_CHECK("head_bf16_finish");
    return 0;
}

// ---- type-erased operation table for the engine (one per compiled element type) -----------------------
static int a_conv_fwd(const void *xpad, const void *wb, const float *bias_p, int H, int W, int Cin, int O, int s, void *z, void *apad,
                      hipStream_t st, int c_real, OrnHeadFuse *head)
{ return orn_launch_conv_bf16_fwd((const h16 *)xpad, (const h16 *)wb, bias_p, H, W, Cin, O, s, (h16 *)z, (h16 *)apad, st, c_real, head); }
static int a_conv_dgrad(const void *dypad, const void *wd, int H, int W, int O, int C, const void *zprev, void *dyprev, int sp,
                        float *dx_f32, hipStream_t st, int c_real)
{ return orn_launch_conv_bf16_dgrad((const h16 *)dypad, (const h16 *)wd, H, W, O, C, (const h16 *)zprev, (h16 *)dyprev, sp, dx_f32, st, c_real); }
static int a_wgrad(const void *xpad, const void *dypad, int H, int W, int C, int O, int s, float gscale, float *slabs, float *dwf,
                   float *dbf, hipStream_t st)
{ return orn_launch_wgrad_bf16((const h16 *)xpad, (const h16 *)dypad, H, W, C, O, s, gscale, slabs, dwf, dbf, st); }
static int a_to_nhwc(const float *src, int C, int Cp, int H, int W, void *dst, hipStream_t st)
{ return orn_launch_nchw_to_nhwc_pad_bf16(src, C, Cp, H, W, (h16 *)dst, st); }
static int a_to_nchw_f32(const float *src, int C, int Cp, int H, int W, int nslab, float scale, float *dst, hipStream_t st, const OrnScaleState *sc)
{ return orn_launch_nhwc_to_nchw_f32(src, C, Cp, H, W, nslab, scale, dst, st, sc); }
static int a_head_fwd(const void *z, const float *w, const float *b, int C, size_t HW, int sigmoid, float *out, hipStream_t st)
{ return orn_launch_head_fwd_bf16((const h16 *)z, w, b, C, HW, sigmoid, out, st); }
static int a_head_bwd(const void *z, const float *w, const float *out, const float *dout, int C, int H, int W, int sigmoid, int sp,
                      float gs_up, void *dypad, float *dw, float *db, float *ws, hipStream_t st, const OrnScaleState *sc, const OrnLossFinalJob *fin)
{ return orn_launch_head_bwd_bf16((const h16 *)z, w, out, dout, C, H, W, sigmoid, sp, gs_up, (h16 *)dypad, dw, db, ws, st, sc, fin); }

const OrnHalfOps ops = {a_conv_fwd, a_conv_dgrad, orn_wgrad_bf16_ws_floats, a_wgrad, orn_launch_wgrad_bf16_batch, orn_launch_wgrad_reduce_all, orn_launch_prep_weights_bf16_all, a_to_nhwc,
                        a_to_nchw_f32, orn_dgrad_f32_slabs, a_head_fwd, orn_head_bwd_bf16_ws_floats, orn_head_bwd_bf16_blocks, a_head_bwd};

// ================================================================================================
// test / per-op hooks: the 16-bit block on PyTorch-layout fp32 tensors (conversions included).  Built in both element
// types: the bf16 build exports orn_*_bf16, the IEEE-half build the orn_*_f16 twins (same arguments, half buffers).
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
        (h16)(da[src] * orn_silu_grad((float)zq));
}

static inline size_t alh(size_t halfs) { return orn_align(halfs * 2) / 2; }

#ifdef ORN_FP16
extern "C" size_t orn_conv3x3_ps_silu_bf16_ws_bytes(int C, int O, int H, int W, int s);     // element size is the same: one definition
#else
extern "C" size_t orn_conv3x3_ps_silu_bf16_ws_bytes(int C, int O, int H, int W, int s)
{
    const size_t Hs = (size_t)H * s, Ws = (size_t)W * s, Cn = O / (s * s);
    size_t b = 0;
    b += alh((size_t)(H + 2) * (W + 2) * C) * 2;          // xpad
    b += 2 * alh((size_t)9 * O * C + 96 * C) * 2;         // wb, wd (+ the rows a ragged last N tile reads past the end)
    b += orn_align((size_t)O * 4);                        // bias'
    b += alh(Hs * Ws * Cn) * 2;                           // z bf16
    b += alh((Hs + 2) * (Ws + 2) * Cn) * 2;               // apad
    b += alh((size_t)(H + 2) * (W + 2) * O + 128) * 2;    // dypad (+ what a ragged last wgrad tile reads past the end)
    b += orn_align(orn_wgrad_bf16_ws_floats(H, W, O) * 4);
    b += orn_align(orn_dbias_bf16_ws_floats(H, O) * 4);
    b += orn_align((size_t)H * W * C * 4 * 8);            // dx fp32 NHWC (up to 8 chunk slabs)
    return b;
}
#endif

struct Bf16Ws {
    h16 *xpad, *wb, *wd, *zb, *apad, *dypad;
    float *biasp, *slabs, *dbp, *dxn;
};

static Bf16Ws carve_bf16(void *ws, int C, int O, int H, int W, int s)
{
    const size_t Hs = (size_t)H * s, Ws = (size_t)W * s, Cn = O / (s * s);
    unsigned char *p = (unsigned char *)ws;
    Bf16Ws r;
    r.xpad = (h16 *)p; p += alh((size_t)(H + 2) * (W + 2) * C) * 2;
    r.wb = (h16 *)p; p += alh((size_t)9 * O * C + 96 * C) * 2;
    r.wd = (h16 *)p; p += alh((size_t)9 * O * C + 96 * C) * 2;
    r.biasp = (float *)p; p += orn_align((size_t)O * 4);
    r.zb = (h16 *)p; p += alh(Hs * Ws * Cn) * 2;
    r.apad = (h16 *)p; p += alh((Hs + 2) * (Ws + 2) * Cn) * 2;
    r.dypad = (h16 *)p; p += alh((size_t)(H + 2) * (W + 2) * O + 128) * 2;
    r.slabs = (float *)p; p += orn_align(orn_wgrad_bf16_ws_floats(H, W, O) * 4);
    r.dbp = (float *)p; p += orn_align(orn_dbias_bf16_ws_floats(H, O) * 4);
    r.dxn = (float *)p;
    return r;
}

// Same contract as orn_conv3x3_ps_silu_fwd (B = 1) but computed on the bf16 MFMA path.
// `ws` must be zero-filled by the caller before the first use (the padded borders are never written).
extern "C" int HOOK(orn_conv3x3_ps_silu_fwd_bf16, orn_conv3x3_ps_silu_fwd_f16)(const float *x, const float *wf, const float *bf, int C, int O, int H, int W,
                                            int s, float *z, float *a, void *ws, size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(x && wf && bf && (z || a) && ws, "conv3x3_ps_silu_fwd_bf16: null pointer");   // a == NULL: the last block's form (z only)
    ORN_REQUIRE(C % CB_CK == 0 && O % 32 == 0 && O % (s * s) == 0, "conv3x3_ps_silu_fwd_bf16: unsupported C=%d O=%d s=%d", C, O, s);
    if (ws_bytes < orn_conv3x3_ps_silu_bf16_ws_bytes(C, O, H, W, s)) { orn_set_error("conv3x3_ps_silu_fwd_bf16: workspace too small"); return ORN_E_WS; }
    hipStream_t st = (hipStream_t)stream;
    const Bf16Ws b = carve_bf16(ws, C, O, H, W, s);
    const int Cn = O / (s * s), Hs = H * s, Ws = W * s;
    ORN_TRY(orn_launch_nchw_to_nhwc_pad_bf16(x, C, C, H, W, b.xpad, st));
    ORN_TRY(orn_launch_prep_weights_bf16(wf, bf, O, C, s, b.wb, b.wd, b.biasp, st));
    ORN_TRY(orn_launch_conv_bf16_fwd(b.xpad, b.wb, b.biasp, H, W, C, O, s, b.zb, a ? b.apad : nullptr, st, C));
    const long n = (long)Cn * Hs * Ws;
    if (z) hipLaunchKernelGGL(k_nhwc_bf16_to_nchw_f32, dim3(orn_cdiv(n, 256)), dim3(256), 0, st, b.zb, Cn, Hs, Ws, 0, z);
    if (a) hipLaunchKernelGGL(k_nhwc_bf16_to_nchw_f32, dim3(orn_cdiv(n, 256)), dim3(256), 0, st, b.apad, Cn, Hs, Ws, 1, a);
    ORN_LAUNCH_CHECK("nhwc_bf16_to_nchw_f32");
    return 0;
}

extern "C" int HOOK(orn_conv3x3_ps_silu_bwd_bf16, orn_conv3x3_ps_silu_bwd_f16)(const float *x, const float *wf, const float *z, const float *da, int C, int O,
                                            int H, int W, int s, float *dx, float *dwf, float *dbf, void *ws,
                                            size_t ws_bytes, void *stream)
{
    ORN_REQUIRE(x && wf && z && da && dwf && dbf && ws, "conv3x3_ps_silu_bwd_bf16: null pointer");
    ORN_REQUIRE(C == 96 && O % 96 == 0 && O % (s * s) == 0, "conv3x3_ps_silu_bwd_bf16: unsupported C=%d O=%d", C, O);
    if (ws_bytes < orn_conv3x3_ps_silu_bf16_ws_bytes(C, O, H, W, s)) { orn_set_error("conv3x3_ps_silu_bwd_bf16: workspace too small"); return ORN_E_WS; }
    hipStream_t st = (hipStream_t)stream;
    const Bf16Ws b = carve_bf16(ws, C, O, H, W, s);
    const int Cn = O / (s * s);
    ORN_TRY(orn_launch_nchw_to_nhwc_pad_bf16(x, C, C, H, W, b.xpad, st));
    ORN_TRY(orn_launch_prep_weights_bf16(wf, dbf /*scratch: overwritten below*/, O, C, s, b.wb, b.wd, b.biasp, st));
    const long n = (long)Cn * H * s * W * s;
    hipLaunchKernelGGL(k_make_dy_bf16, dim3(orn_cdiv(n, 256)), dim3(256), 0, st, z, da, Cn, H, W, s, b.zb, b.dypad);
    ORN_LAUNCH_CHECK("make_dy_bf16");
    ORN_TRY(orn_launch_wgrad_bf16(b.xpad, b.dypad, H, W, C, O, s, 1.0f, b.slabs, dwf, dbf, st));
    if (dx) {
        ORN_TRY(orn_launch_conv_bf16_dgrad(b.dypad, b.wd, H, W, O, C, nullptr, nullptr, 1, b.dxn, st, C));
        ORN_TRY(orn_launch_nhwc_to_nchw_f32(b.dxn, C, C, H, W, orn_dgrad_f32_slabs(H, W, O), 1.0f, dx, st));
    }
    return 0;
}

// Raw channels-last entry points (the engine's own layouts; used by bench.py's roofline leg).
extern "C" int HOOK(orn_conv_nhwc_bf16_fwd, orn_conv_nhwc_f16_fwd)(const void *xpad, const void *wb, const float *bias_p, int H, int W, int C, int O,
                                      int s, void *z, void *apad, void *stream)
{
    ORN_REQUIRE(xpad && wb && z, "conv_nhwc_bf16_fwd: null pointer");
    return orn_launch_conv_bf16_fwd((const h16 *)xpad, (const h16 *)wb, bias_p, H, W, C, O, s, (h16 *)z, (h16 *)apad,
                                    (hipStream_t)stream, C);
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
                                      nullptr, (hipStream_t)stream, C);
}

// Test entry points (include/orn_debug.h): the two conv launchers with the engine's full argument lists, so that a test reaches
// every kernel form they select (the narrow c_real forms, the split dgrad + finish, the fp32 hand-off) with the engine's buffers.
extern "C" int HOOK(orn_debug_conv_fwd_bf16, orn_debug_conv_fwd_f16)(const void *xpad, const void *wb, const float *bias_p, int H, int W,
                                                                   int Cin, int O, int s, void *z, void *apad, int c_real, void *stream)
{
    return orn_launch_conv_bf16_fwd((const h16 *)xpad, (const h16 *)wb, bias_p, H, W, Cin, O, s, (h16 *)z, (h16 *)apad,
                                    (hipStream_t)stream, c_real, nullptr);
}
extern "C" int HOOK(orn_debug_conv_dgrad_bf16, orn_debug_conv_dgrad_f16)(const void *dypad, const void *wd, int H, int W, int O, int C,
                                                                       const void *zprev, void *dyprev, int sp, float *dx_f32, int c_real,
                                                                       void *stream)
{
    return orn_launch_conv_bf16_dgrad((const h16 *)dypad, (const h16 *)wd, H, W, O, C, (const h16 *)zprev, (h16 *)dyprev, sp, dx_f32,
                                      (hipStream_t)stream, c_real);
}

#ifdef ORN_CONV_STAMP
void set_stamps_fwd(void *buf);
void set_stamps(void *buf) { g_conv_stamps = (unsigned long long *)buf; set_stamps_fwd(buf); }
#endif

}  // namespace HNS

#ifndef ORN_FP16
// probe-only switches (include/orn_debug.h) reach both builds
namespace orn_f16 { void set_debug(int flags); void set_stamps(void *buf); }
extern "C" void orn_debug_set(int flags) { orn_bf16::set_debug(flags); orn_f16::set_debug(flags); }
#ifdef ORN_CONV_STAMP
extern "C" void orn_debug_set_stamps(void *buf) { orn_bf16::set_stamps(buf); orn_f16::set_stamps(buf); }
#endif
#endif

const OrnHalfOps *
#ifdef ORN_FP16
orn_half_ops_f16()
#else
orn_half_ops_bf16()
#endif
{
    return &HNS::ops;
}
