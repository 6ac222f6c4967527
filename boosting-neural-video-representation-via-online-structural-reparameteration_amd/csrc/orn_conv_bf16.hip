// A4 fast path, DGRAD of the NeRVBlock conv (model.py:539,567), first form: one work-group per CU on v_mfma_f32_16x16x32
// (fp32 accumulate), for the layers that carry 99 % of the step's FLOPs (96 input channels of the forward conv).  Large images
// with a fused epilogue take the two-work-groups-per-CU family instead (orn_conv2_bf16.hip); this kernel serves the small
// images (chunk-split into fp32 slabs + k_dgrad_finish) and the hand-off to an fp32 layer below.
// Activations live in HBM as channels-last 16-bit with a one-pixel zero border:
//
//   xpad [H+2][W+2][C]      conv input  (= previous block's a = SiLU(z), border = conv zero padding)
//   z    [Hs][Ws][Cn]       pre-activation after PixelShuffle (kept for SiLU')
//   dypad[H+2][W+2][O']     gradient wrt the conv output, out-channel order o' = (i*s+j)*Cn + n so
//                           that PixelShuffle / unshuffle move whole Cn-channel rows
//   Wb   [9][O'][C]         merged kernel, 16-bit, tap-major, o' order      (forward B operand)
//   Wd   [9][C][O']         flipped taps, transposed                        (dgrad B operand)
//
// The dgrad is a conv of dypad with Wd: work-group = 8x32 output pixels x all 96 channels; the (8+2)x(32+2) input patch of a
// 96-channel chunk stays in LDS for all 9 taps -- each input byte is read 1.33x instead of 9x -- while [BN][96] weight tiles
// stream from L2 through a three-slot LDS ring.  The forward (orn_conv_fwd_bf16.hip) has the same machinery on the other MFMA
// shape; the wgrad is in orn_wgrad_bf16.hip; weight prep, layout converters, the head and the per-op C ABI in orn_ops_bf16.hip.
// Compiled twice (orn_h16.h): bf16 and, with -DORN_FP16, IEEE half.
#include "orn_h16.h"

namespace HNS {

static int g_conv_dbg = 0;   // timing experiments only (tools/probes), see orn_debug_set
#ifdef ORN_CONV_STAMP
static unsigned long long *g_conv_stamps = nullptr;
#define STAMP_LDS_OFF 0        // the stamps sit right behind the weight ring
#endif

struct ConvBP {
    const h16 *xpad;     // [H+2][W+2][Cin]: the padded gradient wrt the conv output (dypad)
    const h16 *w;        // [9][Nout][Cin]: Wd
    int H, W, Cin, Nout;
    int tiles_w, tiles_h;
    int qsplit;          // small images: blockIdx.y = input chunk, one fp32 partial slab per chunk
    float *dx_f32;       // [H][W][Nout] (x one slab per chunk when chunk-split)
    int dbg;             // timing-only ablation flags (tools/probes): 1 no weight restage, 2 no patch stage, 4 no stores
    unsigned long long *stamps;   // -DORN_CONV_STAMP diagnostic builds only: 64 time stamps per work-group (tools/probes/conv_stamps.py)
};

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
#pragma unroll
    for (int i = 0; i < 2 * MB; ++i)
#pragma unroll
        for (int j = 0; j < 2 * NB; ++j) acc[i][j] = MFMA16_H16(fb[SET][j], fa[SET][i], acc[i][j]);
}

// One work-group: 8 x 32 pixels of dx, all BN = WAVES_N * NB * 32 channels of it (the whole N in ONE tile: 96, or 32 for the
// all-taps form), walking the conv output's channels in chunks of CK = 96 and writing fp32 slabs (EPI_B_DGRAD_F32) -- always:
// the two parameters keep the kernel's name, which the benchmark's roofline table prints.
// ALLTAPS: all nine weight tiles of the (single) K chunk resident, one rendezvous -- the chunk-split dgrad of a layer with
// <= 32 real OUTPUT channels (N tile 32: 9 x 6 KB next to the 64 KB patch).
template <int WAVES_M, int WAVES_N, int MB, int NB, int EPI, int CK = CB_CK, bool ALLTAPS = (CK != CB_CK)>
__global__ void __launch_bounds__(WAVES_M *WAVES_N * 64) k_conv_nhwc_bf16(ConvBP p)
{
    ORN_PRIO_HIGH();
    static_assert(EPI == EPI_B_DGRAD_F32 && CK == CB_CK, "this file holds the dgrad kernels (forward: orn_conv_fwd_bf16.hip)");
    constexpr int NCH = CK / 8;                        // 16-byte chunks per LDS row
    constexpr int NBUF = ALLTAPS ? 9 : 3;              // weight tiles resident at once
    constexpr int NT = WAVES_M * WAVES_N * 64;
    constexpr int BN = WAVES_N * NB * 32;
    static_assert(WAVES_M * MB == CB_TH, "M tile must be 8 rows of 32 pixels");
    // LDS images: UNPADDED 192-byte rows (12 x 16-byte chunks) filled by LDS-DMA (global_load_lds_dwordx4: 1 KiB per
    // wave-instruction, lane-linear destination, no VGPRs, no ds_write).  Conflict-free ds_read_b128 comes from an
    // XOR swizzle -- logical chunk c of row R sits at position c ^ ((R >> 1) & 3) -- applied on the DMA's
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
    static_assert(PATCH_INSTR % NWAVES == 0 && BS_BYTES % 1024 == 0, "tile geometry");
    unsigned char *patch = smem;
    unsigned char *bs0 = smem + PATCH_LDS;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l31 = lane & 31, hh = lane >> 5;
    const int wm = wave / WAVES_N, wn = wave % WAVES_N;
    const int tile = blockIdx.x;                       // one work-group per pixel tile (x one per input chunk when chunk-split)
    const int tw = tile % p.tiles_w, th = tile / p.tiles_w;
    const int h0 = th * CB_TH, w0 = tw * CB_TW;
    const int H = p.H, W = p.W, Cin = p.Cin;
    const int q_base = p.qsplit ? (int)blockIdx.y : 0;   // chunk split: this WG's chunk
    // chunks of the input channels walked by one work-group (the all-taps-resident form is launched chunk-split: one)
    constexpr bool MULTI_CHUNK = !ALLTAPS;
    const int Q = (!MULTI_CHUNK || p.qsplit) ? 1 : Cin / CB_CK;
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
#define DMA_B(buf_, q_, tap_)                                                                                   \
    {                                                                                                           \
        if (NLOAD == NWAVES || uwave < NLOAD) {                                                                 \
            const h16 *wbase = p.w + ((size_t)((tap_) * p.Nout) * Cin + ((q_) + q_base) * CK);                \
            _Pragma("unroll") for (int k = 0; k < B_PER_WAVE; ++k)                                              \
                DMA16((const char *)wbase + b_goff[k], PATCH_LDS + (buf_) * BS_BYTES + ((uwave + NLOAD * k) % B_INSTR) * 1024); \
        }                                                                                                       \
    }
#define DMA_PATCH(q_)                                                                                           \
    {                                                                                                           \
        _Pragma("unroll") for (int k = 0; k < P_PER_WAVE; ++k)                                                  \
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
    constexpr int NSET = 2, LEAD = NSET - 1;            // fragment register sets: reads run LEAD k-steps ahead of their MFMAs
    h16x8 fa[NSET][2 * MB], fb[NSET][2 * NB];
    STAMP(2)
    // acc[pi][ci]: 16 x 16 tiles.  D rows = 16 output channels (A operand = weights), D cols = 16 pixels (B operand = input
    // patch): pixel sub-block pi = 2 * row + half, channel sub-block ci; lane (l15, g4) owns pixel l15 of the sub-block and the
    // 4 consecutive channels 4 * g4 + r of the 16.
    f32x4 acc[2 * MB][2 * NB];
#pragma unroll
    for (int i = 0; i < 2 * MB; ++i)
#pragma unroll
        for (int j = 0; j < 2 * NB; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // prologue: the patch (chunk 0) and weight tiles 0, 1 (all nine of the all-taps form); tile 2 stays in flight behind the
    // first rendezvous.
    BARRIER();
    if (!(PDBG(p) & 2)) DMA_PATCH(0)
    DMA_B(0, 0, 0)
    if (n_tiles > 1) DMA_B(1, 0, 1)
    if (ALLTAPS) {                                 // the whole K: taps 2..8 too, then the only rendezvous
#pragma unroll
        for (int tp = 2; tp < 9; ++tp) DMA_B(tp, 0, tp)
    }
    WAIT_VM(0);
    BARRIER();
    if (!ALLTAPS && n_tiles > 2) DMA_B(2, 0, 2)
    // One software pipeline over all k-steps (chunks of 96 input channels outside; nine taps x CK/32 k-slices inside,
    // unrolled at compile time so tap, kernel row / column, ring slot, register set and LDS offsets are constants): step s
    // issues the fragment reads of step s+LEAD into another register set, waits with a COUNTED lgkmcnt for its own
    // (issued LEAD steps earlier), then runs its MFMAs -- also across a tap boundary, so the rendezvous at the end of a tap
    // sits between MFMAs whose operands are already in registers or in flight.  (LEAD = 2 measured the same as 1 on the
    // 720p shapes.)  Reading tile t+1 before rendezvous t is legal because every wave waits for
    // ALL its outstanding DMA pieces (tile t+2 included) before rendezvous t: tile t+1 was complete, and known to be, at
    // rendezvous t-1.  Ring: after rendezvous t the DMA of tile t+3 overwrites tile t.
    constexpr int KS = CK / 32, NR = 2 * (MB + NB), NSTEP = 9 * KS;
    static_assert(NSET == 2 && LEAD == 1, "two register sets, reads one k-step ahead");
#define READ_STEP(set_, tap_, ks_) conv_read_step<NSET, MB, NB, ROWB, BS_BYTES, ALLTAPS, set_, tap_, ks_>(fa, fb, a_lane, wm * MB * CB_PW + l15, b_lane, g4)
    STAMP(3)
    READ_STEP(0, 0, 0);
    for (int q = 0; q < Q; ++q) {
        const bool last_chunk = (q + 1 >= Q);
        const bool more_segs = !last_chunk;                            // another chunk follows in the stream
        const int qn = last_chunk ? 0 : q + 1;
        // one segment = the 9 taps of one chunk; its first k-step always finds its operands in set 0
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
                            STAMP_BAR(q, tap, 0)
                            WAIT_VM(0);         // this wave's pieces of every tile in flight (tile tt+2) have landed
                            STAMP_BAR(q, tap, 1)
                            if (!(PDBG(p) & 8)) BARRIER();
                            STAMP_BAR(q, tap, 2)
                        }
                    }
                    conv_mfma_step<NSET, MB, NB, cur>(fa, fb, acc);
                });
                STAMP_TAP(q, tap)
                if (!ALLTAPS && ((tap < 8) || more_segs)) {
                    if constexpr (tap == 8) {
                        if (MULTI_CHUNK && Q > 1) {   // next chunk: everyone is done with the old chunk's patch
                            if (!(PDBG(p) & 2)) DMA_PATCH(qn)
                            WAIT_VM(0);
                            BARRIER();
                        }
                    }
                    if (!(PDBG(p) & 1)) {       // tile tt + 3 into the buffer of tile tt (free now)
                        if constexpr (tap < 6) DMA_B(buf, q, tap + 3)
                        else if (more_segs) DMA_B(buf, qn, tap - 6)
                    }
                    if constexpr (tap == 8) {
                        if (MULTI_CHUNK && Q > 1) READ_STEP(0, 0, 0);  // fresh pipeline on the new patch: set 0
                    }
                }
            });
        }
    }
#undef READ_STEP
    STAMP(4)

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
            const int cb = (wn * NB + j) * 32;                      // first output channel of the 32-channel block
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
                if (ok) {
                    float *dst = p.dx_f32 + (size_t)q_base * H * W * p.Nout + ((size_t)gh * W + gw) * p.Nout + c8;
                    *reinterpret_cast<float4 *>(dst) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4 *>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
                }
            }
        }
    }
    STAMP(5)
    STAMP(6)
    STAMP_RT(1)
    STAMP_FLUSH()
}

#undef DMA16
#undef DMA_B
#undef DMA_PATCH
#undef WAIT_VM
#undef BARRIER

template <int WAVES_M, int WAVES_N, int MB, int NB, int EPI, int CK = CB_CK, bool ALLTAPS = (CK != CB_CK)>
static int launch_conv_cfg(const ConvBP &p, hipStream_t st)
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
        // opt in once (the ceiling the forward's launcher asks for, with its bias copy: more than any request made here)
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(LDS_IMG + 8192));
        if (e != hipSuccess) { orn_set_error("conv_bf16: hipFuncSetAttribute: %s", hipGetErrorString(e)); return (int)e; }
        attr_done = true;
    }
    // one work-group per pixel tile; chunk-split: times one per 96-channel chunk of the conv output
    const dim3 grid(p.tiles_w * p.tiles_h, p.qsplit ? p.Cin / CB_CK : 1);
    hipLaunchKernelGGL(kern, grid, dim3(NT), smem, st, p);
    ORN_LAUNCH_CHECK("conv_nhwc_bf16");
    return 0;
}

void set_debug(int flags) { g_conv_dbg = flags; set_debug_fwd(flags); set_debug_wgrad(flags); }

// dx_f32 must hold orn_dgrad_f32_slabs(H, W, O) partial slabs of H*W*C floats; the NCHW convert sums them.
int orn_dgrad_f32_slabs(int H, int W, int O)
{
    return (orn_cdiv(W, CB_TW) * orn_cdiv(H, CB_TH) < 128 && O / CB_CK > 1) ? O / CB_CK : 1;
}

// Small images (too few pixel tiles to fill the chip): the dgrad runs split over the input chunks into fp32 partial
// slabs [Q][H][W][96]; this pass sums them (fixed order), applies SiLU'(z_prev) and scatters into the previous layer's
// dypad -- what the dgrad epilogue of orn_conv2_bf16.hip does in one go on large images.
template <int ACT>
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
    for (int e = 0; e < 8; ++e) o8[e] = (h16)(v[e] * OrnAct<ACT>::df((float)zz[e]));
    const int ph = gh / sp, pw = gw / sp, sub = (gh - ph * sp) * sp + (gw - pw * sp);
    *reinterpret_cast<h16x8 *>(dyprev + ((size_t)(ph + 1) * (W / sp + 2) + (pw + 1)) * (96 * sp * sp) + sub * 96 + c8) = o8;
}

// dx_f32 alone: fp32 output slabs (layer below is fp32).  zprev/dyprev alone: fused epilogue.  Both: dx_f32 is scratch for
// orn_dgrad_f32_slabs(H, W, O) partial slabs and the result is finished into dyprev (small images).
// c_real (fp32-output form only): output channels that are not zero padding; <= 32 of them on a chunk-split launch take the
// all-taps-resident N = 32 form and only channels [0, 32) of the slabs are written
int orn_launch_conv_bf16_dgrad(const h16 *dypad, const h16 *wd, int H, int W, int O, int C, const h16 *zprev,
                               h16 *dyprev, int sp, float *dx_f32, hipStream_t st, int c_real, int act)
{
    ORN_REQUIRE(orn_act_known(act), "conv_bf16_dgrad: unknown activation %d", act);
    ORN_REQUIRE(O % CB_CK == 0 && C == 96, "conv_bf16_dgrad: unsupported O=%d C=%d", O, C);
    ConvBP p = {};
    p.dbg = g_conv_dbg;
#ifdef ORN_CONV_STAMP
    p.stamps = g_conv_stamps;
#endif
    p.xpad = dypad; p.w = wd; p.H = H; p.W = W; p.Cin = O; p.Nout = C;
    p.tiles_w = orn_cdiv(W, CB_TW); p.tiles_h = orn_cdiv(H, CB_TH);
    p.dx_f32 = dx_f32;
    ORN_REQUIRE(H < 65536 && W < 65536 && sp >= 1 && sp < 65536, "conv_bf16_dgrad: sizes exceed the epilogue's index math");
    if (dx_f32) {
        p.qsplit = (p.tiles_w * p.tiles_h < 128 && O / CB_CK > 1) ? 1 : 0;   // few pixel tiles: one work-group per input chunk
        if (!zprev && p.qsplit && c_real > 0 && c_real <= 32) return launch_conv_cfg<8, 1, 1, 1, EPI_B_DGRAD_F32, CB_CK, true>(p, st);
        if (!zprev) return launch_conv_cfg<8, 1, 1, 3, EPI_B_DGRAD_F32>(p, st);
        ORN_REQUIRE(dyprev && sp >= 1 && H % sp == 0 && W % sp == 0 && p.qsplit, "conv_bf16_dgrad: bad split-epilogue arguments");
        ORN_TRY((launch_conv_cfg<8, 1, 1, 3, EPI_B_DGRAD_F32>(p, st)));
        ORN_ACT_SWITCH(act, A, hipLaunchKernelGGL(k_dgrad_finish<A>, dim3(orn_cdiv((long)H * W * 12, 256)), dim3(256), 0, st, dx_f32, O / CB_CK, zprev, H, W,
                                                  sp, dyprev));
        ORN_LAUNCH_CHECK("dgrad_finish");
        return 0;
    }
    ORN_REQUIRE(zprev && dyprev && sp >= 1 && H % sp == 0 && W % sp == 0, "conv_bf16_dgrad: bad epilogue arguments");
    // (Round 3 also built the block's own wgrad riding behind these dgrad tiles in one launch: the two combined launches took 17 us
    // less than the launches they replaced, the STEP 13 us more -- DESIGN 4.5; removed in round 4.)
    return orn_launch_dgrad2(dypad, wd, H, W, O, zprev, dyprev, sp, st, act);       // two work-groups per CU: orn_conv2_bf16.hip
}

#ifdef ORN_CONV_STAMP
void set_stamps(void *buf) { g_conv_stamps = (unsigned long long *)buf; set_stamps_fwd(buf); }
#endif

}  // namespace HNS
