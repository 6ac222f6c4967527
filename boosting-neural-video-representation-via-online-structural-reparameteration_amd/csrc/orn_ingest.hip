// K11  frame ingest: ToTensor + F.adaptive_avg_pool2d(data, (h, w))      main_train.py:200,239,420; main_eval.py:467,807
//
// The reference forms every target with adaptive_avg_pool2d(data, output.shape[-2:]) inside the step; frames never change during a
// fit, so here the pool runs once per video, from the uint8 pixels as PIL decodes them (orn_frames_ingest_u8) or from fp32 frames
// an API caller hands over (orn_frames_pool_f32).  Arithmetic of ATen's CPU kernel, bit for bit: output (i, j) sums its window
// rows [floor(i*H/h), ceil((i+1)*H/h)) x cols [floor(j*W/w), ceil((j+1)*W/w)) in fp32, row-major from 0, then divides by the
// window height and by the window width (two correctly rounded divisions).  A byte's value is (float)b / 255.0f from a 256-entry
// LDS table of exactly those quotients (ToTensor).
//
// Work distribution: one 256-thread work-group per tile of ING_TX x ING_TH output pixels of one frame, all three channels.  The
// tile's source rows are staged in LDS as they lie in memory -- interleaved bytes, or one line per channel plane for fp32 -- in
// passes of as many rows as fit ING_STAGE_BYTES, with 16-byte loads from 16-byte aligned global addresses (a line's first and last
// partial chunks go byte by byte: row starts of interleaved RGB are not aligned when 3*W % 4 != 0, and nothing outside the line is
// read).  Each thread owns one output column and ING_K output rows; its window loops run over the staged rows of each pass, so a
// window taller than a pass continues in the next one in the same order.  Stores are planar with consecutive lanes along w.
// No atomics, no scratch, nothing synchronises: capturable.
#include "orn_common.h"

#define ING_TX 128                       // output columns of a tile (lanes along w)
#define ING_TY 2                         // output rows of a tile in flight (256 threads = ING_TX * ING_TY)
#define ING_K 4                          // output rows per thread
#define ING_TH (ING_TY * ING_K)          // output rows of a tile
#define ING_STAGE_BYTES 32768            // LDS staging buffer of one pass, at most (a call takes what its tiles need)
#define ING_MAX_DIM 32768                // H, W, h, w: index products stay inside int32

struct OrnIngestGeom {
    int H, W, h, w;
    int tw;          // output columns a tile covers (ING_TX, fewer when the source span of ING_TX columns would not fit one pass)
    int pitch;       // bytes between staged lines (multiple of 16, >= 15 + the longest line)
    int rows_pass;   // source rows per staging pass
    int stage_bytes; // LDS of one pass: rows_pass rows (x 3 planes for fp32) of pitch bytes
};

// window [ing_lo, ing_hi) of output index i; i < n_out <= ING_MAX_DIM and n_in <= ING_MAX_DIM keep (i + 1) * n_in + n_out below 2^31
__device__ __forceinline__ int ing_lo(int i, int n_in, int n_out) { return (int)((unsigned)(i * n_in) / (unsigned)n_out); }
__device__ __forceinline__ int ing_hi(int i, int n_in, int n_out) { return (int)((unsigned)((i + 1) * n_in + n_out - 1) / (unsigned)n_out); }

// x / (float)k, correctly rounded.  For k = 2^m the quotient is x * 2^-m -- the same real number, so the one rounding gives the same
// float -- which spares the ten-instruction IEEE sequence at identity size and at every 2x2 window (1080p -> 720p).
__device__ __forceinline__ float ing_div(float x, int k)
{
    const float kf = (float)k;
    if ((k & (k - 1)) == 0) return x * __int_as_float(0x7F000000 - __float_as_int(kf));      // 2^-m from the exponent of 2^m
    return __fdiv_rn(x, kf);
}

// U8: src [n][H][W][3] bytes, a staged line = the tile's columns of one source row (3 bytes per pixel);
// else src [n][3][H][W] fp32, three staged lines per source row, one per channel plane.
template <bool U8>
__global__ void __launch_bounds__(256) k_frames_ingest(const unsigned char *__restrict__ src, float *__restrict__ dst, OrnIngestGeom g)
{
    constexpr int E = U8 ? 3 : 4, LPR = U8 ? 1 : 3;
    // all LDS is dynamic, sized by the call (ingest_geom): a small tile footprint lets up to eight work-groups share a CU, and the
    // loads of one overlap the sums and stores of the others
    extern __shared__ __align__(16) unsigned char ing_lds[];
    unsigned char *stage = ing_lds;                                        // rows_pass staged rows
    float *tab = reinterpret_cast<float *>(ing_lds + g.stage_bytes);       // 256 floats (uint8 entry)
    const int t = threadIdx.x, tx = t % ING_TX;
    const int ty = __builtin_amdgcn_readfirstlane(t / ING_TX);            // a wave lies in one row of the tile: row windows are scalar
    const int H = g.H, W = g.W, h = g.h, w = g.w, pitch = g.pitch;
    if (U8) tab[t] = __fdiv_rn((float)t, 255.0f);          // ToTensor's quotients; read after the first staging barrier
    const size_t n = blockIdx.z;
    const int j0 = blockIdx.x * g.tw, j1 = min(j0 + g.tw, w);
    const int i0 = blockIdx.y * ING_TH, i1 = min(i0 + ING_TH, h);
    const int cs0 = ing_lo(j0, W, w), cs1 = ing_hi(j1 - 1, W, w);
    const int rs0 = ing_lo(i0, H, h), rs1 = ing_hi(i1 - 1, H, h);
    const int len = (cs1 - cs0) * E;                       // bytes of one staged line
    // global address of the first staged byte of source row 0 (channel plane ch for fp32); a row further down lies row_bytes on
    const size_t row_bytes = (size_t)W * E, plane_bytes = (size_t)H * row_bytes;
    const uintptr_t base = (uintptr_t)src + n * (U8 ? plane_bytes : 3 * plane_bytes) + (size_t)cs0 * E;
    // ... and its phase inside a 16-byte chunk, from the low address bits alone
    auto phase = [&](int r, int ch) -> unsigned {
        return ((unsigned)base + (U8 ? 0u : (unsigned)ch * (unsigned)plane_bytes) + (unsigned)r * (unsigned)row_bytes) & 15u;
    };

    const int j = j0 + tx;
    const bool col_ok = tx < g.tw && j < w;
    const int c0 = col_ok ? ing_lo(j, W, w) : 0, c1 = col_ok ? ing_hi(j, W, w) : 0;      // no column: an empty window
    int r0[ING_K], r1[ING_K];
    float acc[ING_K][3];
#pragma unroll
    for (int k = 0; k < ING_K; ++k) {
        const int i = i0 + k * ING_TY + ty;
        r0[k] = i < h ? ing_lo(i, H, h) : 0;               // no row: an empty window
        r1[k] = i < h ? ing_hi(i, H, h) : 0;
        acc[k][0] = acc[k][1] = acc[k][2] = 0.f;
    }

    const int nch = pitch >> 4;                            // 16-byte chunks of a staged line
    const int dl = 256 / nch, dc = 256 - dl * nch;         // a thread's next chunk: 256 further on in (line, chunk) order
    const int l_first = t / nch, c_first = t - l_first * nch;
    for (int p = rs0; p < rs1; p += g.rows_pass) {
        const int nrows = min(g.rows_pass, rs1 - p);
        __syncthreads();                                   // the previous pass has been read
        for (int l = l_first, c16 = c_first; l < nrows * LPR;) {
            const int r = p + l / LPR, ch = l % LPR;
            const uintptr_t ga = base + (U8 ? 0 : ch * plane_bytes) + r * row_bytes, gb = ga + len;
            const uintptr_t a = (ga & ~(uintptr_t)15) + 16 * (uintptr_t)c16;    // the line keeps its phase inside a 16-byte chunk
            unsigned char *ld = stage + l * pitch + 16 * c16;
            if (a >= ga && a + 16 <= gb) {
                *reinterpret_cast<uint4 *>(ld) = *reinterpret_cast<const uint4 *>(a);
            } else {
                for (int b = 0; b < 16; ++b)
                    if (a + b >= ga && a + b < gb) ld[b] = *reinterpret_cast<const unsigned char *>(a + b);
            }
            l += dl;
            c16 += dc;
            if (c16 >= nch) { c16 -= nch; ++l; }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < ING_K; ++k) {
            const int ra = max(r0[k], p), rb = min(r1[k], p + nrows);
            for (int r = ra; r < rb; ++r) {
                if (U8) {
                    const unsigned char *b = stage + (r - p) * pitch + phase(r, 0) + (c0 - cs0) * 3;
                    for (int c = 0; c < c1 - c0; ++c) {
                        acc[k][0] += tab[b[3 * c]];
                        acc[k][1] += tab[b[3 * c + 1]];
                        acc[k][2] += tab[b[3 * c + 2]];
                    }
                } else {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float *f = reinterpret_cast<const float *>(stage + ((r - p) * 3 + ch) * pitch + phase(r, ch)) + (c0 - cs0);
                        for (int c = 0; c < c1 - c0; ++c) acc[k][ch] += f[c];
                    }
                }
            }
        }
    }

    if (!col_ok) return;
    const int kw = c1 - c0;
#pragma unroll
    for (int k = 0; k < ING_K; ++k) {
        const int i = i0 + k * ING_TY + ty;
        if (i >= h) continue;
        const int kh = r1[k] - r0[k];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            dst[((n * 3 + ch) * h + i) * w + j] = ing_div(ing_div(acc[k][ch], kh), kw);
    }
}

// Tile width and staging geometry for one call: the widest tile (<= ING_TX columns) whose source rows fit a pass one at a time.
static bool ingest_geom(bool u8, int H, int W, int h, int w, OrnIngestGeom *g)
{
    const int E = u8 ? 3 : 4, LPR = u8 ? 1 : 3;
    for (int tw = ING_TX; tw >= 1; tw >>= 1) {
        const long span = ((long)tw * W + w - 1) / w + 1;                 // source columns under tw output columns, at most
        const long pitch = (span * E + 15 + 15) / 16 * 16;
        if (pitch * LPR <= ING_STAGE_BYTES) {
            long need = ((long)ING_TH * H + h - 1) / h + 1;              // source rows under a tile's ING_TH output rows, at most
            if (need > H) need = H;
            long rows = ING_STAGE_BYTES / (pitch * LPR);
            if (rows > need) rows = need;                                 // one pass then, and no more LDS than it takes
            *g = OrnIngestGeom{H, W, h, w, tw, (int)pitch, (int)rows, (int)(rows * LPR * pitch)};
            return true;
        }
    }
    return false;
}

static int ingest_launch(const char *name, bool u8, const void *src, int n, int H, int W, float *dst, int h, int w, hipStream_t st)
{
    ORN_REQUIRE(n >= 0 && H >= 1 && W >= 1 && h >= 1 && w >= 1, "%s: bad sizes n=%d %dx%d -> %dx%d", name, n, H, W, h, w);
    ORN_REQUIRE(H <= ING_MAX_DIM && W <= ING_MAX_DIM && h <= ING_MAX_DIM && w <= ING_MAX_DIM,
                "%s: %dx%d -> %dx%d beyond %d per side", name, H, W, h, w, ING_MAX_DIM);
    if (n == 0) return 0;
    ORN_REQUIRE(src && dst, "%s: null pointer", name);
    ORN_REQUIRE((uintptr_t)dst % 4 == 0 && (u8 || (uintptr_t)src % 4 == 0), "%s: fp32 pointers must be 4-byte aligned", name);
    OrnIngestGeom g;
    ORN_REQUIRE(ingest_geom(u8, H, W, h, w, &g), "%s: the window of %dx%d -> %dx%d does not fit the staging buffer", name, H, W, h, w);
    if (!u8 && H == h && W == w) {                                        // an exact copy
        if ((const void *)dst != src) ORN_HIP(hipMemcpyAsync(dst, src, (size_t)n * 3 * H * W * 4, hipMemcpyDeviceToDevice, st));
        return 0;
    }
    const size_t in_frame = (size_t)H * W * 3 * (u8 ? 1 : 4), out_frame = (size_t)h * w * 3;
    for (int k = 0; k < n; k += 65535) {                                  // gridDim.z
        const int m = n - k < 65535 ? n - k : 65535;
        const dim3 grid(orn_cdiv(w, g.tw), orn_cdiv(h, ING_TH), m);
        const unsigned char *s = (const unsigned char *)src + (size_t)k * in_frame;
        float *d = dst + (size_t)k * out_frame;
        if (u8) hipLaunchKernelGGL(k_frames_ingest<true>, grid, dim3(256), g.stage_bytes + 256 * sizeof(float), st, s, d, g);
        else hipLaunchKernelGGL(k_frames_ingest<false>, grid, dim3(256), g.stage_bytes, st, s, d, g);
        ORN_LAUNCH_CHECK(name);
    }
    return 0;
}

extern "C" int orn_frames_ingest_u8(const uint8_t *src, int n, int H, int W, float *dst, int h, int w, void *stream)
{
    return ingest_launch("frames_ingest_u8", true, src, n, H, W, dst, h, w, (hipStream_t)stream);
}

extern "C" int orn_frames_pool_f32(const float *src, int n, int H, int W, float *dst, int h, int w, void *stream)
{
    return ingest_launch("frames_pool_f32", false, src, n, H, W, dst, h, w, (hipStream_t)stream);
}
