/*
 * sws_yuy2.hip — packed 4:2:2 SOURCES (yuyv422 / uyvy422 / yvyu422: MI355_SWS_SRC_YUYV422 ... _YVYU422): the instances of the tile kernels (sws_dev.h)
 * whose horizontal pass picks its samples from the packed bytes — k_sws_generic A / B / C to rgb24, bgr24 and the four 32-bit orders, k_sws_planar
 * A / B / C at both chroma widths, plain, SEMI, RANGE and DEEP: every key of source class SWS_SRC_YUY2 (sws_dev.h: SwsKey; the key is sws.hip's) —
 * with their launch, k_sws_ident1_yuy2 (equal size to a packed RGB destination), the
 * four unscaled special converters the reference has for these sources in one kernel (k_sws_yuy2_split: yuyvToYuv420Wrapper, uyvyToYuv420Wrapper, yuyvToYuv422Wrapper, uyvyToYuv422Wrapper,
 * swscale_unscaled.c:227-287 over yuyvtoyuv420_c ... uyvytoyuv422_c, rgb2rgb_template.c:854-928), and the two Tier-1 line entries
 * mi355_sws_yuy2ToY / _yuy2ToUV (yuy2ToY_c, yuy2ToUV_c, yvy2ToUV_c, uyvyToY_c, uyvyToUV_c, input.c:369-473) with their line kernels.  The context,
 * the plan and the picture entry points are sws.hip's (mi355_sws_create_src_layout with layout 16 .. 18).  A file of its own so that it compiles
 * beside sws.hip, not behind it.
 */
#include "mi355_rt.h"
#define MI355_SWS_TILE_KERNELS_ONLY
#include "sws_dev.h"
#include "../../include/mi355dsp.h"

using namespace mi355;

namespace {
/* ---- the unscaled splitter: yuyv422 / uyvy422 -> yuv420p / yuv422p at equal size ------------------------------------------------------------
 * Every byte is a pick: luma is byte luma_off of each pair (srcW bytes on each of srcH rows), U and V bytes 1 - luma_off and 3 - luma_off of each
 * group of four — (srcW + 1) >> 1 of each on every row (4:2:2), or on srcH / 2 rows ROUNDED DOWN the truncating mean (a + b) >> 1 of source lines
 * 2r and 2r + 1 (4:2:0: the last chroma row of an odd height is never written, a one-line picture writes none).  The width rounds UP: with an odd
 * srcW the last chroma sample takes the second half of the last group, the two bytes behind the line's width, as the reference does.
 * Tiled like k_sws_nv12_split: YUY2_COLS x YUY2_ROWS luma samples a workgroup (blockIdx.z: the picture); a thread takes 32 luma samples — 64 source
 * bytes — of ONE pair of rows, so the 4:2:0 mean is taken between registers and every plane leaves in 16-byte pieces (luma two, each chroma plane
 * one), and requests every load before its first store.
 * The source: four 16-byte pieces where the plane's pointer and stride are multiples of 16 and the pieces lie inside the stride (such a plane is
 * readable over its whole stride); else the dwords that lie whole inside the bytes the reference reads (4 * ((srcW + 1) >> 1) of a line) — one load
 * each on a plane of 4-byte multiples, four byte loads each on any other.  The destination: 32 luma bytes / 16 bytes of each chroma plane in 16-byte
 * pieces where the plane's pointer and stride are multiples of 16 and the pieces lie inside the width; else byte by byte up to the width. */
constexpr int YUY2_COLS = 2048, YUY2_ROWS = 8, YUY2_PER = 32;     /* luma samples a thread and row */
static_assert(YUY2_COLS == 64 * YUY2_PER && 2 * (NT / 64) == YUY2_ROWS, "a wave covers a pair of tile rows, the waves cover the tile");

/* the truncating mean of the four bytes of a and b */
__device__ __forceinline__ uint32_t yuy2_avg4(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xFEFEFEFEu) >> 1); }

/* the bytes of one row's 64 source bytes: 32 luma bytes in l[8], 16 U bytes in u[4], 16 V bytes in v[4] */
__device__ __forceinline__ void yuy2_pick(const uint32_t *w, int luma_off, uint32_t *l, uint32_t *u, uint32_t *v)
{
    uint32_t c[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t e = sws_even4(w[2 * j], w[2 * j + 1]), o = sws_odd4(w[2 * j], w[2 * j + 1]);
        l[j] = luma_off ? o : e;
        c[j] = luma_off ? e : o;                                   /* U V U V */
    }
#pragma unroll
    for (int j = 0; j < 4; j++) { u[j] = sws_even4(c[2 * j], c[2 * j + 1]); v[j] = sws_odd4(c[2 * j], c[2 * j + 1]); }
}
/* n <= 4 * N bytes of w to d, one at a time */
template <int N> __device__ __forceinline__ void yuy2_store_bytes(uint8_t *d, const uint32_t *w, int n)
{
#pragma unroll
    for (int i = 0; i < 4 * N; i++) if (i < n) d[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
}
/* 16 * N bytes of w to d in 16-byte pieces */
template <int N> __device__ __forceinline__ void yuy2_store_wide(uint8_t *d, const uint32_t *w)
{
#pragma unroll
    for (int i = 0; i < N; i++) reinterpret_cast<sws_u32x4 *>(d)[i] = sws_u32x4{ w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3] };
}

__global__ void __launch_bounds__(NT) k_sws_yuy2_split(int luma_off, int c420, int srcW, int srcH, const mi355_sws_planar_frame *frames)
{
    mi355_sws_planar_frame fr = frames[blockIdx.z];
    fr.src[0] = mi355_global(fr.src[0]);
    for (int k = 0; k < 3; k++) fr.dst[k] = mi355_global(fr.dst[k]);
    const int tid = threadIdx.x, lane = tid & 63, rg = tid >> 6;
    const int x = blockIdx.x * YUY2_COLS + YUY2_PER * lane, r = blockIdx.y * (YUY2_ROWS / 2) + rg;      /* r: the thread's pair of rows */
    if (x >= srcW) return;                                         /* (no barrier in this kernel) */
    const int cw = (srcW + 1) >> 1, ch = c420 ? srcH >> 1 : srcH, cx = x >> 1;      /* chroma: the width rounds up, the 4:2:0 rows down */
    const int limit = 4 * cw;                                      /* bytes of a line the reference reads */
    const uintptr_t sal = reinterpret_cast<uintptr_t>(fr.src[0]) | (uintptr_t)fr.src_stride[0];
    const bool swide = (sal & 15) == 0 && 2 * x + 2 * YUY2_PER <= fr.src_stride[0], sal4 = (sal & 3) == 0;
    const int nd = imin(16, (limit - 2 * x) >> 2);                 /* dwords of the thread's 64 bytes inside the line */
    const bool lwide = x + YUY2_PER <= srcW && ((reinterpret_cast<uintptr_t>(fr.dst[0]) | (uintptr_t)fr.dst_stride[0]) & 15) == 0;
    const bool cwide = cx + YUY2_PER / 2 <= cw && ((reinterpret_cast<uintptr_t>(fr.dst[1]) | (uintptr_t)fr.dst_stride[1] |
                                                     reinterpret_cast<uintptr_t>(fr.dst[2]) | (uintptr_t)fr.dst_stride[2]) & 15) == 0;
    uint32_t w[2][16] = {};
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int y = 2 * r + j;
        if (y >= srcH) continue;                                   /* (uniform over the wave) */
        const uint8_t *sp = fr.src[0] + (size_t)y * fr.src_stride[0] + 2 * (size_t)x;
        if (swide) {
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const sws_u32x4 a = reinterpret_cast<const sws_u32x4 *>(sp)[q];
#pragma unroll
                for (int d = 0; d < 4; d++) w[j][4 * q + d] = a[d];
            }
        } else if (sal4) {
#pragma unroll
            for (int d = 0; d < 16; d++) if (d < nd) w[j][d] = reinterpret_cast<const uint32_t *>(sp)[d];
        } else {
#pragma unroll
            for (int d = 0; d < 16; d++)
                if (d < nd) w[j][d] = (uint32_t)sp[4 * d] | ((uint32_t)sp[4 * d + 1] << 8) | ((uint32_t)sp[4 * d + 2] << 16) | ((uint32_t)sp[4 * d + 3] << 24);
        }
    }
    uint32_t l[2][8], u[2][4], v[2][4];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        yuy2_pick(w[j], luma_off, l[j], u[j], v[j]);
        const int y = 2 * r + j;
        if (y >= srcH) continue;
        uint8_t *d = fr.dst[0] + (size_t)y * fr.dst_stride[0] + x;
        if (lwide) yuy2_store_wide<2>(d, l[j]);
        else yuy2_store_bytes<8>(d, l[j], imin(YUY2_PER, srcW - x));
    }
    if (c420) {
        /* chroma row r from source lines 2r and 2r + 1, both inside the picture */
        if (r >= ch) return;
        uint32_t mu[4], mv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) { mu[k] = yuy2_avg4(u[0][k], u[1][k]); mv[k] = yuy2_avg4(v[0][k], v[1][k]); }
        uint8_t *du = fr.dst[1] + (size_t)r * fr.dst_stride[1] + cx, *dv = fr.dst[2] + (size_t)r * fr.dst_stride[2] + cx;
        if (cwide) {
            yuy2_store_wide<1>(du, mu);
            yuy2_store_wide<1>(dv, mv);
        } else {
            yuy2_store_bytes<4>(du, mu, imin(YUY2_PER / 2, cw - cx));
            yuy2_store_bytes<4>(dv, mv, imin(YUY2_PER / 2, cw - cx));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int y = 2 * r + j;
            if (y >= ch) continue;
            uint8_t *du = fr.dst[1] + (size_t)y * fr.dst_stride[1] + cx, *dv = fr.dst[2] + (size_t)y * fr.dst_stride[2] + cx;
            if (cwide) {
                yuy2_store_wide<1>(du, u[j]);
                yuy2_store_wide<1>(dv, v[j]);
            } else {
                yuy2_store_bytes<4>(du, u[j], imin(YUY2_PER / 2, cw - cx));
                yuy2_store_bytes<4>(dv, v[j], imin(YUY2_PER / 2, cw - cx));
            }
        }
    }
}

/* ---- Tier-1 line kernels: yuy2ToY_c / uyvyToY_c and yuy2ToUV_c / yvy2ToUV_c / uyvyToUV_c (input.c:369-473) of one line ---------------------- */
__global__ void __launch_bounds__(NT) k_sws_line_yuy2_y(uint8_t *dst, const uint8_t *src, int width, int off)
{
    for (int i = threadIdx.x; i < width; i += NT) dst[i] = src[2 * (size_t)i + off];
}
__global__ void __launch_bounds__(NT) k_sws_line_yuy2_uv(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int uoff, int voff)
{
    for (int i = threadIdx.x; i < width; i += NT) { dstU[i] = src[4 * (size_t)i + uoff]; dstV[i] = src[4 * (size_t)i + voff]; }
}
}  // namespace

namespace {
/* ---- the scaler from these sources: the tile instances ----------------------------------------------------------------------------------------
 * k_sws_generic / k_sws_planar with the pick converter in the staging round of hscale_tile_rgb (a 2-byte "pixel" for luma, a 4-byte one for chroma):
 * the staged line holds the picked bytes, so every instance has the LDS, the waves per SIMD and the workgroups per CU of its 8-bit yuv422p twin. */
static_assert(stage_bytes<SwsPxYuy2>() == STAGE_BYTES, "the twins' staging lines");

/* (k_sws_ident1_yuy2, the equal-size form of these sources, is sws_dev.h's: sws_yuy2dst.hip compiles its packed 4:2:2 destination) */
}  // namespace

bool mi355_sws_launch_yuy2(const SwsKey &key, const SwsOperands &op)
{
    if (key.src != SWS_SRC_YUY2) return false;
    const SwsDev *dev = static_cast<const SwsDev *>(op.d);
    if (key.kernel == SWS_KERNEL_YUY2_SPLIT) {
        /* the kernel's own grid (op.grid.z: the pictures); the byte of a pair that is luma, chroma rows averaged in pairs to yuv420p */
        const SwsDev &h = *static_cast<const SwsDev *>(op.h);
        hipLaunchKernelGGL(k_sws_yuy2_split, dim3((h.srcW + YUY2_COLS - 1) / YUY2_COLS, (h.srcH + YUY2_ROWS - 1) / YUY2_ROWS, op.grid.z), dim3(NT), 0, op.s,
                           sws_yuy2_luma(h.src_layout), h.planar == MI355_SWS_DST_YUV420P ? 1 : 0, h.srcW, h.srcH, static_cast<const mi355_sws_planar_frame *>(op.frames));
        return true;
    }
    if (key.kernel == SWS_KERNEL_IDENT1_1)
        return sws_pick_dst_rgb(key.dst, [&](auto dst) {
            hipLaunchKernelGGL(k_sws_ident1_yuy2<decltype(dst)::value>, op.grid, dim3(NT), 0, op.s, dev, static_cast<const mi355_sws_frame *>(op.frames));
            return true;
        });
    return sws_launch<sws_bit(SWS_SRC_YUY2), SWS_ALL_KINDS, SWS_ALL_DSTS>(key, op);
}

extern "C" void mi355_sws_yuy2ToY(uint8_t *dst, const uint8_t *src, int width, int layout)
{
    if (width <= 0 || !sws_yuy2_src(layout)) return;
    sws_line<1>(k_sws_line_yuy2_y, &dst, src, (size_t)2 * width, width, sws_yuy2_luma(layout));
}
extern "C" void mi355_sws_yuy2ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int layout)
{
    if (width <= 0 || !sws_yuy2_src(layout)) return;
    uint8_t *const out[2] = { dstU, dstV };
    sws_line<2>(k_sws_line_yuy2_uv, out, src, (size_t)4 * width, width, sws_yuy2_u(layout), sws_yuy2_v(layout));
}
