/*
 * sws_dev.h — the device side of sws.hip and of the files that compile instances beside it (sws_deep.hip, sws_packed.hip, sws_rgb32.hip,
 * sws_yuy2.hip, sws_yuy2dst.hip — the last one the DST_YUY2 form of the packed kernels: yuyv422 / uyvy422 / yvyu422 destinations, vertical_yuy2 — and sws_p010.hip: the
 * SwsPxP010 instances, a p010le source, hscale_tile_p010): the tile geometry and its instance table, the steps of the scaler (horizontal pass into LDS, packed and planar vertical passes),
 * at the end the host side of a launch (the launch key SwsKey, the dispatcher sws_launch, the grids, the line helper) and the kernels:
 *   k_sws_generic   the generic scaler of swscale() (libswscale/swscale.c:343-722) for whole pictures,
 *                   fused per output tile: horizontal 8->15 bit FIR of the source lines the tile needs
 *                   (hScale8To15_c :133-147) into LDS, vertical FIR + yuv->rgb LUT
 *                   (yuv2rgb24_{1,2,X}_c output.c:937-1110) from LDS, RGB rows staged in LDS and
 *                   written as dwords.  No int16 intermediate ever goes to HBM.
 *   k_sws_planar    the same loop's planar branch (swscale.c:618-645, yuv2planeX_8_c / yuv2plane1_8_c output.c:242-266): the
 *                   horizontal pass into LDS as above, the vertical pass from LDS straight to the three destination planes — or, for
 *                   NV12 / NV21 (yuv2nv12cX_c :267-301), to the luma plane and one plane of interleaved chroma pairs.
 *   k_sws_nv12_pack the unscaled packer planarToNv12Wrapper (swscale_unscaled.c:138-156) for 8-bit yuv420p -> NV12 / NV21.
 *   k_sws_nv12_split the unscaled splitter nv12ToPlanarWrapper (swscale_unscaled.c:158-177) for 8-bit NV12 / NV21 -> yuv420p.
 *   k_sws_c24       the unscaled converter yuv2rgb_c_24_rgb (yuv2rgb.c:335-363) for 8-bit yuv420p and yuv422p.
 *   k_sws_ident1    the generic scaler on an 8-bit context that does not scale, from the source bytes.
 * The tile kernels are instantiated per sample type: the uint16_t instances differ in the horizontal pass (its staging lines are twice
 * as long, so is their LDS) and, for planar destinations, in the dither rows.  The NV instances of the tile kernels and of k_sws_ident1 read
 * an NV12 / NV21 source: both chroma planes from one pass over its plane of byte pairs (hscale_tile_nv).  The RGB instances of the tile kernels
 * read a packed rgb24 / bgr24 source: the reference's input converters in front of the 8-bit horizontal pass (hscale_tile_rgb).  The RANGE
 * instances of k_sws_planar convert the range of the int16 lines between the two passes (lumConvertRange / chrConvertRange: range_lines).  The DEEP
 * instances of k_sws_planar write 9- or 10-bit planes of 16-bit little-endian samples (yuv2plane1_10 / yuv2planeX_10: planar_rows16).  The DST_BGR24 /
 * DST_RGB32 instances of k_sws_generic, k_sws_ident1 and k_sws_c24 write bgr24 or one of rgba / bgra / argb / abgr in place of rgb24 (write_pair_d,
 * store8_d; compiled in sws_packed.hip).  The RGB instances whose sample type is a 32-bit pixel (SwsPx32: rgba / bgra / argb / abgr sources; compiled in
 * sws_rgb32.hip) run the same converters on a pixel that is one aligned dword; SwsPx32A: the ALPHA form of k_sws_generic, a fourth LDS tile of the
 * source's alpha through the luma banks into the alpha byte of a 32-bit destination.
 *   k_sws_fbl_generic / k_sws_fbl_planar   the two tile kernels again for SWS_FAST_BILINEAR contexts (compiled in sws_fastbl.hip): the horizontal pass
 *                   reads no filter bank (hscale_tile_fbl: hyscale_fast_c / hcscale_fast_c swscale.c:238-301), the range step and the vertical pass are
 *                   the device functions of the two kernels above.  Kernels of their own names: k_sws_generic / k_sws_planar gain no instance.
 *   k_sws_gbrp      k_sws_planar's FULL tile with the vertical pass of a planar RGB destination (compiled in sws_gbrp.hip): yuv2gbrp_full_X_c
 *                   output.c:1275-1355, the arithmetic yuv -> rgb path with six integer coefficients, no LUT.  A kernel of its own name too.
 *   k_sws_line_*    the individual inner loops for the Tier-1 entry points.
 * Execution model: 256-thread workgroups (4 waves) sharing one LDS tile; integer only, no MFMA.
 */
#ifndef MI355_SWS_DEV_H
#define MI355_SWS_DEV_H

#include <type_traits>
#include "mi355_rt.h"
#include "../../include/mi355_sws.h"

namespace {

constexpr int TW = 128;      /* output samples per tile row */
constexpr int MAXTH = 16;    /* output rows per tile (upper bound) */
constexpr int MAXL = 48;     /* source luma lines a tile may need (upper bound: the LDS tile is sized per context, sws_plan) */
constexpr int MAXC = 24;     /* source chroma lines a tile may need */
constexpr int MAXCP = 48;    /* ... of a planar destination (its tile holds no LUT and no output rows; a 4:2:0 chroma plane's filters are as long as the luma's) */
constexpr int NT = 256;

/* LCAP / CCAP of the three instances of k_sws_generic and of k_sws_planar (MI355_SWS_K_*_A / _B / _C): the source lines the LDS tile holds.
 * The context's largest tile span picks the instance (sws_kernel), and with it how many workgroups a CU's 160 KB hold (one wave of each
 * per SIMD).  Planar: the B instance's chroma lines cover the 2 x 7 + 8 of a 2:1 4:2:0 reduction at 16-row tiles (seven workgroups a CU) */
struct SwsShape { int lcap, ccap; };
constexpr SwsShape GENERIC_SHAPES[3] = { { 28, 16 }, { 40, 20 }, { MAXL, MAXC } };
constexpr SwsShape PLANAR_SHAPES[3] = { { 28, 16 }, { 40, 24 }, { MAXL, MAXCP } };

struct SwsRangeMap { int cap, mul, add, shift; };
struct SwsDev {
    int srcW, srcH, dstW, dstH, chrSrcW, chrSrcH, chrDstW, special;
    int hls, hcs, vls, vcs;                 /* filter sizes */
    const int16_t *hLumC, *hChrC, *vLumC, *vChrC;
    const int32_t *hLumP, *hChrP, *vLumP, *vChrP;
    int th;                                 /* output rows per tile chosen at create time */
    int lum_lines, chr_lines;               /* source lines the LDS tile holds (the largest span of a tile of th rows) */
    int hstage;                             /* horizontal filter positions never decrease: source spans can be staged in LDS */
    int hident_l, hident_c;                 /* the horizontal filter of the plane is the identity (one tap of 1 << 14 at position i: an unscaled
                                             * conversion through the generic path): hScale8To15 is then src << 7 */
    mi355_sws_luts luts;
    /* planar destinations (mi355_sws_create_planar): the MI355_SWS_DST_* format, its chroma subsampling and chroma rows (0 / 0 / 0 / dstH for rgb24) */
    int planar, hshift, vshift, chrDstH;
    /* the source side (mi355_sws_create_src): bits per sample (8: bytes; 9 / 10: uint16_t little endian), its chroma shifts, and the 8x8
     * dither rows a planar destination takes from a source deeper than 8 bits (swscale.c:553-556); src_layout: MI355_SWS_SRC_* — 1 / 2: the
     * second source plane holds chrSrcW byte pairs (NV12: U V, NV21: V U) and there is no third; 4 / 5 and 8 .. 11: one packed plane of three / four
     * bytes a pixel */
    int depth, src_hsub, src_vsub, src_layout;
    __attribute__((aligned(8))) uint8_t dither[8][8];
    /* range conversion between the horizontal and the vertical pass (mi355_sws_create_src_layout_range): MI355_SWS_RANGE_*, and the affine map
     * of each plane kind — (min(v, cap) * mul + add) >> shift, lumConvertRange / chrConvertRange of an 8-bit destination (swscale.c:168-198) */
    int range;
    SwsRangeMap rng_l, rng_c;
    /* a planar destination deeper than 8 bits (mi355_sws_create_src_layout_range_depth): bits per sample (8 / 9 / 10) and, for the DEEP instances,
     * the rounding term and the shift of the one-tap form and of the X form (yuv2plane1_10 / yuv2planeX_10, output.c:183-213) */
    int dst_bits;
    int v1_rnd, v1_sh, vx_rnd, vx_sh;
    /* a packed destination other than rgb24 (mi355_sws_create_src_layout_range_depth with MI355_SWS_DST_BGR24 ... _ABGR; 0: rgb24 or a planar one)
     * and, for the four 32-bit orders, the byte selector of the order (sws_rgb32_sel: read by the 32-bit instances only) */
    int packed;
    uint32_t dst_sel;
};

/* the context record with its bank pointers in the global address space (mi355_rt.h): what the tile kernels open with */
__device__ __forceinline__ SwsDev sws_dev(const SwsDev *cp)
{
    SwsDev c = *cp;
    c.hLumC = mi355_global(c.hLumC); c.hChrC = mi355_global(c.hChrC); c.vLumC = mi355_global(c.vLumC); c.vChrC = mi355_global(c.vChrC);
    c.hLumP = mi355_global(c.hLumP); c.hChrP = mi355_global(c.hChrP); c.vLumP = mi355_global(c.vLumP); c.vChrP = mi355_global(c.vChrP);
    return c;
}

struct LutLds {
    uint8_t y[1024];
    int16_t rV[256], gU[256], gV[256], bU[256];
};
__device__ __forceinline__ void lut_load(LutLds &s, const mi355_sws_luts *g, int tid)
{
    const uint32_t *src = reinterpret_cast<const uint32_t *>(g);
    uint32_t *dst = reinterpret_cast<uint32_t *>(&s);
    static_assert(sizeof(LutLds) == 3 * 4 * NT, "three dwords per thread");
    const uint32_t a = src[tid], b = src[tid + NT], c = src[tid + 2 * NT];      /* in flight together */
    dst[tid] = a; dst[tid + NT] = b; dst[tid + 2 * NT] = c;
}
__device__ __forceinline__ int clip_u8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int imax(int a, int b) { return a > b ? a : b; }
__device__ __forceinline__ int imin(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

typedef uint32_t sws_u32x2 __attribute__((vector_size(8)));
typedef uint32_t sws_u32x4 __attribute__((vector_size(16)));
/* int16 lane k of a vector (or row) of dwords: two 16-bit values a dword, as the LDS tiles and the packed taps hold them */
template <typename V> __device__ __forceinline__ int lane16(const V &v, int k) { return (int16_t)(v[k >> 1] >> (16 * (k & 1))); }
/* the LUT row offsets of a pair's chroma */
__device__ __forceinline__ void lut_rows(const LutLds &t, int U, int V, int &r, int &g, int &b) { r = t.rV[V]; g = t.gU[U] + t.gV[V]; b = t.bU[U]; }
/* yuv2rgb_write, rgb24 branch (output.c:853-866) */
__device__ __forceinline__ void write_pair(const LutLds &t, uint8_t *dest, int Y1, int Y2, int U, int V)
{
    int r, g, b;
    lut_rows(t, U, V, r, g, b);
    dest[0] = t.y[r + Y1]; dest[1] = t.y[g + Y1]; dest[2] = t.y[b + Y1];
    dest[3] = t.y[r + Y2]; dest[4] = t.y[g + Y2]; dest[5] = t.y[b + Y2];
}
/* ---- packed destinations other than rgb24: the DST template forms of the packed kernels (DST_RGB24 is the code above and below, unchanged) ----
 * DST_BGR24: yuv2rgb_write with r_b / b_r the other way round (output.c:853-866) — the r and the b row offsets change places at compile time, every
 *   store stays.
 * DST_RGB32: rgba / bgra / argb / abgr, one dword a pixel: the reference's r[Y] + g[Y] + b[Y] over its uint32_t tables (output.c:831-851,
 *   yuv2rgb.c:864-888) is the 24-bpp case's clipped byte in three lanes and 255 in the fourth (a source without alpha) — here the three byte reads
 *   of y_table assembled as r | g << 8 | b << 16 | 255 << 24 and put into the order's bytes by ONE byte permute; its selector is the same on every
 *   lane (SwsDev::dst_sel, or a kernel argument), so one form serves the four orders. */
/* DST_YUY2: yuyv422 / yvyu422 / uyvy422, two bytes a pixel (yuv2422_X / _2 / _1_c_template output.c:451-582: the templates' Y1, Y2, U, V, and no table behind
 *   them) — a pair is ONE dword Y1 | U << 8 | Y2 << 16 | V << 24, each value truncated to its byte as the reference's stores truncate it, put into the
 *   order's bytes by the same byte permute (sws_yuy2_dst_sel).  The form has no LUT: neither lut_load nor LutLds (compiled in sws_yuy2dst.hip). */
constexpr int DST_RGB24 = 0, DST_BGR24 = 1, DST_RGB32 = 2, DST_YUY2 = 3;
template <int DST> __host__ __device__ constexpr int dst_bpp() { return DST == DST_RGB32 ? 4 : (DST == DST_YUY2 ? 2 : 3); }
/* the selector of a 32-bit order (MI355_SWS_DST_RGBA ... _ABGR): byte k of the stored dword is byte (sel >> 8 k) & 3 of r | g << 8 | b << 16 | a << 24 */
__host__ __device__ constexpr uint32_t sws_rgb32_sel(int dst_format)
{
    return dst_format == MI355_SWS_DST_RGBA ? 0x03020100u : (dst_format == MI355_SWS_DST_BGRA ? 0x03000102u :
           (dst_format == MI355_SWS_DST_ARGB ? 0x02010003u : 0x00010203u));
}
/* the selector of a packed 4:2:2 order (MI355_SWS_DST_YUYV422 / _UYVY422 / _YVYU422) over Y1 | U << 8 | Y2 << 16 | V << 24: Y1 U Y2 V, U Y1 V Y2, Y1 V Y2 U */
__host__ __device__ constexpr bool sws_yuy2_dst(int dst_format) { return dst_format >= MI355_SWS_DST_YUYV422 && dst_format <= MI355_SWS_DST_YVYU422; }
__host__ __device__ constexpr uint32_t sws_yuy2_dst_sel(int dst_format)
{
    return dst_format == MI355_SWS_DST_UYVY422 ? 0x02030001u : (dst_format == MI355_SWS_DST_YVYU422 ? 0x01020300u : 0x03020100u);
}
#ifdef MI355_HIP_EMU_H
static inline uint32_t sws_order4(uint32_t w, uint32_t sel)
{
    uint32_t o = 0;
    for (int k = 0; k < 4; k++) o |= ((w >> (8 * ((sel >> (8 * k)) & 3))) & 0xFFu) << (8 * k);
    return o;
}
#else
__device__ __forceinline__ uint32_t sws_order4(uint32_t w, uint32_t sel) { return __builtin_amdgcn_perm(0u, w, sel); }     /* v_perm_b32 */
#endif
template <int DST> __device__ __forceinline__ void lut_rows_d(const LutLds &t, int U, int V, int &r, int &g, int &b)
{
    if constexpr (DST == DST_BGR24) lut_rows(t, U, V, b, g, r);
    else lut_rows(t, U, V, r, g, b);
}
/* one pixel of a 32-bit order from its row offsets */
__device__ __forceinline__ uint32_t rgb32_pixel(const LutLds &t, int r, int g, int b, int Y, uint32_t sel)
{
    return sws_order4((uint32_t)t.y[r + Y] | ((uint32_t)t.y[g + Y] << 8) | ((uint32_t)t.y[b + Y] << 16) | 0xFF000000u, sel);
}
/* ... with the pixel's own alpha (yuv2rgb_write with hasAlpha, output.c:843-847: the reference's tables then hold 0 in the alpha lane and A << 24 — or
 * << 0 for the two orders with alpha first — is added; here A enters the assembled dword where 255 goes otherwise, and the same permute places it) */
__device__ __forceinline__ uint32_t rgb32_pixel_a(const LutLds &t, int r, int g, int b, int Y, int A, uint32_t sel)
{
    return sws_order4((uint32_t)t.y[r + Y] | ((uint32_t)t.y[g + Y] << 8) | ((uint32_t)t.y[b + Y] << 16) | ((uint32_t)A << 24), sel);
}
__device__ __forceinline__ void write_pair_a(const LutLds &t, uint8_t *dest, int Y1, int Y2, int U, int V, int A1, int A2, uint32_t sel)
{
    int r, g, b;
    lut_rows(t, U, V, r, g, b);
    uint32_t *q = reinterpret_cast<uint32_t *>(dest);
    q[0] = rgb32_pixel_a(t, r, g, b, Y1, A1, sel); q[1] = rgb32_pixel_a(t, r, g, b, Y2, A2, sel);
}
/* yuv2rgb_write of one pair: six bytes, or two dwords at dest (a multiple of 4) */
/* one group of a packed 4:2:2 order: the four values as they are, truncated to bytes (output_pixels, output.c:451-467) */
__device__ __forceinline__ uint32_t yuy2_group(int Y1, int U, int Y2, int V, uint32_t sel)
{
    return sws_order4(((uint32_t)Y1 & 0xFFu) | (((uint32_t)U & 0xFFu) << 8) | (((uint32_t)Y2 & 0xFFu) << 16) | ((uint32_t)V << 24), sel);
}
template <int DST> __device__ __forceinline__ void write_pair_d(const LutLds &t, uint8_t *dest, int Y1, int Y2, int U, int V, uint32_t sel)
{
    if constexpr (DST == DST_YUY2) {
        /* four bytes at any address (a line entry's dest, a ragged row of k_sws_ident1) */
        const uint32_t w = yuy2_group(Y1, U, Y2, V, sel);
        dest[0] = (uint8_t)w; dest[1] = (uint8_t)(w >> 8); dest[2] = (uint8_t)(w >> 16); dest[3] = (uint8_t)(w >> 24);
    } else
    if constexpr (DST == DST_RGB24) write_pair(t, dest, Y1, Y2, U, V);
    else {
        int r, g, b;
        lut_rows_d<DST>(t, U, V, r, g, b);
        if constexpr (DST == DST_BGR24) {
            dest[0] = t.y[r + Y1]; dest[1] = t.y[g + Y1]; dest[2] = t.y[b + Y1];
            dest[3] = t.y[r + Y2]; dest[4] = t.y[g + Y2]; dest[5] = t.y[b + Y2];
        } else {
            uint32_t *q = reinterpret_cast<uint32_t *>(dest);
            q[0] = rgb32_pixel(t, r, g, b, Y1, sel); q[1] = rgb32_pixel(t, r, g, b, Y2, sel);
        }
    }
}

/* one output pair of the three packed templates; rows are addressed through accessors so the same
 * code serves LDS tiles (whole pictures) and packed global rows (Tier-1 line calls).  vertical_rows keeps its own statement of them over
 * the taps it holds in registers: a register-resident accessor here was tried and gave another instruction stream */
/* ALPHA (DST_RGB32): the hasAlpha branches of the three templates — A from R.alp() with the LUMA taps, clipped as each template clips it */
template <int DST = DST_RGB24, bool ALPHA = false, typename Rows>
__device__ __forceinline__ void rgb_pair(const LutLds &t, uint8_t *dest, const Rows &R, int i, int mode, const int16_t *lumF, int ls,
                                         const int16_t *chrF, int cs, int yalpha, int uvalpha, uint32_t sel = 0)
{
    int Y1, Y2, U, V;
    [[maybe_unused]] int A1 = 0, A2 = 0;
    if constexpr (ALPHA) {
        static_assert(DST == DST_RGB32, "alpha goes to a 32-bit destination");
        if (mode == 1) { A1 = clip_u8(R.alp(0, 2 * i) >> 7); A2 = clip_u8(R.alp(0, 2 * i + 1) >> 7); }
        else if (mode == 2) {
            const int ya1 = 4096 - yalpha;
            A1 = clip_u8((R.alp(0, 2 * i) * ya1 + R.alp(1, 2 * i) * yalpha) >> 19);
            A2 = clip_u8((R.alp(0, 2 * i + 1) * ya1 + R.alp(1, 2 * i + 1) * yalpha) >> 19);
        } else {
            A1 = A2 = 1 << 18;
            for (int j = 0; j < ls; j++) { const int f = lumF[j]; A1 += R.alp(j, 2 * i) * f; A2 += R.alp(j, 2 * i + 1) * f; }
            A1 >>= 19; A2 >>= 19;
            if ((A1 | A2) & 0x100) { A1 = clip_u8(A1); A2 = clip_u8(A2); }
        }
    }
    if (mode == 1) {          /* yuv2rgb_1_c_template output.c:1043-1110 */
        Y1 = clip_u8(R.lum(0, 2 * i) >> 7); Y2 = clip_u8(R.lum(0, 2 * i + 1) >> 7);
        if (uvalpha < 2048) { U = clip_u8(R.cu(0, i) >> 7); V = clip_u8(R.cv(0, i) >> 7); }
        else { U = clip_u8((R.cu(0, i) + R.cu(1, i)) >> 8); V = clip_u8((R.cv(0, i) + R.cv(1, i)) >> 8); }
    } else if (mode == 2) {   /* yuv2rgb_2_c_template :998-1041 */
        const int ya1 = 4096 - yalpha, ua1 = 4096 - uvalpha;
        Y1 = clip_u8((R.lum(0, 2 * i) * ya1 + R.lum(1, 2 * i) * yalpha) >> 19);
        Y2 = clip_u8((R.lum(0, 2 * i + 1) * ya1 + R.lum(1, 2 * i + 1) * yalpha) >> 19);
        U = clip_u8((R.cu(0, i) * ua1 + R.cu(1, i) * uvalpha) >> 19);
        V = clip_u8((R.cv(0, i) * ua1 + R.cv(1, i) * uvalpha) >> 19);
    } else {                  /* yuv2rgb_X_c_template :937-996: clipped only if a value has bit 8 set */
        Y1 = Y2 = U = V = 1 << 18;
        for (int j = 0; j < ls; j++) { const int f = lumF[j]; Y1 += R.lum(j, 2 * i) * f; Y2 += R.lum(j, 2 * i + 1) * f; }
        for (int j = 0; j < cs; j++) { const int f = chrF[j]; U += R.cu(j, i) * f; V += R.cv(j, i) * f; }
        Y1 >>= 19; Y2 >>= 19; U >>= 19; V >>= 19;
        if ((Y1 | Y2 | U | V) & 0x100) { Y1 = clip_u8(Y1); Y2 = clip_u8(Y2); U = clip_u8(U); V = clip_u8(V); }
    }
    if constexpr (ALPHA) write_pair_a(t, dest, Y1, Y2, U, V, A1, A2, sel);
    else
    write_pair_d<DST>(t, dest, Y1, Y2, U, V, sel);
}
/* eight neighbouring samples of a line (four pairs sharing a chroma sample each): Y values 0..255 in Y[8], the pairs' LUT
 * row offsets in r/g/b -> 24 RGB bytes at d (8-byte aligned), three 8-byte stores */
__device__ __forceinline__ void rgb24_store8(const LutLds &t, uint8_t *d, const int *Y, const int *r, const int *g, const int *b)
{
    uint32_t o[6];
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const int Y1 = Y[2 * p], Y2 = Y[2 * p + 1];
        const uint32_t r1 = t.y[r[p] + Y1], g1 = t.y[g[p] + Y1], b1 = t.y[b[p] + Y1];
        const uint32_t r2 = t.y[r[p] + Y2], g2 = t.y[g[p] + Y2], b2 = t.y[b[p] + Y2];
        /* six bytes per pair: pairs 0,2 start on a dword, pairs 1,3 in the middle of one */
        if ((p & 1) == 0) {
            o[3 * (p >> 1)] = r1 | (g1 << 8) | (b1 << 16) | (r2 << 24);
            o[3 * (p >> 1) + 1] = g2 | (b2 << 8);
        } else {
            o[3 * (p >> 1) + 1] |= (r1 << 16) | (g1 << 24);
            o[3 * (p >> 1) + 2] = b1 | (r2 << 8) | (g2 << 16) | (b2 << 24);
        }
    }
    sws_u32x2 *q = reinterpret_cast<sws_u32x2 *>(d);
    q[0] = sws_u32x2{ o[0], o[1] }; q[1] = sws_u32x2{ o[2], o[3] }; q[2] = sws_u32x2{ o[4], o[5] };
}
/* the same eight samples as 32-bit pixels: 32 bytes at d (16-byte aligned), two 16-byte stores */
__device__ __forceinline__ void rgb32_store8(const LutLds &t, uint8_t *d, const int *Y, const int *r, const int *g, const int *b, uint32_t sel)
{
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = rgb32_pixel(t, r[k >> 1], g[k >> 1], b[k >> 1], Y[k], sel);
    sws_u32x4 *q = reinterpret_cast<sws_u32x4 *>(d);
    q[0] = sws_u32x4{ o[0], o[1], o[2], o[3] }; q[1] = sws_u32x4{ o[4], o[5], o[6], o[7] };
}
/* ... each with its own alpha A[k] */
__device__ __forceinline__ void rgb32_store8_a(const LutLds &t, uint8_t *d, const int *Y, const int *A, const int *r, const int *g, const int *b, uint32_t sel)
{
    uint32_t o[8];
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = rgb32_pixel_a(t, r[k >> 1], g[k >> 1], b[k >> 1], Y[k], A[k], sel);
    sws_u32x4 *q = reinterpret_cast<sws_u32x4 *>(d);
    q[0] = sws_u32x4{ o[0], o[1], o[2], o[3] }; q[1] = sws_u32x4{ o[4], o[5], o[6], o[7] };
}
/* ... of destination form DST (bgr24: the row offsets came exchanged from lut_rows_d, the packing is rgb24's) */
template <int DST> __device__ __forceinline__ void store8_d(const LutLds &t, uint8_t *d, const int *Y, const int *r, const int *g, const int *b, uint32_t sel)
{
    if constexpr (DST == DST_RGB32) rgb32_store8(t, d, Y, r, g, b, sel);
    else rgb24_store8(t, d, Y, r, g, b);
}
__device__ __forceinline__ int packed_mode(int ls, int cs) { return (ls == 1 && cs <= 2) ? 1 : ((ls == 2 && cs == 2) ? 2 : 0); }  /* swscale.c:658-682 */

/* hScale8To15_c swscale.c:133-147 for one output sample; ST uint16_t: hScale16To15_c :110-130, sh = depth - 1 (samples below 1 << depth:
 * the sum stays inside an int) */
template <typename ST = uint8_t>
__device__ __forceinline__ int hscale_one(const uint8_t *src, const int16_t *f, int pos, int fs, int sh = 7)
{
    const ST *s = reinterpret_cast<const ST *>(src);
    int val = 0;
    for (int j = 0; j < fs; j++) val += (int)s[pos + j] * f[j];
    val >>= sh;
    return val < 32767 ? val : 32767;
}
/* the shift behind the horizontal sum: 7 for bytes, depth - 1 for 16-bit samples */
template <typename ST> __device__ __forceinline__ int hscale_shift(int depth) { return sizeof(ST) == 1 ? 7 : depth - 1; }

struct TileRows {
    const int16_t (*lumT)[TW];
    const int16_t (*cuT)[TW / 2];
    const int16_t (*cvT)[TW / 2];
    int lfirst, llo, lmax, cfirst, clo, cmax;   /* first tap line, first staged line, last picture line */
    const int16_t (*alpT)[TW] = nullptr;        /* the alpha tile of an ALPHA instance: the luma tile's lines */
    __device__ __forceinline__ int alp(int j, int x) const { return alpT[clampi(lfirst + j, 0, lmax) - llo][x]; }
    __device__ __forceinline__ int lum(int j, int x) const { return lumT[clampi(lfirst + j, 0, lmax) - llo][x]; }
    __device__ __forceinline__ int cu(int j, int x) const { return cuT[clampi(cfirst + j, 0, cmax) - clo][x]; }
    __device__ __forceinline__ int cv(int j, int x) const { return cvT[clampi(cfirst + j, 0, cmax) - clo][x]; }
};
/* Horizontal pass of one plane for a tile: COLS output columns starting at gx0, source lines lo..hi, results
 * to out[line - lo][x].  The source span the columns need ([pos[gx0], pos[last] + fs), monotonic positions)
 * is staged in LDS SG lines at a time with aligned 16-byte (or dword) loads — a few coalesced loads per thread
 * instead of fs single-byte loads per output sample; spans wider than the stage, unaligned planes and non-monotonic
 * filters take the direct path. */
constexpr int SG = 16;                /* source lines per staging round (a round costs two workgroup barriers) */
constexpr int SRC_DW = 76;            /* dwords per staged line: 2:1 with 8 taps needs 128 * 2 + 8 bytes (+2 of slack for zero taps) */
constexpr int STAGE_BYTES = (int)sizeof(uint32_t) * SG * SRC_DW;
/* a chroma tile row is half as wide: its staged lines are about half as long (64 * 2 + 8 bytes + the 15 of a 16-byte aligned start) and a
 * round holds half as many again in the same storage (the 20 chroma lines of a 2:1 reduction: one round instead of two) */
constexpr int SRC_DW_HALF = 40;
/* 16-bit samples: the same spans are twice as many bytes — (128 * 2 + 8) * 2 bytes + the 15 of an aligned start and the two dwords of slack;
 * a chroma tile row (64 * 2 + 8) * 2 + 15.  The same number of lines per round, so a 16-bit instance's staging storage is its own size. */
constexpr int SRC_DW16 = 140, SRC_DW16_HALF = 76;
constexpr int STAGE_BYTES16 = (int)sizeof(uint32_t) * SG * SRC_DW16;
/* the sample types of a packed 32-bit source (the RGB instances of rgba / bgra / argb / abgr): one pixel — SwsPx32A: its alpha byte is carried to a
 * 32-bit destination (the ALPHA form of k_sws_generic).  The pixels are converted to 8-bit samples before they are staged: the 8-bit staging lines */
struct SwsPx32 { uint32_t v; };
struct SwsPx32A { uint32_t v; };
struct SwsPxYuy2 { uint8_t v; };          /* a packed 4:2:2 source (the picked bytes are staged in the 8-bit instances' staging lines) */
struct SwsPxP010 { uint16_t v; };         /* a P010 source (the samples, word >> 6, are staged in the 16-bit instances' staging lines) */
template <typename ST> __host__ __device__ constexpr int stage_bytes() { return sizeof(ST) == 2 ? STAGE_BYTES16 : STAGE_BYTES; }
/* dwords per staged line of `cols` columns of `bytes`-byte samples: a multiple of four (16-byte LDS stores) */
__host__ __device__ constexpr int stage_pitch(int cols, int bytes) { return bytes == 1 ? (cols == TW ? SRC_DW : SRC_DW_HALF) : (cols == TW ? SRC_DW16 : SRC_DW16_HALF); }
/* a tile's source span, bytes s0 .. s1 read from the aligned start a0, as dwords; it is staged if it fits the line with two dwords to spare */
__host__ __device__ constexpr int span_dwords(int a0, int s1) { return (s1 - a0 + 3) >> 2; }
__host__ __device__ constexpr bool span_fits(int nd, int s0, int s1, int pitch) { return nd <= pitch - 2 && s1 >= s0; }
template <int COLS, typename ST = uint8_t> struct StageGeom {
    static constexpr int PITCH = stage_pitch(COLS, (int)sizeof(ST));
    static constexpr int LINES = COLS == TW ? SG : (3 * SG) / 2;       /* staged lines per round */
    static_assert(PITCH % 4 == 0 && (size_t)PITCH * LINES * sizeof(uint32_t) <= (size_t)stage_bytes<ST>(), "a round fits the staging storage");
};
constexpr int OUT_ROWS = STAGE_BYTES / (TW * 3);            /* rows of a narrow tile written per pass (they reuse the staging lines) */
static_assert(OUT_ROWS >= 8, "the narrow form needs at most two passes over a tile of MAXTH rows");
/* ... of destination form DST: a 32-bit row is TW * 4 bytes, the staging lines hold nine of them */
template <int DST> __host__ __device__ constexpr int out_rows() { return STAGE_BYTES / (TW * dst_bpp<DST>()); }
static_assert(out_rows<DST_RGB24>() == OUT_ROWS && out_rows<DST_BGR24>() == OUT_ROWS && out_rows<DST_RGB32>() == 9, "two passes at most for every form");
/* byte funnel shift, byte permute and the two-term 16-bit dot product (v_alignbyte_b32, v_perm_b32, v_dot2_i32_i16); plain C
 * under the SIMT emulator */
#ifdef MI355_HIP_EMU_H
static inline uint32_t sws_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) { return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (s & 3))); }
static inline uint32_t sws_pair(uint32_t w, int k) { return ((w >> (16 * k)) & 0xFFu) | (((w >> (16 * k + 8)) & 0xFFu) << 16); }
static inline int sws_dot2(uint32_t a, uint32_t b, int c) { return c + (int16_t)(a & 0xFFFF) * (int16_t)(b & 0xFFFF) + (int16_t)(a >> 16) * (int16_t)(b >> 16); }
static inline uint32_t sws_lo2(uint32_t a, uint32_t b) { return (a & 0xFFFFu) | (b << 16); }            /* (a.lo, b.lo) */
static inline uint32_t sws_hi2(uint32_t a, uint32_t b) { return (a >> 16) | (b & 0xFFFF0000u); }        /* (a.hi, b.hi) */
static inline uint32_t sws_zip_lo(uint32_t a, uint32_t b) { return (a & 0xFFu) | ((b & 0xFFu) << 8) | ((a & 0xFF00u) << 8) | ((b & 0xFF00u) << 16); }   /* a0 b0 a1 b1 */
static inline uint32_t sws_zip_hi(uint32_t a, uint32_t b) { return sws_zip_lo(a >> 16, b >> 16); }                                               /* a2 b2 a3 b3 */
static inline uint32_t sws_even2(uint32_t w) { return (w & 0xFFu) | (w & 0xFF0000u); }                  /* bytes 0, 2 as two 16-bit values */
static inline uint32_t sws_odd2(uint32_t w) { return ((w >> 8) & 0xFFu) | ((w >> 8) & 0xFF0000u); }     /* bytes 1, 3 */
static inline uint32_t sws_even4(uint32_t lo, uint32_t hi) { return (lo & 0xFFu) | ((lo >> 8) & 0xFF00u) | ((hi & 0xFFu) << 16) | ((hi << 8) & 0xFF000000u); }   /* bytes 0 2 4 6 of the eight */
static inline uint32_t sws_odd4(uint32_t lo, uint32_t hi) { return sws_even4(lo >> 8, hi >> 8); }                                                        /* bytes 1 3 5 7 */
#else
__device__ __forceinline__ uint32_t sws_alignbyte(uint32_t hi, uint32_t lo, uint32_t s) { return __builtin_amdgcn_alignbyte(hi, lo, s); }
/* bytes 2k, 2k + 1 of w as two 16-bit values */
__device__ __forceinline__ uint32_t sws_pair(uint32_t w, int k) { return __builtin_amdgcn_perm(0u, w, k ? 0x0C030C02u : 0x0C010C00u); }
__device__ __forceinline__ uint32_t sws_lo2(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }      /* (a.lo, b.lo) */
__device__ __forceinline__ uint32_t sws_hi2(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }      /* (a.hi, b.hi) */
/* the bytes of two dwords interleaved: a0 b0 a1 b1 / a2 b2 a3 b3 */
__device__ __forceinline__ uint32_t sws_zip_lo(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05010400u); }
__device__ __forceinline__ uint32_t sws_zip_hi(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07030602u); }
/* the de-interleave of byte pairs (an NV12 / NV21 source plane): bytes 0, 2 / 1, 3 of a dword as two 16-bit values (what v_dot2_i32_i16 takes),
 * and bytes 0 2 4 6 / 1 3 5 7 of two dwords as one */
__device__ __forceinline__ uint32_t sws_even2(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0C020C00u); }
__device__ __forceinline__ uint32_t sws_odd2(uint32_t w) { return __builtin_amdgcn_perm(0u, w, 0x0C030C01u); }
__device__ __forceinline__ uint32_t sws_even4(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x06040200u); }
__device__ __forceinline__ uint32_t sws_odd4(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_perm(hi, lo, 0x07050301u); }
typedef short sws_short2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int sws_dot2(uint32_t a, uint32_t b, int c)
{
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(sws_short2, a), __builtin_bit_cast(sws_short2, b), c, false);
}
#endif
/* a value the optimiser may not combine with what follows (an empty asm in a vector register) */
#ifdef MI355_HIP_EMU_H
static inline uint32_t sws_opaque(uint32_t v) { return v; }
#else
__device__ __forceinline__ uint32_t sws_opaque(uint32_t v)
{
    asm volatile("" : "+v"(v));
    return v;
}
#endif
/* eight taps: the column's byte offset inside a dword is the same on every staged line, so a line's eight samples are
 * three aligned dwords funnel-shifted into two, expanded to four 16-bit pairs and multiplied with the coefficient pairs
 * (3 LDS reads and 10 arithmetic instructions per output instead of 8 byte reads and 8 multiply-adds).  Products and sums
 * are the same integers (samples 0..255, coefficients 16 bits, |sum| < 2^31).
 * 16-bit samples are already the lanes of the dot product: a line's eight samples are five aligned dwords funnel-shifted by
 * the column's odd sample (two bytes) into four pairs. */
template <int COLS, int OP = COLS, typename ST = uint8_t>
__device__ __forceinline__ void hscale_lines8(const uint8_t *row0, int16_t *out0, const uint32_t *cp, int left, int hsh = 7)
{
    constexpr int per = NT / COLS, DW = sizeof(ST) == 1 ? 3 : 5;
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(row0) & 3);
    const uint32_t *w0 = reinterpret_cast<const uint32_t *>(row0 - sh);
    const uint32_t c01 = cp[0], c23 = cp[1], c45 = cp[2], c67 = cp[3];
    static_assert(COLS >= 64, "a wave's threads share their first line: `left` is the same on all of them");
    /* four (chroma: three) lines at a time: their LDS reads go out together, then the arithmetic of the group (one read-wait-compute chain
     * per line leaves the wave waiting for the LDS once per output).  A short last round ends at a branch of the wave, between
     * groups or inside one (the reads of a group are unconditional: the staged lines exist). */
    constexpr int N = StageGeom<COLS, ST>::LINES / per, G = N % 4 == 0 ? 4 : 3, PITCH = StageGeom<COLS, ST>::PITCH;
    static_assert(StageGeom<COLS, ST>::LINES % per == 0 && N % G == 0, "whole groups of lines");
#pragma unroll
    for (int g = 0; g < N; g += G) {
        if (g * per > left) break;
        uint32_t d[G][DW];
#pragma unroll
        for (int q = 0; q < G; q++) {
            const uint32_t *w = w0 + (g + q) * per * PITCH;
#pragma unroll
            for (int k = 0; k < DW; k++) d[q][k] = w[k];
        }
#pragma unroll
        for (int q = 0; q < G; q++) {
            if ((g + q) * per > left) break;                 /* of the wave, like the one between groups */
            int v;
            if constexpr (sizeof(ST) == 1) {
                const uint32_t lo = sws_alignbyte(d[q][1], d[q][0], sh), hi = sws_alignbyte(d[q][2], d[q][1], sh);
                v = sws_dot2(sws_pair(lo, 0), c01, 0);
                v = sws_dot2(sws_pair(lo, 1), c23, v);
                v = sws_dot2(sws_pair(hi, 0), c45, v);
                v = sws_dot2(sws_pair(hi, 1), c67, v);
            } else {
                v = sws_dot2(sws_alignbyte(d[q][1], d[q][0], sh), c01, 0);
                v = sws_dot2(sws_alignbyte(d[q][2], d[q][1], sh), c23, v);
                v = sws_dot2(sws_alignbyte(d[q][3], d[q][2], sh), c45, v);
                v = sws_dot2(sws_alignbyte(d[q][4], d[q][3], sh), c67, v);
            }
            v >>= hsh;
            out0[(g + q) * per * OP] = (int16_t)(v < 32767 ? v : 32767);
        }
    }
}
/* the general line loop: TAPS taps from the registers cp, or (TAPS 0) fs taps read from the bank entry f as it goes */
template <int COLS, int TAPS, int OP = COLS, typename ST = uint8_t>
__device__ __forceinline__ void hscale_lines(const uint8_t *row0, int16_t *out0, const uint32_t *cp, int left, int hsh = 7, const int16_t *f = nullptr, int fs = 0)
{
    constexpr int per = NT / COLS, LINES = StageGeom<COLS, ST>::LINES, PITCH = StageGeom<COLS, ST>::PITCH;
    if constexpr (TAPS == 0) {
        for (int k = 0; k < LINES / per && k * per <= left; k++) {
            const ST *row = reinterpret_cast<const ST *>(row0 + k * per * (PITCH * 4));
            int val = 0;
            for (int j = 0; j < fs; j++) val += (int)row[j] * f[j];
            val >>= hsh;
            out0[k * per * OP] = (int16_t)(val < 32767 ? val : 32767);
        }
    } else {
        int cf[TAPS];
#pragma unroll
        for (int j = 0; j < TAPS; j++) cf[j] = (int16_t)(cp[j >> 1] >> (16 * (j & 1)));
#pragma unroll
        for (int k = 0; k < LINES / per; k++) {
            if (k * per > left) break;
            const ST *row = reinterpret_cast<const ST *>(row0 + k * per * (PITCH * 4));
            int val = 0;
#pragma unroll
            for (int j = 0; j < TAPS; j++) val += (int)row[j] * cf[j];
            val >>= hsh;
            out0[k * per * OP] = (int16_t)(val < 32767 ? val : 32767);
        }
    }
}
/* OP: int16 samples per line of `out` (a line may hold two planes' tiles side by side) */
/* ST: the source's sample type (uint8_t, or uint16_t for 9 / 10 bit: `depth`); srcW in samples, stride in bytes */
template <int COLS, int OP = COLS, typename ST = uint8_t>
__device__ __forceinline__ void hscale_tile(int16_t (*out)[OP], const uint8_t *src, int stride, int srcW, const int32_t *posT,
                                            const int16_t *coefT, int fs, int gx0, int ncols, int lo, int hi,
                                            uint32_t *stage_mem, int tid, bool zero_tail, bool may_stage, bool identity, int depth = 8)
{
    constexpr int PITCH = StageGeom<COLS, ST>::PITCH, LINES = StageGeom<COLS, ST>::LINES, B = (int)sizeof(ST);
    const int hsh = hscale_shift<ST>(depth);
    uint32_t (*stage)[PITCH] = reinterpret_cast<uint32_t (*)[PITCH]>(stage_mem);
    /* two bodies: one parameterised on the sample size was tried and gave another instruction stream of the 8-bit tile kernels */
    if constexpr (B == 2) if (identity) {
        /* one tap of 1 << 14 at position i: (src * 16384) >> (depth - 1) = src << (15 - depth), below the clamp for samples below
         * 1 << depth; two samples a dword, shifted in place.  Eight columns per thread: one 16-byte load, one 16-byte LDS write */
        constexpr int TPL = COLS / 8;
        const int xg = 8 * (tid % TPL), gxi = gx0 + xg, up = 15 - depth;
        const bool al16 = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride | (uintptr_t)(2 * gx0)) & 15) == 0;
        for (int l = lo + tid / TPL; l <= hi; l += NT / TPL) {
            const uint8_t *p = src + (size_t)l * stride + 2 * gxi;
            sws_u32x4 o = { 0u, 0u, 0u, 0u };
            if (al16 && gxi + 8 <= srcW && gxi + 8 <= ncols) o = *reinterpret_cast<const sws_u32x4 *>(p);
            else {
                for (int k = 0; k < 8; k++)
                    if (gxi + k < ncols && gxi + k < srcW) o[k >> 1] |= (uint32_t)reinterpret_cast<const uint16_t *>(p)[k] << (16 * (k & 1));
            }
            for (int k = 0; k < 4; k++) o[k] <<= up;
            if (zero_tail || gxi < ncols) *reinterpret_cast<sws_u32x4 *>(&out[l - lo][xg]) = o;
        }
        return;
    }
    if (identity) {
        /* one tap of 1 << 14 at position i: (src * 16384) >> 7 = src << 7 (below the 32767 clamp).  Eight columns per thread:
         * one 8-byte load (aligned planes, inside the line), one 16-byte LDS write */
        constexpr int TPL = COLS / 8;                  /* threads per line */
        const int xg = 8 * (tid % TPL), gxi = gx0 + xg;
        const bool al8 = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride | (uintptr_t)gx0) & 7) == 0;
        for (int l = lo + tid / TPL; l <= hi; l += NT / TPL) {
            const uint8_t *p = src + (size_t)l * stride + gxi;
            uint32_t b0 = 0, b1 = 0;
            if (al8 && gxi + 8 <= srcW && gxi + 8 <= ncols) { const sws_u32x2 w = *reinterpret_cast<const sws_u32x2 *>(p); b0 = w[0]; b1 = w[1]; }
            else {
                for (int k = 0; k < 4; k++) {
                    if (gxi + k < ncols && gxi + k < srcW) b0 |= (uint32_t)p[k] << (8 * k);
                    if (gxi + 4 + k < ncols && gxi + 4 + k < srcW) b1 |= (uint32_t)p[4 + k] << (8 * k);
                }
            }
            /* bytes -> int16 << 7, two per dword */
            sws_u32x4 o;
            o[0] = ((b0 & 0xFFu) << 7) | ((b0 & 0xFF00u) << 15);
            o[1] = ((b0 >> 9) & 0x7F80u) | ((b0 >> 1) & 0x7F800000u);
            o[2] = ((b1 & 0xFFu) << 7) | ((b1 & 0xFF00u) << 15);
            o[3] = ((b1 >> 9) & 0x7F80u) | ((b1 >> 1) & 0x7F800000u);
            if (zero_tail || gxi < ncols) *reinterpret_cast<sws_u32x4 *>(&out[l - lo][xg]) = o;
        }
        return;
    }
    const int x = tid & (COLS - 1), gx = gx0 + x, per = NT / COLS;
    const bool col_ok = gx < ncols;
    /* no load below sits under a lane condition (a conditional load is a branch, the load and a wait for it: a memory round
     * trip per tap): columns past the picture read the last column's entries and do not use them */
    const int gxc = col_ok ? gx : ncols - 1;
    const int pos = posT[gxc];
    const int16_t *f = coefT + (size_t)gxc * fs;
    const int last = imin(gx0 + COLS, ncols) - 1;
    /* 16-byte pieces when the plane allows it, dwords otherwise */
    const bool al16 = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const int s0 = B * posT[gx0], s1 = B * (posT[last] + fs), a0 = al16 ? (s0 & ~15) : (s0 & ~3), nd = (s1 - a0 + 3) >> 2;     /* bytes */
    /* the column's filter in registers as four pairs of 16-bit taps (taps past fs are zero): the line loops below multiply by
     * them instead of reloading.  Eight taps: the column's entry of the bank is one aligned 16-byte word (the banks are
     * hipMalloc'ed by mi355_sws_create) */
    uint32_t cp[4];
    if (fs == 8) {
        const uint4 w = *reinterpret_cast<const uint4 *>(f);
        cp[0] = w.x; cp[1] = w.y; cp[2] = w.z; cp[3] = w.w;
    } else {
        int t[8];
#pragma unroll
        for (int j = 0; j < 8; j++) t[j] = f[j < fs ? j : 0];
#pragma unroll
        for (int j = 0; j < 4; j++) cp[j] = (2 * j < fs ? (uint32_t)t[2 * j] & 0xFFFFu : 0u) | (2 * j + 1 < fs ? (uint32_t)t[2 * j + 1] << 16 : 0u);
    }
    /* span_fits(nd, s0, s1, PITCH) spelled out: the call here was tried and gave another instruction stream of every tile kernel */
    const bool staged = may_stage && nd <= PITCH - 2 && s1 >= s0 && ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 3) == 0;
    if (!staged) {
        if (col_ok) {
            for (int l = lo + tid / COLS; l <= hi; l += per) out[l - lo][x] = (int16_t)hscale_one<ST>(src + (size_t)l * stride, f, pos, fs, hsh);
        } else if (zero_tail) {
            for (int l = lo + tid / COLS; l <= hi; l += per) out[l - lo][x] = 0;
        }
        return;
    }
    /* idx / n as a 24-bit multiply and a shift (mi355_div20: exact for idx * n < 2^19; here idx < LINES * n, n <= PITCH) */
    static_assert(LINES * PITCH * PITCH < (1 << 19), "mi355_div20 range");
    const int np = al16 ? (nd + 3) >> 2 : nd, inv = mi355_inv20(np);
    /* 16-byte pieces travel through registers, one round ahead: the loads of round r + 1 are issued before round r's
     * arithmetic and stored to the staging lines after it (a round's loads would otherwise be waited for at its first
     * barrier with nothing to do: a third of the kernel's time on a 2:1 reduction).  At most PF pieces per thread and round. */
    constexpr int PF = (LINES * ((PITCH + 3) / 4) + NT - 1) / NT;
    uint4 pre[PF];
    /* which piece of a round a thread moves does not change from round to round: its staging row, source column and LDS address are
     * worked out once per plane.  Nothing sits under a lane condition: a piece past the round's last repeats the last one, a line past
     * the plane's last needed line repeats that one (the same bytes to the same place, or to a staging line nothing reads). */
    int p_row[PF], p_col[PF];
    uint32_t *p_lds[PF];
#pragma unroll
    for (int j = 0; j < PF; j++) {
        const int idx = imin(tid + j * NT, LINES * np - 1), r = mi355_div20(idx, inv), d = idx - r * np, off = a0 + 16 * d;
        p_row[j] = r;
        p_col[j] = imin(off, (B * srcW - 1) & ~15);
        p_lds[j] = &stage[r][4 * d];
    }
    auto fetch16 = [&](int base) {
#pragma unroll
        for (int j = 0; j < PF; j++) {
            if (j * NT >= LINES * np) break;                 /* a narrow plane's round is fewer pieces than threads: the same for every thread */
            /* the aligned 16 bytes lie inside the line's stride (both multiples of 16, column < srcW <= stride): always readable.
             * Bytes at and past srcW (padding) are whatever the plane holds there: no tap with a non-zero coefficient reads them —
             * mi355_sws_create stages only filter banks whose every position + size stays inside the line, as the reference's
             * initFilter builds them (utils.c "fix borders") — and a tap past the filter's size multiplies them by zero. */
            const uint4 w = *reinterpret_cast<const uint4 *>(src + (size_t)imin(base + p_row[j], hi) * stride + p_col[j]);
            pre[j] = w;
        }
    };
    if (al16) fetch16(lo);
    for (int base = lo; base <= hi; base += LINES) {
        if (al16) {
#pragma unroll
            for (int j = 0; j < PF; j++) {
                if (j * NT >= LINES * np) break;
                *reinterpret_cast<uint4 *>(p_lds[j]) = pre[j];
            }
        } else
        for (int idx = tid; idx < LINES * np; idx += NT) {
            const int r = mi355_div20(idx, inv), d = idx - r * np, line = base + r;
            if (line > hi) continue;
            const uint8_t *p = src + (size_t)line * stride + a0 + 4 * d;
            uint32_t w;
            if (a0 + 4 * d + 4 <= B * srcW) w = *reinterpret_cast<const uint32_t *>(p);
            else {
                w = 0;
                for (int b = 0; b < 4; b++) if (a0 + 4 * d + b < B * srcW) w |= (uint32_t)p[b] << (8 * b);
            }
            stage[r][d] = w;
        }
        __syncthreads();
        if (al16 && base + LINES <= hi) fetch16(base + LINES);
        /* the thread's column over the staged lines: fixed trip count, so line and output addresses are
         * immediate offsets from one base each; tap count rounded up to 1 / 2 / 4 / 8 (taps past fs are zero, the
         * bytes exist: slack) */
        const int r0 = tid / COLS;
        const uint8_t *row0 = reinterpret_cast<const uint8_t *>(stage[r0]) + (B * pos - a0);
        int16_t *out0 = &out[base + r0 - lo][x];
        const int left = uniform(hi - base - r0);            /* lines r0, r0 + per, ... while k * per <= left (r0: one value per wave) */
        if (col_ok) {
            if (fs == 1) hscale_lines<COLS, 1, OP, ST>(row0, out0, cp, left, hsh);
            else if (fs <= 2) hscale_lines<COLS, 2, OP, ST>(row0, out0, cp, left, hsh);
            else if (fs <= 4) hscale_lines<COLS, 4, OP, ST>(row0, out0, cp, left, hsh);
            else if (fs <= 8) hscale_lines8<COLS, OP, ST>(row0, out0, cp, left, hsh);
            else hscale_lines<COLS, 0, OP, ST>(row0, out0, cp, left, hsh, f, fs);
        } else if (zero_tail) {
            for (int k = 0; k < LINES / per && k * per <= left; k++) out0[k * per * OP] = 0;
        }
        __syncthreads();
    }
}

/* ---- an NV12 / NV21 source: both chroma planes of a tile in ONE pass over the plane of byte pairs ------------------------------------
 * The reference de-interleaves each chroma line into two temporary lines (nv12ToUV_c / nv21ToUV_c, input.c:475-497: dstU[i] = src[2 * i],
 * dstV[i] = src[2 * i + 1]) and runs hcScale on each: column x reads its taps at bytes 2 * (pos + j) for the first plane of a pair and
 * 2 * (pos + j) + 1 for the second, with the same coefficients.  out_a takes the first bytes of the pairs, out_b the second ones (the
 * caller passes U, V for NV12 and V, U for NV21).  A function of its own beside hscale_tile, not a parameter of it: the three-plane
 * instances keep their instruction streams.
 * A tile's span is 2 * (pos[last] + fs - pos[gx0]) bytes — (64 * 2 + 8) * 2 + the 15 of an aligned start for a 2:1 reduction with 8 taps: 72
 * dwords, the LUMA staging geometry (SRC_DW, SG lines a round) as it is, one round where the two planes take one each of the half geometry.
 * 2 * pos is even, so after the funnel shift by 0 or 2 a staged dword holds A0 B0 A1 B1: one permute each gives the (A0, A1) and (B0, B1)
 * 16-bit pairs of the dot product.  NPAIR tap pairs (taps rounded up to 2 / 4 / 8, those past fs carry a zero coefficient; the bytes exist:
 * the two dwords of slack), 0: fs taps read as it goes. */
template <int COLS, int NPAIR, int OP>
__device__ __forceinline__ void hscale_lines_nv(const uint8_t *row0, int16_t *oa, int16_t *ob, const uint32_t *cp, int left, const int16_t *f = nullptr, int fs = 0)
{
    constexpr int per = NT / COLS, LINES = StageGeom<TW>::LINES, PITCH = StageGeom<TW>::PITCH, N = LINES / per;
    static_assert(COLS >= 64, "a wave's threads share their first line: `left` is the same on all of them");
    if constexpr (NPAIR == 0) {
        for (int k = 0; k < N && k * per <= left; k++) {
            const uint8_t *row = row0 + k * per * (PITCH * 4);
            int a = 0, b = 0;
            for (int j = 0; j < fs; j++) { a += (int)row[2 * j] * f[j]; b += (int)row[2 * j + 1] * f[j]; }
            a >>= 7; b >>= 7;
            oa[k * per * OP] = (int16_t)(a < 32767 ? a : 32767);
            ob[k * per * OP] = (int16_t)(b < 32767 ? b : 32767);
        }
    } else {
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(row0) & 3);       /* 0 or 2 */
        const uint32_t *w0 = reinterpret_cast<const uint32_t *>(row0 - sh);
        /* four lines at a time: their LDS reads go out together, then the arithmetic of the group (as hscale_lines8; the reads of a group are
         * unconditional: the staged lines exist) */
        constexpr int G = 4;
        static_assert(N % G == 0, "whole groups of lines");
#pragma unroll
        for (int g = 0; g < N; g += G) {
            if (g * per > left) break;
            uint32_t d[G][NPAIR + 1];
#pragma unroll
            for (int q = 0; q < G; q++) {
                const uint32_t *w = w0 + (g + q) * per * PITCH;
#pragma unroll
                for (int k = 0; k <= NPAIR; k++) d[q][k] = w[k];
            }
#pragma unroll
            for (int q = 0; q < G; q++) {
                if ((g + q) * per > left) break;                 /* of the wave, like the one between groups */
                int a = 0, b = 0;
#pragma unroll
                for (int k = 0; k < NPAIR; k++) {
                    const uint32_t m = sws_alignbyte(d[q][k + 1], d[q][k], sh);
                    a = sws_dot2(sws_even2(m), cp[k], a);
                    b = sws_dot2(sws_odd2(m), cp[k], b);
                }
                a >>= 7; b >>= 7;
                oa[(g + q) * per * OP] = (int16_t)(a < 32767 ? a : 32767);
                ob[(g + q) * per * OP] = (int16_t)(b < 32767 ? b : 32767);
            }
        }
    }
}
/* srcW: pairs of a line (chrSrcW); stride in bytes.  Identity, staged and direct forms as hscale_tile's (a plane off 4-byte multiples — a pair
 * may start on an odd address — a span wider than the staged line and non-monotonic banks: direct, two bytes a step) */
template <int COLS, int OP>
__device__ __forceinline__ void hscale_tile_nv(int16_t (*out_a)[OP], int16_t (*out_b)[OP], const uint8_t *src, int stride, int srcW, const int32_t *posT,
                                               const int16_t *coefT, int fs, int gx0, int ncols, int lo, int hi,
                                               uint32_t *stage_mem, int tid, bool may_stage, bool identity)
{
    constexpr int PITCH = StageGeom<TW>::PITCH, LINES = StageGeom<TW>::LINES;
    uint32_t (*stage)[PITCH] = reinterpret_cast<uint32_t (*)[PITCH]>(stage_mem);
    if (identity) {
        /* src << 7 of both bytes of a pair.  Eight columns per thread: one 16-byte load of pairs (aligned planes, inside the line), two 16-byte
         * LDS writes */
        constexpr int TPL = COLS / 8;                  /* threads per line */
        const int xg = 8 * (tid % TPL), gxi = gx0 + xg;
        const bool al16 = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride | (uintptr_t)(2 * gx0)) & 15) == 0;
        for (int l = lo + tid / TPL; l <= hi; l += NT / TPL) {
            const uint8_t *p = src + (size_t)l * stride + 2 * gxi;
            sws_u32x4 w = { 0u, 0u, 0u, 0u };
            if (al16 && gxi + 8 <= srcW && gxi + 8 <= ncols) w = *reinterpret_cast<const sws_u32x4 *>(p);
            else {
                for (int k = 0; k < 8; k++)
                    if (gxi + k < ncols && gxi + k < srcW) w[k >> 1] |= ((uint32_t)p[2 * k] | ((uint32_t)p[2 * k + 1] << 8)) << (16 * (k & 1));
            }
            sws_u32x4 a, b;
            for (int k = 0; k < 4; k++) { a[k] = sws_even2(w[k]) << 7; b[k] = sws_odd2(w[k]) << 7; }
            if (gxi < ncols) {
                *reinterpret_cast<sws_u32x4 *>(&out_a[l - lo][xg]) = a;
                *reinterpret_cast<sws_u32x4 *>(&out_b[l - lo][xg]) = b;
            }
        }
        return;
    }
    const int x = tid & (COLS - 1), gx = gx0 + x, per = NT / COLS;
    const bool col_ok = gx < ncols;
    /* no load below sits under a lane condition: columns past the picture read the last column's entries and do not use them */
    const int gxc = col_ok ? gx : ncols - 1;
    const int pos = posT[gxc];
    const int16_t *f = coefT + (size_t)gxc * fs;
    const int last = imin(gx0 + COLS, ncols) - 1;
    const bool al16 = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const int s0 = 2 * posT[gx0], s1 = 2 * (posT[last] + fs), a0 = al16 ? (s0 & ~15) : (s0 & ~3), nd = (s1 - a0 + 3) >> 2;     /* bytes */
    uint32_t cp[4];
    if (fs == 8) {
        const uint4 w = *reinterpret_cast<const uint4 *>(f);
        cp[0] = w.x; cp[1] = w.y; cp[2] = w.z; cp[3] = w.w;
    } else {
        int t[8];
#pragma unroll
        for (int j = 0; j < 8; j++) t[j] = f[j < fs ? j : 0];
#pragma unroll
        for (int j = 0; j < 4; j++) cp[j] = (2 * j < fs ? (uint32_t)t[2 * j] & 0xFFFFu : 0u) | (2 * j + 1 < fs ? (uint32_t)t[2 * j + 1] << 16 : 0u);
    }
    const bool staged = may_stage && span_fits(nd, s0, s1, PITCH) && ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 3) == 0;
    if (!staged) {
        if (col_ok) {
            for (int l = lo + tid / COLS; l <= hi; l += per) {
                const uint8_t *s = src + (size_t)l * stride + 2 * pos;
                int a = 0, b = 0;
                for (int j = 0; j < fs; j++) { a += (int)s[2 * j] * f[j]; b += (int)s[2 * j + 1] * f[j]; }
                a >>= 7; b >>= 7;
                out_a[l - lo][x] = (int16_t)(a < 32767 ? a : 32767);
                out_b[l - lo][x] = (int16_t)(b < 32767 ? b : 32767);
            }
        }
        return;
    }
    static_assert(LINES * PITCH * PITCH < (1 << 19), "mi355_div20 range");
    const int np = al16 ? (nd + 3) >> 2 : nd, inv = mi355_inv20(np);
    /* 16-byte pieces travel through registers, one round ahead, as in hscale_tile */
    constexpr int PF = (LINES * ((PITCH + 3) / 4) + NT - 1) / NT;
    uint4 pre[PF];
    int p_row[PF], p_col[PF];
    uint32_t *p_lds[PF];
#pragma unroll
    for (int j = 0; j < PF; j++) {
        const int idx = imin(tid + j * NT, LINES * np - 1), r = mi355_div20(idx, inv), d = idx - r * np, off = a0 + 16 * d;
        p_row[j] = r;
        p_col[j] = imin(off, (2 * srcW - 1) & ~15);
        p_lds[j] = &stage[r][4 * d];
    }
    auto fetch16 = [&](int base) {
#pragma unroll
        for (int j = 0; j < PF; j++) {
            if (j * NT >= LINES * np) break;
            /* the aligned 16 bytes lie inside the line's stride (both multiples of 16, column < 2 * srcW <= stride): always readable */
            const uint4 w = *reinterpret_cast<const uint4 *>(src + (size_t)imin(base + p_row[j], hi) * stride + p_col[j]);
            pre[j] = w;
        }
    };
    if (al16) fetch16(lo);
    for (int base = lo; base <= hi; base += LINES) {
        if (al16) {
#pragma unroll
            for (int j = 0; j < PF; j++) {
                if (j * NT >= LINES * np) break;
                *reinterpret_cast<uint4 *>(p_lds[j]) = pre[j];
            }
        } else
        for (int idx = tid; idx < LINES * np; idx += NT) {
            const int r = mi355_div20(idx, inv), d = idx - r * np, line = base + r;
            if (line > hi) continue;
            const uint8_t *p = src + (size_t)line * stride + a0 + 4 * d;
            uint32_t w;
            if (a0 + 4 * d + 4 <= 2 * srcW) w = *reinterpret_cast<const uint32_t *>(p);
            else {
                w = 0;
                for (int b = 0; b < 4; b++) if (a0 + 4 * d + b < 2 * srcW) w |= (uint32_t)p[b] << (8 * b);
            }
            stage[r][d] = w;
        }
        __syncthreads();
        if (al16 && base + LINES <= hi) fetch16(base + LINES);
        const int r0 = tid / COLS;
        const uint8_t *row0 = reinterpret_cast<const uint8_t *>(stage[r0]) + (2 * pos - a0);
        int16_t *oa = &out_a[base + r0 - lo][x], *ob = &out_b[base + r0 - lo][x];
        const int left = uniform(hi - base - r0);
        if (col_ok) {
            if (fs <= 2) hscale_lines_nv<COLS, 1, OP>(row0, oa, ob, cp, left);
            else if (fs <= 4) hscale_lines_nv<COLS, 2, OP>(row0, oa, ob, cp, left);
            else if (fs <= 8) hscale_lines_nv<COLS, 4, OP>(row0, oa, ob, cp, left);
            else hscale_lines_nv<COLS, 0, OP>(row0, oa, ob, cp, left, f, fs);
        }
        __syncthreads();
    }
}

/* ---- a packed rgb24 / bgr24 source: the input converters in front of the 8-bit horizontal pass --------------------------------------------
 * The reference converts each source line into 8-bit lines of its formatConvBuffer (rgb24ToY_c / bgr24ToY_c, the ...ToUV_c and ...ToUV_half_c
 * pairs, input.c:539-623, fixed BT.601 constants :38-47) and runs hyScale / hcScale on those bytes (swscale.c:252-334).  Here a staging round
 * makes those bytes in the staged LDS lines (StageGeom as it is: the staged line holds what formatConvBuffer holds), and hscale_lines8 /
 * hscale_lines consume them unchanged; the identity form is converted sample << 7, the direct form converts the samples a column needs as it goes.
 * Luma (NP 1) and both chroma planes (NP 2: U and V from ONE pass over the pixels, each taking half of the staged lines of a round) read the
 * same plane.  A pixel is three bytes c0 c1 c2 (rgb24: R G B, bgr24: B G R): sample = (K0 c0 + K1 c1 + K2 c2 + rnd) >> sh, the halving chroma
 * converter over the sums of two neighbouring pixels with one more bit of rounding and shift.  The byte order only swaps which constant meets
 * c0 and c2.  Results lie in 16 .. 240 by the constants' sums: no clip, as the reference has none. */
constexpr int RGB_SH = 15;
constexpr int RGB_RY = (int)(0.299 * 219 / 255 * (1 << RGB_SH) + 0.5), RGB_GY = (int)(0.587 * 219 / 255 * (1 << RGB_SH) + 0.5), RGB_BY = (int)(0.114 * 219 / 255 * (1 << RGB_SH) + 0.5);
constexpr int RGB_RU = -(int)(0.169 * 224 / 255 * (1 << RGB_SH) + 0.5), RGB_GU = -(int)(0.331 * 224 / 255 * (1 << RGB_SH) + 0.5), RGB_BU = (int)(0.500 * 224 / 255 * (1 << RGB_SH) + 0.5);
constexpr int RGB_RV = (int)(0.500 * 224 / 255 * (1 << RGB_SH) + 0.5), RGB_GV = -(int)(0.419 * 224 / 255 * (1 << RGB_SH) + 0.5), RGB_BV = -(int)(0.081 * 224 / 255 * (1 << RGB_SH) + 0.5);
static_assert(RGB_GY < 32768 && RGB_BU < 32768, "the constants are 16-bit lanes of the dot product");
/* the constants of one call: plane a (Y, or U) and plane b (V) as the (K0, K1) pair of the dot product and K2; luma leaves b zero */
struct RgbK {
    uint32_t a01, b01;
    int a2, b2, rnd, sh;
};
__device__ __forceinline__ uint32_t rgb_k2(int lo, int hi) { return ((uint32_t)lo & 0xFFFFu) | ((uint32_t)hi << 16); }
__device__ __forceinline__ RgbK rgb_consts(bool chroma, bool half, bool bgr)
{
    RgbK k;
    if (!chroma) {
        k.a01 = rgb_k2(bgr ? RGB_BY : RGB_RY, RGB_GY); k.a2 = bgr ? RGB_RY : RGB_BY;
        k.b01 = 0; k.b2 = 0;
        k.rnd = 33 << (RGB_SH - 1); k.sh = RGB_SH;
    } else {
        k.a01 = rgb_k2(bgr ? RGB_BU : RGB_RU, RGB_GU); k.a2 = bgr ? RGB_RU : RGB_BU;
        k.b01 = rgb_k2(bgr ? RGB_BV : RGB_RV, RGB_GV); k.b2 = bgr ? RGB_RV : RGB_BV;
        k.rnd = half ? 257 << RGB_SH : 257 << (RGB_SH - 1); k.sh = half ? RGB_SH + 1 : RGB_SH;
    }
    return k;
}
/* any four bytes of two dwords (v_perm_b32: selector bytes 0-3 pick from lo, 4-7 from hi, 0x0C gives zero) */
#ifdef MI355_HIP_EMU_H
static inline uint32_t sws_perm(uint32_t hi, uint32_t lo, uint32_t sel)
{
    const uint64_t w = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (int k = 0; k < 4; k++) {
        const uint32_t s = (sel >> (8 * k)) & 0xFFu;
        if (s < 8) r |= (uint32_t)((w >> (8 * s)) & 0xFFu) << (8 * k);
    }
    return r;
}
#else
__device__ __forceinline__ uint32_t sws_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
#endif
/* four pixels are three dwords: each pixel's (c0, c1) as the two 16-bit lanes of the dot product and its c2 */
__device__ __forceinline__ void rgb_unpack4(const uint32_t *w, uint32_t *p01, uint32_t *c2)
{
    p01[0] = sws_perm(0u, w[0], 0x0C010C00u);   c2[0] = (w[0] >> 16) & 0xFFu;
    p01[1] = sws_perm(w[1], w[0], 0x0C040C03u); c2[1] = (w[1] >> 8) & 0xFFu;
    p01[2] = sws_perm(0u, w[1], 0x0C030C02u);   c2[2] = w[2] & 0xFFu;
    p01[3] = sws_perm(0u, w[2], 0x0C020C01u);   c2[3] = w[2] >> 24;
}
/* N dwords at byte `boff` of a line of which `limit` bytes may be read: dword loads where the plane allows it and the piece lies inside,
 * else byte by byte (bytes at and past the limit read as zero: no tap with a non-zero coefficient meets a sample made of them) */
template <int N>
__device__ __forceinline__ void rgb_load(const uint8_t *line, int boff, int limit, bool al4, uint32_t *w)
{
    if (al4 && boff + 4 * N <= limit) {
#pragma unroll
        for (int k = 0; k < N; k++) w[k] = reinterpret_cast<const uint32_t *>(line + boff)[k];
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) {
            w[k] = 0;
            for (int b = 0; b < 4; b++) if (boff + 4 * k + b < limit) w[k] |= (uint32_t)line[boff + 4 * k + b] << (8 * b);
        }
    }
}
/* converted samples s .. s + 3 of a line (s a multiple of four) as one dword per plane: 12 source bytes, 24 under halving.  The bytes pass
 * sws_opaque before they are packed, as in planar_rows */
template <int NP>
__device__ __forceinline__ void rgb_unit(const uint8_t *line, int s, bool half, bool al4, int limit, const RgbK &k, uint32_t &oa, uint32_t &ob)
{
    uint32_t p[4], c[4];
    if (half) {
        uint32_t w[6], pa[4], ca[4], pb[4], cb[4];
        rgb_load<6>(line, 6 * s, limit, al4, w);
        rgb_unpack4(w, pa, ca); rgb_unpack4(w + 3, pb, cb);
        /* the sums of two pixels stay inside the 16-bit lanes */
        p[0] = pa[0] + pa[1]; p[1] = pa[2] + pa[3]; p[2] = pb[0] + pb[1]; p[3] = pb[2] + pb[3];
        c[0] = ca[0] + ca[1]; c[1] = ca[2] + ca[3]; c[2] = cb[0] + cb[1]; c[3] = cb[2] + cb[3];
    } else {
        uint32_t w[3];
        rgb_load<3>(line, 3 * s, limit, al4, w);
        rgb_unpack4(w, p, c);
    }
    oa = ob = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        oa |= sws_opaque((uint32_t)(sws_dot2(p[q], k.a01, (int)c[q] * k.a2 + k.rnd) >> k.sh)) << (8 * q);
        if (NP > 1) ob |= sws_opaque((uint32_t)(sws_dot2(p[q], k.b01, (int)c[q] * k.b2 + k.rnd) >> k.sh)) << (8 * q);
    }
}
/* one converted sample from its bytes (the direct form and the Tier-1 line kernels): px the sample's first pixel */
__device__ __forceinline__ void rgb_sample(const uint8_t *px, bool half, const RgbK &k, int &a, int &b)
{
    int c0 = px[0], c1 = px[1], c2 = px[2];
    if (half) { c0 += px[3]; c1 += px[4]; c2 += px[5]; }
    a = (c0 * (int16_t)(k.a01 & 0xFFFF) + c1 * (int16_t)(k.a01 >> 16) + c2 * k.a2 + k.rnd) >> k.sh;
    b = (c0 * (int16_t)(k.b01 & 0xFFFF) + c1 * (int16_t)(k.b01 >> 16) + c2 * k.b2 + k.rnd) >> k.sh;
}
/* ---- a packed 32-bit source: rgba / bgra / argb / abgr (rgb16_32ToY_c_template and its ToUV / ToUV_half forms, input.c:165-255, through the four
 * wrappers with S = RGB2YUV_SHIFT + 8 :288-291) ----
 * The wrappers' constants are the rgb24 ones shifted up by eight, their rounding term 33u / 257u << (S - 1) likewise, and the masks take the alpha
 * byte away before anything is summed (the halving form adds the g fields and the r / b fields of two pixels apart, each field a nine-bit sum):
 * sample = (K0 c0 + K1 c1 + K2 c2 + rnd) >> sh over the three colour bytes, the rgb24 arithmetic with RgbK as it is.  A pixel is ONE aligned dword
 * (the reference reads AV_RN32A): shifted right by `ash` — 8 where alpha is the first byte in memory (argb / abgr), else 0 — its bytes 0, 1, 2 are
 * c0 c1 c2; bytes 0, 1 as the two 16-bit lanes of the dot product (sws_pair: alpha is not among them), byte 2 apart.  ash and which constant meets
 * c0 (bgr: bgra / abgr) are uniform values of the context, one form serves the four orders. */
__host__ __device__ constexpr bool sws_rgb32_src(int layout) { return layout >= MI355_SWS_SRC_RGBA && layout <= MI355_SWS_SRC_ABGR; }
/* a packed 4:2:2 source (yuyv422 / uyvy422 / yvyu422): where the luma, U and V bytes of a group of four lie */
__host__ __device__ constexpr bool sws_yuy2_src(int layout) { return layout >= MI355_SWS_SRC_YUYV422 && layout <= MI355_SWS_SRC_YVYU422; }
__host__ __device__ constexpr int sws_yuy2_luma(int layout) { return layout == MI355_SWS_SRC_UYVY422 ? 1 : 0; }
__host__ __device__ constexpr int sws_yuy2_u(int layout) { return layout == MI355_SWS_SRC_UYVY422 ? 0 : (layout == MI355_SWS_SRC_YVYU422 ? 3 : 1); }
__host__ __device__ constexpr int sws_yuy2_v(int layout) { return layout == MI355_SWS_SRC_UYVY422 ? 2 : (layout == MI355_SWS_SRC_YVYU422 ? 1 : 3); }
__host__ __device__ constexpr bool sws_src_bgr(int layout) { return layout == MI355_SWS_SRC_BGR24 || layout == MI355_SWS_SRC_BGRA || layout == MI355_SWS_SRC_ABGR; }
__host__ __device__ constexpr uint32_t sws_src_ash(int layout) { return layout == MI355_SWS_SRC_ARGB || layout == MI355_SWS_SRC_ABGR ? 8u : 0u; }
/* N pixels at byte `boff` (a multiple of 16) of a line of which `limit` bytes may be read: 16-byte loads on a plane of 16-byte multiples, dwords on
 * one of 4-byte multiples, while the piece lies inside; else byte by byte (bytes at and past the limit read as zero) */
template <int N>
__device__ __forceinline__ void rgb32_load(const uint8_t *line, int boff, int limit, bool al4, bool al16, uint32_t *w)
{
    static_assert(N % 4 == 0, "whole 16-byte pieces");
    if (al16 && boff + 4 * N <= limit) {
#pragma unroll
        for (int k = 0; k < N; k += 4) {
            const sws_u32x4 v = *reinterpret_cast<const sws_u32x4 *>(line + boff + 4 * k);
            w[k] = v[0]; w[k + 1] = v[1]; w[k + 2] = v[2]; w[k + 3] = v[3];
        }
    } else rgb_load<N>(line, boff, limit, al4, w);
}
/* converted samples s .. s + 3 of a line (s a multiple of four) as one dword per plane: 16 source bytes, 32 under halving; NP as rgb_unit's.
 * ALPHA: the four pixels' alpha bytes as a third dword (rgbaToA_c / abgrToA_c, input.c:305-319; never under halving: alpha is a luma-sized plane) */
template <int NP, bool ALPHA = false>
__device__ __forceinline__ void rgb32_unit(const uint8_t *line, int s, bool half, bool al4, bool al16, int limit, uint32_t ash, const RgbK &k, uint32_t &oa, uint32_t &ob,
                                           uint32_t *alpha = nullptr)
{
    uint32_t p[4], c[4];
    if (half) {
        uint32_t w[8];
        rgb32_load<8>(line, 8 * s, limit, al4, al16, w);
#pragma unroll
        for (int q = 0; q < 4; q++) {
            /* alpha leaves before the sum: the two nine-bit sums of (c0, c1) stay inside the 16-bit lanes */
            const uint32_t v0 = w[2 * q] >> ash, v1 = w[2 * q + 1] >> ash;
            p[q] = sws_pair(v0, 0) + sws_pair(v1, 0);
            c[q] = ((v0 >> 16) & 0xFFu) + ((v1 >> 16) & 0xFFu);
        }
    } else {
        uint32_t w[4];
        rgb32_load<4>(line, 4 * s, limit, al4, al16, w);
        if constexpr (ALPHA) {
            /* the alpha byte: byte 0 where the colours were shifted down, else byte 3 */
            const uint32_t sel = ash ? 0x0C0C0C00u : 0x0C0C0C03u;
            *alpha = sws_perm(0u, w[0], sel) | (sws_perm(0u, w[1], sel) << 8) | (sws_perm(0u, w[2], sel) << 16) | (sws_perm(0u, w[3], sel) << 24);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const uint32_t v = w[q] >> ash;
            p[q] = sws_pair(v, 0);
            c[q] = (v >> 16) & 0xFFu;
        }
    }
    oa = ob = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        oa |= sws_opaque((uint32_t)(sws_dot2(p[q], k.a01, (int)c[q] * k.a2 + k.rnd) >> k.sh)) << (8 * q);
        if (NP > 1) ob |= sws_opaque((uint32_t)(sws_dot2(p[q], k.b01, (int)c[q] * k.b2 + k.rnd) >> k.sh)) << (8 * q);
    }
}
/* one converted sample from its bytes (the direct form and the Tier-1 line kernels): px the sample's first pixel, first: 1 where alpha is the
 * pixel's first byte */
__device__ __forceinline__ void rgb32_sample(const uint8_t *px, bool half, int first, const RgbK &k, int &a, int &b)
{
    int c0 = px[first], c1 = px[first + 1], c2 = px[first + 2];
    if (half) { c0 += px[first + 4]; c1 += px[first + 5]; c2 += px[first + 6]; }
    a = (c0 * (int16_t)(k.a01 & 0xFFFF) + c1 * (int16_t)(k.a01 >> 16) + c2 * k.a2 + k.rnd) >> k.sh;
    b = (c0 * (int16_t)(k.b01 & 0xFFFF) + c1 * (int16_t)(k.b01 >> 16) + c2 * k.b2 + k.rnd) >> k.sh;
}
/* ---- packed 4:2:2 sources (yuyv422 / uyvy422 / yvyu422): the input converters are byte picks (yuy2ToY_c, yuy2ToUV_c, yvy2ToUV_c, uyvyToY_c, uyvyToUV_c,
 * input.c:369-473) — nothing is weighted, rounded or clipped.  Samples s .. s + 3 of a line (s a multiple of four) as one dword per plane.
 * NP 1: luma, byte sws_yuy2_luma of each pair — 8 source bytes (one 8-byte load inside a 16-byte piece of a plane of 16-byte multiples, dwords on a
 * plane of 4-byte multiples, else byte by byte).  NP 2: U into oa, V into ob, bytes sws_yuy2_u / _v of each group of four — 16 source bytes (one 16-byte
 * load, dwords, or bytes).  Bytes at and past the limit read as zero, as rgb_load's. */
template <int NP>
__device__ __forceinline__ void yuy2_unit(const uint8_t *line, int s, bool al4, bool al16, int limit, int layout, uint32_t &oa, uint32_t &ob)
{
    const bool uy = sws_yuy2_luma(layout) != 0;
    if constexpr (NP == 1) {
        uint32_t w[2];
        const int boff = 2 * s;
        if (al16 && boff + 8 <= limit) {
            const sws_u32x2 v = *reinterpret_cast<const sws_u32x2 *>(line + boff);
            w[0] = v[0]; w[1] = v[1];
        } else rgb_load<2>(line, boff, limit, al4, w);
        oa = uy ? sws_odd4(w[0], w[1]) : sws_even4(w[0], w[1]);
        ob = 0;
    } else {
        uint32_t w[4];
        rgb32_load<4>(line, 4 * s, limit, al4, al16, w);
        /* the chroma bytes of two groups as they lie (U V U V; V U V U in yvyu422), then every other one */
        const uint32_t c01 = uy ? sws_even4(w[0], w[1]) : sws_odd4(w[0], w[1]), c23 = uy ? sws_even4(w[2], w[3]) : sws_odd4(w[2], w[3]);
        const uint32_t e = sws_even4(c01, c23), o = sws_odd4(c01, c23);
        const bool vu = layout == MI355_SWS_SRC_YVYU422;
        oa = vu ? o : e; ob = vu ? e : o;
    }
}
/* one sample from its bytes (the direct form): px the sample's pair (luma) or group of four (chroma) */
__device__ __forceinline__ void yuy2_sample(const uint8_t *px, bool chroma, int layout, int &a, int &b)
{
    a = chroma ? px[sws_yuy2_u(layout)] : px[sws_yuy2_luma(layout)];
    b = chroma ? px[sws_yuy2_v(layout)] : 0;
}
/* the unit and the sample of a pixel of BPX bytes: 3 — the rgb24 forms above, 4 — the 32-bit ones, 2 — packed 4:2:2 (ash carries the layout; the
 * chroma planes are the halving form: a sample every four bytes) */
template <int NP, int BPX>
__device__ __forceinline__ void px_unit(const uint8_t *line, int s, bool half, bool al4, bool al16, int limit, uint32_t ash, const RgbK &k, uint32_t &oa, uint32_t &ob)
{
    if constexpr (BPX == 2) yuy2_unit<NP>(line, s, al4, al16, limit, (int)ash, oa, ob);
    else
    if constexpr (BPX == 4) rgb32_unit<NP>(line, s, half, al4, al16, limit, ash, k, oa, ob);
    else rgb_unit<NP>(line, s, half, al4, limit, k, oa, ob);
}
template <int BPX>
__device__ __forceinline__ void px_sample(const uint8_t *px, bool half, uint32_t ash, const RgbK &k, int &a, int &b)
{
    if constexpr (BPX == 2) yuy2_sample(px, half, (int)ash, a, b);
    else
    if constexpr (BPX == 4) rgb32_sample(px, half, (int)(ash >> 3), k, a, b);
    else rgb_sample(px, half, k, a, b);
}
/* bytes -> int16 << 7, two per dword (the identity form) */
__device__ __forceinline__ sws_u32x4 bytes_shl7(uint32_t b0, uint32_t b1)
{
    sws_u32x4 o;
    o[0] = ((b0 & 0xFFu) << 7) | ((b0 & 0xFF00u) << 15);
    o[1] = ((b0 >> 9) & 0x7F80u) | ((b0 >> 1) & 0x7F800000u);
    o[2] = ((b1 & 0xFFu) << 7) | ((b1 & 0xFF00u) << 15);
    o[3] = ((b1 >> 9) & 0x7F80u) | ((b1 >> 1) & 0x7F800000u);
    return o;
}
/* srcW: pixels of a line; nsamp: converted samples of a line (srcW, or chrSrcW); stride in bytes.  half: the halving converter — with an odd
 * srcW its last sample reads pixel srcW, three bytes past the line's width, as the reference does.  NP 1: luma into out_a; NP 2: U into out_a,
 * V into out_b.  Planes on 4-byte multiples are fetched in dwords (12 / 24 bytes a unit of four samples, whole inside the bytes the reference
 * reads), any other byte by byte — the staged form takes either, so a plane's alignment never sends a tile to the direct form.  Identity,
 * staged and direct forms as hscale_tile's (direct: spans wider than a staged line and non-monotonic banks).
 * BPX 4: a 32-bit source, a pixel one dword (ash: sws_src_ash of its order) — 16 / 32 bytes a unit, in 16-byte pieces on planes of 16-byte multiples,
 * dwords on 4-byte multiples (what the contract asks for), byte by byte otherwise; with an odd srcW the halving converter reads the four bytes of
 * pixel srcW.  ALPHA (BPX 4, luma): out_b takes the alpha plane from the same pixel fetch — the reference's rgbaToA_c / abgrToA_c line through
 * hyScale with the LUMA bank (swscale.c:269-276); two planes staged, as for chroma. */
template <int COLS, int OP, int NP, int BPX = 3, bool ALPHA = false>
__device__ __forceinline__ void hscale_tile_rgb(int16_t (*out_a)[OP], int16_t (*out_b)[OP], const uint8_t *src, int stride, int srcW, int nsamp, bool half, bool bgr,
                                                const int32_t *posT, const int16_t *coefT, int fs, int gx0, int ncols, int lo, int hi,
                                                uint32_t *stage_mem, int tid, bool zero_tail, bool may_stage, bool identity, uint32_t ash = 0)
{
    static_assert(!ALPHA || (BPX == 4 && NP == 2), "the alpha plane rides with the luma of a 32-bit source as a second staged plane");
    constexpr int PITCH = StageGeom<COLS>::PITCH, LR = StageGeom<COLS>::LINES / NP;      /* staged lines of a plane per round */
    static_assert(StageGeom<COLS>::LINES % NP == 0 && LR >= NT / COLS, "every thread's first line is staged");
    const RgbK K = rgb_consts(NP > 1 && !ALPHA, half, bgr);
    const bool al4 = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 3) == 0;
    const bool al16 = BPX != 3 && ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const int limit = BPX * (half ? (srcW + 1) & ~1 : srcW);                             /* bytes of a line the reference reads */
    if (identity) {
        /* converted sample << 7.  Eight columns per thread: two units, one 16-byte LDS write per plane */
        constexpr int TPL = COLS / 8;                  /* threads per line */
        const int xg = 8 * (tid % TPL), gxi = gx0 + xg;
        uint32_t keep[2] = { 0, 0 };                   /* the bytes of columns inside the plane */
        for (int q = 0; q < 8; q++) if (gxi + q < ncols && gxi + q < nsamp) keep[q >> 2] |= 0xFFu << (8 * (q & 3));
        for (int l = lo + tid / TPL; l <= hi; l += NT / TPL) {
            const uint8_t *line = src + (size_t)l * stride;
            uint32_t a0 = 0, a1 = 0, b0 = 0, b1 = 0;
            if constexpr (ALPHA) {
                uint32_t none;
                if (keep[0]) rgb32_unit<1, true>(line, gxi, false, al4, al16, limit, ash, K, a0, none, &b0);
                if (keep[1]) rgb32_unit<1, true>(line, gxi + 4, false, al4, al16, limit, ash, K, a1, none, &b1);
            } else {
            if (keep[0]) px_unit<NP, BPX>(line, gxi, half, al4, al16, limit, ash, K, a0, b0);
            if (keep[1]) px_unit<NP, BPX>(line, gxi + 4, half, al4, al16, limit, ash, K, a1, b1);
            }
            if (zero_tail || gxi < ncols) {
                *reinterpret_cast<sws_u32x4 *>(&out_a[l - lo][xg]) = bytes_shl7(a0 & keep[0], a1 & keep[1]);
                if (NP > 1) *reinterpret_cast<sws_u32x4 *>(&out_b[l - lo][xg]) = bytes_shl7(b0 & keep[0], b1 & keep[1]);
            }
        }
        return;
    }
    const int x = tid & (COLS - 1), gx = gx0 + x, per = NT / COLS;
    const bool col_ok = gx < ncols;
    /* columns past the picture read the last column's entries and do not use them */
    const int gxc = col_ok ? gx : ncols - 1;
    const int pos = posT[gxc];
    const int16_t *f = coefT + (size_t)gxc * fs;
    const int last = imin(gx0 + COLS, ncols) - 1;
    /* the tile's span in converted samples, from a multiple of four: whole units */
    const int s0 = posT[gx0], s1 = posT[last] + fs, a0 = s0 & ~3, nd = span_dwords(a0, s1);
    uint32_t cp[4];
    if (fs == 8) {
        const uint4 w = *reinterpret_cast<const uint4 *>(f);
        cp[0] = w.x; cp[1] = w.y; cp[2] = w.z; cp[3] = w.w;
    } else {
        int t[8];
#pragma unroll
        for (int j = 0; j < 8; j++) t[j] = f[j < fs ? j : 0];
#pragma unroll
        for (int j = 0; j < 4; j++) cp[j] = (2 * j < fs ? (uint32_t)t[2 * j] & 0xFFFFu : 0u) | (2 * j + 1 < fs ? (uint32_t)t[2 * j + 1] << 16 : 0u);
    }
    if (!(may_stage && span_fits(nd, s0, s1, PITCH))) {
        if (col_ok) {
            const int step = half ? 2 * BPX : BPX;
            for (int l = lo + tid / COLS; l <= hi; l += per) {
                const uint8_t *s = src + (size_t)l * stride + (size_t)step * pos;
                int a = 0, b = 0;
                for (int j = 0; j < fs; j++) {
                    int ya, yb;
                    px_sample<BPX>(s + step * j, half, ash, K, ya, yb);
                    if constexpr (ALPHA) yb = s[step * j + (ash ? 0 : 3)];
                    a += ya * f[j]; b += yb * f[j];
                }
                a >>= 7; b >>= 7;
                out_a[l - lo][x] = (int16_t)(a < 32767 ? a : 32767);
                if (NP > 1) out_b[l - lo][x] = (int16_t)(b < 32767 ? b : 32767);
            }
        } else if (zero_tail) {
            for (int l = lo + tid / COLS; l <= hi; l += per) {
                out_a[l - lo][x] = 0;
                if constexpr (ALPHA) out_b[l - lo][x] = 0;
            }
        }
        return;
    }
    static_assert(StageGeom<COLS>::LINES * PITCH * PITCH < (1 << 19), "mi355_div20 range");
    const int inv = mi355_inv20(nd);
    uint32_t (*stage)[LR][PITCH] = reinterpret_cast<uint32_t (*)[LR][PITCH]>(stage_mem);      /* [plane][line][dword] */
    for (int base = lo; base <= hi; base += LR) {
        for (int idx = tid; idx < LR * nd; idx += NT) {
            const int r = mi355_div20(idx, inv), d = idx - r * nd, line = base + r;
            if (line > hi) continue;
            uint32_t oa, ob;
            if constexpr (ALPHA) { uint32_t none; rgb32_unit<1, true>(src + (size_t)line * stride, a0 + 4 * d, false, al4, al16, limit, ash, K, oa, none, &ob); }
            else px_unit<NP, BPX>(src + (size_t)line * stride, a0 + 4 * d, half, al4, al16, limit, ash, K, oa, ob);
            stage[0][r][d] = oa;
            if (NP > 1) stage[1][r][d] = ob;
        }
        __syncthreads();
        /* the thread's column over the staged lines of each plane, as hscale_tile; a plane's round is LR lines */
        const int r0 = tid / COLS;
        const int left = uniform(imin(hi - base, LR - 1) - r0);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const uint8_t *row0 = reinterpret_cast<const uint8_t *>(stage[p][r0]) + (pos - a0);
            int16_t *out0 = p ? &out_b[base + r0 - lo][x] : &out_a[base + r0 - lo][x];
            if (col_ok) {
                if (fs == 1) hscale_lines<COLS, 1, OP>(row0, out0, cp, left);
                else if (fs <= 2) hscale_lines<COLS, 2, OP>(row0, out0, cp, left);
                else if (fs <= 4) hscale_lines<COLS, 4, OP>(row0, out0, cp, left);
                else if (fs <= 8) hscale_lines8<COLS, OP>(row0, out0, cp, left);
                else hscale_lines<COLS, 0, OP>(row0, out0, cp, left, 7, f, fs);
            } else if (zero_tail) {
                for (int k = 0; k < LR / per && k * per <= left; k++) out0[k * per * OP] = 0;
            }
        }
        __syncthreads();
    }
}

/* ---- a P010 source (p010le): the input converters in front of the 16-bit horizontal pass ----------------------------------------------------
 * The reference converts each source line into 16-bit lines of its formatConvBuffer (p010LEToY_c / p010LEToUV_c, input.c:499-524: dst[i] =
 * word >> 6; U from the first, V from the second word of a pair) and runs hScale16To15_c with depth 10 on them (swscale.c:110-130).  Here a staging
 * round makes those lines in the 16-bit instances' staging storage (StageGeom<COLS, uint16_t> as it is: a staged line holds what formatConvBuffer
 * holds), and hscale_lines8 / hscale_lines consume them unchanged with hsh = 9.  Every uint16_t value is a sample: the low six bits are dropped.
 * NP 1: the luma plane, srcW words a line.  NP 2: the plane of pairs, chrSrcW pairs of four bytes a line — de-interleaved as it is staged (sws_lo2 /
 * sws_hi2 over two dwords), so U and V each lie in a line of the chroma geometry and take half of the staged lines of a round, as the two
 * planes of a packed source do in hscale_tile_rgb.  A unit is eight samples of a line, 16 bytes of the luma plane and 32 of the pair plane: aligned
 * 16-byte pieces on a plane of 16-byte multiples, dwords on one of 4-byte multiples, 16-bit loads otherwise (pointers and strides are even), each
 * while the piece lies whole inside the 2 * srcW / 4 * chrSrcW bytes of the line; words at and past that read as zero (no tap with a non-zero
 * coefficient meets them: mi355_sws_create stages only banks whose every position + size stays inside the line). */
__device__ __forceinline__ uint32_t p010_shr6(uint32_t w) { return (w >> 6) & 0x03FF03FFu; }      /* both 16-bit lanes of a dword */
template <int N>
__device__ __forceinline__ void p010_load(const uint8_t *line, int boff, int limit, bool al4, bool al16, uint32_t *w)
{
    static_assert(N % 4 == 0, "whole 16-byte pieces");
    if (al16 && boff + 4 * N <= limit) {
#pragma unroll
        for (int k = 0; k < N; k += 4) {
            const sws_u32x4 v = *reinterpret_cast<const sws_u32x4 *>(line + boff + 4 * k);
            w[k] = v[0]; w[k + 1] = v[1]; w[k + 2] = v[2]; w[k + 3] = v[3];
        }
    } else if (al4 && boff + 4 * N <= limit) {
#pragma unroll
        for (int k = 0; k < N; k++) w[k] = reinterpret_cast<const uint32_t *>(line + boff)[k];
    } else {
#pragma unroll
        for (int k = 0; k < N; k++) {
            w[k] = 0;
            for (int h = 0; h < 2; h++)
                if (boff + 4 * k + 2 * h < limit) w[k] |= (uint32_t)*reinterpret_cast<const uint16_t *>(line + boff + 4 * k + 2 * h) << (16 * h);
        }
    }
}
/* samples s .. s + 7 of a line (s a multiple of eight) as four dwords per plane: NP 1 luma into oa; NP 2 U into oa, V into ob */
template <int NP>
__device__ __forceinline__ void p010_unit(const uint8_t *line, int s, bool al4, bool al16, int limit, sws_u32x4 &oa, sws_u32x4 &ob)
{
    if constexpr (NP == 1) {
        uint32_t w[4];
        p010_load<4>(line, 2 * s, limit, al4, al16, w);
#pragma unroll
        for (int k = 0; k < 4; k++) { oa[k] = p010_shr6(w[k]); ob[k] = 0; }
    } else {
        uint32_t w[8];
        p010_load<8>(line, 4 * s, limit, al4, al16, w);
#pragma unroll
        for (int k = 0; k < 4; k++) { oa[k] = p010_shr6(sws_lo2(w[2 * k], w[2 * k + 1])); ob[k] = p010_shr6(sws_hi2(w[2 * k], w[2 * k + 1])); }
    }
}
/* nsamp: samples of a line and plane (srcW, or chrSrcW pairs); stride in bytes.  Identity, staged and direct forms as hscale_tile's: the identity
 * columns are sample << 5 (one tap of 1 << 14 shifted down by depth - 1 = 9), the direct form (spans wider than a staged line, non-monotonic banks)
 * reads word by word.  A tile's span is staged from a multiple of eight samples — the aligned 16 bytes the planar 16-bit source starts from — so a
 * span fits here exactly where it fits a staged line of that source; the plane's alignment picks the loads of a unit, never the form. */
template <int COLS, int OP, int NP>
__device__ __forceinline__ void hscale_tile_p010(int16_t (*out_a)[OP], int16_t (*out_b)[OP], const uint8_t *src, int stride, int nsamp, const int32_t *posT,
                                                 const int16_t *coefT, int fs, int gx0, int ncols, int lo, int hi,
                                                 uint32_t *stage_mem, int tid, bool zero_tail, bool may_stage, bool identity)
{
    constexpr int PITCH = StageGeom<COLS, uint16_t>::PITCH, LR = StageGeom<COLS, uint16_t>::LINES / NP;      /* staged lines of a plane per round */
    static_assert(StageGeom<COLS, uint16_t>::LINES % NP == 0 && LR >= NT / COLS, "every thread's first line is staged");
    constexpr int HSH = 9, UP = 5;                     /* hScale16To15_c's shift at depth 10, and 14 - HSH */
    const bool al4 = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 3) == 0;
    const bool al16 = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride) & 15) == 0;
    const int limit = 2 * NP * nsamp;                  /* bytes of a line the reference reads */
    if (identity) {
        /* eight columns per thread: one unit, one 16-byte LDS write per plane */
        constexpr int TPL = COLS / 8;                  /* threads per line */
        const int xg = 8 * (tid % TPL), gxi = gx0 + xg;
        uint32_t keep[4];                              /* the lanes of columns inside the picture */
#pragma unroll
        for (int k = 0; k < 4; k++) keep[k] = (gxi + 2 * k < ncols ? 0xFFFFu : 0u) | (gxi + 2 * k + 1 < ncols ? 0xFFFF0000u : 0u);
        for (int l = lo + tid / TPL; l <= hi; l += NT / TPL) {
            sws_u32x4 a = { 0u, 0u, 0u, 0u }, b = { 0u, 0u, 0u, 0u };
            if (keep[0]) p010_unit<NP>(src + (size_t)l * stride, gxi, al4, al16, limit, a, b);
#pragma unroll
            for (int k = 0; k < 4; k++) { a[k] = (a[k] & keep[k]) << UP; b[k] = (b[k] & keep[k]) << UP; }
            if (zero_tail || gxi < ncols) {
                *reinterpret_cast<sws_u32x4 *>(&out_a[l - lo][xg]) = a;
                if (NP > 1) *reinterpret_cast<sws_u32x4 *>(&out_b[l - lo][xg]) = b;
            }
        }
        return;
    }
    const int x = tid & (COLS - 1), gx = gx0 + x, per = NT / COLS;
    const bool col_ok = gx < ncols;
    /* columns past the picture read the last column's entries and do not use them */
    const int gxc = col_ok ? gx : ncols - 1;
    const int pos = posT[gxc];
    const int16_t *f = coefT + (size_t)gxc * fs;
    const int last = imin(gx0 + COLS, ncols) - 1;
    /* the tile's span in samples, from a multiple of eight: whole units; nd: the dwords of its staged line */
    const int s0 = posT[gx0], s1 = posT[last] + fs, a0 = s0 & ~7, nd = span_dwords(2 * a0, 2 * s1);
    uint32_t cp[4];
    if (fs == 8) {
        const uint4 w = *reinterpret_cast<const uint4 *>(f);
        cp[0] = w.x; cp[1] = w.y; cp[2] = w.z; cp[3] = w.w;
    } else {
        int t[8];
#pragma unroll
        for (int j = 0; j < 8; j++) t[j] = f[j < fs ? j : 0];
#pragma unroll
        for (int j = 0; j < 4; j++) cp[j] = (2 * j < fs ? (uint32_t)t[2 * j] & 0xFFFFu : 0u) | (2 * j + 1 < fs ? (uint32_t)t[2 * j + 1] << 16 : 0u);
    }
    if (!(may_stage && span_fits(nd, s0, s1, PITCH))) {
        if (col_ok) {
            for (int l = lo + tid / COLS; l <= hi; l += per) {
                const uint16_t *s = reinterpret_cast<const uint16_t *>(src + (size_t)l * stride) + (size_t)NP * pos;
                int a = 0, b = 0;
                for (int j = 0; j < fs; j++) {
                    a += (int)(s[NP * j] >> 6) * f[j];
                    if (NP > 1) b += (int)(s[NP * j + 1] >> 6) * f[j];
                }
                a >>= HSH; b >>= HSH;
                out_a[l - lo][x] = (int16_t)(a < 32767 ? a : 32767);
                if (NP > 1) out_b[l - lo][x] = (int16_t)(b < 32767 ? b : 32767);
            }
        } else if (zero_tail) {
            for (int l = lo + tid / COLS; l <= hi; l += per) out_a[l - lo][x] = 0;
        }
        return;
    }
    /* units of four staged dwords: 4 * nu <= PITCH (a multiple of four, nd <= PITCH - 2) */
    static_assert(StageGeom<COLS, uint16_t>::LINES * PITCH * PITCH < (1 << 19), "mi355_div20 range");
    const int nu = (nd + 3) >> 2, inv = mi355_inv20(nu);
    uint32_t (*stage)[LR][PITCH] = reinterpret_cast<uint32_t (*)[LR][PITCH]>(stage_mem);      /* [plane][line][dword] */
    for (int base = lo; base <= hi; base += LR) {
        for (int idx = tid; idx < LR * nu; idx += NT) {
            const int r = mi355_div20(idx, inv), u = idx - r * nu, line = base + r;
            if (line > hi) continue;
            sws_u32x4 oa, ob;
            p010_unit<NP>(src + (size_t)line * stride, a0 + 8 * u, al4, al16, limit, oa, ob);
            *reinterpret_cast<sws_u32x4 *>(&stage[0][r][4 * u]) = oa;
            if (NP > 1) *reinterpret_cast<sws_u32x4 *>(&stage[1][r][4 * u]) = ob;
        }
        __syncthreads();
        /* the thread's column over the staged lines of each plane, as hscale_tile; a plane's round is LR lines */
        const int r0 = tid / COLS;
        const int left = uniform(imin(hi - base, LR - 1) - r0);
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const uint8_t *row0 = reinterpret_cast<const uint8_t *>(stage[p][r0]) + 2 * (pos - a0);
            int16_t *out0 = p ? &out_b[base + r0 - lo][x] : &out_a[base + r0 - lo][x];
            if (col_ok) {
                if (fs == 1) hscale_lines<COLS, 1, OP, uint16_t>(row0, out0, cp, left, HSH);
                else if (fs <= 2) hscale_lines<COLS, 2, OP, uint16_t>(row0, out0, cp, left, HSH);
                else if (fs <= 4) hscale_lines<COLS, 4, OP, uint16_t>(row0, out0, cp, left, HSH);
                else if (fs <= 8) hscale_lines8<COLS, OP, uint16_t>(row0, out0, cp, left, HSH);
                else hscale_lines<COLS, 0, OP, uint16_t>(row0, out0, cp, left, HSH, f, fs);
            } else if (zero_tail) {
                for (int k = 0; k < LR / per && k * per <= left; k++) out0[k * per * OP] = 0;
            }
        }
        __syncthreads();
    }
}

/* Vertical pass + LUT for the output rows of a tile with the row's filter taps and source-line indices in
 * registers: NL / NC = luma / chroma tap counts rounded up to 1, 2, 4 or 8 (taps past the real size carry a
 * zero coefficient and a valid line index).  A thread owns one output row and every 16th pair of it. */
/* DST: the destination form (DST_RGB24 / DST_BGR24 / DST_RGB32) — the row offsets of a pair (lut_rows_d), the bytes of a pixel and the store (store8_d,
 * write_pair_d); everything up to the LUT is one text for the three */
/* ALPHA (DST_RGB32): the row's alpha from s_alp — the luma tile's lines and the LUMA taps, in the form of the row's template (output.c:972-985,
 * :1030-1035, :1070-1075) — enters each pixel where 255 goes otherwise */
template <int NL, int NC, bool WIDE, int DST = DST_RGB24, bool ALPHA = false>
__device__ __forceinline__ void vertical_rows(const SwsDev &c, const LutLds &lut, const int16_t (*s_lum)[TW], const int16_t (*s_cu)[TW / 2],
                                              const int16_t (*s_cv)[TW / 2], uint8_t (*s_out)[TW * dst_bpp<DST>()], int tid, int y0, int y1, int llo, int clo,
                                              int npairs, int mode, uint8_t *wide_dst, int dst_stride, int out_row0, const int16_t (*s_alp)[TW] = nullptr)
{
    static_assert(!ALPHA || DST == DST_RGB32, "alpha goes to a 32-bit destination");
    /* out_row0: first tile row of this pass of the narrow form (s_out holds OUT_ROWS rows at a time; nine of a 32-bit destination) */
    constexpr int BPP = dst_bpp<DST>();
    const uint32_t sel = DST == DST_RGB32 ? c.dst_sel : 0u;
    const int row = tid >> 4, gy = y0 + row;
    if (gy > y1 || (!WIDE && (row < out_row0 || row >= out_row0 + out_rows<DST>()))) return;
    const int ls = c.vls, cs = c.vcs;
    const int lfirst = imax(1 - ls, c.vLumP[gy]), cfirst = imax(1 - cs, c.vChrP[gy]);
    /* the taps: every load unconditional (a tap past the filter reads tap 0 and becomes zero), so that they are in flight together */
    int lf[NL], li[NL], cf[NC], ci[NC];
#pragma unroll
    for (int j = 0; j < NL; j++) lf[j] = c.vLumC[(size_t)gy * ls + (j < ls ? j : 0)];
#pragma unroll
    for (int j = 0; j < NC; j++) cf[j] = c.vChrC[(size_t)gy * cs + (j < cs ? j : 0)];
#pragma unroll
    for (int j = 0; j < NL; j++) {
        lf[j] = j < ls ? lf[j] : 0;
        li[j] = clampi(lfirst + (j < ls ? j : 0), 0, c.srcH - 1) - llo;
    }
#pragma unroll
    for (int j = 0; j < NC; j++) {
        cf[j] = j < cs ? cf[j] : 0;
        ci[j] = clampi(cfirst + (j < cs ? j : 0), 0, c.chrSrcH - 1) - clo;
    }
    if (WIDE) {
        /* full tile, 8-byte aligned destination: a thread takes eight neighbouring samples (16 / 8 bytes per LDS read)
         * and stores its 24 RGB bytes directly */
        const int grp = tid & 15;
        int Y[8], U[4], V[4];
        if (mode == 1) {
            const int uvalpha = cs == 1 ? 0 : cf[NC > 1 ? 1 : 0];
            const sws_u32x4 l0 = *reinterpret_cast<const sws_u32x4 *>(&s_lum[li[0]][8 * grp]);
            const sws_u32x2 u0 = *reinterpret_cast<const sws_u32x2 *>(&s_cu[ci[0]][4 * grp]), v0 = *reinterpret_cast<const sws_u32x2 *>(&s_cv[ci[0]][4 * grp]);
            const sws_u32x2 u1 = *reinterpret_cast<const sws_u32x2 *>(&s_cu[ci[NC > 1 ? 1 : 0]][4 * grp]), v1 = *reinterpret_cast<const sws_u32x2 *>(&s_cv[ci[NC > 1 ? 1 : 0]][4 * grp]);
#pragma unroll
            for (int k = 0; k < 8; k++) Y[k] = clip_u8(lane16(l0, k) >> 7);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int a = lane16(u0, k), b = lane16(v0, k);
                const int a1 = lane16(u1, k), b1 = lane16(v1, k);
                if (uvalpha < 2048) { U[k] = clip_u8(a >> 7); V[k] = clip_u8(b >> 7); }
                else { U[k] = clip_u8((a + a1) >> 8); V[k] = clip_u8((b + b1) >> 8); }
            }
        } else if (mode == 2) {
            const int ya = lf[NL > 1 ? 1 : 0], ua = cf[NC > 1 ? 1 : 0], ya1 = 4096 - ya, ua1 = 4096 - ua;
            const sws_u32x4 l0 = *reinterpret_cast<const sws_u32x4 *>(&s_lum[li[0]][8 * grp]), l1 = *reinterpret_cast<const sws_u32x4 *>(&s_lum[li[NL > 1 ? 1 : 0]][8 * grp]);
            const sws_u32x2 u0 = *reinterpret_cast<const sws_u32x2 *>(&s_cu[ci[0]][4 * grp]), v0 = *reinterpret_cast<const sws_u32x2 *>(&s_cv[ci[0]][4 * grp]);
            const sws_u32x2 u1 = *reinterpret_cast<const sws_u32x2 *>(&s_cu[ci[NC > 1 ? 1 : 0]][4 * grp]), v1 = *reinterpret_cast<const sws_u32x2 *>(&s_cv[ci[NC > 1 ? 1 : 0]][4 * grp]);
#pragma unroll
            for (int k = 0; k < 8; k++)
                Y[k] = clip_u8((lane16(l0, k) * ya1 + lane16(l1, k) * ya) >> 19);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                U[k] = clip_u8((lane16(u0, k) * ua1 + lane16(u1, k) * ua) >> 19);
                V[k] = clip_u8((lane16(v0, k) * ua1 + lane16(v1, k) * ua) >> 19);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) Y[k] = 1 << 18;
#pragma unroll
            for (int k = 0; k < 4; k++) U[k] = V[k] = 1 << 18;
            /* two taps at a time: the same sample of two source lines side by side in a dword (one byte-permute) against the
             * tap pair, v_dot2_i32_i16 — the same integer sum as the reference's per-tap multiply-add (15-bit samples,
             * 16-bit coefficients, int accumulators) */
            if (NL >= 2) {
#pragma unroll
                for (int j = 0; j + 1 < NL; j += 2) {
                    const sws_u32x4 la = *reinterpret_cast<const sws_u32x4 *>(&s_lum[li[j]][8 * grp]), lb = *reinterpret_cast<const sws_u32x4 *>(&s_lum[li[j + 1]][8 * grp]);
                    const uint32_t cp = ((uint32_t)lf[j] & 0xFFFFu) | ((uint32_t)lf[j + 1] << 16);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        Y[2 * q] = sws_dot2(sws_lo2(la[q], lb[q]), cp, Y[2 * q]);
                        Y[2 * q + 1] = sws_dot2(sws_hi2(la[q], lb[q]), cp, Y[2 * q + 1]);
                    }
                }
            } else {
                const sws_u32x4 l = *reinterpret_cast<const sws_u32x4 *>(&s_lum[li[0]][8 * grp]);
#pragma unroll
                for (int k = 0; k < 8; k++) Y[k] += lane16(l, k) * lf[0];
            }
            if (NC >= 2) {
#pragma unroll
                for (int j = 0; j + 1 < NC; j += 2) {
                    const sws_u32x2 ua = *reinterpret_cast<const sws_u32x2 *>(&s_cu[ci[j]][4 * grp]), ub = *reinterpret_cast<const sws_u32x2 *>(&s_cu[ci[j + 1]][4 * grp]);
                    const sws_u32x2 va = *reinterpret_cast<const sws_u32x2 *>(&s_cv[ci[j]][4 * grp]), vb = *reinterpret_cast<const sws_u32x2 *>(&s_cv[ci[j + 1]][4 * grp]);
                    const uint32_t cp = ((uint32_t)cf[j] & 0xFFFFu) | ((uint32_t)cf[j + 1] << 16);
#pragma unroll
                    for (int q = 0; q < 2; q++) {
                        U[2 * q] = sws_dot2(sws_lo2(ua[q], ub[q]), cp, U[2 * q]);
                        U[2 * q + 1] = sws_dot2(sws_hi2(ua[q], ub[q]), cp, U[2 * q + 1]);
                        V[2 * q] = sws_dot2(sws_lo2(va[q], vb[q]), cp, V[2 * q]);
                        V[2 * q + 1] = sws_dot2(sws_hi2(va[q], vb[q]), cp, V[2 * q + 1]);
                    }
                }
            } else {
                const sws_u32x2 u = *reinterpret_cast<const sws_u32x2 *>(&s_cu[ci[0]][4 * grp]), v = *reinterpret_cast<const sws_u32x2 *>(&s_cv[ci[0]][4 * grp]);
#pragma unroll
                for (int k = 0; k < 4; k++) { U[k] += lane16(u, k) * cf[0]; V[k] += lane16(v, k) * cf[0]; }
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {       /* clipped per pair, only if one of its four values has bit 8 set (output.c:963) */
                int &Y1 = Y[2 * p], &Y2 = Y[2 * p + 1], &Up = U[p], &Vp = V[p];
                Y1 >>= 19; Y2 >>= 19; Up >>= 19; Vp >>= 19;
                if ((Y1 | Y2 | Up | Vp) & 0x100) { Y1 = clip_u8(Y1); Y2 = clip_u8(Y2); Up = clip_u8(Up); Vp = clip_u8(Vp); }
            }
        }
        int r[4], g[4], b[4];
#pragma unroll
        for (int p = 0; p < 4; p++) lut_rows_d<DST>(lut, U[p], V[p], r[p], g[p], b[p]);
        if constexpr (ALPHA) {
            int A[8];
            if (mode == 1) {
                const sws_u32x4 a0 = *reinterpret_cast<const sws_u32x4 *>(&s_alp[li[0]][8 * grp]);
#pragma unroll
                for (int k = 0; k < 8; k++) A[k] = clip_u8(lane16(a0, k) >> 7);
            } else if (mode == 2) {
                const int ya = lf[NL > 1 ? 1 : 0], ya1 = 4096 - ya;
                const sws_u32x4 a0 = *reinterpret_cast<const sws_u32x4 *>(&s_alp[li[0]][8 * grp]), a1 = *reinterpret_cast<const sws_u32x4 *>(&s_alp[li[NL > 1 ? 1 : 0]][8 * grp]);
#pragma unroll
                for (int k = 0; k < 8; k++) A[k] = clip_u8((lane16(a0, k) * ya1 + lane16(a1, k) * ya) >> 19);
            } else {
#pragma unroll
                for (int k = 0; k < 8; k++) A[k] = 1 << 18;
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const sws_u32x4 a = *reinterpret_cast<const sws_u32x4 *>(&s_alp[li[j]][8 * grp]);
#pragma unroll
                    for (int k = 0; k < 8; k++) A[k] += lane16(a, k) * lf[j];
                }
#pragma unroll
                for (int p = 0; p < 4; p++) {       /* clipped per pair, only if one of its two values has bit 8 set (output.c:981) */
                    int &A1 = A[2 * p], &A2 = A[2 * p + 1];
                    A1 >>= 19; A2 >>= 19;
                    if ((A1 | A2) & 0x100) { A1 = clip_u8(A1); A2 = clip_u8(A2); }
                }
            }
            rgb32_store8_a(lut, wide_dst + (size_t)row * dst_stride + 8 * BPP * grp, Y, A, r, g, b, sel);
        } else
        store8_d<DST>(lut, wide_dst + (size_t)row * dst_stride + 8 * BPP * grp, Y, r, g, b, sel);
        return;
    }
    /* fixed trip count: the pairs of a thread are 16 apart, so every LDS address is one base plus an immediate */
#pragma unroll
    for (int k = 0; k < TW / 32; k++) {
        const int i = (tid & 15) + 16 * k;
        if (i >= npairs) continue;
        int Y1, Y2, U, V;
        if (mode == 1) {          /* yuv2rgb_1_c_template output.c:1043-1110 (ls == 1, cs <= 2) */
            const int uvalpha = cs == 1 ? 0 : cf[NC > 1 ? 1 : 0];
            Y1 = clip_u8(s_lum[li[0]][2 * i] >> 7); Y2 = clip_u8(s_lum[li[0]][2 * i + 1] >> 7);
            if (uvalpha < 2048) { U = clip_u8(s_cu[ci[0]][i] >> 7); V = clip_u8(s_cv[ci[0]][i] >> 7); }
            else { U = clip_u8((s_cu[ci[0]][i] + s_cu[ci[NC > 1 ? 1 : 0]][i]) >> 8); V = clip_u8((s_cv[ci[0]][i] + s_cv[ci[NC > 1 ? 1 : 0]][i]) >> 8); }
        } else if (mode == 2) {   /* yuv2rgb_2_c_template :998-1041 (ls == cs == 2) */
            const int ya = lf[NL > 1 ? 1 : 0], ua = cf[NC > 1 ? 1 : 0], ya1 = 4096 - ya, ua1 = 4096 - ua;
            Y1 = clip_u8((s_lum[li[0]][2 * i] * ya1 + s_lum[li[NL > 1 ? 1 : 0]][2 * i] * ya) >> 19);
            Y2 = clip_u8((s_lum[li[0]][2 * i + 1] * ya1 + s_lum[li[NL > 1 ? 1 : 0]][2 * i + 1] * ya) >> 19);
            U = clip_u8((s_cu[ci[0]][i] * ua1 + s_cu[ci[NC > 1 ? 1 : 0]][i] * ua) >> 19);
            V = clip_u8((s_cv[ci[0]][i] * ua1 + s_cv[ci[NC > 1 ? 1 : 0]][i] * ua) >> 19);
        } else {                  /* yuv2rgb_X_c_template :937-996: clipped only if a value has bit 8 set */
            Y1 = Y2 = U = V = 1 << 18;
#pragma unroll
            for (int j = 0; j < NL; j++) {
                const uint32_t two = *reinterpret_cast<const uint32_t *>(&s_lum[li[j]][2 * i]);
                Y1 += (int16_t)(two & 0xFFFF) * lf[j]; Y2 += (int16_t)(two >> 16) * lf[j];
            }
#pragma unroll
            for (int j = 0; j < NC; j++) { U += s_cu[ci[j]][i] * cf[j]; V += s_cv[ci[j]][i] * cf[j]; }
            Y1 >>= 19; Y2 >>= 19; U >>= 19; V >>= 19;
            if ((Y1 | Y2 | U | V) & 0x100) { Y1 = clip_u8(Y1); Y2 = clip_u8(Y2); U = clip_u8(U); V = clip_u8(V); }
        }
        if constexpr (ALPHA) {
            int A1, A2;
            if (mode == 1) { A1 = clip_u8(s_alp[li[0]][2 * i] >> 7); A2 = clip_u8(s_alp[li[0]][2 * i + 1] >> 7); }
            else if (mode == 2) {
                const int ya = lf[NL > 1 ? 1 : 0], ya1 = 4096 - ya;
                A1 = clip_u8((s_alp[li[0]][2 * i] * ya1 + s_alp[li[NL > 1 ? 1 : 0]][2 * i] * ya) >> 19);
                A2 = clip_u8((s_alp[li[0]][2 * i + 1] * ya1 + s_alp[li[NL > 1 ? 1 : 0]][2 * i + 1] * ya) >> 19);
            } else {
                A1 = A2 = 1 << 18;
#pragma unroll
                for (int j = 0; j < NL; j++) {
                    const uint32_t two = *reinterpret_cast<const uint32_t *>(&s_alp[li[j]][2 * i]);
                    A1 += (int16_t)(two & 0xFFFF) * lf[j]; A2 += (int16_t)(two >> 16) * lf[j];
                }
                A1 >>= 19; A2 >>= 19;
                if ((A1 | A2) & 0x100) { A1 = clip_u8(A1); A2 = clip_u8(A2); }
            }
            write_pair_a(lut, &s_out[row - out_row0][i * 2 * BPP], Y1, Y2, U, V, A1, A2, sel);
        } else
        write_pair_d<DST>(lut, &s_out[row - out_row0][i * 2 * BPP], Y1, Y2, U, V, sel);
    }
}
/* LDS of a workgroup, sized per context (sws_plan): the horizontal pass's results for the source lines a tile needs, the tables, and one
 * block shared by the staging lines (horizontal pass) and the output rows of tiles that cannot store from registers (after it). */
/* alpha: with the alpha tile of an ALPHA instance, as many lines as the luma tile */
/* lut: with the tables (every form but DST_YUY2) */
__host__ __device__ constexpr int sws_lds_bytes(int lum_lines, int chr_lines, int stage = STAGE_BYTES, bool alpha = false, bool lut = true)
{
    return lum_lines * TW * 2 + 2 * chr_lines * (TW / 2) * 2 + (lut ? (int)sizeof(LutLds) : 0) + stage + (alpha ? lum_lines * TW * 2 : 0);
}
/* the waves per SIMD the register allocation of a tile kernel aims at: a CU's 160 KB of LDS hold that many of its workgroups, one wave of
 * each per SIMD */
__host__ __device__ constexpr int sws_waves(int lds_bytes) { return 160 * 1024 / lds_bytes < 8 ? 160 * 1024 / lds_bytes : 8; }

/* tap counts in registers are rounded up to 1 / 2 / 4 / 8 (taps past the real size carry a zero coefficient): the bucket of a size of at most
 * eight.  The ladders of hscale_tile and planar_pass test fs == 1 first: one dispatcher on this bucket for all three was tried and gave
 * another instruction stream.  So did every indirection between the sixteen-case switch on the two buckets and vertical_rows (a function, a
 * lambda, a helper taking the lambda): the switch is written out at its two places */
__host__ __device__ constexpr int tap_bucket(int fs) { return fs <= 1 ? 0 : (fs <= 2 ? 1 : (fs <= 4 ? 2 : 3)); }
/* Tiles that cannot store from registers (the picture's right edge, a destination that is not 8-byte aligned, filters of more than
 * eight taps): the rows go through s_out, OUT_ROWS at a time. */
template <int DST = DST_RGB24, bool ALPHA = false>
__device__ __forceinline__ void vertical_narrow(const SwsDev *cp, const LutLds *lutp, const int16_t (*s_lum)[TW], const int16_t (*s_cu)[TW / 2],
                                                          const int16_t (*s_cv)[TW / 2], uint8_t (*s_out)[TW * dst_bpp<DST>()], uint8_t *tile_dst, int dst_stride,
                                                          int x0, int y0, int y1, int llo, int clo, const int16_t (*s_alp)[TW] = nullptr)
{
    constexpr int BPP = dst_bpp<DST>(), OUT_ROWS = out_rows<DST>();
    const SwsDev c = sws_dev(cp);
    const LutLds &s_lut = *lutp;
    const int tid = threadIdx.x, ls = c.vls, cs = c.vcs, mode = packed_mode(ls, cs);
    const int npairs = imin(TW, c.dstW - x0 + 1) >> 1;     /* (dstW + 1) >> 1 pairs in the picture */
    const int nbytes = imin(TW, c.dstW - x0) * BPP, nrows_all = y1 - y0 + 1;
    const int bl = tap_bucket(ls), bc = tap_bucket(cs);
    for (int r0 = 0; r0 < nrows_all; r0 += OUT_ROWS) {
        if (ls <= 8 && cs <= 8) {
            switch (bl * 4 + bc) {
            case 0: vertical_rows<1, 1, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 1: vertical_rows<1, 2, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 2: vertical_rows<1, 4, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 3: vertical_rows<1, 8, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 4: vertical_rows<2, 1, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 5: vertical_rows<2, 2, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 6: vertical_rows<2, 4, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 7: vertical_rows<2, 8, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 8: vertical_rows<4, 1, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 9: vertical_rows<4, 2, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 10: vertical_rows<4, 4, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 11: vertical_rows<4, 8, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 12: vertical_rows<8, 1, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 13: vertical_rows<8, 2, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            case 14: vertical_rows<8, 4, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            default: vertical_rows<8, 8, false, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, nullptr, dst_stride, r0, s_alp); break;
            }
        } else
        for (int p = tid; p < OUT_ROWS * (TW / 2); p += NT) {
            const int row = r0 + (p >> 6), i = p & 63, gy = y0 + row;
            if (gy > y1 || i >= npairs) continue;
            TileRows R{ s_lum, s_cu, s_cv, imax(1 - ls, c.vLumP[gy]), llo, c.srcH - 1, imax(1 - cs, c.vChrP[gy]), clo, c.chrSrcH - 1 };
            int ya = 0, ua = 0;
            if (mode == 1) ua = cs == 1 ? 0 : c.vChrC[2 * gy + 1];
            else if (mode == 2) { ya = c.vLumC[2 * gy + 1]; ua = c.vChrC[2 * gy + 1]; }
            if constexpr (ALPHA) {
                R.alpT = s_alp;
                rgb_pair<DST, true>(s_lut, &s_out[row - r0][i * 2 * BPP], R, i, mode, c.vLumC + (size_t)gy * ls, ls, c.vChrC + (size_t)gy * cs, cs, ya, ua, c.dst_sel);
            } else
            rgb_pair<DST>(s_lut, &s_out[row - r0][i * 2 * BPP], R, i, mode, c.vLumC + (size_t)gy * ls, ls, c.vChrC + (size_t)gy * cs, cs, ya, ua, c.dst_sel);
        }
        __syncthreads();
        /* rows out: only samples below dstW (for odd dstW the reference also writes the phantom partner of
         * the last sample from uninitialised ring-buffer data; that sample is not reproduced) */
        {
            uint8_t *d0 = tile_dst + (size_t)r0 * dst_stride;
            const int nrows = imin(OUT_ROWS, nrows_all - r0);
            const unsigned al = (unsigned)(uintptr_t)d0 | (unsigned)dst_stride | (unsigned)nbytes;
            /* mi355_div20 below: idx < nrows * n with nrows <= 16 and n <= TW * 3 / 4 = 96: idx * n < 2^18 (32 bits: nrows <= 9, n <= TW = 128: the same bound) */
            if ((al & 15) == 0) {                     /* 16 bytes per thread and store */
                const int n = nbytes >> 4, inv = mi355_inv20(n);
                for (int idx = tid; idx < nrows * n; idx += NT) {
                    const int row = mi355_div20(idx, inv), k = idx - row * n;
                    reinterpret_cast<uint4 *>(d0 + (size_t)row * dst_stride)[k] = reinterpret_cast<const uint4 *>(s_out[row])[k];
                }
            } else if ((al & 3) == 0) {
                const int n = nbytes >> 2, inv = mi355_inv20(n);
                for (int idx = tid; idx < nrows * n; idx += NT) {
                    const int row = mi355_div20(idx, inv), k = idx - row * n;
                    reinterpret_cast<uint32_t *>(d0 + (size_t)row * dst_stride)[k] = reinterpret_cast<const uint32_t *>(s_out[row])[k];
                }
            } else {
                for (int row = 0; row < nrows; row++)
                    for (int k = tid; k < nbytes; k += NT) d0[(size_t)row * dst_stride + k] = s_out[row][k];
            }
        }
        __syncthreads();                           /* the next pass overwrites s_out */
    }
}

/* ---- DST_YUY2: the vertical pass of a packed 4:2:2 destination (yuv2422_1 / _2 / _X_c_template, output.c:469-576) --------------------------------
 * range conversion of the tile's lines between the two passes (lumConvertRange over dstW, chrConvertRange over chrDstW samples, swscale.c:284-285,
 * :334-335): only the samples of the picture — the phantom partner of an odd width's last sample stays the 0 the horizontal pass left (the
 * reference's converters never reach sample dstW of its zero-allocated line) */
__device__ __forceinline__ int range_one(int v, const SwsRangeMap &m);      /* (below, with the planar kernel's range_lines) */
__device__ __forceinline__ void yuy2_range_tile(const SwsDev &c, int16_t (*s_lum)[TW], int16_t (*s_cu)[TW / 2], int16_t (*s_cv)[TW / 2], int nlum, int nchr, int x0, int tid)
{
    const int wl = imin(TW, c.dstW - x0), wc = imin(TW / 2, c.chrDstW - (x0 >> 1));
    for (int i = tid; i < nlum * TW; i += NT) {
        const int l = i / TW, x = i % TW;
        if (x < wl) s_lum[l][x] = (int16_t)range_one(s_lum[l][x], c.rng_l);
    }
    for (int i = tid; i < nchr * (TW / 2); i += NT) {
        const int l = i / (TW / 2), x = i % (TW / 2);
        if (x < wc) { s_cu[l][x] = (int16_t)range_one(s_cu[l][x], c.rng_c); s_cv[l][x] = (int16_t)range_one(s_cv[l][x], c.rng_c); }
    }
}
/* A thread owns one output row of the tile and eight neighbouring samples of it — four groups, 16 bytes: one 16-byte LDS read a luma tap line, one
 * 8-byte read a chroma tap line and plane.  The X form takes two taps at a time (v_dot2_i32_i16 over the same sample of two lines, as
 * vertical_rows; a tap past the filter has a zero coefficient and the last line's index); the taps are read as the loop goes, so any filter size
 * runs here.  A full tile of a row whose pointer and stride are multiples of 16 leaves from registers; every other tile goes through s_out (the
 * staging lines: TW * 2 bytes a row, all MAXTH rows at once) and leaves in 16-byte, 4-byte or single-byte pieces.  The row extent is
 * 4 * ((dstW + 1) >> 1) bytes: the phantom partner of an odd width's last sample is written — 0, the luma tile's zero tail through any of the three
 * forms. */
__device__ __forceinline__ void vertical_yuy2(const SwsDev &c, const int16_t (*s_lum)[TW], const int16_t (*s_cu)[TW / 2], const int16_t (*s_cv)[TW / 2],
                                              uint8_t (*s_out)[TW * 2], int tid, int x0, int y0, int y1, int llo, int clo, uint8_t *tile_dst, int dst_stride)
{
    static_assert(STAGE_BYTES >= MAXTH * TW * 2 && NT / 16 >= MAXTH, "one pass over the rows of a tile");
    const int ls = c.vls, cs = c.vcs, mode = packed_mode(ls, cs);
    const int row = tid >> 4, grp = tid & 15, gy = y0 + row;
    const uint32_t sel = c.dst_sel;
    const bool wide = c.dstW - x0 >= TW && ((reinterpret_cast<uintptr_t>(tile_dst) | (uintptr_t)dst_stride) & 15) == 0;      /* uniform over the workgroup */
    if (gy <= y1) {
        const int lfirst = imax(1 - ls, c.vLumP[gy]), cfirst = imax(1 - cs, c.vChrP[gy]);
        const int16_t *lumF = c.vLumC + (size_t)gy * ls, *chrF = c.vChrC + (size_t)gy * cs;
        auto lline = [&](int j) { return *reinterpret_cast<const sws_u32x4 *>(&s_lum[clampi(lfirst + j, 0, c.srcH - 1) - llo][8 * grp]); };
        auto uline = [&](int j) { return *reinterpret_cast<const sws_u32x2 *>(&s_cu[clampi(cfirst + j, 0, c.chrSrcH - 1) - clo][4 * grp]); };
        auto vline = [&](int j) { return *reinterpret_cast<const sws_u32x2 *>(&s_cv[clampi(cfirst + j, 0, c.chrSrcH - 1) - clo][4 * grp]); };
        int Y[8], U[4], V[4];
        if (mode == 1) {
            const int uvalpha = cs == 1 ? 0 : chrF[1];
            const sws_u32x4 l0 = lline(0);
            const sws_u32x2 u0 = uline(0), v0 = vline(0), u1 = uline(cs - 1), v1 = vline(cs - 1);
#pragma unroll
            for (int k = 0; k < 8; k++) Y[k] = clip_u8(lane16(l0, k) >> 7);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (uvalpha < 2048) { U[k] = clip_u8(lane16(u0, k) >> 7); V[k] = clip_u8(lane16(v0, k) >> 7); }
                else { U[k] = clip_u8((lane16(u0, k) + lane16(u1, k)) >> 8); V[k] = clip_u8((lane16(v0, k) + lane16(v1, k)) >> 8); }
            }
        } else if (mode == 2) {
            const int ya = lumF[1], ua = chrF[1], ya1 = 4096 - ya, ua1 = 4096 - ua;
            const sws_u32x4 l0 = lline(0), l1 = lline(1);
            const sws_u32x2 u0 = uline(0), v0 = vline(0), u1 = uline(1), v1 = vline(1);
#pragma unroll
            for (int k = 0; k < 8; k++) Y[k] = clip_u8((lane16(l0, k) * ya1 + lane16(l1, k) * ya) >> 19);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                U[k] = clip_u8((lane16(u0, k) * ua1 + lane16(u1, k) * ua) >> 19);
                V[k] = clip_u8((lane16(v0, k) * ua1 + lane16(v1, k) * ua) >> 19);
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) Y[k] = 1 << 18;
#pragma unroll
            for (int k = 0; k < 4; k++) U[k] = V[k] = 1 << 18;
            for (int j = 0; j < ls; j += 2) {
                const int j1 = j + 1 < ls ? j + 1 : j;
                const uint32_t cp = ((uint32_t)lumF[j] & 0xFFFFu) | (j + 1 < ls ? (uint32_t)lumF[j1] << 16 : 0u);
                const sws_u32x4 la = lline(j), lb = lline(j1);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    Y[2 * q] = sws_dot2(sws_lo2(la[q], lb[q]), cp, Y[2 * q]);
                    Y[2 * q + 1] = sws_dot2(sws_hi2(la[q], lb[q]), cp, Y[2 * q + 1]);
                }
            }
            for (int j = 0; j < cs; j += 2) {
                const int j1 = j + 1 < cs ? j + 1 : j;
                const uint32_t cp = ((uint32_t)chrF[j] & 0xFFFFu) | (j + 1 < cs ? (uint32_t)chrF[j1] << 16 : 0u);
                const sws_u32x2 ua = uline(j), ub = uline(j1), va = vline(j), vb = vline(j1);
#pragma unroll
                for (int q = 0; q < 2; q++) {
                    U[2 * q] = sws_dot2(sws_lo2(ua[q], ub[q]), cp, U[2 * q]);
                    U[2 * q + 1] = sws_dot2(sws_hi2(ua[q], ub[q]), cp, U[2 * q + 1]);
                    V[2 * q] = sws_dot2(sws_lo2(va[q], vb[q]), cp, V[2 * q]);
                    V[2 * q + 1] = sws_dot2(sws_hi2(va[q], vb[q]), cp, V[2 * q + 1]);
                }
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {       /* clipped per group, only if one of its four values has bit 8 set (output.c:498); else stored as they are */
                int &Y1 = Y[2 * p], &Y2 = Y[2 * p + 1], &Up = U[p], &Vp = V[p];
                Y1 >>= 19; Y2 >>= 19; Up >>= 19; Vp >>= 19;
                if ((Y1 | Y2 | Up | Vp) & 0x100) { Y1 = clip_u8(Y1); Y2 = clip_u8(Y2); Up = clip_u8(Up); Vp = clip_u8(Vp); }
            }
        }
        const sws_u32x4 o = { yuy2_group(Y[0], U[0], Y[1], V[0], sel), yuy2_group(Y[2], U[1], Y[3], V[1], sel), yuy2_group(Y[4], U[2], Y[5], V[2], sel),
                              yuy2_group(Y[6], U[3], Y[7], V[3], sel) };
        if (wide) *reinterpret_cast<sws_u32x4 *>(tile_dst + (size_t)row * dst_stride + 16 * grp) = o;
        else *reinterpret_cast<sws_u32x4 *>(&s_out[row][16 * grp]) = o;
    }
    if (wide) return;
    __syncthreads();
    const int nbytes = 4 * (imin(TW, c.dstW - x0 + 1) >> 1), nrows = y1 - y0 + 1;        /* whole groups: (dstW + 1) >> 1 of them in the picture */
    const unsigned al = (unsigned)(uintptr_t)tile_dst | (unsigned)dst_stride;
    if ((al & 15) == 0 && (nbytes & 15) == 0) {
        const int n = nbytes >> 4;
        for (int idx = tid; idx < nrows * n; idx += NT) {
            const int r = idx / n, k = idx - r * n;
            reinterpret_cast<uint4 *>(tile_dst + (size_t)r * dst_stride)[k] = reinterpret_cast<const uint4 *>(s_out[r])[k];
        }
    } else if ((al & 3) == 0) {
        const int n = nbytes >> 2;
        for (int idx = tid; idx < nrows * n; idx += NT) {
            const int r = idx / n, k = idx - r * n;
            reinterpret_cast<uint32_t *>(tile_dst + (size_t)r * dst_stride)[k] = reinterpret_cast<const uint32_t *>(s_out[r])[k];
        }
    } else {
        for (int r = 0; r < nrows; r++)
            for (int k = tid; k < nbytes; k += NT) tile_dst[(size_t)r * dst_stride + k] = s_out[r][k];
    }
}

/* LCAP / CCAP: a row of GENERIC_SHAPES; WAVES: sws_waves() of the instance's LDS */
/* ST: the source's sample type; the uint16_t instances (9 / 10 bit sources) differ in the horizontal pass and its staging lines only */
/* NV: an NV12 / NV21 source (8 bit) — both chroma tiles from ONE pass over fr.src[1], the plane of pairs (hscale_tile_nv); fr.src[2] is not read.
 * The same LDS, so the same workgroups per CU.  The three-plane instances are the NV false ones, unchanged.
 * RGB: a packed rgb24 / bgr24 source (8 bit) — luma and both chroma tiles from fr.src[0] through the input converters (hscale_tile_rgb);
 * fr.src[1] and fr.src[2] are not read.  The same LDS again. */
/* DST: the destination form — DST_RGB24 (the instances above, unchanged), DST_BGR24 or DST_RGB32 (compiled in sws_packed.hip).  The same LDS: the
 * output rows of the narrow form share the staging lines, nine rows of TW * 4 bytes where rgb24 has twelve of TW * 3.
 * DST_YUY2 (compiled in sws_yuy2dst.hip): yuyv422 / uyvy422 / yvyu422 — the same horizontal pass, then vertical_yuy2; no table in LDS (WAVES follows the
 * smaller tile), and the range conversion of such a context as a run-time branch of this form alone */
template <int LCAP, int CCAP, int WAVES, typename ST = uint8_t, bool NV = false, bool RGB = false, int DST = DST_RGB24>
#ifndef MI355_HIP_EMU_H
__attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
#endif
__global__ void __launch_bounds__(NT) k_sws_generic(const SwsDev *cp, const mi355_sws_frame *frames)
{
    __shared__ __attribute__((aligned(16))) int16_t s_lum[LCAP][TW];
    __shared__ __attribute__((aligned(16))) int16_t s_cu[CCAP][TW / 2], s_cv[CCAP][TW / 2];
    __shared__ LutLds s_lut;
    /* the staging lines of the horizontal pass; the output rows of tiles that cannot store from registers reuse them after it */
    __shared__ __attribute__((aligned(16))) uint8_t s_io[stage_bytes<ST>()];
    constexpr int BPP = dst_bpp<DST>();
    uint8_t (*s_out)[TW * BPP] = reinterpret_cast<uint8_t (*)[TW * BPP]>(s_io);
    /* ALPHA: a 32-bit source whose alpha goes to a 32-bit destination — a fourth tile of the luma tile's lines (sws_lds_bytes(..., true)) */
    constexpr bool ALPHA = std::is_same<ST, SwsPx32A>::value;
    static_assert(!ALPHA || (RGB && DST == DST_RGB32), "alpha is carried from a 32-bit source to a 32-bit destination");
    [[maybe_unused]] int16_t (*s_alp_w)[TW] = nullptr;
    if constexpr (ALPHA) {
        __shared__ __attribute__((aligned(16))) int16_t s_alp_tile[LCAP][TW];
        s_alp_w = s_alp_tile;
    }
    [[maybe_unused]] const int16_t (*const s_alp)[TW] = s_alp_w;
    const SwsDev c = sws_dev(cp);
    mi355_sws_frame fr = frames[blockIdx.z];
    for (int k = 0; k < 3; k++) fr.src[k] = mi355_global(fr.src[k]);
    fr.dst = mi355_global(fr.dst);
    const int tid = threadIdx.x, th = c.th;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * th, y1 = imin(y0 + th, c.dstH) - 1;
    const int ls = c.vls, cs = c.vcs;
    /* source lines this tile needs (swscale.c:459-468 for the first tap, :571-616 for the clamping) */
    const int lfirst0 = imax(1 - ls, c.vLumP[y0]), lfirst1 = imax(1 - ls, c.vLumP[y1]);
    const int cfirst0 = imax(1 - cs, c.vChrP[y0]), cfirst1 = imax(1 - cs, c.vChrP[y1]);
    const int llo = clampi(lfirst0, 0, c.srcH - 1), lhi = clampi(lfirst1 + ls - 1, 0, c.srcH - 1);
    const int clo = clampi(cfirst0, 0, c.chrSrcH - 1), chi = clampi(cfirst1 + cs - 1, 0, c.chrSrcH - 1);
    if constexpr (DST != DST_YUY2)
    lut_load(s_lut, &cp->luts, tid);
    /* horizontal pass: luma (the phantom partner of the last sample of an odd-width picture reads the
     * zero-initialised tail of the reference's line buffer, utils.c:1241-1262), then the chroma planes */
    uint32_t *s_stage = reinterpret_cast<uint32_t *>(s_io);
    if constexpr (std::is_same<ST, SwsPxP010>::value) {
        /* a P010 source: luma from fr.src[0], both chroma tiles from ONE pass over fr.src[1], the plane of pairs; fr.src[2] is not read */
        static_assert(NV && !RGB, "a P010 source is a luma plane and a plane of pairs");
        hscale_tile_p010<TW, TW, 1>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi,
                                    s_stage, tid, true, c.hstage != 0, c.hident_l != 0);
        hscale_tile_p010<TW / 2, TW / 2, 2>(s_cu, s_cv, fr.src[1], fr.src_stride[1], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> 1, c.chrDstW, clo, chi,
                                            s_stage, tid, false, c.hstage != 0, c.hident_c != 0);
    } else
    if constexpr (std::is_same<ST, SwsPxYuy2>::value) {
        /* a packed 4:2:2 source: luma from the pairs, both chroma tiles from ONE pass over the groups of four of the same plane */
        static_assert(RGB && !NV, "packed 4:2:2 sources have one plane");
        const uint32_t lay = (uint32_t)c.src_layout;
        hscale_tile_rgb<TW, TW, 1, 2>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, false, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi,
                                      s_stage, tid, true, c.hstage != 0, c.hident_l != 0, lay);
        hscale_tile_rgb<TW / 2, TW / 2, 2, 2>(s_cu, s_cv, fr.src[0], fr.src_stride[0], c.srcW, c.chrSrcW, true, false, c.hChrP, c.hChrC, c.hcs, x0 >> 1, c.chrDstW, clo, chi,
                                              s_stage, tid, false, c.hstage != 0, c.hident_c != 0, lay);
    } else
    if constexpr (RGB && sizeof(ST) == 4) {
        /* a 32-bit source: the order's two uniform values from the record */
        static_assert(!NV, "packed RGB sources have one plane");
        const bool bgr = sws_src_bgr(c.src_layout), half = c.src_hsub != 0;
        const uint32_t ash = sws_src_ash(c.src_layout);
        if constexpr (ALPHA)
            hscale_tile_rgb<TW, TW, 2, 4, true>(s_lum, s_alp_w, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, bgr, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi,
                                                s_stage, tid, true, c.hstage != 0, c.hident_l != 0, ash);
        else
        hscale_tile_rgb<TW, TW, 1, 4>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, bgr, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi,
                                      s_stage, tid, true, c.hstage != 0, c.hident_l != 0, ash);
        hscale_tile_rgb<TW / 2, TW / 2, 2, 4>(s_cu, s_cv, fr.src[0], fr.src_stride[0], c.srcW, c.chrSrcW, half, bgr, c.hChrP, c.hChrC, c.hcs, x0 >> 1, c.chrDstW, clo, chi,
                                              s_stage, tid, false, c.hstage != 0, c.hident_c != 0, ash);
    } else
    if constexpr (RGB) {
        static_assert(sizeof(ST) == 1 && !NV, "packed RGB sources are 8 bit");
        const bool bgr = c.src_layout == MI355_SWS_SRC_BGR24, half = c.src_hsub != 0;
        hscale_tile_rgb<TW, TW, 1>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, bgr, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi,
                                   s_stage, tid, true, c.hstage != 0, c.hident_l != 0);
        hscale_tile_rgb<TW / 2, TW / 2, 2>(s_cu, s_cv, fr.src[0], fr.src_stride[0], c.srcW, c.chrSrcW, half, bgr, c.hChrP, c.hChrC, c.hcs, x0 >> 1, c.chrDstW, clo, chi,
                                           s_stage, tid, false, c.hstage != 0, c.hident_c != 0);
    } else {
    hscale_tile<TW, TW, ST>(s_lum, fr.src[0], fr.src_stride[0], c.srcW, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi, s_stage, tid, true, c.hstage != 0, c.hident_l != 0, c.depth);
    if constexpr (NV) {
        static_assert(sizeof(ST) == 1, "NV12 / NV21 sources are 8 bit");
        const bool vu = c.src_layout == MI355_SWS_SRC_NV21;         /* the first byte of a pair is V */
        hscale_tile_nv<TW / 2, TW / 2>(vu ? s_cv : s_cu, vu ? s_cu : s_cv, fr.src[1], fr.src_stride[1], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> 1, c.chrDstW, clo, chi,
                                       s_stage, tid, c.hstage != 0, c.hident_c != 0);
    } else {
    hscale_tile<TW / 2, TW / 2, ST>(s_cu, fr.src[1], fr.src_stride[1], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> 1, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0, c.depth);
    hscale_tile<TW / 2, TW / 2, ST>(s_cv, fr.src[2], fr.src_stride[2], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> 1, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0, c.depth);
    }
    }
    __syncthreads();
    if constexpr (DST == DST_YUY2) {
        /* a packed 4:2:2 destination: no table; a context that converts the range (uniform over the grid) does so on the tile's lines first */
        static_assert(!ALPHA, "no alpha in a packed 4:2:2 destination");
        if (c.range) {
            yuy2_range_tile(c, s_lum, s_cu, s_cv, lhi - llo + 1, chi - clo + 1, x0, tid);
            __syncthreads();
        }
        vertical_yuy2(c, s_lum, s_cu, s_cv, s_out, tid, x0, y0, y1, llo, clo, fr.dst + (size_t)y0 * fr.dst_stride + (size_t)x0 * BPP, fr.dst_stride);
        return;
    }
    /* vertical pass + LUT */
    const int mode = packed_mode(ls, cs);
    const int npairs = imin(TW, c.dstW - x0 + 1) >> 1;     /* (dstW + 1) >> 1 pairs in the picture */
    /* full tiles with an 8-byte aligned destination leave straight from registers; the others go through s_out, OUT_ROWS rows at a time
     * (a 32-bit destination: 16-byte aligned, two 16-byte stores a thread) */
    constexpr uintptr_t WIDE_MASK = DST == DST_RGB32 ? 15 : 7;
    uint8_t *const tile_dst = fr.dst + (size_t)y0 * fr.dst_stride + (size_t)x0 * BPP;
    uint8_t *const wide_dst = (ls <= 8 && cs <= 8 && c.dstW - x0 >= TW && ((reinterpret_cast<uintptr_t>(tile_dst) | (uintptr_t)fr.dst_stride) & WIDE_MASK) == 0)
                                  ? tile_dst : nullptr;
    const int bl = tap_bucket(ls), bc = tap_bucket(cs);
    if (wide_dst) {                               /* uniform over the workgroup: every row leaves from registers */
        switch (bl * 4 + bc) {
        case 0: vertical_rows<1, 1, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 1: vertical_rows<1, 2, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 2: vertical_rows<1, 4, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 3: vertical_rows<1, 8, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 4: vertical_rows<2, 1, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 5: vertical_rows<2, 2, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 6: vertical_rows<2, 4, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 7: vertical_rows<2, 8, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 8: vertical_rows<4, 1, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 9: vertical_rows<4, 2, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 10: vertical_rows<4, 4, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 11: vertical_rows<4, 8, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 12: vertical_rows<8, 1, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 13: vertical_rows<8, 2, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        case 14: vertical_rows<8, 4, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        default: vertical_rows<8, 8, true, DST, ALPHA>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, s_alp); break;
        }
        return;
    }
    vertical_narrow<DST, ALPHA>(cp, &s_lut, s_lum, s_cu, s_cv, s_out, tile_dst, fr.dst_stride, x0, y0, y1, llo, clo, s_alp);
}

/* ---- planar destinations: yuv420p -> yuv420p / yuv422p / yuv444p ----------------------------------------------------------
 * The planar branch of swscale() (swscale.c:618-645) for 8-bit samples.  should_dither is 0 for an 8-bit source (:389, :445): every
 * dither value is 64.  A plane whose vertical filter has ONE tap takes yuv2plane1_8_c (output.c:257-266), (s + 64) >> 7 with the
 * coefficient unused; the others yuv2planeX_8_c (:242-255), ((64 << 12) + sum s_j * f_j) >> 19; both clipped to 0..255.
 * A thread takes eight neighbouring samples of one LDS line (one ds_read_b128 per tap) and stores their eight bytes at once.  Sixteen
 * lanes cover one line's 256 bytes, so each 16-lane group of a ds_read_b128 meets every bank once, whichever lines the rows read.
 * NTAP: 1 plane1; 2 / 4 / 8 planeX with the taps in registers (taps past fs carry a zero coefficient); 0 planeX with fs taps read as it goes.
 * GPP: 16-byte groups of a plane's tile row; NP: planes side by side in an LDS line (chroma: U | V). */
/* DITH (a source deeper than 8 bits, should_dither swscale.c:389): the row's eight dither values come from the context's 8x8 table — row
 * y & 7 of the plane's own row counter (dstY for luma, chrDstY for chroma, :553-556), V read three columns on (:636-644); a group starts
 * on a multiple of eight columns, so sample k of a group takes value (k + offset) & 7. */
template <int NTAP, int GPP, int NP, bool DITH = false>
__device__ __forceinline__ void planar_rows(const int16_t *s, int lo, int maxl, const int16_t *vC, const int32_t *vP, int fs, int row0, int nrows,
                                            int gx0, int width, uint8_t *d0, int st0, uint8_t *d1, int st1, int tid, const uint8_t (*dith)[8] = nullptr)
{
    constexpr int G = GPP * NP;                        /* groups per LDS line */
    for (int t = tid; t < nrows * G; t += NT) {
        const int r = t / G, g = t % G, gx = gx0 + 8 * (g % GPP), y = row0 + r;
        if (gx >= width) continue;
        const int first = imax(1 - fs, vP[y]);
        const int16_t *col = s + 8 * g;
        auto line = [&](int j) { return *reinterpret_cast<const sws_u32x4 *>(col + (size_t)(clampi(first + j, 0, maxl) - lo) * (G * 8)); };
        int v[8], dv[8];
        if (DITH) {
            const sws_u32x2 w = *reinterpret_cast<const sws_u32x2 *>(dith[y & 7]);
            uint64_t q = ((uint64_t)w[1] << 32) | w[0];
            if (NP > 1 && g >= GPP) q = (q >> 24) | (q << 40);      /* the V plane: offset 3 */
#pragma unroll
            for (int k = 0; k < 8; k++) dv[k] = (int)((q >> (8 * k)) & 0xFF);
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) dv[k] = 64;
        }
        if (NTAP == 1) {
            const sws_u32x4 a = line(0);
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = (lane16(a, k) + dv[k]) >> 7;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = dv[k] << 12;
            if (NTAP == 0) {
                for (int j = 0; j < fs; j++) {
                    const int f = vC[(size_t)y * fs + j];
                    const sws_u32x4 a = line(j);
#pragma unroll
                    for (int k = 0; k < 8; k++) v[k] += lane16(a, k) * f;
                }
            } else {
                constexpr int N = NTAP > 1 ? NTAP : 2;
                int lf[N];
#pragma unroll
                for (int j = 0; j < N; j++) lf[j] = vC[(size_t)y * fs + (j < fs ? j : 0)];   /* unconditional: in flight together */
                /* two taps at a time: the same sample of two lines side by side in a dword against the tap pair (v_dot2_i32_i16: the
                 * reference's integer sum, as vertical_rows) */
#pragma unroll
                for (int j = 0; j < N; j += 2) {
                    const sws_u32x4 la = line(j < fs ? j : 0), lb = line(j + 1 < fs ? j + 1 : 0);
                    const uint32_t cp = (j < fs ? (uint32_t)lf[j] & 0xFFFFu : 0u) | (j + 1 < fs ? (uint32_t)lf[j + 1] << 16 : 0u);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        v[2 * q] = sws_dot2(sws_lo2(la[q], lb[q]), cp, v[2 * q]);
                        v[2 * q + 1] = sws_dot2(sws_hi2(la[q], lb[q]), cp, v[2 * q + 1]);
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] >>= 19;
        }
        /* the clipped bytes pass sws_opaque before they are packed: left to itself the compiler fuses shift, clip and packing of two of them into
         * v_ashr_pk_u8_i32 and ORs the next two bytes over its destination's upper half as if it were zero — on the device that half kept
         * what the register held before (wrong 7th / 8th samples of a group, depending on the data) */
        uint32_t w0 = 0, w1 = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { w0 |= sws_opaque((uint32_t)clip_u8(v[k])) << (8 * k); w1 |= sws_opaque((uint32_t)clip_u8(v[4 + k])) << (8 * k); }
        const bool second = NP > 1 && g >= GPP;
        uint8_t *d = (second ? d1 : d0) + (size_t)r * (second ? st1 : st0) + gx;
        if (gx + 8 <= width && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
            *reinterpret_cast<sws_u32x2 *>(d) = sws_u32x2{ w0, w1 };
        } else {                                       /* the plane's right edge, or a row that is not 8-byte aligned */
            const int n = imin(8, width - gx);
            for (int k = 0; k < n; k++) d[k] = (uint8_t)((k < 4 ? w0 : w1) >> (8 * (k & 3)));
        }
    }
}
/* the vertical pass of one LDS tile: its tap count rounded up to 1 / 2 / 4 / 8, more from memory */
template <int GPP, int NP, bool DITH = false>
__device__ __forceinline__ void planar_pass(const int16_t *s, int lo, int maxl, const int16_t *vC, const int32_t *vP, int fs, int row0, int nrows,
                                            int gx0, int width, uint8_t *d0, int st0, uint8_t *d1, int st1, int tid, const uint8_t (*dith)[8] = nullptr)
{
    if (fs == 1) planar_rows<1, GPP, NP, DITH>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, dith);
    else if (fs <= 2) planar_rows<2, GPP, NP, DITH>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, dith);
    else if (fs <= 4) planar_rows<4, GPP, NP, DITH>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, dith);
    else if (fs <= 8) planar_rows<8, GPP, NP, DITH>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, dith);
    else planar_rows<0, GPP, NP, DITH>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, dith);
}

/* ---- planar destinations of 9 or 10 bits: yuv420p9le ... yuv444p10le -----------------------------------------------------------
 * yuv2plane1_10_c_template / yuv2planeX_10_c_template (output.c:183-213) on the same int16 lines (a destination of 15 bits or fewer keeps the
 * 15-bit intermediates, swscale.c:733-752): one tap (s + (1 << (14 - bits))) >> (15 - bits), the others ((1 << (26 - bits)) + sum s_j * f_j)
 * >> (27 - bits), both clipped to 0 .. (1 << bits) - 1 and stored as uint16_t, little endian.  No dither, whatever the source's depth.
 * The thread-to-group mapping, the reads and the tap ladder are planar_rows'; rnd / sh: the form's rounding term and shift (uniform, from
 * SwsDev), top: (1 << bits) - 1.  A group's eight samples are four dwords: one 16-byte store where the address is a multiple of 16 and the
 * group lies inside the plane, 2-byte stores at the right edge or on a row that is not so aligned (d0 / d1 and the strides are even). */
template <int NTAP, int GPP, int NP>
__device__ __forceinline__ void planar_rows16(const int16_t *s, int lo, int maxl, const int16_t *vC, const int32_t *vP, int fs, int row0, int nrows,
                                              int gx0, int width, uint8_t *d0, int st0, uint8_t *d1, int st1, int tid, int rnd, int sh, int top)
{
    constexpr int G = GPP * NP;                        /* groups per LDS line */
    for (int t = tid; t < nrows * G; t += NT) {
        const int r = t / G, g = t % G, gx = gx0 + 8 * (g % GPP), y = row0 + r;
        if (gx >= width) continue;
        const int first = imax(1 - fs, vP[y]);
        const int16_t *col = s + 8 * g;
        auto line = [&](int j) { return *reinterpret_cast<const sws_u32x4 *>(col + (size_t)(clampi(first + j, 0, maxl) - lo) * (G * 8)); };
        int v[8];
        if (NTAP == 1) {
            const sws_u32x4 a = line(0);
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = lane16(a, k) + rnd;
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) v[k] = rnd;
            if (NTAP == 0) {
                for (int j = 0; j < fs; j++) {
                    const int f = vC[(size_t)y * fs + j];
                    const sws_u32x4 a = line(j);
#pragma unroll
                    for (int k = 0; k < 8; k++) v[k] += lane16(a, k) * f;
                }
            } else {
                constexpr int N = NTAP > 1 ? NTAP : 2;
                int lf[N];
#pragma unroll
                for (int j = 0; j < N; j++) lf[j] = vC[(size_t)y * fs + (j < fs ? j : 0)];   /* unconditional: in flight together */
#pragma unroll
                for (int j = 0; j < N; j += 2) {
                    const sws_u32x4 la = line(j < fs ? j : 0), lb = line(j + 1 < fs ? j + 1 : 0);
                    const uint32_t cp = (j < fs ? (uint32_t)lf[j] & 0xFFFFu : 0u) | (j + 1 < fs ? (uint32_t)lf[j + 1] << 16 : 0u);
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        v[2 * q] = sws_dot2(sws_lo2(la[q], lb[q]), cp, v[2 * q]);
                        v[2 * q + 1] = sws_dot2(sws_hi2(la[q], lb[q]), cp, v[2 * q + 1]);
                    }
                }
            }
        }
        /* the clipped samples pass sws_opaque before they are packed, as in planar_rows: nothing fuses the clip of one sample with the
         * packing of its neighbour */
        sws_u32x4 o;
#pragma unroll
        for (int q = 0; q < 4; q++)
            o[q] = sws_opaque((uint32_t)clampi(v[2 * q] >> sh, 0, top)) | (sws_opaque((uint32_t)clampi(v[2 * q + 1] >> sh, 0, top)) << 16);
        const bool second = NP > 1 && g >= GPP;
        uint8_t *d = (second ? d1 : d0) + (size_t)r * (second ? st1 : st0) + 2 * gx;
        if (gx + 8 <= width && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
            *reinterpret_cast<sws_u32x4 *>(d) = o;
        } else {                                       /* the plane's right edge, or a row that is not 16-byte aligned */
            const int n = imin(8, width - gx);
            for (int k = 0; k < n; k++) reinterpret_cast<uint16_t *>(d)[k] = (uint16_t)(o[k >> 1] >> (16 * (k & 1)));
        }
    }
}
/* the vertical pass of one LDS tile to a 9- / 10-bit plane: the form's constants, its tap count rounded up as planar_pass does */
template <int GPP, int NP>
__device__ __forceinline__ void planar_pass16(const SwsDev &c, const int16_t *s, int lo, int maxl, const int16_t *vC, const int32_t *vP, int fs, int row0, int nrows,
                                              int gx0, int width, uint8_t *d0, int st0, uint8_t *d1, int st1, int tid)
{
    const int top = (1 << c.dst_bits) - 1;
    if (fs == 1) planar_rows16<1, GPP, NP>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, c.v1_rnd, c.v1_sh, top);
    else if (fs <= 2) planar_rows16<2, GPP, NP>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, c.vx_rnd, c.vx_sh, top);
    else if (fs <= 4) planar_rows16<4, GPP, NP>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, c.vx_rnd, c.vx_sh, top);
    else if (fs <= 8) planar_rows16<8, GPP, NP>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, c.vx_rnd, c.vx_sh, top);
    else planar_rows16<0, GPP, NP>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st0, d1, st1, tid, c.vx_rnd, c.vx_sh, top);
}

/* ---- semi-planar destinations: NV12 / NV21 (yuv2nv12cX_c, output.c:267-301) ------------------------------------------------------
 * The chroma rows of a 4:2:0 destination as ONE plane of U V (NV21: V U) byte pairs.  Always the X form, also for a one-tap bank:
 * ((dither << 12) + sum s_j * f_j) >> 19 with the coefficient — (s + d) >> 7 only while it is 4096.  U takes dither column i & 7, V
 * column (i + 3) & 7 of row chrDstY & 7 (64 everywhere for an 8-bit source).
 * A thread takes group g (eight samples) of U AND group g of V of one row: one ds_read_b128 each per tap, the row's taps for both.  An LDS
 * line is U | V, 2 x 64 samples = 256 bytes = all 64 banks once, so every line starts on bank 0; eight lanes cover a row's U groups (banks
 * 0..31) and its V groups lie 32 banks on.  A 16-lane group of ds_read_b128 is lanes {0-3, 12-15, 20-27} and its like: four quarter rows of
 * four different rows, two of them on the same 16 banks if every lane read U — so the lanes of odd rows read V where the even rows read U and
 * the other way round (the quarter rows of a lane group are two even and two odd rows on different halves: every bank once).  The two planes
 * share their taps, so a lane just accumulates "first read" and "second read" and sorts them out when it packs.
 * NTAP: 2 / 4 / 8 taps in registers (taps past fs carry a zero coefficient; one tap is the two-tap form), 0: fs taps read as it goes. */
template <int NTAP, bool DITH>
__device__ __forceinline__ void semiplanar_rows(const int16_t *s, int lo, int maxl, const int16_t *vC, const int32_t *vP, int fs, int row0, int nrows,
                                                int gx0, int width, uint8_t *d0, int st, int tid, const uint8_t (*dith)[8], bool swap_uv)
{
    constexpr int CW = TW / 2, GPP = CW / 8;           /* samples of a plane's tile row, its groups */
    for (int t = tid; t < nrows * GPP; t += NT) {
        const int r = t / GPP, g = t % GPP, gx = gx0 + 8 * g, y = row0 + r;
        if (gx >= width) continue;
        const int first = imax(1 - fs, vP[y]);
        const bool flip = (r & 1) != 0;                /* this lane reads V first */
        const int16_t *colA = s + 8 * g + (flip ? CW : 0), *colB = s + 8 * g + (flip ? 0 : CW);
        auto off = [&](int j) { return (size_t)(clampi(first + j, 0, maxl) - lo) * (2 * CW); };
        int a[8], b[8];
        if (DITH) {
            const sws_u32x2 w = *reinterpret_cast<const sws_u32x2 *>(dith[y & 7]);
            const uint64_t qu = ((uint64_t)w[1] << 32) | w[0], qv = (qu >> 24) | (qu << 40);      /* V: three columns on */
            const uint64_t qa = flip ? qv : qu, qb = flip ? qu : qv;
#pragma unroll
            for (int k = 0; k < 8; k++) { a[k] = (int)((qa >> (8 * k)) & 0xFF) << 12; b[k] = (int)((qb >> (8 * k)) & 0xFF) << 12; }
        } else {
#pragma unroll
            for (int k = 0; k < 8; k++) a[k] = b[k] = 64 << 12;
        }
        if constexpr (NTAP == 0) {
            for (int j = 0; j < fs; j++) {
                const int f = vC[(size_t)y * fs + j];
                const size_t o = off(j);
                const sws_u32x4 la = *reinterpret_cast<const sws_u32x4 *>(colA + o), lb = *reinterpret_cast<const sws_u32x4 *>(colB + o);
#pragma unroll
                for (int k = 0; k < 8; k++) { a[k] += lane16(la, k) * f; b[k] += lane16(lb, k) * f; }
            }
        } else {
            int lf[NTAP];
#pragma unroll
            for (int j = 0; j < NTAP; j++) lf[j] = vC[(size_t)y * fs + (j < fs ? j : 0)];   /* unconditional: in flight together */
#pragma unroll
            for (int j = 0; j < NTAP; j += 2) {
                const size_t o0 = off(j < fs ? j : 0), o1 = off(j + 1 < fs ? j + 1 : 0);
                const sws_u32x4 a0 = *reinterpret_cast<const sws_u32x4 *>(colA + o0), a1 = *reinterpret_cast<const sws_u32x4 *>(colA + o1);
                const sws_u32x4 b0 = *reinterpret_cast<const sws_u32x4 *>(colB + o0), b1 = *reinterpret_cast<const sws_u32x4 *>(colB + o1);
                const uint32_t cp = (j < fs ? (uint32_t)lf[j] & 0xFFFFu : 0u) | (j + 1 < fs ? (uint32_t)lf[j + 1] << 16 : 0u);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    a[2 * q] = sws_dot2(sws_lo2(a0[q], a1[q]), cp, a[2 * q]);
                    a[2 * q + 1] = sws_dot2(sws_hi2(a0[q], a1[q]), cp, a[2 * q + 1]);
                    b[2 * q] = sws_dot2(sws_lo2(b0[q], b1[q]), cp, b[2 * q]);
                    b[2 * q + 1] = sws_dot2(sws_hi2(b0[q], b1[q]), cp, b[2 * q + 1]);
                }
            }
        }
        /* the clipped bytes pass sws_opaque before they are packed, as in planar_rows (v_ashr_pk_u8_i32) */
        uint32_t wa[2] = { 0, 0 }, wb[2] = { 0, 0 };
#pragma unroll
        for (int k = 0; k < 8; k++) {
            wa[k >> 2] |= sws_opaque((uint32_t)clip_u8(a[k] >> 19)) << (8 * (k & 3));
            wb[k >> 2] |= sws_opaque((uint32_t)clip_u8(b[k] >> 19)) << (8 * (k & 3));
        }
        /* the plane whose byte comes first: U (NV21: V) — the first read on even rows, the second on odd ones */
        const bool a_first = flip == swap_uv;
        const uint32_t p0 = a_first ? wa[0] : wb[0], p1 = a_first ? wa[1] : wb[1], q0 = a_first ? wb[0] : wa[0], q1 = a_first ? wb[1] : wa[1];
        const sws_u32x4 o = { sws_zip_lo(p0, q0), sws_zip_hi(p0, q0), sws_zip_lo(p1, q1), sws_zip_hi(p1, q1) };
        uint8_t *d = d0 + (size_t)r * st + 2 * gx;
        if (gx + 8 <= width && (reinterpret_cast<uintptr_t>(d) & 15) == 0) {
            *reinterpret_cast<sws_u32x4 *>(d) = o;
        } else if (gx + 8 <= width && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
            reinterpret_cast<sws_u32x2 *>(d)[0] = sws_u32x2{ o[0], o[1] };
            reinterpret_cast<sws_u32x2 *>(d)[1] = sws_u32x2{ o[2], o[3] };
        } else {                                       /* the plane's right edge, or a row that is not 8-byte aligned */
            const int n = 2 * imin(8, width - gx);
            for (int k = 0; k < n; k++) d[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
        }
    }
}
template <bool DITH>
__device__ __forceinline__ void semiplanar_pass(const int16_t *s, int lo, int maxl, const int16_t *vC, const int32_t *vP, int fs, int row0, int nrows,
                                                int gx0, int width, uint8_t *d0, int st, int tid, const uint8_t (*dith)[8], bool swap_uv)
{
    if (fs <= 2) semiplanar_rows<2, DITH>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st, tid, dith, swap_uv);
    else if (fs <= 4) semiplanar_rows<4, DITH>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st, tid, dith, swap_uv);
    else if (fs <= 8) semiplanar_rows<8, DITH>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st, tid, dith, swap_uv);
    else semiplanar_rows<0, DITH>(s, lo, maxl, vC, vP, fs, row0, nrows, gx0, width, d0, st, tid, dith, swap_uv);
}

/* LDS of a planar workgroup: the luma lines, the chroma lines (U | V side by side, CW samples each) and the staging lines; no LUT, no output rows */
__host__ __device__ constexpr int sws_planar_lds_bytes(int lum_lines, int chr_lines, int cw, int stage = STAGE_BYTES)
{
    return lum_lines * TW * 2 + chr_lines * 2 * cw * 2 + stage;
}
__host__ __device__ constexpr int sws_planar_waves(int lum_lines, int chr_lines, int cw, int stage = STAGE_BYTES)
{
    return sws_waves(sws_planar_lds_bytes(lum_lines, chr_lines, cw, stage));
}

/* lumConvertRange / chrConvertRange (lumRangeFromJpeg_c, lumRangeToJpeg_c, chrRangeFromJpeg_c, chrRangeToJpeg_c, swscale.c:168-198) of two int16
 * samples of a dword: 32-bit arithmetic, the result stored back as int16 (truncated, as the reference's store).  |v| < 2^15 and the four
 * multipliers are below 2^15: the product is a 24-bit multiply-add */
__device__ __forceinline__ int range_one(int v, const SwsRangeMap &m)
{
    return (__mul24(imin(v, m.cap), m.mul) + m.add) >> m.shift;
}
__device__ __forceinline__ uint32_t range_pair(uint32_t w, const SwsRangeMap &m)
{
    const int a = range_one((int16_t)w, m), b = range_one((int)w >> 16, m);
    return ((uint32_t)a & 0xFFFFu) | ((uint32_t)b << 16);
}
/* ... of `nvec` 16-byte pieces of LDS lines, in place: a pass of its own over the tile's lines between two workgroup barriers */
__device__ __forceinline__ void range_lines(int16_t *lines, int nvec, const SwsRangeMap &m, int tid)
{
    sws_u32x4 *q = reinterpret_cast<sws_u32x4 *>(lines);
    for (int i = tid; i < nvec; i += NT) {
        sws_u32x4 w = q[i];
        for (int k = 0; k < 4; k++) w[k] = range_pair(w[k], m);
        q[i] = w;
    }
}

/* The horizontal pass of a planar workgroup's tile, up to (not including) its barrier: luma lines llo .. lhi into s_lum, the chroma lines the rows
 * cy0 .. cy1 need into s_chr (U | V side by side, CW samples each), by the staging round of the source class (ST / NV / RGB as k_sws_planar's).
 * clo: the first chroma line held, nchr: their count (0: the tile has no chroma row).  This is k_sws_planar's own text up to its barrier, stated
 * again for k_sws_gbrp: with that kernel calling this function instead, 150 of its instances came out with another register allocation
 * (tools/isa_kernel_hash.py), so k_sws_planar keeps its text and a change to either goes to both. */
template <int CW, typename ST, bool NV, bool RGB>
__device__ __forceinline__ void planar_hscale(const SwsDev &c, const mi355_sws_planar_frame &fr, int16_t (*s_lum)[TW], int16_t (*s_chr)[2 * CW], uint32_t *s_stage, int tid,
                                              int x0, int hs, int llo, int lhi, int cy0, int cy1, int &clo, int &nchr)
{
    const int cs = c.vcs;
    if constexpr (std::is_same<ST, SwsPxP010>::value) {
        static_assert(NV && !RGB, "a P010 source is a luma plane and a plane of pairs");
        hscale_tile_p010<TW, TW, 1>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi, s_stage, tid, false,
                                    c.hstage != 0, c.hident_l != 0);
    } else
    if constexpr (std::is_same<ST, SwsPxYuy2>::value) {
        static_assert(RGB && !NV, "packed 4:2:2 sources have one plane");
        hscale_tile_rgb<TW, TW, 1, 2>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, false, c.hLumP, c.hLumC, c.hls, x0, c.dstW,
                                      llo, lhi, s_stage, tid, false, c.hstage != 0, c.hident_l != 0, (uint32_t)c.src_layout);
    } else
    if constexpr (RGB && sizeof(ST) == 4) {
        static_assert(!NV, "packed RGB sources have one plane");
        hscale_tile_rgb<TW, TW, 1, 4>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, sws_src_bgr(c.src_layout), c.hLumP, c.hLumC, c.hls, x0, c.dstW,
                                      llo, lhi, s_stage, tid, false, c.hstage != 0, c.hident_l != 0, sws_src_ash(c.src_layout));
    } else
    if constexpr (RGB) {
        static_assert(sizeof(ST) == 1 && !NV, "packed RGB sources are 8 bit");
        hscale_tile_rgb<TW, TW, 1>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, c.src_layout == MI355_SWS_SRC_BGR24, c.hLumP, c.hLumC, c.hls, x0, c.dstW,
                                   llo, lhi, s_stage, tid, false, c.hstage != 0, c.hident_l != 0);
    } else
    hscale_tile<TW, TW, ST>(s_lum, fr.src[0], fr.src_stride[0], c.srcW, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi, s_stage, tid, false, c.hstage != 0, c.hident_l != 0, c.depth);
    clo = 0; nchr = 0;
    if (cy0 <= cy1) {
        clo = clampi(imax(1 - cs, c.vChrP[cy0]), 0, c.chrSrcH - 1);
        const int chi = clampi(imax(1 - cs, c.vChrP[cy1]) + cs - 1, 0, c.chrSrcH - 1);
        nchr = chi - clo + 1;
        if constexpr (std::is_same<ST, SwsPxP010>::value) {
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            hscale_tile_p010<CW, 2 * CW, 2>(s_u, s_v, fr.src[1], fr.src_stride[1], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false,
                                            c.hstage != 0, c.hident_c != 0);
        } else
        if constexpr (std::is_same<ST, SwsPxYuy2>::value) {
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            hscale_tile_rgb<CW, 2 * CW, 2, 2>(s_u, s_v, fr.src[0], fr.src_stride[0], c.srcW, c.chrSrcW, true, false, c.hChrP, c.hChrC, c.hcs,
                                              x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0, (uint32_t)c.src_layout);
        } else
        if constexpr (RGB && sizeof(ST) == 4) {
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            hscale_tile_rgb<CW, 2 * CW, 2, 4>(s_u, s_v, fr.src[0], fr.src_stride[0], c.srcW, c.chrSrcW, c.src_hsub != 0, sws_src_bgr(c.src_layout), c.hChrP, c.hChrC, c.hcs,
                                              x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0, sws_src_ash(c.src_layout));
        } else
        if constexpr (RGB) {
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            hscale_tile_rgb<CW, 2 * CW, 2>(s_u, s_v, fr.src[0], fr.src_stride[0], c.srcW, c.chrSrcW, c.src_hsub != 0, c.src_layout == MI355_SWS_SRC_BGR24, c.hChrP, c.hChrC, c.hcs,
                                           x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0);
        } else
        if constexpr (NV) {
            static_assert(sizeof(ST) == 1, "NV12 / NV21 sources are 8 bit");
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            const bool vu = c.src_layout == MI355_SWS_SRC_NV21;
            hscale_tile_nv<CW, 2 * CW>(vu ? s_v : s_u, vu ? s_u : s_v, fr.src[1], fr.src_stride[1], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> hs, c.chrDstW, clo, chi,
                                       s_stage, tid, c.hstage != 0, c.hident_c != 0);
        } else {
        hscale_tile<CW, 2 * CW, ST>(s_chr, fr.src[1], fr.src_stride[1], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false,
                                    c.hstage != 0, c.hident_c != 0, c.depth);
        hscale_tile<CW, 2 * CW, ST>(reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]), fr.src[2], fr.src_stride[2], c.chrSrcW, c.hChrP, c.hChrC, c.hcs,
                                    x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0, c.depth);
        }
    }
}

/* One workgroup per output tile of TW luma columns x th luma rows (blockIdx.z: the picture of the batch).  The tile's chroma is CW = TW >> hshift
 * columns and the chroma rows cy with cy << vshift inside the tile's rows (swscale.c:618-645: a chroma row is written with the luma row
 * cy << vshift, chrSkipMask).  Horizontal pass of the source lines the tile needs into LDS (hscale_tile, as k_sws_generic), then the
 * vertical pass from LDS straight to the three planes.  LCAP / CCAP: a row of PLANAR_SHAPES.
 * SEMI: an NV12 / NV21 destination (4:2:0, CW = TW / 2) — the chroma rows go to ONE plane of byte pairs, fr.dst[1] (semiplanar_rows);
 * fr.dst[2] is not used.  The three-plane instances are the SEMI false ones, unchanged.
 * NV: an NV12 / NV21 source, as k_sws_generic's — U | V of an LDS line from one pass over fr.src[1].
 * RGB: a packed rgb24 / bgr24 source, as k_sws_generic's — luma and U | V from fr.src[0].
 * RANGE: a context whose source and destination differ in range — the int16 samples the horizontal pass left in s_lum / s_chr go through
 * c.rng_l / c.rng_c before the vertical pass reads them (range_lines: the direction is the constants, the same for the whole grid).
 * DEEP: a three-plane destination of c.dst_bits = 9 or 10 bits — everything up to the barrier is the source form's code, the vertical pass is
 * planar_pass16 (no dither, 16-bit samples; dst pointers and strides stay bytes).  No SEMI and no RANGE instance is DEEP. */
template <int LCAP, int CCAP, int CW, typename ST = uint8_t, bool SEMI = false, bool NV = false, bool RGB = false, bool RANGE = false, bool DEEP = false>
#ifndef MI355_HIP_EMU_H
__attribute__((amdgpu_waves_per_eu(sws_planar_waves(LCAP, CCAP, CW, stage_bytes<ST>()), sws_planar_waves(LCAP, CCAP, CW, stage_bytes<ST>()))))
#endif
__global__ void __launch_bounds__(NT) k_sws_planar(const SwsDev *cp, const mi355_sws_planar_frame *frames)
{
    constexpr bool DITH = sizeof(ST) == 2;            /* a source deeper than 8 bits dithers its 8-bit planes */
    __shared__ __attribute__((aligned(16))) int16_t s_lum[LCAP][TW];
    __shared__ __attribute__((aligned(16))) int16_t s_chr[CCAP][2 * CW];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[stage_bytes<ST>() / 4];
    const SwsDev c = sws_dev(cp);
    mi355_sws_planar_frame fr = frames[blockIdx.z];
    for (int k = 0; k < 3; k++) { fr.src[k] = mi355_global(fr.src[k]); fr.dst[k] = mi355_global(fr.dst[k]); }
    const int tid = threadIdx.x, th = c.th, hs = c.hshift, vs = c.vshift;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * th, y1 = imin(y0 + th, c.dstH) - 1;
    const int cy0 = (y0 + (1 << vs) - 1) >> vs, cy1 = y1 >> vs;       /* the tile's chroma rows (none: a one-row tile on an odd row of 4:2:0) */
    const int ls = c.vls, cs = c.vcs;
    /* source lines the tile needs (swscale.c:459-468 for the first tap, :571-616 for the clamping) */
    const int llo = clampi(imax(1 - ls, c.vLumP[y0]), 0, c.srcH - 1), lhi = clampi(imax(1 - ls, c.vLumP[y1]) + ls - 1, 0, c.srcH - 1);
    if constexpr (std::is_same<ST, SwsPxP010>::value) {
        static_assert(NV && !RGB, "a P010 source is a luma plane and a plane of pairs");
        hscale_tile_p010<TW, TW, 1>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi, s_stage, tid, false,
                                    c.hstage != 0, c.hident_l != 0);
    } else
    if constexpr (std::is_same<ST, SwsPxYuy2>::value) {
        static_assert(RGB && !NV, "packed 4:2:2 sources have one plane");
        hscale_tile_rgb<TW, TW, 1, 2>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, false, c.hLumP, c.hLumC, c.hls, x0, c.dstW,
                                      llo, lhi, s_stage, tid, false, c.hstage != 0, c.hident_l != 0, (uint32_t)c.src_layout);
    } else
    if constexpr (RGB && sizeof(ST) == 4) {
        static_assert(!NV, "packed RGB sources have one plane");
        hscale_tile_rgb<TW, TW, 1, 4>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, sws_src_bgr(c.src_layout), c.hLumP, c.hLumC, c.hls, x0, c.dstW,
                                      llo, lhi, s_stage, tid, false, c.hstage != 0, c.hident_l != 0, sws_src_ash(c.src_layout));
    } else
    if constexpr (RGB) {
        static_assert(sizeof(ST) == 1 && !NV, "packed RGB sources are 8 bit");
        hscale_tile_rgb<TW, TW, 1>(s_lum, nullptr, fr.src[0], fr.src_stride[0], c.srcW, c.srcW, false, c.src_layout == MI355_SWS_SRC_BGR24, c.hLumP, c.hLumC, c.hls, x0, c.dstW,
                                   llo, lhi, s_stage, tid, false, c.hstage != 0, c.hident_l != 0);
    } else
    hscale_tile<TW, TW, ST>(s_lum, fr.src[0], fr.src_stride[0], c.srcW, c.hLumP, c.hLumC, c.hls, x0, c.dstW, llo, lhi, s_stage, tid, false, c.hstage != 0, c.hident_l != 0, c.depth);
    int clo = 0, nchr = 0;
    if (cy0 <= cy1) {
        clo = clampi(imax(1 - cs, c.vChrP[cy0]), 0, c.chrSrcH - 1);
        const int chi = clampi(imax(1 - cs, c.vChrP[cy1]) + cs - 1, 0, c.chrSrcH - 1);
        nchr = chi - clo + 1;
        if constexpr (std::is_same<ST, SwsPxP010>::value) {
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            hscale_tile_p010<CW, 2 * CW, 2>(s_u, s_v, fr.src[1], fr.src_stride[1], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false,
                                            c.hstage != 0, c.hident_c != 0);
        } else
        if constexpr (std::is_same<ST, SwsPxYuy2>::value) {
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            hscale_tile_rgb<CW, 2 * CW, 2, 2>(s_u, s_v, fr.src[0], fr.src_stride[0], c.srcW, c.chrSrcW, true, false, c.hChrP, c.hChrC, c.hcs,
                                              x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0, (uint32_t)c.src_layout);
        } else
        if constexpr (RGB && sizeof(ST) == 4) {
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            hscale_tile_rgb<CW, 2 * CW, 2, 4>(s_u, s_v, fr.src[0], fr.src_stride[0], c.srcW, c.chrSrcW, c.src_hsub != 0, sws_src_bgr(c.src_layout), c.hChrP, c.hChrC, c.hcs,
                                              x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0, sws_src_ash(c.src_layout));
        } else
        if constexpr (RGB) {
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            hscale_tile_rgb<CW, 2 * CW, 2>(s_u, s_v, fr.src[0], fr.src_stride[0], c.srcW, c.chrSrcW, c.src_hsub != 0, c.src_layout == MI355_SWS_SRC_BGR24, c.hChrP, c.hChrC, c.hcs,
                                           x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0);
        } else
        if constexpr (NV) {
            static_assert(sizeof(ST) == 1, "NV12 / NV21 sources are 8 bit");
            int16_t (*const s_u)[2 * CW] = s_chr, (*const s_v)[2 * CW] = reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]);
            const bool vu = c.src_layout == MI355_SWS_SRC_NV21;
            hscale_tile_nv<CW, 2 * CW>(vu ? s_v : s_u, vu ? s_u : s_v, fr.src[1], fr.src_stride[1], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> hs, c.chrDstW, clo, chi,
                                       s_stage, tid, c.hstage != 0, c.hident_c != 0);
        } else {
        hscale_tile<CW, 2 * CW, ST>(s_chr, fr.src[1], fr.src_stride[1], c.chrSrcW, c.hChrP, c.hChrC, c.hcs, x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false,
                                    c.hstage != 0, c.hident_c != 0, c.depth);
        hscale_tile<CW, 2 * CW, ST>(reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]), fr.src[2], fr.src_stride[2], c.chrSrcW, c.hChrP, c.hChrC, c.hcs,
                                    x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false, c.hstage != 0, c.hident_c != 0, c.depth);
        }
    }
    __syncthreads();
    if constexpr (RANGE) {
        /* whole lines of the tile, the columns past the picture with them (nothing stores what the vertical pass makes of those); the lines are
         * contiguous: TW / 8 and 2 * CW / 8 pieces each */
        range_lines(&s_lum[0][0], (lhi - llo + 1) * (TW / 8), c.rng_l, tid);
        range_lines(&s_chr[0][0], nchr * (2 * CW / 8), c.rng_c, tid);
        __syncthreads();
    }
    if constexpr (DEEP) {
        static_assert(!SEMI && !RANGE, "a deep destination is three planes of one range");
        planar_pass16<TW / 8, 1>(c, &s_lum[0][0], llo, c.srcH - 1, c.vLumC, c.vLumP, ls, y0, y1 - y0 + 1, x0, c.dstW,
                                 fr.dst[0] + (size_t)y0 * fr.dst_stride[0], fr.dst_stride[0], nullptr, 0, tid);
        if (cy0 <= cy1)
            planar_pass16<CW / 8, 2>(c, &s_chr[0][0], clo, c.chrSrcH - 1, c.vChrC, c.vChrP, cs, cy0, cy1 - cy0 + 1, x0 >> hs, c.chrDstW,
                                     fr.dst[1] + (size_t)cy0 * fr.dst_stride[1], fr.dst_stride[1], fr.dst[2] + (size_t)cy0 * fr.dst_stride[2], fr.dst_stride[2], tid);
        return;
    }
    const uint8_t (*dith)[8] = DITH ? mi355_global(cp)->dither : nullptr;
    planar_pass<TW / 8, 1, DITH>(&s_lum[0][0], llo, c.srcH - 1, c.vLumC, c.vLumP, ls, y0, y1 - y0 + 1, x0, c.dstW,
                                 fr.dst[0] + (size_t)y0 * fr.dst_stride[0], fr.dst_stride[0], nullptr, 0, tid, dith);
    if constexpr (SEMI) {
        static_assert(CW == TW / 2, "a semi-planar destination is 4:2:0");
        if (cy0 <= cy1)
            semiplanar_pass<DITH>(&s_chr[0][0], clo, c.chrSrcH - 1, c.vChrC, c.vChrP, cs, cy0, cy1 - cy0 + 1, x0 >> 1, c.chrDstW,
                                  fr.dst[1] + (size_t)cy0 * fr.dst_stride[1], fr.dst_stride[1], tid, dith, c.planar == MI355_SWS_DST_NV21);
        return;
    }
    if (cy0 <= cy1)
        planar_pass<CW / 8, 2, DITH>(&s_chr[0][0], clo, c.chrSrcH - 1, c.vChrC, c.vChrP, cs, cy0, cy1 - cy0 + 1, x0 >> hs, c.chrDstW,
                                     fr.dst[1] + (size_t)cy0 * fr.dst_stride[1], fr.dst_stride[1], fr.dst[2] + (size_t)cy0 * fr.dst_stride[2], fr.dst_stride[2], tid, dith);
}

/* ---- SWS_FAST_BILINEAR contexts: the bank-free horizontal pass and its two tile kernels (compiled in sws_fastbl.hip) ------------------------
 * The reference's hyscale_fast_c / hcscale_fast_c (swscale.c:238-249, :288-301; selected at :733-739 for 8-bit sources) read no filter bank: output
 * sample i of a plane sits at xpos = i * xInc (unsigned 32 bit, 16.16), xx = xpos >> 16, a = (xpos & 0xFFFF) >> 9 (0 .. 127), and is
 *   luma    (src[xx] << 7) + (src[xx + 1] - src[xx]) * a
 *   chroma   src[xx] * (a ^ 127) + src[xx + 1] * a                    (the weights sum to 127)
 * with xInc the context's lumXInc / chrXInc as the reference's init left them — kernel arguments here, never recomputed.  There is no tail fix-up:
 * a column with xx == srcW - 1 reads src[srcW], the byte behind the line in the caller's plane, and with a != 0 that byte is part of the result.  No
 * result reaches the 32767 clip (255 * 128, 255 * 127).
 * A tile's span [xx(gx0), xx(last) + 1] is staged as hscale_tile stages a monotonic bank — aligned 16-byte pieces on a plane of 16-byte multiples
 * (read over the stride), dwords that lie whole inside the span on one of 4-byte multiples — and every thread works out xx and a of its column in
 * registers.  The byte at x = srcW is read on a tile whose last column has xx == srcW - 1 and on no other: a piece that starts at the stride
 * (srcW == stride) is that one byte.  Spans wider than a staged line and planes off 4-byte multiples read byte by byte.  mi355_sws_create_fast_bilinear
 * refuses a plane whose last column has xx > srcW - 1; the min() below keeps such a column inside the same extent all the same.
 * Unlike hscale_tile the 16-byte pieces do NOT travel through registers one round ahead (its fetch16): a round loads, stores to LDS, waits at its
 * barrier and computes.  Where this pass is slower than it should be, that is the first thing to try. */
template <bool CHROMA> __device__ __forceinline__ int fbl_blend(int v0, int v1, int a) { return CHROMA ? v0 * (a ^ 127) + v1 * a : (v0 << 7) + (v1 - v0) * a; }
template <int COLS, int OP, bool CHROMA>
__device__ __forceinline__ void hscale_tile_fbl(int16_t (*out)[OP], const uint8_t *src, int stride, int srcW, uint32_t xinc, int gx0, int ncols, int lo, int hi,
                                                uint32_t *stage_mem, int tid, bool zero_tail)
{
    constexpr int PITCH = StageGeom<COLS>::PITCH, LINES = StageGeom<COLS>::LINES, per = NT / COLS;
    static_assert(LINES % per == 0 && LINES * PITCH * PITCH < (1 << 19), "whole rounds; mi355_div20 range");
    uint32_t (*stage)[PITCH] = reinterpret_cast<uint32_t (*)[PITCH]>(stage_mem);
    const int x = tid & (COLS - 1), gx = gx0 + x;
    const bool col_ok = gx < ncols;
    /* columns past the picture work on the last column's position and store nothing of it */
    const uint32_t xpos = (uint32_t)(col_ok ? gx : ncols - 1) * xinc;
    const int xx = imin((int)(xpos >> 16), srcW - 1), a = (int)((xpos & 0xFFFFu) >> 9);
    const int last = imin(gx0 + COLS, ncols) - 1;
    /* the tile's span in bytes: s1 is one past the last byte the reference reads, srcW + 1 at the most */
    const int s0 = imin((int)(((uint32_t)gx0 * xinc) >> 16), srcW - 1), s1 = imin((int)(((uint32_t)last * xinc) >> 16), srcW - 1) + 2;
    const uintptr_t al = reinterpret_cast<uintptr_t>(src) | (uintptr_t)stride;
    const bool al16 = (al & 15) == 0;
    const int a0 = al16 ? (s0 & ~15) : (s0 & ~3), nd = span_dwords(a0, s1);
    if (!(span_fits(nd, s0, s1, PITCH) && (al & 3) == 0)) {
        for (int l = lo + tid / COLS; l <= hi; l += per) {
            const uint8_t *p = src + (size_t)l * stride + xx;
            if (col_ok) out[l - lo][x] = (int16_t)fbl_blend<CHROMA>(p[0], p[1], a);
            else if (zero_tail) out[l - lo][x] = 0;
        }
        return;
    }
    const int np = al16 ? (nd + 3) >> 2 : nd, inv = mi355_inv20(np);      /* pieces of a staged line */
    for (int base = lo; base <= hi; base += LINES) {
        for (int idx = tid; idx < LINES * np; idx += NT) {
            const int r = mi355_div20(idx, inv), d = idx - r * np, line = base + r;
            if (line > hi) continue;
            const uint8_t *row = src + (size_t)line * stride;
            if (al16) {
                const int off = a0 + 16 * d;
                sws_u32x4 w = { 0u, 0u, 0u, 0u };
                if (off + 16 <= stride) w = *reinterpret_cast<const sws_u32x4 *>(row + off);
                else {
                    /* the piece starts at the stride: srcW == stride, and the span's one byte there is x = srcW */
                    for (int b = 0; b < 16; b++) if (off + b < s1) w[b >> 2] |= (uint32_t)row[off + b] << (8 * (b & 3));
                }
                *reinterpret_cast<sws_u32x4 *>(&stage[r][4 * d]) = w;
            } else {
                const int off = a0 + 4 * d;
                uint32_t w = 0;
                if (off + 4 <= s1) w = *reinterpret_cast<const uint32_t *>(row + off);
                else {
                    for (int b = 0; b < 4; b++) if (off + b < s1) w |= (uint32_t)row[off + b] << (8 * b);
                }
                stage[r][d] = w;
            }
        }
        __syncthreads();
        const int r0 = tid / COLS;
        const uint8_t *p = reinterpret_cast<const uint8_t *>(stage[r0]) + (xx - a0);
        for (int k = 0; k < LINES / per && base + r0 + k * per <= hi; k++) {
            const uint8_t *q = p + k * per * (PITCH * 4);
            if (col_ok) out[base + r0 + k * per - lo][x] = (int16_t)fbl_blend<CHROMA>(q[0], q[1], a);
            else if (zero_tail) out[base + r0 + k * per - lo][x] = 0;
        }
        __syncthreads();
    }
}

/* k_sws_generic's tile (LCAP / CCAP / WAVES / DST as there: an 8-bit three-plane source, no alpha) with the bank-free horizontal pass: the same LDS,
 * the same vertical pass.  lum_inc / chr_inc: the context's lumXInc / chrXInc */
template <int LCAP, int CCAP, int WAVES, int DST = DST_RGB24>
#ifndef MI355_HIP_EMU_H
__attribute__((amdgpu_waves_per_eu(WAVES, WAVES)))
#endif
__global__ void __launch_bounds__(NT) k_sws_fbl_generic(const SwsDev *cp, uint32_t lum_inc, uint32_t chr_inc, const mi355_sws_frame *frames)
{
    __shared__ __attribute__((aligned(16))) int16_t s_lum[LCAP][TW];
    __shared__ __attribute__((aligned(16))) int16_t s_cu[CCAP][TW / 2], s_cv[CCAP][TW / 2];
    __shared__ LutLds s_lut;
    __shared__ __attribute__((aligned(16))) uint8_t s_io[STAGE_BYTES];
    constexpr int BPP = dst_bpp<DST>();
    uint8_t (*s_out)[TW * BPP] = reinterpret_cast<uint8_t (*)[TW * BPP]>(s_io);
    const SwsDev c = sws_dev(cp);
    mi355_sws_frame fr = frames[blockIdx.z];
    for (int k = 0; k < 3; k++) fr.src[k] = mi355_global(fr.src[k]);
    fr.dst = mi355_global(fr.dst);
    const int tid = threadIdx.x, th = c.th;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * th, y1 = imin(y0 + th, c.dstH) - 1;
    const int ls = c.vls, cs = c.vcs;
    const int lfirst0 = imax(1 - ls, c.vLumP[y0]), lfirst1 = imax(1 - ls, c.vLumP[y1]);
    const int cfirst0 = imax(1 - cs, c.vChrP[y0]), cfirst1 = imax(1 - cs, c.vChrP[y1]);
    const int llo = clampi(lfirst0, 0, c.srcH - 1), lhi = clampi(lfirst1 + ls - 1, 0, c.srcH - 1);
    const int clo = clampi(cfirst0, 0, c.chrSrcH - 1), chi = clampi(cfirst1 + cs - 1, 0, c.chrSrcH - 1);
    if constexpr (DST != DST_YUY2) lut_load(s_lut, &cp->luts, tid);
    uint32_t *s_stage = reinterpret_cast<uint32_t *>(s_io);
    hscale_tile_fbl<TW, TW, false>(s_lum, fr.src[0], fr.src_stride[0], c.srcW, lum_inc, x0, c.dstW, llo, lhi, s_stage, tid, true);
    hscale_tile_fbl<TW / 2, TW / 2, true>(s_cu, fr.src[1], fr.src_stride[1], c.chrSrcW, chr_inc, x0 >> 1, c.chrDstW, clo, chi, s_stage, tid, false);
    hscale_tile_fbl<TW / 2, TW / 2, true>(s_cv, fr.src[2], fr.src_stride[2], c.chrSrcW, chr_inc, x0 >> 1, c.chrDstW, clo, chi, s_stage, tid, false);
    __syncthreads();
    if constexpr (DST == DST_YUY2) {
        if (c.range) {
            yuy2_range_tile(c, s_lum, s_cu, s_cv, lhi - llo + 1, chi - clo + 1, x0, tid);
            __syncthreads();
        }
        vertical_yuy2(c, s_lum, s_cu, s_cv, s_out, tid, x0, y0, y1, llo, clo, fr.dst + (size_t)y0 * fr.dst_stride + (size_t)x0 * BPP, fr.dst_stride);
        return;
    }
    /* vertical pass + LUT, as k_sws_generic: full tiles with an aligned destination leave from registers, the others through s_out */
    const int mode = packed_mode(ls, cs);
    const int npairs = imin(TW, c.dstW - x0 + 1) >> 1;
    constexpr uintptr_t WIDE_MASK = DST == DST_RGB32 ? 15 : 7;
    uint8_t *const tile_dst = fr.dst + (size_t)y0 * fr.dst_stride + (size_t)x0 * BPP;
    uint8_t *const wide_dst = (ls <= 8 && cs <= 8 && c.dstW - x0 >= TW && ((reinterpret_cast<uintptr_t>(tile_dst) | (uintptr_t)fr.dst_stride) & WIDE_MASK) == 0)
                                  ? tile_dst : nullptr;
    if (wide_dst) {
#define FBL_ROWS(NL, NC) vertical_rows<NL, NC, true, DST, false>(c, s_lut, s_lum, s_cu, s_cv, s_out, tid, y0, y1, llo, clo, npairs, mode, wide_dst, fr.dst_stride, 0, nullptr)
        switch (tap_bucket(ls) * 4 + tap_bucket(cs)) {
        case 0: FBL_ROWS(1, 1); break;   case 1: FBL_ROWS(1, 2); break;   case 2: FBL_ROWS(1, 4); break;   case 3: FBL_ROWS(1, 8); break;
        case 4: FBL_ROWS(2, 1); break;   case 5: FBL_ROWS(2, 2); break;   case 6: FBL_ROWS(2, 4); break;   case 7: FBL_ROWS(2, 8); break;
        case 8: FBL_ROWS(4, 1); break;   case 9: FBL_ROWS(4, 2); break;   case 10: FBL_ROWS(4, 4); break;  case 11: FBL_ROWS(4, 8); break;
        case 12: FBL_ROWS(8, 1); break;  case 13: FBL_ROWS(8, 2); break;  case 14: FBL_ROWS(8, 4); break;  default: FBL_ROWS(8, 8); break;
        }
#undef FBL_ROWS
        return;
    }
    vertical_narrow<DST, false>(cp, &s_lut, s_lum, s_cu, s_cv, s_out, tile_dst, fr.dst_stride, x0, y0, y1, llo, clo, nullptr);
}

/* k_sws_planar's tile (LCAP / CCAP / CW / SEMI / RANGE / DEEP as there: an 8-bit three-plane source, no dither) with the bank-free horizontal pass */
template <int LCAP, int CCAP, int CW, bool SEMI = false, bool RANGE = false, bool DEEP = false>
#ifndef MI355_HIP_EMU_H
__attribute__((amdgpu_waves_per_eu(sws_planar_waves(LCAP, CCAP, CW), sws_planar_waves(LCAP, CCAP, CW))))
#endif
__global__ void __launch_bounds__(NT) k_sws_fbl_planar(const SwsDev *cp, uint32_t lum_inc, uint32_t chr_inc, const mi355_sws_planar_frame *frames)
{
    __shared__ __attribute__((aligned(16))) int16_t s_lum[LCAP][TW];
    __shared__ __attribute__((aligned(16))) int16_t s_chr[CCAP][2 * CW];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[STAGE_BYTES / 4];
    const SwsDev c = sws_dev(cp);
    mi355_sws_planar_frame fr = frames[blockIdx.z];
    for (int k = 0; k < 3; k++) { fr.src[k] = mi355_global(fr.src[k]); fr.dst[k] = mi355_global(fr.dst[k]); }
    const int tid = threadIdx.x, th = c.th, hs = c.hshift, vs = c.vshift;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * th, y1 = imin(y0 + th, c.dstH) - 1;
    const int cy0 = (y0 + (1 << vs) - 1) >> vs, cy1 = y1 >> vs;
    const int ls = c.vls, cs = c.vcs;
    const int llo = clampi(imax(1 - ls, c.vLumP[y0]), 0, c.srcH - 1), lhi = clampi(imax(1 - ls, c.vLumP[y1]) + ls - 1, 0, c.srcH - 1);
    hscale_tile_fbl<TW, TW, false>(s_lum, fr.src[0], fr.src_stride[0], c.srcW, lum_inc, x0, c.dstW, llo, lhi, s_stage, tid, false);
    int clo = 0, nchr = 0;
    if (cy0 <= cy1) {
        clo = clampi(imax(1 - cs, c.vChrP[cy0]), 0, c.chrSrcH - 1);
        const int chi = clampi(imax(1 - cs, c.vChrP[cy1]) + cs - 1, 0, c.chrSrcH - 1);
        nchr = chi - clo + 1;
        hscale_tile_fbl<CW, 2 * CW, true>(s_chr, fr.src[1], fr.src_stride[1], c.chrSrcW, chr_inc, x0 >> hs, c.chrDstW, clo, chi, s_stage, tid, false);
        hscale_tile_fbl<CW, 2 * CW, true>(reinterpret_cast<int16_t (*)[2 * CW]>(&s_chr[0][CW]), fr.src[2], fr.src_stride[2], c.chrSrcW, chr_inc, x0 >> hs, c.chrDstW,
                                          clo, chi, s_stage, tid, false);
    }
    __syncthreads();
    if constexpr (RANGE) {
        range_lines(&s_lum[0][0], (lhi - llo + 1) * (TW / 8), c.rng_l, tid);
        range_lines(&s_chr[0][0], nchr * (2 * CW / 8), c.rng_c, tid);
        __syncthreads();
    }
    if constexpr (DEEP) {
        static_assert(!SEMI && !RANGE, "a deep destination is three planes of one range");
        planar_pass16<TW / 8, 1>(c, &s_lum[0][0], llo, c.srcH - 1, c.vLumC, c.vLumP, ls, y0, y1 - y0 + 1, x0, c.dstW,
                                 fr.dst[0] + (size_t)y0 * fr.dst_stride[0], fr.dst_stride[0], nullptr, 0, tid);
        if (cy0 <= cy1)
            planar_pass16<CW / 8, 2>(c, &s_chr[0][0], clo, c.chrSrcH - 1, c.vChrC, c.vChrP, cs, cy0, cy1 - cy0 + 1, x0 >> hs, c.chrDstW,
                                     fr.dst[1] + (size_t)cy0 * fr.dst_stride[1], fr.dst_stride[1], fr.dst[2] + (size_t)cy0 * fr.dst_stride[2], fr.dst_stride[2], tid);
        return;
    }
    planar_pass<TW / 8, 1, false>(&s_lum[0][0], llo, c.srcH - 1, c.vLumC, c.vLumP, ls, y0, y1 - y0 + 1, x0, c.dstW,
                                  fr.dst[0] + (size_t)y0 * fr.dst_stride[0], fr.dst_stride[0], nullptr, 0, tid, nullptr);
    if constexpr (SEMI) {
        static_assert(CW == TW / 2, "a semi-planar destination is 4:2:0");
        if (cy0 <= cy1)
            semiplanar_pass<false>(&s_chr[0][0], clo, c.chrSrcH - 1, c.vChrC, c.vChrP, cs, cy0, cy1 - cy0 + 1, x0 >> 1, c.chrDstW,
                                   fr.dst[1] + (size_t)cy0 * fr.dst_stride[1], fr.dst_stride[1], tid, nullptr, c.planar == MI355_SWS_DST_NV21);
        return;
    }
    if (cy0 <= cy1)
        planar_pass<CW / 8, 2, false>(&s_chr[0][0], clo, c.chrSrcH - 1, c.vChrC, c.vChrP, cs, cy0, cy1 - cy0 + 1, x0 >> hs, c.chrDstW,
                                      fr.dst[1] + (size_t)cy0 * fr.dst_stride[1], fr.dst_stride[1], fr.dst[2] + (size_t)cy0 * fr.dst_stride[2], fr.dst_stride[2], tid, nullptr);
}

/* ---- planar RGB destinations: gbrp (compiled in sws_gbrp.hip) -----------------------------------------------------------------------------------
 * The reference's arithmetic yuv -> rgb path, yuv2gbrp_full_X_c (output.c:1275-1355; c->yuv2anyX, swscale.c:683-689).  It forces SWS_FULL_CHR_H_INT
 * for this destination (utils.c:986-994): chroma is filtered to the full width (chrDstW = dstW, the chroma bank indexed by dstY), there is no LUT, no
 * dither and no range step — range and colourspace are the six integers of mi355_sws_rgb_coefs (c->yuv2rgb_*, yuv2rgb.c:735-740), a kernel argument
 * here.  Always the X form, also with one tap: the tap is multiplied by its coefficient.  Per pixel, in 32 bits:
 *   Y = (1 << 9) + sum lum_j * f_j;   U, V = (1 << 9) - (128 << 19) + sum chr_j * f_j;   Y >>= 10; U >>= 10; V >>= 10
 *   Y = (Y - y_offset) * y_coeff + (1 << 21);   R = Y + V * v2r;   G = Y + V * v2g + U * u2g;   B = Y + U * u2b
 *   a sum with bit 30 or 31 set is clipped to 0 .. 2^30 - 1 (av_clip_uintp2(, 30): negative -> 0);   plane 0 = G >> 22, plane 1 = B >> 22, plane 2 = R >> 22
 * The matrix runs in uint32_t: the reference's sums leave int32 on content the format allows (BT.601 limited range, Y = 255 with U = 255: B near
 * 2.24e9) and its compiled code wraps; the clip then reads the wrapped bits.  The reference tests (R | G | B) & 0xC0000000 once and clips all three:
 * clipping a sum without those bits is the identity, so each sum is clipped on its own bits here.
 * The multiplies: both operands fit 24 signed bits whatever the banks — a tap sum is an int32, so a sum >> 10 lies inside +-2^21 and Y - y_offset
 * inside +-(2^21 + 2^22) (mi355_sws_create_gbrp refuses a y_offset of 2^22 or more), and it refuses coefficients of 2^23 or more — so they are __mul24 (v_mul_i32_i24 / v_mad_i32_i24: the low 32
 * bits of the product, which is the wrapped product).  The two kernel guides give no issue rate for either integer multiply on gfx950; the 24-bit
 * form is the one range_one already uses on the same grounds, and it can fold the add that follows. */
__device__ __forceinline__ uint32_t gbrp_clip30(uint32_t v) { return (v & 0xC0000000u) ? ((v >> 31) ? 0u : 0x3FFFFFFFu) : v; }
/* the three bytes of one pixel from its three sums >> 10 */
__device__ __forceinline__ void gbrp_pixel(const mi355_sws_rgb_coefs &k, int y, int u, int v, uint32_t &g, uint32_t &b, uint32_t &r)
{
    const uint32_t Y = (uint32_t)__mul24(y - k.y_offset, k.y_coeff) + (1u << 21);
    r = gbrp_clip30(Y + (uint32_t)__mul24(v, k.v2r)) >> 22;
    g = gbrp_clip30(Y + (uint32_t)__mul24(v, k.v2g) + (uint32_t)__mul24(u, k.u2g)) >> 22;
    b = gbrp_clip30(Y + (uint32_t)__mul24(u, k.u2b)) >> 22;
}
constexpr int GBRP_LUM_SEED = 1 << 9, GBRP_CHR_SEED = (1 << 9) - (128 << 19);
/* eight neighbouring samples of NP planes that lie side by side in an LDS line (`pw` samples apart, `pitch` samples a line) through one row of a
 * vertical bank: seed + sum line_j * f_j, not shifted.  f: the row's fs coefficients; first: its first line, lines clamped to 0 .. maxl as the
 * reference's ring buffer repeats them.  NTAP 2 / 4 / 8: the taps in registers, two at a time through sws_dot2 as planar_rows16 (taps past fs carry a
 * zero coefficient — ONE tap is a pair with a zero, never a shortcut); 0: fs taps read as it goes. */
template <int NTAP, int NP>
__device__ __forceinline__ void gbrp_taps(const int16_t *col, int pitch, int pw, int lo, int maxl, const int16_t *f, int first, int fs, int seed, int (*v)[8])
{
    auto line = [&](int j, int p) { return *reinterpret_cast<const sws_u32x4 *>(col + (size_t)(clampi(first + j, 0, maxl) - lo) * pitch + p * pw); };
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int k = 0; k < 8; k++) v[p][k] = seed;
    if (NTAP == 0) {
        for (int j = 0; j < fs; j++) {
            const int c = f[j];
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const sws_u32x4 a = line(j, p);
#pragma unroll
                for (int k = 0; k < 8; k++) v[p][k] += lane16(a, k) * c;
            }
        }
    } else {
        constexpr int N = NTAP > 1 ? NTAP : 2;
        int lf[N];
#pragma unroll
        for (int j = 0; j < N; j++) lf[j] = f[j < fs ? j : 0];      /* unconditional: in flight together */
#pragma unroll
        for (int j = 0; j < N; j += 2) {
            const uint32_t cp = (j < fs ? (uint32_t)lf[j] & 0xFFFFu : 0u) | (j + 1 < fs ? (uint32_t)lf[j + 1] << 16 : 0u);
#pragma unroll
            for (int p = 0; p < NP; p++) {
                const sws_u32x4 la = line(j < fs ? j : 0, p), lb = line(j + 1 < fs ? j + 1 : 0, p);
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    v[p][2 * q] = sws_dot2(sws_lo2(la[q], lb[q]), cp, v[p][2 * q]);
                    v[p][2 * q + 1] = sws_dot2(sws_hi2(la[q], lb[q]), cp, v[p][2 * q + 1]);
                }
            }
        }
    }
}
/* ... its tap count rounded up to 2 / 4 / 8, more from memory */
template <int NP>
__device__ __forceinline__ void gbrp_bank(const int16_t *col, int pitch, int pw, int lo, int maxl, const int16_t *f, int first, int fs, int seed, int (*v)[8])
{
    if (fs <= 2) gbrp_taps<2, NP>(col, pitch, pw, lo, maxl, f, first, fs, seed, v);
    else if (fs <= 4) gbrp_taps<4, NP>(col, pitch, pw, lo, maxl, f, first, fs, seed, v);
    else if (fs <= 8) gbrp_taps<8, NP>(col, pitch, pw, lo, maxl, f, first, fs, seed, v);
    else gbrp_taps<0, NP>(col, pitch, pw, lo, maxl, f, first, fs, seed, v);
}
/* the vertical pass of a tile to the three planes: a thread takes eight neighbouring columns of a row — Y from s_lum, U | V from the two halves of
 * an s_chr line (one ds_read_b128 per tap and plane; sixteen lanes cover a line's 256 bytes) — and stores eight bytes to each plane at once where
 * the row address is a multiple of 8 and the group lies inside the picture, byte by byte at the right edge or on an unaligned row.  The bytes pass
 * sws_opaque before they are packed, as in planar_rows (v_ashr_pk_u8_i32) */
__device__ __forceinline__ void gbrp_rows(const SwsDev &c, const mi355_sws_rgb_coefs &k, const int16_t *s_lum, const int16_t *s_chr, int llo, int clo, int y0, int nrows,
                                          int x0, uint8_t *const dst[3], const int dst_stride[3], int tid)
{
    constexpr int G = TW / 8;
    const int ls = c.vls, cs = c.vcs;
    for (int t = tid; t < nrows * G; t += NT) {
        const int r = t / G, g = t % G, gx = x0 + 8 * g, y = y0 + r;
        if (gx >= c.dstW) continue;
        int yv[1][8], cv[2][8];
        gbrp_bank<1>(s_lum + 8 * g, TW, 0, llo, c.srcH - 1, c.vLumC + (size_t)y * ls, imax(1 - ls, c.vLumP[y]), ls, GBRP_LUM_SEED, yv);
        gbrp_bank<2>(s_chr + 8 * g, 2 * TW, TW, clo, c.chrSrcH - 1, c.vChrC + (size_t)y * cs, imax(1 - cs, c.vChrP[y]), cs, GBRP_CHR_SEED, cv);
        uint32_t w[3][2] = { { 0, 0 }, { 0, 0 }, { 0, 0 } };
#pragma unroll
        for (int i = 0; i < 8; i++) {
            uint32_t pg, pb, pr;
            gbrp_pixel(k, yv[0][i] >> 10, cv[0][i] >> 10, cv[1][i] >> 10, pg, pb, pr);
            w[0][i >> 2] |= sws_opaque(pg) << (8 * (i & 3));
            w[1][i >> 2] |= sws_opaque(pb) << (8 * (i & 3));
            w[2][i >> 2] |= sws_opaque(pr) << (8 * (i & 3));
        }
#pragma unroll
        for (int p = 0; p < 3; p++) {
            uint8_t *d = dst[p] + (size_t)y * dst_stride[p] + gx;
            if (gx + 8 <= c.dstW && (reinterpret_cast<uintptr_t>(d) & 7) == 0) {
                *reinterpret_cast<sws_u32x2 *>(d) = sws_u32x2{ w[p][0], w[p][1] };
            } else {                                   /* the picture's right edge, or a row that is not 8-byte aligned */
                const int n = imin(8, c.dstW - gx);
                for (int i = 0; i < n; i++) d[i] = (uint8_t)(w[p][i >> 2] >> (8 * (i & 3)));
            }
        }
    }
}

/* k_sws_planar's FULL tile (LCAP / CCAP / ST / NV / RGB as there; CW = TW: the tile of a 4:4:4 destination holds exactly the lines this one needs)
 * up to the barrier — the source class's own staging round, the same LDS and workgroups per CU as the yuv444p twin — then gbrp_rows.  No dither
 * whatever the source's depth, no range step.  k: the context's six coefficients */
template <int LCAP, int CCAP, typename ST = uint8_t, bool NV = false, bool RGB = false>
#ifndef MI355_HIP_EMU_H
__attribute__((amdgpu_waves_per_eu(sws_planar_waves(LCAP, CCAP, TW, stage_bytes<ST>()), sws_planar_waves(LCAP, CCAP, TW, stage_bytes<ST>()))))
#endif
__global__ void __launch_bounds__(NT) k_sws_gbrp(const SwsDev *cp, mi355_sws_rgb_coefs k, const mi355_sws_planar_frame *frames)
{
    __shared__ __attribute__((aligned(16))) int16_t s_lum[LCAP][TW];
    __shared__ __attribute__((aligned(16))) int16_t s_chr[CCAP][2 * TW];
    __shared__ __attribute__((aligned(16))) uint32_t s_stage[stage_bytes<ST>() / 4];
    const SwsDev c = sws_dev(cp);
    mi355_sws_planar_frame fr = frames[blockIdx.z];
    for (int p = 0; p < 3; p++) { fr.src[p] = mi355_global(fr.src[p]); fr.dst[p] = mi355_global(fr.dst[p]); }
    const int tid = threadIdx.x, th = c.th;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * th, y1 = imin(y0 + th, c.dstH) - 1;
    const int ls = c.vls;
    const int llo = clampi(imax(1 - ls, c.vLumP[y0]), 0, c.srcH - 1), lhi = clampi(imax(1 - ls, c.vLumP[y1]) + ls - 1, 0, c.srcH - 1);
    int clo = 0, nchr = 0;
    planar_hscale<TW, ST, NV, RGB>(c, fr, s_lum, s_chr, s_stage, tid, x0, 0, llo, lhi, y0, y1, clo, nchr);      /* every row has chroma: cy = y */
    __syncthreads();
    gbrp_rows(c, k, &s_lum[0][0], &s_chr[0][0], llo, clo, y0, y1 - y0 + 1, x0, fr.dst, fr.dst_stride, tid);
}

/* MI355_SWS_TILE_KERNELS_ONLY (sws_deep.hip): the kernels that are no templates — the packer, the splitter, the line kernels — are sws.hip's
 * alone; a second file would emit a copy of each */
#ifndef MI355_SWS_TILE_KERNELS_ONLY
/* ---- the unscaled packer: 8-bit yuv420p -> NV12 / NV21 at equal size (planarToNv12Wrapper, swscale_unscaled.c:138-156) -------------
 * srcW x srcH luma bytes copied (copyPlane), srcW / 2 pairs on srcH / 2 rows interleaved (interleaveBytes_c, rgb2rgb_template.c:693-709) —
 * both divisions round down: the last pair of an odd width's chroma rows and the last chroma row of an odd height are neither read nor
 * written.  One grid over tiles of PACK_COLS x PACK_ROWS luma samples (blockIdx.z: the picture), luma copy and interleave in the same
 * launch: a thread moves 16 luma bytes of four rows and eight pairs of two chroma rows, every load requested before the first store.
 * 16-byte luma pieces where the two luma planes' pointers and strides are multiples of 16, and 8 + 8 -> 16 byte chroma pieces where the
 * source chroma planes are on 8-byte and the pair plane on 16-byte multiples; otherwise sample by sample. */
constexpr int PACK_COLS = 1024, PACK_ROWS = 16;
__global__ void __launch_bounds__(NT) k_sws_nv12_pack(int srcW, int srcH, int swap_uv, const mi355_sws_planar_frame *frames)
{
    mi355_sws_planar_frame fr = frames[blockIdx.z];
    for (int k = 0; k < 3; k++) fr.src[k] = mi355_global(fr.src[k]);
    fr.dst[0] = mi355_global(fr.dst[0]); fr.dst[1] = mi355_global(fr.dst[1]);
    const int tid = threadIdx.x, lane = tid & 63, rg = tid >> 6;
    const int x = blockIdx.x * PACK_COLS + 16 * lane, y0 = blockIdx.y * PACK_ROWS;
    const int cw = srcW >> 1, ch = srcH >> 1, cx = x >> 1, cy0 = y0 >> 1;                     /* pairs, chroma rows: rounded down */
    const uint8_t *first = swap_uv ? fr.src[2] : fr.src[1], *second = swap_uv ? fr.src[1] : fr.src[2];
    const int st_first = swap_uv ? fr.src_stride[2] : fr.src_stride[1], st_second = swap_uv ? fr.src_stride[1] : fr.src_stride[2];
    const bool lwide = x + 16 <= srcW &&
                       ((reinterpret_cast<uintptr_t>(fr.src[0]) | (uintptr_t)fr.src_stride[0] | reinterpret_cast<uintptr_t>(fr.dst[0]) | (uintptr_t)fr.dst_stride[0]) & 15) == 0;
    const bool cwide = cx + 8 <= cw && ((reinterpret_cast<uintptr_t>(fr.dst[1]) | (uintptr_t)fr.dst_stride[1]) & 15) == 0 &&
                       ((reinterpret_cast<uintptr_t>(first) | (uintptr_t)st_first | reinterpret_cast<uintptr_t>(second) | (uintptr_t)st_second) & 7) == 0;
    constexpr int LR = PACK_ROWS / (NT / 64), CR = PACK_ROWS / 2 / (NT / 64);                 /* luma / chroma rows of a thread */
    sws_u32x4 l[LR] = {};
    sws_u32x2 p[CR] = {}, q[CR] = {};
#pragma unroll
    for (int k = 0; k < LR; k++) {
        const int y = y0 + rg + k * (NT / 64);
        if (lwide && y < srcH) l[k] = *reinterpret_cast<const sws_u32x4 *>(fr.src[0] + (size_t)y * fr.src_stride[0] + x);
    }
#pragma unroll
    for (int k = 0; k < CR; k++) {
        const int cy = cy0 + rg + k * (NT / 64);
        if (cwide && cy < ch) {
            p[k] = *reinterpret_cast<const sws_u32x2 *>(first + (size_t)cy * st_first + cx);
            q[k] = *reinterpret_cast<const sws_u32x2 *>(second + (size_t)cy * st_second + cx);
        }
    }
#pragma unroll
    for (int k = 0; k < LR; k++) {
        const int y = y0 + rg + k * (NT / 64);
        if (y >= srcH || x >= srcW) continue;
        uint8_t *d = fr.dst[0] + (size_t)y * fr.dst_stride[0] + x;
        if (lwide) *reinterpret_cast<sws_u32x4 *>(d) = l[k];
        else {
            const uint8_t *sp = fr.src[0] + (size_t)y * fr.src_stride[0] + x;
            const int n = imin(16, srcW - x);
            for (int i = 0; i < n; i++) d[i] = sp[i];
        }
    }
#pragma unroll
    for (int k = 0; k < CR; k++) {
        const int cy = cy0 + rg + k * (NT / 64);
        if (cy >= ch || cx >= cw) continue;
        uint8_t *d = fr.dst[1] + (size_t)cy * fr.dst_stride[1] + 2 * cx;
        if (cwide) {
            *reinterpret_cast<sws_u32x4 *>(d) = sws_u32x4{ sws_zip_lo(p[k][0], q[k][0]), sws_zip_hi(p[k][0], q[k][0]), sws_zip_lo(p[k][1], q[k][1]), sws_zip_hi(p[k][1], q[k][1]) };
        } else {
            const uint8_t *s1 = first + (size_t)cy * st_first + cx, *s2 = second + (size_t)cy * st_second + cx;
            const int n = imin(8, cw - cx);
            for (int i = 0; i < n; i++) { d[2 * i] = s1[i]; d[2 * i + 1] = s2[i]; }
        }
    }
}

/* ---- the unscaled splitter: 8-bit NV12 / NV21 -> yuv420p at equal size (nv12ToPlanarWrapper, swscale_unscaled.c:158-177) -------------
 * The packer's mirror: srcW x srcH luma bytes copied, srcW / 2 pairs on srcH / 2 rows de-interleaved (deinterleaveBytes), both rounded
 * down — the last byte of an odd width's chroma rows and the last chroma row of an odd height are neither read nor written.  The same
 * tile and launch shape, every load requested before the first store.  A 16-byte piece of pairs becomes two 8-byte stores where the pair
 * plane is on 16-byte and both destination chroma planes on 8-byte multiples; otherwise sample by sample.  swap_uv (NV21): the first byte
 * of a pair goes to dst[2]. */
__global__ void __launch_bounds__(NT) k_sws_nv12_split(int srcW, int srcH, int swap_uv, const mi355_sws_planar_frame *frames)
{
    mi355_sws_planar_frame fr = frames[blockIdx.z];
    fr.src[0] = mi355_global(fr.src[0]); fr.src[1] = mi355_global(fr.src[1]);
    for (int k = 0; k < 3; k++) fr.dst[k] = mi355_global(fr.dst[k]);
    const int tid = threadIdx.x, lane = tid & 63, rg = tid >> 6;
    const int x = blockIdx.x * PACK_COLS + 16 * lane, y0 = blockIdx.y * PACK_ROWS;
    const int cw = srcW >> 1, ch = srcH >> 1, cx = x >> 1, cy0 = y0 >> 1;                     /* pairs, chroma rows: rounded down */
    uint8_t *first = swap_uv ? fr.dst[2] : fr.dst[1], *second = swap_uv ? fr.dst[1] : fr.dst[2];
    const int st_first = swap_uv ? fr.dst_stride[2] : fr.dst_stride[1], st_second = swap_uv ? fr.dst_stride[1] : fr.dst_stride[2];
    const bool lwide = x + 16 <= srcW &&
                       ((reinterpret_cast<uintptr_t>(fr.src[0]) | (uintptr_t)fr.src_stride[0] | reinterpret_cast<uintptr_t>(fr.dst[0]) | (uintptr_t)fr.dst_stride[0]) & 15) == 0;
    const bool cwide = cx + 8 <= cw && ((reinterpret_cast<uintptr_t>(fr.src[1]) | (uintptr_t)fr.src_stride[1]) & 15) == 0 &&
                       ((reinterpret_cast<uintptr_t>(first) | (uintptr_t)st_first | reinterpret_cast<uintptr_t>(second) | (uintptr_t)st_second) & 7) == 0;
    constexpr int LR = PACK_ROWS / (NT / 64), CR = PACK_ROWS / 2 / (NT / 64);                 /* luma / chroma rows of a thread */
    sws_u32x4 l[LR] = {}, p[CR] = {};
#pragma unroll
    for (int k = 0; k < LR; k++) {
        const int y = y0 + rg + k * (NT / 64);
        if (lwide && y < srcH) l[k] = *reinterpret_cast<const sws_u32x4 *>(fr.src[0] + (size_t)y * fr.src_stride[0] + x);
    }
#pragma unroll
    for (int k = 0; k < CR; k++) {
        const int cy = cy0 + rg + k * (NT / 64);
        if (cwide && cy < ch) p[k] = *reinterpret_cast<const sws_u32x4 *>(fr.src[1] + (size_t)cy * fr.src_stride[1] + 2 * cx);
    }
#pragma unroll
    for (int k = 0; k < LR; k++) {
        const int y = y0 + rg + k * (NT / 64);
        if (y >= srcH || x >= srcW) continue;
        uint8_t *d = fr.dst[0] + (size_t)y * fr.dst_stride[0] + x;
        if (lwide) *reinterpret_cast<sws_u32x4 *>(d) = l[k];
        else {
            const uint8_t *sp = fr.src[0] + (size_t)y * fr.src_stride[0] + x;
            const int n = imin(16, srcW - x);
            for (int i = 0; i < n; i++) d[i] = sp[i];
        }
    }
#pragma unroll
    for (int k = 0; k < CR; k++) {
        const int cy = cy0 + rg + k * (NT / 64);
        if (cy >= ch || cx >= cw) continue;
        uint8_t *d1 = first + (size_t)cy * st_first + cx, *d2 = second + (size_t)cy * st_second + cx;
        if (cwide) {
            *reinterpret_cast<sws_u32x2 *>(d1) = sws_u32x2{ sws_even4(p[k][0], p[k][1]), sws_even4(p[k][2], p[k][3]) };
            *reinterpret_cast<sws_u32x2 *>(d2) = sws_u32x2{ sws_odd4(p[k][0], p[k][1]), sws_odd4(p[k][2], p[k][3]) };
        } else {
            const uint8_t *sp = fr.src[1] + (size_t)cy * fr.src_stride[1] + 2 * cx;
            const int n = imin(8, cw - cx);
            for (int i = 0; i < n; i++) { d1[i] = sp[2 * i]; d2[i] = sp[2 * i + 1]; }
        }
    }
}
#endif

constexpr int C24_ROWS = 16, C24_COLS = 512, IDENT_ROWS = 16;      /* rows of a tile of k_sws_c24 / of k_sws_ident1 */
/* eight samples of one line: Y bytes in (y0, y1), the four pairs' LUT row offsets in r/g/b -> 24 RGB bytes */
__device__ __forceinline__ void c24_line(const LutLds &t, uint8_t *d, uint32_t y0, uint32_t y1, const int *r, const int *g, const int *b)
{
    int Y[8];
#pragma unroll
    for (int k = 0; k < 8; k++) Y[k] = ((k < 4 ? y0 : y1) >> (8 * (k & 3))) & 0xFF;
    rgb24_store8(t, d, Y, r, g, b);
}
template <int DST> __device__ __forceinline__ void c24_line_d(const LutLds &t, uint8_t *d, uint32_t y0, uint32_t y1, const int *r, const int *g, const int *b, uint32_t sel)
{
    if constexpr (DST == DST_RGB32) {
        int Y[8];
#pragma unroll
        for (int k = 0; k < 8; k++) Y[k] = ((k < 4 ? y0 : y1) >> (8 * (k & 3))) & 0xFF;
        rgb32_store8(t, d, Y, r, g, b, sel);
    } else c24_line(t, d, y0, y1, r, g, b);
}
/* yuv2rgb_c_24_rgb (yuv2rgb.c:335-363): a block converts a 512 x 16 sample tile; a thread takes eight samples of two
 * lines per step (8-byte luma loads, 4-byte chroma loads, three 8-byte stores per line) — one (U,V) pair serves both
 * lines (LOADCHROMA :67-72, nearest chroma).  Unaligned planes and the right edge go pair by pair. */
/* CS 1: an 8-bit yuv422p source — the reference doubles the chroma strides and so reads every other chroma line (yuv2rgb.c:133-136): line
 * (y >> 1) << 1 at the frame's own stride */
/* DST: the destination form — DST_BGR24: yuv2rgb_c_24_bgr (yuv2rgb.c:366-394), DST_RGB32: yuv2rgb_c_32 (:237-265), a thread's eight samples of a line
 * two 16-byte stores.  The kernel has no context record, so the 32-bit form takes the order's byte selector beside the slice's first row: its fourth
 * argument is a C24Slice (the 24-bit forms keep the int) */
struct C24Slice { int y; uint32_t sel; };
template <int DST> struct C24Arg { typedef int type; };
template <> struct C24Arg<DST_RGB32> { typedef C24Slice type; };
__host__ __device__ __forceinline__ int c24_slice_y(int a) { return a; }
__host__ __device__ __forceinline__ int c24_slice_y(const C24Slice &a) { return a.y; }
__host__ __device__ __forceinline__ uint32_t c24_slice_sel(int) { return 0; }
__host__ __device__ __forceinline__ uint32_t c24_slice_sel(const C24Slice &a) { return a.sel; }
template <int CS = 0, int DST = DST_RGB24>
__global__ void __launch_bounds__(NT) k_sws_c24(const mi355_sws_luts *luts, int dstW, int sliceH, typename C24Arg<DST>::type slice, const mi355_sws_frame *frames)
{
    __shared__ LutLds s_lut;
    constexpr int BPP = dst_bpp<DST>();
    constexpr uintptr_t WIDE_MASK = DST == DST_RGB32 ? 15 : 7;       /* of the destination: 16-byte stores; the 24-bit forms 8-byte ones */
    const int sliceY = c24_slice_y(slice);
    const uint32_t sel = c24_slice_sel(slice);
    const int tid = threadIdx.x;
    /* the frame fix-up and the coordinate / mine / wide lines are k_sws_ident1's too: a helper for either was tried and gave another
     * instruction stream of both kernels */
    mi355_sws_frame fr = frames[blockIdx.z];
    for (int k = 0; k < 3; k++) fr.src[k] = mi355_global(fr.src[k]);
    fr.dst = mi355_global(fr.dst);
    const int x = blockIdx.x * C24_COLS + (tid & 63) * 8;   /* first of the thread's eight samples */
    const int npairs = dstW >> 1;                            /* pairs i < dstW >> 1 (8 + 4 + 2 sample groups, yuv2rgb.c:129-171) */
    const bool mine = (x >> 1) < npairs;
    const bool wide = mine && (x >> 1) + 4 <= npairs &&
                      ((reinterpret_cast<uintptr_t>(fr.src[0]) | (uintptr_t)fr.src_stride[0] | reinterpret_cast<uintptr_t>(fr.dst) | (uintptr_t)fr.dst_stride) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(fr.src[1]) | (uintptr_t)fr.src_stride[1] | reinterpret_cast<uintptr_t>(fr.src[2]) | (uintptr_t)fr.src_stride[2]) & 3) == 0 &&
                      (WIDE_MASK == 7 || ((reinterpret_cast<uintptr_t>(fr.dst) | (uintptr_t)fr.dst_stride) & WIDE_MASK) == 0);
    /* the samples of both of the thread's line pairs are requested before the LUT copy below: the block pays one memory
     * round trip, not three (LUT, first pair, second pair) */
    constexpr int NR = C24_ROWS / 2 / (NT / 64);
    sws_u32x2 ya[NR], yc[NR];
    uint32_t u4[NR], v4[NR];
#pragma unroll
    for (int q = 0; q < NR; q++) {
        const int y = blockIdx.y * C24_ROWS + 2 * ((tid >> 6) + q * (NT / 64));
        ya[q] = yc[q] = sws_u32x2{ 0u, 0u }; u4[q] = v4[q] = 0;
        if (wide && y < sliceH) {
            const uint8_t *py1 = fr.src[0] + (size_t)y * fr.src_stride[0] + x;
            ya[q] = *reinterpret_cast<const sws_u32x2 *>(py1); yc[q] = *reinterpret_cast<const sws_u32x2 *>(py1 + fr.src_stride[0]);
            u4[q] = *reinterpret_cast<const uint32_t *>(fr.src[1] + (size_t)((y >> 1) << CS) * fr.src_stride[1] + (x >> 1));
            v4[q] = *reinterpret_cast<const uint32_t *>(fr.src[2] + (size_t)((y >> 1) << CS) * fr.src_stride[2] + (x >> 1));
        }
    }
    MI355_ISSUE_FENCE();
    lut_load(s_lut, luts, tid);
    __syncthreads();
    if (!mine) return;
#pragma unroll
    for (int q = 0; q < NR; q++) {
        const int rr = (tid >> 6) + q * (NT / 64);
        const int y = blockIdx.y * C24_ROWS + 2 * rr;
        if (y >= sliceH) break;
        const uint8_t *py1 = fr.src[0] + (size_t)y * fr.src_stride[0] + x, *py2 = py1 + fr.src_stride[0];
        const uint8_t *pu = fr.src[1] + (size_t)((y >> 1) << CS) * fr.src_stride[1] + (x >> 1), *pv = fr.src[2] + (size_t)((y >> 1) << CS) * fr.src_stride[2] + (x >> 1);
        uint8_t *d1 = fr.dst + (size_t)(y + sliceY) * fr.dst_stride + (size_t)x * BPP, *d2 = d1 + fr.dst_stride;
        if (wide) {
            const sws_u32x2 a = ya[q], c = yc[q];
            int r[4], g[4], b[4];
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int U = (u4[q] >> (8 * p)) & 0xFF, V = (v4[q] >> (8 * p)) & 0xFF;
                lut_rows_d<DST>(s_lut, U, V, r[p], g[p], b[p]);
            }
            c24_line_d<DST>(s_lut, d1, a[0], a[1], r, g, b, sel);
            c24_line_d<DST>(s_lut, d2, c[0], c[1], r, g, b, sel);
        } else {
            for (int p = 0; p < 4 && (x >> 1) + p < npairs; p++) {
                write_pair_d<DST>(s_lut, d1 + 2 * BPP * p, py1[2 * p], py1[2 * p + 1], pu[p], pv[p], sel);
                write_pair_d<DST>(s_lut, d2 + 2 * BPP * p, py2[2 * p], py2[2 * p + 1], pu[p], pv[p], sel);
            }
        }
    }
}

/* The generic scaler on a context that does not scale (round 6): identity horizontal filters (hident_l / hident_c) and ONE vertical luma tap — what swscale() runs for an
 * unscaled yuv420p -> rgb24 conversion that may not take the special converter (SWS_ACCURATE_RND): hScale8To15 is src << 7, and the vertical pass reads those 15-bit values of
 * one luma line and of the row's one to four chroma lines (bicubic: four taps on the chroma planes' half height).  The same integers k_sws_generic computes through its LDS tile
 * (vertical_rows), straight from the source bytes to the LUT:
 *   X false, yuv2rgb24_1_c (output.c:1043-1110; vChrFilterSize <= 2): Y = (src << 7) >> 7, U / V = the first chroma line's sample, or ((c0 << 7) + (c1 << 7)) >> 8 = the mean of
 *     the two lines when the row's second coefficient is >= 2048;
 *   X true, yuv2rgb24_X_c (:937-996; three or four chroma taps): Y = ((1 << 18) + (src << 7) * lumFilter[0]) >> 19, U / V = ((1 << 18) + sum (c_j << 7) * chrFilter[j]) >> 19,
 *     a pair's four values clipped only if one of them has bit 8 set.
 * 512 x 16 sample tiles, a thread eight samples of a line per step; the rows' table entries, then all the samples of a thread are requested before the LUT copy (two round
 * trips per workgroup instead of the tile's staging rounds and barriers).  Only for even dstW (the phantom partner of an odd width's last sample stays with k_sws_generic). */
/* NV: an NV12 / NV21 source — per tap line one 8-byte load of four pairs from fr.src[1] in place of the two 4-byte loads, U and V out of it with
 * one permute each; the wide form asks the pair plane for 8-byte multiples; fr.src[2] is not read */
/* DST: the destination form, as k_sws_generic's (the selector of a 32-bit order from the record; its wide form asks the destination for 16-byte multiples) */
/* DST_YUY2: a thread's eight samples are four groups, 16 bytes — the pair's Y1, Y2, U, V of either form straight into the group, no table and no barrier;
 * the wide form asks the destination for 16-byte multiples, ragged rows leave group by group in bytes */
template <bool X, bool NV = false, int DST = DST_RGB24>
__global__ void __launch_bounds__(NT) k_sws_ident1(const SwsDev *cp, const mi355_sws_frame *frames)
{
    __shared__ LutLds s_lut;
    constexpr int NC = X ? 4 : 2;
    constexpr int BPP = dst_bpp<DST>();
    const uint32_t sel = DST == DST_RGB32 || DST == DST_YUY2 ? cp->dst_sel : 0u;
    const int tid = threadIdx.x;
    const int dstW = cp->dstW, dstH = cp->dstH, cs = cp->vcs, srcH = cp->srcH, chrSrcH = cp->chrSrcH;
    /* only the vertical banks and five sizes of the record: read one by one */
    const int32_t *vLumP = mi355_global(cp->vLumP), *vChrP = mi355_global(cp->vChrP);
    const int16_t *vLumC = mi355_global(cp->vLumC), *vChrC = mi355_global(cp->vChrC);
    mi355_sws_frame fr = frames[blockIdx.z];
    for (int k = 0; k < 3; k++) fr.src[k] = mi355_global(fr.src[k]);
    fr.dst = mi355_global(fr.dst);
    const int x = blockIdx.x * C24_COLS + (tid & 63) * 8;   /* first of the thread's eight samples */
    const int npairs = dstW >> 1;
    const bool mine = (x >> 1) < npairs;
    bool wide = mine && (x >> 1) + 4 <= npairs &&
                ((reinterpret_cast<uintptr_t>(fr.src[0]) | (uintptr_t)fr.src_stride[0] | reinterpret_cast<uintptr_t>(fr.dst) | (uintptr_t)fr.dst_stride) & 7) == 0;
    if constexpr (DST == DST_RGB32 || DST == DST_YUY2) wide = wide && ((reinterpret_cast<uintptr_t>(fr.dst) | (uintptr_t)fr.dst_stride) & 15) == 0;
    if constexpr (NV) wide = wide && ((reinterpret_cast<uintptr_t>(fr.src[1]) | (uintptr_t)fr.src_stride[1]) & 7) == 0;
    else wide = wide && ((reinterpret_cast<uintptr_t>(fr.src[1]) | (uintptr_t)fr.src_stride[1] | reinterpret_cast<uintptr_t>(fr.src[2]) | (uintptr_t)fr.src_stride[2]) & 3) == 0;
    const int vu = NV && cp->src_layout == MI355_SWS_SRC_NV21;      /* the first byte of a pair is V */
    constexpr int NR = IDENT_ROWS / (NT / 64);
    /* the rows' lines and taps: every load unconditional (rows past the picture repeat its last row and are not written; a tap past the filter reads tap 0 and becomes zero) */
    int li[NR], lf[NR], c0[NR], cf[NR][NC];
#pragma unroll
    for (int q = 0; q < NR; q++) {
        const int gy = imin(blockIdx.y * IDENT_ROWS + (tid >> 6) + q * (NT / 64), dstH - 1);
        li[q] = vLumP[gy]; lf[q] = vLumC[gy]; c0[q] = vChrP[gy];
#pragma unroll
        for (int j = 0; j < NC; j++) cf[q][j] = vChrC[(size_t)gy * cs + (j < cs ? j : 0)];
    }
    sws_u32x2 ya[NR];
    uint32_t u[NR][NC], v[NR][NC];
    sws_u32x2 uv[NR][NC];                            /* NV: a tap line's four pairs as they lie */
    int ci[NR][NC];
#pragma unroll
    for (int q = 0; q < NR; q++) {
        li[q] = clampi(imax(0, li[q]), 0, srcH - 1);
        const int cfirst = imax(1 - cs, c0[q]);
        ya[q] = sws_u32x2{ 0u, 0u };
        if (wide) ya[q] = *reinterpret_cast<const sws_u32x2 *>(fr.src[0] + (size_t)li[q] * fr.src_stride[0] + x);
#pragma unroll
        for (int j = 0; j < NC; j++) {
            cf[q][j] = j < cs ? cf[q][j] : 0;
            ci[q][j] = clampi(cfirst + (j < cs ? j : 0), 0, chrSrcH - 1);
            u[q][j] = v[q][j] = 0;
            if constexpr (NV) {
                /* the pairs are taken apart behind the barrier, so that no load is waited for before the last one is requested */
                uv[q][j] = sws_u32x2{ 0u, 0u };
                if (wide) uv[q][j] = *reinterpret_cast<const sws_u32x2 *>(fr.src[1] + (size_t)ci[q][j] * fr.src_stride[1] + x);
            } else
            if (wide) {
                u[q][j] = *reinterpret_cast<const uint32_t *>(fr.src[1] + (size_t)ci[q][j] * fr.src_stride[1] + (x >> 1));
                v[q][j] = *reinterpret_cast<const uint32_t *>(fr.src[2] + (size_t)ci[q][j] * fr.src_stride[2] + (x >> 1));
            }
        }
    }
    MI355_ISSUE_FENCE();
    if constexpr (DST != DST_YUY2) {
    lut_load(s_lut, &cp->luts, tid);
    __syncthreads();
    }
    if (!mine) return;
#pragma unroll
    for (int q = 0; q < NR; q++) {
        const int gy = blockIdx.y * IDENT_ROWS + (tid >> 6) + q * (NT / 64);
        if (gy >= dstH) break;
        uint8_t *d = fr.dst + (size_t)gy * fr.dst_stride + (size_t)x * BPP;
        const bool mean = !X && cs > 1 && cf[q][1] >= 2048;
        /* one pair of the row from its bytes: two luma samples, the pair's chroma sample of each tap line */
        auto pair = [&](int y1, int y2, const int *us, const int *vs, int &Y1, int &Y2, int &U, int &V) {
            if (!X) {
                Y1 = y1; Y2 = y2;
                U = mean ? (us[0] + us[1]) >> 1 : us[0];
                V = mean ? (vs[0] + vs[1]) >> 1 : vs[0];
                return;
            }
            Y1 = ((1 << 18) + (y1 << 7) * lf[q]) >> 19; Y2 = ((1 << 18) + (y2 << 7) * lf[q]) >> 19;
            U = V = 1 << 18;
#pragma unroll
            for (int j = 0; j < NC; j++) { U += (us[j] << 7) * cf[q][j]; V += (vs[j] << 7) * cf[q][j]; }
            U >>= 19; V >>= 19;
            if ((Y1 | Y2 | U | V) & 0x100) { Y1 = clip_u8(Y1); Y2 = clip_u8(Y2); U = clip_u8(U); V = clip_u8(V); }
        };
        if (wide) {
            int Y[8], r[4], g[4], b[4];
            [[maybe_unused]] uint32_t grp4[4];                  /* DST_YUY2: the four groups as they leave */
            if constexpr (NV) {
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    const uint32_t e = sws_even4(uv[q][j][0], uv[q][j][1]), o = sws_odd4(uv[q][j][0], uv[q][j][1]);
                    u[q][j] = vu ? o : e; v[q][j] = vu ? e : o;
                }
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                int us[NC], vs[NC], U, V;
#pragma unroll
                for (int j = 0; j < NC; j++) { us[j] = (u[q][j] >> (8 * p)) & 0xFF; vs[j] = (v[q][j] >> (8 * p)) & 0xFF; }
                const uint32_t w = ya[q][p >> 1] >> (16 * (p & 1));
                pair((int)(w & 0xFF), (int)((w >> 8) & 0xFF), us, vs, Y[2 * p], Y[2 * p + 1], U, V);
                if constexpr (DST == DST_YUY2) grp4[p] = yuy2_group(Y[2 * p], U, Y[2 * p + 1], V, sel);
                else
                lut_rows_d<DST>(s_lut, U, V, r[p], g[p], b[p]);
            }
            /* (through store8_d the rgb24 instances got another instruction stream: the two stores are named here) */
            if constexpr (DST == DST_YUY2) *reinterpret_cast<sws_u32x4 *>(d) = sws_u32x4{ grp4[0], grp4[1], grp4[2], grp4[3] };
            else
            if constexpr (DST == DST_RGB32) rgb32_store8(s_lut, d, Y, r, g, b, sel);
            else rgb24_store8(s_lut, d, Y, r, g, b);
        } else {
            const uint8_t *py = fr.src[0] + (size_t)li[q] * fr.src_stride[0] + x;
            for (int p = 0; p < 4 && (x >> 1) + p < npairs; p++) {
                int us[NC], vs[NC], Y1, Y2, U, V;
#pragma unroll
                for (int j = 0; j < NC; j++) {
                    if constexpr (NV) {
                        const uint8_t *pp = fr.src[1] + (size_t)ci[q][j] * fr.src_stride[1] + x + 2 * p;
                        us[j] = pp[vu]; vs[j] = pp[1 - vu];
                    } else {
                    us[j] = fr.src[1][(size_t)ci[q][j] * fr.src_stride[1] + (x >> 1) + p];
                    vs[j] = fr.src[2][(size_t)ci[q][j] * fr.src_stride[2] + (x >> 1) + p];
                    }
                }
                pair(py[2 * p], py[2 * p + 1], us, vs, Y1, Y2, U, V);
                write_pair_d<DST>(s_lut, d + 2 * BPP * p, Y1, Y2, U, V, sel);
            }
        }
    }
}

/* ---- equal size to a packed RGB destination: k_sws_ident1's _1 form straight from the packed bytes ---------------------------------------------
 * The reference has no special converter from these sources to RGB: its scaler runs with identity horizontal filters and ONE vertical luma tap, and
 * with chroma on every source line the chroma filter has one or two taps — yuv2rgb24_1_c and its kin (output.c:1043-1110): Y = the luma byte, U / V
 * the first chroma line's byte, or the mean of two lines where the row's second coefficient is >= 2048.  k_sws_ident1's grid, tile and LUT copy; a
 * thread's eight samples of a row are 16 source bytes that hold luma AND chroma — one 16-byte load on a plane of 16-byte multiples, four dwords on
 * one of 4-byte multiples; a chroma tap line other than the luma line (uniform over the row's wave) is loaded the same way.  Ragged rows, and planes
 * on neither multiple, go byte by byte.  A kernel of its own name: another template parameter of k_sws_ident1 would rename its existing instances.
 * DST_YUY2: as k_sws_ident1's — four groups a thread, no table and no barrier (a re-ordering of the packed bytes, with the chroma mean where the row has it).
 * With chroma on every line no context of these sources reaches the X template (more than two chroma taps): sws.hip sends such a one to the tile. */
template <int DST>
__global__ void __launch_bounds__(NT) k_sws_ident1_yuy2(const SwsDev *cp, const mi355_sws_frame *frames)
{
    __shared__ LutLds s_lut;
    constexpr int NC = 2;
    constexpr int BPP = dst_bpp<DST>();
    const uint32_t sel = DST == DST_RGB32 || DST == DST_YUY2 ? cp->dst_sel : 0u;
    const int tid = threadIdx.x;
    const int dstW = cp->dstW, dstH = cp->dstH, cs = cp->vcs, srcH = cp->srcH, chrSrcH = cp->chrSrcH, layout = cp->src_layout;
    const int32_t *vLumP = mi355_global(cp->vLumP), *vChrP = mi355_global(cp->vChrP);
    const int16_t *vChrC = mi355_global(cp->vChrC);
    mi355_sws_frame fr = frames[blockIdx.z];
    fr.src[0] = mi355_global(fr.src[0]);
    fr.dst = mi355_global(fr.dst);
    const int x = blockIdx.x * C24_COLS + (tid & 63) * 8;   /* first of the thread's eight samples */
    const int npairs = dstW >> 1;
    const bool mine = (x >> 1) < npairs;
    const uintptr_t sal = reinterpret_cast<uintptr_t>(fr.src[0]) | (uintptr_t)fr.src_stride[0];
    const bool al16 = (sal & 15) == 0;
    constexpr uintptr_t DMASK = DST == DST_RGB32 || DST == DST_YUY2 ? 15 : 7;
    /* the wide form: four whole pairs (x + 8 <= dstW <= srcW: the 16 bytes lie inside the line's 2 * srcW) */
    const bool wide = mine && (x >> 1) + 4 <= npairs && (sal & 3) == 0 && ((reinterpret_cast<uintptr_t>(fr.dst) | (uintptr_t)fr.dst_stride) & DMASK) == 0;
    const bool uy = sws_yuy2_luma(layout) != 0, vu = layout == MI355_SWS_SRC_YVYU422;
    constexpr int NR = IDENT_ROWS / (NT / 64);
    int li[NR], ci[NR][NC], cf1[NR];
    uint32_t wl[NR][4], wc[NR][NC][4];
    auto load16 = [&](const uint8_t *p, uint32_t *w) {
        if (al16) {
            const sws_u32x4 v = *reinterpret_cast<const sws_u32x4 *>(p);
            w[0] = v[0]; w[1] = v[1]; w[2] = v[2]; w[3] = v[3];
        } else {
#pragma unroll
            for (int d = 0; d < 4; d++) w[d] = reinterpret_cast<const uint32_t *>(p)[d];
        }
    };
#pragma unroll
    for (int q = 0; q < NR; q++) {
        /* rows past the picture repeat its last row and are not written; a tap past the filter reads tap 0 */
        const int gy = imin(blockIdx.y * IDENT_ROWS + (tid >> 6) + q * (NT / 64), dstH - 1);
        li[q] = clampi(vLumP[gy], 0, srcH - 1);
        const int cfirst = imax(1 - cs, vChrP[gy]);
        cf1[q] = cs > 1 ? vChrC[(size_t)gy * cs + 1] : 0;
#pragma unroll
        for (int j = 0; j < NC; j++) ci[q][j] = clampi(cfirst + (j < cs ? j : 0), 0, chrSrcH - 1);
#pragma unroll
        for (int d = 0; d < 4; d++) wl[q][d] = 0;
        if (wide) load16(fr.src[0] + (size_t)li[q] * fr.src_stride[0] + 2 * (size_t)x, wl[q]);
#pragma unroll
        for (int j = 0; j < NC; j++) {
#pragma unroll
            for (int d = 0; d < 4; d++) wc[q][j][d] = wl[q][d];
            if (wide && ci[q][j] != li[q]) load16(fr.src[0] + (size_t)ci[q][j] * fr.src_stride[0] + 2 * (size_t)x, wc[q][j]);
        }
    }
    MI355_ISSUE_FENCE();
    if constexpr (DST != DST_YUY2) {
    lut_load(s_lut, &cp->luts, tid);
    __syncthreads();
    }
    if (!mine) return;
#pragma unroll
    for (int q = 0; q < NR; q++) {
        const int gy = blockIdx.y * IDENT_ROWS + (tid >> 6) + q * (NT / 64);
        if (gy >= dstH) break;
        uint8_t *d = fr.dst + (size_t)gy * fr.dst_stride + (size_t)x * BPP;
        const bool mean = cs > 1 && cf1[q] >= 2048;
        if (wide) {
            int Y[8], r[4], g[4], b[4];
            [[maybe_unused]] uint32_t grp4[4];                  /* DST_YUY2: the four groups as they leave */
            const uint32_t ya[2] = { uy ? sws_odd4(wl[q][0], wl[q][1]) : sws_even4(wl[q][0], wl[q][1]), uy ? sws_odd4(wl[q][2], wl[q][3]) : sws_even4(wl[q][2], wl[q][3]) };
            uint32_t u[NC], v[NC];
#pragma unroll
            for (int j = 0; j < NC; j++) {
                const uint32_t *w = wc[q][j];
                const uint32_t c01 = uy ? sws_even4(w[0], w[1]) : sws_odd4(w[0], w[1]), c23 = uy ? sws_even4(w[2], w[3]) : sws_odd4(w[2], w[3]);
                const uint32_t e = sws_even4(c01, c23), o = sws_odd4(c01, c23);
                u[j] = vu ? o : e; v[j] = vu ? e : o;
            }
#pragma unroll
            for (int p = 0; p < 4; p++) {
                const int u0 = (u[0] >> (8 * p)) & 0xFF, u1 = (u[1] >> (8 * p)) & 0xFF, v0 = (v[0] >> (8 * p)) & 0xFF, v1 = (v[1] >> (8 * p)) & 0xFF;
                const uint32_t w = ya[p >> 1] >> (16 * (p & 1));
                Y[2 * p] = (int)(w & 0xFF); Y[2 * p + 1] = (int)((w >> 8) & 0xFF);
                if constexpr (DST == DST_YUY2) grp4[p] = yuy2_group(Y[2 * p], mean ? (u0 + u1) >> 1 : u0, Y[2 * p + 1], mean ? (v0 + v1) >> 1 : v0, sel);
                else
                lut_rows_d<DST>(s_lut, mean ? (u0 + u1) >> 1 : u0, mean ? (v0 + v1) >> 1 : v0, r[p], g[p], b[p]);
            }
            if constexpr (DST == DST_YUY2) *reinterpret_cast<sws_u32x4 *>(d) = sws_u32x4{ grp4[0], grp4[1], grp4[2], grp4[3] };
            else
            if constexpr (DST == DST_RGB32) rgb32_store8(s_lut, d, Y, r, g, b, sel);
            else rgb24_store8(s_lut, d, Y, r, g, b);
        } else {
            const int lo = sws_yuy2_luma(layout), uo = sws_yuy2_u(layout), vo = sws_yuy2_v(layout);
            const uint8_t *py = fr.src[0] + (size_t)li[q] * fr.src_stride[0] + 2 * (size_t)x;
            for (int p = 0; p < 4 && (x >> 1) + p < npairs; p++) {
                const uint8_t *p0 = fr.src[0] + (size_t)ci[q][0] * fr.src_stride[0] + 2 * (size_t)x + 4 * p, *p1 = fr.src[0] + (size_t)ci[q][1] * fr.src_stride[0] + 2 * (size_t)x + 4 * p;
                const int U = mean ? (p0[uo] + p1[uo]) >> 1 : p0[uo], V = mean ? (p0[vo] + p1[vo]) >> 1 : p0[vo];
                write_pair_d<DST>(s_lut, d + 2 * BPP * p, py[4 * p + lo], py[4 * p + lo + 2], U, V, sel);
            }
        }
    }
}

/* ---- Tier-1 line kernels ---------------------------------------------------------------------------- */
template <typename ST = uint8_t>
__global__ void __launch_bounds__(NT) k_sws_line_hscale(int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter, const int32_t *pos, int fs, int sh)
{
    for (int i = threadIdx.x; i < dstW; i += NT) dst[i] = (int16_t)hscale_one<ST>(src, filter + (size_t)i * fs, pos[i], fs, sh);
}
#ifndef MI355_SWS_TILE_KERNELS_ONLY
/* rgb24ToY_c / bgr24ToY_c and the ...ToUV_c / ...ToUV_half_c pairs (input.c:539-623) of one line: one sample per thread and step */
__global__ void __launch_bounds__(NT) k_sws_line_rgb24_y(uint8_t *dst, const uint8_t *src, int width, int bgr)
{
    const RgbK K = rgb_consts(false, false, bgr != 0);
    for (int i = threadIdx.x; i < width; i += NT) {
        int a, b;
        rgb_sample(src + 3 * (size_t)i, false, K, a, b);
        dst[i] = (uint8_t)a;
    }
}
__global__ void __launch_bounds__(NT) k_sws_line_rgb24_uv(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int bgr, int half)
{
    const RgbK K = rgb_consts(true, half != 0, bgr != 0);
    for (int i = threadIdx.x; i < width; i += NT) {
        int a, b;
        rgb_sample(src + (half ? 6 : 3) * (size_t)i, half != 0, K, a, b);
        dstU[i] = (uint8_t)a; dstV[i] = (uint8_t)b;
    }
}
/* lumConvertRange / chrConvertRange of one line, in place */
__global__ void __launch_bounds__(NT) k_sws_line_range(int16_t *line, int width, SwsRangeMap m)
{
    for (int i = threadIdx.x; i < width; i += NT) line[i] = (int16_t)range_one(line[i], m);
}
/* yuv2planeX_8_c output.c:242-255 (fs >= 1 rows at `pitch` elements) / yuv2plane1_8_c :257-266 (fs == 0) */
__global__ void __launch_bounds__(NT) k_sws_line_plane(const int16_t *filter, int fs, const int16_t *rows, int pitch, uint8_t *dest, int dstW,
                                                       const uint8_t *dither, int offset)
{
    for (int i = threadIdx.x; i < dstW; i += NT) {
        if (fs == 0) { dest[i] = (uint8_t)clip_u8((rows[i] + dither[(i + offset) & 7]) >> 7); continue; }
        int val = dither[(i + offset) & 7] << 12;
        for (int j = 0; j < fs; j++) val += rows[(size_t)j * pitch + i] * filter[j];
        dest[i] = (uint8_t)clip_u8(val >> 19);
    }
}
/* yuv2planeX_10_c_template output.c:196-213 (fs >= 1 rows at `pitch` elements) / yuv2plane1_10_c_template :183-194 (fs == 0), little endian */
__global__ void __launch_bounds__(NT) k_sws_line_plane16(const int16_t *filter, int fs, const int16_t *rows, int pitch, uint16_t *dest, int dstW, int bits)
{
    const int top = (1 << bits) - 1;
    for (int i = threadIdx.x; i < dstW; i += NT) {
        if (fs == 0) { dest[i] = (uint16_t)clampi((rows[i] + (1 << (14 - bits))) >> (15 - bits), 0, top); continue; }
        int val = 1 << (26 - bits);
        for (int j = 0; j < fs; j++) val += rows[(size_t)j * pitch + i] * filter[j];
        dest[i] = (uint16_t)clampi(val >> (27 - bits), 0, top);
    }
}
/* yuv2nv12cX_c output.c:267-301: fs >= 1 rows of U and of V at `pitch` elements, the pairs in U V (swap_uv: V U) order */
__global__ void __launch_bounds__(NT) k_sws_line_nv12(const int16_t *filter, int fs, const int16_t *urows, const int16_t *vrows, int pitch, uint8_t *dest,
                                                      int chrDstW, const uint8_t *dither, int swap_uv)
{
    for (int i = threadIdx.x; i < chrDstW; i += NT) {
        int u = dither[i & 7] << 12, v = dither[(i + 3) & 7] << 12;
        for (int j = 0; j < fs; j++) { u += urows[(size_t)j * pitch + i] * filter[j]; v += vrows[(size_t)j * pitch + i] * filter[j]; }
        dest[2 * i + (swap_uv ? 1 : 0)] = (uint8_t)clip_u8(u >> 19);
        dest[2 * i + (swap_uv ? 0 : 1)] = (uint8_t)clip_u8(v >> 19);
    }
}
#endif
struct PackedRows {
    const int16_t *l, *u, *v;
    int pitch;
    const int16_t *a = nullptr;                 /* the alpha lines of the _a line entries: the luma lines' count and pitch */
    __device__ __forceinline__ int alp(int j, int x) const { return a[(size_t)j * pitch + x]; }
    __device__ __forceinline__ int lum(int j, int x) const { return l[(size_t)j * pitch + x]; }
    __device__ __forceinline__ int cu(int j, int x) const { return u[(size_t)j * pitch + x]; }
    __device__ __forceinline__ int cv(int j, int x) const { return v[(size_t)j * pitch + x]; }
};
/* yuv2rgb_X_c / _2_c / _1_c (output.c:937-1110) with target bgr24 (DST_BGR24) or one of the four 32-bit orders (DST_RGB32, `sel`: sws_rgb32_sel): the
 * line kernel below with the destination form of the whole-picture kernels; dest holds (dstW + 1) >> 1 pairs of 2 * dst_bpp<DST>() bytes */
template <int DST>
__global__ void __launch_bounds__(NT) k_sws_line_packed(const mi355_sws_luts *luts, int mode, const int16_t *lumF, const int16_t *l, int ls,
                                                        const int16_t *chrF, const int16_t *u, const int16_t *v, int cs, int pitch, uint8_t *dest,
                                                        int dstW, int yalpha, int uvalpha, uint32_t sel)
{
    __shared__ LutLds s_lut;
    if constexpr (DST != DST_YUY2) {                /* (a packed 4:2:2 order has no table: luts is not read) */
    lut_load(s_lut, luts, threadIdx.x);
    __syncthreads();
    }
    PackedRows R{ l, u, v, pitch };
    for (int i = threadIdx.x; i < ((dstW + 1) >> 1); i += NT)
        rgb_pair<DST>(s_lut, dest + (size_t)i * 2 * dst_bpp<DST>(), R, i, mode, lumF, ls, chrF, cs, yalpha, uvalpha, sel);
}
#ifndef MI355_SWS_TILE_KERNELS_ONLY
__global__ void __launch_bounds__(NT) k_sws_line_rgb(const mi355_sws_luts *luts, int mode, const int16_t *lumF, const int16_t *l, int ls,
                                                     const int16_t *chrF, const int16_t *u, const int16_t *v, int cs, int pitch, uint8_t *dest,
                                                     int dstW, int yalpha, int uvalpha)
{
    __shared__ LutLds s_lut;
    lut_load(s_lut, luts, threadIdx.x);
    __syncthreads();
    PackedRows R{ l, u, v, pitch };
    for (int i = threadIdx.x; i < ((dstW + 1) >> 1); i += NT) rgb_pair(s_lut, dest + (size_t)i * 6, R, i, mode, lumF, ls, chrF, cs, yalpha, uvalpha);
}
#endif
}  // namespace

/* ---- the launch key --------------------------------------------------------------------------------------------------------------------
 * Which instance of which kernel a launch runs, named once.  sws.hip fills a key from a context (sws_key) and hands it to the file that owns the
 * instance; every file maps it to hipLaunchKernelGGL through the one dispatcher below (sws_launch).
 *   kernel  GENERIC / PLANAR: the tile kernels k_sws_generic / k_sws_planar, instance i; IDENT1_1 / IDENT1_X: k_sws_ident1<false / true> (a packed
 *           4:2:2 source: k_sws_ident1_yuy2); C24 / C24_422: k_sws_c24<0 / 1> (yuv422p: every other chroma line); LINE: k_sws_line_packed of one line
 *           (alpha: k_sws_line_packed_a); YUY2_SPLIT: k_sws_yuy2_split; YUY2_PACK: k_sws_yuy2_pack
 *   i       0 / 1 / 2: the A / B / C row of GENERIC_SHAPES / PLANAR_SHAPES, as sws_kernel() chose it
 *   src     the source class — P8 / P16: three planes of bytes / of 16-bit samples, NV: NV12 / NV21, RGB24: rgb24 / bgr24, RGB32: rgba / bgra /
 *           argb / abgr, YUY2: yuyv422 / uyvy422 / yvyu422 (the order inside a class is read from the context on the device), P010: p010le, a plane of
 *           16-bit words and a plane of pairs of them
 *   form    of k_sws_planar — HALF: three planes, chroma tiles of CW = TW / 2, FULL: of CW = TW (a 4:4:4 destination), SEMI: NV12 / NV21
 *   kind    of k_sws_planar — PLAIN, RANGE (range conversion between the passes), DEEP (9- / 10-bit planes; three planes, no range)
 *   dst     of the packed kernels — DST_RGB24 / DST_BGR24 / DST_RGB32 (the 32-bit order is the operands' sel) / DST_YUY2 (the 4:2:2 order likewise)
 *   alpha   the ALPHA form: a 32-bit source's alpha to a 32-bit destination
 * A key a file has no instance for (DEEP with SEMI, ALPHA outside RGB32 -> DST_RGB32, another file's source class, kind or destination) is not
 * launched: the launch functions return false and the entry point -2. */
enum SwsKernel { SWS_KERNEL_GENERIC, SWS_KERNEL_PLANAR, SWS_KERNEL_IDENT1_1, SWS_KERNEL_IDENT1_X, SWS_KERNEL_C24, SWS_KERNEL_C24_422, SWS_KERNEL_LINE, SWS_KERNEL_YUY2_SPLIT,
                 SWS_KERNEL_YUY2_PACK };
enum SwsSrcClass { SWS_SRC_P8, SWS_SRC_P16, SWS_SRC_NV, SWS_SRC_RGB24, SWS_SRC_RGB32, SWS_SRC_YUY2, SWS_SRC_P010 };
enum SwsForm { SWS_FORM_HALF, SWS_FORM_FULL, SWS_FORM_SEMI };
enum SwsKind { SWS_KIND_PLAIN, SWS_KIND_RANGE, SWS_KIND_DEEP };
struct SwsKey {
    SwsKernel kernel;
    int i;
    SwsSrcClass src;
    SwsForm form;
    SwsKind kind;
    int dst;
    bool alpha;
};
/* the arguments of k_sws_line_rgb / k_sws_line_packed / k_sws_line_packed_a (a: the alpha lines of the last one) */
struct SwsLine {
    const mi355_sws_luts *luts;
    int mode;
    const int16_t *lumF, *l;
    int ls;
    const int16_t *chrF, *u, *v;
    int cs;
    const int16_t *a;
    int pitch;
    uint8_t *dest;
    int dstW, yalpha, uvalpha;
};
/* what a launch takes besides its key.  h / d: the context's SwsDev on the host / on the device (none for a slice or a line); frames: the
 * mi355_sws_frame / mi355_sws_planar_frame records on the device; luts, dstW, rows: the tables, width and slice rows of k_sws_c24; sel: the byte
 * selector of a 32-bit order where the kernel takes it as an argument (k_sws_c24, the line kernels); line: the operands of SWS_KERNEL_LINE */
struct SwsOperands {
    dim3 grid;
    hipStream_t s;
    const void *h, *d, *frames;
    const mi355_sws_luts *luts;
    int dstW, rows;
    uint32_t sel;
    const SwsLine *line;
    uint32_t lum_inc, chr_inc;     /* a fast-bilinear context's lumXInc / chrXInc (mi355_sws_launch_fastbl alone reads them) */
    const mi355_sws_rgb_coefs *coefs;      /* a gbrp context's six coefficients, on the host (mi355_sws_launch_gbrp alone reads them) */
};
/* one launch function a file: false for a key the file has no instance for */
bool mi355_sws_launch_deep(const SwsKey &key, const SwsOperands &op);       /* sws_deep.hip: the DEEP instances of the four classic source classes */
bool mi355_sws_launch_packed(const SwsKey &key, const SwsOperands &op);     /* sws_packed.hip: DST_BGR24 / DST_RGB32 of k_sws_generic, k_sws_ident1, k_sws_c24, k_sws_line_packed */
bool mi355_sws_launch_rgb32(const SwsKey &key, const SwsOperands &op);      /* sws_rgb32.hip: every tile instance of SWS_SRC_RGB32, k_sws_line_packed_a */
bool mi355_sws_launch_yuy2(const SwsKey &key, const SwsOperands &op);       /* sws_yuy2.hip: every tile instance of SWS_SRC_YUY2, k_sws_ident1_yuy2, k_sws_yuy2_split */
bool mi355_sws_launch_p010(const SwsKey &key, const SwsOperands &op);       /* sws_p010.hip: every tile instance of SWS_SRC_P010, DST_YUY2 included */
bool mi355_sws_launch_fastbl(const SwsKey &key, const SwsOperands &op);     /* sws_fastbl.hip: every instance of k_sws_fbl_generic / k_sws_fbl_planar (a fast-bilinear context's key is its twin's) */
bool mi355_sws_launch_gbrp(const SwsKey &key, const SwsOperands &op);       /* sws_gbrp.hip: every instance of k_sws_gbrp (a gbrp context's key is its yuv444p twin's: PLANAR, FULL, PLAIN) */
bool mi355_sws_launch_yuy2dst(const SwsKey &key, const SwsOperands &op);    /* sws_yuy2dst.hip: DST_YUY2 of k_sws_generic, k_sws_ident1, k_sws_ident1_yuy2, k_sws_line_packed from every source class; k_sws_yuy2_pack */

namespace {
/* the three grids of the picture kernels: the tile kernels' (th rows of TW samples), k_sws_ident1's and k_sws_c24's (rows: source rows of the slice) */
inline dim3 sws_tile_grid(const SwsDev &h, int nframes) { return dim3((h.dstW + TW - 1) / TW, (h.dstH + h.th - 1) / h.th, nframes); }
inline dim3 sws_ident1_grid(const SwsDev &h, int nframes) { return dim3((h.dstW + C24_COLS - 1) / C24_COLS, (h.dstH + IDENT_ROWS - 1) / IDENT_ROWS, nframes); }
inline dim3 sws_c24_grid(int dstW, int rows, int nframes) { return dim3((dstW + C24_COLS - 1) / C24_COLS, (rows + C24_ROWS - 1) / C24_ROWS, nframes); }

/* f(std::integral_constant<E, V>()) for the V of Vs that v equals: a run-time code as a template argument.  false where v is none of them */
template <typename E, E... Vs, typename F> bool sws_pick(E v, F f)
{
    bool done = false;
    (void)((v == Vs && ((done = f(std::integral_constant<E, Vs>())), true)) || ...);
    return done;
}
template <typename F> bool sws_pick_dst(int dst, F f) { return sws_pick<int, DST_RGB24, DST_BGR24, DST_RGB32, DST_YUY2>(dst, f); }
/* ... of the three RGB forms alone (a file that compiles no DST_YUY2 instance of a kernel it picks for) */
template <typename F> bool sws_pick_dst_rgb(int dst, F f) { return sws_pick<int, DST_RGB24, DST_BGR24, DST_RGB32>(dst, f); }
/* instance i as I: the row of GENERIC_SHAPES / PLANAR_SHAPES that sws_launch_generic / sws_launch_planar read */
template <typename F> bool sws_pick_instance(int i, F f) { return sws_pick<int, 0, 1, 2>(i, f); }
constexpr unsigned sws_bit(int v) { return 1u << v; }
constexpr unsigned SWS_CLASSIC_SRCS = sws_bit(SWS_SRC_P8) | sws_bit(SWS_SRC_P16) | sws_bit(SWS_SRC_NV) | sws_bit(SWS_SRC_RGB24);
constexpr unsigned SWS_ALL_KINDS = sws_bit(SWS_KIND_PLAIN) | sws_bit(SWS_KIND_RANGE) | sws_bit(SWS_KIND_DEEP);
constexpr unsigned SWS_ALL_DSTS = sws_bit(DST_RGB24) | sws_bit(DST_BGR24) | sws_bit(DST_RGB32);

/* what a source class is to the tile kernels: the sample type and the NV / RGB arguments (the ALPHA form: SwsPx32A in place of SwsPx32) */
template <SwsSrcClass C> struct SwsSrc { typedef uint8_t ST; static constexpr bool NV = false, RGB = false; };
template <> struct SwsSrc<SWS_SRC_P16> { typedef uint16_t ST; static constexpr bool NV = false, RGB = false; };
template <> struct SwsSrc<SWS_SRC_NV> { typedef uint8_t ST; static constexpr bool NV = true, RGB = false; };
template <> struct SwsSrc<SWS_SRC_RGB24> { typedef uint8_t ST; static constexpr bool NV = false, RGB = true; };
template <> struct SwsSrc<SWS_SRC_RGB32> { typedef SwsPx32 ST; static constexpr bool NV = false, RGB = true; };
template <> struct SwsSrc<SWS_SRC_YUY2> { typedef SwsPxYuy2 ST; static constexpr bool NV = false, RGB = true; };
template <> struct SwsSrc<SWS_SRC_P010> { typedef SwsPxP010 ST; static constexpr bool NV = true, RGB = false; };

/* instance I of k_sws_generic: its waves per SIMD are what its LDS allows (the staging lines of its sample type, the alpha tile of the ALPHA form),
 * like the planar kernel's own */
template <int I, SwsSrcClass C, int DST, bool ALPHA> void sws_launch_generic(const SwsOperands &op)
{
    typedef typename std::conditional<ALPHA, SwsPx32A, typename SwsSrc<C>::ST>::type ST;
    constexpr SwsShape S = GENERIC_SHAPES[I];
    hipLaunchKernelGGL((k_sws_generic<S.lcap, S.ccap, sws_waves(sws_lds_bytes(S.lcap, S.ccap, stage_bytes<ST>(), ALPHA, DST != DST_YUY2)), ST, SwsSrc<C>::NV, SwsSrc<C>::RGB, DST>), op.grid, dim3(NT), 0,
                       op.s, static_cast<const SwsDev *>(op.d), static_cast<const mi355_sws_frame *>(op.frames));
}
template <int I, SwsSrcClass C, SwsForm F, SwsKind K> void sws_launch_planar(const SwsOperands &op)
{
    constexpr SwsShape S = PLANAR_SHAPES[I];
    hipLaunchKernelGGL((k_sws_planar<S.lcap, S.ccap, F == SWS_FORM_FULL ? TW : TW / 2, typename SwsSrc<C>::ST, F == SWS_FORM_SEMI, SwsSrc<C>::NV, SwsSrc<C>::RGB, K == SWS_KIND_RANGE,
                                     K == SWS_KIND_DEEP>), op.grid, dim3(NT), 0, op.s, static_cast<const SwsDev *>(op.d), static_cast<const mi355_sws_planar_frame *>(op.frames));
}
template <int CS, int DST> void sws_launch_c24(const SwsOperands &op)
{
    typename C24Arg<DST>::type slice{};                     /* the slice starts at row 0; a 32-bit form: with the order's selector */
    if constexpr (DST == DST_RGB32) slice.sel = op.sel;
    hipLaunchKernelGGL((k_sws_c24<CS, DST>), op.grid, dim3(NT), 0, op.s, op.luts, op.dstW, op.rows, slice, static_cast<const mi355_sws_frame *>(op.frames));
}
template <bool X, bool NV, int DST> void sws_launch_ident1(const SwsOperands &op)
{
    hipLaunchKernelGGL((k_sws_ident1<X, NV, DST>), op.grid, dim3(NT), 0, op.s, static_cast<const SwsDev *>(op.d), static_cast<const mi355_sws_frame *>(op.frames));
}

/* THE dispatcher: the picture kernels of sws_dev.h for a key, restricted at compile time to the slice of the instance space the calling file owns —
 * SRCS: its source classes, KINDS: its kinds of k_sws_planar, DSTS: its destination forms of the packed kernels (masks of sws_bit).  What lies outside
 * the masks is not instantiated, and a key that asks for it comes back false. */
template <unsigned SRCS, unsigned KINDS, unsigned DSTS> bool sws_launch(const SwsKey &key, const SwsOperands &op)
{
    return sws_pick<SwsSrcClass, SWS_SRC_P8, SWS_SRC_P16, SWS_SRC_NV, SWS_SRC_RGB24, SWS_SRC_RGB32, SWS_SRC_YUY2, SWS_SRC_P010>(key.src, [&](auto src) {
        constexpr SwsSrcClass C = decltype(src)::value;
        if constexpr ((SRCS & sws_bit(C)) == 0) return false;
        else if (key.kernel == SWS_KERNEL_PLANAR) {
            return sws_pick<SwsKind, SWS_KIND_PLAIN, SWS_KIND_RANGE, SWS_KIND_DEEP>(key.kind, [&](auto kind) {
                constexpr SwsKind K = decltype(kind)::value;
                if constexpr ((KINDS & sws_bit(K)) == 0) return false;
                else return sws_pick<SwsForm, SWS_FORM_HALF, SWS_FORM_FULL, SWS_FORM_SEMI>(key.form, [&](auto form) {
                    constexpr SwsForm F = decltype(form)::value;
                    if constexpr (K == SWS_KIND_DEEP && F == SWS_FORM_SEMI) return false;
                    else return sws_pick_instance(key.i, [&](auto i) { sws_launch_planar<decltype(i)::value, C, F, K>(op); return true; });
                });
            });
        } else {
            return sws_pick_dst(key.dst, [&](auto dst) {
                constexpr int DST = decltype(dst)::value;
                if constexpr ((DSTS & sws_bit(DST)) == 0) return false;
                else if (key.kernel == SWS_KERNEL_GENERIC) {
                    constexpr bool HAS_ALPHA = C == SWS_SRC_RGB32 && DST == DST_RGB32;       /* the one pair that has an ALPHA form */
                    if (key.alpha && !HAS_ALPHA) return false;
                    return sws_pick_instance(key.i, [&](auto i) {
                        if constexpr (HAS_ALPHA) if (key.alpha) { sws_launch_generic<decltype(i)::value, C, DST, true>(op); return true; }
                        sws_launch_generic<decltype(i)::value, C, DST, false>(op);
                        return true;
                    });
                } else if constexpr (C == SWS_SRC_P8 || C == SWS_SRC_NV) {
                    /* k_sws_ident1 reads three planes of bytes or an NV source, k_sws_c24 three planes of bytes */
                    if (key.kernel == SWS_KERNEL_IDENT1_1) { sws_launch_ident1<false, C == SWS_SRC_NV, DST>(op); return true; }
                    if (key.kernel == SWS_KERNEL_IDENT1_X) { sws_launch_ident1<true, C == SWS_SRC_NV, DST>(op); return true; }
                    if constexpr (C == SWS_SRC_P8 && DST != DST_YUY2) {          /* (no special converter writes a packed 4:2:2 order) */
                        if (key.kernel == SWS_KERNEL_C24) { sws_launch_c24<0, DST>(op); return true; }
                        if (key.kernel == SWS_KERNEL_C24_422) { sws_launch_c24<1, DST>(op); return true; }
                    }
                    return false;
                } else return false;
            });
        }
    });
}

/* one line through a Tier-1 line kernel on the staging arena: nsrc source bytes in, NOUT (1 / 2) planes of `width` bytes out; tail: the kernel's
 * arguments behind (dst..., src, width) */
template <int NOUT, typename K, typename... A>
void sws_line(K kernel, uint8_t *const *out, const uint8_t *src, size_t nsrc, int width, A... tail)
{
    mi355::Arena &a = mi355::arena();
    a.reserve(nsrc + (size_t)NOUT * (width + 32) + 64);
    const size_t o_src = a.take(nsrc);
    size_t o_d[NOUT];
    for (int p = 0; p < NOUT; p++) o_d[p] = a.take((size_t)width);
    std::memcpy(a.h<uint8_t>(o_src), src, nsrc);
    a.upload();
    if constexpr (NOUT == 2) hipLaunchKernelGGL(kernel, dim3(1), dim3(NT), 0, a.stream, a.d<uint8_t>(o_d[0]), a.d<uint8_t>(o_d[1]), a.d<const uint8_t>(o_src), width, tail...);
    else hipLaunchKernelGGL(kernel, dim3(1), dim3(NT), 0, a.stream, a.d<uint8_t>(o_d[0]), a.d<const uint8_t>(o_src), width, tail...);
    a.download();
    for (int p = 0; p < NOUT; p++) std::memcpy(out[p], a.h<uint8_t>(o_d[p]), (size_t)width);
}
}  // namespace

#endif
