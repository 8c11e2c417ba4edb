/*
 * sws_rgb32.hip — packed 32-bit SOURCES (rgba / bgra / argb / abgr: MI355_SWS_SRC_RGBA ... _ABGR): the RGB instances of the tile kernels (sws_dev.h)
 * whose sample type is a 32-bit pixel, once for every instance the rgb24 / bgr24 source has — k_sws_generic A / B / C to rgb24, bgr24 and the four
 * 32-bit orders, and its ALPHA form; k_sws_planar A / B / C at both chroma widths, plain, SEMI, RANGE and DEEP: every key of source class
 * SWS_SRC_RGB32 (sws_dev.h: SwsKey) — their launch, the three Tier-1 line entries mi355_sws_rgb32ToY / _rgb32ToUV / _rgb32ToA with their line kernels,
 * and the line kernel of mi355_sws_yuv2packed_X_a / _2_a / _1_a.  The context, the plan, the key and the picture entry points are sws.hip's
 * (mi355_sws_create_src_layout with layout 8 .. 11).  A file of its own so that the instances compile beside sws.hip, not behind it.
 *
 * The converted samples are staged as bytes in the 8-bit instances' staging lines (stage_bytes<SwsPx32>() is STAGE_BYTES), so every instance has
 * the LDS, the waves per SIMD and the workgroups per CU of its rgb24-source twin.
 */
#include "mi355_rt.h"
#define MI355_SWS_TILE_KERNELS_ONLY
#include "sws_dev.h"
#include "../../include/mi355dsp.h"

using namespace mi355;

/* the sample type of these instances is one pixel (SwsSrc<SWS_SRC_RGB32>) */
static_assert(stage_bytes<SwsPx32>() == STAGE_BYTES && stage_bytes<SwsPx32A>() == STAGE_BYTES, "the twins' staging lines");

/* the ALPHA form (a 32-bit destination that takes the source's alpha): the twin's LDS plus the alpha tile, as many lines as the luma tile —
 * A 19200 -> 26368 bytes, B 23296 -> 33536, C 26368 -> 38656: 6 / 4 / 4 workgroups a CU where the colour-only twins have 8 / 7 / 6 */
static_assert(sws_waves(sws_lds_bytes(GENERIC_SHAPES[0].lcap, GENERIC_SHAPES[0].ccap, STAGE_BYTES, true)) == 6 &&
              sws_waves(sws_lds_bytes(GENERIC_SHAPES[1].lcap, GENERIC_SHAPES[1].ccap, STAGE_BYTES, true)) == 4 &&
              sws_waves(sws_lds_bytes(GENERIC_SHAPES[2].lcap, GENERIC_SHAPES[2].ccap, STAGE_BYTES, true)) == 4, "workgroups per CU of the ALPHA instances");

/* yuv2rgba32_X_c / _2_c / _1_c ... with hasAlpha (output.c:937-1110): k_sws_line_packed<DST_RGB32> with the alpha lines */
namespace {
__global__ void __launch_bounds__(NT) k_sws_line_packed_a(const mi355_sws_luts *luts, int mode, const int16_t *lumF, const int16_t *l, int ls,
                                                          const int16_t *chrF, const int16_t *u, const int16_t *v, int cs, const int16_t *a, int pitch, uint8_t *dest,
                                                          int dstW, int yalpha, int uvalpha, uint32_t sel)
{
    __shared__ LutLds s_lut;
    lut_load(s_lut, luts, threadIdx.x);
    __syncthreads();
    PackedRows R{ l, u, v, pitch, a };
    for (int i = threadIdx.x; i < ((dstW + 1) >> 1); i += NT)
        rgb_pair<DST_RGB32, true>(s_lut, dest + (size_t)i * 8, R, i, mode, lumF, ls, chrF, cs, yalpha, uvalpha, sel);
}
}  // namespace

bool mi355_sws_launch_rgb32(const SwsKey &key, const SwsOperands &op)
{
    if (key.kernel != SWS_KERNEL_LINE) return sws_launch<sws_bit(SWS_SRC_RGB32), SWS_ALL_KINDS, SWS_ALL_DSTS>(key, op);
    /* one line with its alpha lines, one workgroup (the colour-only forms are sws.hip's and sws_packed.hip's) */
    if (!key.alpha || key.dst != DST_RGB32) return false;
    const SwsLine &n = *op.line;
    hipLaunchKernelGGL(k_sws_line_packed_a, dim3(1), dim3(NT), 0, op.s, n.luts, n.mode, n.lumF, n.l, n.ls, n.chrF, n.u, n.v, n.cs, n.a, n.pitch, n.dest, n.dstW, n.yalpha, n.uvalpha,
                       op.sel);
    return true;
}

/* ---- Tier-1 line entries ------------------------------------------------------------------------------------------------------------ */
namespace {
/* rgb32ToY_c ... bgr321ToY_c and the ...ToUV_c / ...ToUV_half_c forms (input.c:165-291) of one line: one sample per thread and step */
__global__ void __launch_bounds__(NT) k_sws_line_rgb32_y(uint8_t *dst, const uint8_t *src, int width, int layout)
{
    const RgbK K = rgb_consts(false, false, sws_src_bgr(layout));
    const int first = (int)(sws_src_ash(layout) >> 3);
    for (int i = threadIdx.x; i < width; i += NT) {
        int a, b;
        rgb32_sample(src + 4 * (size_t)i, false, first, K, a, b);
        dst[i] = (uint8_t)a;
    }
}
__global__ void __launch_bounds__(NT) k_sws_line_rgb32_uv(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int layout, int half)
{
    const RgbK K = rgb_consts(true, half != 0, sws_src_bgr(layout));
    const int first = (int)(sws_src_ash(layout) >> 3);
    for (int i = threadIdx.x; i < width; i += NT) {
        int a, b;
        rgb32_sample(src + (half ? 8 : 4) * (size_t)i, half != 0, first, K, a, b);
        dstU[i] = (uint8_t)a; dstV[i] = (uint8_t)b;
    }
}
/* rgbaToA_c / abgrToA_c (input.c:305-319) */
__global__ void __launch_bounds__(NT) k_sws_line_rgb32_a(uint8_t *dst, const uint8_t *src, int width, int layout)
{
    const int at = sws_src_ash(layout) ? 0 : 3;
    for (int i = threadIdx.x; i < width; i += NT) dst[i] = src[4 * (size_t)i + at];
}
}  // namespace

extern "C" void mi355_sws_rgb32ToY(uint8_t *dst, const uint8_t *src, int width, int layout)
{
    if (width <= 0 || !sws_rgb32_src(layout)) return;
    sws_line<1>(k_sws_line_rgb32_y, &dst, src, (size_t)4 * width, width, layout);
}
extern "C" void mi355_sws_rgb32ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int layout, int half)
{
    if (width <= 0 || !sws_rgb32_src(layout)) return;
    uint8_t *const out[2] = { dstU, dstV };
    sws_line<2>(k_sws_line_rgb32_uv, out, src, (size_t)(half ? 8 : 4) * width, width, layout, half);
}
extern "C" void mi355_sws_rgb32ToA(uint8_t *dst, const uint8_t *src, int width, int layout)
{
    if (width <= 0 || !sws_rgb32_src(layout)) return;
    sws_line<1>(k_sws_line_rgb32_a, &dst, src, (size_t)4 * width, width, layout);
}
