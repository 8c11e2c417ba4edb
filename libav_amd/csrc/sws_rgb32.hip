/*
 * sws_rgb32.hip — packed 32-bit SOURCES (rgba / bgra / argb / abgr: MI355_SWS_SRC_RGBA ... _ABGR): the RGB instances of the tile kernels (sws_dev.h)
 * whose sample type is a 32-bit pixel, once for every instance the rgb24 / bgr24 source has — k_sws_generic A / B / C to rgb24, bgr24 and the four
 * 32-bit orders, and its ALPHA form; k_sws_planar A / B / C at both chroma widths, plain, SEMI, RANGE and DEEP — their launches, the three Tier-1
 * line entries mi355_sws_rgb32ToY / _rgb32ToUV / _rgb32ToA with their line kernels, and the line kernel of mi355_sws_yuv2packed_X_a / _2_a / _1_a.  The context, the plan and the picture entry points are sws.hip's
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

typedef SwsPx32 Px32;                                   /* the sample type of these instances: one pixel */
static_assert(stage_bytes<Px32>() == STAGE_BYTES && stage_bytes<SwsPx32A>() == STAGE_BYTES, "the twins' staging lines");

template <int I, int DST> static void launch_generic32(dim3 grid, hipStream_t s, const SwsDev *d, const mi355_sws_frame *frames)
{
    constexpr SwsShape S = GENERIC_SHAPES[I];
    hipLaunchKernelGGL((k_sws_generic<S.lcap, S.ccap, sws_waves(sws_lds_bytes(S.lcap, S.ccap, STAGE_BYTES)), Px32, false, true, DST>), grid, dim3(NT), 0, s, d, frames);
}
template <int DST> static void launch_generic32(int i, dim3 grid, hipStream_t s, const SwsDev *d, const mi355_sws_frame *frames)
{
    if (i == 0) launch_generic32<0, DST>(grid, s, d, frames);
    else if (i == 1) launch_generic32<1, DST>(grid, s, d, frames);
    else launch_generic32<2, DST>(grid, s, d, frames);
}
/* the ALPHA form (a 32-bit destination that takes the source's alpha): the twin's LDS plus the alpha tile, as many lines as the luma tile —
 * A 19200 -> 26368 bytes, B 23296 -> 33536, C 26368 -> 38656: 6 / 4 / 4 workgroups a CU where the colour-only twins have 8 / 7 / 6 */
template <int I> static void launch_generic32a(dim3 grid, hipStream_t s, const SwsDev *d, const mi355_sws_frame *frames)
{
    constexpr SwsShape S = GENERIC_SHAPES[I];
    hipLaunchKernelGGL((k_sws_generic<S.lcap, S.ccap, sws_waves(sws_lds_bytes(S.lcap, S.ccap, STAGE_BYTES, true)), SwsPx32A, false, true, DST_RGB32>), grid, dim3(NT), 0, s, d, frames);
}
static_assert(sws_waves(sws_lds_bytes(GENERIC_SHAPES[0].lcap, GENERIC_SHAPES[0].ccap, STAGE_BYTES, true)) == 6 &&
              sws_waves(sws_lds_bytes(GENERIC_SHAPES[1].lcap, GENERIC_SHAPES[1].ccap, STAGE_BYTES, true)) == 4 &&
              sws_waves(sws_lds_bytes(GENERIC_SHAPES[2].lcap, GENERIC_SHAPES[2].ccap, STAGE_BYTES, true)) == 4, "workgroups per CU of the ALPHA instances");
void mi355_sws_launch_generic_rgb32(int i, int dst_format, int alpha, dim3 grid, hipStream_t s, const void *d, const mi355_sws_frame *frames)
{
    const SwsDev *dev = static_cast<const SwsDev *>(d);
    if (alpha) {
        if (i == 0) launch_generic32a<0>(grid, s, dev, frames);
        else if (i == 1) launch_generic32a<1>(grid, s, dev, frames);
        else launch_generic32a<2>(grid, s, dev, frames);
        return;
    }
    if (dst_format == 0) launch_generic32<DST_RGB24>(i, grid, s, dev, frames);
    else if (dst_format == MI355_SWS_DST_BGR24) launch_generic32<DST_BGR24>(i, grid, s, dev, frames);
    else launch_generic32<DST_RGB32>(i, grid, s, dev, frames);
}

/* form 0: three planes at CW = TW / 2, 1: at CW = TW, 2: a semi-planar destination; kind 0: plain, 1: RANGE, 2: DEEP (three planes only) */
template <int I, bool RANGE, bool DEEP> static void launch_planar32(int form, dim3 grid, hipStream_t s, const SwsDev *d, const mi355_sws_planar_frame *frames)
{
    constexpr SwsShape S = PLANAR_SHAPES[I];
    if (form == 0) hipLaunchKernelGGL((k_sws_planar<S.lcap, S.ccap, TW / 2, Px32, false, false, true, RANGE, DEEP>), grid, dim3(NT), 0, s, d, frames);
    else if (form == 1) hipLaunchKernelGGL((k_sws_planar<S.lcap, S.ccap, TW, Px32, false, false, true, RANGE, DEEP>), grid, dim3(NT), 0, s, d, frames);
    else if constexpr (!DEEP) hipLaunchKernelGGL((k_sws_planar<S.lcap, S.ccap, TW / 2, Px32, true, false, true, RANGE, false>), grid, dim3(NT), 0, s, d, frames);
}
template <int I> static void launch_planar32(int kind, int form, dim3 grid, hipStream_t s, const SwsDev *d, const mi355_sws_planar_frame *frames)
{
    if (kind == 0) launch_planar32<I, false, false>(form, grid, s, d, frames);
    else if (kind == 1) launch_planar32<I, true, false>(form, grid, s, d, frames);
    else launch_planar32<I, false, true>(form, grid, s, d, frames);
}
void mi355_sws_launch_planar_rgb32(int i, int kind, int form, dim3 grid, hipStream_t s, const void *d, const mi355_sws_planar_frame *frames)
{
    const SwsDev *dev = static_cast<const SwsDev *>(d);
    if (i == 0) launch_planar32<0>(kind, form, grid, s, dev, frames);
    else if (i == 1) launch_planar32<1>(kind, form, grid, s, dev, frames);
    else launch_planar32<2>(kind, form, grid, s, dev, frames);
}

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
void mi355_sws_launch_line_packed_a(int dst_format, hipStream_t s, const mi355_sws_luts *luts, int mode, const int16_t *lumF, const int16_t *l, int ls, const int16_t *chrF,
                                    const int16_t *u, const int16_t *v, int cs, const int16_t *a, int pitch, uint8_t *dest, int dstW, int yalpha, int uvalpha)
{
    hipLaunchKernelGGL(k_sws_line_packed_a, dim3(1), dim3(NT), 0, s, luts, mode, lumF, l, ls, chrF, u, v, cs, a, pitch, dest, dstW, yalpha, uvalpha, sws_rgb32_sel(dst_format));
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

/* one line through a line kernel: nsrc source bytes in, nout planes of `width` bytes out */
template <typename K, typename... A>
static void line32(K kernel, uint8_t *const out[], int nout, const uint8_t *src, size_t nsrc, int width, A... tail)
{
    Arena &a = arena();
    a.reserve(nsrc + (size_t)nout * (width + 32) + 64);
    const size_t o_src = a.take(nsrc);
    size_t o_d[2] = { 0, 0 };
    for (int p = 0; p < nout; p++) o_d[p] = a.take((size_t)width);
    std::memcpy(a.h<uint8_t>(o_src), src, nsrc);
    a.upload();
    if constexpr (sizeof...(A) == 2) hipLaunchKernelGGL(kernel, dim3(1), dim3(NT), 0, a.stream, a.d<uint8_t>(o_d[0]), a.d<uint8_t>(o_d[1]), a.d<const uint8_t>(o_src), width, tail...);
    else hipLaunchKernelGGL(kernel, dim3(1), dim3(NT), 0, a.stream, a.d<uint8_t>(o_d[0]), a.d<const uint8_t>(o_src), width, tail...);
    a.download();
    for (int p = 0; p < nout; p++) std::memcpy(out[p], a.h<uint8_t>(o_d[p]), (size_t)width);
}
extern "C" void mi355_sws_rgb32ToY(uint8_t *dst, const uint8_t *src, int width, int layout)
{
    if (width <= 0 || !sws_rgb32_src(layout)) return;
    line32(k_sws_line_rgb32_y, &dst, 1, src, (size_t)4 * width, width, layout);
}
extern "C" void mi355_sws_rgb32ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int layout, int half)
{
    if (width <= 0 || !sws_rgb32_src(layout)) return;
    uint8_t *const out[2] = { dstU, dstV };
    line32(k_sws_line_rgb32_uv, out, 2, src, (size_t)(half ? 8 : 4) * width, width, layout, half);
}
extern "C" void mi355_sws_rgb32ToA(uint8_t *dst, const uint8_t *src, int width, int layout)
{
    if (width <= 0 || !sws_rgb32_src(layout)) return;
    line32(k_sws_line_rgb32_a, &dst, 1, src, (size_t)4 * width, width, layout);
}
