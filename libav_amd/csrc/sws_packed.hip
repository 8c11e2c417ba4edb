/*
 * sws_packed.hip — the DST_BGR24 and DST_RGB32 instances of the packed kernels (sws_dev.h): bgr24 and rgba / bgra / argb / abgr destinations of
 * k_sws_generic, k_sws_ident1, k_sws_c24 and of the line kernel, from every source the rgb24 destination takes.  The launches only: the context, the
 * plan and the entry points are sws.hip's (mi355_sws_create_src_layout_range_depth with MI355_SWS_DST_BGR24 ... _ABGR, mi355_sws_scale_frames_dev,
 * mi355_sws_yuv2packed_X / _2 / _1, mi355_sws_yuv2rgb_c).  A file of its own so that the instances compile beside sws.hip, not behind it.
 *
 * Two forms, not five: bgr24 is the rgb24 text with the r and b row offsets exchanged; the four 32-bit orders are one form whose byte selector
 * comes from the context.  Every instance has the LDS of its rgb24 twin (the narrow form's output rows reuse the staging lines: nine rows of
 * TW * 4 bytes in the 4864 bytes where rgb24 has twelve of TW * 3), so the same waves per SIMD and workgroups per CU:
 *   k_sws_generic A / B / C   8-bit, NV and RGB sources 8 / 7 / 6 workgroups a CU, 16-bit sources 7 / 5 / 5 (generic_waves in sws.hip)
 *   k_sws_ident1, k_sws_c24   the 3072 bytes of the tables, as the twins
 */
#include "mi355_rt.h"
#define MI355_SWS_TILE_KERNELS_ONLY
#include "sws_dev.h"

/* instance I (0 / 1 / 2: A / B / C) of k_sws_generic for samples of type ST / an NV12 / NV21 / a packed RGB source, destination form DST: the
 * waves per SIMD are those of the twin's LDS (sws_lds_bytes does not depend on DST) */
template <int I, typename ST, bool NV, bool RGB, int DST> static void launch_generic(dim3 grid, hipStream_t s, const SwsDev *d, const mi355_sws_frame *frames)
{
    constexpr SwsShape S = GENERIC_SHAPES[I];
    hipLaunchKernelGGL((k_sws_generic<S.lcap, S.ccap, sws_waves(sws_lds_bytes(S.lcap, S.ccap, stage_bytes<ST>())), ST, NV, RGB, DST>), grid, dim3(NT), 0, s, d, frames);
}
template <int I, int DST> static void launch_generic(int src, dim3 grid, hipStream_t s, const SwsDev *d, const mi355_sws_frame *frames)
{
    if (src == 0) launch_generic<I, uint8_t, false, false, DST>(grid, s, d, frames);
    else if (src == 1) launch_generic<I, uint16_t, false, false, DST>(grid, s, d, frames);
    else if (src == 2) launch_generic<I, uint8_t, true, false, DST>(grid, s, d, frames);
    else launch_generic<I, uint8_t, false, true, DST>(grid, s, d, frames);
}
template <int DST> static void launch_packed(int k, int src, uint32_t sel, dim3 grid, hipStream_t s, const SwsDev *d, int dstW, int sliceH, const mi355_sws_frame *frames)
{
    if (k == MI355_SWS_K_C24) {
        typename C24Arg<DST>::type slice{};                     /* the slice starts at row 0; a 32-bit form: with the order's selector */
        if constexpr (DST == DST_RGB32) slice.sel = sel;
        if (src) hipLaunchKernelGGL((k_sws_c24<1, DST>), grid, dim3(NT), 0, s, &d->luts, dstW, sliceH, slice, frames);      /* yuv422p: every other chroma line */
        else hipLaunchKernelGGL((k_sws_c24<0, DST>), grid, dim3(NT), 0, s, &d->luts, dstW, sliceH, slice, frames);
    } else if (k == MI355_SWS_K_IDENT1_1) {
        if (src == 2) hipLaunchKernelGGL((k_sws_ident1<false, true, DST>), grid, dim3(NT), 0, s, d, frames);
        else hipLaunchKernelGGL((k_sws_ident1<false, false, DST>), grid, dim3(NT), 0, s, d, frames);
    } else if (k == MI355_SWS_K_IDENT1_X) {
        if (src == 2) hipLaunchKernelGGL((k_sws_ident1<true, true, DST>), grid, dim3(NT), 0, s, d, frames);
        else hipLaunchKernelGGL((k_sws_ident1<true, false, DST>), grid, dim3(NT), 0, s, d, frames);
    } else if (k == MI355_SWS_K_GENERIC_A) launch_generic<0, DST>(src, grid, s, d, frames);
    else if (k == MI355_SWS_K_GENERIC_B) launch_generic<1, DST>(src, grid, s, d, frames);
    else launch_generic<2, DST>(src, grid, s, d, frames);
}
void mi355_sws_launch_packed(int k, int src, int dst_format, dim3 grid, hipStream_t s, const void *d, int dstW, int sliceH, const mi355_sws_frame *frames)
{
    const SwsDev *dev = static_cast<const SwsDev *>(d);
    if (dst_format == MI355_SWS_DST_BGR24) launch_packed<DST_BGR24>(k, src, 0, grid, s, dev, dstW, sliceH, frames);
    else launch_packed<DST_RGB32>(k, src, sws_rgb32_sel(dst_format), grid, s, dev, dstW, sliceH, frames);
}

void mi355_sws_launch_line_packed(int dst_format, hipStream_t s, const mi355_sws_luts *luts, int mode, const int16_t *lumF, const int16_t *l, int ls, const int16_t *chrF,
                                  const int16_t *u, const int16_t *v, int cs, int pitch, uint8_t *dest, int dstW, int yalpha, int uvalpha)
{
    if (dst_format == MI355_SWS_DST_BGR24)
        hipLaunchKernelGGL(k_sws_line_packed<DST_BGR24>, dim3(1), dim3(NT), 0, s, luts, mode, lumF, l, ls, chrF, u, v, cs, pitch, dest, dstW, yalpha, uvalpha, 0u);
    else
        hipLaunchKernelGGL(k_sws_line_packed<DST_RGB32>, dim3(1), dim3(NT), 0, s, luts, mode, lumF, l, ls, chrF, u, v, cs, pitch, dest, dstW, yalpha, uvalpha,
                           sws_rgb32_sel(dst_format));
}

void mi355_sws_launch_c24_slice(int dst_format, dim3 grid, hipStream_t s, const mi355_sws_luts *luts, int dstW, int rows, const mi355_sws_frame *frames)
{
    if (dst_format == MI355_SWS_DST_BGR24) hipLaunchKernelGGL((k_sws_c24<0, DST_BGR24>), grid, dim3(NT), 0, s, luts, dstW, rows, 0, frames);
    else hipLaunchKernelGGL((k_sws_c24<0, DST_RGB32>), grid, dim3(NT), 0, s, luts, dstW, rows, C24Slice{ 0, sws_rgb32_sel(dst_format) }, frames);
}
