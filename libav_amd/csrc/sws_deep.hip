/*
 * sws_deep.hip — the DEEP instances of k_sws_planar (sws_dev.h): planar yuv420p / yuv422p / yuv444p destinations of 9 or 10 bits
 * (yuv420p9le ... yuv444p10le), from every source the 8-bit planar destinations take.  The launches only: the context, the plan and the
 * entry points are sws.hip's (mi355_sws_create_src_layout_range_depth, mi355_sws_scale_planar_frames_dev).  A file of its own so that
 * the 24 instances compile beside sws.hip, not behind it.
 */
#include "mi355_rt.h"
#define MI355_SWS_TILE_KERNELS_ONLY
#include "sws_dev.h"

/* instance I (0 / 1 / 2: A / B / C) for samples of type ST / an NV12 / NV21 / a packed RGB source: the LDS, and so the waves per SIMD, of the
 * 8-bit destination's instance of the same source (sws_planar_waves, unchanged) */
template <int I, typename ST, bool NV, bool RGB> static void launch_deep(int full_cw, dim3 grid, hipStream_t s, const SwsDev *d, const mi355_sws_planar_frame *frames)
{
    constexpr SwsShape S = PLANAR_SHAPES[I];
    if (full_cw) hipLaunchKernelGGL((k_sws_planar<S.lcap, S.ccap, TW, ST, false, NV, RGB, false, true>), grid, dim3(NT), 0, s, d, frames);
    else hipLaunchKernelGGL((k_sws_planar<S.lcap, S.ccap, TW / 2, ST, false, NV, RGB, false, true>), grid, dim3(NT), 0, s, d, frames);
}
template <int I> static void launch_deep(int src, int full_cw, dim3 grid, hipStream_t s, const SwsDev *d, const mi355_sws_planar_frame *frames)
{
    if (src == 0) launch_deep<I, uint8_t, false, false>(full_cw, grid, s, d, frames);
    else if (src == 1) launch_deep<I, uint16_t, false, false>(full_cw, grid, s, d, frames);
    else if (src == 2) launch_deep<I, uint8_t, true, false>(full_cw, grid, s, d, frames);
    else launch_deep<I, uint8_t, false, true>(full_cw, grid, s, d, frames);
}
void mi355_sws_launch_planar_deep(int i, int src, int full_cw, dim3 grid, hipStream_t s, const void *d, const mi355_sws_planar_frame *frames)
{
    const SwsDev *dev = static_cast<const SwsDev *>(d);
    if (i == 0) launch_deep<0>(src, full_cw, grid, s, dev, frames);
    else if (i == 1) launch_deep<1>(src, full_cw, grid, s, dev, frames);
    else launch_deep<2>(src, full_cw, grid, s, dev, frames);
}
