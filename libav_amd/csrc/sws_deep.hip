/*
 * sws_deep.hip — the DEEP instances of k_sws_planar (sws_dev.h): planar yuv420p / yuv422p / yuv444p destinations of 9 or 10 bits
 * (yuv420p9le ... yuv444p10le), from the four classic source classes (three planes of 8- or 16-bit samples, NV12 / NV21, rgb24 / bgr24).  The launch
 * only: the context, the plan, the key (sws_dev.h: SwsKey) and the entry points are sws.hip's.  A file of its own so that the 24 instances compile
 * beside sws.hip, not behind it.  Every instance has the LDS, and so the waves per SIMD, of the 8-bit destination's instance of the same source.
 */
#include "mi355_rt.h"
#define MI355_SWS_TILE_KERNELS_ONLY
#include "sws_dev.h"

bool mi355_sws_launch_deep(const SwsKey &key, const SwsOperands &op)
{
    return sws_launch<SWS_CLASSIC_SRCS, sws_bit(SWS_KIND_DEEP), 0>(key, op);
}
