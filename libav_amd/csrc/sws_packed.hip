/*
 * sws_packed.hip — the DST_BGR24 and DST_RGB32 instances of the packed kernels (sws_dev.h): bgr24 and rgba / bgra / argb / abgr destinations of
 * k_sws_generic, k_sws_ident1, k_sws_c24 and of the line kernel, from the four classic source classes.  The launch only: the context, the plan, the
 * key (sws_dev.h: SwsKey) and the entry points are sws.hip's (mi355_sws_create_src_layout_range_depth with MI355_SWS_DST_BGR24 ... _ABGR,
 * mi355_sws_scale_frames_dev, mi355_sws_yuv2packed_X / _2 / _1, mi355_sws_yuv2rgb_c).  A file of its own so that the instances compile beside
 * sws.hip, not behind it.
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

constexpr unsigned PACKED_DSTS = sws_bit(DST_BGR24) | sws_bit(DST_RGB32);

bool mi355_sws_launch_packed(const SwsKey &key, const SwsOperands &op)
{
    if (key.kernel != SWS_KERNEL_LINE) return sws_launch<SWS_CLASSIC_SRCS, 0, PACKED_DSTS>(key, op);
    /* one line, one workgroup (the ALPHA form is sws_rgb32.hip's) */
    if (key.alpha) return false;
    return sws_pick_dst(key.dst, [&](auto dst) {
        constexpr int DST = decltype(dst)::value;
        if constexpr ((PACKED_DSTS & sws_bit(DST)) == 0) return false;
        else {
            const SwsLine &n = *op.line;
            hipLaunchKernelGGL(k_sws_line_packed<DST>, dim3(1), dim3(NT), 0, op.s, n.luts, n.mode, n.lumF, n.l, n.ls, n.chrF, n.u, n.v, n.cs, n.pitch, n.dest, n.dstW, n.yalpha,
                               n.uvalpha, op.sel);
            return true;
        }
    });
}
