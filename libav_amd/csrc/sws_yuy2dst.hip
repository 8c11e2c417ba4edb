/*
 * sws_yuy2dst.hip — packed 4:2:2 DESTINATIONS (yuyv422 / uyvy422 / yvyu422: MI355_SWS_DST_YUYV422 ... _YVYU422): the DST_YUY2 instances of the packed
 * kernels (sws_dev.h) — k_sws_generic A / B / C from every source class (three planes of bytes or of 16-bit samples, NV12 / NV21, rgb24 / bgr24, the four
 * 32-bit orders, the three packed 4:2:2 orders), k_sws_ident1 in its _1 and X forms from three planes and from NV12 / NV21, k_sws_ident1_yuy2, and the
 * line kernel k_sws_line_packed behind mi355_sws_yuv2packed_X / _2 / _1: every key whose dst is DST_YUY2 (sws_dev.h: SwsKey; the key is sws.hip's) —
 * with their launch, and the reference's four unscaled packers in one kernel (k_sws_yuy2_pack: yuv422pToYuy2Wrapper, yuv422pToUyvyWrapper,
 * planarToYuy2Wrapper, planarToUyvyWrapper, swscale_unscaled.c:179-225 over yuvPlanartoyuy2_c / yuvPlanartouyvy_c, rgb2rgb_template.c:364-476).  The
 * context, the plan and the picture entry points are sws.hip's (dst_format 48 .. 50).  A file of its own so that it compiles beside the others, not
 * behind them.
 */
#include "mi355_rt.h"
#define MI355_SWS_TILE_KERNELS_ONLY
#include "sws_dev.h"
#include "../../include/mi355dsp.h"

using namespace mi355;

namespace {
/* the form has no table in LDS: a workgroup's tile is smaller by sizeof(LutLds), and the waves per SIMD follow it */
static_assert(sws_lds_bytes(28, 16, STAGE_BYTES, false, false) == sws_lds_bytes(28, 16) - (int)sizeof(LutLds), "no LUT in the tile of this form");
static_assert(sws_waves(sws_lds_bytes(GENERIC_SHAPES[0].lcap, GENERIC_SHAPES[0].ccap, STAGE_BYTES, false, false)) == 8 &&
              sws_waves(sws_lds_bytes(GENERIC_SHAPES[1].lcap, GENERIC_SHAPES[1].ccap, STAGE_BYTES, false, false)) == 8 &&
              sws_waves(sws_lds_bytes(GENERIC_SHAPES[2].lcap, GENERIC_SHAPES[2].ccap, STAGE_BYTES, false, false)) == 7, "workgroups per CU of the 8-bit instances");
static_assert(dst_bpp<DST_YUY2>() == 2 && MAXTH * TW * dst_bpp<DST_YUY2>() <= STAGE_BYTES, "the rows of a tile fit the staging lines");

/* ---- the unscaled packer: 8-bit yuv422p / yuv420p -> yuyv422 / uyvy422 at equal size ---------------------------------------------------------
 * Every byte is a pick: group g of row y is Y[2g] U[g] Y[2g + 1] V[g] (uyvy: U[g] Y[2g] V[g] Y[2g + 1]) with the chroma of row y >> vsub (the
 * reference's vertLumPerChroma: a 4:2:0 chroma row serves two rows, no interpolation).  The reference's loop writes two groups a step,
 * G = 2 * ceil((srcW >> 1) / 2) of them on a row; here min(G, (srcW + 1) >> 1) — `groups` — so that nothing is written behind the row: with
 * srcW % 4 == 3 the last group's second luma byte is the source byte at x = srcW, as the reference reads it; with srcW % 4 == 1 the last pixel stays
 * untouched; with srcW % 4 == 2 the reference's extra group behind the row is not reproduced.
 * Tiled like k_sws_nv12_pack: YPACK_COLS x YPACK_ROWS luma samples a workgroup (blockIdx.z: the picture); a thread takes eight luma samples — four
 * groups, 16 destination bytes — of four rows, every load requested before the first store, so that a wave's store of a row is ONE contiguous
 * kilobyte.  8 + 4 + 4 source bytes become one 16-byte store (two byte zips) where all four groups lie inside `groups` and the width, the destination's
 * pointer and stride are multiples of 16, the luma plane's of 8 and the chroma planes' of 4; otherwise group by group, byte by byte. */
constexpr int YPACK_COLS = 512, YPACK_ROWS = 16;
static_assert(YPACK_COLS == 64 * 8 && YPACK_ROWS % (NT / 64) == 0, "a wave covers a tile row, the waves share the tile's rows");

__global__ void __launch_bounds__(NT) k_sws_yuy2_pack(int srcW, int srcH, int vsub, int uyvy, const mi355_sws_frame *frames)
{
    mi355_sws_frame fr = frames[blockIdx.z];
    for (int k = 0; k < 3; k++) fr.src[k] = mi355_global(fr.src[k]);
    fr.dst = mi355_global(fr.dst);
    const int tid = threadIdx.x, lane = tid & 63, rg = tid >> 6;
    const int x = blockIdx.x * YPACK_COLS + 8 * lane, y0 = blockIdx.y * YPACK_ROWS, g0 = x >> 1;
    const int groups = imin(2 * (((srcW >> 1) + 1) >> 1), (srcW + 1) >> 1);
    const int n = imin(4, groups - g0);                            /* the thread's groups (none: n <= 0) */
    const bool wide = n == 4 && x + 8 <= srcW && ((reinterpret_cast<uintptr_t>(fr.dst) | (uintptr_t)fr.dst_stride) & 15) == 0 &&
                      ((reinterpret_cast<uintptr_t>(fr.src[0]) | (uintptr_t)fr.src_stride[0]) & 7) == 0 &&
                      ((reinterpret_cast<uintptr_t>(fr.src[1]) | (uintptr_t)fr.src_stride[1] | reinterpret_cast<uintptr_t>(fr.src[2]) | (uintptr_t)fr.src_stride[2]) & 3) == 0;
    constexpr int NR = YPACK_ROWS / (NT / 64);
    sws_u32x2 l[NR] = {};
    uint32_t u[NR] = {}, v[NR] = {};
#pragma unroll
    for (int k = 0; k < NR; k++) {
        const int y = y0 + rg + k * (NT / 64);
        if (wide && y < srcH) {
            l[k] = *reinterpret_cast<const sws_u32x2 *>(fr.src[0] + (size_t)y * fr.src_stride[0] + x);
            u[k] = *reinterpret_cast<const uint32_t *>(fr.src[1] + (size_t)(y >> vsub) * fr.src_stride[1] + g0);
            v[k] = *reinterpret_cast<const uint32_t *>(fr.src[2] + (size_t)(y >> vsub) * fr.src_stride[2] + g0);
        }
    }
#pragma unroll
    for (int k = 0; k < NR; k++) {
        const int y = y0 + rg + k * (NT / 64);
        if (y >= srcH || n <= 0) continue;
        uint8_t *d = fr.dst + (size_t)y * fr.dst_stride + 4 * (size_t)g0;
        if (wide) {
            /* U0 V0 U1 V1 ..., then luma and chroma byte by byte: Y0 U0 Y1 V0 ... (uyvy: the other way round) */
            const uint32_t c0 = sws_zip_lo(u[k], v[k]), c1 = sws_zip_hi(u[k], v[k]);
            *reinterpret_cast<sws_u32x4 *>(d) = uyvy ? sws_u32x4{ sws_zip_lo(c0, l[k][0]), sws_zip_hi(c0, l[k][0]), sws_zip_lo(c1, l[k][1]), sws_zip_hi(c1, l[k][1]) }
                                                     : sws_u32x4{ sws_zip_lo(l[k][0], c0), sws_zip_hi(l[k][0], c0), sws_zip_lo(l[k][1], c1), sws_zip_hi(l[k][1], c1) };
        } else {
            const uint8_t *py = fr.src[0] + (size_t)y * fr.src_stride[0] + x;
            const uint8_t *pu = fr.src[1] + (size_t)(y >> vsub) * fr.src_stride[1] + g0, *pv = fr.src[2] + (size_t)(y >> vsub) * fr.src_stride[2] + g0;
            for (int g = 0; g < n; g++) {
                const uint8_t y1 = py[2 * g], y2 = py[2 * g + 1], cu = pu[g], cv = pv[g];      /* (py[2g + 1] of the last group of srcW % 4 == 3: the byte at x = srcW) */
                if (uyvy) { d[4 * g] = cu; d[4 * g + 1] = y1; d[4 * g + 2] = cv; d[4 * g + 3] = y2; }
                else { d[4 * g] = y1; d[4 * g + 1] = cu; d[4 * g + 2] = y2; d[4 * g + 3] = cv; }
            }
        }
    }
}
}  // namespace

bool mi355_sws_launch_yuy2dst(const SwsKey &key, const SwsOperands &op)
{
    if (key.dst != DST_YUY2 || key.alpha) return false;
    const SwsDev *dev = static_cast<const SwsDev *>(op.d);
    const mi355_sws_frame *frames = static_cast<const mi355_sws_frame *>(op.frames);
    if (key.kernel == SWS_KERNEL_YUY2_PACK) {
        /* the kernel's own grid (op.grid.z: the pictures); the chroma shift of the source, the order of the destination */
        const SwsDev &h = *static_cast<const SwsDev *>(op.h);
        hipLaunchKernelGGL(k_sws_yuy2_pack, dim3((h.srcW + YPACK_COLS - 1) / YPACK_COLS, (h.srcH + YPACK_ROWS - 1) / YPACK_ROWS, op.grid.z), dim3(NT), 0, op.s,
                           h.srcW, h.srcH, h.src_vsub, h.packed == MI355_SWS_DST_UYVY422 ? 1 : 0, frames);
        return true;
    }
    if (key.kernel == SWS_KERNEL_LINE) {
        const SwsLine &n = *op.line;
        hipLaunchKernelGGL(k_sws_line_packed<DST_YUY2>, dim3(1), dim3(NT), 0, op.s, n.luts, n.mode, n.lumF, n.l, n.ls, n.chrF, n.u, n.v, n.cs, n.pitch, n.dest, n.dstW,
                           n.yalpha, n.uvalpha, op.sel);
        return true;
    }
    if (key.src == SWS_SRC_YUY2 && key.kernel == SWS_KERNEL_IDENT1_1) {
        hipLaunchKernelGGL(k_sws_ident1_yuy2<DST_YUY2>, op.grid, dim3(NT), 0, op.s, dev, frames);
        return true;
    }
    /* the tile kernel from every source class, k_sws_ident1 from three planes of bytes and from NV12 / NV21 */
    constexpr unsigned ALL_SRCS = SWS_CLASSIC_SRCS | sws_bit(SWS_SRC_RGB32) | sws_bit(SWS_SRC_YUY2);
    if (key.kernel != SWS_KERNEL_GENERIC && key.kernel != SWS_KERNEL_IDENT1_1 && key.kernel != SWS_KERNEL_IDENT1_X) return false;
    return sws_launch<ALL_SRCS, 0u, sws_bit(DST_YUY2)>(key, op);
}
