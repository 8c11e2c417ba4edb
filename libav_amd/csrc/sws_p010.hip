/*
 * sws_p010.hip — P010 SOURCES (p010le: MI355_SWS_SRC_P010): the instances of the tile kernels (sws_dev.h) whose horizontal pass makes its 16-bit samples
 * from a plane of words and a plane of word pairs, word >> 6 (hscale_tile_p010: p010LEToY_c / p010LEToUV_c, input.c:499-524, in the staging round, in
 * front of the 16-bit line loops with depth 10) — k_sws_generic A / B / C to rgb24, bgr24, the four 32-bit orders and the three packed 4:2:2 orders,
 * k_sws_planar A / B / C at both chroma widths, plain, SEMI, RANGE and DEEP: every key of source class SWS_SRC_P010 (sws_dev.h: SwsKey; the key is
 * sws.hip's) — with their launch, and the two Tier-1 line entries mi355_sws_p010ToY / _p010ToUV with their line kernels.  The reference has no unscaled
 * converter from P010 and a 10-bit context is never k_sws_ident1's: every P010 context runs a tile kernel.  The context, the plan and the picture entry
 * points are sws.hip's (mi355_sws_create_src_layout with layout 24).  A file of its own so that it compiles beside sws.hip, not behind it.
 */
#include "mi355_rt.h"
#define MI355_SWS_TILE_KERNELS_ONLY
#include "sws_dev.h"
#include "../../include/mi355dsp.h"

using namespace mi355;

/* the samples are staged as 16-bit values in the 16-bit instances' staging lines, the pair plane de-interleaved into two lines of the chroma geometry:
 * every instance has the LDS, the waves per SIMD and the workgroups per CU of its yuv420p10le twin */
static_assert(sizeof(SwsPxP010) == 2 && stage_bytes<SwsPxP010>() == STAGE_BYTES16, "the twins' staging lines");
static_assert(2 * StageGeom<TW / 2, uint16_t>::PITCH * (StageGeom<TW / 2, uint16_t>::LINES / 2) * 4 <= STAGE_BYTES16 &&
              2 * StageGeom<TW, uint16_t>::PITCH * (StageGeom<TW, uint16_t>::LINES / 2) * 4 <= STAGE_BYTES16, "U and V lines of a round fit the staging storage");

namespace {
/* ---- Tier-1 line kernels: p010LEToY_c / p010LEToUV_c (input.c:499-524) of one line; nbytes: 2 * width, the bytes of an output line ---------------- */
__global__ void __launch_bounds__(NT) k_sws_line_p010_y(uint8_t *dst, const uint8_t *src, int nbytes)
{
    const uint16_t *s = reinterpret_cast<const uint16_t *>(src);
    uint16_t *d = reinterpret_cast<uint16_t *>(dst);
    for (int i = threadIdx.x; i < (nbytes >> 1); i += NT) d[i] = (uint16_t)(s[i] >> 6);
}
__global__ void __launch_bounds__(NT) k_sws_line_p010_uv(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int nbytes)
{
    const uint16_t *s = reinterpret_cast<const uint16_t *>(src);
    uint16_t *u = reinterpret_cast<uint16_t *>(dstU), *v = reinterpret_cast<uint16_t *>(dstV);
    for (int i = threadIdx.x; i < (nbytes >> 1); i += NT) { u[i] = (uint16_t)(s[2 * i] >> 6); v[i] = (uint16_t)(s[2 * i + 1] >> 6); }
}
}  // namespace

bool mi355_sws_launch_p010(const SwsKey &key, const SwsOperands &op)
{
    if (key.src != SWS_SRC_P010 || key.alpha || (key.kernel != SWS_KERNEL_GENERIC && key.kernel != SWS_KERNEL_PLANAR)) return false;
    return sws_launch<sws_bit(SWS_SRC_P010), SWS_ALL_KINDS, SWS_ALL_DSTS | sws_bit(DST_YUY2)>(key, op);
}

/* the line entries take host pointers at any address: the staging arena's copies are aligned (sws_line), the words are little endian */
extern "C" void mi355_sws_p010ToY(uint16_t *dst, const uint8_t *src, int width)
{
    if (width <= 0) return;
    uint8_t *out = reinterpret_cast<uint8_t *>(dst);
    sws_line<1>(k_sws_line_p010_y, &out, src, (size_t)2 * width, 2 * width);
}
extern "C" void mi355_sws_p010ToUV(uint16_t *dstU, uint16_t *dstV, const uint8_t *src, int width)
{
    if (width <= 0) return;
    uint8_t *const out[2] = { reinterpret_cast<uint8_t *>(dstU), reinterpret_cast<uint8_t *>(dstV) };
    sws_line<2>(k_sws_line_p010_uv, out, src, (size_t)4 * width, 2 * width);
}
