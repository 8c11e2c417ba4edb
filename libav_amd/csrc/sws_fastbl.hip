/*
 * sws_fastbl.hip — SWS_FAST_BILINEAR contexts of 8-bit planar sources (mi355_sws_create_fast_bilinear): the instances of the two tile kernels whose
 * horizontal pass reads no filter bank (sws_dev.h: hscale_tile_fbl, k_sws_fbl_generic, k_sws_fbl_planar — hyscale_fast_c / hcscale_fast_c,
 * swscale.c:238-249, :288-301, every position and weight from one 16.16 increment) — k_sws_fbl_generic A / B / C to rgb24, bgr24, the four 32-bit
 * orders and the three packed 4:2:2 orders (12 instances), k_sws_fbl_planar A / B / C at both chroma widths, plain, SEMI, RANGE and DEEP (24) — with
 * their launch, and the two Tier-1 line entries mi355_sws_hyscale_fast / _hcscale_fast with their line kernel.  The range step and the vertical pass
 * are the device functions of k_sws_generic / k_sws_planar; those kernels gain no instance here.  The context, the plan and the picture entry points
 * are sws.hip's.  A file of its own so that it compiles beside sws.hip, not behind it.
 */
#include "mi355_rt.h"
#define MI355_SWS_TILE_KERNELS_ONLY
#include "sws_dev.h"
#include "../../include/mi355dsp.h"

using namespace mi355;

/* every instance has the LDS of its bank-driven twin of the 8-bit three-plane source: the same tiles, the 8-bit staging lines */
static_assert(StageGeom<TW>::PITCH * StageGeom<TW>::LINES * 4 <= STAGE_BYTES && StageGeom<TW / 2>::PITCH * StageGeom<TW / 2>::LINES * 4 <= STAGE_BYTES,
              "a round of either tile width fits the twins' staging storage");

namespace {
/* ---- Tier-1 line kernel: hyscale_fast_c (chroma 0) / one plane of hcscale_fast_c (chroma 1) of one line; nbytes: 2 * dstWidth ------------------- */
__global__ void __launch_bounds__(NT) k_sws_line_fbl(uint8_t *dst, const uint8_t *src, int nbytes, uint32_t xinc, int chroma)
{
    int16_t *d = reinterpret_cast<int16_t *>(dst);
    for (int i = threadIdx.x; i < (nbytes >> 1); i += NT) {
        const uint32_t xpos = (uint32_t)i * xinc;
        const int xx = (int)(xpos >> 16), a = (int)((xpos & 0xFFFFu) >> 9);
        d[i] = (int16_t)(chroma ? fbl_blend<true>(src[xx], src[xx + 1], a) : fbl_blend<false>(src[xx], src[xx + 1], a));
    }
}
/* the bytes of a line the reference's loop reads: up to xx + 1 of the last sample (positions never decrease) */
size_t fbl_line_bytes(int dstWidth, int xInc) { return (size_t)(((uint32_t)(dstWidth - 1) * (uint32_t)xInc) >> 16) + 2; }
/* the loops take any xInc the reference's would; a position that does not fit 32 bits wraps there too and is not ours */
bool fbl_line_ok(int dstWidth, int xInc) { return dstWidth > 0 && xInc > 0 && (uint64_t)(dstWidth - 1) * (uint64_t)xInc <= 0xFFFFFFFFull; }
}  // namespace

bool mi355_sws_launch_fastbl(const SwsKey &key, const SwsOperands &op)
{
    if (key.src != SWS_SRC_P8 || key.alpha) return false;
    const SwsDev *d = static_cast<const SwsDev *>(op.d);
    if (key.kernel == SWS_KERNEL_PLANAR) {
        const mi355_sws_planar_frame *fr = static_cast<const mi355_sws_planar_frame *>(op.frames);
        return sws_pick<SwsKind, SWS_KIND_PLAIN, SWS_KIND_RANGE, SWS_KIND_DEEP>(key.kind, [&](auto kind) {
            constexpr SwsKind K = decltype(kind)::value;
            return sws_pick<SwsForm, SWS_FORM_HALF, SWS_FORM_FULL, SWS_FORM_SEMI>(key.form, [&](auto form) {
                constexpr SwsForm F = decltype(form)::value;
                if constexpr (K == SWS_KIND_DEEP && F == SWS_FORM_SEMI) return false;
                else return sws_pick_instance(key.i, [&](auto i) {
                    constexpr SwsShape S = PLANAR_SHAPES[decltype(i)::value];
                    hipLaunchKernelGGL((k_sws_fbl_planar<S.lcap, S.ccap, F == SWS_FORM_FULL ? TW : TW / 2, F == SWS_FORM_SEMI, K == SWS_KIND_RANGE, K == SWS_KIND_DEEP>),
                                       op.grid, dim3(NT), 0, op.s, d, op.lum_inc, op.chr_inc, fr);
                    return true;
                });
            });
        });
    }
    if (key.kernel != SWS_KERNEL_GENERIC) return false;
    const mi355_sws_frame *fr = static_cast<const mi355_sws_frame *>(op.frames);
    return sws_pick_dst(key.dst, [&](auto dst) {
        constexpr int DST = decltype(dst)::value;
        return sws_pick_instance(key.i, [&](auto i) {
            constexpr SwsShape S = GENERIC_SHAPES[decltype(i)::value];
            hipLaunchKernelGGL((k_sws_fbl_generic<S.lcap, S.ccap, sws_waves(sws_lds_bytes(S.lcap, S.ccap, STAGE_BYTES, false, DST != DST_YUY2)), DST>), op.grid, dim3(NT), 0,
                               op.s, d, op.lum_inc, op.chr_inc, fr);
            return true;
        });
    });
}

/* the line entries take host pointers at any address (the staging arena's copies are aligned: sws_line) and read what the reference's loops read:
 * ((dstWidth - 1) * xInc >> 16) + 2 bytes of each source line, whatever srcW says */
extern "C" void mi355_sws_hyscale_fast(int16_t *dst, int dstWidth, const uint8_t *src, int srcW, int xInc)
{
    (void)srcW;
    if (!fbl_line_ok(dstWidth, xInc)) return;
    uint8_t *out = reinterpret_cast<uint8_t *>(dst);
    sws_line<1>(k_sws_line_fbl, &out, src, fbl_line_bytes(dstWidth, xInc), 2 * dstWidth, (uint32_t)xInc, 0);
}
extern "C" void mi355_sws_hcscale_fast(int16_t *dst1, int16_t *dst2, int dstWidth, const uint8_t *src1, const uint8_t *src2, int srcW, int xInc)
{
    (void)srcW;
    if (!fbl_line_ok(dstWidth, xInc)) return;
    uint8_t *out1 = reinterpret_cast<uint8_t *>(dst1), *out2 = reinterpret_cast<uint8_t *>(dst2);
    sws_line<1>(k_sws_line_fbl, &out1, src1, fbl_line_bytes(dstWidth, xInc), 2 * dstWidth, (uint32_t)xInc, 1);
    sws_line<1>(k_sws_line_fbl, &out2, src2, fbl_line_bytes(dstWidth, xInc), 2 * dstWidth, (uint32_t)xInc, 1);
}
