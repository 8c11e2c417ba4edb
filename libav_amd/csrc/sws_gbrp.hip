/*
 * sws_gbrp.hip — planar RGB (gbrp) DESTINATIONS (mi355_sws_create_gbrp): the instances of k_sws_gbrp (sws_dev.h: k_sws_planar's FULL tile up to the
 * barrier, then gbrp_rows — the reference's yuv2gbrp_full_X_c, output.c:1275-1355: both banks in their X form, six integer coefficients in place of the
 * LUTs, the sums modulo 2^32) — one for each of the seven source classes at A / B / C (21 instances), with their launch, and the Tier-1 line entry
 * mi355_sws_yuv2gbrp_full_X with its line kernel.  The staging rounds are the device functions of k_sws_planar; that kernel gains no instance here.
 * The context, the plan and the picture entry points are sws.hip's.  A file of its own so that it compiles beside sws.hip, not behind it.
 */
#include "mi355_rt.h"
#define MI355_SWS_TILE_KERNELS_ONLY
#include "sws_dev.h"
#include "../../include/mi355dsp.h"

using namespace mi355;

namespace {
/* ---- Tier-1 line kernel: yuv2gbrp_full_X_c of one line; the ls luma and cs chroma lines lie `pitch` samples apart ------------------------------- */
__global__ void __launch_bounds__(NT) k_sws_line_gbrp(mi355_sws_rgb_coefs k, const int16_t *lumF, const int16_t *l, int ls, const int16_t *chrF, const int16_t *u,
                                                      const int16_t *v, int cs, int pitch, uint8_t *dg, uint8_t *db, uint8_t *dr, int dstW)
{
    for (int i = threadIdx.x; i < dstW; i += NT) {
        int Y = GBRP_LUM_SEED, U = GBRP_CHR_SEED, V = GBRP_CHR_SEED;
        for (int j = 0; j < ls; j++) Y += l[(size_t)j * pitch + i] * lumF[j];
        for (int j = 0; j < cs; j++) { U += u[(size_t)j * pitch + i] * chrF[j]; V += v[(size_t)j * pitch + i] * chrF[j]; }
        uint32_t g, b, r;
        gbrp_pixel(k, Y >> 10, U >> 10, V >> 10, g, b, r);
        dg[i] = (uint8_t)g; db[i] = (uint8_t)b; dr[i] = (uint8_t)r;
    }
}

template <int I, SwsSrcClass C> void launch_gbrp(const SwsOperands &op)
{
    constexpr SwsShape S = PLANAR_SHAPES[I];
    typedef typename SwsSrc<C>::ST ST;
    /* the LDS and the workgroups per CU of the yuv444p twin's instance */
    static_assert(sizeof(int16_t) * (S.lcap * TW + S.ccap * 2 * TW) + stage_bytes<ST>() == sws_planar_lds_bytes(S.lcap, S.ccap, TW, stage_bytes<ST>()), "the twin's tiles");
    hipLaunchKernelGGL((k_sws_gbrp<S.lcap, S.ccap, ST, SwsSrc<C>::NV, SwsSrc<C>::RGB>), op.grid, dim3(NT), 0, op.s, static_cast<const SwsDev *>(op.d), *op.coefs,
                       static_cast<const mi355_sws_planar_frame *>(op.frames));
}
}  // namespace

bool mi355_sws_launch_gbrp(const SwsKey &key, const SwsOperands &op)
{
    /* a gbrp context's key is its yuv444p twin's: the planar kernel's FULL form, no range, 8 bits */
    if (key.kernel != SWS_KERNEL_PLANAR || key.form != SWS_FORM_FULL || key.kind != SWS_KIND_PLAIN || key.alpha || !op.coefs) return false;
    return sws_pick<SwsSrcClass, SWS_SRC_P8, SWS_SRC_P16, SWS_SRC_NV, SWS_SRC_RGB24, SWS_SRC_RGB32, SWS_SRC_YUY2, SWS_SRC_P010>(key.src, [&](auto src) {
        return sws_pick_instance(key.i, [&](auto i) { launch_gbrp<decltype(i)::value, decltype(src)::value>(op); return true; });
    });
}

/* the line entry takes host pointers at any address: the lines are packed into the staging arena at a pitch of whole 16-byte pieces */
extern "C" void mi355_sws_yuv2gbrp_full_X(const mi355_sws_rgb_coefs *coefs, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize,
                                          const int16_t *chrFilter, const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize,
                                          uint8_t *const dest[3], int dstW)
{
    if (!coefs || !lumFilter || !lumSrc || !chrFilter || !chrUSrc || !chrVSrc || !dest || dstW <= 0 || lumFilterSize < 1 || chrFilterSize < 1) return;
    Arena &a = arena();
    const int ls = lumFilterSize, cs = chrFilterSize, pitch = (dstW + 7) & ~7;
    a.reserve((size_t)(ls + 2 * cs) * pitch * 2 + (size_t)(ls + cs) * 2 + (size_t)3 * dstW + 256);
    auto rows = [&](const int16_t **src, int n) {
        const size_t o = a.take((size_t)n * pitch * 2);
        for (int j = 0; j < n; j++) std::memcpy(a.h<int16_t>(o) + (size_t)j * pitch, src[j], (size_t)dstW * 2);
        return o;
    };
    const size_t o_l = rows(lumSrc, ls), o_u = rows(chrUSrc, cs), o_v = rows(chrVSrc, cs);
    const size_t o_lf = a.take((size_t)ls * 2), o_cf = a.take((size_t)cs * 2);
    size_t o_d[3];
    for (int p = 0; p < 3; p++) o_d[p] = a.take((size_t)dstW);
    std::memcpy(a.h<int16_t>(o_lf), lumFilter, (size_t)ls * 2);
    std::memcpy(a.h<int16_t>(o_cf), chrFilter, (size_t)cs * 2);
    a.upload();
    hipLaunchKernelGGL(k_sws_line_gbrp, dim3(1), dim3(NT), 0, a.stream, *coefs, a.d<const int16_t>(o_lf), a.d<const int16_t>(o_l), ls, a.d<const int16_t>(o_cf),
                       a.d<const int16_t>(o_u), a.d<const int16_t>(o_v), cs, pitch, a.d<uint8_t>(o_d[0]), a.d<uint8_t>(o_d[1]), a.d<uint8_t>(o_d[2]), dstW);
    a.download();
    for (int p = 0; p < 3; p++) std::memcpy(dest[p], a.h<uint8_t>(o_d[p]), (size_t)dstW);
}
