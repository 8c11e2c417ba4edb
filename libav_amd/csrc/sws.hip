/*
 * sws.hip — the libswscale part of the path: planar yuv 4:2:0 / 4:2:2 / 4:4:4 sources at 8, 9 or 10 bits (16-bit
 * little-endian samples above 8: hScale16To15_c swscale.c:110-130 in place of hScale8To15_c), 8-bit NV12 / NV21 and packed rgb24 / bgr24 sources -> rgb24,
 * -> 8-bit yuv420p / yuv422p / yuv444p and -> NV12 / NV21 (dithered from a deeper source, swscale.c:553-556), the unscaled 8-bit
 * yuv420p -> NV12 / NV21 packer and the unscaled NV12 / NV21 -> yuv420p splitter; to the YUV destinations also with range conversion between the two
 * passes (yuvj420p <-> yuv420p and their kin: lumConvertRange / chrConvertRange swscale.c:168-198), and to the three planar destinations at 9 or
 * 10 bits (yuv420p9le ... yuv444p10le: yuv2planeX_10 / yuv2plane1_10 output.c:183-213; their tile instances are launched from sws_deep.hip), and
 * to bgr24 / rgba / bgra / argb / abgr wherever rgb24 is written (yuv2rgb_write output.c:825-867; their instances are launched from sws_packed.hip);
 * packed 32-bit rgba / bgra / argb / abgr SOURCES to all of these, with the source's alpha carried to a 32-bit destination where the caller asks for it
 * (mi355_sws_create_src_layout_alpha; their instances, line kernels and line entries are sws_rgb32.hip's); and packed 4:2:2 yuyv422 / uyvy422 / yvyu422
 * SOURCES to all of these, with the unscaled yuyv422 / uyvy422 -> yuv420p / yuv422p splitter (their tile instances, k_sws_ident1_yuy2, k_sws_yuy2_split
 * and the line entries mi355_sws_yuy2ToY / _yuy2ToUV are sws_yuy2.hip's); and packed 4:2:2 yuyv422 / uyvy422 / yvyu422 DESTINATIONS from every one of these
 * sources wherever rgb24 is written, also with range conversion, with the unscaled yuv422p / yuv420p -> yuyv422 / uyvy422 packer (yuv2422_X / _2 / _1_c_template
 * output.c:451-582; their DST_YUY2 instances and k_sws_yuy2_pack are sws_yuy2dst.hip's); and p010le SOURCES (MI355_SWS_SRC_P010: a plane of 16-bit words and a
 * plane of word pairs, the sample word >> 6 — p010LEToY_c / p010LEToUV_c input.c:499-524) to every destination the yuv420p10le source takes (their tile
 * instances, line kernels and the line entries mi355_sws_p010ToY / _p010ToUV are sws_p010.hip's); and SWS_FAST_BILINEAR contexts of the planar 8-bit
 * sources (mi355_sws_create_fast_bilinear: hyscale_fast_c / hcscale_fast_c swscale.c:238-301 in place of the bank-driven horizontal pass; the tile kernels
 * k_sws_fbl_generic / k_sws_fbl_planar and the line entries mi355_sws_hyscale_fast / _hcscale_fast are sws_fastbl.hip's); and planar RGB (gbrp)
 * destinations from every source (mi355_sws_create_gbrp: yuv2gbrp_full_X_c output.c:1275-1355; the tile kernel k_sws_gbrp and the line entry
 * mi355_sws_yuv2gbrp_full_X are sws_gbrp.hip's).  This file:
 * the context, the plan (which kernel a context gets) and the entry points of include/mi355_sws.h.  The device side is sws_dev.h:
 * k_sws_generic, k_sws_planar, k_sws_c24, k_sws_ident1, k_sws_nv12_pack, k_sws_nv12_split and the k_sws_line_* kernels of the Tier-1 entry points.
 * Filter banks and LUTs are inputs (built by the reference's init code, see include/mi355_sws.h).
 * Launches: sws_key() names a context's instance once (sws_dev.h: SwsKey), sws_run() hands the key to the file that compiles that instance — here
 * the plain and RANGE instances of k_sws_planar and the rgb24 destination of k_sws_generic / k_sws_ident1 / k_sws_c24 for the four classic source
 * classes; sws_deep.hip, sws_packed.hip, sws_rgb32.hip, sws_yuy2.hip, sws_yuy2dst.hip and sws_p010.hip hold the rest, one launch function each — and every file maps the key to its
 * instance through the one dispatcher sws_launch() of sws_dev.h.  A fast-bilinear context has its twin's key and goes to sws_fastbl.hip with it.
 */
#include "mi355_rt.h"
#include "sws_dev.h"
#include "../../include/mi355_sws.h"
#include "../../include/mi355dsp.h"

using namespace mi355;

/* ---- context ------------------------------------------------------------------------------------------- */
struct mi355_sws_ctx {
    SwsDev h;
    SwsDev *d = nullptr;
    void *banks[8] = {};
    /* Tier-1 picture staging */
    uint8_t *d_src[3] = {}, *d_dst = nullptr;
    mi355_sws_frame *d_frame = nullptr;
    mi355_sws_planar_frame *d_pframe = nullptr;      /* ... of a planar context (d_dst then holds its three planes) */
    hipStream_t stream = nullptr;
    int device = -1;            /* the device of the thread that created the context: its entry points switch to it */
    int alpha = 0;              /* a 32-bit source's alpha goes to the 32-bit destination (mi355_sws_create_src_layout_alpha): the ALPHA instances */
    int hfit = 0;               /* a plane with a horizontal filter other than the identity has a tile whose source span fits a staged line (ctx_hfit) */
    /* a SWS_FAST_BILINEAR context (mi355_sws_create_fast_bilinear): the horizontal pass reads no bank — the reference's two 16.16 increments, as its init
     * left them; the tile kernels are sws_fastbl.hip's k_sws_fbl_generic / k_sws_fbl_planar under the twin's key */
    int fast_bilinear = 0, lumXInc = 0, chrXInc = 0;
    /* a gbrp context (mi355_sws_create_gbrp): created as its yuv444p twin (h.planar stays MI355_SWS_DST_YUV444P: the same tiles, the same three planes of
     * dstW x dstH bytes) and marked; the vertical pass is sws_gbrp.hip's k_sws_gbrp under the twin's key, with the reference's six coefficients */
    int gbrp = 0;
    mi355_sws_rgb_coefs coefs = {};
};

template <typename T> static const T *upload_bank(mi355_sws_ctx *c, int slot, const T *host, size_t n)
{
    if (!n || !host) return nullptr;
    void *p;
    MI355_CHECK(hipMalloc(&p, n * sizeof(T)));
    MI355_CHECK(hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    c->banks[slot] = p;
    return static_cast<const T *>(p);
}

/* rows per tile: the largest power of two <= MAXTH for which no tile needs more source lines than the
 * LDS tile may hold; 0 if even single rows do not fit (filters larger than the tile: not supported).  lines[2]: the largest
 * luma / chroma span of a tile — what the context's LDS tile is sized for. */
static int choose_rows(const mi355_sws_desc *d, int lines[2], int vshift = 0, int maxc = MAXC)
{
    for (int th = MAXTH; th >= 1; th >>= 1) {
        bool ok = true;
        lines[0] = lines[1] = 1;
        for (int y0 = 0; y0 < d->dstH && ok; y0 += th) {
            const int y1 = (y0 + th < d->dstH ? y0 + th : d->dstH) - 1;
            /* the span of filter rows a..b (none: 0) */
            auto span = [&](const mi355_sws_filter &f, int srcH, int a, int b) {
                if (a > b) return 0;
                int lo = f.pos[a] > 1 - f.size ? f.pos[a] : 1 - f.size, hi = (f.pos[b] > 1 - f.size ? f.pos[b] : 1 - f.size) + f.size - 1;
                for (int y = a; y < b; y++) if (f.pos[y + 1] < f.pos[y]) return 1 << 30;   /* not monotonic */
                lo = lo < 0 ? 0 : (lo > srcH - 1 ? srcH - 1 : lo);
                hi = hi < 0 ? 0 : (hi > srcH - 1 ? srcH - 1 : hi);
                return hi - lo + 1;
            };
            /* chroma rows: those cy with cy << vshift in y0..y1 (rgb24: vshift 0, the tile's rows) */
            const int sl = span(d->vLum, d->srcH, y0, y1), sc = span(d->vChr, d->chrSrcH, (y0 + (1 << vshift) - 1) >> vshift, y1 >> vshift);
            ok = sl <= MAXL && sc <= maxc;
            lines[0] = sl > lines[0] ? sl : lines[0];
            lines[1] = sc > lines[1] ? sc : lines[1];
        }
        if (ok) return th;
    }
    return 0;
}

/* what mi355_sws_create and mi355_sws_create_planar share: the descriptor's sizes and the horizontal banks' properties */
static mi355_sws_ctx *ctx_new(const mi355_sws_desc *desc)
{
    mi355_sws_ctx *c = new mi355_sws_ctx;
    c->device = current_device();
    SwsDev &h = c->h;
    h.srcW = desc->srcW; h.srcH = desc->srcH; h.dstW = desc->dstW; h.dstH = desc->dstH;
    h.chrSrcW = desc->chrSrcW; h.chrSrcH = desc->chrSrcH; h.chrDstW = desc->chrDstW; h.special = desc->unscaled_special;
    h.hls = desc->hLum.size; h.hcs = desc->hChr.size; h.vls = desc->vLum.size; h.vcs = desc->vChr.size;
    h.luts = desc->luts;
    h.th = 0;
    h.lum_lines = h.chr_lines = 1;
    h.hstage = 1;
    for (int i = 1; i < desc->hLum.n && desc->hLum.pos; i++) if (desc->hLum.pos[i] < desc->hLum.pos[i - 1]) h.hstage = 0;
    for (int i = 1; i < desc->hChr.n && desc->hChr.pos; i++) if (desc->hChr.pos[i] < desc->hChr.pos[i - 1]) h.hstage = 0;
    /* ... and every tap inside its line (the staged form does not clear what lies past the line's end) */
    for (int i = 0; i < desc->hLum.n && desc->hLum.pos; i++) if (desc->hLum.pos[i] < 0 || desc->hLum.pos[i] + desc->hLum.size > desc->srcW) h.hstage = 0;
    for (int i = 0; i < desc->hChr.n && desc->hChr.pos; i++) if (desc->hChr.pos[i] < 0 || desc->hChr.pos[i] + desc->hChr.size > desc->chrSrcW) h.hstage = 0;
    auto identity = [](const mi355_sws_filter &f, int src_w) {
        if (f.size != 1 || !f.coef || !f.pos || f.n > src_w) return 0;
        for (int i = 0; i < f.n; i++) if (f.coef[i] != 16384 || f.pos[i] != i) return 0;
        return 1;
    };
    h.hident_l = identity(desc->hLum, h.srcW);
    h.hident_c = identity(desc->hChr, h.chrSrcW);
    h.hLumC = h.hChrC = h.vLumC = h.vChrC = nullptr;
    h.hLumP = h.hChrP = h.vLumP = h.vChrP = nullptr;
    h.planar = h.hshift = h.vshift = 0;
    h.chrDstH = h.dstH;
    h.depth = 8; h.src_hsub = h.src_vsub = 1; h.src_layout = MI355_SWS_SRC_PLANAR;
    std::memset(h.dither, 64, sizeof(h.dither));
    h.dst_bits = 8;
    h.v1_rnd = h.v1_sh = h.vx_rnd = h.vx_sh = 0;
    h.packed = 0; h.dst_sel = 0;
    return c;
}
/* the source side of a context (mi355_sws_create_src); false for a combination outside 8 / 9 / 10 bit 4:2:0 / 4:2:2 / 4:4:4 or a descriptor
 * whose chroma size is not that subsampling's */
static bool ctx_source(mi355_sws_ctx *c, const mi355_sws_src *src)
{
    SwsDev &h = c->h;
    if (!src) return false;
    if (src->depth < 8 || src->depth > 10 || (src->hsub | src->vsub) & ~1 || (src->vsub && !src->hsub)) return false;
    if (h.chrSrcW != (h.srcW + (1 << src->hsub) - 1) >> src->hsub || h.chrSrcH != (h.srcH + (1 << src->vsub) - 1) >> src->vsub) return false;
    /* the unscaled special converter: 8-bit 4:2:0 and 4:2:2 only (swscale_unscaled.c:1051-1055) */
    if (h.special && (src->depth != 8 || !src->hsub)) return false;
    h.depth = src->depth; h.src_hsub = src->hsub; h.src_vsub = src->vsub;
    if (src->depth > 8) std::memcpy(h.dither, src->dither, sizeof(h.dither));
    return true;
}
/* a packed destination other than rgb24: bgr24 or one of the four 32-bit orders */
static bool packed_dst(int dst_format) { return dst_format >= MI355_SWS_DST_BGR24 && dst_format <= MI355_SWS_DST_ABGR; }
static int packed_bpp(const SwsDev &h) { return h.packed >= MI355_SWS_DST_RGBA ? 4 : 3; }
/* a packed 4:2:2 destination: yuyv422 / uyvy422 / yvyu422 (a YUV destination in ONE plane: it converts the range, and its instances are sws_yuy2dst.hip's) */
static bool yuy2_dst(int dst_format) { return sws_yuy2_dst(dst_format); }
static bool yuy2_dst(const SwsDev &h) { return sws_yuy2_dst(h.packed); }
/* a destination of ONE packed plane, for the creators: everything but the planar and semi-planar formats */
static bool one_plane_dst(int dst_format) { return dst_format == 0 || packed_dst(dst_format) || yuy2_dst(dst_format); }
/* groups of four bytes the unscaled packer writes to a row: the reference's two-at-a-time loop, held inside the row (include/mi355_sws.h) */
static int yuy2_pack_groups(const SwsDev &h) { const int g = 2 * (((h.srcW >> 1) + 1) >> 1), r = (h.srcW + 1) >> 1; return g < r ? g : r; }
/* a packed RGB source: rgb24 / bgr24, or one of the four 32-bit orders (rgb32_src: its tile instances are launched from sws_rgb32.hip) */
static bool rgb32_src(const SwsDev &h) { return sws_rgb32_src(h.src_layout); }
static bool packed_rgb(const SwsDev &h) { return h.src_layout == MI355_SWS_SRC_RGB24 || h.src_layout == MI355_SWS_SRC_BGR24 || rgb32_src(h); }
static int src_bpx(const SwsDev &h) { return rgb32_src(h) ? 4 : 3; }
/* a packed 4:2:2 source: yuyv422 / uyvy422 / yvyu422 (its tile instances, ident1 form, splitter and line entries are sws_yuy2.hip's) */
static bool yuy2_src(const SwsDev &h) { return sws_yuy2_src(h.src_layout); }
/* a source of ONE plane whose converted samples are staged (hscale_tile_rgb): packed RGB, or packed 4:2:2 */
static bool converted_src(const SwsDev &h) { return packed_rgb(h) || yuy2_src(h); }
/* a P010 source: p010le, a plane of 16-bit words and a plane of pairs of them, the sample word >> 6 (its tile instances and line entries are sws_p010.hip's) */
static bool p010_src(const SwsDev &h) { return h.src_layout == MI355_SWS_SRC_P010; }
/* the layouts the creators take: 0, 1, 2, 4, 5, 8 .. 11, 16 .. 18 and 24 */
static bool src_layout_taken(int l) { return (l >= MI355_SWS_SRC_PLANAR && l <= MI355_SWS_SRC_BGR24 && l != 3) || sws_rgb32_src(l) || sws_yuy2_src(l) || l == MI355_SWS_SRC_P010; }
/* a context that does not scale, to rgb24: what k_sws_ident1 takes */
static bool ident1_shape(const SwsDev &h)
{
    return h.depth == 8 && h.hident_l && h.hident_c && h.vls == 1 && h.vcs <= 4 && !(h.dstW & 1) && h.srcW >= h.dstW && 2 * h.chrSrcW >= h.dstW;
}
/* the tile kernels stage a plane's source spans when the context allows it (hstage), the plane's filter is not the identity and a tile's span
 * fits the staged line (hscale_tile; planes and strides that are multiples of 16: the longest aligned start) */
static void ctx_hfit(mi355_sws_ctx *c, const mi355_sws_desc *desc)
{
    const SwsDev &h = c->h;
    const int B = h.depth > 8 ? 2 : 1, cw = h.planar ? TW >> h.hshift : TW / 2;
    auto fits = [&](const mi355_sws_filter &f, int ident, int cols) {
        if (ident || !f.pos) return false;
        for (int g = 0; g < f.n; g += cols) {
            const int last = (g + cols < f.n ? g + cols : f.n) - 1, s0 = B * f.pos[g], s1 = B * (f.pos[last] + f.size);
            if (span_fits(span_dwords(s0 & ~15, s1), s0, s1, stage_pitch(cols, B))) return true;
        }
        return false;
    };
    /* a plane of pairs: the span of a chroma tile in bytes against the luma staging line (hscale_tile_nv) */
    auto fits_nv = [&](const mi355_sws_filter &f, int ident, int cols) {
        if (ident || !f.pos) return false;
        for (int g = 0; g < f.n; g += cols) {
            const int last = (g + cols < f.n ? g + cols : f.n) - 1, s0 = 2 * f.pos[g], s1 = 2 * (f.pos[last] + f.size);
            if (span_fits(span_dwords(s0 & ~15, s1), s0, s1, stage_pitch(TW, 1))) return true;
        }
        return false;
    };
    /* a packed RGB plane: the span in converted samples from a multiple of four, both planes (hscale_tile_rgb) */
    auto fits_rgb = [&](const mi355_sws_filter &f, int ident, int cols) {
        if (ident || !f.pos) return false;
        for (int g = 0; g < f.n; g += cols) {
            const int last = (g + cols < f.n ? g + cols : f.n) - 1, s0 = f.pos[g], s1 = f.pos[last] + f.size;
            if (span_fits(span_dwords(s0 & ~3, s1), s0, s1, stage_pitch(cols, 1))) return true;
        }
        return false;
    };
    if (converted_src(h)) c->hfit = fits_rgb(desc->hLum, h.hident_l, TW) || fits_rgb(desc->hChr, h.hident_c, cw);
    else
    /* (a P010 source: the pair plane is de-interleaved as it is staged — U and V each in a line of the planar 16-bit source's chroma geometry) */
    c->hfit = fits(desc->hLum, h.hident_l, TW) || (h.src_layout && !p010_src(h) ? fits_nv(desc->hChr, h.hident_c, cw) : fits(desc->hChr, h.hident_c, cw));
}
static void upload_banks(mi355_sws_ctx *c, const mi355_sws_desc *desc)
{
    SwsDev &h = c->h;
    ctx_hfit(c, desc);
    h.hLumC = upload_bank(c, 0, desc->hLum.coef, (size_t)h.dstW * h.hls);    h.hLumP = upload_bank(c, 1, desc->hLum.pos, (size_t)h.dstW);
    h.hChrC = upload_bank(c, 2, desc->hChr.coef, (size_t)h.chrDstW * h.hcs); h.hChrP = upload_bank(c, 3, desc->hChr.pos, (size_t)h.chrDstW);
    h.vLumC = upload_bank(c, 4, desc->vLum.coef, (size_t)h.dstH * h.vls);    h.vLumP = upload_bank(c, 5, desc->vLum.pos, (size_t)h.dstH);
    h.vChrC = upload_bank(c, 6, desc->vChr.coef, (size_t)h.chrDstH * h.vcs); h.vChrP = upload_bank(c, 7, desc->vChr.pos, (size_t)h.chrDstH);
}
static mi355_sws_ctx *ctx_upload(mi355_sws_ctx *c)
{
    const SwsDev &h = c->h;
    MI355_CHECK(hipMalloc(reinterpret_cast<void **>(&c->d), sizeof(SwsDev)));
    MI355_CHECK(hipMemcpy(c->d, &h, sizeof(SwsDev), hipMemcpyHostToDevice));
    MI355_CHECK(hipStreamCreate(&c->stream));
    return c;
}

/* the four maps of lumConvertRange / chrConvertRange for an 8-bit destination (swscale.c:168-198): full -> limited has no cap of its own — 32767,
 * what an int16 holds, so the kernel's min is the same instruction both ways */
static SwsRangeMap range_map(int range, bool chroma)
{
    if (range == MI355_SWS_RANGE_TO_JPEG) return chroma ? SwsRangeMap{ 30775, 4663, -9289992, 12 } : SwsRangeMap{ 30189, 19077, -39057361, 14 };
    return chroma ? SwsRangeMap{ 32767, 1799, 4081085, 11 } : SwsRangeMap{ 32767, 14071, 33561947, 14 };
}
/* what the create entry points share: the source check, the destination family (rgb24, or planar: dst_format MI355_SWS_DST_*), the bank
 * validation with its diagnostics.  The unscaled special converter (rgb24) and the unscaled packer (NV12 / NV21) have no banks. */
static mi355_sws_ctx *ctx_create(const mi355_sws_desc *desc, const mi355_sws_src *src, bool planar, int dst_format, const char *who, int layout = MI355_SWS_SRC_PLANAR,
                                 int range = MI355_SWS_RANGE_NONE, int dst_depth = 8)
{
    const bool semi = dst_format == MI355_SWS_DST_NV12 || dst_format == MI355_SWS_DST_NV21;
    if (planar && (!desc || ((dst_format < MI355_SWS_DST_YUV420P || dst_format > MI355_SWS_DST_YUV444P) && !semi))) {
        std::fprintf(stderr, "mi355dsp: %s: destination format %d is not yuv420p / yuv422p / yuv444p / nv12 / nv21\n", who, dst_format);
        return nullptr;
    }
    mi355_sws_ctx *c = ctx_new(desc);
    SwsDev &h = c->h;
    /* bgr24 / rgba / bgra / argb / abgr: an rgb24 context in everything but the store (the order's byte selector is read by the 32-bit instances only) */
    if (!planar && packed_dst(dst_format)) { h.packed = dst_format; h.dst_sel = dst_format >= MI355_SWS_DST_RGBA ? sws_rgb32_sel(dst_format) : 0; }
    /* yuyv422 / uyvy422 / yvyu422: an rgb24 context too in everything but the vertical pass's store (the order's byte selector is read by the DST_YUY2 instances) */
    if (!planar && yuy2_dst(dst_format)) { h.packed = dst_format; h.dst_sel = sws_yuy2_dst_sel(dst_format); }
    h.range = range;
    h.rng_l = range_map(range, false); h.rng_c = range_map(range, true);      /* (read by the RANGE instances only) */
    if (dst_depth > 8) {
        /* yuv2plane1_10 / yuv2planeX_10 (output.c:183-213): rounding term and shift of the two forms (read by the DEEP instances only) */
        h.dst_bits = dst_depth;
        h.v1_rnd = 1 << (14 - dst_depth); h.v1_sh = 15 - dst_depth;
        h.vx_rnd = 1 << (26 - dst_depth); h.vx_sh = 27 - dst_depth;
    }
    if (src && !ctx_source(c, src)) {
        std::fprintf(stderr, "mi355dsp: %s: source %d bit, chroma shifts %d/%d (chroma %dx%d of %dx%d) is outside this backend\n", who, src->depth, src->hsub, src->vsub,
                     h.chrSrcW, h.chrSrcH, h.srcW, h.srcH);
        delete c;
        return nullptr;
    }
    const char *const packed_name = sws_rgb32_src(layout) ? "rgba / bgra / argb / abgr" : "rgb24 / bgr24";
    if (layout == MI355_SWS_SRC_P010) {
        /* p010le: 10-bit 4:2:0 (ctx_source has checked chrSrcW / chrSrcH against the shifts).  The reference has no unscaled converter from it, not even the
         * plane copy (swscale_unscaled.c:1162-1167): every context is the scaler's, with the banks, the plan and the refusals of the yuv420p10le source of
         * the same descriptor */
        if (h.depth != 10 || !h.src_hsub || !h.src_vsub) {
            std::fprintf(stderr, "mi355dsp: %s: a p010 source is 10-bit 4:2:0 (%d bit, shifts %d/%d)\n", who, h.depth, h.src_hsub, h.src_vsub);
            delete c;
            return nullptr;
        }
        h.src_layout = layout;
        if (h.special) {
            std::fprintf(stderr, "mi355dsp: %s: no unscaled special converter takes a p010 source\n", who);
            delete c;
            return nullptr;
        }
    } else
    if (sws_yuy2_src(layout)) {
        /* packed 4:2:2 (two bytes a pixel): 8 bit, chroma on every line at half the width (ctx_source has checked chrSrcW / chrSrcH against the shifts) */
        if (h.depth != 8 || !h.src_hsub || h.src_vsub) {
            std::fprintf(stderr, "mi355dsp: %s: a yuyv422 / uyvy422 / yvyu422 source is 8-bit 4:2:2 (%d bit, shifts %d/%d)\n", who, h.depth, h.src_hsub, h.src_vsub);
            delete c;
            return nullptr;
        }
        h.src_layout = layout;
        /* the four unscaled converters (yuyvToYuv420Wrapper ... uyvyToYuv422Wrapper): none from yvyu422, to 8-bit yuv420p / yuv422p at equal size, no range */
        if (h.special) {
        if (layout == MI355_SWS_SRC_YVYU422 || !planar || (dst_format != MI355_SWS_DST_YUV420P && dst_format != MI355_SWS_DST_YUV422P) || range != MI355_SWS_RANGE_NONE ||
            dst_depth != 8 || h.srcW != h.dstW || h.srcH != h.dstH || h.chrDstW != (h.dstW + 1) >> 1) {
            std::fprintf(stderr, "mi355dsp: %s: the unscaled special converters of a packed 4:2:2 source are yuyv422 / uyvy422 -> yuv420p / yuv422p at equal size "
                         "(layout %d, destination %d, %d bit, range %d, %dx%d -> %dx%d, chrDstW %d)\n", who, layout, dst_format, dst_depth, range, h.srcW, h.srcH, h.dstW, h.dstH,
                         h.chrDstW);
            delete c;
            return nullptr;
        }
        h.planar = dst_format; h.hshift = 1; h.vshift = dst_format == MI355_SWS_DST_YUV420P ? 1 : 0;
        h.chrDstH = (h.dstH + (1 << h.vshift) - 1) >> h.vshift;
        return ctx_upload(c);
        }
        /* any other context is the scaler's: the banks, the plan and the refusals of the 8-bit yuv422p source of the same descriptor */
    } else
    if (layout == MI355_SWS_SRC_RGB24 || layout == MI355_SWS_SRC_BGR24 || sws_rgb32_src(layout)) {
        /* packed RGB (three or four bytes a pixel): 8 bit, chroma on every line, the full or the halving converter (ctx_source has checked chrSrcW / chrSrcH against the shifts);
         * no special converter */
        if (h.depth != 8 || h.src_vsub) {
            std::fprintf(stderr, "mi355dsp: %s: an %s source is 8 bit with chroma on every line (%d bit, shifts %d/%d)\n", who, packed_name, h.depth, h.src_hsub, h.src_vsub);
            delete c;
            return nullptr;
        }
        h.src_layout = layout;
        if (h.special) {
            std::fprintf(stderr, "mi355dsp: %s: no unscaled special converter takes an %s source here\n", who, packed_name);
            delete c;
            return nullptr;
        }
    } else
    if (layout) {
        /* NV12 / NV21: 8-bit 4:2:0; the only special context is the splitter (nv12ToPlanarWrapper: to yuv420p at equal size, no banks) */
        if (h.depth != 8 || !h.src_hsub || !h.src_vsub) {
            std::fprintf(stderr, "mi355dsp: %s: an nv12 / nv21 source is 8-bit 4:2:0 (%d bit, shifts %d/%d)\n", who, h.depth, h.src_hsub, h.src_vsub);
            delete c;
            return nullptr;
        }
        h.src_layout = layout;
        if (h.special) {
            if (dst_format != MI355_SWS_DST_YUV420P || h.srcW != h.dstW || h.srcH != h.dstH || h.chrDstW != (h.dstW + 1) >> 1) {
                std::fprintf(stderr, "mi355dsp: %s: the only unscaled special converter of an nv12 / nv21 source is the splitter to yuv420p at equal size "
                             "(destination %d, %dx%d -> %dx%d, chrDstW %d)\n", who, dst_format, h.srcW, h.srcH, h.dstW, h.dstH, h.chrDstW);
                delete c;
                return nullptr;
            }
            h.planar = dst_format; h.hshift = h.vshift = 1;
            h.chrDstH = (h.dstH + 1) >> 1;
            return ctx_upload(c);
        }
    }
    bool ok = true;                                   /* what only a planar destination asks for */
    if (planar) {
        h.planar = dst_format;
        h.hshift = dst_format == MI355_SWS_DST_YUV444P ? 0 : 1;
        h.vshift = dst_format == MI355_SWS_DST_YUV420P || semi ? 1 : 0;
        h.chrDstH = (h.dstH + (1 << h.vshift) - 1) >> h.vshift;               /* AV_CEIL_RSHIFT, utils.c:1040 */
        if (semi && h.special) {
            /* the unscaled packer (planarToNv12Wrapper): 8-bit 4:2:0 at equal size, no banks */
            if (h.depth != 8 || !h.src_hsub || !h.src_vsub || h.srcW != h.dstW || h.srcH != h.dstH || h.chrDstW != (h.dstW + 1) >> 1) {
                std::fprintf(stderr, "mi355dsp: %s: the unscaled nv12 / nv21 packer takes 8-bit 4:2:0 at equal size only (%d bit, shifts %d/%d, %dx%d -> %dx%d, chrDstW %d)\n",
                             who, h.depth, h.src_hsub, h.src_vsub, h.srcW, h.srcH, h.dstW, h.dstH, h.chrDstW);
                delete c;
                return nullptr;
            }
            return ctx_upload(c);
        }
        if (semi && (h.chrDstW != (h.dstW + 1) >> 1 || desc->vChr.n != h.chrDstH)) {
            std::fprintf(stderr, "mi355dsp: %s: chrDstW %d / vChr.n %d are not those of a 4:2:0 destination of %dx%d (%d / %d)\n", who, h.chrDstW, desc->vChr.n,
                         h.dstW, h.dstH, (h.dstW + 1) >> 1, h.chrDstH);
            delete c;
            return nullptr;
        }
        ok = !h.special && desc->hLum.coef && desc->hLum.pos && desc->hChr.coef && desc->hChr.pos && desc->vLum.coef && desc->vLum.pos &&
             desc->vChr.coef && desc->vChr.pos && h.chrDstW == (h.dstW + (1 << h.hshift) - 1) >> h.hshift;
    } else if (h.special && yuy2_dst(h)) {
        /* the four unscaled packers (yuv422pToYuy2Wrapper, yuv422pToUyvyWrapper, planarToYuy2Wrapper, planarToUyvyWrapper): three planes of bytes at 4:2:2 or
         * 4:2:0 (ctx_source has refused 4:4:4 and deeper samples) to yuyv422 / uyvy422 — none to yvyu422 — at equal size, no range */
        if (h.src_layout != MI355_SWS_SRC_PLANAR || dst_format == MI355_SWS_DST_YVYU422 || range != MI355_SWS_RANGE_NONE || h.srcW != h.dstW || h.srcH != h.dstH ||
            h.chrDstW != (h.dstW + 1) >> 1) {
            std::fprintf(stderr, "mi355dsp: %s: the unscaled packers to a packed 4:2:2 destination are 8-bit yuv422p / yuv420p -> yuyv422 / uyvy422 at equal size "
                         "(layout %d, destination %d, range %d, %dx%d -> %dx%d, chrDstW %d)\n", who, h.src_layout, dst_format, range, h.srcW, h.srcH, h.dstW, h.dstH, h.chrDstW);
            delete c;
            return nullptr;
        }
        return ctx_upload(c);
    } else if (h.special) return ctx_upload(c);
    int lines[2] = { 1, 1 };
    if (!ok || desc->hLum.n != h.dstW || desc->hChr.n != h.chrDstW || desc->vLum.n != h.dstH || desc->vChr.n != h.chrDstH ||
        h.hls < 1 || h.hcs < 1 || h.vls < 1 || h.vcs < 1 || !(h.th = choose_rows(desc, lines, h.vshift, planar ? MAXCP : MAXC))) {
        std::fprintf(stderr, "mi355dsp: %s: filter banks do not fit this backend (sizes %d/%d/%d/%d)\n", who, h.hls, h.hcs, h.vls, h.vcs);
        delete c;
        return nullptr;
    }
    h.lum_lines = lines[0]; h.chr_lines = lines[1];
    /* (to a packed 4:2:2 destination the reference does build that context: it runs the tile kernel) */
    if (packed_rgb(h) && !planar && !yuy2_dst(h) && ident1_shape(h)) {
        /* rgb in, rgb out, nothing scaled: the reference never runs its scaler on that (a copy, or rgbToRgbWrapper) */
        std::fprintf(stderr, "mi355dsp: %s: an %s source to rgb24 without scaling is not a context of the scaler\n", who, packed_name);
        delete c;
        return nullptr;
    }
    upload_banks(c, desc);
    return ctx_upload(c);
}
/* what the creators open with, each under the name `who` of the entry point: a thread bound to its device (no CPU fallback: abort), ... */
static void creator_bind(const char *who)
{
    if (!bind()) { std::fprintf(stderr, "mi355dsp: %s without mi355_init(); no CPU fallback\n", who); std::abort(); }
}
/* ... a descriptor and a source side, ... */
static bool creator_args(const char *who, const mi355_sws_desc *desc, const mi355_sws_src *src)
{
    creator_bind(who);
    if (!desc || !src) { std::fprintf(stderr, "mi355dsp: %s: no descriptor\n", who); return false; }
    return true;
}
/* ... and a source layout of the list (the layered creators check their own argument first, so this is a step of its own) */
static bool creator_layout(const char *who, int src_layout)
{
    if (src_layout_taken(src_layout)) return true;
    std::fprintf(stderr, "mi355dsp: %s: source layout %d is not planar / nv12 / nv21 / rgb24 / bgr24 / rgba / bgra / argb / abgr / yuyv422 / uyvy422 / yvyu422 / p010\n", who, src_layout);
    return false;
}
extern "C" mi355_sws_ctx *mi355_sws_create(const mi355_sws_desc *desc)
{
    creator_bind("mi355_sws_create");
    return ctx_create(desc, nullptr, false, 0, "mi355_sws_create");
}
extern "C" mi355_sws_ctx *mi355_sws_create_planar(const mi355_sws_desc *desc, int dst_format)
{
    creator_bind("mi355_sws_create_planar");
    return ctx_create(desc, nullptr, true, dst_format, "mi355_sws_create_planar");
}
extern "C" mi355_sws_ctx *mi355_sws_create_src(const mi355_sws_desc *desc, const mi355_sws_src *src, int dst_format)
{
    if (!creator_args("mi355_sws_create_src", desc, src)) return nullptr;
    return ctx_create(desc, src, !one_plane_dst(dst_format), dst_format, "mi355_sws_create_src");
}
extern "C" mi355_sws_ctx *mi355_sws_create_src_layout(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, int dst_format)
{
    if (!creator_args("mi355_sws_create_src_layout", desc, src)) return nullptr;
    if (!creator_layout("mi355_sws_create_src_layout", src_layout)) return nullptr;
    return ctx_create(desc, src, !one_plane_dst(dst_format), dst_format, "mi355_sws_create_src_layout", src_layout);
}
extern "C" int mi355_sws_source_layout(const mi355_sws_ctx *c) { return c ? c->h.src_layout : -1; }
extern "C" mi355_sws_ctx *mi355_sws_create_src_layout_alpha(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, int dst_format, int alpha)
{
    if (!alpha) return mi355_sws_create_src_layout(desc, src, src_layout, dst_format);
    if (!creator_args("mi355_sws_create_src_layout_alpha", desc, src)) return nullptr;
    if (alpha != 1 || !sws_rgb32_src(src_layout) || dst_format < MI355_SWS_DST_RGBA || dst_format > MI355_SWS_DST_ABGR || desc->unscaled_special) {
        std::fprintf(stderr, "mi355dsp: mi355_sws_create_src_layout_alpha: alpha (%d) is carried from an rgba / bgra / argb / abgr source (layout %d) to an rgba / bgra / "
                     "argb / abgr destination (format %d) by the scaler only (unscaled_special %d)\n", alpha, src_layout, dst_format, desc->unscaled_special);
        return nullptr;
    }
    mi355_sws_ctx *c = ctx_create(desc, src, false, dst_format, "mi355_sws_create_src_layout_alpha", src_layout);
    if (c) c->alpha = 1;
    return c;
}
extern "C" int mi355_sws_alpha(const mi355_sws_ctx *c) { return c ? c->alpha : -1; }
extern "C" mi355_sws_ctx *mi355_sws_create_src_layout_range(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, int dst_format, int range)
{
    if (range == MI355_SWS_RANGE_NONE) return mi355_sws_create_src_layout(desc, src, src_layout, dst_format);
    if (!creator_args("mi355_sws_create_src_layout_range", desc, src)) return nullptr;
    if (range != MI355_SWS_RANGE_FROM_JPEG && range != MI355_SWS_RANGE_TO_JPEG) {
        std::fprintf(stderr, "mi355dsp: mi355_sws_create_src_layout_range: range %d is not none / from-jpeg / to-jpeg\n", range);
        return nullptr;
    }
    if (!creator_layout("mi355_sws_create_src_layout_range", src_layout)) return nullptr;
    /* the reference converts the range of YUV destinations only (an RGB one takes it into its LUTs), and never in an unscaled special converter */
    if (dst_format == 0 || packed_dst(dst_format)) {
        std::fprintf(stderr, "mi355dsp: mi355_sws_create_src_layout_range: a packed RGB destination (%d) has its range in the LUTs, not in a conversion step\n", dst_format);
        return nullptr;
    }
    if (desc->unscaled_special) {
        std::fprintf(stderr, "mi355dsp: mi355_sws_create_src_layout_range: no unscaled special converter converts the range\n");
        return nullptr;
    }
    /* (a packed 4:2:2 destination is a YUV destination in one plane: the rgb24 form of the context, with the range) */
    return ctx_create(desc, src, !yuy2_dst(dst_format), dst_format, "mi355_sws_create_src_layout_range", src_layout, range);
}
extern "C" int mi355_sws_range(const mi355_sws_ctx *c) { return c ? c->h.range : -1; }
extern "C" mi355_sws_ctx *mi355_sws_create_src_layout_range_depth(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, int dst_format, int range,
                                                                  int dst_depth)
{
    if (dst_depth == 8) return mi355_sws_create_src_layout_range(desc, src, src_layout, dst_format, range);
    if (!creator_args("mi355_sws_create_src_layout_range_depth", desc, src)) return nullptr;
    if (dst_depth != 9 && dst_depth != 10) {
        std::fprintf(stderr, "mi355dsp: mi355_sws_create_src_layout_range_depth: destination depth %d is not 8 / 9 / 10\n", dst_depth);
        return nullptr;
    }
    if (!creator_layout("mi355_sws_create_src_layout_range_depth", src_layout)) return nullptr;
    if (dst_format < MI355_SWS_DST_YUV420P || dst_format > MI355_SWS_DST_YUV444P) {
        std::fprintf(stderr, "mi355dsp: mi355_sws_create_src_layout_range_depth: a %d-bit destination is yuv420p / yuv422p / yuv444p (format %d)\n", dst_depth, dst_format);
        return nullptr;
    }
    if (range != MI355_SWS_RANGE_NONE) {
        std::fprintf(stderr, "mi355dsp: mi355_sws_create_src_layout_range_depth: no range conversion (%d) to a %d-bit destination\n", range, dst_depth);
        return nullptr;
    }
    /* a deep destination at equal size with equal subsampling is a plane copy of the reference's (planarCopyWrapper), never its scaler */
    if (desc->unscaled_special) {
        std::fprintf(stderr, "mi355dsp: mi355_sws_create_src_layout_range_depth: no unscaled special converter writes a %d-bit destination\n", dst_depth);
        return nullptr;
    }
    return ctx_create(desc, src, true, dst_format, "mi355_sws_create_src_layout_range_depth", src_layout, MI355_SWS_RANGE_NONE, dst_depth);
}
extern "C" int mi355_sws_dest_depth(const mi355_sws_ctx *c) { return c ? c->h.dst_bits : -1; }

/* ---- SWS_FAST_BILINEAR contexts: the reference's hyscale_fast_c / hcscale_fast_c in place of the bank-driven horizontal pass ---------------------
 * The context of the planar 8-bit source (layout 0, no alpha: the creator has neither argument) whose horizontal pass is the bank-free one of
 * sws_dev.h.  Everything else is the twin's — the bank-driven context of the same descriptor, source and destination: it is created as that twin
 * (ctx_create through the layered creators: the destination, range and depth checks, the vertical banks against the tiles, the plan) with a
 * one-tap stand-in for the two horizontal banks, which the fast pass never reads, and then marked.  Never IDENT1_* (no bank is an identity),
 * never C24 or a packer (unscaled_special is refused). */
extern "C" mi355_sws_ctx *mi355_sws_create_fast_bilinear(const mi355_sws_desc *desc, const mi355_sws_src *src, int dst_format, int range, int dst_depth,
                                                         int lumXInc, int chrXInc)
{
    const char *const who = "mi355_sws_create_fast_bilinear";
    if (!creator_args(who, desc, src)) return nullptr;
    if (src->depth != 8) {
        std::fprintf(stderr, "mi355dsp: %s: the reference runs its fast bilinear pass on 8-bit sources only (%d bit)\n", who, src->depth);
        return nullptr;
    }
    if (desc->unscaled_special) {
        std::fprintf(stderr, "mi355dsp: %s: an unscaled special converter has no horizontal pass\n", who);
        return nullptr;
    }
    if (lumXInc <= 0 || chrXInc <= 0) {
        std::fprintf(stderr, "mi355dsp: %s: increments %d / %d are not positive\n", who, lumXInc, chrXInc);
        return nullptr;
    }
    /* the last column of a plane: its position fits the reference's unsigned 32-bit xpos, and it reads no further than sample w (one behind the line) */
    auto plane_ok = [&](const char *name, int n, int w, int inc) {
        if (n < 1 || w < 1) { std::fprintf(stderr, "mi355dsp: %s: %s plane of %d -> %d samples\n", who, name, w, n); return false; }
        const uint64_t last = (uint64_t)(n - 1) * (uint64_t)inc;
        if (last > 0xFFFFFFFFull) {
            std::fprintf(stderr, "mi355dsp: %s: %s position (%d - 1) * %d does not fit 32 bits\n", who, name, n, inc);
            return false;
        }
        if ((last >> 16) > (uint64_t)(w - 1)) {
            std::fprintf(stderr, "mi355dsp: %s: the last %s column reads sample %llu of %d: more than one behind the line\n", who, name, (unsigned long long)(last >> 16) + 1, w);
            return false;
        }
        return true;
    };
    if (!plane_ok("luma", desc->dstW, desc->srcW, lumXInc) || !plane_ok("chroma", desc->chrDstW, desc->chrSrcW, chrXInc)) return nullptr;
    /* the twin, with stand-ins for hLum / hChr (one tap of 0 at position 0: no identity, monotonic, inside the line).  ctx_create uploads them like any
     * bank: dstW + chrDstW zero taps and positions stay on the device for the life of the context (SwsDev's hLumC / hLumP / hChrC / hChrP point at
     * them) and no kernel of this context reads them */
    const int nmax = desc->dstW > desc->chrDstW ? desc->dstW : desc->chrDstW;
    int16_t *coef = new int16_t[nmax]();
    int32_t *pos = new int32_t[nmax]();
    mi355_sws_desc twin = *desc;
    twin.hLum = mi355_sws_filter{ coef, pos, 1, desc->dstW };
    twin.hChr = mi355_sws_filter{ coef, pos, 1, desc->chrDstW };
    mi355_sws_ctx *c = mi355_sws_create_src_layout_range_depth(&twin, src, MI355_SWS_SRC_PLANAR, dst_format, range, dst_depth);
    delete[] coef;
    delete[] pos;
    if (!c) {
        std::fprintf(stderr, "mi355dsp: %s: the bank-driven context of this descriptor is refused (above)\n", who);
        return nullptr;
    }
    c->fast_bilinear = 1; c->lumXInc = lumXInc; c->chrXInc = chrXInc;
    /* a tile's span [xx(first), xx(last) + 1] fits a staged line (hscale_tile_fbl) */
    const SwsDev &h = c->h;
    auto fits = [](int n, uint32_t inc, int cols) {
        for (int g = 0; g < n; g += cols) {
            const int last = (g + cols < n ? g + cols : n) - 1, s0 = (int)(((uint32_t)g * inc) >> 16), s1 = (int)(((uint32_t)last * inc) >> 16) + 2;
            if (span_fits(span_dwords(s0 & ~15, s1), s0, s1, stage_pitch(cols, 1))) return true;
        }
        return false;
    };
    c->hfit = fits(h.dstW, (uint32_t)lumXInc, TW) || fits(h.chrDstW, (uint32_t)chrXInc, h.planar ? TW >> h.hshift : TW / 2);
    return c;
}
extern "C" int mi355_sws_fast_bilinear(const mi355_sws_ctx *c, int *lumXInc, int *chrXInc)
{
    if (!c) return -1;
    if (lumXInc) *lumXInc = c->lumXInc;
    if (chrXInc) *chrXInc = c->chrXInc;
    return c->fast_bilinear;
}

/* ---- planar RGB destinations: gbrp, the reference's yuv2gbrp_full_X_c with six coefficients in place of the LUTs -------------------------------
 * Everything but the vertical pass is the yuv444p twin's — the context of the same descriptor and source to an 8-bit 4:4:4 destination without range
 * conversion: it is created as that twin (the source checks of every layout, the vertical banks against the FULL tiles, the plan, hfit) and then
 * marked.  A 9 / 10-bit source's twin dithers; this destination does not (k_sws_gbrp reads no dither table). */
extern "C" mi355_sws_ctx *mi355_sws_create_gbrp(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, const mi355_sws_rgb_coefs *coefs)
{
    const char *const who = "mi355_sws_create_gbrp";
    if (!creator_args(who, desc, src)) return nullptr;
    if (!coefs) {
        std::fprintf(stderr, "mi355dsp: %s: no coefficients (c->yuv2rgb_* of the reference's context)\n", who);
        return nullptr;
    }
    if (desc->unscaled_special) {
        std::fprintf(stderr, "mi355dsp: %s: an unscaled special converter to gbrp (rgbToPlanarRgbWrapper) is not a context of the scaler\n", who);
        return nullptr;
    }
    /* the device multiplies 24-bit operands (sws_dev.h: gbrp_pixel) */
    auto fits = [](int v, int bits) { return v > -(1 << bits) && v < (1 << bits); };
    if (!fits(coefs->y_offset, 22) || !fits(coefs->y_coeff, 23) || !fits(coefs->v2r, 23) || !fits(coefs->v2g, 23) || !fits(coefs->u2g, 23) || !fits(coefs->u2b, 23)) {
        std::fprintf(stderr, "mi355dsp: %s: coefficients %d / %d / %d / %d / %d / %d do not fit 24 bits\n", who, coefs->y_offset, coefs->y_coeff, coefs->v2r, coefs->v2g,
                     coefs->u2g, coefs->u2b);
        return nullptr;
    }
    mi355_sws_ctx *c = mi355_sws_create_src_layout_range_depth(desc, src, src_layout, MI355_SWS_DST_YUV444P, MI355_SWS_RANGE_NONE, 8);
    if (!c) {
        std::fprintf(stderr, "mi355dsp: %s: the yuv444p context of this descriptor and source is refused (above)\n", who);
        return nullptr;
    }
    c->gbrp = 1; c->coefs = *coefs;
    return c;
}
extern "C" int mi355_sws_rgb_coefs_of(const mi355_sws_ctx *c, mi355_sws_rgb_coefs *coefs)
{
    if (!c) return -1;
    if (coefs) *coefs = c->coefs;
    return c->gbrp;
}

extern "C" void mi355_sws_destroy(mi355_sws_ctx *c)
{
    if (!c) return;
    DeviceScope on(c->device);
    for (void *p : c->banks) if (p) MI355_CHECK(hipFree(p));
    for (uint8_t *p : c->d_src) if (p) MI355_CHECK(hipFree(p));
    if (c->d_dst) MI355_CHECK(hipFree(c->d_dst));
    if (c->d_frame) MI355_CHECK(hipFree(c->d_frame));
    if (c->d_pframe) MI355_CHECK(hipFree(c->d_pframe));
    if (c->d) MI355_CHECK(hipFree(c->d));
    if (c->stream) MI355_CHECK(hipStreamDestroy(c->stream));
    delete c;
}

/* the kernel mi355_sws_scale_frames_dev launches for a context (MI355_SWS_K_*): the launch and mi355_sws_plan both ask here */
static int sws_kernel(const SwsDev &h)
{
    /* the smallest instance of the table whose LDS tile holds the context's lines (the C instances hold whatever choose_rows accepted) */
    auto instance = [&](const SwsShape (&shapes)[3]) {
        for (int i = 0; i < 2; i++) if (h.lum_lines <= shapes[i].lcap && h.chr_lines <= shapes[i].ccap) return i;
        return 2;
    };
    static_assert(MI355_SWS_K_GENERIC_C == MI355_SWS_K_GENERIC_A + 2 && MI355_SWS_K_PLANAR_C == MI355_SWS_K_PLANAR_A + 2, "A / B / C follow each other");
    if (h.planar && h.special) return yuy2_src(h) ? MI355_SWS_K_YUY2_SPLIT : (h.src_layout ? MI355_SWS_K_NV12_SPLIT : MI355_SWS_K_NV12_PACK);
    if (h.planar) return MI355_SWS_K_PLANAR_A + instance(PLANAR_SHAPES);
    if (h.special) return yuy2_dst(h) ? MI355_SWS_K_YUY2_PACK : MI355_SWS_K_C24;
    /* a context that does not scale: straight from the source bytes (k_sws_ident1; MI355_SWS_NO_IDENT1=1, developer switch: through the tile all the same) */
    static const bool no_ident1 = std::getenv("MI355_SWS_NO_IDENT1") != nullptr;
    /* (a context that converts the range — to a packed 4:2:2 destination only — goes through the tile: the conversion sits between its two passes) */
    if (!no_ident1 && ident1_shape(h) && !packed_rgb(h) && !(yuy2_src(h) && h.vcs > 2) && !h.range)      /* (a packed 4:2:2 source has the _1 form only: chroma on every line) */
        return h.vcs <= 2 ? MI355_SWS_K_IDENT1_1 : MI355_SWS_K_IDENT1_X;      /* packed_mode() 1 / the X template */
    return MI355_SWS_K_GENERIC_A + instance(GENERIC_SHAPES);
}

extern "C" int mi355_sws_plan(const mi355_sws_ctx *c, mi355_sws_plan_info *p)
{
    if (!c || !p) return -1;
    const SwsDev &h = c->h;
    p->kernel = sws_kernel(h);
    p->th = h.th; p->hstage = h.hstage; p->lum_lines = h.lum_lines; p->chr_lines = h.chr_lines;
    /* k_sws_generic: the wide form needs a full tile (dstW - x0 >= TW) and vertical filters of at most eight taps; k_sws_planar: every tile
     * stores bytewise (dstW < TW) or reads its taps from memory (more than eight) */
    p->narrow = !h.special && (h.dstW < TW || h.vls > 8 || h.vcs > 8);
    return 0;
}

extern "C" int mi355_sws_source(const mi355_sws_ctx *c, mi355_sws_source_info *p)
{
    if (!c || !p) return -1;
    p->depth = c->h.depth; p->hsub = c->h.src_hsub; p->vsub = c->h.src_vsub;
    const int k = sws_kernel(c->h);
    p->hstaged = k >= MI355_SWS_K_GENERIC_A && k <= MI355_SWS_K_PLANAR_C && c->h.hstage && c->hfit;
    return 0;
}

static bool semi_planar(const SwsDev &h) { return h.planar == MI355_SWS_DST_NV12 || h.planar == MI355_SWS_DST_NV21; }
/* what the packed-4:2:2 splitter writes to each chroma plane: bytes a row, rows */
static int yuy2_chr_bytes(const SwsDev &h) { return (h.srcW + 1) >> 1; }
static int yuy2_chr_rows(const SwsDev &h) { return h.planar == MI355_SWS_DST_YUV420P ? h.srcH >> 1 : h.srcH; }

extern "C" int mi355_sws_destination(const mi355_sws_ctx *c, mi355_sws_dest_info *p)
{
    if (!c || !p) return -1;
    const SwsDev &h = c->h;
    p->format = h.planar ? h.planar : h.packed;
    p->planes = !h.planar ? 1 : (semi_planar(h) ? 2 : 3);
    /* the packer rounds both extents down (planarToNv12Wrapper) */
    /* ... and so does the splitter (nv12ToPlanarWrapper) */
    p->chr_bytes = !h.planar ? 0 : (semi_planar(h) ? 2 * (h.special ? h.srcW >> 1 : h.chrDstW) : (h.special ? h.srcW >> 1 : h.chrDstW));
    p->chr_rows = !h.planar ? 0 : (h.special ? h.srcH >> 1 : h.chrDstH);
    /* the packed-4:2:2 splitter rounds the width UP and, to yuv420p, the rows down (yuyvtoyuv420_c); to yuv422p every row has chroma */
    if (h.special && yuy2_src(h)) { p->chr_bytes = yuy2_chr_bytes(h); p->chr_rows = yuy2_chr_rows(h); }
    if (h.dst_bits > 8) p->chr_bytes = 2 * h.chrDstW;       /* 16-bit samples (mi355_sws_dest_depth) */
    if (c->gbrp) p->format = MI355_SWS_DST_GBRP;            /* (planes, chr_bytes = dstW and chr_rows = dstH are the yuv444p twin's) */
    return 0;
}

/* ---- launches --------------------------------------------------------------------------------------------------------------------------- */
/* the destination form of the packed kernels for a dst_format (0: rgb24, MI355_SWS_DST_BGR24 ... _ABGR) */
static int dst_form(int dst_format) { return !dst_format ? DST_RGB24 : (dst_format == MI355_SWS_DST_BGR24 ? DST_BGR24 : (sws_yuy2_dst(dst_format) ? DST_YUY2 : DST_RGB32)); }

/* the launch key (sws_dev.h: SwsKey) of a context whose kernel is k = sws_kernel(): the one place where the context's fields become the key's codes */
static SwsKey sws_key(const mi355_sws_ctx *c, int k)
{
    const SwsDev &h = c->h;
    SwsKey key{};
    if (k >= MI355_SWS_K_PLANAR_A && k <= MI355_SWS_K_PLANAR_C) { key.kernel = SWS_KERNEL_PLANAR; key.i = k - MI355_SWS_K_PLANAR_A; }
    else if (k >= MI355_SWS_K_GENERIC_A && k <= MI355_SWS_K_GENERIC_C) { key.kernel = SWS_KERNEL_GENERIC; key.i = k - MI355_SWS_K_GENERIC_A; }
    else if (k == MI355_SWS_K_C24) key.kernel = h.src_vsub ? SWS_KERNEL_C24 : SWS_KERNEL_C24_422;
    else if (k == MI355_SWS_K_IDENT1_1) key.kernel = SWS_KERNEL_IDENT1_1;
    else if (k == MI355_SWS_K_IDENT1_X) key.kernel = SWS_KERNEL_IDENT1_X;
    else if (k == MI355_SWS_K_YUY2_PACK) key.kernel = SWS_KERNEL_YUY2_PACK;
    else key.kernel = SWS_KERNEL_YUY2_SPLIT;
    key.src = p010_src(h) ? SWS_SRC_P010 : rgb32_src(h) ? SWS_SRC_RGB32 : yuy2_src(h) ? SWS_SRC_YUY2 : packed_rgb(h) ? SWS_SRC_RGB24 : h.src_layout ? SWS_SRC_NV : h.depth > 8 ? SWS_SRC_P16 : SWS_SRC_P8;
    key.form = semi_planar(h) ? SWS_FORM_SEMI : (h.hshift ? SWS_FORM_HALF : SWS_FORM_FULL);
    key.kind = h.dst_bits > 8 ? SWS_KIND_DEEP : (h.range ? SWS_KIND_RANGE : SWS_KIND_PLAIN);
    key.dst = dst_form(h.packed);
    key.alpha = c->alpha != 0;
    return key;
}
static dim3 key_grid(const SwsKey &key, const SwsDev &h, int nframes)
{
    switch (key.kernel) {
    case SWS_KERNEL_GENERIC: case SWS_KERNEL_PLANAR: return sws_tile_grid(h, nframes);
    case SWS_KERNEL_IDENT1_1: case SWS_KERNEL_IDENT1_X: return sws_ident1_grid(h, nframes);
    case SWS_KERNEL_C24: case SWS_KERNEL_C24_422: return sws_c24_grid(h.dstW, h.srcH, nframes);
    default: return dim3(1, 1, nframes);        /* k_sws_yuy2_split, k_sws_yuy2_pack: the tile is its file's, the pictures are z */
    }
}
/* the launch of a key by the file that holds its instance; this file: the plain and RANGE instances of k_sws_planar and the rgb24 destination of the
 * packed kernels, of the four classic source classes */
static bool sws_run(const SwsKey &key, const SwsOperands &op)
{
    if (key.src == SWS_SRC_P010) return mi355_sws_launch_p010(key, op);        /* (to every destination, the packed 4:2:2 orders included) */
    if (key.dst == DST_YUY2) return mi355_sws_launch_yuy2dst(key, op);         /* (from every other source class) */
    if (key.src == SWS_SRC_RGB32) return mi355_sws_launch_rgb32(key, op);
    if (key.src == SWS_SRC_YUY2) return mi355_sws_launch_yuy2(key, op);
    if (key.kernel == SWS_KERNEL_PLANAR && key.kind == SWS_KIND_DEEP) return mi355_sws_launch_deep(key, op);
    if (key.kernel != SWS_KERNEL_PLANAR && key.dst != DST_RGB24) return mi355_sws_launch_packed(key, op);
    return sws_launch<SWS_CLASSIC_SRCS, sws_bit(SWS_KIND_PLAIN) | sws_bit(SWS_KIND_RANGE), sws_bit(DST_RGB24)>(key, op);
}
/* the context's kernel k on nframes pictures; -2: no file has the key's instance, or the launch failed */
static int ctx_launch(const mi355_sws_ctx *c, int k, const void *d_frames, int nframes, hipStream_t s)
{
    const SwsDev &h = c->h;
    const SwsKey key = sws_key(c, k);
    const SwsOperands op{ key_grid(key, h, nframes), s, &h, c->d, d_frames, &c->d->luts, h.dstW, h.srcH, h.dst_sel, nullptr, (uint32_t)c->lumXInc, (uint32_t)c->chrXInc, &c->coefs };
    /* a fast-bilinear context: the twin's key names its instance of the bank-free tile kernels; a gbrp context: the yuv444p twin's key its instance of k_sws_gbrp */
    if (!(c->gbrp ? mi355_sws_launch_gbrp(key, op) : c->fast_bilinear ? mi355_sws_launch_fastbl(key, op) : sws_run(key, op))) return -2;
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

/* workgroups per CU of the instances (8-bit, then 16-bit: their staging lines are STAGE_BYTES16); the NV instances stage the pair plane in the
 * 8-bit instances' staging lines (StageGeom<TW>) and hold the same tiles: the 8-bit rows below are theirs too */
static_assert(StageGeom<TW>::PITCH * StageGeom<TW>::LINES * 4 == STAGE_BYTES, "the pair plane's rounds fill the 8-bit staging storage");
constexpr int generic_waves(int i, int stage) { return sws_waves(sws_lds_bytes(GENERIC_SHAPES[i].lcap, GENERIC_SHAPES[i].ccap, stage)); }
constexpr int planar_waves(int i, int cw, int stage) { return sws_planar_waves(PLANAR_SHAPES[i].lcap, PLANAR_SHAPES[i].ccap, cw, stage); }
static_assert(generic_waves(0, STAGE_BYTES) == 8 && generic_waves(1, STAGE_BYTES) == 7 && generic_waves(2, STAGE_BYTES) == 6, "workgroups per CU of the instances");
static_assert(generic_waves(0, STAGE_BYTES16) == 7 && generic_waves(1, STAGE_BYTES16) == 5 && generic_waves(2, STAGE_BYTES16) == 5, "workgroups per CU of the 16-bit instances");
static_assert(planar_waves(0, TW / 2, STAGE_BYTES) == 8 && planar_waves(1, TW / 2, STAGE_BYTES) == 7 && planar_waves(2, TW / 2, STAGE_BYTES) == 5 &&
              planar_waves(2, TW, STAGE_BYTES) == 3, "workgroups per CU of the planar instances");
static_assert(planar_waves(0, TW / 2, STAGE_BYTES16) == 8 && planar_waves(1, TW / 2, STAGE_BYTES16) == 6 && planar_waves(2, TW / 2, STAGE_BYTES16) == 4 &&
              planar_waves(2, TW, STAGE_BYTES16) == 3, "workgroups per CU of the 16-bit planar instances");

extern "C" int mi355_sws_scale_frames_dev(mi355_sws_ctx *c, const mi355_sws_frame *d_frames, int nframes, void *stream)
{
    if (!c || !d_frames || nframes <= 0 || c->h.planar) return -1;
    DeviceScope on(c->device);
    return ctx_launch(c, sws_kernel(c->h), d_frames, nframes, static_cast<hipStream_t>(stream));
}

extern "C" int mi355_sws_scale_planar_frames_dev(mi355_sws_ctx *c, const mi355_sws_planar_frame *d_frames, int nframes, void *stream)
{
    if (!c || !d_frames || nframes <= 0 || !c->h.planar) return -1;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const SwsDev &h = c->h;
    DeviceScope on(c->device);
    const int k = sws_kernel(h);
    if (k == MI355_SWS_K_NV12_PACK || k == MI355_SWS_K_NV12_SPLIT) {
        /* the unscaled packer and splitter: one kernel each, the NV side's pair order as an argument */
        const dim3 grid((h.srcW + PACK_COLS - 1) / PACK_COLS, (h.srcH + PACK_ROWS - 1) / PACK_ROWS, nframes);
        if (k == MI355_SWS_K_NV12_PACK) hipLaunchKernelGGL(k_sws_nv12_pack, grid, dim3(NT), 0, s, h.srcW, h.srcH, h.planar == MI355_SWS_DST_NV21 ? 1 : 0, d_frames);
        else hipLaunchKernelGGL(k_sws_nv12_split, grid, dim3(NT), 0, s, h.srcW, h.srcH, h.src_layout == MI355_SWS_SRC_NV21 ? 1 : 0, d_frames);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    return ctx_launch(c, k, d_frames, nframes, s);
}

/* copy a host plane into a tightly pitched device plane */
static bool plane_h2d(uint8_t *d, int dpitch, const uint8_t *h, int hstride, int wbytes, int rows, hipStream_t s)
{
    return hipMemcpy2DAsync(d, dpitch, h, hstride, wbytes, rows, hipMemcpyHostToDevice, s) == hipSuccess;
}

/* What mi355_sws_scale and mi355_sws_scale_planar share: a picture through the context's own device planes.  A packed picture is a planar one with
 * ONE destination plane (ndst 1).  ow / oh: bytes per row and rows of each destination plane as the device writes them, back: the bytes of a row
 * that go back to the caller (the caller's padding stays untouched), slack: rows (packed) or bytes (planar) behind the destination.
 * Every failure comes back as a negative value and leaves the context usable: the caller (contrib/libav/mi355_sws_glue.c) falls
 * back to the reference's function for that picture.  Strides must be positive and cover a line: sws_scale() itself also
 * takes negative ones (bottom-up pictures, vf_vflip) — not these entry points (-1), a 2-D copy has no negative pitch. */
static int scale_staged(mi355_sws_ctx *c, const uint8_t *const src[3], const int src_stride[3], int ndst, uint8_t *const dst[], const int dst_stride[],
                        const int ow[], const int oh[], const int back[])
{
    const SwsDev &h = c->h;
    const bool planar = h.planar != 0;
    const int B = h.depth > 8 ? 2 : 1;                                  /* bytes per source sample */
    /* an NV12 / NV21 source: two planes, the second one 2 * chrSrcW bytes of pairs; src[2] is not touched */
    /* a packed rgb24 / bgr24 source: one plane of 3 * srcW bytes a row; the halving converter of an odd width also reads pixel srcW, the three
     * bytes behind each row as they lie in the caller's picture (a second copy: they may belong to the next row).  A 32-bit source: four bytes a
     * pixel, pointer and stride on 4-byte multiples (the reference reads dwords) */
    /* a packed 4:2:2 source: one plane of 2 * srcW bytes a row; an odd width's last chroma sample takes the two bytes behind each row in the same way */
    const bool rgb = packed_rgb(h) || yuy2_src(h);
    const int bpx = yuy2_src(h) ? 2 : src_bpx(h);
    if (rgb32_src(h) && (!src[0] || ((reinterpret_cast<uintptr_t>(src[0]) | (uintptr_t)src_stride[0]) & 3))) return -1;
    /* the packer to a packed 4:2:2 destination: with srcW % 4 == 3 its last group takes the luma byte behind each row in the same way */
    const bool pack3 = h.special && yuy2_dst(h) && (h.srcW & 3) == 3;
    /* a fast-bilinear context: the byte behind srcW / chrSrcW of every line of every plane travels with the picture in the same way (ftail) */
    const int nsrc = rgb ? 1 : (h.src_layout ? 2 : 3), ftail = c->fast_bilinear ? 1 : 0, tail = pack3 || ftail ? 1 : (rgb && h.src_hsub && (h.srcW & 1) ? bpx : 0);
    /* a P010 source: two planes of 16-bit words — 2 * srcW bytes of luma and 4 * chrSrcW bytes of pairs a row (B is 2), pointers and strides even */
    const int w[3] = { rgb ? bpx * h.srcW : h.srcW * B, rgb ? 0 : (h.src_layout ? 2 * h.chrSrcW * B : h.chrSrcW * B), h.src_layout ? 0 : h.chrSrcW * B },
              ph[3] = { h.srcH, h.chrSrcH, h.chrSrcH };
    if (p010_src(h))
        for (int p = 0; p < 2; p++) if (!src[p] || ((reinterpret_cast<uintptr_t>(src[p]) | (uintptr_t)src_stride[p]) & 1)) return -1;
    for (int p = 0; p < nsrc; p++) if (!src[p] || src_stride[p] < w[p]) return -1;
    for (int p = 0; p < ndst; p++) if (!dst[p] || dst_stride[p] < back[p]) return -1;
    DeviceScope on(c->device);
    const int pw[3] = { (w[0] + tail + 15) & ~15, (w[1] + ftail + 15) & ~15, (w[2] + ftail + 15) & ~15 };
    int dp[3] = {};
    size_t doff[4] = {};
    for (int p = 0; p < ndst; p++) { dp[p] = (ow[p] + 15) & ~15; doff[p + 1] = doff[p] + (size_t)dp[p] * oh[p]; }
    if (!c->d_dst) {
        uint8_t *ns[3] = { nullptr, nullptr, nullptr }, *nd = nullptr;
        void *nf = nullptr;
        bool ok = true;
        for (int p = 0; p < nsrc && ok; p++) ok = hipMalloc(reinterpret_cast<void **>(&ns[p]), (size_t)pw[p] * ph[p] + 64) == hipSuccess;
        /* a packed destination has one row of slack, the planar planes 64 bytes */
        ok = ok && hipMalloc(reinterpret_cast<void **>(&nd), planar ? doff[ndst] + 64 : (size_t)dp[0] * (oh[0] + 1)) == hipSuccess;
        ok = ok && hipMalloc(&nf, planar ? sizeof(mi355_sws_planar_frame) : sizeof(mi355_sws_frame)) == hipSuccess;
        if (ok && planar) {
            mi355_sws_planar_frame f;
            for (int p = 0; p < 3; p++) { f.src[p] = ns[p]; f.src_stride[p] = pw[p]; f.dst[p] = p < ndst ? nd + doff[p] : nullptr; f.dst_stride[p] = dp[p]; }
            ok = hipMemcpy(nf, &f, sizeof(f), hipMemcpyHostToDevice) == hipSuccess;
        } else if (ok) {
            mi355_sws_frame f;
            for (int p = 0; p < 3; p++) { f.src[p] = ns[p]; f.src_stride[p] = pw[p]; }
            f.dst = nd; f.dst_stride = dp[0];
            ok = hipMemcpy(nf, &f, sizeof(f), hipMemcpyHostToDevice) == hipSuccess;
        }
        if (!ok) {
            for (int p = 0; p < 3; p++) if (ns[p]) (void)hipFree(ns[p]);
            if (nd) (void)hipFree(nd);
            if (nf) (void)hipFree(nf);
            (void)hipGetLastError();
            return -4;
        }
        for (int p = 0; p < 3; p++) c->d_src[p] = ns[p];
        c->d_dst = nd;
        if (planar) c->d_pframe = static_cast<mi355_sws_planar_frame *>(nf);
        else c->d_frame = static_cast<mi355_sws_frame *>(nf);
    }
    for (int p = 0; p < nsrc; p++)
        if (!plane_h2d(c->d_src[p], pw[p], src[p], src_stride[p], w[p], ph[p], c->stream)) { (void)hipGetLastError(); (void)hipStreamSynchronize(c->stream); return -4; }
    if (tail && !plane_h2d(c->d_src[0] + w[0], pw[0], src[0] + w[0], src_stride[0], tail, ph[0], c->stream)) { (void)hipGetLastError(); (void)hipStreamSynchronize(c->stream); return -4; }
    for (int p = 1; p < 3 && ftail; p++)
        if (!plane_h2d(c->d_src[p] + w[p], pw[p], src[p] + w[p], src_stride[p], 1, ph[p], c->stream)) { (void)hipGetLastError(); (void)hipStreamSynchronize(c->stream); return -4; }
    if ((planar ? mi355_sws_scale_planar_frames_dev(c, c->d_pframe, 1, c->stream) : mi355_sws_scale_frames_dev(c, c->d_frame, 1, c->stream)) != 0) {
        (void)hipStreamSynchronize(c->stream);
        return -2;
    }
    for (int p = 0; p < ndst; p++)
        if (back[p] > 0 && oh[p] > 0 && hipMemcpy2DAsync(dst[p], dst_stride[p], c->d_dst + doff[p], dp[p], back[p], oh[p], hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
            (void)hipGetLastError(); (void)hipStreamSynchronize(c->stream); return -4;
        }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return -4;
    return 0;
}

extern "C" int mi355_sws_scale(mi355_sws_ctx *c, const uint8_t *const src[3], const int src_stride[3], uint8_t *dst, int dst_stride)
{
    if (!c || !src || !src_stride || !dst || c->h.planar) return -1;
    const SwsDev &h = c->h;
    if (yuy2_dst(h)) {
        /* a packed 4:2:2 row: whole groups of four bytes, the phantom partner of an odd width's last sample with them; the packer: its groups */
        const int ow = 4 * ((h.dstW + 1) >> 1), back = h.special ? 4 * yuy2_pack_groups(h) : ow;
        const int r = scale_staged(c, src, src_stride, 1, &dst, &dst_stride, &ow, &h.dstH, &back);
        return r ? r : (h.special ? h.srcH : h.dstH);
    }
    /* a 32-bit destination is stored in dwords */
    const int bpp = packed_bpp(h);
    if (bpp == 4 && ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)dst_stride) & 3)) return -1;
    /* only the samples the converter writes go back */
    const int ow = h.dstW * bpp, back = h.special ? (h.dstW & ~1) * bpp : h.dstW * bpp;
    const int r = scale_staged(c, src, src_stride, 1, &dst, &dst_stride, &ow, &h.dstH, &back);
    return r ? r : (h.special ? h.srcH : h.dstH);
}

extern "C" int mi355_sws_scale_planar(mi355_sws_ctx *c, const uint8_t *const src[3], const int src_stride[3], uint8_t *const dst[3], const int dst_stride[3])
{
    if (!c || !src || !src_stride || !dst || !dst_stride || !c->h.planar) return -1;
    const SwsDev &h = c->h;
    if (semi_planar(h)) {
        /* two planes, the second one 2 * chrDstW bytes of pairs; the packer writes (and so hands back) the rounded-down extents only */
        const int ow[2] = { h.dstW, 2 * (h.special ? h.srcW >> 1 : h.chrDstW) }, oh[2] = { h.dstH, h.special ? h.srcH >> 1 : h.chrDstH };
        const int r = scale_staged(c, src, src_stride, 2, dst, dst_stride, ow, oh, ow);
        return r ? r : h.dstH;
    }
    /* the splitter writes (and so hands back) the rounded-down extents only */
    /* ... and the packed-4:2:2 splitter its own: the width rounded up */
    const bool yuy2 = h.special && yuy2_src(h);
    const int cwb = yuy2 ? yuy2_chr_bytes(h) : (h.special ? h.srcW >> 1 : h.chrDstW), chr = yuy2 ? yuy2_chr_rows(h) : (h.special ? h.srcH >> 1 : h.chrDstH);
    if (h.dst_bits > 8) {
        /* 16-bit samples: rows of 2 * width bytes, even strides (scale_staged returns -1 for a stride below a row) */
        for (int p = 0; p < 3; p++) if (dst_stride[p] & 1) return -1;
        const int ow16[3] = { 2 * h.dstW, 2 * h.chrDstW, 2 * h.chrDstW }, oh16[3] = { h.dstH, h.chrDstH, h.chrDstH };
        const int r = scale_staged(c, src, src_stride, 3, dst, dst_stride, ow16, oh16, ow16);
        return r ? r : h.dstH;
    }
    const int ow[3] = { h.dstW, cwb, cwb }, oh[3] = { h.dstH, chr, chr };
    const int r = scale_staged(c, src, src_stride, 3, dst, dst_stride, ow, oh, ow);
    return r ? r : h.dstH;
}

/* ---- Tier-1 line entry points ------------------------------------------------------------------------------ */
/* a line kernel: one workgroup on the staging arena's stream */
template <typename K, typename... A> static void launch_line(K kernel, Arena &a, A... args)
{
    hipLaunchKernelGGL(kernel, dim3(1), dim3(NT), 0, a.stream, args...);
}

/* hScale8To15_c / hScale16To15_c (swscale.c:133-147 / :110-130) of one line: samples of type ST, the sum shifted down by sh */
template <typename ST>
static void hscale_line(int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter, const int32_t *filterPos, int filterSize, int sh)
{
    Arena &a = arena();
    int last = 0;
    for (int i = 0; i < dstW; i++) if (filterPos[i] > last) last = filterPos[i];
    const size_t nsrc = ((size_t)last + filterSize) * sizeof(ST);
    a.reserve(nsrc + (size_t)dstW * filterSize * 2 + (size_t)dstW * 6 + 64);
    const size_t o_src = a.take(nsrc), o_f = a.take((size_t)dstW * filterSize * 2), o_p = a.take((size_t)dstW * 4), o_d = a.take((size_t)dstW * 2);
    std::memcpy(a.h<uint8_t>(o_src), src, nsrc);
    std::memcpy(a.h<int16_t>(o_f), filter, (size_t)dstW * filterSize * 2);
    std::memcpy(a.h<int32_t>(o_p), filterPos, (size_t)dstW * 4);
    a.upload();
    launch_line(k_sws_line_hscale<ST>, a, a.d<int16_t>(o_d), dstW, a.d<const uint8_t>(o_src), a.d<const int16_t>(o_f), a.d<const int32_t>(o_p), filterSize, sh);
    a.download();
    std::memcpy(dst, a.h<int16_t>(o_d), (size_t)dstW * 2);
}
extern "C" void mi355_sws_hscale8to15(int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter, const int32_t *filterPos, int filterSize)
{
    hscale_line<uint8_t>(dst, dstW, src, filter, filterPos, filterSize, 7);
}
/* uint16_t samples below 1 << depth */
extern "C" void mi355_sws_hscale16to15(int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter, const int32_t *filterPos, int filterSize, int depth)
{
    hscale_line<uint16_t>(dst, dstW, src, filter, filterPos, filterSize, depth - 1);
}

/* rgb24ToY_c / bgr24ToY_c and the ...ToUV_c / ...ToUV_half_c pairs (input.c:539-623) of one line */
extern "C" void mi355_sws_rgb24ToY(uint8_t *dst, const uint8_t *src, int width, int bgr)
{
    if (width <= 0) return;
    sws_line<1>(k_sws_line_rgb24_y, &dst, src, (size_t)3 * width, width, bgr);
}
extern "C" void mi355_sws_rgb24ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int bgr, int half)
{
    if (width <= 0) return;
    uint8_t *const out[2] = { dstU, dstV };
    sws_line<2>(k_sws_line_rgb24_uv, out, src, (size_t)(half ? 6 : 3) * width, width, bgr, half);
}

/* lumRangeFromJpeg_c / lumRangeToJpeg_c and chrRangeFromJpeg_c / chrRangeToJpeg_c (swscale.c:168-198) of one line, in place */
static void range_line(int16_t *const lines[], int n, int width, const SwsRangeMap &m)
{
    if (width <= 0) return;
    Arena &a = arena();
    const size_t bytes = ((size_t)width * 2 + 15) & ~(size_t)15;
    a.reserve(n * bytes + 64);
    const size_t o = a.take(n * bytes);
    for (int k = 0; k < n; k++) std::memcpy(a.h<uint8_t>(o) + k * bytes, lines[k], (size_t)width * 2);
    a.upload();
    for (int k = 0; k < n; k++) launch_line(k_sws_line_range, a, reinterpret_cast<int16_t *>(a.d<uint8_t>(o) + k * bytes), width, m);
    a.download();
    for (int k = 0; k < n; k++) std::memcpy(lines[k], a.h<uint8_t>(o) + k * bytes, (size_t)width * 2);
}
extern "C" void mi355_sws_lumConvertRange(int16_t *dst, int width, int to_jpeg)
{
    range_line(&dst, 1, width, range_map(to_jpeg ? MI355_SWS_RANGE_TO_JPEG : MI355_SWS_RANGE_FROM_JPEG, false));
}
extern "C" void mi355_sws_chrConvertRange(int16_t *dstU, int16_t *dstV, int width, int to_jpeg)
{
    int16_t *const lines[2] = { dstU, dstV };
    range_line(lines, 2, width, range_map(to_jpeg ? MI355_SWS_RANGE_TO_JPEG : MI355_SWS_RANGE_FROM_JPEG, true));
}

static size_t pack_rows(Arena &a, const int16_t **rows, int n, int elems, int pitch)
{
    const size_t o = a.take((size_t)(n > 0 ? n : 1) * pitch * 2);
    for (int j = 0; j < n; j++) std::memcpy(a.h<int16_t>(o) + (size_t)j * pitch, rows[j], (size_t)elems * 2);
    return o;
}

static void plane_line(const int16_t *filter, int fs, const int16_t **rows, uint8_t *dest, int dstW, const uint8_t *dither, int offset)
{
    Arena &a = arena();
    const int n = fs ? fs : 1, pitch = (dstW + 7) & ~7;
    a.reserve((size_t)n * pitch * 2 + (size_t)n * 2 + (size_t)dstW + 128);
    const size_t o_r = pack_rows(a, rows, n, dstW, pitch), o_f = a.take((size_t)n * 2), o_di = a.take(8), o_d = a.take((size_t)dstW);
    if (fs) std::memcpy(a.h<int16_t>(o_f), filter, (size_t)fs * 2);
    std::memcpy(a.h<uint8_t>(o_di), dither, 8);
    a.upload();
    launch_line(k_sws_line_plane, a, a.d<const int16_t>(o_f), fs, a.d<const int16_t>(o_r), pitch, a.d<uint8_t>(o_d), dstW, a.d<const uint8_t>(o_di), offset);
    a.download();
    std::memcpy(dest, a.h<uint8_t>(o_d), (size_t)dstW);
}
extern "C" void mi355_sws_yuv2planeX_8(const int16_t *filter, int filterSize, const int16_t **src, uint8_t *dest, int dstW, const uint8_t *dither, int offset)
{
    plane_line(filter, filterSize, src, dest, dstW, dither, offset);
}
extern "C" void mi355_sws_yuv2plane1_8(const int16_t *src, uint8_t *dest, int dstW, const uint8_t *dither, int offset)
{
    plane_line(nullptr, 0, &src, dest, dstW, dither, offset);
}
/* yuv2planeX_9LE_c / _10LE_c and yuv2plane1_9LE_c / _10LE_c (output.c:183-236) of one line: bits 9 or 10, anything else does nothing */
static void plane_line16(const int16_t *filter, int fs, const int16_t **rows, uint16_t *dest, int dstW, int bits)
{
    if ((bits != 9 && bits != 10) || dstW <= 0) return;
    Arena &a = arena();
    const int n = fs ? fs : 1, pitch = (dstW + 7) & ~7;
    a.reserve((size_t)n * pitch * 2 + (size_t)n * 2 + (size_t)dstW * 2 + 128);
    const size_t o_r = pack_rows(a, rows, n, dstW, pitch), o_f = a.take((size_t)n * 2), o_d = a.take((size_t)dstW * 2);
    if (fs) std::memcpy(a.h<int16_t>(o_f), filter, (size_t)fs * 2);
    a.upload();
    launch_line(k_sws_line_plane16, a, a.d<const int16_t>(o_f), fs, a.d<const int16_t>(o_r), pitch, a.d<uint16_t>(o_d), dstW, bits);
    a.download();
    std::memcpy(dest, a.h<uint16_t>(o_d), (size_t)dstW * 2);
}
extern "C" void mi355_sws_yuv2planeX_nbps(const int16_t *filter, int filterSize, const int16_t **src, uint16_t *dest, int dstW, int bits)
{
    if (filterSize < 1) return;
    plane_line16(filter, filterSize, src, dest, dstW, bits);
}
extern "C" void mi355_sws_yuv2plane1_nbps(const int16_t *src, uint16_t *dest, int dstW, int bits)
{
    plane_line16(nullptr, 0, &src, dest, dstW, bits);
}

extern "C" void mi355_sws_yuv2nv12cX(const int16_t *chrFilter, int chrFilterSize, const int16_t **chrUSrc, const int16_t **chrVSrc, uint8_t *dest, int chrDstW,
                                     const uint8_t *chrDither, int swap_uv)
{
    Arena &a = arena();
    const int n = chrFilterSize, pitch = (chrDstW + 7) & ~7;
    a.reserve((size_t)2 * n * pitch * 2 + (size_t)n * 2 + (size_t)2 * chrDstW + 192);
    const size_t o_u = pack_rows(a, chrUSrc, n, chrDstW, pitch), o_v = pack_rows(a, chrVSrc, n, chrDstW, pitch);
    const size_t o_f = a.take((size_t)n * 2 + 2), o_di = a.take(8), o_d = a.take((size_t)2 * chrDstW);
    std::memcpy(a.h<int16_t>(o_f), chrFilter, (size_t)n * 2);
    std::memcpy(a.h<uint8_t>(o_di), chrDither, 8);
    a.upload();
    launch_line(k_sws_line_nv12, a, a.d<const int16_t>(o_f), n, a.d<const int16_t>(o_u), a.d<const int16_t>(o_v), pitch, a.d<uint8_t>(o_d), chrDstW,
                a.d<const uint8_t>(o_di), swap_uv);
    a.download();
    std::memcpy(dest, a.h<uint8_t>(o_d), (size_t)2 * chrDstW);
}

/* dst_format 0: rgb24 (k_sws_line_rgb); MI355_SWS_DST_BGR24 ... _ABGR: k_sws_line_packed of that form (sws_packed.hip), pairs of 6 or 8 bytes;
 * MI355_SWS_DST_YUYV422 ... _YVYU422: of DST_YUY2 (sws_yuy2dst.hip), groups of 4 bytes, luts not read */
/* alp: the ls alpha lines of the _a entries (a 32-bit order): k_sws_line_packed_a (sws_rgb32.hip) */
static void rgb_line(const mi355_sws_luts *luts, int mode, const int16_t *lumF, const int16_t **l, int ls, const int16_t *chrF,
                     const int16_t **u, const int16_t **v, int cs, uint8_t *dest, int dstW, int yalpha, int uvalpha, int dst_format = 0, const int16_t **alp = nullptr)
{
    Arena &a = arena();
    const int npair = (dstW + 1) >> 1, pitch = (2 * npair + 7) & ~7, pb = sws_yuy2_dst(dst_format) ? 4 : (dst_format >= MI355_SWS_DST_RGBA ? 8 : 6);
    a.reserve(sizeof(mi355_sws_luts) + (size_t)(2 * ls + 2 * cs + 4) * pitch * 2 + (size_t)(ls + cs) * 2 + (size_t)npair * pb + 256);
    const size_t o_t = a.take(sizeof(mi355_sws_luts));
    if (luts) std::memcpy(a.h<uint8_t>(o_t), luts, sizeof(mi355_sws_luts));      /* (a packed 4:2:2 order reads none) */
    const size_t o_l = pack_rows(a, l, ls, 2 * npair, pitch), o_u = pack_rows(a, u, cs, npair, pitch), o_v = pack_rows(a, v, cs, npair, pitch);
    const size_t o_a = alp ? pack_rows(a, alp, ls, 2 * npair, pitch) : 0;
    const size_t o_lf = a.take((size_t)ls * 2 + 2), o_cf = a.take((size_t)cs * 2 + 2), o_d = a.take((size_t)npair * pb);
    if (lumF) std::memcpy(a.h<int16_t>(o_lf), lumF, (size_t)ls * 2);
    if (chrF) std::memcpy(a.h<int16_t>(o_cf), chrF, (size_t)cs * 2);
    a.upload();
    const SwsLine n{ a.d<const mi355_sws_luts>(o_t), mode, a.d<const int16_t>(o_lf), a.d<const int16_t>(o_l), ls, a.d<const int16_t>(o_cf), a.d<const int16_t>(o_u),
                     a.d<const int16_t>(o_v), cs, alp ? a.d<const int16_t>(o_a) : nullptr, pitch, a.d<uint8_t>(o_d), dstW, yalpha, uvalpha };
    if (dst_format) {
        SwsKey key{};
        key.kernel = SWS_KERNEL_LINE; key.dst = dst_form(dst_format); key.alpha = alp != nullptr;
        const SwsOperands op{ dim3(1), a.stream, nullptr, nullptr, nullptr, nullptr, 0, 0,
                              key.dst == DST_RGB32 ? sws_rgb32_sel(dst_format) : (key.dst == DST_YUY2 ? sws_yuy2_dst_sel(dst_format) : 0u), &n };
        if (!(alp ? mi355_sws_launch_rgb32(key, op) : (key.dst == DST_YUY2 ? mi355_sws_launch_yuy2dst(key, op) : mi355_sws_launch_packed(key, op)))) {
            std::fprintf(stderr, "mi355dsp: no line kernel for destination format %d%s\n", dst_format, alp ? " with alpha" : "");
            std::abort();
        }
    } else
    launch_line(k_sws_line_rgb, a, n.luts, n.mode, n.lumF, n.l, n.ls, n.chrF, n.u, n.v, n.cs, n.pitch, n.dest, n.dstW, n.yalpha, n.uvalpha);
    a.download();
    std::memcpy(dest, a.h<uint8_t>(o_d), (size_t)npair * pb);   /* like the reference: whole pairs, also for odd dstW */
}
extern "C" void mi355_sws_yuv2rgb24_X(const mi355_sws_luts *luts, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize,
                                      const int16_t *chrFilter, const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize,
                                      uint8_t *dest, int dstW)
{
    rgb_line(luts, 0, lumFilter, lumSrc, lumFilterSize, chrFilter, chrUSrc, chrVSrc, chrFilterSize, dest, dstW, 0, 0);
}
extern "C" void mi355_sws_yuv2rgb24_2(const mi355_sws_luts *luts, const int16_t *buf[2], const int16_t *ubuf[2], const int16_t *vbuf[2],
                                      uint8_t *dest, int dstW, int yalpha, int uvalpha)
{
    rgb_line(luts, 2, nullptr, buf, 2, nullptr, ubuf, vbuf, 2, dest, dstW, yalpha, uvalpha);
}
extern "C" void mi355_sws_yuv2rgb24_1(const mi355_sws_luts *luts, const int16_t *buf0, const int16_t *ubuf[2], const int16_t *vbuf[2],
                                      uint8_t *dest, int dstW, int uvalpha)
{
    /* ubuf[1]/vbuf[1] are only looked at when uvalpha >= 2048 (output.c:1052, :1079) */
    const int cs = uvalpha < 2048 ? 1 : 2;
    rgb_line(luts, 1, nullptr, &buf0, 1, nullptr, ubuf, vbuf, cs, dest, dstW, 0, uvalpha);
}

/* yuv2rgb_c_24_rgb / yuv2rgb_c_24_bgr / yuv2rgb_c_32 (yuv2rgb.c:237-394) on one 4:2:0 slice, to dst_format 0 (rgb24) or MI355_SWS_DST_BGR24 ... _ABGR;
 * who: the entry point that was called */
static int c24_slice(const char *who, const mi355_sws_luts *luts, int dst_format, int dstW, const uint8_t *const src[3], const int srcStride[3], int srcSliceY, int srcSliceH,
                     uint8_t *dst, int dstStride)
{
    if (dst_format != 0 && !packed_dst(dst_format)) return -1;
    if (!ready()) { std::fprintf(stderr, "mi355dsp: %s without mi355_init(); no CPU fallback\n", who); std::abort(); }
    const int bpp = dst_format >= MI355_SWS_DST_RGBA ? 4 : 3;
    if (bpp == 4 && ((reinterpret_cast<uintptr_t>(dst) | (uintptr_t)dstStride) & 3)) return -1;      /* a 32-bit destination is stored in dwords */
    /* a slice may be a whole picture: device buffers per call instead of the staging arena */
    const int rows = srcSliceH, cw = dstW >> 1, crow = (rows + 1) >> 1;   /* even slices, as the reference's callers guarantee */
    const int pw[3] = { (dstW + 15) & ~15, (cw + 15) & ~15, (cw + 15) & ~15 }, ph[3] = { rows, crow, crow }, w[3] = { dstW & ~1, cw, cw };
    const int dpitch = (dstW * bpp + 15) & ~15;
    hipStream_t s = arena().stream;
    mi355_sws_frame f, *d_f;
    uint8_t *d_l, *d_dst;
    for (int p = 0; p < 3; p++) {
        uint8_t *d;
        MI355_CHECK(hipMalloc(reinterpret_cast<void **>(&d), (size_t)pw[p] * (ph[p] + 1) + 64));
        plane_h2d(d, pw[p], src[p], srcStride[p], w[p], ph[p], s);
        f.src[p] = d; f.src_stride[p] = pw[p];
    }
    MI355_CHECK(hipMalloc(reinterpret_cast<void **>(&d_dst), (size_t)dpitch * (rows + 1)));
    MI355_CHECK(hipMalloc(reinterpret_cast<void **>(&d_f), sizeof(f)));
    MI355_CHECK(hipMalloc(reinterpret_cast<void **>(&d_l), sizeof(mi355_sws_luts)));
    f.dst = d_dst; f.dst_stride = dpitch;
    MI355_CHECK(hipMemcpyAsync(d_f, &f, sizeof(f), hipMemcpyHostToDevice, s));
    MI355_CHECK(hipMemcpyAsync(d_l, luts, sizeof(mi355_sws_luts), hipMemcpyHostToDevice, s));
    SwsKey key{};
    key.kernel = SWS_KERNEL_C24; key.src = SWS_SRC_P8; key.dst = dst_form(dst_format);
    const bool launched = sws_run(key, SwsOperands{ sws_c24_grid(dstW, rows, 1), s, nullptr, nullptr, d_f, reinterpret_cast<const mi355_sws_luts *>(d_l), dstW, rows,
                                                    bpp == 4 ? sws_rgb32_sel(dst_format) : 0u, nullptr });
    MI355_CHECK(hipMemcpy2DAsync(dst + (ptrdiff_t)srcSliceY * dstStride, dstStride, d_dst, dpitch, (dstW & ~1) * bpp, rows, hipMemcpyDeviceToHost, s));
    MI355_CHECK(hipStreamSynchronize(s));
    for (int p = 0; p < 3; p++) MI355_CHECK(hipFree(const_cast<uint8_t *>(f.src[p])));
    MI355_CHECK(hipFree(d_dst)); MI355_CHECK(hipFree(d_f)); MI355_CHECK(hipFree(d_l));
    return launched ? srcSliceH : -2;
}
extern "C" int mi355_sws_yuv2rgb_c_24_rgb(const mi355_sws_luts *luts, int dstW, const uint8_t *const src[3], const int srcStride[3],
                                          int srcSliceY, int srcSliceH, uint8_t *dst, int dstStride)
{
    return c24_slice("mi355_sws_yuv2rgb_c_24_rgb", luts, 0, dstW, src, srcStride, srcSliceY, srcSliceH, dst, dstStride);
}

/* ---- the same entries for any packed destination (dst_format 0: rgb24, the entries above; MI355_SWS_DST_BGR24 ... _ABGR) ---------------- */
static bool packed_line_format(int dst_format) { return one_plane_dst(dst_format); }
extern "C" void mi355_sws_yuv2packed_X(const mi355_sws_luts *luts, int dst_format, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize,
                                       const int16_t *chrFilter, const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize,
                                       uint8_t *dest, int dstW)
{
    if (!packed_line_format(dst_format)) return;
    rgb_line(luts, 0, lumFilter, lumSrc, lumFilterSize, chrFilter, chrUSrc, chrVSrc, chrFilterSize, dest, dstW, 0, 0, dst_format);
}
extern "C" void mi355_sws_yuv2packed_2(const mi355_sws_luts *luts, int dst_format, const int16_t *buf[2], const int16_t *ubuf[2], const int16_t *vbuf[2],
                                       uint8_t *dest, int dstW, int yalpha, int uvalpha)
{
    if (!packed_line_format(dst_format)) return;
    rgb_line(luts, 2, nullptr, buf, 2, nullptr, ubuf, vbuf, 2, dest, dstW, yalpha, uvalpha, dst_format);
}
extern "C" void mi355_sws_yuv2packed_1(const mi355_sws_luts *luts, int dst_format, const int16_t *buf0, const int16_t *ubuf[2], const int16_t *vbuf[2],
                                       uint8_t *dest, int dstW, int uvalpha)
{
    if (!packed_line_format(dst_format)) return;
    const int cs = uvalpha < 2048 ? 1 : 2;                      /* as mi355_sws_yuv2rgb24_1 */
    rgb_line(luts, 1, nullptr, &buf0, 1, nullptr, ubuf, vbuf, cs, dest, dstW, 0, uvalpha, dst_format);
}

/* the alpha forms of the three (yuv2rgba32_X_c ... with hasAlpha, output.c:937-1110): a 32-bit order, the alpha line(s) beside the luma line(s) */
static bool alpha_line_format(int dst_format) { return dst_format >= MI355_SWS_DST_RGBA && dst_format <= MI355_SWS_DST_ABGR; }
extern "C" void mi355_sws_yuv2packed_X_a(const mi355_sws_luts *luts, int dst_format, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize,
                                         const int16_t *chrFilter, const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize,
                                         const int16_t **alpSrc, uint8_t *dest, int dstW)
{
    if (!alpha_line_format(dst_format) || !alpSrc) return;
    rgb_line(luts, 0, lumFilter, lumSrc, lumFilterSize, chrFilter, chrUSrc, chrVSrc, chrFilterSize, dest, dstW, 0, 0, dst_format, alpSrc);
}
extern "C" void mi355_sws_yuv2packed_2_a(const mi355_sws_luts *luts, int dst_format, const int16_t *buf[2], const int16_t *ubuf[2], const int16_t *vbuf[2],
                                         const int16_t *abuf[2], uint8_t *dest, int dstW, int yalpha, int uvalpha)
{
    if (!alpha_line_format(dst_format) || !abuf) return;
    rgb_line(luts, 2, nullptr, buf, 2, nullptr, ubuf, vbuf, 2, dest, dstW, yalpha, uvalpha, dst_format, abuf);
}
extern "C" void mi355_sws_yuv2packed_1_a(const mi355_sws_luts *luts, int dst_format, const int16_t *buf0, const int16_t *ubuf[2], const int16_t *vbuf[2],
                                         const int16_t *abuf0, uint8_t *dest, int dstW, int uvalpha)
{
    if (!alpha_line_format(dst_format) || !abuf0) return;
    const int cs = uvalpha < 2048 ? 1 : 2;                      /* as mi355_sws_yuv2rgb24_1 */
    rgb_line(luts, 1, nullptr, &buf0, 1, nullptr, ubuf, vbuf, cs, dest, dstW, 0, uvalpha, dst_format, &abuf0);
}

/* ... and the slice entry with the destination's format */
extern "C" int mi355_sws_yuv2rgb_c(const mi355_sws_luts *luts, int dst_format, int dstW, const uint8_t *const src[3], const int srcStride[3],
                                   int srcSliceY, int srcSliceH, uint8_t *dst, int dstStride)
{
    /* (dst_format 0 is mi355_sws_yuv2rgb_c_24_rgb, under its name) */
    return c24_slice(dst_format ? "mi355_sws_yuv2rgb_c" : "mi355_sws_yuv2rgb_c_24_rgb", luts, dst_format, dstW, src, srcStride, srcSliceY, srcSliceH, dst, dstStride);
}
