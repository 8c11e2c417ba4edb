/*
 * mi355_sws_glue.c — libswscale binding: PRODUCT glue that lives beside the reference's libswscale.
 *
 * Compiled against the reference's own (private) swscale_internal.h; nothing in the reference tree changes.  Link with
 *   -Wl,--wrap=ff_getSwsFunc,--wrap=ff_yuv2rgb_get_func_ptr
 * (the two selectors of SwsContext.swscale, swscale_internal.h:263: ff_getSwsFunc, swscale.c:773, is the last step of
 * sws_init_context, utils.c:1336; ff_yuv2rgb_get_func_ptr, yuv2rgb.c:570, is what ff_get_unscaled_swscale,
 * swscale_unscaled.c:1054, takes for unscaled yuv -> rgb).
 *
 *   whole pictures (default)  both selectors return mi355_swsfunc for yuv420p -> rgb24 contexts: a call that hands over the
 *                          whole picture (srcSliceY == 0, srcSliceH == srcH — what sws_scale() callers such as vf_scale
 *                          without slices do) is ONE device pass (mi355_sws_scale: horizontal scaling, vertical scaling and
 *                          the table look-ups fused, no int16 lines in memory); a sliced call goes to the function the
 *                          reference had chosen.  The device context of a SwsContext is kept in a side table keyed by the
 *                          context's address (no field is added to the private struct) and built at the first call from the
 *                          filter banks and tables the reference built; it is rebuilt when the tables have changed
 *                          (sws_setColorspaceDetails).  Contexts outside the path (other formats, SWS_FULL_CHR_H_INT,
 *                          filters longer than the device tiles hold) keep the reference's function.
 *   inner loops (MI355_SWS_LINES=1)  the arch-hook form (cf. ff_sws_init_swscale_x86, swscale.c:773-790): after the
 *                          reference has chosen its C inner loops, c->hyScale / c->hcScale (hScale8To15_c, swscale.c:133)
 *                          and c->yuv2packed1 / 2 / X (yuv2rgb24_{1,2,X}_c, output.c:937-1110) are pointed at shims that
 *                          forward each call to the device (mi355_sws_hscale8to15, mi355_sws_yuv2rgb24_*).  swscale()'s
 *                          line-pull loop, ring buffers and filter banks stay the reference's.  ff_sws_init_mi355x().
 *   mi355_sws_describe()   fills the plain descriptor of include/mi355_sws.h from a live SwsContext (filter banks and
 *                          yuv->rgb tables exactly as the reference built them): what mi355_sws_create() takes for the
 *                          whole-picture and batched entry points.
 *   planar destinations    yuv420p -> yuv420p / yuv422p / yuv444p contexts of the generic scaler take the same two forms: whole
 *                          pictures through mi355_sws_scale_planar (all three destination planes), inner loops through shims
 *                          over mi355_sws_hscale8to15 / mi355_sws_yuv2planeX_8 / mi355_sws_yuv2plane1_8.
 *                          mi355_sws_describe_planar() fills the descriptor mi355_sws_create_planar() takes; it declines
 *                          SWS_FAST_BILINEAR, range conversion and the unscaled converters (planar_format()).
 *   other sources          yuv420p / yuv422p / yuv444p at 8 bits and their 9le / 10le forms, to rgb24 or to 8-bit yuv420p / yuv422p / yuv444p,
 *                          take the same two forms through mi355_sws_describe_src() / mi355_sws_create_src(): whole pictures, and with
 *                          MI355_SWS_LINES=1 the inner loops (hyScale / hcScale of a deeper source: mi355_sws_hscale16to15).  Declined: what
 *                          taken() / planar_format() decline, contexts with an input converter, big-endian sources and the plane copies
 *                          (no filter banks: planarCopyWrapper).  mi355_sws_describe / _planar keep their answers (yuv420p only).
 *   NV12 / NV21            destinations of the generic scaler take the same two forms under the same conditions as the three-plane ones
 *                          (MI355_SWS_DST_NV12 / _NV21; the inner-loop form also forwards c->yuv2nv12cX to mi355_sws_yuv2nv12cX).
 *                          mi355_sws_describe_src() also recognises the unscaled packer (yuv420p -> nv12 / nv21 at equal size,
 *                          planarToNv12Wrapper: unscaled_special = 1 with the format) for callers of the C ABI; the whole-picture binding
 *                          cannot take it — ff_get_unscaled_swscale sets c->swscale outside the two wrapped selectors — so such a
 *                          context runs the reference's function.
 *   NV12 / NV21 sources    (the reference runs nv12ToUV_c / nv21ToUV_c, c->chrToYV12, on each chroma line and then the ordinary hcScale) take
 *                          the same two forms to every destination above through mi355_sws_describe_fmt() / mi355_sws_create_src_layout():
 *                          whole pictures hand over TWO source planes (srcStride[2] is not looked at); with MI355_SWS_LINES=1 c->chrToYV12
 *                          stays the reference's function — a one-line de-interleave on the host leaves the device nothing to do — and the
 *                          inner loops behind it are forwarded as for the other sources.  mi355_sws_describe_fmt() also recognises the
 *                          unscaled splitter (nv12 / nv21 -> yuv420p at equal size, nv12ToPlanarWrapper) for callers of the C ABI; like the
 *                          packer it is set outside the two wrapped selectors.  mi355_sws_describe / _planar / _src keep their answers:
 *                          they decline these sources.
 *   packed RGB sources     rgb24 / bgr24 (the reference runs c->lumToYV12 and c->chrToYV12 — rgb24ToY_c, rgb24ToUV_c or rgb24ToUV_half_c and their
 *                          bgr24 forms — on each line and then the ordinary hyScale / hcScale) take the same two forms to every destination
 *                          above through mi355_sws_describe_fmt() / mi355_sws_create_src_layout(): whole pictures hand over ONE source plane;
 *                          with MI355_SWS_LINES=1 the two converters are forwarded too (mi355_sws_rgb24ToY / mi355_sws_rgb24ToUV).  The
 *                          unscaled converters of these sources (bgr24ToYv12Wrapper, rgbToRgbWrapper, the copy) stay the reference's.
 *   range conversion       contexts of the generic scaler whose source and destination differ in range, to a YUV destination (yuvj420p <-> yuv420p
 *                          and their kin: c->lumConvertRange / c->chrConvertRange between the horizontal and the vertical pass) take the same
 *                          two forms from every source above through mi355_sws_describe_range() / mi355_sws_create_src_layout_range().  The
 *                          direction is read from the converters the context holds (range_probe), at bind time and again on every call: a
 *                          mismatch is the reference's function for that picture.  With MI355_SWS_LINES=1 the two converters are forwarded
 *                          too (mi355_sws_lumConvertRange / mi355_sws_chrConvertRange).  The four describers above keep declining these.
 *   9- / 10-bit destinations  yuv420p9le / yuv422p9le / yuv444p9le and their 10le forms, from every source above, where the reference runs its generic
 *                          scaler (15-bit intermediates, yuv2planeX_10 / yuv2plane1_10 without dither) take the same two forms through
 *                          mi355_sws_describe_depth() / mi355_sws_create_src_layout_range_depth(); the depth is remembered beside layout and
 *                          range and read again on every call.  With MI355_SWS_LINES=1 c->yuv2planeX / c->yuv2plane1 go to
 *                          mi355_sws_yuv2planeX_nbps / mi355_sws_yuv2plane1_nbps.  Declined: big-endian, 12 / 14 / 16-bit, P010 and gray
 *                          destinations, the plane copies (equal size with equal subsampling: planarCopyWrapper, no banks) and a deep
 *                          destination with range converters.  The five describers above keep declining a destination deeper than 8 bits.
 *   bgr24 / 32-bit RGB     destinations bgr24, rgba, bgra, argb and abgr, from every source above, where the reference runs its generic scaler or
 *                          the unscaled special converter (yuv2rgb_c_24_bgr / yuv2rgb_c_32) take the same two forms through
 *                          mi355_sws_describe_packed() / mi355_sws_create_src_layout_range_depth(); the format is remembered beside the layout and
 *                          read again on every call, and the tables are compared in the form the device context was built from.  With
 *                          MI355_SWS_LINES=1 c->yuv2packedX / 2 / 1 go to mi355_sws_yuv2packed_X / _2 / _1.  Declined: SWS_FULL_CHR_H_INT,
 *                          SWS_FAST_BILINEAR, a source with alpha, 15 / 16-bit and lower RGB, rgb48 / rgba64, planar GBR, rgbToRgbWrapper.  The six
 *                          describers above keep declining these destinations; this one declines rgb24.
 *   32-bit RGB sources     rgba, bgra, argb and abgr (the reference runs rgb32ToY_c / bgr32ToY_c / rgb321ToY_c / bgr321ToY_c, their ...ToUV_c or
 *                          ...ToUV_half_c forms and — where source AND destination have alpha — rgbaToA_c / abgrToA_c on each line, then the
 *                          ordinary hyScale / hcScale) take the same two forms to every destination above through ONE describer,
 *                          mi355_sws_describe_rgb32(), which also reports range, depth and alpha, and mi355_sws_create_src_layout_range_depth() /
 *                          mi355_sws_create_src_layout_alpha().  The converters the context holds are probed with one pixel (rgb32_probe, as
 *                          range_probe does: they are static functions), alpToYV12 must be set exactly when the context has an alpha buffer;
 *                          layout, destination, range, depth and alpha are remembered and described again on every call.  Whole pictures hand
 *                          over ONE source plane; a plane whose pointer or stride is no multiple of 4 is the reference's for that picture
 *                          (mi355_sws_scale returns -1).  With MI355_SWS_LINES=1 the three input converters go to mi355_sws_rgb32ToY / _rgb32ToUV /
 *                          _rgb32ToA and the packed loops of an alpha context to mi355_sws_yuv2packed_X_a / _2_a / _1_a.  Declined: the unscaled
 *                          converters of these sources (rgbToRgbWrapper, the plain copy: no banks), YUVA on either side, 15 / 16-bit RGB,
 *                          SWS_FULL_CHR_H_INT, SWS_FAST_BILINEAR.  The seven describers above keep declining these sources.
 *   packed 4:2:2 sources   yuyv422, uyvy422 and yvyu422 (the reference runs the byte picks yuy2ToY_c / uyvyToY_c and yuy2ToUV_c / yvy2ToUV_c /
 *                          uyvyToUV_c on each line, then the ordinary hyScale / hcScale; at equal size to yuv420p / yuv422p it takes one of
 *                          its four unscaled converters, yuyvToYuv420Wrapper ... uyvyToYuv422Wrapper) have a describer of their own,
 *                          mi355_sws_describe_yuy2(), for mi355_sws_create_src_layout_range_depth(): a context without banks whose swscale
 *                          is one of the four wrappers is described with unscaled_special = 1 (the device's k_sws_yuy2_split) for callers
 *                          of the C ABI — ff_get_unscaled_swscale sets c->swscale without passing a selector this file wraps, so like the
 *                          NV splitter it is not bound here.  The generic scaler's contexts are described in full and bound like those of a
 *                          32-bit source: whole pictures through mi355_swsfunc (described again at every picture; one the creators refuse
 *                          stays the reference's).  With MI355_SWS_LINES=1 their two input converters go to mi355_sws_yuy2ToY / _yuy2ToUV,
 *                          the horizontal and output loops as for every other source.
 *                          The eight describers above keep declining these sources.
 *   packed 4:2:2 destinations  yuyv422, uyvy422 and yvyu422 (c->yuv2packedX / 2 / 1 are yuv2yuyv422_X_c ... yuv2uyvy422_1_c; from 8-bit yuv422p / yuv420p at
 *                          equal size the reference takes one of its four unscaled packers, yuv422pToYuy2Wrapper ... planarToUyvyWrapper) have the
 *                          tenth describer, mi355_sws_describe_yuy2dst(), for mi355_sws_create_src_layout_range_depth(): from every source above,
 *                          with the range read from the converters the context holds.  A context without banks whose source and destination are
 *                          those of a packer is described with unscaled_special = 1 (the device's k_sws_yuy2_pack) for callers of the C ABI and,
 *                          set outside the wrapped selectors, never bound.  The generic scaler's contexts are bound like those of a 32-bit source:
 *                          whole pictures through mi355_swsfunc (described again at every picture; one the creators refuse stays the
 *                          reference's).  With MI355_SWS_LINES=1 c->yuv2packedX / 2 / 1 go to mi355_sws_yuv2packed_X / _2 / _1 with the format (no
 *                          tables), the input converters, horizontal loops and range converters as for the source.  Declined:
 *                          SWS_FAST_BILINEAR scaled contexts, SWS_FULL_CHR_H_INT / _INP where the describers above decline them, alpha / YUVA,
 *                          other sources, and contexts without banks that are not one of the four packers (the plain copy of a packed 4:2:2
 *                          source to its own order; to another order the reference runs its scaler, and that context is taken).  The nine describers above keep declining these destinations.
 *   p010le sources         (the reference runs p010LEToY_c / p010LEToUV_c on each line, word >> 6, then hScale16To15_c with depth 10; it has NO unscaled
 *                          converter from P010, so every context is the generic scaler's) have the eleventh describer, mi355_sws_describe_p010(), for
 *                          mi355_sws_create_src_layout_range_depth(): to every destination above, the packed 4:2:2 ones included, with the range read
 *                          from the converters the context holds.  Bound like a 32-bit source: whole pictures through mi355_swsfunc, TWO source planes
 *                          (described again at every picture; one the creators refuse stays the reference's).  With MI355_SWS_LINES=1 the two input
 *                          converters go to mi355_sws_p010ToY / _p010ToUV, the horizontal loops to mi355_sws_hscale16to15.  Declined: p010be,
 *                          SWS_FULL_CHR_H_INT, a chroma line drop, YUVA destinations (SWS_FAST_BILINEAR leaves a 16-bit source on hScale16To15_c with
 *                          bilinear banks: taken).  The ten describers above keep declining it.
 *   SWS_FAST_BILINEAR      contexts of the planar 8-bit sources (c->hyscale_fast / c->hcscale_fast = hyscale_fast_c / hcscale_fast_c in place of hyScale /
 *                          hcScale: no filter bank, every position and weight from c->lumXInc / c->chrXInc) have the twelfth describer,
 *                          mi355_sws_describe_fast(), for mi355_sws_create_fast_bilinear(): a context is taken when both functions are the C ones
 *                          (fast_probe) and one of the describers above takes it without them (the context is only read).  Bound like a 32-bit source —
 *                          asked before every other describer, since mi355_sws_describe() looks at the formats alone — the two
 *                          increments kept in the slot.  With MI355_SWS_LINES=1 the two functions go to mi355_sws_hyscale_fast / _hcscale_fast, the
 *                          other loops as for the same context without them.  Declined: the flag from any other source (the reference's conversion
 *                          buffer holds an uninitialised sample behind the width there), the x86 build's MMXEXT scaler.
 *   gbrp destinations      (AV_PIX_FMT_GBRP: c->yuv2anyX = yuv2gbrp_full_X_c, the arithmetic yuv -> rgb path under the SWS_FULL_CHR_H_INT the reference forces for
 *                          planar RGB) have the thirteenth describer, mi355_sws_describe_gbrp(), for mi355_sws_create_gbrp(): from every source above, with the
 *                          six c->yuv2rgb_* coefficients as the context holds them.  Bound like a 32-bit source — asked before every other describer, whole
 *                          pictures through mi355_sws_scale_planar (dst[0..2] = G, B, R); coefficients changed since (sws_setColorspaceDetails) build the device
 *                          side anew.  With MI355_SWS_LINES=1 c->yuv2anyX goes to mi355_sws_yuv2gbrp_full_X, the other loops stay the reference's.  Declined:
 *                          gbrap, deeper gbrp, planar RGB sources, rgbToPlanarRgbWrapper (no banks), SWS_FAST_BILINEAR, a chroma line drop.
 * The device is MI355_DEVICE (default 0), as for the decoder bridges.
 */
#include <pthread.h>
#include <stdlib.h>
#include <string.h>
#include "libswscale/swscale.h"
#include "libswscale/swscale_internal.h"
#include "libavutil/pixdesc.h"
#include "mi355_sws.h"
#include "mi355dsp.h"

/* -DMI355_SWS_DESCRIBE_ONLY: only mi355_sws_describe() (a build that wants the descriptor of a context without binding the
 * library: the plain reference library the tests compare against) */
#ifndef MI355_SWS_DESCRIBE_ONLY
static int mi355_swsfunc(SwsContext *c, const uint8_t *src[], int srcStride[], int srcSliceY, int srcSliceH, uint8_t *dst[], int dstStride[]);
#define mi355_swsfunc_entry mi355_swsfunc
static unsigned long n_calls;
unsigned long mi355_sws_glue_calls(void) { return n_calls; }      /* inner-loop calls forwarded so far (diagnostics) */

#endif

static void luts_of(const SwsContext *c, mi355_sws_luts *t)
{
    memcpy(t->y_table, c->yuvTable, 1024);
    for (int i = 0; i < 256; i++) {
        t->rV[i] = c->table_rV[i] - (uint8_t *)c->yuvTable;
        t->gU[i] = c->table_gU[i] - (uint8_t *)c->yuvTable;
        t->gV[i] = c->table_gV[i];
        t->bU[i] = c->table_bU[i] - (uint8_t *)c->yuvTable;
    }
}

/* 0: the context is one this path takes; the chroma lines of SWS_FULL_CHR_H_INT contexts are full width (chrDstHSubSample = 0,
 * utils.c:998-1014; yuv2rgb24_full_X_c, output.c:1392-1452) — not the 2:1 sharing these kernels restate */
static int taken(const SwsContext *c)
{
    return c->srcFormat == AV_PIX_FMT_YUV420P && c->dstFormat == AV_PIX_FMT_RGB24 && !(c->flags & SWS_FULL_CHR_H_INT);
}
static int describe(struct SwsContext *c, mi355_sws_desc *d, int special)
{
    if (!taken(c)) return -1;
    d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
    d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
    d->unscaled_special = special;                               /* yuv2rgb_c_24_rgb was selected (yuv2rgb.c:570) */
    d->hLum = (mi355_sws_filter){ c->hLumFilter, c->hLumFilterPos, c->hLumFilterSize, c->dstW };
    d->hChr = (mi355_sws_filter){ c->hChrFilter, c->hChrFilterPos, c->hChrFilterSize, c->chrDstW };
    d->vLum = (mi355_sws_filter){ c->vLumFilter, c->vLumFilterPos, c->vLumFilterSize, c->dstH };
    d->vChr = (mi355_sws_filter){ c->vChrFilter, c->vChrFilterPos, c->vChrFilterSize, c->dstH };
    luts_of(c, &d->luts);
    return 0;
}
/* the unscaled special converter was selected (ff_get_unscaled_swscale, utils.c:1045: sws_init_context returns before it
 * builds any filter bank) */
int mi355_sws_describe(struct SwsContext *c, mi355_sws_desc *d) { return describe(c, d, c->vLumFilter == NULL); }

/* planar destinations: the MI355_SWS_DST_* of a yuv420p -> yuv420p / yuv422p / yuv444p context whose generic scaler (swscale.c:618-645) the
 * planar kernel restates, else 0.  Declined: SWS_FAST_BILINEAR (hyscale_fast / hcscale_fast, swscale.c:737), range conversion
 * (lumConvertRange / chrConvertRange, :748-763), a chroma line drop (vChrDrop), alpha, and any context without the generic scaler's
 * filter banks (the unscaled converters and plane copies, utils.c:1043-1048). */
static int planar_format(const SwsContext *c)
{
    if (c->srcFormat != AV_PIX_FMT_YUV420P || c->srcBpc != 8 || c->dstBpc != 8) return 0;
    if (c->hyscale_fast || c->hcscale_fast || c->lumConvertRange || c->chrConvertRange || c->vChrDrop) return 0;
    if (c->lumToYV12 || c->chrToYV12 || c->readLumPlanar || c->readChrPlanar || !c->vLumFilter || !c->vChrFilter || !c->hLumFilter || !c->hChrFilter) return 0;
    switch (c->dstFormat) {
    case AV_PIX_FMT_YUV420P: return MI355_SWS_DST_YUV420P;
    case AV_PIX_FMT_YUV422P: return MI355_SWS_DST_YUV422P;
    case AV_PIX_FMT_YUV444P: return MI355_SWS_DST_YUV444P;
    case AV_PIX_FMT_NV12:    return MI355_SWS_DST_NV12;
    case AV_PIX_FMT_NV21:    return MI355_SWS_DST_NV21;
    default: return 0;
    }
}
/* the descriptor of a planar context for mi355_sws_create_planar (0), -1 for a context it declines */
int mi355_sws_describe_planar(struct SwsContext *c, mi355_sws_desc *d, int *dst_format)
{
    const int fmt = planar_format(c);
    if (!fmt) return -1;
    memset(d, 0, sizeof(*d));
    d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
    d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
    d->hLum = (mi355_sws_filter){ c->hLumFilter, c->hLumFilterPos, c->hLumFilterSize, c->dstW };
    d->hChr = (mi355_sws_filter){ c->hChrFilter, c->hChrFilterPos, c->hChrFilterSize, c->chrDstW };
    d->vLum = (mi355_sws_filter){ c->vLumFilter, c->vLumFilterPos, c->vLumFilterSize, c->dstH };
    d->vChr = (mi355_sws_filter){ c->vChrFilter, c->vChrFilterPos, c->vChrFilterSize, c->chrDstH };
    *dst_format = fmt;
    return 0;
}

/* ---- any source of the path: planar yuv 4:2:0 / 4:2:2 / 4:4:4, 8 bits or 9 / 10 bits little endian ------------------------------------
 * 0 and the source's depth and chroma shifts, -1 for another format */
static int source_of(const SwsContext *c, mi355_sws_src *s)
{
    memset(s, 0, sizeof(*s));
    switch (c->srcFormat) {
    case AV_PIX_FMT_YUV420P:     s->depth = 8;  s->hsub = 1; s->vsub = 1; break;
    case AV_PIX_FMT_YUV422P:     s->depth = 8;  s->hsub = 1; s->vsub = 0; break;
    case AV_PIX_FMT_YUV444P:     s->depth = 8;  s->hsub = 0; s->vsub = 0; break;
    case AV_PIX_FMT_YUV420P9LE:  s->depth = 9;  s->hsub = 1; s->vsub = 1; break;
    case AV_PIX_FMT_YUV422P9LE:  s->depth = 9;  s->hsub = 1; s->vsub = 0; break;
    case AV_PIX_FMT_YUV444P9LE:  s->depth = 9;  s->hsub = 0; s->vsub = 0; break;
    case AV_PIX_FMT_YUV420P10LE: s->depth = 10; s->hsub = 1; s->vsub = 1; break;
    case AV_PIX_FMT_YUV422P10LE: s->depth = 10; s->hsub = 1; s->vsub = 0; break;
    case AV_PIX_FMT_YUV444P10LE: s->depth = 10; s->hsub = 0; s->vsub = 0; break;
    default: return -1;
    }
    if (c->chrSrcHSubSample != s->hsub || c->chrSrcVSubSample != s->vsub) return -1;
    memcpy(s->dither, ff_dither_8x8_128, sizeof(s->dither));      /* the rows should_dither selects (swscale.c:553-556) */
    return 0;
}
/* 0: rgb24, MI355_SWS_DST_*: planar or semi-planar, -1: a context this path leaves to the reference.  special: the context's swscale is
 * yuv2rgb_c_24_rgb or, with an NV12 / NV21 destination, planarToNv12Wrapper */
/* the destination of a context that runs the generic scaler, -1 for one this path leaves to the reference */
/* ranged: the context may hold lumConvertRange / chrConvertRange (mi355_sws_describe_range); the existing describers ask with 0.
 * ranged == MI355_ASK_DEEP (mi355_sws_describe_depth alone): the destination is one of the six 9- / 10-bit planar formats instead of the 8-bit
 * ones, and there is no range */
#define MI355_ASK_DEEP 2
/* ranged == MI355_ASK_PACKED (mi355_sws_describe_packed alone): the destination is bgr24 or one of the four 32-bit orders instead; no range either (an
 * RGB destination takes it into its tables) */
#define MI355_ASK_PACKED 3
/* ranged == MI355_ASK_YUY2DST (mi355_sws_describe_yuy2dst alone): the destination is yuyv422 / uyvy422 / yvyu422 instead, with or without range converters
 * (a YUV destination) */
#define MI355_ASK_YUY2DST 4
static int generic_dst_r(const SwsContext *c, int ranged);
/* set by mi355_sws_describe_fast (this thread, for the length of its call): generic_dst_r() then looks past the two fast functions, so that the
 * describers below answer for a fast-bilinear context what they answer for the same context without them — the context itself is not written to */
static __thread int describing_fast;
/* the MI355_SWS_DST_* of a packed 4:2:2 destination, 0 for any other format */
static int yuy2_dst_of(const SwsContext *c)
{
    switch (c->dstFormat) {
    case AV_PIX_FMT_YUYV422: return MI355_SWS_DST_YUYV422;
    case AV_PIX_FMT_UYVY422: return MI355_SWS_DST_UYVY422;
    case AV_PIX_FMT_YVYU422: return MI355_SWS_DST_YVYU422;
    default: return 0;
    }
}
/* the MI355_SWS_DST_* of a packed destination beside rgb24, 0 for any other format.  The reference's RGB32 / BGR32 / RGB32_1 / BGR32_1 are
 * host-endian aliases of the four byte-order names: resolved here, once */
static int packed_dst_of(const SwsContext *c)
{
    switch (c->dstFormat) {
    case AV_PIX_FMT_BGR24: return MI355_SWS_DST_BGR24;
    case AV_PIX_FMT_RGBA:  return MI355_SWS_DST_RGBA;
    case AV_PIX_FMT_BGRA:  return MI355_SWS_DST_BGRA;
    case AV_PIX_FMT_ARGB:  return MI355_SWS_DST_ARGB;
    case AV_PIX_FMT_ABGR:  return MI355_SWS_DST_ABGR;
    default: return 0;
    }
}
/* the MI355_SWS_DST_* and the depth of a 9- / 10-bit little-endian planar destination, 0 for any other format (big endian, 12 / 14 / 16 bits,
 * P010, gray: not ours) */
static int deep_dst(const SwsContext *c, int *depth)
{
    switch (c->dstFormat) {
    case AV_PIX_FMT_YUV420P9LE:  *depth = 9;  return MI355_SWS_DST_YUV420P;
    case AV_PIX_FMT_YUV422P9LE:  *depth = 9;  return MI355_SWS_DST_YUV422P;
    case AV_PIX_FMT_YUV444P9LE:  *depth = 9;  return MI355_SWS_DST_YUV444P;
    case AV_PIX_FMT_YUV420P10LE: *depth = 10; return MI355_SWS_DST_YUV420P;
    case AV_PIX_FMT_YUV422P10LE: *depth = 10; return MI355_SWS_DST_YUV422P;
    case AV_PIX_FMT_YUV444P10LE: *depth = 10; return MI355_SWS_DST_YUV444P;
    default: return 0;
    }
}
static int src_format_r(const SwsContext *c, mi355_sws_src *s, int special, int ranged)
{
    if (source_of(c, s) != 0 || (c->flags & SWS_FULL_CHR_H_INT)) return -1;       /* (every destination below is 8 bits) */
    if (c->lumToYV12 || c->chrToYV12 || c->readLumPlanar || c->readChrPlanar || c->alpToYV12 || c->readAlpPlanar) return -1;      /* an input converter */
    if (special && (c->dstFormat == AV_PIX_FMT_NV12 || c->dstFormat == AV_PIX_FMT_NV21))          /* the packer: planarToNv12Wrapper */
        return c->srcFormat == AV_PIX_FMT_YUV420P ? (c->dstFormat == AV_PIX_FMT_NV12 ? MI355_SWS_DST_NV12 : MI355_SWS_DST_NV21) : -1;
    if (special && ranged == MI355_ASK_PACKED)                    /* yuv2rgb_c_24_bgr / yuv2rgb_c_32: where rgb24 has yuv2rgb_c_24_rgb */
        return packed_dst_of(c) && s->depth == 8 && s->hsub == 1 ? packed_dst_of(c) : -1;
    if (special) return c->dstFormat == AV_PIX_FMT_RGB24 && s->depth == 8 && s->hsub == 1 ? 0 : -1;
    return generic_dst_r(c, ranged);
}
static int src_format(const SwsContext *c, mi355_sws_src *s, int special) { return src_format_r(c, s, special, 0); }
static int generic_dst_r(const SwsContext *c, int ranged)
{
    /* the generic scaler: no fast bilinear, no range conversion (unless asked for), no chroma line drop, and its four banks (an unscaled
     * converter or a plane copy has none, utils.c:1043-1048) */
    const int deep = ranged == MI355_ASK_DEEP, packed = ranged == MI355_ASK_PACKED;
    if ((!describing_fast && (c->hyscale_fast || c->hcscale_fast)) || ((!ranged || deep || packed) && (c->lumConvertRange || c->chrConvertRange)) || c->vChrDrop) return -1;
    if (!c->vLumFilter || !c->vChrFilter || !c->hLumFilter || !c->hChrFilter) return -1;
    if (packed) return packed_dst_of(c) && !isALPHA(c->srcFormat) ? packed_dst_of(c) : -1;
    if (ranged == MI355_ASK_YUY2DST) return yuy2_dst_of(c) && !isALPHA(c->srcFormat) ? yuy2_dst_of(c) : -1;
    if (deep) {
        int bits;
        const int fmt = deep_dst(c, &bits);
        return fmt ? fmt : -1;
    }
    switch (c->dstFormat) {
    case AV_PIX_FMT_RGB24:   return 0;
    case AV_PIX_FMT_YUV420P: return MI355_SWS_DST_YUV420P;
    case AV_PIX_FMT_YUV422P: return MI355_SWS_DST_YUV422P;
    case AV_PIX_FMT_YUV444P: return MI355_SWS_DST_YUV444P;
    case AV_PIX_FMT_NV12:    return MI355_SWS_DST_NV12;
    case AV_PIX_FMT_NV21:    return MI355_SWS_DST_NV21;
    default: return -1;
    }
}
static int describe_src_r(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *dst_format, int special, int ranged)
{
    const int fmt = src_format_r(c, s, special, ranged);
    if (fmt < 0) return -1;
    memset(d, 0, sizeof(*d));
    d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
    d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
    d->unscaled_special = special;
    if (!special) {
        d->hLum = (mi355_sws_filter){ c->hLumFilter, c->hLumFilterPos, c->hLumFilterSize, c->dstW };
        d->hChr = (mi355_sws_filter){ c->hChrFilter, c->hChrFilterPos, c->hChrFilterSize, c->chrDstW };
        d->vLum = (mi355_sws_filter){ c->vLumFilter, c->vLumFilterPos, c->vLumFilterSize, c->dstH };
        d->vChr = (mi355_sws_filter){ c->vChrFilter, c->vChrFilterPos, c->vChrFilterSize, fmt ? c->chrDstH : c->dstH };
    }
    if (!fmt) luts_of(c, &d->luts);
    *dst_format = fmt;
    return 0;
}
static int describe_src(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *dst_format, int special) { return describe_src_r(c, d, s, dst_format, special, 0); }
/* what mi355_sws_create_src takes for a live context (0), -1 for a context this path declines.  A context without the vertical banks whose
 * swscale is the reference's yuv2rgb_c_24_rgb is the unscaled special converter; any other without them (a plane copy) is declined. */
int mi355_sws_describe_src(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *dst_format)
{
    int special = 0;
    if (!c->vLumFilter && (c->dstFormat == AV_PIX_FMT_NV12 || c->dstFormat == AV_PIX_FMT_NV21)) {
        /* swscale_unscaled.c:1040-1044: whatever the flags */
        if (c->srcFormat != AV_PIX_FMT_YUV420P || c->srcW != c->dstW || c->srcH != c->dstH) return -1;
        special = 1;
    } else if (!c->vLumFilter) {
        if (c->dstFormat != AV_PIX_FMT_RGB24 || (c->flags & SWS_ACCURATE_RND) || (c->dstH & 1) || c->srcW != c->dstW || c->srcH != c->dstH ||
            (c->srcFormat != AV_PIX_FMT_YUV420P && c->srcFormat != AV_PIX_FMT_YUV422P)) return -1;
        special = 1;                                             /* swscale_unscaled.c:1051-1055 */
    }
    return describe_src(c, d, s, dst_format, special);
}

/* ---- NV12 / NV21 sources beside the planar ones ------------------------------------------------------------------------------------------
 * src_format() with the source's layout (MI355_SWS_SRC_*): an NV12 / NV21 source is the one context whose input converter this path takes —
 * c->chrToYV12 alone (nv12ToUV_c / nv21ToUV_c, input.c:475-497) — as an 8-bit 4:2:0 source of the layout.  special: nv12ToPlanarWrapper */
static int fmt_format_r(const SwsContext *c, mi355_sws_src *s, int special, int *layout, int ranged)
{
    *layout = c->srcFormat == AV_PIX_FMT_NV12 ? MI355_SWS_SRC_NV12 : (c->srcFormat == AV_PIX_FMT_NV21 ? MI355_SWS_SRC_NV21 :
              (c->srcFormat == AV_PIX_FMT_RGB24 ? MI355_SWS_SRC_RGB24 : (c->srcFormat == AV_PIX_FMT_BGR24 ? MI355_SWS_SRC_BGR24 : MI355_SWS_SRC_PLANAR)));
    if (!*layout) return src_format_r(c, s, special, ranged);
    memset(s, 0, sizeof(*s));
    if (*layout == MI355_SWS_SRC_RGB24 || *layout == MI355_SWS_SRC_BGR24) {
        /* packed RGB: BOTH input converters (rgb24ToY_c / rgb24ToUV_c or rgb24ToUV_half_c and their bgr24 forms, input.c:539-623) and no other;
         * which chroma converter runs is the context's chrSrcHSubSample (utils.c:1023-1038), handed over as it is.  No special converter of
         * these sources is taken (bgr24ToYv12Wrapper, rgbToRgbWrapper, the copy) */
        s->depth = 8; s->hsub = c->chrSrcHSubSample; s->vsub = 0;
        memcpy(s->dither, ff_dither_8x8_128, sizeof(s->dither));
        if (special || c->chrSrcVSubSample != 0 || (c->chrSrcHSubSample & ~1) || (c->flags & SWS_FULL_CHR_H_INT)) return -1;
        if (!c->lumToYV12 || !c->chrToYV12 || c->readLumPlanar || c->readChrPlanar || c->alpToYV12 || c->readAlpPlanar || c->srcBpc != 8) return -1;
        return generic_dst_r(c, ranged);
    }
    s->depth = 8; s->hsub = 1; s->vsub = 1;
    memcpy(s->dither, ff_dither_8x8_128, sizeof(s->dither));
    if (c->chrSrcHSubSample != 1 || c->chrSrcVSubSample != 1 || (c->flags & SWS_FULL_CHR_H_INT)) return -1;
    if (c->lumToYV12 || c->readLumPlanar || c->readChrPlanar || c->alpToYV12 || c->readAlpPlanar) return -1;      /* no other input converter */
    /* (the unscaled path leaves sws_init_context before srcBpc is set and the input converters are chosen: the splitter's context has neither) */
    if (special) return c->dstFormat == AV_PIX_FMT_YUV420P ? MI355_SWS_DST_YUV420P : -1;
    if (c->srcBpc != 8 || !c->chrToYV12) return -1;
    return generic_dst_r(c, ranged);
}
static int fmt_format(const SwsContext *c, mi355_sws_src *s, int special, int *layout) { return fmt_format_r(c, s, special, layout, 0); }
/* what mi355_sws_create_src_layout takes for a live context (0), -1 for a context this path declines: mi355_sws_describe_src plus the two
 * NV sources.  An NV context without the vertical banks is the splitter when it goes to yuv420p at equal size (swscale_unscaled.c:1045-1049,
 * whatever the flags); any other without them (nv12 -> nv12: a plane copy) is declined. */
static int describe_fmt_r(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, int *dst_format, int ranged)
{
    int special = 0;
    const int rgb = c->srcFormat == AV_PIX_FMT_RGB24 || c->srcFormat == AV_PIX_FMT_BGR24;
    if (c->srcFormat != AV_PIX_FMT_NV12 && c->srcFormat != AV_PIX_FMT_NV21 && !rgb) {
        *src_layout = MI355_SWS_SRC_PLANAR;
        return ranged ? describe_src_r(c, d, s, dst_format, 0, ranged) : mi355_sws_describe_src(c, d, s, dst_format);
    }
    if (rgb && !c->vLumFilter) return -1;                        /* an unscaled converter or a copy: the reference's */
    if (!c->vLumFilter) {
        if (c->dstFormat != AV_PIX_FMT_YUV420P || c->srcW != c->dstW || c->srcH != c->dstH) return -1;
        special = 1;
    }
    const int fmt = fmt_format_r(c, s, special, src_layout, ranged);
    if (fmt < 0) return -1;
    memset(d, 0, sizeof(*d));
    d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
    d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
    d->unscaled_special = special;
    if (!special) {
        d->hLum = (mi355_sws_filter){ c->hLumFilter, c->hLumFilterPos, c->hLumFilterSize, c->dstW };
        d->hChr = (mi355_sws_filter){ c->hChrFilter, c->hChrFilterPos, c->hChrFilterSize, c->chrDstW };
        d->vLum = (mi355_sws_filter){ c->vLumFilter, c->vLumFilterPos, c->vLumFilterSize, c->dstH };
        d->vChr = (mi355_sws_filter){ c->vChrFilter, c->vChrFilterPos, c->vChrFilterSize, fmt ? c->chrDstH : c->dstH };
    }
    if (!fmt) luts_of(c, &d->luts);
    *dst_format = fmt;
    return 0;
}
int mi355_sws_describe_fmt(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, int *dst_format)
{
    return describe_fmt_r(c, d, s, src_layout, dst_format, 0);
}

/* ---- range conversion: contexts whose only obstacle above is lumConvertRange / chrConvertRange ---------------------------------------------
 * The MI355_SWS_RANGE_* of the converters the context HOLDS (sws_setColorspaceDetails rewrites c->srcRange after init without touching the
 * pointers; the functions are static in the reference): one sample of 0 through each — luma 2048 / chroma 1992 from-JPEG, -2384 / -2269
 * to-JPEG.  0: neither converter; -1: one of the two only, two directions, other functions, or a destination other than 8 bits — NOTHING is
 * called then: behind the same pointer types a destination of 16 bits holds the ...Jpeg16_c forms (swscale.c:200-236, :757-764), which read and
 * write an int32_t per sample, four bytes where the probe has two; every destination of this path is 8 bits, so such a context is not ours
 * whatever its converters are */
static int range_probe(const SwsContext *c)
{
    int16_t y = 0, u = 0, v = 0;
    if (!c->lumConvertRange && !c->chrConvertRange) return MI355_SWS_RANGE_NONE;
    if (!c->lumConvertRange || !c->chrConvertRange || c->dstBpc != 8) return -1;
    c->lumConvertRange(&y, 1);
    c->chrConvertRange(&u, &v, 1);
    if (y == 2048 && u == 1992 && v == 1992) return MI355_SWS_RANGE_FROM_JPEG;
    if (y == -2384 && u == -2269 && v == -2269) return MI355_SWS_RANGE_TO_JPEG;
    return -1;
}
/* what mi355_sws_create_src_layout_range takes for a live context (0), -1 for a context this path declines: mi355_sws_describe_fmt (range 0)
 * plus the contexts of the generic scaler with a YUV destination that convert the range */
int mi355_sws_describe_range(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, int *dst_format, int *range)
{
    const int r = range_probe(c);
    if (r < 0) return -1;
    *range = r;
    if (!r) return mi355_sws_describe_fmt(c, d, s, src_layout, dst_format);
    /* the reference sets the converters for YUV destinations of its generic scaler only (swscale.c:748, utils.c:1044) */
    if (!c->vLumFilter || isAnyRGB(c->dstFormat)) return -1;
    return describe_fmt_r(c, d, s, src_layout, dst_format, 1) == 0 && *dst_format > 0 ? 0 : -1;
}

/* ---- destinations of 9 or 10 bits: yuv420p9le ... yuv444p10le ------------------------------------------------------------------------------
 * what mi355_sws_create_src_layout_range_depth takes for a live context (0), -1 for a context this path declines: mi355_sws_describe_range
 * (depth 8) plus the contexts of the generic scaler to one of the six formats of deep_dst().  Such a context keeps the 15-bit intermediates
 * (dstBpc <= 15, swscale.c:733-752) and differs from its 8-bit twin in c->yuv2planeX / c->yuv2plane1 alone.  Declined: what generic_dst_r()
 * declines (fast bilinear, a chroma line drop, no banks — at equal size with equal subsampling the reference copies planes,
 * planarCopyWrapper), SWS_FULL_CHR_H_INT, a source the other describers do not take, and a deep destination WITH range converters (the
 * device has no such instance) */
int mi355_sws_describe_depth(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, int *dst_format, int *range, int *dst_depth)
{
    int bits = 8;
    if (!deep_dst(c, &bits)) {
        *dst_depth = 8;
        return mi355_sws_describe_range(c, d, s, src_layout, dst_format, range);
    }
    if (!c->vLumFilter || c->dstBpc != bits) return -1;
    if (describe_fmt_r(c, d, s, src_layout, dst_format, MI355_ASK_DEEP) != 0 || *dst_format <= 0) return -1;
    *range = MI355_SWS_RANGE_NONE;
    *dst_depth = bits;
    return 0;
}

/* ---- packed destinations beside rgb24: bgr24, rgba, bgra, argb, abgr -----------------------------------------------------------------------
 * The tables of such a context in the form of mi355_sws_luts.  bgr24 has the 24-bpp tables (yuv2rgb.c:850-863): luts_of().  A 32-bit order has one
 * uint32_t table of three planes (:864-888): entry i of the r plane holds the clipped value of the 24-bpp table shifted into the r lane (plus 255
 * in the alpha lane, a source without alpha), the g and b planes the same value in their lanes, 1024 and 2048 ELEMENTS up; fill_table gives the three
 * pointer rows the same element offsets into their planes, fill_gv_table a byte offset of four bytes an element.  So y_table[i] is the r lane of
 * entry i and the offset rows are the pointers' element offsets with the plane bases removed */
static void luts_packed(const SwsContext *c, int fmt, mi355_sws_luts *t)
{
    if (fmt == MI355_SWS_DST_BGR24) { luts_of(c, t); return; }
    const uint32_t *y32 = c->yuvTable;
    /* rbase of :865-867: base 8 for the two orders with alpha in the low byte of the host's dword, r above b for RGB32 / RGB32_1 */
    const int base = c->dstFormat == AV_PIX_FMT_RGB32_1 || c->dstFormat == AV_PIX_FMT_BGR32_1 ? 8 : 0;
    const int rbase = base + (c->dstFormat == AV_PIX_FMT_RGB32 || c->dstFormat == AV_PIX_FMT_RGB32_1 ? 16 : 0);
    for (int i = 0; i < 1024; i++) t->y_table[i] = (uint8_t)(y32[i] >> rbase);
    for (int i = 0; i < 256; i++) {
        t->rV[i] = (const uint32_t *)c->table_rV[i] - y32;
        t->gU[i] = (const uint32_t *)c->table_gU[i] - y32 - 1024;
        t->gV[i] = c->table_gV[i] / 4;
        t->bU[i] = (const uint32_t *)c->table_bU[i] - y32 - 2048;
    }
}
/* what mi355_sws_create_src_layout_range_depth (range 0, depth 8) takes for a live context to one of the five formats (0), -1 for every other
 * context — rgb24 included: that is mi355_sws_describe_fmt's.  The generic scaler's contexts under the conditions of the rgb24 ones (no
 * SWS_FULL_CHR_H_INT, no SWS_FAST_BILINEAR, a source without alpha, the four banks); a context without the vertical banks is the unscaled special
 * converter where ff_yuv2rgb_get_func_ptr gave yuv2rgb_c_24_bgr / yuv2rgb_c_32 (swscale_unscaled.c:1051-1055: 8-bit yuv420p / yuv422p at equal size,
 * an even height, no SWS_ACCURATE_RND); any other without them (rgbToRgbWrapper, a copy) is declined */
int mi355_sws_describe_packed(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, int *dst_format)
{
    const int fmt = packed_dst_of(c);
    if (!fmt) return -1;
    if (!c->vLumFilter) {
        if ((c->flags & SWS_ACCURATE_RND) || (c->dstH & 1) || c->srcW != c->dstW || c->srcH != c->dstH ||
            (c->srcFormat != AV_PIX_FMT_YUV420P && c->srcFormat != AV_PIX_FMT_YUV422P)) return -1;
        *src_layout = MI355_SWS_SRC_PLANAR;
        if (describe_src_r(c, d, s, dst_format, 1, MI355_ASK_PACKED) != 0 || *dst_format != fmt) return -1;
    } else if (describe_fmt_r(c, d, s, src_layout, dst_format, MI355_ASK_PACKED) != 0 || *dst_format != fmt) return -1;
    luts_packed(c, fmt, &d->luts);
    return 0;
}

/* ---- packed 32-bit sources: rgba, bgra, argb, abgr -----------------------------------------------------------------------------------------
 * The MI355_SWS_SRC_* of such a source, 0 for any other format (the reference's RGB32 / BGR32 / _1 names are host-endian aliases: resolved here) */
static int rgb32_layout_of(const SwsContext *c)
{
    switch (c->srcFormat) {
    case AV_PIX_FMT_RGBA: return MI355_SWS_SRC_RGBA;
    case AV_PIX_FMT_BGRA: return MI355_SWS_SRC_BGRA;
    case AV_PIX_FMT_ARGB: return MI355_SWS_SRC_ARGB;
    case AV_PIX_FMT_ABGR: return MI355_SWS_SRC_ABGR;
    default: return 0;
    }
}
/* the input converters the context HOLDS are the 32-bit ones of `layout` (the functions are static in the reference: one pixel through each, as
 * range_probe does).  The pixel has its first colour byte at 255, the other two at 0 and alpha at 0x5A; rgb24ToY_c / rgb24ToUV_c give
 * 16 + (K0 * 255 >> 15) ... for it, and the four orders differ in K0 and in where the colour bytes start */
static int rgb32_probe(const SwsContext *c, int layout, int alpha)
{
    static const int RY = 8414, BY = 3208, RU = -4865, BU = 14392, RV = 14392, BV = -2332;      /* input.c:38-47 at RGB2YUV_SHIFT 15 */
    const int bgr = layout == MI355_SWS_SRC_BGRA || layout == MI355_SWS_SRC_ABGR, first = layout == MI355_SWS_SRC_ARGB || layout == MI355_SWS_SRC_ABGR;
    uint32_t px[4] = { 0, 0, 0, 0 };
    uint8_t *b = (uint8_t *)px, y[4] = { 0 }, u[4] = { 0 }, v[4] = { 0 }, a[4] = { 0 };
    if (!c->lumToYV12 || !c->chrToYV12 || (c->alpToYV12 != NULL) != (alpha != 0)) return -1;
    for (int i = 0; i < 2; i++) { b[4 * i + first] = 255; b[4 * i + (first ? 0 : 3)] = 0x5A; }
    c->lumToYV12(y, b, 1, NULL);
    c->chrToYV12(u, v, b, b, 1, NULL);                            /* (the halving form reads both pixels: the same value) */
    if (alpha) c->alpToYV12(a, b, 1, NULL);
    if (y[0] != (((bgr ? BY : RY) * 255 + (33 << 14)) >> 15) || u[0] != (((bgr ? BU : RU) * 255 + (257 << 14)) >> 15) ||
        v[0] != (((bgr ? BV : RV) * 255 + (257 << 14)) >> 15)) return -1;
    return !alpha || a[0] == 0x5A ? 0 : -1;
}
/* what mi355_sws_create_src_layout_range_depth takes for a live context FROM one of the four formats (0), -1 for every other context — the seven
 * describers above keep declining these sources.  The generic scaler's contexts only (the unscaled converters of these sources — rgbToRgbWrapper,
 * the plain copy, the ...ToYv12 wrappers — have no banks): both input converters the 32-bit ones (rgb32_probe), no other reader; to rgb24, to bgr24
 * and the four 32-bit orders, to 8-bit planar / semi-planar YUV with or without range converters, to 9- / 10-bit planar YUV.
 * *alpha: the context carries the source's alpha plane to its 32-bit destination (c->alpPixBuf: both formats have alpha, utils.c:1244) — it then
 * holds alpToYV12 too, and exactly then; the device writes 255 there, so a caller hands such a context over only for pictures whose alpha is 255
 * everywhere or keeps it with the reference.  Declined: SWS_FULL_CHR_H_INT, SWS_FAST_BILINEAR, a chroma line drop, YUVA destinations, 15 / 16-bit RGB */
int mi355_sws_describe_rgb32(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, int *dst_format, int *range, int *dst_depth, int *alpha)
{
    const int layout = rgb32_layout_of(c);
    int fmt, bits = 8;
    if (!layout || !c->vLumFilter || !c->vChrFilter || !c->hLumFilter || !c->hChrFilter) return -1;
    if (c->hyscale_fast || c->hcscale_fast || c->vChrDrop || (c->flags & SWS_FULL_CHR_H_INT)) return -1;
    if (c->chrSrcVSubSample != 0 || (c->chrSrcHSubSample & ~1) || c->srcBpc != 8 || c->readLumPlanar || c->readChrPlanar || c->readAlpPlanar) return -1;
    *alpha = c->alpPixBuf != NULL;
    if (rgb32_probe(c, layout, *alpha) != 0) return -1;
    const int r = range_probe(c);
    if (r < 0) return -1;
    if (deep_dst(c, &bits)) {
        if (r || c->dstBpc != bits) return -1;
        fmt = deep_dst(c, &bits);
    } else if (packed_dst_of(c) || c->dstFormat == AV_PIX_FMT_RGB24) {
        if (r) return -1;
        fmt = packed_dst_of(c);
    } else {
        switch (c->dstFormat) {
        case AV_PIX_FMT_YUV420P: fmt = MI355_SWS_DST_YUV420P; break;
        case AV_PIX_FMT_YUV422P: fmt = MI355_SWS_DST_YUV422P; break;
        case AV_PIX_FMT_YUV444P: fmt = MI355_SWS_DST_YUV444P; break;
        case AV_PIX_FMT_NV12:    fmt = MI355_SWS_DST_NV12; break;
        case AV_PIX_FMT_NV21:    fmt = MI355_SWS_DST_NV21; break;
        default: return -1;
        }
    }
    if (*alpha && fmt < MI355_SWS_DST_RGBA) return -1;            /* (the reference allocates alpPixBuf for a destination with alpha only) */
    const int yuv = fmt >= MI355_SWS_DST_YUV420P && fmt <= MI355_SWS_DST_NV21;
    memset(s, 0, sizeof(*s));
    s->depth = 8; s->hsub = c->chrSrcHSubSample; s->vsub = 0;
    memcpy(s->dither, ff_dither_8x8_128, sizeof(s->dither));
    memset(d, 0, sizeof(*d));
    d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
    d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
    d->hLum = (mi355_sws_filter){ c->hLumFilter, c->hLumFilterPos, c->hLumFilterSize, c->dstW };
    d->hChr = (mi355_sws_filter){ c->hChrFilter, c->hChrFilterPos, c->hChrFilterSize, c->chrDstW };
    d->vLum = (mi355_sws_filter){ c->vLumFilter, c->vLumFilterPos, c->vLumFilterSize, c->dstH };
    d->vChr = (mi355_sws_filter){ c->vChrFilter, c->vChrFilterPos, c->vChrFilterSize, yuv ? c->chrDstH : c->dstH };
    if (!fmt) luts_of(c, &d->luts);
    else if (!yuv) luts_packed(c, fmt, &d->luts);
    *src_layout = layout; *dst_format = fmt; *range = r; *dst_depth = bits;
    return 0;
}

/* ---- packed 4:2:2 sources: yuyv422, uyvy422, yvyu422 ---------------------------------------------------------------------------------------
 * The MI355_SWS_SRC_* of such a source, 0 for any other format */
static int yuy2_layout_of(const SwsContext *c)
{
    switch (c->srcFormat) {
    case AV_PIX_FMT_YUYV422: return MI355_SWS_SRC_YUYV422;
    case AV_PIX_FMT_UYVY422: return MI355_SWS_SRC_UYVY422;
    case AV_PIX_FMT_YVYU422: return MI355_SWS_SRC_YVYU422;
    default: return 0;
    }
}
/* the input converters the context HOLDS are the byte picks of `layout` (the functions are static in the reference: one group of four distinct bytes
 * through each, as rgb32_probe does) */
static int yuy2_probe(const SwsContext *c, int layout)
{
    static const uint8_t b[8] = { 0x11, 0x22, 0x33, 0x44, 0x55, 0x66, 0x77, 0x88 };
    const int lum = layout == MI355_SWS_SRC_UYVY422, uo = layout == MI355_SWS_SRC_UYVY422 ? 0 : (layout == MI355_SWS_SRC_YVYU422 ? 3 : 1);
    uint8_t y[4] = { 0 }, u[4] = { 0 }, v[4] = { 0 };
    if (!c->lumToYV12 || !c->chrToYV12 || c->alpToYV12) return -1;
    c->lumToYV12(y, b, 1, NULL);
    c->chrToYV12(u, v, b, b, 1, NULL);
    return y[0] == b[lum] && u[0] == b[uo] && v[0] == b[uo ^ 2] ? 0 : -1;
}
/* what mi355_sws_create_src_layout_range_depth takes for a live context FROM one of the three formats (0), -1 for every other context — the eight
 * describers above keep declining these sources.  A context without the vertical banks is one of the four unscaled converters (yuyvToYuv420Wrapper,
 * uyvyToYuv420Wrapper, yuyvToYuv422Wrapper, uyvyToYuv422Wrapper, swscale_unscaled.c:1140-1149: yuyv422 / uyvy422 to yuv420p / yuv422p at equal size and
 * equal range, whatever the flags): unscaled_special = 1, no banks; any other without them (a copy, the packed-to-packed wrappers, yvyu422) is
 * declined.  The generic scaler's contexts: both input converters the byte picks of the layout (yuy2_probe), no other reader; to rgb24, bgr24 and the four
 * 32-bit orders, to 8-bit planar / semi-planar YUV with or without range converters, to 9- / 10-bit planar YUV — described in full, whether or not the
 * device's creators take them yet.  Declined: SWS_FULL_CHR_H_INT, SWS_FAST_BILINEAR, a chroma line drop, YUVA destinations, 15 / 16-bit RGB */
int mi355_sws_describe_yuy2(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, int *dst_format, int *range, int *dst_depth)
{
    const int layout = yuy2_layout_of(c);
    int fmt, bits = 8, r = MI355_SWS_RANGE_NONE;
    if (!layout || c->chrSrcHSubSample != 1 || c->chrSrcVSubSample != 0) return -1;
    const int special = !c->vLumFilter;
    if (special) {
        if (layout == MI355_SWS_SRC_YVYU422 || !c->swscale || c->srcW != c->dstW || c->srcH != c->dstH || c->hLumFilter || c->hChrFilter || c->vChrFilter) return -1;
        if (c->dstFormat != AV_PIX_FMT_YUV420P && c->dstFormat != AV_PIX_FMT_YUV422P) return -1;
        fmt = c->dstFormat == AV_PIX_FMT_YUV420P ? MI355_SWS_DST_YUV420P : MI355_SWS_DST_YUV422P;
    } else {
        if (!c->vChrFilter || !c->hLumFilter || !c->hChrFilter) return -1;
        if (c->hyscale_fast || c->hcscale_fast || c->vChrDrop || (c->flags & SWS_FULL_CHR_H_INT)) return -1;
        if (c->srcBpc != 8 || c->readLumPlanar || c->readChrPlanar || c->readAlpPlanar || c->alpPixBuf) return -1;
        if (yuy2_probe(c, layout) != 0) return -1;
        r = range_probe(c);
        if (r < 0) return -1;
        if (deep_dst(c, &bits)) {
            if (r || c->dstBpc != bits) return -1;
            fmt = deep_dst(c, &bits);
        } else if (packed_dst_of(c) || c->dstFormat == AV_PIX_FMT_RGB24) {
            if (r) return -1;
            fmt = packed_dst_of(c);
        } else {
            switch (c->dstFormat) {
            case AV_PIX_FMT_YUV420P: fmt = MI355_SWS_DST_YUV420P; break;
            case AV_PIX_FMT_YUV422P: fmt = MI355_SWS_DST_YUV422P; break;
            case AV_PIX_FMT_YUV444P: fmt = MI355_SWS_DST_YUV444P; break;
            case AV_PIX_FMT_NV12:    fmt = MI355_SWS_DST_NV12; break;
            case AV_PIX_FMT_NV21:    fmt = MI355_SWS_DST_NV21; break;
            default: return -1;
            }
        }
    }
    const int yuv = fmt >= MI355_SWS_DST_YUV420P && fmt <= MI355_SWS_DST_NV21;
    memset(s, 0, sizeof(*s));
    s->depth = 8; s->hsub = 1; s->vsub = 0;
    memcpy(s->dither, ff_dither_8x8_128, sizeof(s->dither));
    memset(d, 0, sizeof(*d));
    d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
    d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
    d->unscaled_special = special;
    if (!special) {
        d->hLum = (mi355_sws_filter){ c->hLumFilter, c->hLumFilterPos, c->hLumFilterSize, c->dstW };
        d->hChr = (mi355_sws_filter){ c->hChrFilter, c->hChrFilterPos, c->hChrFilterSize, c->chrDstW };
        d->vLum = (mi355_sws_filter){ c->vLumFilter, c->vLumFilterPos, c->vLumFilterSize, c->dstH };
        d->vChr = (mi355_sws_filter){ c->vChrFilter, c->vChrFilterPos, c->vChrFilterSize, yuv ? c->chrDstH : c->dstH };
        if (!fmt) luts_of(c, &d->luts);
        else if (!yuv) luts_packed(c, fmt, &d->luts);
    }
    *src_layout = layout; *dst_format = fmt; *range = r; *dst_depth = bits;
    return 0;
}

/* ---- packed 4:2:2 destinations: yuyv422, uyvy422, yvyu422 ----------------------------------------------------------------------------------
 * what mi355_sws_create_src_layout_range_depth takes for a live context TO one of the three formats (0), -1 for every other context — the nine
 * describers above keep declining these destinations.  The generic scaler's contexts from every source of the describers above (three planes at 8 / 9 /
 * 10 bits, NV12 / NV21, rgb24 / bgr24, the four 32-bit orders, the three packed 4:2:2 orders — each under the checks of its own describer), with the
 * range the context's converters give (range_probe) and depth 8; the descriptor has the rgb24 form (vChr.n = dstH) and no tables.  A context without the
 * vertical banks is one of the four unscaled packers — 8-bit yuv422p (whatever the flags) or yuv420p (the reference takes it under SWS_POINT /
 * SWS_FAST_BILINEAR only, swscale_unscaled.c:1123-1139) to yuyv422 / uyvy422 at equal size: unscaled_special = 1, no banks; any other without them (the plain
 * copy) is declined.  Declined too: SWS_FAST_BILINEAR scaled contexts, SWS_FULL_CHR_H_INT, a chroma line drop, a source
 * with alpha */
int mi355_sws_describe_yuy2dst(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, int *dst_format, int *range, int *dst_depth)
{
    const int fmt = yuy2_dst_of(c);
    int r = MI355_SWS_RANGE_NONE, layout = MI355_SWS_SRC_PLANAR;
    if (!fmt || (isALPHA(c->srcFormat) && !rgb32_layout_of(c))) return -1;
    if (!c->vLumFilter) {
        if ((c->srcFormat != AV_PIX_FMT_YUV422P && c->srcFormat != AV_PIX_FMT_YUV420P) || fmt == MI355_SWS_DST_YVYU422 || !c->swscale || c->srcW != c->dstW ||
            c->srcH != c->dstH || c->hLumFilter || c->hChrFilter || c->vChrFilter || c->lumConvertRange || c->chrConvertRange) return -1;
        if (source_of(c, s) != 0) return -1;
        memset(d, 0, sizeof(*d));
        d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
        d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
        d->unscaled_special = 1;
        *src_layout = layout; *dst_format = fmt; *range = r; *dst_depth = 8;
        return 0;
    }
    r = range_probe(c);
    if (r < 0) return -1;
    if (rgb32_layout_of(c) || yuy2_layout_of(c)) {
        /* the checks of mi355_sws_describe_rgb32 / mi355_sws_describe_yuy2 on the source side: no alpha is carried to these destinations */
        layout = rgb32_layout_of(c) ? rgb32_layout_of(c) : yuy2_layout_of(c);
        if (!c->vChrFilter || !c->hLumFilter || !c->hChrFilter) return -1;
        if (c->hyscale_fast || c->hcscale_fast || c->vChrDrop || (c->flags & SWS_FULL_CHR_H_INT)) return -1;
        if (c->chrSrcVSubSample != 0 || (c->chrSrcHSubSample & ~1) || c->srcBpc != 8 || c->readLumPlanar || c->readChrPlanar || c->readAlpPlanar || c->alpPixBuf) return -1;
        if (rgb32_layout_of(c) ? rgb32_probe(c, layout, 0) != 0 : (c->chrSrcHSubSample != 1 || yuy2_probe(c, layout) != 0)) return -1;
        memset(s, 0, sizeof(*s));
        s->depth = 8; s->hsub = c->chrSrcHSubSample; s->vsub = 0;
        memcpy(s->dither, ff_dither_8x8_128, sizeof(s->dither));
        memset(d, 0, sizeof(*d));
        d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
        d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
        d->hLum = (mi355_sws_filter){ c->hLumFilter, c->hLumFilterPos, c->hLumFilterSize, c->dstW };
        d->hChr = (mi355_sws_filter){ c->hChrFilter, c->hChrFilterPos, c->hChrFilterSize, c->chrDstW };
        d->vLum = (mi355_sws_filter){ c->vLumFilter, c->vLumFilterPos, c->vLumFilterSize, c->dstH };
        d->vChr = (mi355_sws_filter){ c->vChrFilter, c->vChrFilterPos, c->vChrFilterSize, c->dstH };
        *src_layout = layout; *dst_format = fmt; *range = r; *dst_depth = 8;
        return 0;
    }
    if (describe_fmt_r(c, d, s, src_layout, dst_format, MI355_ASK_YUY2DST) != 0 || *dst_format != fmt || d->unscaled_special) return -1;
    d->vChr.n = c->dstH;
    *range = r; *dst_depth = 8;
    return 0;
}

/* ---- P010 sources: p010le -----------------------------------------------------------------------------------------------------------------
 * the input converters the context HOLDS are word >> 6 of a little-endian word, U from the first and V from the second word of a pair (the functions are
 * static in the reference: one pair of distinct words through each, as yuy2_probe does; the big-endian forms give other values) */
static int p010_probe(const SwsContext *c)
{
    static const uint8_t b[8] = { 0xC1, 0x12, 0x83, 0x34, 0x45, 0x56, 0x07, 0x78 };      /* 0x12C1 0x3483 0x5645 0x7807 */
    uint16_t y[2] = { 0 }, u[2] = { 0 }, v[2] = { 0 };
    if (!c->lumToYV12 || !c->chrToYV12 || c->alpToYV12) return -1;
    c->lumToYV12((uint8_t *)y, b, 1, NULL);
    c->chrToYV12((uint8_t *)u, (uint8_t *)v, b, b, 1, NULL);
    return y[0] == (0x12C1 >> 6) && u[0] == (0x12C1 >> 6) && v[0] == (0x3483 >> 6) ? 0 : -1;
}
/* what mi355_sws_create_src_layout_range_depth takes for a live context FROM p010le (0), -1 for every other context — the describers above keep declining
 * this source.  The reference has no unscaled converter from P010 (swscale_unscaled.c:1162-1167 keeps it off the plane copy too): a context without the
 * banks is declined.  The generic scaler's contexts: both input converters (p010LEToY_c / p010LEToUV_c, p010_probe), no other reader, srcBpc 10, no
 * alpha; to rgb24, bgr24, the four 32-bit orders and the three packed 4:2:2 orders (the descriptor's rgb24 form: vChr.n = dstH), to 8-bit planar /
 * semi-planar YUV, to 9- / 10-bit planar YUV; with the range the context's converters give (range_probe) to the 8-bit YUV destinations, the packed 4:2:2
 * ones included.  Declined: p010be, SWS_FULL_CHR_H_INT, the fast bilinear horizontal functions (the reference sets them for 8-bit sources only), a chroma
 * line drop, YUVA destinations, 15 / 16-bit RGB */
int mi355_sws_describe_p010(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, int *dst_format, int *range, int *dst_depth)
{
    int fmt, bits = 8, r;
    if (c->srcFormat != AV_PIX_FMT_P010LE || c->chrSrcHSubSample != 1 || c->chrSrcVSubSample != 1) return -1;
    if (!c->vLumFilter || !c->vChrFilter || !c->hLumFilter || !c->hChrFilter) return -1;
    if (c->hyscale_fast || c->hcscale_fast || c->vChrDrop || (c->flags & SWS_FULL_CHR_H_INT)) return -1;
    if (c->srcBpc != 10 || c->readLumPlanar || c->readChrPlanar || c->readAlpPlanar || c->alpPixBuf) return -1;
    if (p010_probe(c) != 0) return -1;
    r = range_probe(c);
    if (r < 0) return -1;
    if (deep_dst(c, &bits)) {
        if (r || c->dstBpc != bits) return -1;
        fmt = deep_dst(c, &bits);
    } else if (packed_dst_of(c) || c->dstFormat == AV_PIX_FMT_RGB24) {
        if (r) return -1;
        fmt = packed_dst_of(c);
    } else if (yuy2_dst_of(c)) {
        fmt = yuy2_dst_of(c);
    } else {
        switch (c->dstFormat) {
        case AV_PIX_FMT_YUV420P: fmt = MI355_SWS_DST_YUV420P; break;
        case AV_PIX_FMT_YUV422P: fmt = MI355_SWS_DST_YUV422P; break;
        case AV_PIX_FMT_YUV444P: fmt = MI355_SWS_DST_YUV444P; break;
        case AV_PIX_FMT_NV12:    fmt = MI355_SWS_DST_NV12; break;
        case AV_PIX_FMT_NV21:    fmt = MI355_SWS_DST_NV21; break;
        default: return -1;
        }
    }
    const int yuv = fmt >= MI355_SWS_DST_YUV420P && fmt <= MI355_SWS_DST_NV21;
    memset(s, 0, sizeof(*s));
    s->depth = 10; s->hsub = 1; s->vsub = 1;
    memcpy(s->dither, ff_dither_8x8_128, sizeof(s->dither));      /* the rows should_dither selects (swscale.c:553-556) */
    memset(d, 0, sizeof(*d));
    d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
    d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
    d->hLum = (mi355_sws_filter){ c->hLumFilter, c->hLumFilterPos, c->hLumFilterSize, c->dstW };
    d->hChr = (mi355_sws_filter){ c->hChrFilter, c->hChrFilterPos, c->hChrFilterSize, c->chrDstW };
    d->vLum = (mi355_sws_filter){ c->vLumFilter, c->vLumFilterPos, c->vLumFilterSize, c->dstH };
    d->vChr = (mi355_sws_filter){ c->vChrFilter, c->vChrFilterPos, c->vChrFilterSize, yuv ? c->chrDstH : c->dstH };
    if (!fmt) luts_of(c, &d->luts);
    else if (!yuv && !yuy2_dst_of(c)) luts_packed(c, fmt, &d->luts);
    *src_layout = MI355_SWS_SRC_P010; *dst_format = fmt; *range = r; *dst_depth = bits;
    return 0;
}

/* ---- SWS_FAST_BILINEAR contexts of the planar 8-bit sources ------------------------------------------------------------------------------------
 * the two fast functions the context HOLDS are the C ones, hyscale_fast_c / hcscale_fast_c (static in the reference: three samples through each at an
 * increment with a fraction, as range_probe does — six samples on the host, nothing on the device; the x86 build's generated code is not called:
 * canMMXEXTBeUsed is declined before).  A context whose two functions are this file's own shims (ff_sws_init_mi355x set them for a context that passed
 * this probe) is taken without calling them: no line goes to the device and no call is counted for a question */
#ifndef MI355_SWS_DESCRIBE_ONLY
static void t1_hyscale_fast(SwsContext *c, int16_t *dst, int dstWidth, const uint8_t *src, int srcW, int xInc);
static void t1_hcscale_fast(SwsContext *c, int16_t *dst1, int16_t *dst2, int dstWidth, const uint8_t *src1, const uint8_t *src2, int srcW, int xInc);
#endif
static int fast_probe(const SwsContext *c)
{
    static const uint8_t b[4] = { 10, 200, 77, 0 };
    int16_t y[3] = { 0 }, u[3] = { 0 }, v[3] = { 0 };
    if (!c->hyscale_fast || !c->hcscale_fast || c->canMMXEXTBeUsed) return -1;
#ifndef MI355_SWS_DESCRIBE_ONLY
    if (c->hyscale_fast == t1_hyscale_fast && c->hcscale_fast == t1_hcscale_fast) return 0;
#endif
    /* (the reference's prototypes take a writable context; the two C functions do not look at it) */
    c->hyscale_fast((SwsContext *)c, y, 3, b, 3, 40000);       /* xx, a: 0, 0 / 0, 78 / 1, 28 */
    c->hcscale_fast((SwsContext *)c, u, v, 3, b, b, 3, 40000);
    return y[0] == 1280 && y[1] == 16100 && y[2] == 22156 && u[0] == 1270 && u[1] == 16090 && u[2] == 21956 && v[0] == 1270 && v[1] == 16090 && v[2] == 21956 ? 0 : -1;
}
/* what mi355_sws_create_fast_bilinear takes for a live context (0), -1 for every other context — the eleven describers above keep declining these.  A
 * context is taken exactly when both fast functions are the C ones (fast_probe) AND one of those describers would take it without the two functions
 * (describing_fast: asked of generic_dst_r, the one place their chain looks at the two fields; the context is read only) — as a source of layout 0
 * and 8 bits in the generic scaler.  The descriptor is that describer's (the horizontal banks the reference built all the same travel with it; the
 * device does not read them); lumXInc / chrXInc are the context's fields as its init left them.  Declined: every source but 8-bit yuv420p / yuv422p /
 * yuv444p (the reference runs the fast pass of the others on its conversion buffer, whose sample behind the width is uninitialised),
 * SWS_FULL_CHR_H_INT, YUVA, a chroma line drop, the x86 build's MMXEXT scaler */
int mi355_sws_describe_fast(const struct SwsContext *cc, mi355_sws_desc *d, mi355_sws_src *s, int *dst_format, int *range, int *dst_depth, int *lumXInc, int *chrXInc)
{
    struct SwsContext *c = (struct SwsContext *)cc;          /* (the describers' parameter type; none of them writes to a context) */
    int layout = -1, rc;
    if (fast_probe(cc) != 0 || cc->lumXInc <= 0 || cc->chrXInc <= 0) return -1;
    *range = MI355_SWS_RANGE_NONE; *dst_depth = 8;
    describing_fast = 1;
    if (yuy2_dst_of(c)) rc = mi355_sws_describe_yuy2dst(c, d, s, &layout, dst_format, range, dst_depth);
    else if (packed_dst_of(c)) rc = mi355_sws_describe_packed(c, d, s, &layout, dst_format);
    else rc = mi355_sws_describe_depth(c, d, s, &layout, dst_format, range, dst_depth);
    describing_fast = 0;
    if (rc != 0 || layout != MI355_SWS_SRC_PLANAR || s->depth != 8 || d->unscaled_special) return -1;
    *lumXInc = cc->lumXInc; *chrXInc = cc->chrXInc;
    return 0;
}

/* ---- planar RGB destinations: gbrp -------------------------------------------------------------------------------------------------------------
 * the output function the context HOLDS is the C one, yuv2gbrp_full_X_c (static in the reference: two pixels through it — one inside the range, one that
 * clips — with one tap a bank, as range_probe does; nothing runs on the device).  A context whose function is this file's own shim (ff_sws_init_mi355x
 * set it for a context that passed this probe) is taken without calling it */
#ifndef MI355_SWS_DESCRIBE_ONLY
static void t1_gbrpX(SwsContext *c, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize, const int16_t *chrFilter, const int16_t **chrUSrc,
                     const int16_t **chrVSrc, int chrFilterSize, const int16_t **alpSrc, uint8_t **dest, int dstW, int y);
#endif
static void coefs_of(const SwsContext *c, mi355_sws_rgb_coefs *k)
{
    k->y_offset = c->yuv2rgb_y_offset; k->y_coeff = c->yuv2rgb_y_coeff;
    k->v2r = c->yuv2rgb_v2r_coeff; k->v2g = c->yuv2rgb_v2g_coeff; k->u2g = c->yuv2rgb_u2g_coeff; k->u2b = c->yuv2rgb_u2b_coeff;
}
/* one byte of the formula above mi355_sws_create_gbrp (include/mi355_sws.h): a sum modulo 2^32, clipped on its bits 30 / 31 */
static uint8_t gbrp_byte(uint32_t v) { return (uint8_t)(((v & 0xC0000000u) ? ((v >> 31) ? 0u : 0x3FFFFFFFu) : v) >> 22); }
static int gbrp_probe(const SwsContext *c)
{
    static const int16_t f[1] = { 4096 }, l[2] = { 100 << 7, 255 << 7 }, u[2] = { 90 << 7, 255 << 7 }, v[2] = { 200 << 7, 10 << 7 };
    const int16_t *lp[1] = { l }, *up[1] = { u }, *vp[1] = { v };
    uint8_t g[2] = { 0 }, b[2] = { 0 }, r[2] = { 0 }, *dest[4] = { g, b, r, NULL };
    mi355_sws_rgb_coefs k;
    if (!c->yuv2anyX) return -1;
#ifndef MI355_SWS_DESCRIBE_ONLY
    if (c->yuv2anyX == t1_gbrpX) return 0;
#endif
    coefs_of(c, &k);
    /* (the reference's prototype takes a writable context; the C function reads dstFormat and the six coefficients) */
    c->yuv2anyX((SwsContext *)c, f, lp, 1, f, up, vp, 1, NULL, dest, 2, 0);
    for (int i = 0; i < 2; i++) {
        const int Y = ((1 << 9) + l[i] * 4096) >> 10, U = ((1 << 9) - (128 << 19) + u[i] * 4096) >> 10, V = ((1 << 9) - (128 << 19) + v[i] * 4096) >> 10;
        const uint32_t y = (uint32_t)(Y - k.y_offset) * (uint32_t)k.y_coeff + (1u << 21);
        if (r[i] != gbrp_byte(y + (uint32_t)V * (uint32_t)k.v2r) || g[i] != gbrp_byte(y + (uint32_t)V * (uint32_t)k.v2g + (uint32_t)U * (uint32_t)k.u2g) ||
            b[i] != gbrp_byte(y + (uint32_t)U * (uint32_t)k.u2b)) return -1;
    }
    return 0;
}
/* what mi355_sws_create_gbrp takes for a live context (0), -1 for every other context — the twelve describers above keep declining this destination
 * (it is none of their formats, and the reference forces SWS_FULL_CHR_H_INT for it, utils.c:986-994).  The generic scaler's contexts to AV_PIX_FMT_GBRP
 * whose yuv2anyX is the C function (gbrp_probe): chrDstW = dstW, chrDstH = dstH, no range converter, no alpha; from every source of the describers
 * above, each under the source-side checks of its own describer (three planes at 8 / 9 / 10 bits; NV12 / NV21; rgb24 / bgr24; the four 32-bit orders,
 * whose alpha is not carried: gbrp has none; the three packed 4:2:2 orders; p010le).  *coefs: c->yuv2rgb_* as they are NOW (sws_setColorspaceDetails
 * rewrites them after init).  Declined: a context without the banks (rgbToPlanarRgbWrapper from an 8-bit packed RGB source at equal size,
 * swscale_unscaled.c:1090-1092), gbrap and the deeper gbrp formats, planar RGB sources, SWS_FAST_BILINEAR, a chroma line drop */
int mi355_sws_describe_gbrp(struct SwsContext *c, mi355_sws_desc *d, mi355_sws_src *s, int *src_layout, mi355_sws_rgb_coefs *coefs)
{
    int layout = MI355_SWS_SRC_PLANAR;
    if (c->dstFormat != AV_PIX_FMT_GBRP || c->dstBpc != 8 || !c->vLumFilter || !c->vChrFilter || !c->hLumFilter || !c->hChrFilter) return -1;
    if (c->hyscale_fast || c->hcscale_fast || c->vChrDrop || c->lumConvertRange || c->chrConvertRange || c->alpPixBuf) return -1;
    if (c->chrDstHSubSample || c->chrDstVSubSample || c->chrDstW != c->dstW || c->chrDstH != c->dstH) return -1;
    if (c->readLumPlanar || c->readChrPlanar || c->readAlpPlanar || c->alpToYV12) return -1;
    if (rgb32_layout_of(c) || yuy2_layout_of(c)) {
        /* the checks of mi355_sws_describe_rgb32 / mi355_sws_describe_yuy2 on the source side */
        layout = rgb32_layout_of(c) ? rgb32_layout_of(c) : yuy2_layout_of(c);
        if (c->chrSrcVSubSample != 0 || (c->chrSrcHSubSample & ~1) || c->srcBpc != 8) return -1;
        if (rgb32_layout_of(c) ? rgb32_probe(c, layout, 0) != 0 : (c->chrSrcHSubSample != 1 || yuy2_probe(c, layout) != 0)) return -1;
        memset(s, 0, sizeof(*s));
        s->depth = 8; s->hsub = c->chrSrcHSubSample; s->vsub = 0;
    } else if (c->srcFormat == AV_PIX_FMT_P010LE) {
        /* ... of mi355_sws_describe_p010 */
        layout = MI355_SWS_SRC_P010;
        if (c->chrSrcHSubSample != 1 || c->chrSrcVSubSample != 1 || c->srcBpc != 10 || p010_probe(c) != 0) return -1;
        memset(s, 0, sizeof(*s));
        s->depth = 10; s->hsub = 1; s->vsub = 1;
    } else if (c->srcFormat == AV_PIX_FMT_RGB24 || c->srcFormat == AV_PIX_FMT_BGR24) {
        /* ... of fmt_format_r: both input converters, the chroma one by the context's chrSrcHSubSample */
        layout = c->srcFormat == AV_PIX_FMT_RGB24 ? MI355_SWS_SRC_RGB24 : MI355_SWS_SRC_BGR24;
        if (c->chrSrcVSubSample != 0 || (c->chrSrcHSubSample & ~1) || c->srcBpc != 8 || !c->lumToYV12 || !c->chrToYV12) return -1;
        memset(s, 0, sizeof(*s));
        s->depth = 8; s->hsub = c->chrSrcHSubSample; s->vsub = 0;
    } else if (c->srcFormat == AV_PIX_FMT_NV12 || c->srcFormat == AV_PIX_FMT_NV21) {
        /* ... of fmt_format_r: the chroma converter alone */
        layout = c->srcFormat == AV_PIX_FMT_NV12 ? MI355_SWS_SRC_NV12 : MI355_SWS_SRC_NV21;
        if (c->chrSrcHSubSample != 1 || c->chrSrcVSubSample != 1 || c->srcBpc != 8 || c->lumToYV12 || !c->chrToYV12) return -1;
        memset(s, 0, sizeof(*s));
        s->depth = 8; s->hsub = 1; s->vsub = 1;
    } else {
        /* ... of src_format_r: three planes, no input converter */
        if (source_of(c, s) != 0 || c->lumToYV12 || c->chrToYV12) return -1;
    }
    if (gbrp_probe(c) != 0) return -1;
    memcpy(s->dither, ff_dither_8x8_128, sizeof(s->dither));      /* (part of the source record; this destination does not dither) */
    memset(d, 0, sizeof(*d));
    d->srcW = c->srcW; d->srcH = c->srcH; d->dstW = c->dstW; d->dstH = c->dstH;
    d->chrSrcW = c->chrSrcW; d->chrSrcH = c->chrSrcH; d->chrDstW = c->chrDstW;
    d->hLum = (mi355_sws_filter){ c->hLumFilter, c->hLumFilterPos, c->hLumFilterSize, c->dstW };
    d->hChr = (mi355_sws_filter){ c->hChrFilter, c->hChrFilterPos, c->hChrFilterSize, c->chrDstW };
    d->vLum = (mi355_sws_filter){ c->vLumFilter, c->vLumFilterPos, c->vLumFilterSize, c->dstH };
    d->vChr = (mi355_sws_filter){ c->vChrFilter, c->vChrFilterPos, c->vChrFilterSize, c->dstH };
    *src_layout = layout;
    coefs_of(c, coefs);
    return 0;
}

#ifndef MI355_SWS_DESCRIBE_ONLY
static void t1_hscale16(SwsContext *c, int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter, const int32_t *filterPos, int filterSize)
{
    n_calls++;
    mi355_sws_hscale16to15(dst, dstW, src, filter, filterPos, filterSize, c->srcBpc);
}
static void t1_hscale(SwsContext *c, int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter, const int32_t *filterPos, int filterSize)
{
    (void)c; n_calls++;
    mi355_sws_hscale8to15(dst, dstW, src, filter, filterPos, filterSize);
}
static void t1_packedX(SwsContext *c, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize, const int16_t *chrFilter,
                       const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize, const int16_t **alpSrc, uint8_t *dest, int dstW, int y)
{
    mi355_sws_luts t;
    (void)alpSrc; (void)y; n_calls++;
    luts_of(c, &t);
    mi355_sws_yuv2rgb24_X(&t, lumFilter, lumSrc, lumFilterSize, chrFilter, chrUSrc, chrVSrc, chrFilterSize, dest, dstW);
}
static void t1_packed2(SwsContext *c, const int16_t *lumSrc[2], const int16_t *chrUSrc[2], const int16_t *chrVSrc[2], const int16_t *alpSrc[2],
                       uint8_t *dest, int dstW, int yalpha, int uvalpha, int y)
{
    mi355_sws_luts t;
    (void)alpSrc; (void)y; n_calls++;
    luts_of(c, &t);
    mi355_sws_yuv2rgb24_2(&t, lumSrc, chrUSrc, chrVSrc, dest, dstW, yalpha, uvalpha);
}
static void t1_packed1(SwsContext *c, const int16_t *lumSrc, const int16_t *chrUSrc[2], const int16_t *chrVSrc[2], const int16_t *alpSrc,
                       uint8_t *dest, int dstW, int uvalpha, int y)
{
    mi355_sws_luts t;
    (void)alpSrc; (void)y; n_calls++;
    luts_of(c, &t);
    mi355_sws_yuv2rgb24_1(&t, lumSrc, chrUSrc, chrVSrc, dest, dstW, uvalpha);
}

/* yuv2packedX / 2 / 1 of a bgr24 or 32-bit context (yuv2bgr24_X_c ..., yuv2rgbx32_X_c ... and their _2 / _1 forms): the format and the tables are read
 * from the context at every call, as the rgb24 shims read theirs */
static void t1_pkX(SwsContext *c, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize, const int16_t *chrFilter,
                   const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize, const int16_t **alpSrc, uint8_t *dest, int dstW, int y)
{
    mi355_sws_luts t;
    const int fmt = packed_dst_of(c);
    (void)alpSrc; (void)y; n_calls++;
    luts_packed(c, fmt, &t);
    mi355_sws_yuv2packed_X(&t, fmt, lumFilter, lumSrc, lumFilterSize, chrFilter, chrUSrc, chrVSrc, chrFilterSize, dest, dstW);
}
static void t1_pk2(SwsContext *c, const int16_t *lumSrc[2], const int16_t *chrUSrc[2], const int16_t *chrVSrc[2], const int16_t *alpSrc[2],
                   uint8_t *dest, int dstW, int yalpha, int uvalpha, int y)
{
    mi355_sws_luts t;
    const int fmt = packed_dst_of(c);
    (void)alpSrc; (void)y; n_calls++;
    luts_packed(c, fmt, &t);
    mi355_sws_yuv2packed_2(&t, fmt, lumSrc, chrUSrc, chrVSrc, dest, dstW, yalpha, uvalpha);
}
static void t1_pk1(SwsContext *c, const int16_t *lumSrc, const int16_t *chrUSrc[2], const int16_t *chrVSrc[2], const int16_t *alpSrc,
                   uint8_t *dest, int dstW, int uvalpha, int y)
{
    mi355_sws_luts t;
    const int fmt = packed_dst_of(c);
    (void)alpSrc; (void)y; n_calls++;
    luts_packed(c, fmt, &t);
    mi355_sws_yuv2packed_1(&t, fmt, lumSrc, chrUSrc, chrVSrc, dest, dstW, uvalpha);
}

static int device_ready(void)
{
    const char *dev = getenv("MI355_DEVICE");
    return mi355_init(dev ? atoi(dev) : 0) == 0;
}

/* yuv2planeX_8_c / yuv2plane1_8_c (output.c:242-266): the planar output's inner loops */
static void t1_planeX(const int16_t *filter, int filterSize, const int16_t **src, uint8_t *dest, int dstW, const uint8_t *dither, int offset)
{
    n_calls++;
    mi355_sws_yuv2planeX_8(filter, filterSize, src, dest, dstW, dither, offset);
}
static void t1_plane1(const int16_t *src, uint8_t *dest, int dstW, const uint8_t *dither, int offset)
{
    n_calls++;
    mi355_sws_yuv2plane1_8(src, dest, dstW, dither, offset);
}

/* yuv2planeX_9LE_c / _10LE_c and yuv2plane1_9LE_c / _10LE_c (output.c:183-236): no context in their argument lists, one shim per depth; the
 * dither and the offset are ignored, as the reference ignores them */
#define T1_NBPS(bits) \
static void t1_planeX_ ## bits(const int16_t *filter, int filterSize, const int16_t **src, uint8_t *dest, int dstW, const uint8_t *dither, int offset) \
{ (void)dither; (void)offset; n_calls++; mi355_sws_yuv2planeX_nbps(filter, filterSize, src, (uint16_t *)dest, dstW, bits); } \
static void t1_plane1_ ## bits(const int16_t *src, uint8_t *dest, int dstW, const uint8_t *dither, int offset) \
{ (void)dither; (void)offset; n_calls++; mi355_sws_yuv2plane1_nbps(src, (uint16_t *)dest, dstW, bits); }
T1_NBPS(9)
T1_NBPS(10)

/* yuv2nv12cX_c (output.c:267-301): the semi-planar output's chroma loop, with the two context fields it reads */
static void t1_nv12cX(SwsContext *c, const int16_t *chrFilter, int chrFilterSize, const int16_t **chrUSrc, const int16_t **chrVSrc, uint8_t *dest, int chrDstW)
{
    n_calls++;
    mi355_sws_yuv2nv12cX(chrFilter, chrFilterSize, chrUSrc, chrVSrc, dest, chrDstW, c->chrDither8, c->dstFormat == AV_PIX_FMT_NV21);
}

/* the input converters of a packed rgb24 / bgr24 source (c->lumToYV12 / c->chrToYV12): their argument lists carry no context, so one shim per
 * byte order and chroma converter */
static void t1_rgb24ToY(uint8_t *dst, const uint8_t *src, int width, uint32_t *pal) { (void)pal; n_calls++; mi355_sws_rgb24ToY(dst, src, width, 0); }
static void t1_bgr24ToY(uint8_t *dst, const uint8_t *src, int width, uint32_t *pal) { (void)pal; n_calls++; mi355_sws_rgb24ToY(dst, src, width, 1); }
#define T1_TOUV(name, bgr, half) \
static void name(uint8_t *dstU, uint8_t *dstV, const uint8_t *src1, const uint8_t *src2, int width, uint32_t *pal) \
{ (void)src2; (void)pal; n_calls++; mi355_sws_rgb24ToUV(dstU, dstV, src1, width, bgr, half); }
T1_TOUV(t1_rgb24ToUV, 0, 0)
T1_TOUV(t1_rgb24ToUV_half, 0, 1)
T1_TOUV(t1_bgr24ToUV, 1, 0)
T1_TOUV(t1_bgr24ToUV_half, 1, 1)
static void rgb_converters(SwsContext *c, int layout)
{
    const int bgr = layout == MI355_SWS_SRC_BGR24;
    if (layout != MI355_SWS_SRC_RGB24 && !bgr) return;
    c->lumToYV12 = bgr ? t1_bgr24ToY : t1_rgb24ToY;
    c->chrToYV12 = c->chrSrcHSubSample ? (bgr ? t1_bgr24ToUV_half : t1_rgb24ToUV_half) : (bgr ? t1_bgr24ToUV : t1_rgb24ToUV);
}

/* ... of a 32-bit source (rgb32ToY_c ... bgr321ToUV_half_c, rgbaToA_c / abgrToA_c): one shim per byte order and converter */
#define T1_RGB32(order, layout) \
static void t1_ ## order ## ToY(uint8_t *dst, const uint8_t *src, int width, uint32_t *pal) { (void)pal; n_calls++; mi355_sws_rgb32ToY(dst, src, width, layout); } \
static void t1_ ## order ## ToA(uint8_t *dst, const uint8_t *src, int width, uint32_t *pal) { (void)pal; n_calls++; mi355_sws_rgb32ToA(dst, src, width, layout); } \
static void t1_ ## order ## ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src1, const uint8_t *src2, int width, uint32_t *pal) \
{ (void)src2; (void)pal; n_calls++; mi355_sws_rgb32ToUV(dstU, dstV, src1, width, layout, 0); } \
static void t1_ ## order ## ToUV_half(uint8_t *dstU, uint8_t *dstV, const uint8_t *src1, const uint8_t *src2, int width, uint32_t *pal) \
{ (void)src2; (void)pal; n_calls++; mi355_sws_rgb32ToUV(dstU, dstV, src1, width, layout, 1); }
T1_RGB32(rgba, MI355_SWS_SRC_RGBA)
T1_RGB32(bgra, MI355_SWS_SRC_BGRA)
T1_RGB32(argb, MI355_SWS_SRC_ARGB)
T1_RGB32(abgr, MI355_SWS_SRC_ABGR)
static void rgb32_converters(SwsContext *c, int layout, int alpha)
{
#define T1_SET(order) do { c->lumToYV12 = t1_ ## order ## ToY; c->chrToYV12 = c->chrSrcHSubSample ? t1_ ## order ## ToUV_half : t1_ ## order ## ToUV; \
                           if (alpha) c->alpToYV12 = t1_ ## order ## ToA; } while (0)
    if (layout == MI355_SWS_SRC_RGBA) T1_SET(rgba);
    else if (layout == MI355_SWS_SRC_BGRA) T1_SET(bgra);
    else if (layout == MI355_SWS_SRC_ARGB) T1_SET(argb);
    else if (layout == MI355_SWS_SRC_ABGR) T1_SET(abgr);
#undef T1_SET
}
/* yuv2packedX / 2 / 1 of a 32-bit context that carries alpha (the hasAlpha forms: yuv2rgba32_X_c ...) */
static void t1_pkX_a(SwsContext *c, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize, const int16_t *chrFilter,
                     const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize, const int16_t **alpSrc, uint8_t *dest, int dstW, int y)
{
    mi355_sws_luts t;
    const int fmt = packed_dst_of(c);
    (void)y; n_calls++;
    luts_packed(c, fmt, &t);
    mi355_sws_yuv2packed_X_a(&t, fmt, lumFilter, lumSrc, lumFilterSize, chrFilter, chrUSrc, chrVSrc, chrFilterSize, alpSrc, dest, dstW);
}
static void t1_pk2_a(SwsContext *c, const int16_t *lumSrc[2], const int16_t *chrUSrc[2], const int16_t *chrVSrc[2], const int16_t *alpSrc[2],
                     uint8_t *dest, int dstW, int yalpha, int uvalpha, int y)
{
    mi355_sws_luts t;
    const int fmt = packed_dst_of(c);
    (void)y; n_calls++;
    luts_packed(c, fmt, &t);
    mi355_sws_yuv2packed_2_a(&t, fmt, lumSrc, chrUSrc, chrVSrc, alpSrc, dest, dstW, yalpha, uvalpha);
}
static void t1_pk1_a(SwsContext *c, const int16_t *lumSrc, const int16_t *chrUSrc[2], const int16_t *chrVSrc[2], const int16_t *alpSrc,
                     uint8_t *dest, int dstW, int uvalpha, int y)
{
    mi355_sws_luts t;
    const int fmt = packed_dst_of(c);
    (void)y; n_calls++;
    luts_packed(c, fmt, &t);
    mi355_sws_yuv2packed_1_a(&t, fmt, lumSrc, chrUSrc, chrVSrc, alpSrc, dest, dstW, uvalpha);
}

/* lumConvertRange / chrConvertRange: no context in their argument lists either, one shim per direction */
static void t1_lumFromJpeg(int16_t *dst, int width) { n_calls++; mi355_sws_lumConvertRange(dst, width, 0); }
static void t1_lumToJpeg(int16_t *dst, int width) { n_calls++; mi355_sws_lumConvertRange(dst, width, 1); }
static void t1_chrFromJpeg(int16_t *dstU, int16_t *dstV, int width) { n_calls++; mi355_sws_chrConvertRange(dstU, dstV, width, 0); }
static void t1_chrToJpeg(int16_t *dstU, int16_t *dstV, int width) { n_calls++; mi355_sws_chrConvertRange(dstU, dstV, width, 1); }

/* the inner loops of a context from a 32-bit source (mi355_sws_describe_rgb32 takes it): the three input converters, the horizontal loops and
 * the output loops of its destination */
static int init_rgb32(SwsContext *c)
{
    mi355_sws_desc d;
    mi355_sws_src s;
    int layout, fmt, range, depth, alpha;
    if (!rgb32_layout_of(c)) return 0;
    if (mi355_sws_describe_rgb32(c, &d, &s, &layout, &fmt, &range, &depth, &alpha) != 0 || !device_ready() || !c->hyScale || !c->hcScale) return 1;
    const int yuv = fmt >= MI355_SWS_DST_YUV420P && fmt <= MI355_SWS_DST_NV21;
    if (yuv ? (!c->yuv2planeX || !c->yuv2plane1) : (!c->yuv2packedX || !c->yuv2packed2 || !c->yuv2packed1)) return 1;
    rgb32_converters(c, layout, alpha);
    c->hyScale = c->hcScale = t1_hscale;
    if (range > 0) {
        c->lumConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_lumToJpeg : t1_lumFromJpeg;
        c->chrConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_chrToJpeg : t1_chrFromJpeg;
    }
    if (yuv) {
        c->yuv2planeX = depth == 9 ? t1_planeX_9 : (depth == 10 ? t1_planeX_10 : t1_planeX);
        c->yuv2plane1 = depth == 9 ? t1_plane1_9 : (depth == 10 ? t1_plane1_10 : t1_plane1);
        if (c->yuv2nv12cX) c->yuv2nv12cX = t1_nv12cX;
    } else if (!fmt) {
        c->yuv2packedX = t1_packedX; c->yuv2packed2 = t1_packed2; c->yuv2packed1 = t1_packed1;
    } else {
        c->yuv2packedX = alpha ? t1_pkX_a : t1_pkX; c->yuv2packed2 = alpha ? t1_pk2_a : t1_pk2; c->yuv2packed1 = alpha ? t1_pk1_a : t1_pk1;
    }
    return 1;
}

/* ... of a packed 4:2:2 source (yuy2ToY_c / uyvyToY_c, yuy2ToUV_c / yvy2ToUV_c / uyvyToUV_c): one shim per byte order and converter */
#define T1_YUY2(order, layout) \
static void t1_ ## order ## ToY(uint8_t *dst, const uint8_t *src, int width, uint32_t *pal) { (void)pal; n_calls++; mi355_sws_yuy2ToY(dst, src, width, layout); } \
static void t1_ ## order ## ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src1, const uint8_t *src2, int width, uint32_t *pal) \
{ (void)src2; (void)pal; n_calls++; mi355_sws_yuy2ToUV(dstU, dstV, src1, width, layout); }
T1_YUY2(yuyv, MI355_SWS_SRC_YUYV422)
T1_YUY2(uyvy, MI355_SWS_SRC_UYVY422)
T1_YUY2(yvyu, MI355_SWS_SRC_YVYU422)
/* the inner loops of a context of the generic scaler from a packed 4:2:2 source (mi355_sws_describe_yuy2 takes it): the two input converters, the
 * horizontal loops and the output loops of its destination.  The four unscaled converters have no inner loops: they stay the reference's here */
static int init_yuy2(SwsContext *c)
{
    mi355_sws_desc d;
    mi355_sws_src s;
    int layout, fmt, range, depth;
    if (!yuy2_layout_of(c)) return 0;
    /* (returning 1 for a context this describer declines is deliberate: ff_sws_init_mi355x ends there, no older describer takes these sources) */
    if (mi355_sws_describe_yuy2(c, &d, &s, &layout, &fmt, &range, &depth) != 0 || d.unscaled_special || !device_ready() || !c->hyScale || !c->hcScale) return 1;
    const int yuv = fmt >= MI355_SWS_DST_YUV420P && fmt <= MI355_SWS_DST_NV21;
    if (yuv ? (!c->yuv2planeX || !c->yuv2plane1) : (!c->yuv2packedX || !c->yuv2packed2 || !c->yuv2packed1)) return 1;
    if (layout == MI355_SWS_SRC_YUYV422) { c->lumToYV12 = t1_yuyvToY; c->chrToYV12 = t1_yuyvToUV; }
    else if (layout == MI355_SWS_SRC_UYVY422) { c->lumToYV12 = t1_uyvyToY; c->chrToYV12 = t1_uyvyToUV; }
    else { c->lumToYV12 = t1_yvyuToY; c->chrToYV12 = t1_yvyuToUV; }
    c->hyScale = c->hcScale = t1_hscale;
    if (range > 0) {
        c->lumConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_lumToJpeg : t1_lumFromJpeg;
        c->chrConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_chrToJpeg : t1_chrFromJpeg;
    }
    if (yuv) {
        c->yuv2planeX = depth == 9 ? t1_planeX_9 : (depth == 10 ? t1_planeX_10 : t1_planeX);
        c->yuv2plane1 = depth == 9 ? t1_plane1_9 : (depth == 10 ? t1_plane1_10 : t1_plane1);
        if (c->yuv2nv12cX) c->yuv2nv12cX = t1_nv12cX;
    } else if (!fmt) {
        c->yuv2packedX = t1_packedX; c->yuv2packed2 = t1_packed2; c->yuv2packed1 = t1_packed1;
    } else {
        c->yuv2packedX = t1_pkX; c->yuv2packed2 = t1_pk2; c->yuv2packed1 = t1_pk1;
    }
    return 1;
}

/* yuv2packedX / 2 / 1 of a packed 4:2:2 context (yuv2yuyv422_X_c ... yuv2uyvy422_1_c): the format is read from the context at every call; no tables */
static void t1_y2X(SwsContext *c, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize, const int16_t *chrFilter,
                   const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize, const int16_t **alpSrc, uint8_t *dest, int dstW, int y)
{
    (void)alpSrc; (void)y; n_calls++;
    mi355_sws_yuv2packed_X(NULL, yuy2_dst_of(c), lumFilter, lumSrc, lumFilterSize, chrFilter, chrUSrc, chrVSrc, chrFilterSize, dest, dstW);
}
static void t1_y22(SwsContext *c, const int16_t *lumSrc[2], const int16_t *chrUSrc[2], const int16_t *chrVSrc[2], const int16_t *alpSrc[2],
                   uint8_t *dest, int dstW, int yalpha, int uvalpha, int y)
{
    (void)alpSrc; (void)y; n_calls++;
    mi355_sws_yuv2packed_2(NULL, yuy2_dst_of(c), lumSrc, chrUSrc, chrVSrc, dest, dstW, yalpha, uvalpha);
}
static void t1_y21(SwsContext *c, const int16_t *lumSrc, const int16_t *chrUSrc[2], const int16_t *chrVSrc[2], const int16_t *alpSrc,
                   uint8_t *dest, int dstW, int uvalpha, int y)
{
    (void)alpSrc; (void)y; n_calls++;
    mi355_sws_yuv2packed_1(NULL, yuy2_dst_of(c), lumSrc, chrUSrc, chrVSrc, dest, dstW, uvalpha);
}
/* the inner loops of a context of the generic scaler to a packed 4:2:2 destination (mi355_sws_describe_yuy2dst takes it): the input converters of its
 * source, the horizontal loops, the range converters and the three packed loops.  The four unscaled packers have no inner loops */
static int init_yuy2dst(SwsContext *c)
{
    mi355_sws_desc d;
    mi355_sws_src s;
    int layout, fmt, range, depth;
    if (!yuy2_dst_of(c)) return 0;
    /* (returning 1 for a context this describer declines is deliberate: no other describer takes these destinations) */
    if (mi355_sws_describe_yuy2dst(c, &d, &s, &layout, &fmt, &range, &depth) != 0 || d.unscaled_special || !device_ready() || !c->hyScale || !c->hcScale) return 1;
    if (!c->yuv2packedX || !c->yuv2packed2 || !c->yuv2packed1) return 1;
    rgb_converters(c, layout);
    rgb32_converters(c, layout, 0);
    if (layout == MI355_SWS_SRC_YUYV422) { c->lumToYV12 = t1_yuyvToY; c->chrToYV12 = t1_yuyvToUV; }
    else if (layout == MI355_SWS_SRC_UYVY422) { c->lumToYV12 = t1_uyvyToY; c->chrToYV12 = t1_uyvyToUV; }
    else if (layout == MI355_SWS_SRC_YVYU422) { c->lumToYV12 = t1_yvyuToY; c->chrToYV12 = t1_yvyuToUV; }
    c->hyScale = c->hcScale = s.depth > 8 ? t1_hscale16 : t1_hscale;
    if (range > 0) {
        c->lumConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_lumToJpeg : t1_lumFromJpeg;
        c->chrConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_chrToJpeg : t1_chrFromJpeg;
    }
    c->yuv2packedX = t1_y2X; c->yuv2packed2 = t1_y22; c->yuv2packed1 = t1_y21;
    return 1;
}

/* ... of a p010le source (p010LEToY_c / p010LEToUV_c): the output lines are host-order uint16_t */
static void t1_p010ToY(uint8_t *dst, const uint8_t *src, int width, uint32_t *pal) { (void)pal; n_calls++; mi355_sws_p010ToY((uint16_t *)dst, src, width); }
static void t1_p010ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src1, const uint8_t *src2, int width, uint32_t *pal)
{ (void)src2; (void)pal; n_calls++; mi355_sws_p010ToUV((uint16_t *)dstU, (uint16_t *)dstV, src1, width); }
/* the inner loops of a context from a p010le source (mi355_sws_describe_p010 takes it): the two input converters, the 16-bit horizontal loops (srcBpc 10),
 * the range converters and the output loops of its destination */
static int init_p010(SwsContext *c)
{
    mi355_sws_desc d;
    mi355_sws_src s;
    int layout, fmt, range, depth;
    if (c->srcFormat != AV_PIX_FMT_P010LE) return 0;
    /* (returning 1 for a context this describer declines is deliberate: ff_sws_init_mi355x ends there, no other describer takes this source) */
    if (mi355_sws_describe_p010(c, &d, &s, &layout, &fmt, &range, &depth) != 0 || !device_ready() || !c->hyScale || !c->hcScale) return 1;
    const int yuv = fmt >= MI355_SWS_DST_YUV420P && fmt <= MI355_SWS_DST_NV21;
    if (yuv ? (!c->yuv2planeX || !c->yuv2plane1) : (!c->yuv2packedX || !c->yuv2packed2 || !c->yuv2packed1)) return 1;
    c->lumToYV12 = t1_p010ToY; c->chrToYV12 = t1_p010ToUV;
    c->hyScale = c->hcScale = t1_hscale16;
    if (range > 0) {
        c->lumConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_lumToJpeg : t1_lumFromJpeg;
        c->chrConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_chrToJpeg : t1_chrFromJpeg;
    }
    if (yuv) {
        c->yuv2planeX = depth == 9 ? t1_planeX_9 : (depth == 10 ? t1_planeX_10 : t1_planeX);
        c->yuv2plane1 = depth == 9 ? t1_plane1_9 : (depth == 10 ? t1_plane1_10 : t1_plane1);
        if (c->yuv2nv12cX) c->yuv2nv12cX = t1_nv12cX;
    } else if (!fmt) {
        c->yuv2packedX = t1_packedX; c->yuv2packed2 = t1_packed2; c->yuv2packed1 = t1_packed1;
    } else if (yuy2_dst_of(c)) {
        c->yuv2packedX = t1_y2X; c->yuv2packed2 = t1_y22; c->yuv2packed1 = t1_y21;
    } else {
        c->yuv2packedX = t1_pkX; c->yuv2packed2 = t1_pk2; c->yuv2packed1 = t1_pk1;
    }
    return 1;
}

/* ... of a fast-bilinear context (hyscale_fast_c / hcscale_fast_c): the two lines of a chroma pair go through one entry */
static void t1_hyscale_fast(SwsContext *c, int16_t *dst, int dstWidth, const uint8_t *src, int srcW, int xInc)
{ (void)c; n_calls++; mi355_sws_hyscale_fast(dst, dstWidth, src, srcW, xInc); }
static void t1_hcscale_fast(SwsContext *c, int16_t *dst1, int16_t *dst2, int dstWidth, const uint8_t *src1, const uint8_t *src2, int srcW, int xInc)
{ (void)c; n_calls++; mi355_sws_hcscale_fast(dst1, dst2, dstWidth, src1, src2, srcW, xInc); }

/* ... of a gbrp context (yuv2gbrp_full_X_c): the three destination lines through one entry, the coefficients the context holds at the call */
static void t1_gbrpX(SwsContext *c, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize, const int16_t *chrFilter, const int16_t **chrUSrc,
                     const int16_t **chrVSrc, int chrFilterSize, const int16_t **alpSrc, uint8_t **dest, int dstW, int y)
{
    mi355_sws_rgb_coefs k;
    (void)alpSrc; (void)y;
    coefs_of(c, &k);
    n_calls++;
    mi355_sws_yuv2gbrp_full_X(&k, lumFilter, lumSrc, lumFilterSize, chrFilter, chrUSrc, chrVSrc, chrFilterSize, dest, dstW);
}

static void init_loops(SwsContext *c);
void ff_sws_init_mi355x(SwsContext *c)
{
    if (c->dstFormat == AV_PIX_FMT_GBRP) {
        /* a gbrp context mi355_sws_describe_gbrp takes: its output function alone (the other loops stay the reference's); any other stays as it is */
        mi355_sws_desc d;
        mi355_sws_src s;
        mi355_sws_rgb_coefs k;
        int layout;
        if (mi355_sws_describe_gbrp(c, &d, &s, &layout, &k) == 0 && device_ready()) c->yuv2anyX = t1_gbrpX;
        return;
    }
    if (c->hyscale_fast || c->hcscale_fast) {
        /* a fast-bilinear context mi355_sws_describe_fast takes: the other loops as for the same context without the two fast functions (the range
         * converters, the vertical loops), then the two fast functions themselves; any other context with them stays the reference's */
        mi355_sws_desc d;
        mi355_sws_src s;
        int fmt, range, depth, li, ci;
        if (mi355_sws_describe_fast(c, &d, &s, &fmt, &range, &depth, &li, &ci) != 0 || !device_ready()) return;
        c->hyscale_fast = NULL; c->hcscale_fast = NULL;
        init_loops(c);
        c->hyscale_fast = t1_hyscale_fast; c->hcscale_fast = t1_hcscale_fast;
        return;
    }
    init_loops(c);
}
static void init_loops(SwsContext *c)
{
    mi355_sws_src s;
    int layout;
    if (init_p010(c)) return;
    if (init_yuy2dst(c)) return;
    if (init_rgb32(c)) return;
    if (init_yuy2(c)) return;
    const int range = range_probe(c);
    /* (an NV12 / NV21 source: c->chrToYV12 stays the reference's) */
    const int fmt = range > 0 ? fmt_format_r(c, &s, 0, &layout, 1) : fmt_format(c, &s, 0, &layout);
    if (fmt > 0) {
        if (!device_ready() || !c->hyScale || !c->hcScale || !c->yuv2planeX || !c->yuv2plane1) return;
        rgb_converters(c, layout);
        if (range > 0) {
            c->lumConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_lumToJpeg : t1_lumFromJpeg;
            c->chrConvertRange = range == MI355_SWS_RANGE_TO_JPEG ? t1_chrToJpeg : t1_chrFromJpeg;
        }
        c->hyScale = c->hcScale = s.depth > 8 ? t1_hscale16 : t1_hscale;
        c->yuv2planeX = t1_planeX;
        c->yuv2plane1 = t1_plane1;
        if (c->yuv2nv12cX) c->yuv2nv12cX = t1_nv12cX;
        return;
    }
    /* a 9- / 10-bit planar destination: the horizontal loops as above (the intermediates stay 15 bits), the two output loops of its depth */
    int bits = 8;
    if (fmt < 0 && !range && deep_dst(c, &bits) && fmt_format_r(c, &s, 0, &layout, MI355_ASK_DEEP) > 0 && c->dstBpc == bits) {
        if (!device_ready() || !c->hyScale || !c->hcScale || !c->yuv2planeX || !c->yuv2plane1) return;
        rgb_converters(c, layout);
        c->hyScale = c->hcScale = s.depth > 8 ? t1_hscale16 : t1_hscale;
        c->yuv2planeX = bits == 9 ? t1_planeX_9 : t1_planeX_10;
        c->yuv2plane1 = bits == 9 ? t1_plane1_9 : t1_plane1_10;
        return;
    }
    /* bgr24 / rgba / bgra / argb / abgr: the horizontal loops as above, the three packed loops of the format */
    if (fmt < 0 && !range && packed_dst_of(c) && fmt_format_r(c, &s, 0, &layout, MI355_ASK_PACKED) > 0) {
        if (!device_ready() || !c->hyScale || !c->hcScale || !c->yuv2packedX || !c->yuv2packed2 || !c->yuv2packed1) return;
        rgb_converters(c, layout);
        c->hyScale = c->hcScale = s.depth > 8 ? t1_hscale16 : t1_hscale;
        c->yuv2packedX = t1_pkX;
        c->yuv2packed2 = t1_pk2;
        c->yuv2packed1 = t1_pk1;
        return;
    }
    /* rgb24: yuv420p as before (taken(): also contexts with range conversion, which swscale() applies between the loops); the other sources
     * where src_format() takes them */
    if (!(taken(c) || fmt == 0) || c->hyscale_fast) return;
    if (!device_ready()) return;                                /* no usable MI355X: the reference's functions stay */
    /* only what the reference set to the functions these shims restate (a context whose selectors left one of them empty
     * uses another template) */
    if (!c->hyScale || !c->hcScale || !c->yuv2packedX || !c->yuv2packed2 || !c->yuv2packed1) return;
    c->hyScale = c->hcScale = s.depth > 8 ? t1_hscale16 : t1_hscale;
    if (fmt == 0) rgb_converters(c, layout);
    c->yuv2packedX = t1_packedX;
    c->yuv2packed2 = t1_packed2;
    c->yuv2packed1 = t1_packed1;
}

/* ---- whole pictures: SwsContext.swscale ------------------------------------------------------------------------------ */
#define MI355_SWS_SLOTS 256
typedef struct Bound {
    SwsContext *c;
    SwsFunc real;                 /* what the reference chose */
    int special;                  /* ... through ff_yuv2rgb_get_func_ptr */
    int planar;                   /* MI355_SWS_DST_* of a planar context (mi355_sws_scale_planar), 0 for rgb24 */
    int other;                    /* a source other than 8-bit yuv420p: described by mi355_sws_describe_fmt, built by mi355_sws_create_src_layout */
    int layout;                   /* ... its MI355_SWS_SRC_* (NV12 / NV21: two source planes) */
    int range;                    /* ... the MI355_SWS_RANGE_* its converters gave when it was bound (mi355_sws_describe_range / mi355_sws_create_src_layout_range) */
    int depth;                    /* ... the bits of its planar destination: 8, or 9 / 10 (mi355_sws_describe_depth / mi355_sws_create_src_layout_range_depth) */
    int packed;                   /* ... MI355_SWS_DST_BGR24 ... _ABGR of a packed destination beside rgb24 (mi355_sws_describe_packed), else 0; planar is 0 then */
    int rgb32;                    /* 1: a 32-bit source (mi355_sws_describe_rgb32: layout, planar / packed, range and depth above are what it gave) ...;
                                   * 2: a packed 4:2:2 source in the generic scaler (mi355_sws_describe_yuy2, the same fields; never alpha);
                                   * 3: a packed 4:2:2 DESTINATION from any source (mi355_sws_describe_yuy2dst, the same fields; packed is its format, no tables);
                                   * 4: a p010le source to any destination (mi355_sws_describe_p010, the same fields; TWO source planes; never alpha);
                                   * 5: a fast-bilinear context of a planar 8-bit source (mi355_sws_describe_fast, the same fields and the two increments below;
                                   *    built by mi355_sws_create_fast_bilinear);
                                   * 6: a gbrp destination from any source (mi355_sws_describe_gbrp: layout as it gave it, planar is MI355_SWS_DST_GBRP; built by
                                   *    mi355_sws_create_gbrp from the coefficients below) */
    int lumXInc, chrXInc;         /* ... the increments it was bound with */
    mi355_sws_rgb_coefs coefs;    /* ... the six coefficients the device context was built from (sws_setColorspaceDetails rewrites the context's: built anew then) */
    int alpha;                    /* ... whose alpha goes to the 32-bit destination (mi355_sws_create_src_layout_alpha) */
    mi355_sws_ctx *dev;
    int failed;                   /* the device side does not take this context: the reference's function from now on */
    int busy;                     /* calls of mi355_sws_scale in flight on `dev` (under bound_mu): the device context is destroyed only at 0 */
    unsigned long stamp;          /* last use (diagnostics) */
    uint8_t y_table[1024];        /* the tables the device context was built from */
    int32_t gv0;
} Bound;
static Bound bound[MI355_SWS_SLOTS];
static pthread_mutex_t bound_mu = PTHREAD_MUTEX_INITIALIZER;
static pthread_cond_t bound_idle = PTHREAD_COND_INITIALIZER;
static unsigned long n_pictures, n_stamp;
unsigned long mi355_sws_glue_pictures(void) { return n_pictures; }   /* whole pictures converted on the device so far (diagnostics) */
int mi355_sws_glue_live_contexts(void)                                /* contexts that hold a device side right now (diagnostics) */
{
    int n = 0;
    pthread_mutex_lock(&bound_mu);
    for (int i = 0; i < MI355_SWS_SLOTS; i++) n += bound[i].c && bound[i].dev;
    pthread_mutex_unlock(&bound_mu);
    return n;
}

/* under bound_mu: wait until no call runs on the slot's device context, then drop it */
static void slot_release(Bound *b)
{
    while (b->busy) pthread_cond_wait(&bound_idle, &bound_mu);
    if (b->dev) mi355_sws_destroy(b->dev);
    memset(b, 0, sizeof(*b));
}
static Bound *bound_find(SwsContext *c, int create)
{
    Bound *free_slot = NULL;
    for (int i = 0; i < MI355_SWS_SLOTS; i++) {
        if (bound[i].c == c) return &bound[i];
        if (!free_slot && !bound[i].c) free_slot = &bound[i];
    }
    if (!create) return NULL;
    /* Table full: the new context stays UNBOUND (bind() hands back the reference's function).  A slot is never taken from another context: it may be
     * alive — its SwsContext.swscale points here, and without its slot a call could neither reach the device nor the reference's function
     * (an eviction turned such a call into "0 lines, no error").  Slots come back through sws_freeContext (--wrap) or when a new context
     * is built at a freed one's address; a host linked without the wrap that leaks 256 addresses runs further contexts on the CPU, correctly. */
    if (free_slot) { memset(free_slot, 0, sizeof(*free_slot)); free_slot->c = c; }
    return free_slot;
}
/* a selector runs for this context: sws_init_context() of a new context — possibly at the address of one that was freed */
static SwsFunc bind(SwsContext *c, SwsFunc real, int special)
{
    int planar = special ? 0 : planar_format(c), other = 0, layout = MI355_SWS_SRC_PLANAR, range = MI355_SWS_RANGE_NONE, depth = 8, packed = 0;
    int rgb32 = 0, alpha = 0, lum_inc = 0, chr_inc = 0;
    if (c->dstFormat == AV_PIX_FMT_GBRP) {
        /* a gbrp destination: one describer for every source it comes from, asked before every branch below (none of them takes the format) */
        mi355_sws_desc d;
        mi355_sws_src s;
        mi355_sws_rgb_coefs k;
        if (special || mi355_sws_describe_gbrp(c, &d, &s, &layout, &k) != 0) return real;
        rgb32 = 6; other = 1; planar = MI355_SWS_DST_GBRP;
    } else
    if (!special && (c->hyscale_fast || c->hcscale_fast)) {
        /* a fast-bilinear context: asked FIRST, before every branch below, and built through its own creator.  The ten describers behind those branches
         * decline such a context anyway, but taken() — mi355_sws_describe's test — looks at the two formats alone and would hand yuv420p -> rgb24 to the
         * bank-driven kernels; a context the new describer declines stays the reference's */
        mi355_sws_desc d;
        mi355_sws_src s;
        int fmt;
        if (mi355_sws_describe_fast(c, &d, &s, &fmt, &range, &depth, &lum_inc, &chr_inc) != 0) return real;
        rgb32 = 5; other = 1; planar = 0;
        if (fmt >= MI355_SWS_DST_BGR24) packed = fmt; else planar = fmt;
    } else
    if (!special && c->srcFormat == AV_PIX_FMT_P010LE) {
        /* a p010le source: one describer for every destination it goes to, the packed 4:2:2 ones included (every such context is the generic scaler's) */
        mi355_sws_desc d;
        mi355_sws_src s;
        int fmt;
        if (mi355_sws_describe_p010(c, &d, &s, &layout, &fmt, &range, &depth) != 0) return real;
        rgb32 = 4; other = 1;
        if (fmt >= MI355_SWS_DST_BGR24) packed = fmt; else planar = fmt;
    } else
    if (!special && yuy2_dst_of(c)) {
        /* a packed 4:2:2 destination: one describer for every source it comes from.  Only the generic scaler's contexts get here (the four unscaled
         * packers are set without a selector) */
        mi355_sws_desc d;
        mi355_sws_src s;
        int fmt;
        if (mi355_sws_describe_yuy2dst(c, &d, &s, &layout, &fmt, &range, &depth) != 0 || d.unscaled_special) return real;
        rgb32 = 3; other = 1; packed = fmt;
    } else
    if (!special && rgb32_layout_of(c)) {
        /* a 32-bit source: one describer for every destination it goes to */
        mi355_sws_desc d;
        mi355_sws_src s;
        int fmt;
        if (mi355_sws_describe_rgb32(c, &d, &s, &layout, &fmt, &range, &depth, &alpha) != 0) return real;
        rgb32 = other = 1;
        if (fmt >= MI355_SWS_DST_BGR24) packed = fmt; else planar = fmt;
    } else
    if (!special && yuy2_layout_of(c)) {
        /* a packed 4:2:2 source: one describer as well.  Only the generic scaler's contexts get here (the four unscaled wrappers are set without a
         * selector: they stay the reference's, like every context the describer declines) */
        mi355_sws_desc d;
        mi355_sws_src s;
        int fmt;
        if (mi355_sws_describe_yuy2(c, &d, &s, &layout, &fmt, &range, &depth) != 0 || d.unscaled_special) return real;
        rgb32 = 2; other = 1;
        if (fmt >= MI355_SWS_DST_BGR24) packed = fmt; else planar = fmt;
    } else
    if (!(taken(c) || planar)) {
        mi355_sws_src s;
        int fmt = fmt_format(c, &s, special, &layout);
        if (fmt < 0 && !special && (range = range_probe(c)) > 0) {
            /* the generic scaler with lumConvertRange / chrConvertRange between its passes, to a YUV destination */
            fmt = fmt_format_r(c, &s, 0, &layout, 1);
            if (fmt == 0) fmt = -1;
        } else if (fmt < 0 && !special && range == MI355_SWS_RANGE_NONE && deep_dst(c, &depth)) {
            /* the generic scaler to a 9- / 10-bit planar destination, no range */
            fmt = c->dstBpc == depth ? fmt_format_r(c, &s, 0, &layout, MI355_ASK_DEEP) : -1;
            if (fmt == 0) fmt = -1;
        } else range = MI355_SWS_RANGE_NONE;
        if (fmt < 0 && range <= 0 && packed_dst_of(c)) {
            /* bgr24 or a 32-bit order: the generic scaler, or (special) yuv2rgb_c_24_bgr / yuv2rgb_c_32 */
            range = MI355_SWS_RANGE_NONE; depth = 8;
            packed = fmt_format_r(c, &s, special, &layout, MI355_ASK_PACKED);
            if (packed > 0) fmt = 0; else packed = 0;
        }
        if (fmt < 0) return real;
        other = 1; planar = fmt;
    }
    if (!real || getenv("MI355_SWS_PLAIN")) return real;
    pthread_mutex_lock(&bound_mu);
    Bound *b = bound_find(c, 1);
    if (b) {
        slot_release(b);
        b->c = c; b->real = real; b->special = special; b->planar = planar; b->other = other; b->layout = layout; b->range = range; b->depth = depth;
        b->packed = packed; b->rgb32 = rgb32; b->alpha = alpha; b->lumXInc = lum_inc; b->chrXInc = chr_inc;
        b->stamp = ++n_stamp;
    }
    pthread_mutex_unlock(&bound_mu);
    return b ? mi355_swsfunc_entry : real;
}

static int mi355_swsfunc(SwsContext *c, const uint8_t *src[], int srcStride[], int srcSliceY, int srcSliceH, uint8_t *dst[], int dstStride[])
{
    pthread_mutex_lock(&bound_mu);
    Bound *b = bound_find(c, 0);
    SwsFunc real = b ? b->real : NULL;
    mi355_sws_ctx *dev = NULL;
    /* the device path takes whole pictures with positive strides (a 2-D copy has no negative pitch; sws_scale() itself also takes bottom-up
     * pictures — vf_vflip makes them — and those go to the reference's function) */
    /* a planar context: all three destination planes; range conversion set since the context was bound (sws_setColorspaceDetails) is
     * the reference's for that picture */
    mi355_sws_src s_now;
    int l_now, d_now = 8;
    const int semi = b && (b->planar == MI355_SWS_DST_NV12 || b->planar == MI355_SWS_DST_NV21);      /* two planes: dstStride[2] is not looked at */
    /* a context bound with range conversion: the converters it holds NOW give the direction it was bound with (range_probe), else the
     * reference's function for that picture too */
    /* a 32-bit source: described again — layout, destination, range, depth and alpha must be what the context was bound with; a packed 4:2:2 source
     * likewise, through its own describer */
    mi355_sws_desc d32;
    mi355_sws_src s32;
    int l32 = 0, f32 = 0, r32 = 0, dp32 = 8, a32 = 0, li32 = 0, ci32 = 0;
    mi355_sws_rgb_coefs k32;
    memset(&k32, 0, sizeof(k32));
    if (b && b->rgb32 == 6) f32 = MI355_SWS_DST_GBRP;              /* (its describer has no format, range or depth to give: a gbrp context has one of each) */
    const int rgb32_ok = b && b->rgb32 && (b->rgb32 == 6 ? mi355_sws_describe_gbrp(c, &d32, &s32, &l32, &k32) == 0 :
                                           b->rgb32 == 5 ? mi355_sws_describe_fast(c, &d32, &s32, &f32, &r32, &dp32, &li32, &ci32) == 0 && li32 == b->lumXInc && ci32 == b->chrXInc :
                                           b->rgb32 == 4 ? mi355_sws_describe_p010(c, &d32, &s32, &l32, &f32, &r32, &dp32) == 0 :
                                           b->rgb32 == 3 ? mi355_sws_describe_yuy2dst(c, &d32, &s32, &l32, &f32, &r32, &dp32) == 0 && !d32.unscaled_special :
                                           b->rgb32 == 2 ? mi355_sws_describe_yuy2(c, &d32, &s32, &l32, &f32, &r32, &dp32) == 0 && !d32.unscaled_special
                                                         : mi355_sws_describe_rgb32(c, &d32, &s32, &l32, &f32, &r32, &dp32, &a32) == 0) && l32 == b->layout &&
                         f32 == (b->packed ? b->packed : b->planar) && r32 == b->range && dp32 == b->depth && a32 == b->alpha;
    const int planar_ok = b && b->planar && dstStride[1] > 0 && (semi || dstStride[2] > 0) && (b->rgb32 ? rgb32_ok :
                          (b->other ? fmt_format_r(c, &s_now, 0, &l_now, b->depth > 8 ? MI355_ASK_DEEP : b->range != 0) : planar_format(c)) == b->planar &&
                          (!b->range || range_probe(c) == b->range) &&
                          (b->depth <= 8 || (deep_dst(c, &d_now) == b->planar && d_now == b->depth)));  /* (with converters set since: the reference's) */
    /* an rgb24 context of another source: range conversion set since it was bound is the reference's for that picture, as above */
    const int other_ok = !b || !b->other || (b->rgb32 ? rgb32_ok : (b->planar || (b->packed ? fmt_format_r(c, &s_now, b->special, &l_now, MI355_ASK_PACKED) == b->packed
                                                                                                  : fmt_format(c, &s_now, b->special, &l_now) == 0)));
    /* an NV12 / NV21 source has two planes: srcStride[2] is not looked at; a packed rgb24 / bgr24, 32-bit or 4:2:2 source has one */
    const int one_plane = b && (b->layout == MI355_SWS_SRC_RGB24 || b->layout == MI355_SWS_SRC_BGR24 || b->rgb32 == 1 || b->rgb32 == 2 ||
                                (b->layout >= MI355_SWS_SRC_RGBA && b->layout <= MI355_SWS_SRC_ABGR) || (b->layout >= MI355_SWS_SRC_YUYV422 && b->layout <= MI355_SWS_SRC_YVYU422));
    if (b && !b->failed && srcSliceY == 0 && srcSliceH == c->srcH &&
        srcStride[0] > 0 && (one_plane || srcStride[1] > 0) && (b->layout || srcStride[2] > 0) && dstStride[0] > 0 && (!b->planar || planar_ok) && other_ok) {
        if (b->dev && !b->busy && !b->planar && !b->packed && (memcmp(b->y_table, c->yuvTable, 1024) || b->gv0 != c->table_gV[0])) { mi355_sws_destroy(b->dev); b->dev = NULL; }
        if (b->dev && !b->busy && b->packed && b->rgb32 != 3 && b->packed < MI355_SWS_DST_YUYV422) {      /* (a packed 4:2:2 destination has no tables) */
            /* the tables in the form the device context was built from (a 32-bit order's first 1024 table BYTES are 256 entries below every colour) */
            mi355_sws_luts now;
            luts_packed(c, b->packed, &now);
            if (memcmp(b->y_table, now.y_table, 1024) || b->gv0 != c->table_gV[0]) { mi355_sws_destroy(b->dev); b->dev = NULL; }
        }
        /* a gbrp context whose coefficients changed since its device side was built */
        if (b->dev && !b->busy && b->rgb32 == 6 && rgb32_ok && memcmp(&b->coefs, &k32, sizeof(k32))) { mi355_sws_destroy(b->dev); b->dev = NULL; }
        if (!b->dev) {
            mi355_sws_desc d;
            int fmt;
            if (b->rgb32) {
                if (device_ready() && rgb32_ok) {
                    b->coefs = k32;
                    b->dev = b->rgb32 == 6 ? mi355_sws_create_gbrp(&d32, &s32, l32, &k32) :
                             b->rgb32 == 5 ? mi355_sws_create_fast_bilinear(&d32, &s32, f32, r32, dp32, li32, ci32) :
                             a32 ? mi355_sws_create_src_layout_alpha(&d32, &s32, l32, f32, 1) : mi355_sws_create_src_layout_range_depth(&d32, &s32, l32, f32, r32, dp32);
                    d = d32;
                }
            } else
            if (b->packed) {
                mi355_sws_src s;
                int layout;
                if (device_ready() && mi355_sws_describe_packed(c, &d, &s, &layout, &fmt) == 0 && layout == b->layout && fmt == b->packed &&
                    d.unscaled_special == b->special)
                    b->dev = mi355_sws_create_src_layout_range_depth(&d, &s, layout, fmt, MI355_SWS_RANGE_NONE, 8);
            } else
            if (b->other) {
                mi355_sws_src s;
                int layout, range = MI355_SWS_RANGE_NONE, depth = 8;
                if (device_ready() && (b->depth > 8 ? mi355_sws_describe_depth(c, &d, &s, &layout, &fmt, &range, &depth) == 0 && layout == b->layout && depth == b->depth :
                                       b->range ? mi355_sws_describe_range(c, &d, &s, &layout, &fmt, &range) == 0 && layout == b->layout && range == b->range :
                                       b->layout ? mi355_sws_describe_fmt(c, &d, &s, &layout, &fmt) == 0 && layout == b->layout
                                                 : describe_src(c, &d, &s, &fmt, b->special) == 0) && fmt == b->planar)
                    b->dev = mi355_sws_create_src_layout_range_depth(&d, &s, b->layout, fmt, range, depth);
            } else if (b->planar) {
                if (device_ready() && mi355_sws_describe_planar(c, &d, &fmt) == 0) b->dev = mi355_sws_create_planar(&d, fmt);
            } else if (device_ready() && describe(c, &d, b->special) == 0) b->dev = mi355_sws_create(&d);
            if (b->dev && (b->rgb32 == 3 || b->packed >= MI355_SWS_DST_YUYV422)) ;
            else if (b->dev && b->packed) { memcpy(b->y_table, d.luts.y_table, 1024); b->gv0 = c->table_gV[0]; }
            else if (b->dev && !b->planar) { memcpy(b->y_table, c->yuvTable, 1024); b->gv0 = c->table_gV[0]; }
            else if (!b->dev) b->failed = 1;
        }
        dev = b->dev;
        if (dev) { b->busy++; b->stamp = ++n_stamp; }          /* the context stays until this call is back (a bind() or free for its address waits) */
    }
    pthread_mutex_unlock(&bound_mu);
    if (dev) {
        const int st[3] = { srcStride[0], srcStride[1], srcStride[2] }, dst_st[3] = { dstStride[0], dstStride[1], dstStride[2] };
        const int n = b->planar ? mi355_sws_scale_planar(dev, src, st, dst, dst_st) : mi355_sws_scale(dev, src, st, dst[0], dstStride[0]);
        pthread_mutex_lock(&bound_mu);
        b->busy--;
        pthread_cond_broadcast(&bound_idle);
        pthread_mutex_unlock(&bound_mu);
        if (n > 0) { __sync_fetch_and_add(&n_pictures, 1); return n; }
        /* a failed copy / launch / allocation: this picture by the reference's function (mi355_sws_scale leaves the context usable) */
    }
    /* real == NULL: no slot for a context whose swscale points here — only a context used after sws_freeContext gets this far (slots are never taken away) */
    return real ? real(c, src, srcStride, srcSliceY, srcSliceH, dst, dstStride) : 0;
}

/* sws_freeContext: the context's device side goes with it (--wrap=sws_freeContext; without the wrap an entry stays until its address is
 * bound again or the table recycles it) */
void __real_sws_freeContext(SwsContext *c);
void __wrap_sws_freeContext(SwsContext *c)
{
    if (c) {
        pthread_mutex_lock(&bound_mu);
        Bound *b = bound_find(c, 0);
        if (b) slot_release(b);
        pthread_mutex_unlock(&bound_mu);
    }
    __real_sws_freeContext(c);
}

SwsFunc __real_ff_getSwsFunc(SwsContext *c);
SwsFunc __wrap_ff_getSwsFunc(SwsContext *c)
{
    SwsFunc f = __real_ff_getSwsFunc(c);
    if (getenv("MI355_SWS_LINES")) { ff_sws_init_mi355x(c); return f; }
    return bind(c, f, 0);
}
SwsFunc __real_ff_yuv2rgb_get_func_ptr(SwsContext *c);
SwsFunc __wrap_ff_yuv2rgb_get_func_ptr(SwsContext *c)
{
    SwsFunc f = __real_ff_yuv2rgb_get_func_ptr(c);
    if (getenv("MI355_SWS_LINES")) return f;
    return bind(c, f, 1);
}
#endif
