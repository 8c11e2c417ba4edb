/*
 * mi355_sws.h — C ABI of the libswscale part of the hot path:
 * horizontal 8->15 bit FIR, vertical FIR to planar 8 bit or through the yuv->rgb LUTs to RGB24,
 * and the unscaled yuv420p -> rgb24 converter; whole pictures to RGB24, to planar yuv420p / yuv422p / yuv444p or to semi-planar
 * NV12 / NV21 (yuv2nv12cX, and the unscaled yuv420p -> NV12 / NV21 packer); from planar sources or from NV12 / NV21 (the reference's
 * nv12ToUV_c / nv21ToUV_c in front of hcScale, and the unscaled NV12 / NV21 -> yuv420p splitter) or from packed rgb24 / bgr24 (the
 * reference's rgb24ToY_c / rgb24ToUV_c / rgb24ToUV_half_c and their bgr24 forms in front of hyScale / hcScale); the three planar
 * destinations also at 9 or 10 bits (yuv420p9le ... yuv444p10le: yuv2planeX_10 / yuv2plane1_10); packed destinations also as bgr24 and as
 * rgba / bgra / argb / abgr (yuv2rgb_write output.c:825-867; yuv2rgb_c_24_bgr / yuv2rgb_c_32), from every source rgb24 is written from; and from
 * packed 32-bit rgba / bgra / argb / abgr sources (rgb32ToY_c ... bgr321ToUV_half_c input.c:165-291 in front of hyScale / hcScale) to all of these,
 * the source's alpha carried to a 32-bit destination where asked for (rgbaToA_c / abgrToA_c and the hasAlpha forms of the packed templates); and
 * from packed 4:2:2 yuyv422 / uyvy422 / yvyu422 sources (the byte picks yuy2ToY_c ... uyvyToUV_c input.c:369-473 in front of hyScale / hcScale) to all
 * of these, with the reference's four unscaled converters yuyv422 / uyvy422 -> yuv420p / yuv422p (yuyvToYuv420Wrapper ... uyvyToYuv422Wrapper
 * swscale_unscaled.c:227-287); and TO packed 4:2:2 yuyv422 / uyvy422 / yvyu422 (yuv2422_X / _2 / _1_c_template output.c:451-582), from every source
 * rgb24 is written from, with range conversion, and the reference's four unscaled packers yuv422p / yuv420p -> yuyv422 / uyvy422
 * (yuv422pToYuy2Wrapper, yuv422pToUyvyWrapper, planarToYuy2Wrapper, planarToUyvyWrapper swscale_unscaled.c:179-225); and from p010le sources
 * (p010LEToY_c / p010LEToUV_c input.c:499-524 in front of hScale16To15_c, depth 10) to every destination the yuv420p10le source takes; and
 * SWS_FAST_BILINEAR contexts of the planar 8-bit sources (hyscale_fast_c / hcscale_fast_c swscale.c:238-301 in place of hyScale / hcScale:
 * mi355_sws_create_fast_bilinear) to every destination those sources take; and TO planar RGB, gbrp (the arithmetic path yuv2gbrp_full_X_c
 * output.c:1275-1355 with six integer coefficients in place of the LUTs: mi355_sws_create_gbrp), from every source layout.
 *
 * The reference keeps these behind function pointers of the (private) SwsContext
 * (libswscale/swscale_internal.h:253-540): hyScale/hcScale :526-531, yuv2plane1/yuv2planeX/
 * yuv2packed1/2/X :437-443, swscale :263.  SwsContext is not a public type, so this ABI carries
 * the handful of fields those functions consume in a plain descriptor; the few lines of glue that
 * fill it from a SwsContext inside the reference tree are in INTEGRATION.md (and compiled for the
 * tests as oracle/ref_sws_glue.c).  Filter banks and LUTs stay the product of the reference's own
 * init code (initFilter utils.c:249-632, ff_yuv2rgb_c_init_tables yuv2rgb.c:671-896).
 */
#ifndef MI355_SWS_H
#define MI355_SWS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* yuv->rgb tables of the 24-bpp case (yuv2rgb.c:850-863) as offsets instead of pointers:
 *   r = y_table[rV[V] + Y], g = y_table[gU[U] + gV[V] + Y], b = y_table[bU[U] + Y]
 * with rV[v] = c->table_rV[v] - c->yuvTable, gU[u] = c->table_gU[u] - c->yuvTable,
 * gV[v] = c->table_gV[v], bU[u] = c->table_bU[u] - c->yuvTable. */
typedef struct mi355_sws_luts {
    uint8_t y_table[1024];
    int16_t rV[256], gU[256], gV[256], bU[256];
} mi355_sws_luts;

/* one filter bank as built by initFilter: n outputs, `size` taps each */
typedef struct mi355_sws_filter {
    const int16_t *coef;   /* [n * size]; horizontal: 1.0 = 1<<14, vertical: 1.0 = 1<<12 */
    const int32_t *pos;    /* [n] first input sample / line */
    int size, n;
} mi355_sws_filter;

typedef struct mi355_sws_desc {
    int srcW, srcH, dstW, dstH;
    int chrSrcW, chrSrcH, chrDstW;          /* SwsContext :267-269 (yuv420p in, rgb24 out: chrDstH = dstH) */
    int unscaled_special;                   /* c->swscale is yuv2rgb_c_24_rgb (swscale_unscaled.c:1050-1055) */
    mi355_sws_filter hLum, hChr, vLum, vChr;
    mi355_sws_luts luts;
} mi355_sws_desc;

typedef struct mi355_sws_ctx mi355_sws_ctx;   /* descriptor + filter banks resident in HBM */

/* one picture of a batch, device pointers.  A source plane whose pointer and stride are multiples of 16 is fetched in aligned 16-byte
 * pieces: every line must be readable over its whole STRIDE (src_stride[k] bytes, also the last line's — the bytes between the width
 * and the stride may hold anything; the reference's own buffers are allocated that way, libavutil/frame.c).  Planes with other
 * pointers or strides are read sample-exactly. */
typedef struct mi355_sws_frame {
    const uint8_t *src[3];
    int src_stride[3];
    uint8_t *dst;          /* packed RGB24 (or bgr24 / rgba / bgra / argb / abgr: MI355_SWS_DST_BGR24 ... below; or yuyv422 / uyvy422 / yvyu422: MI355_SWS_DST_YUYV422 ...) */
    int dst_stride;
} mi355_sws_frame;

mi355_sws_ctx *mi355_sws_create(const mi355_sws_desc *desc);
void mi355_sws_destroy(mi355_sws_ctx *ctx);

/* Tier 1: replaces c->swscale(c, src, srcStride, 0, srcH, dst, dstStride) for a whole picture
 * (SwsFunc, swscale_internal.h:62-64; generic swscale() swscale.c:343-722 or yuv2rgb_c_24_rgb
 * yuv2rgb.c:335-363 according to desc->unscaled_special).  Host pointers, synchronous.
 * Returns the number of output lines. */
int mi355_sws_scale(mi355_sws_ctx *ctx, const uint8_t *const src[3], const int src_stride[3],
                    uint8_t *dst, int dst_stride);

/* Tier 2: a batch of pictures resident in HBM, one launch; d_frames is a device array. */
int mi355_sws_scale_frames_dev(mi355_sws_ctx *ctx, const mi355_sws_frame *d_frames, int nframes, void *stream);   /* 0, -1 bad argument, -2 launch failure */

/* What mi355_sws_scale_frames_dev launches for a context (read only; the launch takes its kernel from the same helper). */
enum {
    MI355_SWS_K_C24 = 0,          /* the unscaled special converter (k_sws_c24) */
    MI355_SWS_K_IDENT1_1 = 1,     /* no scaling, one luma tap, up to two chroma taps: yuv2rgb24_1 from the source bytes */
    MI355_SWS_K_IDENT1_X = 2,     /* no scaling, one luma tap, three or four chroma taps: yuv2rgb24_X from the source bytes */
    MI355_SWS_K_GENERIC_A = 3,    /* the generic tile kernel holding 28 luma / 16 chroma source lines */
    MI355_SWS_K_GENERIC_B = 4,    /* ... 40 / 20 */
    MI355_SWS_K_GENERIC_C = 5,    /* ... 48 / 24 */
    MI355_SWS_K_PLANAR_A = 6,     /* a planar destination (mi355_sws_create_planar): the tile kernel holding 28 luma / 16 chroma source lines */
    MI355_SWS_K_PLANAR_B = 7,     /* ... 40 / 24 */
    MI355_SWS_K_PLANAR_C = 8,     /* ... 48 / 48 */
    MI355_SWS_K_NV12_PACK = 9,    /* the unscaled yuv420p -> NV12 / NV21 packer (k_sws_nv12_pack); scaled NV12 / NV21 contexts report PLANAR_A / B / C */
    MI355_SWS_K_NV12_SPLIT = 10,  /* the unscaled NV12 / NV21 -> yuv420p splitter (k_sws_nv12_split); scaled NV12 / NV21 SOURCES report the values above */
    MI355_SWS_K_YUY2_SPLIT = 11,  /* the unscaled yuyv422 / uyvy422 -> yuv420p / yuv422p splitter (k_sws_yuy2_split) */
    MI355_SWS_K_YUY2_PACK = 12    /* the unscaled yuv422p / yuv420p -> yuyv422 / uyvy422 packer (k_sws_yuy2_pack); scaled contexts to these destinations report the values above */
};
typedef struct mi355_sws_plan_info {
    int kernel;                   /* MI355_SWS_K_* */
    int th;                       /* output rows per tile of the generic kernel (0 for c24) */
    int hstage;                   /* horizontal source spans staged in LDS (monotonic positions, every tap inside its line) */
    int lum_lines, chr_lines;     /* the largest luma / chroma source span of a tile */
    int narrow;                   /* generic kernel: every tile takes the narrow form (dstW < 128 or a vertical filter of more than 8 taps);
                                   * 0: full tiles of an 8-byte aligned destination store from registers.  Planar kernels: dstW < 128 (every
                                   * tile partial) or a vertical filter of more than 8 taps (taps read from memory, not held in registers) */
} mi355_sws_plan_info;
int mi355_sws_plan(const mi355_sws_ctx *ctx, mi355_sws_plan_info *plan);   /* 0, -1 bad argument */

/* ---- planar destinations: yuv420p -> yuv420p / yuv422p / yuv444p, 8 bit (the planar branch of swscale(), swscale.c:618-645) ----
 * The descriptor is the one above with: chrDstW = the chroma output width (AV_CEIL_RSHIFT(dstW, chrDstHSubSample)), vChr.n = the chroma
 * output rows (chrDstH = AV_CEIL_RSHIFT(dstH, chrDstVSubSample), utils.c:1039-1040), unscaled_special = 0; the LUTs are not used.
 * The contexts of the RGB24 entry points and of these are not interchangeable: each entry point returns -1 on the other kind. */
enum { MI355_SWS_DST_YUV420P = 1, MI355_SWS_DST_YUV422P = 2, MI355_SWS_DST_YUV444P = 3 };
/* NULL (and a message) for banks the device tiles cannot hold, as mi355_sws_create */
mi355_sws_ctx *mi355_sws_create_planar(const mi355_sws_desc *desc, int dst_format);
/* one picture of a batch, device pointers; source planes as in mi355_sws_frame */
typedef struct mi355_sws_planar_frame {
    const uint8_t *src[3];
    int src_stride[3];
    uint8_t *dst[3];       /* Y, U, V planes of the destination */
    int dst_stride[3];
} mi355_sws_planar_frame;
/* Tier 2: a batch resident in HBM, one launch (0, -1 bad argument or not a planar context, -2 launch failure) */
int mi355_sws_scale_planar_frames_dev(mi355_sws_ctx *ctx, const mi355_sws_planar_frame *d_frames, int nframes, void *stream);
/* Tier 1: a whole picture, host pointers, synchronous; writes the first dstW / chrDstW bytes of each row (the caller's padding stays
 * untouched).  Returns the number of output lines, negative on failure. */
int mi355_sws_scale_planar(mi355_sws_ctx *ctx, const uint8_t *const src[3], const int src_stride[3],
                           uint8_t *const dst[3], const int dst_stride[3]);

/* ---- semi-planar destinations: NV12 / NV21, 8 bit (yuv2nv12cX_c output.c:267-301; planarToNv12Wrapper swscale_unscaled.c:138-156) ----
 * Both creators above and below take these two values as dst_format (4 .. 15 stay refused).  The descriptor is the reference's for that
 * context: chrDstW = AV_CEIL_RSHIFT(dstW, 1), vChr.n = chrDstH = AV_CEIL_RSHIFT(dstH, 1) (anything else is refused with a message), the LUTs
 * are not used.  Frames stay mi355_sws_planar_frame through mi355_sws_scale_planar_frames_dev / mi355_sws_scale_planar: dst[0] is luma,
 * dst[1] the interleaved plane — 2 * chrDstW bytes (U V U V ..., NV21: V U V U ...) on each of chrDstH rows; dst[2] and dst_stride[2] are
 * never read and may be NULL / 0.
 * The unscaled packer: desc->unscaled_special = 1 with one of these destinations — 8-bit 4:2:0 source, srcW == dstW, srcH == dstH, no banks
 * (any other combination: NULL and a message).  Like the reference it copies srcW x srcH luma bytes and interleaves srcW / 2 pairs on
 * srcH / 2 rows, both ROUNDED DOWN: the last pair of an odd width's chroma rows and the last chroma row of an odd height stay untouched. */
enum { MI355_SWS_DST_NV12 = 16, MI355_SWS_DST_NV21 = 17 };
/* the destination side of a context (read only) */
typedef struct mi355_sws_dest_info {
    int format;                   /* 0 rgb24, else MI355_SWS_DST_* */
    int planes;                   /* 1 rgb24 and the other packed destinations, 2 NV12 / NV21, 3 planar */
    int chr_bytes, chr_rows;      /* bytes per row and rows the context writes to each chroma plane (0 / 0 for rgb24; the packer: 2 * (srcW / 2), srcH / 2;
                                   * the splitter: srcW / 2, srcH / 2; the packed-4:2:2 splitter: (srcW + 1) / 2, and srcH / 2 to yuv420p, srcH to yuv422p) */
} mi355_sws_dest_info;
int mi355_sws_destination(const mi355_sws_ctx *ctx, mi355_sws_dest_info *info);   /* 0, -1 bad argument */

/* ---- other sources: planar yuv 4:2:0 / 4:2:2 / 4:4:4 at 8, 9 or 10 bits (yuv420p ... yuv444p10le) -----------------------------------------
 * The descriptor is the one above as the reference's init built it for that source (chrSrcW / chrSrcH and the four banks follow the
 * subsampling, utils.c:1035-1040).  A source deeper than 8 bits takes hScale16To15_c (swscale.c:110-130) in place of hScale8To15_c, and an
 * 8-bit planar destination is then dithered (should_dither :389, :553-556): the 8x8 rows are an input like the banks (ff_dither_8x8_128).
 * Samples deeper than 8 bits are uint16_t, little endian, BELOW 1 << depth (what a decoder writes; the sums then stay inside an int as the
 * reference's do) — larger values are outside the contract.  Source pointers stay const uint8_t * and strides are bytes; for 16-bit samples
 * both must be even.  The alignment paragraph above mi355_sws_frame holds unchanged in bytes: a plane whose pointer and stride are multiples
 * of 16 is fetched in aligned 16-byte pieces (eight samples) and must be readable over its whole stride; a plane on 4-byte multiples is
 * staged in dwords; any other (2-byte multiples) is read sample by sample. */
typedef struct mi355_sws_src {
    int depth;                    /* 8, 9 or 10 */
    int hsub, vsub;               /* chroma shifts: 1,1 4:2:0; 1,0 4:2:2; 0,0 4:4:4 */
    uint8_t dither[8][8];         /* read for a planar destination with depth > 8 */
} mi355_sws_src;
/* dst_format 0: rgb24 (a context for mi355_sws_scale / mi355_sws_scale_frames_dev), else MI355_SWS_DST_* (for the planar entry points).
 * NULL (and a message) for banks the device tiles cannot hold and for combinations outside the list above; the unscaled special converter
 * (desc->unscaled_special) takes 8-bit 4:2:0 and 4:2:2 only to rgb24, and 8-bit 4:2:0 only to NV12 / NV21 (the packer).  depth 8, shifts 1,1 builds the context of mi355_sws_create /
 * mi355_sws_create_planar. */
mi355_sws_ctx *mi355_sws_create_src(const mi355_sws_desc *desc, const mi355_sws_src *src, int dst_format);
/* the source side of a context (read only) */
typedef struct mi355_sws_source_info {
    int depth, hsub, vsub;
    int hstaged;                  /* a tile kernel whose horizontal pass stages source spans in LDS for this context: monotonic positions, every tap
                                   * inside its line, a plane whose filter is not the identity and a tile of it whose span fits a staged line
                                   * (planes on 4-byte multiples; the others, and the other contexts, read sample by sample) */
} mi355_sws_source_info;
int mi355_sws_source(const mi355_sws_ctx *ctx, mi355_sws_source_info *info);   /* 0, -1 bad argument */

/* ---- semi-planar sources: NV12 / NV21, 8 bit (nv12ToUV_c / nv21ToUV_c input.c:475-497 in front of hcScale; nv12ToPlanarWrapper
 * swscale_unscaled.c:158-177) ----
 * layout 0: exactly mi355_sws_create_src.  1 / 2: an 8-bit 4:2:0 source whose second plane holds chrSrcW byte pairs (U V .., NV21: V U ..)
 * on chrSrcH rows; src->depth must be 8 and the shifts 1,1 (anything else: NULL and a message).  The descriptor is the reference's for that
 * context — its banks are those of the yuv420p context of the same sizes and flags.  dst_format takes every value mi355_sws_create_src takes.
 * Frames stay mi355_sws_frame / mi355_sws_planar_frame through the four scale entry points: src[1] is the pair plane, 2 * chrSrcW bytes a row;
 * src[2] and src_stride[2] are never read and may be NULL / 0.  The alignment paragraph above mi355_sws_frame holds for the pair plane in
 * bytes: pointer and stride on 16-byte multiples — aligned 16-byte pieces, readable over the whole stride; on 4-byte multiples — dwords;
 * anything else is read sample-exactly (a pair may start on an odd address).
 * The unscaled splitter: desc->unscaled_special = 1 with layout 1 / 2 and dst_format MI355_SWS_DST_YUV420P — srcW == dstW, srcH == dstH, no banks
 * (every other special combination with such a layout, rgb24 included: NULL and a message; the reference has no special converter from these
 * sources to rgb24, it runs its generic scaler).  Like the reference it copies srcW x srcH luma bytes and de-interleaves srcW / 2 pairs on
 * srcH / 2 rows, both ROUNDED DOWN: the last byte of an odd width's chroma rows and the last chroma row of an odd height stay untouched
 * (mi355_sws_destination reports chr_bytes = srcW / 2, chr_rows = srcH / 2). */
enum { MI355_SWS_SRC_PLANAR = 0, MI355_SWS_SRC_NV12 = 1, MI355_SWS_SRC_NV21 = 2 };
mi355_sws_ctx *mi355_sws_create_src_layout(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, int dst_format);
int mi355_sws_source_layout(const mi355_sws_ctx *ctx);   /* MI355_SWS_SRC_*, -1 bad argument */

/* ---- packed sources: rgb24 / bgr24 (rgb24ToY_c / bgr24ToY_c and the ...ToUV_c / ...ToUV_half_c pairs, input.c:539-623, in front of
 * hyScale / hcScale) ----
 * layout 4 / 5 of mi355_sws_create_src_layout (3 stays refused): ONE source plane of srcW pixels, three bytes each (R G B, bgr24: B G R), which
 * the reference converts line by line into 8-bit Y, U and V lines with fixed BT.601 constants and then scales like an 8-bit planar source.  The
 * source record says which chroma converter the reference chose (utils.c:1023-1038, carried as it is, not second-guessed): src->hsub 1 — the
 * halving one (each chroma sample from the sum of two neighbouring pixels, chrSrcW = AV_CEIL_RSHIFT(srcW, 1)), src->hsub 0 — the full one
 * (chrSrcW = srcW); src->depth must be 8, src->vsub 0 and desc->chrSrcH == desc->srcH (anything else: NULL and a message).  dst_format takes
 * every value mi355_sws_create_src takes.  These sources have no special converter here: desc->unscaled_special = 1 is refused with a message
 * (bgr24ToYv12Wrapper, rgbToRgbWrapper and the plain copy stay with the reference), and so is a context that scales neither way to rgb24
 * (the reference never builds one).  mi355_sws_plan reports GENERIC_A .. C / PLANAR_A .. C as for the planar source of the same banks.
 * Frames stay mi355_sws_frame / mi355_sws_planar_frame through the four scale entry points: src[0] is the packed plane, 3 * srcW bytes a row;
 * src[1], src[2] and their strides are never read and may be NULL / 0.  A packed plane whose pointer and stride are multiples of 4 is fetched in
 * dwords that lie whole inside the bytes of the line named here; any other plane is read byte by byte.  No byte past them is read:
 * a line is read over 3 * srcW bytes — and, with hsub == 1 and an ODD srcW, over 3 * (srcW + 1) bytes, as the reference reads it (its last
 * chroma sample takes pixel srcW, whatever lies there: the next line's first pixel, padding, or the bytes behind the picture).  The caller keeps
 * those three bytes readable on the last line too.  The Tier-1 host entry points return -1 when src_stride[0] < 3 * srcW. */
enum { MI355_SWS_SRC_RGB24 = 4, MI355_SWS_SRC_BGR24 = 5 };

/* ---- packed 32-bit sources: rgba / bgra / argb / abgr (the reference's rgb32ToY_c / bgr32ToY_c / rgb321ToY_c / bgr321ToY_c and their ...ToUV_c /
 * ...ToUV_half_c forms: rgb16_32ToY_c_template and its kin behind the four wrappers with S = RGB2YUV_SHIFT + 8, input.c:165-291) ----
 * layout 8 .. 11 of mi355_sws_create_src_layout and of every creator that forwards to it (3, 6 and 7 stay refused).  The names give the byte order IN
 * MEMORY, as for the destinations.  The wrappers' constants are the rgb24 ones shifted up by eight and their masks remove the alpha byte before
 * anything is summed (also in the halving form): the Y, U and V bytes are those of rgb24ToY_c / rgb24ToUV_c / rgb24ToUV_half_c on the pixel's three
 * colour bytes.  Everything said of the rgb24 / bgr24 sources holds with four bytes a pixel: ONE source plane, 4 * srcW bytes a row; src->depth 8,
 * src->vsub 0, desc->chrSrcH == desc->srcH, src->hsub 1 / 0 the halving / the full chroma converter as the reference chose it; every dst_format the
 * rgb24 source takes (0, 32 .. 36, the planar and semi-planar ones, a range to a YUV destination, a 9- / 10-bit planar depth) and its refusals
 * (desc->unscaled_special, a context that scales neither way to a packed RGB destination, banks the tiles cannot hold); mi355_sws_plan reports
 * GENERIC_A .. C / PLANAR_A .. C.  To a 32-bit destination these creators write 255 as the alpha byte (the colour bytes never depend on alpha);
 * mi355_sws_create_src_layout_alpha below carries the source's alpha there, as the reference does.
 * The plane's pointer and stride must be multiples of 4 — the reference reads a pixel as one aligned dword (AV_RN32A): the Tier-1 host entry points
 * return -1 otherwise, and for a stride below 4 * srcW.  A plane on 16-byte multiples is fetched in 16-byte pieces, any other in dwords, each whole
 * inside the bytes named here: a line is read over 4 * srcW bytes — and, with hsub == 1 and an ODD srcW, over 4 * (srcW + 1) bytes, as the reference
 * reads it.  No byte past that is read; the caller keeps those four bytes readable on the last line too. */
enum { MI355_SWS_SRC_RGBA = 8, MI355_SWS_SRC_BGRA = 9, MI355_SWS_SRC_ARGB = 10, MI355_SWS_SRC_ABGR = 11 };
/* ... with the source's alpha carried to a 32-bit destination, as a reference context does whose source AND destination both have alpha: it keeps a
 * third ring buffer (alpPixBuf, utils.c:1244), reads alpha through rgbaToA_c / abgrToA_c (input.c:305-319), scales it with the LUMA banks
 * (swscale.c:269-276, :511-513) and writes it through the hasAlpha forms of yuv2rgb_X / _2 / _1_c_template (output.c:937-1110; its tables then hold
 * 0 in the alpha lane).  So a resized picture's alpha is filtered like its luma — not 255, and not a copy.
 * alpha 0: exactly mi355_sws_create_src_layout (a 32-bit destination gets 255: a reference without an alpha buffer).  alpha 1: src_layout 8 .. 11 to
 * dst_format MI355_SWS_DST_RGBA ... _ABGR with desc->unscaled_special 0; NULL and a message for anything else, and for everything the colour-only
 * context is refused for.  The descriptor, the frames (mi355_sws_frame) and the entry points are the colour-only context's; mi355_sws_plan reports
 * its values (lum_lines then also counts the lines of the alpha tile).  The alpha tile holds as many lines as the luma tile, in LDS of its own: 7 / 10 /
 * 12 KB on top of the 19 / 23 / 26 KB of GENERIC_A / B / C — every context the colour-only creator takes still fits a workgroup's LDS, so none is refused
 * for its alpha; fewer workgroups share a CU (6 / 4 / 4 where the twins have 8 / 7 / 6). */
mi355_sws_ctx *mi355_sws_create_src_layout_alpha(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, int dst_format, int alpha);
int mi355_sws_alpha(const mi355_sws_ctx *ctx);   /* 0 / 1, -1 bad argument */

/* ---- packed 4:2:2 sources: yuyv422 / uyvy422 / yvyu422 (what capture devices deliver; the reference's yuy2ToY_c / yuy2ToUV_c / yvy2ToUV_c /
 * uyvyToY_c / uyvyToUV_c input.c:369-473, pure byte picks in front of hyScale / hcScale, and its four unscaled converters yuyvToYuv420Wrapper /
 * uyvyToYuv420Wrapper / yuyvToYuv422Wrapper / uyvyToYuv422Wrapper swscale_unscaled.c:227-287 over yuyvtoyuv420_c ... uyvytoyuv422_c
 * rgb2rgb_template.c:854-928) ----
 * layout 16 .. 18 of mi355_sws_create_src_layout and of every creator that forwards to it (3, 6, 7 and 12 .. 15 stay refused).  The names give the
 * byte order IN MEMORY, per group of four bytes covering pixels 2i and 2i + 1:
 *   yuyv422  Y0 U Y1 V   luma x at byte 2x,     U i at 4i + 1, V i at 4i + 3
 *   yvyu422  Y0 V Y1 U   luma x at byte 2x,     U i at 4i + 3, V i at 4i + 1
 *   uyvy422  U Y0 V Y1   luma x at byte 2x + 1, U i at 4i,     V i at 4i + 2
 * Nothing is rounded, weighted or clipped in front of the scaler: the picked bytes are the samples of an 8-bit 4:2:2 source.  The source record is
 * that source's: src->depth 8, src->hsub 1, src->vsub 0, desc->chrSrcW == AV_CEIL_RSHIFT(srcW, 1), desc->chrSrcH == desc->srcH (anything else: NULL
 * and a message).  The frame is ONE source plane of 2 * srcW bytes a row in src[0]; src[1], src[2] and their strides are never read and may be
 * NULL / 0.  mi355_sws_create_src_layout_alpha with alpha 1 refuses these layouts (NULL and a message).
 * The SCALER (desc->unscaled_special 0) takes all three layouts to every dst_format the rgb24 source takes: 0 and 32 .. 36, MI355_SWS_DST_YUV420P /
 * _YUV422P / _YUV444P at 8, 9 and 10 bits, _NV12 / _NV21, and both ranges (FROM_JPEG and TO_JPEG: unlike an RGB source a YUV source can differ from its
 * destination either way) to every 8-bit YUV destination.  Twin rule: such a context has the banks, the plan (GENERIC_A .. C, PLANAR_A .. C, IDENT1_1)
 * and the refusals of the 8-bit yuv422p-source context with the same descriptor — it is refused exactly where that twin's tiles cannot hold the
 * lines; chroma sits on every source line.  At equal size to a packed RGB destination (the reference has no special converter there and runs its
 * scaler with one luma and one chroma tap) the plan is MI355_SWS_K_IDENT1_1, straight from the packed bytes (k_sws_ident1_yuy2), never the tile
 * kernel; with vsub 0 no context reaches MI355_SWS_K_IDENT1_X.
 * The four unscaled special converters: desc->unscaled_special = 1 with layout 16 / 17 (the reference has no wrapper for
 * yvyu422: layout 18 is refused) to MI355_SWS_DST_YUV420P or _YUV422P — 8 bit, no range, srcW == dstW, srcH == dstH, chrDstW == AV_CEIL_RSHIFT(dstW, 1),
 * no banks; every other special combination gets NULL and a message.  Frames go through the planar entry points (mi355_sws_planar_frame).  Luma:
 * srcW bytes on each of srcH rows.  To yuv422p: AV_CEIL_RSHIFT(srcW, 1) bytes of each chroma plane on each of srcH rows.  To yuv420p: chroma row r is
 * (a + b) >> 1 of source lines 2r and 2r + 1, truncating as the C template does — AV_CEIL_RSHIFT(srcW, 1) bytes on srcH / 2 rows ROUNDED DOWN: the
 * last chroma row of an odd height stays untouched and a one-line picture writes no chroma at all (NOT the NV splitter's rule, which rounds the width
 * down too).  mi355_sws_destination reports those chr_bytes / chr_rows, mi355_sws_plan MI355_SWS_K_YUY2_SPLIT.
 * Read extent and alignment.  A line is read over 2 * srcW bytes — and, with an ODD srcW, over 2 * (srcW + 1) bytes, as the reference reads it: its
 * last chroma sample takes the second half of the last group, whatever lies there (the next line's first bytes, padding, or the bytes behind the
 * picture).  The caller keeps those two bytes readable on the last line too.  No byte past that is read, except on a plane whose pointer and stride
 * are multiples of 16: it is fetched in aligned 16-byte pieces and must be readable over its whole stride.  A plane on 4-byte multiples is fetched
 * in dwords that lie whole inside the bytes named here; any other plane is read byte by byte (the reference has no alignment demand on these
 * formats: a pixel pair may start on an odd address).  The Tier-1 host entry points return -1 for src_stride[0] < 2 * srcW. */
enum { MI355_SWS_SRC_YUYV422 = 16, MI355_SWS_SRC_UYVY422 = 17, MI355_SWS_SRC_YVYU422 = 18 };

/* ---- P010 sources: p010le (what hardware decoders and 10-bit HEVC / AV1 pipelines hand over; the reference's p010LEToY_c / p010LEToUV_c
 * input.c:499-524 in front of hScale16To15_c with depth 10.  A source only in the reference, utils.c:205-206, and without any unscaled converter: it is
 * even kept off the plane copy, swscale_unscaled.c:1162-1167 — every P010 context, equal size included, is a context of the generic scaler) ----
 * layout 24 of mi355_sws_create_src_layout and of every creator that forwards to it (3, 6, 7, 12 .. 15, 19 .. 23 and 25 and up stay refused; p010be is
 * not taken, no big-endian format is).  The source record is that of a 10-bit 4:2:0 source: src->depth 10, src->hsub 1, src->vsub 1,
 * desc->chrSrcW == AV_CEIL_RSHIFT(srcW, 1), desc->chrSrcH == AV_CEIL_RSHIFT(srcH, 1); src->dither is read for an 8-bit planar / semi-planar destination,
 * as for any deep source (anything else: NULL and a message).  desc->unscaled_special = 1 is refused with a message: the reference has no wrapper from
 * P010.  mi355_sws_create_src_layout_alpha with alpha 1 refuses the layout.
 * Frames stay mi355_sws_frame / mi355_sws_planar_frame through the four scale entry points: src[0] is the luma plane, srcW little-endian uint16_t on
 * each of srcH rows; src[1] is the pair plane, chrSrcW pairs U V of uint16_t — four bytes a pair — on chrSrcH rows; src[2] and src_stride[2] are never
 * read and may be NULL / 0.  Pointers and strides are bytes and must be even: the Tier-1 host entry points return -1 otherwise, and for a stride below
 * 2 * srcW or 4 * chrSrcW.
 * The sample is word >> 6, exactly as the reference's two converters compute it, and EVERY uint16_t value is inside the contract: the low six bits are
 * dropped, not required to be zero.  (This differs from the planar 9- / 10-bit sources above, whose samples must lie below 1 << depth.)
 * Destinations: every dst_format the yuv420p10le source takes — 0 and 32 .. 36, 48 .. 50, MI355_SWS_DST_YUV420P / _YUV422P / _YUV444P at 8, 9 and 10
 * bits, _NV12 / _NV21, and range 1 / 2 to every 8-bit YUV destination, the packed 4:2:2 ones included.  Twin rule: a P010 context has the banks, the
 * plan (GENERIC_A .. C / PLANAR_A .. C), the narrow / hstage report and the refusals of the planar context with src_layout 0, depth 10, shifts 1, 1
 * and the same descriptor; like every deep source it is never IDENT1_* or C24, and it is refused exactly where the twin's tiles cannot hold the lines.
 * mi355_sws_source_layout returns 24, mi355_sws_source 10 / 1 / 1 and hstaged under the rule stated there (the pair plane is de-interleaved as it is
 * staged: a chroma tile's span fits where the twin's fits).
 * Read extent and alignment, in bytes as in the paragraph above mi355_sws_frame: a plane whose pointer and stride are multiples of 16 is fetched in
 * aligned 16-byte pieces and must be readable over its whole stride; a plane on 4-byte multiples is fetched in dwords that lie whole inside the row;
 * anything else (2-byte multiples: a pair may start at an address that is 2 mod 4) is read sample by sample.  No byte behind 2 * srcW of a luma row or
 * 4 * chrSrcW of a pair row is read otherwise; with an odd srcW the last pair is ordinary plane content, not a read behind the width. */
enum { MI355_SWS_SRC_P010 = 24 };

/* ---- range conversion: contexts whose source and destination differ in range, to a YUV destination (yuvj420p <-> yuv420p and their kin:
 * c->srcRange != c->dstRange && !isAnyRGB(c->dstFormat), lumConvertRange / chrConvertRange swscale.c:168-198, :748-766) ----
 * The reference applies the two converters to every horizontally scaled int16 line, between hyScale / hcScale and the vertical pass
 * (swscale.c:284-285, :334-335); so does a context created here, on the lines of its LDS tile.  Such a context has the banks of its same-range
 * twin (and is refused exactly where the twin is), and runs the generic scaler at equal size too (utils.c:1044 keeps it off the unscaled
 * converters).  The 8-bit destination forms, 32-bit arithmetic, the result stored back as int16 (truncated, as the reference's store):
 *   FROM_JPEG (full -> limited)  luma (v * 14071 + 33561947) >> 14                  chroma (v * 1799 + 4081085) >> 11
 *   TO_JPEG   (limited -> full)  luma (min(v, 30189) * 19077 - 39057361) >> 14      chroma (min(v, 30775) * 4663 - 9289992) >> 12
 * range 0: exactly mi355_sws_create_src_layout (same plan, same kernel, same bytes).  1 / 2: every src_layout (0, 1, 2, 4, 5), depth and
 * subsampling that creator takes, to every YUV dst_format (MI355_SWS_DST_YUV420P / 422P / 444P / NV12 / NV21).  NULL and a message for a range
 * outside 0..2, for a range with dst_format 0 (an rgb24 destination takes the range into its LUTs: create it without one) and for a range with
 * desc->unscaled_special (the reference never builds either).  Frames go through mi355_sws_scale_planar_frames_dev / mi355_sws_scale_planar;
 * mi355_sws_plan reports PLANAR_A / B / C as for the same banks without a range. */
enum { MI355_SWS_RANGE_NONE = 0, MI355_SWS_RANGE_FROM_JPEG = 1, MI355_SWS_RANGE_TO_JPEG = 2 };
mi355_sws_ctx *mi355_sws_create_src_layout_range(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, int dst_format, int range);
int mi355_sws_range(const mi355_sws_ctx *ctx);   /* MI355_SWS_RANGE_*, -1 bad argument */

/* ---- planar destinations of 9 or 10 bits: yuv420p9le / yuv422p9le / yuv444p9le / yuv420p10le / yuv422p10le / yuv444p10le
 * (yuv2plane1_10_c_template / yuv2planeX_10_c_template, output.c:183-213) ----
 * For a destination of 15 bits or fewer the reference keeps its 15-bit int16 intermediates (swscale.c:733-752), so such a context has the plan, the
 * banks and the refusals of its 8-bit twin; only the vertical store differs.  32-bit arithmetic, no dither (also from a 9- or 10-bit source):
 *   one vertical tap (the coefficient is unused)   clip((s + (1 << (14 - bits))) >> (15 - bits))
 *   otherwise                                      clip(((1 << (26 - bits)) + sum s_j * f_j) >> (27 - bits))
 * with clip to 0 .. (1 << bits) - 1.
 * dst_depth 8: exactly mi355_sws_create_src_layout_range (same plan, same kernel, same bytes).  9 / 10: every src_layout (0, 1, 2, 4, 5), depth and
 * subsampling that creator takes, to dst_format MI355_SWS_DST_YUV420P / 422P / 444P only — the format names the subsampling, the depth travels
 * beside it; range must be 0 and desc->unscaled_special 0 (at equal size with equal subsampling the reference copies planes, planarCopyWrapper:
 * not a context of the scaler).  The descriptor is the reference's for that context: chrDstW, vChr.n = chrDstH as for the 8-bit planar
 * destination.  NULL and a message for any other depth, for a depth with dst_format 0 / NV12 / NV21, with a range or with a special converter,
 * and for everything the 8-bit twin is refused for.
 * Frames stay mi355_sws_planar_frame through mi355_sws_scale_planar_frames_dev / mi355_sws_scale_planar: dst[k] and dst_stride[k] stay byte
 * pointers and byte strides, both EVEN; a row holds uint16_t samples, little endian, below 1 << dst_depth; only the first dstW / chrDstW samples
 * of a row are written.  A row whose address is a multiple of 16 is stored in 16-byte pieces, any other sample by sample.  The Tier-1 host entry
 * returns -1 for an odd stride or a stride below 2 * width.  mi355_sws_destination reports format 1 / 2 / 3, three planes and
 * chr_bytes = 2 * chrDstW; mi355_sws_plan PLANAR_A / B / C as for the twin; mi355_sws_range 0. */
mi355_sws_ctx *mi355_sws_create_src_layout_range_depth(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, int dst_format, int range,
                                                       int dst_depth);
int mi355_sws_dest_depth(const mi355_sws_ctx *ctx);   /* 8 / 9 / 10, -1 bad argument */

/* ---- packed destinations beside rgb24: bgr24 and the four 32-bit orders rgba / bgra / argb / abgr (yuv2rgb_write output.c:825-867 behind the three
 * packed templates yuv2rgb_X / _2 / _1_c_template :937-1110; yuv2rgb_c_24_bgr yuv2rgb.c:366-394 and yuv2rgb_c_32 :237-265) ----
 * The names give the byte order IN MEMORY (the reference's RGB32 / BGR32 / _1 names are host-endian aliases of these).  mi355_sws_create_src_layout_range_depth
 * and the creators that forward to it (mi355_sws_create_src, _src_layout, _src_layout_range) take the five values as dst_format with every source the
 * rgb24 destination takes: src_layout 0, 1, 2, 4, 5, depth 8 / 9 / 10 at 4:2:0 / 4:2:2 / 4:4:4.  The descriptor is the reference's for that context and
 * has the form of the rgb24 one: chrDstW = AV_CEIL_RSHIFT(dstW, 1), vChr.n = dstH, and the LUTs in the form of mi355_sws_luts — for a 32-bit order
 * y_table[i] is the colour byte of the reference's uint32_t table entry i (the same clipped value the 24-bpp table holds, yuv2rgb.c:850-888) and the
 * four offset rows count ELEMENTS of that table with the g / b plane bases (1024 / 2048 elements) removed; the device adds 255 as the alpha byte (a
 * source without alpha).  Such a context has the banks, the plan (GENERIC_A / B / C, IDENT1_1 / _X, C24) and the refusals of its rgb24 twin: NULL and a
 * message for banks the device tiles cannot hold, for a packed-RGB source that scales neither way and for desc->unscaled_special from a packed or an
 * NV source; and, as for rgb24, for a range other than 0, a dst_depth other than 8, and for values of 37 and up (4 .. 15 and 18 .. 31 stay refused).
 * desc->unscaled_special = 1 with one of the five values is the unscaled special converter to that format: 8-bit 4:2:0 and 4:2:2 sources, exactly where
 * rgb24 takes k_sws_c24.
 * Frames stay mi355_sws_frame — ONE packed destination plane — through mi355_sws_scale / mi355_sws_scale_frames_dev; the planar entry points return -1.
 * A row holds 3 * dstW or 4 * dstW bytes: exactly dstW pixels are written, as for rgb24 (the reference's pair loops also write a partner of an odd
 * width's last pixel, from a line-buffer sample it never initialised; that pixel is not reproduced and the bytes behind the row stay untouched; the
 * special converter writes dstW & ~1 pixels, as the reference's).  A 32-bit destination's pointer and stride must be multiples of 4 (a pixel is stored
 * as a dword): the Tier-1 host entry returns -1 otherwise, and for a stride below the row.  A full tile (128 pixels of the tile kernel, eight of
 * k_sws_ident1 / k_sws_c24) of a 32-bit row whose pointer and stride are multiples of 16 is stored from registers in 16-byte pieces; of a 24-bit row
 * on multiples of 8 in 8-byte pieces (the rgb24 rule); every other tile of the tile kernel goes through LDS rows and leaves in 16-byte, 4-byte or
 * (24-bit only) single-byte pieces as pointer, stride and row length allow, and the other two kernels write it pair by pair.
 * mi355_sws_destination reports the format, planes = 1 and chr_bytes = chr_rows = 0; mi355_sws_dest_depth 8; mi355_sws_range 0; mi355_sws_plan the
 * twin's values — there is no MI355_SWS_K_* of these destinations: the twin's value with the destination's format names the kernel.
 * Not taken (the reference's): 15 / 16-bit and lower RGB (dithered, other tables), rgb48 / rgba64, planar GBR of 9 / 10 / 12 / 16 bits and gbrap
 * (8-bit gbrp: mi355_sws_create_gbrp below), alpha from a YUVA source, SWS_FULL_CHR_H_INT to THESE destinations (the reference forces it for gbrp
 * alone), rgbToRgbWrapper, and a range or a 9 / 10-bit depth with these destinations. */
enum { MI355_SWS_DST_BGR24 = 32, MI355_SWS_DST_RGBA = 33, MI355_SWS_DST_BGRA = 34, MI355_SWS_DST_ARGB = 35, MI355_SWS_DST_ABGR = 36 };

/* ---- packed 4:2:2 destinations: yuyv422 / uyvy422 / yvyu422 (what capture, SDI and display pipelines take back; yuv2422_X / _2 / _1_c_template
 * output.c:451-582 behind c->yuv2packedX / 2 / 1, and the four unscaled packers yuv422pToYuy2Wrapper / yuv422pToUyvyWrapper / planarToYuy2Wrapper /
 * planarToUyvyWrapper swscale_unscaled.c:179-225, :1123-1139) ----
 * The names give the byte order IN MEMORY, per group of four bytes covering pixels 2i and 2i + 1, as for the sources:
 *   yuyv422  Y1 U Y2 V      yvyu422  Y1 V Y2 U      uyvy422  U Y1 V Y2
 * mi355_sws_create_src_layout_range_depth and the creators that forward to it take the three values as dst_format with every source the rgb24
 * destination takes: src_layout 0, 1, 2, 4, 5, 8 .. 11 and 16 .. 18, depth 8 / 9 / 10 at 4:2:0 / 4:2:2 / 4:4:4; mi355_sws_create_src_layout_alpha with
 * alpha 1 refuses them (NULL and a message).  37 .. 47 and 51 and up stay refused.  The descriptor is the reference's for that context and has the form
 * of the rgb24 one: chrDstW = AV_CEIL_RSHIFT(dstW, 1), vChr.n = dstH; the LUTs are not read.
 * Twin rule: such a context has the plan (GENERIC_A / B / C, IDENT1_1 / _X), the instance and the refusals of the rgb24-destination context of the same
 * descriptor and source — NULL and a message exactly where that twin's tiles cannot hold the lines — with ONE exception: a packed-RGB source at equal
 * size IS a context of the reference's scaler to these destinations (to rgb24 it is a copy or rgbToRgbWrapper), so the "scales neither way" refusal
 * does not apply and such a context runs the tile kernel.
 * Range: these are YUV destinations, so range 1 / 2 is accepted (mi355_sws_create_src_layout_range's formulas on the lines of the LDS tile between the
 * two passes, over dstW luma and chrDstW chroma samples); such a context has the banks of its same-range twin.  dst_depth must be 8.
 * The arithmetic, 32 bit, per pair i (luma samples 2i and 2i + 1, chroma sample i); the form is chosen as for the packed RGB destinations
 * (one luma tap and at most two chroma taps: _1; two and two: _2; otherwise X):
 *   X    each of Y1, Y2, U, V is ((1 << 18) + sum s_j * f_j) >> 19; if (Y1 | Y2 | U | V) & 0x100 all four are clipped to 0 .. 255, otherwise the four
 *        values are stored as they are, truncated to a byte (the reference's rule: 600 has bit 9 but not bit 8 and is stored as 88)
 *   _2   (a * (4096 - alpha) + b * alpha) >> 19, always clipped
 *   _1   luma >> 7; chroma >> 7 for uvalpha < 2048, else (u0 + u1) >> 8; always clipped
 * Frames stay mi355_sws_frame — ONE packed destination plane — through mi355_sws_scale / mi355_sws_scale_frames_dev; the planar entry points return -1.
 * A row holds 4 * ((dstW + 1) >> 1) bytes: all of them are written and no byte behind them.  With an odd dstW the last group's second luma byte is 0
 * in all three forms, with and without a range (the reference computes it from the sample behind the line of its zero-allocated line buffer, which
 * neither the horizontal scaler nor the range converter touches).  The destination has no alignment demand: a full tile (128 pixels) of a row whose
 * pointer and stride are multiples of 16 leaves from registers in 16-byte pieces, eight pixels a thread; every other tile goes through LDS rows and
 * leaves in 16-byte, 4-byte or single-byte pieces as pointer, stride and row length allow.  The Tier-1 host entry returns -1 for a stride below the row.
 * mi355_sws_destination reports the format, planes = 1 and chr_bytes = chr_rows = 0; mi355_sws_dest_depth 8; mi355_sws_range the range;
 * mi355_sws_plan the twin's values.
 * The four unscaled packers: desc->unscaled_special = 1 with src_layout 0, depth 8, source shifts 1,0 (yuv422pToYuy2Wrapper / yuv422pToUyvyWrapper, any
 * flags) or 1,1 (planarToYuy2Wrapper / planarToUyvyWrapper: the reference takes them under SWS_POINT / SWS_FAST_BILINEAR only) to
 * MI355_SWS_DST_YUYV422 or _UYVY422 (the reference has no wrapper to yvyu422) — srcW == dstW, srcH == dstH, no banks, range 0; every other special
 * combination with these destinations gets NULL and a message.  Byte picks only, chroma of row y from chroma row y >> vsub; mi355_sws_plan reports
 * MI355_SWS_K_YUY2_PACK.  The reference's loop writes two groups a step — G = 2 * ceil((srcW >> 1) / 2) groups on a row; the device writes
 * min(G, (srcW + 1) >> 1) groups and never past the row:
 *   srcW % 4 == 0 or 2   srcW / 2 groups (at remainder 2 the reference's extra group BEHIND the row is not reproduced)
 *   srcW % 4 == 1        (srcW - 1) / 2 groups: the last pixel stays untouched, as in the reference
 *   srcW % 4 == 3        (srcW + 1) / 2 groups: the last group's second luma byte is the source byte at x = srcW, as the reference reads it — the
 *                        caller keeps that one byte readable on the last line too; it is the only read behind a width (the last group's chroma is
 *                        sample (srcW - 1) / 2, inside the chroma width)
 * A plane on 16-byte multiples is fetched in aligned 16-byte pieces over its stride, as everywhere else.
 * A packed 4:2:2 source to ANOTHER packed 4:2:2 order at equal size is a context of the reference's scaler (banks of one tap each: it has no converter
 * between the orders) and has its twin's plan, MI355_SWS_K_IDENT1_1 straight from the packed bytes; to the SAME order the reference copies.
 * Not taken (the reference's): 9 / 10 / 16-bit packed YUV (y210 and kin), a YUVA source's alpha, SWS_FAST_BILINEAR scaled contexts of any source but the
 * planar 8-bit ones (those: mi355_sws_create_fast_bilinear below), gbrp / gbrap SOURCES, and the plain copy. */
enum { MI355_SWS_DST_YUYV422 = 48, MI355_SWS_DST_UYVY422 = 49, MI355_SWS_DST_YVYU422 = 50 };

/* ---- SWS_FAST_BILINEAR contexts: the reference's cheap scaler (c->hyscale_fast / c->hcscale_fast = hyscale_fast_c / hcscale_fast_c, swscale.c:238-249,
 * :288-301, chosen at :733-739 when srcBpc == 8, dstBpc <= 15 and the flag is set) ----
 * Its horizontal pass reads NO filter bank: output sample i of a plane is
 *   xpos = i * xInc (unsigned 32 bit);  xx = xpos >> 16;  a = (xpos & 0xFFFF) >> 9          (0 .. 127)
 *   luma    (src[xx] << 7) + (src[xx + 1] - src[xx]) * a
 *   chroma   src[xx] * (a ^ 127) + src[xx + 1] * a                                           (the weights sum to 127, not 128)
 * with xInc = c->lumXInc for luma and c->chrXInc for chroma AS THE REFERENCE'S INIT LEFT THEM (utils.c:968, :1081-1101: a plain-C build has
 * ((srcW << 16) + (dstW >> 1)) / dstW, other builds alter it by +-20): the binding hands both over unchanged, nothing here recomputes them.  At equal
 * width (xInc 65536) luma is src << 7 but chroma src * 127: such a context is never MI355_SWS_K_IDENT1_*.  The range converters and the vertical pass
 * follow on the int16 lines as in every other context; the vertical banks are the reference's ordinary ones.
 * Source: layout 0 (three planes) with src->depth == 8 at 4:2:0, 4:2:2 or 4:4:4, no alpha — the creator has no layout and no alpha argument, so
 * mi355_sws_source_layout is 0 and mi355_sws_alpha 0 for every such context.  NV12 / NV21, packed RGB, packed 4:2:2 and P010 sources stay the
 * reference's: it runs the fast pass on its conversion buffer for those, and the sample behind the width is then uninitialised heap memory that no
 * device code can reproduce.  Deeper sources never take the fast pass in the reference (srcBpc == 8 only).
 * Descriptor: the reference's for that context.  vLum / vChr are its vertical banks (vChr.n = dstH for a one-plane destination, chrDstH otherwise, as for
 * the twin); hLum / hChr are NOT read and may be empty (coef / pos NULL).
 * Twin rule: the twin is the bank-driven context of mi355_sws_create_src_layout_range_depth(desc, src, 0, dst_format, range, dst_depth).  A
 * fast-bilinear context takes every dst_format, range and dst_depth the twin takes (0 and 32 .. 36, 48 .. 50, the three planar formats at 8 / 9 / 10 bits,
 * NV12 / NV21, range 1 / 2 to the 8-bit YUV destinations) and has the twin's plan by lum_lines / chr_lines (MI355_SWS_K_GENERIC_A .. C / _PLANAR_A ..
 * C), th, narrow report and vertical refusals; hstage is always 1; it is never IDENT1_*, C24 or a packer.  Frames are mi355_sws_frame /
 * mi355_sws_planar_frame through the four scale entry points, and mi355_sws_destination / _range / _dest_depth / _source report the twin's values
 * (hstaged: a tile's span fits a staged line).
 * NULL and a message for: src->depth other than 8; desc->unscaled_special; an increment <= 0; a plane whose last column has
 * ((n - 1) * xInc) >> 16 > w - 1 (n its output width, w its source width: an extreme upscale, n * n above roughly w << 17, where the reference reads
 * two or more samples behind the line); (n - 1) * xInc not fitting 32 bits; a dst_format, range or dst_depth the twin refuses; vertical banks the
 * twin's tiles cannot hold.
 * Read extent, in bytes as in the paragraph above mi355_sws_frame: the reference has no tail fix-up — a column with xx == w - 1 reads src[w], the byte
 * BEHIND the line as it lies in the caller's plane (padding, the next line's first byte, or the byte behind the plane), and with a != 0 that byte is
 * part of the result.  So the caller keeps ONE byte behind srcW of every luma line and behind chrSrcW of every chroma line readable, the last line
 * included, and the device reads it — never more, and only on a line of a plane whose last column has xx == w - 1.  The Tier-1 host entry points copy
 * that byte of every line along.  A plane whose pointer and stride are multiples of 16 is fetched in aligned 16-byte pieces over its stride, as
 * everywhere else; one on 4-byte multiples in dwords that lie whole inside the bytes the reference reads; any other byte by byte. */
mi355_sws_ctx *mi355_sws_create_fast_bilinear(const mi355_sws_desc *desc, const mi355_sws_src *src, int dst_format, int range, int dst_depth,
                                              int lumXInc, int chrXInc);
int mi355_sws_fast_bilinear(const mi355_sws_ctx *ctx, int *lumXInc, int *chrXInc);   /* 1 / 0 (the increments: 0 then), -1 bad argument; either pointer may be NULL */

/* ---- planar RGB destinations: gbrp (AV_PIX_FMT_GBRP, three planes of bytes: G, B, R) ----
 * The one destination that runs the reference's ARITHMETIC yuv -> rgb path, yuv2gbrp_full_X_c (output.c:1275-1355, c->yuv2anyX reached at
 * swscale.c:683-689).  The reference forces SWS_FULL_CHR_H_INT for it (utils.c:986-994): chrDstHSubSample = chrDstVSubSample = 0, so chroma is filtered
 * horizontally to the full width and the chroma bank is indexed by dstY; no LUT is read, there is no dither (whatever the source's depth) and no range
 * step here (this version of the reference sets its range converters, swscale.c:748-766, for a gbrp destination whose range differs from the
 * source's — its isAnyRGB() does not know planar RGB — in front of coefficients that already carry the range: such a context is not created here,
 * the binding declines it) — range and colourspace live in six integers, c->yuv2rgb_y_offset, _y_coeff, _v2r_coeff, _v2g_coeff, _u2g_coeff,
 * _u2b_coeff AS THE REFERENCE'S INIT LEFT THEM (yuv2rgb.c:735-740; sws_setColorspaceDetails changes them): the binding hands them over, nothing here
 * recomputes them.  The vertical form is always the X form, also with one tap.  Per pixel, in 32 bits:
 *   Y = (1 << 9) + sum lum[j][i] * lumFilter[j];   U, V = (1 << 9) - (128 << 19) + sum chr[j][i] * chrFilter[j];   Y >>= 10; U >>= 10; V >>= 10
 *   Y = (Y - y_offset) * y_coeff + (1 << 21);   R = Y + V * v2r;   G = Y + V * v2g + U * u2g;   B = Y + U * u2b
 *   if ((R | G | B) & 0xC0000000) each = av_clip_uintp2(each, 30);   dst[0] = G >> 22, dst[1] = B >> 22, dst[2] = R >> 22
 * The three sums are computed modulo 2^32, as the reference's compiled code computes them: on content the format allows they leave int32 (BT.601
 * limited range, Y = 255 with U = 255: B near 2.24e9) and wrap, and the clip reads the wrapped bits.
 * Source: every layout — MI355_SWS_SRC_PLANAR at 8 / 9 / 10 bits and 4:2:0 / 4:2:2 / 4:4:4, NV12 / NV21, rgb24 / bgr24, the four 32-bit orders, the three
 * packed 4:2:2 orders, P010 — each with its own read extents and alignment rules, unchanged.
 * Descriptor: the reference's for that context: chrDstW = dstW, vChr.n = dstH.  desc->luts is not read.
 * Twin rule: the twin is mi355_sws_create_src_layout_range_depth(desc, src, src_layout, MI355_SWS_DST_YUV444P, MI355_SWS_RANGE_NONE, 8).  A gbrp context
 * has the twin's banks, plan (MI355_SWS_K_PLANAR_A .. C by lum_lines / chr_lines), th, narrow / hstage / hstaged report and refusals: it is refused
 * exactly where the twin's tiles cannot hold the lines (and where the twin refuses the source).  It is never a packer, a splitter or IDENT1_*: at
 * equal size the reference has no special converter from a YUV source to gbrp (ff_yuv2rgb_get_func_ptr has no such case) and runs its scaler with
 * one-tap banks; from an 8-bit packed RGB source at equal size it takes rgbToPlanarRgbWrapper (swscale_unscaled.c:1090-1092), which stays the
 * reference's.
 * Also NULL and a message for: desc->unscaled_special; coefs == NULL; a coefficient of magnitude 2^23 or more or a y_offset of 2^22 or more (the device
 * multiplies 24-bit operands; the reference's are int16 coefficients and a y_offset below 2^16).  The other operand needs no rule of its own, whatever
 * the vertical banks: a tap sum is an int32 (the reference's too; banks whose sums leave int32 overflow there as here), so a sum >> 10 lies inside
 * +-2^21 and Y - y_offset inside +-(2^21 + 2^22) — both fit 24 signed bits, and the 24-bit product's low 32 bits are the 32-bit product's.  There is no alpha: the creator has no such argument,
 * mi355_sws_alpha is 0, a 32-bit source's alpha byte is dropped as the reference drops it, and gbrap stays the reference's.
 * Frames are mi355_sws_planar_frame through mi355_sws_scale_planar_frames_dev / mi355_sws_scale_planar with dst[0..2] = G, B, R: exactly dstW bytes of
 * each of the dstH rows of each plane are written, a destination plane needs no alignment (rows on 8-byte multiples are stored eight bytes at a time).
 * mi355_sws_destination reports format MI355_SWS_DST_GBRP, 3 planes, chr_bytes = dstW, chr_rows = dstH; mi355_sws_range is 0, mi355_sws_dest_depth 8.
 * Not taken (the reference's): gbrp of 9 / 10 / 12 / 16 bits, gbrap, gbrp SOURCES, SWS_FULL_CHR_H_INT to the packed RGB destinations, and
 * SWS_FAST_BILINEAR contexts to gbrp (mi355_sws_create_fast_bilinear refuses the format). */
enum { MI355_SWS_DST_GBRP = 64 };
typedef struct mi355_sws_rgb_coefs { int y_offset, y_coeff, v2r, v2g, u2g, u2b; } mi355_sws_rgb_coefs;
mi355_sws_ctx *mi355_sws_create_gbrp(const mi355_sws_desc *desc, const mi355_sws_src *src, int src_layout, const mi355_sws_rgb_coefs *coefs);
int mi355_sws_rgb_coefs_of(const mi355_sws_ctx *ctx, mi355_sws_rgb_coefs *coefs);   /* 1: a gbrp context (*coefs: its six) / 0 (*coefs: zeros), -1 bad argument; coefs may be NULL */

/* ---- the individual inner loops (Tier 1, host pointers), argument lists of the reference's
 * function-pointer types minus the SwsContext ------------------------------------------------ */
/* hScale8To15_c swscale.c:133-147 (c->hyScale / c->hcScale) */
void mi355_sws_hscale8to15(int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter,
                           const int32_t *filterPos, int filterSize);
/* hScale16To15_c swscale.c:110-130: uint16_t samples below 1 << depth (9 ... 15), the shift behind the sum is depth - 1 */
void mi355_sws_hscale16to15(int16_t *dst, int dstW, const uint8_t *src, const int16_t *filter,
                            const int32_t *filterPos, int filterSize, int depth);
/* rgb24ToY_c / bgr24ToY_c input.c:539-593 (c->lumToYV12): `width` samples from 3 * width bytes; bgr: the pixels are B G R */
void mi355_sws_rgb24ToY(uint8_t *dst, const uint8_t *src, int width, int bgr);
/* rgb24ToUV_c / bgr24ToUV_c and their _half forms input.c:552-623 (c->chrToYV12): `width` OUTPUT samples of each plane; half 0 reads
 * 3 * width bytes, half 1 (each sample from the sum of two neighbouring pixels) 6 * width */
void mi355_sws_rgb24ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int bgr, int half);
/* the same three converters of a 32-bit source and its alpha reader (rgb32ToY_c ... bgr321ToUV_half_c input.c:288-291; rgbaToA_c / abgrToA_c
 * :305-319): layout MI355_SWS_SRC_RGBA ... _ABGR (any other value does nothing); `width` OUTPUT samples from 4 * width bytes, 8 * width with half 1;
 * src is a multiple of 4 (the reference reads dwords) */
void mi355_sws_rgb32ToY(uint8_t *dst, const uint8_t *src, int width, int layout);
void mi355_sws_rgb32ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int layout, int half);
void mi355_sws_rgb32ToA(uint8_t *dst, const uint8_t *src, int width, int layout);
/* yuy2ToY_c / uyvyToY_c and yuy2ToUV_c / yvy2ToUV_c / uyvyToUV_c input.c:369-473 (c->lumToYV12 / c->chrToYV12 of a packed 4:2:2 source): layout
 * MI355_SWS_SRC_YUYV422 ... _YVYU422 (any other value does nothing); `width` OUTPUT samples — ToY reads 2 * width bytes, ToUV 4 * width */
void mi355_sws_yuy2ToY(uint8_t *dst, const uint8_t *src, int width, int layout);
void mi355_sws_yuy2ToUV(uint8_t *dstU, uint8_t *dstV, const uint8_t *src, int width, int layout);
/* p010LEToY_c / p010LEToUV_c input.c:499-524 (c->lumToYV12 / c->chrToYV12 of a p010le source): `width` OUTPUT samples, host-order uint16_t, each the
 * little-endian source word >> 6; ToY reads 2 * width bytes, ToUV 4 * width (U from the first, V from the second word of a pair); host pointers at any
 * address */
void mi355_sws_p010ToY(uint16_t *dst, const uint8_t *src, int width);
void mi355_sws_p010ToUV(uint16_t *dstU, uint16_t *dstV, const uint8_t *src, int width);
/* hyscale_fast_c / hcscale_fast_c swscale.c:238-249, :288-301 (c->hyscale_fast / c->hcscale_fast): `dstWidth` int16 samples of each plane by the two
 * formulas above mi355_sws_create_fast_bilinear.  Like the reference's loops they read ((dstWidth - 1) * xInc >> 16) + 2 bytes of each source line,
 * whatever srcW says (srcW is not looked at); nothing is done for dstWidth <= 0, xInc <= 0 or a last position that does not fit 32 bits */
void mi355_sws_hyscale_fast(int16_t *dst, int dstWidth, const uint8_t *src, int srcW, int xInc);
void mi355_sws_hcscale_fast(int16_t *dst1, int16_t *dst2, int dstWidth, const uint8_t *src1, const uint8_t *src2, int srcW, int xInc);
/* yuv2gbrp_full_X_c output.c:1275-1355 (c->yuv2anyX of an 8-bit gbrp destination without alpha): `dstW` bytes to each of dest[0] = G, dest[1] = B,
 * dest[2] = R by the formula above mi355_sws_create_gbrp; nothing is done for dstW <= 0, a filter size below 1 or a NULL argument */
void mi355_sws_yuv2gbrp_full_X(const mi355_sws_rgb_coefs *coefs, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize,
                               const int16_t *chrFilter, const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize,
                               uint8_t *const dest[3], int dstW);
/* lumRangeFromJpeg_c / lumRangeToJpeg_c and chrRangeFromJpeg_c / chrRangeToJpeg_c swscale.c:168-198 (c->lumConvertRange / c->chrConvertRange):
 * `width` int16 samples converted in place, any int16 value (a result outside int16 is stored truncated, as the reference stores it) */
void mi355_sws_lumConvertRange(int16_t *dst, int width, int to_jpeg);
void mi355_sws_chrConvertRange(int16_t *dstU, int16_t *dstV, int width, int to_jpeg);
/* yuv2planeX_8_c output.c:242-255, yuv2plane1_8_c :257-266 */
void mi355_sws_yuv2planeX_8(const int16_t *filter, int filterSize, const int16_t **src, uint8_t *dest, int dstW,
                            const uint8_t *dither, int offset);
void mi355_sws_yuv2plane1_8(const int16_t *src, uint8_t *dest, int dstW, const uint8_t *dither, int offset);
/* yuv2planeX_9LE_c / _10LE_c and yuv2plane1_9LE_c / _10LE_c output.c:183-236: the reference's arguments minus the dither, which it ignores, plus
 * `bits` (9 or 10; anything else does nothing); dstW little-endian uint16_t samples */
void mi355_sws_yuv2planeX_nbps(const int16_t *filter, int filterSize, const int16_t **src, uint16_t *dest, int dstW, int bits);
void mi355_sws_yuv2plane1_nbps(const int16_t *src, uint16_t *dest, int dstW, int bits);
/* yuv2nv12cX_c output.c:267-301 with the two context fields it reads spelled out: c->chrDither8 and (c->dstFormat == AV_PIX_FMT_NV21) */
void mi355_sws_yuv2nv12cX(const int16_t *chrFilter, int chrFilterSize, const int16_t **chrUSrc, const int16_t **chrVSrc, uint8_t *dest, int chrDstW,
                          const uint8_t *chrDither, int swap_uv);
/* yuv2rgb24_X_c / _2_c / _1_c  output.c:937-1110 with target AV_PIX_FMT_RGB24, no alpha */
void mi355_sws_yuv2rgb24_X(const mi355_sws_luts *luts, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize,
                           const int16_t *chrFilter, const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize,
                           uint8_t *dest, int dstW);
void mi355_sws_yuv2rgb24_2(const mi355_sws_luts *luts, const int16_t *buf[2], const int16_t *ubuf[2], const int16_t *vbuf[2],
                           uint8_t *dest, int dstW, int yalpha, int uvalpha);
void mi355_sws_yuv2rgb24_1(const mi355_sws_luts *luts, const int16_t *buf0, const int16_t *ubuf[2], const int16_t *vbuf[2],
                           uint8_t *dest, int dstW, int uvalpha);
/* yuv2rgb_c_24_rgb yuv2rgb.c:335-363 (SwsFunc slice interface; returns srcSliceH) */
int mi355_sws_yuv2rgb_c_24_rgb(const mi355_sws_luts *luts, int dstW, const uint8_t *const src[3], const int srcStride[3],
                               int srcSliceY, int srcSliceH, uint8_t *dst, int dstStride);
/* the same trio and slice converter for any packed destination: dst_format 0 (rgb24: the bytes of the four entries above) or
 * MI355_SWS_DST_BGR24 ... _ABGR (yuv2bgr24_X_c ..., yuv2rgba32_X_c ... and their _2 / _1 forms; yuv2rgb_c_24_bgr yuv2rgb.c:366-394, yuv2rgb_c_32
 * :237-265); any other value does nothing (the slice entry returns -1).  dest holds (dstW + 1) >> 1 pairs — 6 bytes each, 8 for a 32-bit order —
 * as the reference's loops write them; luts in the form the creators take.
 * MI355_SWS_DST_YUYV422 / _UYVY422 / _YVYU422 (yuv2yuyv422_X_c ..., output.c:451-582): dest receives (dstW + 1) >> 1 groups of 4 bytes, luts is not
 * read and may be NULL; the slice entry returns -1 for these values */
void mi355_sws_yuv2packed_X(const mi355_sws_luts *luts, int dst_format, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize,
                            const int16_t *chrFilter, const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize,
                            uint8_t *dest, int dstW);
void mi355_sws_yuv2packed_2(const mi355_sws_luts *luts, int dst_format, const int16_t *buf[2], const int16_t *ubuf[2], const int16_t *vbuf[2],
                            uint8_t *dest, int dstW, int yalpha, int uvalpha);
void mi355_sws_yuv2packed_1(const mi355_sws_luts *luts, int dst_format, const int16_t *buf0, const int16_t *ubuf[2], const int16_t *vbuf[2],
                            uint8_t *dest, int dstW, int uvalpha);
int mi355_sws_yuv2rgb_c(const mi355_sws_luts *luts, int dst_format, int dstW, const uint8_t *const src[3], const int srcStride[3],
                        int srcSliceY, int srcSliceH, uint8_t *dst, int dstStride);
/* the alpha forms of the trio (yuv2rgba32_X_c ... yuv2rgbx32_1_1_c with hasAlpha, output.c:937-1110): dst_format MI355_SWS_DST_RGBA ... _ABGR only
 * (any other value, or no alpha line, does nothing); alpSrc / abuf / abuf0 are the alpha lines beside the luma lines — as many, as long, filtered
 * with the luma taps; luts as the creators take them (the alpha lane is not in them) */
void mi355_sws_yuv2packed_X_a(const mi355_sws_luts *luts, int dst_format, const int16_t *lumFilter, const int16_t **lumSrc, int lumFilterSize,
                              const int16_t *chrFilter, const int16_t **chrUSrc, const int16_t **chrVSrc, int chrFilterSize,
                              const int16_t **alpSrc, uint8_t *dest, int dstW);
void mi355_sws_yuv2packed_2_a(const mi355_sws_luts *luts, int dst_format, const int16_t *buf[2], const int16_t *ubuf[2], const int16_t *vbuf[2],
                              const int16_t *abuf[2], uint8_t *dest, int dstW, int yalpha, int uvalpha);
void mi355_sws_yuv2packed_1_a(const mi355_sws_luts *luts, int dst_format, const int16_t *buf0, const int16_t *ubuf[2], const int16_t *vbuf[2],
                              const int16_t *abuf0, uint8_t *dest, int dstW, int uvalpha);

#ifdef __cplusplus
}
#endif
#endif
