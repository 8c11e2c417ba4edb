"""Packed destinations of the device swscale path beside rgb24 (include/mi355_sws.h: MI355_SWS_DST_BGR24 / _RGBA / _BGRA / _ARGB / _ABGR through
mi355_sws_create_src_layout_range_depth — bgr24 and the four 32-bit orders), from every source the rgb24 destination takes (8 / 9 / 10-bit planar,
NV12 / NV21, packed rgb24 / bgr24), the unscaled special converter to them, and the Tier-1 line entries mi355_sws_yuv2packed_X / _2 / _1 and
mi355_sws_yuv2rgb_c.

A named table of contexts in the style of tests/sws_deepdst.py, captured from the reference's own libswscale (oracle/_ref/libswsref.so) and the
binding's mi355_sws_describe_packed, committed as data (tests/golden/sws_packeddst_contexts.npz: the format of sws_nvsrc_contexts.npz; regenerated
by running this file).  Every picture comparison is byte equality with the reference's own sws_scale() of the same buffers over the dstW pixels
of every row — 3 * dstW or 4 * dstW bytes; no byte outside them may change.  (The reference's pair loops also write a partner of an odd width's
last pixel, from a line-buffer sample it never initialised: like the rgb24 path the device does not write it, and the reference's own picture is
taken into a plane with room for it.)"""
import ctypes as C
import os

import numpy as np

import sws_deepdst as D
import sws_nvsrc as V
import sws_planar as P
import sws_range as G
import sws_sources as X
import sws_support as S

REF_LIB, REF_GPU_LIB, REF_TIER1_LIB = X.REF_LIB, X.REF_GPU_LIB, X.REF_TIER1_LIB
CONTEXTS = os.path.join(P.GOLDEN, "sws_packeddst_contexts.npz")
DESCRIBER = "mi355_sws_describe_packed"
CREATOR = "mi355_sws_create_src_layout_range_depth"

LAYOUTS = G.LAYOUTS                                           # MI355_SWS_SRC_* (planar: 0)
DSTS = {"bgr24": 32, "rgba": 33, "bgra": 34, "argb": 35, "abgr": 36}      # MI355_SWS_DST_*: the names give the byte order in memory
KERNELS = V.KERNELS
# where the bytes R, G, B of a pixel lie, and the alpha byte (None: three bytes a pixel)
ORDER = {"rgb24": (0, 1, 2, None), "bgr24": (2, 1, 0, None), "rgba": (0, 1, 2, 3), "bgra": (2, 1, 0, 3), "argb": (1, 2, 3, 0), "abgr": (3, 2, 1, 0)}

# name: (srcW, srcH, dstW, dstH, source, destination, bicubic, accurate_rnd, bitexact)
SHAPES = {
    # 2:1 down from an 8-bit planar source to each of the five: 8 taps, staged spans, the X template, narrow tiles
    "d2_420_bgr24": (128, 96, 64, 48, "yuv420p", "bgr24", 1, 1, 1),
    "d2_420_rgba": (128, 96, 64, 48, "yuv420p", "rgba", 1, 1, 1),
    "d2_420_bgra": (128, 96, 64, 48, "yuv420p", "bgra", 1, 1, 1),
    "d2_420_argb": (128, 96, 64, 48, "yuv420p", "argb", 1, 1, 1),
    "d2_420_abgr": (128, 96, 64, 48, "yuv420p", "abgr", 1, 1, 1),
    # ... and from each other source kind to bgr24 and to one 32-bit order
    "d2_420d10_bgr24": (128, 96, 64, 48, "yuv420p10le", "bgr24", 1, 1, 1),
    "d2_420d10_argb": (128, 96, 64, 48, "yuv420p10le", "argb", 1, 1, 1),
    "d2_444_bgr24": (128, 96, 64, 48, "yuv444p", "bgr24", 1, 1, 1),
    "d2_444_rgba": (128, 96, 64, 48, "yuv444p", "rgba", 1, 1, 1),
    "d2_nv12_bgr24": (128, 96, 64, 48, "nv12", "bgr24", 1, 1, 1),
    "d2_nv12_bgra": (128, 96, 64, 48, "nv12", "bgra", 1, 1, 1),
    "d2_nv21_bgr24": (128, 96, 64, 48, "nv21", "bgr24", 1, 1, 1),
    "d2_nv21_abgr": (128, 96, 64, 48, "nv21", "abgr", 1, 1, 1),
    "d2_rgb_bgr24": (128, 96, 64, 48, "rgb24", "bgr24", 1, 1, 1),                         # the halving converter
    "d2_rgb_rgba": (128, 96, 64, 48, "rgb24", "rgba", 1, 1, 1),
    # an upscale to 129 x 45: a full tile (the wide store) and a second tile of one column; the full converter of a packed source
    "up_bgr_bgr24_w129": (100, 30, 129, 45, "bgr24", "bgr24", 1, 1, 1),
    "up_bgr_argb_w129": (100, 30, 129, 45, "bgr24", "argb", 1, 1, 1),
    "up_420_bgra_w129": (100, 30, 129, 45, "yuv420p", "bgra", 1, 1, 1),
    "up_420_rgba_w129_bilinear": (100, 30, 129, 45, "yuv420p", "rgba", 0, 1, 1),          # two taps each: the _2 template
    "up_422d9_bgr24_w129_bilinear": (100, 30, 129, 45, "yuv422p9le", "bgr24", 0, 1, 1),
    # 4:1 horizontally: the span of a tile exceeds a staged line (direct form); dstW 128: one full tile, 130: a second tile of two columns
    "h4_420_abgr_w128": (512, 24, 128, 24, "yuv420p", "abgr", 1, 1, 1),
    "h4_nv12_bgr24_w130": (520, 24, 130, 24, "nv12", "bgr24", 1, 1, 1),
    "h4_420_rgba_w130": (520, 24, 130, 24, "yuv420p", "rgba", 1, 1, 1),
    # dstW 127: every tile partial
    "w127_444d10_bgra": (200, 40, 127, 40, "yuv444p10le", "bgra", 1, 1, 1),
    "w127_420_bgr24": (200, 40, 127, 40, "yuv420p", "bgr24", 1, 1, 1),
    # odd everything; one output row
    "odd_420_argb": (33, 17, 97, 61, "yuv420p", "argb", 1, 1, 1),
    "odd_nv21_bgr24": (33, 17, 97, 61, "nv21", "bgr24", 1, 1, 1),
    "h1_420_bgra": (100, 9, 70, 1, "yuv420p", "bgra", 1, 1, 1),
    # equal size through the generic scaler (SWS_ACCURATE_RND keeps it off the special converter).  An odd width stays with the tile kernel: one
    # luma tap with two chroma taps (bilinear: uvalpha 1024 and 3072 on alternate rows, both branches of the _1 template) or with one (4:2:2)
    "e_420_bgra_w127_bilinear": (127, 17, 127, 17, "yuv420p", "bgra", 0, 1, 1),
    "e_422_bgr24_w127": (127, 17, 127, 17, "yuv422p", "bgr24", 1, 1, 1),
    # ... an even one takes k_sws_ident1: up to two chroma taps (IDENT1_1), four (IDENT1_X); from planes and from pairs
    "i1_422_bgr24": (72, 40, 72, 40, "yuv422p", "bgr24", 0, 1, 1),
    "i1_420_rgba_bilinear": (64, 48, 64, 48, "yuv420p", "rgba", 0, 1, 1),
    "i1_nv12_abgr_w126": (126, 31, 126, 31, "nv12", "abgr", 0, 1, 1),
    "ix_420_bgr24": (64, 48, 64, 48, "yuv420p", "bgr24", 1, 1, 1),
    "ix_nv21_argb_w128": (128, 33, 128, 33, "nv21", "argb", 1, 1, 1),
    # vertical reductions: the instances A / B / C of the tile kernel, banks of more than eight taps (the narrow form, taps from memory)
    "v2_420_bgra": (64, 128, 64, 64, "yuv420p", "bgra", 1, 1, 1),
    "v4_420_bgr24": (64, 192, 64, 48, "yuv420p", "bgr24", 1, 1, 1),
    "v8_nv12_rgba": (64, 384, 64, 48, "nv12", "rgba", 1, 1, 1),
    "v12_420d9_argb": (64, 576, 64, 48, "yuv420p9le", "argb", 1, 1, 1),
    # the unscaled special converter (yuv2rgb_c_24_bgr / yuv2rgb_c_32): 4:2:0 to three of the five, 4:2:2, a width off the eight-sample groups
    "k_420_bgr24": (64, 48, 64, 48, "yuv420p", "bgr24", 1, 0, 0),
    "k_420_rgba": (64, 48, 64, 48, "yuv420p", "rgba", 1, 0, 0),
    "k_420_argb": (64, 48, 64, 48, "yuv420p", "argb", 1, 0, 0),
    "k_422_bgra_w70": (70, 50, 70, 50, "yuv422p", "bgra", 1, 0, 0),
    # the twin of sws_sources' r420d10_vdown16: the lines of one output row do not fit a tile — refused
    "v16_420d10_bgra": (64, 512, 64, 32, "yuv420p10le", "bgra", 1, 1, 1),
}
NAMES = list(SHAPES)
# the creator returns NULL: a context to one of the five has its rgb24 twin's banks and is refused exactly where the twin is
REFUSED = {"v16_420d10_bgra"}
REFUSED_CAP = X.REFUSED_CAP
SPECIAL = {n for n, c in SHAPES.items() if n.startswith("k_")}


def cfg(name):
    """the row of a name; a row itself passes through (tools/bench_sws.py --packeddst hands over its full-size rows that way)"""
    return name if isinstance(name, tuple) else SHAPES[name]


def bpp(name):
    return 3 if cfg(name)[5] in ("bgr24", "rgb24") else 4


def grow(name):
    """the row in the form of sws_range's table (no range): its helpers for sources and pictures take it as it is"""
    sw, sh, dw, dh, src, dst, bic, acc, bitexact = cfg(name)
    return (sw, sh, dw, dh, src, 0, dst, 0, bic, acc, bitexact)


def src_kind(name):
    return G.src_kind(grow(name))


class Entry(V.Entry):
    """as sws_nvsrc.Entry (a context, its source record with its layout, its destination: one of DSTS, or 0 for the rgb24 twin)"""

    @staticmethod
    def of(e):
        return Entry(e.ctx, e.depth, e.hsub, e.vsub, e.dither, e.fmt, e.layout)

    @staticmethod
    def from_arrays(z, prefix):
        return Entry.of(V.Entry.from_arrays(z, prefix))

    def edited(self, **kw):
        return Entry.of(super().edited(**kw))

    def out_sizes(self):
        """(BYTES per row, rows) of the one destination plane"""
        d = self.ctx.desc
        return [(d.dstW * (4 if self.fmt >= 33 else 3), d.dstH)]


def make_fresh(target):
    """as sws_deepdst.make_fresh, for a library linked before the glue had mi355_sws_describe_packed"""
    import subprocess
    path = D.make_fresh(target)
    if not P.exports(path, DESCRIBER):
        subprocess.run(["make", "-s", "-C", os.path.join(X.ROOT, "oracle"), "-W", "../contrib/libav/mi355_sws_glue.c", target], check=True)
    return path


# ---- the reference's libswscale ----------------------------------------------------------------------------------------------
class Ref(D.Ref):
    def __init__(self, lib):
        super().__init__(lib)
        if hasattr(lib, DESCRIBER):
            lib.mi355_sws_describe_packed.argtypes = [C.c_void_p] * 5

    def flags(self, name):
        return self.lib.ref_sws_flags_word(*cfg(name)[6:9])

    def open(self, name, more=0):
        sw, sh, dw, dh, src, dst = cfg(name)[:6]
        return self.open_formats(sw, sh, src.encode(), dw, dh, dst.encode(), self.flags(name) | more)

    def open_twin(self, name):
        """the context of the same source, sizes and flags to rgb24"""
        sw, sh, dw, dh, src, _ = cfg(name)[:6]
        return self.open_formats(sw, sh, src.encode(), dw, dh, b"rgb24", self.flags(name))

    def describe_packed(self, c):
        """the Entry of a live context through mi355_sws_describe_packed, None where the binding declines it"""
        d, s, lay, f = S.Desc(), X.Src(), C.c_int(-1), C.c_int(-1)
        if self.lib.mi355_sws_describe_packed(c, C.byref(d), C.byref(s), C.byref(lay), C.byref(f)) != 0:
            return None
        return Entry(S.Context.from_desc(d), s.depth, s.hsub, s.vsub, np.array(list(s.dither), np.uint8), f.value, lay.value)

    def describe(self, c):
        return self.describe_packed(c)

    def declined_by_the_six_describers(self, c):
        """mi355_sws_describe / _planar / _src / _fmt / _range / _depth all decline the context"""
        return self.declined_by_the_five_describers(c) and self.describe_depth(c) is None

    def entry(self, name):
        c = self.open(name)
        e = self.describe_packed(c)
        self.free(c)
        _, depth, (hsub, vsub) = src_kind(name)
        assert e is not None, name
        assert (e.depth, e.hsub, e.vsub, e.layout, e.fmt) == (depth, hsub, vsub, LAYOUTS.get(cfg(name)[4], 0), DSTS[cfg(name)[5]]), (name, e.hsub, e.layout, e.fmt)
        assert bool(e.ctx.desc.unscaled_special) == (name in SPECIAL), name
        return e

    def twin_entry(self, name):
        """the rgb24 context of the same source, sizes and flags through mi355_sws_describe_fmt"""
        c = self.open_twin(name)
        e = self.describe_fmt(c)
        self.free(c)
        return e


def stored_entry(name):
    """the entry as committed in tests/golden/sws_packeddst_contexts.npz"""
    with np.load(CONTEXTS) as z:
        return Entry.from_arrays(z, name)


def write_contexts_golden(ref):
    arrays = {}
    for name in SHAPES:
        arrays.update(ref.entry(name).arrays(name))
    np.savez_compressed(CONTEXTS, **arrays)


# ---- pictures: sws_range's, of the row's source -------------------------------------------------------------------------------
PICTURES = G.PICTURES


def picture(name, what, seed=1, pad=0):
    return G.picture(grow(name), what, seed, pad)


def batch_pictures(name):
    """six frames: noise, the two-pixel checkerboard, the ramp, the noise again at other strides, all-0 and all-maximum planes"""
    return G.batch_pictures(grow(name))


def tier1_pictures(name, seed):
    return G.tier1_pictures(grow(name), seed)


# ---- the product ------------------------------------------------------------------------------------------------------------
def create(lib, e, range_=0, dst_depth=8):
    fn = getattr(lib, CREATOR)
    fn.restype = C.c_void_p
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    return fn(C.byref(e.ctx.desc), C.byref(e.src), e.layout, e.fmt, range_, dst_depth)


def plan_of(lib, handle):
    return D.plan_of(lib, handle)


def plan(lib, e):
    h = create(lib, e)
    try:
        return plan_of(lib, h)
    finally:
        if h:
            lib.mi355_sws_destroy(C.c_void_p(h))


differing_rows = X.differing_rows


def scale_tier1(lib, handle, e, planes, pad=8, skew=0):
    """mi355_sws_scale (host pointers) into a plane `pad` bytes wider than the picture and starting `skew` bytes into its buffer (0x5A); the
    return value is checked against the context's rows"""
    (w, h), = e.out_sizes()
    buf = np.full(h * (w + pad) + skew + 64, 0x5A, np.uint8)
    base = (-buf.ctypes.data) % 16 + skew                          # `skew` bytes past a 16-byte multiple
    out = buf[base:base + h * (w + pad)].reshape(h, w + pad)
    src = (C.c_void_p * 3)(*([p.ctypes.data for p in planes] + [None] * (3 - len(planes))))
    ss = (C.c_int * 3)(*([p.strides[0] for p in planes] + [0] * (3 - len(planes))))
    lib.mi355_sws_scale.restype = C.c_int
    lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    n = lib.mi355_sws_scale(C.c_void_p(handle), src, ss, C.c_void_p(out.ctypes.data), out.strides[0])
    assert n == (e.ctx.desc.srcH if e.ctx.desc.unscaled_special else e.ctx.desc.dstH), n
    return [out]


# where a destination row starts past a 16-byte boundary, per frame, and the line pads in PIXELS (sws_sources' pads): a 32-bit row lies on a
# 16-byte multiple (frames 0 and 2: the wide store in 16-byte pieces), or on a 4-byte multiple that is no multiple of 16 (narrow form, dwords);
# a 24-bit row also on an odd address (frame 1, whose line pad of five pixels puts its rows on every residue in turn; its 4-byte class is frame 2,
# whose pad of sixteen pixels keeps the stride a multiple of 16)
STARTS = {3: (0, 1, 4, 8), 4: (0, 4, 0, 12)}
DST_PADS = X.DST_PADS
GAPS = (64, 66, 72, 62)                                       # 0x5A bytes (at least) before the destination plane of each frame


def layout(sizes, n, bytes_pp):
    """[frame][0] = (byte offset, byte stride) and the end: the planes one after another, each a gap behind the last and STARTS bytes past a
    16-byte boundary"""
    out, off = [], 0
    (w, h), = sizes
    for f in range(n):
        off += GAPS[f % 4]
        off += (STARTS[bytes_pp][f % 4] - off) % 16
        st = w + DST_PADS[f % 4] * bytes_pp
        out.append([(off, st)])
        off += st * h
    return out, off


def store_class(off, stride):
    """what a row's alignment allows: 16 — 16-byte pieces, 8, 4, 1"""
    v = off | stride
    return 16 if v % 16 == 0 else (8 if v % 8 == 0 else (4 if v % 4 == 0 else 1))


class Batch(X.Batch):
    """as sws_range.Batch (one, two or three source planes per frame), ONE packed destination plane per frame laid out by layout() above in a
    256-byte aligned buffer: the alignment classes of layout() are those of the device addresses"""

    def __init__(self, lib, e, pictures, n, src_offs=X.SRC_OFFS):
        self.lib, self.e, self.bufs, self.n = lib, e, [], n
        lib.mi355_malloc.restype = C.c_void_p
        lib.mi355_malloc.argtypes = [C.c_size_t]
        lib.mi355_free.argtypes = [C.c_void_p]
        for f in ("mi355_memcpy_h2d", "mi355_memcpy_d2h"):
            getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        self.sizes = e.out_sizes()
        self.layout, off = layout(self.sizes, n, 4 if e.fmt >= 33 else 3)
        self.total = off + X.GUARD
        self.dst = (self.alloc(self.total + 256) + 255) & ~255
        fill = np.full(self.total, 0x5A, np.uint8)
        lib.mi355_memcpy_h2d(self.dst, fill.ctypes.data, fill.nbytes)
        del fill
        arr = (S.SwsFrame * n)()
        b = 1 if e.depth == 8 else 2
        for f, planes in zip(range(n), pictures):
            for p, plane in enumerate(planes):
                nb = plane.strides[0] * (plane.shape[0] - 1) + plane.shape[1] * b + (3 if e.layout >= 4 else 0)       # the spare line holds them
                o = src_offs[f % len(src_offs)] * b
                dev = self.alloc(nb + o + X.SLACK)
                lib.mi355_memcpy_h2d(dev + o, plane.ctypes.data, nb)
                arr[f].src[p], arr[f].src_stride[p] = dev + o, plane.strides[0]
            arr[f].dst, arr[f].dst_stride = self.dst + self.layout[f][0][0], self.layout[f][0][1]
        self.d_frames = self.alloc(C.sizeof(arr))
        lib.mi355_memcpy_h2d(self.d_frames, C.addressof(arr), C.sizeof(arr))

    def launch(self, handle, stream=None):
        fn = self.lib.mi355_sws_scale_frames_dev
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        return fn(C.c_void_p(handle), C.c_void_p(self.d_frames), self.n, C.c_void_p(stream))


def written(e):
    """(BYTES per row, rows) the context writes: the special converter takes whole pairs (dstW & ~1 pixels), the scaler dstW"""
    (w, h), = e.out_sizes()
    d = e.ctx.desc
    return [((d.dstW & ~1) * (w // d.dstW), h)] if d.unscaled_special else [(w, h)]


def check_batch(lib, ref, name, e=None):
    """one entry through mi355_sws_scale_frames_dev of `lib` on the six frames of batch_pictures(): every row equals the reference's sws_scale()
    of the same buffer into a 0x5A plane, no byte outside the written pixels changes.  Returns the plan, None where the creator refuses."""
    e = e or ref.entry(name)
    handle = create(lib, e)
    if not handle:
        return None
    try:
        p = plan_of(lib, handle)
        pics = batch_pictures(name)
        batch = Batch(lib, e, pics, len(pics))
        try:
            out = batch.run(handle)
            assert batch.untouched(out), (name, p, "bytes outside the plane changed")
            for f, planes in enumerate(pics):
                got = batch.frame(out, f)
                bad = differing_rows(got, ref.scale(name, planes, batch.sizes), batch.sizes)
                assert not any(bad), (name, p, f, "rows", bad)
                if e.fmt >= 33:                               # the alpha byte of every written pixel
                    a = ORDER[cfg(name)[5]][3]
                    ww = written(e)[0][0]
                    assert (got[0][:, a:ww:4] == 255).all(), (name, f)
        finally:
            batch.close()
    finally:
        lib.mi355_sws_destroy(C.c_void_p(handle))
    return p


def check_tier1(lib, ref, name, pictures, skew=0):
    """one entry through mi355_sws_scale of `lib` (host pointers) on each picture"""
    e = stored_entry(name)
    h = create(lib, e)
    assert h, name
    try:
        sizes = e.out_sizes()
        for planes in pictures:
            want = ref.scale(name, planes, sizes)
            got = scale_tier1(lib, h, e, planes, pad=8, skew=skew)
            assert not any(differing_rows(got, want, sizes)), name
            assert all((g[:, w:] == 0x5A).all() for g, (w, _) in zip(got, sizes)), name       # the caller's padding untouched
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))


# ---- the line entries: the rgb24 trio's bytes in the order of the format ----------------------------------------------------------------
def reorder(rgb, dst):
    """rgb24 pixels [n, 3] as the bytes of `dst` ([n, 3] or [n, 4], alpha 255)"""
    r, g, b, a = ORDER[dst]
    out = np.full((rgb.shape[0], 3 if a is None else 4), 255, np.uint8)
    out[:, r], out[:, g], out[:, b] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    return out


def check_line_entries(lib, luts):
    """mi355_sws_yuv2packed_X / _2 / _1 on noise lines: dst_format 0 gives the bytes of mi355_sws_yuv2rgb24_X / _2 / _1, each of the five formats
    those pixels in its byte order (alpha 255); whole pairs are written, nothing behind them; any other format writes nothing.  `luts`: the
    tables of a stored rgb24-shaped entry (S.Luts)"""
    from rng import SplitMix64
    r = SplitMix64(20261021)
    pp = C.c_void_p
    n = 0
    lt = C.byref(luts)
    for width in (1, 2, 7, 64, 129):
        npair = (width + 1) // 2
        for taps_l, taps_c in ((1, 1), (1, 2), (2, 2), (4, 4), (11, 6)):
            lum = r.randint(0, 32767, (taps_l, 2 * npair)).astype(np.int16)
            cu = r.randint(0, 32767, (taps_c, npair)).astype(np.int16)
            cv = r.randint(0, 32767, (taps_c, npair)).astype(np.int16)
            lf = np.array(D.BANKS.get(taps_l, [4096] if taps_l == 1 else None), np.int16)
            cf = np.array({1: [4096], 2: D.BANKS[2], 4: D.BANKS[4], 6: [-100, 600, 1548, 1548, 600, -100]}[taps_c], np.int16)
            lp = (pp * taps_l)(*[lum[j].ctypes.data for j in range(taps_l)])
            up = (pp * max(taps_c, 2))(*([cu[j].ctypes.data for j in range(taps_c)] + [cu[0].ctypes.data] * (2 - min(taps_c, 2))))
            vp = (pp * max(taps_c, 2))(*([cv[j].ctypes.data for j in range(taps_c)] + [cv[0].ctypes.data] * (2 - min(taps_c, 2))))

            def run(fmt, which):
                out = np.full(npair * 8 + 16, 0x5A, np.uint8)
                o = pp(out.ctypes.data)
                if which == "X":
                    if fmt is None:
                        lib.mi355_sws_yuv2rgb24_X(lt, pp(lf.ctypes.data), lp, taps_l, pp(cf.ctypes.data), up, vp, taps_c, o, width)
                    else:
                        lib.mi355_sws_yuv2packed_X(lt, fmt, pp(lf.ctypes.data), lp, taps_l, pp(cf.ctypes.data), up, vp, taps_c, o, width)
                elif which == "2":
                    if fmt is None:
                        lib.mi355_sws_yuv2rgb24_2(lt, lp, up, vp, o, width, 1365, 2731)
                    else:
                        lib.mi355_sws_yuv2packed_2(lt, fmt, lp, up, vp, o, width, 1365, 2731)
                else:
                    ua = 3072 if taps_c == 2 else 1024
                    if fmt is None:
                        lib.mi355_sws_yuv2rgb24_1(lt, pp(lum[0].ctypes.data), up, vp, o, width, ua)
                    else:
                        lib.mi355_sws_yuv2packed_1(lt, fmt, pp(lum[0].ctypes.data), up, vp, o, width, ua)
                return out

            which = "1" if taps_l == 1 else ("2" if (taps_l, taps_c) == (2, 2) else "X")
            old = run(None, which)
            assert (old[6 * npair:] == 0x5A).all()
            assert (run(0, which) == old).all(), (width, taps_l, taps_c)
            rgb = old[:6 * npair].reshape(-1, 3)
            for dst, fmt in DSTS.items():
                got = run(fmt, which)
                want = reorder(rgb, dst).reshape(-1)
                assert (got[:want.size] == want).all() and (got[want.size:] == 0x5A).all(), (dst, width, taps_l, taps_c)
                n += 1
            for fmt in (1, 16, 31, 37, -1):
                assert (run(fmt, which) == 0x5A).all(), fmt
    return n


def check_slice_entry(lib, ref, name):
    """mi355_sws_yuv2rgb_c on the two halves of a 4:2:0 picture of a special row equals the reference's sws_scale(); format 0 is
    mi355_sws_yuv2rgb_c_24_rgb"""
    e = stored_entry(name)
    d = e.ctx.desc
    planes = picture(name, "noise", seed=13, pad=3)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    (w, h), = sizes
    out = np.full((h, w + 8), 0x5A, np.uint8)
    fn = lib.mi355_sws_yuv2rgb_c
    fn.restype = C.c_int
    half = (h // 2) & ~1
    ss = (C.c_int * 3)(*[p.strides[0] for p in planes])
    for y0, rows in ((0, half), (half, h - half)):
        src = (C.c_void_p * 3)(planes[0][y0:].ctypes.data, planes[1][y0 // 2:].ctypes.data, planes[2][y0 // 2:].ctypes.data)
        assert fn(C.byref(e.ctx.desc.luts), e.fmt, d.dstW, src, ss, y0, rows, C.c_void_p(out.ctypes.data), out.strides[0]) == rows
    assert not any(differing_rows([out], want, written(e))), name
    assert (out[:, written(e)[0][0]:] == 0x5A).all(), name
    if e.fmt >= 33:
        src = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
        assert fn(C.byref(e.ctx.desc.luts), e.fmt, d.dstW, src, ss, 0, h, C.c_void_p(out.ctypes.data + 1), out.strides[0]) == -1
        assert fn(C.byref(e.ctx.desc.luts), e.fmt, d.dstW, src, ss, 0, h, C.c_void_p(out.ctypes.data), out.strides[0] + 2) == -1
    src = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    assert fn(C.byref(e.ctx.desc.luts), 37, d.dstW, src, ss, 0, h, C.c_void_p(out.ctypes.data), out.strides[0]) == -1


# the entries the binding tests run: bgr24 and 32 bits, a deeper, a semi-planar and a packed source, k_sws_ident1, the special converter, the
# refused one
BINDING = ["d2_420_bgr24", "d2_420d10_argb", "d2_nv12_bgra", "d2_rgb_rgba", "ix_420_bgr24", "k_420_rgba", "v16_420d10_bgra"]
TAKEN = [n for n in BINDING if n not in REFUSED]


if __name__ == "__main__":
    make_fresh("_ref/libswsref.so")
    write_contexts_golden(Ref(P.bind(REF_LIB)))
