"""A named table of swscale contexts (yuv420p -> rgb24) chosen to reach every kernel the device path of include/mi355_sws.h picks
(mi355_sws_plan: k_sws_c24, k_sws_ident1 in both forms, the three instances of k_sws_generic), every tile height, both forms of a
generic tile, unstaged horizontal filters and the contexts mi355_sws_create refuses — at widths and heights on the tiles' edges
(TW = 128 columns, C24_COLS = 512, 16-row tiles) and one off them.

The contexts are the reference's own: captured at run time from oracle/_ref/libswsref.so (sws_getContext + ref_sws_describe).
One entry is built from a captured one by editing its horizontal bank (SYNTH): the reference never makes it, the oracle is then the
only reference."""
import ctypes as C
import os

import numpy as np

import sws_support as S
from rng import SplitMix64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libswsref.so")
REF_GPU_LIB = os.path.join(ROOT, "oracle", "_ref", "libswsref_gpu.so")

# name: (srcW, srcH, dstW, dstH, bicubic, accurate_rnd, bitexact)
SHAPES = {
    # (the reference takes no source narrower than 4 and no destination narrower than 8: utils.c "invalid scaling dimension")
    # unscaled, no accurate rounding, even height: the special converter (k_sws_c24); every width residue mod 8 and the edges of its 512-column tiles
    "c24_w8": (8, 16, 8, 16, 1, 0, 0),
    "c24_w10": (10, 10, 10, 10, 1, 0, 0),
    "c24_w9": (9, 18, 9, 18, 1, 0, 0),
    "c24_w67": (67, 34, 67, 34, 1, 0, 0),
    "c24_w68": (68, 14, 68, 14, 0, 0, 0),
    "c24_w133": (133, 16, 133, 16, 1, 0, 0),
    "c24_w135": (135, 20, 135, 20, 1, 0, 0),
    "c24_w510": (510, 18, 510, 18, 1, 0, 0),
    "c24_w512": (512, 16, 512, 16, 1, 0, 0),
    "c24_w514": (514, 20, 514, 20, 1, 0, 0),
    "c24_w1026": (1026, 34, 1026, 34, 1, 0, 0),
    # ... an odd height is not the special converter's (swscale_unscaled.c: !(dstH & 1)): the generic scaler without scaling
    "noacc_h17": (64, 17, 64, 17, 1, 0, 0),
    "noacc_h33": (130, 33, 130, 33, 1, 0, 0),
    # unscaled with accurate rounding, even width: k_sws_ident1 (bilinear: two chroma taps, the _1 template; bicubic: four, the X template)
    "id1_w8_h17": (8, 17, 8, 17, 0, 1, 1),
    "idx_w10_h15": (10, 15, 10, 15, 1, 1, 1),
    "id1_w126_h31": (126, 31, 126, 31, 0, 1, 1),
    "idx_w128_h33": (128, 33, 128, 33, 1, 1, 1),
    "id1_w130_h47": (130, 47, 130, 47, 0, 1, 0),
    "id1_w510_h1": (510, 1, 510, 1, 1, 1, 1),          # bicubic, but one source line: one chroma tap
    "id1_w512_h15": (512, 15, 512, 15, 0, 1, 1),
    "idx_w514_h17": (514, 17, 514, 17, 1, 1, 0),
    # ... an odd width falls to k_sws_generic (the phantom partner of the last sample)
    "idodd_w127": (127, 17, 127, 17, 1, 1, 1),
    "idodd_w129": (129, 16, 129, 16, 0, 1, 1),
    "idodd_w511": (511, 15, 511, 15, 1, 1, 1),
    # generic: destinations narrower than a tile (the narrow form), one off a tile or two
    "g_w8": (40, 30, 8, 30, 1, 1, 1),
    "g_w13": (20, 16, 13, 11, 0, 1, 1),
    "g_w16": (16, 12, 16, 24, 1, 1, 1),
    "g_w127": (200, 40, 127, 40, 1, 1, 1),
    "g_w129": (100, 30, 129, 45, 1, 1, 1),
    "g_w255": (300, 20, 255, 20, 0, 1, 1),
    "g_w257": (128, 24, 257, 37, 1, 1, 1),
    # generic: one direction only
    "g_honly": (96, 40, 64, 40, 1, 1, 1),
    "g_vonly": (64, 96, 64, 40, 1, 1, 1),
    # generic: upscales 1:2, 1:3, 1:4 and odd to odd
    "g_up2": (48, 32, 96, 64, 0, 1, 1),
    "g_up3": (40, 20, 120, 60, 1, 1, 1),
    "g_up4": (32, 16, 128, 64, 1, 1, 1),
    "g_odd": (33, 17, 97, 61, 1, 1, 1),
    # generic: vertical downscales (the tile height shrinks, the source lines a tile needs pick the instance); 16:1 does not fit any
    "g_vdown2": (64, 128, 64, 64, 1, 1, 1),
    "g_vdown3": (64, 144, 64, 48, 1, 1, 1),
    "g_vdown4": (64, 192, 64, 48, 1, 1, 1),
    "g_vdown6": (64, 288, 64, 48, 1, 1, 1),
    "g_vdown8": (64, 384, 64, 48, 1, 1, 1),
    "g_vdown12": (64, 576, 64, 48, 1, 1, 1),
    "g_vdown16": (64, 512, 64, 32, 1, 1, 1),
    # generic: a single output row
    "g_h1": (100, 9, 70, 1, 1, 1, 1),
    # generic: the flags
    "g_flags_000": (80, 60, 56, 44, 0, 0, 0),
    "g_flags_101": (80, 60, 56, 44, 1, 0, 1),
    "g_flags_110": (80, 60, 56, 44, 1, 1, 0),
    # full-size odd shapes (device only)
    "big_1921": (1921, 1081, 1280, 721, 1, 1, 1),
    "big_3839": (3839, 2161, 1919, 1079, 1, 1, 1),
}
# built from a captured context: the last luma outputs' taps moved to cross the line's end (zero coefficients there) — unstaged horizontal pass
SYNTH = {"synth_hstage0": "g_honly"}
NAMES = list(SHAPES) + list(SYNTH)
BIG = {"big_1921", "big_3839"}
REFUSED = {"g_vdown16"}            # mi355_sws_create returns NULL: the glue leaves these to the reference
SMALL_PIXELS = 100_000


def cfg(name):
    return SHAPES[name if name in SHAPES else SYNTH[name]]


def bind(path):
    lib = C.CDLL(path)
    lib.sws_getContext.restype = C.c_void_p
    lib.sws_getContext.argtypes = [C.c_int] * 7 + [C.c_void_p] * 3
    lib.sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.sws_freeContext.argtypes = [C.c_void_p]
    lib.ref_sws_describe.argtypes = [C.c_void_p, C.c_void_p]
    return lib


class Ref:
    """sws_getContext / sws_scale / ref_sws_describe of one build of the reference's libswscale (a library loaded by bind() below or by
    test_sws_tier1_reference.bind())"""

    def __init__(self, lib):
        self.lib = lib
        lib.ref_sws_describe.argtypes = [C.c_void_p, C.c_void_p]
        # a library with the binding: its device side of the context goes with the context (--wrap=sws_freeContext)
        self.free = getattr(lib, "__wrap_sws_freeContext", lib.sws_freeContext)
        self.free.argtypes = [C.c_void_p]

    def open(self, name):
        sw, sh, dw, dh, bic, acc, bitexact = SHAPES[name]
        lib = self.lib
        c = lib.sws_getContext(sw, sh, lib.ref_pix_fmt(0), dw, dh, lib.ref_pix_fmt(1), lib.ref_sws_flags_word(bic, acc, bitexact), None, None, None)
        assert c, "the reference refuses %s %s" % (name, SHAPES[name])
        return c

    def context(self, name):
        c = self.open(name)
        d = S.Desc()
        assert self.lib.ref_sws_describe(c, C.byref(d)) == 0
        ctx = S.Context.from_desc(d)
        self.free(c)
        return ctx

    def scale(self, name, planes, dst_pad=8):
        sw, sh, dw, dh = SHAPES[name][:4]
        c = self.open(name)
        out = np.full((dh, dw * 3 + dst_pad), 0x5A, np.uint8)
        src = (C.c_void_p * 4)(*[p.ctypes.data for p in planes], None)
        strides = (C.c_int * 4)(*[p.strides[0] for p in planes], 0)
        dst = (C.c_void_p * 4)(out.ctypes.data, None, None, None)
        dstrides = (C.c_int * 4)(out.strides[0], 0, 0, 0)
        n = self.lib.sws_scale(c, src, strides, 0, sh, dst, dstrides)
        self.free(c)
        assert n == dh, (name, n)
        return out


def synth_hstage0(ctx):
    """the last quarter of the luma outputs (at least two) read from three samples before the line's end on: their taps past it carry zero"""
    ints = dict(ctx.ints)
    coef, pos = (a.copy() for a in ctx.banks["hLum"])
    n, fs, sw = len(pos), coef.size // len(pos), ints["srcW"]
    assert fs > 3
    coef = coef.reshape(n, fs)
    for i in range(n - max(2, n // 4), n):
        pos[i] = sw - 3
        coef[i, 3:] = 0
    banks = dict(ctx.banks)
    banks["hLum"] = (coef.reshape(-1), pos)
    return S.Context(ints, banks, ctx.luts)


def context(ref, name):
    if name in SYNTH:
        return synth_hstage0(ref.context(SYNTH[name]))
    return ref.context(name)


def out_pixels(name):
    sw, sh, dw, dh = cfg(name)[:4]
    return dw * dh


# ---- pictures -------------------------------------------------------------------------------------------------------------
def picture(name, seed, pad=0):
    """uniform random yuv420p planes, each line `pad` bytes longer than the plane (the bytes hold noise); every plane is a view into a buffer
    with one spare line behind it, so a tap that reaches a little past the last line's end reads memory that exists"""
    sw, sh = cfg(name)[:2]
    r = SplitMix64(seed * 7919 + sum(map(ord, name)))
    cw, ch = -(-sw // 2), -(-sh // 2)
    planes = []
    for w, h in ((sw, sh), (cw, ch), (cw, ch)):
        buf = r.u8((h + 1, w + pad))
        planes.append(buf[:h])
    return planes


def restride(planes, pad):
    """the same picture with lines `pad` bytes longer than the plane (and a spare line behind each plane, as picture() makes them)"""
    out = []
    for p in planes:
        h, w = p.shape
        buf = np.zeros((h + 1, w + pad), np.uint8)
        buf[:h, :w] = p
        out.append(buf[:h])
    return out


def oracle_scale(oracle, ctx, planes, dst_pad=8):
    d = ctx.desc
    out = np.full((d.dstH, d.dstW * 3 + dst_pad), 0x5A, np.uint8)
    src = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    strides = (C.c_int * 3)(*[p.strides[0] for p in planes])
    fn = oracle.lib.oracle_sws_scale
    fn.restype = C.c_int
    assert fn(C.byref(d), src, strides, C.c_void_p(out.ctypes.data), C.c_int(out.strides[0])) == d.dstH
    return out


# ---- the plan query --------------------------------------------------------------------------------------------------------
class PlanInfo(C.Structure):
    _fields_ = [("kernel", C.c_int), ("th", C.c_int), ("hstage", C.c_int), ("lum_lines", C.c_int), ("chr_lines", C.c_int), ("narrow", C.c_int)]


KERNELS = S.KERNELS[:6]            # what an rgb24 context of this table may report: c24 ... generic_c


def create(lib, ctx):
    lib.mi355_sws_create.restype = C.c_void_p
    lib.mi355_sws_create.argtypes = [C.c_void_p]
    return lib.mi355_sws_create(C.byref(ctx.desc))


def plan_of(lib, handle):
    """the plan of a created context as a dict; None for a context mi355_sws_create refused (handle NULL)"""
    if not handle:
        return None
    p = PlanInfo()
    lib.mi355_sws_plan.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.mi355_sws_plan(C.c_void_p(handle), C.byref(p)) == 0
    return {"kernel": S.KERNELS[p.kernel], "th": p.th, "hstage": p.hstage, "lum_lines": p.lum_lines, "chr_lines": p.chr_lines, "narrow": p.narrow}


def plan(lib, ctx):
    h = create(lib, ctx)
    try:
        return plan_of(lib, h)
    finally:
        if h:
            lib.mi355_sws_destroy(C.c_void_p(h))


# ---- Tier 2: a batch in device memory, guarded ------------------------------------------------------------------------------
SRC_PADS = (0, 3, 16, 7)          # line pads of the four frames' source planes: frame 3 is frame 0's picture again, at other strides
DST_PADS = (0, 5, 16, 2)          # ... and of their destinations
GAP, GUARD, SLACK = 64, 4096, 4096


def batch_pictures(name):
    pics = [picture(name, seed=s, pad=p) for s, p in zip((1, 2, 3), SRC_PADS)]
    return pics + [restride(pics[0], SRC_PADS[3])]


class Batch:
    """four frames in device memory: each plane its own allocation (+ SLACK behind it), the destinations one after another in one
    buffer with GAP bytes between them and GUARD bytes after the last, all 0x5A"""

    def __init__(self, lib, ctx, pictures):
        self.lib, self.ctx, self.bufs = lib, ctx, []
        lib.mi355_malloc.restype = C.c_void_p
        lib.mi355_malloc.argtypes = [C.c_size_t]
        lib.mi355_free.argtypes = [C.c_void_p]
        for f in ("mi355_memcpy_h2d", "mi355_memcpy_d2h"):
            getattr(lib, f).argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        d = ctx.desc
        self.rowb = d.dstW * 3
        self.dst_strides = [self.rowb + p for p in DST_PADS]
        self.offs, off = [], GAP
        for ds in self.dst_strides:
            self.offs.append(off)
            off += ds * d.dstH + GAP
        self.total = off + GUARD
        self.dst = self.alloc(self.total)
        fill = np.full(self.total, 0x5A, np.uint8)
        lib.mi355_memcpy_h2d(self.dst, fill.ctypes.data, fill.nbytes)
        arr = (S.SwsFrame * len(pictures))()
        for f, planes in enumerate(pictures):
            for p, plane in enumerate(planes):
                n = plane.strides[0] * (plane.shape[0] + 1)            # the plane and the spare line behind it (T.picture)
                dev = self.alloc(n + SLACK)
                lib.mi355_memcpy_h2d(dev, plane.ctypes.data, n)
                arr[f].src[p], arr[f].src_stride[p] = dev, plane.strides[0]
            arr[f].dst, arr[f].dst_stride = self.dst + self.offs[f], self.dst_strides[f]
        self.n = len(pictures)
        self.d_frames = self.alloc(C.sizeof(arr))
        lib.mi355_memcpy_h2d(self.d_frames, C.addressof(arr), C.sizeof(arr))

    def alloc(self, n):
        p = self.lib.mi355_malloc(n)
        assert p
        self.bufs.append(p)
        return p

    def run(self, handle):
        self.lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        assert self.lib.mi355_sws_scale_frames_dev(C.c_void_p(handle), C.c_void_p(self.d_frames), self.n, None) == 0
        self.lib.mi355_sync(None)
        out = np.empty(self.total, np.uint8)
        self.lib.mi355_memcpy_d2h(out.ctypes.data, self.dst, out.nbytes)
        return out

    def frame(self, out, f):
        d = self.ctx.desc
        return out[self.offs[f]:self.offs[f] + self.dst_strides[f] * d.dstH].reshape(d.dstH, self.dst_strides[f])

    def untouched(self, out):
        """every byte outside the frames' pictures still 0x5A"""
        mask = np.ones(self.total, bool)
        d = self.ctx.desc
        for f in range(self.n):
            rows = self.offs[f] + np.arange(d.dstH)[:, None] * self.dst_strides[f] + np.arange(self.rowb)[None, :]
            mask[rows.ravel()] = False
        return bool((out[mask] == 0x5A).all())

    def close(self):
        for p in self.bufs:
            self.lib.mi355_free(p)
        self.bufs = []


def check_batch(lib, oracle, ref, name):
    """one entry through mi355_sws_scale_frames_dev of `lib` on the four frames of batch_pictures(): every row's first dstW * 3 bytes equal the
    oracle and (a context of the reference's) the reference's own sws_scale(), every other byte of the destination buffer is still 0x5A,
    frame 3 equals frame 0.  Returns the plan, None where mi355_sws_create refuses the context."""
    ctx = context(ref, name)
    d = ctx.desc
    handle = create(lib, ctx)
    if not handle:
        return None
    try:
        plan = plan_of(lib, handle)
        pics = batch_pictures(name)
        batch = Batch(lib, ctx, pics)
        try:
            out = batch.run(handle)
            frames = [batch.frame(out, f) for f in range(len(pics))]
            assert batch.untouched(out), (name, plan, "bytes outside the pictures changed")
            rb = 3 * d.dstW
            for f in range(3):
                want = oracle_scale(oracle, ctx, pics[f])
                bad = np.nonzero((frames[f][:, :rb] != want[:, :rb]).any(axis=1))[0]
                assert len(bad) == 0, (name, plan, f, "rows", bad[:8])
                if name in SHAPES:
                    assert (frames[f][:, :rb] == ref.scale(name, pics[f])[:, :rb]).all(), (name, plan, f)
            assert (frames[3][:, :rb] == frames[0][:, :rb]).all(), (name, plan)
        finally:
            batch.close()
    finally:
        lib.mi355_sws_destroy(C.c_void_p(handle))
    return plan
