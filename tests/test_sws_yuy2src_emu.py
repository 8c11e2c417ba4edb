"""CPU: packed 4:2:2 sources (yuyv422 / uyvy422 / yvyu422) of the device swscale path through the emulated product library.

The table of tests/sws_yuy2src.py must reach what its census lists (asserted from the plan, source, source-layout, destination, range and depth
queries).  Every taken entry equals the reference's own sws_scale() of the same buffers through Tier 1 and through a guarded four-frame Tier-2 batch
whose packed planes lie on a 16-byte multiple, on 4-byte multiples that are none of 16 and on an ODD address with an odd stride, at line pads of 0, 1,
4 and 3 pixels, on noise, a ramp, all 0, all 255 and a checkerboard; without the reference, every context of the scaler equals the device context of
the SAME descriptor as a yuv422p source on the de-interleaved planes, the three byte orders of one picture give identical output, and the wrappers'
batches equal the four wrappers written out in numpy; the line entries equal the byte table written out; the creators refuse what lies outside the
list, and the table's refused rows are those of the yuv422p twin; the describer reproduces every committed entry from a live reference context;
the binding runs whole pictures of the scaler's contexts on the device and forwards the inner loops under MI355_SWS_LINES=1.

FATE: fate-pixfmt-yuyv422 is yuv420p -> yuyv422 -> yuv444p (the reference's tests/fate-run.sh, pixfmt_conversion).  Its first stage needs the packed
destination, so the reference's stage-1 picture is committed and the device runs stage 2 — a context of the generic scaler; the full chain waits for
the destination."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_nvsrc as V
import sws_planar as P
import sws_rgb32src as Q
import sws_sources as X
import sws_yuy2src as Y

HAVE_REF_LIB = os.path.exists(Y.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        Y.make_fresh("_ref/libswsref.so")
    return Y.Ref(P.bind(Y.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: Y.plan(emu.lib, Y.stored_entry(name)) for name in Y.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_form_of_the_splitter(plans):
    plans = {n: plans[n] for n in Y.SPECIAL}
    assert all(plans.values()), plans
    cfgs = {n: Y.cfg(n) for n in Y.SPECIAL}
    for n, p in plans.items():
        sw, sh, _, _, src, dst = cfgs[n][:6]
        assert p["kernel"] == "yuy2_split" and (p["depth"], p["hsub"], p["vsub"], p["layout"]) == (8, 1, 0, Y.LAYOUTS[src]), (n, p)
        assert (p["format"], p["planes"], p["range"], p["dst_depth"], p["hstaged"]) == (Y.DSTS[dst][0], 3, 0, 8, 0), (n, p)
        # the width rounds up; to yuv420p the rows round down, to yuv422p every row has chroma
        assert (p["chr_bytes"], p["chr_rows"]) == ((sw + 1) // 2, sh // 2 if dst == "420" else sh), (n, p)
    # YUY2_SPLIT in both subsamplings and both layouts
    assert {(cfgs[n][4], cfgs[n][5]) for n in plans} == {("yuyv", "420"), ("uyvy", "420"), ("yuyv", "422"), ("uyvy", "422")}
    # odd widths (the two bytes behind the line) and odd heights in both subsamplings, a picture without a chroma row, a second column tile
    for dst in ("420", "422"):
        assert any(cfgs[n][0] % 2 and cfgs[n][1] % 2 for n in plans if cfgs[n][5] == dst), dst
    assert any(p["chr_rows"] == 0 for p in plans.values()) and any(cfgs[n][0] > 2048 for n in plans) and any(cfgs[n][1] > 8 for n in plans)
    # a ragged tail: a width that is no multiple of the thread's 32 luma samples (byte stores), and whole threads before it (16-byte stores)
    assert {cfgs[n][0] % 32 for n in plans} >= {0, 2, 3, 6} and all(cfgs[n][0] >= 64 for n in plans)
    # the batch's planes hit the three alignment classes; the last frame lies on an odd address at an odd stride
    classes = {Y.align_class(o, st) for n in plans for o, st in Y.src_layouts(n)}
    assert classes == {16, 4, 1}, classes
    for n in plans:
        o, st = Y.src_layouts(n)[3]
        assert o % 2 and st % 2, n
    assert Y.SRC_PADS == (0, 1, 4, 3)


def test_table_reaches_every_form_of_the_scaler(plans):
    taken = {n: plans[n] for n in Y.SCALED if plans[n] is not None}
    entries = {n: Y.stored_entry(n) for n in taken}
    for n, p in taken.items():
        dst = Y.cfg(n)[5]
        assert (p["depth"], p["hsub"], p["vsub"], p["layout"]) == (8, 1, 0, Y.LAYOUTS[Y.order_of(n)]), (n, p)
        assert (p["format"], p["dst_depth"]) == Y.DSTS[dst][:2] and p["range"] == (2 if dst in Y.Q.RANGED else Y.src_range(n)), (n, p)
        assert p["kernel"] != "yuy2_split" and p["kernel"] != "ident1_x", (n, p)                     # no row reports IDENT1_X: chroma sits on every line
    kernels = {p["kernel"] for p in taken.values()}
    assert kernels >= {"ident1_1", "generic_a", "generic_b", "generic_c", "planar_a", "planar_b", "planar_c"}, kernels
    # IDENT1_1 in three DST forms (rgb24, bgr24, a 32-bit order), and only at equal size to a packed destination
    ident = {n for n, p in taken.items() if p["kernel"] == "ident1_1"}
    assert {Y.DSTS[Y.cfg(n)[5]][0] for n in ident} >= {0, 32, 34}, ident
    assert all(Y.cfg(n)[:2] == Y.cfg(n)[2:4] and Y.cfg(n)[5] in Y.Q.PACKED for n in ident), ident
    assert ident == {n for n in taken if Y.cfg(n)[:2] == Y.cfg(n)[2:4] and Y.cfg(n)[5] in Y.Q.PACKED}, ident        # the equal-size case never takes the tile
    generic = {n for n, p in taken.items() if p["kernel"].startswith("generic")}
    assert {Y.DSTS[Y.cfg(n)[5]][0] for n in generic} >= {0, 32, 33}, generic
    # the wide and the narrow store, in both families
    for fam in ("generic", "planar"):
        assert {p["narrow"] for p in taken.values() if p["kernel"].startswith(fam)} == {0, 1}, fam
    # identity, staged and direct horizontal forms
    forms = {n: Y.hforms(entries[n], taken[n]) for n in taken if not taken[n]["kernel"].startswith("ident")}
    luma, chroma = set().union(*(f[0] for f in forms.values())), set().union(*(f[1] for f in forms.values()))
    assert luma == {"identity", "staged", "direct"} and chroma >= {"identity", "staged"}, (luma, chroma)
    assert {p["hstaged"] for p in taken.values()} == {0, 1}
    for n, f in forms.items():
        assert taken[n]["hstaged"] == int("staged" in f[0] | f[1]), (n, f, taken[n])
    # SEMI (both pair orders), both ranges, both deep depths
    assert {p["format"] for p in taken.values() if p["planes"] == 2} == {16, 17}
    assert {p["range"] for p in taken.values()} == {0, 1, 2}
    assert {p["dst_depth"] for p in taken.values()} == {8, 9, 10}
    # all three layouts in each family
    for fam in ("generic", "planar", "ident1"):
        assert {p["layout"] for p in taken.values() if p["kernel"].startswith(fam)} == {16, 17, 18}, fam
    # odd widths: under a filter, and with identity luma
    assert any(Y.cfg(n)[0] % 2 and "identity" in forms[n][0] for n in forms) and any(Y.cfg(n)[0] % 2 and "identity" not in forms[n][0] for n in forms)


def test_refused_entries_are_those_of_the_yuv422p_twin(emu, plans):
    """REFUSED is derived from the twin (the same descriptor as an 8-bit yuv422p source), and the packed layouts are refused exactly there; a taken
    row has its twin's plan"""
    twin = Y.refused_by_the_twin(emu.lib)
    assert twin == Y.REFUSED, twin
    assert {n for n, p in plans.items() if p is None} == Y.REFUSED
    assert len(Y.REFUSED) * Y.REFUSED_CAP <= len(Y.NAMES), (len(Y.REFUSED), len(Y.NAMES))
    for n in Y.SCALED:
        if n in Y.REFUSED:
            continue
        t = Y.plan(emu.lib, Y.twin_entry(Y.stored_entry(n)))
        for k in ("kernel", "th", "lum_lines", "chr_lines", "narrow", "format", "planes", "chr_bytes", "chr_rows", "range", "dst_depth"):
            assert plans[n][k] == t[k], (n, k, plans[n], t)


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    """every row is opened by the reference (open_formats asserts it) and described as the table expects; the committed arrays are those"""
    for name in Y.SHAPES:
        assert Y.stored_entry(name).same(ref.entry(name)), name


@needs_sources
def test_the_table_stays_within_the_cap_with_the_reference_alone(ref, emu):
    """the refused rows from live reference contexts of the yuv422p twins (open_twin), not from the committed file"""
    refused = set()
    for name in Y.SCALED:
        if Y.src_range(name):
            continue                                                            # (its twin is the committed descriptor's: checked above)
        c = ref.open_twin(name)
        dst = Y.cfg(name)[5]
        t = ref.describe_packed(c) if Y.DSTS[dst][0] >= 32 else (ref.describe_depth(c) if Y.DSTS[dst][1] > 8 else (ref.describe_range(c) if dst in Q.RANGED else ref.describe_fmt(c)))
        ref.free(c)
        assert t is not None, name
        t = Y.Entry(t.ctx, t.depth, t.hsub, t.vsub, t.dither, t.fmt, t.layout, getattr(t, "range", 0), getattr(t, "dst_depth", 8), 0)
        assert t.layout == 0
        if Y.plan(emu.lib, t) is None:
            refused.add(name)
    assert refused == Y.REFUSED and len(refused) * Y.REFUSED_CAP <= len(Y.NAMES), refused


# ---- parity with the reference ------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", Y.TAKEN)
def test_emulated_tier1_matches_reference(emu, ref, name):
    Y.check_tier1(emu.lib, ref, name, Y.tier1_pictures(name, seed=11))


@needs_ref
@pytest.mark.parametrize("padb", [0, 1, 2, 8])
def test_emulated_tier1_odd_width_at_every_pad(emu, ref, padb):
    """the read of the two bytes behind the width: the next line's first bytes at pad 0, padding noise otherwise, the spare line on the last line"""
    for name in ("s_uyvy_420_odd", "s_uyvy_422_oddw", "g_uyvy_odd", "g_yuyv_420_oddw_same"):
        Y.check_tier1(emu.lib, ref, name, Y.tier1_pictures(name, seed=31 + padb, pads=(padb, padb, padb)))


@needs_ref
@pytest.mark.parametrize("kinds", [("noise", "ramp", "ones"), ("checker", "zeros", "noise")])
@pytest.mark.parametrize("name", Y.TAKEN)
def test_emulated_batched(emu, ref, plans, name, kinds):
    p = Y.check_batch(emu.lib, ref, name, e=Y.stored_entry(name), kinds=kinds)
    assert p is not None and p == plans[name], name


@needs_ref
@pytest.mark.parametrize("name", ["s_uyvy_420_odd", "s_uyvy_422_oddw", "g_uyvy_odd", "g_yuyv_420_oddw_same"])
def test_emulated_odd_width_extra_bytes_in_the_next_frame(emu, ref, name):
    Y.check_contiguous(emu.lib, ref, name)


# ---- the split model: no reference needed ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds", [("noise", "ramp", "ones"), ("checker", "zeros", "noise")])
@pytest.mark.parametrize("name", Y.SPECIAL)
def test_emulated_batched_equals_the_wrappers_written_out(emu, name, kinds):
    """picks and (a + b) >> 1 in numpy; the model leaves the guard value in the last chroma row of an odd height and behind chr_bytes, and so does
    the device (the comparison runs over the rounded-up extents, and Batch.untouched over everything else)"""
    p = Y.check_batch(emu.lib, None, name, e=Y.stored_entry(name), kinds=kinds)
    assert p is not None and p["kernel"] == "yuy2_split"


def test_the_model_leaves_the_last_chroma_row_and_the_tail_untouched():
    for name in Y.SPECIAL:
        e = Y.stored_entry(name)
        sw, sh, _, _, _, dst = Y.cfg(name)[:6]
        sizes = [(w + 3, h) for w, h in e.out_sizes()]
        out = Y.model_split(name, Y.picture(name, "noise", seed=2), sizes, guard=0xA5)
        assert (out[0][:, sw:] == 0xA5).all(), name
        rows = sh // 2 if dst == "420" else sh
        for c in out[1:]:
            assert c.shape[0] == (-(-sh // 2) if dst == "420" else sh), name
            assert (c[rows:] == 0xA5).all() and (c[:, (sw + 1) // 2:] == 0xA5).all(), name
    assert Y.model_split("s_yuyv_420_h1", Y.picture("s_yuyv_420_h1", "noise"), Y.stored_entry("s_yuyv_420_h1").out_sizes(), guard=0xA5)[1].tolist() == [[0xA5] * 32]


def test_the_two_layouts_of_one_picture_give_identical_output(emu):
    """a yuyv422 picture re-interleaved as uyvy422 (every byte pair swapped) through the other layout's wrapper: the same planes"""
    lib = emu.lib
    for name in ("s_yuyv_420", "s_yuyv_422_w130", "s_yuyv_420_noflags"):
        e = Y.stored_entry(name)
        a = Y.picture(name, "noise", seed=7, padb=2)
        b = [a[0].copy()]
        sw = Y.cfg(name)[0]
        b[0][:, 0:2 * sw:2], b[0][:, 1:2 * sw:2] = a[0][:, 1:2 * sw:2], a[0][:, 0:2 * sw:2]
        outs = []
        for planes, layout in ((a, 16), (b, 17)):
            h = Y.create(lib, e.edited(layout=layout))
            assert h, (name, layout)
            try:
                outs.append(Y.scale_tier1(lib, h, e, planes, pad=4))
            finally:
                lib.mi355_sws_destroy(C.c_void_p(h))
        assert all((x == y).all() for x, y in zip(*outs)), name


# ---- the twin property: no reference needed -------------------------------------------------------------------------------------------
EVEN = [n for n in Y.SCALED if n not in Y.REFUSED and Y.cfg(n)[0] % 2 == 0]


def _run(lib, e, planes):
    h = Y.create(lib, e)
    assert h
    try:
        return Y.scale_tier1(lib, h, e, planes, pad=4)
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))


@pytest.mark.parametrize("name", EVEN)
def test_packed_context_equals_its_yuv422p_twin_on_the_deinterleaved_planes(emu, name):
    """the device context of the packed layout on an interleaved picture against the device context created from the SAME descriptor as a yuv422p
    source on the picture's three planes; and the picture re-interleaved in the two other byte orders through their layouts: identical output"""
    e = Y.stored_entry(name)
    for what, seed in (("noise", 3), ("ramp", 4)):
        packed = Y.picture(name, what, seed=seed, padb=2)
        yuv = Y.deinterleave(name, packed)
        want = _run(emu.lib, Y.twin_entry(e), yuv)
        got = _run(emu.lib, e, packed)
        assert all((g == w).all() for g, w in zip(got, want)), (name, what)
        for order, layout in Y.LAYOUTS.items():
            other = _run(emu.lib, e.edited(layout=layout), Y.interleave(name, yuv, order))
            assert all((g == w).all() for g, w in zip(other, want)), (name, what, order)


# ---- the line entries: no reference needed -----------------------------------------------------------------------------------------
def test_line_entries_match_the_byte_table_written_out(emu):
    assert Y.check_line_entries(emu.lib) == 6 * 4 * 3 * 2


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_creators_refuse_what_is_outside_the_list(emu):
    lib = emu.lib
    e = Y.stored_entry("s_yuyv_420")
    assert Y.plan(lib, e)["kernel"] == "yuy2_split" and (e.layout, e.fmt, e.ctx.desc.unscaled_special) == (16, 1, 1)
    assert Y.plan(lib, e.edited(layout=17))["layout"] == 17 and Y.plan(lib, e.edited(fmt=2))["format"] == 2       # the byte order and the subsampling are the caller's word
    g = Y.stored_entry("g_yuyv_420_down2")                                              # a context of the scaler, to yuv420p ...
    k = Y.stored_entry("p_yuyv_rgb_down2")                                              # ... and to rgb24
    assert Y.plan(lib, g)["kernel"].startswith("planar") and Y.plan(lib, k)["kernel"].startswith("generic")
    for base in (e, g, k):
        for layout in (3, 6, 7, 12, 13, 14, 15, 19, -1):
            assert not Y.create(lib, base.edited(layout=layout)), layout
            assert not Y.create(lib, base.edited(layout=layout, range_=2)) and not Y.create(lib, base.edited(layout=layout, dst_depth=10)), layout
        assert not Y.create(lib, base.edited(depth=10))
        assert not Y.create(lib, base.edited(hsub=0)) and not Y.create(lib, base.edited(hsub=0, chrSrcW=base.ctx.ints["srcW"]))
        assert not Y.create(lib, base.edited(vsub=1)) and not Y.create(lib, base.edited(vsub=1, chrSrcH=base.ctx.ints["srcH"] // 2))
        assert not Y.create(lib, base.edited(chrSrcW=base.ctx.ints["chrSrcW"] + 1)) and not Y.create(lib, base.edited(chrSrcW=base.ctx.ints["chrSrcW"] - 1))
        assert not Y.create(lib, base.edited(chrSrcH=base.ctx.ints["srcH"] - 1))
        for layout in (16, 17, 18):
            assert not Y.create(lib, base.edited(layout=layout), alpha=1) and not Y.create(lib, base.edited(layout=layout, fmt=34), alpha=1), layout
        for fmt in list(range(4, 16)) + [18, 31, 37]:
            assert not Y.create(lib, base.edited(fmt=fmt)), fmt
        assert not Y.create(lib, base.edited(fmt=0, range_=2)) and not Y.create(lib, base.edited(fmt=34, range_=1))      # a range with a packed RGB destination
        assert not Y.create(lib, base.edited(range_=3))
    # the scaler takes all three layouts
    assert Y.plan(lib, g.edited(layout=18))["layout"] == 18 and Y.plan(lib, k.edited(layout=17))["layout"] == 17
    # the special converters: yuyv422 / uyvy422 to 8-bit yuv420p / yuv422p at equal size and equal range, nothing else
    assert not Y.create(lib, e.edited(layout=18))
    for fmt in (0, 3, 16, 17, 32, 33, 34, 35, 36):
        assert not Y.create(lib, e.edited(fmt=fmt)), fmt
    assert not Y.create(lib, e.edited(range_=1)) and not Y.create(lib, e.edited(range_=2))
    assert not Y.create(lib, e.edited(dst_depth=10)) and not Y.create(lib, e.edited(dst_depth=9))
    assert not Y.create(lib, e.edited(dstW=32, chrDstW=16)) and not Y.create(lib, e.edited(dstH=24)) and not Y.create(lib, e.edited(chrDstW=31))
    # the queries on nothing; the entry points across context kinds; a stride below the line
    for f in (lib.mi355_sws_source_layout, lib.mi355_sws_range, lib.mi355_sws_dest_depth):
        f.argtypes = [C.c_void_p]
        assert f(None) == -1
    lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale_planar_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.mi355_sws_scale_planar.argtypes = [C.c_void_p] * 5
    buf = (C.c_uint8 * 1024)()
    plane = np.zeros((49, 128), np.uint8)
    out = [np.zeros((48, 64), np.uint8), np.zeros((24, 32), np.uint8), np.zeros((24, 32), np.uint8)]
    src = (C.c_void_p * 3)(plane.ctypes.data, None, None)
    dst, ds = (C.c_void_p * 3)(*[o.ctypes.data for o in out]), (C.c_int * 3)(64, 32, 32)
    for entry in (e, Y.stored_entry("g_yvyu_420_same")):                                # a wrapper's context and the scaler's, both 64x48 to yuv420p
        h = Y.create(lib, entry)
        assert h
        try:
            assert lib.mi355_sws_scale_frames_dev(C.c_void_p(h), buf, 1, None) == -1
            assert lib.mi355_sws_scale(C.c_void_p(h), src, (C.c_int * 3)(128, 0, 0), out[0].ctypes.data, 64) == -1
            assert lib.mi355_sws_scale_planar(C.c_void_p(h), src, (C.c_int * 3)(128, 0, 0), dst, ds) == 48
            assert lib.mi355_sws_scale_planar(C.c_void_p(h), src, (C.c_int * 3)(127, 0, 0), dst, ds) == -1          # src_stride[0] = 2 * srcW - 1
        finally:
            lib.mi355_sws_destroy(C.c_void_p(h))
    h = Y.create(lib, Y.stored_entry("p_yuyv_rgb_same"))                                # a packed-destination context on the planar entry points
    assert h
    try:
        rgb = np.zeros((48, 192), np.uint8)
        assert lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(h), buf, 1, None) == -1
        assert lib.mi355_sws_scale_planar(C.c_void_p(h), src, (C.c_int * 3)(128, 0, 0), dst, ds) == -1
        assert lib.mi355_sws_scale(C.c_void_p(h), src, (C.c_int * 3)(128, 0, 0), rgb.ctypes.data, 192) == 48
        assert lib.mi355_sws_scale(C.c_void_p(h), src, (C.c_int * 3)(127, 0, 0), rgb.ctypes.data, 192) == -1
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))


# ---- FATE ------------------------------------------------------------------------------------------------------------------------------
def test_fate_stage2_matches_the_pin(emu):
    """stage 2 of fate-pixfmt-yuyv422 (yuyv422 -> yuv444p, the generic scaler) of the committed stage-1 picture: the md5 of Y, U, V is the first
    word of the reference tree's tests/ref/pixfmt/yuyv422.  Stage 1 (yuv420p -> yuyv422) needs the packed destination: the full chain waits for it."""
    assert Y.fate_md5(emu.lib) == Y.fate_gold()["yuyv422"]


@needs_sources
def test_fate_fixtures_are_the_reference_s(ref):
    pin = open("/root/reference/tests/ref/pixfmt/yuyv422").read().split()[0]
    assert Y.fate_gold()["yuyv422"] == pin
    w, h = 352, 288
    c = ref.open_formats(w, h, b"yuv420p", w, h, b"yuyv422", ref.lib.ref_sws_flags_word(1, 1, 1))
    try:
        mid = ref.scale_ctx(c, P.S.fate_frame(), [(2 * w, h)], 0)
    finally:
        ref.free(c)
    assert (mid[0] == Y.fate_mid()[0]).all()


# ---- the describers on live contexts ---------------------------------------------------------------------------------------------------
@needs_sources
def test_describers_on_live_contexts(ref):
    lib = ref.lib
    flags = lib.ref_sws_flags_word(1, 1, 1)
    for name in Y.NAMES:
        c = ref.open(name)
        e = ref.describe(c)
        assert ref.declined_by_the_eight_describers(c), name                        # the eight existing describers keep declining these sources
        ref.free(c)
        assert e is not None and (e.layout, e.hsub, e.vsub, e.depth, e.alpha) == (Y.LAYOUTS[Y.order_of(name)], 1, 0, 8, 0), name
        assert bool(e.ctx.desc.unscaled_special) == (name in Y.SPECIAL), name
    declined = [
        (64, 48, b"yvyu422", 64, 48, b"yuv422p", flags),                        # the generic scaler does run here, but at equal size ...
        (64, 48, b"yuyv422", 64, 48, b"yuyv422", flags),                        # the reference's plain copy
        (64, 48, b"yuyv422", 64, 48, b"uyvy422", flags),                        # no banks, no wrapper of ours
        (64, 48, b"yuyv422", 64, 48, b"yuva420p", flags),                       # the wrapper also fills alpha: YUVA is not ours
        (96, 40, b"yuyv422", 64, 40, b"yuv420p", (flags & ~0x7) | 0x1),         # SWS_FAST_BILINEAR
        (96, 40, b"uyvy422", 64, 40, b"rgb565le", flags),
        (96, 40, b"uyvy422", 64, 40, b"bgra", flags | 0x2000),                  # SWS_FULL_CHR_H_INT
        (96, 40, b"yuv422p", 64, 40, b"yuv420p", flags),                        # the other describers' sources
        (96, 40, b"rgba", 64, 40, b"yuv420p", flags),
        (96, 40, b"nv12", 64, 40, b"yuv420p", flags),
    ]
    for args in declined[1:]:
        c = ref.open_formats(*args)
        assert ref.describe(c) is None, args
        ref.free(c)
    # yvyu422 has no wrapper: at equal size to yuv422p the generic scaler runs, and is described as such
    c = ref.open_formats(*declined[0])
    e = ref.describe(c)
    ref.free(c)
    assert e is not None and (e.layout, e.fmt, e.ctx.desc.unscaled_special) == (18, 2, 0)
    # the contexts of the other sources' tables, one row each
    for mod, name in ((Q, "q_420_down2"), (V, "v_420_down2"), (X, "s420d8_down2" if "s420d8_down2" in X.SHAPES else next(iter(X.SHAPES)))):
        r = mod.Ref(lib)
        c = r.open(name)
        assert ref.describe(c) is None, name
        r.free(c)


@needs_sources
def test_described_scaler_contexts_have_the_banks_of_their_yuv422p_twins(ref):
    """utils.c:1023-1040 treats a packed 4:2:2 source as chrSrcHSubSample 1, chrSrcVSubSample 0: the descriptor mi355_sws_describe_yuy2 fills for a
    context of the scaler is the one the matching describer fills for the yuv422p context of the same sizes, destination and flags"""
    for name in Y.SCALED:
        if Y.src_range(name):
            continue                                                            # (a full-range yuv422p twin is opened by another name: yuvj422p)
        e = ref.entry(name)
        c = ref.open_twin(name)
        dst = Y.cfg(name)[5]
        t = ref.describe_packed(c) if Y.DSTS[dst][0] >= 32 else (ref.describe_depth(c) if Y.DSTS[dst][1] > 8 else (ref.describe_range(c) if dst in Q.RANGED else ref.describe_fmt(c)))
        ref.free(c)
        assert t is not None and (t.depth, t.hsub, t.vsub, t.fmt) == (8, 1, 0, e.fmt), name
        assert e.ctx.ints == t.ctx.ints and V.same_banks(e, t), name
        assert all((np.asarray(e.ctx.luts[k]) == np.asarray(t.ctx.luts[k])).all() for k in P.S.LUTS), name


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return Y.Ref(P.bind(Y.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", Y.BINDING + Y.BINDING_UNBOUND)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    """whole pictures of the scaler's contexts go through mi355_swsfunc to the device (the picture counter moves); a context the creators refuse is
    left to the reference, and no selector this binding wraps runs for a wrapper's context: the counter stays and the picture is the reference's"""
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = Y.picture(name, "ramp", seed=5, padb=6)
    sizes = Y.out_sizes(name)
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    # the binding's describer knows every one of them, the refused one too (the creator refuses it, not the describer)
    c = hooked.open(name)
    e = hooked.describe(c)
    hooked.free(c)
    assert e is not None and e.layout == Y.LAYOUTS[Y.order_of(name)] and bool(e.ctx.desc.unscaled_special) == (name in Y.SPECIAL), name
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_pictures() == before + (1 if name in Y.BINDING_TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls, name
    assert not any(Y.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("name", Y.BINDING + Y.BINDING_UNBOUND)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    """MI355_SWS_LINES=1: c->lumToYV12 / c->chrToYV12 of a context of the scaler go to mi355_sws_yuy2ToY / _yuy2ToUV (the call counter moves);
    a wrapper has no inner loops"""
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = Y.picture(name, "noise", seed=6, padb=6)
    sizes = Y.out_sizes(name)
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    if name in Y.BINDING:
        assert lib.ref_sws_tier1_calls() > before, name
    else:
        assert lib.ref_sws_tier1_calls() == before, name
    assert lib.ref_sws_pictures() == pics
    assert not any(Y.differing_rows(got, want, sizes)), name
