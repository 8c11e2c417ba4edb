"""CPU: packed rgb24 / bgr24 sources of the device swscale path through the emulated product library.

The table of tests/sws_rgbsrc.py must reach what its census lists (asserted from the plan, source, source-layout and destination queries and
from the banks).  Every entry equals the reference's own sws_scale() of the same buffers through Tier 1 (noise, the checkerboard, the ramp
picture) and through a guarded four-frame Tier-2 batch whose packed planes lie on a 16-byte multiple, on a 4-byte multiple and on an odd
address; the two line entries equal the converters' arithmetic written out in numpy; the FATE pin fate-pixfmt-rgb24 is reproduced with both
stages on the product; the creator refuses what lies outside the list; the binding takes these contexts in both of its forms
(oracle/_ref/libswsref_tier1.so)."""
import ctypes as C
import json
import os

import pytest

import sws_nvsrc as V
import sws_planar as P
import sws_rgbsrc as R
import sws_sources as X

HAVE_REF_LIB = os.path.exists(R.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")
GOLD = json.load(open(os.path.join(P.GOLDEN, "sws_ref_sha1.json")))


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        R.make_fresh("_ref/libswsref.so")
    return R.Ref(P.bind(R.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: R.plan(emu.lib, R.stored_entry(name)) for name in R.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_what_the_issue_lists(plans):
    got = {n: p for n, p in plans.items() if p}
    cfgs = {n: R.cfg(n) for n in R.NAMES}
    for n, p in got.items():
        src, dst = cfgs[n][4:6]
        assert (p["depth"], p["hsub"], p["vsub"], p["layout"]) == (8, R.hsub_of(n), 0, R.LAYOUTS[src]), (n, p)
        assert p["format"] == R.DSTS[dst] and p["planes"] == {"rgb": 1, "nv12": 2, "nv21": 2}.get(dst, 3), (n, p)
    fam = lambda *dsts: {n: p for n, p in got.items() if cfgs[n][5] in dsts}        # noqa: E731
    rgb, planar, semi = fam("rgb"), fam("420", "422", "444"), fam("nv12", "nv21")
    # every tile instance, and never k_sws_ident1 or a special converter
    assert {p["kernel"] for p in rgb.values()} == {"generic_a", "generic_b", "generic_c"}
    assert {p["kernel"] for p in {**planar, **semi}.values()} == {"planar_a", "planar_b", "planar_c"}
    assert {cfgs[n][5] for n in planar} == {"420", "422", "444"} and {cfgs[n][5] for n in semi} == {"nv12", "nv21"}
    # the identity, staged and direct forms of the horizontal pass, for luma and for chroma
    forms = {n: R.hforms(R.stored_entry(n), p) for n, p in got.items()}
    for plane in (0, 1):
        reached = set().union(*(f[plane] for f in forms.values()))
        assert reached == {"identity", "staged", "direct"}, (plane, reached)
    for n, p in got.items():
        assert p["hstaged"] == int(any("staged" in f for f in forms[n])), (n, p, forms[n])
    # both converters, in front of identity and of filtered chroma banks; both byte orders in each destination family
    for hsub in (0, 1):
        assert {"identity"} in [forms[n][1] for n in got if got[n]["hsub"] == hsub], hsub
        assert any("staged" in forms[n][1] for n in got if got[n]["hsub"] == hsub), hsub
    for group in (rgb, planar, semi):
        assert {cfgs[n][4] for n in group} == {"rgb24", "bgr24"}, sorted(group)
    # the halving converter on an odd width (pixel srcW is read), odd sizes everywhere
    assert any(got[n]["hsub"] == 1 and cfgs[n][0] % 2 for n in got)
    for k in range(4):
        assert any(cfgs[n][k] % 2 for n in got), k
    # the batch's packed planes hit all three alignment classes
    for n in ("s_420_same", "s_420_down2", "s_rgb_down2", "s_rgb_w384_up", "s_420_hdown4"):
        assert {R.align_class(o, st) for o, st in R.src_layouts(n)} == {16, 4, 1}, (n, R.src_layouts(n))
    # the odd width runs at every pad, 0 included
    assert 0 in X.SRC_PADS and "s_420_oddw" in got


def test_refused_entries_are_named_and_few(plans):
    refused = {n for n, p in plans.items() if p is None}
    assert refused == R.REFUSED, refused
    assert len(refused) * R.REFUSED_CAP <= len(R.NAMES), (len(refused), len(R.NAMES))
    assert not refused & R.FATE and "s_420_vdown8" in refused


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    """every row is opened by the reference (open_formats asserts it) and described as the table expects; the committed arrays are those"""
    for name in R.SHAPES:
        assert R.stored_entry(name).same(ref.entry(name)), name


# ---- parity ------------------------------------------------------------------------------------------------------------------------
TAKEN = [n for n in R.NAMES if n not in R.REFUSED]


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_tier1_matches_reference(emu, ref, name):
    R.check_tier1(emu.lib, ref, name, R.tier1_pictures(name, seed=11))


@needs_ref
@pytest.mark.parametrize("pad", X.SRC_PADS)
def test_emulated_tier1_odd_width_at_every_pad(emu, ref, pad):
    """the halving converter's read of pixel srcW: the next line's first pixel at pad 0, padding noise otherwise, the spare line on the last line"""
    R.check_tier1(emu.lib, ref, "s_420_oddw", R.tier1_pictures("s_420_oddw", seed=31 + pad, pads=(pad, pad, pad)))


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_batched(emu, ref, plans, name):
    p = R.check_batch(emu.lib, ref, name, e=R.stored_entry(name))
    assert p is not None and p == plans[name], name


def test_tier1_refuses_a_stride_below_the_line(emu):
    e = R.stored_entry("s_rgb_down2")
    h = R.create(emu.lib, e)
    assert h
    try:
        lib = emu.lib
        lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        buf = (C.c_uint8 * (128 * 3 * 97))()
        out = (C.c_uint8 * (64 * 3 * 48))()
        src, ss = (C.c_void_p * 3)(C.addressof(buf), None, None), (C.c_int * 3)(3 * 128 - 1, 0, 0)
        assert lib.mi355_sws_scale(C.c_void_p(h), src, ss, out, 192) == -1
    finally:
        emu.lib.mi355_sws_destroy(C.c_void_p(h))


# ---- the line entries: no reference needed -----------------------------------------------------------------------------------------
def test_line_entries_match_the_arithmetic_written_out(emu):
    k = R.constants()
    # the luma constants sum to 219 / 255 and each chroma row to zero, within the rounding of three terms
    assert abs(k["RY"] + k["GY"] + k["BY"] - (219 << 15) / 255) < 2 and abs(k["RU"] + k["GU"] + k["BU"]) < 2 and abs(k["RV"] + k["GV"] + k["BV"]) < 2
    assert R.check_line_entries(emu.lib) > 0


# ---- FATE: both stages on the product, no reference -----------------------------------------------------------------------------------
def test_fate_pixfmt_rgb24_both_stages(emu):
    assert R.fate_md5(emu) == GOLD["fate_pixfmt_rgb24_md5"]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_creator_refuses_what_is_outside_the_list(emu):
    lib = emu.lib
    e = R.stored_entry("s_420_down2")                                                # bgr24, halving
    assert R.plan(lib, e) is not None and (e.layout, e.hsub) == (5, 1)
    assert R.plan(lib, e.edited(layout=4))["layout"] == 4                           # the byte order is the caller's word
    assert not R.create(lib, e.edited(layout=3)) and not R.create(lib, e.edited(layout=6)) and not R.create(lib, e.edited(layout=-1))
    assert not R.create(lib, e.edited(layout=4, depth=10))
    assert not R.create(lib, e.edited(layout=4, vsub=1)) and not R.create(lib, e.edited(layout=4, vsub=1, chrSrcH=48))
    assert not R.create(lib, e.edited(layout=4, chrSrcH=e.ctx.ints["srcH"] - 1))
    assert not R.create(lib, e.edited(layout=4, hsub=2)) and not R.create(lib, e.edited(layout=4, hsub=2, chrSrcW=32))
    assert not R.create(lib, e.edited(layout=4, chrSrcW=e.ctx.ints["chrSrcW"] + 1)) and not R.create(lib, e.edited(layout=4, chrSrcW=e.ctx.ints["chrSrcW"] - 1))
    assert not R.create(lib, e.edited(layout=4, hsub=0))                            # the full converter's chrSrcW is srcW
    assert not R.create(lib, e.edited(layout=4, unscaled_special=1))
    assert not R.create(lib, R.stored_entry("s_rgb_down2").edited(unscaled_special=1))
    for fmt in list(range(4, 16)) + [18]:
        assert not R.create(lib, e.edited(fmt=fmt)), fmt
    # rgb in, rgb out, nothing scaled: the stored NV entry of k_sws_ident1's shape under a packed layout
    nv = V.stored_entry("v_id1_w126")
    assert V.plan(lib, nv)["kernel"] == "ident1_1"
    for layout in (4, 5):
        assert not R.create(lib, nv.edited(layout=layout, vsub=0, chrSrcH=nv.ctx.ints["srcH"])), layout
    # the existing entry points still return -1 across context kinds, and the queries on nothing
    lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale_planar_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.mi355_sws_scale_planar.argtypes = [C.c_void_p] * 5
    buf = (C.c_uint8 * 1024)()
    src, ss = (C.c_void_p * 3)(C.addressof(buf), None, None), (C.c_int * 3)(384, 0, 0)
    dst, ds = (C.c_void_p * 3)(C.addressof(buf), C.addressof(buf), C.addressof(buf)), (C.c_int * 3)(64, 32, 32)
    for name, rgb in (("s_rgb_down2", True), ("s_420_down2", False), ("s_nv21_down2", False)):
        h = R.create(lib, R.stored_entry(name))
        assert h, name
        try:
            if rgb:
                assert lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(h), buf, 1, None) == -1
                assert lib.mi355_sws_scale_planar(C.c_void_p(h), src, ss, dst, ds) == -1
            else:
                assert lib.mi355_sws_scale_frames_dev(C.c_void_p(h), buf, 1, None) == -1
                assert lib.mi355_sws_scale(C.c_void_p(h), src, ss, buf, 192) == -1
        finally:
            lib.mi355_sws_destroy(C.c_void_p(h))
    lib.mi355_sws_source_layout.argtypes = [C.c_void_p]
    assert lib.mi355_sws_source_layout(None) == -1


# ---- the describers on live contexts ---------------------------------------------------------------------------------------------------
@needs_sources
def test_describers_on_live_contexts(ref):
    lib = ref.lib
    flags = lib.ref_sws_flags_word(1, 1, 1)
    for name in R.NAMES:
        c = ref.open(name)
        e = ref.describe(c)
        assert ref.describe_src(c) is None, name                                    # mi355_sws_describe_src keeps declining these sources
        ref.free(c)
        assert e is not None and (e.layout, e.hsub, e.vsub, e.depth) == (R.LAYOUTS[R.cfg(name)[4]], R.hsub_of(name), 0, 8), name
    declined = [
        (64, 48, b"rgb24", 64, 48, b"rgb24", flags),                            # the reference's plain copy
        (64, 48, b"bgr24", 64, 48, b"rgb24", flags),                            # rgbToRgbWrapper
        (64, 48, b"bgr24", 64, 48, b"yuv420p", lib.ref_sws_flags_word(1, 0, 1)),    # bgr24ToYv12Wrapper
        (96, 40, b"rgb24", 64, 40, b"yuv420p", (flags & ~0x7) | 0x1),           # SWS_FAST_BILINEAR
        (96, 40, b"rgb24", 64, 40, b"rgb24", (flags & ~0x7) | 0x1),
        (96, 40, b"rgba", 64, 40, b"yuv420p", flags),
        (96, 40, b"rgb565le", 64, 40, b"yuv420p", flags),
        (96, 40, b"gbrp", 64, 40, b"yuv420p", flags),
        (96, 40, b"rgb24", 64, 40, b"bgr24", flags),
        (64, 48, b"rgb24", 64, 48, b"bgr24", flags),
    ]
    for args in declined:
        c = ref.open_formats(*args)
        assert ref.describe(c) is None, args
        ref.free(c)
    # rgb24 -> yuv420p at equal size runs the generic scaler whatever the flags, and so does bgr24 with SWS_ACCURATE_RND
    for src, fl in ((b"rgb24", lib.ref_sws_flags_word(1, 0, 1)), (b"rgb24", lib.ref_sws_flags_word(0, 0, 0)), (b"bgr24", flags)):
        c = ref.open_formats(64, 48, src, 64, 48, b"yuv420p", fl)
        e = ref.describe(c)
        ref.free(c)
        assert e is not None and (e.layout, e.hsub, e.fmt, e.ctx.desc.unscaled_special) == (R.LAYOUTS[src.decode()], 1, 1, 0), (src, fl)


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return R.Ref(P.bind(R.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", R.BINDING)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = R.ramp(name, seed=5, pad=3)
    sizes = R.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    # the binding's describer knows every one of them, the refused one too (the creator refuses it, not the describer)
    c = hooked.open(name)
    e = hooked.describe(c)
    hooked.free(c)
    assert e is not None and (e.layout, e.hsub, e.fmt) == (R.LAYOUTS[R.cfg(name)[4]], R.hsub_of(name), R.DSTS[R.cfg(name)[5]]), name
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    # a refused context is left to the reference: the picture counter does not move
    assert lib.ref_sws_pictures() == before + (1 if name in R.TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls
    assert not any(R.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("name", R.BINDING)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = R.picture(name, seed=6, pad=3)
    sizes = R.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_tier1_calls() > before, name
    assert lib.ref_sws_pictures() == pics
    assert not any(R.differing_rows(got, want, sizes)), name
