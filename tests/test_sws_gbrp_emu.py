"""CPU: planar RGB (gbrp) destinations (mi355_sws_create_gbrp) of the device swscale path through the emulated product library.

The table of tests/sws_gbrp.py must reach what its census lists: every instance of k_sws_gbrp the emulated library holds (read from its symbol
table: seven source classes at A / B / C), every source layout class, the rules named beside its rows.  Every row equals the reference's own
sws_scale() of the same buffers — the committed fixture — through a guarded four-frame Tier-2 batch and through Tier 1; the fixture equals the numpy
restatement of the whole context computed modulo 2^32, and its wrap counts are the restatement's; the line entry equals the restatement over one /
two / four / nine taps; the creator refuses what the header lists and the queries follow the twin rule.  With the reference's sources: the committed
fixture is what the reference gives today, the other describers keep declining the destination, and the binding runs it on the device."""
import re
import subprocess

import numpy as np
import pytest

import sws_gbrp as B
import sws_instances as I
import sws_planar as P

needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    B.make_fresh("_ref/libswsref.so")
    return B.Ref(P.bind(B.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: B.plan(emu.lib, B.stored_entry(name)) for name in B.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def gbrp_instances(path=I.EMU_LIB):
    """the instances of k_sws_gbrp in the library at `path`: (i, source class)"""
    out = subprocess.run(["nm", "-C", path], capture_output=True, text=True, check=True).stdout
    keys = set()
    for args in set(re.findall(r"::k_sws_gbrp<([^<>]*)>\(", out)):              # LCAP, CCAP, ST, NV, RGB
        a = [s.strip() for s in args.split(",")]
        flag = lambda s: {"true": True, "false": False}[s]                      # noqa: E731
        keys.add((I.SHAPES["planar"].index((int(a[0]), int(a[1]))), I._src_class(a[2], flag(a[3]), flag(a[4]))))
    return keys


def key_of(name, p):
    fam, i = p["kernel"].split("_")
    assert fam == "planar", p
    return ("abc".index(i), B.src_class(name))


def test_the_new_kernel_has_a_name_of_its_own(emu):
    """21 instances: seven source classes at A / B / C; the five pinned kernels keep their instance space (tests/test_sws_instances_emu.py counts it)"""
    assert gbrp_instances() == {(i, c) for i in range(3) for c in B.CLASSES}
    assert I.instance_space() and not any("gbrp" in str(k) for k in I.instance_space())


def test_the_two_statements_of_the_horizontal_pass_are_one_text():
    """planar_hscale (k_sws_gbrp's) restates k_sws_planar's body up to its barrier, because the pinned kernel must keep its own text (sws_dev.h says
    why): the two are the same lines, but for the declaration of clo / nchr, so a change to one that misses the other fails here"""
    import os
    text = open(os.path.join(B.X.ROOT, "libav_amd", "csrc", "sws_dev.h")).read()
    first = "    if constexpr (std::is_same<ST, SwsPxP010>::value) {\n        static_assert(NV && !RGB"
    f0 = text.index(first)
    shared = text[f0:text.index("}\n\n/* One workgroup per output tile", f0)]
    k0 = text.index(first, text.index("__global__ void __launch_bounds__(NT) k_sws_planar("))
    own = text[k0:text.index("    __syncthreads();", k0)]
    assert f0 < k0 and len(shared) > 4000
    assert shared.replace("    clo = 0; nchr = 0;\n", "    int clo = 0, nchr = 0;\n") == own


def test_table_reaches_every_instance_and_rule(emu, plans):
    assert all(p is not None for p in plans.values()), [n for n, p in plans.items() if p is None]
    for n, p in plans.items():
        e = B.stored_entry(n)
        d = e.ctx.desc
        assert (p["gbrp"], p["coefs"], p["alpha"], p["range"], p["dst_depth"]) == (1, e.coefs, 0, 0, 8), (n, p)
        assert (p["format"], p["planes"], p["chr_bytes"], p["chr_rows"]) == (B.DST_GBRP, 3, d.dstW, d.dstH), (n, p)
        assert (p["layout"], p["depth"]) == B.SOURCES[B.icfg(n)[4]] and p["kernel"].startswith("planar_"), (n, p)
        assert d.chrDstW == d.dstW and d.vChr.n == d.dstH and not d.unscaled_special, n
    # every instance of the new kernel, as the emulated library's symbol table lists them: each created at least once
    assert {key_of(n, p) for n, p in plans.items()} == gbrp_instances()
    for tag in B.SPAN_ROWS:
        assert all(plans["%s_%s" % (tag, s)]["kernel"] == "planar_" + tag for s in B.SPAN_SOURCES), tag
    # every source layout class of the header's list; both chroma converters of a 32-bit source
    assert {p["layout"] for p in plans.values()} >= {0, 1, 2, 4, 5, 8, 10, 16, 17, 24}
    assert {(p["depth"], p["hsub"], p["vsub"]) for p in plans.values() if p["layout"] == 0} >= {(8, 1, 1), (8, 1, 0), (8, 0, 0), (9, 1, 0), (10, 1, 1)}
    assert {p["hsub"] for p in plans.values() if 8 <= p["layout"] <= 11} == {0, 1}
    # the rules beside the rows
    size = lambda n, k: getattr(B.stored_entry(n).ctx.desc, k).size      # noqa: E731
    assert (size("same_420", "vLum"), size("same_444", "vLum"), size("same_444", "vChr")) == (1, 1, 1) and size("same_420", "vChr") > 1
    assert size("shrink_420_taps", "vLum") > 8 and plans["shrink_420_taps"]["narrow"] == 1
    assert max(size(n, "vLum") for n in B.NAMES if n != "shrink_420_taps") <= 8        # ... and the others take the taps from registers
    assert {size(n, k) for n in B.NAMES for k in ("vLum", "vChr")} >= {1, 2, 4}
    assert B.cfg("up_420_w130")[2] == 130 and B.cfg("down_420_w260")[2] > 2 * B.TW and B.cfg("up_420_h1")[3] == 1 and B.cfg("odd_422_w71")[2] % 8
    d = B.stored_entry("down_420_w260").ctx.desc
    assert d.srcW * B.TW // d.dstW > 4 * 76 and plans["up_420_w130"]["hstaged"] == 1     # a full luma tile's span against the staged line (76 dwords): unstaged
    assert all(v % 16 == 0 for v in B.cfg("up_420_w256_al16")[:4:2])
    assert {plans[n]["narrow"] for n in B.NAMES} == {0, 1}
    assert max(B.cfg(n)[0] for n in B.NAMES) <= 900 and max(B.cfg(n)[1] for n in B.NAMES) <= 48
    assert max(B.cfg(n)[2] for n in B.NAMES) <= 260 and max(B.cfg(n)[3] for n in B.NAMES) <= 24
    # full-range and ITU-709 coefficients beside the default ones
    default = B.stored_entry("up_420_w130").coefs
    full = B.stored_entry("up_yuvj420p").coefs
    assert default[0] == 16 << 9 and full[:2] == (0, 8192) and all(full[2:]) and (full[2] > 0 > full[3]) and (full[5] > 0 > full[4]), (default, full)
    assert all(abs(a) < abs(b) for a, b in zip(full[2:], default[2:]))                  # (full-range chroma has the smaller gain)
    assert all(any(B.stored_entry(n).coefs[1:]) for n in B.NAMES)
    e = B.stored_entry("up_yuvj420p")
    planes = B.restate("up_yuvj420p", e, B.frames("up_yuvj420p")[2])[0]
    assert all(len(np.unique(p)) > 32 for p in planes)                                   # the row's planes are pictures, not a constant
    assert len({B.stored_entry(n).coefs for n in ("up_420_w130", "up_yuvj420p", "up_420_bt709")}) == 3
    assert all(B.stored_entry(n).coefs == default for n in B.NAMES if n not in ("up_yuvj420p", "up_420_bt709"))
    # the four source layouts of a batch: every fetch form of every plane
    for n in B.NAMES:
        lay = B.src_layouts(n)
        assert {I.align_class(*lay[f][0]) for f in range(4)} >= ({16, 4} if I.granule(B.icfg(n)) == 4 else {16, 4, I.granule(B.icfg(n))}), n


def test_the_wrap_is_tested():
    """at least one full-range frame wraps; frames 2 and 3 of no bilinear row do — the nominal-range frames of the YUV sources, and the packed RGB
    sources' too (full-range noise there: they have no nominal range, and their converters give nominal YUV)"""
    wraps = {n: B.stored_wraps(n) for n in B.NAMES}
    assert any(sum(w[:2]) for w in wraps.values())
    assert sum(1 for n in B.NAMES if B.bilinear(n) and B.yuv_source(n)) >= 8 and sum(1 for n in B.NAMES if B.bilinear(n) and not B.yuv_source(n)) >= 5
    for n in B.NAMES:
        if B.bilinear(n):
            assert wraps[n][2:] == [0, 0], (n, wraps[n])


@pytest.mark.parametrize("name", B.NAMES)
def test_fixture_equals_the_wrapped_restatement(name):
    """the whole context in numpy, the three sums modulo 2^32: the committed bytes and the committed wrap counts"""
    e = B.stored_entry(name)
    sizes, want = e.out_sizes(), B.stored_hashes(name)
    for f, planes in enumerate(B.frames(name)):
        got, n = B.restate(name, e, planes)
        assert [bytes(h) for h in B.plane_hashes(got, sizes)] == want[f], (name, f)
        assert n == B.stored_wraps(name)[f], (name, f)


def test_the_restatement_is_the_formula():
    k = (8192, 9539, 13075, -6660, -3209, 16525)
    # Y = 16, U = V = 128: black; Y = 235: white; Y = 255 with U = 255: B leaves int32 and wraps to a negative sum, which clips to 0
    px = lambda y, u, v: [int(p[0]) for p in B.matrix(k, np.array([y << 9]), np.array([(u - 128) << 9]), np.array([(v - 128) << 9]))[0]]      # noqa: E731
    assert px(16, 128, 128) == [0, 0, 0] and px(235, 128, 128) == [255, 255, 255]
    y = ((255 << 9) - k[0]) * k[1] + (1 << 21)
    b = y + ((255 - 128) << 9) * k[5]
    assert b >= 1 << 31 and px(255, 255, 128)[1] == 0
    assert int(B.matrix(k, np.array([255 << 9]), np.array([127 << 9]), np.array([0]))[1].sum()) == 1
    assert B.clip30(np.array([-1, 0, (1 << 30) - 1, 1 << 30])).tolist() == [0, 0, (1 << 30) - 1, (1 << 30) - 1]


# ---- parity with the reference: the committed fixture --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", B.NAMES)
def test_emulated_batched(emu, plans, name):
    p = B.check_batch(emu.lib, name)
    assert p == plans[name], name


@pytest.mark.parametrize("name", B.NAMES)
def test_emulated_tier1(emu, name):
    B.check_tier1(emu.lib, name)


@needs_sources
def test_committed_fixture_matches_the_reference(ref):
    """every row is opened by the reference to AV_PIX_FMT_GBRP and taken by mi355_sws_describe_gbrp; the committed arrays and hashes are those"""
    for name in B.NAMES:
        e = ref.entry(name)
        assert B.stored_entry(name).same(e), name
        sizes = e.out_sizes()
        got = [[bytes(h) for h in B.plane_hashes(ref.scale(name, planes, sizes), sizes)] for planes in B.frames(name)]
        assert got == B.stored_hashes(name), name


@needs_sources
def test_the_other_describers_keep_declining(ref):
    """a gbrp context: the twelve existing describers decline it before and after the new one has looked at it; the contexts that stay the reference's"""
    for name in B.NAMES:
        c = ref.open(name)
        assert ref.declined_by_the_other_describers(c), name
        assert ref.describe_gbrp(c) is not None and ref.declined_by_the_other_describers(c), name
        ref.free(c)
        c = ref.open(name, dst=b"yuv444p")                                                 # the same context to the twin's format: not this describer's
        assert ref.describe_gbrp(c) is None, name
        ref.free(c)
    flags = ref.lib.ref_sws_flags_word(1, 1, 1)
    for args in ((96, 40, b"yuv420p", 128, 40, b"gbrap", flags),                            # alpha, the deeper formats
                 (96, 40, b"yuv420p", 128, 40, b"gbrp10le", flags),
                 (96, 40, b"gbrp", 128, 40, b"gbrp", flags),                                # a planar RGB source
                 (96, 40, b"yuva420p", 128, 40, b"gbrp", flags),
                 (96, 40, b"rgb24", 96, 40, b"gbrp", flags),                                # rgbToPlanarRgbWrapper: no banks
                 (96, 40, b"yuv420p", 128, 40, b"gbrp", (flags & ~0x7) | 0x1),              # SWS_FAST_BILINEAR
                 (96, 40, b"yuvj420p", 128, 40, b"gbrp", flags)):                           # range converters in front of full-range coefficients
        c = ref.open_formats(*args)
        assert ref.describe_gbrp(c) is None, args
        ref.free(c)


# ---- the line entry ------------------------------------------------------------------------------------------------------------------
def test_line_entry_matches_the_restatement(emu):
    assert B.LINE_TAPS == (1, 2, 4, 9) and B.LINE_WIDTHS == (1, 7, 8, 129)
    assert B.check_line_entry(emu.lib) == 4 * 4 * 2


# ---- refusals and queries --------------------------------------------------------------------------------------------------------------
_CASES = [c[0] for c in B.refusal_cases()]


@pytest.mark.parametrize("what", _CASES)
def test_creator_refuses(emu, what):
    _, e, with_coefs = next(c for c in B.refusal_cases() if c[0] == what)
    assert not B.create(emu.lib, e, with_coefs), what


def test_the_base_of_the_refusal_cases_is_taken_and_the_twin_refuses_with_it(emu):
    assert B.plan(emu.lib, B.stored_entry("up_420_w130"))["gbrp"] == 1
    cases = {c[0]: c[1] for c in B.refusal_cases()}
    for what in ("layout 3", "layout 7", "depth 12", "nv12 at 4:4:4", "chrDstW of a 4:2:0 destination", "vertical banks of 64 taps", "unscaled_special"):
        assert B.plan(emu.lib, cases[what], B.create_twin) is None, what                   # a refusal of the twin's
    for what in ("y_coeff of 2^23", "u2b of -2^23", "y_offset of 2^22"):
        assert B.plan(emu.lib, cases[what], B.create_twin) is not None, what               # a refusal of this creator's own


def test_the_existing_creators_keep_refusing_the_format(emu):
    e = B.stored_entry("up_420_w130")
    assert not B.create_twin(emu.lib, e, B.DST_GBRP)
    f = emu.lib.mi355_sws_create_fast_bilinear
    f.restype = B.C.c_void_p
    f.argtypes = [B.C.c_void_p, B.C.c_void_p] + [B.C.c_int] * 5
    d = e.ctx.desc
    li, ci = B.F.plain_c_increment(d.srcW, d.dstW), B.F.plain_c_increment(d.chrSrcW, d.chrDstW)
    assert not f(B.C.byref(d), B.C.byref(e.src), B.DST_GBRP, 0, 8, li, ci)
    h = f(B.C.byref(d), B.C.byref(e.src), B.DST_YUV444P, 0, 8, li, ci)                    # (the same call to the twin's format is taken)
    assert h
    emu.lib.mi355_sws_destroy(B.C.c_void_p(h))


def test_queries_follow_the_twin_rule(emu, plans):
    for n in B.NAMES:
        e = B.stored_entry(n)
        t = B.plan(emu.lib, e, B.create_twin)
        assert t is not None and (t["gbrp"], t["coefs"], t["format"]) == (0, (0,) * 6, B.DST_YUV444P), n      # the existing creators answer as before
        for k in B.TWIN_KEYS:
            assert plans[n][k] == t[k], (n, k, plans[n], t)
    emu.lib.mi355_sws_rgb_coefs_of.argtypes = [B.C.c_void_p] * 2
    assert emu.lib.mi355_sws_rgb_coefs_of(None, None) == -1
    h = B.create(emu.lib, B.stored_entry("same_444"))
    assert emu.lib.mi355_sws_rgb_coefs_of(B.C.c_void_p(h), None) == 1
    emu.lib.mi355_sws_destroy(B.C.c_void_p(h))


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
BINDING = ["up_420_w130", "odd_422_w71", "same_420", "up_p10_420", "up_nv12", "up_bgr24", "down_rgba_h1", "up_uyvy422", "up_p010", "up_yuvj420p", "up_420_bt709",
           "c_yuv420p"]


@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return B.Ref(P.bind(B.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", BINDING)
def test_binding_whole_pictures(hooked, name, monkeypatch):
    """whole pictures of a gbrp context go through mi355_swsfunc to the device (the picture counter moves) and are the unbound reference's bytes"""
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = B.stored_entry(name)
    sizes, planes = e.out_sizes(), B.frames(name)[1]
    lib = hooked.lib
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_pictures() == before + 1 and lib.ref_sws_tier1_calls() == calls, name
    assert [bytes(h) for h in B.plane_hashes(got, sizes)] == B.stored_hashes(name)[1], name


@pytest.mark.parametrize("name", BINDING)
def test_binding_inner_loop(hooked, name, monkeypatch):
    """MI355_SWS_LINES=1: c->yuv2anyX goes to mi355_sws_yuv2gbrp_full_X, one call an output row (the call counter moves) — but for the last two rows
    of a picture, for which the reference's swscale() fetches its C output functions afresh (swscale.c: dstY >= dstH - 2)"""
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    e = B.stored_entry(name)
    sizes, planes = e.out_sizes(), B.frames(name)[2]
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_tier1_calls() == before + e.ctx.desc.dstH - 2 and lib.ref_sws_pictures() == pics, name
    assert [bytes(h) for h in B.plane_hashes(got, sizes)] == B.stored_hashes(name)[2], name


def test_binding_builds_the_device_side_anew_when_the_coefficients_change(hooked, ref, monkeypatch):
    """one bound context scales a picture, takes ITU-709 coefficients through sws_setColorspaceDetails, and scales the picture again: both go to the
    device, the first with the default coefficients (the unbound reference's bytes), the second with the new ones (the committed up_420_bt709 row)"""
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    name = "up_420_bt709"
    plain = B.cfg(name)[:7] + (None,)                                                      # the row's context as sws_getContext() leaves it
    e = B.stored_entry(name)
    sizes, planes = e.out_sizes(), B.frames(name)[1]
    want0 = ref.scale(plain, planes, sizes)
    lib = hooked.lib
    before = lib.ref_sws_pictures()
    c = hooked.open(plain)
    try:
        got0 = hooked.scale_ctx(c, planes, sizes, 8)
        hooked.set_colorspace(c, B.cfg(name)[7])
        got1 = hooked.scale_ctx(c, planes, sizes, 8)
    finally:
        hooked.free(c)
    assert lib.ref_sws_pictures() == before + 2
    assert not any(B.X.differing_rows(got0, want0, sizes))
    h0, h1 = ([bytes(h) for h in B.plane_hashes(g, sizes)] for g in (got0, got1))
    assert h1 == B.stored_hashes(name)[1] and h0 != h1
