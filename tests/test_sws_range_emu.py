"""CPU: range conversion of the device swscale path through the emulated product library.

The table of tests/sws_range.py must reach what its census lists (asserted from the plan, source, source-layout, destination and range queries,
from the banks, and from the reference's own horizontal function).  Every entry equals the reference's own sws_scale() of the same buffers
through Tier 1 (noise, the checkerboard, the ramp, all-0 and all-maximum pictures) and through a guarded six-frame Tier-2 batch whose planes lie
on a 16-byte multiple, on a 4-byte multiple and on an odd address; the two line entries equal the four formulas written out in numpy over all
65536 int16 values; the three conversions of fate-filter-pixfmts-copy's yuvj rows give the reference's md5s; range 0 through the new creator is
mi355_sws_create_src_layout; the creator refuses what lies outside the list; the binding takes these contexts in both of its forms
(oracle/_ref/libswsref_tier1.so)."""
import ctypes as C
import os

import pytest

import sws_nvsrc as V
import sws_planar as P
import sws_range as G
import sws_rgbsrc as R
import sws_sources as X

HAVE_REF_LIB = os.path.exists(G.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        G.make_fresh("_ref/libswsref.so")
    return G.Ref(P.bind(G.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: G.plan(emu.lib, G.stored_entry(name)) for name in G.NAMES}


DST_KIND = {"yuv420p": "420", "yuv422p": "422", "yuv444p": "444", "nv12": "nv12", "nv21": "nv21"}


def source_class(name):
    """8-bit planar, 9-bit, 10-bit planar (dithered), nv, rgb with the halving / the full chroma converter"""
    kind, depth, (hsub, _) = G.src_kind(name)
    return {"planar": "d%d" % depth, "nv": "nv", "rgb": "rgb_half" if hsub else "rgb_full"}[kind]


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_what_the_issue_lists(plans):
    got = {n: p for n, p in plans.items() if p}
    cfgs = {n: G.cfg(n) for n in G.NAMES}
    for n, p in got.items():
        kind, depth, (hsub, vsub) = G.src_kind(n)
        assert (p["depth"], p["hsub"], p["vsub"], p["layout"], p["range"]) == (depth, hsub, vsub, G.LAYOUTS.get(cfgs[n][4], 0), G.direction(n)), (n, p)
        assert p["format"] == G.DSTS[cfgs[n][6]] and p["planes"] == (2 if cfgs[n][6] in ("nv12", "nv21") else 3), (n, p)
        assert p["kernel"].startswith("planar_"), (n, p)
    for way in (G.FROM_JPEG, G.TO_JPEG):
        rows = {n: p for n, p in got.items() if p["range"] == way}
        # each destination kind, each source kind, the three instances, staged and not, narrow and not
        assert {DST_KIND[cfgs[n][6]] for n in rows} == {"420", "422", "444", "nv12", "nv21"}, way
        assert {source_class(n) for n in rows} == {"d8", "d9", "d10", "nv", "rgb_half", "rgb_full"}, (way, {source_class(n) for n in rows})
        assert {p["kernel"] for p in rows.values()} == {"planar_a", "planar_b", "planar_c"}, (way, {n: p["kernel"] for n, p in rows.items()})
        assert {p["hstaged"] for p in rows.values()} == {0, 1} and {p["narrow"] for p in rows.values()} == {0, 1}, way
        # a vertical bank of more than eight taps; equal size with identity banks and one vertical tap (yuv2plane1)
        assert any(G.stored_entry(n).ctx.desc.vLum.size > 8 for n in rows), way
        same = [n for n in rows if cfgs[n][:2] == cfgs[n][2:4]]
        assert any(G.stored_entry(n).ctx.desc.vLum.size == 1 and G.stored_entry(n).ctx.desc.hLum.size == 1 for n in same), way
        # the forms of the horizontal pass: identity, staged, direct (a 4:1 reduction at dstW 128 or 130)
        forms = set()
        for n in rows:
            if G.src_kind(n)[0] == "planar" and G.src_kind(n)[1] == 8:
                forms |= set().union(*R.hforms(G.stored_entry(n), rows[n]))
        assert forms == {"identity", "staged", "direct"}, (way, forms)
    # the rows the issue names
    named = {"f_420_same": ("yuv420p", 1, "yuv420p", 0), "t_420_same": ("yuv420p", 0, "yuv420p", 1), "f_nv12_same": ("yuv420p", 1, "nv12", 0),
             "t_rgb_420_same": ("rgb24", 0, "yuv420p", 1)}
    for n, want in named.items():
        assert cfgs[n][:4] == (64, 48, 64, 48) and cfgs[n][4:8] == want and n in got, n
    assert {cfgs[n][2] for n in got} >= {127, 128, 129, 130} and cfgs["t_d10_422_w129_up"][:4] == (100, 30, 129, 45)
    assert cfgs["f_nv21_422_odd"][:4] == (33, 17, 97, 61) and any(cfgs[n][3] == 1 for n in got)
    assert {cfgs[n][2] for n in got if cfgs[n][0] == 4 * cfgs[n][2]} == {128, 130}
    # the batch's first planes hit all three alignment classes
    for n in ("f_420_same", "t_420_down2", "t_rgb_420_same"):
        assert {G.align_class(o, st) for o, st in G.src_layouts(n)} == {16, 4, 1}, (n, G.src_layouts(n))


@needs_ref
def test_the_cap_and_negative_samples_are_live(ref):
    """from the reference's own c->hyScale: a to-JPEG row is handed luma above its cap of 30189 and below 0, a from-JPEG row the 32767 of the
    horizontal clamp"""
    lo, hi = ref.hscale_extremes("t_d10_422_w129_up", G.picture("t_d10_422_w129_up", "checker"))
    assert hi > 30189 and lo < 0, (lo, hi)
    lo, hi = ref.hscale_extremes("f_d10_444_w127", G.picture("f_d10_444_w127", "checker"))
    assert hi == 32767 and lo < 0, (lo, hi)
    # ... and the 8-bit rows: the bicubic overshoot of noise under a 2:1 reduction
    lo, hi = ref.hscale_extremes("t_420_nv12_down2", G.picture("t_420_nv12_down2", "noise"))
    assert hi > 30189 and lo < 0, (lo, hi)


def test_refused_entries_are_named_and_few(emu, plans):
    refused = {n for n, p in plans.items() if p is None}
    assert refused == G.REFUSED, refused
    assert len(refused) * G.REFUSED_CAP <= len(G.NAMES), (len(refused), len(G.NAMES))
    assert not refused & G.FATE
    # a ranged context has its twin's banks: it is refused exactly where the twin is
    for n in G.NAMES:
        e = G.stored_entry(n)
        assert (V.plan(emu.lib, e) is None) == (n in refused), n


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    """every row is opened by the reference and described as the table expects; the committed arrays are those, and the banks the twin's"""
    for name in G.SHAPES:
        e = G.stored_entry(name)
        assert e.same(ref.entry(name)), name
        c = ref.open_twin(name)
        twin = ref.describe_fmt(c)
        ref.free(c)
        if twin is not None and not twin.ctx.desc.unscaled_special:
            assert G.V.same_banks(e, twin), name


# ---- parity ------------------------------------------------------------------------------------------------------------------------
TAKEN = [n for n in G.NAMES if n not in G.REFUSED]


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_tier1_matches_reference(emu, ref, name):
    G.check_tier1(emu.lib, ref, name, G.tier1_pictures(name, seed=11))


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_batched(emu, ref, plans, name):
    p = G.check_batch(emu.lib, ref, name, e=G.stored_entry(name))
    assert p is not None and p == plans[name], name


@needs_ref
def test_the_direction_matters(emu, ref):
    """a context created with the other direction than the one the reference's converters gave is another picture: what the binding's per-call
    probe guards against (simulated by editing the entry, not the reference)"""
    for name in ("f_420_same", "t_420_down2"):
        e = G.stored_entry(name)
        planes = G.picture(name, "noise", 3)
        want = ref.scale(name, planes, e.out_sizes())
        for rng, equal in ((e.range, True), (3 - e.range, False)):
            h = G.create(emu.lib, e.edited(range=rng))
            assert h
            try:
                got = G.scale_tier1(emu.lib, h, e, planes)
                assert (not any(G.differing_rows(got, want, e.out_sizes()))) == equal, (name, rng)
            finally:
                emu.lib.mi355_sws_destroy(C.c_void_p(h))


# ---- the line entries: no reference needed -----------------------------------------------------------------------------------------
def test_line_entries_match_the_formulas_written_out(emu):
    # the probes the binding reads the direction from
    assert [int(G.model([0], c, t)[0]) for c in (False, True) for t in (0, 1)] == [2048, -2384, 1992, -2269]
    assert G.check_line_entries(emu.lib) > 0


# ---- FATE ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(G.FATE))
def test_fate_pixfmts_copy_yuvj_rows(emu, name):
    assert G.fate_md5(emu.lib, name) == G.fate_gold()[name]


@needs_ref
def test_fate_golden_is_the_references(ref):
    for name in sorted(G.FATE):
        sizes = G.stored_entry(name).out_sizes()
        assert G.md5_planes(ref.scale(name, G.fate_planes(), sizes, pad=0), sizes) == G.fate_gold()[name], name


# ---- the creator -------------------------------------------------------------------------------------------------------------------
def test_range_0_is_the_existing_creator(emu):
    """same plan and same bytes on two stored entries of the sibling tables"""
    lib = emu.lib
    for mod, name in ((V, "v_420_down2"), (R, "s_nv21_down2")):
        e = mod.stored_entry(name)
        g = G.Entry(e.ctx, e.depth, e.hsub, e.vsub, e.dither, e.fmt, e.layout, 0)
        old, new = mod.create(lib, e), G.create(lib, g)
        assert old and new, name
        try:
            po, pn = mod.plan_of(lib, old), G.plan_of(lib, new)
            assert pn.pop("range") == 0 and po == pn, name
            planes = mod.picture(name, seed=9, pad=3)
            a, b = X.scale_tier1(lib, old, e, planes), X.scale_tier1(lib, new, e, planes)
            assert all((x == y).all() for x, y in zip(a, b)), name
        finally:
            lib.mi355_sws_destroy(C.c_void_p(old))
            lib.mi355_sws_destroy(C.c_void_p(new))


def test_creator_refuses_what_the_reference_never_builds(emu):
    lib = emu.lib
    e = G.stored_entry("f_420_down2")
    assert G.plan(lib, e)["range"] == G.FROM_JPEG and G.plan(lib, e.edited(range=G.TO_JPEG))["range"] == G.TO_JPEG
    for rng in (-1, 3, 4):
        assert not G.create(lib, e.edited(range=rng)), rng
    # a range to rgb24, and with the unscaled special converters (rgb24, the packer, the splitter)
    rgb = V.stored_entry("v_rgb_down2")
    for rng in (G.FROM_JPEG, G.TO_JPEG):
        assert not G.create(lib, G.Entry(rgb.ctx, rgb.depth, rgb.hsub, rgb.vsub, rgb.dither, 0, rgb.layout, rng)), rng
        assert not G.create(lib, e.edited(range=rng, fmt=0)), rng
        assert not G.create(lib, e.edited(range=rng, unscaled_special=1)), rng
        split = V.stored_entry("k_split")
        assert V.plan(lib, split)["kernel"] == "nv12_split"
        assert not G.create(lib, G.Entry(split.ctx, split.depth, split.hsub, split.vsub, split.dither, split.fmt, split.layout, rng)), rng
        # what the existing creator refuses stays refused with a range
        for layout in (3, 6, -1):
            assert not G.create(lib, e.edited(range=rng, layout=layout)), (rng, layout)
        for fmt in list(range(4, 16)) + [18]:
            assert not G.create(lib, e.edited(range=rng, fmt=fmt)), (rng, fmt)
        assert not G.create(lib, e.edited(range=rng, depth=11)) and not G.create(lib, e.edited(range=rng, layout=1, depth=10))
    lib.mi355_sws_range.argtypes = [C.c_void_p]
    assert lib.mi355_sws_range(None) == -1


def test_existing_entry_points_on_a_ranged_descriptor(emu):
    """the existing creators answer as before on a ranged context's descriptor (it is its twin's), and the RGB entry points return -1 on a
    ranged context"""
    lib = emu.lib
    e = G.stored_entry("t_420_down2")
    assert V.plan(lib, e) == {k: v for k, v in G.plan(lib, e).items() if k != "range"}
    assert X.plan(lib, e)["kernel"] == V.plan(lib, e)["kernel"] and P.plan(lib, e.ctx, "420")["kernel"] == V.plan(lib, e)["kernel"]
    lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    buf = (C.c_uint8 * 1024)()
    src, ss = (C.c_void_p * 3)(C.addressof(buf), C.addressof(buf), C.addressof(buf)), (C.c_int * 3)(128, 64, 64)
    h = G.create(lib, e)
    assert h
    try:
        assert lib.mi355_sws_scale_frames_dev(C.c_void_p(h), buf, 1, None) == -1
        assert lib.mi355_sws_scale(C.c_void_p(h), src, ss, buf, 192) == -1
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))


# ---- the describers on live contexts ---------------------------------------------------------------------------------------------------
@needs_sources
def test_describers_on_live_contexts(ref):
    lib = ref.lib
    flags = lib.ref_sws_flags_word(1, 1, 1)
    for name in G.NAMES:
        c = ref.open(name)
        e = ref.describe_range(c)
        assert ref.declined_by_the_old_describers(c), name
        ref.free(c)
        assert e is not None and e.range == G.direction(name) and e.layout == G.LAYOUTS.get(G.cfg(name)[4], 0), name
    declined = [
        (64, 48, "yuv420p", 1, 64, 48, "yuv420p", 1, flags),                    # yuvj420p -> yuvj420p: a plane copy
        (96, 40, "yuv420p", 1, 64, 40, "yuv420p", 0, (flags & ~0x7) | 0x1),     # SWS_FAST_BILINEAR with range
        (96, 40, "yuv420p", 0, 64, 40, "yuv420p", 1, (flags & ~0x7) | 0x1),
        (96, 40, "yuv420p", 1, 64, 40, "bgr24", 0, flags),                      # range to bgr24
        (96, 40, "yuv420p", 1, 64, 40, "yuv440p", 0, flags),                    # 4:4:0
        (96, 40, "yuv420p", 1, 64, 40, "yuv420p10le", 0, flags),                # a 10-bit destination: the 8-bit converters (dstBpc <= 15), no kernel for it
        (96, 40, "yuv420p", 1, 64, 40, "yuv420p16le", 0, flags),                # 16-bit destinations hold the ...Jpeg16_c forms (int32 samples): never called
        (96, 40, "yuv420p", 0, 64, 40, "yuv420p16le", 1, flags),
        (64, 48, "yuv420p", 1, 64, 48, "gray16le", 0, flags),
    ]
    for args in declined:
        c = ref.open_ranges(*args)
        assert ref.describe_range(c) is None, args
        ref.free(c)
    # yuvj420p -> rgb24 keeps its answer: the range is in the LUTs, the same entry through the old describer
    c = ref.open_ranges(128, 96, "yuv420p", 1, 64, 48, "rgb24", 0, flags)
    e, old = ref.describe_range(c), ref.describe_fmt(c)
    ref.free(c)
    assert e is not None and old is not None and e.range == 0 and e.fmt == 0 and V.Entry.same(e, old)
    # same-range contexts answer as through mi355_sws_describe_fmt
    for name in ("v_420_down2", "v_rgb_down2", "k_split"):
        vref = V.Ref(lib)
        c = vref.open(name)
        e, old = ref.describe_range(c), vref.describe(c)
        ref.free(c)
        assert e is not None and e.range == 0 and V.Entry.same(e, old), name


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return G.Ref(P.bind(G.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", G.BINDING)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = G.picture(name, "ramp", seed=5, pad=3)
    sizes = G.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    # the binding's describer knows every one of them, the refused one too (the creator refuses it, not the describer)
    c = hooked.open(name)
    e = hooked.describe_range(c)
    hooked.free(c)
    assert e is not None and e.range == G.direction(name), name
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    # a refused context is left to the reference: the picture counter does not move
    assert lib.ref_sws_pictures() == before + (1 if name in G.TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls
    assert not any(G.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("name", G.BINDING)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = G.picture(name, "noise", seed=6, pad=3)
    sizes = G.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_tier1_calls() > before, name
    assert lib.ref_sws_pictures() == pics
    assert not any(G.differing_rows(got, want, sizes)), name


def test_binding_forwards_the_range_converters(hooked, monkeypatch):
    """with MI355_SWS_LINES=1 a ranged context makes more line calls than its same-range twin: one luma and one chroma conversion per line"""
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    lib = hooked.lib
    name = "t_420_down2"
    planes = G.picture(name, "noise", seed=7)
    sizes = G.stored_entry(name).out_sizes()
    counts = []
    for opener in (hooked.open, hooked.open_twin):
        c = opener(name)
        before = lib.ref_sws_tier1_calls()
        hooked.scale_ctx(c, planes, sizes)
        counts.append(lib.ref_sws_tier1_calls() - before)
        hooked.free(c)
    sh, ch = G.cfg(name)[1], -(-G.cfg(name)[1] // 2)
    assert counts[0] == counts[1] + sh + ch, counts
