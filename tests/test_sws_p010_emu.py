"""CPU: P010 sources (p010le, MI355_SWS_SRC_P010) of the device swscale path through the emulated product library.

The table of tests/sws_p010.py must reach what its census lists (asserted from the plan, source, source-layout, destination, range and depth queries).
Every taken entry equals the reference's own sws_scale() of the same buffers through Tier 1 and through a guarded four-frame Tier-2 batch whose two
source planes lie on 16-byte multiples, on 4-byte multiples that are none of 16 and — the pair plane — at an address 2 mod 4 with a stride 2 mod 4, at
line pads of 0, 1, 4 and 3 samples, on noise, a ramp, all 0, all 0xFFFF and a checkerboard over the full uint16_t range; without the reference, a P010
context equals the device context of the SAME descriptor as a yuv420p10le source on the de-interleaved word >> 6 planes; the line entries equal the
byte table written out; the creators refuse what the header lists, and the table's refused rows are those of the planar 10-bit twin; the describer
reproduces every committed entry from a live reference context; the binding runs whole pictures on the device and forwards the two input converters
under MI355_SWS_LINES=1.

There is no FATE row: the reference has no fate-pixfmt-p010le pin, because it cannot write P010."""
import os

import numpy as np
import pytest

import sws_planar as P
import sws_p010 as Z
import sws_sources as X

HAVE_REF_LIB = os.path.exists(Z.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        Z.make_fresh("_ref/libswsref.so")
    return Z.Ref(P.bind(Z.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: Z.plan(emu.lib, Z.stored_entry(name)) for name in Z.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_form(plans):
    taken = {n: plans[n] for n in Z.NAMES if plans[n] is not None}
    for n, p in taken.items():
        dst = Z.cfg(n)[5]
        assert (p["depth"], p["hsub"], p["vsub"], p["layout"]) == (10, 1, 1, Z.LAYOUT), (n, p)
        assert (p["format"], p["dst_depth"]) == Z.DSTS[dst][:2] and p["range"] == Z.expected_range(n), (n, p)
        # never IDENT1_* or C24, as for every deep source: the tile kernels alone
        assert p["kernel"].startswith(("generic_", "planar_")), (n, p)
    kernels = {p["kernel"] for p in taken.values()}
    assert kernels == {"generic_a", "generic_b", "generic_c", "planar_a", "planar_b", "planar_c"}, kernels
    # equal size to packed destinations runs the tile kernel
    assert taken["p_rgb_same"]["kernel"].startswith("generic") and taken["p_bgra_same_w126"]["kernel"].startswith("generic")
    # every packed destination form: rgb24, bgr24, 32-bit orders, packed 4:2:2 orders
    generic = {Z.DSTS[Z.cfg(n)[5]][0] for n, p in taken.items() if p["kernel"].startswith("generic")}
    assert generic >= {0, 32, 33, 34, 35, 48, 49, 50}, generic
    # the wide and the narrow store, in both families
    for fam in ("generic", "planar"):
        assert {p["narrow"] for p in taken.values() if p["kernel"].startswith(fam)} == {0, 1}, fam
    # staged and unstaged contexts
    assert {p["hstaged"] for p in taken.values()} == {0, 1}
    # SEMI (both pair orders), all three ranges, the three depths, the FULL form
    assert {p["format"] for p in taken.values() if p["planes"] == 2} == {16, 17}
    assert {p["range"] for p in taken.values()} == {0, 1, 2}
    assert {p["dst_depth"] for p in taken.values()} == {8, 9, 10}
    assert {p["format"] for p in taken.values() if p["planes"] == 3} == {1, 2, 3}
    # a range to a packed 4:2:2 destination
    assert taken["y_yvyuj_down2"]["range"] == Z.TO_JPEG and taken["y_yvyuj_down2"]["format"] == 50
    # odd widths: under a filter, and with identity luma
    assert any(Z.cfg(n)[0] % 2 and Z.cfg(n)[:2] == Z.cfg(n)[2:4] for n in taken) and any(Z.cfg(n)[0] % 2 and Z.cfg(n)[:2] != Z.cfg(n)[2:4] for n in taken)
    # the batch's planes hit the three alignment classes, both planes; frames 1 and 3: the pair plane at an address 2 mod 4 with a stride 2 mod 4
    for plane in (0, 1):
        assert {Z.align_class(*Z.src_layouts(n)[f][plane]) for n in taken for f in range(4)} == {16, 4, 2}, plane
    for n in taken:
        lay = Z.src_layouts(n)
        for f in (1, 3):
            o, st = lay[f][1]
            assert o % 4 == 2 and st % 4 == 2, (n, f)
        assert all(Z.align_class(o, st) == 4 for o, st in lay[2]) or Z.cfg(n)[0] % 2, n
    assert any(all(Z.align_class(o, st) == 16 for o, st in Z.src_layouts(n)[0]) for n in taken)
    assert Z.SRC_PADS == (0, 1, 4, 3)


def test_refused_entries_are_those_of_the_planar_twin(emu, plans):
    """REFUSED is derived from the twin (the same descriptor with src_layout 0, depth 10, shifts 1, 1), and P010 is refused exactly there; a taken row
    has its twin's plan, narrow / hstage report included"""
    twin = Z.refused_by_the_twin(emu.lib)
    assert twin == Z.REFUSED, twin
    assert {n for n, p in plans.items() if p is None} == Z.REFUSED
    assert Z.REFUSED == {"g_420_vdown16", "p_rgb_vdown16"}
    assert Z.REFUSED_CAP == X.REFUSED_CAP and len(Z.REFUSED) * Z.REFUSED_CAP <= len(Z.NAMES), (len(Z.REFUSED), len(Z.NAMES))
    for n in Z.TAKEN:
        t = Z.plan(emu.lib, Z.twin_entry(Z.stored_entry(n)))
        assert t["layout"] == 0 and plans[n]["layout"] == Z.LAYOUT, n
        for k in Z.TWIN_KEYS:
            assert plans[n][k] == t[k], (n, k, plans[n], t)


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    """every row is opened by the reference (open_formats asserts it) and described as the table expects; the committed arrays are those"""
    for name in Z.SHAPES:
        assert Z.stored_entry(name).same(ref.entry(name)), name


@needs_sources
def test_described_contexts_have_the_banks_of_their_yuv420p10le_twins(ref):
    """the descriptor mi355_sws_describe_p010 fills is the one the matching describer fills for the yuv420p10le context of the same sizes, ranges,
    destination and flags; every other describer declines the P010 context"""
    import sws_nvsrc as V
    for name in Z.NAMES:
        e = ref.entry(name)
        c = ref.open(name)
        assert ref.declined_by_the_nine_describers(c) and ref.describe_yuy2dst(c) is None, name
        ref.free(c)
        c = ref.open_twin(name)
        t = ref.describe_twin(name, c)
        assert ref.describe_p010(c) is None, name                                   # ... and this one declines the twin
        ref.free(c)
        if t is None:
            # at equal size to a planar destination of the same subsampling the reference converts yuv420p10le with planarCopyWrapper — no scaler
            # context, no banks — where P010 is kept off it (swscale_unscaled.c:1162-1167): the P010 row has no live twin to compare with
            assert Z.cfg(name)[:2] == Z.cfg(name)[2:4] and Z.cfg(name)[5] in ("420", "420p10") and not Z.expected_range(name), name
            continue
        assert (t.depth, t.hsub, t.vsub, t.layout, t.fmt) == (10, 1, 1, 0, e.fmt), name
        assert e.ctx.ints == t.ctx.ints and V.same_banks(e, t), name
        assert all((np.asarray(e.ctx.luts[k]) == np.asarray(t.ctx.luts[k])).all() for k in P.S.LUTS), name
        assert (e.dither == t.dither).all(), name
    flags = ref.lib.ref_sws_flags_word(1, 1, 1)
    for args in ((96, 40, b"p010be", 64, 40, b"yuv420p", flags),                     # big endian
                 (96, 40, b"p010le", 64, 40, b"yuva420p", flags),                    # YUVA
                 (96, 40, b"p010le", 64, 40, b"rgb565le", flags),
                 (96, 40, b"p010le", 64, 40, b"bgra", flags | 0x2000),               # SWS_FULL_CHR_H_INT
                 (96, 40, b"nv12", 64, 40, b"yuv420p", flags)):
        c = ref.open_formats(*args)
        assert ref.describe_p010(c) is None, args
        ref.free(c)


# ---- parity with the reference ------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("kinds", [("noise", "ramp", "ones"), ("checker", "zeros", "noise")])
@pytest.mark.parametrize("name", Z.TAKEN)
def test_emulated_batched(emu, ref, plans, name, kinds):
    p = Z.check_batch(emu.lib, ref, name, e=Z.stored_entry(name), kinds=kinds)
    assert p is not None and p == plans[name], name


@needs_ref
@pytest.mark.parametrize("name", Z.TAKEN)
def test_emulated_tier1_matches_reference(emu, ref, name):
    Z.check_tier1(emu.lib, ref, name, Z.tier1_pictures(name, seed=11))


# ---- the twin property: no reference needed -------------------------------------------------------------------------------------------
# at least one row per kind (PLAIN, RANGE, DEEP), per planar form (HALF, FULL, SEMI) and per packed destination form
TWINS = ["g_420_down2", "g_odd", "g_444_oddw_same", "g_nv21_down2", "g_j420_same", "g_full_420_down2", "g_420p10_same", "g_444p9_w129_up", "g_420_hdown4",
         "p_rgb_same", "p_bgr_w257_up", "p_rgba_w384_up", "y_uyvy_down2", "y_yvyuj_down2"]


@pytest.mark.parametrize("name", TWINS)
def test_p010_context_equals_its_planar_twin_on_the_shifted_planes(emu, name):
    """the device context of layout 24 on a P010 picture against the device context created from the SAME descriptor as a yuv420p10le source on the
    de-interleaved word >> 6 planes: byte for byte, with the same plan"""
    e = Z.stored_entry(name)
    assert Z.plan(emu.lib, e)["kernel"] == Z.plan(emu.lib, Z.twin_entry(e))["kernel"]
    for what, seed in (("noise", 3), ("ramp", 4), ("ones", 5)):
        pic = Z.picture(name, what, seed=seed, pad=3)
        want = Z.run_tier1(emu.lib, Z.twin_entry(e), Z.planar_twin_planes(name, pic))
        got = Z.run_tier1(emu.lib, e, pic)
        assert all((g == w).all() for g, w in zip(got, want)), (name, what)


def test_the_twin_table_covers_every_kind_and_form():
    rows = {n: (Z.cfg(n), Z.DSTS[Z.cfg(n)[5]]) for n in TWINS}
    planar = {n for n, (c, d) in rows.items() if 1 <= d[0] <= 17}
    assert {d[1] > 8 for n, (c, d) in rows.items() if n in planar} == {False, True}                  # DEEP and not
    assert any(Z.expected_range(n) for n in planar) and any(not Z.expected_range(n) for n in planar)    # RANGE and PLAIN
    assert {d[0] for n, (c, d) in rows.items() if n in planar} >= {1, 3, 17}                           # HALF, FULL, SEMI
    assert {min(d[0], 48) if d[0] >= 48 else min(d[0], 33) for n, (c, d) in rows.items() if n not in planar} == {0, 32, 33, 48}      # the four packed forms


# ---- the line entries: no reference needed -----------------------------------------------------------------------------------------
def test_line_entries_match_the_byte_table_written_out(emu):
    assert Z.LINE_WIDTHS == (1, 7, 64, 131)
    assert Z.check_line_entries(emu.lib) == 4 * 2 * 2


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
_E420, _ERGB = "g_420_down2", "p_rgb_down2"
_CASES = [c[0] for c in Z.refusal_cases(Z.stored_entry(_E420), Z.stored_entry(_ERGB))] if os.path.exists(Z.CONTEXTS) else []


def test_the_bases_of_the_refusal_cases_are_taken(emu):
    a, b = Z.plan(emu.lib, Z.stored_entry(_E420)), Z.plan(emu.lib, Z.stored_entry(_ERGB))
    assert a["kernel"].startswith("planar") and b["kernel"].startswith("generic") and a["layout"] == b["layout"] == 24
    # the forwarding creators take the layout: a range and a depth
    assert Z.plan(emu.lib, Z.stored_entry("g_j420_same"))["range"] == 2 and Z.plan(emu.lib, Z.stored_entry("g_420p10_same"))["dst_depth"] == 10


@pytest.mark.parametrize("what", _CASES)
def test_creators_refuse(emu, what):
    cases = {c[0]: c for c in Z.refusal_cases(Z.stored_entry(_E420), Z.stored_entry(_ERGB))}
    _, e, alpha = cases[what]
    assert not Z.create(emu.lib, e, alpha), what


def test_tier1_refuses_an_odd_stride(emu):
    Z.check_odd_stride_refused(emu.lib)


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return Z.Ref(P.bind(Z.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", Z.BINDING)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    """whole pictures go through mi355_swsfunc to the device (the picture counter moves); a context the creators refuse is left to the reference"""
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = Z.picture(name, "ramp", seed=5, pad=3)
    sizes = Z.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    c = hooked.open(name)
    e = hooked.describe(c)
    hooked.free(c)
    assert e is not None and e.layout == Z.LAYOUT, name                                  # (the creator refuses a row, not the describer)
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_pictures() == before + (1 if name in Z.BINDING_TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls, name
    assert not any(Z.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("name", Z.BINDING)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    """MI355_SWS_LINES=1: c->lumToYV12 / c->chrToYV12 go to mi355_sws_p010ToY / _p010ToUV (the call counter moves), whole pictures stay the reference's"""
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = Z.picture(name, "noise", seed=6, pad=3)
    sizes = Z.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_tier1_calls() > before, name
    assert lib.ref_sws_pictures() == pics
    assert not any(Z.differing_rows(got, want, sizes)), name
