"""CPU: SWS_FAST_BILINEAR contexts (mi355_sws_create_fast_bilinear) of the device swscale path through the emulated product library.

The table of tests/sws_fastbl.py must reach what its census lists: every instance of k_sws_fbl_generic / k_sws_fbl_planar the emulated library holds
(read from its symbol table), both padding classes and all three fetch forms, both "reads x = srcW" classes per plane.  Every row equals the
reference's own sws_scale() of the same buffers — the committed fixture — through a guarded four-frame Tier-2 batch and through Tier 1; without any
fixture, every row whose increments never reach x = srcW equals the EXISTING creator's context on the equivalent two-tap banks; the line entries equal
the numpy restatement of the two formulas; the creator refuses what the header lists and the queries follow the twin rule.  With the reference's
sources: the committed fixture is what the reference gives today, the eleven existing describers answer as before, and the binding runs
them on the device."""
import re
import subprocess

import numpy as np
import pytest

import sws_fastbl as F
import sws_instances as I
import sws_planar as P

needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    F.make_fresh("_ref/libswsref.so")
    return F.Ref(P.bind(F.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: F.plan(emu.lib, F.stored_entry(name)) for name in F.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def fbl_instances(path=I.EMU_LIB):
    """the instances of the two new kernels in the library at `path`, as launch keys: ("generic", i, dst form) / ("planar", i, form, kind)"""
    out = subprocess.run(["nm", "-C", path], capture_output=True, text=True, check=True).stdout
    keys = set()
    for kernel, args in set(re.findall(r"::k_sws_fbl_(generic|planar)<([^<>]*)>\(", out)):
        a = [s.strip() for s in args.split(",")]
        flag = lambda s: {"true": True, "false": False}[s]                          # noqa: E731
        if kernel == "generic":                                                      # LCAP, CCAP, WAVES, DST
            keys.add(("generic", I.SHAPES["generic"].index((int(a[0]), int(a[1]))), I.DST_FORMS[int(a[3])]))
        else:                                                                        # LCAP, CCAP, CW, SEMI, RANGE, DEEP
            form = "SEMI" if flag(a[3]) else ("FULL" if int(a[2]) == F.TW else "HALF")
            keys.add(("planar", I.SHAPES["planar"].index((int(a[0]), int(a[1]))), form, "DEEP" if flag(a[5]) else ("RANGE" if flag(a[4]) else "PLAIN")))
    return keys


def key_of(p):
    """the instance a plan launches (sws_key() of sws.hip restated for these contexts)"""
    fam, i = p["kernel"].split("_")
    i = "abc".index(i)
    if fam == "generic":
        fmt = p["format"]
        return ("generic", i, "rgb24" if fmt == 0 else ("bgr24" if fmt == 32 else ("yuy2" if fmt >= 48 else "rgb32")))
    form = "SEMI" if p["planes"] == 2 else ("FULL" if p["format"] == 3 else "HALF")
    return ("planar", i, form, "DEEP" if p["dst_depth"] > 8 else ("RANGE" if p["range"] else "PLAIN"))


def test_the_new_kernels_have_names_of_their_own(emu):
    """12 packed-destination and 24 planar instances; the five pinned kernels keep their instance space (tests/test_sws_instances_emu.py counts it)"""
    keys = fbl_instances()
    assert len([k for k in keys if k[0] == "generic"]) == 12 and len([k for k in keys if k[0] == "planar"]) == 24, sorted(keys)
    assert {k[2] for k in keys if k[0] == "generic"} == {"rgb24", "bgr24", "rgb32", "yuy2"}
    assert ("planar", 0, "SEMI", "DEEP") not in keys


def test_table_reaches_every_instance_and_class(emu, plans):
    assert all(p is not None for p in plans.values()), [n for n, p in plans.items() if p is None]
    for n, p in plans.items():
        dst = F.cfg(n)[6]
        assert (p["fast"], p["layout"], p["alpha"], p["depth"], p["hstage"]) == (1, 0, 0, 8, 1), (n, p)
        assert (p["hsub"], p["vsub"]) == F.SUBS[F.cfg(n)[4]] and (p["format"], p["dst_depth"]) == F.DSTS[dst][:2] and p["range"] == F.expected_range(n), (n, p)
        assert p["kernel"].startswith(("generic_", "planar_")), (n, p)                    # never IDENT1_*, C24 or a packer
    # every instance of the two new kernels, as the emulated library's symbol table lists them
    assert {key_of(p) for p in plans.values()} == fbl_instances()
    # every destination form of the header's list
    assert {p["format"] for p in plans.values() if p["planes"] == 1} == {0, 32, 33, 34, 35, 36, 48, 49, 50}
    assert {(p["format"], p["dst_depth"]) for p in plans.values() if p["planes"] == 3} >= {(1, 8), (2, 8), (3, 8), (1, 10), (2, 9), (3, 10)}
    assert {p["format"] for p in plans.values() if p["planes"] == 2} == {16, 17}
    # both ranges to a planar and to a packed 4:2:2 destination
    for rng in (F.FROM_JPEG, F.TO_JPEG):
        assert {p["planes"] > 1 for p in plans.values() if p["range"] == rng} == {False, True}, rng
    # the wide and the narrow store in both families; staged contexts, and one whose full tiles take the direct form
    for fam in ("generic", "planar"):
        assert {p["narrow"] for p in plans.values() if p["kernel"].startswith(fam)} == {0, 1}, fam
    d = F.stored_entry("down_420_abgr_w260").ctx.desc
    assert d.srcW * F.TW // d.dstW > 4 * 76                                               # a full tile's span against the staged line (SRC_DW dwords)
    # both "reads x = srcW" classes, per plane
    behind = [F.stored_entry(n).reads_behind() for n in F.NAMES]
    assert {b[0] for b in behind} == {False, True} and {b[1] for b in behind} == {False, True}
    # ... with a != 0 at the last column (the byte behind the line is part of the result) and with a == 0 (equal width: weight 0)
    e = F.stored_entry("up_420_rgb24_w130")
    assert F.positions(130, e.lum_inc)[1][-1] != 0 and F.positions(96, F.stored_entry("same_444_rgb24").lum_inc)[1][-1] == 0
    assert F.stored_entry("same_444_rgb24").lum_inc == 65536 and list(F.positions(128, F.stored_entry("up2_420_420").lum_inc)[1][:4]) == [0, 64, 0, 64]
    # the padding classes: stride = width + 1, 16-aligned planes with a wider stride, stride == width; and the three fetch forms per plane
    assert set(F.PADS) == {"al16", "plus1", "tight"}
    for plane in (0, 1):
        assert {F.align_class(*F.src_layouts(n)[f][plane]) for n in F.NAMES for f in range(4)} == {16, 4, 1}, plane
    for n in F.NAMES:
        lay = F.src_layouts(n)
        assert all(F.align_class(o, st) == 16 and st >= w + 16 for (o, st), (w, _) in zip(lay[0], F.plane_dims(n))), n
        assert all(st == w + 1 for (o, st), (w, _) in zip(lay[1], F.plane_dims(n))) and all(st == w for (o, st), (w, _) in zip(lay[2], F.plane_dims(n))), n
    # x = srcW read on a tight plane of 16-byte multiples (the width a multiple of 16): the piece that starts at the stride, luma and chroma
    for plane in (0, 1):
        assert any(F.align_class(*F.src_layouts(n)[2][plane]) == 16 and F.stored_entry(n).reads_behind()[min(plane, 1)] for n in F.NAMES), plane
    # a 128-pixel tile boundary with a short last tile; an odd width; one output row
    assert F.cfg("up_420_rgb24_w130")[2] == 130 and F.cfg("odd_422_bgra")[2] % 2 == 1 and F.cfg("up_420_rgb24_h1")[3] == 1


def test_a_third_of_the_rows_cross_check_and_a_third_do_not():
    q = [n for n in F.NAMES if F.qualifies(n)]
    assert 3 * len(q) >= len(F.NAMES) and 3 * (len(F.NAMES) - len(q)) >= len(F.NAMES), (len(q), len(F.NAMES))
    # the synthetic entries have the increments the reference's plain-C init leaves (the committed ones)
    for n in F.NAMES:
        e, s = F.stored_entry(n), F.synth_entry(n)
        assert (e.lum_inc, e.chr_inc, e.ctx.ints) == (s.lum_inc, s.chr_inc, s.ctx.ints), n
        assert e.ctx.desc.hLum.n == 0 and e.ctx.desc.hChr.n == 0 and e.ctx.desc.vLum.size in (1, 2), n      # no horizontal bank is stored; the vertical banks of utils.c:296
    assert {F.stored_entry(n).ctx.desc.vLum.size for n in F.NAMES} == {1, 2}


# ---- parity with the reference: the committed fixture --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.NAMES)
def test_emulated_batched(emu, plans, name):
    p = F.check_batch(emu.lib, name)
    assert p == plans[name], name


@pytest.mark.parametrize("name", F.NAMES)
def test_emulated_tier1(emu, name):
    F.check_tier1(emu.lib, name)


@needs_sources
def test_committed_fixture_matches_the_reference(ref):
    """every row is opened by the reference with SWS_FAST_BILINEAR and taken by mi355_sws_describe_fast; the committed arrays and hashes are those"""
    for name in F.NAMES:
        e = ref.entry(name)
        assert F.stored_entry(name).same(e), name
        sizes = e.out_sizes()
        got = [bytes(F.planes_hash(ref.scale(name, planes, sizes), sizes)) for planes in F.frames(name)]
        assert got == F.stored_hashes(name), name
    # the byte behind the line is part of the reference's result: the same picture in two padding classes differs
    name = "up_420_rgb24_w130"
    assert F.stored_hashes(name)[0] != F.stored_hashes(name)[3]


@needs_sources
def test_the_existing_describers_keep_declining(ref):
    """a fast-bilinear context: the describers answer what they answered before — ten decline, and mi355_sws_describe, which looks at the two formats
    alone, takes yuv420p -> rgb24 as ever (the binding asks the new describer first) — and the new one takes it; the same context without the flag: the
    new one declines, one of the others takes it"""
    for name in F.NAMES:
        first = F.cfg(name)[4] == "420" and F.cfg(name)[6] == "rgb24"
        c = ref.open(name)
        assert ref.declined_by_the_ten_describers(c) and ref.first_describer_takes(c) == first, name
        assert ref.describe_fast(c) is not None, name
        assert ref.declined_by_the_ten_describers(c) and ref.first_describer_takes(c) == first, name      # ... and the context is left as it was
        ref.free(c)
        c = ref.open(name, fast=False)
        assert ref.describe_fast(c) is None and (first or not ref.declined_by_the_ten_describers(c)), name
        ref.free(c)
    flags = ref.flags()
    for args in ((96, 40, b"nv12", 128, 40, b"yuv420p", flags),                          # the sources that stay the reference's
                 (96, 40, b"rgb24", 128, 40, b"yuv420p", flags),
                 (96, 40, b"yuyv422", 128, 40, b"yuv420p", flags),
                 (96, 40, b"rgba", 128, 40, b"yuv420p", flags),
                 (96, 40, b"yuv420p10le", 128, 40, b"yuv420p", flags),                   # (no fast pass in the reference: srcBpc 10)
                 (96, 40, b"yuva420p", 128, 40, b"rgba", flags),                         # YUVA
                 (96, 40, b"yuv420p", 128, 40, b"rgb565le", flags),
                 (96, 40, b"yuv420p", 128, 40, b"bgra", flags | 0x2000)):                # SWS_FULL_CHR_H_INT
        c = ref.open_formats(*args)
        assert ref.describe_fast(c) is None, args
        ref.free(c)


# ---- the independent cross-check: no fixture, no reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in F.NAMES if F.qualifies(n)])
def test_equals_the_existing_creator_on_two_tap_banks(emu, name):
    F.check_cross(emu.lib, name)


# ---- the line entries ----------------------------------------------------------------------------------------------------------------
def test_line_entries_match_the_numpy_restatement(emu):
    assert F.LINE_WIDTHS == (1, 2, 127, 128, 129) and set(F.LINE_INCS) >= {65536, 32768, 131072} and sum(i % 2 for i in F.LINE_INCS) == 2
    assert F.check_line_entries(emu.lib) == 5 * 5 * 2


def test_the_numpy_restatement_is_the_two_formulas():
    src = np.array([10, 200, 77, 0], np.uint8)
    assert F.hyscale_fast(src, 3, 40000).tolist() == [1280, 16100, 22156]              # xx, a: 0, 0 / 0, 78 / 1, 28
    assert F.hcscale_fast(src, 3, 40000).tolist() == [1270, 16090, 21956]
    assert F.hcscale_fast(src, 3, 65536).tolist() == [10 * 127, 200 * 127, 77 * 127] and F.hyscale_fast(src, 3, 65536).tolist() == [10 << 7, 200 << 7, 77 << 7]


# ---- refusals and queries --------------------------------------------------------------------------------------------------------------
_CASES = [c[0] for c in F.refusal_cases()]


@pytest.mark.parametrize("what", _CASES)
def test_creator_refuses(emu, what):
    e = dict(F.refusal_cases())[what]
    assert not F.create(emu.lib, e), what


def test_the_bases_of_the_refusal_cases_are_taken_and_the_twin_refuses_with_it(emu):
    for n in ("up2_420_420", "up_420_rgb24_w130"):
        assert F.plan(emu.lib, F.synth_entry(n))["fast"] == 1, n
    cases = dict(F.refusal_cases())
    for what in ("range 3", "range to rgb24", "depth 10 to rgb24", "depth 11", "depth 10 with a range", "format 7", "vertical banks of 64 taps"):
        assert F.twin_plan(emu.lib, cases[what]) is None, what                            # a refusal of the twin's
    for what in ("lumXInc 0", "luma two samples behind the line", "chroma position over 32 bits"):
        assert F.twin_plan(emu.lib, cases[what]) is not None, what                        # a refusal of this creator's own


def test_queries_follow_the_twin_rule(emu, plans):
    for n in F.NAMES:
        e = F.stored_entry(n)
        t = F.twin_plan(emu.lib, e)
        assert t is not None and (t["fast"], t["lum_inc"], t["chr_inc"]) == (0, 0, 0), n     # the existing creators answer as before
        for k in F.TWIN_KEYS:
            assert plans[n][k] == t[k], (n, k, plans[n], t)
        assert (plans[n]["fast"], plans[n]["lum_inc"], plans[n]["chr_inc"]) == (1, e.lum_inc, e.chr_inc), n
    emu.lib.mi355_sws_fast_bilinear.argtypes = [F.C.c_void_p] * 3
    assert emu.lib.mi355_sws_fast_bilinear(None, None, None) == -1


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
BINDING = ["up_420_rgb24_w130", "up2_420_420", "odd_422_bgra", "down_444_yuyv", "same_420_444", "up_420_nv12", "up_420_420p10", "fromjpeg_up_420_420",
           "tojpeg_up_422_yuyv", "c0_420_rgb24"]


@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return F.Ref(P.bind(F.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", BINDING)
def test_binding_whole_pictures(hooked, name, monkeypatch):
    """whole pictures of a fast-bilinear context go through mi355_swsfunc to the device (the picture counter moves) and are the reference's bytes"""
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = F.stored_entry(name)
    sizes, planes = e.out_sizes(), F.frames(name)[1]
    lib = hooked.lib
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_pictures() == before + 1 and lib.ref_sws_tier1_calls() == calls, name
    assert bytes(F.planes_hash(got, sizes)) == F.stored_hashes(name)[1], name


@pytest.mark.parametrize("name", BINDING)
def test_binding_inner_loops(hooked, name, monkeypatch):
    """MI355_SWS_LINES=1: c->hyscale_fast / c->hcscale_fast go to mi355_sws_hyscale_fast / _hcscale_fast (the call counter moves)"""
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    e = F.stored_entry(name)
    sizes, planes = e.out_sizes(), F.frames(name)[2]
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_tier1_calls() >= before + e.ctx.desc.srcH + e.ctx.desc.chrSrcH and lib.ref_sws_pictures() == pics, name      # one call a source line
    assert bytes(F.planes_hash(got, sizes)) == F.stored_hashes(name)[2], name
