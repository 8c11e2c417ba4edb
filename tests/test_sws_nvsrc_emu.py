"""CPU: NV12 / NV21 sources of the device swscale path and the unscaled NV12 / NV21 -> yuv420p splitter through the emulated product library.

The table of tests/sws_nvsrc.py must reach what its census lists (asserted from the plan, source, source-layout and destination queries).
Every entry equals the reference's own sws_scale() of the NV picture through Tier 1 (noise, the checkerboard, both colour-split pictures) and
through a guarded four-frame Tier-2 batch whose pair planes lie on a 16-byte multiple, on a 4-byte multiple and on an odd address; the
committed contexts are the reference's and their banks those of the yuv420p twin; the creator refuses what lies outside the list; the
binding takes the scaled contexts in both of its forms and leaves the splitter to the reference (oracle/_ref/libswsref_tier1.so)."""
import ctypes as C
import os

import pytest

import sws_nvsrc as V
import sws_planar as P
import sws_sources as X

HAVE_REF_LIB = os.path.exists(V.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        V.make_fresh("_ref/libswsref.so")
    return V.Ref(P.bind(V.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: V.plan(emu.lib, V.stored_entry(name)) for name in V.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_what_the_issue_lists(plans):
    got = {n: p for n, p in plans.items() if p}
    cfgs = {n: V.cfg(n) for n in V.NAMES}
    for n, p in got.items():
        sw, sh, dw, dh, src, dst = cfgs[n][:6]
        assert (p["depth"], p["hsub"], p["vsub"], p["layout"]) == (8, 1, 1, V.LAYOUTS[src]), (n, p)
        assert p["format"] == V.DSTS[dst] and p["planes"] == {"rgb": 1, "nv12": 2, "nv21": 2}.get(dst, 3), (n, p)
        if p["kernel"] == "nv12_split":
            assert n in V.SPLIT and (p["chr_bytes"], p["chr_rows"]) == (sw // 2, sh // 2), (n, p)
        else:
            assert n not in V.SPLIT, (n, p)
    fam = lambda *dsts: {n: p for n, p in got.items() if cfgs[n][5] in dsts and n not in V.SPLIT}      # noqa: E731
    rgb, planar, semi = fam("rgb"), fam("420", "422", "444"), fam("nv12", "nv21")
    split = {n: p for n, p in got.items() if n in V.SPLIT}
    assert {p["kernel"] for p in rgb.values()} == {"ident1_1", "ident1_x", "generic_a", "generic_b", "generic_c"}
    assert {p["kernel"] for p in {**planar, **semi}.values()} == {"planar_a", "planar_b", "planar_c"}
    assert {p["kernel"] for p in planar.values()} == {"planar_a", "planar_b", "planar_c"} and {p["kernel"] for p in semi.values()} >= {"planar_a", "planar_b"}
    assert split and {p["kernel"] for p in split.values()} == {"nv12_split"}
    for group in (rgb, planar, semi):
        assert {p["hstaged"] for p in group.values()} == {0, 1}
        assert {p["narrow"] for p in group.values()} == {0, 1}
    # both layouts in each destination family and in the splitter
    for group in (rgb, planar, semi, split):
        assert {cfgs[n][4] for n in group} == {"nv12", "nv21"}, sorted(group)
    # CW = TW / 2, CW = TW and SEMI
    assert {cfgs[n][5] for n in planar} == {"420", "422", "444"} and {cfgs[n][5] for n in semi} == {"nv12", "nv21"}
    # odd srcW, srcH, dstW and dstH
    scaled = {**rgb, **planar, **semi}
    for k in range(4):
        assert any(cfgs[n][k] % 2 for n in scaled), k
    assert any(cfgs[n][0] % 2 for n in split) and any(cfgs[n][1] % 2 for n in split)
    # identity and filtered chroma banks; filtered ones of every tap bucket of the staged pass (2, 4, 8 in registers, more from memory) and
    # a tile that takes the direct pass
    hcs = {n: V.stored_entry(n).ctx.desc.hChr.size for n in scaled}
    bucket = lambda s: 2 if s <= 2 else (4 if s <= 4 else (8 if s <= 8 else 0))      # noqa: E731
    assert any(s == 1 for s in hcs.values()) and {bucket(s) for n, s in hcs.items() if s > 1 and got[n]["hstaged"]} == {2, 4, 8, 0}
    assert any(hcs[n] > 1 and got[n]["hstage"] and not got[n]["hstaged"] for n in scaled)
    # the batch's pair planes hit all three alignment classes
    for n in ("v_rgb_down2", "v_420_down2", "v_nv12_down2", "k_split", "v_idx_w128"):
        assert {V.align_class(o, st) for o, st in V.pair_layouts(n)} == {16, 4, 1}, (n, V.pair_layouts(n))


def test_refused_entries_are_named_and_few(plans):
    refused = {n for n, p in plans.items() if p is None}
    assert refused == V.REFUSED, refused
    assert len(refused) * V.REFUSED_CAP <= len(V.NAMES), (len(refused), len(V.NAMES))
    assert not refused & V.CHAIN


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference_and_the_twins_banks(ref):
    twins = 0
    for name in V.SHAPES:
        e = V.stored_entry(name)
        assert e.same(ref.entry(name)), name
        # the yuv420p context of the same sizes, destination and flags through mi355_sws_describe_src: the same four banks (where the twin
        # runs the generic scaler — not a special converter, the packer or a plane copy)
        c = ref.open_twin(name)
        t = ref.describe_src(c)
        ref.free(c)
        if name in V.SPLIT:
            assert t is None, name                                                  # a plane copy
        elif t is not None and not t.ctx.desc.unscaled_special:
            assert V.same_banks(e, t) and e.ctx.ints == t.ctx.ints, name
            twins += 1
    assert twins >= len(V.SHAPES) - len(V.SPLIT) - 2, twins                         # all but v_noacc_same (yuv2rgb_c_24_rgb) and v_swap_same (the packer)


# ---- parity ------------------------------------------------------------------------------------------------------------------------
TAKEN = [n for n in V.NAMES if n not in V.REFUSED]


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_tier1_matches_reference(emu, ref, name):
    V.check_tier1(emu.lib, ref, name, V.tier1_pictures(name, seed=11))


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_batched(emu, ref, plans, name):
    p = V.check_batch(emu.lib, ref, name, e=V.stored_entry(name))
    assert p is not None and p == plans[name], name


@needs_ref
def test_splitter_leaves_the_rounded_down_rest_alone(emu, ref):
    """the reference's own output says which bytes of the chroma planes stay 0x5A: the last of 26 rows of 70x51, the last byte a row of 71x50"""
    for name, rows, cols in (("k_split_70x51", slice(25, 26), slice(0, 35)), ("k_split_71x50", slice(0, 25), slice(35, 36))):
        e = V.stored_entry(name)
        planes = V.colour_split(name, seed=3)
        want = ref.scale(name, planes, e.out_sizes())
        h = V.create(emu.lib, e)
        try:
            got = V.scale_tier1(emu.lib, h, e, planes)
        finally:
            emu.lib.mi355_sws_destroy(C.c_void_p(h))
        for p in (1, 2):
            assert (want[p][rows, cols] == 0x5A).all() and (got[p][rows, cols] == 0x5A).all(), (name, p)
        assert all((g == w).all() for g, w in zip(got, want)), name


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_creator_refuses_what_is_outside_the_list(emu):
    lib = emu.lib
    e = V.stored_entry("v_rgb_down2")
    assert V.plan(lib, e) is not None
    assert not V.create(lib, e.edited(layout=3)) and not V.create(lib, e.edited(layout=-1))
    assert not V.create(lib, e.edited(depth=10))                                    # depth 10 with layout 1
    assert not V.create(lib, e.edited(vsub=0, chrSrcH=e.ctx.ints["srcH"]))          # shifts 1,0 with layout 1
    for fmt in list(range(4, 16)) + [18]:
        assert not V.create(lib, e.edited(fmt=fmt)), fmt
    # the special converter: the splitter only
    k = V.stored_entry("k_split")
    assert V.plan(lib, k)["kernel"] == "nv12_split"
    assert not V.create(lib, k.edited(fmt=0))                                       # special to rgb24
    assert not V.create(lib, k.edited(fmt=2)) and not V.create(lib, k.edited(fmt=16))
    assert not V.create(lib, k.edited(dstW=62, chrDstW=31)) and not V.create(lib, k.edited(dstH=46))      # special at unequal size
    # the existing entry points still return -1 across context kinds, and the queries on nothing
    lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale_planar_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.mi355_sws_scale_planar.argtypes = [C.c_void_p] * 5
    buf = (C.c_uint8 * 256)()
    src, ss = (C.c_void_p * 3)(C.addressof(buf), C.addressof(buf), None), (C.c_int * 3)(64, 64, 0)
    dst, ds = (C.c_void_p * 3)(C.addressof(buf), C.addressof(buf), C.addressof(buf)), (C.c_int * 3)(64, 32, 32)
    for name, rgb in (("v_rgb_down2", True), ("v_420_down2", False), ("k_split", False)):
        h = V.create(lib, V.stored_entry(name))
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


@needs_ref
def test_layout_0_is_mi355_sws_create_src(emu, ref):
    """the planar layout builds the context mi355_sws_create_src builds: the same plan, the same bytes"""
    name = "r420d8_down"
    x = X.stored_entry(name)
    e = V.Entry(x.ctx, x.depth, x.hsub, x.vsub, x.dither, x.fmt, 0)
    planes = X.picture(name, seed=2, pad=3)
    outs = []
    for make in (lambda: X.create(emu.lib, x), lambda: V.create(emu.lib, e)):
        h = make()
        assert h
        try:
            p = V.plan_of(emu.lib, h)
            outs.append((p, X.scale_tier1(emu.lib, h, x, planes)))
        finally:
            emu.lib.mi355_sws_destroy(C.c_void_p(h))
    assert outs[0][0] == outs[1][0] and outs[0][0]["layout"] == 0
    assert all((a == b).all() for a, b in zip(outs[0][1], outs[1][1]))
    assert not any(X.differing_rows(outs[1][1], X.Ref(ref.lib).scale(name, planes, x.out_sizes()), x.out_sizes()))


# ---- the describers on live contexts ---------------------------------------------------------------------------------------------------
@needs_sources
def test_describers_on_live_contexts(ref):
    lib = ref.lib
    flags = lib.ref_sws_flags_word(1, 1, 1)
    # mi355_sws_describe_src keeps declining every NV source; the new describer answers for the planar ones as it does
    for name in ("v_rgb_down2", "v_420_down2", "v_nv12_down2", "k_split"):
        c = ref.open(name)
        assert ref.describe_src(c) is None and ref.describe(c) is not None, name
        ref.free(c)
    c = X.Ref(lib).open("r422d10_w129_oddw")
    a, b = ref.describe_src(c), ref.describe(c)
    ref.free(c)
    assert a is not None and b is not None and b.layout == 0 and a.same(b)
    declined = [
        (96, 40, b"yuyv422", 64, 40, b"rgb24", flags),                          # a packed source
        (96, 40, b"p010le", 64, 40, b"rgb24", flags),                           # a deeper semi-planar source
        (96, 40, b"gray", 64, 40, b"rgb24", flags),
        (96, 40, b"nv12", 64, 40, b"rgb24", (flags & ~0x7) | 0x1),              # SWS_FAST_BILINEAR
        (96, 40, b"nv21", 64, 40, b"yuv420p", (flags & ~0x7) | 0x1),
        (64, 48, b"nv12", 64, 48, b"nv12", flags),                              # the reference's plain copy
        (96, 40, b"nv12", 64, 40, b"bgr24", flags),
    ]
    for args in declined:
        c = ref.open_formats(*args)
        assert ref.describe(c) is None, args
        ref.free(c)
    # the splitter whatever the flags
    for fl in (flags, lib.ref_sws_flags_word(0, 0, 0), (flags & ~0x7) | 0x1):
        c = ref.open_formats(64, 48, b"nv21", 64, 48, b"yuv420p", fl)
        e = ref.describe(c)
        ref.free(c)
        assert e is not None and (e.layout, e.fmt, e.ctx.desc.unscaled_special) == (2, 1, 1), fl


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return V.Ref(P.bind(V.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", V.BINDING)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = V.colour_split(name, seed=5, pad=3, ramp=True)
    sizes = V.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    # the binding's describer knows every one of them, the splitter as the splitter
    c = hooked.open(name)
    e = hooked.describe(c)
    hooked.free(c)
    assert e is not None and (e.layout, e.fmt, e.ctx.desc.unscaled_special) == (V.LAYOUTS[V.cfg(name)[4]], V.DSTS[V.cfg(name)[5]], name in V.SPLIT), name
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    # the splitter (c->swscale set outside the wrapped selectors) is left to the reference: the picture counter does not move
    assert lib.ref_sws_pictures() == before + (1 if name in V.TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls
    assert not any(V.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("name", V.BINDING)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = V.picture(name, seed=6, pad=3)
    sizes = V.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    if name in V.SPLIT:
        assert lib.ref_sws_tier1_calls() == before, name                       # no inner loop runs: nv12ToPlanarWrapper
    else:
        assert lib.ref_sws_tier1_calls() > before, name
    assert lib.ref_sws_pictures() == pics
    assert not any(V.differing_rows(got, want, sizes)), name
