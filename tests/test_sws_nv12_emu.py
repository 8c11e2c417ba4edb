"""CPU: NV12 / NV21 destinations of the device swscale path and the unscaled yuv420p -> NV12 / NV21 packer through the emulated product library.

The table of tests/sws_nv12.py must reach what its census lists (asserted from the plan, source and destination queries).  Every small
entry equals the reference's own sws_scale() through Tier 1 and through a guarded four-frame Tier-2 batch; the committed contexts are the
reference's; the line entry equals yuv2nv12cX_c written out in numpy; the creators refuse what lies outside the list; the binding takes the
scaled contexts in both of its forms and leaves the packer to the reference (oracle/_ref/libswsref_tier1.so)."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_nv12 as N
import sws_planar as P
import sws_sources as X

HAVE_REF_LIB = os.path.exists(N.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        X.make_fresh("_ref/libswsref.so")
    return N.Ref(P.bind(N.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: N.plan(emu.lib, N.stored_entry(name)) for name in N.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_what_the_issue_lists(plans):
    got = {n: p for n, p in plans.items() if p}
    cfgs = {n: N.cfg(n) for n in N.NAMES}
    for n, p in got.items():
        dw, dh = cfgs[n][2:4]
        assert (p["depth"], (p["hsub"], p["vsub"])) == (cfgs[n][5], N.SUBS[cfgs[n][4]]), (n, p)
        assert (p["format"], p["planes"]) == (N.DSTS[cfgs[n][6]], 2), (n, p)
        if p["kernel"] == "nv12_pack":
            assert n in N.PACKED and (p["chr_bytes"], p["chr_rows"]) == (2 * (dw // 2), dh // 2), (n, p)
        else:
            assert n not in N.PACKED and (p["chr_bytes"], p["chr_rows"]) == (2 * -(-dw // 2), -(-dh // 2)), (n, p)
    # all three planar instances at 8 and at 16 bits, and the packer
    assert {p["kernel"] for p in got.values() if p["depth"] == 8} == {"planar_a", "planar_b", "planar_c", "nv12_pack"}
    assert {p["kernel"] for p in got.values() if p["depth"] > 8} == {"planar_a", "planar_b", "planar_c"}
    scaled = {n: p for n, p in got.items() if p["kernel"] != "nv12_pack"}
    assert {p["narrow"] for p in scaled.values()} == {0, 1}
    assert {p["hstaged"] for p in scaled.values() if p["depth"] > 8} == {0, 1}
    # one-tap and multi-tap chroma banks on a dithered source
    taps = {min(N.stored_entry(n).ctx.desc.vChr.size, 2) for n, p in scaled.items() if p["depth"] > 8}
    assert taps == {1, 2}, taps
    # taps in registers and from memory
    sizes = {N.stored_entry(n).ctx.desc.vChr.size for n in scaled}
    assert any(s <= 8 for s in sizes) and any(s > 8 for s in sizes), sizes
    # both byte orders, scaled and packed
    assert {cfgs[n][6] for n in scaled} == {"nv12", "nv21"} and {cfgs[n][6] for n in got if n in N.PACKED} == {"nv12", "nv21"}
    # dstW on and off 128, odd dstW and dstH, odd packer width and height
    assert any(cfgs[n][2] % 128 == 0 for n in scaled) and any(cfgs[n][2] % 128 for n in scaled)
    assert any(cfgs[n][2] % 2 for n in scaled) and any(cfgs[n][3] % 2 for n in scaled)
    assert any(cfgs[n][0] % 2 for n in N.PACKED) and any(cfgs[n][1] % 2 for n in N.PACKED)
    # the batch puts destination planes and strides on and off 16- and 8-byte alignment (the three store forms of the chroma pass)
    for n in ("n420d8_w256_up", "n420d8_w384_nv21"):
        lay = N.dst_layouts(N.stored_entry(n))[1::2]
        assert any((o | st) % 16 == 0 for o, st in lay) and any((o | st) % 16 == 8 for o, st in lay) and any((o | st) % 8 for o, st in lay), (n, lay)


def test_refused_entries_are_named_and_few(plans):
    refused = {n for n, p in plans.items() if p is None}
    assert refused == N.REFUSED, refused
    assert len(refused) * N.REFUSED_CAP <= len(N.NAMES), (len(refused), len(N.NAMES))
    assert not refused & (N.BIG | N.CHAIN)


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    for name in N.SHAPES:
        assert N.stored_entry(name).same(ref.entry(name)), name


# ---- parity ------------------------------------------------------------------------------------------------------------------------
TAKEN_SMALL = [n for n in N.SMALL if n not in N.REFUSED]          # (the refused entry: test_refused_entries_are_named_and_few, and the binding)


@needs_ref
@pytest.mark.parametrize("name", TAKEN_SMALL)
def test_emulated_tier1_matches_reference(emu, ref, name):
    e = N.stored_entry(name)
    h = N.create(emu.lib, e)
    assert h, name
    try:
        sizes = e.out_sizes()
        for planes in (N.picture(name, seed=11, pad=5), N.checkerboard(name, pad=2)):
            want = ref.scale(name, planes, sizes)
            got = N.scale_tier1(emu.lib, h, e, planes, pad=8)
            # the whole rounded-up extent: what the packer leaves alone is 0x5A on both sides
            assert not any(N.differing_rows(got, want, sizes)), name
            assert all((g[:, w:] == 0x5A).all() for g, (w, _) in zip(got, sizes))       # the caller's padding untouched
    finally:
        emu.lib.mi355_sws_destroy(C.c_void_p(h))


@needs_ref
@pytest.mark.parametrize("name", TAKEN_SMALL)
def test_emulated_batched(emu, ref, plans, name):
    p = N.check_batch(emu.lib, ref, name, e=N.stored_entry(name))
    assert p is not None and p == plans[name], name


@needs_ref
def test_packer_leaves_the_rounded_down_rest_alone(emu, ref):
    """the reference's own output says which bytes of the second plane stay 0x5A: one chroma row of 70x51, one pair a row of 71x50"""
    for name, rows, cols in (("k420d8_pack_70x51", slice(25, 26), slice(0, 70)), ("k420d8_pack_71x50", slice(0, 25), slice(70, 72))):
        e = N.stored_entry(name)
        planes = N.picture(name, seed=3)
        want = ref.scale(name, planes, e.out_sizes())
        assert (want[1][rows, cols] == 0x5A).all(), name
        h = N.create(emu.lib, e)
        try:
            got = N.scale_tier1(emu.lib, h, e, planes)
        finally:
            emu.lib.mi355_sws_destroy(C.c_void_p(h))
        assert (got[1][rows, cols] == 0x5A).all() and (got[1] == want[1]).all() and (got[0] == want[0]).all(), name


# ---- the line entry ------------------------------------------------------------------------------------------------------------------
def test_yuv2nv12cx_line_entry(emu):
    N.check_nv12cx(emu.lib)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_creators_refuse_what_is_outside_the_list(emu):
    lib = emu.lib
    e = N.stored_entry("n420d8_down2")
    for fmt in list(range(4, 16)) + [18]:
        assert not N.create(lib, N.Entry(e.ctx, e.depth, e.hsub, e.vsub, e.dither, fmt)), fmt
        lib.mi355_sws_create_planar.restype = C.c_void_p
        lib.mi355_sws_create_planar.argtypes = [C.c_void_p, C.c_int]
        assert not lib.mi355_sws_create_planar(C.byref(e.ctx.desc), fmt), fmt
    # mi355_sws_create_planar takes the two new values for its 8-bit 4:2:0 source
    h = lib.mi355_sws_create_planar(C.byref(e.ctx.desc), 16)
    assert h and N.plan_of(lib, h)["format"] == 16
    lib.mi355_sws_destroy(C.c_void_p(h))

    def edited(entry, **ints):
        c = entry.ctx
        return N.Entry(P.S.Context({**c.ints, **ints}, dict(c.banks), c.luts), entry.depth, entry.hsub, entry.vsub, entry.dither, entry.fmt)

    # the packer: depth 8, 4:2:0, equal sizes only
    k = N.stored_entry("k420d8_pack")
    assert N.plan(lib, k)["kernel"] == "nv12_pack"
    assert not N.create(lib, N.Entry(k.ctx, 10, 1, 1, k.dither, 16))
    assert not N.create(lib, N.Entry(edited(k, chrSrcH=48).ctx, 8, 1, 0, k.dither, 16))
    assert not N.create(lib, edited(k, dstW=62, chrDstW=31))
    assert not N.create(lib, edited(k, dstH=46))
    # a descriptor whose chroma rows are not those of a 4:2:0 destination: the yuv422p context of the same shape
    p422 = X.stored_entry("p444d9_to422_w257")
    assert p422.ctx.desc.vChr.n == p422.ctx.desc.dstH
    assert not N.create(lib, N.Entry(p422.ctx, p422.depth, p422.hsub, p422.vsub, p422.dither, 16))
    # ... and a chrDstW that does not follow from dstW
    assert not N.create(lib, edited(e, chrDstW=e.ctx.ints["chrDstW"] - 1))
    # the rgb entry points on a semi-planar context, and the queries on nothing
    h = N.create(lib, e)
    assert h
    try:
        lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        buf = (C.c_uint8 * 256)()
        assert lib.mi355_sws_scale_frames_dev(C.c_void_p(h), buf, 1, None) == -1
        lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        src, ss = (C.c_void_p * 3)(C.addressof(buf), C.addressof(buf), C.addressof(buf)), (C.c_int * 3)(64, 32, 32)
        assert lib.mi355_sws_scale(C.c_void_p(h), src, ss, buf, 192) == -1
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))
    lib.mi355_sws_destination.argtypes = [C.c_void_p, C.c_void_p]
    assert lib.mi355_sws_destination(None, None) == -1


def test_destination_query_of_the_existing_contexts(emu):
    for name, want in (("r420d10_down2", (0, 1, 0, 0)), ("p420d10_to420_down2", (1, 3, 32, 24)), ("p444d9_to422_w257", (2, 3, 129, 37))):
        e = X.stored_entry(name)
        h = X.create(emu.lib, e)
        assert h
        try:
            p = N.plan_of(emu.lib, h)
            assert (p["format"], p["planes"], p["chr_bytes"], p["chr_rows"]) == want, (name, p)
        finally:
            emu.lib.mi355_sws_destroy(C.c_void_p(h))


# ---- the describers on live contexts ---------------------------------------------------------------------------------------------------
@needs_sources
def test_describers_on_live_contexts(ref):
    lib = ref.lib
    for name in N.SHAPES:
        e = ref.entry(name)                                                         # (asserts format and unscaled_special)
        assert e.ctx.desc.chrDstW == -(-N.cfg(name)[2] // 2)
        if name not in N.PACKED:
            assert e.ctx.desc.vChr.n == -(-N.cfg(name)[3] // 2), name
    # mi355_sws_describe_planar: the 8-bit yuv420p rows of the generic scaler, not the packer
    pr = P.Ref(lib)
    for name, want in (("n420d8_down2", 16), ("n420d8_w384_nv21", 17)):
        c = ref.open(name)
        got = pr.describe(c)
        ref.free(c)
        assert got is not None and got[1] == want and got[0].desc.vChr.n == -(-N.cfg(name)[3] // 2), name
    c = ref.open("k420d8_pack")
    assert pr.describe(c) is None
    ref.free(c)
    flags = lib.ref_sws_flags_word(1, 1, 1)
    declined = [
        (96, 40, b"nv12", 64, 40, b"rgb24", flags),                             # a semi-planar source
        (96, 40, b"nv12", 64, 40, b"nv12", flags),
        (64, 48, b"nv12", 64, 48, b"yuv420p", flags),
        (64, 48, b"yuv420p10le", 64, 48, b"yuv420p", flags),                    # a plane copy
        (96, 40, b"yuv422p", 64, 40, b"nv12", (flags & ~0x7) | 0x1),            # SWS_FAST_BILINEAR
        (96, 40, b"yuv420p", 64, 40, b"nv21", (flags & ~0x7) | 0x1),
        (96, 40, b"yuv420p12le", 64, 40, b"nv12", flags),
    ]
    for args in declined:
        c = ref.open_formats(*args)
        assert ref.describe(c) is None, args
        ref.free(c)
    # the packer whatever the flags
    for fl in (flags, lib.ref_sws_flags_word(0, 0, 0), (flags & ~0x7) | 0x1):
        c = ref.open_formats(64, 48, b"yuv420p", 64, 48, b"nv21", fl)
        e = ref.describe(c)
        ref.free(c)
        assert e is not None and (e.fmt, e.ctx.desc.unscaled_special) == (17, 1), fl


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return N.Ref(P.bind(X.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", N.BINDING)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = N.picture(name, seed=5, pad=3)
    sizes = N.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    # the binding's describer knows every one of them, the packer as the packer
    c = hooked.open(name)
    e = hooked.describe(c)
    hooked.free(c)
    assert e is not None and (e.fmt, e.ctx.desc.unscaled_special) == (N.DSTS[N.cfg(name)[6]], name in N.PACKED), name
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    # the packer (c->swscale set outside the wrapped selectors) and the refused entry are left to the reference
    assert lib.ref_sws_pictures() == before + (1 if name in N.TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls
    assert not any(N.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("name", N.BINDING)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = N.picture(name, seed=6, pad=3)
    sizes = N.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    if name in N.PACKED:
        c = hooked.open(name)
        e = hooked.describe(c)
        hooked.free(c)
        assert e is not None and e.ctx.desc.unscaled_special == 1, name         # known to the describer, and still the reference's function
        assert lib.ref_sws_tier1_calls() == before, name                       # no inner loop runs: planarToNv12Wrapper
    else:
        assert lib.ref_sws_tier1_calls() > before, name                         # (the line form does not depend on the device tiles)
    assert lib.ref_sws_pictures() == pics
    assert not any(N.differing_rows(got, want, sizes)), name
