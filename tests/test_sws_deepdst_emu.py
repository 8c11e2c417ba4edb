"""CPU: 9- and 10-bit planar destinations of the device swscale path through the emulated product library.

The table of tests/sws_deepdst.py must reach what its census lists (asserted from the plan, source, source-layout, destination, range and depth
queries and from the banks).  Every entry equals the reference's own sws_scale() of the same buffers through Tier 1 (noise, the checkerboard,
the ramp, all-0 and all-maximum pictures) and through a guarded six-frame Tier-2 batch whose planes lie at the three alignment classes of the
16-bit store; the two line entries equal the two formulas written out in numpy; depth 8 through the new creator is
mi355_sws_create_src_layout_range; the creator refuses what lies outside the list; the five existing describers decline every row; the binding
takes these contexts in both of its forms (oracle/_ref/libswsref_tier1.so)."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_deepdst as D
import sws_nv12 as N
import sws_nvsrc as V
import sws_planar as P
import sws_range as G
import sws_rgbsrc as R
import sws_sources as X

HAVE_REF_LIB = os.path.exists(D.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        D.make_fresh("_ref/libswsref.so")
    return D.Ref(P.bind(D.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: D.plan(emu.lib, D.stored_entry(name)) for name in D.NAMES}


def source_class(name):
    """8-bit planar, 9-bit, 10-bit planar, nv, rgb with the halving / the full chroma converter"""
    kind, depth, (hsub, _) = D.src_kind(name)
    return {"planar": "d%d" % depth, "nv": "nv", "rgb": "rgb_half" if hsub else "rgb_full"}[kind]


def rung(taps):
    """the NTAP instance of the vertical pass a bank of `taps` taps takes: 1 / 2 / 4 / 8, 0 from memory"""
    return 1 if taps == 1 else (2 if taps <= 2 else (4 if taps <= 4 else (8 if taps <= 8 else 0)))


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_what_the_issue_lists(plans):
    got = {n: p for n, p in plans.items() if p}
    cfgs = {n: D.cfg(n) for n in D.NAMES}
    assert 28 <= len(D.NAMES) <= 34
    for n, p in got.items():
        _, depth, (hsub, vsub) = D.src_kind(n)
        sub, bits = D.dst_kind(n)
        e = D.stored_entry(n)
        assert (p["depth"], p["hsub"], p["vsub"], p["layout"], p["range"], p["dst_depth"]) == (depth, hsub, vsub, D.LAYOUTS.get(cfgs[n][4], 0), 0, bits), (n, p)
        assert p["format"] == D.DSTS[sub] and p["planes"] == 3 and p["chr_bytes"] == 2 * e.ctx.desc.chrDstW, (n, p)
        assert p["kernel"].startswith("planar_"), (n, p)
    for bits in (9, 10):
        rows = {n: p for n, p in got.items() if p["dst_depth"] == bits}
        assert {D.dst_kind(n)[0] for n in rows} == {"420", "422", "444"}, bits
        assert {p["kernel"] for p in rows.values()} == {"planar_a", "planar_b", "planar_c"}, (bits, {n: p["kernel"] for n, p in rows.items()})
        assert {p["narrow"] for p in rows.values()} == {0, 1}, bits
        # a vertical bank of more than eight taps; the one-tap form (identity banks at equal size)
        assert any(D.stored_entry(n).ctx.desc.vLum.size > 8 for n in rows), bits
        assert any(D.stored_entry(n).ctx.desc.vLum.size == 1 and D.stored_entry(n).ctx.desc.hLum.size == 1 for n in rows if cfgs[n][:2] == cfgs[n][2:4]), bits
        # vertical banks on the rungs of the ladder a bicubic context reaches: one tap, up to four, up to eight, more (from memory)
        assert {rung(D.stored_entry(n).ctx.desc.vLum.size) for n in rows} >= {1, 4, 8, 0}, bits
    # ... and the two-tap rung, from a bilinear upscale
    assert {rung(D.stored_entry(n).ctx.desc.vLum.size) for n in got} == {1, 2, 4, 8, 0}
    assert {source_class(n) for n in got} == {"d8", "d9", "d10", "nv", "rgb_half", "rgb_full"}
    assert {p["hstaged"] for p in got.values()} == {0, 1}
    # the forms of the horizontal pass: identity, staged, direct (a 4:1 reduction at dstW 128 or 130)
    forms = set()
    for n in got:
        if D.src_kind(n)[0] == "planar" and D.src_kind(n)[1] == 8:
            forms |= set().union(*R.hforms(D.stored_entry(n), got[n]))
    assert forms == {"identity", "staged", "direct"}, forms
    # the rows the issue names
    assert cfgs["e_420_422d10_same"][:6] == (64, 48, 64, 48, "yuv420p", "yuv422p10le") and cfgs["e_444d10_420d9_same"][:6] == (64, 48, 64, 48, "yuv444p10le", "yuv420p9le")
    down2 = {(c[4], c[5]) for c in cfgs.values() if c[:4] == (128, 96, 64, 48)}
    assert down2 >= {("yuv420p", "yuv420p10le"), ("yuv422p9le", "yuv420p10le"), ("yuv420p10le", "yuv420p10le"), ("yuv444p10le", "yuv444p10le"),
                     ("nv12", "yuv420p10le"), ("nv21", "yuv422p9le"), ("rgb24", "yuv420p10le"), ("bgr24", "yuv444p10le")}
    assert D.src_kind("d2_rgb_420d10")[2][0] == 1                                          # the halving converter
    assert {cfgs[n][2] for n in got} >= {127, 128, 129, 130} and any(cfgs[n][:4] == (100, 30, 129, 45) for n in got)
    assert any(cfgs[n][:4] == (33, 17, 97, 61) for n in got) and any(cfgs[n][3] == 1 for n in got)
    assert {cfgs[n][2] for n in got if cfgs[n][0] == 4 * cfgs[n][2]} == {128, 130}
    for ratio in (2, 3, 6):
        assert {D.dst_kind(n)[1] for n in got if cfgs[n][0] == cfgs[n][2] and cfgs[n][1] == ratio * cfgs[n][3]} == {9, 10}, ratio
    # the batch's destination planes hit the three alignment classes of the store, on even addresses and strides
    for n in ("e_420_422d10_same", "d2_420_420d10", "odd_nv21_422d10"):
        lay, _ = D.layout(D.stored_entry(n).out_sizes(), 6)
        assert {D.store_class(o) for row in lay for o, _ in row} == {16, 4, 2}, n
        assert all(o % 2 == 0 and st % 2 == 0 for row in lay for o, st in row), n
    # the line pads are sws_sources' in samples
    assert D.DST_PADS == tuple(2 * p for p in X.DST_PADS)


def test_refused_entries_are_named_and_few(emu, plans):
    refused = {n for n, p in plans.items() if p is None}
    assert refused == D.REFUSED == {"v16_420d10_420d10"}, refused
    assert len(refused) * D.REFUSED_CAP <= len(D.NAMES), (len(refused), len(D.NAMES))
    # a deep context has its 8-bit twin's banks: it is refused exactly where the twin is (the same descriptor at depth 8)
    for n in D.NAMES:
        e = D.stored_entry(n)
        assert (V.plan(emu.lib, e) is None) == (n in refused), n
    # ... and the refused row is the deep twin of sws_sources' refused one
    assert D.cfg("v16_420d10_420d10")[:4] == X.SHAPES["p420d10_to420_vdown16"][:4] and "p420d10_to420_vdown16" in X.REFUSED


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    """every row is opened by the reference and described as the table expects; the committed arrays are those, and the banks the 8-bit twin's"""
    for name in D.SHAPES:
        e = D.stored_entry(name)
        assert e.same(ref.entry(name)), name
        c = ref.open_twin(name)
        twin = ref.describe_fmt(c)
        ref.free(c)
        assert twin is not None and not twin.ctx.desc.unscaled_special, name
        assert V.same_banks(e, twin) and e.ctx.ints == twin.ctx.ints, name


# ---- parity ------------------------------------------------------------------------------------------------------------------------
TAKEN = [n for n in D.NAMES if n not in D.REFUSED]


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_tier1_matches_reference(emu, ref, name):
    D.check_tier1(emu.lib, ref, name, D.tier1_pictures(name, seed=11))


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_batched(emu, ref, plans, name):
    p = D.check_batch(emu.lib, ref, name, e=D.stored_entry(name))
    assert p is not None and p == plans[name], name


@needs_ref
def test_both_clips_are_live(ref):
    """the reference's own pictures of the table hold 0 under a negative sum and (1 << bits) - 1 under one above it"""
    for name in ("up_420d10_422d10_w129", "up_nv12_444d9_w129"):                          # the bicubic overshoot of an upscaled checkerboard
        e = D.stored_entry(name)
        bits, sizes = e.dst_depth, e.out_sizes()
        out = ref.scale(name, D.picture(name, "checker", 2), sizes)
        luma = np.ascontiguousarray(out[0][:, :sizes[0][0]]).view("<u2")
        assert luma.max() == (1 << bits) - 1 and luma.min() == 0, (name, int(luma.min()), int(luma.max()))
    # all-maximum 10-bit planes stay 1023 to a 10-bit destination: (32736 + 16) >> 5
    e = D.stored_entry("e_444d10_420d9_same")
    out = ref.scale("e_444d10_420d9_same", D.picture("e_444d10_420d9_same", "ones", 6), e.out_sizes())
    assert (np.ascontiguousarray(out[0][:, :e.out_sizes()[0][0]]).view("<u2") == 511).all()


@needs_ref
def test_the_depth_matters(emu, ref):
    """a context created with the other depth than the reference's is another picture: what the binding's per-call look at the format guards"""
    name = "d2_420_420d10"
    e = D.stored_entry(name)
    planes = D.picture(name, "noise", 3)
    want = ref.scale(name, planes, e.out_sizes())
    for bits, equal in ((10, True), (9, False)):
        h = D.create(emu.lib, e.edited(dst_depth=bits))
        assert h
        try:
            got = D.scale_tier1(emu.lib, h, e, planes)
            assert (not any(D.differing_rows(got, want, e.out_sizes()))) == equal, bits
        finally:
            emu.lib.mi355_sws_destroy(C.c_void_p(h))


def test_tier1_refuses_odd_and_short_strides(emu):
    lib = emu.lib
    name = "e_420_422d10_same"
    e = D.stored_entry(name)
    planes = D.picture(name, "noise", 3)
    h = D.create(lib, e)
    assert h
    try:
        sizes = e.out_sizes()
        src = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
        ss = (C.c_int * 3)(*[p.strides[0] for p in planes])
        lib.mi355_sws_scale_planar.argtypes = [C.c_void_p] * 5
        for plane in range(3):
            for bad in (sizes[plane][0] + 1, sizes[plane][0] - 2, sizes[plane][0] // 2):
                out = [np.full((hh, w + 8), 0x5A, np.uint8) for w, hh in sizes]
                st = [o.strides[0] for o in out]
                st[plane] = bad
                dst = (C.c_void_p * 3)(*[o.ctypes.data for o in out])
                assert lib.mi355_sws_scale_planar(C.c_void_p(h), src, ss, dst, (C.c_int * 3)(*st)) == -1, (plane, bad)
                assert all((o == 0x5A).all() for o in out)
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))


# ---- the line entries: no reference needed -----------------------------------------------------------------------------------------
def test_line_entries_match_the_formulas_written_out(emu):
    assert int(D.model_plane1([32767], 10)[0]) == 1023 and (32767 + 16) >> 5 == 1024
    assert D.check_line_entries(emu.lib) > 0


# ---- the creator -------------------------------------------------------------------------------------------------------------------
def test_depth_8_is_the_existing_creator(emu):
    """same plan and same bytes as mi355_sws_create_src_layout_range on stored entries of the sibling tables, range 1 / 2 included"""
    lib = emu.lib
    for name in ("f_420_down2", "t_nv12_444_down2", "t_d10_422_w129_up"):
        e = G.stored_entry(name)
        assert e.range in (1, 2)
        for g in (e, e.edited(range=0)):
            old, new = G.create(lib, g), D.create(lib, D.Entry.of(g, 8))
            assert old and new, name
            try:
                po, pn = G.plan_of(lib, old), D.plan_of(lib, new)
                assert pn.pop("dst_depth") == 8 and po == pn and po["range"] == g.range, name
                lib.mi355_sws_dest_depth.argtypes = [C.c_void_p]
                assert lib.mi355_sws_dest_depth(C.c_void_p(old)) == 8
                planes = G.picture(name, "noise", seed=9, pad=3)
                a, b = X.scale_tier1(lib, old, g, planes), X.scale_tier1(lib, new, g, planes)
                assert all((x == y).all() for x, y in zip(a, b)), name
            finally:
                lib.mi355_sws_destroy(C.c_void_p(old))
                lib.mi355_sws_destroy(C.c_void_p(new))
    # rgb24 and the special converters stay reachable at depth 8
    for name in ("v_rgb_down2", "k_split"):
        e = V.stored_entry(name)
        assert D.plan(lib, D.Entry.of(e, 8))["kernel"] == V.plan(lib, e)["kernel"], name


def test_creator_refuses_what_lies_outside_the_list(emu):
    lib = emu.lib
    e = D.stored_entry("d2_420_420d10")
    assert D.plan(lib, e)["dst_depth"] == 10 and D.plan(lib, e.edited(dst_depth=9))["dst_depth"] == 9
    for bits in (7, 11, 12, 16, 0, -1):
        assert not D.create(lib, e.edited(dst_depth=bits)), bits
    for bits in (9, 10):
        # a depth with rgb24 / NV12 / NV21, and with the formats every creator refuses
        for fmt in [0, 16, 17] + list(range(4, 16)) + [18]:
            assert not D.create(lib, e.edited(dst_depth=bits, fmt=fmt)), (bits, fmt)
        for rng in (1, 2, 3, -1):
            assert not D.create(lib, e.edited(dst_depth=bits, range=rng)), (bits, rng)
        assert not D.create(lib, e.edited(dst_depth=bits, unscaled_special=1)), bits
        for layout in (3, 6, -1):
            assert not D.create(lib, e.edited(dst_depth=bits, layout=layout)), (bits, layout)
        assert not D.create(lib, e.edited(dst_depth=bits, depth=11)) and not D.create(lib, e.edited(dst_depth=bits, layout=1, depth=10))
        # the packer, the splitter and the rgb special under a depth
        pack = N.stored_entry(sorted(N.PACKED)[0])
        assert N.plan(lib, pack)["kernel"] == "nv12_pack"
        assert not D.create(lib, D.Entry(pack.ctx, pack.depth, pack.hsub, pack.vsub, pack.dither, pack.fmt, 0, 0, bits)), bits
        split = V.stored_entry("k_split")
        assert V.plan(lib, split)["kernel"] == "nv12_split"
        assert not D.create(lib, D.Entry.of(split, bits)), bits
        special = X.stored_entry("r422d8_special")
        assert X.plan(lib, special)["kernel"] == "c24"
        assert not D.create(lib, D.Entry(special.ctx, special.depth, special.hsub, special.vsub, special.dither, special.fmt, 0, 0, bits)), bits
        assert not D.create(lib, D.Entry(special.ctx, special.depth, special.hsub, special.vsub, special.dither, 2, 0, 0, bits)), bits
    lib.mi355_sws_dest_depth.argtypes = [C.c_void_p]
    lib.mi355_sws_range.argtypes = [C.c_void_p]
    assert lib.mi355_sws_dest_depth(None) == -1 and lib.mi355_sws_range(None) == -1
    for f in (lib.mi355_sws_plan, lib.mi355_sws_destination, lib.mi355_sws_source):
        f.argtypes = [C.c_void_p, C.c_void_p]
        assert f(None, None) == -1


def test_existing_entry_points_on_a_deep_descriptor(emu):
    """the existing creators answer as before on a deep context's descriptor (it is its twin's), and the RGB entry points return -1 on a deep
    context"""
    lib = emu.lib
    e = D.stored_entry("d2_420_420d10")
    deep = D.plan(lib, e)
    twin = G.plan(lib, e)
    assert twin["chr_bytes"] * 2 == deep["chr_bytes"]
    assert {k: v for k, v in deep.items() if k not in ("dst_depth", "chr_bytes")} == {k: v for k, v in twin.items() if k != "chr_bytes"}
    assert V.plan(lib, e) == {k: v for k, v in twin.items() if k != "range"}
    lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    buf = (C.c_uint8 * 1024)()
    src, ss = (C.c_void_p * 3)(C.addressof(buf), C.addressof(buf), C.addressof(buf)), (C.c_int * 3)(128, 64, 64)
    h = D.create(lib, e)
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
    for name in D.NAMES:
        c = ref.open(name)
        e = ref.describe_depth(c)
        assert ref.declined_by_the_five_describers(c), name
        ref.free(c)
        sub, bits = D.dst_kind(name)
        assert e is not None and (e.layout, e.fmt, e.range, e.dst_depth) == (D.LAYOUTS.get(D.cfg(name)[4], 0), D.DSTS[sub], 0, bits), name
    declined = [
        (64, 48, "yuv420p", 0, 64, 48, "yuv420p10le", 0, flags),                 # a plane copy (planarCopyWrapper): no banks
        (64, 48, "yuv420p10le", 0, 64, 48, "yuv420p9le", 0, flags),
        (128, 96, "yuv420p", 0, 64, 48, "yuv420p10be", 0, flags),                # big endian
        (128, 96, "yuv420p", 0, 64, 48, "yuv420p12le", 0, flags),
        (128, 96, "yuv420p", 0, 64, 48, "yuv420p16le", 0, flags),
        (128, 96, "yuv420p", 0, 64, 48, "gray10le", 0, flags),
        (128, 96, "yuv420p", 0, 64, 48, "yuv420p10le", 0, (flags & ~0x7) | 0x1),  # SWS_FAST_BILINEAR
        (128, 96, "yuv420p", 1, 64, 48, "yuv420p10le", 0, flags),                # a deep destination with a range, both directions
        (128, 96, "yuv420p", 0, 64, 48, "yuv422p9le", 1, flags),
    ]
    for args in declined:
        c = ref.open_ranges(*args)
        assert ref.describe_depth(c) is None and ref.declined_by_the_five_describers(c), args
        ref.free(c)
    # P010: this reference has no such output ("p010le is not supported as output pixel format"), so no context of it reaches a describer
    p010 = lib.av_get_pix_fmt(b"p010le")
    assert p010 >= 0 and not lib.sws_getContext(128, 96, lib.av_get_pix_fmt(b"yuv420p"), 64, 48, p010, flags, None, None, None)
    # 8-bit destinations answer as through mi355_sws_describe_range, with depth 8
    for name in ("f_420_same", "t_rgb_420_down2", "f_420_vdown16"):
        gref = G.Ref(lib)
        c = gref.open(name)
        e, old = ref.describe_depth(c), gref.describe_range(c)
        ref.free(c)
        assert e is not None and e.dst_depth == 8 and G.Entry.same(e, old), name
    for name in ("v_420_down2", "v_rgb_down2", "k_split"):
        vref = V.Ref(lib)
        c = vref.open(name)
        e, old = ref.describe_depth(c), vref.describe(c)
        ref.free(c)
        assert e is not None and e.dst_depth == 8 and e.range == 0 and V.Entry.same(e, old), name


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return D.Ref(P.bind(D.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", D.BINDING)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = D.picture(name, "ramp", seed=5, pad=3)
    sizes = D.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    # the binding's describer knows every one of them, the refused one too (the creator refuses it, not the describer)
    c = hooked.open(name)
    e = hooked.describe_depth(c)
    hooked.free(c)
    assert e is not None and e.dst_depth == D.dst_kind(name)[1], name
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    # a refused context is left to the reference: the picture counter does not move
    assert lib.ref_sws_pictures() == before + (1 if name in D.TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls
    assert not any(D.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("name", D.BINDING)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = D.picture(name, "noise", seed=6, pad=3)
    sizes = D.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    # the horizontal entries of every source line and the output entry of every destination row
    dh = D.cfg(name)[3]
    assert lib.ref_sws_tier1_calls() >= before + dh + D.stored_entry(name).ctx.desc.vChr.n * 2, name
    assert lib.ref_sws_pictures() == pics
    assert not any(D.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("lines", [False, True])
def test_binding_leaves_a_plane_copy_to_the_reference(hooked, ref, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    row = D.PLANE_COPY
    planes = D.picture(row, "noise", seed=8, pad=3)
    sizes = [(2 * 64, 48), (2 * 32, 24), (2 * 32, 24)]
    want = ref.scale(row, planes, sizes)
    lib = hooked.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(row, planes, sizes)
    assert (lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()) == (pics, calls)
    assert not any(D.differing_rows(got, want, sizes))
