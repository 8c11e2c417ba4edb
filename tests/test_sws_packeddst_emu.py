"""CPU: bgr24 and 32-bit rgba / bgra / argb / abgr destinations of the device swscale path through the emulated product library.

The table of tests/sws_packeddst.py must reach what its census lists (asserted from the plan, source, source-layout and destination queries and
from the banks).  Every entry equals the reference's own sws_scale() of the same buffers through Tier 1 (noise, the checkerboard, the ramp, all-0
and all-maximum pictures) and through a guarded six-frame Tier-2 batch whose rows lie on a 16-byte multiple, on a 4-byte multiple that is no
multiple of 16 and (24 bits) on an odd address, at line pads of 0, 5, 16 and 3 pixels; the creator refuses what lies outside the list, each with
its message; Tier 1 returns -1 for a 32-bit destination off 4-byte multiples; the planar entry points return -1; the line entries at format 0
equal the rgb24 trio; the six existing describers decline every row and the new one declines rgb24; the LUTs of a 32-bit context equal those of
its rgb24 twin; the binding takes these contexts in both of its forms (oracle/_ref/libswsref_tier1.so)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sws_packeddst as K
import sws_nvsrc as V
import sws_planar as P
import sws_sources as X
import sws_support as S

HAVE_REF_LIB = os.path.exists(K.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        K.make_fresh("_ref/libswsref.so")
    return K.Ref(P.bind(K.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: K.plan(emu.lib, K.stored_entry(name)) for name in K.NAMES}


def twin(e):
    """the rgb24 context of the same descriptor"""
    return V.Entry(e.ctx, e.depth, e.hsub, e.vsub, e.dither, 0, e.layout)


def source_class(name):
    kind, depth, (hsub, _) = K.src_kind(name)
    return {"planar": "d%d" % depth, "nv": "nv", "rgb": "rgb_half" if hsub else "rgb_full"}[kind]


def template(e):
    """which packed template a context of the generic scaler runs (swscale.c:658-682): "1" with one or two chroma taps, "2", "X" """
    d = e.ctx.desc
    ls, cs = d.vLum.size, d.vChr.size
    return "1/%d" % cs if ls == 1 and cs <= 2 else ("2" if (ls, cs) == (2, 2) else "X")


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_what_the_issue_lists(plans):
    got = {n: p for n, p in plans.items() if p}
    cfgs = {n: K.cfg(n) for n in K.NAMES}
    entries = {n: K.stored_entry(n) for n in K.NAMES}
    for n, p in got.items():
        _, depth, (hsub, vsub) = K.src_kind(n)
        assert (p["depth"], p["hsub"], p["vsub"], p["layout"], p["range"], p["dst_depth"]) == (depth, hsub, vsub, K.LAYOUTS.get(cfgs[n][4], 0), 0, 8), (n, p)
        assert p["format"] == K.DSTS[cfgs[n][5]] and p["planes"] == 1 and p["chr_bytes"] == 0 and p["chr_rows"] == 0, (n, p)
        d = entries[n].ctx.desc
        assert d.chrDstW == (d.dstW + 1) >> 1 and (d.unscaled_special or d.vChr.n == d.dstH), n
    down2 = {(c[4], c[5]) for c in cfgs.values() if c[:4] == (128, 96, 64, 48)}
    # each of the five from an 8-bit planar source under a 2:1 reduction; bgr24 and one 32-bit order from each other source kind
    assert down2 >= {("yuv420p", d) for d in K.DSTS}
    for src in ("yuv420p10le", "yuv444p", "nv12", "nv21", "rgb24", "bgr24"):
        dsts = {c[5] for c in cfgs.values() if c[4] == src}
        assert "bgr24" in dsts and dsts - {"bgr24"}, src
    assert K.src_kind("d2_rgb_bgr24")[2][0] == 1 and K.src_kind("up_bgr_argb_w129")[2][0] == 0       # the halving and the full converter
    assert {source_class(n) for n in got} >= {"d8", "d9", "d10", "nv", "rgb_half", "rgb_full"}
    # the three packed templates of the tile kernel, for 24 and for 32 bits: one luma tap with one and with two chroma taps (equal size), two, X
    generic = {n for n, p in got.items() if p["kernel"].startswith("generic")}
    for bytes_pp in (3, 4):
        assert {template(entries[n]) for n in generic if K.bpp(n) == bytes_pp} >= ({"1/1", "2", "X"} if bytes_pp == 3 else {"1/2", "2", "X"}), bytes_pp
    assert {template(entries[n]) for n in generic} == {"1/1", "1/2", "2", "X"}
    # ... both uvalpha branches on the rows of the two-chroma-tap one
    coef = entries["e_420_bgra_w127_bilinear"].ctx.banks["vChr"][0].reshape(-1, 2)[:, 1]
    assert (coef < 2048).any() and (coef >= 2048).any()
    for bytes_pp in (3, 4):
        rows = {n: p for n, p in got.items() if K.bpp(n) == bytes_pp}
        assert {p["kernel"] for p in rows.values()} == {"c24", "ident1_1", "ident1_x", "generic_a", "generic_b", "generic_c"}, bytes_pp
        assert {p["narrow"] for n, p in rows.items() if n in generic} == {0, 1}, bytes_pp
        # a bank of more than eight vertical taps: the narrow form with its taps from memory
        assert any(entries[n].ctx.desc.vLum.size > 8 for n in rows if n in generic), bytes_pp
        # partial tiles, a second tile of one and of two columns, an odd width, one output row or an odd everything
        assert {cfgs[n][2] for n in rows} >= {127, 129, 130}, bytes_pp
    assert any(cfgs[n][3] == 1 for n in got) and any(cfgs[n][:4] == (33, 17, 97, 61) for n in got)
    # the special converter: 4:2:0 to bgr24, rgba and argb, 4:2:2 to one
    special = {n for n, p in got.items() if p["kernel"] == "c24"}
    assert special == K.SPECIAL and all(entries[n].ctx.desc.unscaled_special for n in special)
    assert {cfgs[n][5] for n in special if cfgs[n][4] == "yuv420p"} >= {"bgr24", "rgba", "argb"} and any(cfgs[n][4] == "yuv422p" for n in special)
    # the batch's destination rows hit the alignment classes of the stores
    # (a 32-bit row is on a 16-byte multiple only where dstW is a multiple of 4: the full tile of dstW 128 is the batch's wide store, the
    # first tiles of 129 and 130 are Tier 1's, whose own planes are 16-byte aligned)
    for n in ("d2_420_rgba", "h4_420_abgr_w128", "ix_nv21_argb_w128"):
        lay, _ = K.layout(entries[n].out_sizes(), 6, 4)
        assert {K.store_class(o, st) for (o, st), in lay} >= {16, 4} and all(o % 4 == 0 and st % 4 == 0 for (o, st), in lay), n
    for n in ("d2_420_bgr24", "ix_420_bgr24", "k_420_bgr24"):
        lay, _ = K.layout(entries[n].out_sizes(), 6, 3)
        assert {K.store_class(o, st) for (o, st), in lay} >= {16, 4, 1}, n
    assert K.DST_PADS == X.DST_PADS and set(K.DST_PADS) >= {0, 5, 16}


def test_refused_entries_are_named_and_few(emu, plans):
    refused = {n for n, p in plans.items() if p is None}
    assert refused == K.REFUSED == {"v16_420d10_bgra"}, refused
    assert len(refused) * K.REFUSED_CAP <= len(K.NAMES), (len(refused), len(K.NAMES))
    # a context to one of the five has its rgb24 twin's plan and is refused exactly where the twin is
    for n in K.NAMES:
        e = K.stored_entry(n)
        t = V.plan(emu.lib, twin(e))
        assert (t is None) == (n in refused), n
        if t is not None:
            same = ("kernel", "th", "hstage", "lum_lines", "chr_lines", "narrow", "hstaged")
            assert {k: plans[n][k] for k in same} == {k: t[k] for k in same}, n
    assert K.cfg("v16_420d10_bgra")[:4] == X.SHAPES["r420d10_vdown16"][:4] and "r420d10_vdown16" in X.REFUSED


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    """every row is opened by the reference and described as the table expects; the committed arrays are those, and the banks the rgb24 twin's"""
    for name in K.SHAPES:
        e = K.stored_entry(name)
        assert e.same(ref.entry(name)), name
        t = ref.twin_entry(name)
        assert t is not None and t.fmt == 0 and bool(t.ctx.desc.unscaled_special) == (name in K.SPECIAL), name
        assert e.ctx.ints == t.ctx.ints and (name in K.SPECIAL or V.same_banks(e, t)), name


@needs_sources
def test_luts_are_the_rgb24_twins(ref):
    """the LUT claim: the tables of a context to each of the five — for a 32-bit order converted from the reference's uint32_t table — equal those of
    the rgb24 context of the same source, sizes and flags"""
    seen = set()
    for name in K.SHAPES:
        e, t = K.stored_entry(name), ref.twin_entry(name)
        for k in S.LUTS:
            assert (np.asarray(e.ctx.luts[k]) == np.asarray(t.ctx.luts[k])).all(), (name, k)
        seen.add(K.cfg(name)[5])
    assert seen == set(K.DSTS)


# ---- parity ------------------------------------------------------------------------------------------------------------------------
TAKEN = [n for n in K.NAMES if n not in K.REFUSED]


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_tier1_matches_reference(emu, ref, name):
    K.check_tier1(emu.lib, ref, name, K.tier1_pictures(name, seed=11))


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_batched(emu, ref, plans, name):
    p = K.check_batch(emu.lib, ref, name, e=K.stored_entry(name))
    assert p is not None and p == plans[name], name


@needs_ref
@pytest.mark.parametrize("name", ["d2_420_rgba", "up_420_bgra_w129", "ix_nv21_argb_w128", "k_420_argb", "d2_420_bgr24", "up_bgr_bgr24_w129", "k_420_bgr24"])
def test_tier1_destination_alignments(emu, ref, name):
    """the caller's plane on a 16-byte multiple, on a 4-byte multiple that is no multiple of 16 and (24 bits) on an odd address"""
    for skew in (0, 4, 8) + ((1, 3) if K.bpp(name) == 3 else ()):
        K.check_tier1(emu.lib, ref, name, [K.picture(name, "noise", seed=21 + skew, pad=2)], skew=skew)


@needs_ref
def test_the_order_matters(emu, ref):
    """a context created with another order than the reference's is another picture: what the binding's per-call look at the format guards"""
    name = "d2_420_bgra"
    e = K.stored_entry(name)
    planes = K.picture(name, "noise", 3)
    want = ref.scale(name, planes, e.out_sizes())
    for fmt in (33, 34, 35, 36):
        h = K.create(emu.lib, e.edited(fmt=fmt))
        assert h
        try:
            got = K.scale_tier1(emu.lib, h, e, planes)
            assert (not any(K.differing_rows(got, want, e.out_sizes()))) == (fmt == 34), fmt
        finally:
            emu.lib.mi355_sws_destroy(C.c_void_p(h))


def test_tier1_refuses_32_bit_planes_off_four_and_short_strides(emu):
    lib = emu.lib
    lib.mi355_sws_scale.restype = C.c_int
    lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    for name, bad in (("d2_420_rgba", [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (0, -4), (0, -256)]), ("d2_420_bgr24", [(0, -1), (0, -192)]),
                      ("k_420_argb", [(2, 0), (0, 2), (0, -4)])):
        e = K.stored_entry(name)
        planes = K.picture(name, "noise", 3)
        (w, hh), = e.out_sizes()
        h = K.create(lib, e)
        assert h
        try:
            src = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
            ss = (C.c_int * 3)(*[p.strides[0] for p in planes])
            buf = np.full(hh * (w + 16) + 64, 0x5A, np.uint8)
            base = (-buf.ctypes.data) % 16
            for skew, extra in bad:
                assert lib.mi355_sws_scale(C.c_void_p(h), src, ss, C.c_void_p(buf.ctypes.data + base + skew), w + extra) == -1, (name, skew, extra)
                assert (buf == 0x5A).all()
            # a 24-bit plane may lie anywhere
            if K.bpp(name) == 3:
                assert lib.mi355_sws_scale(C.c_void_p(h), src, ss, C.c_void_p(buf.ctypes.data + base + 1), w + 1) == hh
        finally:
            lib.mi355_sws_destroy(C.c_void_p(h))


# ---- the line entries: no reference needed -----------------------------------------------------------------------------------------
def test_line_entries_at_format_0_are_the_rgb24_trio_and_the_five_are_its_pixels_reordered(emu):
    assert K.check_line_entries(emu.lib, K.stored_entry("d2_420_rgba").ctx.desc.luts) > 0


@needs_ref
@pytest.mark.parametrize("name", ["k_420_bgr24", "k_420_rgba", "k_420_argb"])
def test_slice_entry_matches_reference(emu, ref, name):
    K.check_slice_entry(emu.lib, ref, name)


def test_slice_entry_at_format_0_is_the_rgb24_one(emu):
    lib = emu.lib
    e = K.stored_entry("k_420_bgr24")
    d = e.ctx.desc
    planes = K.picture("k_420_bgr24", "noise", seed=3)
    src = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    ss = (C.c_int * 3)(*[p.strides[0] for p in planes])
    a, b = np.full((d.dstH, d.dstW * 3 + 8), 0x5A, np.uint8), np.full((d.dstH, d.dstW * 3 + 8), 0x5A, np.uint8)
    assert lib.mi355_sws_yuv2rgb_c_24_rgb(C.byref(d.luts), d.dstW, src, ss, 0, d.dstH, C.c_void_p(a.ctypes.data), a.strides[0]) == d.dstH
    assert lib.mi355_sws_yuv2rgb_c(C.byref(d.luts), 0, d.dstW, src, ss, 0, d.dstH, C.c_void_p(b.ctypes.data), b.strides[0]) == d.dstH
    assert (a == b).all() and (a[:, :d.dstW * 3] != 0x5A).any()


# ---- the creator -------------------------------------------------------------------------------------------------------------------
def messages(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("mi355dsp:")]


def test_creator_refuses_what_lies_outside_the_list(emu, capfd):
    lib = emu.lib
    e = K.stored_entry("d2_420_bgra")
    assert K.plan(lib, e)["format"] == 34
    capfd.readouterr()

    def refused(handle, pattern):
        assert not handle
        msg = messages(capfd)
        assert len(msg) == 1 and re.search(pattern, msg[0]), (pattern, msg)

    for fmt in K.DSTS.values():
        g = e.edited(fmt=fmt)
        for rng in (1, 2):
            refused(K.create(lib, g, range_=rng), "range in the LUTs")
        for rng in (3, -1):
            refused(K.create(lib, g, range_=rng), "range %d is not" % rng)
        for bits in (9, 10):
            refused(K.create(lib, g, dst_depth=bits), "%d-bit destination is yuv420p" % bits)
        for bits in (7, 11, 16, 0):
            refused(K.create(lib, g, dst_depth=bits), "destination depth %d is not" % bits)
        for layout in (3, 6, -1):
            refused(K.create(lib, g.edited(layout=layout)), "source layout %d is not" % layout)
        refused(K.create(lib, g.edited(depth=11)), "outside this backend")
        # the special converter takes 8-bit 4:2:0 and 4:2:2 planes only
        refused(K.create(lib, K.stored_entry("d2_444_rgba").edited(fmt=fmt, unscaled_special=1)), "outside this backend")
        refused(K.create(lib, K.stored_entry("d2_420d10_argb").edited(fmt=fmt, unscaled_special=1)), "outside this backend")
        refused(K.create(lib, K.stored_entry("d2_nv12_bgra").edited(fmt=fmt, unscaled_special=1)), "only unscaled special converter of an nv12 / nv21 source")
        refused(K.create(lib, K.stored_entry("d2_rgb_rgba").edited(fmt=fmt, unscaled_special=1)), "no unscaled special converter takes an rgb24 / bgr24 source")
        # the twin's refusals: banks the tiles cannot hold
        refused(K.create(lib, K.stored_entry("v16_420d10_bgra").edited(fmt=fmt)), "filter banks do not fit")
    # a packed-RGB source that scales neither way: identity banks on an even width (built from a 4:4:4 row's sizes)
    same = K.stored_entry("i1_422_bgr24")
    for fmt in [0] + list(K.DSTS.values()):
        refused(K.create(lib, same.edited(fmt=fmt, layout=4, hsub=1, vsub=0)), "without scaling is not a context of the scaler")
    # values of 37 and up, and the ones between the families
    for fmt in [37, 38, 64, 1000] + list(range(4, 16)) + list(range(18, 32)):
        refused(K.create(lib, e.edited(fmt=fmt)), "destination format %d is not" % fmt)
    # the special converter to each of the five, where rgb24 has k_sws_c24
    for fmt in K.DSTS.values():
        assert K.plan(lib, K.stored_entry("k_422_bgra_w70").edited(fmt=fmt))["kernel"] == "c24"
    assert not messages(capfd)


def test_the_creators_that_forward_take_the_five(emu):
    lib = emu.lib
    e = K.stored_entry("d2_nv12_bgra")
    want = K.plan(lib, e)
    lib.mi355_sws_create_src_layout.restype = lib.mi355_sws_create_src_layout_range.restype = lib.mi355_sws_create_src.restype = C.c_void_p
    handles = [lib.mi355_sws_create_src_layout(C.byref(e.ctx.desc), C.byref(e.src), e.layout, e.fmt),
               lib.mi355_sws_create_src_layout_range(C.byref(e.ctx.desc), C.byref(e.src), e.layout, e.fmt, 0)]
    p = K.stored_entry("d2_420_abgr")
    handles.append(lib.mi355_sws_create_src(C.byref(p.ctx.desc), C.byref(p.src), p.fmt))
    try:
        assert all(handles)
        assert K.plan_of(lib, handles[0]) == want and K.plan_of(lib, handles[1]) == want
        assert K.plan_of(lib, handles[2]) == K.plan(lib, p)
    finally:
        for h in handles:
            lib.mi355_sws_destroy(C.c_void_p(h))


def test_planar_entry_points_return_minus_one(emu):
    lib = emu.lib
    lib.mi355_sws_scale_planar_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale_planar.argtypes = [C.c_void_p] * 5
    buf = (C.c_uint8 * 4096)()
    src, ss = (C.c_void_p * 3)(C.addressof(buf), C.addressof(buf), C.addressof(buf)), (C.c_int * 3)(128, 64, 64)
    for name in ("d2_420_bgr24", "d2_420_rgba", "ix_420_bgr24", "k_420_argb"):
        h = K.create(lib, K.stored_entry(name))
        assert h
        try:
            assert lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(h), buf, 1, None) == -1
            assert lib.mi355_sws_scale_planar(C.c_void_p(h), src, ss, src, ss) == -1
            lib.mi355_sws_dest_depth.argtypes = lib.mi355_sws_range.argtypes = [C.c_void_p]
            assert lib.mi355_sws_dest_depth(C.c_void_p(h)) == 8 and lib.mi355_sws_range(C.c_void_p(h)) == 0
        finally:
            lib.mi355_sws_destroy(C.c_void_p(h))


def test_rgb24_contexts_answer_as_before(emu):
    """format 0 through the creator: the twin's plan, destination format 0"""
    for name in ("d2_420_bgr24", "ix_nv21_argb_w128", "k_420_rgba"):
        p = K.plan(emu.lib, K.Entry.of(twin(K.stored_entry(name))))
        assert p["format"] == 0 and p == {**V.plan(emu.lib, twin(K.stored_entry(name))), "range": 0, "dst_depth": 8}, name


# ---- the describers on live contexts ---------------------------------------------------------------------------------------------------
@needs_sources
def test_describers_on_live_contexts(ref):
    lib = ref.lib
    flags = lib.ref_sws_flags_word(1, 1, 1)
    for name in K.NAMES:
        c = ref.open(name)
        e = ref.describe_packed(c)
        assert ref.declined_by_the_six_describers(c), name
        ref.free(c)
        assert e is not None and (e.layout, e.fmt) == (K.LAYOUTS.get(K.cfg(name)[4], 0), K.DSTS[K.cfg(name)[5]]), name
        # the new describer declines the rgb24 twin, which mi355_sws_describe_fmt takes
        c = ref.open_twin(name)
        assert ref.describe_packed(c) is None and ref.describe_fmt(c) is not None, name
        ref.free(c)
    full_chr, fast = 0x2000, (flags & ~0x7) | 0x1                 # SWS_FULL_CHR_H_INT, SWS_FAST_BILINEAR
    declined = [
        (128, 96, b"yuv420p", 64, 48, b"bgra", flags | full_chr),
        (128, 96, b"yuv420p", 64, 48, b"bgr24", flags | full_chr),
        (128, 96, b"yuv420p", 64, 48, b"rgba", fast),
        (128, 96, b"yuva420p", 64, 48, b"rgba", flags),          # alpha from the source
        (128, 96, b"yuv420p", 64, 48, b"rgb565le", flags),       # dithered, other tables
        (128, 96, b"yuv420p", 64, 48, b"rgb48le", flags),
        (128, 96, b"yuv420p", 64, 48, b"gbrp", flags),
        (128, 96, b"yuv420p12le", 64, 48, b"bgra", flags),
        (64, 48, b"rgb24", 64, 48, b"bgr24", flags),             # rgbToRgbWrapper
        (64, 48, b"bgr24", 64, 48, b"rgba", flags),
        (64, 48, b"yuv444p", 64, 48, b"bgra", lib.ref_sws_flags_word(1, 0, 0)),       # no special converter from 4:4:4: the generic scaler — taken below
    ]
    for args in declined[:-1]:
        c = ref.open_formats(args[0], args[1], args[2], args[3], args[4], args[5], args[6])
        assert ref.describe_packed(c) is None and ref.declined_by_the_six_describers(c), args
        ref.free(c)
    a = declined[-1]
    c = ref.open_formats(*a)
    e = ref.describe_packed(c)
    ref.free(c)
    assert e is not None and not e.ctx.desc.unscaled_special and e.fmt == 34


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return K.Ref(P.bind(K.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", K.BINDING)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = K.picture(name, "ramp", seed=5, pad=3)
    e = K.stored_entry(name)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    # the binding's describer knows every one of them, the refused one too (the creator refuses it, not the describer)
    c = hooked.open(name)
    d = hooked.describe_packed(c)
    hooked.free(c)
    assert d is not None and d.fmt == e.fmt, name
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    # a refused context is left to the reference: the picture counter does not move
    assert lib.ref_sws_pictures() == before + (1 if name in K.TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls
    assert not any(K.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("name", K.BINDING)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = K.picture(name, "noise", seed=6, pad=3)
    sizes = K.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    # the output entry of every destination row (the special converter has no inner loops to forward: the reference's function runs)
    assert lib.ref_sws_tier1_calls() >= before + (0 if name in K.SPECIAL else K.cfg(name)[3]), name
    assert lib.ref_sws_pictures() == pics
    assert not any(K.differing_rows(got, want, sizes)), name


def test_binding_rebuilds_a_32_bit_context_when_the_tables_change(hooked, ref, monkeypatch):
    """sws_setColorspaceDetails after the first picture: the binding compares the tables in the form the device context was built from"""
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    name = "d2_420_bgra"
    planes = K.picture(name, "noise", seed=7, pad=0)
    sizes = K.stored_entry(name).out_sizes()
    for h in (hooked, ref):
        h.lib.sws_getCoefficients.restype = C.c_void_p
        h.lib.sws_getCoefficients.argtypes = [C.c_int]
        h.lib.sws_setColorspaceDetails.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    before = hooked.lib.ref_sws_pictures()
    outs = []
    for h in (hooked, ref):
        c = h.open(name)
        first = h.scale_ctx(c, planes, sizes)
        coef = h.lib.sws_getCoefficients(1)                       # SWS_CS_ITU709
        assert h.lib.sws_setColorspaceDetails(c, coef, 0, coef, 0, 0, 1 << 16, 1 << 16) >= 0
        second = h.scale_ctx(c, planes, sizes)
        h.free(c)
        outs.append((first, second))
    assert hooked.lib.ref_sws_pictures() == before + 2            # both pictures on the device
    assert not any(K.differing_rows(outs[0][0], outs[1][0], sizes)) and not any(K.differing_rows(outs[0][1], outs[1][1], sizes))
    assert any(K.differing_rows(outs[1][0], outs[1][1], sizes))    # the tables did change
