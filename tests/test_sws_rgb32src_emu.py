"""CPU: packed 32-bit sources (rgba / bgra / argb / abgr) of the device swscale path through the emulated product library.

The table of tests/sws_rgb32src.py must reach what its census lists (asserted from the plan, source, source-layout, destination, range, depth
and alpha queries and from the banks).  Every entry equals the reference's own sws_scale() of the same buffers through Tier 1 and through a
guarded four-frame Tier-2 batch whose packed planes lie on a 16-byte multiple and on a 4-byte multiple that is none of 16, at line pads of 0, 1,
4 and 3 pixels; the alpha rows also on alpha planes of noise, 0, 255 and a checkerboard, and with alpha 0 against the colour bytes with 255; the
line entries equal the reference's templates written out in numpy; fate-pixfmt-rgb32 and fate-pixfmt-bgr24 are reproduced with both stages on the
product; the creators refuse what lies outside the list."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_packeddst as K
import sws_planar as P
import sws_rgb32src as Q
import sws_rgbsrc as R

HAVE_REF_LIB = os.path.exists(Q.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        Q.make_fresh("_ref/libswsref.so")
    return Q.Ref(P.bind(Q.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: Q.plan(emu.lib, Q.stored_entry(name)) for name in Q.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_new_instance_family(plans):
    got = {n: p for n, p in plans.items() if p}
    cfgs = {n: Q.cfg(n) for n in Q.NAMES}
    for n, p in got.items():
        src, dst = cfgs[n][4:6]
        fmt, bits, _ = Q.DSTS[dst]
        assert (p["depth"], p["hsub"], p["vsub"], p["layout"]) == (8, Q.hsub_of(n), 0, Q.LAYOUTS[src]), (n, p)
        assert p["format"] == fmt and p["dst_depth"] == bits and p["range"] == (2 if dst in Q.RANGED else 0), (n, p)
        assert p["planes"] == (1 if dst in Q.PACKED else (2 if dst in ("nv12", "nv21") else 3)), (n, p)
        assert p["alpha"] == int(n in Q.ALPHA), (n, p)
    fam = lambda *dsts: {n: p for n, p in got.items() if cfgs[n][5] in dsts and n not in Q.ALPHA}     # noqa: E731
    rgb24, bgr24, planar, semi = fam("rgb24"), fam("bgr24"), fam("420", "422", "444"), fam("nv12", "nv21")
    deep, ranged, alpha = fam("420p10", "444p9"), fam(*Q.RANGED), {n: got[n] for n in Q.ALPHA}
    # k_sws_generic A / B / C x three destination forms (the 32-bit form through the alpha rows' colour-only twins, below), never k_sws_ident1
    assert {p["kernel"] for p in {**rgb24, **bgr24}.values()} == {"generic_a", "generic_b", "generic_c"} and rgb24 and bgr24
    assert {p["kernel"] for p in alpha.values()} >= {"generic_a", "generic_b"}
    # k_sws_planar A / B / C, both chroma widths, plain / SEMI / RANGE / DEEP
    assert {p["kernel"] for p in {**planar, **semi}.values()} == {"planar_a", "planar_b", "planar_c"}
    assert {cfgs[n][5] for n in planar} == {"420", "422", "444"} and {cfgs[n][5] for n in semi} == {"nv12", "nv21"}
    assert {cfgs[n][5] for n in deep} == {"420p10", "444p9"} and {cfgs[n][5] for n in ranged} == set(Q.RANGED)
    # the four byte orders, each to a packed and to a planar destination
    for group in ({**rgb24, **bgr24, **alpha}, {**planar, **semi, **deep, **ranged}):
        assert {cfgs[n][4] for n in group} == set(Q.LAYOUTS), sorted(group)
    assert {cfgs[n][5] for n in alpha} == set(Q.LAYOUTS)
    # the identity, staged and direct forms of the horizontal pass, for luma and for chroma
    forms = {n: Q.hforms(Q.stored_entry(n), p) for n, p in got.items()}
    for plane in (0, 1):
        reached = set().union(*(f[plane] for f in forms.values()))
        assert reached == {"identity", "staged", "direct"}, (plane, reached)
    for n, p in got.items():
        assert p["hstaged"] == int(any("staged" in f for f in forms[n])), (n, p, forms[n])
    # both converters, in front of identity and of filtered chroma banks
    for hsub in (0, 1):
        assert {"identity"} in [forms[n][1] for n in got if got[n]["hsub"] == hsub], hsub
        assert any("staged" in forms[n][1] for n in got if got[n]["hsub"] == hsub), hsub
    assert any(cfgs[n][9] & Q.SWS_FULL_CHR_H_INP for n in got)
    # the halving converter on an odd width (pixel srcW is read), odd sizes everywhere
    assert any(got[n]["hsub"] == 1 and cfgs[n][0] % 2 for n in got)
    for k in range(4):
        assert any(cfgs[n][k] % 2 for n in got), k
    # the alpha rows: the three templates, the wide and the narrow form, taps from memory
    e = {n: Q.stored_entry(n) for n in alpha}
    modes = {n: (e[n].ctx.desc.vLum.size, e[n].ctx.desc.vChr.size) for n in alpha}
    assert any(ls == 1 and cs <= 2 for ls, cs in modes.values()) and any(ls == 2 and cs == 2 for ls, cs in modes.values())
    assert any(2 < ls <= 8 for ls, _ in modes.values()) and any(ls > 8 for ls, _ in modes.values())
    assert {p["narrow"] for p in alpha.values()} == {0, 1}
    # the batch's planes hit both alignment classes, at the four line pads
    for n in ("q_420_same", "q_420_down2", "q_rgb_down2", "a_down2"):
        assert {Q.align_class(o, st) for o, st in Q.src_layouts(n)} == {16, 4}, (n, Q.src_layouts(n))
    assert Q.SRC_PADS == (0, 1, 4, 3)


def test_alpha_rows_have_their_colour_only_twins(emu):
    """the same descriptor with alpha 0: the twin's plan — its kernel value, th, lines — and alpha 0 in the query"""
    kernels = set()
    for n in sorted(Q.ALPHA):
        e = Q.stored_entry(n)
        a, c = Q.plan(emu.lib, e, alpha=1), Q.plan(emu.lib, e, alpha=0)
        assert a is not None and c is not None and (a["alpha"], c["alpha"]) == (1, 0), n
        assert {k: v for k, v in a.items() if k != "alpha"} == {k: v for k, v in c.items() if k != "alpha"}, n
        kernels.add(c["kernel"])
    assert kernels >= {"generic_a", "generic_b"}


def test_refused_entries_are_derived_from_the_table(plans):
    refused = {n for n, p in plans.items() if p is None}
    assert refused == Q.REFUSED, refused
    assert len(refused) * Q.REFUSED_CAP <= len(Q.NAMES), (len(refused), len(Q.NAMES))
    assert not refused & Q.FATE and not refused & Q.ALPHA
    # exactly the rows whose rgb24-source twins of tests/sws_rgbsrc.py are refused: the same sizes to the same destination family
    twins = {Q.cfg(n)[:4] + (("rgb",) if Q.cfg(n)[5] in ("rgb24", "bgr24") else (Q.cfg(n)[5],)) for n in refused}
    assert twins == {R.cfg(n)[:4] + (R.cfg(n)[5],) for n in ("s_rgb_vdown8", "s_420_vdown8")} and {"s_rgb_vdown8", "s_420_vdown8"} <= R.REFUSED


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    """every row is opened by the reference (open_formats asserts it) and described as the table expects; the committed arrays are those"""
    for name in Q.SHAPES:
        assert Q.stored_entry(name).same(ref.entry(name)), name
    for name in Q.FATE_EXTRA:
        assert Q.stored_fate_entry(name).same(Q.fate_extra_entry(ref, name)), name


@needs_sources
def test_alpha_context_tables_equal_the_colour_only_ones(ref):
    """a reference context that carries alpha builds its 32-bit table with 0 in the alpha lane (needAlpha, yuv2rgb.c): converted by the glue it is
    the table of the context to the same destination from rgb24 — which has no alpha — and of the one from yuv420p"""
    for name in sorted(Q.ALPHA):
        want = Q.stored_entry(name).ctx.luts
        for src in (b"rgb24", b"yuv420p"):
            c = ref.open_twin(name, src)
            twin = ref.describe_packed(c)
            ref.free(c)
            assert twin is not None, (name, src)
            for k in P.S.LUTS:
                assert (np.asarray(want[k]) == np.asarray(twin.ctx.luts[k])).all(), (name, src, k)


# ---- parity ------------------------------------------------------------------------------------------------------------------------
TAKEN = [n for n in Q.NAMES if n not in Q.REFUSED]
ALPHA = sorted(Q.ALPHA)


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_tier1_matches_reference(emu, ref, name):
    Q.check_tier1(emu.lib, ref, name, Q.tier1_pictures(name, seed=11))


@needs_ref
@pytest.mark.parametrize("pad", Q.SRC_PADS)
def test_emulated_tier1_odd_width_at_every_pad(emu, ref, pad):
    """the halving converter's read of pixel srcW: the next line's first pixel at pad 0, padding noise otherwise, the spare line on the last line"""
    Q.check_tier1(emu.lib, ref, "q_420_oddw", Q.tier1_pictures("q_420_oddw", seed=31 + pad, pads=(pad, pad, pad)))


@needs_ref
@pytest.mark.parametrize("name", TAKEN)
def test_emulated_batched(emu, ref, plans, name):
    p = Q.check_batch(emu.lib, ref, name, e=Q.stored_entry(name))
    assert p is not None and p == plans[name], name


@needs_ref
def test_emulated_odd_width_extra_pixel_in_the_next_frame(emu, ref):
    Q.check_contiguous(emu.lib, ref, "q_420_oddw")


@needs_ref
@pytest.mark.parametrize("name", ALPHA)
def test_emulated_alpha_planes(emu, ref, name):
    """alpha of noise, 0, 255, a checkerboard; one colour under noisy alpha; noisy colour under one alpha"""
    p = Q.check_batch(emu.lib, ref, name, e=Q.stored_entry(name), pictures=Q.alpha_pictures(name))
    assert p is not None and p["alpha"] == 1


@needs_ref
@pytest.mark.parametrize("name", ALPHA)
def test_emulated_alpha_0_is_colour_with_255(emu, ref, name):
    p = Q.check_batch(emu.lib, ref, name, e=Q.stored_entry(name), alpha=0)
    assert p is not None and p["alpha"] == 0
    Q.check_tier1(emu.lib, ref, name, [Q.picture(name, "noise", seed=41, pad=2)], alpha=0)


# ---- Tier 1: what it refuses ------------------------------------------------------------------------------------------------------------
def test_tier1_refuses_short_and_unaligned_planes(emu):
    lib = emu.lib
    lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.mi355_sws_scale.restype = C.c_int
    e = Q.stored_entry("q_rgb_down2")
    h = Q.create(lib, e)
    assert h
    try:
        buf = np.zeros(128 * 4 * 97 + 64, np.uint8)
        base = buf.ctypes.data + (-buf.ctypes.data) % 16
        out = np.zeros(64 * 3 * 48, np.uint8)

        def run(ptr, stride):
            src, ss = (C.c_void_p * 3)(ptr, None, None), (C.c_int * 3)(stride, 0, 0)
            return lib.mi355_sws_scale(C.c_void_p(h), src, ss, out.ctypes.data, 192)

        assert run(base, 512) == 48 and run(base + 4, 516) == 48
        assert run(base, 508) == -1                                # below the row
        for off in (1, 2, 3):
            assert run(base + off, 512) == -1 and run(base, 512 + off) == -1
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))


# ---- the line entries: no reference needed -----------------------------------------------------------------------------------------
def test_line_entries_match_the_templates_written_out(emu):
    assert Q.check_line_entries(emu.lib) > 0


def test_alpha_output_loops_match_the_templates_written_out(emu):
    assert Q.check_alpha_line_entries(emu.lib) == 4 * 9


def test_the_templates_written_out_agree_with_the_rgb24_arithmetic():
    """the issue's first observation, on the models alone: alpha masked off, the 32-bit templates give rgb24ToY_c / rgb24ToUV_c / rgb24ToUV_half_c
    of the three colour bytes — also under halving, whatever the alpha bytes carry"""
    for width in (5, 64):
        for order in Q.LAYOUTS:
            ir, ig, ib, _ = Q.ORDER[order]
            for label, src in Q.line_sources(2 * width, order):
                rgb = np.stack([src[ir::4], src[ig::4], src[ib::4]], axis=1).reshape(-1)
                assert (Q.model_y(src, width, order) == R.model_y(rgb, width, 0)).all(), (order, label)
                for half in (0, 1):
                    for a, b in zip(Q.model_uv(src, width, order, half), R.model_uv(rgb, width, 0, half)):
                        assert (a == b).all(), (order, label, half)


# ---- FATE: both stages on the product, no reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", sorted(Q.FATE_CHAINS))
def test_fate_pixfmt_both_stages(emu, chain):
    assert Q.fate_md5(emu, chain) == Q.fate_gold()["fate_pixfmt_%s_md5" % chain]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_creators_refuse_what_is_outside_the_list(emu):
    lib = emu.lib
    e = Q.stored_entry("q_420_down2")                                                # argb, halving
    assert Q.plan(lib, e) is not None and (e.layout, e.hsub) == (10, 1)
    for layout in (8, 9, 10, 11):
        assert Q.plan(lib, e.edited(layout=layout))["layout"] == layout             # the byte order is the caller's word
    for layout in (3, 6, 7, 12, -1):
        assert not Q.create(lib, e.edited(layout=layout)), layout
        assert not Q.create(lib, e.edited(layout=layout, range_=2)) and not Q.create(lib, e.edited(layout=layout, dst_depth=10)), layout
    assert not Q.create(lib, e.edited(depth=10))
    assert not Q.create(lib, e.edited(vsub=1)) and not Q.create(lib, e.edited(vsub=1, chrSrcH=48))
    assert not Q.create(lib, e.edited(chrSrcH=e.ctx.ints["srcH"] - 1))
    assert not Q.create(lib, e.edited(hsub=2)) and not Q.create(lib, e.edited(hsub=0))
    assert not Q.create(lib, e.edited(chrSrcW=e.ctx.ints["chrSrcW"] + 1))
    assert not Q.create(lib, e.edited(unscaled_special=1))
    assert not Q.create(lib, Q.stored_entry("q_rgb_down2").edited(unscaled_special=1))
    for fmt in list(range(4, 16)) + [18, 31, 37]:
        assert not Q.create(lib, e.edited(fmt=fmt)), fmt
    # a packed destination takes no range and no depth; a deep one no range
    rgb = Q.stored_entry("q_rgb_down2")
    assert not Q.create(lib, rgb.edited(range_=1)) and not Q.create(lib, rgb.edited(dst_depth=10))
    assert not Q.create(lib, Q.stored_entry("q_420p10_down2").edited(range_=2))
    # 32 in, packed RGB out, nothing scaled: the stored packed-destination entry of k_sws_ident1's shape under a 32-bit layout
    nv = K.stored_entry("i1_nv12_abgr_w126")
    assert K.plan(lib, nv)["kernel"] == "ident1_1"
    for layout in (8, 11):
        for fmt in (0, 32, 36):
            assert not Q.create(lib, Q.Entry(nv.ctx, 8, 1, 0, nv.dither, fmt, layout).edited(chrSrcH=nv.ctx.ints["srcH"])), (layout, fmt)
    # alpha 1: a 32-bit source to a 32-bit destination by the scaler, nothing else
    a = Q.stored_entry("a_down2")
    assert Q.plan(lib, a, alpha=1)["alpha"] == 1
    assert not Q.create(lib, a, alpha=2) and not Q.create(lib, a, alpha=-1)
    for fmt in (0, 32):
        assert not Q.create(lib, a.edited(fmt=fmt), alpha=1), fmt
    for name in ("q_420_down2", "q_nv21_down2", "q_420p10_down2", "q_j420_down2"):
        assert not Q.create(lib, Q.stored_entry(name), alpha=1), name
    assert not Q.create(lib, a.edited(unscaled_special=1), alpha=1)
    for name in ("d2_rgb_rgba", "d2_420_bgra", "d2_nv12_bgra", "d2_420d10_argb"):       # every source that is no 32-bit one
        k = K.stored_entry(name)
        assert not Q.create(lib, Q.Entry(k.ctx, k.depth, k.hsub, k.vsub, k.dither, k.fmt, k.layout), alpha=1), name
    # the queries on nothing; the entry points across context kinds
    lib.mi355_sws_alpha.argtypes = [C.c_void_p]
    assert lib.mi355_sws_alpha(None) == -1
    lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale_planar_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    buf = (C.c_uint8 * 1024)()
    for name, packed in (("q_rgb_down2", True), ("a_down2", True), ("q_420_down2", False), ("q_nv21_down2", False)):
        h = Q.create(lib, Q.stored_entry(name))
        assert h, name
        try:
            if packed:
                assert lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(h), buf, 1, None) == -1
            else:
                assert lib.mi355_sws_scale_frames_dev(C.c_void_p(h), buf, 1, None) == -1
        finally:
            lib.mi355_sws_destroy(C.c_void_p(h))


# ---- the describers on live contexts ---------------------------------------------------------------------------------------------------
@needs_sources
def test_describers_on_live_contexts(ref):
    lib = ref.lib
    flags = lib.ref_sws_flags_word(1, 1, 1)
    for name in Q.NAMES:
        c = ref.open(name)
        e = ref.describe(c)
        assert ref.declined_by_the_seven_describers(c), name                        # the seven existing describers keep declining these sources
        ref.free(c)
        assert e is not None and (e.layout, e.hsub, e.vsub, e.depth, e.alpha) == (Q.LAYOUTS[Q.cfg(name)[4]], Q.hsub_of(name), 0, 8, int(name in Q.ALPHA)), name
    declined = [
        (64, 48, b"rgba", 64, 48, b"rgba", flags),                              # the reference's plain copy
        (64, 48, b"bgra", 64, 48, b"rgba", flags),                              # rgbToRgbWrapper
        (64, 48, b"bgra", 64, 48, b"rgb24", flags),
        (96, 40, b"rgba", 64, 40, b"yuv420p", (flags & ~0x7) | 0x1),            # SWS_FAST_BILINEAR
        (96, 40, b"rgba", 64, 40, b"yuva420p", flags),                          # YUVA
        (96, 40, b"yuva420p", 64, 40, b"rgba", flags),
        (96, 40, b"rgb565le", 64, 40, b"yuv420p", flags),                       # 15 / 16-bit RGB
        (96, 40, b"rgb555le", 64, 40, b"rgba", flags),
        (96, 40, b"rgb24", 64, 40, b"yuv420p", flags),                          # the other describers' sources
        (96, 40, b"yuv420p", 64, 40, b"bgra", flags),
        (96, 40, b"rgba", 64, 40, b"rgb565le", flags),
        (96, 40, b"rgba", 64, 40, b"bgra", flags | 0x2000),                     # SWS_FULL_CHR_H_INT
    ]
    for args in declined:
        c = ref.open_formats(*args)
        assert ref.describe(c) is None, args
        ref.free(c)
    # to yuv420p at equal size the generic scaler runs whatever the flags (the reference has a ...ToYv12 wrapper for bgr24 alone), and is described
    for fl in (flags, lib.ref_sws_flags_word(1, 0, 1), lib.ref_sws_flags_word(0, 0, 0)):
        c = ref.open_formats(64, 48, b"bgra", 64, 48, b"yuv420p", fl)
        e = ref.describe(c)
        ref.free(c)
        assert e is not None and (e.layout, e.hsub, e.fmt, e.alpha, e.ctx.desc.unscaled_special) == (9, 1, 1, 0, 0), fl


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return Q.Ref(P.bind(Q.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", Q.BINDING)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = Q.picture(name, "ramp", seed=5, pad=3)
    sizes = Q.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    # the binding's describer knows every one of them, the refused one too (the creator refuses it, not the describer)
    c = hooked.open(name)
    e = hooked.describe(c)
    hooked.free(c)
    assert e is not None and (e.layout, e.hsub, e.fmt, e.alpha) == (Q.LAYOUTS[Q.cfg(name)[4]], Q.hsub_of(name), Q.DSTS[Q.cfg(name)[5]][0], int(name in Q.ALPHA)), name
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    # a refused context is left to the reference: the picture counter does not move
    assert lib.ref_sws_pictures() == before + (1 if name in Q.TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls
    assert not any(Q.differing_rows(got, want, sizes)), name


def test_binding_leaves_an_unaligned_plane_to_the_reference(hooked, ref, monkeypatch):
    """a stride that is a multiple of 4 goes to the device, a picture two bytes into its buffer (the reference reads it all the same) does not"""
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    name = "q_rgb_down2"
    sw, sh = Q.cfg(name)[:2]
    sizes = Q.stored_entry(name).out_sizes()
    buf = np.zeros((sh + 1) * 4 * sw + 64, np.uint8)
    base = (-buf.ctypes.data) % 16
    for skew, taken in ((0, 1), (2, 0)):
        plane = buf[base + skew:base + skew + sh * 4 * sw].reshape(sh, 4 * sw)
        plane[:] = Q.picture(name, "noise", seed=8)[0]
        before = hooked.lib.ref_sws_pictures()
        got = hooked.scale(name, [plane], sizes)
        assert hooked.lib.ref_sws_pictures() == before + taken, skew
        assert not any(Q.differing_rows(got, ref.scale(name, [plane], sizes), sizes)), skew


@pytest.mark.parametrize("name", Q.BINDING)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = Q.picture(name, "noise", seed=6, pad=3)
    sizes = Q.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_tier1_calls() > before, name
    assert lib.ref_sws_pictures() == pics
    assert not any(Q.differing_rows(got, want, sizes)), name
