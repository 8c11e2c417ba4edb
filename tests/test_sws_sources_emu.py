"""CPU: 4:2:2 / 4:4:4 and 9 / 10-bit planar YUV sources of the device swscale path (mi355_sws_create_src) through the emulated product library.

The table of tests/sws_sources.py must reach what its census lists (asserted from the plan and source queries).  Every small entry equals
the reference's own sws_scale() through Tier 1 and through a guarded four-frame Tier-2 batch; the committed contexts are the reference's;
depth 8 / 4:2:0 through mi355_sws_create_src is the context of the existing entry points; the binding declines what the kernels do not
restate and gives the plain reference's bytes in both of its forms (oracle/_ref/libswsref_tier1.so)."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_planar as P
import sws_sources as X

HAVE_REF_LIB = os.path.exists(X.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        X.make_fresh("_ref/libswsref.so")
    return X.Ref(P.bind(X.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: X.plan(emu.lib, X.stored_entry(name)) for name in X.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_what_the_issue_lists(plans):
    got = {n: p for n, p in plans.items() if p}
    cfgs = {n: X.cfg(n) for n in X.NAMES}
    # each subsampling at each depth, and the queries say so
    assert {(c[4], c[5]) for n, c in cfgs.items() if n in got} == {(s, d) for s in X.SUBS for d in (8, 9, 10)}
    for n, p in got.items():
        assert (p["depth"], (p["hsub"], p["vsub"])) == (cfgs[n][5], X.SUBS[cfgs[n][4]]), (n, p)
    # rgb24 and each planar destination, from 16-bit samples
    assert {cfgs[n][6] for n, p in got.items() if p["depth"] > 8} == set(X.DSTS)
    # every generic and planar instance, at 16 bits
    deep = {n: p for n, p in got.items() if p["depth"] > 8}
    assert {p["kernel"] for p in deep.values()} == set(X.KERNELS[3:]), {n: p["kernel"] for n, p in deep.items()}
    # the special converter and both forms of k_sws_ident1 on 8-bit 4:2:2
    assert {p["kernel"] for n, p in got.items() if (cfgs[n][4], cfgs[n][5]) == ("422", 8)} >= {"c24", "ident1_1", "ident1_x"}
    # staged and direct horizontal passes at 16 bits (tile kernels only stage)
    assert {p["hstaged"] for p in deep.values()} == {0, 1}
    for dst in ("rgb", "420"):
        assert {p["hstaged"] for n, p in deep.items() if cfgs[n][6] == dst} == {0, 1}, dst
    # both tile forms
    for planar in (False, True):
        assert {p["narrow"] for n, p in deep.items() if (cfgs[n][6] != "rgb") == planar} == {0, 1}, planar
    # one-tap and multi-tap vertical banks on a dithered destination
    taps = {(min(e.ctx.desc.vLum.size, 2), min(e.ctx.desc.vChr.size, 2)) for n, e in ((n, X.stored_entry(n)) for n in deep) if e.fmt}
    assert {t[0] for t in taps} == {1, 2} and {t[1] for t in taps} == {1, 2}, taps
    # tile heights 16 down to 1
    assert {p["th"] for p in deep.values()} >= {16, 8, 4, 2, 1}, {n: p["th"] for n, p in deep.items()}
    # widths on and off the 128-column tiles; odd srcW with 4:2:2, odd srcH with 4:2:0
    assert any(cfgs[n][2] % 128 == 0 for n in deep) and any(cfgs[n][2] % 128 for n in deep)
    assert any(cfgs[n][4] == "422" and cfgs[n][0] % 2 for n in deep) and any(cfgs[n][4] == "420" and cfgs[n][1] % 2 for n in deep)
    # planes and strides off 16-byte, and for 16-bit off 4-byte, alignment (the batch's layouts)
    for n in deep:
        lay = X.src_layouts(n)
        assert any((o | st) % 16 for o, st in lay), n
    assert any(any((o | st) % 4 == 2 for o, st in X.src_layouts(n)) for n in deep)
    assert any(all((o | st) % 16 == 0 for o, st in X.src_layouts(n)[:1]) for n in deep if got[n]["hstaged"])


def test_refused_entries_are_named_and_few(plans):
    refused = {n for n, p in plans.items() if p is None}
    assert refused == X.REFUSED, refused
    assert len(refused) * X.REFUSED_CAP <= len(X.NAMES), (len(refused), len(X.NAMES))
    assert not refused & (X.BIG | X.CHAIN)


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    for name in X.SHAPES:
        assert X.stored_entry(name).same(ref.entry(name)), name


@needs_ref
@pytest.mark.parametrize("depth", [9, 10])
def test_checkerboard_reaches_the_clamp_of_the_horizontal_pass(ref, depth):
    """the reference's own 15-bit lines (c->hyScale: hScale16To15_c) of the checkerboard reach 32767"""
    name = {9: "r420d9_w257_h37", 10: "r420d10_w384_up"}[depth]
    assert X.cfg(name)[5] == depth
    assert ref.hscale_max(name, X.checkerboard(name)) == 32767
    assert ref.hscale_max(name, X.picture(name, seed=1)) <= 32767


# ---- parity ------------------------------------------------------------------------------------------------------------------------
SMALL = X.SMALL


@needs_ref
@pytest.mark.parametrize("name", SMALL)
def test_emulated_tier1_matches_reference(emu, oracle, ref, plans, name):
    if plans[name] is None:
        assert name in X.REFUSED
        return
    e = X.stored_entry(name)
    h = X.create(emu.lib, e)
    try:
        for planes in (X.picture(name, seed=11, pad=5), X.checkerboard(name, pad=2)):
            want = X.expected(ref, oracle, name, e, planes)
            got = X.scale_tier1(emu.lib, h, e, planes, pad=8)
            sizes = e.out_sizes()
            assert not any(X.differing_rows(got, want, sizes)), name
            assert all((g[:, w:] == 0x5A).all() for g, (w, _) in zip(got, sizes))       # the caller's padding untouched
    finally:
        emu.lib.mi355_sws_destroy(C.c_void_p(h))


@needs_ref
@pytest.mark.parametrize("name", SMALL)
def test_emulated_batched(emu, oracle, ref, plans, name):
    assert X.check_batch(emu.lib, oracle, ref, name, e=X.stored_entry(name)) == plans[name]


# ---- depth 8 / 4:2:0: the context of the existing entry points ----------------------------------------------------------------------
def test_depth8_420_is_the_existing_context(emu):
    import sws_shapes as T
    lib = emu.lib
    dither = np.zeros(64, np.uint8)
    for name in ("generic_64x48", "down2_128x96", "special_70x50", "up2_bilinear"):
        ctx = T.S.load_context(name)
        e = X.Entry(ctx, 8, 1, 1, dither, 0)
        old, new = T.create(lib, ctx), X.create(lib, e)
        assert old and new
        try:
            po, pn = T.plan_of(lib, old), X.plan_of(lib, new)
            assert {k: pn[k] for k in po} == po and (pn["depth"], pn["hsub"], pn["vsub"]) == (8, 1, 1), (name, po, pn)
            planes = T.S.picture(name, stride_pad=3)
            a = X.scale_tier1(lib, old, e, planes)
            b = X.scale_tier1(lib, new, e, planes)
            assert (a[0] == b[0]).all(), name
        finally:
            lib.mi355_sws_destroy(C.c_void_p(old))
            lib.mi355_sws_destroy(C.c_void_p(new))
    for name in ("p420_w13_h11", "p444_unscaled", "p422_w385_h17"):
        ctx, fmt = P.stored_context(name), P.fmt_of(name)
        e = X.Entry(ctx, 8, 1, 1, dither, P.FMTS[fmt])
        old, new = P.create(lib, ctx, fmt), X.create(lib, e)
        assert old and new
        try:
            po, pn = P.plan_of(lib, old), X.plan_of(lib, new)
            assert {k: pn[k] for k in po} == po, (name, po, pn)
            planes = P.picture(name, seed=3, pad=5)
            a, b = P.scale_planar(lib, old, ctx, fmt, planes), X.scale_tier1(lib, new, e, planes)
            assert all((x == y).all() for x, y in zip(a, b)), name
        finally:
            lib.mi355_sws_destroy(C.c_void_p(old))
            lib.mi355_sws_destroy(C.c_void_p(new))


def test_create_src_refuses_what_is_outside_the_list(emu):
    e = X.stored_entry("r420d10_down2")
    for depth, hsub, vsub in ((12, 1, 1), (7, 1, 1), (10, 0, 1), (10, 2, 1), (10, 0, 0)):       # (the last: not this descriptor's chroma size)
        assert not X.create(emu.lib, X.Entry(e.ctx, depth, hsub, vsub, e.dither, 0)), (depth, hsub, vsub)
    assert not X.create(emu.lib, X.Entry(e.ctx, 10, 1, 1, e.dither, 4))
    sp = X.stored_entry("r422d8_special")
    assert not X.create(emu.lib, X.Entry(sp.ctx, 10, 1, 0, sp.dither, 0))                       # no deeper source takes the special converter
    emu.lib.mi355_sws_source.argtypes = [C.c_void_p, C.c_void_p]
    assert emu.lib.mi355_sws_source(None, None) == -1


def test_hscale16to15_line_entry(emu):
    """the Tier-1 line entry against the arithmetic of hScale16To15_c written out in numpy"""
    e = X.stored_entry("r420d10_down2")
    coef, pos = e.ctx.banks["hLum"]
    n, fs = len(pos), len(coef) // len(pos)
    for depth, line in ((10, X.picture("r420d10_down2", seed=2)[0][0]), (10, X.checkerboard("r420d10_down2")[0][0]),
                        (9, X.picture("r420d10_down2", seed=3)[0][1] >> 1)):
        line = np.ascontiguousarray(line)
        out = np.zeros(n, np.int16)
        emu.lib.mi355_sws_hscale16to15.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
        emu.lib.mi355_sws_hscale16to15(out.ctypes.data, n, line.ctypes.data, coef.ctypes.data, pos.ctypes.data, fs, depth)
        idx = pos[:, None] + np.arange(fs)[None, :]
        want = np.minimum((line.astype(np.int64)[idx] * coef.reshape(n, fs).astype(np.int64)).sum(axis=1) >> (depth - 1), 32767)
        assert (out == want).all(), depth


# ---- what the binding declines -------------------------------------------------------------------------------------------------------
@needs_sources
def test_describe_src_declines_what_the_kernels_do_not_restate(ref):
    lib = ref.lib
    flags = lib.ref_sws_flags_word(1, 1, 1)
    declined = [
        (64, 48, b"yuv420p10le", 64, 48, b"yuv420p", flags),                    # a plane copy (planarCopyWrapper): no filter banks
        (64, 48, b"yuv420p", 64, 48, b"yuv420p", flags),                        # ... the 8-bit one
        (96, 40, b"yuv420p10be", 64, 40, b"rgb24", flags),                      # a big-endian source
        (96, 40, b"yuv420p12le", 64, 40, b"rgb24", flags),                      # a 12-bit source
        (96, 40, b"yuv422p", 64, 40, b"yuv420p", (flags & ~0x7) | 0x1),         # SWS_FAST_BILINEAR (hyscale_fast: 8-bit sources only, swscale.c:737)
        (96, 40, b"yuv444p", 64, 40, b"rgb24", (flags & ~0x7) | 0x1),
        (96, 40, b"yuv422p10le", 64, 40, b"yuv420p10le", flags),                # an output deeper than 8 bits
        (96, 40, b"nv12", 64, 40, b"rgb24", flags),                             # a semi-planar source
        (96, 40, b"yuv444p", 64, 40, b"bgr24", flags),
    ]
    for args in declined:
        c = ref.open_formats(*args)
        assert ref.describe(c) is None, args
        ref.free(c)
    taken = [(96, 40, b"yuv422p10le", 64, 40, b"yuv420p", flags), (64, 48, b"yuv422p", 64, 48, b"rgb24", lib.ref_sws_flags_word(1, 0, 0)),
             (96, 40, b"yuv420p", 64, 40, b"rgb24", flags)]
    for args in taken:
        c = ref.open_formats(*args)
        assert ref.describe(c) is not None, args
        ref.free(c)
    # the existing describers keep their answers: yuv420p only
    lib.ref_sws_describe.argtypes = [C.c_void_p, C.c_void_p]
    c = ref.open_formats(96, 40, b"yuv422p", 64, 40, b"rgb24", flags)
    assert lib.ref_sws_describe(c, C.byref(P.S.Desc())) != 0
    ref.free(c)
    c = ref.open_formats(96, 40, b"yuv420p10le", 64, 40, b"yuv420p", flags)
    assert P.Ref(lib).describe(c) is None
    ref.free(c)


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("/root/reference not present")
    return X.Ref(P.bind(X.make_fresh("_ref/libswsref_tier1.so")))


BINDING = ["r420d10_down2", "r422d10_w129_oddw", "r444d9_w256_unscaled", "r422d8_special_w70", "r422d8_ident1", "r444d8_down",
           "p420d10_to420_honly", "p422d10_to420_w385", "p444d10_to444_w129", "p422d8_to420_unscaled"] + sorted(X.REFUSED)


@pytest.mark.parametrize("name", BINDING)
def test_binding_whole_pictures(hooked, ref, plans, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = X.picture(name, seed=5, pad=3)
    sizes = X.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_pictures() == before + (1 if plans[name] else 0), name        # a refused context is left to the reference
    assert lib.ref_sws_tier1_calls() == calls
    assert not any(X.differing_rows(got, want, sizes)), name


@pytest.mark.parametrize("name", [n for n in BINDING if "special" not in n])
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = X.picture(name, seed=6, pad=3)
    sizes = X.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_tier1_calls() > before
    assert lib.ref_sws_pictures() == pics
    assert not any(X.differing_rows(got, want, sizes)), name
