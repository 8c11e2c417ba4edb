"""CPU: planar destinations (yuv420p -> yuv420p / yuv422p / yuv444p) of the device swscale path through the emulated product library.

The table of tests/sws_planar.py must reach every planar kernel instance, three or more tile heights, both horizontal passes, both tile forms
and a context mi355_sws_create_planar refuses.  On every small entry the model (swscale()'s planar branch over the oracle's line functions)
equals the reference's own sws_scale(), and so do mi355_sws_scale_planar and a guarded four-frame mi355_sws_scale_planar_frames_dev batch.
The FATE vectors filter-scale200 / filter-scale500 (frames 0-4) are reproduced from the committed frames and contexts, by the model and by
the emulated product; where the reference's sources exist the frames and md5s are derived again from them.  The binding
(oracle/_ref/libswsref_tier1.so) gives the plain reference's bytes in both of its forms."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_planar as P

HAVE_REF_LIB = os.path.exists(P.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        P.make_fresh("_ref/libswsref.so")
    return P.Ref(P.bind(P.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: P.plan(emu.lib, P.stored_context(name), P.fmt_of(name)) for name in P.NAMES}


# ---- the FATE vectors (no reference library needed) ----------------------------------------------------------------------------
@pytest.mark.parametrize("vector", list(P.FATE))
def test_fate_scale_model(oracle, vector):
    """filter-scale200 / filter-scale500: the model on the committed frames and contexts gives the reference's per-frame md5s.  (The FATE
    md5 itself covers a NUT container, which is out of scope.)"""
    ctx = P.fate_contexts()[vector]
    gold = P.fate_gold()["md5_per_frame"][vector]
    assert [P.md5_planes(P.model(oracle, ctx, "420", f)) for f in P.fate_frames()] == gold


@pytest.mark.parametrize("vector", list(P.FATE))
def test_fate_scale_emulated(emu, vector):
    ctx = P.fate_contexts()[vector]
    gold = P.fate_gold()["md5_per_frame"][vector]
    frames = P.fate_frames()
    h = P.create(emu.lib, ctx, "420")
    assert h
    try:
        assert P.plan_of(emu.lib, h)["kernel"].startswith("planar")
        got = [P.md5_planes([p[:, :w] for p, (w, _) in zip(P.scale_planar(emu.lib, h, ctx, "420", f), P.plane_sizes(ctx, "420"))]) for f in frames]
    finally:
        emu.lib.mi355_sws_destroy(C.c_void_p(h))
    assert got == gold


@pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources")
def test_fate_golden_rederived_from_the_reference(ref):
    frames = P.make_fate_frames()
    committed = P.fate_frames()
    for a, b in zip(frames, committed):
        assert all((x == y).all() for x, y in zip(a, b))
    ctxs, md5s = P.fate_reference(ref, frames)
    assert md5s == P.fate_gold()["md5_per_frame"]
    for name, ctx in ctxs.items():
        want = P.fate_contexts()[name]
        for k in P.S.BANKS:
            assert all((a == b).all() for a, b in zip(ctx.banks[k], want.banks[k])), (name, k)


def test_rgb_entry_points_refuse_a_planar_context(emu):
    """a planar context is not an rgb24 one and the reverse: each entry point returns -1 on the other kind"""
    ctx = P.fate_contexts()["scale200"]
    lib = emu.lib
    h = P.create(lib, ctx, "420")
    assert h
    try:
        lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        assert lib.mi355_sws_scale_frames_dev(C.c_void_p(h), C.c_void_p(16), 1, None) == -1
        src = (C.c_void_p * 3)(16, 16, 16)
        st = (C.c_int * 3)(4096, 4096, 4096)
        lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        assert lib.mi355_sws_scale(C.c_void_p(h), src, st, C.c_void_p(16), 1 << 20) == -1
        lib.mi355_sws_scale_planar_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        assert lib.mi355_sws_scale_planar_frames_dev(None, C.c_void_p(16), 1, None) == -1
        assert lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(h), None, 1, None) == -1
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))
    import sws_shapes as T
    rgb = T.S.load_context("generic_64x48")
    h = T.create(lib, rgb)
    assert h
    try:
        assert lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(h), C.c_void_p(16), 1, None) == -1
        lib.mi355_sws_scale_planar.argtypes = [C.c_void_p] * 5
        src = (C.c_void_p * 3)(16, 16, 16)
        st = (C.c_int * 3)(4096, 4096, 4096)
        assert lib.mi355_sws_scale_planar(C.c_void_p(h), src, st, src, st) == -1
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))
    # an unknown destination format
    lib.mi355_sws_create_planar.restype = C.c_void_p
    lib.mi355_sws_create_planar.argtypes = [C.c_void_p, C.c_int]
    assert not lib.mi355_sws_create_planar(C.byref(ctx.desc), 4)


# ---- the table (the committed contexts: no reference library needed) -------------------------------------------------------------
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


def test_table_reaches_every_branch(plans):
    got = [p for p in plans.values() if p]
    assert {p["kernel"] for p in got} == set(P.KERNELS.values()), plans
    assert len({p["th"] for p in got}) >= 3, plans
    assert {1, 16} <= {p["th"] for p in got}, plans
    assert {p["hstage"] for p in got} == {0, 1}, plans
    assert {p["narrow"] for p in got} == {0, 1}, plans
    assert {n for n, p in plans.items() if p is None} == P.REFUSED
    # every instance of every chroma tile width
    for fmts in (("420", "422"), ("444",)):
        assert {p["kernel"] for n, p in plans.items() if p and P.fmt_of(n) in fmts} == set(P.KERNELS.values()), (fmts, plans)
    assert {P.fmt_of(n) for n in P.NAMES} == set(P.FMTS)
    assert plans["psynth_hstage0"]["hstage"] == 0 and plans["p420_honly"]["hstage"] == 1


@needs_sources
def test_committed_contexts_match_the_reference(ref):
    """tests/golden/sws_planar_contexts.npz (what the GPU tests run) holds the contexts the reference builds for the table"""
    for name in P.SHAPES:
        got, want = P.stored_context(name), P.context(ref, name)
        assert got.ints == want.ints, name
        for k in P.S.BANKS:
            assert all((a == b).all() for a, b in zip(got.banks[k], want.banks[k])), (name, k)


@needs_sources
def test_describe_declines_what_the_kernel_does_not_restate(ref):
    """SWS_FAST_BILINEAR and an rgb24 destination are not planar contexts of this path; an unscaled yuv420p -> yuv420p context is a plane copy"""
    c = ref.open_shape(96, 40, 64, 40, "420", 1, 1, 1, fast_bilinear=True)
    assert ref.describe(c) is None
    ref.free(c)
    lib = ref.lib
    c = lib.sws_getContext(64, 48, lib.ref_pix_fmt(0), 64, 48, lib.ref_pix_fmt(1), lib.ref_sws_flags_word(1, 1, 1), None, None, None)
    assert ref.describe(c) is None
    ref.free(c)
    c = ref.open_shape(64, 48, 64, 48, "420", 1, 1, 1)
    assert ref.describe(c) is None
    ref.free(c)


SMALL = P.SMALL


@needs_ref
@pytest.mark.parametrize("name", SMALL)
def test_model_matches_reference(oracle, ref, name):
    ctx = P.stored_context(name)
    planes = P.picture(name, seed=11, pad=5)
    got = P.model(oracle, ctx, P.fmt_of(name), planes)
    if name in P.SHAPES:
        want = ref.scale(name, planes)
        assert not any(P.same_rows(got, want, P.plane_sizes(ctx, P.fmt_of(name))))


@needs_ref
@pytest.mark.parametrize("name", SMALL)
def test_emulated_tier1_matches_reference(emu, oracle, ref, plans, name):
    if plans[name] is None:
        return
    ctx, fmt = P.stored_context(name), P.fmt_of(name)
    planes = P.picture(name, seed=11, pad=5)
    want = ref.scale(name, planes) if name in P.SHAPES else P.model(oracle, ctx, fmt, planes)
    h = P.create(emu.lib, ctx, fmt)
    try:
        got = P.scale_planar(emu.lib, h, ctx, fmt, planes, pad=8)
    finally:
        emu.lib.mi355_sws_destroy(C.c_void_p(h))
    sizes = P.plane_sizes(ctx, fmt)
    assert not any(P.same_rows(got, want, sizes))
    assert all((g[:, w:] == 0x5A).all() for g, (w, _) in zip(got, sizes))       # the caller's padding untouched


@needs_ref
@pytest.mark.parametrize("name", SMALL)
def test_emulated_batched(emu, oracle, ref, plans, name):
    assert P.check_batch(emu.lib, oracle, ref, name, use_model=False, ctx=P.stored_context(name)) == plans[name]


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("/root/reference not present")
    return P.Ref(P.bind(P.make_fresh("_ref/libswsref_tier1.so")))


BINDING = ["p420_w13_h11", "p422_w127", "p444_unscaled", "p420_honly", "p420_down4", "p420_vdown16", "p422_up"]


@pytest.mark.parametrize("name", BINDING)
def test_binding_whole_pictures(hooked, ref, plans, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = P.picture(name, seed=5, pad=3)
    want = ref.scale(name, planes)
    lib = hooked.lib
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes)
    assert lib.ref_sws_pictures() == before + (1 if plans[name] else 0), name
    assert lib.ref_sws_tier1_calls() == calls
    assert all((g == w).all() for g, w in zip(got, want)), name


@pytest.mark.parametrize("name", BINDING)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = P.picture(name, seed=6, pad=3)
    want = ref.scale(name, planes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes)
    assert lib.ref_sws_tier1_calls() > before
    assert lib.ref_sws_pictures() == pics
    assert all((g == w).all() for g, w in zip(got, want)), name
