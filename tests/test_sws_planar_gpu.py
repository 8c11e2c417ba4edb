"""GPU: planar destinations of the device swscale path (include/mi355_sws.h: mi355_sws_create_planar, mi355_sws_scale_planar[_frames_dev]).

Every entry of tests/sws_planar.py through mi355_sws_scale_planar_frames_dev on four frames with their own source strides (pads 0, odd, 16,
odd), destination strides and plane offsets that defeat the 8-byte store, 0x5A before, between and after the planes: every row equals the
reference's own sws_scale() (oracle/_ref/libswsref.so; the edited entry: the model) on the contexts committed in tests/golden/sws_planar_contexts.npz, no guard byte changes, frame 3 equals frame 0.  The
full-size entries at 64 distinct pictures in one launch, a fixed sample compared.  The FATE vectors filter-scale200 / filter-scale500.  The
Tier-1 entry point.  The binding (oracle/_ref/libswsref_gpu.so) in both forms on every entry, its counters moving exactly for the contexts
the plan takes.  Nothing under the reference's sources is read here."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_planar as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (P.REF_LIB, P.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return P.Ref(P.bind(P.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    if not P.exports(P.REF_GPU_LIB, "mi355_sws_describe_planar"):
        pytest.skip(P.REF_GPU_LIB + " was linked before the planar binding existed: __graft_entry__.build() relinks it where the reference exists")
    return P.Ref(P.bind(P.REF_GPU_LIB))


@pytest.mark.parametrize("name", [n for n in P.NAMES if n not in P.BIG])
def test_planar_batched_on_the_device(mi355, oracle, ref, name):
    p = P.check_batch(mi355.lib, oracle, ref, name, use_model=False, ctx=P.stored_context(name))
    assert (p is None) == (name in P.REFUSED), (name, p)


@pytest.mark.parametrize("name", sorted(P.BIG))
def test_planar_full_size_64_pictures(mi355, ref, name):
    """64 distinct pictures in one launch (each a rolled and offset copy of one random picture); pictures 0, 37 and 63 against the reference"""
    ctx, fmt = P.stored_context(name), P.fmt_of(name)
    base = P.picture(name, seed=9)
    pics = [[np.ascontiguousarray(np.roll(pl, 3 * f + 1, axis=1) ^ np.uint8(f)) for pl in base] for f in range(64)]
    h = P.create(mi355.lib, ctx, fmt)
    assert h
    try:
        batch = P.Batch(mi355.lib, ctx, fmt, pics, dst_pads=(0, 5, 16, 3), gaps=(64, 67, 72, 61))
        try:
            out = batch.run(h)
            assert batch.untouched(out), name
            for f in (0, 37, 63):
                want = ref.scale(name, pics[f])
                assert not any(P.same_rows(batch.frame(out, f), want, batch.sizes)), (name, f)
        finally:
            batch.close()
    finally:
        mi355.lib.mi355_sws_destroy(C.c_void_p(h))


@pytest.mark.parametrize("vector", list(P.FATE))
def test_fate_scale_on_the_device(mi355, vector):
    ctx = P.fate_contexts()[vector]
    gold = P.fate_gold()["md5_per_frame"][vector]
    frames = P.fate_frames()
    h = P.create(mi355.lib, ctx, "420")
    assert h
    try:
        batch = P.Batch(mi355.lib, ctx, "420", frames)
        try:
            out = batch.run(h)
            assert batch.untouched(out)
            assert [P.md5_planes(batch.frame(out, f)) for f in range(len(frames))] == gold
        finally:
            batch.close()
        # ... and through the Tier-1 entry point
        sizes = P.plane_sizes(ctx, "420")
        got = [P.md5_planes([p[:, :w] for p, (w, _) in zip(P.scale_planar(mi355.lib, h, ctx, "420", f), sizes)]) for f in frames]
        assert got == gold
    finally:
        mi355.lib.mi355_sws_destroy(C.c_void_p(h))


@pytest.mark.parametrize("name", ["p420_w13_h11", "p444_unscaled", "p422_w385_h17", "p420_vdown12", "big_hd_to_720"])
def test_planar_tier1(mi355, ref, name):
    ctx, fmt = P.stored_context(name), P.fmt_of(name)
    planes = P.picture(name, seed=4, pad=7)
    h = P.create(mi355.lib, ctx, fmt)
    assert h
    try:
        got = P.scale_planar(mi355.lib, h, ctx, fmt, planes, pad=8)
        got2 = P.scale_planar(mi355.lib, h, ctx, fmt, planes, pad=8)         # the context's device buffers are reused
    finally:
        mi355.lib.mi355_sws_destroy(C.c_void_p(h))
    sizes = P.plane_sizes(ctx, fmt)
    want = ref.scale(name, planes)
    assert not any(P.same_rows(got, want, sizes))
    assert all((a == b).all() for a, b in zip(got, got2))
    assert all((g[:, w:] == 0x5A).all() for g, (w, _) in zip(got, sizes))


# the inner-loop form is one Tier-1 launch per line: the full-size pictures take the whole-picture form only
@pytest.mark.parametrize("name,lines", [(n, False) for n in P.SHAPES] + [(n, True) for n in P.SHAPES if n not in P.BIG])
def test_planar_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    ctx, fmt = P.stored_context(name), P.fmt_of(name)
    on_device = P.plan(mi355.lib, ctx, fmt) is not None
    planes = P.picture(name, seed=5, pad=3)
    want = ref.scale(name, planes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes)
    if lines:
        assert lib.ref_sws_tier1_calls() > calls and lib.ref_sws_pictures() == pics, name
    else:
        assert lib.ref_sws_pictures() == pics + (1 if on_device else 0) and lib.ref_sws_tier1_calls() == calls, name
    assert all((g == w).all() for g, w in zip(got, want)), name
