"""GPU: 4:2:2 / 4:4:4 and 9 / 10-bit planar YUV sources of the device swscale path (include/mi355_sws.h: mi355_sws_create_src).

Every entry of tests/sws_sources.py on the contexts committed in tests/golden/sws_source_contexts.npz: Tier 1 (noise and the checkerboard
that reaches the clamp of the horizontal pass) and a guarded four-frame Tier-2 batch (source strides and plane starts off 16-byte and, for
the 16-bit sources, off 4-byte alignment; destination strides and plane offsets that defeat the 8-byte store) equal the reference's own
sws_scale() (oracle/_ref/libswsref.so), byte for byte.  The full-size entries at 64 distinct pictures in one launch, every picture
compared.  The binding (oracle/_ref/libswsref_gpu.so) in both forms, its counters moving exactly for the contexts the plan takes.  Nothing
under the reference's sources is read here."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_planar as P
import sws_sources as X

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (X.REF_LIB, X.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return X.Ref(P.bind(X.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    if not P.exports(X.REF_GPU_LIB, "mi355_sws_describe_src"):
        pytest.skip(X.REF_GPU_LIB + " was linked before mi355_sws_describe_src existed: __graft_entry__.build() relinks it where the reference exists")
    return X.Ref(P.bind(X.REF_GPU_LIB))


@pytest.mark.parametrize("name", X.SMALL)
def test_sources_batched_on_the_device(mi355, oracle, ref, name):
    p = X.check_batch(mi355.lib, oracle, ref, name, e=X.stored_entry(name))
    assert (p is None) == (name in X.REFUSED), (name, p)


@pytest.mark.parametrize("name", [n for n in X.SMALL if n not in X.REFUSED])
def test_sources_tier1(mi355, oracle, ref, name):
    e = X.stored_entry(name)
    h = X.create(mi355.lib, e)
    assert h
    try:
        sizes = e.out_sizes()
        for planes in (X.picture(name, seed=4, pad=7), X.checkerboard(name, pad=2)):
            want = X.expected(ref, oracle, name, e, planes)
            got = X.scale_tier1(mi355.lib, h, e, planes, pad=8)             # (the second picture reuses the context's device buffers)
            assert not any(X.differing_rows(got, want, sizes)), name
            assert all((g[:, w:] == 0x5A).all() for g, (w, _) in zip(got, sizes))
    finally:
        mi355.lib.mi355_sws_destroy(C.c_void_p(h))


def test_hscale16to15_on_the_device(mi355):
    e = X.stored_entry("r420d10_down2")
    coef, pos = e.ctx.banks["hLum"]
    n, fs = len(pos), len(coef) // len(pos)
    fn = mi355.lib.mi355_sws_hscale16to15
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    for depth, line in ((10, X.picture("r420d10_down2", seed=2)[0][0]), (10, X.checkerboard("r420d10_down2")[0][0]),
                        (9, X.picture("r420d10_down2", seed=3)[0][1] >> 1)):
        line = np.ascontiguousarray(line)
        out = np.zeros(n, np.int16)
        fn(out.ctypes.data, n, line.ctypes.data, coef.ctypes.data, pos.ctypes.data, fs, depth)
        idx = pos[:, None] + np.arange(fs)[None, :]
        want = np.minimum((line.astype(np.int64)[idx] * coef.reshape(n, fs).astype(np.int64)).sum(axis=1) >> (depth - 1), 32767)
        assert (out == want).all(), depth


@pytest.mark.parametrize("name", sorted(X.BIG))
def test_sources_full_size_64_pictures(mi355, ref, name):
    """64 distinct pictures in one launch (each a rolled copy of one random picture with its low bits flipped); every picture against the
    reference"""
    e = X.stored_entry(name)
    base = X.picture(name, seed=9)

    def pic(f):
        return [np.ascontiguousarray(np.roll(pl, 3 * f + 1, axis=1) ^ pl.dtype.type(f)) for pl in base]

    h = X.create(mi355.lib, e)
    assert h
    try:
        p = X.plan_of(mi355.lib, h)
        batch = X.Batch(mi355.lib, e, (pic(f) for f in range(64)), 64, src_offs=(0,))
        try:
            out = batch.run(h)
            assert batch.untouched(out), (name, p)
            c = ref.open(name)
            try:
                for f in range(64):
                    want = ref.scale_ctx(c, pic(f), batch.sizes)
                    assert not any(X.differing_rows(batch.frame(out, f), want, batch.sizes)), (name, p, f)
            finally:
                ref.free(c)
        finally:
            batch.close()
    finally:
        mi355.lib.mi355_sws_destroy(C.c_void_p(h))


# the inner-loop form is one Tier-1 launch per line: the full-size pictures take the whole-picture form only
BOUND = [(n, False) for n in X.SHAPES] + [(n, True) for n in X.SHAPES if n not in X.BIG and "special" not in n]


@pytest.mark.parametrize("name,lines", BOUND)
def test_sources_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = X.stored_entry(name)
    on_device = X.plan(mi355.lib, e) is not None
    assert on_device == (name not in X.REFUSED)
    planes = X.picture(name, seed=5, pad=3)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    if lines:
        assert lib.ref_sws_tier1_calls() > calls and lib.ref_sws_pictures() == pics, name
    else:
        assert lib.ref_sws_pictures() == pics + (1 if on_device else 0) and lib.ref_sws_tier1_calls() == calls, name
    assert not any(X.differing_rows(got, want, sizes)), name
