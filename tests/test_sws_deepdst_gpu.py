"""GPU: 9- and 10-bit planar destinations of the device swscale path (include/mi355_sws.h).

Every entry of tests/sws_deepdst.py on the contexts committed in tests/golden/sws_deepdst_contexts.npz: a guarded six-frame Tier-2 batch (noise,
the two-pixel checkerboard, the ramp, the noise at other strides, all-0 and all-maximum planes; destination planes on a 16-byte multiple, on a
4-byte multiple that is no multiple of 16 and on a 2-byte multiple that is no multiple of 4, at line pads of 0, 5, 16 and 3 samples) equals the
reference's own sws_scale() of the same buffers (oracle/_ref/libswsref.so), byte for byte, over the whole rounded-up extent of every
destination plane, and no byte outside the written samples changes; one Tier-1 call per depth and subsampling; the two line entries against
the two formulas written out; the binding (oracle/_ref/libswsref_gpu.so) in both forms.  Nothing under the reference's sources is read here."""
import os

import pytest

import sws_deepdst as D
import sws_planar as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (D.REF_LIB, D.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return D.Ref(P.bind(D.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    # a library linked from an older binding declines every deep context (and its sws_scale() is then the plain reference's): ask the
    # library itself, as tests/test_sws_range_gpu.py does — the binding can only be relinked where the reference's sources are
    if not P.exports(D.REF_GPU_LIB, D.DESCRIBER):
        pytest.skip(D.REF_GPU_LIB + " was linked before the binding took deep destinations: __graft_entry__.build() relinks it where the reference exists")
    return D.Ref(P.bind(D.REF_GPU_LIB))


TAKEN = [n for n in D.NAMES if n not in D.REFUSED]
# one Tier-1 call per depth and subsampling, a deeper, a semi-planar and a packed source among them
TIER1 = ["e_420_422d10_same", "d2_420d10_420d10", "d2_444d10_444d10", "d2_nv21_422d9", "w127_rgb_420d9", "v6_420d10_444d9"]


@pytest.mark.parametrize("name", TAKEN)
def test_deepdst_batched_on_the_device(mi355, ref, name):
    p = D.check_batch(mi355.lib, ref, name, e=D.stored_entry(name))
    assert p is not None and p["dst_depth"] == D.dst_kind(name)[1] and p["range"] == 0, name


@pytest.mark.parametrize("name", TIER1)
def test_deepdst_tier1(mi355, ref, name):
    # (the second picture reuses the context's device buffers)
    D.check_tier1(mi355.lib, ref, name, [D.picture(name, "noise", seed=4, pad=0), D.picture(name, "checker", seed=5, pad=2)])


def test_deepdst_refused_on_the_device(mi355):
    """the real library refuses what the emulated one refuses, and nothing else of the table"""
    assert {n for n in D.NAMES if D.plan(mi355.lib, D.stored_entry(n)) is None} == D.REFUSED


def test_deepdst_line_entries_on_the_device(mi355):
    assert D.check_line_entries(mi355.lib) > 0


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", D.BINDING)
def test_deepdst_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = D.stored_entry(name)
    planes = D.picture(name, "ramp", seed=5, pad=3)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    if lines:
        assert lib.ref_sws_tier1_calls() > calls and lib.ref_sws_pictures() == pics, name
    else:
        assert lib.ref_sws_pictures() == pics + (0 if name in D.REFUSED else 1) and lib.ref_sws_tier1_calls() == calls, name
    assert not any(D.differing_rows(got, want, sizes)), name
