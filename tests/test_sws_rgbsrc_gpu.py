"""GPU: packed rgb24 / bgr24 sources of the device swscale path (include/mi355_sws.h).

Every entry of tests/sws_rgbsrc.py on the contexts committed in tests/golden/sws_rgbsrc_contexts.npz: a guarded four-frame Tier-2 batch
(packed planes on a 16-byte multiple, on a 4-byte multiple and on an odd address, at line pads 0, 3, 16 and 7) equals the reference's own
sws_scale() of the same buffers (oracle/_ref/libswsref.so), byte for byte, over the whole rounded-up extent of every destination plane; one
Tier-1 call per destination kind, and the odd width whose halving converter reads pixel srcW; the two line entries against their arithmetic
written out; the FATE pin with both stages on the device; the binding (oracle/_ref/libswsref_gpu.so) in both forms.  Nothing under the
reference's sources is read here."""
import json
import os

import pytest

import sws_planar as P
import sws_rgbsrc as R

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(P.GOLDEN, "sws_ref_sha1.json")))


@pytest.fixture(scope="module")
def ref():
    for p in (R.REF_LIB, R.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return R.Ref(P.bind(R.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    # a library linked from an older binding declines every packed RGB source (and its sws_scale() is then the plain reference's): ask the
    # library itself, as tests/test_sws_nv12_gpu.py does
    lib = R.Ref(P.bind(R.REF_GPU_LIB))
    c = lib.open("s_420_same") if P.exports(R.REF_GPU_LIB, R.DESCRIBER) else None
    new = c is not None and lib.describe(c) is not None
    if c:
        lib.free(c)
    if not new:
        pytest.skip(R.REF_GPU_LIB + " was linked before the binding took rgb24 / bgr24 sources: __graft_entry__.build() relinks it where the reference exists")
    return lib


TAKEN = [n for n in R.NAMES if n not in R.REFUSED]
# one Tier-1 call per destination kind, and the odd width
TIER1 = ["s_rgb_down2", "s_420_down2", "s_422_w127", "s_444_w129_up", "s_nv12_same", "s_nv21_down2", "s_420_oddw"]


@pytest.mark.parametrize("name", TAKEN)
def test_rgbsrc_batched_on_the_device(mi355, ref, name):
    assert R.check_batch(mi355.lib, ref, name, e=R.stored_entry(name)) is not None, name


@pytest.mark.parametrize("name", TIER1)
def test_rgbsrc_tier1(mi355, ref, name):
    # (the second picture reuses the context's device buffers)
    R.check_tier1(mi355.lib, ref, name, [R.picture(name, seed=4, pad=0), R.ramp(name, seed=5, pad=2)])


def test_rgbsrc_refused_on_the_device(mi355):
    """the real library refuses what the emulated one refuses, and nothing else of the table"""
    assert {n for n in R.NAMES if R.plan(mi355.lib, R.stored_entry(n)) is None} == R.REFUSED


def test_rgbsrc_line_entries_on_the_device(mi355):
    assert R.check_line_entries(mi355.lib) > 0


def test_fate_pixfmt_rgb24_both_stages_on_the_device(mi355):
    assert R.fate_md5(mi355) == GOLD["fate_pixfmt_rgb24_md5"]


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", ["s_420_same", "s_420_oddw", "s_rgb_w257_up", "s_rgb_vdown8"])
def test_rgbsrc_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = R.stored_entry(name)
    planes = R.ramp(name, seed=5, pad=3)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    if lines:
        assert lib.ref_sws_tier1_calls() > calls and lib.ref_sws_pictures() == pics, name
    else:
        assert lib.ref_sws_pictures() == pics + (0 if name in R.REFUSED else 1) and lib.ref_sws_tier1_calls() == calls, name
    assert not any(R.differing_rows(got, want, sizes)), name
