"""GPU: range conversion of the device swscale path (include/mi355_sws.h).

Every entry of tests/sws_range.py on the contexts committed in tests/golden/sws_range_contexts.npz: a guarded six-frame Tier-2 batch (noise,
the checkerboard, the ramp, the noise at another stride, all-0 and all-maximum planes; planes on a 16-byte multiple, on a 4-byte multiple and
on an odd address, at line pads 0, 3, 16 and 7) equals the reference's own sws_scale() of the same buffers (oracle/_ref/libswsref.so), byte
for byte, over the whole rounded-up extent of every destination plane; one Tier-1 call per direction and destination kind; the two line
entries against the four formulas written out, over all 65536 int16 values; the FATE rows; the binding (oracle/_ref/libswsref_gpu.so) in both
forms.  Nothing under the reference's sources is read here."""
import os

import pytest

import sws_planar as P
import sws_range as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (G.REF_LIB, G.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return G.Ref(P.bind(G.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    # a library linked from an older binding declines every ranged context (and its sws_scale() is then the plain reference's): ask the
    # library itself, as tests/test_sws_rgbsrc_gpu.py does
    if not P.exports(G.REF_GPU_LIB, G.DESCRIBER):
        pytest.skip(G.REF_GPU_LIB + " was linked before the binding took range conversion: __graft_entry__.build() relinks it where the reference exists")
    return G.Ref(P.bind(G.REF_GPU_LIB))


TAKEN = [n for n in G.NAMES if n not in G.REFUSED]
# one Tier-1 call per direction and destination kind, a deeper and a packed source among them
TIER1 = ["f_420_same", "t_420_same", "f_422_nv21_down2", "t_420_nv12_down2", "t_d10_422_w129_up", "f_d10_444_w127", "f_nv12_nv12_down2", "t_d10_nv21_w129_up",
         "t_bgr_444_w129_up", "f_rgb_422_down2"]


@pytest.mark.parametrize("name", TAKEN)
def test_range_batched_on_the_device(mi355, ref, name):
    p = G.check_batch(mi355.lib, ref, name, e=G.stored_entry(name))
    assert p is not None and p["range"] == G.direction(name), name


@pytest.mark.parametrize("name", TIER1)
def test_range_tier1(mi355, ref, name):
    # (the second picture reuses the context's device buffers)
    G.check_tier1(mi355.lib, ref, name, [G.picture(name, "noise", seed=4, pad=0), G.picture(name, "checker", seed=5, pad=2)])


def test_range_refused_on_the_device(mi355):
    """the real library refuses what the emulated one refuses, and nothing else of the table"""
    assert {n for n in G.NAMES if G.plan(mi355.lib, G.stored_entry(n)) is None} == G.REFUSED


def test_range_line_entries_on_the_device(mi355):
    assert G.check_line_entries(mi355.lib) > 0


@pytest.mark.parametrize("name", sorted(G.FATE))
def test_fate_pixfmts_copy_yuvj_rows_on_the_device(mi355, name):
    assert G.fate_md5(mi355.lib, name) == G.fate_gold()[name]


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", ["f_420_same", "t_rgb_420_same", "t_d10_422_w129_up", "f_420_vdown16"])
def test_range_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = G.stored_entry(name)
    planes = G.picture(name, "ramp", seed=5, pad=3)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    if lines:
        assert lib.ref_sws_tier1_calls() > calls and lib.ref_sws_pictures() == pics, name
    else:
        assert lib.ref_sws_pictures() == pics + (0 if name in G.REFUSED else 1) and lib.ref_sws_tier1_calls() == calls, name
    assert not any(G.differing_rows(got, want, sizes)), name
