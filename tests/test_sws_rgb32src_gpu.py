"""GPU: packed 32-bit sources (rgba / bgra / argb / abgr) of the device swscale path (include/mi355_sws.h).

Every entry of tests/sws_rgb32src.py on the contexts committed in tests/golden/sws_rgb32src_contexts.npz: a guarded four-frame Tier-2 batch
(packed planes on a 16-byte multiple and on a 4-byte multiple that is none of 16, at line pads of 0, 1, 4 and 3 pixels) equals the reference's
own sws_scale() of the same buffers (oracle/_ref/libswsref.so), byte for byte, over the whole extent of every destination plane; the alpha rows
also on alpha planes of noise, 0, 255 and a checkerboard, and with alpha 0 against the colour bytes with 255; the odd width whose halving
converter reads pixel srcW, in its own padding and in the next frame's buffer; one Tier-1 call per destination kind; the line entries against
the reference's templates written out; both FATE pins with both stages on the device; the binding (oracle/_ref/libswsref_gpu.so) in both forms.
Nothing under the reference's sources is read here."""
import os

import pytest

import sws_planar as P
import sws_rgb32src as Q

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (Q.REF_LIB, Q.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return Q.Ref(P.bind(Q.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    # a library linked from an older binding has no describer of these sources (and its sws_scale() is then the plain reference's)
    if not P.exports(Q.REF_GPU_LIB, Q.DESCRIBER):
        pytest.skip(Q.REF_GPU_LIB + " was linked before the binding took 32-bit sources: __graft_entry__.build() relinks it where the reference exists")
    return Q.Ref(P.bind(Q.REF_GPU_LIB))


TAKEN = [n for n in Q.NAMES if n not in Q.REFUSED]
ALPHA = sorted(Q.ALPHA)
# one Tier-1 call per destination kind, the odd width, an alpha row
TIER1 = ["q_rgb_down2", "q_bgr_w257_up", "q_420_down2", "q_422_w127", "q_444_w129_up", "q_nv12_same", "q_nv21_down2", "q_420p10_down2", "q_j420_down2",
         "q_420_oddw", "a_w129_up"]


@pytest.mark.parametrize("name", TAKEN)
def test_rgb32src_batched_on_the_device(mi355, ref, name):
    assert Q.check_batch(mi355.lib, ref, name, e=Q.stored_entry(name)) is not None, name


@pytest.mark.parametrize("name", ALPHA)
def test_rgb32src_alpha_planes_on_the_device(mi355, ref, name):
    p = Q.check_batch(mi355.lib, ref, name, e=Q.stored_entry(name), pictures=Q.alpha_pictures(name))
    assert p is not None and p["alpha"] == 1


@pytest.mark.parametrize("name", ALPHA)
def test_rgb32src_alpha_0_is_colour_with_255_on_the_device(mi355, ref, name):
    p = Q.check_batch(mi355.lib, ref, name, e=Q.stored_entry(name), alpha=0)
    assert p is not None and p["alpha"] == 0


def test_rgb32src_odd_width_extra_pixel_in_the_next_frame(mi355, ref):
    Q.check_contiguous(mi355.lib, ref, "q_420_oddw")


@pytest.mark.parametrize("name", TIER1)
def test_rgb32src_tier1(mi355, ref, name):
    # (the second picture reuses the context's device buffers)
    Q.check_tier1(mi355.lib, ref, name, [Q.picture(name, "noise", seed=4, pad=0), Q.picture(name, "ramp", seed=5, pad=2)])


def test_rgb32src_refused_on_the_device(mi355):
    """the real library refuses what the emulated one refuses, and nothing else of the table"""
    assert {n for n in Q.NAMES if Q.plan(mi355.lib, Q.stored_entry(n)) is None} == Q.REFUSED


def test_rgb32src_line_entries_on_the_device(mi355):
    assert Q.check_line_entries(mi355.lib) > 0
    assert Q.check_alpha_line_entries(mi355.lib) == 4 * 9


@pytest.mark.parametrize("chain", sorted(Q.FATE_CHAINS))
def test_fate_pixfmt_both_stages_on_the_device(mi355, chain):
    assert Q.fate_md5(mi355, chain) == Q.fate_gold()["fate_pixfmt_%s_md5" % chain]


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", ["q_420_same", "q_420_oddw", "q_bgr_w257_up", "a_down2", "q_rgb_vdown8"])
def test_rgb32src_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = Q.stored_entry(name)
    planes = Q.picture(name, "ramp", seed=5, pad=3)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    if lines:
        assert lib.ref_sws_tier1_calls() > calls and lib.ref_sws_pictures() == pics, name
    else:
        assert lib.ref_sws_pictures() == pics + (0 if name in Q.REFUSED else 1) and lib.ref_sws_tier1_calls() == calls, name
    assert not any(Q.differing_rows(got, want, sizes)), name
