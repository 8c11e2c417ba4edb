"""GPU: bgr24 and 32-bit rgba / bgra / argb / abgr destinations of the device swscale path (include/mi355_sws.h).

Every entry of tests/sws_packeddst.py on the contexts committed in tests/golden/sws_packeddst_contexts.npz: a guarded six-frame Tier-2 batch
(noise, the two-pixel checkerboard, the ramp, the noise at other strides, all-0 and all-maximum planes; destination rows on a 16-byte multiple, on
a 4-byte multiple that is no multiple of 16 and — 24 bits — on an odd address, at line pads of 0, 5, 16 and 3 pixels) equals the reference's own
sws_scale() of the same buffers (oracle/_ref/libswsref.so), byte for byte, and no byte outside the written pixels changes; a handful of Tier-1
calls over both pixel sizes and the special converter; the refused set; the line entries; the binding (oracle/_ref/libswsref_gpu.so) in both
forms.  Nothing under the reference's sources is read here."""
import os

import pytest

import sws_packeddst as K
import sws_planar as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (K.REF_LIB, K.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return K.Ref(P.bind(K.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    # a library linked from an older binding declines every one of these contexts (and its sws_scale() is then the plain reference's): ask the
    # library itself, as tests/test_sws_deepdst_gpu.py does — the binding can only be relinked where the reference's sources are
    if not P.exports(K.REF_GPU_LIB, K.DESCRIBER):
        pytest.skip(K.REF_GPU_LIB + " was linked before the binding took these destinations: __graft_entry__.build() relinks it where the reference exists")
    return K.Ref(P.bind(K.REF_GPU_LIB))


TAKEN = [n for n in K.NAMES if n not in K.REFUSED]
# Tier 1: both pixel sizes through the tile kernel (a full tile and a partial one), k_sws_ident1 and the special converter
TIER1 = ["d2_420_bgr24", "up_420_bgra_w129", "h4_420_rgba_w130", "up_bgr_bgr24_w129", "ix_nv21_argb_w128", "k_420_rgba", "k_422_bgra_w70"]


@pytest.mark.parametrize("name", TAKEN)
def test_packeddst_batched_on_the_device(mi355, ref, name):
    p = K.check_batch(mi355.lib, ref, name, e=K.stored_entry(name))
    assert p is not None and p["format"] == K.DSTS[K.cfg(name)[5]] and p["dst_depth"] == 8 and p["range"] == 0, name


@pytest.mark.parametrize("name", TIER1)
def test_packeddst_tier1(mi355, ref, name):
    # (the second picture reuses the context's device buffers)
    K.check_tier1(mi355.lib, ref, name, [K.picture(name, "noise", seed=4, pad=0), K.picture(name, "checker", seed=5, pad=2)])


def test_packeddst_refused_on_the_device(mi355):
    """the real library refuses what the emulated one refuses, and nothing else of the table"""
    assert {n for n in K.NAMES if K.plan(mi355.lib, K.stored_entry(n)) is None} == K.REFUSED


def test_packeddst_line_entries_on_the_device(mi355):
    assert K.check_line_entries(mi355.lib, K.stored_entry("d2_420_rgba").ctx.desc.luts) > 0


@pytest.mark.parametrize("name", ["k_420_bgr24", "k_420_argb"])
def test_packeddst_slice_entry_on_the_device(mi355, ref, name):
    K.check_slice_entry(mi355.lib, ref, name)


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", K.BINDING)
def test_packeddst_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = K.stored_entry(name)
    planes = K.picture(name, "ramp", seed=5, pad=3)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    if lines:
        # (the special converter has no inner loops to forward: the reference's function runs)
        assert (lib.ref_sws_tier1_calls() > calls or name in K.SPECIAL) and lib.ref_sws_pictures() == pics, name
    else:
        assert lib.ref_sws_pictures() == pics + (0 if name in K.REFUSED else 1) and lib.ref_sws_tier1_calls() == calls, name
    assert not any(K.differing_rows(got, want, sizes)), name
