"""GPU: packed 4:2:2 sources (yuyv422 / uyvy422 / yvyu422) of the device swscale path (include/mi355_sws.h): the scaler's tile instances, the ident1
form and the unscaled splitter k_sws_yuy2_split.

Every entry of tests/sws_yuy2src.py on the contexts committed in tests/golden/sws_yuy2src_contexts.npz: a guarded four-frame Tier-2 batch (packed
planes on a 16-byte multiple, on 4-byte multiples and on an odd address with an odd stride, at line pads of 0, 1, 4 and 3 pixels) equals the
reference's own sws_scale() of the same buffers (oracle/_ref/libswsref.so), byte for byte, over the whole extent of every destination plane; the
odd widths whose last chroma sample reads the two bytes behind the line, in their own padding and in the next frame's buffer; one Tier-1 call per
destination kind and per split form; the line entries against the byte table written out; stage 2 of fate-pixfmt-yuyv422 against its pin; the binding
(oracle/_ref/libswsref_gpu.so) with whole pictures on the device and with the inner loops forwarded.
Nothing under the reference's sources is read here."""
import os

import pytest

import sws_planar as P
import sws_yuy2src as Y

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (Y.REF_LIB, Y.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return Y.Ref(P.bind(Y.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    # a library linked from an older binding has no describer of these sources (and its sws_scale() is then the plain reference's)
    if not P.exports(Y.REF_GPU_LIB, Y.DESCRIBER):
        pytest.skip(Y.REF_GPU_LIB + " was linked before the binding took packed 4:2:2 sources: __graft_entry__.build() relinks it where the reference exists")
    return Y.Ref(P.bind(Y.REF_GPU_LIB))


# one Tier-1 call per split form (yuyv422 / uyvy422 to yuv420p / yuv422p, and the picture without a chroma row) and per destination kind of the scaler:
# three planes at both chroma widths, SEMI, a range, a deep depth, the three packed forms through the tile, ident1 to a 24-bit and a 32-bit order
TIER1 = ["s_yuyv_420", "s_uyvy_420_odd", "s_yuyv_422_w130", "s_uyvy_422_oddw", "s_yuyv_420_h1",
         "g_yuyv_420_down2", "g_yuyv_444_w129_up", "g_uyvy_nv12_same", "g_uyvyj_420_down2", "g_uyvy_420p10_down2",
         "p_yuyv_rgb_down2", "p_uyvy_bgr_w257_up", "p_yvyu_rgba_w384_up", "p_yuyv_rgb_same", "p_uyvy_bgra_same_w126"]


@pytest.mark.parametrize("kinds", [("noise", "ramp", "ones"), ("checker", "zeros", "noise")])
@pytest.mark.parametrize("name", Y.TAKEN)
def test_yuy2src_batched_on_the_device(mi355, ref, name, kinds):
    p = Y.check_batch(mi355.lib, ref, name, e=Y.stored_entry(name), kinds=kinds)
    assert p is not None and (p["kernel"] == "yuy2_split") == (name in Y.SPECIAL), name


@pytest.mark.parametrize("name", Y.SPECIAL)
def test_yuy2src_batched_equals_the_wrappers_written_out_on_the_device(mi355, name):
    assert Y.check_batch(mi355.lib, None, name, e=Y.stored_entry(name)) is not None, name


@pytest.mark.parametrize("name", ["s_uyvy_420_odd", "s_uyvy_422_oddw", "g_uyvy_odd"])
def test_yuy2src_odd_width_extra_bytes_in_the_next_frame(mi355, ref, name):
    Y.check_contiguous(mi355.lib, ref, name)


@pytest.mark.parametrize("name", TIER1)
def test_yuy2src_tier1(mi355, ref, name):
    # (the second picture reuses the context's device buffers)
    Y.check_tier1(mi355.lib, ref, name, [Y.picture(name, "noise", seed=4, padb=0), Y.picture(name, "ramp", seed=5, padb=3)])


def test_yuy2src_refused_on_the_device(mi355):
    """the real library refuses what the emulated one refuses (the yuv422p twin's refusals), and nothing else of the table"""
    plans = {n: Y.plan(mi355.lib, Y.stored_entry(n)) for n in Y.NAMES}
    assert {n for n, p in plans.items() if p is None} == Y.REFUSED
    assert Y.refused_by_the_twin(mi355.lib) == Y.REFUSED
    assert not any(p["kernel"] == "ident1_x" for p in plans.values() if p)
    e = Y.stored_entry("s_yuyv_420")
    for edit in ({"layout": 18}, {"fmt": 3}, {"fmt": 0}, {"fmt": 16}, {"range_": 1}, {"dst_depth": 10}, {"dstH": 24}):
        assert not Y.create(mi355.lib, e.edited(**edit)), edit
    g = Y.stored_entry("g_yuyv_420_down2")
    for edit in ({"layout": 19}, {"fmt": 18}, {"depth": 10}, {"hsub": 0}, {"vsub": 1}, {"range_": 3}):
        assert not Y.create(mi355.lib, g.edited(**edit)), edit
    assert not Y.create(mi355.lib, g, alpha=1)


def test_yuy2src_line_entries_on_the_device(mi355):
    assert Y.check_line_entries(mi355.lib) == 6 * 4 * 3 * 2


def test_yuy2src_fate_stage2_on_the_device(mi355):
    """stage 2 of fate-pixfmt-yuyv422 (yuyv422 -> yuv444p) of the committed stage-1 picture against the pin; the full chain waits for the destination"""
    assert Y.fate_md5(mi355.lib) == Y.fate_gold()["yuyv422"]


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", Y.BINDING + Y.BINDING_UNBOUND)
def test_yuy2src_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = Y.picture(name, "ramp", seed=5, padb=6)
    sizes = Y.out_sizes(name)
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    # whole pictures of the scaler's contexts run on the device (a refused one and a wrapper's stay the reference's); under MI355_SWS_LINES=1 the
    # inner loops of the scaler's contexts are forwarded instead
    assert lib.ref_sws_pictures() == pics + (1 if not lines and name in Y.BINDING_TAKEN else 0), name
    assert (lib.ref_sws_tier1_calls() > calls) == (lines and name in Y.BINDING), name
    assert not any(Y.differing_rows(got, want, sizes)), name
