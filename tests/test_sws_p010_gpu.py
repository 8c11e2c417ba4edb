"""GPU: P010 sources (p010le, MI355_SWS_SRC_P010) of the device swscale path (include/mi355_sws.h): the tile instances of sws_p010.hip.

Every taken entry of tests/sws_p010.py on the contexts committed in tests/golden/sws_p010_contexts.npz: a guarded four-frame Tier-2 batch (both source
planes on 16-byte multiples, on 4-byte multiples, the pair plane at an address 2 mod 4 with a stride 2 mod 4, at line pads of 0, 1, 4 and 3 samples)
equals the reference's own sws_scale() of the same buffers (oracle/_ref/libswsref.so), byte for byte, over the whole extent of every destination
plane; one Tier-1 call per destination kind; the refusal set on the real library; the line entries against the byte table written out; the binding
(oracle/_ref/libswsref_gpu.so) with whole pictures on the device and with the inner loops forwarded.

There is no FATE row: the reference has no fate-pixfmt-p010le pin, because it cannot write P010.  Nothing under the reference's sources is read here."""
import os

import pytest

import sws_planar as P
import sws_p010 as Z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (Z.REF_LIB, Z.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return Z.Ref(P.bind(Z.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    # a library linked from an older binding has no describer of this source (and its sws_scale() is then the plain reference's)
    if not P.exports(Z.REF_GPU_LIB, Z.DESCRIBER):
        pytest.skip(Z.REF_GPU_LIB + " was linked before the binding took P010 sources: __graft_entry__.build() relinks it where the reference exists")
    return Z.Ref(P.bind(Z.REF_GPU_LIB))


# one Tier-1 call per destination kind: three planes at both chroma widths, SEMI, both ranges, both deep depths, rgb24, bgr24, a 32-bit order at equal
# size and scaled, a packed 4:2:2 order with and without a range
TIER1 = ["g_420_down2", "g_444_oddw_same", "g_nv12_same", "g_j420_same", "g_full_420_down2", "g_420p10_same", "g_444p9_w129_up",
         "p_rgb_down2", "p_bgr_w257_up", "p_bgra_same_w126", "p_rgba_w384_up", "y_uyvy_down2", "y_yvyuj_down2"]


@pytest.mark.parametrize("kinds", [("noise", "ramp", "ones"), ("checker", "zeros", "noise")])
@pytest.mark.parametrize("name", Z.TAKEN)
def test_p010_batched_on_the_device(mi355, ref, name, kinds):
    p = Z.check_batch(mi355.lib, ref, name, e=Z.stored_entry(name), kinds=kinds)
    assert p is not None and p["layout"] == Z.LAYOUT and p["kernel"].startswith(("generic_", "planar_")), name


@pytest.mark.parametrize("name", TIER1)
def test_p010_tier1(mi355, ref, name):
    # (the second picture reuses the context's device buffers)
    Z.check_tier1(mi355.lib, ref, name, [Z.picture(name, "noise", seed=4, pad=0), Z.picture(name, "ramp", seed=5, pad=3)])


def test_p010_refused_on_the_device(mi355):
    """the real library refuses what the emulated one refuses (the planar 10-bit twin's refusals), nothing else of the table, and what the header lists"""
    plans = {n: Z.plan(mi355.lib, Z.stored_entry(n)) for n in Z.NAMES}
    assert {n for n, p in plans.items() if p is None} == Z.REFUSED
    assert Z.refused_by_the_twin(mi355.lib) == Z.REFUSED
    for n in Z.TAKEN:
        t = Z.plan(mi355.lib, Z.twin_entry(Z.stored_entry(n)))
        assert all(plans[n][k] == t[k] for k in Z.TWIN_KEYS), (n, plans[n], t)
    for what, e, alpha in Z.refusal_cases(Z.stored_entry("g_420_down2"), Z.stored_entry("p_rgb_down2")):
        assert not Z.create(mi355.lib, e, alpha), what
    Z.check_odd_stride_refused(mi355.lib)


def test_p010_line_entries_on_the_device(mi355):
    assert Z.check_line_entries(mi355.lib) == 4 * 2 * 2


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", Z.BINDING)
def test_p010_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = Z.picture(name, "ramp", seed=5, pad=3)
    sizes = Z.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    # whole pictures run on the device (a refused row stays the reference's); under MI355_SWS_LINES=1 the inner loops are forwarded instead
    assert lib.ref_sws_pictures() == pics + (1 if not lines and name in Z.BINDING_TAKEN else 0), name
    assert (lib.ref_sws_tier1_calls() > calls) == lines, name
    assert not any(Z.differing_rows(got, want, sizes)), name
