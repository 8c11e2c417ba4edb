"""GPU: packed 4:2:2 destinations (yuyv422 / uyvy422 / yvyu422) of the device swscale path (include/mi355_sws.h): the DST_YUY2 instances of the tile
kernel and of k_sws_ident1 / k_sws_ident1_yuy2, and the unscaled packer k_sws_yuy2_pack.

Every entry of tests/sws_yuy2dst.py on the contexts committed in tests/golden/sws_yuy2dst_contexts.npz: a guarded four-frame Tier-2 batch (destination
rows on 16-byte multiples, on 4-byte multiples and on an odd address with an odd stride) equals the reference's own sws_scale() of the same buffers
(oracle/_ref/libswsref.so), byte for byte, over the whole row extent; the packers against the wrappers written out; one Tier-1 call per form; the line
entries against the reference's own loops; the plan and the refusals of the rgb24 twin; both stages of fate-pixfmt-yuyv422 on the device against the
pin; the binding (oracle/_ref/libswsref_gpu.so) with whole pictures on the device and with the inner loops forwarded.
Nothing under the reference's sources is read here."""
import ctypes as C
import os

import pytest

import sws_planar as P
import sws_yuy2dst as Z
import sws_yuy2src as Y

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (Z.REF_LIB, Z.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return Z.Ref(P.bind(Z.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    # a library linked from an older binding has no describer of these destinations (and its sws_scale() is then the plain reference's): as in the
    # source modules, such a copy of oracle/_ref says nothing about this tree's binding, which tests/test_sws_yuy2dst_emu.py runs where it can be linked
    if not P.exports(Z.REF_GPU_LIB, Z.DESCRIBER):
        pytest.skip(Z.REF_GPU_LIB + " was linked before the binding took packed 4:2:2 destinations: __graft_entry__.build() relinks it where the reference exists")
    return Z.Ref(P.bind(Z.REF_GPU_LIB))


# one Tier-1 call per packer form and per form of the scaler: X narrow, odd, _2 with a full tile, the wide store, one row, _1, k_sws_ident1 from planes,
# from pairs and from packed bytes, a deeper source, packed sources scaled and at equal size, both ranges with an odd width
TIER1 = ["s_422_yuyv", "s_422_uyvy_w129", "s_422_uyvy_w131", "s_420_yuyv_w130", "s_420_uyvy_w131",
         "g_420_yuyv_down2", "g_420_yuyv_odd", "g_420_uyvy_w129_up_bilinear", "g_420_yuyv_w384_up", "g_420_uyvy_h1", "g_420_yuyv_honly",
         "g_420_yuyv_same", "g_nv21_uyvy_same_w126", "g_uyvy_yuyv_same", "g_420p10_yvyu_down2", "g_bgra_yvyu_down2", "g_rgb_uyvy_same",
         "r_j420_yuyv_odd", "r_420_yvyuj_odd_bilinear"]


@pytest.mark.parametrize("name", Z.TAKEN)
def test_yuy2dst_batched_on_the_device(mi355, ref, name):
    p = Z.check_batch(mi355.lib, ref, name, e=Z.stored_entry(name))
    assert p is not None and (p["kernel"] == "yuy2_pack") == (name in Z.SPECIAL), name


@pytest.mark.parametrize("name", Z.SPECIAL)
def test_yuy2dst_batched_equals_the_packers_written_out_on_the_device(mi355, name):
    e = Z.stored_entry(name)
    h = Z.create(mi355.lib, e)
    assert h
    try:
        pics = Z.batch_pictures(name)
        batch = Z.Batch(mi355.lib, e, pics, len(pics))
        try:
            out = batch.run(h)
            assert batch.untouched_behind(out, e.written()), name
            for f in range(len(pics)):
                assert (batch.frame(out, f)[0] == Z.model_pack(name, pics[f])[0]).all(), (name, f)
        finally:
            batch.close()
    finally:
        mi355.lib.mi355_sws_destroy(C.c_void_p(h))


@pytest.mark.parametrize("name", TIER1)
def test_yuy2dst_tier1(mi355, ref, name):
    # (the second picture reuses the context's device buffers)
    Z.check_tier1(mi355.lib, ref, name, [Z.picture(name, "noise", seed=4, pad=0), Z.picture(name, "ramp", seed=5, pad=3)], skew=len(name) % 2)


def test_yuy2dst_plans_and_refusals_on_the_device(mi355):
    """the real library refuses what the emulated one refuses (the rgb24 twin's refusals), and a taken row has its twin's plan"""
    lib = mi355.lib
    plans = {n: Z.plan(lib, Z.stored_entry(n)) for n in Z.NAMES}
    assert {n for n, p in plans.items() if p is None} == Z.REFUSED
    assert Z.refused_by_the_twin(lib) == Z.REFUSED
    for n in Z.SCALED:
        e = Z.stored_entry(n)
        t = Z.twin_plan(lib, e)
        if n in Z.REFUSED or t is None:
            continue
        for k in Z.PLAN_KEYS:
            if k == "kernel" and e.range and t[k].startswith("ident1"):
                continue
            assert plans[n][k] == t[k], (n, k)
    g, s = Z.stored_entry("g_420_yuyv_down2"), Z.stored_entry("s_422_yuyv")
    for edit in ({"fmt": 47}, {"fmt": 51}, {"dst_depth": 9}, {"dst_depth": 10}, {"range_": 3}, {"layout": 19}):
        assert not Z.create(lib, g.edited(**edit)), edit
    assert not Z.create(lib, g, alpha=1)
    for edit in ({"fmt": 50}, {"depth": 10}, {"layout": 1}, {"range_": 1}, {"dstH": 24}):
        assert not Z.create(lib, s.edited(**edit)), edit
    assert not Z.create(lib, s.edited(hsub=0, chrSrcW=s.ctx.ints["srcW"]))


def test_yuy2dst_line_entries_on_the_device(mi355, ref):
    assert Z.check_line_entries(mi355.lib, ref) > 400
    Z.check_line_entries_refuse(mi355.lib)


def test_yuy2dst_fate_chain_on_the_device(mi355):
    """stage 1 (yuv420p -> yuyv422) equals the reference's committed stage-1 picture; stages 1 + 2 on the device give the pin of fate-pixfmt-yuyv422"""
    assert (Z.fate_stage1(mi355.lib) == Y.fate_mid()[0]).all()
    assert Z.fate_chain_md5(mi355.lib) == Y.fate_gold()["yuyv422"]


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", Z.BINDING + Z.BINDING_UNBOUND)
def test_yuy2dst_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
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
    # whole pictures of the scaler's contexts run on the device (a refused one and a packer's stay the reference's); under MI355_SWS_LINES=1 the
    # inner loops of the scaler's contexts are forwarded instead
    assert lib.ref_sws_pictures() == pics + (1 if not lines and name in Z.BINDING_TAKEN else 0), name
    assert (lib.ref_sws_tier1_calls() > calls) == (lines and name in Z.BINDING), name
    assert not any(Z.differing_rows(got, want, sizes)), name
