"""CPU: the table of tests/sws_shapes.py through the emulated product library.  mi355_sws_plan on every entry must reach every kernel
the device path has, several tile heights, both horizontal passes, both tile forms and a refused context (the table must not shrink below
that); the entries of at most about 100 K output pixels must equal the oracle byte for byte, and the reference's own sws_scale(), through
the whole-picture entry point and on a guarded batch."""
import ctypes as C
import os
import subprocess

import pytest

import sws_shapes as T

pytestmark = pytest.mark.skipif(not os.path.exists(T.REF_LIB) and not T.S.HAVE_REFERENCE,
                                reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")


@pytest.fixture(scope="module")
def ref():
    if T.S.HAVE_REFERENCE:
        subprocess.run(["make", "-s", "-C", os.path.join(T.ROOT, "oracle"), "_ref/libswsref.so"], check=True)
    return T.Ref(T.bind(T.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu, ref):
    return {name: T.plan(emu.lib, T.context(ref, name)) for name in T.NAMES}


def test_table_reaches_every_branch(plans):
    got = [p for p in plans.values() if p]
    assert {p["kernel"] for p in got} == set(T.KERNELS), plans
    generic = [p for p in got if p["kernel"].startswith("generic")]
    assert len({p["th"] for p in generic}) >= 3, plans
    assert {p["hstage"] for p in got if p["kernel"] != "c24"} == {0, 1}, plans
    assert {p["narrow"] for p in generic} == {0, 1}, plans
    assert any(p is None for p in plans.values()), "no context that mi355_sws_create refuses"
    # the entries named for a branch take it
    for name, p in plans.items():
        if name.startswith("c24_"):
            assert p["kernel"] == "c24", (name, p)
        elif name.startswith("id1_"):
            assert p["kernel"] == "ident1_1", (name, p)
        elif name.startswith("idx_"):
            assert p["kernel"] == "ident1_x", (name, p)
        elif name.startswith(("idodd_", "g_w")):
            assert p["kernel"].startswith("generic"), (name, p)
    assert plans["synth_hstage0"]["hstage"] == 0 and plans["g_honly"]["hstage"] == 1
    assert {n for n, p in plans.items() if p is None} == T.REFUSED


def test_plan_query_refuses_bad_arguments(emu):
    emu.lib.mi355_sws_plan.argtypes = [C.c_void_p, C.c_void_p]
    assert emu.lib.mi355_sws_plan(None, C.byref(T.PlanInfo())) == -1


SMALL = [n for n in T.NAMES if n not in T.BIG and T.out_pixels(n) <= T.SMALL_PIXELS]


@pytest.mark.parametrize("name", SMALL)
def test_emulated_shape_matches_oracle_and_reference(emu, oracle, ref, plans, name):
    ctx = T.context(ref, name)
    dw = ctx.desc.dstW
    planes = T.picture(name, seed=11, pad=5)
    want = T.oracle_scale(oracle, ctx, planes, dst_pad=8)
    if name in T.SHAPES:
        # the reference writes pixels in pairs: at an odd width one more than the picture has (yuv2rgb_write, output.c), and so does the oracle
        assert (want[:, :3 * dw] == ref.scale(name, planes, dst_pad=8)[:, :3 * dw]).all()
    if plans[name] is None:
        return                                   # mi355_sws_create refuses it: the reference's own code converts it (the glue)
    got = T.S.product_backend(emu).scale(ctx, planes, dst_pad=8)
    assert (got[:, :3 * dw] == want[:, :3 * dw]).all()
    assert (got[:, 3 * dw:] == 0x5A).all()


@pytest.mark.parametrize("name", SMALL)
def test_emulated_shape_batched(emu, oracle, ref, plans, name):
    """the Tier-2 entry point on four guarded frames with their own strides (what tests/test_sws_shapes_gpu.py runs on the device)"""
    assert T.check_batch(emu.lib, oracle, ref, name) == plans[name]
