"""GPU: every instance of the picture kernels of the device swscale path that no feature table launches (tests/sws_instances.py: one row an instance).

Every row on the contexts committed in tests/golden/sws_instances_contexts.npz: the product library's plan gives the key the row names, the launch
returns 0, and a guarded four-frame Tier-2 batch (source planes and strides on 16-byte multiples, on 4-byte multiples, in the source's least aligned
position, and frame 0's picture again at other strides; noise, a ramp and the all-maximum / all-minimum rows, in two orders, so that a picture that
varies along x meets every load form) equals the reference's own sws_scale() of the same buffers (oracle/_ref/libswsref.so), byte for byte, over the
whole extent of every destination plane; one Tier-1 call per (source class, destination kind) of the tile kernels and one per small-kernel row; the
plans stated in the table.  Nothing under the reference's sources is read here."""
import os

import pytest

import sws_instances as I
import sws_planar as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    if not os.path.exists(I.REF_LIB):
        pytest.fail(I.REF_LIB + " missing: __graft_entry__.build() makes it where the reference exists")
    return I.Ref(P.bind(I.REF_LIB))


@pytest.mark.parametrize("kinds", I.ORDERS)
@pytest.mark.parametrize("name", I.NAMES)
def test_instance_on_the_device(mi355, ref, name, kinds):
    p = I.check_batch(mi355.lib, ref, name, kinds=kinds)
    assert I.key_of(p) == I.key_for(name), (name, I.key_text(I.key_of(p)))


@pytest.mark.parametrize("name", I.TIER1)
def test_instance_tier1(mi355, ref, name):
    I.check_tier1(mi355.lib, ref, name)


def test_plans_on_the_device(mi355):
    """the product library plans every row as the table states (kernel letter, th, narrow, hstaged): what the emulated library gave when the row was
    chosen"""
    for name in I.NAMES:
        p = I.plan(mi355.lib, I.stored_entry(name))
        assert p is not None, (name, "refused")
        assert I.plan_summary(p) == I.expected_plan(name) and I.key_of(p) == I.key_for(name), (name, p)
