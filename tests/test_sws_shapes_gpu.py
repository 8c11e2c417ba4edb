"""GPU: every context of tests/sws_shapes.py that mi355_sws_create takes, through mi355_sws_scale_frames_dev on a batch of four frames with
their own source strides (pads 0, odd, 16, odd) and destination strides, the destination filled with 0x5A and guarded before, between and after
the frames.  Every row's first dstW * 3 bytes must equal the oracle and the reference's own sws_scale(); nothing right of them and no
guard byte may change; a picture gives the same output wherever it sits in the batch.  Then every entry through the reference's
sws_scale() bound to the library (oracle/_ref/libswsref_gpu.so): the same output as the plain reference, and the binding converts on the
device exactly the contexts mi355_sws_plan describes (nothing under /root/reference is read here)."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_shapes as T
import sws_support as S
from test_sws_tier1_reference import bind

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (T.REF_LIB, T.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return T.Ref(T.bind(T.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    b = bind(S.Reference.__new__(S.Reference), T.REF_GPU_LIB)
    return T.Ref(b.lib)


@pytest.mark.parametrize("name", T.NAMES)
def test_shape_batched_on_the_device(mi355, oracle, ref, name):
    plan = T.check_batch(mi355.lib, oracle, ref, name)
    assert (plan is None) == (name in T.REFUSED), (name, plan)


@pytest.mark.parametrize("name", list(T.SHAPES))
def test_shape_through_the_binding(mi355, ref, bound, name, monkeypatch):
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    ctx = T.context(ref, name)
    on_device = T.plan(mi355.lib, ctx) is not None
    planes = T.picture(name, seed=5, pad=3)
    want = ref.scale(name, planes)
    before = bound.lib.ref_sws_pictures()
    got = bound.scale(name, planes)
    assert bound.lib.ref_sws_pictures() == before + (1 if on_device else 0), name
    rb = 3 * ctx.desc.dstW
    assert (got[:, :rb] == want[:, :rb]).all(), name
    # right of the picture: the device writes nothing there, the reference its phantom pixel of an odd width
    assert (got[:, rb:] == (0x5A if on_device else want[:, rb:])).all(), name
