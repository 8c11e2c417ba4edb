"""GPU: the HEVC reconstruction tables (tests/hevc_recon_tables.py) vs the oracle, bit-exact, 8 / 9 / 10 bit: every row, every class, every entry point; the
jobs of one class in one launch per entry point."""
import pytest

import hevc_recon_tables as T

pytestmark = pytest.mark.gpu
DEPTHS = (8, 9, 10)


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("cls", T.MC_CLASSES)
def test_gpu_motion_table(mi355, oracle, cls, bd):
    assert T.check_mc_table(mi355, oracle, bd, cls) == len(T.mc_rows())


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("cls", T.MC_CLASSES)
def test_gpu_prediction_table(mi355, oracle, cls, bd):
    assert T.check_pred_table(mi355, oracle, bd, cls) > 0


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("pad", (0, 2))
@pytest.mark.parametrize("cls", T.MC_CLASSES)
def test_gpu_fused_motion_prediction_table(mi355, oracle, cls, pad, bd):
    """pad: samples of padding in the reference rows — 0: the block kernels' matrix path takes the one-reference blocks of 16-sample sides, 2: their general path"""
    assert T.check_scene(mi355, oracle, T.mc_scene(bd, cls, pad=pad), "fused table %s pad %d" % (cls, pad), T.ENTRIES if pad == 0 else ("ctbs",)) > 0


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("cls", T.TU_CLASSES)
def test_gpu_transform_table(mi355, oracle, cls, bd):
    assert T.check_scene(mi355, oracle, T.tu_scene(bd, cls), "transform table %s" % cls) > 0


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("cls,tu_cls", (("tap-max", "clip-high"), ("tap-min", "clip-low"), ("noise", "uniform")))
def test_gpu_ctb_geometries(mi355, oracle, cls, tu_cls, bd):
    s = T.geometry_scene(bd, cls, tu_cls)
    assert T.check_scene(mi355, oracle, s, "geometry table") > 0
    assert T.check_promise(mi355, oracle, s, "geometry table") > 0
