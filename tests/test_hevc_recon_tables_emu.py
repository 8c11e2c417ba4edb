"""CPU: the HEVC reconstruction tables (tests/hevc_recon_tables.py) on the emulated kernels vs the oracle, bit depths 8 and 10.  Every transform row and
every coding-tree-block geometry; of the motion / prediction table every row with noise and the saturating classes by hevc_recon_tables.emu_keeps; which
classes also go through the block kernels: hevc_recon_tables.emu_entries."""
import pytest

import hevc_recon_tables as T

DEPTHS = (8, 10)


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("cls", T.MC_CLASSES)
def test_emulated_motion_table(emu, oracle, cls, bd):
    assert T.check_mc_table(emu, oracle, bd, cls, keep=T.emu_keeps) > 0


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("cls", ("noise", "tap-max"))
def test_emulated_prediction_table(emu, oracle, cls, bd):
    assert T.check_pred_table(emu, oracle, bd, cls) > 0


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("cls", T.MC_CLASSES)
def test_emulated_fused_motion_prediction_table(emu, oracle, cls, bd):
    """the fused jobs through mi355_hevc_mcpred_batch_dev, _recon_level_dev, _recon_levels_dev and (a block per luma + chroma job) _recon_ctbs_dev"""
    assert T.check_scene(emu, oracle, T.mc_scene(bd, cls, keep=T.emu_keeps), "fused table %s" % cls, T.emu_entries("mc", cls, bd)) > 0


@pytest.mark.parametrize("bd", DEPTHS)
@pytest.mark.parametrize("cls", T.TU_CLASSES)
def test_emulated_transform_table(emu, oracle, cls, bd):
    assert T.check_scene(emu, oracle, T.tu_scene(bd, cls), "transform table %s" % cls, T.emu_entries("tu", cls, bd)) > 0


@pytest.mark.parametrize("bd", DEPTHS)
def test_emulated_ctb_geometries(emu, oracle, bd):
    s = T.geometry_scene(bd)
    assert T.check_scene(emu, oracle, s, "geometry table") > 0
    assert T.check_promise(emu, oracle, s, "geometry table") > 0
