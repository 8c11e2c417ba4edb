"""GPU: the table of deblock_step_cases (test_deblock_tiled_steps_emu.py asserts what it reaches) through k_deblock_tiled and
k_deblock_tiled2, every sample against the oracle."""
import pytest

import deblock_step_cases as S


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", S.SHAPES, ids=["%dx%d" % s for s in S.SHAPES])
def test_tiled_forms_step_table_gpu(mi355, w, h):
    S.run_shape(mi355, w, h)
