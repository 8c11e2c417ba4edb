"""GPU: the table of deblock_resident_cases (test_deblock_resident_emu.py asserts what it reaches) through k_deblock_tiled as 1, 2, 4,
tickets - 1, tickets and tickets + 5 resident waves and with the rule's count, every sample against the oracle; the pipelines object
with two resident waves per launch."""
import pytest

import deblock_resident_cases as R


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.BATCHES))
def test_resident_batches_gpu(mi355, name):
    R.run_batch(mi355, name)


@pytest.mark.gpu
def test_pipelines_object_with_resident_waves_gpu(mi355, oracle):
    """(the fixtures: the library loads and the oracle is built before the child process looks for them)"""
    R.run_pinned("mi355")
