"""GPU: every entry of tests/h264_pair_tables.py through the Tier-2 bridge (oracle/_ref/h264_bridge_gpu), as tests/test_h264_pair_tables_emu.py: direct with one decoder
and lazy with three (batches of several pictures, four pictures per wave in the pair filter), loop filter on; direct with the loop filter off.  One or two short child
processes per test, each under a time limit of ten times the entry's time on the emulator (at least 30 s).  Run this file with -x: nothing more on a card after a fault."""
import os

import pytest

import h264_pair_tables as PT

pytestmark = pytest.mark.gpu


def _need():
    if not os.path.exists(PT.exe("h264_bridge_gpu")):
        pytest.fail("oracle/_ref/h264_bridge_gpu missing: run __graft_entry__.build() where the reference tree exists")


@pytest.mark.parametrize("lazy", (False, True))
@pytest.mark.parametrize("name", PT.NAMES)
def test_pair_table_entry_gpu(tmp_path, mi355, name, lazy):
    _need()
    PT.run_entry("h264_bridge_gpu", name, tmp_path, lazy=lazy)


@pytest.mark.parametrize("name", PT.NAMES)
def test_pair_table_entry_without_loop_filter_gpu(tmp_path, mi355, name):
    _need()
    PT.run_entry("h264_bridge_gpu", name, tmp_path, nofilter=True)
