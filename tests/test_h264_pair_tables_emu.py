"""CPU: every entry of tests/h264_pair_tables.py through the Tier-2 bridge on the SIMT emulator (oracle/_ref/h264_bridge_emu): the bridge's pictures = the same
binary's with everything left to the reference's C functions, sample by sample; the plain side pinned by the recorded md5.  Direct mode with the loop filter on for
every entry; the filter-off pass (reconstruction alone) for every entry too — the whole file takes seconds here (tests/golden/h264_pair_tables_md5.json: emu_seconds
per entry, 0.03 .. 0.6 s when recorded; wall-clock figures that move with every regeneration, all far below the 30 s floor of h264_pair_tables.limit()) — and the lazy / three-thread mode for the named subset h264_pair_tables.EMU_LAZY."""
import os
import subprocess

import pytest

import h264_pair_tables as PT

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/libavcodec"), reason="needs the reference decoder objects (/root/reference)")


@pytest.fixture(scope="module")
def bridge(emu):                # conftest's emu: builds tests/_emu/libmi355dsp_emu.so from the kernels as they are now; the bridge binary links against it
    subprocess.run(["make", "-s", "-C", os.path.join(PT.ROOT, "oracle"), "_ref/h264_bridge_emu"], check=True)
    return "h264_bridge_emu"


@pytest.mark.parametrize("name", PT.NAMES)
def test_pair_table_entry_emulated(tmp_path, bridge, name):
    PT.run_entry(bridge, name, tmp_path)


@pytest.mark.parametrize("name", PT.NAMES)
def test_pair_table_entry_without_loop_filter_emulated(tmp_path, bridge, name):
    PT.run_entry(bridge, name, tmp_path, nofilter=True)


@pytest.mark.parametrize("name", PT.EMU_LAZY)
def test_pair_table_entry_lazy_three_decoders_emulated(tmp_path, bridge, name):
    PT.run_entry(bridge, name, tmp_path, lazy=True)
