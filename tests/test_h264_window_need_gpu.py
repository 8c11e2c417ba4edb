"""GPU: the luma window request that leaves out what a vector's position does not read (tests/h264_window_tables.py), on the device against the oracle."""
import pytest

import h264_window_tables as W


@pytest.mark.parametrize("order,run", W.PHASE_CASES, ids=lambda v: str(v).replace(" ", "-"))
@pytest.mark.gpu
def test_phase_table_whatever_came_before(mi355, oracle, order, run):
    """Every (position, o, window row phase) of a plain macroblock with its windows inside the picture, bit-exact on every sample.
    The purpose of the cases: NO PIECE LEFT OUT OF A REQUEST REACHES A STORED SAMPLE.  The same 2048 entries are decoded at run lengths 1, 4 and 15 (what MI355_RECON_RUN
    names) and with the macroblocks of every row in two other orders; the entry that last wrote a macroblock's window set — a full 3 x 21 window, a trimmed one, none at
    all at the head of a run — differs from case to case, and every case must give the oracle's pictures."""
    W.run_phase(mi355, oracle, order, run)


@pytest.mark.parametrize("run", (1, 3))
@pytest.mark.parametrize("mb_w", (2, 3))
@pytest.mark.gpu
def test_windows_over_the_borders(mi355, oracle, mb_w, run):
    """left, right (fq_windows_patch mends only what was requested), top and bottom (rows clamped) at every o, positions 0, 2, 8 and 15; 2 wide: two window tile columns are one tile"""
    W.run_edges(mi355, oracle, mb_w, run)


@pytest.mark.parametrize("run", (1, 4))
@pytest.mark.gpu
def test_two_partitions_with_different_needs(mi355, oracle, run):
    """fq_two: each partition's request trimmed by its own position, inside the picture and over its side borders"""
    W.run_two(mi355, oracle, run)
