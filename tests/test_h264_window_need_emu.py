"""CPU: the luma window request that leaves out what a vector's position does not read (tests/h264_window_tables.py), under the SIMT emulator against the oracle —
the emulator's LDS-DMA honours the same lane set as the device's, so a piece that was not requested holds what an earlier macroblock left there — and the rule's census."""
import numpy as np
import pytest

import h264_frames as HF
import h264_window_tables as W


@pytest.mark.parametrize("order,run", W.PHASE_CASES, ids=lambda v: str(v).replace(" ", "-"))
def test_phase_table_whatever_came_before_emulated(emu, oracle, order, run):
    """Every (position, o, window row phase) of a plain macroblock with its windows inside the picture, bit-exact on every sample.
    The purpose of the cases: NO PIECE LEFT OUT OF A REQUEST REACHES A STORED SAMPLE.  The same 2048 entries are decoded at run lengths 1, 4 and 15 (what MI355_RECON_RUN
    names) and with the macroblocks of every row in two other orders; the entry that last wrote a macroblock's window set — a full 3 x 21 window, a trimmed one, none at
    all at the head of a run — differs from case to case, and every case must give the oracle's pictures."""
    W.run_phase(emu, oracle, order, run)


@pytest.mark.parametrize("run", (1, 3))
@pytest.mark.parametrize("mb_w", (2, 3))
def test_windows_over_the_borders_emulated(emu, oracle, mb_w, run):
    """left, right (fq_windows_patch mends only what was requested), top and bottom (rows clamped) at every o, positions 0, 2, 8 and 15; 2 wide: two window tile columns are one tile"""
    W.run_edges(emu, oracle, mb_w, run)


@pytest.mark.parametrize("run", (1, 4))
def test_two_partitions_with_different_needs_emulated(emu, oracle, run):
    """fq_two: each partition's request trimmed by its own position, inside the picture and over its side borders"""
    W.run_two(emu, oracle, run)


def test_edge_table_census():
    """what the border pictures hold: every side with every tile set the rule knows, patched and (3 wide, top / bottom) merely clamped"""
    for mb_w in (2, 3):
        _, c = W.edge_set(mb_w)
        masks = {bin(W.need(pos, o)[0]) for pos in W.EDGE_POS for o in range(16)}
        assert masks == {"0b11", "0b10", "0b110", "0b111"}
        for side in W.SIDES:
            kind = "clamped" if mb_w == 3 and side in ("top", "bottom") else "patched"
            assert {m for (s, k, m) in c if s == side and k == kind} == masks, (mb_w, side)


def test_need_rule_and_line_census():
    """The rule: tile column 1 is in every (position, o) entry — a request never goes out without lanes — and the tile columns are the ones the columns read
    lie in.  On the headline's content (synth_frames_fast, seed 0x264, one 1080p picture) a plain macroblock's request touches fewer 128-byte lines on average than the
    3 tile columns x 21 rows it used to ask for; both averages are printed (derived on paper: about 10.5 and 7.3)."""
    for pos in range(16):
        for o in range(16):
            tiles, r0, r1 = W.need(pos, o)
            assert tiles & 2
            cols = range(o + 2, o + 23) if pos & 3 else range(o + 4, o + 20)
            assert tiles == sum(1 << t for t in {c >> 4 for c in cols})
            assert (r0, r1) == ((0, 20) if pos & 12 else (2, 17))
    fs = HF.synth_frames_fast(1, 120, 68, seed=0x264)
    old = new = n = 0
    for m in range(120 * 68):
        if int(fs.mb[0, m]["mb_type"]) & 7:
            continue
        o, pos, y0, t0 = W.window_origin(fs.mv[0, 0, m, 0], m % 120, m // 120)
        old += len(W.lines(7, 0, 20, y0, t0, 120, 68))
        new += len(W.lines(*W.need(pos, o), y0, t0, 120, 68))
        n += 1
    print("luma window lines per macroblock over %d macroblocks: %.2f for 3 x 21, %.2f for the positions' needs" % (n, old / n, new / n))
    assert new < old
