"""CPU: the tables of tests/hevc_recon_tables.py reach what they are for — a census of the inputs, from the oracle's own outputs and numpy int64
restatements of the unclipped passes; the saturating classes pinned on the reference's objects and on tests/golden/hevc_recon_tables_sha1.json."""
import json
import os

import numpy as np
import pytest

import hevc_recon_tables as T
from cases_hevc import EW, QW

DEPTHS = (8, 9, 10)
GOLD = os.path.join(os.path.dirname(__file__), "golden", "hevc_recon_tables_sha1.json")


def test_motion_and_prediction_tables_cover_every_shape():
    rows = T.mc_rows()
    assert {(r["chroma"], r["wi"], r["mx"], r["my"]) for r in rows} == ({(0, wi, mx, my) for wi in range(8) for mx in range(4) for my in range(4)} |
                                                                        {(1, wi, mx, my) for wi in range(8) for mx in range(8) for my in range(8)})
    assert len(rows) == 8 * 16 + 8 * 64
    # every width of the reference's put_hevc_qpel / put_hevc_epel tables with every height (luma 4..64, chroma 2..32)
    assert {(r["w"], r["h"]) for r in rows if not r["chroma"]} == {(w, h) for w in QW for h in T.HL}
    assert {(r["w"], r["h"]) for r in rows if r["chroma"]} == {(w, h) for w in EW for h in T.HC}
    pr = T.pred_rows()
    for kind in (1, 2, 3):
        for chroma in (0, 1):
            for wi in range(8):
                sel = [r for r in pr if (r["kind"], r["chroma"], r["wi"]) == (kind, chroma, wi)]
                assert sel and {c for r in sel for c in r["cls"]} == {"tap-max", "tap-min"}
                if kind > 1:
                    assert {r["denom"] for r in sel} == {0, 7} and {r["wt"][0] for r in sel} == {-128, 127} and {r["wt"][2] for r in sel} == {-128, 127}
                if kind == 3:
                    assert {r["wt"][1] for r in sel} == {-128, 127} and {r["wt"][3] for r in sel} == {-128, 127}
    # the emulator's share: noise everywhere, the tap classes for every two-direction fraction of every width
    for j in T.pred_jobs("tap-max"):
        assert T.emu_keeps(j, "noise")
        if j["kind"] == 0 and j["f"][0] and j["f"][1]:
            assert T.emu_keeps(j, "tap-max") and T.emu_keeps(j, "tap-min")


@pytest.mark.parametrize("bd", DEPTHS)
def test_tap_tables_are_the_oracles_impulse_responses(oracle, bd):
    """one sample of 1 << (bd - 8) in an empty window: the one-direction filters answer with their taps, unshifted"""
    c, at = oracle.hevcdsp(bd), 4
    for chroma in (0, 1):
        before, n = (1, 4) if chroma else (3, 8)
        for f in range(1, 8 if chroma else 4):
            want = np.array([T.taps_of(chroma, f)[at + before - x] if 0 <= at + before - x < n else 0 for x in range(16)])
            for horizontal in (1, 0):
                row = dict(chroma=chroma, wi=5 if chroma else 3, w=16, h=16, mx=f if horizontal else 0, my=0 if horizontal else f)
                win = np.zeros((1, T.CELL, T.CELL), np.uint16 if bd > 8 else np.uint8)
                win[0, T.ORG + (0 if horizontal else at), T.ORG + (at if horizontal else 0)] = 1 << (bd - 8)
                out = T.mc_expected(c, bd, [row], win)[0].reshape(64, 64)
                assert np.array_equal(out[0, :16] if horizontal else out[:16, 0], want), (chroma, f, horizontal, bd)


@pytest.mark.parametrize("bd", DEPTHS)
def test_tap_classes_reach_the_filters_bounds(oracle, bd):
    c, rows, top = oracle.hevcdsp(bd), T.mc_rows(), (1 << bd) - 1
    noise = T.mc_expected(c, bd, rows, T.mc_windows(rows, "noise", bd))
    wraps = 0
    for cls in ("tap-max", "tap-min"):
        win = T.mc_windows(rows, cls, bd)
        out = T.mc_expected(c, bd, rows, win)
        for k, row in enumerate(rows):
            o = out[k].reshape(64, 64)[:row["h"], :row["w"]].astype(np.int64)
            rest = T.mc_restated(row, win[k], bd)
            assert np.array_equal(o, rest.astype(np.int16)), "%s %s bd%d: the oracle is not the restated passes" % (row["name"], cls, bd)
            wraps += int((rest != rest.astype(np.int16)).any())
            if not (row["mx"] and row["my"]):
                t = T.taps_of(row["chroma"], row["mx"] or row["my"])
                bound = (top * int(t[t > 0].sum() if cls == "tap-max" else t[t < 0].sum())) >> (bd - 8)
                assert o[0, 0] == bound and (o.max() if cls == "tap-max" else o.min()) == bound, "%s %s bd%d" % (row["name"], cls, bd)
            else:
                n = noise[k].reshape(64, 64)[:row["h"], :row["w"]]
                assert rest[0, 0] > n.max() if cls == "tap-max" else rest[0, 0] < n.min(), "%s %s bd%d" % (row["name"], cls, bd)
    # the 8-tap filter in both directions passes int16 on tap-max (the reference's intermediate wraps there): that row exists
    assert wraps > 0


@pytest.mark.parametrize("bd", DEPTHS)
def test_transform_table_reaches_the_clips(oracle, bd):
    c, top = oracle.hevcdsp(bd), (1 << bd) - 1
    up, down, second, res_lo, res_hi, aligned = set(), set(), set(), 0, 0, set()
    rows = T.tu_rows()
    for size in (4, 8, 16, 32):
        assert {r["lim"] for r in rows if r["kind"] == 0 and r["rule"] == "decoder" and 1 << r["log2"] == size} == set(T.decoder_lims(size)), size
        assert {r["lim"] for r in rows if r["rule"] == "plain" and 1 << r["log2"] == size} == set(range(1, size + 1))
    assert {(r["log2"], r["kind"]) for r in rows} == {(l, 0) for l in (2, 3, 4, 5)} | {(l, 1) for l in (2, 3, 4, 5)} | {(2, 2), (2, 3)}
    for cls in T.TU_CLASSES:
        for row, coef, dcls, al in T.tu_units(bd, cls):
            size = 1 << row["log2"]
            aligned.add((size, al))
            if not al:
                continue                                   # the same coefficients as the aligned unit before it
            blk = coef.reshape(-1).copy()
            T.call_tu(c, row, blk)
            res = blk.astype(np.int64)
            res_lo += int(dcls == "zero" and (res < 0).any())
            res_hi += int(dcls == "max" and (res > 0).any())
            if row["kind"] != 0 or dcls != T.tu_dst_classes(cls, 0)[0] and len(T.tu_dst_classes(cls, 0)) > 1:
                continue
            t1 = T.first_pass_unclipped(row, coef)
            t2 = T.second_pass_unclipped(row, np.clip(t1, -32768, 32767), bd)
            assert np.array_equal(np.clip(t2, -32768, 32767).reshape(-1), res), "%s %s bd%d: the oracle is not the restated passes" % (row["name"], cls, bd)
            if (t1 > 32767).any():
                up.add(size)
            if (t1 < -32768).any():
                down.add(size)
            if (t2 > 32767).any() or (t2 < -32768).any():
                second.add(size)
    assert up == {4, 8, 16, 32} and down == {4, 8, 16, 32}
    assert res_lo > 0 and res_hi > 0                       # add_residual clips at 0 and at the maximum
    for size in (16, 32):
        assert (size, True) in aligned and (size, False) in aligned
    for size in (4, 8, 16, 32):
        can = (int(np.abs(T.dct_matrix(size)).sum(axis=0).max()) * 32767) >> (20 - bd) > 32767
        assert (size in second) == can, "second pass at size %d, bd %d: the matrix allows a clip: %s, the table reaches one: %s" % (size, bd, can, size in second)
    assert (32 in second) == (bd == 10)                    # at 10 bits the 32-point rows can pass int16; at 8 bits no size can


def test_decoder_made_blocks_lie_inside_what_the_pruned_passes_read():
    """include/mi355_hevc_batch.h's precondition for the matrix-path inverse DCT — rows and columns below col_limit + 4, and nothing where the reference's
    pruned passes do not read — holds for every last significant position of the diagonal scan"""
    for size in (8, 16, 32):
        ys, xs = np.mgrid[0:size, 0:size]
        for lx in range(size):
            for ly in range(size):
                if lx or ly:
                    lim = T.decoder_lim(lx, ly)
                    allowed = T.pruned_mask(size, lim) & (ys < lim + 4) & (xs < lim + 4)
                    assert not (T.keep_mask(size, lx, ly) & ~allowed).any(), (size, lx, ly, lim)


@pytest.mark.parametrize("bd", (8, 10))
def test_clipping_units_reach_the_matrix_path_and_the_general_body(bd):
    """of the clip-high table, 32x32 and 16x16 units whose first pass passes int16 upward AND downward lie 16-byte aligned in blocks the matrix-path kernel takes
    (hevc_ctb_fast.h), and 8 bytes off in blocks of the general kernel (the batch kernels' body, hevc_dev.h)"""
    s = T.tu_scene(bd, "clip-high")
    seen = set()
    for b in s.ctbs:
        fast = T.ctb_takes_matrix_path(s, b)
        for u in s.tu[b["tu"][0]:b["tu"][0] + b["tu"][1]]:
            row = u["row"]
            if row["kind"] == 0 and row["log2"] >= 4:
                n = 1 << (2 * row["log2"])
                t1 = T.first_pass_unclipped(row, s.arr[u["coef"][0]].reshape(-1)[u["coef"][1] // 2:u["coef"][1] // 2 + n])
                if (t1 > 32767).any() and (t1 < -32768).any():
                    seen.add((row["log2"], fast, u["coef"][0] == "coef"))
    for log2 in (4, 5):
        assert (log2, True, True) in seen and (log2, False, False) in seen, sorted(seen)


@pytest.mark.parametrize("bd", (8, 10))
def test_geometry_table_covers_every_combination(bd):
    s = T.geometry_scene(bd)
    seen = {(b["log2"], b["w"] % (1 << b["log2"]), b["h"] % (1 << b["log2"]), b["flags"]) for b in s.ctbs}
    for log2 in (4, 5, 6):
        rems = [0] + [q for q in (8, 24, 56) if q < 1 << log2]
        for rw in rems:
            for rh in rems:
                for partial in (0, 1):
                    assert (log2, rw, rh, partial) in seen, (log2, rw, rh, partial)
    heavy = [b for b in s.ctbs if b["fine"]]
    assert len(heavy) == 1 and heavy[0]["mc"][1] + heavy[0]["tu"][1] > 512       # more jobs than the larger kernel has threads
    assert {j["chroma"] for j in s.mc} == {0, 1, 2}                              # single chroma jobs and Cb + Cr pairs
    assert {j["ss"][0] % (16 if bd > 8 else 8) == 0 for j in s.mc} == {True, False}          # reference rows for the matrix path and for the general one
    uni = [T.ctb_takes_matrix_path(s, b) for b in s.ctbs]
    assert 0 < sum(uni) < len(uni)
    assert {u["coef"][0] for u in s.tu} == {"coef", "coef8"}
    assert any(b["w"] < 16 for b in s.ctbs if b["log2"] == 6)                    # a picture narrower than one block


@pytest.fixture(scope="module")
def oracle_digests(oracle):
    return T.saturating_digests(oracle)


def test_saturating_classes_match_the_reference_objects(oracle_digests, ref):
    want, got = T.saturating_digests(ref), oracle_digests
    bad = [k for k in want if want[k] != got[k]]
    assert set(want) == set(got) and not bad, bad[:20]


def test_saturating_classes_match_the_recorded_digests(oracle_digests):
    with open(GOLD) as f:
        gold = json.load(f)
    got = oracle_digests
    bad = [k for k in gold if gold[k] != got.get(k)]
    assert set(gold) == set(got) and not bad, bad[:20]
