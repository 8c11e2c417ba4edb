"""CPU: the loop-filter cases of tests/deblock_cases.py reach what they are there for.  The census is computed from the records (the oracle's
boundary-strength rule restated) and from the oracle's own (recon, dst); it fails when the generator's content is thinned."""
import numpy as np
import pytest

import deblock_cases as D
import h264_frames as HF


@pytest.fixture(scope="module")
def counts(oracle):
    c = {}
    for name in D.LF_CASES:
        fs, recon, dst = D.case(name)
        D.census(fs, recon, dst, c)
    return c


def test_records_are_consistent():
    """qpc and the chroma DC multipliers follow each macroblock's QP through its picture's tables; one table pair per picture, Cb != Cr;
    LEFT / TOP only where a neighbour exists; alpha / beta offsets even and inside -12..12"""
    for name in D.LF_CASES:
        fs, _, _ = D.case(name)
        for f in range(fs.F):
            mb, sl = fs.mb[f], fs.slices[f]
            assert (sl["chroma_qp_table"] == sl["chroma_qp_table"][0]).all(), name
            cb, cr = (int(o) for o in fs.chroma_offset[f])
            assert cb != cr and -12 <= cb <= 12 and -12 <= cr <= 12
            tab = sl[0]["chroma_qp_table"]
            assert list(tab[0]) == HF.chroma_qp_table(cb) and list(tab[1]) == HF.chroma_qp_table(cr)
            qp = mb["qp"].astype(np.int64)
            assert (mb["qpc"][:, 0] == tab[0][qp]).all() and (mb["qpc"][:, 1] == tab[1][qp]).all(), name
            assert (mb["dc_qmul"][:, 1] == [HF.dc_qmul(int(q)) for q in tab[0][qp]]).all()
            assert (mb["dc_qmul"][:, 2] == [HF.dc_qmul(int(q)) for q in tab[1][qp]]).all()
            assert (qp[(mb["mb_type"] & HF.PCM) != 0] == 0).all()
            for k in ("alpha", "beta"):
                assert (mb[k] % 2 == 0).all() and (np.abs(mb[k]) <= 12).all()
            x, y = np.arange(fs.mb_w * fs.mb_h) % fs.mb_w, np.arange(fs.mb_w * fs.mb_h) // fs.mb_w
            assert not ((mb["flags"] & HF.F_LEFT) != 0)[x == 0].any() and not ((mb["flags"] & HF.F_TOP) != 0)[y == 0].any()
            inter = (mb["mb_type"] & 7) == 0
            assert not (mb["mb_type"][inter & ((mb["cbp"] & 15) == 0)] & HF.DCT8).any()
            assert not fs.coef[f][inter & (mb["cbp"] == 0)].any()


def test_table_shapes():
    """odd widths, 1-row and 1-column pictures, P and B pictures, and a picture of 25+ macroblock rows (7+ bands)"""
    kw = D.LF_CASES.values()
    assert any(k["mb_h"] == 1 for k in kw) and any(k["mb_w"] == 1 for k in kw) and any(k["mb_h"] >= 25 for k in kw)
    assert any(k["mb_w"] % 2 and k["mb_w"] > 1 for k in kw)
    assert any(k.get("bframes") for k in kw) and any(not k.get("bframes") for k in kw)
    assert 6 <= len(D.LF_CASES) <= 10


def test_edge_strengths(counts):
    """bS 0, 1, 2 on macroblock and internal edges, 4 on macroblock edges, 3 on internal edges, both directions (the census asserts that an
    intra macroblock's edges are always 4 / 3 as it goes)"""
    for d in (0, 1):
        for b in (0, 1, 2):
            assert counts.get("bs%d_mb_%d" % (b, d), 0) > 0 and counts.get("bs%d_in_%d" % (b, d), 0) > 0, (b, d)
        assert counts.get("bs4_mb_%d" % d, 0) > 0 and counts.get("bs3_in_%d" % d, 0) > 0


def test_slice_edges(counts):
    assert counts.get("cross_slice_edge", 0) > 0             # filtered macroblock edges between two slices
    assert counts.get("nodb_next_to_filtered", 0) > 0        # NO_DEBLOCK macroblocks beside filtered ones
    assert counts.get("own_slice_suppressed", 0) > 0         # edges FILTER_OWN_SLICE leaves alone


def test_qp_indices(counts):
    assert counts.get("qpc_differ", 0) > 0                   # Cb and Cr QPs differ in filtered macroblocks
    assert counts.get("luma_qp_below_16", 0) > 0 and counts.get("luma_qp_above_45", 0) > 0     # edge QPs over the whole 0..51
    assert counts.get("index_below_0", 0) > 0 and counts.get("index_above_51", 0) > 0
    assert counts.get("alpha0_edge", 0) > 0 and counts.get("index51_edge", 0) > 0


def test_picture_kinds(counts):
    assert counts.get("b_picture", 0) > 0 and counts.get("dct8", 0) > 0 and counts.get("pcm_inter_edge", 0) > 0
    assert counts.get("crossed_pair", 0) > 0                 # B pictures: the neighbour's lists crossed
    for k in ("mvd3_x", "mvd3_y", "mvd4_x", "mvd4_y"):
        assert counts.get(k, 0) > 0, k


@pytest.mark.parametrize("cls", ("luma123", "luma4", "chroma"))
def test_filter_decisions_go_both_ways(counts, cls):
    """macroblock-edge segments with bS > 0 and alpha > 0: the oracle changed p0 / q0 in at least 5 % of them and left all of them alone in
    at least 5 % (luma bS 1-3, luma bS 4 and chroma counted apart)"""
    n = counts.get("seg_" + cls, 0)
    assert n >= 100
    assert counts.get("seg_%s_changed" % cls, 0) >= 0.05 * n and counts.get("seg_%s_kept" % cls, 0) >= 0.05 * n, counts


@pytest.mark.parametrize("bit_depth", (9, 10))
def test_widened_records_follow_the_chroma_offsets(bit_depth):
    """widen_records at 9 / 10 bits: the chroma QP is Table 8-15 at clip(qp + offset, -QpBdOffsetC, 51) plus QpBdOffsetC, the chroma DC
    multiplier that QP's (the DC levels are widened by the shift); luma QPs raised by QpBdOffsetY"""
    sh = bit_depth - 8
    seen_negative = False
    for name in D.LF_CASES:
        fs, _, _ = D.case(name)
        mb, _ = HF.widen_records(fs, sh)
        assert (mb["qp"].astype(int) == fs.mb["qp"].astype(int) + 6 * sh).all()
        for f in range(fs.F):
            for p in range(2):
                for m in range(fs.mb_w * fs.mb_h):
                    x = min(max(int(fs.mb["qp"][f, m]) + int(fs.chroma_offset[f, p]), -6 * sh), 51)
                    want = (x if x < 0 else HF.CHROMA_QP[x]) + 6 * sh
                    seen_negative |= x < 0
                    assert int(mb["qpc"][f, m][p]) == want
                    assert int(mb["dc_qmul"][f, m][1 + p]) << sh == HF.dc_qmul(want)
    assert seen_negative
