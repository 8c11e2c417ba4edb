"""CPU: the tables of tests/hevc_filter_tables.py reach what they are for — a census of the decisions of the deblocking filter, of boundary_strength and of SAO
from plain restatements (no product, no emulator), the oracle pinned on the reference's own functions and on tests/golden/hevc_filter_tables_sha1.json."""
import collections
import ctypes as C
import json
import os

import numpy as np
import pytest

import hevc_filter_tables as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "hevc_filter_tables_sha1.json")


def _ref_lib():
    import subprocess
    if not os.path.isdir("/root/reference/libavcodec"):
        pytest.skip("/root/reference not present")
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/libhevcfilterref.so"], check=True)
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libhevcfilterref.so"))
    lib.ref_hevc_deblock_picture.restype = C.c_int
    return lib


def _oracle_deblock(oracle):
    oracle.lib.oracle_hevc_deblock_picture.restype = None
    return oracle.lib.oracle_hevc_deblock_picture


# ---- deblocking -------------------------------------------------------------------------------------------------------------------------------
def test_deblock_table_holds_every_shape():
    rows = [T.LfCase(n) for n in T.LF_CASES]
    assert {c.l2ctb for c in rows} == {4, 5, 6} and {(c.l2cb, c.l2pu) for c in rows} == {(3, 2), (4, 3), (5, 4)}
    for c in rows:
        assert c.w % (1 << c.l2cb) == 0 and c.h % (1 << c.l2cb) == 0 and c.w <= 208 and c.h <= 136 and 1 <= c.npics <= 3
    for bd in T.DEPTHS:
        sel = [c for c in rows if c.bd == bd]
        assert any((c.w, c.h) == (16, 16) for c in sel) and any(c.w == 8 for c in sel) and any(c.h == 8 for c in sel)
        assert any(c.w % 16 == 8 and c.h % 16 == 8 for c in sel)
        assert any(c.w % (1 << c.l2ctb) and c.h % (1 << c.l2ctb) for c in sel)
        assert {c.pcmf for c in sel} == {0, 1} and {c.npics for c in sel} == {1, 2, 3}
        pics = [p for c in sel for p in T.lf_launch(c.name)]
        for k in (0, 1):
            assert {-12, 12} <= {(p.cb_off, p.cr_off)[k] for p in pics}
            assert {-12, 12} <= {int(v) for p in pics for v in p.db[:, k]}
        assert min(int(p.qp.min()) for p in pics) == T.QP_MIN[bd] and max(int(p.qp.max()) for p in pics) == 51
    # the launch's workgroups: (luma segments / 64 + chroma segments / 64, each rounded up) per picture; a multiple of eight takes the kernel's XCD order
    assert T.lf_workgroups(104, 72, 2) == (8, 8) and T.lf_workgroups(160, 128, 1) == (8, 8)          # r104 (two pictures), c160 (one)
    assert T.lf_workgroups(200, 136, 3) == (33, 33) and T.lf_workgroups(16, 16, 1) == (2, 2)         # r200 (three pictures), s16
    for c in rows:
        assert all(n % 8 == 0 for n in T.lf_workgroups(c.w, c.h, c.npics)) == (c.name.split("_")[0] in ("r104", "c160"))


@pytest.fixture(scope="module")
def lf_counts(oracle):
    fn = _oracle_deblock(oracle)
    per_depth = {bd: collections.Counter() for bd in T.DEPTHS}
    for name in T.LF_CASES:
        for case in T.lf_launch(name):
            per_depth[case.bd].update(T.lf_census(case, case.typed(), case.typed(T.lf_host(fn, case, vertical_only=True))))
    return per_depth


@pytest.mark.parametrize("bd", T.DEPTHS)
def test_deblock_census_reaches_every_class(lf_counts, bd):
    """every decision class of the luma and chroma edge filters and of their parameters occurs in the table at this bit depth.  Left out, with the reason:
    a negative QP at 8 bits (QpBdOffset is 0 there: qp_y_tab holds 0..51); saturation in the strong filter (its outputs are clipped towards a weighted mean of
    samples, never out of range: the reference does not clip them to the sample range either)."""
    cnt = lf_counts[bd]
    wanted = T.LF_LUMA_CLASSES + T.LF_CHROMA_CLASSES + (T.LF_DEEP_CLASSES if bd > 8 else [])
    print("\n".join("%-60s %d" % (k, cnt[k]) for k in wanted))
    assert not [k for k in wanted if cnt[k] == 0]


@pytest.mark.parametrize("name", T.LF_CASES)
def test_deblock_oracle_matches_reference(oracle, name):
    ref = _ref_lib()
    for case in T.lf_launch(name):
        want, got = T.lf_host(ref.ref_hevc_deblock_picture, case), T.lf_host(_oracle_deblock(oracle), case)
        for c in range(3):
            assert np.array_equal(want[c], got[c]), "%s picture %d: plane %d differs (%d bytes)" % (name, case.pic, c, int((want[c] != got[c]).sum()))
            assert T.outside_is_poison(got[c], *case.plane_size(c), case.bd)


@pytest.mark.parametrize("name", T.LF_CASES)
def test_deblock_oracle_matches_golden(oracle, name):
    gold = json.load(open(GOLD))["deblock"][name]
    assert [T.digest(T.lf_host(_oracle_deblock(oracle), case)) for case in T.lf_launch(name)] == gold


# ---- boundary strengths -------------------------------------------------------------------------------------------------------------------------
def test_bs_table_holds_every_granule():
    rows = [T.BsCase(n) for n in T.BS_CASES]
    assert {(c.l2pu, c.l2tb) for c in rows} == {(p, t) for p in (2, 3) for t in (2, 3, 4)}
    assert min((c.w, c.h) for c in rows) == (8, 8) and max(c.w for c in rows) == 160
    assert any(c.w % T.BS_CASES[c.name][2] and c.h % T.BS_CASES[c.name][2] for c in rows)
    for c in rows:
        # motion fields and cbf maps are arrays AT their granules: constant over them by construction
        assert c.mvf.shape == (-(-c.h >> c.l2pu), -(-c.w >> c.l2pu)) and c.cbf.shape == (-(-c.h >> c.l2tb), -(-c.w >> c.l2tb))
    assert max(int(c.mvf["ref_idx"].max()) for c in rows) == 15
    for l in range(2):
        assert len(set(T.BS_POCS[l].tolist())) < 16 and set(T.BS_POCS[0].tolist()) & set(T.BS_POCS[1].tolist())


def test_bs_census_reaches_every_branch(oracle):
    cnt = collections.Counter()
    for name in T.BS_CASES:
        c = T.BsCase(name)
        v, h, k = T.bs_census(c)
        cnt.update(k)
        ov, oh = T.bs_host(oracle.lib.oracle_hevc_boundary_strengths, c)
        assert np.array_equal(v, ov) and np.array_equal(h, oh), name          # the restatement that counts is the function the oracle computes
    print("\n".join("%-60s %d" % (k, cnt[k]) for k in T.BS_CLASSES))
    assert not [k for k in T.BS_CLASSES if cnt[k] == 0]


@pytest.mark.parametrize("name", list(T.BS_CASES))
def test_bs_oracle_matches_reference_function(oracle, name):
    ref = _ref_lib()
    c = T.BsCase(name)
    rv, rh = T.bs_host(ref.ref_hevc_boundary_strengths, c, with_blocks=True)
    ov, oh = T.bs_host(oracle.lib.oracle_hevc_boundary_strengths, c)
    assert np.array_equal(rv, ov), "vertical_bs differs at %s" % np.flatnonzero(rv != ov)[:8]
    assert np.array_equal(rh, oh), "horizontal_bs differs at %s" % np.flatnonzero(rh != oh)[:8]
    assert T.bs_digest(c, ov, oh) == json.load(open(GOLD))["bs"][name]


@pytest.mark.parametrize("name", list(T.BS_CASES))
def test_bs_oracle_matches_golden(oracle, name):
    c = T.BsCase(name)
    assert T.bs_digest(c, *T.bs_host(oracle.lib.oracle_hevc_boundary_strengths, c)) == json.load(open(GOLD))["bs"][name]


# ---- SAO ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bd", T.DEPTHS)
def test_sao_census_reaches_every_class(bd):
    cnt = collections.Counter()
    across = set()
    for log2_ctb in T.SAO_SIZES:
        for rot in range(T.SAO_ROTATIONS):
            case = T.SaoCase(bd, log2_ctb, rot)
            assert (case.cw, case.chn) == (4, 3) and case.W % 16 == 8 and case.H % (1 << log2_ctb) == 8
            cnt.update(T.sao_census(case))
            across.add(case.filter_edges[-1])
            assert len(set(case.slice_addr)) == 2
    print("\n".join("%-60s %d" % (k, cnt[k]) for k in T.SAO_CLASSES))
    assert not [k for k in T.SAO_CLASSES if cnt[k] == 0]
    assert across == {0, 1}
