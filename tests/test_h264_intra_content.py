"""CPU: what the intra tables (tests/h264_intra_tables.py) hold — the launch-form rule of the intra pass, and a census of every table read off the records and the carriers'
samples: no class the tables are built for may be empty.  No backend runs here (the oracle only; the plan function is host arithmetic)."""
import ctypes as C
import os

import numpy as np
import pytest

import h264_frames as HF
import h264_intra_tables as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = [(bool(c & 1), bool(c & 2), bool(c & 4), bool(c & 8)) for c in range(16)]


@pytest.fixture(scope="module")
def product():
    """the product library, loaded without a device"""
    path = os.path.join(ROOT, "libav_amd", "libmi355dsp.so")
    if not os.path.exists(path):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return C.CDLL(path)


def plan(lib, mb_w, mb_h, widths, pinned=-1):
    fn = lib.mi355_h264_recon_intra_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lw = (C.c_int32 * max(1, len(widths)))(*widths)
    single, per = C.c_int(-1), C.c_longlong(-1)
    assert fn(mb_w, mb_h, len(widths), lw, pinned, C.byref(single), C.byref(per)) == 0
    return single.value, per.value


def test_intra_plan_pins_the_threshold(product):
    """sixteen levels take the single launch, fifteen the launch per level; MI355_INTRA_SINGLE pins a form; widths that sum to 0 launch nothing"""
    assert "MI355_INTRA_SINGLE" not in os.environ, "the rule itself is pinned here: unset MI355_INTRA_SINGLE"
    assert plan(product, 40, 22, [3] * 15) == (0, 0) and plan(product, 40, 22, [3] * 16) == (1, 48)
    assert plan(product, 40, 22, []) == (0, 0) and plan(product, 120, 68, [1] * 254) == (1, 254)
    assert plan(product, 4, 3, [5] * 16) == (1, 12)                       # bounded by the grid
    assert plan(product, 40, 22, [0] * 16) == (1, 0) and plan(product, 40, 22, [-2] * 20) == (1, 0)
    assert plan(product, 40, 22, [3] * 16, pinned=0) == (0, 0) and plan(product, 40, 22, [3] * 2, pinned=1) == (1, 6) and plan(product, 40, 22, [0, 0], pinned=1) == (1, 0)
    fn = product.mi355_h264_recon_intra_plan
    one, s, p = (C.c_int32 * 1)(1), C.c_int(0), C.c_longlong(0)
    for args in ((0, 22, 1, one, -1, C.byref(s), C.byref(p)), (40, 0, 1, one, -1, C.byref(s), C.byref(p)), (40, 22, -1, one, -1, C.byref(s), C.byref(p)),
                 (40, 22, 1, None, -1, C.byref(s), C.byref(p)), (40, 22, 1, one, -1, None, C.byref(p)), (40, 22, 1, one, -1, C.byref(s), None)):
        assert fn(*args) == -1


@pytest.fixture(scope="module")
def counts(oracle):
    """the census of every 8-bit entry, and of tables B and C at every format where the checker of that format is built"""
    c, poisoned = {}, {}
    for name in T.ENTRIES:
        fs, ref = T.entry(oracle, name)
        c[name] = T.census(fs, ref[0])
        if name != "D-chains":
            poisoned[name] = T.poison_census(fs, ref[0])
    return c, poisoned


def missing(c, want):
    return [k for k in want if not c.get(k)]


def test_table_a_census(counts):
    c, poisoned = counts
    for kind in ("i4", "i8"):
        want, cc = [], c["A-" + kind]
        for cls in CLASSES:
            left, top, tl, tr = cls
            tlm, _ = HF._avail_masks(top, left, tl, tr)
            for b in (range(4) if kind == "i8" else T.REACH4):
                i = 4 * b if kind == "i8" else b
                x4, y4 = HF.blk_xy(i)
                btop, bleft, btl = top or y4 > 0, left or x4 > 0, bool((tlm << i) & 0x8000)
                modes = ([0, 1, 2, 3, 7, 8] + ([4, 5, 6] if btl else [])) if btop and bleft else ([1, 8, 9] if bleft else ([0, 3, 7, 10] if btop else [11]))
                want += [(kind, cls, b, m) for m in modes]
        assert not missing(cc, want), missing(cc, want)
    c4 = c["A-i4"]
    # above-right: blocks 1 and 4 read the macroblock above (present wherever their modes are legal), block 5 the macroblock above-right: present and replicated
    want = [("tr", b, m, True) for b in (1, 4, 5) for m in (3, 7)] + [("tr", b, m, False) for b in (5, 3, 7, 11, 13, 15) for m in (3, 7)]
    assert not missing(c4, want), missing(c4, want)
    # Intra 8x8: what a legal stream can hold — a mode that reads the row above never has both off (block 0 then has the row above, has_tr; block 1 the corner, has_tl);
    # the down-right modes need the corner
    want = [("i8_tl_tr", m, a, b) for m in (0, 2, 3, 7) for (a, b) in ((True, True), (True, False), (False, True))]
    want += [("i8_tl_tr", m, True, b) for m in (4, 5, 6) for b in (True, False)] + [("i8_tl_tr", m, a, b) for m in (1, 8) for a in (True, False) for b in (True, False)]
    # TOP_DC: no left neighbour, so blocks 0 and 2, which always have has_tr with a row above; LEFT_DC: no row above, so block 0 (no has_tr) and block 1 (no has_tl)
    want += [("i8_tl_tr", 10, True, True), ("i8_tl_tr", 10, False, True), ("i8_tl_tr", 9, True, False), ("i8_tl_tr", 9, False, False), ("i8_tl_tr", 9, False, True)]
    want += [("i8_tl_tr", 11, False, False)]
    assert not missing(c["A-i8"], want), missing(c["A-i8"], want)
    c16 = c["A-i16"]
    for cls in CLASSES:
        slots = T.mb_cands(cls[0], cls[1], cls[2])
        assert sorted(slots) == sorted(([0, 1, 2] + ([3] if cls[2] else [])) if cls[0] and cls[1] else ([1, 4] if cls[0] else ([2, 5] if cls[1] else [6])))
        want = [("i16", cls, s) for s in slots] + [("chroma", cls[:3], s) for s in slots]
        assert not missing(c16, want), missing(c16, want)
    for name in ("A-i4", "A-i8", "A-i16"):
        assert not missing(poisoned[name], ["left", "top", "tl", "tr"]), (name, poisoned[name])


def test_table_b_census(oracle, counts):
    c, _ = counts
    for depth, idc in T.FORMATS:
        maxv = (1 << depth) - 1
        fs, ref = T.entry(oracle, "B-plane", depth, idc)
        if ref is None:
            continue                            # the checker above 8 bits is not built here: the 8-bit census stands
        cp = T.census(fs, ref[0])
        assert cp[("plane16", "H")] == (-36 * maxv, 36 * maxv) and cp[("plane16", "V")] == (-36 * maxv, 36 * maxv), (depth, cp[("plane16", "H")], cp[("plane16", "V")])
        assert cp[("planec", idc, "H")] == (-10 * maxv, 10 * maxv), (depth, idc)
        assert cp[("planec", idc, "V")] == ((-36 * maxv, 36 * maxv) if idc == 2 else (-10 * maxv, 10 * maxv)), (depth, idc)
        want = [("clip", col, how) for col in range(4) for how in ("low", "high", "inside")]
        want += [("planec_plane", idc, p, s, s) for p in (1, 2) for s in (1, -1)]
        assert not missing(cp, want), (depth, idc, missing(cp, want))
        fs, ref = T.entry(oracle, "B-dc", depth, idc)
        cd = T.census(fs, ref[0])
        want = [("dc", form, variant, case) for form in ("i4", "i8", "i16", "chroma") for variant in ("full", "left", "top") for case in T.DC_CASES]
        want += [("dc", form, "mid", "zero") for form in ("i4", "i8", "i16", "chroma")]
        assert not missing(cd, want), (depth, idc, missing(cd, want))
        fs, ref = T.entry(oracle, "B-taps", depth, idc)
        ct = T.census(fs, ref[0])
        want = [("alt", kind, mode, ph) for kind in ("i4", "i8") for mode in range(9) for ph in (0, 1)]
        assert not missing(ct, want), (depth, idc, missing(ct, want))
        # carriers at the depth's own extremes
        assert max(int(pl.max()) for cv in fs.canvases for pl in cv.pl) == maxv and min(int(pl.min()) for cv in fs.canvases for pl in cv.pl) == 0


def test_table_c_census(oracle, counts):
    c, poisoned = counts
    for depth, idc in T.FORMATS:
        fs, ref = T.entry(oracle, "C-chroma", depth, idc)
        if ref is None:
            continue
        cc = T.census(fs, ref[0])
        assert not missing(cc, [("slot", idc, s) for s in range(11)]), (depth, idc)
        pz = T.poison_census(fs, ref[0])
        assert pz.get("left rows", 0) >= 4 and pz.get("top") and pz.get("left")
        # Cb and Cr carry different edges
        for f, m, spec in fs.tests:
            if spec["edges"]:
                x, y = m % fs.mb_w, m // fs.mb_w
                cv = fs.canvases[f]
                assert any(not np.array_equal(cv.pl[1][cv.region(1, x, y, n)], cv.pl[2][cv.region(2, x, y, n)]) for n in ("top", "left"))


def test_table_d_census(oracle, product):
    fs, ref = T.entry(oracle, "D-chains")
    levels = T.chain_census(fs)
    assert sorted(levels) == sorted(T.DIRS) and all(v >= 16 for v in levels.values()), levels
    assert plan(product, fs.mb_w, fs.mb_h, fs.level_widths[:fs.max_intra_level])[0] == 1
    for name in T.ENTRIES:          # tables A to C too: the all-I_PCM pictures give them their levels
        g, _ = T.entry(oracle, name)
        assert g.max_intra_level >= 16 and plan(product, g.mb_w, g.mb_h, g.level_widths[:g.max_intra_level])[0] == 1, name
    # a change of the first link's residual: the next link changes with it in every chain, the LAST one where the chain hands whole rows or columns on
    # (left, above, above-right).  The above-left chain hands ONE sample on, which enters every predictor with weight 1/2 at most (plane: 0.31 of it reaches
    # the next corner): a change there is gone after a few links whatever the content, so that chain is held by its links one by one.
    for direction, (f, links) in fs.chains.items():
        bumped = T.chain_set(8, 1, bump=(f, 600))
        rec2, _ = HF.run_oracle(oracle, bumped, deblock=False)
        changed = [not np.array_equal(T.mb_view(ref[0], fs, f, m), T.mb_view(rec2, fs, f, m)) for m in links]
        assert changed[0] and changed[1], (direction, changed)
        if direction != "above-left":
            assert all(changed), (direction, changed)
    # every link hangs on the one before it: stale samples in link k - 1 show in link k
    for direction, (f, links) in fs.chains.items():
        base = HF.run_oracle(oracle, fs, deblock=False)[0]
        for k in (5, 16):
            g = T.chain_set(8, 1)
            g.coef[f, links[k]][0:256:16 if g.mb[f, links[k]]["mb_type"] & HF.I4 else 64] += 600
            other = HF.run_oracle(oracle, g, deblock=False)[0]
            assert not np.array_equal(T.mb_view(base, fs, f, links[k + 1]), T.mb_view(other, fs, f, links[k + 1])), (direction, k)
