"""CPU: what the run kernel's tables (tests/h264_run_tables.py) hold — the run-length rule at the benchmark's batch, and a census of every table: no class
the tables are built for may be empty.  No backend runs here (the oracle only, for the weighted samples of table C)."""
import ctypes as C
import os

import pytest

import h264_run_tables as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def product():
    """the product library, loaded without a device: the run plan is host arithmetic"""
    path = os.path.join(ROOT, "libav_amd", "libmi355dsp.so")
    if not os.path.exists(path):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return C.CDLL(path)


def test_run_plan_pins_the_headline(product):
    assert T.run_plan(product, 2048, 120, 68) == (15, 8)          # bench.py's batch: eight runs of fifteen to a row
    assert T.run_plan(product, 1, 120, 68) == (4, 30)             # the largest batch the other tests run
    assert T.run_plan(product, 683, 120, 68) == (15, 8)
    assert T.run_plan(product, 256, 120, 68) == (6, 20)           # 2 088 960 macroblocks / (40 x 8192) = 6
    assert T.run_plan(product, 2048, 3, 68) == (3, 1) and T.run_plan(product, 1, 1, 1) == (1, 1)      # rows shorter than four
    assert T.run_plan(product, 2048, 17, 68) == (6, 3)            # 2 367 488 / (40 x 8192) = 7, three runs to a row, made equal: 17 = 6 + 6 + 5
    # a named length: bounded by the row, runs of a row made equal — 17 at 15 is 9 + 8, 31 at 15 is 11 + 11 + 9
    assert T.run_plan(product, 4, 17, 2, 15) == (9, 2) and T.run_plan(product, 4, 31, 2, 15) == (11, 3) and T.run_plan(product, 4, 31, 2, 11) == (11, 3)
    assert T.run_plan(product, 4, 30, 2, 8) == (8, 4) and T.run_plan(product, 4, 4, 2, 15) == (4, 1) and T.run_plan(product, 4, 16, 2, 16) == (16, 1)
    for args in ((n, w, h, forced) for n in (1, 4, 300, 2048, 100000) for w in (1, 2, 3, 4, 7, 15, 16, 17, 30, 31, 120, 240) for h in (1, 2, 68) for forced in (0, 1, 4, 5, 8, 11, 15, 16)):
        assert T.run_plan(product, *args) == T.plan_rule(*args), args


def test_run_plan_refuses_what_a_run_word_cannot_hold(product):
    """bit i and bit 16 + i of a run's word stand for its macroblock i: no run of more than 16"""
    assert T.run_plan(product, 4, 120, 2, 20) is None and T.run_plan(product, 4, 64, 2, 32) is None and T.run_plan(product, 4, 17, 2, 17) is None
    assert T.run_plan(product, 4, 16, 2, 40) == (16, 1) and T.run_plan(product, 4, 120, 2, 17) == (15, 8)       # bounded by the row and made equal first
    for args in ((0, 8, 5, 0), (1, 0, 5, 0), (1, 8, 0, 0), (1, 8, 5, -1)):
        assert T.run_plan(product, *args) is None, args
    fn = product.mi355_h264_recon_run_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 4 + [C.c_void_p] * 2
    run = C.c_int(0)
    assert fn(1, 8, 5, 0, None, C.byref(run)) == -1 and fn(1, 8, 5, 0, C.byref(run), None) == -1


def test_run_table_census(product):
    tot = {}
    entries = [(run, (w,)) for run, w in T.RUN_ENTRIES] + [T.MIXED_ENTRY]
    for run, widths in entries:
        sets = [T.run_kinds_set(run, w) for w in widths]
        mw = max(widths)
        planned = T.run_plan(product, sum(fs.F for fs in sets), mw, 2, run)
        assert planned == T.plan_rule(sum(fs.F for fs in sets), mw, 2, run)
        if run == 15 and mw in (17, 31):
            assert planned == {17: (9, 2), 31: (11, 3)}[mw]
        for k, v in T.kind_census(sets, planned[0], mw).items():
            tot[k] = tot.get(k, 0) + v
            if run == 15 and planned[0] == 15 and k[0] == "i14":
                tot[("i14_at_15", k[1])] = tot.get(("i14_at_15", k[1]), 0) + v
    kinds = range(len(T.KINDS))
    missing = [("pair", a, b) for a in kinds for b in kinds] + [(cls, k) for cls in ("first", "last_full", "last_short") for k in kinds]
    missing += [("i14_at_15", 4), ("i14_at_15", 5), ("i15", 4), ("i15", 5)] + [("window_set", s, k) for s in (0, 1) for k in (2, 3)] + [("deferred_bit", i) for i in range(15)]
    missing += [("cut_run", False), ("cut_run", True)]             # the narrower picture of the mixed launch: a run cut short, and runs wholly beside it
    assert not [k for k in missing if not tot.get(k)], [k for k in missing if not tot.get(k)]


def test_filter_table_census():
    c = {}
    for name, build in T.B_ENTRIES.items():
        form = name.rsplit("-", 2)[1] if name.startswith("extreme") else name.rsplit("-", 1)[1]
        if name.startswith("extreme") and not name.endswith("none"):
            continue                                    # the same pictures and vectors with residual on top
        T.filter_census(build(), form, c)
    for form in T.FORMS:           # the run kernel, fq_two and the general code each see the sums their exactness arguments are about
        assert c[("H", form)] == (-2550, 10710) and c[("J", form)] == (-214200, 475320), (form, c[("H", form)], c[("J", form)])
    assert c["chroma"] == (0, 255 * 64)
    want = [(comp, form, how) for comp in "bhj" for form in T.FORMS for how in ("low", "high", "inside")]
    want += [("pos", p, form) for p in range(16) for form in T.FORMS] + [("chroma_pos", x, y) for x in range(8) for y in range(8)]
    want += [(k, o) for k in ("col_offset", "row_offset") for o in range(16)]
    want += [("border", form, side, rel) for form in T.FORMS for side in ("left", "top", "right", "bottom") for rel in (1, 0, -1)]
    want += [("border", form, "corner", k) for form in T.FORMS for k in range(4)] + [("border", form, "far", k) for form in T.FORMS for k in range(4)]
    assert not [k for k in want if not c.get(k)], [k for k in want if not c.get(k)]


def test_weight_table_census(oracle):
    c = {}
    for name, build in T.C_ENTRIES.items():
        T.weight_census(oracle, build(), c)
    want = [("denom", plane, d, way) for plane in ("luma", "chroma") for d in range(8) for way in ("l0", "l1", "bi")]
    want += [("use_weight_chroma", v) for v in (0, 1)] + [("chroma_left_alone", l) for l in (0, 1)] + [("implicit", w) for w in T.IMPLICIT]
    want += [("width", "luma", w) for w in (16, 8, 4)] + [("width", "chroma", w) for w in (8, 4, 2)]
    want += [("clip", plane, kind, how) for plane in ("luma", "chroma") for kind in ("uni", "bi") for how in ("low", "high", "inside")]
    assert not [k for k in want if not c.get(k)], [k for k in want if not c.get(k)]
