"""CPU: k_deblock_tiled as resident waves under the SIMT emulator (the same kernel source; its workgroups run one after the other, so
the first wave takes every ticket in order: the single-wave case, which finishes only if no band ever waits on a higher ticket — the
emulator aborts on such a wait), the rule's query, and what the table's content reaches at the band boundaries."""
import ctypes as C
import os

import pytest

import deblock_cases as D
import deblock_resident_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESIDENT_HALVES = 3           # h264_deblock.hip, DEBLOCK_RESIDENT_HALVES: half waves per SIMD and launch beside other shares; 0: a wave per band


def expected(tickets, cus, shares):
    n = tickets
    if shares > 1 and RESIDENT_HALVES:
        n = (4 * cus * RESIDENT_HALVES + 1) // 2
    return max(1, min(n, tickets))


@pytest.fixture(scope="module")
def product():
    """the product library, loaded without a device: the query with an explicit CU count needs none"""
    path = os.path.join(ROOT, "libav_amd", "libmi355dsp.so")
    if not os.path.exists(path):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return C.CDLL(path)


def test_table_reaches_both_sides_of_a_band_boundary():
    """from the oracle's pictures alone: the filter changes samples above and below band boundaries — in the rows a band hands down and
    the band below finishes — in the table as a whole and in the smooth sets in particular (a broken hand-down must not pass)"""
    whole, smooth = {}, {}
    for name, kw in R.SETS.items():
        fs, recon, dst = R.pictures(name)
        R.boundary_changes(fs, recon, dst, whole)
        if kw["refs"] == "smooth":
            R.boundary_changes(fs, recon, dst, smooth)
    for c in (whole, smooth):
        assert c["boundaries"] >= 8
        for k in ("luma_above", "luma_below", "luma_both", "chroma_above", "chroma_below"):
            assert c[k] >= 2, (k, c)


def test_batches_cover_the_ticket_counts():
    tickets = sorted(R.grid(parts)[4] for parts, _ in R.BATCHES.values())
    assert tickets[0] == 2 and tickets[-1] == 21 and {3, 10, 14, 15} <= set(tickets)
    assert any(launches == 2 for _, launches in R.BATCHES.values())
    for parts, _ in R.BATCHES.values():
        assert sorted(R.order(parts)) == sorted((k, i) for k, (s, _) in enumerate(parts) for i in range(R.SETS[s]["nframes"]))


def test_rule_query(product):
    assert not os.environ.get("MI355_DEBLOCK_RESIDENT") and not os.environ.get("MI355_DEBLOCK_WAVES") and not os.environ.get("MI355_DEBLOCK_FORM")
    for n, w, h in ((683, 120, 68), (682, 120, 68), (2048, 120, 68), (512, 120, 68), (171, 120, 68), (5000, 20, 15), (300, 20, 15)):
        tickets = n * ((h + 3) // 4)
        for cus in (256, 64, 304):
            for shares in (1, 2, 3, 4):
                if D.plan(product, n, w, h, D.LAYOUT_TILED, cus)[0] != 1:
                    assert R.rule(product, n, w, h, D.LAYOUT_TILED, cus, shares) == 0
                    continue
                got = R.rule(product, n, w, h, D.LAYOUT_TILED, cus, shares)
                assert got == expected(tickets, cus, shares), (n, w, h, cus, shares, got)
                assert 1 <= got <= tickets
                if shares == 1:
                    assert got == tickets, "nothing beside it: a wave per band"
    # the bench's shares on 256 CUs: one and a half waves per SIMD and launch; a 171-picture share (512 pictures) the same; one share: a wave per band
    assert R.rule(product, 683, 120, 68, D.LAYOUT_TILED, 256, 3) == 1536 and R.rule(product, 171, 120, 68, D.LAYOUT_TILED, 256, 3) == 1536
    assert R.rule(product, 2048, 120, 68, D.LAYOUT_TILED, 256, 1) == 2048 * 17
    # no one-wave tiled launch: the two-wave form (few bands), line-stride pictures only
    assert R.rule(product, 64, 120, 68, D.LAYOUT_TILED, 256, 3) == 0
    assert R.rule(product, 3, 3, 9, D.LAYOUT_TILED, 256, 3) == 0
    assert R.rule(product, 2048, 120, 68, D.LAYOUT_LINEAR, 256, 3) == 0
    assert R.rule(product, 2048, 120, 68, D.LAYOUT_LINEAR | D.LAYOUT_TILED, 256, 1) == 2048 * 17


def test_rule_query_rejects_bad_arguments(product):
    for args in ((0, 8, 5, 2, 256, 1), (1, 0, 5, 2, 256, 1), (1, 8, 0, 2, 256, 1), (1, 8, 5, 0, 256, 1), (1, 8, 5, 2, -1, 1), (1, 8, 5, 2, 256, 0)):
        assert R.rule(product, *args) is None, args
    R.bind(product)
    assert product.mi355_h264_deblock_resident(1, 8, 5, 2, 256, 1, None) == -1


def test_entry_rejects_bad_arguments(emu):
    fs, recon, _ = R.pictures("p15x1")
    R.bind(emu.lib)
    d = D.upload(emu, fs, recon, True)
    try:
        fn = emu.lib.mi355_h264_deblock_resident_dev
        for n, w, h, layouts, resident in ((0, 1, 5, 2, 1), (1, 0, 5, 2, 1), (1, 1, 0, 2, 1), (1, 1, 5, 0, 1), (1, 1, 5, 2, -1)):
            assert fn(d.d_desc, n, w, h, layouts, resident, None) == -1, (n, w, h, layouts, resident)
        assert fn(None, 1, 1, 5, 2, 1, None) == -1
    finally:
        d.free()


@pytest.mark.parametrize("name", list(R.BATCHES))
def test_resident_batches_emulated(emu, name):
    R.run_batch(emu, name)


def test_pipelines_object_with_resident_waves_emulated(emu, oracle):
    """(the fixtures: the emulator library and the oracle are built before the child process looks for them)"""
    R.run_pinned("emu")
