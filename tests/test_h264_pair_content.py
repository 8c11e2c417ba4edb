"""CPU: the census of tests/h264_pair_tables.py.  It does not trust the stream writer: it reads the records the bridge hands to the kernels (the dump of
contrib/libav/mi355_h264_bridge.c, MI355_BRIDGE_DEBUG=<file>, one run per entry on the SIMT emulator) and counts, over the whole table, the macroblocks and edges of
every kind the pair filter, the field-macroblock branches of prediction and the bypass branches tell apart; and it decodes every entry with the reference's decoder
alone, loop filter on and off, to show that the filter had something to do on edges of every class and left others alone.  Minimum per class: 20, or 5 for the classes
marked rare below (they need a coincidence of three or four independent draws).  The bounds are conditions on the INPUTS, computed from the reference decoder and the
records; nothing here looks at what the kernels compute (tests/test_h264_pair_tables_emu.py / _gpu.py do)."""
import collections
import os
import subprocess

import numpy as np
import pytest

import h264_pair_tables as PT

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/libavcodec"), reason="needs the reference decoder objects (/root/reference)")

FIELD, INTRA, I4, I16, PCM, SKIP, DCT8 = 0x80, 7, 1, 2, 4, 0x800, 0x01000000
F_LEFT, F_TOP, F_NODB, F_WEIGHTED, F_BYPASS, F_PRED, F_OLD, F_OWN = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
KIND = {0: "frame", FIELD: "field"}


@pytest.fixture(scope="module")
def table(emu, tmp_path_factory):
    """per entry: the records (decoding order) and the reference's luma with / without the loop filter (output order)"""
    subprocess.run(["make", "-s", "-C", os.path.join(PT.ROOT, "oracle"), "_ref/h264_bridge_emu"], check=True)
    td = tmp_path_factory.mktemp("pairs")
    out = {}
    for name in PT.NAMES:
        dump = td / (name + ".txt")
        PT.run("h264_bridge_emu", name, "-", debug=dump)
        on, off = td / (name + ".on.yuv"), td / (name + ".off.yuv")
        PT.run("h264_bridge_emu", name, on, plain=True)
        PT.run("h264_bridge_emu", name, off, plain=True, nofilter=True)
        PT.check_md5(on, name, "md5")
        PT.check_md5(off, name, "md5_nofilter")
        out[name] = dict(records=PT.parse_dump(dump), on=PT.load_pictures(on, name)[0], off=PT.load_pictures(off, name)[0])
        assert len(out[name]["records"]) == PT.TABLE[name]["npics"], name
    return out


def _rows(m, n=16):
    """luma lines of a macroblock of a pair picture: a field macroblock owns every other line of its pair"""
    py, pos = m["y"] >> 1, m["y"] & 1
    return [32 * py + pos + 2 * i for i in range(n)] if m["mb_type"] & FIELD else [16 * m["y"] + i for i in range(n)]


# Table 8-15: QPc of qPI 30..51 (below 30 it is qPI itself); at more than 8 bits both sides move by QpBdOffset
_QPC = (29, 30, 31, 32, 32, 33, 34, 34, 35, 35, 36, 36, 37, 37, 37, 38, 38, 38, 39, 39, 39, 39)


def _qpc_without_offset(qp, off):
    """the chroma QP' a macroblock of luma QP' qp has when chroma_qp_index_offset is 0"""
    q = qp - off
    return qp if q < 30 else _QPC[q - 30] + off


def _band(qp, off):
    """low: 0..15 + QpBdOffset (alpha is 0: the filter is off by its table, whatever the strength); high: the last seven QPs; middle: the rest"""
    return "low (0..15)" if qp - off <= 15 else ("high (45..51)" if qp - off >= 45 else "middle (16..44)")


def _above_rows(m, top_mb, above):
    """the luma lines ABOVE a macroblock's top edge that its filter may change: the last three lines of the neighbour, on the current macroblock's own field lines where it
    is a field macroblock; a frame macroblock under a field pair is filtered against both fields: the last three lines of each = the pair's last six"""
    y0 = 32 * (m["y"] >> 1)
    if m["mb_type"] & FIELD:
        return [y0 - 6 + (m["y"] & 1) + 2 * i for i in range(3)]
    if m["y"] & 1:
        return _rows(top_mb)[-3:]
    return list(range(y0 - 6, y0)) if above["mb_type"] & FIELD else list(range(y0 - 3, y0))


def _census(table):
    c = collections.Counter()
    touched = collections.defaultdict(lambda: [0, 0])        # class -> [edges the filter changed, edges it left alone]
    for name, t in table.items():
        e = PT.TABLE[name]
        c["width %d" % e["mb_w"]] += 1
        order = PT.decode_order(name)
        shown = {d: f for f, d in enumerate(order)}
        for d, pic in enumerate(t["records"]):
            c["chroma_format_idc %d, %d bit" % (pic["idc"], pic["depth"])] += 1
            mbs = pic["mbs"]
            ptype = "B" if any(1 in m.get("lists", ()) for m in mbs.values()) else ("P" if any("lists" in m for m in mbs.values()) else "I")
            c["chroma_format_idc %d, %d bit, %s picture" % (pic["idc"], pic["depth"], ptype)] += 1
            off = 6 * (pic["depth"] - 8)                             # QpBdOffset: the records hold QP'
            changed = t["on"][shown[d]] != t["off"][shown[d]]
            if not pic["mbaff"]:
                for m in mbs.values():
                    f = m["flags"]
                    if f & F_BYPASS and m["mb_type"] & PCM:
                        c["bypass: I_PCM in a bypass picture"] += 1
                    if f & F_BYPASS and m["mb_type"] & I4 and m["mb_type"] & DCT8:
                        tag = "BYPASS + PRED + X264OLD" if f & F_OLD and f & F_PRED else ("BYPASS + PRED" if f & F_PRED else ("BYPASS + X264OLD (no PRED)" if f & F_OLD else "BYPASS alone"))
                        c["bypass: Intra 8x8, %s" % tag] += 1
                        if f & F_OLD and f & F_PRED:
                            for k in (0, 4, 8, 12):
                                if m["modes"][k] in (0, 1):
                                    c["bypass: X264OLD Intra 8x8 block %s" % ("vertical", "horizontal")[m["modes"][k]]] += 1
                            if pic["idc"] != 3 and m["cmode"] in (1, 2):
                                c["bypass: X264OLD Intra 8x8 macroblock with chroma mode %s (rare)" % {1: "horizontal", 2: "vertical"}[m["cmode"]]] += 1
                continue
            c["pair rows %d" % (pic["rows"] // 2)] += 1
            if not e.get("lossless") and len(set(_band(m["qp"], off) for m in mbs.values() if not m["flags"] & F_NODB)) > 1:
                c["QP: pair picture whose filtered macroblocks span two or three QP bands"] += 1
            for (x, y), m in sorted(mbs.items()):
                t_, f = m["mb_type"], m["flags"]
                py, pos, cur = y >> 1, y & 1, t_ & FIELD
                kind, intra = KIND[cur], bool(t_ & INTRA)
                top_mb, bot_mb = mbs[(x, 2 * py)], mbs[(x, 2 * py + 1)]
                if f & F_BYPASS:
                    c["bypass: a pair picture, %s macroblock" % kind] += 1
                else:
                    c["bypass: neither flag"] += 1
                # ---- prediction
                if t_ & I16:
                    c["Intra 16x16 mode %d, %s" % (m["i16"] if m["i16"] < 4 else 0, kind)] += 1          # the reference's numbering: 0 DC (4..6: DC without an edge), 1 horizontal, 2 vertical, 3 plane
                elif t_ & I4:
                    for k in ((0, 4, 8, 12) if t_ & DCT8 else range(16)):
                        c["Intra %s mode %d, %s" % ("8x8" if t_ & DCT8 else "4x4", m["modes"][k] if m["modes"][k] < 9 else 2, kind)] += 1
                    if t_ & DCT8:
                        c["Intra 8x8 with the above-left sample, %s" % kind] += bool(m["topleft"] & 0x8000)
                if intra and not t_ & PCM and pic["idc"] != 3:
                    c["chroma mode %d, %s" % (m["cmode"] if m["cmode"] < 4 else 0, kind)] += 1
                if t_ & DCT8 and cur:
                    c["8x8 transform in a field macroblock"] += 1
                # the above-left sample from ANOTHER pair: block 0 of Intra 4x4 / 8x8 with modes 4, 5, 6, plane prediction
                uses_tl = (t_ & I16 and m["i16"] == 3) or (t_ & I4 and m["modes"][0] in (4, 5, 6)) or (intra and not t_ & (PCM) and pic["idc"] != 3 and m["cmode"] == 3)
                if uses_tl and x > 0:
                    lk = KIND[mbs[(x - 1, 2 * py)]["mb_type"] & FIELD]
                    if pos == 1 and not cur:
                        c["above-left from the left pair: frame bottom, left pair %s" % lk] += 1
                    elif py > 0:
                        c["above-left from pair D: %s %s, left pair %s, pair D %s (rare)" % (kind, ("top", "bottom")[pos], lk, KIND[mbs[(x - 1, 2 * py - 1)]["mb_type"] & FIELD])] += 1
                if intra and e.get("cip") and cur and x > 0:
                    la, lb = mbs[(x - 1, 2 * py)], mbs[(x - 1, 2 * py + 1)]
                    if not la["mb_type"] & FIELD and bool(la["mb_type"] & INTRA) != bool(lb["mb_type"] & INTRA):
                        c["constrained intra: field macroblock with half a left edge (rare)"] += 1
                if not intra:
                    for l, L in m["lists"].items():
                        for q in range(4):
                            if L["ref_idx"][q] >= 0 and cur:
                                c["field macroblock predicting from the %s-parity field" % ("same" if L["chroma_dy"][q] == 0 else "opposite")] += 1
                    if cur and f & F_WEIGHTED:
                        c["weighted field macroblock"] += 1
                    # vertical vector difference of 2..3 quarter samples across an inner horizontal edge, same reference: limit 2 (field) against 4 (frame)
                    L = m["lists"].get(0)
                    if L and not t_ & SKIP:
                        for yy in range(1, 4):
                            for xx in range(4):
                                qa, qb = (yy - 1) // 2 * 2 + xx // 2, yy // 2 * 2 + xx // 2
                                if L["ref_idx"][qa] >= 0 and L["ref_pic"][qa] == L["ref_pic"][qb] and abs(int(L["mv"][yy][xx][0]) - int(L["mv"][yy - 1][xx][0])) < 4 \
                                        and abs(int(L["mv"][yy][xx][1]) - int(L["mv"][yy - 1][xx][1])) in (2, 3):
                                    c["vertical vector difference 2..3 across an inner edge, %s macroblock" % kind] += 1
                # ---- skips: which pairs carry no mb_field_decoding_flag
                if pos == 0 and top_mb["mb_type"] & SKIP:
                    if not bot_mb["mb_type"] & SKIP:
                        c["skip: top skipped, bottom coded"] += 1
                    else:
                        a = mbs.get((x - 1, y))
                        b_ = mbs.get((x, y - 1))
                        a_in = a is not None and a["slice_id"] == m["slice_id"]
                        b_in = b_ is not None and b_["slice_id"] == m["slice_id"]
                        if a_in:
                            assert cur == a["mb_type"] & FIELD, (name, d, x, y)
                            c["skip: pair with the flag inferred from A (%s)" % KIND[cur]] += 1
                        elif b_in:
                            assert cur == b_["mb_type"] & FIELD, (name, d, x, y)
                            c["skip: pair with the flag inferred from B (%s) (rare)" % KIND[cur]] += 1
                        else:
                            assert not cur, (name, d, x, y)
                            c["skip: pair defaulted to frame"] += 1
                # ---- the pair filter's edges
                if f & F_NODB:
                    if x > 0 and not mbs[(x - 1, y)]["flags"] & F_NODB:
                        c["NO_DEBLOCK macroblock to the right of a filtered one (rare)"] += 1
                    continue
                if x > 0 and mbs[(x - 1, y)]["flags"] & F_NODB:
                    c["filtered macroblock to the right of a NO_DEBLOCK one (rare)"] += 1
                rows = _rows(m)
                if not f & F_BYPASS:
                    c["QP: filtered macroblock, luma QP %s" % _band(m["qp"], off)] += 1
                    # every picture parameter set of the writer has chroma QP offsets (Cb 2, -4, 6; Cr -3, 5, 0 for sets 0, 1, 2): npps decides which of them occur
                    for p, pl in enumerate(("Cb", "Cr")):
                        moved = m["qpc"][p] != _qpc_without_offset(m["qp"], off)
                        c["QP: filtered macroblock, luma QP %s, %s QP %s" % (_band(m["qp"], off), pl, "moved by its offset" if moved else "as without an offset")] += 1
                        if 0 < m["qp"] - off < 30 and 0 < m["qpc"][p] - off < 29:          # a chroma QP below 29 is qPI itself (Table 8-15), unclipped above 0: the offset can be read off
                            c["QP: filtered macroblock with a %s QP offset of %d" % (pl, m["qpc"][p] - m["qp"])] += 1
                if x > 0:
                    la, lb = mbs[(x - 1, 2 * py)], mbs[(x - 1, 2 * py + 1)]
                    lkind = KIND[la["mb_type"] & FIELD]
                    either = intra or bool(la["mb_type"] & INTRA) or bool(lb["mb_type"] & INTRA)
                    key = "left edge: %s beside a %s pair, %s" % (kind, lkind, "intra on either side" if either else "inter")
                    if f & F_OWN and la["slice_id"] != m["slice_id"]:            # the pair filter compares slice_id itself
                        c["left edge suppressed at a slice boundary (FILTER_OWN_SLICE): %s beside %s" % (kind, lkind)] += 1
                    else:
                        c[key] += 1
                        if la["slice_id"] == m["slice_id"]:
                            c["left edge inside a slice: %s beside %s" % (kind, lkind)] += 1
                        if kind != lkind and la["qp"] != lb["qp"]:
                            c["left edge of a mixed pair with two left QPs: %s beside %s" % (kind, lkind)] += 1
                        if not f & F_BYPASS:                   # the neighbour in this macroblock row is one of the edge's left macroblocks in every combination
                            c["QP: left edge, average luma QP %s" % _band((m["qp"] + mbs[(x - 1, y)]["qp"] + 1) >> 1, off)] += 1
                        touched[key][0 if changed[rows, 16 * x - 3:16 * x + 3].any() else 1] += 1
                above = None
                if pos == 1 and not cur:
                    key, above = "top edge: frame bottom macroblock (its own pair's top)", top_mb
                elif py == 0:
                    key = "top edge: first pair row, %s %s" % (kind, ("top", "bottom")[pos])
                else:
                    above = mbs[(x, 2 * py - 1)]
                    akind = KIND[above["mb_type"] & FIELD]
                    key = ("top edge: field bottom macroblock under a %s pair" % akind) if pos else ("top edge: %s top macroblock under a %s pair%s" % (kind, akind, " (filtered twice)" if not cur and akind == "field" else ""))
                if above is not None:
                    if f & F_OWN and above["slice_id"] != m["slice_id"]:
                        c[key.replace("top edge:", "top edge suppressed at a slice boundary (FILTER_OWN_SLICE):")] += 1
                        continue
                    key += ", intra" if intra or above["mb_type"] & INTRA else ", inter"
                    touched[key][0 if changed[rows[:3] + _above_rows(m, top_mb, above), 16 * x:16 * x + 16].any() else 1] += 1
                c[key] += 1
    return c, touched


def test_census_of_the_pair_tables(table):
    c, touched = _census(table)
    for k in sorted(c):
        print("%6d  %s" % (c[k], k))
    for k in sorted(touched):
        print("%6d changed %6d unchanged  %s" % (touched[k][0], touched[k][1], k))
    need = []
    kinds = ("frame", "field")
    for cur in kinds:
        for left in kinds:
            need += ["left edge: %s beside a %s pair, %s" % (cur, left, w) for w in ("intra on either side", "inter")]
            need += ["left edge inside a slice: %s beside %s" % (cur, left), "left edge suppressed at a slice boundary (FILTER_OWN_SLICE): %s beside %s" % (cur, left)]
            if cur != left:
                need.append("left edge of a mixed pair with two left QPs: %s beside %s" % (cur, left))
    tops = ["frame bottom macroblock (its own pair's top)", "frame top macroblock under a frame pair", "frame top macroblock under a field pair (filtered twice)",
            "field top macroblock under a field pair", "field top macroblock under a frame pair", "field bottom macroblock under a frame pair", "field bottom macroblock under a field pair"]
    need += ["top edge: %s, %s" % (t, w) for t in tops for w in ("intra", "inter")]
    need += ["top edge: first pair row, %s %s" % (k, p) for k in kinds for p in ("top", "bottom") if not (k == "frame" and p == "bottom")]
    need += ["top edge suppressed at a slice boundary (FILTER_OWN_SLICE): %s" % t for t in tops[1:]]
    need += ["NO_DEBLOCK macroblock to the right of a filtered one (rare)", "filtered macroblock to the right of a NO_DEBLOCK one (rare)"]
    need += ["vertical vector difference 2..3 across an inner edge, %s macroblock" % k for k in kinds]
    need += ["8x8 transform in a field macroblock", "weighted field macroblock", "constrained intra: field macroblock with half a left edge (rare)"]
    need += ["field macroblock predicting from the %s-parity field" % p for p in ("same", "opposite")]
    for k in kinds:
        need += ["Intra 4x4 mode %d, %s" % (i, k) for i in range(9)] + ["Intra 8x8 mode %d, %s" % (i, k) for i in range(9)]
        need += ["Intra 16x16 mode %d, %s" % (i, k) for i in range(4)] + ["chroma mode %d, %s" % (i, k) for i in range(4)]
        need += ["Intra 8x8 with the above-left sample, %s" % k, "bypass: a pair picture, %s macroblock" % k]
        need += ["above-left from the left pair: frame bottom, left pair %s" % k]
        need += ["above-left from pair D: %s %s, left pair %s, pair D %s (rare)" % (cur, p, k, dk) for cur, p in (("frame", "top"), ("field", "top"), ("field", "bottom")) for dk in kinds]
    need += ["skip: top skipped, bottom coded", "skip: pair with the flag inferred from A (frame)", "skip: pair with the flag inferred from A (field)",
             "skip: pair with the flag inferred from B (field) (rare)", "skip: pair with the flag inferred from B (frame) (rare)", "skip: pair defaulted to frame"]
    need += ["bypass: Intra 8x8, %s" % t for t in ("BYPASS alone", "BYPASS + PRED", "BYPASS + PRED + X264OLD", "BYPASS + X264OLD (no PRED)")]
    need += ["bypass: neither flag", "bypass: I_PCM in a bypass picture", "bypass: X264OLD Intra 8x8 block vertical", "bypass: X264OLD Intra 8x8 block horizontal"]
    # Intra 8x8 (one intra macroblock in four or five) x profile 244 outside 4:4:4 x one chroma mode of four: rare
    need += ["bypass: X264OLD Intra 8x8 macroblock with chroma mode %s (rare)" % k for k in ("vertical", "horizontal")]
    bands = ("low (0..15)", "middle (16..44)", "high (45..51)")
    need += ["QP: filtered macroblock, luma QP %s" % b for b in bands] + ["QP: filtered macroblock, luma QP %s, %s QP %s" % (b, p, w) for b in bands for p, w in (("Cb", "moved by its offset"), ("Cr", "moved by its offset"), ("Cr", "as without an offset"))]
    need += ["QP: left edge, average luma QP %s" % b for b in bands] + ["QP: pair picture whose filtered macroblocks span two or three QP bands"]
    need += ["QP: filtered macroblock with a Cb QP offset of %d" % o for o in (2, -4, 6)] + ["QP: filtered macroblock with a Cr QP offset of %d" % o for o in (-3, 5, 0)]
    missing = ["%s: %d" % (k, c[k]) for k in need if c[k] < (5 if "(rare)" in k else 20)]
    # geometry and formats: present at all
    missing += [k for k in ["width %d" % w for w in (2, 3, 5, 9)] + ["pair rows %d" % r for r in (1, 2, 3, 5)] if not c[k]]
    missing += ["format %d/%d, %s pictures" % (i, b, t) for i, b in ((1, 8), (1, 9), (1, 10), (2, 8), (2, 10), (3, 8), (3, 10)) for t in "IPB"
                if not c["chroma_format_idc %d, %d bit, %s picture" % (i, b, t)]]
    # the loop filter had work on edges of every class and none on others
    missing += ["%s: changed %d, unchanged %d" % (k, v[0], v[1]) for k, v in sorted(touched.items()) if not (v[0] and v[1])]
    assert not missing, "the tables do not reach:\n  " + "\n  ".join(missing)


def test_loop_filter_has_work_in_every_stream(table):
    """per stream the reference's loop filter changed between 2 % and 90 % of the luma samples — unless the stream switches it off throughout (disable_deblocking_filter_idc 1)
    or is lossless.  The lossless entries are held to exactly 0 % instead: at QP' 0 alpha and beta are 0, so no edge can pass the filter's sample test and the
    2 % floor cannot be met by any lossless content"""
    bad = []
    for name, t in table.items():
        share = float((t["on"] != t["off"]).mean())
        print("%-40s %5.1f %% of the luma samples changed by the loop filter" % (name, 100 * share))
        e = PT.TABLE[name]
        if e["deblock_idc"] == 1 or e.get("lossless"):
            assert share == 0.0, name
        elif not 0.02 <= share <= 0.90:
            bad.append("%s: %.1f %%" % (name, 100 * share))
    assert not bad, bad
