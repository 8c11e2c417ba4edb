"""Stream tables for the second H.264 kernel set's macroblock-PAIR (MBAFF) and transform-bypass paths (libav_amd/csrc/h264_frame_wide.hip: k_wide_deblock_mbaff,
the field-macroblock branches of k_wide_inter / k_wide_intra, the MI355_MBF_BYPASS* branches).  name -> parameters of the stream writer
(tests/golden/make_h264_streams.py); the streams are committed as tests/golden/h264_pairs_<name>.samples, and what the reference's own decoder makes of them
(oracle/_ref/h264_bridge_emu with MI355_BRIDGE_PLAIN, loop filter on and off) as tests/golden/h264_pair_tables_md5.json — both written by
tests/golden/make_h264_pair_tables.py.  run_entry() decodes an entry twice with one binary — bridge stepped aside / bridge active — and compares the pictures
sample by sample; tests/test_h264_pair_content.py (the census) shows from the records the bridge hands to the kernels that the table reaches what it is for.

What the writer's new parameters add over the h264_synth_*_mbaff* streams: pair_skips (P_Skip / B_Skip in pairs: top skipped and bottom coded, both skipped with the
field flag inferred from pair A, from pair B, or defaulted to frame), above_left (neighbour D of 6.4.12.2: Intra 4x4 / 8x8 modes 4, 5, 6, plane prediction, the
above-left sample of the Intra 8x8 edge filter), qp_walk (mb_qp_delta walks a QP range: the two macroblocks of a left pair differ, one picture spans the alpha / beta /
tc0 tables), x264_build (user-data SEI: MI355_MBF_BYPASS_X264OLD when below 151), and transform bypass in pair pictures.

Pictures two macroblocks wide: the bridge leaves 4:2:0 / 4:2:2 ones to the reference (its bi-prediction scratch rows overlap there, the quirk of 420_8_2wide_b), so the
two-wide entry is 4:4:4.  One macroblock wide stays out: the reference is not self-consistent there.

Census counts observed when the table was recorded (tests/test_h264_pair_content.py prints them; minimum 20, or 5 where the test marks the class (rare)): see
CENSUS_RECORDED at the end of this module."""
import hashlib
import json
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

_P = dict(mbaff=True, pair_skips=True, above_left=True)
# geometry: mb_w x mb_h macroblocks (mb_h = 2 x pair rows)
PAIRS = {
    # widths 2 (4:4:4), 3, 5, 9; pair rows 1, 2, 3, 5
    "444_8_w2_r3_p": dict(_P, mb_w=2, mb_h=6, chroma_idc=3, depth=8, seed=201, nslices=2, deblock_idc=0, nrefs=2, npics=6, qp_walk=(18, 44)),
    "420_8_w3_r1_p_ref1": dict(_P, mb_w=3, mb_h=2, chroma_idc=1, depth=8, seed=202, nslices=1, deblock_idc=0, nrefs=1, npics=8, qp_walk=(20, 40), t8x8=True),
    "420_8_w5_r2_b_implicit_skips": dict(_P, mb_w=5, mb_h=4, chroma_idc=1, depth=8, seed=203, nslices=2, deblock_idc=2, nrefs=2, npics=15, bmode=1, skip=0.5, qp_walk=(24, 46)),
    "420_8_w9_r5_b_explicit": dict(_P, mb_w=9, mb_h=10, chroma_idc=1, depth=8, seed=204, nslices=5, deblock_idc=-1, nrefs=4, npics=7, bmode=2, far=24, t8x8=True, npps=3,
                                   qp_walk=(10, 51)),
    "420_8_w5_r3_p_own_slice_cip": dict(_P, mb_w=5, mb_h=6, chroma_idc=1, depth=8, seed=205, nslices=4, deblock_idc=2, nrefs=3, npics=8, cip=True, t8x8=True, far=24,
                                        qp_walk=(28, 51), npps=2),
    "420_8_w5_r3_p_skips_high": dict(_P, mb_w=5, mb_h=6, chroma_idc=1, depth=8, seed=206, nslices=2, deblock_idc=0, nrefs=2, npics=16, skip=0.7, qp_walk=(30, 48), weighted=False),
    "420_8_w3_r2_p_nofilter": dict(_P, mb_w=3, mb_h=4, chroma_idc=1, depth=8, seed=207, nslices=2, deblock_idc=1, nrefs=2, npics=6, qp_walk=(20, 44)),
    "420_8_w5_r2_p_lowqp": dict(_P, mb_w=5, mb_h=4, chroma_idc=1, depth=8, seed=208, nslices=1, deblock_idc=0, nrefs=2, npics=6, qp_walk=(4, 28), npps=3),
    "420_9_w3_r2_b_average": dict(_P, mb_w=3, mb_h=4, chroma_idc=1, depth=9, seed=209, nslices=2, deblock_idc=-1, nrefs=2, npics=7, bmode=3, weighted=False, qp_walk=(14, 45)),
    "420_10_w5_r3_b_cip": dict(_P, mb_w=5, mb_h=6, chroma_idc=1, depth=10, seed=210, nslices=3, deblock_idc=2, nrefs=2, npics=7, bmode=1, cip=True, t8x8=True, qp_walk=(-12, 26)),
    "420_10_w3_r2_p_high": dict(_P, mb_w=3, mb_h=4, chroma_idc=1, depth=10, seed=211, nslices=1, deblock_idc=0, nrefs=2, npics=6, qp_walk=(45, 51), far=24),
    "422_8_w3_r2_p": dict(_P, mb_w=3, mb_h=4, chroma_idc=2, depth=8, seed=212, nslices=2, deblock_idc=-1, nrefs=2, npics=6, qp_walk=(16, 51), cip=True),
    "422_8_w5_r1_b_implicit": dict(_P, mb_w=5, mb_h=2, chroma_idc=2, depth=8, seed=213, nslices=1, deblock_idc=0, nrefs=2, npics=15, bmode=1, skip=0.5, qp_walk=(26, 50)),
    "422_10_w3_r3_b_explicit": dict(_P, mb_w=3, mb_h=6, chroma_idc=2, depth=10, seed=214, nslices=3, deblock_idc=2, nrefs=3, npics=7, bmode=2, t8x8=True, qp_walk=(20, 51), npps=2),
    "444_8_w5_r2_b_cip": dict(_P, mb_w=5, mb_h=4, chroma_idc=3, depth=8, seed=215, nslices=3, deblock_idc=2, nrefs=2, npics=7, bmode=1, cip=True, qp_walk=(22, 51)),
    "444_10_w3_r2_p": dict(_P, mb_w=3, mb_h=4, chroma_idc=3, depth=10, seed=216, nslices=2, deblock_idc=0, nrefs=2, npics=6, t8x8=True, qp_walk=(10, 48)),
    "444_10_w5_r2_b_explicit": dict(_P, mb_w=5, mb_h=4, chroma_idc=3, depth=10, seed=217, nslices=2, deblock_idc=-1, nrefs=2, npics=7, bmode=2, skip=0.5, qp_walk=(24, 51)),
    # intra-heavy content for the above-left neighbour and the Intra 8x8 / 16x16 modes: few skips, pictures 0 and 4 all intra
    "420_8_w5_r3_p_intra_t8x8": dict(_P, mb_w=5, mb_h=6, chroma_idc=1, depth=8, seed=218, nslices=1, deblock_idc=0, nrefs=2, npics=24, t8x8=True, skip=0.05, qp_walk=(22, 42)),
    "422_8_w5_r2_p_intra_t8x8": dict(_P, mb_w=5, mb_h=4, chroma_idc=2, depth=8, seed=219, nslices=2, deblock_idc=2, nrefs=2, npics=24, t8x8=True, skip=0.05, qp_walk=(24, 44)),
    "420_10_w5_r2_p_intra_t8x8": dict(_P, mb_w=5, mb_h=4, chroma_idc=1, depth=10, seed=220, nslices=1, deblock_idc=0, nrefs=2, npics=24, t8x8=True, skip=0.05, qp_walk=(16, 40)),
    "444_8_w5_r2_p_intra": dict(_P, mb_w=5, mb_h=4, chroma_idc=3, depth=8, seed=231, nslices=1, deblock_idc=0, nrefs=2, npics=32, skip=0.05, qp_walk=(22, 44)),
}
_L = dict(weighted=False, lossless=True, deblock_idc=0, nrefs=2)
BYPASS = {
    # transform bypass: x264_build absent / 150 (MI355_MBF_BYPASS_X264OLD) / 151 (the boundary: not set); profile 244 = MI355_MBF_BYPASS_PRED
    "ll_420_8_w4_r3": dict(_L, mb_w=4, mb_h=3, chroma_idc=1, depth=8, seed=221, nslices=2, npics=14),
    "ll_420_8_w4_r3_t8x8_x150": dict(_L, mb_w=4, mb_h=3, chroma_idc=1, depth=8, seed=222, nslices=1, npics=28, t8x8=True, x264_build=150),
    "ll_420_8_w4_r3_t8x8_x151": dict(_L, mb_w=4, mb_h=3, chroma_idc=1, depth=8, seed=222, nslices=1, npics=28, t8x8=True, x264_build=151),
    "ll_422_10_w3_r4_t8x8_x150": dict(_L, mb_w=3, mb_h=4, chroma_idc=2, depth=10, seed=223, nslices=2, npics=28, t8x8=True, x264_build=150),
    "ll_444_8_w4_r3_t8x8": dict(_L, mb_w=4, mb_h=3, chroma_idc=3, depth=8, seed=224, nslices=1, npics=14, t8x8=True),
    "ll_444_8_w3_r3_t8x8_x150": dict(_L, mb_w=3, mb_h=3, chroma_idc=3, depth=8, seed=225, nslices=2, npics=28, t8x8=True, x264_build=150),
    "ll_444_8_w3_r3_t8x8_x151": dict(_L, mb_w=3, mb_h=3, chroma_idc=3, depth=8, seed=225, nslices=2, npics=28, t8x8=True, x264_build=151),      # same content: other pictures
    "ll_444_10_w3_r4_t8x8_x150": dict(_L, mb_w=3, mb_h=4, chroma_idc=3, depth=10, seed=226, nslices=1, npics=28, t8x8=True, x264_build=150),
    "ll_444_10_w3_r3": dict(_L, mb_w=3, mb_h=3, chroma_idc=3, depth=10, seed=227, nslices=1, npics=14),
    "ll_444_8_w5_r4_t8x8_x100": dict(_L, mb_w=5, mb_h=4, chroma_idc=3, depth=8, seed=229, nslices=1, npics=32, t8x8=True, x264_build=100),
    "ll_422_8_w4_r3_t8x8": dict(_L, mb_w=4, mb_h=3, chroma_idc=2, depth=8, seed=230, nslices=2, npics=20, t8x8=True),
    # profile 244 with 4:2:0 / 4:2:2: MI355_MBF_BYPASS_PRED (and X264OLD) on macroblocks that have a chroma prediction mode, vertical and horizontal among them
    "ll_420_8_w5_r4_t8x8_p244_x150": dict(_L, mb_w=5, mb_h=4, chroma_idc=1, depth=8, seed=232, nslices=1, npics=32, t8x8=True, x264_build=150, profile=244),
    "ll_422_10_w4_r4_t8x8_p244_x150": dict(_L, mb_w=4, mb_h=4, chroma_idc=2, depth=10, seed=233, nslices=2, npics=32, t8x8=True, x264_build=150, profile=244),
    # the two paths meet in k_wide_intra: a lossless pair picture
    "ll_420_8_w3_r2_pairs_t8x8_x150": dict(_L, mbaff=True, above_left=True, pair_skips=True, mb_w=3, mb_h=4, chroma_idc=1, depth=8, seed=228, nslices=1, npics=14, t8x8=True,
                                           x264_build=150),
}
TABLE = dict(PAIRS, **BYPASS)
NAMES = sorted(TABLE)
# the lazy / three-thread mode on the CPU emulator: one entry per format class and the largest picture (the GPU test runs every entry in both modes)
EMU_LAZY = ["420_8_w9_r5_b_explicit", "422_10_w3_r3_b_explicit", "444_8_w5_r2_b_cip", "ll_420_8_w3_r2_pairs_t8x8_x150"]

MD5_FILE = os.path.join(GOLD, "h264_pair_tables_md5.json")
MD5 = json.load(open(MD5_FILE)) if os.path.exists(MD5_FILE) else {}
# seconds one direct, filter-on decode of the entry took on the SIMT emulator when the table was recorded (MD5[name]["emu_seconds"]); every child process gets ten
# times that, at least 30 s (process start and the device runtime's start-up do not scale with the picture)
def limit(name, runs=1):
    return max(30.0, 10.0 * runs * MD5.get(name, {}).get("emu_seconds", 3.0))


def samples(name):
    return os.path.join(GOLD, "h264_pairs_%s.samples" % name)


def exe(which):
    return os.path.join(ROOT, "oracle", "_ref", which)


def geometry(name):
    """planes of one output picture: [(name, height, width)], bytes per sample"""
    e = TABLE[name]
    w, h, idc = 16 * e["mb_w"], 16 * e["mb_h"], e["chroma_idc"]
    cw, ch = (w, h) if idc == 3 else (w // 2, h if idc == 2 else h // 2)
    return [("Y", h, w), ("Cb", ch, cw), ("Cr", ch, cw)], 2 if e["depth"] > 8 else 1


def decode_order(name):
    """output picture index -> index in decoding order (the writer's build_b: I0 P4 b2 P8 b6 ..., picture order counts)"""
    e = TABLE[name]
    if not e.get("bmode"):
        return list(range(e["npics"]))
    pocs, k = [0], 1
    while len(pocs) < e["npics"]:
        pocs.append(4 * k)
        if len(pocs) < e["npics"]:
            pocs.append(4 * k - 2)
        k += 1
    return sorted(range(len(pocs)), key=lambda i: pocs[i])


def load_pictures(path, name):
    planes, bps = geometry(name)
    raw = np.fromfile(str(path), np.uint16 if bps == 2 else np.uint8)
    per = sum(h * w for _, h, w in planes)
    assert raw.size == per * TABLE[name]["npics"], (name, raw.size, per)
    raw = raw.reshape(-1, per)
    out, o = [], 0
    for _, h, w in planes:
        out.append(raw[:, o:o + h * w].reshape(-1, h, w))
        o += h * w
    return out


def run(which, name, out, plain=False, nofilter=False, lazy=False, threads=1, debug=None, runs=1):
    """one child process of oracle/_ref/<which>; a clean environment for every switch the harness reads (as synth_streams.run_bridge)"""
    env = dict(os.environ)
    for k in ("MI355_BRIDGE_LAZY", "MI355_BRIDGE_DIRECT", "MI355_BRIDGE_PLAIN", "MI355_BRIDGE_SESSION", "MI355_BRIDGE_LINEAR", "MI355_BRIDGE_NO_WIDE", "MI355_BRIDGE_DEBUG",
              "MI355_HARNESS_SKIP_LOOP_FILTER", "MI355_BRIDGE_KEEP_FIELD_IDC2"):
        env.pop(k, None)
    if plain:
        env["MI355_BRIDGE_PLAIN"] = "1"
    elif lazy:
        env["MI355_BRIDGE_LAZY"] = "1"
    else:
        env["MI355_BRIDGE_DIRECT"] = "1"
    if nofilter:
        env["MI355_HARNESS_SKIP_LOOP_FILTER"] = "1"
    if debug:
        env["MI355_BRIDGE_DEBUG"] = str(debug)
    try:
        r = subprocess.run([exe(which), samples(name), str(out), str(threads), "1"], capture_output=True, text=True, env=env, timeout=limit(name, runs))
    except subprocess.TimeoutExpired as e:
        raise AssertionError("%s %s: no result after %.0f s\n%s" % (which, name, e.timeout, (e.stderr or b"")[-2000:]))
    assert r.returncode == 0, "%s %s ended with %d%s\n%s" % (which, name, r.returncode, " (a signal)" if r.returncode < 0 else "", r.stderr[-2000:])
    stats = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert stats, r.stdout[-500:] + r.stderr[-2000:]
    stats[-1]["stderr"] = r.stderr
    return stats[-1]


def check_md5(path, name, key):
    raw = open(str(path), "rb").read()
    assert len(raw) == MD5[name]["bytes"], (name, len(raw), MD5[name]["bytes"])
    assert hashlib.md5(raw).hexdigest() == MD5[name][key], "%s: the plain decode is not what the reference decoder gave when the table was recorded (%s)" % (name, key)


def parse_dump(path):
    """the bridge's record dump (MI355_BRIDGE_DEBUG=<file>, contrib/libav/mi355_h264_bridge.c) -> a list of pictures in decoding order:
    dict(mbaff, mb_w, rows, depth, idc, mbs = {(x, y): dict})"""
    pics = []
    for line in open(str(path)):
        t = line.split()
        if not t:
            continue
        if t[0] == "P":                                      # t[1], the bridge's own picture count, is not used: the pictures are taken in the order of the lines
            pics.append(dict(mbaff=int(t[2]), mb_w=int(t[3]), rows=int(t[4]), depth=int(t[5]), idc=int(t[6]), mbs={}))
        elif t[0] == "M":
            v = [int(x) for x in t[1:13]]
            m = dict(x=v[0], y=v[1], mb_type=v[2], flags=v[3], slice_id=v[4], qp=v[5], qpc=(v[6], v[7]), cbp=v[8], i16=v[9], cmode=v[10], topleft=v[11])
            rest = t[13:]
            if m["mb_type"] & 7:
                m["modes"] = [int(x) for x in rest[:16]]
            else:
                m["lists"] = {}
                while rest:
                    assert rest[0] == "L"
                    n = [int(x) for x in rest[1:46]]
                    m["lists"][n[0]] = dict(ref_idx=n[1:5], ref_pic=n[5:9], chroma_dy=n[9:13], mv=np.array(n[13:45]).reshape(4, 4, 2))      # mv[y4][x4] = (x, y)
                    rest = rest[46:]
            pics[-1]["mbs"][(m["x"], m["y"])] = m
    return pics


def first_difference(name, ref, got, records=None):
    """names the first picture / plane / macroblock at which two decodes differ; records: parse_dump() of the same stream (frame or field coding of that macroblock)"""
    planes, _ = geometry(name)
    e = TABLE[name]
    for f in range(ref[0].shape[0]):
        for p, (pname, h, w) in enumerate(planes):
            d = ref[p][f] != got[p][f]
            if not d.any():
                continue
            mh, mw = h // e["mb_h"], w // e["mb_w"]
            ys, xs = np.nonzero(d)
            my, mx = int(ys[0]) // mh, int(xs[0]) // mw
            kind = ""
            if records is not None:
                mbs = records[decode_order(name)[f]]["mbs"]
                if records[decode_order(name)[f]]["mbaff"] and mbs[(mx, my & ~1)]["mb_type"] & 0x80:
                    my = (my & ~1) | (int(ys[0]) & 1)          # a pair of field macroblocks: the top one owns the even lines
                m = mbs.get((mx, my))
                kind = ", a %s macroblock (mb_type 0x%x, flags 0x%x)" % ("FIELD" if m["mb_type"] & 0x80 else "frame", m["mb_type"], m["flags"]) if m else ""
            nmb = len(set(zip((ys // mh).tolist(), (xs // mw).tolist())))
            return ("%s: output picture %d (decoding order %d), plane %s, macroblock x %d of pair row %d (%s of the pair, macroblock row %d)%s: first of %d differing samples "
                    "in %d macroblocks of this plane, at line %d column %d: %d for the reference's %d"
                    % (name, f, decode_order(name)[f], pname, mx, my // 2, "bottom" if my & 1 else "top", my, kind, int(d.sum()), nmb, int(ys[0]), int(xs[0]),
                       int(got[p][f][ys[0], xs[0]]), int(ref[p][f][ys[0], xs[0]])))
    return None


def run_entry(which, name, tmp, lazy=False, nofilter=False):
    """the entry through oracle/_ref/<which> twice — bridge stepped aside, bridge active (direct with one decoder thread, or lazy with three: batches of several pictures) —
    the plain pictures pinned by the recorded md5, the two compared sample by sample, every picture decoded on the device"""
    tmp = str(tmp)
    plain, dev = os.path.join(tmp, "plain.yuv"), os.path.join(tmp, "device.yuv")
    st = run(which, name, plain, plain=True, nofilter=nofilter)
    assert st["pictures_on_device"] == 0 and st["pictures_output"] == TABLE[name]["npics"], st
    check_md5(plain, name, "md5_nofilter" if nofilter else "md5")
    threads = 3 if lazy else 1
    st = run(which, name, dev, lazy=lazy, threads=threads, nofilter=nofilter, runs=threads)
    a, b = load_pictures(plain, name), load_pictures(dev, name)
    if any(not np.array_equal(x, y) for x, y in zip(a, b)):
        records = None
        if os.path.exists(exe("h264_bridge_emu")):               # which macroblocks are field coded: the records of a run on the CPU emulator
            dump = os.path.join(tmp, "records.txt")
            run("h264_bridge_emu", name, "-", nofilter=nofilter, debug=dump)
            records = parse_dump(dump)
        raise AssertionError(first_difference(name, a, b, records) + (" [loop filter off: the reconstruction differs]" if nofilter else ""))
    assert st["pictures_on_device"] == threads * TABLE[name]["npics"], st


def build_stream(T, name):
    """the entry's access units (tests/golden/make_h264_pair_tables.py: T = the writer's code tables)"""
    import sys
    sys.path.insert(0, GOLD)
    import make_h264_streams as W
    k = dict(TABLE[name])
    return (W.MbaffStream if k.pop("mbaff", False) else W.Stream)(T, name, **k).build()


CENSUS_RECORDED = """
   302  8x8 transform in a field macroblock
   235  Intra 16x16 mode 0, field
   206  Intra 16x16 mode 0, frame
   123  Intra 16x16 mode 1, field
   112  Intra 16x16 mode 1, frame
    39  Intra 16x16 mode 2, field
   107  Intra 16x16 mode 2, frame
    43  Intra 16x16 mode 3, field
    52  Intra 16x16 mode 3, frame
   364  Intra 4x4 mode 0, field
   477  Intra 4x4 mode 0, frame
   443  Intra 4x4 mode 1, field
   458  Intra 4x4 mode 1, frame
   583  Intra 4x4 mode 2, field
   611  Intra 4x4 mode 2, frame
   375  Intra 4x4 mode 3, field
   452  Intra 4x4 mode 3, frame
   313  Intra 4x4 mode 4, field
   404  Intra 4x4 mode 4, frame
   326  Intra 4x4 mode 5, field
   372  Intra 4x4 mode 5, frame
   312  Intra 4x4 mode 6, field
   381  Intra 4x4 mode 6, frame
   379  Intra 4x4 mode 7, field
   451  Intra 4x4 mode 7, frame
   473  Intra 4x4 mode 8, field
   474  Intra 4x4 mode 8, frame
    40  Intra 8x8 mode 0, field
    47  Intra 8x8 mode 0, frame
    70  Intra 8x8 mode 1, field
    36  Intra 8x8 mode 1, frame
    97  Intra 8x8 mode 2, field
    86  Intra 8x8 mode 2, frame
    41  Intra 8x8 mode 3, field
    49  Intra 8x8 mode 3, frame
    37  Intra 8x8 mode 4, field
    42  Intra 8x8 mode 4, frame
    26  Intra 8x8 mode 5, field
    31  Intra 8x8 mode 5, frame
    20  Intra 8x8 mode 6, field
    41  Intra 8x8 mode 6, frame
    51  Intra 8x8 mode 7, field
    56  Intra 8x8 mode 7, frame
    74  Intra 8x8 mode 8, field
    56  Intra 8x8 mode 8, frame
    35  Intra 8x8 with the above-left sample, field
    63  Intra 8x8 with the above-left sample, frame
    16  NO_DEBLOCK macroblock to the right of a filtered one (rare)
    65  QP: filtered macroblock with a Cb QP offset of -4
   937  QP: filtered macroblock with a Cb QP offset of 2
   131  QP: filtered macroblock with a Cb QP offset of 6
  1385  QP: filtered macroblock with a Cr QP offset of -3
   164  QP: filtered macroblock with a Cr QP offset of 0
    73  QP: filtered macroblock with a Cr QP offset of 5
   601  QP: filtered macroblock, luma QP high (45..51)
   314  QP: filtered macroblock, luma QP high (45..51), Cb QP as without an offset
   287  QP: filtered macroblock, luma QP high (45..51), Cb QP moved by its offset
   183  QP: filtered macroblock, luma QP high (45..51), Cr QP as without an offset
   418  QP: filtered macroblock, luma QP high (45..51), Cr QP moved by its offset
   464  QP: filtered macroblock, luma QP low (0..15)
     9  QP: filtered macroblock, luma QP low (0..15), Cb QP as without an offset
   455  QP: filtered macroblock, luma QP low (0..15), Cb QP moved by its offset
   222  QP: filtered macroblock, luma QP low (0..15), Cr QP as without an offset
   242  QP: filtered macroblock, luma QP low (0..15), Cr QP moved by its offset
  4043  QP: filtered macroblock, luma QP middle (16..44)
   189  QP: filtered macroblock, luma QP middle (16..44), Cb QP as without an offset
  3854  QP: filtered macroblock, luma QP middle (16..44), Cb QP moved by its offset
   134  QP: filtered macroblock, luma QP middle (16..44), Cr QP as without an offset
  3909  QP: filtered macroblock, luma QP middle (16..44), Cr QP moved by its offset
   430  QP: left edge, average luma QP high (45..51)
   322  QP: left edge, average luma QP low (0..15)
  3084  QP: left edge, average luma QP middle (16..44)
   128  QP: pair picture whose filtered macroblocks span two or three QP bands
    15  above-left from pair D: field bottom, left pair field, pair D field (rare)
    11  above-left from pair D: field bottom, left pair field, pair D frame (rare)
    13  above-left from pair D: field bottom, left pair frame, pair D field (rare)
    15  above-left from pair D: field bottom, left pair frame, pair D frame (rare)
    12  above-left from pair D: field top, left pair field, pair D field (rare)
    17  above-left from pair D: field top, left pair field, pair D frame (rare)
    16  above-left from pair D: field top, left pair frame, pair D field (rare)
    16  above-left from pair D: field top, left pair frame, pair D frame (rare)
    12  above-left from pair D: frame top, left pair field, pair D field (rare)
    16  above-left from pair D: frame top, left pair field, pair D frame (rare)
    17  above-left from pair D: frame top, left pair frame, pair D field (rare)
    16  above-left from pair D: frame top, left pair frame, pair D frame (rare)
    66  above-left from the left pair: frame bottom, left pair field
    43  above-left from the left pair: frame bottom, left pair frame
   117  bypass: I_PCM in a bypass picture
    30  bypass: Intra 8x8, BYPASS + PRED
   120  bypass: Intra 8x8, BYPASS + PRED + X264OLD
    29  bypass: Intra 8x8, BYPASS + X264OLD (no PRED)
    32  bypass: Intra 8x8, BYPASS alone
    68  bypass: X264OLD Intra 8x8 block horizontal
    68  bypass: X264OLD Intra 8x8 block vertical
    17  bypass: X264OLD Intra 8x8 macroblock with chroma mode horizontal (rare)
    11  bypass: X264OLD Intra 8x8 macroblock with chroma mode vertical (rare)
    86  bypass: a pair picture, field macroblock
    82  bypass: a pair picture, frame macroblock
  5348  bypass: neither flag
   331  chroma mode 0, field
   312  chroma mode 0, frame
   162  chroma mode 1, field
   137  chroma mode 1, frame
    76  chroma mode 2, field
   149  chroma mode 2, frame
    46  chroma mode 3, field
    80  chroma mode 3, frame
    37  chroma_format_idc 1, 10 bit
     3  chroma_format_idc 1, 10 bit, B picture
     5  chroma_format_idc 1, 10 bit, I picture
    29  chroma_format_idc 1, 10 bit, P picture
   206  chroma_format_idc 1, 8 bit
    10  chroma_format_idc 1, 8 bit, B picture
    24  chroma_format_idc 1, 8 bit, I picture
   172  chroma_format_idc 1, 8 bit, P picture
     7  chroma_format_idc 1, 9 bit
     3  chroma_format_idc 1, 9 bit, B picture
     1  chroma_format_idc 1, 9 bit, I picture
     3  chroma_format_idc 1, 9 bit, P picture
    67  chroma_format_idc 2, 10 bit
     3  chroma_format_idc 2, 10 bit, B picture
     5  chroma_format_idc 2, 10 bit, I picture
    59  chroma_format_idc 2, 10 bit, P picture
    65  chroma_format_idc 2, 8 bit
     7  chroma_format_idc 2, 8 bit, B picture
     7  chroma_format_idc 2, 8 bit, I picture
    51  chroma_format_idc 2, 8 bit, P picture
    55  chroma_format_idc 3, 10 bit
     3  chroma_format_idc 3, 10 bit, B picture
     7  chroma_format_idc 3, 10 bit, I picture
    45  chroma_format_idc 3, 10 bit, P picture
   147  chroma_format_idc 3, 8 bit
     3  chroma_format_idc 3, 8 bit, B picture
    13  chroma_format_idc 3, 8 bit, I picture
   131  chroma_format_idc 3, 8 bit, P picture
    10  constrained intra: field macroblock with half a left edge (rare)
  2510  field macroblock predicting from the opposite-parity field
  5310  field macroblock predicting from the same-parity field
    14  filtered macroblock to the right of a NO_DEBLOCK one (rare)
  1010  left edge inside a slice: field beside field
   876  left edge inside a slice: field beside frame
   860  left edge inside a slice: frame beside field
  1134  left edge inside a slice: frame beside frame
   404  left edge of a mixed pair with two left QPs: field beside frame
   416  left edge of a mixed pair with two left QPs: frame beside field
    46  left edge suppressed at a slice boundary (FILTER_OWN_SLICE): field beside field
    48  left edge suppressed at a slice boundary (FILTER_OWN_SLICE): field beside frame
    72  left edge suppressed at a slice boundary (FILTER_OWN_SLICE): frame beside field
    54  left edge suppressed at a slice boundary (FILTER_OWN_SLICE): frame beside frame
   480  left edge: field beside a field pair, inter
   542  left edge: field beside a field pair, intra on either side
   346  left edge: field beside a frame pair, inter
   552  left edge: field beside a frame pair, intra on either side
   328  left edge: frame beside a field pair, inter
   546  left edge: frame beside a field pair, intra on either side
   531  left edge: frame beside a frame pair, inter
   623  left edge: frame beside a frame pair, intra on either side
    23  pair rows 1
   160  pair rows 2
    68  pair rows 3
     7  pair rows 5
    44  skip: pair defaulted to frame
   102  skip: pair with the flag inferred from A (field)
   126  skip: pair with the flag inferred from A (frame)
     6  skip: pair with the flag inferred from B (field) (rare)
     9  skip: pair with the flag inferred from B (frame) (rare)
   165  skip: top skipped, bottom coded
    69  top edge suppressed at a slice boundary (FILTER_OWN_SLICE): field bottom macroblock under a field pair
   103  top edge suppressed at a slice boundary (FILTER_OWN_SLICE): field bottom macroblock under a frame pair
    69  top edge suppressed at a slice boundary (FILTER_OWN_SLICE): field top macroblock under a field pair
   103  top edge suppressed at a slice boundary (FILTER_OWN_SLICE): field top macroblock under a frame pair
    81  top edge suppressed at a slice boundary (FILTER_OWN_SLICE): frame top macroblock under a field pair (filtered twice)
   100  top edge suppressed at a slice boundary (FILTER_OWN_SLICE): frame top macroblock under a frame pair
   169  top edge: field bottom macroblock under a field pair, inter
   115  top edge: field bottom macroblock under a field pair, intra
   144  top edge: field bottom macroblock under a frame pair, inter
   126  top edge: field bottom macroblock under a frame pair, intra
   151  top edge: field top macroblock under a field pair, inter
   133  top edge: field top macroblock under a field pair, intra
   147  top edge: field top macroblock under a frame pair, inter
   123  top edge: field top macroblock under a frame pair, intra
   544  top edge: first pair row, field bottom
   544  top edge: first pair row, field top
   583  top edge: first pair row, frame top
   732  top edge: frame bottom macroblock (its own pair's top), inter
   636  top edge: frame bottom macroblock (its own pair's top), intra
   155  top edge: frame top macroblock under a field pair (filtered twice), inter
   141  top edge: frame top macroblock under a field pair (filtered twice), intra
   166  top edge: frame top macroblock under a frame pair, inter
   142  top edge: frame top macroblock under a frame pair, intra
   225  vertical vector difference 2..3 across an inner edge, field macroblock
   208  vertical vector difference 2..3 across an inner edge, frame macroblock
  1499  weighted field macroblock
     1  width 2
    13  width 3
     6  width 4
    14  width 5
     1  width 9
   423 changed     57 unchanged  left edge: field beside a field pair, inter
   467 changed     75 unchanged  left edge: field beside a field pair, intra on either side
   315 changed     31 unchanged  left edge: field beside a frame pair, inter
   500 changed     52 unchanged  left edge: field beside a frame pair, intra on either side
   295 changed     33 unchanged  left edge: frame beside a field pair, inter
   496 changed     50 unchanged  left edge: frame beside a field pair, intra on either side
   480 changed     51 unchanged  left edge: frame beside a frame pair, inter
   533 changed     90 unchanged  left edge: frame beside a frame pair, intra on either side
   146 changed     23 unchanged  top edge: field bottom macroblock under a field pair, inter
   101 changed     14 unchanged  top edge: field bottom macroblock under a field pair, intra
   128 changed     16 unchanged  top edge: field bottom macroblock under a frame pair, inter
   114 changed     12 unchanged  top edge: field bottom macroblock under a frame pair, intra
   133 changed     18 unchanged  top edge: field top macroblock under a field pair, inter
   116 changed     17 unchanged  top edge: field top macroblock under a field pair, intra
   128 changed     19 unchanged  top edge: field top macroblock under a frame pair, inter
   107 changed     16 unchanged  top edge: field top macroblock under a frame pair, intra
   654 changed     78 unchanged  top edge: frame bottom macroblock (its own pair's top), inter
   560 changed     76 unchanged  top edge: frame bottom macroblock (its own pair's top), intra
   151 changed      4 unchanged  top edge: frame top macroblock under a field pair (filtered twice), inter
   130 changed     11 unchanged  top edge: frame top macroblock under a field pair (filtered twice), intra
   149 changed     17 unchanged  top edge: frame top macroblock under a frame pair, inter
   124 changed     18 unchanged  top edge: frame top macroblock under a frame pair, intra
"""
