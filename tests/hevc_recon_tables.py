"""Tables in place of draws for the HEVC reconstruction kernels (include/mi355_hevc_batch.h: motion compensation, prediction, transform units, the
coding-tree-block kernels): every block shape, every fraction, every col_limit the decoder's rule produces, and content that reaches the clips —
built by fixed rules, run in a few large launches through every entry point that executes these bodies, and compared with the oracle's
HEVCDSPContext called job by job on a host copy.  tests/test_hevc_recon_content.py proves on the CPU that the tables reach what they are for.

A Scene is a set of named host arrays plus job records whose pointers are (array name, byte offset): the oracle runs on copies of the arrays, the
device on uploads of them, and every byte of every array the device may write is compared afterwards (guard bands included)."""
import ctypes as C
import hashlib

import numpy as np

from cases_hevc import EW, QW
from hevc_batch import CtbJob, Dev, Level, McJob, McPredJob, PredJob, TuJob, _i16p, _u8p
from rng import SplitMix64

# the standard's interpolation filters (H.265 tables 8-11 / 8-12); the census checks them against the oracle's impulse responses
QPEL = np.array([[0, 0, 0, 64, 0, 0, 0, 0], [-1, 4, -10, 58, 17, -5, 1, 0], [-1, 4, -11, 40, 40, -11, 4, -1], [0, 1, -5, 17, 58, -10, 4, -1]], np.int64)
EPEL = np.array([[0, 64, 0, 0], [-2, 58, 10, -2], [-4, 54, 16, -2], [-6, 46, 28, -4], [-4, 36, 36, -4], [-4, 28, 46, -6], [-2, 16, 54, -4],
                 [-2, 10, 58, -2]], np.int64)
HL = [4, 8, 12, 16, 24, 32, 48, 64]          # luma heights
HC = [2, 4, 6, 8, 12, 16, 24, 32]            # chroma heights
MC_CLASSES = ("noise", "tap-max", "tap-min", "zero", "max")
SATURATING = ("tap-max", "tap-min", "zero", "max")
CELL, ORG = 80, 8                            # a job's reference window: CELL x CELL samples, the block's first sample at (ORG, ORG)
POISON = 0xA5


def taps_of(chroma, f):
    return (EPEL if chroma else QPEL)[f]


# ---------------------------------------------------------------------------------------------------------------- motion compensation rows

def mc_rows():
    """every (chroma, width index, mx, my); the height walks the list with (mx, my, width index), so that per width every height occurs"""
    rows = []
    for chroma in (0, 1):
        nf = 8 if chroma else 4
        for wi in range(8):
            for my in range(nf):
                for mx in range(nf):
                    h = (HC if chroma else HL)[(mx + (my if chroma else 4 * my) + wi) % 8]
                    w = (EW if chroma else QW)[wi]
                    rows.append(dict(chroma=chroma, wi=wi, w=w, h=h, mx=mx, my=my, name="%s w%d h%d mx%d my%d" % ("epel" if chroma else "qpel", w, h, mx, my)))
    return rows


def emu_keeps(job, cls):
    """the emulator's share of the motion / prediction table, over pred_jobs() records (check_mc_table hands its rows over in that shape): every job with
    noise; of the saturating classes tap-max / tap-min for every two-direction fraction (mx != 0 and my != 0: both filters' extremes multiply) and for the
    one-direction fractions 0, 1 and the largest, the constants where mx + my is a multiple of 4; the weighted kinds on the tap-max intermediates"""
    if cls == "noise":
        return True
    if job["kind"]:
        return job["kind"] == 1 or job["cls"][0] == "tap-max"
    mx, my = job["f"][0], job["f"][1]
    if mx and my:
        return cls in ("tap-max", "tap-min") or (mx + my) % 4 == 0
    return cls in ("tap-max", "tap-min") and max(mx, my) in (0, 1, 7 if job["chroma"] else 3)


def tap_signs(chroma, f):
    t = taps_of(chroma, f)
    return np.where(t < 0, -1, 1) if f else np.ones(len(t), np.int64)


def window(row, cls, bd, r, pad=0):
    """the CELL x (CELL + pad) reference window of one job.  tap-max: the maximum where the product of the row's horizontal and vertical taps is
    positive, 0 where it is negative, with the period of the filter and phased to the block's first sample (a direction without a fraction
    counts as positive everywhere); tap-min: the inverse"""
    top, cols = (1 << bd) - 1, CELL + pad
    if cls == "noise":
        a = r.randint(0, top, (CELL, cols))
    elif cls in ("zero", "max"):
        a = np.full((CELL, cols), top if cls == "max" else 0, np.int64)
    else:
        taps, before = (4, 1) if row["chroma"] else (8, 3)
        sh, sv = tap_signs(row["chroma"], row["mx"]), tap_signs(row["chroma"], row["my"])
        prod = sv[(np.arange(CELL) - ORG + before) % taps][:, None] * sh[(np.arange(cols) - ORG + before) % taps][None, :]
        a = np.where((prod > 0) == (cls == "tap-max"), top, 0)
    return a.astype(np.uint16 if bd > 8 else np.uint8)


def swapped(cls):
    return {"noise": "noise", "tap-max": "tap-min", "tap-min": "tap-max", "zero": "max", "max": "zero"}[cls]


def mc_windows(rows, cls, bd, pad=0, seed=1):
    r = SplitMix64(0x4D43 * 131 + bd * 7 + seed)
    return np.stack([window(row, cls, bd, r, pad) for row in rows])


def mc_expected(c, bd, rows, win):
    """the provider's put_hevc_qpel / put_hevc_epel row by row: (n, 64 * 64) int16, rows of 64"""
    px = 2 if bd > 8 else 1
    out = np.full((len(rows), 64 * 64), 0x2222, np.int16)
    mcbuf = np.zeros((64 + 24) * 64, np.int16)
    stride = win.strides[1]
    for k, row in enumerate(rows):
        tab = c.put_hevc_epel if row["chroma"] else c.put_hevc_qpel
        tab[int(row["my"] != 0)][int(row["mx"] != 0)][row["wi"]](_i16p(out[k]), 128, _u8p(win[k], ORG * stride + ORG * px), stride, row["h"], row["mx"], row["my"], _i16p(mcbuf))
    return out


def mc_restated(row, win, bd):
    """numpy int64 restatement of the two passes with their shifts (hevcdsp_template.c put_hevc_qpel_hv / epel_hv and the one-pass forms)"""
    chroma, mx, my, w, h = row["chroma"], row["mx"], row["my"], row["w"], row["h"]
    before, n = (1, 4) if chroma else (3, 8)
    a = win.astype(np.int64)
    if not mx and not my:
        return a[ORG:ORG + h, ORG:ORG + w] << (14 - bd)
    if mx:
        t = taps_of(chroma, mx)
        a = sum(int(t[k]) * a[:, ORG - before + k:ORG - before + k + w] for k in range(n)) >> (bd - 8)
    else:
        a = a[:, ORG:ORG + w]
    if my:
        t = taps_of(chroma, my)
        a = sum(int(t[k]) * a[ORG - before + k:ORG - before + k + h] for k in range(n)) >> (6 if mx else bd - 8)
    else:
        a = a[ORG:ORG + h]
    return a


def bad_rows(got, exp, names):
    bad = np.nonzero((got != exp).reshape(len(names), -1).any(1))[0]
    return "%d of %d rows differ, first: %s" % (len(bad), len(names), "; ".join(names[k] for k in bad[:6]))


def check_mc_table(prov, oracle, bd, cls, keep=None):
    """mi355_hevc_mc_batch_dev: all rows of one class in one launch"""
    rows = [r for r, j in zip(mc_rows(), pred_jobs(cls)) if keep is None or keep(j, cls)]
    win = mc_windows(rows, cls, bd)
    exp = mc_expected(oracle.hevcdsp(bd), bd, rows, win)
    px, stride = (2 if bd > 8 else 1), win.strides[1]
    d = Dev(prov.lib)
    try:
        p_win, p_out = d.up(win), d.up(np.full_like(exp, 0x2222))
        jobs = [McJob(p_win + k * win.strides[0] + ORG * stride + ORG * px, p_out + k * 8192, stride, 128, row["w"], row["h"], row["mx"], row["my"], row["chroma"])
                for k, row in enumerate(rows)]
        assert prov.lib.mi355_hevc_mc_batch_dev(C.c_void_p(d.up_jobs(jobs)), len(jobs), bd, None) == 0
        got = d.down(p_out, exp)
    finally:
        d.free()
    assert np.array_equal(got, exp), "mc batch: " + bad_rows(got, exp, ["%s %s bd%d" % (r["name"], cls, bd) for r in rows])
    return len(rows)


# ---------------------------------------------------------------------------------------------------------------- prediction rows

def pred_rows():
    """kinds 1..3 over every (kind, chroma, width index): denom 0 and 7, weights at -128 / 127, offsets at both ends, on intermediates of the
    tap-max / tap-min windows; fractions and heights walk their lists with the row's number"""
    rows = []
    for chroma in (0, 1):
        nf = 8 if chroma else 4
        for wi in range(8):
            w = (EW if chroma else QW)[wi]
            sets = [(1, 0, 0, 0, 0, 0, a, b) for a, b in (("tap-max", "tap-max"), ("tap-min", "tap-min"), ("tap-max", "tap-min"))]
            for denom in (0, 7):
                for w0 in (-128, 127):
                    for o0 in (-128, 127):
                        sets += [(2, denom, w0, 0, o0, 0, a, a) for a in ("tap-max", "tap-min")]
                for w0, w1 in ((127, 127), (-128, -128), (127, -128), (-128, 127)):
                    for o in (-128, 127):
                        sets += [(3, denom, w0, w1, o, o, a, a) for a in ("tap-max", "tap-min")]
            for i, (kind, denom, w0, w1, o0, o1, c0, c1) in enumerate(sets):
                k = i + 3 * wi
                f = (k % nf, (k // nf) % nf, (k + 2) % nf, (k // 3) % nf)
                rows.append(dict(chroma=chroma, wi=wi, w=w, h=(HC if chroma else HL)[k % 8], kind=kind, denom=denom, wt=(w0, w1, o0, o1), f=f, cls=(c0, c1),
                                 name="%s kind%d w%d denom%d w(%d,%d) o(%d,%d) %s/%s" % ("chroma" if chroma else "luma", kind, w, denom, w0, w1, o0, o1, c0, c1)))
    return rows


def pred_tabs(c, chroma):
    return ((c.put_unweighted_pred_chroma, c.put_unweighted_pred_avg_chroma, c.weighted_pred_chroma, c.weighted_pred_avg_chroma) if chroma
            else (c.put_unweighted_pred, c.put_unweighted_pred_avg, c.weighted_pred, c.weighted_pred_avg))


def call_pred(c, chroma, wi, kind, denom, wt, dp, stride, s1, s2, h):
    fn = pred_tabs(c, chroma)[kind][wi]
    w0, w1, o0, o1 = wt
    if kind == 0:
        fn(dp, stride, s1, 128, h)
    elif kind == 1:
        fn(dp, stride, s1, s2, 128, h)
    elif kind == 2:
        fn(denom, w0, o0, dp, stride, s1, 128, h)
    else:
        fn(denom, w0, w1, o0, o1, dp, stride, s1, s2, 128, h)


def pred_jobs(cls):
    """the prediction jobs of one content class: kind 0 for every row of the motion table, and — with the saturating intermediates — kinds 1..3"""
    jobs = [dict(r, kind=0, denom=0, wt=(0, 0, 0, 0), f=(r["mx"], r["my"], r["mx"], r["my"]), cls=(cls, cls), name="%s %s" % (r["name"], cls)) for r in mc_rows()]
    if cls == "tap-max":
        jobs += pred_rows()
    return jobs


def job_windows(jobs, bd, pad=0, seed=2):
    """reference windows 0 and 1 of each job (and, for a pair of chroma planes, of plane B: the swapped class)"""
    r = SplitMix64(0x5052 * 131 + bd * 7 + seed)
    wins = []
    for which in range(4):
        a = []
        for j in jobs:
            cls = j["cls"][which & 1]
            a.append(window(dict(chroma=j["chroma"] != 0, mx=j["f"][2 * (which & 1)], my=j["f"][2 * (which & 1) + 1]), swapped(cls) if which >= 2 else cls, bd, r, pad))
        wins.append(np.stack(a))
    return wins


def check_pred_table(prov, oracle, bd, cls):
    """mi355_hevc_pred_batch_dev on the oracle's intermediates of the class's windows"""
    jobs = pred_jobs(cls)
    w0, w1 = job_windows(jobs, bd)[:2]
    c = oracle.hevcdsp(bd)
    s1 = mc_expected(c, bd, [dict(j, mx=j["f"][0], my=j["f"][1]) for j in jobs], w0)
    s2 = mc_expected(c, bd, [dict(j, mx=j["f"][2], my=j["f"][3]) for j in jobs], w1)
    r = SplitMix64(0x77 + bd)
    pic = r.randint(0, (1 << bd) - 1, (len(jobs), 64, 64)).astype(np.uint16 if bd > 8 else np.uint8)
    exp, stride = pic.copy(), pic.strides[1]
    for k, j in enumerate(jobs):
        call_pred(c, j["chroma"], j["wi"], j["kind"], j["denom"], j["wt"], _u8p(exp[k]), stride, _i16p(s1[k]), _i16p(s2[k]), j["h"])
    d = Dev(prov.lib)
    try:
        p_pic, p1, p2 = d.up(pic), d.up(s1), d.up(s2)
        recs = [PredJob(p_pic + k * pic.strides[0], p1 + k * 8192, p2 + k * 8192, stride, 128, j["w"], j["h"], j["kind"], j["denom"], *j["wt"]) for k, j in enumerate(jobs)]
        assert prov.lib.mi355_hevc_pred_batch_dev(C.c_void_p(d.up_jobs(recs)), len(recs), bd, None) == 0
        got = d.down(p_pic, pic)
    finally:
        d.free()
    assert np.array_equal(got, exp), "pred batch: " + bad_rows(got, exp, ["%s bd%d" % (j["name"], bd) for j in jobs])
    return len(jobs)


# ---------------------------------------------------------------------------------------------------------------- transform rows

def dct_matrix(size):
    """the standard's transform matrix T[k][n] of a size-point inverse DCT (H.265 8.6.4.2: rows 0, 32/size, ... of the 32-point matrix)"""
    mag = [64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0]
    t = np.zeros((size, size), np.int64)
    for k in range(size):
        for n in range(size):
            a = ((2 * n + 1) * k * (32 // size)) & 127
            t[k, n] = 64 if k == 0 else (mag[a] if a <= 32 else (-mag[64 - a] if a <= 64 else (-mag[a - 64] if a <= 96 else mag[128 - a])))
    return t


def decoder_lim(lx, ly):
    """col_limit as hls_residual_coding derives it from the last significant position (hevcdec.c:1245-1256)"""
    mx, lim = max(lx, ly), lx + ly + 4
    return min(4, lim) if mx < 4 else (min(8, lim) if mx < 8 else (min(24, lim) if mx < 12 else lim))


def decoder_lims(size):
    return sorted({decoder_lim(lx, ly) for lx in range(size) for ly in range(size) if lx or ly})


def keep_mask(size, lx, ly):
    """where a block whose last significant position is (lx, ly) can hold coefficients: the 4x4 groups the diagonal scan reaches before that one's, and
    inside it up to the position's own diagonal; mask[y][x]"""
    ys, xs = np.mgrid[0:size, 0:size]
    return ((xs >> 2) + (ys >> 2) < (lx >> 2) + (ly >> 2)) | (((xs >> 2) == (lx >> 2)) & ((ys >> 2) == (ly >> 2)) & ((xs & 3) + (ys & 3) <= (lx & 3) + (ly & 3)))


def row_used(size, j, end):
    """does a size-point pass pruned to `end` read input j (hevcdsp_template.c:140-206: TR_8 inside TR_16 inside TR_32, odd inputs up to `end`)"""
    if size == 4:
        return True
    if j & 1:
        return j < end
    if size == 32 and (j >> 1) & 1:
        return (j >> 1) < (end >> 1)
    return True


def column_end(size, lim, i):
    """`end` of the first pass for column i: col_limit + 4, four less after every fourth column (:208-236)"""
    l0 = min(lim + 4, size)
    return l0 - 4 * ((i - 1) >> 2 if i > 0 else 0) if l0 < size else size


def pruned_mask(size, lim):
    """the positions both pruned passes of the reference read: a block with nothing elsewhere transforms the same pruned and in full"""
    return np.array([[row_used(size, y, column_end(size, lim, x)) and row_used(size, x, min(lim, size)) for x in range(size)] for y in range(size)])


IN_GROUP = ((0, 0), (1, 0), (0, 2), (3, 0), (1, 3), (2, 3), (3, 3), (0, 3))


def tu_rows():
    """every size x kind; for the inverse DCT every last position on every 4x4-group diagonal's two ends (eight positions inside the group, so that every
    col_limit of the decoder's rule occurs) and the plain limits 1..size in two forms (see below)"""
    rows = []
    for log2 in (2, 3, 4, 5):
        size, ng = 1 << log2, (1 << log2) // 4
        for gl in range(2 * ng - 1):
            ends = sorted({max(0, gl - ng + 1), min(gl, ng - 1)})
            for gx in ends:
                for (ix, iy) in (IN_GROUP if size > 4 else [(x, y) for y in range(4) for x in range(4)]):
                    lx, ly = 4 * gx + ix, 4 * (gl - gx) + iy
                    if lx or ly:
                        rows.append(dict(log2=log2, kind=0, lim=decoder_lim(lx, ly), mask=keep_mask(size, lx, ly), last=(lx, ly), rule="decoder",
                                         name="idct%d last(%d,%d) lim%d" % (size, lx, ly, decoder_lim(lx, ly))))
        for lim in range(1, size + 1):
            ys, xs = np.mgrid[0:size, 0:size]
            # "plain": the residual batch's contract (rows from limit + 4 on hold zeros, anything else anywhere);
            # "pruned": besides, what both pruned passes of the reference leave unread is zero — the coding-tree-block kernels' contract
            rows.append(dict(log2=log2, kind=0, lim=lim, mask=ys < lim + 4, last=None, rule="plain", name="idct%d plain lim%d" % (size, lim)))
            rows.append(dict(log2=log2, kind=0, lim=lim, mask=pruned_mask(size, lim) & (ys < lim + 4) & (xs < lim + 4), last=None, rule="pruned",
                             name="idct%d pruned lim%d" % (size, lim)))
        rows.append(dict(log2=log2, kind=1, lim=size, mask=np.ones((size, size), bool), last=None, rule="dc", name="dc%d" % size))
    for kind, nm in ((2, "dst4"), (3, "skip4")):
        rows.append(dict(log2=2, kind=kind, lim=4, mask=np.ones((4, 4), bool), last=None, rule=nm, name=nm))
    return rows


TU_CLASSES = ("laplace", "clip-high", "clip-low", "uniform") + tuple("single%s@%d" % (s, c) for s in ("+", "-") for c in range(4))
DST_CLASSES = ("noise", "zero", "max")


def tu_coefficients(row, cls, r, idx):
    """coefficients of a unit, [y][x], inside the row's mask.  clip-high / clip-low: +-32767 whose sign is sign(T[y][n0]) * sign(T[x][m0]) — column x of the
    first pass then overshoots int16 at output n0, upward or downward as T[x][m0] says (m0 odd rows of T change sign along x), and the second pass meets a
    row of saturated values whose signs follow its own matrix row; (n0, m0) walk with the row's number"""
    size = 1 << row["log2"]
    mask = row["mask"]
    if cls == "laplace":
        c = r.laplace_int(300, (size, size), 32767)
    elif cls == "uniform":
        c = r.randint(-32768, 32767, (size, size))
    elif cls in ("clip-high", "clip-low"):
        t = dct_matrix(size)
        n0, m0 = idx % size, (size - 1 - (idx // 3) % size)
        c = 32767 * np.sign(t[:, n0])[:, None] * np.sign(t[:, m0])[None, :] * (1 if cls == "clip-high" else -1)
    else:
        pts = [(int(y), int(x)) for y, x in zip(*np.nonzero(mask))]
        corner = int(cls[-1])
        # the allowed region's corners: first row's first and last sample, first column's last, and the last significant position (plain: the far corner)
        y, x = [min(pts), max(pts, key=lambda p: (-p[0], p[1])), max(pts, key=lambda p: (-p[1], p[0])), (row["last"][1], row["last"][0]) if row["last"] else max(pts)][corner]
        c = np.zeros((size, size), np.int64)
        c[y, x] = 32767 if cls[6] == "+" else -32768
    c = np.where(mask, c, 0)
    if row["last"]:
        lx, ly = row["last"]
        c[ly, lx] = c[ly, lx] or 1
    if row["kind"] == 1:
        c.reshape(-1)[1:] = 0x1111
    return c.astype(np.int16)


def tu_dst_classes(cls, idx):
    """the destination samples a unit adds to: the classes with large residuals on all three, the others on noise / 0 / maximum in turn"""
    return DST_CLASSES if cls in ("clip-high", "clip-low", "uniform") else (DST_CLASSES[idx % 3],)


def first_pass_unclipped(row, coef):
    """(sum_k T[k][n] x[k][i] + 64) >> 7 before the clip, int64, for an inverse DCT unit as the reference's pruned column pass computes it"""
    size = 1 << row["log2"]
    t, c = dct_matrix(size), coef.astype(np.int64).reshape(size, size)
    out = np.zeros((size, size), np.int64)
    for i in range(size):
        used = [j for j in range(size) if row_used(size, j, column_end(size, row["lim"], i))]
        out[:, i] = (t[used].T @ c[used, i] + 64) >> 7
    return out


def second_pass_unclipped(row, tmp, bd):
    size = 1 << row["log2"]
    t = dct_matrix(size)
    used = [j for j in range(size) if row_used(size, j, min(row["lim"], size))]
    return (tmp[:, used] @ t[used] + (1 << (19 - bd))) >> (20 - bd)


def call_tu(c, row, blk):
    i = row["log2"] - 2
    if row["kind"] == 0:
        c.idct[i](_i16p(blk), row["lim"])
    elif row["kind"] == 1:
        c.idct_dc[i](_i16p(blk))
    elif row["kind"] == 2:
        c.transform_4x4_luma(_i16p(blk))
    else:
        c.dequant(_i16p(blk))


# ---------------------------------------------------------------------------------------------------------------- scenes

class Scene:
    """named host arrays; prediction jobs, transform units and coding tree blocks whose pointers are (array name, byte offset)"""

    def __init__(self, bd):
        self.bd, self.px = bd, 2 if bd > 8 else 1
        self.arr, self.written = {}, []
        self.mc, self.tu, self.tu_free, self.ctbs = [], [], [], []      # tu_free: units without a destination (not part of any block)

    def add(self, name, a, written=False):
        self.arr[name] = np.ascontiguousarray(a)
        if written:
            self.written.append(name)
        return name

    def in_blocks(self):
        """the scene with only the jobs its coding tree blocks name"""
        p = Scene(self.bd)
        p.arr, p.written = self.arr, self.written
        for b in self.ctbs:
            p.mc += self.mc[b["mc"][0]:b["mc"][0] + b["mc"][1]]
            p.tu += self.tu[b["tu"][0]:b["tu"][0] + b["tu"][1]]
        return p

    def expected(self, c):
        """every prediction job, then every transform unit, through the provider's tables on a copy"""
        a = {k: v.copy() for k, v in self.arr.items()}

        def at(ref):
            return a[ref[0]].ctypes.data + ref[1]
        t = [np.zeros(64 * 64, np.int16), np.zeros(64 * 64, np.int16)]
        mcbuf = np.zeros((64 + 24) * 64, np.int16)
        for j in self.mc:
            tab = c.put_hevc_epel if j["chroma"] else c.put_hevc_qpel
            for plane in range(2 if j["chroma"] == 2 else 1):
                for which in range(2):
                    mx, my = j["f"][2 * which], j["f"][2 * which + 1]
                    src = j["src_b" if plane else "src"][which]
                    tab[int(my != 0)][int(mx != 0)][j["wi"]](_i16p(t[which]), 128, C.cast(at(src), _U8P), j["ss"][which], j["h"], mx, my, _i16p(mcbuf))
                call_pred(c, j["chroma"] != 0, j["wi"], j["kind"], j["denom"], j["wt"], C.cast(at(j["dst_b" if plane else "dst"]), _U8P), j["ds"], _i16p(t[0]), _i16p(t[1]), j["h"])
        for u in self.tu + self.tu_free:
            size = 1 << u["row"]["log2"]
            blk = np.frombuffer((C.c_int16 * (size * size)).from_address(at(u["coef"])), np.int16)
            call_tu(c, u["row"], blk)
            if u["dst"]:
                c.add_residual[u["row"]["log2"] - 2](C.cast(at(u["dst"]), _U8P), _i16p(blk), u["ds"])
                # include/mi355_hevc_batch.h: coefficients are rewritten in place only when dst == NULL — a unit with a destination leaves them as they were
                name, off = u["coef"]
                blk[:] = self.arr[name].reshape(-1)[off // 2:off // 2 + size * size]
        return a

    def records(self, base, with_free):
        def at(ref):
            return base[ref[0]] + ref[1] if ref else None
        mc = []
        for j in self.mc:
            q = McPredJob(at(j["src"][0]), at(j["src"][1]), at(j["dst"]), j["ss"][0], j["ss"][1], j["ds"], j["w"], j["h"], j["chroma"], j["kind"], *j["f"], j["denom"])
            q.w0, q.w1, q.o0, q.o1 = j["wt"]
            if j["chroma"] == 2:
                q.src0_b, q.src1_b, q.dst_b = at(j["src_b"][0]), at(j["src_b"][1]), at(j["dst_b"])
            mc.append(q)
        tu = [TuJob(at(u["coef"]), at(u["dst"]), u["ds"], u["row"]["log2"], u["row"]["lim"], u["row"]["kind"], 0) for u in self.tu + (self.tu_free if with_free else [])]
        ctbs = []
        for b in self.ctbs:
            q = CtbJob()
            for pl in range(3):
                q.dst[pl], q.stride[pl] = at(b["dst"][pl]), b["stride"][pl]
            q.width, q.height, q.log2_ctb_size, q.flags = b["w"], b["h"], b["log2"], b["flags"]
            q.first_mc, q.n_mc, q.first_tu, q.n_tu = b["mc"][0], b["mc"][1], b["tu"][0], b["tu"][1]
            ctbs.append(q)
        return mc, tu, ctbs

    def launch(self, prov, entry, flags=0):
        """one of the entry points on fresh uploads; returns the written arrays as the device left them (and what mi355_sync said)"""
        lib, bd = prov.lib, self.bd
        _declare(lib)
        d = Dev(lib)
        try:
            base = {k: d.up(v) for k, v in self.arr.items()}
            mc, tu, ctbs = self.records(base, entry != "ctbs")
            p_mc, p_tu = (d.up_jobs(mc) if mc else None), (d.up_jobs(tu) if tu else None)
            if entry == "batch":
                assert not mc or lib.mi355_hevc_mcpred_batch_dev(p_mc, len(mc), bd, None) == 0
                assert not tu or lib.mi355_hevc_residual_batch_dev(p_tu, len(tu), bd, None) == 0
            elif entry == "level":
                assert not mc or lib.mi355_hevc_recon_level_dev(p_mc, len(mc), None, 0, None, None, None, 0, bd, None) == 0
                assert not tu or lib.mi355_hevc_recon_level_dev(None, 0, p_tu, len(tu), None, None, None, 0, bd, None) == 0
            elif entry == "levels":
                # level 0: the prediction jobs; then the units (they add to what level 0 wrote) in levels of 1, 2, 5, 64, 257 units in turn
                levels, wg, k, i = [], 0, 0, 0
                if mc:
                    levels.append(Level(0, 0, len(mc), 0, 0, 0, 0, 0))
                    wg = len(mc)
                while k < len(tu):
                    n = min((1, 2, 5, 64, 257)[i % 5], len(tu) - k)
                    levels.append(Level(wg, 0, 0, k, n, 0, 0, 0))
                    wg, k, i = wg + (n + 1) // 2, k + n, i + 1
                assert lib.mi355_hevc_recon_levels_dev(d.up_jobs(levels), len(levels), wg, p_mc, p_tu, None, None, None, bd, None) == 0
            else:
                assert lib.mi355_hevc_recon_ctbs_dev(d.up_jobs(ctbs), len(ctbs), p_mc, p_tu, bd, flags, None) == 0
            rc = lib.mi355_sync(None)
            got = {k: d.down(base[k], self.arr[k]) for k in self.written}
        finally:
            d.free()
        return got, rc

    def compare(self, got, exp, what):
        """every byte of every written array — planes with their guard bands, coefficient buffers with the words around the slots; a difference is traced to the
        jobs whose samples or coefficients differ"""
        tag, msgs = "%s bd%d" % (what, self.bd), []
        for name in self.written:
            if np.array_equal(got[name], exp[name]):
                continue
            diff = (got[name] != exp[name]).reshape(-1)
            names = []
            for j in self.mc + self.tu + self.tu_free:
                for key in ("dst", "dst_b"):
                    ref = j.get(key)
                    if ref and ref[0] == name:
                        w, h = (j["w"], j["h"]) if "w" in j else (1 << j["row"]["log2"],) * 2
                        o, ss = ref[1] // self.px, j["ds"] // self.px
                        if any(diff[o + y * ss:o + y * ss + w].any() for y in range(h)):
                            names.append(j["name"])
                if "coef" in j and j["coef"][0] == name and diff[j["coef"][1] // 2:j["coef"][1] // 2 + (1 << (2 * j["row"]["log2"]))].any():
                    names.append(j["name"])
            msgs.append("%s differs at %d elements; jobs: %s" % (name, int(diff.sum()), "; ".join(names[:6]) or "none (outside every job: guard band or uncovered samples)"))
        assert not msgs, "%s: %s" % (tag, " | ".join(msgs))


_U8P = C.POINTER(C.c_uint8)


def _declare(lib):
    v = C.c_void_p
    lib.mi355_hevc_mcpred_batch_dev.argtypes = [v, C.c_int, C.c_int, v]
    lib.mi355_hevc_residual_batch_dev.argtypes = [v, C.c_int, C.c_int, v]
    lib.mi355_hevc_recon_level_dev.argtypes = [v, C.c_int, v, C.c_int, v, v, v, C.c_int, C.c_int, v]
    lib.mi355_hevc_recon_levels_dev.argtypes = [v, C.c_int, C.c_int] + [v] * 5 + [C.c_int, v]
    lib.mi355_hevc_recon_ctbs_dev.argtypes = [v, C.c_int, v, v, C.c_int, C.c_uint, v]
    for f in ("mi355_hevc_mcpred_batch_dev", "mi355_hevc_residual_batch_dev", "mi355_hevc_recon_level_dev", "mi355_hevc_recon_levels_dev", "mi355_hevc_recon_ctbs_dev", "mi355_sync"):
        getattr(lib, f).restype = C.c_int
    lib.mi355_error_word_take.restype = C.c_uint


def noise(r, shape, bd):
    return r.randint(0, (1 << bd) - 1, shape).astype(np.uint16 if bd > 8 else np.uint8)


def mc_job(scene, j, k, wins, dst, dst_b, ds):
    """job j with its windows at cell k of the window arrays `wins` (names of four arrays: reference 0 / 1, plane A / B)"""
    px = scene.px
    ss = [scene.arr[wins[0]].strides[1], scene.arr[wins[1]].strides[1]]
    off = [k * scene.arr[w].strides[0] + ORG * scene.arr[w].strides[1] + ORG * px for w in wins]
    return dict(j, src=[(wins[0], off[0]), (wins[1], off[1])], src_b=[(wins[2], off[2]), (wins[3], off[3])], ss=ss, dst=dst, dst_b=dst_b, ds=ds)


def mc_scene(bd, cls, pad=0, pairs=True, keep=None):
    """the motion / prediction table as fused jobs: a picture of 64x64 blocks, each with one luma job and one chroma job (into the block's Cb plane; a pair
    job — both chroma planes in one record, unweighted kinds — into Cb and Cr).  Every block is also a coding tree block with
    MI355_HEVC_CTB_PARTIAL, so the same records go through all four entry points."""
    s = Scene(bd)
    jobs = [j for j in pred_jobs(cls) if keep is None or keep(j, cls)]
    if pairs:
        jobs += [dict(j, chroma=2, name=j["name"] + " pair") for j in jobs if j["chroma"] and j["kind"] < 2]
    r = SplitMix64(0x5343 + bd)
    lum, chrom = [j for j in jobs if not j["chroma"]], [j for j in jobs if j["chroma"]]
    n = max(len(lum), len(chrom))
    blocks = [[q[i] for q in (lum, chrom) if i < len(q)] for i in range(n)]
    jobs = [j for b in blocks for j in b]
    s.add("Y", noise(r, (n, 64, 64), bd), True), s.add("Cb", noise(r, (n, 32, 32), bd), True), s.add("Cr", noise(r, (n, 32, 32), bd), True)
    for i, w in enumerate(job_windows(jobs, bd, pad)):
        s.add("win%d" % i, w)
    wins = ["win0", "win1", "win2", "win3"]
    for i, b in enumerate(blocks):
        first = len(s.mc)
        for j in b:
            pl = "Cb" if j["chroma"] else "Y"
            st = s.arr[pl].strides
            s.mc.append(mc_job(s, j, len(s.mc), wins, (pl, i * st[0]), ("Cr", i * st[0]) if j["chroma"] == 2 else None, st[1]))
        s.ctbs.append(dict(dst=[(p, i * s.arr[p].strides[0]) for p in ("Y", "Cb", "Cr")], stride=[s.arr[p].strides[1] for p in ("Y", "Cb", "Cr")], w=64, h=64, log2=6,
                           flags=1, mc=(first, len(b)), tu=(0, 0), name=b[0]["name"]))
    return s


def tu_units(bd, cls, seed=3):
    """(row, coefficients, destination class, aligned) of every unit of one content class: each row on its destination classes, each at both addresses"""
    r = SplitMix64(0x5455 * 131 + bd * 7 + seed + TU_CLASSES.index(cls) * 1009)
    units = []
    for idx, row in enumerate(tu_rows()):
        c = tu_coefficients(row, cls, r, idx)
        for dcls in tu_dst_classes(cls, idx):
            for aligned in (True, False):
                units.append((row, c, dcls, aligned))
    return units


def tu_scene(bd, cls):
    """the transform table on a picture of 64x64 blocks (MI355_HEVC_CTB_PARTIAL), six units a block: one in each luma quadrant, one in Cb, one in Cr.  A unit's
    coefficients lie in a 2048-byte slot, or 8 bytes into one (int16-aligned, not 16-byte aligned); the 16-byte aligned units come first, so that blocks of
    nothing but aligned 16x16 / 32x32 inverse DCTs (the matrix-path kernel's) occur beside mixed ones.  A "plain" row's aligned 16x16 / 32x32 units are outside the
    block kernels' contract: they come last and belong to no block.  Every unit once more without a destination (rewritten in place): the batch and level entry points only."""
    s = Scene(bd)
    def outside(u):
        return u[0]["rule"] == "plain" and u[3] and u[0]["log2"] >= 4 and u[0]["lim"] < (1 << u[0]["log2"])
    units = sorted(tu_units(bd, cls), key=lambda u: (outside(u), not u[3]))
    n, nb = len(units), -(-len(units) // 6)
    r = SplitMix64(0x5453 + bd)
    top = (1 << bd) - 1
    planes = {"Y": noise(r, (nb, 64, 64), bd), "Cb": noise(r, (nb, 32, 32), bd), "Cr": noise(r, (nb, 32, 32), bd)}
    coef = np.zeros((2 * n, 1024), np.int16)
    coef8 = np.zeros(2 * n * 1024 + 8, np.int16)
    where = []
    for k, (row, c, dcls, aligned) in enumerate(units):
        b, q = divmod(k, 6)
        pl, y0, x0 = ("Y", 32 * (q >> 1), 32 * (q & 1)) if q < 4 else (("Cb", "Cr")[q - 4], 0, 0)
        if dcls != "noise":
            planes[pl][b, y0:y0 + 32, x0:x0 + 32] = top if dcls == "max" else 0
        where.append((pl, b, y0, x0))
        for slot in (k, n + k):
            if aligned:
                coef[slot, :c.size] = c.reshape(-1)
            else:
                coef8[4 + slot * 1024:4 + slot * 1024 + c.size] = c.reshape(-1)
    for name in ("Y", "Cb", "Cr"):
        s.add(name, planes[name], True)
    s.add("coef", coef, True), s.add("coef8", coef8, True)
    in_block = []
    for k, (row, c, dcls, aligned) in enumerate(units):
        name = "%s %s dst-%s %s" % (row["name"], cls, dcls, "slot" if aligned else "slot+8")
        pl, b, y0, x0 = where[k]
        a = s.arr[pl]

        def ref(slot):
            return ("coef", slot * 2048) if aligned else ("coef8", 8 + slot * 2048)
        s.tu.append(dict(row=row, coef=ref(k), dst=(pl, b * a.strides[0] + y0 * a.strides[1] + x0 * s.px), ds=a.strides[1], name=name))
        s.tu_free.append(dict(row=row, coef=ref(n + k), dst=None, ds=0, name=name + " in place"))
        in_block.append(not outside(units[k]))
    for b in range(nb):                               # the units outside the contract are the list's tail: a block's own units are one run from its first
        m = sum(in_block[6 * b:6 * b + 6])
        if m:
            s.ctbs.append(dict(dst=[(p, b * s.arr[p].strides[0]) for p in ("Y", "Cb", "Cr")], stride=[s.arr[p].strides[1] for p in ("Y", "Cb", "Cr")], w=64, h=64, log2=6,
                               flags=1, mc=(0, 0), tu=(6 * b, m), name=s.tu[6 * b]["name"]))
    return s


def ctb_takes_matrix_path(scene, b):
    """include/mi355_hevc_batch.h: one-reference unweighted blocks with sides that are multiples of 16 and reference rows a multiple of the piece size (16 bytes;
    8 at 8 bits), 16x16 / 32x32 inverse DCTs with 16-byte aligned coefficients — for ALL jobs of the block"""
    piece = 16 if scene.bd > 8 else 8
    return (all(j["kind"] == 0 and j["w"] % 16 == 0 and j["h"] % 16 == 0 and j["ss"][0] % piece == 0 for j in scene.mc[b["mc"][0]:b["mc"][0] + b["mc"][1]]) and
            all(u["row"]["kind"] == 0 and u["row"]["log2"] >= 4 and u["coef"][1] % 16 == 0 and u["coef"][0] == "coef" for u in scene.tu[b["tu"][0]:b["tu"][0] + b["tu"][1]]))


ENTRIES = ("batch", "level", "levels", "ctbs")


def emu_entries(table, cls, bd):
    """the emulator runs every row of every class through the batch, level and levels entry points at both bit depths.  A block per workgroup of 512 emulated
    threads is its slow part (two thirds of the emulated tables' time when every class went through it), so the block kernels see, of the fused table, noise at
    8 bits and tap-max at 10, and of the transform table Laplace and clip-high at both depths, clip-low at 10 bits, full range at 8, and the single coefficient
    at the last significant position (+ at 8 bits, - at 10).  The GPU runs every class through all four at 8, 9 and 10 bits."""
    if table == "mc":
        full = {8: ("noise",), 10: ("tap-max",)}[bd]
    else:
        full = ("laplace", "clip-high") + {8: ("uniform", "single+@3"), 10: ("clip-low", "single-@3")}[bd]
    return ENTRIES if cls in full else ENTRIES[:3]


def check_scene(prov, oracle, scene, what, entries=ENTRIES):
    c = oracle.hevcdsp(scene.bd)
    exp = scene.expected(c)
    for entry in entries:
        got, rc = scene.launch(prov, entry)
        assert rc == 0, "%s through %s: mi355_sync says %d" % (what, entry, rc)
        if entry == "ctbs":
            part = scene.in_blocks()
            part.compare(got, part.expected(c), "%s through ctbs" % what)
        else:
            scene.compare(got, exp, "%s through %s" % (what, entry))
    return len(scene.mc) + len(scene.tu) + len(scene.tu_free)


MI355_E_DEVICE_FAULT, MI355_ERR_CTB_NOT_UNIFORM, MI355_HEVC_RECON_UNIFORM = -5, 2, 1        # include/mi355dsp.h, include/mi355_hevc_batch.h


def check_promise(prov, oracle, scene, what):
    """MI355_HEVC_RECON_UNIFORM on a list that breaks the promise: blocks whose jobs are all matrix-path shapes come out as the oracle's, the others are
    untouched, and the error word says MI355_ERR_CTB_NOT_UNIFORM"""
    uni = [ctb_takes_matrix_path(scene, b) for b in scene.ctbs]
    assert 0 < sum(uni) < len(uni), "%s: the list must mix both kinds of block" % what
    # what the promise leaves: the oracle's result with only the uniform blocks' jobs
    part = Scene(scene.bd)
    part.arr, part.written = scene.arr, scene.written
    for b, u in zip(scene.ctbs, uni):
        if u:
            part.mc += scene.mc[b["mc"][0]:b["mc"][0] + b["mc"][1]]
            part.tu += scene.tu[b["tu"][0]:b["tu"][0] + b["tu"][1]]
    want = part.expected(oracle.hevcdsp(scene.bd))
    prov.lib.mi355_error_word_take.restype = C.c_uint
    prov.lib.mi355_error_word_take()
    got, rc = scene.launch(prov, "ctbs", flags=MI355_HEVC_RECON_UNIFORM)
    assert rc == MI355_E_DEVICE_FAULT, "%s: a block outside the promised shapes must be reported (MI355_E_DEVICE_FAULT), got %d" % (what, rc)
    assert prov.lib.mi355_error_word_take() == MI355_ERR_CTB_NOT_UNIFORM and prov.lib.mi355_sync(None) == 0
    part.mc, part.tu = scene.mc, scene.tu                   # for the names in a failure's message
    part.compare(got, want, what + " under MI355_HEVC_RECON_UNIFORM")
    return sum(uni)


# ---------------------------------------------------------------------------------------------------------------- coding tree block geometries

def geometry_pictures():
    """(name, log2_ctb_size, block widths, block heights, first PARTIAL parity, reference row padding): pictures of 2 x 2 blocks whose last column / row is
    whole or ragged (remainders 8, 24, 56 below the block size), each with MI355_HEVC_CTB_PARTIAL on the blocks of either parity; a one-block picture; a
    picture narrower than one block"""
    pics = []
    for log2 in (4, 5, 6):
        s = 1 << log2
        rems = [0] + [q for q in (8, 24, 56) if q < s]
        for rw in rems:
            for rh in rems:
                for parity in (0, 1):
                    pics.append(("ctb%d rem(%d,%d) partial%d" % (s, rw, rh, parity), log2, [s, rw or s], [s, rh or s], parity, 2 * ((rw + rh) // 8 % 2)))
        pics.append(("ctb%d one block" % s, log2, [s], [s], 0, 0))
        pics.append(("ctb%d one block partial" % s, log2, [s], [s], 1, 0))
        pics.append(("ctb%d narrow" % s, log2, [8], [s, 8], 0, 2))
    return pics


def _tile(w, h, sizes_w, sizes_h, k):
    """w x h covered by blocks of the listed sizes: greedily the largest that fits, every third column / row of blocks (by k) one size smaller"""
    out, y, n = [], 0, k
    while y < h:
        fit = [q for q in sizes_h if q <= h - y]
        bh = fit[-1 - (n % 3 == 2 and len(fit) > 1)]
        x = 0
        while x < w:
            fit = [q for q in sizes_w if q <= w - x]
            bw = fit[-1 - (n % 3 == 1 and len(fit) > 1)]
            out.append((x, y, bw, bh))
            x, n = x + bw, n + 1
        y += bh
    return out


def geometry_scene(bd, cls="tap-max", tu_cls="clip-high", heavy=True):
    """every picture of geometry_pictures() in one list of blocks, plus (heavy) one 64x64 block split down to 8x4 / 4x8 prediction blocks and 4x4 units.
    Prediction blocks take their fractions, kinds and weights from the motion / prediction tables' rows of their width in turn, transform units their limits
    and content from the transform table's rows of their size in turn.  Whole 64 / 32 blocks with an even number take only matrix-path shapes.  Planes carry a
    poisoned guard band of 8 samples on all four sides and 4 samples of poisoned row padding."""
    s = Scene(bd)
    px, r = s.px, SplitMix64(0x4745 + bd)
    pj = pred_jobs(cls)
    by_w = {(c, wi): [j for j in pj if j["chroma"] == c and j["wi"] == wi] for c in (0, 1) for wi in range(8)}
    rows = tu_rows()
    by_size = {log2: [q for q in rows if q["log2"] == log2 and q["rule"] != "plain"] for log2 in (2, 3, 4, 5)}
    fast_rows = {log2: [q for q in by_size[log2] if q["kind"] == 0 and q["rule"] == "decoder"] for log2 in (4, 5)}
    turn, jobs, wins_of, coefs = {}, [], [], []
    tr = SplitMix64(0x4746 + bd)

    def nxt(key, lst):
        turn[key] = turn.get(key, -1) + 1
        return lst[(turn[key] * 7) % len(lst)]

    def block(name, planes, x0, y0, w, h, log2, partial, pad, uniform, fine=False):
        first_mc, first_tu = len(s.mc), len(s.tu)
        if fine:
            pus = [(8 * (i % 8) + (4 * k if (i + i // 8) % 2 else 0), 8 * (i // 8) + (0 if (i + i // 8) % 2 else 4 * k), 4 if (i + i // 8) % 2 else 8, 8 if (i + i // 8) % 2 else 4)
                   for i in range(64) for k in range(2)]
        elif uniform:
            pus = _tile(w, h, [32, 64] if w == 64 else [32], [32], 0)
        else:
            pus = _tile(w, h, QW, HL, len(s.ctbs))
        for n, (x, y, bw, bh) in enumerate(pus):
            if partial and not uniform and not fine and n % 3 == 2:
                continue                                                   # a hole: MI355_HEVC_CTB_PARTIAL keeps what was there
            for comp in (0, 1):
                cw, ch, cx, cy = bw >> comp, bh >> comp, (x0 + x) >> comp, (y0 + y) >> comp
                wi = (EW if comp else QW).index(cw)
                j = nxt((comp, wi, uniform), [q for q in by_w[(comp, wi)] if q["kind"] == 0] if uniform else by_w[(comp, wi)])
                pair = comp and j["kind"] < 2 and (n % 2 == 0 or uniform)
                for pl in ((1,) if pair else (1, 2)) if comp else (0,):
                    a = planes[pl]
                    st = s.arr[a].strides[0]
                    dst = (a, (8 + cy) * st + (8 + cx) * px)
                    jj = dict(j, h=ch, chroma=2 if pair else comp, name="%s: %s at (%d,%d) plane %d" % (name, j["name"], cx, cy, pl))
                    s.mc.append(dict(jj, dst=dst, dst_b=(planes[2], dst[1]) if pair else None, ds=st, pad=pad))
        for comp in (0, 1, 2):
            sh = 1 if comp else 0
            sizes = [32] if uniform and not comp else ([16] if uniform else ([4] if fine else [4, 8, 16, 32]))
            a = planes[comp]
            st = s.arr[a].strides[0]
            for n, (x, y, sz) in enumerate(_squares(w >> sh, h >> sh, sizes, len(s.ctbs) + comp)):
                if partial and not uniform and not fine and n % 4 == 3:
                    continue
                log2u = sz.bit_length() - 1
                row = nxt(("tu", log2u, uniform), fast_rows[log2u] if uniform else by_size[log2u])
                ucls = tu_cls if uniform or n % 2 == 0 else TU_CLASSES[(n // 2) % len(TU_CLASSES)]
                aligned = True if uniform else (n % 3 != 1)
                c = tu_coefficients(row, ucls, tr, len(coefs))
                coefs.append((c, aligned))
                s.tu.append(dict(row=row, coef=len(coefs) - 1, aligned=aligned, dst=(a, (8 + ((y0 >> sh) + y)) * st + (8 + ((x0 >> sh) + x)) * px), ds=st,
                                 name="%s: %s %s at (%d,%d) plane %d" % (name, row["name"], ucls, (x0 >> sh) + x, (y0 >> sh) + y, comp)))
        s.ctbs.append(dict(dst=[(planes[pl], (8 + (y0 >> (pl > 0))) * s.arr[planes[pl]].strides[0] + (8 + (x0 >> (pl > 0))) * px) for pl in range(3)],
                           stride=[s.arr[planes[pl]].strides[0] for pl in range(3)], w=w, h=h, log2=log2, flags=1 if partial else 0,
                           mc=(first_mc, len(s.mc) - first_mc), tu=(first_tu, len(s.tu) - first_tu), name=name, fine=fine, rem=(w, h)))

    def picture(name, log2, ws, hs, parity, pad, fine=False):
        W, H = sum(ws), sum(hs)
        planes = []
        for pl in range(3):
            sh = 1 if pl else 0
            a = np.full(((H >> sh) + 16, (W >> sh) + 16 + 4), POISON * 0x0101 if bd > 8 else POISON, np.uint16 if bd > 8 else np.uint8)
            a[8:8 + (H >> sh), 8:8 + (W >> sh)] = noise(r, (H >> sh, W >> sh), bd)
            planes.append(s.add("%s/p%d" % (name, pl), a, True))
        n, y0 = 0, 0
        for h in hs:
            x0 = 0
            for w in ws:
                whole = w == h == (1 << log2) and log2 >= 5
                block("%s block(%d,%d)" % (name, x0, y0), planes, x0, y0, w, h, log2, (n + parity) % 2 == 1 or fine, pad, whole and n % 2 == 0 and not fine, fine)
                x0, n = x0 + w, n + 1
            y0 += h

    for p in geometry_pictures():
        picture(*p)
    if heavy:
        picture("ctb64 split to 8x4 / 4x8 and 4x4", 6, [64], [64], 0, 0, fine=True)
    # the windows and coefficients the jobs named, now that their number is known
    for pad in (0, 2):
        idx = [k for k, j in enumerate(s.mc) if j["pad"] == pad]
        if not idx:
            continue
        wins = job_windows([s.mc[k] for k in idx], bd, pad, seed=5 + pad)
        names = [s.add("win%d/%d" % (pad, i), w) for i, w in enumerate(wins)]
        for n, k in enumerate(idx):
            j = s.mc[k]
            s.mc[k] = mc_job(s, j, n, names, j["dst"], j["dst_b"], j["ds"])
    coef = np.zeros((len(coefs), 1024), np.int16)
    coef8 = np.zeros(len(coefs) * 1024 + 8, np.int16)
    for k, (c, aligned) in enumerate(coefs):
        if aligned:
            coef[k, :c.size] = c.reshape(-1)
        else:
            coef8[4 + k * 1024:4 + k * 1024 + c.size] = c.reshape(-1)
    s.add("coef", coef, True), s.add("coef8", coef8, True)
    for u in s.tu:
        u["coef"] = ("coef", u["coef"] * 2048) if u["aligned"] else ("coef8", 8 + u["coef"] * 2048)
    return s


def _squares(w, h, sizes, k):
    """w x h covered by squares of the listed sizes (each divides the next): 4-sample cells taken by the largest square that fits, is aligned to its own size
    and is free, every third one a size smaller"""
    out, free, n = [], np.ones((h // 4, w // 4), bool), k
    for cy in range(h // 4):
        for cx in range(w // 4):
            if not free[cy, cx]:
                continue
            fit = [q for q in sizes if cx * 4 % q == 0 and cy * 4 % q == 0 and cx * 4 + q <= w and cy * 4 + q <= h and free[cy:cy + q // 4, cx:cx + q // 4].all()]
            q = fit[-1 - (n % 3 == 2 and len(fit) > 1)]
            free[cy:cy + q // 4, cx:cx + q // 4] = False
            out.append((cx * 4, cy * 4, q))
            n += 1
    return out


# ---------------------------------------------------------------------------------------------------------------- digests of the saturating classes

def _sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def saturating_digests(c, depths=(8, 9, 10)):
    """{name: sha1} of a provider's results on the saturating classes: the 14-bit intermediates per (class, filter, width) — the table's rows of that width
    in order —, the predicted planes of the fused table per class, and per transform class the residual-added planes and the coefficients rewritten in place"""
    out = {}
    for bd in depths:
        ctx = c.hevcdsp(bd)
        rows = mc_rows()
        for cls in SATURATING:
            exp = mc_expected(ctx, bd, rows, mc_windows(rows, cls, bd))
            for chroma in (0, 1):
                for wi in range(8):
                    sel = [k for k, q in enumerate(rows) if q["chroma"] == chroma and q["wi"] == wi]
                    out["bd%d %s w%d %s" % (bd, "epel" if chroma else "qpel", (EW if chroma else QW)[wi], cls)] = _sha(exp[sel])
            e = mc_scene(bd, cls).expected(ctx)
            out["bd%d fused table %s" % (bd, cls)] = _sha(e["Y"], e["Cb"], e["Cr"])
        for cls in TU_CLASSES[1:]:
            e = tu_scene(bd, cls).expected(ctx)
            out["bd%d transform table %s samples" % (bd, cls)] = _sha(e["Y"], e["Cb"], e["Cr"])
            out["bd%d transform table %s in place" % (bd, cls)] = _sha(e["coef"], e["coef8"])
    return out
