"""Tables of the HEVC in-loop filters' cases (include/mi355_hevc_batch.h: mi355_hevc_deblock_pictures_dev, mi355_hevc_boundary_strengths_dev,
mi355_hevc_sao_ctbs_dev, mi355_hevc_filter_ctbs_dev): small BUILT pictures — every grid size, ragged size, the whole legal QP / offset range, pcm marks,
reference indices up to 15, every SAO form on every border — with the censuses that tests/test_hevc_filter_content.py takes of them.  Everything is bit-exact, 4:2:0.
The structures are those of hevc_filter_cases / hevc_bs_cases / hevc_batch; what those modules' own CASES produce is untouched."""
import collections
import ctypes as C
import hashlib

import numpy as np

import abi_ctypes as A
from hevc_batch import Dev, SaoCtbJob, sao_ctb_pieces
from hevc_bs_cases import BsPicture, MVF_DT, L_BLOCK, T_BLOCK, L_INNER, T_INNER
from hevc_filter_cases import LfPicture
from rng import SplitMix64

DEPTHS = (8, 9, 10)
POISON = 0xA5
QP_MIN = {8: 0, 9: -6, 10: -12}            # qp_y_tab holds QpY in -QpBdOffset .. 51 (QpBdOffset = 6 * (bit depth - 8))
TCTABLE = [0] * 18 + [1] * 9 + [2] * 4 + [3] * 4 + [4] * 3 + [5, 5, 6, 6, 7, 8, 9, 10, 11, 13, 14, 16, 18, 20, 22, 24]
BETATABLE = [0] * 16 + list(range(6, 19)) + list(range(20, 66, 2))
QP_C = [29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37]
assert len(TCTABLE) == 54 and len(BETATABLE) == 52


def px_of(bd):
    return 2 if bd > 8 else 1


def new_plane(pw, ph, bd, fill=POISON):
    """a plane's buffer: a guard row above and below, rows padded by at least 32 bytes — all of it `fill` (the poison the checks look for afterwards)"""
    stride = (pw * px_of(bd) + 31) // 32 * 32 + 32
    return np.full((ph + 2, stride), fill, np.uint8)


def samples(buf, pw, ph, bd):
    """the picture's samples inside a plane buffer, as a writable view"""
    return buf[1:ph + 1, :pw * px_of(bd)].view(np.uint16 if bd > 8 else np.uint8)


def outside_is_poison(buf, pw, ph, bd, fill=POISON):
    return bool((buf[0] == fill).all() and (buf[-1] == fill).all() and (buf[1:ph + 1, pw * px_of(bd):] == fill).all())


def digest(bufs):
    h = hashlib.sha1()
    for b in bufs:
        h.update(np.ascontiguousarray(b).tobytes())
    return h.hexdigest()[:20]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 1. deblocking table
# tag: (width, height, log2 ctb, log2 min cb, pcmf, pictures per launch, (cb_qp_offset, cr_qp_offset))       log2_min_pu_size = log2_min_cb_size - 1
LF_SHAPES = {
    "s16":  (16, 16, 4, 3, 0, 1, (12, 12)),          # one vertical and one horizontal luma edge, no chroma edge
    "w8":   (8, 40, 4, 3, 1, 1, (-12, -12)),         # 8 wide: no vertical edge at all; the horizontal chroma pair at x = -8 ends the picture
    "h8":   (40, 8, 4, 3, 1, 2, (0, 0)),             # 8 high: no horizontal edge at all
    "r104": (104, 72, 5, 3, 1, 2, (-12, 12)),        # width % 16 == 8 and height % 16 == 8, neither a multiple of the CTB
    "c160": (160, 128, 6, 4, 0, 1, (12, -12)),       # min CB 16; width not a multiple of the CTB
    "b160": (160, 96, 5, 5, 1, 3, (5, -3)),          # min CB 32 = the CTB, min PU 16
    "r200": (200, 136, 6, 3, 1, 3, (-7, 9)),         # width % 16 == 8 and height % 16 == 8 under 64x64 CTBs
}
LF_CASES = ["%s_%d" % (tag, bd) for tag in LF_SHAPES for bd in DEPTHS]


def lf_workgroups(w, h, npics):
    """workgroups of the two launches of mi355_hevc_deblock_pictures_dev (vertical edges, horizontal edges): a workgroup is one wave that looks at 64 candidate
    segments — luma on the 8x8 grid, then the two chroma planes on the 16x16 luma grid (horizontal chroma pairs start at x = -8: one more column).  The kernel
    reorders its workgroups over the eight XCDs when their count is a multiple of eight and takes them as they come otherwise."""
    lc, lr, cr = (w + 7) // 8, (h + 7) // 8, (h + 15) // 16
    out = []
    for d in range(2):
        cc = (w + 8 + 15) // 16 if d else (w + 15) // 16
        out.append(((lc * lr + 63) // 64 + (2 * cc * cr + 63) // 64) * npics)
    return tuple(out)


# sample profiles across an 8-sample block side, in units of 1 << (bit depth - 8): flat, ramps (second differences 0), kinks beside either edge, a peak at the edge
PROFILES = [(0,) * 8, (0,) * 8, (0, 1, 2, 3, 4, 5, 6, 7), (7, 6, 5, 4, 3, 2, 1, 0), (0, 0, 0, 0, 0, 0, 2, 0), (0, 2, 0, 0, 0, 0, 0, 0), (0, 3, 0, 0, 0, 0, 3, 0),
            (0, 0, 1, 1, 1, 1, 0, 0), (4, 0, 0, 0, 0, 0, 0, 4), (0, 9, 0, 0, 0, 0, 9, 0), (0, 0, 0, 1, 1, 0, 0, 0), (2, 1, 0, 0, 0, 0, 1, 2)]
STEPS = [0, 0, 0, 1, -1, 2, -2, 3, -3, 4, -5, 6, -7, 9, -10, 12, -14, 18, -22, 28, -36, 50, -70, 100, -120]


class LfCase:
    """picture `pic` of the launch of table row `name`: built samples plus the frame-level arrays of mi355_hevc_lf_picture"""

    def __init__(self, name, pic=0):
        tag, bd = name.rsplit("_", 1)
        self.name, self.pic, self.bd = name, pic, int(bd)
        self.w, self.h, self.l2ctb, self.l2cb, self.pcmf, self.npics, (self.cb_off, self.cr_off) = LF_SHAPES[tag]
        bd, w, h = self.bd, self.w, self.h
        r = SplitMix64(0x1F7AB1E + 1000 * list(LF_SHAPES).index(tag) + 10 * bd + pic)
        if pic & 1:
            self.cb_off, self.cr_off = self.cr_off, self.cb_off
        self.l2pu = self.l2cb - 1
        mx, sc = (1 << bd) - 1, 1 << (bd - 8)
        self.planes = []
        for c in range(3):
            pw, ph = (w, h) if c == 0 else (w // 2, h // 2)
            nbx, nby = (pw + 7) // 8, (ph + 7) // 8
            # per block: a zone's base (mid grey, or hard at either end of the range), a step from the menu; per block column / row a profile
            zone = np.array([mx // 2, mx // 2, mx // 2, mx // 3, 2 * sc, mx - 2 * sc])[r.randint(2 if c else 0, 5, ((nby + 1) // 2, (nbx + 1) // 2))]
            level = np.kron(zone, np.ones((2, 2), np.int64))[:nby, :nbx] + sc * np.array(STEPS)[r.randint(0, len(STEPS) - 1, (nby, nbx))]
            hp = np.array(PROFILES)[r.randint(0, len(PROFILES) - 1, nbx)].reshape(-1)[:pw]
            vp = np.array(PROFILES)[r.randint(0, len(PROFILES) - 1, nby)].reshape(-1)[:ph]
            a = np.kron(level, np.ones((8, 8), np.int64))[:ph, :pw] + sc * (hp[None, :] + vp[:, None])
            # the seeded remainder: three blocks in ten carry noise of a few steps, a few samples anything
            noisy = np.kron((r.uniform((nby, nbx)) < 0.3).astype(np.int64), np.ones((8, 8), np.int64))[:ph, :pw]
            a = a + noisy * r.randint(-4 * sc, 4 * sc, (ph, pw))
            a = np.where(r.uniform((ph, pw)) < 0.01, r.randint(0, mx, (ph, pw)), a)
            buf = new_plane(pw, ph, bd)
            samples(buf, pw, ph, bd)[:] = np.clip(a, 0, mx)
            self.planes.append(buf)
        cb = 1 << self.l2cb
        self.min_cb_w, self.min_cb_h = w >> self.l2cb, (h + cb - 1) >> self.l2cb
        self.min_pu_w, self.min_pu_h = w >> self.l2pu, h >> self.l2pu
        ctb = 1 << self.l2ctb
        self.ctb_w, self.ctb_h = (w + ctb - 1) >> self.l2ctb, (h + ctb - 1) >> self.l2ctb
        self.bs_w, bs_h = w >> 3, h >> 3
        n = 2 * self.bs_w * (bs_h + 1)
        pick = np.array([0, 0, 1, 1, 1, 2, 2, 2], np.uint8)
        self.vbs, self.hbs = pick[r.randint(0, 7, n)], pick[r.randint(0, 7, n)]
        self.vbs[(h >> 2) * self.bs_w:] = 0          # no strength outside the picture (the decoder never sets one there)
        self.hbs[(h * self.bs_w) >> 2:] = 0
        # QP per min CB over the whole legal range of the bit depth: half of them where filters act, a quarter anywhere, a quarter at the tables' corners
        lo, ncb = QP_MIN[bd], self.min_cb_w * self.min_cb_h
        corners = np.array([lo, lo + 1, 0, 1, 14, 15, 16, 17, 18, 50, 51, 51])
        kind = r.randint(0, 3, ncb)
        self.qp = np.where(kind < 2, r.randint(20, 51, ncb), np.where(kind == 2, r.randint(lo, 51, ncb), corners[r.randint(0, len(corners) - 1, ncb)])).astype(np.int8)
        self.is_pcm = (r.uniform(self.min_pu_w * self.min_pu_h) < 0.2).astype(np.uint8)
        nctb = self.ctb_w * self.ctb_h
        self.db = np.zeros((nctb, 2), np.int32)     # slice_beta_offset_div2 / slice_tc_offset_div2 in -6 .. 6, doubled
        self.db[:, 0] = 2 * r.randint(-6, 6, nctb)
        self.db[:, 1] = 2 * r.randint(-6, 6, nctb)
        self.db[0] = (12, -12) if pic & 1 else (-12, 12)
        if nctb > 1:
            self.db[-1] = (-12, 12) if pic & 1 else (12, -12)

    def descriptor(self, ptr, planes=None):
        """ptr(array) -> address the backend can use (host address, or a device copy)"""
        planes = self.planes if planes is None else planes
        d = LfPicture()
        for c in range(3):
            d.data[c] = ptr(planes[c]) + planes[c].shape[1]      # skip the guard row
            d.linesize[c] = planes[c].shape[1]
        d.width, d.height, d.log2_ctb_size = self.w, self.h, self.l2ctb
        d.log2_min_cb_size, d.log2_min_pu_size = self.l2cb, self.l2pu
        d.min_cb_width, d.min_pu_width, d.min_pu_height = self.min_cb_w, self.min_pu_w, self.min_pu_h
        d.ctb_width, d.bs_width = self.ctb_w, self.bs_w
        d.vertical_bs, d.horizontal_bs, d.qp_y_tab, d.is_pcm, d.deblock = ptr(self.vbs), ptr(self.hbs), ptr(self.qp), ptr(self.is_pcm), ptr(self.db)
        d.pcmf, d.cb_qp_offset, d.cr_qp_offset = self.pcmf, self.cb_off, self.cr_off
        return d

    def plane_size(self, c):
        return (self.w, self.h) if c == 0 else (self.w // 2, self.h // 2)

    def typed(self, planes=None):
        """the three planes' samples as int64 arrays"""
        planes = self.planes if planes is None else planes
        return [samples(planes[c], *self.plane_size(c), self.bd).astype(np.int64) for c in range(3)]


def lf_launch(name):
    return [LfCase(name, i) for i in range(LF_SHAPES[name.rsplit("_", 1)[0]][5])]


def lf_host(fn, case, vertical_only=False):
    """fn(byref(descriptor), bit_depth) with host pointers on a copy of the case's planes; vertical_only: no horizontal strength anywhere"""
    planes = [p.copy() for p in case.planes]
    keep = []

    def ptr(a):
        if vertical_only and a is case.hbs:
            a = np.zeros_like(a)
        keep.append(a)
        return a.ctypes.data
    d = case.descriptor(ptr, planes)
    rc = fn(C.byref(d), case.bd)
    assert rc in (0, None), rc
    return planes


def lf_device(lib, cases):
    """mi355_hevc_deblock_pictures_dev on the launch's pictures: descriptors and every array on the device; returns each picture's three plane buffers"""
    d = Dev(lib)
    try:
        descs = (LfPicture * len(cases))()
        dev_planes = []
        for i, c in enumerate(cases):
            at = {}

            def ptr(a, at=at):
                at[id(a)] = d.up(a)
                return at[id(a)]
            C.memmove(C.byref(descs, i * C.sizeof(LfPicture)), C.byref(c.descriptor(ptr)), C.sizeof(LfPicture))
            dev_planes.append([at[id(pl)] for pl in c.planes])
        lib.mi355_hevc_deblock_pictures_dev.restype = C.c_int
        lib.mi355_hevc_deblock_pictures_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
        assert lib.mi355_hevc_deblock_pictures_dev(d.up_struct(descs), len(cases), cases[0].w, cases[0].h, cases[0].bd, None) == 0
        assert lib.mi355_sync(None) == 0
        return [[d.down(p, pl) for p, pl in zip(dev_planes[i], c.planes)] for i, c in enumerate(cases)]
    finally:
        d.free()


# ---- census of the deblocking decisions: a plain restatement of deblocking_filter_CTB's parameters and of the edge filters' decisions per 4-line half
def _clip(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def _luma_half(cnt, L, beta, tc, no_p, no_q, mx):
    """L[line][0..7] = p3 p2 p1 p0 q0 q1 q2 q3 of the half's four lines (already scaled beta / tc)"""
    if beta == 0:
        cnt["luma beta 0"] += 1
        return
    if tc == 0:
        cnt["luma tc 0, beta > 0"] += 1
    dp = [abs(int(L[l][1]) - 2 * int(L[l][2]) + int(L[l][3])) for l in (0, 3)]
    dq = [abs(int(L[l][6]) - 2 * int(L[l][5]) + int(L[l][4])) for l in (0, 3)]
    d0, d3 = dp[0] + dq[0], dp[1] + dq[1]
    if d0 + d3 >= beta:
        cnt["luma d >= beta"] += 1
        return
    tc25 = (tc * 5 + 1) >> 1
    strong = all(abs(int(L[l][0]) - int(L[l][3])) + abs(int(L[l][7]) - int(L[l][4])) < (beta >> 3) and abs(int(L[l][3]) - int(L[l][4])) < tc25 for l in (0, 3)) and \
        2 * d0 < (beta >> 2) and 2 * d3 < (beta >> 2)
    if strong:
        cnt["luma strong"] += 1
        clipped = False
        for l in range(4):
            p3, p2, p1, p0, q0, q1, q2, q3 = (int(v) for v in L[l])
            for cur, new in ((p0, (p2 + 2 * p1 + 2 * p0 + 2 * q0 + q1 + 4) >> 3), (p1, (p2 + p1 + p0 + q0 + 2) >> 2), (p2, (2 * p3 + 3 * p2 + p1 + p0 + q0 + 4) >> 3),
                             (q0, (p1 + 2 * p0 + 2 * q0 + 2 * q1 + q2 + 4) >> 3), (q1, (p0 + q0 + q1 + q2 + 2) >> 2), (q2, (2 * q3 + 3 * q2 + q1 + q0 + p0 + 4) >> 3)):
                clipped = clipped or abs(new - cur) > 2 * tc
        if clipped:
            cnt["luma strong, clipped at 2 tc"] += 1
        return
    thr = (beta + (beta >> 1)) >> 3
    dEp, dEq = int(dp[0] + dp[1] < thr), int(dq[0] + dq[1] < thr)
    cnt["luma normal dEp %d dEq %d" % (dEp, dEq)] += 1
    for l in range(4):
        p3, p2, p1, p0, q0, q1, q2, q3 = (int(v) for v in L[l])
        delta = (9 * (q0 - p0) - 3 * (q1 - p1) + 8) >> 4
        if abs(delta) >= 10 * tc:
            if tc:
                cnt["luma normal rejected, |delta| >= 10 tc"] += 1
            continue
        if delta > tc:
            cnt["luma delta clipped at +tc"] += 1
        if delta < -tc:
            cnt["luma delta clipped at -tc"] += 1
        delta = _clip(delta, -tc, tc)
        outs = []
        if not no_p:
            outs.append(p0 + delta)
            if dEp:
                s = (((p2 + p0 + 1) >> 1) - p1 + delta) >> 1
                if abs(s) > (tc >> 1):
                    cnt["luma p1 / q1 delta clipped at tc / 2"] += 1
                outs.append(p1 + _clip(s, -(tc >> 1), tc >> 1))
        if not no_q:
            outs.append(q0 - delta)
            if dEq:
                s = (((q2 + q0 + 1) >> 1) - q1 - delta) >> 1
                if abs(s) > (tc >> 1):
                    cnt["luma p1 / q1 delta clipped at tc / 2"] += 1
                outs.append(q1 + _clip(s, -(tc >> 1), tc >> 1))
        if any(v < 0 for v in outs):
            cnt["luma saturated at 0"] += 1
        if any(v > mx for v in outs):
            cnt["luma saturated at the maximum"] += 1


def lf_census(case, before, vfiltered):
    """Counter of the decision classes case's picture reaches: vertical edges on `before`, horizontal ones on `vfiltered` (typed() planes)"""
    cnt = collections.Counter()
    W, H, bd, sh = case.w, case.h, case.bd, case.bd - 8
    mx = (1 << bd) - 1

    def qpy(x, y):
        return int(case.qp[(x >> case.l2cb) + (y >> case.l2cb) * case.min_cb_w])

    def pcm(x, y):
        xp, yp = x >> case.l2pu, y >> case.l2pu
        if x < 0 or y < 0 or xp >= case.min_pu_w or yp >= case.min_pu_h:
            return 2
        return int(case.is_pcm[yp * case.min_pu_w + xp])

    def db(x, y):
        return case.db[(x >> case.l2ctb) + (y >> case.l2ctb) * case.ctb_w]

    def marks(tag, no_p, no_q):
        if no_p and no_q:
            cnt[tag + " no_p and no_q"] += 1
        elif no_p:
            cnt[tag + " no_p only"] += 1
        elif no_q:
            cnt[tag + " no_q only"] += 1

    for dirn, planes in ((0, before), (1, vfiltered)):
        Y = planes[0]
        for y in range(8 if dirn else 0, H, 8):
            for x in range(0 if dirn else 8, W, 8):
                if dirn:
                    bs = [int(case.hbs[(x + y * case.bs_w) >> 2]), int(case.hbs[(x + 4 + y * case.bs_w) >> 2])]
                else:
                    bs = [int(case.vbs[(x >> 3) + (y >> 2) * case.bs_w]), int(case.vbs[(x >> 3) + ((y + 4) >> 2) * case.bs_w])]
                for b in bs:
                    cnt["luma bS %d" % b] += 1
                if not bs[0] and not bs[1]:
                    continue
                if bs[0] != bs[1]:
                    cnt["luma halves differ in bS"] += 1
                beta_off, tc_off = (int(v) for v in db(x, y))
                qp = (qpy(x, y - 1) + qpy(x, y) + 1) >> 1 if dirn else (qpy(x - 1, y) + qpy(x, y) + 1) >> 1
                if qp < 0:
                    cnt["luma negative QP average"] += 1
                if dirn and (x >> case.l2ctb) != ((x + 8) >> case.l2ctb) and x + 8 < W:
                    cnt["luma horizontal segment 8 left of a CTB border"] += 1
                if (y if dirn else x) % (1 << case.l2ctb) == 0:
                    cnt["luma edge on a CTB border"] += 1
                bi = qp + beta_off
                cnt["luma beta index clipped at 0"] += bi < 0
                cnt["luma beta index clipped at 51"] += bi > 51
                beta = BETATABLE[_clip(bi, 0, 51)] << sh
                for j in range(2):
                    if not bs[j]:
                        continue
                    ti = qp + 2 * (bs[j] - 1) + (tc_off >> 1 << 1)
                    cnt["luma tc index clipped at 0"] += ti < 0
                    cnt["luma tc index clipped at 53"] += ti > 53
                    tc = TCTABLE[_clip(ti, 0, 53)] << sh
                    no_p = no_q = 0
                    if case.pcmf:
                        if dirn:
                            no_p, no_q = pcm(x + 4 * j, y - 1), pcm(x + 4 * j, y)
                        else:
                            no_p, no_q = pcm(x - 1, y + 4 * j), pcm(x, y + 4 * j)
                        marks("luma", no_p, no_q)
                    L = Y[y - 4:y + 4, x + 4 * j:x + 4 * j + 4].T if dirn else Y[y + 4 * j:y + 4 * j + 4, x - 4:x + 4]
                    _luma_half(cnt, L, beta, tc, no_p, no_q, mx)
        for c in (1, 2):
            tag = "cb" if c == 1 else "cr"
            P = planes[c]
            off = case.cb_off if c == 1 else case.cr_off
            for y in range(16 if dirn else 0, H, 16):
                for x in range(-8 if dirn else 16, W, 16):
                    pos = [(x, y), (x + 8, y)] if dirn else [(x, y), (x, y + 8)]
                    bs = []
                    for (hx, hy) in pos:
                        if dirn:
                            bs.append(0 if hx < 0 or hx >= W else int(case.hbs[(hx + hy * case.bs_w) >> 2]))
                        else:
                            bs.append(int(case.vbs[(hx >> 3) + (hy >> 2) * case.bs_w]))
                    if bs[0] != 2 and bs[1] != 2:
                        continue
                    if dirn and x < 0:
                        cnt[tag + " left half of a horizontal pair at x = -8"] += 1
                    if dirn and x + 8 >= W:
                        cnt[tag + " right half of a horizontal pair beyond the width"] += 1
                    for j, (hx, hy) in enumerate(pos):
                        if bs[j] != 2:
                            continue
                        qp = (qpy(hx, hy - 1) + qpy(hx, hy) + 1) >> 1 if dirn else (qpy(hx - 1, hy) + qpy(hx, hy) + 1) >> 1
                        tco = int(db(hx, hy)[1]) if dirn else int(db(x, y)[1])
                        qi = qp + off
                        cnt[tag + " qp_i clipped at 0"] += qi < 0
                        cnt[tag + " qp_i clipped at 57"] += qi > 57
                        qi = _clip(qi, 0, 57)
                        cnt[tag + (" qp_i below 30" if qi < 30 else (" qp_i above 43" if qi > 43 else " qp_i in 30..43"))] += 1
                        qpc = qi if qi < 30 else (qi - 6 if qi > 43 else QP_C[qi - 30])
                        tc = TCTABLE[_clip(qpc + 2 + tco, 0, 53)] << sh
                        no_p = no_q = 0
                        if case.pcmf:
                            no_p, no_q = (pcm(hx, hy - 1), pcm(hx, hy)) if dirn else (pcm(hx - 1, hy), pcm(hx, hy))
                            marks(tag, no_p, no_q)
                        if tc <= 0:
                            continue
                        cx, cy = hx >> 1, hy >> 1
                        L = P[cy - 2:cy + 2, cx:cx + 4].T if dirn else P[cy:cy + 4, cx - 2:cx + 2]
                        for l in range(4):
                            p1, p0, q0, q1 = (int(v) for v in L[l])
                            delta = (((q0 - p0) * 4) + p1 - q1 + 4) >> 3
                            cnt[tag + " delta clipped at +tc"] += delta > tc
                            cnt[tag + " delta clipped at -tc"] += delta < -tc
                            delta = _clip(delta, -tc, tc)
                            outs = ([] if no_p else [p0 + delta]) + ([] if no_q else [q0 - delta])
                            cnt[tag + " saturated at 0"] += any(v < 0 for v in outs)
                            cnt[tag + " saturated at the maximum"] += any(v > mx for v in outs)
    return cnt


LF_LUMA_CLASSES = ["luma bS 0", "luma bS 1", "luma bS 2", "luma beta 0", "luma d >= beta", "luma normal dEp 0 dEq 0", "luma normal dEp 0 dEq 1",
                   "luma normal dEp 1 dEq 0", "luma normal dEp 1 dEq 1", "luma normal rejected, |delta| >= 10 tc", "luma delta clipped at +tc",
                   "luma delta clipped at -tc", "luma p1 / q1 delta clipped at tc / 2", "luma strong", "luma strong, clipped at 2 tc", "luma tc 0, beta > 0",
                   "luma no_p only", "luma no_q only", "luma no_p and no_q", "luma saturated at 0", "luma saturated at the maximum",
                   "luma beta index clipped at 0", "luma beta index clipped at 51", "luma tc index clipped at 0", "luma tc index clipped at 53",
                   "luma halves differ in bS", "luma edge on a CTB border", "luma horizontal segment 8 left of a CTB border"]
LF_CHROMA_CLASSES = [t + s for t in ("cb", "cr") for s in (" qp_i below 30", " qp_i in 30..43", " qp_i above 43", " qp_i clipped at 0", " qp_i clipped at 57",
                                                           " delta clipped at +tc", " delta clipped at -tc", " no_p only", " no_q only", " no_p and no_q",
                                                           " left half of a horizontal pair at x = -8", " right half of a horizontal pair beyond the width",
                                                           " saturated at 0", " saturated at the maximum")]
# above 8 bits only: qp_y_tab legally holds QPs below 0 there
LF_DEEP_CLASSES = ["luma negative QP average"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 2. boundary-strength table
# name: (width, height, root block, log2_min_pu_size, log2_min_tb_size)
BS_CASES = {"t8x8": (8, 8, 8, 2, 2), "t40x24_p2t2": (40, 24, 32, 2, 2), "t72x56_p3t2": (72, 56, 32, 3, 2), "t104x88_p2t3": (104, 88, 64, 2, 3),
            "t160x96_p3t3": (160, 96, 64, 3, 3), "t144x80_p2t4": (144, 80, 32, 2, 4), "t112x96_p3t4": (112, 96, 64, 3, 4)}
BS_POCS = np.array([[8, 4, 8, 12, 4, 16, 8, 20, 12, 4, 24, 8, 16, 4, 28, 12],         # a POC repeats within a list and across the two
                    [8, 12, 4, 8, 16, 4, 20, 8, 4, 12, 8, 24, 4, 16, 12, 28]], np.int32)


class BsCase:
    def __init__(self, name):
        w, h, root, l2pu, l2tb = BS_CASES[name]
        r = SplitMix64(0xB57AB1E + list(BS_CASES).index(name))
        self.name, self.w, self.h, self.l2pu, self.l2tb = name, w, h, l2pu, l2tb
        cw, chh = w >> 2, h >> 2
        self.min_pu_w, min_pu_h = (w + (1 << l2pu) - 1) >> l2pu, (h + (1 << l2pu) - 1) >> l2pu
        self.min_tb_w, min_tb_h = (w + (1 << l2tb) - 1) >> l2tb, (h + (1 << l2tb) - 1) >> l2tb
        self.ref_poc = BS_POCS
        # ---- motion field per min PU: families of a base field and its near relations (a component moved by exactly 3 or 4, the two vectors swapped, another
        # index of the same POC, the other list's index of the same POC), a family per 16x16 region so that relations meet across edges
        def field(lists, idx, mv):
            f = np.zeros((), MVF_DT)
            f["pred_flag"] = lists
            f["ref_idx"] = tuple(i if l else -1 for i, l in zip(idx, lists))        # the unused list's index is -1, as the decoder leaves it
            f["mv"] = [m if l else (0, 0) for m, l in zip(mv, lists)]
            return f

        def same_poc(lst, i, other):
            """another index whose POC (in list `other`) equals list lst's POC at i"""
            c = [k for k in range(16) if BS_POCS[other][k] == BS_POCS[lst][i] and (other != lst or k != i)]
            return c[r.randint(0, len(c) - 1)] if c else i

        def moved(m, dx, dy):
            return (int(np.clip(m[0] + dx, -32768, 32767)), int(np.clip(m[1] + dy, -32768, 32767)))

        def family():
            ext = r.randint(0, 5) == 0
            comp = lambda: int(np.array([-32767, 32767, 32764, -32763])[r.randint(0, 3)]) if ext else r.randint(-40, 40)      # noqa: E731
            mv = [(comp(), comp()), (comp(), comp())]
            if r.randint(0, 3) == 0:
                mv[1] = mv[0] if r.randint(0, 1) else moved(mv[0], 3, 0)
            idx = (r.randint(0, 15), r.randint(0, 15))
            kind = r.randint(0, 5)
            lists = (1, 1) if kind < 3 else ((1, 0) if kind < 5 else (0, 1))
            if lists == (1, 1) and r.randint(0, 1):
                idx = (idx[0], same_poc(0, idx[0], 1))         # all four POCs equal once the neighbour shares them
            out = [field(lists, idx, mv)]
            for dx, dy in ((3, 0), (-3, 0), (4, 0), (-4, 0), (0, 3), (0, -3), (0, 4), (0, -4), (3, 3), (3, 4)):
                out.append(field(lists, idx, [moved(mv[0], dx, dy), mv[1]]))
                out.append(field(lists, idx, [mv[0], moved(mv[1], dx, dy)]))
                out.append(field(lists, idx, [moved(mv[0], dx, dy), moved(mv[1], -dx, -dy)]))
            if lists == (1, 1):
                sw = (same_poc(1, idx[1], 0), same_poc(0, idx[0], 1))
                for dx, dy in ((0, 0), (3, 0), (4, 0), (0, -4), (0, 3)):
                    out.append(field(lists, sw, [moved(mv[1], dx, dy), mv[0]]))       # crossed: L0 holds the other's L1 picture and vector
                    out.append(field(lists, sw, [mv[1], moved(mv[0], dx, dy)]))
                out.append(field(lists, (same_poc(0, idx[0], 0), idx[1]), mv))
                out.append(field((1, 0), idx, mv))
            else:
                lst = 0 if lists[0] else 1
                oi = [idx[0], idx[1]]
                oi[1 - lst] = same_poc(lst, idx[lst], 1 - lst)
                for dx, dy in ((0, 0), (3, 0), (0, 4)):
                    out.append(field((lists[1], lists[0]), tuple(oi), [moved(mv[1], dx, dy), moved(mv[0], dx, dy)]))     # the other list, same POC
                oi2 = [idx[0], idx[1]]
                oi2[lst] = same_poc(lst, idx[lst], lst)
                out.append(field(lists, tuple(oi2), mv))
                out.append(field(lists, ((idx[0] + 1) & 15, (idx[1] + 1) & 15), mv))
            intra = np.zeros((), MVF_DT)
            intra["is_intra"] = 1
            return out + [intra, intra]
        pu = 1 << l2pu
        mvf = np.zeros((min_pu_h, self.min_pu_w), MVF_DT)
        for y0 in range(0, h, 16):
            for x0 in range(0, w, 16):
                fam = family() if r.randint(0, 7) else family() + family()
                for y in range(y0, min(y0 + 16, h), pu):
                    for x in range(x0, min(x0 + 16, w), pu):
                        k = 0 if r.randint(0, 2) == 0 else r.randint(0, len(fam) - 1)
                        mvf[y >> l2pu, x >> l2pu] = fam[k]
        self.mvf = mvf
        self.cbf = (r.uniform((min_tb_h, self.min_tb_w)) < 0.25).astype(np.uint8)
        # ---- tiling into the blocks the reference calls the function for: down to the min TB; a block that crosses the picture's edge is split
        blocks = []

        def split(x0, y0, size):
            if x0 >= w or y0 >= h:
                return
            if size > (1 << l2tb) and (x0 + size > w or y0 + size > h or r.uniform() < (0.7 if size > 16 else 0.4)):
                hs = size // 2
                for dy in (0, hs):
                    for dx in (0, hs):
                        split(x0 + dx, y0 + dy, hs)
            else:
                assert x0 + size <= w and y0 + size <= h
                blocks.append((x0, y0, size.bit_length() - 1))
        for y0 in range(0, h, root):
            for x0 in range(0, w, root):
                split(x0, y0, root)
        self.blocks = np.array(blocks, np.int32)
        fl = np.zeros((chh, cw), np.uint8)
        for x0, y0, l2 in blocks:
            size = 1 << l2
            cx, cy, n = x0 >> 2, y0 >> 2, size >> 2
            if x0 > 0 and not (x0 & 7):
                fl[cy:cy + n, cx] |= L_BLOCK
            if y0 > 0 and not (y0 & 7):
                fl[cy, cx:cx + n] |= T_BLOCK
            if l2 > l2pu and not mvf[y0 >> l2pu, x0 >> l2pu]["is_intra"]:
                for j in range(8, size, 8):
                    fl[cy + (j >> 2), cx:cx + n] |= T_INNER
                    fl[cy:cy + n, cx + (j >> 2)] |= L_INNER
        self.flags = fl
        self.bs_w = w >> 3
        self.nbs = 2 * self.bs_w * ((h >> 3) + 1)

    def descriptor(self, ptr, vbs, hbs):
        d = BsPicture()
        d.width, d.height, d.log2_min_pu_size, d.log2_min_tb_size = self.w, self.h, self.l2pu, self.l2tb
        d.min_pu_width, d.min_tb_width, d.bs_width = self.min_pu_w, self.min_tb_w, self.bs_w
        d.tab_mvf, d.cbf_luma, d.edge_flags = ptr(self.mvf), ptr(self.cbf), ptr(self.flags)
        for l in range(2):
            for i in range(16):
                d.ref_poc[l][i] = int(self.ref_poc[l, i])
        d.vertical_bs, d.horizontal_bs = vbs, hbs
        return d


def bs_host(fn, c, with_blocks=False):
    v, h = np.zeros(c.nbs, np.uint8), np.zeros(c.nbs, np.uint8)
    keep = [np.ascontiguousarray(a) for a in (c.mvf, c.cbf, c.flags)]
    at = {id(a): k for a, k in zip((c.mvf, c.cbf, c.flags), keep)}
    d = c.descriptor(lambda a: at[id(a)].ctypes.data, v.ctypes.data, h.ctypes.data)
    if with_blocks:
        fn.restype = C.c_int
        assert fn(C.byref(d), C.c_void_p(c.blocks.ctypes.data), len(c.blocks)) == 0
    else:
        fn.restype = None
        fn(C.byref(d))
    return v, h


def bs_device(lib, c, npics=2):
    d = Dev(lib)
    try:
        descs = (BsPicture * npics)()
        outs = []
        for i in range(npics):
            dv, dh = d.up(np.full(c.nbs, 0xEE, np.uint8)), d.up(np.full(c.nbs, 0xEE, np.uint8))
            C.memmove(C.byref(descs, i * C.sizeof(BsPicture)), C.byref(c.descriptor(d.up, dv, dh)), C.sizeof(BsPicture))
            outs.append((dv, dh))
        lib.mi355_hevc_boundary_strengths_dev.restype = C.c_int
        lib.mi355_hevc_boundary_strengths_dev.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
        assert lib.mi355_hevc_boundary_strengths_dev(d.up_struct(descs), npics, c.w, c.h, None) == 0
        assert lib.mi355_sync(None) == 0
        like = np.zeros(c.nbs, np.uint8)
        return [(d.down(dv, like), d.down(dh, like)) for dv, dh in outs]
    finally:
        d.free()


def bs_grid_mask(c):
    mv, mh = np.zeros(c.nbs, bool), np.zeros(c.nbs, bool)
    for y in range(0, c.h, 4):
        for x in range(0, c.w, 8):
            mv[(x >> 3) + (y >> 2) * c.bs_w] = True
    for y in range(0, c.h, 8):
        for x in range(0, c.w, 4):
            mh[(x + y * c.bs_w) >> 2] = True
    return mv, mh


def bs_digest(c, v, h):
    mv, mh = bs_grid_mask(c)
    return hashlib.sha1(np.where(mv, v, 0).astype(np.uint8).tobytes() + np.where(mh, h, 0).astype(np.uint8).tobytes()).hexdigest()[:20]


def _bs_branch(c, cur, c_cbf, nb, n_cbf, tu_border, cnt):
    """boundary_strength restated; returns the strength and counts the branch taken"""
    def far(a, b):
        return abs(int(a[0]) - int(b[0])) >= 4 or abs(int(a[1]) - int(b[1])) >= 4

    def exact(a, b):
        dx, dy = abs(int(a[0]) - int(b[0])), abs(int(a[1]) - int(b[1]))
        for d, o, t in ((dx, dy, "x"), (dy, dx, "y")):
            if d in (3, 4) and o < 3:
                cnt["vector difference exactly %d in %s alone" % (d, t)] += 1
        if max(abs(int(v)) for v in tuple(a) + tuple(b)) == 32767:
            cnt["a component at +-32767"] += 1
    if tu_border:
        if cur["is_intra"] or nb["is_intra"]:
            cnt["intra on a block edge"] += 1
            return 2
        if c_cbf or n_cbf:
            cnt["cbf on a block edge"] += 1
            return 1
    elif cur["is_intra"] or nb["is_intra"]:
        cnt["intra on an inner edge (ignored)"] += 1
    mvs = int(cur["pred_flag"][0]) + int(cur["pred_flag"][1])
    if mvs != int(nb["pred_flag"][0]) + int(nb["pred_flag"][1]):
        cnt["differing vector counts"] += 1
        return 1
    poc = c.ref_poc
    if mvs == 2:
        c0, c1 = poc[0][cur["ref_idx"][0]], poc[1][cur["ref_idx"][1]]
        n0, n1 = poc[0][nb["ref_idx"][0]], poc[1][nb["ref_idx"][1]]
        if max(int(cur["ref_idx"][0]), int(cur["ref_idx"][1]), int(nb["ref_idx"][0]), int(nb["ref_idx"][1])) > 3:
            cnt["a reference index above 3"] += 1
        straight = far(nb["mv"][0], cur["mv"][0]) or far(nb["mv"][1], cur["mv"][1])
        crossed = far(nb["mv"][1], cur["mv"][0]) or far(nb["mv"][0], cur["mv"][1])
        if c0 == n0 and c0 == c1 and n0 == n1:
            cnt["bi, four POCs equal: straight %s, crossed %s" % ("far" if straight else "near", "far" if crossed else "near")] += 1
            return int(straight and crossed)
        if n0 == c0 and n1 == c1:
            cnt["bi straight, %s" % ("far" if straight else "near")] += 1
            exact(nb["mv"][0], cur["mv"][0])
            return int(straight)
        if n1 == c0 and n0 == c1:
            cnt["bi crossed, %s" % ("far" if crossed else "near")] += 1
            return int(crossed)
        cnt["bi neither"] += 1
        return 1
    if mvs == 0:
        return 0 if not far(cur["mv"][1], nb["mv"][1]) and poc[1][cur["ref_idx"][1]] == poc[1][nb["ref_idx"][1]] else 1        # two intra cells on an inner edge
    lc, ln = (0 if cur["pred_flag"][0] else 1), (0 if nb["pred_flag"][0] else 1)
    if max(int(cur["ref_idx"][lc]), int(nb["ref_idx"][ln])) > 3:
        cnt["a reference index above 3"] += 1
    if poc[lc][cur["ref_idx"][lc]] != poc[ln][nb["ref_idx"][ln]]:
        cnt["uni, different references"] += 1
        return 1
    if lc != ln:
        cnt["L0-only against L1-only, same POC"] += 1
    f = far(cur["mv"][lc], nb["mv"][ln])
    cnt["uni far" if f else "uni near"] += 1
    exact(cur["mv"][lc], nb["mv"][ln])
    return int(f)


def bs_census(c):
    """(vertical_bs, horizontal_bs, Counter) from the restatement: every marked cell side on the 8x8 grid"""
    cnt = collections.Counter()
    v, h = np.zeros(c.nbs, np.uint8), np.zeros(c.nbs, np.uint8)
    mvf = lambda x, y: c.mvf[y >> c.l2pu, x >> c.l2pu]      # noqa: E731
    cbf = lambda x, y: int(c.cbf[y >> c.l2tb, x >> c.l2tb])      # noqa: E731
    for y in range(0, c.h, 4):
        for x in range(0, c.w, 4):
            fl = int(c.flags[y >> 2, x >> 2])
            if not (x & 7) and x > 0 and fl & (L_BLOCK | L_INNER):
                v[(x >> 3) + (y >> 2) * c.bs_w] = _bs_branch(c, mvf(x, y), cbf(x, y), mvf(x - 1, y), cbf(x - 1, y), bool(fl & L_BLOCK), cnt)
            if not (y & 7) and y > 0 and fl & (T_BLOCK | T_INNER):
                h[(x + y * c.bs_w) >> 2] = _bs_branch(c, mvf(x, y), cbf(x, y), mvf(x, y - 1), cbf(x, y - 1), bool(fl & T_BLOCK), cnt)
    return v, h, cnt


BS_CLASSES = ["intra on a block edge", "intra on an inner edge (ignored)", "cbf on a block edge", "differing vector counts",
              "bi, four POCs equal: straight near, crossed near", "bi, four POCs equal: straight near, crossed far", "bi, four POCs equal: straight far, crossed near",
              "bi, four POCs equal: straight far, crossed far", "bi straight, near", "bi straight, far", "bi crossed, near", "bi crossed, far", "bi neither",
              "uni, different references", "uni near", "uni far", "L0-only against L1-only, same POC", "a reference index above 3", "a component at +-32767",
              "vector difference exactly 3 in x alone", "vector difference exactly 4 in x alone", "vector difference exactly 3 in y alone",
              "vector difference exactly 4 in y alone"]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 3. SAO table: 4 x 3 CTBs with a last column 8 luma samples wide (width % 16 == 8) and a last row 8 high, for each CTB size
SAO_SIZES = {4: (56, 40), 5: (104, 72), 6: (200, 136)}
SAO_BANDS = [0, 28, 29, 30, 31, 13, 7, 20]
SAO_OFFSETS = [(7, -7, 7, -7), (-7, 7, -7, 7), (15, -15, 15, -15), (-15, 15, -15, 15), (31, -31, 31, -31), (-31, 31, -31, 31), (1, 0, -2, 3), (-31, -15, 7, 31),
               (31, 15, -7, -31)]
SAO_ROTATIONS = 4          # pictures per row of the table: edge class (i + c + rotation) & 3 puts every class on every border CTB


class SaoCase:
    """a picture, per-CTB parameters and two slices (filtering across their edge on in one, off in the other)"""

    def __init__(self, bd, log2_ctb, rot, size=None):
        r = SplitMix64(0x5A07AB1E + 100 * bd + 10 * log2_ctb + rot)
        self.bd, self.log2_ctb, self.rot = bd, log2_ctb, rot
        self.W, self.H = size or SAO_SIZES[log2_ctb]
        W, H, mx = self.W, self.H, (1 << bd) - 1
        ctb = 1 << log2_ctb
        self.cw, self.chn = -(-W // ctb), -(-H // ctb)
        self.src = []
        for c in range(3):
            pw, ph = W >> (c > 0), H >> (c > 0)
            yy, xx = np.mgrid[0:ph, 0:pw]
            a = mx // 2 + ((xx * 5 + yy * 3) % (mx // 3)) + r.randint(-3, 3, (ph, pw))
            a = np.where(r.uniform((ph, pw)) < 0.3, r.randint(0, mx, (ph, pw)), a)
            # content holding 0 and the maximum next to the offsets that push past them
            ends = np.kron(r.randint(0, 5, ((ph + 7) // 8, (pw + 7) // 8)), np.ones((8, 8), np.int64))[:ph, :pw]
            a = np.where(ends == 0, r.randint(0, 3, (ph, pw)), np.where(ends == 1, mx - r.randint(0, 3, (ph, pw)), a))
            buf = new_plane(pw, ph, bd)
            samples(buf, pw, ph, bd)[:] = np.clip(a, 0, mx)
            self.src.append(buf)
        n = self.cw * self.chn
        self.params, nband = [], 0
        for i in range(n):
            t = [[2, 1, 2, 2, 0, 1][(i + c + rot) % 6] for c in range(3)]
            if i % self.cw in (0, self.cw - 1) or i // self.cw in (0, self.chn - 1):      # on the picture's border: edge offset, but for one in five
                corner = i in (0, self.cw - 1, n - self.cw, n - 1)
                t = [2 if corner or (i + c + rot) % 5 else t[c] for c in range(3)]
            band = []
            for c in range(3):
                band.append(SAO_BANDS[(nband + rot) % len(SAO_BANDS)])
                nband += t[c] == 1
            self.params.append(dict(type=t, off=[[0] + list(SAO_OFFSETS[(i + 2 * c + 3 * rot) % len(SAO_OFFSETS)]) for c in range(3)], band=band,
                                    eo=[(i + c + rot) & 3 for c in range(3)]))
        first2 = r.randint(1, n - 1)
        self.slice_addr = [0 if i < first2 else first2 for i in range(n)]
        across = rot & 1
        self.filter_edges = [1 if i < first2 else across for i in range(n)]


def sao_expected(oracle, bd, src, W, H, log2_ctb, params, slice_addr, filter_edges):
    """sao_filter_CTB restated over the oracle's table functions (hevc_batch._check_sao_ctbs' formulation) on plane buffers of new_plane()'s layout:
    returns the expected output buffers (poison where nothing is written) and the jobs of mi355_hevc_sao_ctbs_dev as (plane, byte offset of dst / src, job)"""
    px, ctb = px_of(bd), 1 << log2_ctb
    cw, chn = -(-W // ctb), -(-H // ctb)
    c_o = oracle.hevcdsp(bd)
    exp = [np.full_like(s, POISON) for s in src]
    owner = {}
    for cy in range(chn):
        for cx in range(cw):
            pieces, borders = sao_ctb_pieces(cx, cy, cw, chn, params, slice_addr, filter_edges)
            bo = np.array(borders, np.int32)
            for c in range(3):
                sh = 1 if c else 0
                size_c = ctb >> sh
                x0, y0 = cx * size_c, cy * size_c
                w, h = min(size_c, (W >> sh) - x0), min(size_c, (H >> sh) - y0)
                s_t, d_t = samples(src[c], W >> sh, H >> sh, bd), samples(exp[c], W >> sh, H >> sh, bd)
                stride = src[c].shape[1]
                xs, ys = (0 if borders[0] else 8 >> sh), (0 if borders[1] else 4 >> sh)
                cwid, chgt = (w + xs if borders[2] else w), (h + ys if borders[3] else h)
                d_t[y0 - ys:y0 - ys + chgt, x0 - xs:x0 - xs + cwid] = s_t[y0 - ys:y0 - ys + chgt, x0 - xs:x0 - xs + cwid]      # copy_CTB
                off = (y0 + 1) * stride + x0 * px
                for (k, p, ve, he, de) in pieces:
                    ox, oy = cx - (k >> 1), cy - (k & 1)
                    owner.setdefault((oy, ox, c), []).append(dict(cls=k, p=p, ve=ve, he=he, de=de, borders=borders, dx=(k >> 1) * size_c, dy=(k & 1) * size_c, w=w, h=h))
                    if p["type"][c] == 0:
                        continue
                    sao = A.SAOParams()
                    for i in range(5):
                        sao.offset_val[c][i] = p["off"][c][i]
                    sao.band_position[c], sao.eo_class[c] = p["band"][c], p["eo"][c]
                    dp, sp = C.cast(exp[c].ctypes.data + off, A.u8p), C.cast(src[c].ctypes.data + off, A.u8p)
                    if p["type"][c] == 2:
                        c_o.sao_edge_filter[k](dp, sp, stride, C.byref(sao), C.cast(bo.ctypes.data, A.intp), w, h, c, ve, he, de)
                    else:
                        c_o.sao_band_filter[k](dp, sp, stride, C.byref(sao), C.cast(bo.ctypes.data, A.intp), w, h, c)
    jobs = []
    for (oy, ox, c), pcs in sorted(owner.items()):
        size_c = ctb >> (1 if c else 0)
        stride = src[c].shape[1]
        j = SaoCtbJob(0, 0, stride)
        j.c_idx, j.npieces = c, len(pcs)
        for n, m in enumerate(pcs):
            q, p = j.piece[n], m["p"]
            q.cls, q.type, q.eo_class, q.band_position, q.vert_edge, q.horiz_edge, q.diag_edge = m["cls"], p["type"][c], p["eo"][c], p["band"][c], m["ve"], m["he"], m["de"]
            q.borders = sum(b << e for e, b in enumerate(m["borders"]))
            q.dx, q.dy, q.width, q.height = m["dx"], m["dy"], m["w"], m["h"]
            for i in range(5):
                q.offset_val[i] = p["off"][c][i]
        jobs.append((c, oy, ox, (oy * size_c + 1) * stride + ox * size_c * px, j))
    return exp, jobs


def sao_device(lib, bd, src, jobs):
    """mi355_hevc_sao_ctbs_dev from `src` into poisoned output buffers; returns them"""
    d = Dev(lib)
    try:
        p_src, p_dst = [d.up(s) for s in src], [d.up(np.full_like(s, POISON)) for s in src]
        arr = []
        for c, _, _, off, j in jobs:
            k = SaoCtbJob.from_buffer_copy(j)
            k.dst, k.src = p_dst[c] + off, p_src[c] + off
            arr.append(k)
        lib.mi355_hevc_sao_ctbs_dev.restype = C.c_int
        assert lib.mi355_hevc_sao_ctbs_dev(C.c_void_p(d.up_jobs(arr)), len(arr), bd, None) == 0
        assert lib.mi355_sync(None) == 0
        return [d.down(p_dst[c], src[c]) for c in range(3)]
    finally:
        d.free()


def sao_census(case):
    """what the case's parameters and samples reach, from the unfiltered source planes (numpy only)"""
    cnt = collections.Counter()
    bd, mx, ctb = case.bd, (1 << case.bd) - 1, 1 << case.log2_ctb
    for i, p in enumerate(case.params):
        cx, cy = i % case.cw, i // case.cw
        for c in range(3):
            sh = 1 if c else 0
            sz, pw, ph = ctb >> sh, case.W >> sh, case.H >> sh
            S = samples(case.src[c], pw, ph, bd).astype(np.int64)
            x0, y0 = cx * sz, cy * sz
            x1, y1 = min(x0 + sz, pw), min(y0 + sz, ph)
            t = p["type"][c]
            cnt["type %d, component %d" % (t, c)] += 1
            off = np.array(p["off"][c])
            for v in (7, 15, 31):
                if t and v in off and -v in off:
                    cnt["offsets +-%d" % v] += 1
            if t == 1:
                bp = p["band"][c]
                cnt["band position %d" % bp] += 1
                k = ((S[y0:y1, x0:x1] >> (bd - 5)) - bp) & 31
                hit = k < 4
                cnt["band hit"] += int(hit.any())
                cnt["band miss"] += int((~hit).any())
                cnt["wrapped band"] += int((hit & ((S[y0:y1, x0:x1] >> (bd - 5)) < bp)).any())
                new = S[y0:y1, x0:x1] + np.where(hit, off[1:][np.minimum(k, 3)], 0)
                cnt["clip low"] += int((new < 0).any())
                cnt["clip high"] += int((new > mx).any())
            if t == 2:
                eo = p["eo"][c]
                for name, on in (("left", cx == 0), ("top", cy == 0), ("right", cx == case.cw - 1), ("bottom", cy == case.chn - 1)):
                    if on:
                        cnt["eo_class %d on the %s border" % (eo, name)] += 1
                for name, on in (("top-left", cx == 0 and cy == 0), ("top-right", cx == case.cw - 1 and cy == 0), ("bottom-left", cx == 0 and cy == case.chn - 1),
                                 ("bottom-right", cx == case.cw - 1 and cy == case.chn - 1)):
                    if on:
                        cnt["eo_class %d in the %s corner" % (eo, name)] += 1
                dx, dy = [(-1, 0), (0, -1), (-1, -1), (1, -1)][eo]
                ys, xs = np.mgrid[max(y0, 1):min(y1, ph - 1), max(x0, 1):min(x1, pw - 1)]
                cat = 2 + np.sign(S[ys, xs] - S[ys + dy, xs + dx]) + np.sign(S[ys, xs] - S[ys - dy, xs - dx])
                edge_idx = np.array([1, 2, 0, 3, 4])
                for k in range(5):
                    cnt["edge category %d" % k] += int((cat == k).any())
                new = S[ys, xs] + off[edge_idx[cat]]
                cnt["clip low"] += int((new < 0).any())
                cnt["clip high"] += int((new > mx).any())
    return cnt


SAO_CLASSES = (["type %d, component %d" % (t, c) for t in range(3) for c in range(3)] + ["offsets +-%d" % v for v in (7, 15, 31)] +
               ["band position %d" % b for b in (0, 28, 29, 30, 31)] + ["band hit", "band miss", "wrapped band", "clip low", "clip high"] +
               ["edge category %d" % k for k in range(5)] + ["eo_class %d on the %s border" % (e, b) for e in range(4) for b in ("left", "top", "right", "bottom")] +
               ["eo_class %d in the %s corner" % (e, b) for e in range(4) for b in ("top-left", "top-right", "bottom-left", "bottom-right")])


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# 4. fused filter table: the deblocking table's pictures, every component of every CTB with a SAO job of the whole-region forms
class FilterCtbJob(C.Structure):
    _fields_ = [("pic", C.c_int32), ("x0", C.c_uint16), ("y0", C.c_uint16), ("sao", C.c_uint32 * 3)]


assert C.sizeof(FilterCtbJob) == 20
ERR_FILTER_CTB_FORM, E_DEVICE_FAULT = 4, -5
FUSED_CASES = [n for n in LF_CASES if not n.startswith(("w8", "h8"))] + ["w8_9", "h8_10"]


def fused_params(case):
    """one slice, filtering across everything: per CTB and component a type, offsets within a signed byte.  A chroma region 4 samples wide (the last CTB column of a
    picture whose width is 8 above a multiple of the CTB) is one the fused entry point takes as a copy only (include/mi355_hevc_batch.h): SAO off there."""
    r = SplitMix64(0xF05ED + 7 * LF_CASES.index(case.name) + case.pic)
    ctb = 1 << case.l2ctb
    out = []
    for i in range(case.ctb_w * case.ctb_h):
        cx = i % case.ctb_w
        t = [[2, 1, 2, 0, 1, 2][(i + c + case.pic) % 6] for c in range(3)]
        for c in (1, 2):
            if (min(ctb, case.w - cx * ctb) >> 1) & 7:
                t[c] = 0
        out.append(dict(type=t, off=[[0] + list(SAO_OFFSETS[r.randint(0, len(SAO_OFFSETS) - 1)]) for _ in range(3)],
                        band=[SAO_BANDS[r.randint(0, len(SAO_BANDS) - 1)] for _ in range(3)], eo=[(i + c) & 3 for c in range(3)]))
    return out


def fused_expected(oracle, case, deblocked, params):
    n = case.ctb_w * case.ctb_h
    return sao_expected(oracle, case.bd, deblocked, case.w, case.h, case.l2ctb, params, [0] * n, [1] * n)


def fused_device(lib, cases, jobs_per_pic, expect_fault=False):
    """mi355_hevc_filter_ctbs_dev on the launch's pictures: returns (outputs per picture, reconstruction surfaces afterwards, mi355_sync's result)"""
    d = Dev(lib)
    try:
        descs = (LfPicture * len(cases))()
        rec, outp, ctbs, sao = [], [], [], []
        for i, c in enumerate(cases):
            at = {}

            def ptr(a, at=at):
                at[id(a)] = d.up(a)
                return at[id(a)]
            C.memmove(C.byref(descs, i * C.sizeof(LfPicture)), C.byref(c.descriptor(ptr)), C.sizeof(LfPicture))
            rec.append([at[id(pl)] for pl in c.planes])
            outp.append([d.up(np.full_like(pl, POISON)) for pl in c.planes])
            index = {}
            for comp, oy, ox, off, j in jobs_per_pic[i]:
                k = SaoCtbJob.from_buffer_copy(j)
                k.dst, k.src = outp[i][comp] + off, 0
                index[(oy, ox, comp)] = len(sao)
                sao.append(k)
            for oy in range(c.ctb_h):
                for ox in range(c.ctb_w):
                    f = FilterCtbJob(i, ox << c.l2ctb, oy << c.l2ctb)
                    for comp in range(3):
                        f.sao[comp] = index[(oy, ox, comp)]
                    ctbs.append(f)
        lib.mi355_hevc_filter_ctbs_dev.restype = C.c_int
        lib.mi355_hevc_filter_ctbs_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        assert lib.mi355_hevc_filter_ctbs_dev(d.up_struct(descs), d.up_jobs(ctbs), len(ctbs), d.up_jobs(sao), cases[0].l2ctb, cases[0].bd, None) == 0
        rc = lib.mi355_sync(None)
        return ([[d.down(p, pl) for p, pl in zip(outp[i], c.planes)] for i, c in enumerate(cases)],
                [[d.down(p, pl) for p, pl in zip(rec[i], c.planes)] for i, c in enumerate(cases)], rc)
    finally:
        d.free()


def region_mask(case, comp, oy, ox):
    """the bytes of component comp's output buffer that CTB (ox, oy)'s job writes"""
    pw, ph = case.plane_size(comp)
    sz, px = (1 << case.l2ctb) >> (comp > 0), px_of(case.bd)
    m = np.zeros_like(case.planes[comp], bool)
    m[1 + oy * sz:1 + min((oy + 1) * sz, ph), ox * sz * px:min((ox + 1) * sz, pw) * px] = True
    return m


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the checks a backend (emulator, GPU) goes through; `gold` = tests/golden/hevc_filter_tables_sha1.json
def _oracle_deblock(oracle):
    oracle.lib.oracle_hevc_deblock_picture.restype = None
    return oracle.lib.oracle_hevc_deblock_picture


def check_deblock(prov, oracle, name, gold):
    """the product equals the oracle and the recorded digest for every picture of the launch, guard rows and row padding (poisoned) included"""
    cases = lf_launch(name)
    outs = lf_device(prov.lib, cases)
    for case, got in zip(cases, outs):
        want = lf_host(_oracle_deblock(oracle), case)
        for c in range(3):
            assert np.array_equal(want[c], got[c]), "%s picture %d: plane %d differs (%d bytes)" % (name, case.pic, c, int((want[c] != got[c]).sum()))
            assert outside_is_poison(got[c], *case.plane_size(c), case.bd), "%s picture %d: plane %d written outside the picture" % (name, case.pic, c)
        assert digest(got) == gold["deblock"][name][case.pic]


def check_bs(prov, oracle, name, gold, npics=2):
    c = BsCase(name)
    ov, oh = bs_host(oracle.lib.oracle_hevc_boundary_strengths, c)
    mv, mh = bs_grid_mask(c)
    for v, h in bs_device(prov.lib, c, npics):
        assert np.array_equal(v[mv], ov[mv]) and np.array_equal(h[mh], oh[mh]), name
        assert (v[~mv] == 0xEE).all() and (h[~mh] == 0xEE).all()          # nothing outside the grid entries is written
        assert bs_digest(c, v, h) == gold["bs"][name]


def check_sao(prov, oracle, bd, log2_ctb):
    for rot in range(SAO_ROTATIONS):
        case = SaoCase(bd, log2_ctb, rot)
        exp, jobs = sao_expected(oracle, bd, case.src, case.W, case.H, log2_ctb, case.params, case.slice_addr, case.filter_edges)
        got = sao_device(prov.lib, bd, case.src, jobs)
        for c in range(3):
            assert np.array_equal(got[c], exp[c]), "SAO differs in plane %d (bd %d, CTB %d, rotation %d: %d bytes)" % (c, bd, 1 << log2_ctb, rot, int((got[c] != exp[c]).sum()))
            assert outside_is_poison(got[c], case.W >> (c > 0), case.H >> (c > 0), bd)


def check_fused(prov, oracle, name):
    """mi355_hevc_filter_ctbs_dev against (1) the oracle's deblocked picture through the oracle's SAO functions and (2) the product's own two separate entry points;
    the reconstruction is only read"""
    cases = lf_launch(name)
    params = [fused_params(c) for c in cases]
    sep_deblocked = lf_device(prov.lib, cases)
    jobs, want, sep = [], [], []
    for case, p, dev_db in zip(cases, params, sep_deblocked):
        exp, j = fused_expected(oracle, case, lf_host(_oracle_deblock(oracle), case), p)
        jobs.append(j)
        want.append(exp)
        sep.append(sao_device(prov.lib, case.bd, dev_db, j))
    outs, rec, rc = fused_device(prov.lib, cases, jobs)
    assert rc == 0
    for i, case in enumerate(cases):
        for c in range(3):
            assert np.array_equal(rec[i][c], case.planes[c]), "%s picture %d: the reconstruction's plane %d was written" % (name, i, c)
            assert np.array_equal(outs[i][c], want[i][c]), "%s picture %d: plane %d differs from the oracle (%d bytes)" % (name, i, c, int((outs[i][c] != want[i][c]).sum()))
            assert np.array_equal(outs[i][c], sep[i][c]), "%s picture %d: plane %d differs from the separate entry points" % (name, i, c)


REFUSED_FORMS = ("pieces of differing types", "an edge-offset job with a restored edge", "an offset outside a signed byte", "a band-offset region 4 samples wide",
                 "an edge-offset region 4 samples wide")


def check_fused_refusal(prov, oracle, form):
    """one job of a form the fused entry point does not take (include/mi355_hevc_batch.h): that component's region of the poisoned output stays unwritten, every
    other region is right, mi355_sync reports the device fault with MI355_ERR_FILTER_CTB_FORM, and mi355_error_word_take() clears the word for the next call"""
    case = LfCase("r104_9")                         # 4 x 3 CTBs of 32 x 32, the last column 8 luma / 4 chroma samples wide
    params = fused_params(case)
    prov.lib.mi355_error_word_take.restype = C.c_uint
    assert prov.lib.mi355_error_word_take() == 0
    # the victim: an interior CTB's luma job of more than one piece ... or a chroma job of the last column
    oy, ox, comp = 1, 1, 0
    if form.endswith("4 samples wide"):
        oy, ox, comp = 1, case.ctb_w - 1, 2
        params[oy * case.ctb_w + ox]["type"][comp] = 1 if form.startswith("a band") else 2
    elif form == "an offset outside a signed byte":
        params[oy * case.ctb_w + ox]["type"][comp] = 1
        params[oy * case.ctb_w + ox]["off"][comp] = [0, 7, -129, 3, 128]
    else:
        params[oy * case.ctb_w + ox]["type"][comp] = 2
    exp, jobs = fused_expected(oracle, case, lf_host(_oracle_deblock(oracle), case), params)
    victim = [j for (c, y, x, _, j) in jobs if (c, y, x) == (comp, oy, ox)][0]
    if form == "pieces of differing types":
        assert victim.npieces > 1
        victim.piece[1].type = 1
    elif form == "an edge-offset job with a restored edge":
        victim.piece[victim.npieces - 1].horiz_edge = 1
    outs, rec, rc = fused_device(prov.lib, [case], [jobs])
    assert rc == E_DEVICE_FAULT
    assert prov.lib.mi355_error_word_take() == ERR_FILTER_CTB_FORM
    assert prov.lib.mi355_error_word_take() == 0 and prov.lib.mi355_sync(None) == 0
    for c in range(3):
        m = region_mask(case, comp, oy, ox) if c == comp else np.zeros_like(exp[c], bool)
        assert m.any() == (c == comp)
        assert (outs[0][c][m] == POISON).all(), "%s: the refused region was written" % form
        assert np.array_equal(outs[0][c][~m], exp[c][~m]), "%s: plane %d differs outside the refused region" % (form, c)
        assert np.array_equal(rec[0][c], case.planes[c])
