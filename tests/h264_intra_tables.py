"""Directed tables for the intra half of the H.264 frame path (k_recon_intra, k_recon_intra_all, k_wide_intra and the predictors of h264_dev.h):
  A  every availability class (left, above, above-left, above-right: sixteen) times every mode the class leaves legal, for Intra 4x4, Intra 8x8 and Intra16x16 + chroma,
     the neighbours a class declares absent holding poison in two variants (table_a);
  B  extremes: the plane predictors' H / V sums at their bounds and the packed clip, every DC form at 0, at the maximum and around its rounding step, the (1, 2, 1) taps
     on the alternating edge (table_b_plane, table_b_dc, table_b_taps);
  C  the eleven chroma slots on plain and extreme edges, Cb and Cr different (table_c);
  D  chains of intra macroblocks whose every link has exactly ONE intra neighbour — left, above-left, above or above-right — for the single launch's waits (chain_set).
Test macroblocks sit at odd (x, y) of a grid of carriers: I_PCM macroblocks, or 16x16 inter macroblocks with a zero vector on a designed reference.  The left column, the row
above, the corner and the eight samples above-right that a test macroblock can read are samples of its own (the carrier above-right of one test macroblock is above-left of the
next, but the two read different samples of it).  Everything is built from fixed seeds AT the set's bit depth; every picture is compared with the frame-level oracle sample
for sample.  The tables never compute an expected sample: what they restate (legal modes, the plane sums, the DC sums) is for the census alone."""
import copy

import numpy as np

import h264_frames as HF
import h264_run_tables as RT
from rng import SplitMix64

FORMATS = ((8, 1), (9, 1), (10, 1), (10, 2))          # (bit depth, chroma_format_idc) the frame-level checkers bind (no 8-bit 4:2:2: oracle_h264frame_hbd_bind_cf takes 9 / 10)
VERT, HOR, DC, DDL, DDR, VR, HD, VL, HU, LEFT_DC, TOP_DC, DC_128 = range(12)
C_DC, C_HOR, C_VERT, C_PLANE, C_LEFT_DC, C_TOP_DC, C_DC128, C_L0T, C_0LT, C_L00, C_0L0 = range(11)
REACH4 = (0, 1, 4, 5, 2, 8, 10)                         # Intra 4x4 blocks in the top row and the left column
GRID_W, GRID_H = 19, 9                                  # 9 x 4 test macroblocks; all carriers I_PCM: 19 + 2 * 8 = 35 levels


def luma_cands(btop, bleft, btl):
    """what the reference's checks leave for a block (ff_h264_check_intra4x4_pred_mode's remaps, h264_parse.c; the down-right modes need the corner)"""
    if btop and bleft:
        return [VERT, HOR, DC, DDL, VL, HU] + ([DDR, VR, HD] if btl else [])
    if bleft:
        return [HOR, HU, LEFT_DC]
    if btop:
        return [VERT, DDL, VL, TOP_DC]
    return [DC_128]


def mb_cands(left, top, tl):
    """Intra16x16 / chroma slots (ff_h264_check_intra_pred_mode): plane needs every neighbour it reads"""
    if left and top:
        return [C_DC, C_HOR, C_VERT] + ([C_PLANE] if tl else [])
    if left:
        return [C_HOR, C_LEFT_DC]
    if top:
        return [C_VERT, C_TOP_DC]
    return [C_DC128]


def block_avail(i, left, top, tlm):
    x4, y4 = HF.blk_xy(i)
    return bool(top or y4 > 0), bool(left or x4 > 0), bool((tlm << i) & 0x8000)


def rec_class(rec):
    """(left, above, above-left, above-right) as the record's masks state them"""
    tlm, trm = int(rec["topleft"]), int(rec["topright"])
    return bool(tlm & 0x2000), bool(tlm & 0x4000), bool(tlm & 0x8000), bool(trm & 0x0400)


# ---- pictures: a canvas of carrier samples at the set's depth, test macroblocks on odd (x, y) ----
class Canvas:
    def __init__(self, r, mb_w, mb_h, depth, idc):
        self.depth, self.idc, self.maxv, self.ch = depth, idc, (1 << depth) - 1, 8 * idc
        self.pl = [r.randint(0, self.maxv, (16 * mb_h, 16 * mb_w)), r.randint(0, self.maxv, (self.ch * mb_h, 8 * mb_w)), r.randint(0, self.maxv, (self.ch * mb_h, 8 * mb_w))]

    def region(self, p, x, y, name):
        """index of a test macroblock's neighbour samples in plane p: 'top', 'left', 'tl', 'tr' (luma: eight samples)"""
        n, h = (16, 16) if p == 0 else (8, self.ch)
        return {"top": (h * y - 1, slice(n * x, n * x + n)), "tr": (h * y - 1, slice(n * x + n, n * x + n + 8)), "tl": (h * y - 1, n * x - 1),
                "left": (slice(h * y, h * y + h), n * x - 1)}[name]

    def mb_samples(self, x, y):
        c = self.ch
        return np.concatenate([self.pl[0][16 * y:16 * y + 16, 16 * x:16 * x + 16].reshape(-1)] + [self.pl[p][c * y:c * y + c, 8 * x:8 * x + 8].reshape(-1) for p in (1, 2)])

    def planes(self):
        return tuple(np.ascontiguousarray(a, np.uint8 if self.depth == 8 and self.idc == 1 else np.uint16) for a in self.pl)


def poison(n, variant, depth):
    """P (variant 0) lies below the mid value, Q = P + mid above it: they differ in every sample and neither is the mid value"""
    mid = 1 << (depth - 1)
    return 1 + (np.arange(n) * 37 + 11) % (mid - 2) + (mid if variant else 0)


def new_set(canvases, mb_w, mb_h, depth, idc):
    fs = RT.new_set(len(canvases), mb_w, mb_h, [[c.planes()] for c in canvases])
    fs.depth, fs.idc, fs.canvases, fs.tests = depth, idc, canvases, []
    if (depth, idc) != (8, 1):
        fs.native = (depth, idc)
        fs.pcm_samples = np.zeros((fs.F, mb_w * mb_h, 256 + 128 * idc), np.int32)
    return fs


def put_pcm(fs, f, m):
    rec = fs.mb[f, m]
    v = fs.canvases[f].mb_samples(m % fs.mb_w, m // fs.mb_w)
    if hasattr(fs, "native"):
        fs.pcm_samples[f, m] = v
    else:
        fs.coef[f, m].view(np.uint8)[:384] = v
    rec["mb_type"], rec["qp"], rec["qpc"], rec["cbp"], rec["nnz_mask"], rec["ref_idx"] = HF.PCM, 0, (HF.CHROMA_QP[0],) * 2, 0x2F, 0xFFFFFF, -1


def put_carrier(fs, f, m, pcm):
    if pcm:
        put_pcm(fs, f, m)
    else:
        RT.put_inter(fs, f, m, 0, [{0: (0, (0, 0))}])


def intra_resid(r, kind, luma_blocks, chroma):
    """a few coded blocks: 4x4 blocks `luma_blocks` (Intra 8x8: quadrants), Intra16x16 DC levels with them; chroma 0 none, 1 DC, 2 DC + AC"""
    cf = np.zeros(384, np.int16)
    for b in luma_blocks:
        if kind == "i8":
            k = r.randint(1, 12)
            cf[64 * b + r.randint(0, 63, k)] = r.laplace_int(24, k, 2047)
            cf[64 * b] = cf[64 * b] or 40
        else:
            k = r.randint(1, 6)
            cf[16 * b + np.array(HF.ZIGZAG4)[:k]] = r.laplace_int(24, k, 2047)
            cf[16 * b + 1] = cf[16 * b + 1] or 33
            if kind == "i16":
                cf[16 * b] = 0
    if kind == "i16" and luma_blocks:
        lv = r.laplace_int(40, 16, 2047)
        for k in range(16):
            cf[HF.luma_dc_slot(k)] = lv[k]
        cf[0] = cf[0] or 21
    if chroma:
        cf[256:384:16] = r.laplace_int(30, 8, 2047)
        cf[256], cf[320] = cf[256] or 5, cf[320] or -7
        if chroma == 2:
            for j in (1, 6):
                cf[256 + 16 * j + 1], cf[256 + 16 * j + 4] = r.randint(20, 90), -r.randint(20, 90)
    return cf


def put_intra(fs, f, m, spec):
    """a test macroblock: its record, its coefficients and the masks that follow from them (hl_decode_mb's view: nnz per block, cbp, the DC bits)"""
    rec = fs.mb[f, m]
    left, top, tl, tr = spec["cls"]
    rec["topleft"], rec["topright"] = HF._avail_masks(top, left, tl, tr)
    kind = spec["kind"]
    rec["mb_type"] = HF.I16 if kind == "i16" else (HF.I4 | (HF.DCT8 if kind == "i8" else 0))
    rec["i16mode"], rec["chroma_mode"], rec["ref_idx"] = spec.get("i16mode", 0), spec["cmode"], -1
    rec["i4mode"] = spec.get("modes", [0] * 16)
    cf = spec.get("resid")
    if cf is None:
        return
    fs.coef[f, m] = cf
    mask = 0
    for i in range(16):
        blk = cf[16 * i:16 * i + 16]
        if kind == "i8":
            mask |= (1 << i) if cf[64 * (i >> 2):64 * (i >> 2) + 64].any() else 0
        elif kind == "i16":
            mask |= (1 << i) if blk[1:].any() else 0
        else:
            mask |= (1 << i) if blk.any() else 0
    if kind == "i16" and cf[[HF.luma_dc_slot(k) for k in range(16)]].any():
        mask |= 1 << 24
    ac = False
    for j in range(8):
        if cf[256 + 16 * j + 1:256 + 16 * j + 16].any():
            mask |= 1 << (16 + j)
            ac = True
    dcs = cf[256:384:16]
    mask |= (1 << 25 if dcs[:4].any() else 0) | (1 << 26 if dcs[4:].any() else 0)
    cbp = (2 if ac else (1 if dcs.any() else 0)) << 4
    for q in range(4):
        if (mask >> (4 * q)) & 0xF:
            cbp |= 1 << q
    if kind == "i16" and mask & 0xFFFF:
        cbp |= 15
    rec["cbp"], rec["nnz_mask"] = cbp, mask


def paint(cv, x, y, spec, variant):
    """the neighbour samples of test macroblock (x, y): the designed edges of the spec, poison where the class declares a neighbour absent (and in the rows of the
    left chroma column a slot does not read: spec['c_unread']), the canvas's noise elsewhere"""
    left, top, tl, tr = spec["cls"]
    edges = spec.get("edges", {})
    for p in range(3):
        for name, have in (("top", top), ("left", left), ("tl", tl), ("tr", tr)):
            if name == "tr" and p:
                continue
            if p and name == "left" and "c_read" in spec:
                continue                      # a slot that reads some rows of the left column: below
            idx = cv.region(p, x, y, name)
            key = ("y", "cb", "cr")[p] + "_" + name
            if key in edges:
                cv.pl[p][idx] = edges[key]
            elif not have:
                n = np.size(cv.pl[p][idx])
                v = poison(n + 3, variant, cv.depth)[p:p + n]
                cv.pl[p][idx] = v if n > 1 else v[0]
        if p and spec.get("c_unread"):
            rows = np.array(spec["c_unread"])
            cv.pl[p][cv.ch * y + rows, 8 * x - 1] = poison(len(rows) + 3, variant, cv.depth)[p:p + len(rows)]
    paint_partial(cv, x, y, spec)


def grid_set(specs, depth, idc, seed, mb_w=GRID_W, mb_h=GRID_H):
    """the specs on as many contents as they need, each content as four pictures: poison P / Q (picture & 1), carriers all I_PCM (picture & 2 == 0: an intra
    dependency on every side, mb_w + 2 (mb_h - 1) levels) or all inter (no intra neighbour at all)"""
    spots = [(x, y) for y in range(1, mb_h, 2) for x in range(1, mb_w, 2)]
    ncont = (len(specs) + len(spots) - 1) // len(spots)
    r = SplitMix64(seed + 977 * depth + idc)
    canvases, where = [], []
    for c in range(ncont):
        part = specs[c * len(spots):(c + 1) * len(spots)]
        base = Canvas(r, mb_w, mb_h, depth, idc)
        for v in range(4):
            cv = copy.copy(base)
            cv.pl = [a.copy() for a in base.pl]
            for (x, y), spec in zip(spots, part):
                paint(cv, x, y, spec, v & 1)
            canvases.append(cv)
            where.append(part)
    fs = new_set(canvases, mb_w, mb_h, depth, idc)
    for f, part in enumerate(where):
        placed = {y * mb_w + x: spec for (x, y), spec in zip(spots, part)}
        for m in range(mb_w * mb_h):
            if m in placed:
                put_intra(fs, f, m, placed[m])
                fs.tests.append((f, m, placed[m]))
            else:
                put_carrier(fs, f, m, pcm=(f & 2) == 0)
    return RT.finish(fs)


# ---- A: availability classes times modes ----
def table_a(kind, seed=0xA4):
    r = SplitMix64(seed + len(kind) * 131 + ord(kind[1]))
    specs = []
    for c in range(16):
        cls = (bool(c & 1), bool(c & 2), bool(c & 4), bool(c & 8))
        left, top, tl, tr = cls
        tlm, _ = HF._avail_masks(top, left, tl, tr)
        mbc = mb_cands(left, top, tl)
        for k in range(4 if kind == "i16" else 9):
            spec = {"kind": kind, "cls": cls, "cmode": mbc[(k + 1) % len(mbc)]}
            if kind == "i16":
                spec["i16mode"] = mbc[k % len(mbc)]
                spec["resid"] = intra_resid(r, kind, [int(b) for b in r.randint(0, 15, 3)] if k & 1 else [], k % 3)
            else:
                modes = [0] * 16
                for i in (range(0, 16, 4) if kind == "i8" else range(16)):
                    cand = luma_cands(*block_avail(i, left, top, tlm))
                    modes[i] = cand[(k + (i >> 2 if kind == "i8" else i)) % len(cand)]
                spec["modes"] = modes
                # the first blocks coded: the later ones predict from reconstructed samples
                spec["resid"] = intra_resid(r, kind, [0, 1 + k % 2] if kind == "i8" else [0, 1, 4 + k % 4, 8 + k % 3, int(r.randint(9, 14))], k % 3)
            specs.append(spec)
    return specs


# ---- B: extremes ----
ALL = (True, True, True, True)


def plane_edges(n, sign, maxv, r):
    """n samples of an edge and the corner before them for a plane sum at its bound: '+' = the far half at the maximum, the near half and the corner at 0 (sum k = 36 or 10
    times the maximum), '-' the other way; '0' flat, 'n' noise, 'g' a gentle ramp"""
    h = n // 2
    if sign in "+-":
        a = np.array([0] * (h + 1) + [maxv] * h)
        a[h] = maxv // 2                      # the middle sample has no tap
        return a if sign == "+" else maxv - a
    if sign == "0":
        return np.full(n + 1, maxv // 2)
    if sign == "g":
        return np.clip(maxv // 3 + np.arange(n + 1) * (maxv // 40), 0, maxv)
    return r.randint(0, maxv, n + 1)


PLANE_DESIGNS = ("++", "--", "+0", "0+", "-0", "0-", "+-", "-+", "gg", "nn", "g-", "+g")


def table_b_plane(depth, idc, seed=0xB1):
    maxv, ch = (1 << depth) - 1, 8 * idc
    r = SplitMix64(seed + depth)
    specs = []
    for k, d in enumerate(PLANE_DESIGNS):
        e = {}
        t, l = plane_edges(16, d[0], maxv, r), plane_edges(16, d[1], maxv, r)
        e["y_tl"], e["y_top"], e["y_left"] = t[0], t[1:], l[1:]         # one corner: a design whose signs differ keeps the top edge's, the V sum then misses its k = 8 term
        for p, name in ((1, "cb"), (2, "cr")):
            dd = d if p == 1 else PLANE_DESIGNS[(k + 1) % len(PLANE_DESIGNS)]        # Cb and Cr carry different edges
            t, l = plane_edges(8, dd[0], maxv, r), plane_edges(ch, dd[1], maxv, r)
            e[name + "_tl"], e[name + "_top"], e[name + "_left"] = t[0], t[1:], l[1:]
        specs.append({"kind": "i16", "cls": ALL, "i16mode": C_PLANE, "cmode": C_PLANE, "edges": e})
    return specs


DC_CASES = ("zero", "max", "below", "at")
DC_VARIANTS = {"full": ((True, True, True, True), DC, C_DC), "left": ((True, False, False, False), LEFT_DC, C_LEFT_DC), "top": ((False, True, False, True), TOP_DC, C_TOP_DC),
               "mid": ((False, False, False, False), DC_128, C_DC128)}


def filt8(top, left, tl, has_tl=True, has_tr=True, tr=None):
    """PREDICT_8x8_LOAD_TOP / _LEFT (h264pred_template.c:849-861), restated for the census and the search below"""
    f3 = lambda a, b, c: (a + 2 * b + c + 2) >> 2
    t = [int(v) for v in top] + [int(tr[0]) if has_tr and tr is not None else int(top[7])]
    l = [int(v) for v in left]
    ft = [f3(int(tl) if has_tl else t[0], t[0], t[1])] + [f3(t[x - 1], t[x], t[x + 1]) for x in range(1, 8)]
    fl = [f3(int(tl) if has_tl else l[0], l[0], l[1])] + [f3(l[y - 1], l[y], l[y + 1]) for y in range(1, 7)] + [(l[6] + 3 * l[7] + 2) >> 2]
    return ft, fl


def dc_edges(form, variant, case, base, maxv):
    """top / left edges (sixteen luma samples each; eight for 'chroma') on which the form's first DC sum is 0, the maximum, one below or at its rounding step: a flat edge
    (the sum then is a multiple of the number of samples = the step) with as many samples raised by one as the case needs"""
    n = 8 if form == "chroma" else 16
    if case in ("zero", "max"):
        v = 0 if case == "zero" else maxv
        return np.full(n, v), np.full(n, v), v
    span = {"i4": 4, "i8": 8, "i16": 16, "chroma": 4}[form]
    count = span * (2 if variant == "full" else 1)
    for j in range(0, 2 * span + 1):
        top, left = np.full(n, base), np.full(n, base)
        which = left if variant == "left" else top
        which[:min(j, span)] += 1
        if j > span:
            left[:j - span] += 1
        if form == "i8":
            ft, fl = filt8(top[:8], left[:8], base, has_tl=variant == "full", tr=top[8:])
            s = (sum(ft) if variant != "left" else 0) + (sum(fl) if variant != "top" else 0)
        else:
            s = (int(top[:span].sum()) if variant != "left" else 0) + (int(left[:span].sum()) if variant != "top" else 0)
        if (s + count // 2) % count == (count - 1 if case == "below" else 0) and s != count * base:
            return top, left, base
    raise AssertionError(("no edge for", form, variant, case))


def dc_case_of(s, count, maxv):
    if s == 0:
        return "zero"
    if s == count * maxv:
        return "max"
    return {count - 1: "below", 0: "at"}.get((s + count // 2) % count)


def table_b_dc(depth, idc):
    maxv = (1 << depth) - 1
    specs = []
    for form in ("i4", "i8", "i16"):
        for variant, (cls, mode, cslot) in DC_VARIANTS.items():
            for ci, case in enumerate(DC_CASES):
                if variant == "mid" and ci:
                    continue
                e = {}
                if variant != "mid":
                    top, left, corner = dc_edges(form, variant, case, maxv // 3 + 1, maxv)
                    e.update({"y_top": top, "y_left": left, "y_tl": corner, "y_tr": top[:8] if form != "i8" else np.full(8, top[-1])})
                    for p, name in ((1, "cb"), (2, "cr")):
                        ccase = case if p == 1 else DC_CASES[(ci + 1) % 4]                  # Cb and Cr at different cases
                        ctop, cleft, ccorner = dc_edges("chroma", variant, ccase, maxv // 4 + 3 * p, maxv)
                        e.update({name + "_top": ctop, name + "_left": np.resize(cleft, 8 * idc), name + "_tl": ccorner})
                    # an absent side keeps its poison
                    for key in list(e):
                        side = key.split("_")[1]
                        if not cls[{"left": 0, "top": 1, "tl": 2, "tr": 3}[side]]:
                            del e[key]
                spec = {"kind": form, "cls": cls, "cmode": cslot, "edges": e}
                if form == "i16":
                    spec["i16mode"] = cslot
                else:
                    tlm, _ = HF._avail_masks(cls[1], cls[0], cls[2], cls[3])
                    modes = [0] * 16
                    for i in range(16):
                        btop, bleft, _ = block_avail(i, cls[0], cls[1], tlm)
                        modes[i] = DC if btop and bleft else (LEFT_DC if bleft else (TOP_DC if btop else DC_128))
                    spec["modes"] = modes
                specs.append(spec)
    return specs


def table_b_taps(depth, idc):
    """the alternating 0 / maximum edge, both phases, under every mode of Intra 4x4 and Intra 8x8 (the pre-filter's and the directional (1, 2, 1) / (1, 1) taps)"""
    maxv = (1 << depth) - 1
    specs = []
    alt = lambda n, ph: np.where((np.arange(n) + ph) & 1, maxv, 0)
    for kind in ("i4", "i8"):
        for ph in range(2):
            for mode in range(9):
                e = {"y_top": alt(16, ph), "y_tr": alt(8, ph), "y_left": alt(16, ph), "y_tl": alt(1, ph + 1)[0]}
                for p, name in ((1, "cb"), (2, "cr")):
                    e.update({name + "_top": alt(8, ph + p), name + "_left": alt(8 * idc, ph + p), name + "_tl": alt(1, ph + p + 1)[0]})
                modes = [[mode, (mode + 3) % 9, (mode + 5) % 9, (mode + 7) % 9][(i >> 2) if kind == "i8" else (i % 4)] for i in range(16)]
                specs.append({"kind": kind, "cls": ALL, "modes": modes, "cmode": (C_DC, C_HOR, C_VERT, C_PLANE)[mode % 4], "edges": e})
    return specs


# ---- C: the chroma slots ----
def slot_reads(slot, idc):
    """(top, corner, rows of the left column) the chroma predictor of a slot reads (h264pred_template.c:563-802; 8x16 :502-846)"""
    ch = 8 * idc
    rows = list(range(ch))
    return {C_DC: (1, 0, rows), C_HOR: (0, 0, rows), C_VERT: (1, 0, []), C_PLANE: (1, 1, rows), C_LEFT_DC: (0, 0, rows), C_TOP_DC: (1, 0, []), C_DC128: (0, 0, []),
            C_L0T: (1, 0, rows[:4]), C_0LT: (1, 0, rows[4:]), C_L00: (0, 0, rows[:4] + rows[8:]), C_0L0: (0, 0, rows[4:])}[slot]


def table_c(depth, idc, seed=0xC4):
    """every slot on noise and on two extreme edges (0 / maximum in halves and alternating; Cb and Cr the other way round).  What a slot does not read — a side, or the
    rows of the left column its quadrants leave out — holds poison.  The luma of these macroblocks: Intra16x16 in a mode its class allows."""
    maxv = (1 << depth) - 1
    r = SplitMix64(seed + depth + idc)
    ch = 8 * idc
    specs = []
    for slot in range(11):
        top, corner, rows = slot_reads(slot, idc)
        left = len(rows) == ch
        cls = (left, bool(top), bool(corner), bool(top))
        for style in range(3):
            e = {}
            if style:
                for p, name in ((1, "cb"), (2, "cr")):
                    flip = (p == 2) != (style == 2)
                    if style == 1:
                        t = np.where(np.arange(8) < 4, 0, maxv)
                        l = np.where((np.arange(ch) // 4) & 1, 0, maxv)
                    else:
                        t, l = np.where(np.arange(8) & 1, maxv, 0), np.where(np.arange(ch) & 1, 0, maxv)
                    if flip:
                        t, l = maxv - t, maxv - l
                    if top:
                        e[name + "_top"] = t
                    if corner:
                        e[name + "_tl"] = 0 if flip else maxv
                    if left:
                        e[name + "_left"] = l
            lc = mb_cands(cls[0], cls[1], cls[2])
            spec = {"kind": "i16", "cls": cls, "i16mode": lc[style % len(lc)], "cmode": slot, "edges": e, "resid": intra_resid(r, "i16", [], style)}
            if rows and not left:
                spec["c_unread"] = [y for y in range(ch) if y not in rows]
                spec["c_read"] = rows
                spec["c_style"] = style
            specs.append(spec)
    return specs


def paint_partial(cv, x, y, spec):
    """the rows of the left chroma column a slot of 7..10 reads, on the extreme styles (the unread rows hold poison, the class says 'no left neighbour')"""
    if "c_read" not in spec or not spec["c_style"]:
        return
    rows = np.array(spec["c_read"])
    for p in (1, 2):
        v = np.where((rows // (4 if spec["c_style"] == 1 else 1)) & 1, 0, cv.maxv)
        cv.pl[p][cv.ch * y + rows, 8 * x - 1] = v if p == 1 else cv.maxv - v


# ---- D: chains for the single launch ----
CHAIN_LEN = 18
DIRS = {"left": (1, 0), "above-left": (1, 1), "above": (0, 1), "above-right": (-1, 1)}         # a link's step from the link before it


def chain_spec(r, direction, k):
    """a link that reads the neighbour it hangs on and hands the samples on to the next: HOR / VERT through every block for left / above; every block diagonal down-left
    for above-right (block 5, Intra 8x8 block 1, read the eight samples above-right; the macroblock's lower left blocks, which the next link reads, follow from them);
    diagonal down-right for above-left (block 0 reads the corner).  Intra 4x4, Intra 8x8 and — where its modes read that neighbour — Intra16x16 in turn; residual in every link."""
    kind = ("i4", "i8", "i16")[k % 3] if direction in ("left", "above") else ("i4", "i8")[k % 2]
    mode = {"left": HOR, "above": VERT, "above-right": DDL, "above-left": DDR}[direction]
    spec = {"kind": kind, "cls": ALL, "cmode": {"left": C_HOR, "above": C_VERT}.get(direction, C_PLANE if direction == "above-left" else C_DC)}
    if kind == "i16":
        spec["i16mode"] = C_HOR if direction == "left" else C_VERT
    else:
        spec["modes"] = [mode] * 16
    spec["resid"] = intra_resid(r, kind, [0, 1, 2, 3] if kind == "i8" else [0, 3, 5, 6, 9, 10, 12, 15], 1 + k % 2)
    return spec


def chain_set(depth, idc, seed=0xD4, bump=None):
    """four pictures 20 x 19, one chain each; everything else inter carriers.  bump = (picture, level to add): the first link's DC level changed (the census)"""
    mb_w, mb_h = 20, 19
    r = SplitMix64(seed + depth + idc)
    canvases = [Canvas(r, mb_w, mb_h, depth, idc) for _ in DIRS]
    fs = new_set(canvases, mb_w, mb_h, depth, idc)
    fs.chains = {}
    for f, (direction, (dx, dy)) in enumerate(DIRS.items()):
        x0, y0 = (18 if dx < 0 else 1), (9 if dy == 0 else 1)
        links = [(x0 + k * dx, y0 + k * dy) for k in range(CHAIN_LEN)]
        at = {y * mb_w + x: k for k, (x, y) in enumerate(links)}
        for m in range(mb_w * mb_h):
            if m in at:
                spec = chain_spec(r, direction, at[m])
                if bump is not None and bump[0] == f and at[m] == 0:
                    spec["resid"][0:256:16] += bump[1]      # the first link is Intra 4x4: every block's DC level (a single column or row can end at a clip)
                put_intra(fs, f, m, spec)
                fs.tests.append((f, m, spec))
            else:
                put_carrier(fs, f, m, pcm=False)
        fs.chains[direction] = (f, [y * mb_w + x for x, y in links])
    return RT.finish(fs)


# ---- entries ----
def build(name, depth=8, idc=1):
    if name.startswith("A-"):
        return grid_set(table_a(name[2:]), depth, idc, 0xA00)
    if name == "D-chains":
        return chain_set(depth, idc)
    specs = {"B-plane": table_b_plane, "B-dc": table_b_dc, "B-taps": table_b_taps, "C-chroma": table_c}[name](depth, idc)
    fs = grid_set(specs, depth, idc, 0xB00 + len(name))
    return fs


ENTRIES = ("A-i4", "A-i8", "A-i16", "B-plane", "B-dc", "B-taps", "C-chroma", "D-chains")
FORMS8 = ("linear-levels", "tiled-levels", "linear-single", "tiled-single", "wide")
FORMS_HBD = ("wide-9", "wide-10", "wide-10-422")
_SETS = {}


def entry(oracle, name, depth=8, idc=1):
    """(set, (recon, dst) of the frame-level oracle), made once per process; None for the pictures where the checker above 8 bits is not built"""
    key = (name, depth, idc)
    if key not in _SETS:
        fs = build(name, depth, idc)
        _SETS[key] = (fs, HF.run_oracle(oracle, fs) if (depth, idc) == (8, 1) else HF.run_oracle_hbd(oracle, fs, depth, idc=idc))
    return _SETS[key]


def wide_pcm(fs):
    """the 8-bit set as the second kernel set takes it: an I_PCM macroblock's samples one per coefficient slot"""
    g = copy.copy(fs)
    g.coef = fs.coef.copy()
    pcm = (fs.mb["mb_type"] & 4) != 0
    g.coef[pcm] = fs.coef[pcm].view(np.uint8)[:, :384].astype(np.int16)
    return g


def run_entry(backend, oracle, name, form):
    """False: the checker above 8 bits is not built here"""
    depth, idc = {"wide-9": (9, 1), "wide-10": (10, 1), "wide-10-422": (10, 2)}.get(form, (8, 1))
    fs, ref = entry(oracle, name, depth, idc)
    if ref is None:
        return False
    if depth > 8:
        d = HF.DeviceFrames(backend, fs, bit_depth=depth, idc=idc)
    else:
        d = HF.DeviceFrames(backend, wide_pcm(fs) if form == "wide" else fs, tiled=form.startswith("tiled"))
    try:
        if form.startswith("wide"):
            d.decode_wide(bit_depth=depth, idc=idc)
        else:
            assert fs.max_intra_level >= 16
            d.decode_intra_form(single=form.endswith("single"))
        RT.compare("%s/%s" % (name, form), fs, ref[0], ref[1], d.fetch(d.recon), d.fetch(d.dst))
    finally:
        d.free()
    return True


# ---- census ----
def mb_view(planes, fs, f, m, p=0):
    h, w = (16, 16) if p == 0 else (8 * fs.idc, 8)
    x, y = m % fs.mb_w, m // fs.mb_w
    return planes[p][f, h * y:h * y + h, w * x:w * x + w]


def census(fs, recon, c=None):
    """what the set's test macroblocks hold, read off their RECORDS and the canvases: {class: count}.  recon: the oracle's reconstruction (the plane and DC restatements
    below must give it where a macroblock has no residual — the census classifies the oracle's own samples, not its idea of them)"""
    c = {} if c is None else c
    maxv = (1 << fs.depth) - 1

    def note(*key):
        c[key] = c.get(key, 0) + 1

    def rng(key, v):
        lo, hi = c.get(key, (v, v))
        c[key] = (min(lo, v), max(hi, v))
    for f, m, spec in fs.tests:
        rec, cv = fs.mb[f, m], fs.canvases[f]
        x, y = m % fs.mb_w, m // fs.mb_w
        cls = rec_class(rec)
        t = int(rec["mb_type"])
        kind = "i16" if t & HF.I16 else ("i8" if t & HF.DCT8 else "i4")
        plain = not int(rec["cbp"]) and not int(rec["nnz_mask"])
        edge = lambda p, name: np.atleast_1d(cv.pl[p][cv.region(p, x, y, name)]).astype(np.int64)
        note("slot", fs.idc, int(rec["chroma_mode"]))
        note("chroma", cls[:3], int(rec["chroma_mode"]))
        if kind == "i16":
            mode = int(rec["i16mode"])
            note("i16", cls, mode)
            if mode == C_PLANE and plain:
                T, L = np.concatenate([edge(0, "tl"), edge(0, "top")]), np.concatenate([edge(0, "tl"), edge(0, "left")])
                H = sum(k * (T[8 + k] - T[8 - k]) for k in range(1, 9))
                V = sum(k * (L[8 + k] - L[8 - k]) for k in range(1, 9))
                rng(("plane16", "H"), int(H))
                rng(("plane16", "V"), int(V))
                h, v = (5 * H + 32) >> 6, (5 * V + 32) >> 6
                a = 16 * (L[16] + T[16] + 1) - 7 * (v + h)
                raw = (a + np.arange(16)[None, :] * h + np.arange(16)[:, None] * v) >> 5
                assert np.array_equal(np.clip(raw, 0, maxv), mb_view(recon, fs, f, m)), ("the census restates the plane otherwise than the oracle", f, m)
                for col in range(4):
                    part = raw[:, col::4]
                    for how, sel in (("low", part < 0), ("high", part > maxv), ("inside", (part > 0) & (part < maxv))):
                        if sel.any():
                            note("clip", col, how)
            if mode in (C_DC, C_LEFT_DC, C_TOP_DC) and plain:
                s = (edge(0, "top").sum() if mode != C_LEFT_DC else 0) + (edge(0, "left").sum() if mode != C_TOP_DC else 0)
                n = 32 if mode == C_DC else 16
                assert (mb_view(recon, fs, f, m) == (s + n // 2) // n).all()
                note("dc", "i16", {C_DC: "full", C_LEFT_DC: "left", C_TOP_DC: "top"}[mode], dc_case_of(int(s), n, maxv))
            if mode == C_DC128:
                note("dc", "i16", "mid", "zero")
        else:
            tlm, trm = int(rec["topleft"]), int(rec["topright"])
            for i in (range(0, 16, 4) if kind == "i8" else range(16)):
                mode = int(rec["i4mode"][i])
                b = i >> 2 if kind == "i8" else i
                if kind == "i8" or i in REACH4:
                    note(kind, cls, b, mode)
                if kind == "i8":
                    note("i8_tl_tr", mode, bool((tlm << i) & 0x8000), bool((trm << i) & 0x4000))
                elif mode in (DDL, VL):
                    note("tr", i, mode, bool((trm << i) & 0x8000))
                if b == 0 and cls == ALL and mode < 9 and all((np.abs(np.diff(np.concatenate([edge(0, n1), edge(0, n2)]))) == maxv).all() for n1, n2 in (("tl", "top"), ("top", "tr"), ("tl", "left"))):
                    note("alt", kind, mode, int(edge(0, "top")[0] != 0))
                if b == 0 and plain and mode in (DC, LEFT_DC, TOP_DC, DC_128):
                    variant = {DC: "full", LEFT_DC: "left", TOP_DC: "top", DC_128: "mid"}[mode]
                    if mode == DC_128:
                        note("dc", kind, "mid", "zero")
                        continue
                    n = 4 if kind == "i4" else 8
                    if kind == "i4":
                        top, left = edge(0, "top")[:4], edge(0, "left")[:4]
                    else:
                        top, left = filt8(edge(0, "top")[:8], edge(0, "left")[:8], edge(0, "tl")[0], bool((tlm << i) & 0x8000), bool((trm << i) & 0x4000), edge(0, "top")[8:])
                    s = (sum(top) if mode != LEFT_DC else 0) + (sum(left) if mode != TOP_DC else 0)
                    cnt = n * (2 if mode == DC else 1)
                    assert (mb_view(recon, fs, f, m)[:n, :n] == (s + cnt // 2) // cnt).all(), ("the census restates the DC otherwise than the oracle", kind, f, m)
                    note("dc", kind, variant, dc_case_of(int(s), cnt, maxv))
        # chroma: the plane sums and the first quadrant's DC, per plane
        cm = int(rec["chroma_mode"])
        for p in (1, 2):
            if cm == C_PLANE and plain:
                T, L = np.concatenate([edge(p, "tl"), edge(p, "top")]), np.concatenate([edge(p, "tl"), edge(p, "left")])
                H = sum(k * (T[4 + k] - T[4 - k]) for k in range(1, 5))
                hv = cv.ch // 2
                V = sum(k * (L[hv + k] - L[hv - k]) for k in range(1, hv + 1))
                rng(("planec", fs.idc, "H"), int(H))
                rng(("planec", fs.idc, "V"), int(V))
                note("planec_plane", fs.idc, p, (int(H) > 0) - (int(H) < 0), (int(V) > 0) - (int(V) < 0))
            if cm in (C_DC, C_LEFT_DC, C_TOP_DC) and plain:
                s = (edge(p, "top")[:4].sum() if cm != C_LEFT_DC else 0) + (edge(p, "left")[:4].sum() if cm != C_TOP_DC else 0)
                cnt = 8 if cm == C_DC else 4
                assert (mb_view(recon, fs, f, m, p)[:4, :4] == (s + cnt // 2) // cnt).all()
                note("dc", "chroma", {C_DC: "full", C_LEFT_DC: "left", C_TOP_DC: "top"}[cm], dc_case_of(int(s), cnt, maxv))
            if cm == C_DC128:
                note("dc", "chroma", "mid", "zero")
    return c


def poison_census(fs, recon):
    """P / Q: the pictures of a content (four in a row: P, Q on I_PCM carriers, P, Q on inter carriers) have the same test macroblocks in the oracle; where a class
    declares a neighbour absent the carriers differ between P and Q in every sample of it.  Returns {absent neighbour: count}"""
    c = {}
    test = np.zeros((fs.F, fs.mb_h, fs.mb_w), bool)
    for f, m, _ in fs.tests:
        test[f, m // fs.mb_w, m % fs.mb_w] = True
    for f0 in range(0, fs.F, 4):
        assert (test[f0] == test[f0:f0 + 4]).all()
        for p in range(3):
            h, w = (16, 16) if p == 0 else (8 * fs.idc, 8)
            sel = np.repeat(np.repeat(test[f0], h, axis=0), w, axis=1)
            for v in range(1, 4):
                assert np.array_equal(recon[p][f0][sel], recon[p][f0 + v][sel]), ("a test macroblock of the oracle depends on poison or on the carrier kind", f0, v, p)
    for f, m, spec in fs.tests:
        if f % 4:
            continue
        x, y = m % fs.mb_w, m // fs.mb_w
        for k, name in enumerate(("left", "top", "tl", "tr")):
            if rec_class(fs.mb[f, m])[k]:
                continue
            for p in range(3 if name != "tr" else 1):
                if p and name == "left" and "c_read" in spec:
                    continue                  # the rows the slot does not read: below
                idx = fs.canvases[f].region(p, x, y, name)
                for a, b in ((0, 1), (2, 3)):
                    pa, pb = recon[p][f + a][idx], recon[p][f + b][idx]
                    assert np.all(pa != pb), ("poison P and Q agree in a sample", f, m, name, p)
            c[name] = c.get(name, 0) + 1
        if spec.get("c_unread"):
            rows = np.array(spec["c_unread"])
            for p in (1, 2):
                assert np.all(recon[p][f][fs.canvases[f].ch * y + rows, 8 * x - 1] != recon[p][f + 1][fs.canvases[f].ch * y + rows, 8 * x - 1])
            c["left rows"] = c.get("left rows", 0) + 1
    return c


def chain_census(fs):
    """every link of every chain: exactly one intra neighbour, in the chain's direction; the levels"""
    out = {}
    intra = ((fs.mb["mb_type"] & 7) != 0)
    for direction, (f, links) in fs.chains.items():
        for k, m in enumerate(links[1:], 1):
            x, y = m % fs.mb_w, m // fs.mb_w
            nb = {"left": (x - 1, y), "above-left": (x - 1, y - 1), "above": (x, y - 1), "above-right": (x + 1, y - 1)}
            have = [d for d, (nx, ny) in nb.items() if 0 <= nx < fs.mb_w and ny >= 0 and intra[f, ny * fs.mb_w + nx]]
            assert have == [direction], (direction, k, have)
            assert nb[direction][0] + nb[direction][1] * fs.mb_w == links[k - 1]
        assert all(0 < m % fs.mb_w < fs.mb_w - 1 and m // fs.mb_w > 0 for m in links)          # no link at a picture border: every neighbour exists
        out[direction] = int(fs.intra_start[f].shape[0]) - 1
    return out
