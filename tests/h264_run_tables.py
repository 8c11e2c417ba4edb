"""Directed tables for the tiled run kernel (k_recon_inter_tiled / k_recon_inter_rest, h264_recon_fast.h) and the code it hands macroblocks to:
  A  run lengths 4..15 on designed rows of macroblock kinds (RUN_ENTRIES, run_sets, kind_census);
  B  the 6-tap filters' extreme sums on frame level, window alignment and borders (filter_set, align_set, border_set, filter_census);
  C  explicit and implicit weights over every denominator, both chroma switches, every partition shape (weight_set, weight_census).
Everything is built here from fixed seeds; every picture is compared with HF.run_oracle sample for sample."""
import ctypes as C

import numpy as np

import h264_frames as HF
from rng import SplitMix64

QP = 26
SHAPE_T = [HF.T16x16, HF.T16x8, HF.T8x16, HF.T8x8]
SUBPARTS = {0: [(0, 0, 2, 2)], 1: [(0, 0, 2, 1), (0, 1, 2, 1)], 2: [(0, 0, 1, 2), (1, 0, 1, 2)], 3: [(0, 0, 1, 1), (1, 0, 1, 1), (0, 1, 1, 1), (1, 1, 1, 1)]}


# ---- building pictures macroblock by macroblock ----
def new_set(nframes, mb_w, mb_h, refs, bframes=False, nslices=1):
    """refs[f][slot] = (Y, Cb, Cr); list 0 maps reference index i to slot i, list 1 to slot nrefs - 1 - i"""
    nrefs = len(refs[0])
    fs = HF.FrameSet(nframes, mb_w, mb_h, nrefs)
    fs.use_l1 = bframes
    fs.slices = np.zeros((nframes, nslices), HF.SLICE_DT)
    sl = fs.slices
    sl["list_count"] = 2 if bframes else 1
    sl["ref_slot"][:, :, 0, :nrefs] = np.arange(nrefs)
    sl["ref_slot"][:, :, 1, :nrefs] = np.arange(nrefs)[::-1]
    sl["chroma_qp_table"][:, :, 0] = HF.CHROMA_QP
    sl["chroma_qp_table"][:, :, 1] = HF.CHROMA_QP
    for f in range(nframes):
        fs.refs[f] = [tuple(np.ascontiguousarray(p) for p in refs[f][s]) for s in range(nrefs)]
    for f in range(nframes):
        for m in range(mb_w * mb_h):
            rec = fs.mb[f, m]
            qpc = HF.CHROMA_QP[QP]
            rec["qp"], rec["qpc"], rec["dc_qmul"] = QP, (qpc, qpc), (HF.dc_qmul(QP), HF.dc_qmul(qpc), HF.dc_qmul(qpc))
            rec["flags"] = (HF.F_LEFT if m % mb_w else 0) | (HF.F_TOP if m // mb_w else 0)
            rec["ref_idx"] = -1
    return fs


def put_inter(fs, f, m, shape, preds, dct8=False, slice_id=0, weighted=False):
    """shape 0 16x16: preds = [pred]; 1 16x8 / 2 8x16: [first, second]; 3 8x8: four (sub, [pred per sub-partition]) with one reference per list in a quadrant.
    pred = {list: (reference index, (mvx, mvy))}"""
    rec = fs.mb[f, m]
    sl = fs.slices[f, slice_id]
    t = SHAPE_T[shape] | (HF.DCT8 if dct8 else 0)
    rec["slice_id"] = slice_id
    rec["ref_idx"] = -1
    rec["sub"] = 0

    def fill(pred, blocks, quads):
        for l, (ref, mv) in pred.items():
            for q in quads:
                rec["ref_idx"][l][q] = ref
            fs.mv[l, f, m, blocks] = mv
    rows = lambda x0, y0, w, h: [x + 4 * y for y in range(y0, y0 + h) for x in range(x0, x0 + w)]
    if shape == 0:
        fill(preds[0], rows(0, 0, 4, 4), [0, 1, 2, 3])
        t |= sum(HF.P0L0 << (2 * l) for l in preds[0])
    elif shape in (1, 2):
        geo = [((0, 0, 4, 2), [0, 1]), ((0, 2, 4, 2), [2, 3])] if shape == 1 else [((0, 0, 2, 4), [0, 2]), ((2, 0, 2, 4), [1, 3])]
        for k, (g, quads) in enumerate(geo):
            fill(preds[k], rows(*g), quads)
            t |= sum(HF.P0L0 << (2 * l + k) for l in preds[k])
    else:
        used = set()
        for q, (sub, parts) in enumerate(preds):
            qx, qy = 2 * (q & 1), 2 * (q >> 1)
            rec["sub"][q] = sub | sum(0x10 << l for l in parts[0])
            used |= set(parts[0])
            for (px, py, pw, ph), pred in zip(SUBPARTS[sub], parts):
                fill(pred, rows(qx + px, qy + py, pw, ph), [q])
        t |= sum((HF.P0L0 | HF.P1L0) << (2 * l) for l in used)
    rec["mb_type"] = t
    if weighted:
        rec["flags"] |= HF.F_WEIGHTED
    for l in range(2):
        for q in range(4):
            ri = int(rec["ref_idx"][l][q])
            rec["i4mode"][4 * l + q] = np.uint8(sl["ref_slot"][l][ri]).astype(np.int8) if ri >= 0 else -1


def put_i16(fs, f, m):
    """Intra16x16 without residual, a mode its neighbours allow"""
    rec = fs.mb[f, m]
    top, left = m >= fs.mb_w, m % fs.mb_w > 0
    rec["topleft"], rec["topright"] = HF._avail_masks(top, left, top and left, top and m % fs.mb_w + 1 < fs.mb_w)
    mode = ([2, 0, 1, 3][m % 4] if top and left else (1 if left else (2 if top else 6)))
    if mode == 2 and not (top and left):
        mode = 5
    rec["mb_type"], rec["i16mode"], rec["chroma_mode"] = HF.I16, mode, ([0, 1, 2, 3][m % 4] if top and left else (1 if left else (2 if top else 6)))
    rec["ref_idx"] = -1


def put_resid(fs, f, m, cf):
    """the coefficients of an inter macroblock (4x4 blocks, or four 8x8 ones with the 8x8 transform; chroma DC levels at 256 + 16 j) and the masks that follow from them"""
    rec = fs.mb[f, m]
    cf = np.asarray(cf, np.int16)
    fs.coef[f, m] = cf
    mask = 0
    if int(rec["mb_type"]) & HF.DCT8:
        for q in range(4):
            if cf[64 * q:64 * q + 64].any():
                mask |= 0xF << (4 * q)
    else:
        for i in range(16):
            if cf[16 * i:16 * i + 16].any():
                mask |= 1 << i
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
    rec["cbp"], rec["nnz_mask"] = cbp, mask


def random_resid(r, dct8=False):
    HF.COEF_B[0], HF.COEF_CLIP[0] = 24, 2047
    cf = np.zeros(384, np.int16)
    if dct8:
        for q in range(4):
            k = r.randint(1, 20)
            cf[64 * q + r.randint(0, 63, k)] = r.laplace_int(24, k, 2047)
        cf[0] = cf[0] or 9
    else:
        blks, coded = HF._gen_block_coefs(r, 16, "dense")
        cf[:256] = blks.reshape(-1)
        cf[0] = cf[0] or 9
    blks, _ = HF._gen_block_coefs(r, 8, "sparse")
    cf[256:] = blks.reshape(-1)
    cf[256:384:16] = r.laplace_int(30, 8, 2047)
    cf[256] = cf[256] or 5
    return cf


def finish(fs):
    for f in range(fs.F):
        fs.max_intra_level = max(fs.max_intra_level, HF.intra_schedule(fs, f))
    return fs


def noise_refs(r, nframes, nrefs, H, W):
    return [[(r.u8((H, W)), r.u8((H // 2, W // 2)), r.u8((H // 2, W // 2))) for _ in range(nrefs)] for _ in range(nframes)]


# ---- A: run lengths ----
def run_plan(lib, nframes, max_w, max_h, forced=0):
    """mi355_h264_recon_run_plan -> (run, runs_row), or None where it refuses"""
    fn = lib.mi355_h264_recon_run_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 4 + [C.c_void_p] * 2
    run, runs_row = C.c_int(-1), C.c_int(-1)
    rc = fn(nframes, max_w, max_h, forced, C.byref(run), C.byref(runs_row))
    assert rc in (0, -1)
    return (run.value, runs_row.value) if rc == 0 else None


def plan_rule(nframes, max_w, max_h, forced=0):
    """the rule as DESIGN.md states it, in python: what the runs of a row are for the census"""
    run = forced if forced > 0 else min(max(nframes * max_w * max_h // (40 * 8192), 4), 15)
    run = min(run, max_w)
    runs_row = (max_w + run - 1) // run
    return (max_w + runs_row - 1) // runs_row, runs_row


KINDS = ("fast_resid", "fast_plain", "fast_patched", "fast_inside", "two", "general", "intra16")
RUNS, WIDTHS = (4, 5, 8, 11, 15), (1, 4, 15, 16, 17, 30, 31)
# ... and the ends of what a named run may be: 16 (bits 15 and 31 of the run's word, lane 15 of the description), and runs shorter than the rule's four
RUN_ENTRIES = [(run, w) for run in RUNS for w in WIDTHS] + [(16, 16), (16, 31), (1, 4), (2, 5), (3, 17)]
MIXED_ENTRY = (15, (31, 17))         # one launch, two pictures of different width: the grid is the wider one's


def kind_sequence():
    """a cycle over the seven kinds in which every ordered pair (previous, next), a kind behind itself included, occurs once: an Euler circuit of the 49 pairs"""
    nxt = {k: [(k + d) % 7 for d in range(7)] for k in range(7)}
    stack, seq = [0], []
    while stack:
        k = stack[-1]
        if nxt[k]:
            stack.append(nxt[k].pop())
        else:
            seq.append(stack.pop())
    return seq[:-1][::-1]


def run_kinds_set(run, mb_w, nframes=4, seed=0xA11):
    """P pictures two macroblock rows high whose rows follow kind_sequence(), each row starting elsewhere in it"""
    mb_h = 2
    r = SplitMix64(seed + 131 * run + mb_w)
    fs = new_set(nframes, mb_w, mb_h, noise_refs(r, nframes, 3, 16 * mb_h, 16 * mb_w))
    seq = kind_sequence()
    # rows start where the kinds asked for at a run's first / last place (two and general at i = run - 1 among them) come up over the table's rows
    for f in range(nframes):
        for y in range(mb_h):
            row = f * mb_h + y
            start = (row * 11 + 5 * run + 3 * mb_w) % len(seq)
            for x in range(mb_w):
                kind = seq[(start + x) % len(seq)]
                m = y * mb_w + x
                put_kind(fs, r, f, m, x, y, kind, row + x)
    return finish(fs)


def put_kind(fs, r, f, m, x, y, kind, n):
    mb_w, mb_h = fs.mb_w, fs.mb_h
    frac = lambda: (r.randint(0, 3), r.randint(0, 3))
    near = lambda: (r.randint(-40, 40), r.randint(-40, 40))
    ref = lambda: r.randint(0, fs.nrefs - 1)
    if kind == 6:
        put_i16(fs, f, m)
        return
    if kind in (0, 1):
        # neither patched nor inside where the picture is three macroblocks wide: the window's three tiles exist, its rows reach over the top or the bottom border
        t0 = min(max(x - n % 2, 0), max(mb_w - 3, 0))
        ix, (fx, fy) = 16 * t0 + 4 + r.randint(0, 11), frac()
        put_inter(fs, f, m, 0, [{0: (ref(), (4 * (ix - 16 * x) + fx, (4 * r.randint(3, 12) + fy) * (1 if y else -1)))}])
        if kind == 0:
            put_resid(fs, f, m, random_resid(r))
    elif kind == 2:
        # a window over the left or the right border (FQA_PATCH_Y / FQA_PATCH_C), by a little or by more than a tile
        ix = (-8 - 16 * (n % 3)) if n & 1 else 16 * mb_w - 6 + 9 * (n % 3)
        fx, fy = frac()
        put_inter(fs, f, m, 0, [{0: (ref(), (4 * (ix - 16 * x) + fx, r.randint(-24, 24)))}])
        if n & 2:
            put_resid(fs, f, m, random_resid(r))
    elif kind == 3:
        # both windows inside (FQA_INSIDE) where the picture is wide enough for one: the luma window's first tile t0 and the two behind it exist, rows 2 .. 13
        t0 = min(max(x - 1 + n % 2, 0), max(mb_w - 3, 0))
        ix, iy = 16 * t0 + 4 + r.randint(0, 11), 2 + r.randint(0, 11)
        fx, fy = frac()
        put_inter(fs, f, m, 0, [{0: (ref(), (4 * (ix - 16 * x) + fx, 4 * (iy - 16 * y) + fy))}])
        if n & 1:
            put_resid(fs, f, m, random_resid(r))
    elif kind == 4:
        put_inter(fs, f, m, 1 + n % 2, [{0: (ref(), near())}, {0: (ref(), (r.randint(-90, 90), r.randint(-40, 40)))}])
        if n & 2:
            put_resid(fs, f, m, random_resid(r))
    else:
        if n % 3 == 0:
            put_inter(fs, f, m, 0, [{0: (ref(), near())}], dct8=True)
            put_resid(fs, f, m, random_resid(r, dct8=True))
        else:
            quads = []
            for q in range(4):
                sub, rq = (q + n) % 4, ref()
                quads.append((sub, [{0: (rq, near())} for _ in SUBPARTS[sub]]))
            put_inter(fs, f, m, 3, quads)
            if n % 3 == 1:
                put_resid(fs, f, m, random_resid(r))


def geometry(mv, x, y, mb_w, mb_h):
    """fq_geometry's flags for a list-0 vector of macroblock (x, y): (patched, inside)"""
    mx, my = int(mv[0]) + 64 * x, int(mv[1]) + 64 * y
    ix, iy, cx, cy = mx >> 2, my >> 2, mx >> 3, my >> 3
    t0, c0 = (ix - 4) >> 4, cx & ~3
    patch_y = not (0 <= t0 < max(mb_w - 2, 0))
    patch_c = not (0 <= c0 < max(8 * mb_w - 11, 0))
    inside = not patch_y and not patch_c and 0 <= iy - 2 < max(16 * mb_h - 20, 0) and 0 <= cy < max(8 * mb_h - 8, 0)
    return patch_y or patch_c, inside


def classify(fs, f, m):
    """the kind fq_describe gives a macroblock (KINDS), from its record"""
    rec = fs.mb[f, m]
    t = int(rec["mb_type"])
    if t & 7:
        return 6
    plain = not int(rec["flags"]) & HF.F_WEIGHTED
    if plain and t & (HF.T16x16 | HF.P0L0 | HF.P0L1 | HF.DCT8) == (HF.T16x16 | HF.P0L0):
        patched, inside = geometry(fs.mv[0, f, m, 0], m % fs.mb_w, m // fs.mb_w, fs.mb_w, fs.mb_h)
        if patched:
            return 2
        if inside:
            return 3
        return 0 if (int(rec["nnz_mask"]) & 0xFFFF) or (int(rec["cbp"]) & 0x30) else 1
    if plain and t & (HF.P0L0 | HF.P1L0 | HF.P0L1 | HF.P1L1 | HF.DCT8) == (HF.P0L0 | HF.P1L0) and t & (HF.T16x8 | HF.T8x16):
        return 4
    return 5


def kind_census(sets, run, max_w):
    """what the runs of a launch over `sets` (pictures of max_w columns at most) hold: {class: count}"""
    c = {}

    def note(*key):
        c[key] = c.get(key, 0) + 1
    for fs in sets:
        for f in range(fs.F):
            for y in range(fs.mb_h):
                for x0 in range(0, max_w, run):
                    n = min(run, max_w - x0)
                    n_row = max(min(n, fs.mb_w - x0), 0)
                    if n_row < n:
                        note("cut_run", n_row == 0)
                    prev = None
                    for i in range(n_row):
                        k = classify(fs, f, y * fs.mb_w + x0 + i)
                        if prev is not None:
                            note("pair", prev, k)
                        prev = k
                        if i == 0:
                            note("first", k)
                        if i == n_row - 1:
                            note("last_full" if n_row == run else "last_short", k)
                        if i == 14:
                            note("i14", k)
                        if i == 15:
                            note("i15", k)
                        if k in (2, 3):
                            note("window_set", i & 1, k)
                        if k in (4, 5):
                            note("deferred_bit", i)
    return c


def concat_descriptors(backend, devs):
    lib = backend.lib
    fsz = C.sizeof(devs[0].host_desc) // devs[0].F
    total = sum(d.F for d in devs)
    lib.mi355_malloc.restype = C.c_void_p
    lib.mi355_malloc.argtypes = [C.c_size_t]
    d_all = lib.mi355_malloc(total * fsz)
    assert d_all
    off = 0
    for d in devs:
        assert lib.mi355_memcpy_h2d(C.c_void_p(d_all + off), C.c_void_p(C.addressof(d.host_desc)), C.c_size_t(d.F * fsz)) == 0
        off += d.F * fsz
    return d_all, total


def compare(tag, fs, recon_o, dst_o, recon_g, dst_g):
    """the reconstruction first: a failure names the pass that made it"""
    for p in range(3):
        bad = np.argwhere(recon_o[p] != recon_g[p])
        assert not len(bad), "%s: reconstruction differs in plane %d at %d samples, first (picture, row, column) %s" % (tag, p, len(bad), bad[0].tolist())
    for p in range(3):
        assert np.array_equal(dst_o[p], dst_g[p]), "%s: deblocked picture differs in plane %d" % (tag, p)


def run_sets(backend, oracle, sets, run, tag):
    """tiled surfaces, all pictures of `sets` in ONE launch of the run kernel with the run length named (mi355_h264_recon_inter_run_dev), then the intra pass and the loop filter"""
    lib = backend.lib
    devs = [HF.DeviceFrames(backend, fs, tiled=True) for fs in sets]
    d_all = None
    try:
        d_all, total = concat_descriptors(backend, devs)
        mw, mh = max(fs.mb_w for fs in sets), max(fs.mb_h for fs in sets)
        ml = max(fs.max_intra_level for fs in sets)
        widths = [0] * max(1, ml)
        for fs in sets:
            for i, w in enumerate(fs.level_widths[:fs.max_intra_level]):
                widths[i] = max(widths[i], w)
        lw = (C.c_int32 * len(widths))(*widths)
        for name, args in (("mi355_h264_recon_inter_run_dev", (mw, mh, run)), ("mi355_h264_recon_intra_all_dev", (mw, mh, ml, lw)), ("mi355_h264_deblock_layouts_dev", (mw, mh, 2))):
            fn = getattr(lib, name)
            fn.restype = C.c_int
            fn.argtypes = [C.c_void_p, C.c_int] + [C.c_int if isinstance(a, int) else C.c_void_p for a in args] + [C.c_void_p]
            assert fn(d_all, total, *args, None) == 0, name
        lib.mi355_sync.restype = C.c_int
        assert lib.mi355_sync(None) == 0
        for k, (fs, d) in enumerate(zip(sets, devs)):
            recon_o, dst_o = HF.run_oracle(oracle, fs)
            compare("%s[%d]" % (tag, k), fs, recon_o, dst_o, d.fetch(d.recon), d.fetch(d.dst))
    finally:
        if d_all:
            lib.mi355_free(C.c_void_p(d_all))
        for d in devs:
            d.free()


def run_entry_refusals(backend):
    """mi355_h264_recon_inter_run_dev on real descriptors (pictures 17 macroblocks wide): a run the plan refuses returns -1 and leaves the surfaces as they were, a run it takes
    returns 0 on the same descriptors and writes them"""
    lib = backend.lib
    fs = run_kinds_set(4, 17, nframes=2)
    d = HF.DeviceFrames(backend, fs, tiled=True)
    try:
        marker = [np.full_like(a, 0xA5) for a in fs.planes()]
        d.put(d.recon, marker)
        fn = lib.mi355_h264_recon_inter_run_dev
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
        lib.mi355_sync.restype = C.c_int
        # (grid width, run): nothing named; one run of 17 to the row; two runs of 20 / one of 40 in a grid wider than the pictures
        for max_w, run in ((17, 0), (17, -3), (17, 17), (17, 18), (17, 64), (40, 20), (40, 64)):
            assert run_plan(lib, d.F, max_w, fs.mb_h, run) is None or run <= 0, (max_w, run)
            assert fn(d.d_desc, d.F, max_w, fs.mb_h, run, None) == -1, (max_w, run)
        assert lib.mi355_sync(None) == 0
        for got, want in zip(d.fetch(d.recon), marker):
            assert np.array_equal(got, want), "a refused call wrote the reconstruction surface"
        for max_w, run in ((17, 16), (40, 16), (17, 9)):
            assert run_plan(lib, d.F, max_w, fs.mb_h, run) is not None
            assert fn(d.d_desc, d.F, max_w, fs.mb_h, run, None) == 0, (max_w, run)
        assert lib.mi355_sync(None) == 0
        recon_o, _ = HF.run_oracle(backend_oracle(), fs, deblock=False)
        inter = ((fs.mb["mb_type"] & 7) == 0).reshape(fs.F, fs.mb_h, fs.mb_w)
        sel = np.repeat(np.repeat(inter, 16, axis=1), 16, axis=2)
        got = d.fetch(d.recon)[0]
        assert np.array_equal(got[sel], recon_o[0][sel]) and (got[~sel] == 0xA5).all()       # the inter pass alone: intra macroblocks keep the marker
    finally:
        d.free()


def backend_oracle():
    import providers
    return providers.oracle()


def run_modes(backend, oracle, fs, mode, tag, ref=None):
    """mode 'tiled' (the run kernel through the layout entry points), 'linear' (first kernel set), 'wide' (second kernel set at 8 bit)"""
    recon_o, dst_o = ref if ref is not None else HF.run_oracle(oracle, fs)
    d = HF.DeviceFrames(backend, fs, tiled=mode == "tiled")
    try:
        if mode == "tiled":
            d.decode_by_layout()
        elif mode == "wide":
            d.decode_wide()
        else:
            d.decode()
        compare("%s/%s" % (tag, mode), fs, recon_o, dst_o, d.fetch(d.recon), d.fetch(d.dst))
    finally:
        d.free()


MODES = ("tiled", "linear", "wide")

# ---- B: filter extremes ----
PATTERNS = [(p, ph) for p in ("max", "min", "flat255", "checker") for ph in range(6)] + [("flat0", 0)]
FORMS = ("p16", "two", "sub4")
RESIDS = ("none", "clip", "wide")


def extreme_plane(h, w, pattern, phase):
    """cases_qpel_extreme's patterns (tests/cases_h264.py) over a whole plane: rows of 255 0 255 255 0 255 (hi: the horizontal sum 10710) and their complement (lo: -2550),
    stacked so that the vertical filter over the sums reaches 475320 (max) and -214200 (min)"""
    if pattern in ("flat0", "flat255"):
        return np.full((h, w), 255 if pattern == "flat255" else 0, np.uint8)
    base = np.array([255, 0, 255, 255, 0, 255], np.uint8)
    hi = base[(np.arange(w) - phase) % 6]
    rows = {"max": [1, 0, 1, 1, 0, 1], "min": [0, 1, 0, 0, 1, 0], "checker": [1, 0] * 3}[pattern]
    return np.stack([hi if rows[(y + phase) % 6] else 255 - hi for y in range(h)])


def extreme_refs(h, w, pats):
    out = []
    for (p, ph) in pats:
        out.append([tuple(extreme_plane(hh, ww, p, (ph + 3 * s) % 6) for hh, ww in ((h, w), (h // 2, w // 2), (h // 2, w // 2))) for s in range(2)])
    return out


def designed_resid(kind, m, dct8=False):
    """'clip': DC levels that lift every other 4x4 block by 10 and lower the rest (a 255 prediction goes over, a 0 one under: fq_luma_out / fq_chroma_out clip), Cb up and Cr down
    or the other way; 'wide': levels of +-20000 / +-9000, the transform's first pass beyond +-8191 (the 16-bit second pass hands the macroblock to the int form)"""
    cf = np.zeros(384, np.int16)
    if kind == "clip":
        for i in range(16):
            cf[16 * i] = 640 if (i + m) & 1 else -640
        cf[256], cf[320] = (8, -8) if m & 1 else (-8, 8)
    else:
        for i in range(0, 16, 3):
            s = 1 if (i + m) & 1 else -1
            cf[16 * i], cf[16 * i + 1], cf[16 * i + 4] = 20000 * s, -9000 * s, 9000
        cf[256 + 16 * (m % 8) + 1] = 3000
        cf[256] = 700
    return cf


def put_form(fs, f, m, form, vec, n, vary=True):
    """a macroblock of form FORMS[..] whose every partition has vector `vec` but for whole steps of two samples (the fraction stays; vary = False: no steps, every partition's
    window is a part of the one window `vec` names): the references alternate"""
    vx, vy = vec
    s8 = 8 if vary else 0
    if form == "p16":
        put_inter(fs, f, m, 0, [{0: (n % fs.nrefs, (vx, vy))}])
    elif form == "two":
        put_inter(fs, f, m, 1 + n % 2, [{0: (n % fs.nrefs, (vx, vy))}, {0: ((n + 1) % fs.nrefs, (vx + s8 * (1 - 2 * (n & 1)), vy - s8 * (1 - (n & 2))))}])
    else:
        quads = []
        for q in range(4):
            quads.append((3, [{0: ((n + q) % fs.nrefs, (vx + s8 * ((q + k) % 3 - 1), vy + s8 * ((q + 2 * k) % 3 - 1)))} for k in range(4)]))
        put_inter(fs, f, m, 3, quads)


def filter_set(form, resid, pats=PATTERNS):
    """one 8 x 8-macroblock picture per (pattern, phase): macroblock (x, y) has the vector fraction (mx & 7, my & 7) = (x, y) — every luma position four times, every chroma
    position once — and whole parts that keep every window inside the picture"""
    fs = new_set(len(pats), 8, 8, extreme_refs(128, 128, pats))
    for f in range(len(pats)):
        for m in range(64):
            x, y = m % 8, m // 8
            vec = (x + (56 if x < 4 else -56), y + (56 if y < 4 else -56))
            put_form(fs, f, m, form, vec, m + f)
            if resid != "none":
                put_resid(fs, f, m, designed_resid(resid, m))
    return finish(fs)


ALIGN_POS = (0, 2, 8, 10)


def align_set(form, seed=0xB0B):
    """3 x 3 pictures on noise: every whole column offset 0..15 and row offset 0..15 of the window against the tile grid, at positions 0, 2, 8 and 10"""
    combos = [(dx, dy, pos) for pos in ALIGN_POS for dy in range(16) for dx in range(16)]
    n = (len(combos) + 8) // 9
    r = SplitMix64(seed)
    fs = new_set(n, 3, 3, noise_refs(r, n, 2, 48, 48))
    for i in range(9 * n):
        dx, dy, pos = combos[i % len(combos)]
        f, m = i // 9, i % 9
        put_form(fs, f, m, form, (4 * (dx - 8) + (pos & 3), 4 * (dy - 8) + (pos >> 2)), i)
        if i % 3 == 0:
            put_resid(fs, f, m, random_resid(r))
    return finish(fs)


def border_entries(W, H):
    """(first window column ix - 2, first window row iy - 2) of a 21 x 21 window (position 10): its outermost tap column / row one inside, on and one outside each border,
    the four corners, and wholly outside by more than the picture"""
    out = []
    for rel in (1, 0, -1):
        out += [(rel, 8), (W - 1 - 20 - rel, 8), (8, rel), (8, H - 1 - 20 - rel)]
    out += [(-1, -1), (W - 20, -1), (-1, H - 20), (W - 20, H - 20)]
    far = 2 * max(W, H) + 40
    out += [(-far, 8), (far, 8), (8, -far), (8, far), (-far, far), (-far, -far)]
    return out


def border_set(form, mb, seed=0xB0D):
    """mb x mb pictures (3 or 1) on noise, a border entry per macroblock, at positions 0, 2, 8 and 10; every partition of a macroblock has the entry's vector, so the
    partitions along an edge of the macroblock have the designed tap column / row (and fq_two, which predicts the whole macroblock from each vector, the designed window)"""
    W = 16 * mb
    ent = [(e, pos) for pos in ALIGN_POS for e in border_entries(W, W)]
    per = mb * mb
    n = (len(ent) + per - 1) // per
    r = SplitMix64(seed + mb)
    fs = new_set(n, mb, mb, noise_refs(r, n, 2, W, W))
    for i in range(per * n):
        (wx, wy), pos = ent[i % len(ent)]
        f, m = i // per, i % per
        ix, iy = wx + 2, wy + 2
        put_form(fs, f, m, form, (4 * (ix - 16 * (m % mb)) + (pos & 3), 4 * (iy - 16 * (m // mb)) + (pos >> 2)), i, vary=False)
        if i % 2 == 0:
            put_resid(fs, f, m, random_resid(r))
    return finish(fs)


TAPS = np.array([1, -5, 20, 20, -5, 1], np.int64)


def inter_parts(fs, f, m):
    """(list, x, y, w, h, reference slot, vector) of every prediction an inter macroblock makes, in luma samples of the macroblock"""
    rec = fs.mb[f, m]
    sl = fs.slices[f, int(rec["slice_id"])]
    out = []
    for blocks, quads, lists, _ in HF._partitions(rec):
        xs, ys = [b % 4 for b in blocks], [b // 4 for b in blocks]
        for l in lists:
            ri = int(rec["ref_idx"][l][quads[0]])
            out.append((l, 4 * min(xs), 4 * min(ys), 4 * (max(xs) - min(xs) + 1), 4 * (max(ys) - min(ys) + 1), int(sl["ref_slot"][l][ri]), fs.mv[l, f, m, blocks[0]]))
    return out


def window(plane, x0, y0, w, h):
    """emulated_edge_mc: the samples at (x0 .., y0 ..), coordinates clamped to the plane"""
    ys = np.clip(np.arange(y0, y0 + h), 0, plane.shape[0] - 1)
    xs = np.clip(np.arange(x0, x0 + w), 0, plane.shape[1] - 1)
    return plane[np.ix_(ys, xs)].astype(np.int64)


def six(a, axis):
    n = a.shape[axis] - 5
    return sum(int(TAPS[k]) * np.take(a, np.arange(k, k + n), axis=axis) for k in range(6))


def filter_census(fs, form, c=None):
    """the 6-tap sums over the windows the pictures' predictions fetch (h264qpel_template.c restated on whole windows): ranges of H and J, how b, h and j clip, the chroma sums,
    (position, form), window offsets against the tile grid, border classes"""
    c = {} if c is None else c

    def note(*key):
        c[key] = c.get(key, 0) + 1

    def rng(name, a):
        c[name] = (min(c.get(name, (1 << 60, 0))[0], int(a.min())), max(c.get(name, (0, -1 << 60))[1], int(a.max())))

    def clips(name, raw):
        if (raw < 0).any():
            note(*name, "low")
        if (raw > 255).any():
            note(*name, "high")
        if ((raw > 0) & (raw < 255)).any():
            note(*name, "inside")
    W, Hh = fs.W, fs.H
    for f in range(fs.F):
        for m in range(fs.mb_w * fs.mb_h):
            if int(fs.mb[f, m]["mb_type"]) & 7:
                continue
            for (l, px, py, w, h, slot, mv) in inter_parts(fs, f, m):
                mx, my = int(mv[0]) + 64 * (m % fs.mb_w) + 4 * px, int(mv[1]) + 64 * (m // fs.mb_w) + 4 * py
                fx, fy, ix, iy = mx & 3, my & 3, mx >> 2, my >> 2
                note("pos", fx | fy << 2, form)
                note("col_offset", (ix - px - 4) & 15)
                note("row_offset", (iy - py) & 15)
                if fx == 2 and fy == 2:
                    # the prediction's own window: columns ix - 2 .. ix + w + 2, rows iy - 2 .. iy + h + 2
                    lo_x, lo_y, hi_x, hi_y = ix - 2, iy - 2, W - 1 - (ix + w + 2), Hh - 1 - (iy + h + 2)
                    for side, v in (("left", lo_x), ("top", lo_y), ("right", hi_x), ("bottom", hi_y)):
                        if v in (1, 0, -1):
                            note("border", form, side, v)
                    if (lo_x < 0 or hi_x < 0) and (lo_y < 0 or hi_y < 0):
                        note("border", form, "corner", (lo_x < 0) + 2 * (lo_y < 0))
                    if ix + w + 2 < -W or lo_x > 2 * W or iy + h + 2 < -Hh or lo_y > 2 * Hh:
                        note("border", form, "far", (ix < 0) + 2 * (iy < 0))
                y_pl, cb, cr = fs.refs[f][slot]
                win = window(y_pl, ix - 2, iy - 2, w + 5, h + 5)
                # mc10..mc33: b where fx != 0 and fy != 2 (row iy, or iy + 1 at fy 3); h where fy != 0 and fx != 2 (column ix, or ix + 1 at fx 3); j on the centre cross
                if fx and fy != 2:
                    r0 = 2 + (fy == 3)
                    clips(("b", form), (six(win[r0:r0 + h], 1) + 16) >> 5)
                if fy and fx != 2:
                    c0 = 2 + (fx == 3)
                    clips(("h", form), (six(win[:, c0:c0 + w], 0) + 16) >> 5)
                if (fx == 2 and fy) or (fy == 2 and fx):
                    hs = six(win, 1)                          # (h + 5, w): the horizontal sums of every window row, as the low / high byte planes carry them
                    J = six(hs, 0)
                    rng(("H", form), hs)
                    rng(("J", form), J)
                    clips(("j", form), (J + 512) >> 10)
                cxm, cym = mx & 7, my & 7
                for pl in (cb, cr):
                    cw = window(pl, mx >> 3, my >> 3, w // 2 + 1, h // 2 + 1)
                    s = (8 - cxm) * (8 - cym) * cw[:-1, :-1] + cxm * (8 - cym) * cw[:-1, 1:] + (8 - cxm) * cym * cw[1:, :-1] + cxm * cym * cw[1:, 1:]
                    rng("chroma", s)
                    note("chroma_pos", cxm, cym)
    return c


# ---- C: weights ----
WEIGHTS, OFFSETS = (-128, -1, 0, 1, None, 127), (-128, 0, 127)         # None: 1 << denominator, the identity
IMPLICIT = (-64, -1, 0, 31, 32, 33, 64, 128)
W_SHAPES = ("16x16", "16x8", "8x16", "8x8", "8x4", "4x8", "4x4")


def mixed_refs(r, nframes, nrefs, H, W):
    """noise with flat 0 and flat 255 regions of 16 x 16 (8 x 8 in chroma)"""
    out = []
    for f in range(nframes):
        pics = []
        for s in range(nrefs):
            planes = []
            for (h, w, b) in ((H, W, 16), (H // 2, W // 2, 8), (H // 2, W // 2, 8)):
                a = r.u8((h, w))
                yy, xx = np.mgrid[0:h, 0:w]
                sel = (xx // b + 2 * (yy // b) + s + f) % 5
                a[sel == 0] = 0
                a[sel == 1] = 255
                planes.append(a)
            pics.append(tuple(planes))
        out.append(pics)
    return out


def put_weight_mb(fs, r, f, m, shape, lists, refs, slice_id):
    """shape of W_SHAPES predicted from `lists` ((0,), (1,) or (0, 1)) with reference index refs[l] (first partition / quadrant; the others step on by one)"""
    mv = lambda: (r.randint(-40, 40), r.randint(-40, 40))
    pred = lambda k: {l: ((refs[l] + k) % fs.nrefs, mv()) for l in lists}
    si = W_SHAPES.index(shape)
    if si < 3:
        put_inter(fs, f, m, si, [pred(k) for k in range(1 if si == 0 else 2)], slice_id=slice_id, weighted=True)
    else:
        sub = si - 3
        put_inter(fs, f, m, 3, [(sub, [pred(q) for _ in SUBPARTS[sub]]) for q in range(4)], slice_id=slice_id, weighted=True)


def explicit_set(bframes, seed=0xC0DE):
    """a slice per (denominator d, use_weight_chroma): luma denominator d, chroma 7 - d; a macroblock row is a slice.  B: each slice holds every shape from list 0, list 1 and both;
    P: every shape from list 0.  Weights and offsets from WEIGHTS / OFFSETS by reference and list; the chroma tables hold other values than the identity also where
    use_weight_chroma is 0 (a uni-predicted block must then leave chroma as predicted: mc_part_weighted, h264_mb.c)"""
    dirs = [(0,), (1,), (0, 1)] if bframes else [(0,)]
    mb_w, mb_h, nrefs = 7 * len(dirs), 16, 6
    r = SplitMix64(seed + bframes)
    fs = new_set(1, mb_w, mb_h, mixed_refs(r, 1, nrefs, 16 * mb_h, 16 * mb_w), bframes=bframes, nslices=16)
    for s in range(16):
        d, uwc = s >> 1, s & 1
        sl = fs.slices[0, s]
        sl["use_weight"], sl["use_weight_chroma"], sl["luma_denom"], sl["chroma_denom"] = 1, uwc, d, 7 - d
        for ref in range(nrefs):
            for l in range(2):
                w = WEIGHTS[(ref + 2 * l + s) % 6]
                sl["luma_weight"][ref, l] = (1 << d if w is None else w, OFFSETS[(ref + l + s) % 3])
                for p in range(2):
                    w = WEIGHTS[(ref + l + p + 3 * s + 1) % 6]
                    sl["chroma_weight"][ref, l, p] = (1 << (7 - d) if w is None else w, OFFSETS[(ref + 2 * l + p + s + 1) % 3])
        for x in range(mb_w):
            lists = dirs[x // 7]
            put_weight_mb(fs, r, 0, s * mb_w + x, W_SHAPES[x % 7], lists, {l: (x + s + 3 * l) % nrefs for l in lists}, s)
    return finish(fs)


def implicit_set(seed=0xC1DE):
    """B picture, use_weight 2: implicit_weight[r0][r1] runs over IMPLICIT; every (r0, r1) pair bi-predicted in every shape, a column of list-0-only macroblocks beside them"""
    nrefs = 4
    mb_w, mb_h = 8, 16
    r = SplitMix64(seed)
    fs = new_set(1, mb_w, mb_h, mixed_refs(r, 1, nrefs, 16 * mb_h, 16 * mb_w), bframes=True)
    sl = fs.slices[0, 0]
    sl["use_weight"], sl["use_weight_chroma"] = 2, 1
    sl["implicit_weight"] = 32
    for r0 in range(nrefs):
        for r1 in range(nrefs):
            sl["implicit_weight"][r0, r1] = IMPLICIT[(3 * r0 + r1) % 8]
    for y in range(mb_h):
        for x in range(mb_w):
            lists = (0, 1) if x < 7 else ((0,) if y & 1 else (1,))
            put_weight_mb(fs, r, 0, y * mb_w + x, W_SHAPES[x % 7], lists, {0: y // 4, 1: y % 4}, 0)
    return finish(fs)


def variant(fs, lists=None, weighted=True):
    """a copy of the set with every inter macroblock's prediction cut down to the lists named, or its weights switched off: what the census computes the weighted samples from"""
    import copy
    g = copy.copy(fs)
    g.mb, g.slices = fs.mb.copy(), fs.slices.copy()
    if not weighted:
        g.slices["use_weight"] = 0
        g.mb["flags"] &= ~np.uint8(HF.F_WEIGHTED)
    if lists is not None:
        drop = 1 - lists[0]
        g.mb["ref_idx"][:, :, drop, :] = -1
        g.mb["i4mode"][:, :, 4 * drop:4 * drop + 4] = -1
        g.mb["mb_type"] &= ~np.uint32((HF.P0L0 | HF.P1L0) << (2 * drop))
        g.mb["sub"] &= ~np.uint8(0x10 << drop)
    return g


def weight_census(oracle, fs, c=None):
    """Which weights the set runs, and where the weighted samples fall: the unweighted predictions of list 0 and list 1 come from the oracle itself (the set with its weights off and
    one list kept), the weight formulas (h264dsp_template.c:30-98) are restated here — and must give the oracle's own reconstruction of the weighted set (no residual anywhere)"""
    c = {} if c is None else c

    def note(*key):
        c[key] = c.get(key, 0) + 1
    assert not fs.mb["cbp"].any()
    full, _ = HF.run_oracle(oracle, fs, deblock=False)
    has = lambda l: (fs.mb["ref_idx"][0, :, l, :] >= 0).any()
    pred = {l: HF.run_oracle(oracle, variant(fs, (l,), False), deblock=False)[0] for l in range(2) if has(l) and (l == 0 or fs.use_l1)}
    for m in range(fs.mb_w * fs.mb_h):
        rec = fs.mb[0, m]
        sl = fs.slices[0, int(rec["slice_id"])]
        mode = int(sl["use_weight"])
        note("use_weight_chroma", int(sl["use_weight_chroma"]))
        x0, y0 = 16 * (m % fs.mb_w), 16 * (m // fs.mb_w)
        seen = set()
        for (l, px, py, w, h, slot, mv) in inter_parts(fs, 0, m):
            if (px, py) in seen:
                continue
            seen.add((px, py))
            q = (px >> 3) + 2 * (py >> 3)
            refn = [int(rec["ref_idx"][k][q]) for k in range(2)]
            lists = [k for k in range(2) if refn[k] >= 0]
            bi = len(lists) == 2
            note("width", "luma", w)
            note("width", "chroma", w // 2)
            for p in range(3):
                sx, sy, sw, sh = (x0 + px, y0 + py, w, h) if p == 0 else ((x0 + px) // 2, (y0 + py) // 2, w // 2, h // 2)
                P = [pred[k][p][0, sy:sy + sh, sx:sx + sw].astype(np.int64) if k in lists else None for k in range(2)]
                plane = "luma" if p == 0 else "chroma"
                if mode == 2:
                    if not bi:
                        raw = P[lists[0]]
                    else:
                        w0 = int(sl["implicit_weight"][refn[0], refn[1]])
                        if p == 0:
                            note("implicit", w0)
                        raw = (P[0] + P[1] + 1) >> 1 if w0 == 32 else (P[0] * w0 + P[1] * (64 - w0) + (1 << 5)) >> 6
                else:
                    d = int(sl["luma_denom"] if p == 0 else sl["chroma_denom"])
                    tab = (lambda k: sl["luma_weight"][refn[k], k]) if p == 0 else (lambda k: sl["chroma_weight"][refn[k], k, p - 1])
                    if bi:
                        (w0, o0), (w1, o1) = [(int(v[0]), int(v[1])) for v in (tab(0), tab(1))]
                        raw = (P[0] * w0 + P[1] * w1 + ((((o0 + o1) + 1) | 1) << d)) >> (d + 1)
                        note("denom", plane, d, "bi")
                    elif p and not int(sl["use_weight_chroma"]):
                        raw = P[lists[0]]
                        note("chroma_left_alone", lists[0])
                    else:
                        k = lists[0]
                        wk, ok = int(tab(k)[0]), int(tab(k)[1])
                        raw = ((P[k] * wk + (1 << (d - 1))) >> d) + ok if d else P[k] * wk + ok
                        note("denom", plane, d, "l%d" % k)
                got = full[p][0, sy:sy + sh, sx:sx + sw]
                assert np.array_equal(np.clip(raw, 0, 255), got), ("the census restates the weights otherwise than the oracle", m, p, px, py)
                kind = "bi" if bi else "uni"
                if (raw < 0).any():
                    note("clip", plane, kind, "low")
                if (raw > 255).any():
                    note("clip", plane, kind, "high")
                if ((raw > 0) & (raw < 255)).any():
                    note("clip", plane, kind, "inside")
    return c


# ---- the tables' entries: name -> builder; a set and its oracle pictures are made once per process ----
B_ENTRIES = {"extreme-%s-%s" % (form, resid): (lambda form=form, resid=resid: filter_set(form, resid)) for form in FORMS for resid in RESIDS}
B_ENTRIES.update({"align-%s" % form: (lambda form=form: align_set(form)) for form in FORMS})
B_ENTRIES.update({"border%d-%s" % (mb, form): (lambda form=form, mb=mb: border_set(form, mb)) for form in FORMS for mb in (3, 1)})
C_ENTRIES = {"explicit-p": lambda: explicit_set(False), "explicit-b": lambda: explicit_set(True), "implicit-b": implicit_set}
_SETS = {}


def entry(oracle, name):
    """(set, (recon, dst) of the oracle) of a B or C entry"""
    if name not in _SETS:
        fs = (B_ENTRIES.get(name) or C_ENTRIES[name])()
        _SETS[name] = (fs, HF.run_oracle(oracle, fs))
    return _SETS[name]


def run_entry(backend, oracle, name, mode):
    fs, ref = entry(oracle, name)
    run_modes(backend, oracle, fs, mode, name, ref)


def run_length_entry(backend, oracle, run, widths):
    sets = [run_kinds_set(run, w) for w in widths]
    run_sets(backend, oracle, sets, run, "run %d, width %s" % (run, "+".join(str(w) for w in widths)))
