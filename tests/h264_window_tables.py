"""Directed tables for the luma window request of the tiled run kernel (fq_need, fq_windows_issue*, fq_windows_patch in h264_recon_fast.h): the request leaves out
the tile columns and rows of the 21 x 3 window that the vector's position does not read, so what lies in their place in LDS is whatever an earlier macroblock left there.
  phase_set    every (position, column phase o, window row phase) of a plain 16x16 macroblock whose windows lie inside the picture;
  edge_set     windows over each border in pictures 2 and 3 macroblocks wide, at every o, for positions with and without either filter;
  two_set      16x8 / 8x16 macroblocks whose partitions need different pieces;
  need / lines the rule restated in python, and the 128-byte lines a request touches (the census).
Everything is built from fixed seeds and compared with HF.run_oracle sample for sample."""
import h264_frames as HF
import h264_run_tables as T
from rng import SplitMix64


# ---- the rule, restated ----
def need(pos, o):
    """(tile columns of the window as a 3-bit mask, first window row, last window row) the prediction at `pos` = (mx & 3) | (my & 3) << 2 reads at column phase o = (ix - 4) & 15"""
    first, last = (o + 2, o + 22) if pos & 3 else (o + 4, o + 19)
    tiles = sum(1 << t for t in range(3) if first <= 16 * t + 15 and last >= 16 * t)
    return (tiles, 0, 20) if pos >> 2 else (tiles, 2, 17)


def lines(tiles, r0, r1, y0, t0, mb_w, mb_h):
    """the 128-byte lines (tile row, tile column, half) a request for window rows r0 .. r1 of the tile columns in `tiles` touches; rows and tile columns clamped as the fetch clamps them"""
    out = set()
    for r in range(r0, r1 + 1):
        y = min(max(y0 + r, 0), 16 * mb_h - 1)
        for t in range(3):
            if tiles >> t & 1:
                out.add((y >> 4, min(max(t0 + t, 0), mb_w - 1), (y & 15) >> 3))
    return out


def window_origin(mv, x, y):
    """(o, position, first window row iy - 2, first tile column t0) of a list-0 vector of macroblock (x, y): fq_geometry"""
    mx, my = int(mv[0]) + 64 * x, int(mv[1]) + 64 * y
    ix, iy = mx >> 2, my >> 2
    return (ix - 4) & 15, (mx & 3) | (my & 3) << 2, iy - 2, (ix - 4) >> 4


# ---- content ----
def headline_resid(r):
    """coefficients as the headline's generator codes them (HF.synth_frames_fast): each of the 24 blocks with probability one half, chroma DC levels two times in three"""
    HF.COEF_B[0], HF.COEF_CLIP[0] = 24, 2047
    blks, _ = HF._gen_block_coefs(r, 24, "sparse")
    cf = blks.reshape(-1).copy()
    mode = r.randint(0, 2)
    if mode < 2:
        cf[256:] = 0
    cf[256:384:16] = r.laplace_int(30, 8, 2047) if mode else 0
    return cf


def vector(x, y, ix, iy, pos):
    return (4 * (ix - 16 * x) + (pos & 3), 4 * (iy - 16 * y) + (pos >> 2))


PHASE_W, PHASE_H, PHASE_F = 16, 8, 16
ORDERS = {"as built": lambda x: x, "reversed": lambda x: PHASE_W - 1 - x, "stride 5": lambda x: (5 * x + 3) % PHASE_W}


def phase_combo(i):
    """entry i of the 2048: (position, o, window row phase); neighbours in a row differ in all three"""
    c = (i * 1237 + 77) % 2048
    return c & 15, (c >> 4) & 15, c >> 8


def phase_set(order="as built", seed=0xF00D):
    """sixteen pictures 16 x 8 macroblocks on noise: macroblock (x, y) of picture f is entry 128 f + 16 y + order(x) — plain 16x16 from list 0, its luma window's three tile
    columns and 21 rows and its chroma window inside the picture (FQA_INSIDE), coefficients as the headline codes them"""
    r = SplitMix64(seed)
    fs = T.new_set(PHASE_F, PHASE_W, PHASE_H, T.noise_refs(r, PHASE_F, 2, 16 * PHASE_H, 16 * PHASE_W))
    perm = ORDERS[order]
    seen = set()
    for f in range(PHASE_F):
        for m in range(PHASE_W * PHASE_H):
            x, y = m % PHASE_W, m // PHASE_W
            i = 128 * f + 16 * y + perm(x)
            pos, o, rp = phase_combo(i)
            t0 = min(max(x - 1 + (i >> 4 & 1), 0), PHASE_W - 3)
            j = min(max(2 * y - 1 + (i >> 5 & 3), 0), (16 * PHASE_H - 21 - rp) // 8)
            mv = vector(x, y, 16 * t0 + 4 + o, 8 * j + rp + 2, pos)
            T.put_inter(fs, f, m, 0, [{0: (i % 2, mv)}])
            assert T.geometry(mv, x, y, PHASE_W, PHASE_H) == (False, True)
            og, pg, y0, _ = window_origin(mv, x, y)
            assert (og, pg, y0 & 7) == (o, pos, rp)
            seen.add((pos, o, rp))
            # the content is the entry's, whatever its place in the row
            T.put_resid(fs, f, m, headline_resid(SplitMix64(seed + 7919 * i)))
    assert len(seen) == 2048
    return T.finish(fs)


EDGE_POS = (0, 2, 8, 15)            # no filter, horizontal, vertical, both
SIDES = ("left", "right", "top", "bottom")


def edge_set(mb_w, seed=0xED6E):
    """pictures mb_w (2 or 3) x 3 macroblocks on noise: per (side, position, o) one plain 16x16 macroblock whose luma window lies over that border.  left: first tile column -1
    (fetched from tile 0 and replicated: fq_windows_patch); right: first tile column mb_w - 2, the third beyond the picture; top / bottom: first tile column 0 — where the
    picture is 2 wide the window's second and third tile column are the same tile — rows clamped in the fetch.  Rows and vertical placement vary with the entry."""
    mb_h = 3
    ent = [(side, pos, o) for side in SIDES for pos in EDGE_POS for o in range(16)]
    per = mb_w * mb_h
    n = (len(ent) + per - 1) // per
    r = SplitMix64(seed + mb_w)
    fs = T.new_set(n, mb_w, mb_h, T.noise_refs(r, n, 2, 16 * mb_h, 16 * mb_w))
    census = {}
    for i in range(per * n):
        side, pos, o = ent[i % len(ent)]
        f, m = i // per, i % per
        x, y = m % mb_w, m // mb_w
        t0 = {"left": -1, "right": mb_w - 2}.get(side, 0)
        y0 = {"top": -3 - i % 8, "bottom": 16 * mb_h - 19 + i % 8}.get(side, 5 * i % 28)
        mv = vector(x, y, 16 * t0 + 4 + o, y0 + 2, pos)
        T.put_inter(fs, f, m, 0, [{0: (i % 2, mv)}])
        patched, inside = T.geometry(mv, x, y, mb_w, mb_h)
        assert not inside and (patched or (side in ("top", "bottom") and mb_w == 3))
        key = (side, "patched" if patched else "clamped", bin(need(pos, o)[0]))
        census[key] = census.get(key, 0) + 1
        if i % 2 == 0:
            T.put_resid(fs, f, m, headline_resid(r))
    return T.finish(fs), census


# (position, o) of the first partition, of the second: the designed pair first, then every o at the four positions against another o — those whose pieces differ
TWO_PAIRS = [(0, 12, 15, 11)] + [p for p in ((EDGE_POS[k % 4], o, EDGE_POS[(k + 1 + o // 4) % 4], (o + 5) & 15) for k in range(4) for o in range(16)) if need(p[0], p[1]) != need(p[2], p[3])]
assert len(TWO_PAIRS) > 40


def two_set(seed=0x2B0):
    """a picture 16 x 9 macroblocks (windows inside) and pictures 3 x 3 (windows over the left and right border): 16x8 and 8x16 macroblocks whose first partition has
    (position, o) and whose second has another pair (TWO_PAIRS: no filter and o = 12 — tile column 1 alone — beside both filters and o = 11 first)"""
    r = SplitMix64(seed)
    ent = [(shape, p) for p in TWO_PAIRS for shape in (1, 2)]
    sets = []
    big = T.new_set(1, 16, 9, T.noise_refs(r, 1, 2, 144, 256))
    for m, (shape, (p0, o0, p1, o1)) in enumerate(ent):
        x, y = m % 16, m // 16
        t0 = min(max(x - 1, 0), 13)
        iy = min(max(16 * y - 3 + m % 7, 2), 16 * 9 - 20)
        mvs = [vector(x, y, 16 * t0 + 4 + o, iy + k, p) for k, (p, o) in enumerate(((p0, o0), (p1, o1)))]
        assert all(T.geometry(mv, x, y, 16, 9) == (False, True) for mv in mvs) and need(p0, o0) != need(p1, o1)
        T.put_inter(big, 0, m, shape, [{0: (m % 2, mvs[0])}, {0: ((m + 1) % 2, mvs[1])}])
        if m % 2:
            T.put_resid(big, 0, m, headline_resid(r))
    for m in range(len(ent), 16 * 9):
        T.put_i16(big, 0, m)
    sets.append(T.finish(big))
    n = (len(ent) + 8) // 9
    small = T.new_set(n, 3, 3, T.noise_refs(r, n, 2, 48, 48))
    for i in range(9 * n):
        shape, (p0, o0, p1, o1) = ent[i % len(ent)]
        f, m = i // 9, i % 9
        x, y = m % 3, m // 3
        # first partition over the left border and the second over the right one, or the other way round
        ta, tb = (-1, 1) if i & 1 else (1, -1)
        mvs = [vector(x, y, 16 * t + 4 + o, 3 + 3 * i % 23, p) for t, (p, o) in ((ta, (p0, o0)), (tb, (p1, o1)))]
        assert all(T.geometry(mv, x, y, 3, 3)[0] for mv in mvs)
        T.put_inter(small, f, m, shape, [{0: (i % 2, mvs[0])}, {0: ((i + 1) % 2, mvs[1])}])
        if i % 2 == 0:
            T.put_resid(small, f, m, headline_resid(r))
    sets.append(T.finish(small))
    return sets


# ---- running: a set and the oracle's pictures of it are made once per process ----
_SETS = {}


def entry(oracle, name, build):
    if name not in _SETS:
        sets = build()
        sets = sets if isinstance(sets, list) else [sets]
        _SETS[name] = (sets, [HF.run_oracle(oracle, fs) for fs in sets])
    return _SETS[name]


def run_named(backend, sets, refs, run, tag):
    """T.run_sets against pictures of the oracle made before (entry): while it runs, HF.run_oracle answers with them instead of decoding the set again"""
    made = {id(fs): ref for fs, ref in zip(sets, refs)}
    real = HF.run_oracle
    HF.run_oracle = lambda oracle, fs: made[id(fs)]
    try:
        T.run_sets(backend, None, sets, run, tag)
    finally:
        HF.run_oracle = real


def run_phase(backend, oracle, order, run):
    sets, refs = entry(oracle, "phase/" + order, lambda: phase_set(order))
    run_named(backend, sets, refs, run, "phase table, %s, run %d" % (order, run))


def run_edges(backend, oracle, mb_w, run):
    sets, refs = entry(oracle, "edge%d" % mb_w, lambda: edge_set(mb_w)[0])
    run_named(backend, sets, refs, run, "edges, %d wide, run %d" % (mb_w, run))


def run_two(backend, oracle, run):
    sets, refs = entry(oracle, "two", two_set)
    for k, (fs, ref) in enumerate(zip(sets, refs)):          # two launches: the pictures differ in height as well as width
        run_named(backend, [fs], [ref], min(run, fs.mb_w), "two partitions[%d], run %d" % (k, run))


PHASE_CASES = [("as built", 1), ("as built", 4), ("as built", 15), ("reversed", 4), ("stride 5", 15)]
