"""The tiled loop filter's step addressing on the smallest pictures at which it can go wrong: a table of P and B pictures of 1 .. 9 by
1 .. 9 macroblocks with the loop filter's hard content (deblock_cases._LF), a runner that sends the oracle's reconstruction through the
two tiled forms, and a census of which edge classes that content changes, read off the oracle's (recon, dst) alone.

Widths: W < 7 never has the four groups of a wave inside the row together; W = 5 .. 8 gives the W + 7 steps of a band every residue
modulo 4 and modulo 2 (every ring slot as the last one).  Heights: 1 = a single row (nothing above, nothing handed down), 4 = one full
band, 5 = a second band with one live row, 8 and 9 = two and three bands with the hand-down on the last columns."""
import numpy as np

import deblock_cases as D
import h264_frames as HF

WIDTHS = (1, 2, 3, 5, 6, 7, 8, 9)
HEIGHTS = (1, 4, 5, 8, 9)
SHAPES = [(w, h) for w in WIDTHS for h in HEIGHTS]
FORMS = [(True, 1, 0), (True, 2, 0)]          # k_deblock_tiled, k_deblock_tiled2
CLASSES = ("left_mb_edge", "inner_vertical_edge", "top_mb_edge", "inner_horizontal_edge", "chroma_vertical_edge", "chroma_horizontal_edge",
           "bs4_edge", "band_boundary_edge", "mb_unchanged")


def kwargs(w, h, b):
    """synth_frames arguments of the P (b = 0) or B (b = 1) picture of a shape: references of threshold steps or smooth ones in turn,
    two or three slices, intra, PCM and 8x8-transform macroblocks, half of the inter macroblocks without residual, vectors on the bS thresholds"""
    i = SHAPES.index((w, h))
    smooth = (i + b) & 1
    return dict(D._LF, nframes=1, mb_w=w, mb_h=h, seed=0x5700 + 2 * i + b, bframes=bool(b), intra_frac=0.12, pcm_frac=0.1, dct8_frac=0.4,
                refs="smooth" if smooth else "steps", coef_b=6 if smooth else 24, slices=2 + (i % 2), full_sample=bool(i & 2), near_mv=0.6,
                cbp0_frac=0.5)


_cache = {}


def case(w, h, b):
    """(FrameSet, oracle recon, oracle dst), made once per process and not changed by anyone"""
    if (w, h, b) not in _cache:
        import providers
        fs = HF.synth_frames(**kwargs(w, h, b))
        _cache[(w, h, b)] = (fs,) + tuple(HF.run_oracle(providers.oracle(), fs))
    return _cache[(w, h, b)]


def run_shape(backend, w, h):
    for b in (0, 1):
        fs, recon_o, dst_o = case(w, h, b)
        D.run_frameset_forms(backend, fs, dst_o, "%dx%d %s" % (w, h, "B" if b else "P"), FORMS, recon=recon_o)


def edge_classes(fs, recon, dst, c=None):
    """Adds to c, per class of CLASSES, the macroblocks of a picture set in which the oracle's filter changed a sample that only an edge of
    that class can have changed.  Positions no other edge reaches:
      - a macroblock with the 8x8 transform filters luma edges 0 and 8 only: a horizontal edge touches at most three rows either side,
        so its rows 3, 4, 11, 12 are touched by vertical edges alone (and its columns 3, 4, 11, 12 by horizontal ones alone).  There,
        columns 0 / 15 belong to a left macroblock edge (its own / its right neighbour's), columns 5 .. 10 to the inner edge 8, and columns
        2 / 13 (p2 / q2 of a macroblock edge) change under the bS 4 filter only;
      - a chroma edge changes p0 and q0 only (columns or rows 7 | 0 and 3 | 4): chroma rows 1, 2, 5, 6 change under vertical edges alone,
        chroma columns 1, 2, 5, 6 under horizontal ones;
      - a top macroblock edge of a row 4k > 0 lies across a band boundary (the rows above came through the hand-down)."""
    c = {} if c is None else c

    def add(k, yes):
        c[k] = c.get(k, 0) + int(bool(yes))
    lone, mid, far = [3, 4, 11, 12], slice(5, 11), [2, 13]
    clone = [1, 2, 5, 6]
    for f in range(fs.F):
        ch = [recon[p][f] != dst[p][f] for p in range(3)]
        dct8 = (fs.mb[f]["mb_type"] & HF.DCT8) != 0
        for m in range(fs.mb_w * fs.mb_h):
            mx, my = m % fs.mb_w, m // fs.mb_w
            Y = ch[0][16 * my:16 * my + 16, 16 * mx:16 * mx + 16]
            UV = [ch[p][8 * my:8 * my + 8, 8 * mx:8 * mx + 8] for p in (1, 2)]
            add("mb_unchanged", not (Y.any() or UV[0].any() or UV[1].any()))
            band_top, band_bottom = my > 0 and my % 4 == 0, my + 1 < fs.mb_h and (my + 1) % 4 == 0
            boundary = False
            if dct8[m]:
                add("left_mb_edge", Y[lone][:, [0, 15]].any())
                add("inner_vertical_edge", Y[lone][:, mid].any())
                add("top_mb_edge", Y[[0, 15]][:, lone].any())
                add("inner_horizontal_edge", Y[mid][:, lone].any())
                add("bs4_edge", Y[lone][:, far].any() or Y[far][:, lone].any())
                boundary = (band_top and Y[[0, 2]][:, lone].any()) or (band_bottom and Y[[13, 15]][:, lone].any())
            add("chroma_vertical_edge", any(u[clone].any() for u in UV))
            add("chroma_horizontal_edge", any(u[:, clone].any() for u in UV))
            boundary = boundary or (band_top and any(u[0, clone].any() for u in UV)) or (band_bottom and any(u[7, clone].any() for u in UV))
            add("band_boundary_edge", boundary)
    return c


def table_census():
    """(edge classes, deblock_cases.census) over the whole table"""
    if "census" not in _cache:
        ec, cen = {}, {}
        for w, h in SHAPES:
            for b in (0, 1):
                fs, recon, dst = case(w, h, b)
                edge_classes(fs, recon, dst, ec)
                D.census(fs, recon, dst, cen)
        _cache["census"] = (ec, cen)
    return _cache["census"]
