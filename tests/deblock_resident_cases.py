"""k_deblock_tiled as resident waves (mi355_h264_deblock_resident_dev): a launch of `resident_waves` waves that take the batch's bands in
turn.  A table of small batches, each run with 1, 2, 4, tickets - 1, tickets, tickets + 5 waves and with the rule's count (0), every sample
of dst against the oracle.

Shapes: 3 x 9 macroblocks (three bands, the last of one row) and 1 x 5 (two bands of eight steps); 1, 5 and 7 pictures: 2 .. 21 tickets.
What the loop over tickets, and only it, can get wrong, a batch each: a short picture in a tall grid (its missing bands' tickets are
skipped), a line-stride picture in a tiled launch (all of its tickets are), P and B pictures in turn (one wave runs both instantiations),
the same launch twice on a stream (the counters zeroed again, a wave's LDS left over from its previous band), smooth content (the
hand-down between bands carries changed samples)."""
import ctypes as C

import deblock_cases as D
import h264_frames as HF


def _kw(w, h, n, seed, b=False, smooth=False):
    return dict(D._LF, nframes=n, mb_w=w, mb_h=h, seed=seed, bframes=b, intra_frac=0.12, pcm_frac=0.1, dct8_frac=0.4,
                refs="smooth" if smooth else "steps", coef_b=4 if smooth else 24, slices=2, full_sample=not smooth, near_mv=0.6, cbp0_frac=0.5)


# picture sets: name -> synth_frames arguments
SETS = {
    "p39x1": _kw(3, 9, 1, 0x5901), "p39x4": _kw(3, 9, 4, 0x5902), "p39x5": _kw(3, 9, 5, 0x5903), "p39x7s": _kw(3, 9, 7, 0x5904, smooth=True),
    "b39x3": _kw(3, 9, 3, 0x5905, b=True), "p34x1": _kw(3, 4, 1, 0x5906), "p39x1s": _kw(3, 9, 1, 0x5907, smooth=True),
    "p15x1": _kw(1, 5, 1, 0x5908), "p15x5": _kw(1, 5, 5, 0x5909, smooth=True), "b15x7": _kw(1, 5, 7, 0x590A, b=True),
}
# batch name -> ([(set, tiled)], launches): the sets' pictures are dealt into the batch in turn (P, B, P, B, ...)
BATCHES = {
    "3x9_one_picture": ([("p39x1", True)], 1),
    "3x9_five_pictures": ([("p39x5", True)], 1),
    "3x9_seven_smooth": ([("p39x7s", True)], 1),
    "1x5_one_picture": ([("p15x1", True)], 1),
    "1x5_five_smooth": ([("p15x5", True)], 1),
    "1x5_seven_b": ([("b15x7", True)], 1),
    "mixed_heights": ([("p39x4", True), ("p34x1", True)], 1),
    "mixed_layouts": ([("p39x4", True), ("p39x1s", False)], 1),
    "mixed_lists": ([("p39x4", True), ("b39x3", True)], 1),
    "repeat_launch": ([("p39x5", True)], 2),
    "repeat_launch_mixed_lists": ([("p39x4", True), ("b39x3", True)], 2),
}

_cache = {}


def pictures(name):
    """(FrameSet, oracle recon, oracle dst) of a set, made once per process and not changed by anyone"""
    if name not in _cache:
        import providers
        fs = HF.synth_frames(**SETS[name])
        _cache[name] = (fs,) + tuple(HF.run_oracle(providers.oracle(), fs))
    return _cache[name]


def order(parts):
    """the batch's pictures as (part, picture of the part), dealt in turn"""
    sizes = [SETS[n]["nframes"] for n, _ in parts]
    return [(k, i) for i in range(max(sizes)) for k in range(len(parts)) if i < sizes[k]]


def grid(parts):
    """(pictures, largest width, largest height, bands, tickets, layouts) of a batch"""
    n = sum(SETS[s]["nframes"] for s, _ in parts)
    mw, mh = max(SETS[s]["mb_w"] for s, _ in parts), max(SETS[s]["mb_h"] for s, _ in parts)
    layouts = 0
    for _, tiled in parts:
        layouts |= D.LAYOUT_TILED if tiled else D.LAYOUT_LINEAR
    nbands = (mh + 3) // 4
    return n, mw, mh, nbands, n * nbands, layouts


def resident_counts(tickets):
    """the counts a batch of `tickets` bands runs with: a single wave (every band in ticket order), a few, one fewer than the bands, a wave
    per band, more than that (the launch stays a wave per band), and 0 = the rule's choice"""
    return [1, 2, 4, tickets - 1, tickets, tickets + 5, 0]


def bind(lib):
    D._bind(lib)
    lib.mi355_h264_deblock_resident_dev.restype = C.c_int
    lib.mi355_h264_deblock_resident_dev.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p]
    lib.mi355_h264_deblock_resident.restype = C.c_int
    lib.mi355_h264_deblock_resident.argtypes = [C.c_int] * 6 + [C.c_void_p]
    lib.mi355_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]


def rule(lib, nframes, mb_w, mb_h, layouts, cus, shares):
    """mi355_h264_deblock_resident -> the count, or None for arguments it rejects"""
    bind(lib)
    n = C.c_int(-7)
    return n.value if lib.mi355_h264_deblock_resident(nframes, mb_w, mb_h, layouts, cus, shares, C.byref(n)) == 0 else None


def run_batch(backend, name):
    """a batch of BATCHES with every count of resident_counts(), every sample of every picture's dst against the oracle after the last launch
    (a repeated launch: dst holds the unfiltered pictures again before the second one, and nothing waits in between)"""
    lib = backend.lib
    bind(lib)
    parts, launches = BATCHES[name]
    sets = [pictures(s) for s, _ in parts]
    devs = [D.upload(backend, s[0], s[1], tiled) for s, (_, tiled) in zip(sets, parts)]
    try:
        fsz = C.sizeof(HF.Frame)
        total, mw, mh, _, tickets, layouts = grid(parts)
        d_all = devs[0].alloc(total * fsz)
        for at, (k, i) in enumerate(order(parts)):
            lib.mi355_memcpy_h2d(d_all + at * fsz, C.addressof(devs[k].host_desc) + i * fsz, fsz)
        for resident in resident_counts(tickets):
            for d in devs:
                D.poison(d)
            for launch in range(launches):
                if launch:
                    for d in devs:
                        lib.mi355_memcpy_d2d(d.dst, d.recon, d.F * d.fsz)
                rc = lib.mi355_h264_deblock_resident_dev(d_all, total, mw, mh, layouts, resident, None)
                assert rc == 0, (rc, resident)
            assert lib.mi355_sync(None) == 0
            for (s, _), pics, d in zip(parts, sets, devs):
                D.check(d, pics[2], "%s: %s, resident_waves %d of %d tickets" % (name, s, resident, tickets))
    finally:
        for d in devs:
            d.free()


def boundary_changes(fs, recon, dst, c=None):
    """adds to c how many band boundaries (the top edge of a macroblock row 4k > 0) of a picture set have a luma sample the oracle's
    filter changed in the three rows ABOVE the edge (what the band above hands down and the band below finishes), in the three rows
    BELOW it, and on both sides at once; the same for the chroma row either side"""
    c = {} if c is None else c
    for f in range(fs.F):
        for my in range(4, fs.mb_h, 4):
            y, yc = 16 * my, 8 * my
            above = (recon[0][f][y - 3:y] != dst[0][f][y - 3:y]).any()
            below = (recon[0][f][y:y + 3] != dst[0][f][y:y + 3]).any()
            cab = any((recon[p][f][yc - 1] != dst[p][f][yc - 1]).any() for p in (1, 2))
            cbe = any((recon[p][f][yc] != dst[p][f][yc]).any() for p in (1, 2))
            for k, v in (("boundaries", True), ("luma_above", above), ("luma_below", below), ("luma_both", above and below), ("chroma_above", cab),
                         ("chroma_below", cbe)):
                c[k] = c.get(k, 0) + int(bool(v))
    return c


PINS = {"MI355_DEBLOCK_WAVES": "1", "MI355_DEBLOCK_RESIDENT": "2"}


def pipelines_pinned(backend):
    """In a process started with PINS (the switches are read once per process): the pipelines object takes the one-wave tiled form and asks
    for two resident waves per launch.  Three shares of seven 3 x 9 pictures (3 + 2 + 2 pictures: 9, 6 and 6 tickets), two calls one
    behind the other, every picture of both surfaces against the oracle."""
    import frame_cases
    import providers
    lib = backend.lib
    for shares, pictures_ in ((3, 3), (3, 2), (1, 7)):
        assert rule(lib, pictures_, 3, 9, D.LAYOUT_TILED, 256, shares) == 2, "the switch pins the count"
    assert rule(lib, 1, 3, 2, D.LAYOUT_TILED, 256, 3) == 1, "never more waves than tickets"
    frame_cases.run_fast_workload_by_layout(backend, providers.oracle(), 7, 3, 9, 0x5920, pipelined=(3, 1, 2), refs="smooth", coef_b=4)


def run_pinned(backend_name):
    """pipelines_pinned() in a child process with PINS set"""
    import os
    import subprocess
    import sys
    env = dict(os.environ, **PINS)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), backend_name], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and "pinned ok" in r.stdout, r.stdout[-4000:]


if __name__ == "__main__":
    import os
    import sys
    assert all(os.environ.get(k) == v for k, v in PINS.items())
    import providers
    pipelines_pinned(getattr(providers, sys.argv[1])())
    print("pinned ok")
