"""The H.264 loop filter's forms against the oracle: a table of pictures made for the filter's hard cases (slices with every
disable_deblocking_filter_idc and offset, chroma QP offsets, QP 0..51, flat blocks with steps around the thresholds, vectors on the bS
thresholds, B pictures with crossed lists), a census of what that content reaches (computed from the records and the oracle's pictures),
and a runner that sends the oracle's reconstruction through one named kernel form (mi355_h264_deblock_form_dev) and compares every sample
of the filtered picture."""
import ctypes as C

import numpy as np

import h264_frames as HF

_LF = dict(mix="mixed", qp_range=(0, 51), chroma_offsets=True)
# name -> synth_frames kwargs.  Odd widths; 1-row and 1-column pictures; 25+ macroblock rows (7+ bands: the 6-band form's second, partial
# launch and the one-wave form's hand-down between bands)
LF_CASES = {
    "lf_p_slices":  dict(_LF, nframes=2, mb_w=23, mb_h=9, seed=301, intra_frac=0.12, pcm_frac=0.15, dct8_frac=0.3, refs="steps", slices=5,
                         full_sample=True, near_mv=0.6, cbp0_frac=0.5),
    "lf_b_slices":  dict(_LF, nframes=2, mb_w=17, mb_h=7, seed=302, bframes=True, intra_frac=0.1, pcm_frac=0.15, dct8_frac=0.3, refs="steps",
                         slices=4, full_sample=True, near_mv=0.7, cbp0_frac=0.6),
    "lf_b_tall":    dict(_LF, nframes=1, mb_w=5, mb_h=27, seed=303, bframes=True, intra_frac=0.1, pcm_frac=0.1, dct8_frac=0.2, refs="steps",
                         slices=6, near_mv=0.6, cbp0_frac=0.5),
    "lf_p_tall":    dict(_LF, nframes=1, mb_w=3, mb_h=29, seed=304, intra_frac=0.15, pcm_frac=0.15, dct8_frac=0.3, refs="smooth", coef_b=6,
                         slices=4, full_sample=True, near_mv=0.5, cbp0_frac=0.4),
    "lf_one_row":   dict(_LF, nframes=2, mb_w=13, mb_h=1, seed=305, bframes=True, intra_frac=0.15, pcm_frac=0.15, refs="steps", slices=3,
                         full_sample=True, near_mv=0.6, cbp0_frac=0.5),
    "lf_one_col":   dict(_LF, nframes=2, mb_w=1, mb_h=11, seed=306, intra_frac=0.2, pcm_frac=0.15, dct8_frac=0.3, refs="steps", slices=3,
                         near_mv=0.6, cbp0_frac=0.5),
    "lf_intra_pcm": dict(_LF, nframes=1, mb_w=9, mb_h=6, seed=307, intra_frac=0.6, pcm_frac=0.3, dct8_frac=0.5, refs="smooth", coef_b=6,
                         slices=3, cbp0_frac=0.5),
    "lf_b_smooth":  dict(_LF, nframes=1, mb_w=11, mb_h=5, seed=308, bframes=True, intra_frac=0.05, dct8_frac=0.4, refs="smooth", coef_b=4,
                         slices=2, near_mv=0.8, cbp0_frac=0.7),
}

TILED = (1, 2)                # k_deblock_tiled, k_deblock_tiled2
LINEAR = (1, 2, 3, 4, 6)      # k_deblock, k_deblock_bands<n>
# (surfaces tiled, tiled_waves, linear_bands): every form a batch of one layout can go through
FORMS = [(True, w, 0) for w in TILED] + [(False, 0, k) for k in LINEAR] + [(True, 0, k) for k in LINEAR]
LAYOUT_LINEAR, LAYOUT_TILED = 1, 2

_cache = {}


def case(name):
    """(FrameSet, oracle recon, oracle dst) of a case of LF_CASES, made once per process"""
    if name not in _cache:
        import providers
        fs = HF.synth_frames(**LF_CASES[name])
        _cache[name] = (fs,) + tuple(HF.run_oracle(providers.oracle(), fs))
    return _cache[name]


def _bind(lib):
    lib.mi355_h264_deblock_form_dev.restype = C.c_int
    lib.mi355_h264_deblock_form_dev.argtypes = [C.c_void_p] + [C.c_int] * 6 + [C.c_void_p]
    lib.mi355_h264_deblock_layouts_dev.restype = C.c_int
    lib.mi355_h264_deblock_layouts_dev.argtypes = [C.c_void_p] + [C.c_int] * 4 + [C.c_void_p]
    lib.mi355_sync.restype = C.c_int


class PlanInfo(C.Structure):
    _fields_ = [("tiled_waves", C.c_int32), ("linear_bands", C.c_int32), ("skip_tiled", C.c_int32), ("linear_launches", C.c_int32)]


def plan(lib, nframes, mb_w, mb_h, layouts, cus):
    """mi355_h264_deblock_plan -> (tiled_waves, linear_bands, skip_tiled, linear_launches)"""
    p = PlanInfo()
    lib.mi355_h264_deblock_plan.restype = C.c_int
    lib.mi355_h264_deblock_plan.argtypes = [C.c_int] * 5 + [C.c_void_p]
    assert lib.mi355_h264_deblock_plan(nframes, mb_w, mb_h, layouts, cus, C.byref(p)) == 0
    return p.tiled_waves, p.linear_bands, p.skip_tiled, p.linear_launches


def upload(backend, fs, recon, tiled, replicate=None):
    """DeviceFrames of a picture set whose recon surfaces hold `recon` (the oracle's reconstruction): the loop filter alone is under test"""
    d = HF.DeviceFrames(backend, fs, tiled=tiled, replicate=replicate)
    d.put(d.recon, recon)
    return d


def poison(d):
    """dst of every picture = 0xA5: a sample the filter's copy misses shows"""
    junk = np.full(d.F * d.fsz, 0xA5, np.uint8)
    d.lib.mi355_memcpy_h2d(d.dst, junk.ctypes.data, junk.nbytes)


def check(d, dst_o, what, first=0, count=None):
    n = count or d.F
    got = d.fetch(d.dst, first, n)
    for i in range(n):
        g = (first + i) % d.fs.F
        for p in range(3):
            if not np.array_equal(got[p][i], dst_o[p][g]):
                bad = np.argwhere(got[p][i] != dst_o[p][g])
                y, x = bad[0]
                raise AssertionError("%s: picture %d plane %d differs at %d samples, first (y %d, x %d): %d, oracle %d"
                                     % (what, first + i, p, len(bad), y, x, got[p][i][y, x], dst_o[p][g][y, x]))


def run_form(backend, name, tiled, waves, bands):
    """one case through one pinned form, every sample of dst against the oracle"""
    fs, recon_o, dst_o = case(name)
    _bind(backend.lib)
    d = upload(backend, fs, recon_o, tiled)
    try:
        poison(d)
        rc = backend.lib.mi355_h264_deblock_form_dev(d.d_desc, d.F, fs.mb_w, fs.mb_h, LAYOUT_TILED if tiled else LAYOUT_LINEAR, waves, bands, None)
        assert rc == 0, rc
        assert backend.lib.mi355_sync(None) == 0
        check(d, dst_o, "%s, tiled %d, tiled_waves %d, linear_bands %d" % (name, tiled, waves, bands))
    finally:
        d.free()


def run_frameset_forms(backend, fs, dst_o, what, forms=FORMS, recon=None):
    """a picture set (oracle's or reference decoder's dst) through each (tiled, waves, bands) form; recon: the unfiltered pictures
    (default: the oracle's reconstruction of fs)"""
    lib = backend.lib
    _bind(lib)
    if recon is None:
        import providers
        recon, _ = HF.run_oracle(providers.oracle(), fs, deblock=False)
    for tiled in (False, True):
        sel = [f for f in forms if f[0] == tiled]
        if not sel:
            continue
        d = upload(backend, fs, recon, tiled)
        try:
            for _, waves, bands in sel:
                poison(d)
                rc = lib.mi355_h264_deblock_form_dev(d.d_desc, d.F, fs.mb_w, fs.mb_h, LAYOUT_TILED if tiled else LAYOUT_LINEAR, waves, bands, None)
                assert rc == 0, rc
                assert lib.mi355_sync(None) == 0
                check(d, dst_o, "%s, tiled %d, tiled_waves %d, linear_bands %d" % (what, tiled, waves, bands))
        finally:
            d.free()


def run_mixed(backend, names, tiled_names, waves, bands):
    """pictures of several cases in ONE call, some on tiled surfaces, some linear, of different sizes (largest width / height given):
    the tiled form `waves` takes the tiled ones (short pictures' bands leave), the linear kernels skip them"""
    lib = backend.lib
    _bind(lib)
    sets = [case(n) for n in names]
    devs = [upload(backend, s[0], s[1], n in tiled_names) for n, s in zip(names, sets)]
    try:
        fsz = C.sizeof(HF.Frame)
        total = sum(d.F for d in devs)
        d_all = devs[0].alloc(total * fsz)
        off = 0
        for d in devs:
            poison(d)
            lib.mi355_memcpy_h2d(d_all + off, C.addressof(d.host_desc), d.F * fsz)
            off += d.F * fsz
        mw, mh = max(s[0].mb_w for s in sets), max(s[0].mb_h for s in sets)
        rc = lib.mi355_h264_deblock_form_dev(d_all, total, mw, mh, LAYOUT_LINEAR | LAYOUT_TILED, waves, bands, None)
        assert rc == 0, rc
        assert lib.mi355_sync(None) == 0
        for n, s, d in zip(names, sets, devs):
            check(d, s[2], "%s in a mixed batch (tiled %d), tiled_waves %d, linear_bands %d" % (n, n in tiled_names, waves, bands))
    finally:
        for d in devs:
            d.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# census: what the content reaches, restated from the records (the oracle's filter_mb, oracle/oracle_h264frame.c) and read off the
# oracle's (recon, dst)
# ---------------------------------------------------------------------------------------------------------------------------------
def _bi(x4, y4):
    return (x4 & 1) + 2 * (y4 & 1) + 4 * (x4 >> 1) + 8 * (y4 >> 1)


def census(fs, recon, dst, c=None):
    """adds the counts of one picture set to the dict c (returned)"""
    c = {} if c is None else c

    def add(k, n=1):
        c[k] = c.get(k, 0) + n
    mw, mh = fs.mb_w, fs.mb_h
    two = fs.use_l1
    for f in range(fs.F):
        mb, sl = fs.mb[f], fs.slices[f]
        if two and sl[0]["list_count"] == 2:
            add("b_picture")
        intra = (mb["mb_type"] & 7) != 0
        pcm = (mb["mb_type"] & HF.PCM) != 0
        nodb = (mb["flags"] & HF.F_NODB) != 0

        def ref_id(m, l, x4, y4):
            if intra[m]:
                return -1
            r = int(mb[m]["ref_idx"][l][(x4 >> 1) + 2 * (y4 >> 1)])
            return -1 if r < 0 else int(sl[mb[m]["slice_id"]]["ref_slot"][l][r])

        def mv(m, l, x4, y4):
            if (l == 1 and not two) or ref_id(m, l, x4, y4) < 0:
                return (0, 0)
            v = fs.mv[l, f, m, x4 + 4 * y4]
            return int(v[0]), int(v[1])

        def far(a, b):
            return abs(a[0] - b[0]) >= 4 or abs(a[1] - b[1]) >= 4

        def check_mv(p, px, py, q, qx, qy, lc):
            r0p, r0q = ref_id(p, 0, px, py), ref_id(q, 0, qx, qy)
            if r0p == r0q and r0p >= 0:
                d = [abs(a - b) for a, b in zip(mv(p, 0, px, py), mv(q, 0, qx, qy))]
                for k, ax in enumerate("xy"):
                    if d[k] in (3, 4):
                        add("mvd%d_%s" % (d[k], ax))
            v = r0p != r0q or (r0p != -1 and far(mv(p, 0, px, py), mv(q, 0, qx, qy)))
            if lc == 2:
                r1p, r1q = ref_id(p, 1, px, py), ref_id(q, 1, qx, qy)
                if not v:
                    v = r1p != r1q or far(mv(p, 1, px, py), mv(q, 1, qx, qy))
                if v:
                    if r0p != r1q or r1p != r0q:
                        return 1
                    add("crossed_pair")
                    return int(far(mv(p, 0, px, py), mv(q, 1, qx, qy)) or far(mv(p, 1, px, py), mv(q, 0, qx, qy)))
            return int(v)

        for m in range(mw * mh):
            mx, my = m % mw, m // mw
            rec = mb[m]
            if nodb[m]:
                nbs = [n for n, ok in ((m - 1, mx > 0), (m + 1, mx + 1 < mw), (m - mw, my > 0), (m + mw, my + 1 < mh)) if ok]
                if any(not nodb[n] for n in nbs):
                    add("nodb_next_to_filtered")
                continue
            add("filtered_mb")
            if rec["qpc"][0] != rec["qpc"][1]:
                add("qpc_differ")
            if rec["mb_type"] & HF.DCT8:
                add("dct8")
            fl = int(rec["flags"])
            if fl & 0x80:
                if mx > 0 and not fl & HF.F_LEFT:
                    add("own_slice_suppressed")
                if my > 0 and not fl & HF.F_TOP:
                    add("own_slice_suppressed")
            a_off, b_off = int(rec["alpha"]), int(rec["beta"])
            lc = int(sl[rec["slice_id"]]["list_count"])
            cq = sl[rec["slice_id"]]["chroma_qp_table"]
            for d in range(2):
                for e in range(4):
                    if e == 0:
                        if not fl & (HF.F_TOP if d else HF.F_LEFT):
                            continue
                        n = m - mw if d else m - 1
                        if intra[m] or intra[n]:
                            bs = [4] * 4
                        else:
                            bs = []
                            for i in range(4):
                                x4, y4, nx, ny = (i, 0, i, 3) if d else (0, i, 3, i)
                                if ((int(rec["nnz_mask"]) >> _bi(x4, y4)) | (int(mb[n]["nnz_mask"]) >> _bi(nx, ny))) & 1:
                                    bs.append(2)
                                else:
                                    bs.append(check_mv(m, x4, y4, n, nx, ny, lc))
                        if not any(bs):
                            continue
                        if pcm[m] != pcm[n] and (not intra[m] or not intra[n]):
                            add("pcm_inter_edge")
                        if rec["slice_id"] != mb[n]["slice_id"]:
                            add("cross_slice_edge")
                        qp = (int(rec["qp"]) + int(mb[n]["qp"]) + 1) >> 1
                        qc = [(int(cq[p][rec["qp"]]) + int(cq[p][mb[n]["qp"]]) + 1) >> 1 for p in range(2)]
                        kind = "mb"
                    else:
                        if rec["mb_type"] & HF.DCT8 and e & 1:
                            continue
                        if intra[m]:
                            bs = [3] * 4
                        else:
                            bs = []
                            for i in range(4):
                                x4, y4, nx, ny = (i, e, i, e - 1) if d else (e, i, e - 1, i)
                                if ((int(rec["nnz_mask"]) >> _bi(x4, y4)) | (int(rec["nnz_mask"]) >> _bi(nx, ny))) & 1:
                                    bs.append(2)
                                else:
                                    bs.append(check_mv(m, x4, y4, m, nx, ny, lc))
                            if not any(bs):
                                continue
                        qp, qc = int(rec["qp"]), [int(cq[p][rec["qp"]]) for p in range(2)]
                        kind = "in"
                    for b in set(bs):
                        add("bs%d_%s_%d" % (b, kind, d))
                    if qp < 16:
                        add("luma_qp_below_16")          # alpha 0 without an offset
                    if qp > 45:
                        add("luma_qp_above_45")
                    if intra[m] and kind == "mb":
                        assert set(bs) == {4}
                    if intra[m] and kind == "in":
                        assert set(bs) == {3}
                    for q in [qp] + (qc if e in (0, 2) else []):
                        for o in (a_off, b_off):
                            if q + o < 0:
                                add("index_below_0")
                            if q + o > 51:
                                add("index_above_51")
                        ia = min(max(q + a_off, 0), 51)
                        if HF.ALPHA[ia] == 0:
                            add("alpha0_edge")
                        if ia == 51:
                            add("index51_edge")
                    if kind != "mb":
                        continue
                    # what the oracle did to p0 / q0 of each segment (MB edges, bS > 0, alpha > 0)
                    for p in range(3):
                        q = qp if p == 0 else qc[p - 1]
                        if HF.ALPHA[min(max(q + a_off, 0), 51)] == 0 or HF.BETA[min(max(q + b_off, 0), 51)] == 0:
                            continue
                        s = 16 if p == 0 else 8
                        lines = 4 if p == 0 else 2
                        for i in range(4):
                            if not bs[i]:
                                continue
                            if d == 0:
                                ys, x = slice(s * my + lines * i, s * my + lines * (i + 1)), s * mx
                                pq = np.r_[recon[p][f][ys, x - 1], recon[p][f][ys, x]], np.r_[dst[p][f][ys, x - 1], dst[p][f][ys, x]]
                            else:
                                xs, y = slice(s * mx + lines * i, s * mx + lines * (i + 1)), s * my
                                pq = np.r_[recon[p][f][y - 1, xs], recon[p][f][y, xs]], np.r_[dst[p][f][y - 1, xs], dst[p][f][y, xs]]
                            cls = "chroma" if p else ("luma4" if bs[i] == 4 else "luma123")
                            add("seg_%s" % cls)
                            add("seg_%s_%s" % (cls, "changed" if (pq[0] != pq[1]).any() else "kept"))
    return c
