"""CPU: packed 4:2:2 destinations (yuyv422 / uyvy422 / yvyu422) of the device swscale path through the emulated product library.

The table of tests/sws_yuy2dst.py must reach what its census lists (asserted from the plan, source, destination, range and depth queries).  Every taken
entry equals the reference's own sws_scale() of the same buffers through Tier 1 and through a guarded four-frame Tier-2 batch whose destination rows lie
on 16-byte multiples, on 4-byte multiples that are none of 16 and on an ODD address with an odd stride; the packers' batches equal the four wrappers
written out in numpy; a context has the plan of its rgb24-destination twin and is refused exactly where the twin is; the line entries equal the
reference's own yuv2packedX / 2 / 1 of a context of each order; the creators refuse what lies outside the list; the tenth describer reproduces every
committed entry from a live reference context and the nine others decline them; the binding runs whole pictures on the device and forwards the inner
loops under MI355_SWS_LINES=1.

FATE: fate-pixfmt-yuyv422 is yuv420p -> yuyv422 -> yuv444p.  Stage 1 through the device equals the reference's stage-1 picture committed with the source
module (tests/golden/sws_yuy2src_fate_mid.npz), and both stages on the device give the pin (tests/golden/sws_yuy2src_fate.json)."""
import ctypes as C
import os

import numpy as np
import pytest

import sws_planar as P
import sws_yuy2dst as Z
import sws_yuy2src as Y

HAVE_REF_LIB = os.path.exists(Z.REF_LIB) or P.S.HAVE_REFERENCE
needs_ref = pytest.mark.skipif(not HAVE_REF_LIB, reason="oracle/_ref/libswsref.so is built by __graft_entry__.build() where the reference exists")
needs_sources = pytest.mark.skipif(not P.S.HAVE_REFERENCE, reason="needs the reference's sources (a fresh oracle/_ref/libswsref.so)")


@pytest.fixture(scope="module")
def ref():
    if P.S.HAVE_REFERENCE:
        Z.make_fresh("_ref/libswsref.so")
    return Z.Ref(P.bind(Z.REF_LIB))


@pytest.fixture(scope="module")
def plans(emu):
    return {name: Z.plan(emu.lib, Z.stored_entry(name)) for name in Z.NAMES}


# ---- the census ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_form_of_the_packer(plans):
    plans = {n: plans[n] for n in Z.SPECIAL}
    assert all(plans.values()), plans
    cfgs = {n: Z.cfg(n) for n in Z.SPECIAL}
    for n, p in plans.items():
        assert p["kernel"] == "yuy2_pack" and (p["depth"], p["hsub"], p["layout"]) == (8, 1, 0), (n, p)
        assert (p["format"], p["planes"], p["chr_bytes"], p["chr_rows"], p["range"], p["dst_depth"]) == (Z.DSTS[Z.order_of(n)], 1, 0, 0, 0, 8), (n, p)
        assert p["vsub"] == int(cfgs[n][4] == "yuv420p"), (n, p)
    # both subsamplings to both orders; no packer to yvyu422
    assert {(cfgs[n][4], cfgs[n][6]) for n in plans} == {("yuv422p", "yuyv"), ("yuv422p", "uyvy"), ("yuv420p", "yuyv"), ("yuv420p", "uyvy")}
    # every remainder of the width by four, odd heights with 4:2:0 chroma, a third column tile and a second row tile of the kernel
    assert {cfgs[n][0] % 4 for n in plans} == {0, 1, 2, 3}
    assert any(cfgs[n][4] == "yuv420p" and cfgs[n][1] % 2 for n in plans)
    assert any(cfgs[n][0] > 2048 and cfgs[n][1] > 16 for n in plans)
    # the batch's destination rows hit the three alignment classes
    for n in plans:
        lay, _ = Z.layout(Z.stored_entry(n).out_sizes(), 4)
        assert {Z.store_class(o, st) for (o, st), in lay} == {16, 4, 1}, n


def test_table_reaches_every_form_of_the_scaler(plans):
    taken = {n: plans[n] for n in Z.SCALED if plans[n] is not None}
    for n, p in taken.items():
        assert (p["depth"], p["hsub"], p["vsub"], p["layout"]) == Z.src_record(n), (n, p)
        assert (p["format"], p["planes"], p["chr_bytes"], p["chr_rows"], p["dst_depth"]) == (Z.DSTS[Z.order_of(n)], 1, 0, 0, 8), (n, p)
        assert p["range"] == Z.expected_range(n), (n, p)
    kernels = {p["kernel"] for p in taken.values()}
    assert kernels == {"ident1_1", "ident1_x", "generic_a", "generic_b", "generic_c"}, kernels
    # all three orders through the tile kernel and through k_sws_ident1; k_sws_ident1 from planes and from pairs, only at equal size without a range
    for fam in ("generic", "ident1"):
        assert {p["format"] for p in taken.values() if p["kernel"].startswith(fam)} == {48, 49, 50}, fam
    ident = {n for n, p in taken.items() if p["kernel"].startswith("ident1")}
    assert {taken[n]["layout"] for n in ident} >= {0, 2, 16, 17} and all(Z.cfg(n)[:2] == Z.cfg(n)[2:4] and not taken[n]["range"] for n in ident), ident
    # a packed RGB source at equal size is a context here, and runs the tile kernel
    for n in ("g_rgb_uyvy_same", "g_bgra_yuyv_same"):
        assert taken[n]["kernel"].startswith("generic"), (n, taken[n])
    # every source class; the wide and the narrow store; the three forms of the vertical pass (_1: one luma tap; _2: bilinear; X)
    assert {p["layout"] for p in taken.values()} >= {0, 1, 2, 4, 9, 17, 18} and {p["depth"] for p in taken.values()} == {8, 9, 10}
    assert {(p["hsub"], p["vsub"]) for p in taken.values() if p["layout"] == 0} == {(1, 1), (1, 0), (0, 0)}
    generic = {n: p for n, p in taken.items() if p["kernel"].startswith("generic")}
    assert {p["narrow"] for p in generic.values()} == {0, 1}
    sizes = {(Z.stored_entry(n).ctx.desc.vLum.size, Z.stored_entry(n).ctx.desc.vChr.size) for n in generic}
    assert any(ls == 1 and cs <= 2 for ls, cs in sizes) and (2, 2) in sizes and any(ls > 2 for ls, cs in sizes) and any(ls > 8 for ls, cs in sizes), sizes
    # both ranges, each with an odd width (the phantom) and with the tile kernel at equal size
    assert {p["range"] for p in taken.values()} == {0, 1, 2}
    for r in (1, 2):
        assert any(p["range"] == r and Z.cfg(n)[2] % 2 for n, p in taken.items()), r
    assert taken["r_420_uyvyj_same"]["kernel"].startswith("generic")
    # odd destination widths in all three forms
    odd = {(Z.stored_entry(n).ctx.desc.vLum.size, Z.stored_entry(n).ctx.desc.vChr.size) for n in generic if Z.cfg(n)[2] % 2}
    assert any(ls == 1 for ls, _ in odd) and (2, 2) in odd and any(ls > 2 for ls, _ in odd), odd


def test_a_context_has_the_plan_and_the_refusals_of_its_rgb24_twin(emu, plans):
    """REFUSED is derived from the twin (the same descriptor and source to rgb24), and these destinations are refused exactly there; a taken row has
    its twin's plan — except that a context with a range never reads the source bytes directly, and a packed RGB source at equal size has no twin"""
    twin = Z.refused_by_the_twin(emu.lib)
    assert twin == Z.REFUSED, twin
    assert {n for n, p in plans.items() if p is None} == Z.REFUSED
    assert len(Z.REFUSED) * Z.REFUSED_CAP <= len(Z.NAMES), (len(Z.REFUSED), len(Z.NAMES))
    checked = 0
    for n in Z.SCALED:
        if n in Z.REFUSED:
            continue
        e = Z.stored_entry(n)
        t = Z.twin_plan(emu.lib, e)
        if t is None:
            assert e.layout in (4, 5, 8, 9, 10, 11) and Z.cfg(n)[:2] == Z.cfg(n)[2:4], n
            continue
        for k in Z.PLAN_KEYS:
            if k == "kernel" and e.range and t[k].startswith("ident1"):
                assert plans[n][k].startswith("generic"), (n, plans[n])
                continue
            assert plans[n][k] == t[k], (n, k, plans[n], t)
        checked += 1
    assert checked >= len(Z.SCALED) - len(Z.REFUSED) - 2


def test_the_equal_size_form_of_a_packed_422_source_reorders_the_bytes(emu):
    """a packed 4:2:2 source to a packed 4:2:2 destination at equal size (the reference's scaler with one tap each where the orders differ, rows
    g_uyvy_yuyv_same and g_yuyv_yvyu_same_w126; its plain copy where they are equal): the creator has the twin's plan for such a descriptor —
    k_sws_ident1_yuy2 — for every pair of orders, the equal ones too, and with one chroma tap it is a re-ordering of the bytes"""
    e = Y.stored_entry("p_yuyv_rgb_same")
    sw, sh = Y.cfg("p_yuyv_rgb_same")[:2]
    packed = Y.picture("p_yuyv_rgb_same", "noise", seed=9, padb=4)
    yuv = Y.deinterleave("p_yuyv_rgb_same", packed)
    for order, fmt in Z.DSTS.items():
        z = Z.Entry.of(e.edited(fmt=fmt))
        assert Z.plan(emu.lib, z)["kernel"] == "ident1_1" == Y.plan(emu.lib, e)["kernel"]
        h = Z.create(emu.lib, z)
        assert h
        try:
            got = Z.scale_tier1(emu.lib, h, z, packed, pad=8)
        finally:
            emu.lib.mi355_sws_destroy(C.c_void_p(h))
        lo, uo, vo = Z.PICKS[order]
        assert (got[0][:, lo:2 * sw:2] == yuv[0]).all() and (got[0][:, uo:2 * sw:4] == yuv[1]).all() and (got[0][:, vo:2 * sw:4] == yuv[2]).all(), order
        assert (got[0][:, 2 * sw:] == 0x5A).all(), order


# ---- the committed contexts -------------------------------------------------------------------------------------------------------
@needs_sources
def test_committed_contexts_match_the_reference(ref):
    for name in Z.SHAPES:
        assert Z.stored_entry(name).same(ref.entry(name)), name


@needs_sources
def test_described_scaler_contexts_have_the_banks_of_their_rgb24_twins(ref):
    """the reference's sizes and all four banks of a context to these destinations equal those of its rgb24-destination context (same range on both
    sides); a packed RGB source at equal size has no such twin"""
    import sws_nvsrc as V
    n = 0
    for name in Z.SCALED:
        e = ref.entry(name)
        if e.range:
            continue
        t = ref.twin_entry(name)
        if t is None:
            assert e.layout in (4, 5, 8, 9, 10, 11) and Z.cfg(name)[:2] == Z.cfg(name)[2:4], name
            continue
        assert (t.depth, t.hsub, t.vsub, t.layout, t.fmt) == (e.depth, e.hsub, e.vsub, e.layout, 0), name
        assert e.ctx.ints == t.ctx.ints and V.same_banks(e, t), name
        n += 1
    assert n >= 25


# ---- parity with the reference ------------------------------------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", Z.TAKEN)
def test_emulated_tier1_matches_reference(emu, ref, name):
    Z.check_tier1(emu.lib, ref, name, Z.tier1_pictures(name, seed=11), skew={0: 0, 1: 4, 2: 1}[len(name) % 3])


@needs_ref
@pytest.mark.parametrize("name", Z.TAKEN)
def test_emulated_batched(emu, ref, plans, name):
    p = Z.check_batch(emu.lib, ref, name, e=Z.stored_entry(name))
    assert p is not None and p == plans[name], name


@needs_ref
def test_the_phantom_luma_byte_of_an_odd_width_is_zero(emu, ref):
    """the last group's second luma byte of an odd dstW is 0 in the X, _2 and _1 forms, with and without a range — in the reference's output and in
    the device's (the equality is test_emulated_tier1_matches_reference's; this states the value)"""
    for name in ("g_420_yuyv_odd", "g_420_uyvy_w129_up_bilinear", "g_420_uyvy_same_w131", "r_j420_yuyv_odd", "r_420_yvyuj_odd_bilinear"):
        e = Z.stored_entry(name)
        dw = Z.cfg(name)[2]
        assert dw % 2
        lo = Z.PICKS[Z.order_of(name)][0]
        planes = Z.picture(name, "noise", seed=21, pad=1)
        want = ref.scale(name, planes, e.out_sizes())
        h = Z.create(emu.lib, e)
        assert h
        try:
            got = Z.scale_tier1(emu.lib, h, e, planes, pad=8)
        finally:
            emu.lib.mi355_sws_destroy(C.c_void_p(h))
        col = 2 * dw + lo                                                         # luma sample dstW of the row
        assert (want[0][:, col] == 0).all() and (got[0][:, col] == 0).all(), name


# ---- the pack model: no reference needed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", Z.SPECIAL)
def test_emulated_batched_equals_the_packers_written_out(emu, name):
    """byte picks in numpy over min(G, (srcW + 1) >> 1) groups; the model leaves the guard value behind them, and so does the device"""
    e = Z.stored_entry(name)
    h = Z.create(emu.lib, e)
    assert h
    try:
        pics = Z.batch_pictures(name)
        batch = Z.Batch(emu.lib, e, pics, len(pics))
        try:
            out = batch.run(h)
            assert batch.untouched_behind(out, e.written()), name
            for f in range(len(pics)):
                assert (batch.frame(out, f)[0] == Z.model_pack(name, pics[f])[0]).all(), (name, f)
        finally:
            batch.close()
    finally:
        emu.lib.mi355_sws_destroy(C.c_void_p(h))


def test_the_packer_writes_the_groups_the_header_names():
    assert [Z.pack_groups(w) for w in (128, 129, 130, 131, 66, 2, 1, 3)] == [64, 64, 65, 66, 33, 1, 0, 2]


# ---- the line entries -----------------------------------------------------------------------------------------------------------------
@needs_ref
def test_line_entries_match_the_reference_s_own_loops(emu, ref):
    assert Z.check_line_entries(emu.lib, ref) > 400


def test_line_entries_refuse_what_is_outside_the_list(emu):
    Z.check_line_entries_refuse(emu.lib)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def _message(capfd, fn):
    capfd.readouterr()
    r = fn()
    return r, capfd.readouterr().err


def test_creators_refuse_what_is_outside_the_list(emu, capfd):
    lib = emu.lib
    g = Z.stored_entry("g_420_yuyv_down2")
    s = Z.stored_entry("s_422_yuyv")
    s420 = Z.stored_entry("s_420_yuyv_w130")
    assert Z.plan(lib, g)["kernel"].startswith("generic") and Z.plan(lib, s)["kernel"] == "yuy2_pack" and Z.plan(lib, s420)["kernel"] == "yuy2_pack"
    # the format is the caller's word: all three orders, and both packer orders
    assert {Z.plan(lib, g.edited(fmt=f))["format"] for f in (48, 49, 50)} == {48, 49, 50} and Z.plan(lib, s.edited(fmt=49))["format"] == 49
    # 37 .. 47 and 51 and up stay refused, with the existing message
    for fmt in (37, 40, 47, 51, 52, 64, 1000):
        for base in (g, s):
            h, err = _message(capfd, lambda: Z.create(lib, base.edited(fmt=fmt)))
            assert not h and "destination format %d is not yuv420p / yuv422p / yuv444p / nv12 / nv21" % fmt in err, (fmt, err)
    # alpha 1
    h, err = _message(capfd, lambda: Z.create(lib, g, alpha=1))
    assert not h and "alpha (1) is carried from an rgba / bgra / argb / abgr source" in err, err
    h, err = _message(capfd, lambda: Z.create(lib, Z.stored_entry("g_bgra_yvyu_down2"), alpha=1))
    assert not h and "alpha (1) is carried" in err, err
    # a 9- or 10-bit depth with these formats
    for depth in (9, 10):
        h, err = _message(capfd, lambda: Z.create(lib, g.edited(dst_depth=depth)))
        assert not h and "a %d-bit destination is yuv420p / yuv422p / yuv444p (format 48)" % depth in err, err
    assert not Z.create(lib, g.edited(dst_depth=12)) and not Z.create(lib, g.edited(range_=3))
    # the range is accepted (a YUV destination), not with a packer
    assert Z.plan(lib, g.edited(range_=1))["range"] == 1 and Z.plan(lib, g.edited(range_=2))["range"] == 2
    h, err = _message(capfd, lambda: Z.create(lib, s.edited(range_=1)))
    assert not h and "no unscaled special converter converts the range" in err, err
    # the packers: to yvyu422, from 4:4:4, 10 bit, nv12, a packed source, at another size
    h, err = _message(capfd, lambda: Z.create(lib, s.edited(fmt=50)))
    assert not h and "the unscaled packers to a packed 4:2:2 destination are 8-bit yuv422p / yuv420p -> yuyv422 / uyvy422 at equal size" in err, err
    h, err = _message(capfd, lambda: Z.create(lib, s.edited(hsub=0, chrSrcW=s.ctx.ints["srcW"])))
    assert not h and "is outside this backend" in err, err
    h, err = _message(capfd, lambda: Z.create(lib, s.edited(depth=10)))
    assert not h and "is outside this backend" in err, err
    h, err = _message(capfd, lambda: Z.create(lib, s420.edited(layout=1)))
    assert not h and "the only unscaled special converter of an nv12 / nv21 source is the splitter" in err, err
    assert not Z.create(lib, s.edited(layout=4, hsub=1, vsub=0)) and not Z.create(lib, s.edited(layout=16)) and not Z.create(lib, s.edited(layout=9))
    h, err = _message(capfd, lambda: Z.create(lib, s.edited(dstW=32, chrDstW=16)))
    assert not h and "at equal size" in err, err
    assert not Z.create(lib, s.edited(dstH=24)) and not Z.create(lib, s.edited(chrDstW=31))
    # the scaler: a descriptor that is not the reference's for these destinations
    assert not Z.create(lib, g.edited(chrDstW=g.ctx.ints["chrDstW"] + 1))
    for layout in (3, 6, 7, 12, 15, 19, -1):
        assert not Z.create(lib, g.edited(layout=layout)), layout
    # the entry points across context kinds; a stride below the row
    lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale_planar_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mi355_sws_scale.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.mi355_sws_scale_planar.argtypes = [C.c_void_p] * 5
    buf = (C.c_uint8 * 1024)()
    for entry, name in ((g, "g_420_yuyv_down2"), (s, "s_422_yuyv")):
        planes = Z.picture(name, "noise", seed=3)
        src = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
        ss = (C.c_int * 3)(*[p.strides[0] for p in planes])
        out = np.zeros((48, 128), np.uint8)
        three = [np.zeros((48, 64), np.uint8), np.zeros((48, 32), np.uint8), np.zeros((48, 32), np.uint8)]
        dst, ds = (C.c_void_p * 3)(*[o.ctypes.data for o in three]), (C.c_int * 3)(64, 32, 32)
        h = Z.create(lib, entry)
        assert h
        try:
            assert lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(h), buf, 1, None) == -1
            assert lib.mi355_sws_scale_planar(C.c_void_p(h), src, ss, dst, ds) == -1
            assert lib.mi355_sws_scale(C.c_void_p(h), src, ss, out.ctypes.data, 128) == 48
            assert lib.mi355_sws_scale(C.c_void_p(h), src, ss, out.ctypes.data, 127) == -1                  # below the row's 4 * ((dstW + 1) >> 1) bytes
        finally:
            lib.mi355_sws_destroy(C.c_void_p(h))
    # an odd width's row holds the phantom's group too
    o = Z.stored_entry("g_420_yuyv_odd")
    planes = Z.picture("g_420_yuyv_odd", "noise", seed=3)
    src = (C.c_void_p * 3)(*[p.ctypes.data for p in planes])
    ss = (C.c_int * 3)(*[p.strides[0] for p in planes])
    out = np.zeros((61, 200), np.uint8)
    h = Z.create(lib, o)
    assert h
    try:
        assert lib.mi355_sws_scale(C.c_void_p(h), src, ss, out.ctypes.data, 2 * 97) == -1 and lib.mi355_sws_scale(C.c_void_p(h), src, ss, out.ctypes.data, 196) == 61
    finally:
        lib.mi355_sws_destroy(C.c_void_p(h))


# ---- FATE ------------------------------------------------------------------------------------------------------------------------------
def test_fate_stage1_matches_the_committed_picture(emu):
    assert (Z.fate_stage1(emu.lib) == Y.fate_mid()[0]).all()


def test_fate_chain_on_the_device_matches_the_pin(emu):
    assert Z.fate_chain_md5(emu.lib) == Y.fate_gold()["yuyv422"]


# ---- the describers on live contexts ---------------------------------------------------------------------------------------------------
@needs_sources
def test_describers_on_live_contexts(ref):
    lib = ref.lib
    flags = lib.ref_sws_flags_word(1, 1, 1)
    for name in Z.NAMES:
        c = ref.open(name)
        e = ref.describe(c)
        assert ref.declined_by_the_nine_describers(c), name                         # the nine existing describers keep declining these destinations
        ref.free(c)
        assert e is not None and (e.depth, e.hsub, e.vsub, e.layout) == Z.src_record(name) and e.fmt == Z.DSTS[Z.order_of(name)], name
        assert bool(e.ctx.desc.unscaled_special) == (name in Z.SPECIAL) and e.range == Z.expected_range(name), name
    declined = [
        (96, 40, b"yuv420p", 64, 40, b"yuyv422", (flags & ~0x7) | 0x1),         # SWS_FAST_BILINEAR, scaled
        (96, 40, b"yuv420p", 64, 40, b"uyvy422", flags | 0x2000),               # SWS_FULL_CHR_H_INT
        (96, 40, b"yuva420p", 64, 40, b"yuyv422", flags),                       # YUVA
        (96, 40, b"gray", 64, 40, b"yuyv422", flags),                           # another source
        (96, 40, b"rgb565le", 64, 40, b"uyvy422", flags),
        (64, 48, b"yuyv422", 64, 48, b"yuyv422", flags),                        # the reference's plain copy: no banks
        (64, 48, b"yvyu422", 64, 48, b"yvyu422", flags),
        (96, 40, b"yuv420p", 64, 40, b"rgb24", flags),                          # the other describers' destinations
        (96, 40, b"yuv420p", 64, 40, b"yuv422p", flags),
        (96, 40, b"yuv420p", 64, 40, b"bgra", flags),
        (96, 40, b"yuv420p", 64, 40, b"y210le", flags) if lib.av_get_pix_fmt(b"y210le") >= 0 else (96, 40, b"yuv420p", 64, 40, b"nv12", flags),
    ]
    for args in declined:
        c = ref.open_formats(*args)
        assert ref.describe(c) is None, args
        ref.free(c)
    # yuv420p at equal size WITHOUT SWS_POINT is the scaler's; yuv444p and another packed 4:2:2 order at equal size too (the reference has no
    # converter between the orders: banks of one tap each)
    for src in (b"yuv420p", b"yuv444p", b"uyvy422", b"yvyu422"):
        c = ref.open_formats(64, 48, src, 64, 48, b"yuyv422", flags)
        e = ref.describe(c)
        ref.free(c)
        assert e is not None and (e.fmt, e.ctx.desc.unscaled_special) == (48, 0), src


# ---- the binding (reference + product glue + emulated product) --------------------------------------------------------------------
@pytest.fixture(scope="module")
def hooked(emu):
    if not P.S.HAVE_REFERENCE:
        pytest.skip("the reference's sources are not present")
    return Z.Ref(P.bind(Z.make_fresh("_ref/libswsref_tier1.so")))


@pytest.mark.parametrize("name", Z.BINDING + Z.BINDING_UNBOUND)
def test_binding_whole_pictures(hooked, ref, name, monkeypatch):
    """whole pictures of the scaler's contexts go through mi355_swsfunc to the device (the picture counter moves); a context the creators refuse is
    left to the reference, and no selector this binding wraps runs for a packer's context: the counter stays and the picture is the reference's"""
    monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    planes = Z.picture(name, "ramp", seed=5, pad=3)
    sizes = Z.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    c = hooked.open(name)
    e = hooked.describe(c)
    hooked.free(c)
    assert e is not None and e.fmt == Z.DSTS[Z.order_of(name)] and bool(e.ctx.desc.unscaled_special) == (name in Z.SPECIAL), name
    before, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = hooked.scale(name, planes, sizes)
    assert lib.ref_sws_pictures() == before + (1 if name in Z.BINDING_TAKEN else 0), name
    assert lib.ref_sws_tier1_calls() == calls, name
    assert not any(Z.differing_rows(got, want, sizes)) and (got[0][:, sizes[0][0]:] == want[0][:, sizes[0][0]:]).all(), name


@pytest.mark.parametrize("name", Z.BINDING + Z.BINDING_UNBOUND)
def test_binding_inner_loops(hooked, ref, name, monkeypatch):
    """MI355_SWS_LINES=1: c->yuv2packedX / 2 / 1 of a context of the scaler go to mi355_sws_yuv2packed_X / _2 / _1 with the format (the call counter
    moves); a packer has no inner loops"""
    monkeypatch.setenv("MI355_SWS_LINES", "1")
    planes = Z.picture(name, "noise", seed=6, pad=3)
    sizes = Z.stored_entry(name).out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = hooked.lib
    before, pics = lib.ref_sws_tier1_calls(), lib.ref_sws_pictures()
    got = hooked.scale(name, planes, sizes)
    if name in Z.BINDING:
        assert lib.ref_sws_tier1_calls() > before, name
    else:
        assert lib.ref_sws_tier1_calls() == before, name
    assert lib.ref_sws_pictures() == pics
    assert not any(Z.differing_rows(got, want, sizes)), name
