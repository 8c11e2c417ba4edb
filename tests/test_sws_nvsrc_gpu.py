"""GPU: NV12 / NV21 sources of the device swscale path and the unscaled NV12 / NV21 -> yuv420p splitter (include/mi355_sws.h).

Every entry of tests/sws_nvsrc.py on the contexts committed in tests/golden/sws_nvsrc_contexts.npz: Tier 1 (noise and a colour-split picture)
and a guarded four-frame Tier-2 batch (pair planes on a 16-byte multiple, on a 4-byte multiple and on an odd address) equal the reference's
own sws_scale() of the NV picture (oracle/_ref/libswsref.so), byte for byte, over the whole rounded-up extent of every destination plane.
The binding (oracle/_ref/libswsref_gpu.so) in both forms.  A picture set decoded on the device goes through the packer and, as NV12, through
the scaler to rgb24 without leaving device memory.  Nothing under the reference's sources is read here."""
import ctypes as C
import os

import numpy as np
import pytest

import h264_frames as HF
import sws_nv12 as N
import sws_nvsrc as V
import sws_planar as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (V.REF_LIB, V.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return V.Ref(P.bind(V.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    if not P.exports(V.REF_GPU_LIB, V.DESCRIBER):
        pytest.skip(V.REF_GPU_LIB + " was linked before mi355_sws_describe_src existed: __graft_entry__.build() relinks it where the reference exists")
    return V.Ref(P.bind(V.REF_GPU_LIB))


TAKEN = [n for n in V.NAMES if n not in V.REFUSED]


@pytest.mark.parametrize("name", TAKEN)
def test_nvsrc_batched_on_the_device(mi355, ref, name):
    assert V.check_batch(mi355.lib, ref, name, e=V.stored_entry(name)) is not None, name


@pytest.mark.parametrize("name", TAKEN)
def test_nvsrc_tier1(mi355, ref, name):
    # (the second picture reuses the context's device buffers)
    V.check_tier1(mi355.lib, ref, name, [V.picture(name, seed=4, pad=7), V.colour_split(name, seed=5, pad=2)])


def test_nvsrc_refused_on_the_device(mi355):
    """the real library refuses what the emulated one refuses, and nothing else of the table"""
    assert {n for n in V.NAMES if V.plan(mi355.lib, V.stored_entry(n)) is None} == V.REFUSED


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", V.BINDING)
def test_nvsrc_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = V.stored_entry(name)
    planes = V.colour_split(name, seed=5, pad=3, ramp=True)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    if lines:
        assert (lib.ref_sws_tier1_calls() > calls) == (name not in V.SPLIT) and lib.ref_sws_pictures() == pics, name
    else:
        assert lib.ref_sws_pictures() == pics + (1 if name in V.TAKEN else 0) and lib.ref_sws_tier1_calls() == calls, name
    assert not any(V.differing_rows(got, want, sizes)), name


def test_decode_packer_and_nv12_scaler_chain_on_the_device(mi355, oracle, ref):
    """three 8-bit 4:2:0 pictures of 9 x 6 macroblocks decoded on the device go from their device planes through the unscaled packer
    (k_sws_nv12_pack) and, as NV12, through chain_v_rgb; one copy back.  The result is the reference's sws_scale(nv12 -> rgb24) of the
    reference-packed pictures of the frame checker."""
    name = "chain_v_rgb"
    sw, sh, dw, dh = V.cfg(name)[:4]
    nframes, mb_w, mb_h = 3, sw // 16, sh // 16
    fs = HF.synth_frames(nframes=nframes, mb_w=mb_w, mb_h=mb_h, seed=37, mix="mixed", intra_frac=0.2, dct8_frac=0.3, refs="smooth", coef_b=8)
    _, dst_o = HF.run_oracle(oracle, fs)
    e = V.stored_entry(name)
    assert (e.layout, e.fmt) == (1, 0)
    # the packer's context at the decoder's size, from the committed one
    k = N.stored_entry("k420d8_pack")
    pk = N.Entry(P.S.Context({**k.ctx.ints, "srcW": sw, "srcH": sh, "dstW": sw, "dstH": sh, "chrSrcW": sw // 2, "chrSrcH": sh // 2, "chrDstW": sw // 2},
                             dict(k.ctx.banks), k.ctx.luts), 8, 1, 1, k.dither, 16)
    nv_sizes = [(sw, sh), (sw, sh // 2)]
    packer = N.Ref(ref.lib)
    c = packer.open_formats(sw, sh, b"yuv420p", sw, sh, b"nv12", ref.lib.ref_sws_flags_word(1, 1, 1))
    try:
        packed = [packer.scale_ctx(c, [np.ascontiguousarray(dst_o[p][f]) for p in range(3)], nv_sizes, pad=0) for f in range(nframes)]
    finally:
        packer.free(c)
    want = [ref.scale(name, packed[f], e.out_sizes(), pad=0)[0] for f in range(nframes)]

    lib = mi355.lib
    lib.mi355_malloc.restype = C.c_void_p
    d = HF.DeviceFrames(mi355, fs)
    bufs, hp, hs = [], None, None
    ysz, csz, osz = sw * sh, sw * (sh // 2), dw * 3 * dh

    def alloc(n):
        p = lib.mi355_malloc(C.c_size_t(n))
        assert p
        bufs.append(p)
        return p

    try:
        d.decode()
        p_nv, p_out = alloc(nframes * (ysz + csz) + 64), alloc(nframes * osz + 64)
        pack_frames, rgb_frames = (P.PlanarFrame * nframes)(), (P.S.SwsFrame * nframes)()
        for f in range(nframes):
            fr = d.host_desc[f]
            for p in range(3):
                pack_frames[f].src[p] = fr.dst[p]
                pack_frames[f].src_stride[p] = fr.dst_stride[0] if p == 0 else fr.dst_stride[1]
            pack_frames[f].dst[0], pack_frames[f].dst_stride[0] = p_nv + f * (ysz + csz), sw
            pack_frames[f].dst[1], pack_frames[f].dst_stride[1] = p_nv + f * (ysz + csz) + ysz, sw
            rgb_frames[f].src[0], rgb_frames[f].src_stride[0] = p_nv + f * (ysz + csz), sw
            rgb_frames[f].src[1], rgb_frames[f].src_stride[1] = p_nv + f * (ysz + csz) + ysz, sw
            rgb_frames[f].dst, rgb_frames[f].dst_stride = p_out + f * osz, dw * 3
        d_pack, d_rgb = alloc(C.sizeof(pack_frames)), alloc(C.sizeof(rgb_frames))
        lib.mi355_memcpy_h2d(C.c_void_p(d_pack), C.addressof(pack_frames), C.c_size_t(C.sizeof(pack_frames)))
        lib.mi355_memcpy_h2d(C.c_void_p(d_rgb), C.addressof(rgb_frames), C.c_size_t(C.sizeof(rgb_frames)))
        hp, hs = N.create(lib, pk), V.create(lib, e)
        assert hp and hs
        assert N.plan_of(lib, hp)["kernel"] == "nv12_pack"
        for fn in (lib.mi355_sws_scale_planar_frames_dev, lib.mi355_sws_scale_frames_dev):
            fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        assert lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(hp), C.c_void_p(d_pack), nframes, None) == 0
        assert lib.mi355_sws_scale_frames_dev(C.c_void_p(hs), C.c_void_p(d_rgb), nframes, None) == 0
        lib.mi355_sync(None)
        got = np.empty((nframes, osz), np.uint8)
        lib.mi355_memcpy_d2h(C.c_void_p(got.ctypes.data), C.c_void_p(p_out), C.c_size_t(got.nbytes))
    finally:
        for h in (hp, hs):
            if h:
                lib.mi355_sws_destroy(C.c_void_p(h))
        for p in bufs:
            lib.mi355_free(C.c_void_p(p))
        d.free()
    for f in range(nframes):
        assert np.array_equal(got[f].reshape(dh, dw * 3), want[f]), "%s: picture %d differs" % (name, f)
