"""GPU: NV12 / NV21 destinations of the device swscale path and the unscaled yuv420p -> NV12 / NV21 packer (include/mi355_sws.h).

Every entry of tests/sws_nv12.py on the contexts committed in tests/golden/sws_nv12_contexts.npz: Tier 1 (noise and the per-depth
checkerboard) and a guarded four-frame Tier-2 batch (destination planes on 16-byte, on 8-byte and on odd starts and strides) equal the
reference's own sws_scale() (oracle/_ref/libswsref.so), byte for byte, over the whole rounded-up extent of both planes.  The full-size
entries at 16 distinct pictures in one launch, every picture compared.  The binding (oracle/_ref/libswsref_gpu.so) in both forms.  A High 10
picture set decoded on the device goes straight into the scaler and comes out as NV12.  Nothing under the reference's sources is read here."""
import ctypes as C
import os

import numpy as np
import pytest

import h264_frames as HF
import sws_nv12 as N
import sws_planar as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ref():
    for p in (N.REF_LIB, N.REF_GPU_LIB):
        if not os.path.exists(p):
            pytest.fail(p + " missing: __graft_entry__.build() makes it where the reference exists")
    return N.Ref(P.bind(N.REF_LIB))


@pytest.fixture(scope="module")
def bound(mi355, ref):
    # the older describer declines every NV12 / NV21 destination: ask the library itself
    lib = N.Ref(P.bind(N.REF_GPU_LIB))
    c = lib.open("n420d8_down2") if P.exports(N.REF_GPU_LIB, N.DESCRIBER) else None
    new = c is not None and lib.describe(c) is not None
    if c:
        lib.free(c)
    if not new:
        pytest.skip(N.REF_GPU_LIB + " was linked before mi355_sws_describe_src existed: __graft_entry__.build() relinks it where the reference exists")
    return lib


@pytest.mark.parametrize("name", [n for n in N.SMALL if n not in N.REFUSED])
def test_nv12_batched_on_the_device(mi355, ref, name):
    assert N.check_batch(mi355.lib, ref, name, e=N.stored_entry(name)) is not None, name


def test_nv12_refused_on_the_device(mi355):
    """the real library refuses what the emulated one refuses, and nothing else of the table"""
    assert {n for n in N.NAMES if N.plan(mi355.lib, N.stored_entry(n)) is None} == N.REFUSED


@pytest.mark.parametrize("name", [n for n in N.SMALL if n not in N.REFUSED])
def test_nv12_tier1(mi355, ref, name):
    e = N.stored_entry(name)
    h = N.create(mi355.lib, e)
    assert h
    try:
        sizes = e.out_sizes()
        for planes in (N.picture(name, seed=4, pad=7), N.checkerboard(name, pad=2)):
            want = ref.scale(name, planes, sizes)
            got = N.scale_tier1(mi355.lib, h, e, planes, pad=8)             # (the second picture reuses the context's device buffers)
            assert not any(N.differing_rows(got, want, sizes)), name
            assert all((g[:, w:] == 0x5A).all() for g, (w, _) in zip(got, sizes))
    finally:
        mi355.lib.mi355_sws_destroy(C.c_void_p(h))


def test_yuv2nv12cx_on_the_device(mi355):
    N.check_nv12cx(mi355.lib)


@pytest.mark.parametrize("name", sorted(N.BIG))
def test_nv12_full_size_16_pictures(mi355, ref, name):
    """16 distinct pictures in one launch (each a rolled copy of one random picture with its low bits flipped); every picture against the
    reference"""
    e = N.stored_entry(name)
    base = N.picture(name, seed=9)

    def pic(f):
        return [np.ascontiguousarray(np.roll(pl, 3 * f + 1, axis=1) ^ pl.dtype.type(f)) for pl in base]

    h = N.create(mi355.lib, e)
    assert h
    try:
        p = N.plan_of(mi355.lib, h)
        batch = N.Batch(mi355.lib, e, (pic(f) for f in range(16)), 16, src_offs=(0,))
        try:
            out = batch.run(h)
            assert batch.untouched(out), (name, p)
            c = ref.open(name)
            try:
                for f in range(16):
                    want = ref.scale_ctx(c, pic(f), batch.sizes)
                    assert not any(N.differing_rows(batch.frame(out, f), want, batch.sizes)), (name, p, f)
            finally:
                ref.free(c)
        finally:
            batch.close()
    finally:
        mi355.lib.mi355_sws_destroy(C.c_void_p(h))


@pytest.mark.parametrize("lines", [False, True])
@pytest.mark.parametrize("name", N.BINDING)
def test_nv12_through_the_binding(mi355, ref, bound, name, lines, monkeypatch):
    if lines:
        monkeypatch.setenv("MI355_SWS_LINES", "1")
    else:
        monkeypatch.delenv("MI355_SWS_LINES", raising=False)
    e = N.stored_entry(name)
    planes = N.picture(name, seed=5, pad=3)
    sizes = e.out_sizes()
    want = ref.scale(name, planes, sizes)
    lib = bound.lib
    pics, calls = lib.ref_sws_pictures(), lib.ref_sws_tier1_calls()
    got = bound.scale(name, planes, sizes)
    if lines:
        assert (lib.ref_sws_tier1_calls() > calls) == (name not in N.PACKED) and lib.ref_sws_pictures() == pics, name
    else:
        assert lib.ref_sws_pictures() == pics + (1 if name in N.TAKEN else 0) and lib.ref_sws_tier1_calls() == calls, name
    assert not any(N.differing_rows(got, want, sizes)), name


def test_wide_decode_feeds_the_nv12_scaler_on_the_device(mi355, oracle, ref):
    """three High 10 4:2:0 pictures of 9 x 6 macroblocks decoded by mi355_h264_decode_frames_wide_dev go straight from their device planes
    through chain_420d10_nv12; the result is the reference's sws_scale() of the frame checker's pictures"""
    name = "chain_420d10_nv12"
    sw, sh, dw, dh = N.cfg(name)[:4]
    nframes, mb_w, mb_h = 3, sw // 16, sh // 16
    fs = HF.synth_frames(nframes=nframes, mb_w=mb_w, mb_h=mb_h, seed=31, mix="mixed", intra_frac=0.2, dct8_frac=0.3, refs="smooth", coef_b=8)
    checked = HF.run_oracle_hbd(oracle, fs, 10, idc=1)
    assert checked is not None, "oracle/_ref/libref.so missing: the frame checker above 8 bits needs it"
    _, dst_o = checked
    e = N.stored_entry(name)
    assert (e.depth, e.hsub, e.vsub, e.fmt) == (10, 1, 1, 16)
    sizes = e.out_sizes()
    want = [ref.scale(name, [np.ascontiguousarray(dst_o[p][f]) for p in range(3)], sizes, pad=0) for f in range(nframes)]

    lib = mi355.lib
    lib.mi355_malloc.restype = C.c_void_p
    d = HF.DeviceFrames(mi355, fs, bit_depth=10, idc=1)
    p_out = p_frames = h = None
    ysz, csz = sizes[0][0] * sizes[0][1], sizes[1][0] * sizes[1][1]
    try:
        d.decode_wide(bit_depth=10, idc=1)
        p_out = lib.mi355_malloc(C.c_size_t(nframes * (ysz + csz) + 64))
        frames = (P.PlanarFrame * nframes)()
        for f in range(nframes):
            fr = d.host_desc[f]
            for p in range(3):
                frames[f].src[p] = fr.dst[p]
                frames[f].src_stride[p] = fr.dst_stride[0] if p == 0 else fr.dst_stride[1]
            frames[f].dst[0], frames[f].dst_stride[0] = p_out + f * (ysz + csz), sizes[0][0]
            frames[f].dst[1], frames[f].dst_stride[1] = p_out + f * (ysz + csz) + ysz, sizes[1][0]
        p_frames = lib.mi355_malloc(C.c_size_t(C.sizeof(frames)))
        lib.mi355_memcpy_h2d(C.c_void_p(p_frames), C.addressof(frames), C.c_size_t(C.sizeof(frames)))
        h = N.create(lib, e)
        assert h
        lib.mi355_sws_scale_planar_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        assert lib.mi355_sws_scale_planar_frames_dev(C.c_void_p(h), C.c_void_p(p_frames), nframes, None) == 0
        lib.mi355_sync(None)
        got = np.empty((nframes, ysz + csz), np.uint8)
        lib.mi355_memcpy_d2h(C.c_void_p(got.ctypes.data), C.c_void_p(p_out), C.c_size_t(got.nbytes))
    finally:
        if h:
            lib.mi355_sws_destroy(C.c_void_p(h))
        for p in (p_out, p_frames):
            if p:
                lib.mi355_free(C.c_void_p(p))
        d.free()
    for f in range(nframes):
        assert np.array_equal(got[f, :ysz].reshape(sizes[0][1], sizes[0][0]), want[f][0]), "%s: luma of picture %d differs" % (name, f)
        assert np.array_equal(got[f, ysz:].reshape(sizes[1][1], sizes[1][0]), want[f][1]), "%s: chroma pairs of picture %d differ" % (name, f)
