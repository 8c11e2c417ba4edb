"""GPU: decode -> swscale on the device for the deeper and wider sources (SURVEY.md §8f.2 beyond 8-bit 4:2:0).

A High 10 4:2:0 and a 10-bit 4:2:2 picture set decoded by the second H.264 kernel set (mi355_h264_decode_frames_wide_dev) go straight from
their device planes (16-bit little-endian samples, byte strides) into mi355_sws_scale_frames_dev on a context of mi355_sws_create_src.  The
result equals the reference's own sws_scale() (oracle/_ref/libswsref.so) of the frame checker's pictures (h264_frames.run_oracle_hbd)."""
import ctypes as C
import os

import numpy as np
import pytest

import h264_frames as HF
import sws_planar as P
import sws_sources as X
import sws_support as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name,idc", [("chain_420d10", 1), ("chain_422d10", 2)])
def test_wide_decode_feeds_the_scaler_on_the_device(mi355, oracle, name, idc):
    if not os.path.exists(X.REF_LIB):
        pytest.fail(X.REF_LIB + " missing: __graft_entry__.build() makes it where the reference exists")
    ref = X.Ref(P.bind(X.REF_LIB))
    sw, sh, dw, dh = X.cfg(name)[:4]
    nframes, mb_w, mb_h = 3, sw // 16, sh // 16
    fs = HF.synth_frames(nframes=nframes, mb_w=mb_w, mb_h=mb_h, seed=31, mix="mixed", intra_frac=0.2, dct8_frac=0.3, refs="smooth", coef_b=8)
    checked = HF.run_oracle_hbd(oracle, fs, 10, idc=idc)
    assert checked is not None, "oracle/_ref/libref.so missing: the frame checker above 8 bits needs it"
    _, dst_o = checked
    e = X.stored_entry(name)
    assert (e.depth, e.hsub, e.vsub, e.fmt) == (10, 1, 2 - idc, 0)
    want = [ref.scale(name, [np.ascontiguousarray(dst_o[p][f]) for p in range(3)], e.out_sizes(), pad=0)[0] for f in range(nframes)]

    lib = mi355.lib
    lib.mi355_malloc.restype = C.c_void_p
    d = HF.DeviceFrames(mi355, fs, bit_depth=10, idc=idc)
    p_rgb = p_frames = h = None
    try:
        d.decode_wide(bit_depth=10, idc=idc)
        rgb_stride = dw * 3
        p_rgb = lib.mi355_malloc(C.c_size_t(nframes * rgb_stride * dh + 64))
        frames = (S.SwsFrame * nframes)()
        for f in range(nframes):
            fr = d.host_desc[f]
            for p in range(3):
                frames[f].src[p] = fr.dst[p]
                frames[f].src_stride[p] = fr.dst_stride[0] if p == 0 else fr.dst_stride[1]
            frames[f].dst = p_rgb + f * rgb_stride * dh
            frames[f].dst_stride = rgb_stride
        p_frames = lib.mi355_malloc(C.c_size_t(C.sizeof(frames)))
        lib.mi355_memcpy_h2d(C.c_void_p(p_frames), C.addressof(frames), C.c_size_t(C.sizeof(frames)))
        h = X.create(lib, e)
        assert h
        lib.mi355_sws_scale_frames_dev.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        assert lib.mi355_sws_scale_frames_dev(C.c_void_p(h), C.c_void_p(p_frames), nframes, None) == 0
        lib.mi355_sync(None)
        got = np.empty((nframes, dh, rgb_stride), np.uint8)
        lib.mi355_memcpy_d2h(C.c_void_p(got.ctypes.data), C.c_void_p(p_rgb), C.c_size_t(got.nbytes))
    finally:
        if h:
            lib.mi355_sws_destroy(C.c_void_p(h))
        for p in (p_rgb, p_frames):
            if p:
                lib.mi355_free(C.c_void_p(p))
        d.free()
    for f in range(nframes):
        assert np.array_equal(got[f], want[f][:, :rgb_stride]), "%s: RGB picture %d differs" % (name, f)
