"""GPU: every form of the loop filter (mi355_h264_deblock_form_dev) on the cases made for it, on the CASES pictures with B pictures or
offsets and on the reference decoder's exported records; the unpinned throughput form; the second kernel set on the same cases."""
import os

import numpy as np
import pytest

import deblock_cases as D
import frame_cases
import h264_frames as HF
import stream_fixture as SF
import synth_streams as SY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORM_IDS = ["%s-w%d-b%d" % ("tiled" if f[0] else "linear", f[1], f[2]) for f in D.FORMS]
EXISTING = [n for n, kw in frame_cases.CASES.items() if kw.get("bframes") or kw.get("offsets")]


@pytest.mark.gpu
@pytest.mark.parametrize("form", D.FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", list(D.LF_CASES))
def test_every_form_gpu(mi355, name, form):
    D.run_form(mi355, name, *form)


@pytest.mark.gpu
@pytest.mark.parametrize("name", EXISTING)
def test_every_form_on_existing_cases_gpu(mi355, oracle, name):
    fs = HF.synth_frames(**frame_cases.CASES[name])
    _, dst = HF.run_oracle(oracle, fs)
    D.run_frameset_forms(mi355, fs, dst, name)


@pytest.mark.gpu
@pytest.mark.parametrize("bands", D.LINEAR)
@pytest.mark.parametrize("waves", D.TILED)
def test_mixed_layout_batch_gpu(mi355, waves, bands):
    """linear and tiled pictures of different sizes in one call: the tiled form takes the tiled ones, the linear kernels skip them"""
    names = ("lf_p_slices", "lf_b_tall", "lf_one_row", "lf_one_col", "lf_b_slices", "lf_intra_pcm", "lf_p_tall", "lf_b_smooth")
    D.run_mixed(mi355, names, {"lf_b_tall", "lf_one_row", "lf_p_slices", "lf_b_smooth"}, waves, bands)


def _reference_streams():
    return [("realshort", os.path.join(ROOT, "tests", "golden", "h264_stream_realshort.npz"))] + [(n, SY.npz(n)) for n in SY.EXPORTED]


@pytest.mark.gpu
@pytest.mark.parametrize("name,path", _reference_streams(), ids=[n for n, _ in _reference_streams()])
def test_reference_records_through_every_form_gpu(mi355, name, path):
    """every picture of realshort and of the exported generated streams: tiled surfaces under both tiled forms, linear and tiled surfaces
    under every linear form, each equal to the reference decoder's own picture"""
    pics = SF.load_npz(path)
    fs = SF.frameset_all(pics)
    dst = [np.stack([pc[k] for pc in pics]) for k in ("y", "cb", "cr")]
    D.run_frameset_forms(mi355, fs, dst, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(D.LF_CASES))
def test_unpinned_throughput_form_gpu(mi355, name):
    """the new cases replicated to 2048 band-pictures or more through the unpinned mi355_h264_deblock_layouts_dev on tiled surfaces: the plan
    query says the one-wave form (k_deblock_tiled, what bench.py times) runs, and every picture equals the oracle's"""
    fs, recon, dst = D.case(name)
    nbands = (fs.mb_h + 3) // 4
    F = -(-2048 // nbands)
    F += (-F) % fs.F
    assert D.plan(mi355.lib, F, fs.mb_w, fs.mb_h, D.LAYOUT_TILED, 0)[0] == 1
    D._bind(mi355.lib)
    d = D.upload(mi355, fs, recon, True, replicate=F)
    try:
        D.poison(d)
        assert mi355.lib.mi355_h264_deblock_layouts_dev(d.d_desc, F, fs.mb_w, fs.mb_h, D.LAYOUT_TILED, None) == 0
        assert mi355.lib.mi355_sync(None) == 0
        for first in range(0, F, 256):
            D.check(d, dst, "%s replicated to %d pictures" % (name, F), first, min(256, F - first))
    finally:
        d.free()


def _wide_case(mi355, name):
    _, recon_o, dst_o = D.case(name)
    fs = HF.synth_frames(**D.LF_CASES[name])
    pcm = (fs.mb["mb_type"] & 4) != 0
    fs.coef[pcm] = fs.coef[pcm].view(np.uint8)[:, :384].astype(np.int16)     # the second kernel set's I_PCM convention
    d = HF.DeviceFrames(mi355, fs)
    try:
        d.decode_wide()
        recon_g, dst_g = d.fetch(d.recon), d.fetch(d.dst)
    finally:
        d.free()
    for p in range(3):
        assert np.array_equal(recon_o[p], recon_g[p]), "%s: reconstruction differs in plane %d" % (name, p)
        assert np.array_equal(dst_o[p], dst_g[p]), "%s: deblocked picture differs in plane %d" % (name, p)


@pytest.mark.gpu
@pytest.mark.parametrize("unit", ("1", "2", "3", "4", ""))
@pytest.mark.parametrize("name", list(D.LF_CASES))
def test_second_kernel_set_on_loop_filter_cases_gpu(mi355, monkeypatch, name, unit):
    """mi355_h264_decode_frames_wide_dev (8-bit 4:2:0 instance) with 1 to 4 macroblocks per group (MI355_WIDE_UNIT, read per call; "": the
    launcher's choice) against the oracle"""
    if unit:
        monkeypatch.setenv("MI355_WIDE_UNIT", unit)
    else:
        monkeypatch.delenv("MI355_WIDE_UNIT", raising=False)
    _wide_case(mi355, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(D.LF_CASES))
def test_second_kernel_set_on_loop_filter_cases_at_10_bits_gpu(mi355, oracle, name):
    fs = HF.synth_frames(**D.LF_CASES[name])
    assert frame_cases.run_case_hbd(mi355, oracle, name, 10, fs=fs), "oracle/_ref/libref.so missing"
