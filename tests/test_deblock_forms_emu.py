"""CPU: the loop filter's kernel forms.  The plan rule (mi355_h264_deblock_plan) for a 256-CU device against the rule the launcher has
always followed, and every form (mi355_h264_deblock_form_dev) under the SIMT emulator against the oracle and the reference decoder."""
import ctypes as C
import os

import pytest

import deblock_cases as D
import frame_cases
import h264_frames as HF
import stream_fixture as SF
import synth_streams as SY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEBLOCK_WAVES_PER_CU, DEBLOCK_LAG = 8, 20       # h264_deblock.hip with chunks of four macroblocks


def rule(nframes, mb_w, mb_h, layouts, cus):
    """the form choice of mi355_h264_deblock_layouts_dev as it stood before the plan query (no developer switch set)"""
    nbands, nsteps = (mb_h + 3) // 4, mb_w + 6
    waves = 0
    if layouts & D.LAYOUT_TILED:
        waves = 2 if nframes * nbands < 2 * 4 * cus else 1
        if not layouts & D.LAYOUT_LINEAR:
            return waves, 0, 0, 0
    best, best_cost = 1, None
    for kw in (1, 2, 3, 4, 6):
        resident = cus * (DEBLOCK_WAVES_PER_CU // kw)
        cost = ((nframes + resident - 1) // resident) * ((nbands + kw - 1) // kw) * (nsteps + DEBLOCK_LAG * (kw - 1)) * (1.25 if kw > 1 else 1.0)
        if best_cost is None or cost < best_cost:
            best, best_cost = kw, cost
    return waves, best, int(waves != 0), (nbands + best - 1) // best


SHAPES = [(683, 120, 68, 2), (2048, 120, 68, 2), (3, 120, 68, 2), (683, 120, 68, 3), (2048, 120, 68, 1), (3, 120, 68, 1), (1, 120, 68, 1),
          (64, 120, 68, 1), (1, 240, 135, 1), (2, 22, 18, 1), (1, 8, 5, 1), (1, 8, 5, 2), (2, 23, 9, 3), (1, 5, 27, 1), (4, 17, 7, 1),
          (8, 40, 22, 1), (1, 37, 9, 1), (300, 20, 15, 1), (5000, 20, 15, 1), (1, 1, 1, 3), (2, 13, 1, 1), (2, 1, 11, 2), (511, 3, 8, 2),
          (512, 3, 8, 2), (1, 1, 29, 1), (16, 120, 68, 1), (1, 60, 34, 1), (12, 1, 30, 1), (1, 40, 30, 1), (1, 120, 16, 3)]


@pytest.fixture(scope="module")
def product():
    """the product library, loaded without a device: the plan query with an explicit CU count needs none"""
    path = os.path.join(ROOT, "libav_amd", "libmi355dsp.so")
    if not os.path.exists(path):
        import sys
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return C.CDLL(path)


def test_plan_is_the_launchers_rule(product):
    assert not os.environ.get("MI355_DEBLOCK_FORM") and not os.environ.get("MI355_DEBLOCK_WAVES")
    seen = set()
    for n, w, h, layouts in SHAPES:
        got = D.plan(product, n, w, h, layouts, 256)
        assert got == rule(n, w, h, layouts, 256), (n, w, h, layouts, got)
        seen.add(("tiled", got[0]))
        seen.add(("linear", got[1]))
    # the bench's batches: the one-wave tiled form at 683 and 2048 1080p pictures, the two-wave form at 3
    assert D.plan(product, 683, 120, 68, D.LAYOUT_TILED, 256)[0] == 1 and D.plan(product, 2048, 120, 68, D.LAYOUT_TILED, 256)[0] == 1
    assert D.plan(product, 3, 120, 68, D.LAYOUT_TILED, 256)[0] == 2
    assert seen >= {("tiled", 1), ("tiled", 2)} | {("linear", k) for k in D.LINEAR}, seen
    # one linear 1080p picture: six bands a workgroup, 17 bands in three launches, the last one partial
    assert D.plan(product, 1, 120, 68, D.LAYOUT_LINEAR, 256) == (0, 6, 0, 3)
    assert D.plan(product, 1, 120, 68, D.LAYOUT_LINEAR | D.LAYOUT_TILED, 256) == (2, 6, 1, 3)


def test_plan_rejects_bad_arguments(product):
    p = D.PlanInfo()
    fn = product.mi355_h264_deblock_plan
    fn.restype = C.c_int
    fn.argtypes = [C.c_int] * 5 + [C.c_void_p]
    for args in ((0, 8, 5, 1, 256), (1, 0, 5, 1, 256), (1, 8, 0, 1, 256), (1, 8, 5, 0, 256), (1, 8, 5, 1, -1)):
        assert fn(*args, C.byref(p)) == -1, args
    assert fn(1, 8, 5, 1, 256, None) == -1


def test_plan_on_the_emulated_device(emu):
    """cus = 0: the device's own CU count (the emulator reports 4)"""
    for n, w, h, layouts in SHAPES:
        assert D.plan(emu.lib, n, w, h, layouts, 0) == rule(n, w, h, layouts, 4)


def test_form_entry_rejects_unknown_forms(emu):
    fs, recon, _ = D.case("lf_one_row")
    D._bind(emu.lib)
    d = D.upload(emu, fs, recon, True)
    try:
        fn = emu.lib.mi355_h264_deblock_form_dev
        for layouts, waves, bands in ((2, 3, 0), (2, -1, 0), (2, 0, 5), (2, 1, 7), (2, 0, 0), (1, 0, 0), (1, 1, 0), (3, 1, 0), (0, 1, 1)):
            assert fn(d.d_desc, d.F, fs.mb_w, fs.mb_h, layouts, waves, bands, None) == -1, (layouts, waves, bands)
    finally:
        d.free()


@pytest.mark.parametrize("form", D.FORMS, ids=lambda f: "%s-w%d-b%d" % ("tiled" if f[0] else "linear", f[1], f[2]))
@pytest.mark.parametrize("name", list(D.LF_CASES))
def test_every_form_emulated(emu, name, form):
    D.run_form(emu, name, *form)


EXISTING = [n for n, kw in frame_cases.CASES.items() if kw.get("bframes") or kw.get("offsets")]


@pytest.mark.parametrize("name", EXISTING)
def test_every_form_on_existing_cases_emulated(emu, oracle, name):
    """the CASES pictures with B pictures or alpha / beta offsets through every form (one case per form in turn on the CPU: the full
    matrix runs on the GPU)"""
    i = EXISTING.index(name)
    forms = [D.FORMS[(i + k * len(EXISTING)) % len(D.FORMS)] for k in range((len(D.FORMS) + len(EXISTING) - 1) // len(EXISTING))]
    fs = HF.synth_frames(**frame_cases.CASES[name])
    _, dst = HF.run_oracle(oracle, fs)
    D.run_frameset_forms(emu, fs, dst, name, forms)


@pytest.mark.parametrize("waves", D.TILED)
def test_mixed_layout_batch_emulated(emu, waves):
    names = ("lf_p_slices", "lf_b_tall", "lf_one_row", "lf_one_col", "lf_b_slices", "lf_intra_pcm")
    for bands in (D.LINEAR if waves == 1 else D.LINEAR[::-1])[:3]:
        D.run_mixed(emu, names, {"lf_b_tall", "lf_one_row", "lf_p_slices"}, waves, bands)


def _reference_streams():
    return [("realshort", os.path.join(ROOT, "tests", "golden", "h264_stream_realshort.npz"))] + [(n, SY.npz(n)) for n in SY.EXPORTED]


@pytest.mark.parametrize("name,path", _reference_streams(), ids=lambda v: v if "/" not in str(v) else "")
def test_reference_records_through_every_form_emulated(emu, oracle, name, path):
    """the reference decoder's exported records and its own pictures: the oracle's reconstruction through tiled surfaces under both tiled
    forms and through linear and tiled surfaces under every linear form, each picture equal to the reference decoder's"""
    pics = SF.load_npz(path)
    fs = SF.frameset_all(pics, 0, min(len(pics), 12))
    dst = [np_stack(pics, fs.F, k) for k in ("y", "cb", "cr")]
    D.run_frameset_forms(emu, fs, dst, name)


def np_stack(pics, n, key):
    import numpy as np
    return np.stack([pics[i][key] for i in range(n)])
