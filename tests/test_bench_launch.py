"""bench.py's launch path on CPU: `--gpus N` without a launcher starts N ranks itself (the flag was parsed and
never read), and a launcher's WORLD_SIZE that disagrees with the flag is an error, not a silent N=1 run.
`--dry --backend gloo` = the control plane only (stream table broadcast, barriers, counter reductions), no GPU.
A plain run and --dump-outputs: on the SIMT-emulated build of the library at a tiny size."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env():
    e = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    return e


def test_gpus_2_spawns_two_ranks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo", "--dry", "--steps", "3", "--frames", "8"],
                       capture_output=True, text=True, env=_env(), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["rccl_world_size"] == 2 and out["steps_per_rank"] == [3, 3] and out["dry"] is True
    assert abs(out["value"] * out["ms_per_step"] * 1e-3 * 3 - 2 * 8 * 8160 * 3) < 1e-3 * 2 * 8 * 8160 * 3      # whole-job units / max time


def test_gpus_1_dry_is_one_rank():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry", "--steps", "2", "--frames", "4"],
                       capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["n_gpus"] == 1 and out["steps_per_rank"] == [2]


def test_world_size_must_match_the_flag():
    e = _env()
    e.update(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--dry"], capture_output=True, text=True, env=e, timeout=120)
    assert r.returncode != 0 and "must agree" in r.stderr


def _bench_on_emulator(args):
    """bench.py's N=1 path on the SIMT-emulated build of the library (libav_amd.load() pointed at it), a tiny batch"""
    lib = os.path.join(ROOT, "tests", "_emu", "libmi355dsp_emu.so")
    code = "import sys, libav_amd; libav_amd.LIB_PATH = %r; sys.argv = ['bench.py'] + %r; import bench; bench.main()" % (lib, args)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=_env(), cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_and_dump_outputs_on_the_emulator(tmp_path, emu):
    """a plain run is the headline alone (--full adds the rest); --steps sets the timed steps; --dump-outputs writes float32
    planes of a fixed sample of the pictures, the same whatever the steps and however the batch is split into pipelines"""
    import numpy as np
    small = ["--frames", "5", "--mb-width", "4", "--mb-height", "3"]
    dumps = []
    for k, extra in enumerate((["--steps", "3", "--warmup", "1"], ["--steps", "1", "--warmup", "0", "--pipelines", "1"])):
        d = tmp_path / ("d%d" % k)
        out = _bench_on_emulator(small + extra + ["--dump-outputs", str(d)])
        assert out["steps"] == int(extra[1]) and out["ms_per_step"] > 0 and out["metric"] == "macroblocks_per_s"
        assert not {"extra", "cpu_baseline"} & set(out) and "alone_us" not in out["roofline"]
        dumps.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    assert sorted(dumps[0]) == ["cb.npy", "cr.npy", "picture_index.npy", "y.npy"]
    n = len(dumps[0]["picture_index.npy"])
    assert 1 <= n <= 4 and dumps[0]["y.npy"].shape == (n, 48, 64) and dumps[0]["cb.npy"].shape == (n, 24, 32)
    assert sum(a.nbytes for a in dumps[0].values()) <= 64 << 20
    for f, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, dumps[1][f]), f
    assert dumps[0]["y.npy"].std() > 0


def test_dump_outputs_needs_a_kernel():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dry", "--dump-outputs", "unused"], capture_output=True, text=True, env=_env(), timeout=120)
    assert r.returncode != 0 and "no outputs" in r.stderr
