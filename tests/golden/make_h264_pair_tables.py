"""Writes the streams of tests/h264_pair_tables.py (tests/golden/h264_pairs_<name>.samples) and records what the REFERENCE's own decoder makes of them
(oracle/_ref/h264_bridge_emu with MI355_BRIDGE_PLAIN: the bridge stepped aside) in tests/golden/h264_pair_tables_md5.json: pictures, bytes, md5 with the loop filter
on and off, and the seconds the same entry takes through the bridge on the SIMT emulator (the tests' time limits are ten times that).  The decoder must not complain
about any stream.  Run from the repository root where the reference tree exists, after __graft_entry__.build():  python tests/golden/make_h264_pair_tables.py [name ...]"""
import hashlib
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import h264_pair_tables as PT  # noqa: E402
import make_h264_streams as W  # noqa: E402


def main():
    T = W.load_tables()
    names = sys.argv[1:] or PT.NAMES
    md5 = dict(PT.MD5)
    for name in names:
        units = PT.build_stream(T, name)
        W.write_samples(PT.samples(name), units)
        size = os.path.getsize(PT.samples(name))
        assert size < 64 << 10, (name, size)
        rec = dict(pictures=len(units), stream_bytes=size)
        with tempfile.TemporaryDirectory() as td:
            for key, nofilter in (("md5", False), ("md5_nofilter", True)):
                out = os.path.join(td, key + ".yuv")
                PT.MD5.setdefault(name, {})["emu_seconds"] = 30.0
                st = PT.run("h264_bridge_emu", name, out, plain=True, nofilter=nofilter)
                assert st["pictures_output"] == len(units) and not st["stderr"].strip(), (name, st)       # every picture decoded, no complaint from the decoder
                raw = open(out, "rb").read()
                rec["bytes"] = len(raw)
                rec[key] = hashlib.md5(raw).hexdigest()
            t0 = time.time()
            st = PT.run("h264_bridge_emu", name, os.path.join(td, "dev.yuv"))
            rec["emu_seconds"] = round(time.time() - t0, 2)
            rec["on_device"] = st["pictures_on_device"]
        md5[name] = rec
        print(name, rec)
    with open(PT.MD5_FILE, "w") as f:
        json.dump({k: md5[k] for k in sorted(md5) if k in PT.TABLE}, f, indent=1, sort_keys=True)
        f.write("\n")
    assert sum(os.path.getsize(PT.samples(n)) for n in PT.NAMES if os.path.exists(PT.samples(n))) < 1 << 20


if __name__ == "__main__":
    main()
