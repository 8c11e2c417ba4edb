"""Records tests/golden/hevc_filter_tables_sha1.json from the REFERENCE's own functions (oracle/_ref/libhevcfilterref.so: hevc_filter.c compiled in place):
the deblocked pictures of tests/hevc_filter_tables.py's deblocking table and the strengths of its boundary-strength table.  Digests only.
Run from the repository root where the reference tree exists:  python tests/golden/make_hevc_filter_tables.py"""
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import hevc_filter_tables as T  # noqa: E402


def main():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "_ref/libhevcfilterref.so"], check=True)
    ref = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libhevcfilterref.so"))
    ref.ref_hevc_deblock_picture.restype = C.c_int
    out = {"source": "libavcodec/hevc_filter.c + hevcdsp_template.c of the reference, driven by oracle/ref_hevc_filter_glue.c", "deblock": {}, "bs": {}}
    for name in T.LF_CASES:
        out["deblock"][name] = [T.digest(T.lf_host(ref.ref_hevc_deblock_picture, case)) for case in T.lf_launch(name)]
    for name in T.BS_CASES:
        c = T.BsCase(name)
        out["bs"][name] = T.bs_digest(c, *T.bs_host(ref.ref_hevc_boundary_strengths, c, with_blocks=True))
    with open(os.path.join(ROOT, "tests", "golden", "hevc_filter_tables_sha1.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
