#!/usr/bin/env python3
"""Static VALU / SALU / LDS counts of one loop of a kernel, grouped by the statement of the loop body they were inlined from
(hipcc -S -gline-tables-only: the outermost `@[ file:line` of a .loc inside the given line range names the phase).
usage: isa_phases.py file.s kernel_label_substring loop_header_label first_line last_line [skip_first-skip_last ...]
  loop_header_label: e.g. BB1_53 (the blocks commented `in Loop: Header=BB1_53`, and the header itself)
  first_line last_line: the source lines of the loop body in the kernel's main file
  skip ranges: source lines (anywhere in the inlining chain) left out of the count, e.g. the edge arithmetic behind a wave-level vote"""
import collections
import re
import sys


def kind(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_")):
        return "vmem"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path, kname, header, lo, hi = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
    skips = [tuple(int(v) for v in a.split("-")) for a in sys.argv[6:]]
    inside, in_loop, phase, skipped = False, False, "?", False
    cnt = collections.defaultdict(collections.Counter)
    for l in open(path):
        if re.match(r"^_Z\w*%s\w*:" % re.escape(kname), l):
            inside = True
            continue
        if inside and l.startswith(".Lfunc_end"):
            break
        if not inside:
            continue
        m = re.match(r"^\.L(BB\d+_\d+):(.*)", l)
        if m:
            in_loop = m.group(1) == header or ("Header=%s " % header) in m.group(2) + " "
            continue
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)\s+\d+.*?;\s*(\S+?):(\d+):\d+(.*)", l)
        if m:
            fileno, line, rest = int(m.group(1)), int(m.group(2)), m.group(5)
            chain = [(m.group(3), line)] + [(f, int(n)) for f, n in re.findall(r"@\[\s*(\S+?):(\d+):\d+", rest)]
            main_file = [n for f, n in chain if f.endswith(".hip") and lo <= n <= hi]
            phase = str(main_file[-1]) if main_file else "outside %d-%d" % (lo, hi)
            skipped = any(f.endswith(".hip") and a <= n <= b for f, n in chain for a, b in skips)
            continue
        m = re.match(r"^\t([a-z_0-9]+)", l)
        if m and in_loop:
            cnt[phase + (" (skipped)" if skipped else "")][kind(m.group(1))] += 1
    tot = collections.Counter()
    for ph, c in sorted(cnt.items()):
        if "(skipped)" not in ph:
            tot.update(c)
        print("%-24s valu %4d salu %4d lds %3d vmem %3d" % (ph, c["valu"], c["salu"], c["lds"], c["vmem"]))
    print("TOTAL (not skipped)", dict(tot))


if __name__ == "__main__":
    main()
