#!/usr/bin/env python3
"""Developer tool: per kernel of a device assembly file (hipcc --cuda-device-only -S), the instruction count, a hash of the
instruction stream from the kernel's label to its s_endpgm (comments stripped) and the resource lines.  Two builds whose lines
agree have the same device code.  Usage: isa_kernel_hash.py FILE.s [NAME_FILTER [DUMP_DIR]]  (DUMP_DIR: each stream as a file, to diff)"""
import hashlib, os, re, subprocess, sys

text = open(sys.argv[1]).read()
want = sys.argv[2] if len(sys.argv) > 2 else ""
dump = sys.argv[3] if len(sys.argv) > 3 else None
if dump:
    os.makedirs(dump, exist_ok=True)
for name, desc in re.findall(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", text, re.S):
    if want not in name:
        continue
    body = re.search(r"^%s:[^\n]*\n(.*?^\s+s_endpgm)" % re.escape(name), text, re.S | re.M).group(1)
    ins = [re.sub(r"\s+", " ", l.split(";")[0]).strip() for l in body.split("\n")]
    ins = [l for l in ins if l and not l.startswith(".")]
    # local labels carry the number of the function in the file (.LBB10_25): a symbol name, not part of the stream
    ins = [re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", l) for l in ins]
    # ... and so does the label of a long branch's s_getpc (.Lpost_getpc8): numbered through the file in the order the kernels are emitted
    ins = [re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", l) for l in ins]
    r = dict(re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|group_segment_fixed_size|private_segment_fixed_size) (\d+)", desc))
    # the instance: the demangled name without its namespace, return type and parameter list (the "(" that follows the template arguments)
    full = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip().replace("(anonymous namespace)::", "")
    full = re.sub(r"^void ", "", full)
    depth, end = 0, len(full)
    for i, ch in enumerate(full):
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            end = i
            break
    short = full[:end]
    print("%-40s %6d instr %s vgpr %s sgpr %s lds %s scratch %s" % (short, len(ins), hashlib.sha1("\n".join(ins).encode()).hexdigest()[:12],
          r["next_free_vgpr"], r["next_free_sgpr"], r["group_segment_fixed_size"], r["private_segment_fixed_size"]))
    if dump:
        open(os.path.join(dump, re.sub(r"\W", "_", short) + ".txt"), "w").write("\n".join(ins) + "\n")
