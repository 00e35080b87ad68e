#!/usr/bin/env python3
"""Per-kernel instruction streams of two csrc trees side by side, for a refactor that must not change the code: compiles the named
sources of each tree for the device only (kernel_meta.py's flags), disassembles them, splits the listing by kernel symbol, drops the
padding behind each function's end and compares (runs without a GPU).  A kernel may have moved to another file.
    python scratch/kernel_diff.py OLD_CSRC old1.hip,old2.hip NEW_CSRC new1.hip,new2.hip
prints one line per kernel (same / DIFF, instructions old -> new) and one SHA-256 per new file over its kernels' streams."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

from kernel_meta import FLAGS

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def streams(csrc, f):
    """{mangled kernel name: [instruction, ...]} of one source"""
    with tempfile.TemporaryDirectory() as d:
        co = os.path.join(d, "k.co")
        subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, "--cuda-device-only", "--no-gpu-bundle-output", "-c", f, "-o", co], check=True, cwd=csrc)
        txt = subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(re.sub(r"\s*//.*$", "", line).strip())
    for k in out.values():  # padding behind the function's end ("...": a run of zero bytes)
        while k and k[-1].split()[0] in ("s_nop", "s_code_end", "..."):
            k.pop()
    return {k: v for k, v in out.items() if v}


def pretty(mangled):
    name = subprocess.run(["c++filt", mangled], capture_output=True, text=True).stdout.strip()
    return re.sub(r"\(.*\)$", "", re.sub(r"^void ", "", name))


def main():
    old_dir, old_files, new_dir, new_files = sys.argv[1], sys.argv[2].split(","), sys.argv[3], sys.argv[4].split(",")
    old = {}
    for f in old_files:
        old.update(streams(old_dir, f))
    n_same = n_diff = 0
    for f in new_files:
        new = streams(new_dir, f)
        h = hashlib.sha256()
        for k in sorted(new):
            h.update(("\n".join([k] + new[k]) + "\n").encode())
            if k not in old:
                print(f"NEW   {f} `{pretty(k)}` {len(new[k])}")
                continue
            o = old.pop(k)
            same = o == new[k]
            n_same += same
            n_diff += not same
            print(f"{'same' if same else 'DIFF'}  {f} `{pretty(k)}` {len(o)} -> {len(new[k])}")
        print(f"sha256 {f} {h.hexdigest()}")
    for k in sorted(old):
        print(f"MISSING `{pretty(k)}`")
    print(f"{n_same} kernels identical, {n_diff} differ, {len(old)} missing")


if __name__ == "__main__":
    main()
