#!/usr/bin/env python3
"""Instruction counts per kernel of one .hip file's gfx950 code, to compare two trees: a change that adds a template parameter with a
default, or a new kernel beside the others, must leave every other kernel's instructions as they were.

  python tools/kernel_instruction_counts.py SRC.hip [-I DIR ...] > counts.json          one tree: {kernel: [instructions, digest]}
  python tools/kernel_instruction_counts.py --diff OLD.json NEW.json                    kernels that differ, appear or vanish

The kernel name is the demangled symbol; the digest is over the instruction text with labels and symbol references blanked (they
carry the mangled name, which a new template parameter changes).  Compiles on any machine with hipcc; needs no device."""
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def flags():
    from __graft_entry__ import load_package
    b = load_package().build
    return b.HIPCC, [f for f in b.HIP_FLAGS if f not in ("-shared", "-fPIC")]


def counts(src, extra):
    hipcc, fl = flags()
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run([hipcc] + fl + extra + ["--cuda-device-only", "-S", "-o", out, src], check=True, capture_output=True)
        text = open(out).read()
    res, name, body = {}, None, []
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):\s", line + " ")
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        s = line.strip()
        if s.startswith(".Lfunc_end"):
            res[name] = body
            name = None
            continue
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        s = s.split(";")[0].strip()
        body.append(re.sub(r"(_Z\w+|\.L\w+)", "@", s))
    names = list(res)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines() if names else []
    return {d: [len(res[n]), hashlib.sha256("\n".join(res[n]).encode()).hexdigest()[:16]] for n, d in zip(names, dem)}


def norm(name, old_names):
    """a symbol carries every template argument, defaults included: a name of the new tree that the old tree does not have is also
    looked up without its last argument where that is 1 (k_dec_gemv8's NPL = 1, added behind the old ones)"""
    short = re.sub(r", 1>\(", ">(", name, count=1)
    return short if name not in old_names and short in old_names else name


def main(argv):
    if argv and argv[0] == "--diff":
        old = json.load(open(argv[1]))
        new = {norm(k, old): v for k, v in json.load(open(argv[2])).items()}
        same = sum(1 for k in old if k in new and old[k] == new[k])
        print(f"{len(old)} kernels before, {len(new)} after, {same} identical")
        for k in sorted(set(old) | set(new)):
            if old.get(k) != new.get(k):
                print(("changed " if k in old and k in new else "added   " if k in new else "removed "), old.get(k, ["-"])[0], new.get(k, ["-"])[0], k[:200])
        return 0
    src, extra = argv[0], argv[1:]
    json.dump(counts(src, extra), sys.stdout, indent=0, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
