#!/usr/bin/env python
"""Is the device code of two source trees the same?  Needs no GPU.

    python tools/device_code_diff.py <parent csrc> <head csrc> [-j N] > profiles/.../device_code.txt

Every *.hip of either tree is compiled with the Makefile's flags plus ``--cuda-device-only -S``; per kernel symbol (.amdhsa_kernel)
the instruction text of its function body and its .amdhsa_* metadata block are compared, as is the set of symbols.  Lines that name
the per-compile random ``__hip_cuid_*`` symbol are dropped: two compiles of one file differ in exactly those.  Kernels are matched by
symbol, not by position, and the function ordinal in block labels (.LBB<ordinal>_<block>) is blanked: host code that instantiates the
same templates in another order moves the kernels within the module and changes nothing in them.  Prints one line per
file, "identical, N kernels" or what differs; exit status 1 when anything differs.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-Wall", "-Wno-unused-function"]      # csrc/Makefile


def device_asm(src, include):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "a.s")
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")] + FLAGS + ["-I" + include, "--cuda-device-only", "-S", src,
                               "-o", out], cwd=os.path.dirname(src))
        with open(out) as f:
            return [l.rstrip() for l in f if "__hip_cuid_" not in l]


def kernels(lines):
    """{symbol: (body lines, metadata lines)}: the body from the symbol's label to its .Lfunc_end, the .amdhsa_kernel block."""
    names = [m.group(1) for l in lines for m in [re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)] if m]
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end") and lines[i].endswith(":"))
        m0 = next(i for i, l in enumerate(lines) if re.match(r"\s*\.amdhsa_kernel\s+" + re.escape(name) + r"$", l))
        m1 = next(i for i in range(m0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        # .LBB<f>_<n>: <f> is the function's ordinal in the module, i.e. the order in which the host code first instantiates the
        # templates, not a property of the kernel; <n>, the block within the function, stays
        body = [re.sub(r"\.LBB\d+_", ".LBB_", l.split(";")[0].rstrip()) for l in lines[start:end]]
        out[name] = ([l for l in body if l.strip()], lines[m0:m1 + 1])
    return out


def compare(name, parent_dir, head_dir, include_parent, include_head):
    paths = [os.path.join(d, name) for d in (parent_dir, head_dir)]
    if not all(os.path.exists(p) for p in paths):
        return "%-28s DIFFERS: the file exists in one tree only" % name, False
    a, b = kernels(device_asm(paths[0], include_parent)), kernels(device_asm(paths[1], include_head))
    if set(a) != set(b):
        return "%-28s DIFFERS: kernel symbols %s" % (name, sorted(set(a) ^ set(b))), False
    bad = [k for k in a if a[k] != b[k]]
    if bad:
        return "%-28s DIFFERS: %d of %d kernels: %s" % (name, len(bad), len(a), bad[:4]), False
    return "%-28s identical, %d kernels (%d instruction lines)" % (name, len(a), sum(len(v[0]) for v in a.values())), True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_csrc")
    ap.add_argument("head_csrc")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("--only", nargs="*", help="file names (default: every *.hip of either tree)")
    args = ap.parse_args()
    inc = lambda csrc: os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(csrc))), "include")
    files = args.only or sorted({f for d in (args.parent_csrc, args.head_csrc) for f in os.listdir(d) if f.endswith(".hip")})
    with ThreadPoolExecutor(args.j) as pool:
        results = list(pool.map(lambda f: compare(f, os.path.abspath(args.parent_csrc), os.path.abspath(args.head_csrc),
                                                  inc(args.parent_csrc), inc(args.head_csrc)), files))
    for line, _ in results:
        print(line)
    same = all(ok for _, ok in results)
    print("%d files, %d kernels: %s" % (len(files), sum(int(re.search(r"(\d+) kernels", l).group(1)) for l, ok in results if ok),
                                        "device code identical" if same else "DEVICE CODE DIFFERS"))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
