#!/usr/bin/env python3
"""Compare two device code objects kernel by kernel: instruction text and register / scratch / LDS use (no GPU needed).

  cd promptable-counterfactual-gan_amd/csrc
  hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Wall -Wno-unused-function --offload-device-only --no-gpu-bundle-output \\
        -c -o new.co conv_igemm.hip                   # and old.co from the parent commit's tree
  python scripts/compare_code_objects.py old.co new.co [--sub REGEX REPL ...]

--sub rewrites the OLD side's demangled names before matching (a template parameter list that changed without changing any
code).  Prints the symbols found on one side only and every common symbol whose instructions or resources differ; exits 1 if
any common symbol differs.  A refactor that claims "no kernel changed" should come out with no differing symbol."""
import argparse
import re
import subprocess
import sys

LLVM = "/opt/rocm/llvm/bin/"
RESOURCES = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
             "group_segment_fixed_size")


def run(cmd, stdin=None):
    return subprocess.run(cmd, input=stdin, capture_output=True, text=True, check=True).stdout


def disassembly(co):
    """{demangled symbol: instruction text without comments}"""
    syms, cur = {}, None
    for line in run([LLVM + "llvm-objdump", "-d", "-C", "--no-show-raw-insn", "--no-leading-addr", co]).splitlines():
        m = re.fullmatch(r"<(.*)>:", line)
        if m:
            cur = syms.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*", "", line))
    return {k: "\n".join(v) for k, v in syms.items()}


def resources(co):
    """{demangled kernel name: (resource counts)} from the AMDGPU metadata note"""
    notes = run([LLVM + "llvm-readelf", "--notes", co])
    rows = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        rows[name] = tuple(int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in RESOURCES)
    names = list(rows)
    demangled = run(["c++filt"], "\n".join(names)).splitlines()
    return {d: rows[n] for n, d in zip(names, demangled)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--sub", nargs=2, action="append", default=[], metavar=("REGEX", "REPL"))
    args = ap.parse_args()

    def rename(d):
        out = {}
        for k, v in d.items():
            for pat, rep in args.sub:
                k = re.sub(pat, rep, k)
            out[k] = v
        return out

    bad = 0
    for what, old, new in (("instructions", rename(disassembly(args.old)), disassembly(args.new)),
                           ("resources", rename(resources(args.old)), resources(args.new))):
        common = sorted(old.keys() & new.keys())
        diff = [k for k in common if old[k] != new[k]]
        print(f"{what}: {len(old)} old, {len(new)} new, {len(common)} common, {len(diff)} differ")
        for k in sorted(old.keys() - new.keys()):
            print(f"  only old: {k}")
        for k in sorted(new.keys() - old.keys()):
            print(f"  only new: {k}")
        for k in diff:
            print(f"  DIFFERS:  {k}" + (f"  {dict(zip(RESOURCES, old[k]))} -> {dict(zip(RESOURCES, new[k]))}" if what == "resources" else ""))
        bad += len(diff)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
