#!/usr/bin/env python3
"""Is the DEVICE code of two versions of csrc the same?  The check of a host-only change (launch layer, dispatch, validation).

Every *.hip of the two directories is compiled with the Makefile's flags to an unbundled gfx950 device ELF (--offload-device-only
--no-gpu-bundle-output), and per file three things are compared: the .text section, the .rodata section (both dumped with
llvm-objcopy --dump-section) and the list of kernel symbols (the *.kd kernel descriptors of the symbol table, in the table's order).
Sections, not whole files: an ELF also carries names and notes that move with any edit of the host code of the same source.
A plain diff of compiler output - it looks at no instruction.

Usage: device_code_diff.py <csrc A> <csrc B> [file.hip ...] [--hipcc PATH] [--jobs N]     (exit code 1 on any difference; the include
directory is <csrc>/../../include of each side, as in the Makefile)"""
import argparse
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wall", "-Wno-unused-function", "-Wno-pass-failed"]      # csrc/Makefile's CXXFLAGS
SECTIONS = (".text", ".rodata")
MAX_JOBS = 16


def device_code(hipcc, tooldir, src, workdir):
    """-> {".text": digest, ".rodata": digest (None: no such section), "kernels": [names]} of one source file."""
    inc = os.path.join(os.path.dirname(src), "..", "..", "include")
    elf = os.path.join(workdir, "device.elf")
    subprocess.run([hipcc, *FLAGS, "-I" + inc, "--offload-device-only", "--no-gpu-bundle-output", "-c", src, "-o", elf], check=True)
    out = {}
    for sec in SECTIONS:
        dump = os.path.join(workdir, "section.bin")
        if os.path.exists(dump):
            os.remove(dump)
        r = subprocess.run([os.path.join(tooldir, "llvm-objcopy"), "--dump-section", f"{sec}={dump}", elf, os.path.join(workdir, "copy.elf")],
                           capture_output=True, text=True)
        out[sec] = hashlib.sha256(open(dump, "rb").read()).hexdigest() if r.returncode == 0 and os.path.exists(dump) else None
    syms = subprocess.run([os.path.join(tooldir, "llvm-readelf"), "--symbols", "--wide", elf], check=True, capture_output=True, text=True).stdout
    out["kernels"] = [line.split()[-1][:-3] for line in syms.splitlines() if line.endswith(".kd")]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("files", nargs="*", help="file names to compare (default: every *.hip)")
    ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
    ap.add_argument("--jobs", type=int, default=MAX_JOBS)
    args = ap.parse_args()
    tooldir = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(args.hipcc))), "lib", "llvm", "bin")
    names = [sorted(f for f in os.listdir(d) if f.endswith(".hip") and (not args.files or f in args.files)) for d in (args.a, args.b)]
    differ = [f"{f}: only in {args.a if f in names[0] else args.b}" for f in sorted(set(names[0]) ^ set(names[1]))]
    common = [f for f in names[0] if f in names[1]]

    def one(job):
        with tempfile.TemporaryDirectory() as d:
            return device_code(args.hipcc, tooldir, os.path.join(job[0], job[1]), d)

    jobs = [(d, f) for f in common for d in (args.a, args.b)]
    with ThreadPoolExecutor(max_workers=max(1, min(args.jobs, MAX_JOBS))) as ex:
        res = dict(zip(jobs, ex.map(one, jobs)))
    nk = 0
    for f in common:
        ra, rb = res[(args.a, f)], res[(args.b, f)]
        nk += len(ra["kernels"])
        for sec in SECTIONS:
            if ra[sec] != rb[sec]:
                differ.append(f"{f}: {sec} differs")
        if ra["kernels"] != rb["kernels"]:
            gone, new = sorted(set(ra["kernels"]) - set(rb["kernels"])), sorted(set(rb["kernels"]) - set(ra["kernels"]))
            differ.append(f"{f}: kernel symbols differ" + (f" (only in A: {gone[:4]}, only in B: {new[:4]})" if gone or new else " (order)"))
    for line in differ:
        print(line)
    print(f"compared {len(common)} files, {nk} kernels, sections {' '.join(SECTIONS)} and the kernel symbols:",
          "identical" if not differ else f"{len(differ)} differences")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
