#!/usr/bin/env python3
"""Compare the device code of two builds of eicos_amd/csrc, unit by unit.  CPU only: hipcc cross-compiles for gfx950.

    tools/dev/compare_device_builds.py A B [--out DIR] [--jobs N] [--lengths]

A and B are each either
  * a source tree (it has eicos_amd/csrc/Makefile): every device unit of the Makefile's DEVOBJ is compiled with the Makefile's
    CXXFLAGS / DEVFLAGS plus `-Rpass-analysis=kernel-resource-usage -save-temps=obj` into DIR/a/<unit>/ or DIR/b/<unit>/, the units
    of both trees side by side, at most 16 at a time (`git worktree add` or `git archive` gives the tree of another commit); or
  * a directory such a run left behind: <unit>/<unit>.log (the compiler's stderr) and <unit>/<unit>-hip-amdgcn-*.s.

Per unit it prints
  * whether the resource remarks (registers, scratch, spills, occupancy, LDS) of every kernel are equal, source locations
    stripped, and both values of every kernel where they are not;
  * how many device functions have identical ISA text and how many differ -- comments, blank lines and .loc / .file / .ident /
    .cfi lines dropped, the function's index taken out of its local labels -- with the name and the instruction-line count
    (A -> B) of each that differs (--lengths: of every function that exists on one side only, too).
The exit status is 0 when every unit has equal remarks, 1 otherwise; differing functions alone do not fail it.

It reports register and size numbers and function equality, nothing else about the ISA.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys

REMARK = re.compile(r"^remark: [^ ]*: (\s*)(.*?) \[-Rpass-analysis=kernel-resource-usage\]$")
DROP = re.compile(r"^\s*\.(loc|file|ident|cfi_\w+)\b")
LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+_")  # .LBB12_3 -> .LBB_3: 12 is the function's position in the unit
COUNTED = re.compile(r"\.L([A-Za-z_]+?)(\d+)\b(?!_)")  # .Lpost_getpc40, .Ltmp7: 40 counts over the whole unit -> renumbered per function


def make_var(csrc, name):
    out = subprocess.run(["make", "-s", "-C", csrc, "--eval", f"print-var: ; @echo $({name})", "print-var"],
                         check=True, capture_output=True, text=True).stdout
    return out.split()


def plan(tree, out):
    """(units, compile jobs) of one side: jobs is empty when `tree` already holds a run's output."""
    csrc = os.path.join(tree, "eicos_amd", "csrc")
    if not os.path.isfile(os.path.join(csrc, "Makefile")):
        return tree, sorted(os.path.basename(os.path.dirname(p)) for p in glob.glob(os.path.join(tree, "*", "*.log"))), []
    units = [o[:-2] for o in make_var(csrc, "DEVOBJ")]
    hipcc, arch = make_var(csrc, "HIPCC")[0], make_var(csrc, "ARCH")[0]
    flags = make_var(csrc, "CXXFLAGS") + make_var(csrc, "DEVFLAGS") + ["-Rpass-analysis=kernel-resource-usage", "-save-temps=obj"]
    jobs = []
    for u in units:
        d = os.path.join(out, u)
        os.makedirs(d, exist_ok=True)
        jobs.append((csrc, [hipcc, f"--offload-arch={arch}"] + flags + ["-c", u + ".hip", "-o", os.path.join(d, u + ".o")], os.path.join(d, u + ".log")))
    return out, units, jobs


def compile_unit(job):
    cwd, cmd, log = job
    with open(log, "w") as f:
        rc = subprocess.run(cmd, cwd=cwd, stderr=f).returncode
    return rc, log


def remarks(log):
    """{kernel: {field: value}} of a compile log."""
    res, cur = {}, None
    for line in open(log):
        m = REMARK.match(line.rstrip("\n"))
        if not m:
            continue
        key, _, val = m.group(2).partition(": ")
        if key == "Function Name":
            cur = res.setdefault(val, {})
        elif cur is not None:
            cur[key] = val
    return res


def functions(asm):
    """{function: [normalised lines]} of a device assembly file: from the function's label to its .Lfunc_end."""
    res, name, body, pending, seen = {}, None, [], None, {}
    renumber = lambda m: f".L{m.group(1)}#{seen.setdefault(m.group(0), len(seen))}"
    for line in open(asm):
        line = line.split(";", 1)[0].rstrip()
        if not line.strip() or DROP.match(line):
            continue
        if name is None:
            m = re.match(r"^\s*\.type\s+(\S+),@function$", line)
            if m:
                pending = m.group(1)
            elif pending and line == pending + ":":
                name, body, pending, seen = pending, [], None, {}
        elif line.startswith(".Lfunc_end"):
            res[name], name = body, None
        else:
            body.append(COUNTED.sub(renumber, LOCAL.sub(r".L\1_", line)))
    return res


def n_instr(body):  # instruction lines: neither directives nor labels
    return sum(1 for l in body if not l.lstrip().startswith(".") and not l.endswith(":"))


def demangler():
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            subprocess.run([tool, "--version"], capture_output=True, check=True)
            return lambda names: dict(zip(names, subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()))
        except (OSError, subprocess.CalledProcessError):
            pass
    return lambda names: {n: n for n in names}


def short(pretty):  # the demangled name without its argument list
    depth = 0
    for i, c in enumerate(pretty):
        depth += c == "<"
        depth -= c == ">"
        if c == "(" and depth == 0:
            return pretty[:i]
    return pretty


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("a"), ap.add_argument("b")
    ap.add_argument("--out", default="build_exp/compare_device_builds", help="where the units of a source tree are compiled (default: %(default)s)")
    ap.add_argument("--jobs", type=int, default=min(16, os.cpu_count() or 1))
    ap.add_argument("--lengths", action="store_true", help="also list the functions that exist on one side only")
    args = ap.parse_args()
    sides = [plan(os.path.abspath(t), os.path.join(os.path.abspath(args.out), s)) for t, s in ((args.a, "a"), (args.b, "b"))]
    jobs = sides[0][2] + sides[1][2]
    if jobs:
        print(f"compiling {len(jobs)} units, {max(1, min(args.jobs, 16))} at a time ...", flush=True)
        with concurrent.futures.ThreadPoolExecutor(max(1, min(args.jobs, 16))) as pool:
            for rc, log in pool.map(compile_unit, jobs):
                if rc != 0:
                    sys.exit(f"the compiler failed: see {log}")
    units = [u for u in sides[0][1] if u in sides[1][1]]
    if not units or set(sides[0][1]) != set(sides[1][1]):
        print(f"units of A: {sides[0][1]}\nunits of B: {sides[1][1]}")
    pretty = demangler()
    all_equal = bool(units)
    for u in units:
        ra, rb = (remarks(os.path.join(d, u, u + ".log")) for d, _, _ in sides)
        asm = [glob.glob(os.path.join(d, u, u + "-hip-amdgcn-*.s")) for d, _, _ in sides]
        if not all(asm):
            sys.exit(f"no device assembly {u}-hip-amdgcn-*.s under {' or '.join(os.path.join(d, u) for (d, _, _), a in zip(sides, asm) if not a)}")
        fa, fb = functions(asm[0][0]), functions(asm[1][0])
        names = pretty(sorted(set(ra) | set(rb) | set(fa) | set(fb)))
        moved = sorted(k for k in set(ra) | set(rb) if ra.get(k) != rb.get(k))
        all_equal &= not moved
        print(f"== {u}: {len(ra)} / {len(rb)} kernels, resource remarks {'EQUAL' if not moved else 'DIFFER'}")
        for k in moved:
            print(f"   {short(names[k])}")
            for f in sorted(set(ra.get(k, {})) | set(rb.get(k, {}))):
                va, vb = ra.get(k, {}).get(f, "-"), rb.get(k, {}).get(f, "-")
                if va != vb:
                    print(f"      {f}: {va} -> {vb}")
        both = sorted(set(fa) & set(fb))
        differ = [k for k in both if fa[k] != fb[k]]
        only = sorted(set(fa) ^ set(fb))
        print(f"   device functions: {len(both) - len(differ)} identical, {len(differ)} differ, {len(only)} on one side only")
        for k in differ:
            print(f"      differs  {short(names[k])}: {n_instr(fa[k])} -> {n_instr(fb[k])} instruction lines")
        for k in only if args.lengths or len(only) <= 8 else []:
            print(f"      only in {'A' if k in fa else 'B'}  {short(names[k])}: {n_instr(fa.get(k) or fb[k])} instruction lines")
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())
