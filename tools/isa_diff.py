#!/usr/bin/env python3
"""Which kernels of a .hip file changed between a git revision and the working tree -- at the instruction level (no GPU).
    python tools/isa_diff.py dtlr_amd/csrc/msda_enc.hip [--rev HEAD] [--defs=-DDTLR_HALF_IS_F16]
    python tools/isa_diff.py --all [--rev HEAD] [--defs=...] [-j N]        every csrc/*.hip: one line per kernel plus a total
    python tools/isa_diff.py --all --moved sg_ln_kernel=gr_layernorm256_kernel ..       a kernel that was renamed or moved to another file:
                                                                           MOVED-SAME (not counted as changed) or MOVED-CHANGED
Compiles both versions for gfx950 with --save-temps and compares every kernel's instruction stream (basic-block label numbers
normalised).  The old side is compiled inside a copy of the REVISION's dtlr_amd/csrc and include (git archive), so a header that
changed between the two does not leak into it.  Use: adding a variant / template instantiation next to a verified kernel, or moving
inline helpers between files, must leave the verified kernels SAME."""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "dtlr_amd/csrc"


def kernels(tree, name, defs):
    """{kernel symbol: [instructions]} of tree/dtlr_amd/csrc/<name>, compiled against that tree's own headers."""
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{tree}/include", f"-I{tree}/{CSRC}",
                               "--save-temps", "-c", f"{tree}/{CSRC}/{name}", "-o", "x.o"] + defs, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        asm = [f for f in os.listdir(d) if f.endswith(".s") and "amdgcn" in f][0]
        lines = open(os.path.join(d, asm)).read().split("\n")
    out, i = {}, 0
    while i < len(lines):
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", lines[i])
        if m and i + 1 < len(lines) and not lines[i].startswith("."):
            j = i + 1                                    # the whole body (a kernel with an early exit has several s_endpgm): up to the kernel
            while j < len(lines) and not re.match(r"^(\.Lfunc_end|\s+\.section\b|_Z\w+:)", lines[j]):      # descriptor's section / .Lfunc_end
                j += 1
            body = [re.sub(r"\.LBB\d+_", ".LBB_", x.split(";")[0].rstrip()) for x in lines[i + 1:j] if x.split(";")[0].strip()]
            if j < len(lines) and not lines[j].startswith("_Z") and any(x.strip().startswith("s_endpgm") for x in body):
                out[m.group(1)] = body
                i = j
        i += 1
    return out


def diff_file(old_tree, name, defs, gone=None, came=None):
    """(report lines, kernels compared, kernels that differ) for one file; a file the revision does not have is all NEW.  gone / came:
    dicts that receive the bodies of the REMOVED / NEW kernels (for --moved)."""
    a = kernels(old_tree, name, defs) if os.path.exists(f"{old_tree}/{CSRC}/{name}") else {}
    b = kernels(ROOT, name, defs) if os.path.exists(f"{ROOT}/{CSRC}/{name}") else {}
    if gone is not None:
        gone.update({k: a[k] for k in a if k not in b})
        came.update({k: b[k] for k in b if k not in a})
    rep, changed = [], 0
    for k in sorted(set(a) | set(b)):
        if k not in a:
            rep.append(f"NEW      {k}  ({len(b[k])} instructions)")
        elif k not in b:
            rep.append(f"REMOVED  {k}")
            changed += 1
        elif a[k] == b[k]:
            rep.append(f"SAME     {k}  ({len(a[k])})")
        else:
            rep.append(f"CHANGED  {k}  ({len(a[k])} -> {len(b[k])})")
            changed += 1
    return rep, len(set(a) | set(b)), changed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("source", nargs="?")
    ap.add_argument("--all", action="store_true", help="every dtlr_amd/csrc/*.hip of the working tree and of the revision")
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--defs", default="")
    ap.add_argument("-j", type=int, default=8, help="files compiled at a time with --all")
    ap.add_argument("--moved", action="append", default=[], metavar="OLD=NEW", help="with --all: a REMOVED kernel whose symbol contains OLD is "
                    "compared with the NEW kernel whose symbol contains NEW (a kernel renamed or moved to another file); repeatable")
    args = ap.parse_args()
    if bool(args.source) == args.all:
        ap.error("give one source file or --all")
    defs = args.defs.split()
    with tempfile.TemporaryDirectory() as old_tree:
        ar = subprocess.Popen(["git", "archive", args.rev, CSRC, "include"], cwd=ROOT, stdout=subprocess.PIPE)
        subprocess.check_call(["tar", "-x", "-C", old_tree], stdin=ar.stdout)
        if ar.wait():
            sys.exit(f"git archive {args.rev} failed")
        if not args.all:
            rel = os.path.relpath(os.path.abspath(args.source), ROOT)
            rep, _, changed = diff_file(old_tree, os.path.basename(rel), defs)
            print("\n".join(rep))
            sys.exit(1 if changed else 0)
        names = sorted({os.path.basename(p) for t in (ROOT, old_tree) for p in glob.glob(f"{t}/{CSRC}/*.hip")})
        total = changed = new = moved = 0
        gone, came = {}, {}
        with concurrent.futures.ThreadPoolExecutor(args.j) as pool:
            reports = list(zip(names, pool.map(lambda f: diff_file(old_tree, f, defs, gone, came), names)))
        verdict = {}                                     # REMOVED symbol -> its line as a moved kernel
        for old, new_ in (m.split("=", 1) for m in args.moved):
            for k in (k for k in gone if old in k):
                to = [n for n in came if new_ in n]
                if len(to) != 1:
                    sys.exit(f"--moved {old}={new_}: {len(to)} NEW kernels contain '{new_}'")
                same = gone[k] == came[to[0]]
                verdict[k] = f"MOVED-{'SAME' if same else 'CHANGED'}  {k} -> {to[0]}  ({len(gone[k])} -> {len(came[to[0]])})"
                moved += same
        for name, (rep, n, c) in reports:
            for line in rep:
                print(f"{name:16s} {verdict.get(line.split()[1], line) if line.startswith('REMOVED') else line}")
            total, changed, new = total + n, changed + c, new + sum(x.startswith("NEW") for x in rep)
        changed -= moved
        print(f"TOTAL    {len(names)} files, {total} kernels: {total - changed - new - moved} SAME, {new} NEW, {moved} MOVED-SAME, {changed} CHANGED or REMOVED  "
              f"(rev {args.rev}, defs '{args.defs}')")
        sys.exit(1 if changed else 0)


if __name__ == "__main__":
    main()
