#!/usr/bin/env python3
"""Are the kernels of two source trees the same machine code?

    scripts/isa_diff.py PARENT_CSRC [THIS_CSRC] [--allow-removed REGEX]

Compiles every .hip file of both csrc directories to device-only gfx950
assembly (no GPU needed), splits the assembly by function symbol and compares,
kernel by kernel, the instruction text, the .amdhsa_* descriptor block and the
compiler's resource summary (registers, LDS, scratch, occupancy).  Kernels are
matched by demangled name whatever file they live in, so code that moved
between translation units compares against where it used to be.  Labels that
number the function inside its file (.LBB12_3) are made position-free first.
Files present in both trees are also compared as a whole.

Exit status 0: every kernel in both trees is identical, nothing was added,
and what was removed matches --allow-removed (if given).
"""
import argparse
import concurrent.futures
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("ARCH", "gfx950")

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):\s*; @")
STATIC = re.compile(r"(\.static\.|__static__)[0-9a-f]+")
POSITION = [(re.compile(r"\.LBB\d+_"), ".LBB_"), (re.compile(r"\bBB\d+_"), "BB_"),
            (re.compile(r"\.Lfunc_(begin|end)\d+"), r".Lfunc_\1"), (re.compile(r"\.LJTI\d+_"), ".LJTI_"),
            (re.compile(r"[ \t]+"), " ")]  # (comments are aligned to a column after the label)
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")  # a hash of the source file's path


def assemble(csrc, out, reuse):
    inc = ["-I" + os.path.join(csrc, "..", "..", "include"), "-I" + csrc]
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))

    def one(f):
        s = os.path.join(out, f[:-4] + ".s")
        if not (reuse and os.path.exists(s)):
            subprocess.run([HIPCC, "--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", *inc, "--cuda-device-only",
                            "-S", os.path.join(csrc, f), "-o", s], check=True, stderr=subprocess.DEVNULL)
        return f, s

    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
        return dict(ex.map(one, files))


def functions(path):
    """{symbol: (is_kernel, text)}: label .. end of the resource summary."""
    lines = open(path).read().split("\n")
    starts = [(i, m.group(1)) for i, l in enumerate(lines) if (m := LABEL.match(l))]
    out = {}
    for n, (i, sym) in enumerate(starts):
        end = starts[n + 1][0] if n + 1 < len(starts) else len(lines)
        body, in_info = [], False
        for l in lines[i:end]:
            if in_info and not l.startswith(";"):
                break  # the next function's preamble
            if ".section\t.AMDGPU.csdata" in l:
                in_info = True
            if l.lstrip().startswith(".section\t.text"):
                continue  # names the section after the symbol: nothing new
            body.append(l)
        text = "\n".join(body).replace(sym, "<SYM>")
        text = STATIC.sub("", text)
        for rx, to in POSITION:
            text = rx.sub(to, text)
        out[STATIC.sub("", sym)] = (".amdhsa_kernel" in text, text)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        r = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def collect(asm):
    fns = {}
    for f, s in asm.items():
        for sym, (k, text) in functions(s).items():
            fns.setdefault(sym, []).append((f, k, text))
    return fns


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gossip_simulator_amd", "csrc")
    ap.add_argument("parent")
    ap.add_argument("this", nargs="?", default=os.path.normpath(here))
    ap.add_argument("--allow-removed", metavar="REGEX", help="every removed kernel's demangled name must match")
    ap.add_argument("--keep", metavar="DIR", help="keep the assembly under DIR/parent and DIR/this")
    ap.add_argument("--reuse-parent", action="store_true", help="with --keep: do not recompile DIR/parent's assembly")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    asm = {}
    for tag, csrc in (("parent", a.parent), ("this", a.this)):
        os.makedirs(os.path.join(tmp, tag), exist_ok=True)
        asm[tag] = assemble(os.path.abspath(csrc), os.path.join(tmp, tag), tag == "parent" and a.reuse_parent)
    old, new = collect(asm["parent"]), collect(asm["this"])
    names = demangle(sorted(set(old) | set(new)))
    bad = 0

    # a symbol compiled in several files of one tree (a library kernel both
    # instantiate) must be the same in each
    same = differ = 0
    for sym in sorted(set(old) & set(new)):
        if not any(k for _, k, _ in old[sym] + new[sym]):
            continue  # device functions that were not inlined: compared below
        ref = old[sym][0][2]
        diffs = [(f, t) for f, _, t in old[sym][1:] + new[sym] if t != ref]
        if not diffs:
            same += 1
            continue
        differ += 1
        for f, t in diffs:
            d = [l for l in difflib.unified_diff(ref.split("\n"), t.split("\n"), lineterm="", n=0)
                 if l[:1] in "+-" and l[:3] not in ("+++", "---")]
            print(f"DIFFERS  {names[sym]}  ({old[sym][0][0]} -> {f}): {len(d)} lines")
            for l in d[:12]:
                print("    " + l)
    print(f"kernels in both trees: {same + differ}, identical: {same}, differing: {differ}")
    bad += differ

    fn_same = fn_diff = 0
    for sym in sorted(set(old) & set(new)):
        if any(k for _, k, _ in old[sym] + new[sym]):
            continue
        ok = all(t == old[sym][0][2] for _, _, t in new[sym])
        fn_same += ok
        fn_diff += not ok
        if not ok:
            print(f"DIFFERS  (device function) {names[sym]}")
    print(f"device functions not inlined, in both trees: {fn_same + fn_diff}, identical: {fn_same}")
    bad += fn_diff

    removed = sorted(names[s] for s in set(old) - set(new))
    added = sorted(names[s] for s in set(new) - set(old))
    print(f"removed: {len(removed)}")
    for n in removed:
        ok = not a.allow_removed or re.search(a.allow_removed, n)
        print(("  " if ok else "  NOT ALLOWED  ") + n)
        bad += not ok
    print(f"added: {len(added)}")
    for n in added:
        print("  " + n)
    bad += len(added)

    for f in sorted(set(asm["parent"]) & set(asm["this"])):
        whole = CUID.sub("", open(asm["parent"][f]).read()) == CUID.sub("", open(asm["this"][f]).read())
        print(f"whole file {f}: {'identical' if whole else 'differs (see the kernels above)'}")
    if not a.keep:
        shutil.rmtree(tmp)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
