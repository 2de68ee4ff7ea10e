#!/usr/bin/env python3
"""Compares the device code of two source trees, kernel by kernel.

    tools/kernel_isa_diff.py <tree A> <tree B> [-j N] [--names A B]

Every cartographer_amd/csrc/*.hip of both trees is compiled device-only to gfx950 assembly with
the tree's own build.HIP_FLAGS (no GPU needed), the output is split per kernel symbol, and for
every kernel the report says whether the instruction stream is the same on both sides (local
labels renumbered, comments dropped) and prints the register, LDS and scratch figures of both.
Kernels are matched by symbol across the whole tree, so one that moved to another file is still
compared with itself.  A symbol that more than one file of a tree defines (kernels of the same
name and signature in two anonymous namespaces mangle alike) names several kernels: those are
matched by file and symbol instead, and a line of the report names them.  Kernels of source files that are byte-equal in both trees must come out
identical (the tool's own sanity check): they are summed up in one line per file unless one
differs or --all is given.  Exit status 1 when a kernel differs or exists on one side only: a refactor
of a kernel file is done when this prints "identical" on every line.
"""
import argparse
import glob
import importlib.util
import os
import re
import shutil
import subprocess
import sys
import tempfile

FIGURES = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")


def load_build(tree):
    path = os.path.join(tree, "cartographer_amd", "build.py")
    spec = importlib.util.spec_from_file_location("build_" + str(abs(hash(tree))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def compile_tree(tree, out_dir, jobs):
    """{file name: assembly text} of the tree's .hip files."""
    build = load_build(tree)
    srcs = sorted(glob.glob(os.path.join(tree, "cartographer_amd", "csrc", "*.hip")))
    pending, running, texts = list(srcs), [], {}
    while pending or running:
        while pending and len(running) < jobs:
            src = pending.pop(0)
            out = os.path.join(out_dir, os.path.basename(src) + ".s")
            cmd = [build.HIPCC] + build.HIP_FLAGS + ["--cuda-device-only", "-S", src, "-o", out]
            running.append((src, out, subprocess.Popen(cmd, stderr=subprocess.PIPE, text=True)))
        src, out, proc = running.pop(0)
        _, err = proc.communicate()
        if proc.returncode != 0:
            sys.exit(f"hipcc failed on {src}:\n{err}")
        with open(out) as f:
            texts[os.path.basename(src)] = f.read()
    return texts


LOCAL_LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+(_\d+)?")


def normalise(line):
    line = line.split(";", 1)[0].strip()
    # .LBB<function>_<block>: the function number depends on what else the file holds.
    return LOCAL_LABEL.sub(lambda m: ".L" + m.group(1) + (m.group(2) or ""), line)


def split_kernels(text):
    """{symbol: (instruction stream, figures)} of one assembly file."""
    lines = text.split("\n")
    figures, entry = {}, None
    meta = [i for i, l in enumerate(lines) if l.startswith("amdhsa.kernels:")]
    if meta:
        for line in lines[meta[0] + 1:]:
            if line.startswith("  - "):
                entry = {}
                line = "    " + line[4:]
            elif not line.startswith(" "):
                break
            m = re.match(r"^    \.(\w+):\s+(\S+)\s*$", line)
            if entry is None or not m:
                continue
            entry[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                figures[m.group(2)] = entry
    kernels = {}
    for symbol, entry in figures.items():
        begin = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
        stream = []
        for line in lines[begin + 1:]:
            if line.startswith(".Lfunc_end"):
                break
            line = normalise(line)
            if line:
                stream.append(line)
        kernels[symbol] = (stream, {k: entry.get(k, "?") for k in FIGURES})
    return kernels


def demangle(symbols):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool] + symbols, capture_output=True, text=True, check=True).stdout
        names = [re.sub(r"^void ", "", n.replace("(anonymous namespace)::", "")).split("(")[0]
                 for n in out.strip().split("\n")]
        return dict(zip(symbols, names))
    except (OSError, subprocess.CalledProcessError):
        return {s: s for s in symbols}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("tree_a")
    ap.add_argument("tree_b")
    ap.add_argument("-j", type=int, default=8, help="concurrent compilations")
    ap.add_argument("--all", action="store_true", help="a line per kernel of untouched files too")
    ap.add_argument("--names", nargs=2, metavar=("A", "B"), help="what the report calls the trees")
    args = ap.parse_args()
    sides = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, tree in enumerate((args.tree_a, args.tree_b)):
            out_dir = os.path.join(tmp, "ab"[k])
            os.makedirs(out_dir)
            found = []
            for name, text in compile_tree(os.path.abspath(tree), out_dir, args.j).items():
                for symbol, (stream, figs) in split_kernels(text).items():
                    found.append((symbol, name, stream, figs))
            sides.append(found)
    # A kernel's key: its symbol, and its file too where the symbol alone does not tell.
    duplicates = {}
    for found in sides:
        files = {}
        for symbol, name, _, _ in found:
            files.setdefault(symbol, set()).add(name)
        for symbol, where in files.items():
            if len(where) > 1:
                duplicates.setdefault(symbol, set()).update(where)
    a, b = ({(symbol, name if symbol in duplicates else ""): (name, stream, figs)
             for symbol, name, stream, figs in found} for found in sides)
    symbols = sorted(set(a) | set(b), key=lambda s: ((a.get(s) or b.get(s))[0], s))
    names = demangle(sorted({s[0] for s in symbols}))
    names = {s: names[s[0]] for s in symbols}
    fmt = lambda f: " ".join(f"{k.split('_')[0]}={f[k]}" for k in FIGURES)
    def source(tree, name):
        with open(os.path.join(tree, "cartographer_amd", "csrc", name), "rb") as f:
            return f.read()
    files = {a[s][0] for s in a} & {b[s][0] for s in b}
    untouched = {f for f in files if source(args.tree_a, f) == source(args.tree_b, f)}
    quiet = {}
    bad = 0
    name_a, name_b = args.names or (args.tree_a, args.tree_b)
    print(f"# A = {name_a}\n# B = {name_b}")
    print("# figures: vgpr_count sgpr_count group_segment_fixed_size private_segment_fixed_size")
    for symbol in sorted(duplicates):
        print(f"# DUPLICATE SYMBOL {symbol} in {', '.join(sorted(duplicates[symbol]))}: "
              "matched by file and symbol")
    for s in symbols:
        if s not in a or s not in b:
            side, (name, _, figs) = ("A", a[s]) if s in a else ("B", b[s])
            print(f"ONLY IN {side}  {name}: {names[s]}  {fmt(figs)}")
            bad += 1
            continue
        (file_a, stream_a, figs_a), (file_b, stream_b, figs_b) = a[s], b[s]
        where = file_a if file_a == file_b else f"{file_a} -> {file_b}"
        same = stream_a == stream_b and figs_a == figs_b
        bad += 0 if same else 1
        if same and file_a in untouched and file_a == file_b and not args.all:
            quiet[file_a] = quiet.get(file_a, 0) + 1
            continue
        verdict = "identical" if same else (
            "DIFFERENT (%d / %d instructions)" % (len(stream_a), len(stream_b)))
        print(f"{verdict}  {where}: {names[s]}  A: {fmt(figs_a)}" +
              ("" if figs_a == figs_b else f"  B: {fmt(figs_b)}"))
    for name in sorted(quiet):
        print(f"identical  {name} (source unchanged): {quiet[name]} kernels")
    print(f"# {len(symbols)} kernels, {bad} not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
