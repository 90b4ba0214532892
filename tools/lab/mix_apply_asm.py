#!/usr/bin/env python3
"""Lab: what the compiler made of the MixedOp epilogue kernels (no GPU needed).

Compiles mr-gnas_amd/csrc/mixedop.hip to gfx950 device assembly (or reads an assembly file that was made before) and prints, per
instance of mix_bwd_apply_k / mix_bwd_apply_any_k, mix_fwd_k and mix_bwd_reduce_k:
  from the kernel descriptor: spilled SGPRs, allocated VGPRs, scratch bytes, static LDS bytes;
  from the ROW LOOP (the outermost loop of the kernel with the most instructions; loops nested in it count with it): the number of
  vector (v_), scalar (s_), LDS (ds_) and memory (global_ / buffer_ / flat_ / scratch_) instructions, by mnemonic prefix.

usage: python tools/lab/mix_apply_asm.py [--asm FILE.s] [--tag TEXT] [--all]      (--all: every kernel of the file)
The committed record of the by-index kernels and of the role kernels is profiles/mix_apply_asm.txt."""
import argparse
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
KERNELS = ("mix_bwd_apply_k", "mix_bwd_apply_any_k", "mix_fwd_k", "mix_bwd_reduce_k")
CLASSES = (("vector", ("v_",)), ("scalar", ("s_",)), ("lds", ("ds_",)), ("memory", ("global_", "buffer_", "flat_", "scratch_")))


def compile_asm(out):
    src = os.path.join(ROOT, "mr-gnas_amd", "csrc", "mixedop.hip")
    t0 = time.time()
    subprocess.run(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S", src, "-o", out], check=True)
    return time.time() - t0


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    """void mrg::mix_fwd_k<4, 64, 1, true, 5, 0>(float const*, ...) -> mix_fwd_k<4, 64, 1, true, 5, 0>"""
    m = re.search(r"mrg::(\w+<[^>]*>)", name)
    return m.group(1) if m else name


def descriptors(text):
    """{kernel symbol: {field: value}} from the amdhsa.kernels metadata (one record per kernel, its fields at one indent)."""
    out, cur = {}, {}
    for line in text.splitlines():
        m = re.match(r"  (- | {2})\.(\w+):\s+(\S+)\s*$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            cur = {}
        cur[m.group(2)] = m.group(3)
        if m.group(2) == "name":
            out[m.group(3)] = cur
    return out


def row_loop_counts(body):
    """Instruction classes of the biggest outermost loop of one kernel's assembly lines."""
    blocks, label, notes = [], None, ""
    cur = []
    for line in body:
        m = re.match(r"(\.LBB\d+_\d+):(.*)", line)
        if m:
            blocks.append((label, notes, cur))
            label, notes, cur = m.group(1)[2:], m.group(2), []
            continue
        if re.match(r"\s+;", line) and not cur:
            notes += line
            continue
        m = re.match(r"\s+([a-z][a-z0-9_]+)", line)
        if m:
            cur.append(m.group(1))
    blocks.append((label, notes, cur))
    parent = {}
    for label, notes, _ in blocks:                          # headers of nested loops name their outermost loop
        if label and "Loop Header" in notes:
            m = re.search(r"Parent Loop (BB\d+_\d+) Depth=1\b", notes)
            parent[label] = m.group(1) if m else label
    per = collections.defaultdict(collections.Counter)
    for label, notes, ins in blocks:
        top = None
        if label in parent:
            top = parent[label]
        else:
            m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", notes)
            if m:
                top = parent.get(m.group(1), m.group(1))
        if top is None:
            continue
        for i in ins:
            for cls, prefixes in CLASSES:
                if i.startswith(prefixes):
                    per[top][cls] += 1
    if not per:
        return collections.Counter()
    return max(per.values(), key=lambda c: sum(c.values()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm", default=None)
    ap.add_argument("--tag", default="")
    ap.add_argument("--all", action="store_true")
    args = ap.parse_args()
    secs = None
    path = args.asm
    if path is None:
        path = os.path.join(tempfile.mkdtemp(prefix="mix_apply_asm_"), "mixedop.s")
        secs = compile_asm(path)
    text = open(path).read()
    desc = descriptors(text)
    lines = text.splitlines()
    starts = [(i, m.group(1)) for i, l in enumerate(lines) for m in [re.match(r"(_Z\w+):\s*;\s*@", l)] if m]
    names = demangle([s for _, s in starts])
    print(f"# {args.tag or path}" + (f"   (device assembly compiled in {secs:.0f} s)" if secs is not None else ""))
    print(f"{'kernel':58s} {'sgpr_spill':>10s} {'vgpr':>5s} {'scratch':>8s} {'lds':>6s} | row loop: {'vector':>6s} {'scalar':>6s} {'lds':>4s} {'memory':>6s}")
    rows = []
    for n, (i, sym) in enumerate(starts):
        name = short(names[sym])
        if not args.all and not name.startswith(tuple(k + "<" for k in KERNELS)):
            continue
        end = starts[n + 1][0] if n + 1 < len(starts) else len(lines)
        body = lines[i:end]
        for j, l in enumerate(body):
            if l.strip().startswith(".section") or l.strip().startswith(".amdhsa_kernel"):
                body = body[:j]
                break
        d = desc.get(sym, {})
        c = row_loop_counts(body)
        rows.append((name, d, c))
    rows.sort(key=lambda r: r[0])
    for name, d, c in rows:
        print(f"{name:58s} {d.get('sgpr_spill_count', '?'):>10s} {d.get('vgpr_count', '?'):>5s} {d.get('private_segment_fixed_size', '?'):>8s} "
              f"{d.get('group_segment_fixed_size', '?'):>6s} | {'':9s} {c['vector']:6d} {c['scalar']:6d} {c['lds']:4d} {c['memory']:6d}")
    apply_rows = [r for r in rows if r[0].startswith("mix_bwd_apply")]
    spills = [int(r[1].get("sgpr_spill_count", 0)) for r in apply_rows]
    scratch = [int(r[1].get("private_segment_fixed_size", 0)) for r in apply_rows]
    if apply_rows:
        print(f"# backward apply: {len(apply_rows)} instances, spilled SGPRs {min(spills)} .. {max(spills)}, scratch bytes {min(scratch)} .. {max(scratch)}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
