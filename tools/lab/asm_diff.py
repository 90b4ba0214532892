#!/usr/bin/env python3
"""Compare two gfx950 device assemblies kernel by kernel (a refactor's acceptance test: no GPU needed).

  hipcc <the Makefile's flags> -S --offload-device-only linear.hip -o old.s      (at the parent commit; likewise new.s)
  tools/lab/asm_diff.py old.s new.s [--map OLDSUBSTR=NEWSUBSTR ...] [-v]

Per kernel one of
  tier 1   identical instruction text (labels renumbered, __hip_cuid_ lines and comments dropped)
  tier 2   address arithmetic only: with scalar-ALU, integer address VALU (v_mov / v_add / v_lshl_add / v_mad_u64 / v_lshlrev)
           and s_nop instructions removed the mnemonic sequence is identical, registers / scratch / LDS not above the old ones
           and occupancy equal; the changed mnemonic counts are printed
  DIFFERS  anything else
--map pairs a kernel that was renamed (its symbol contains OLDSUBSTR) with the one whose symbol contains NEWSUBSTR."""
import collections
import re
import sys

META = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize")
ADDR = re.compile(r"^(s_(?!waitcnt|barrier|endpgm|cbranch|branch|load|buffer_load|setprio|sleep|sendmsg)\w+|s_nop"
                  r"|v_mov_\w+|v_add_(?:u|i|co_u|nc_u)\w*|v_addc_\w+|v_lshl_add_\w+|v_mad_u64_\w+|v_lshlrev_\w+)$")


def parse(path):
    """symbol -> (instruction lines, {meta: int})"""
    kernels, name, body, meta = {}, None, [], {}
    for line in open(path, errors="replace"):
        if "__hip_cuid_" in line:
            continue
        m = re.match(r"^(\w+):\s+; @", line)
        if m:
            name, body, meta = m.group(1), [], {}
            kernels[name] = (body, meta)
            continue
        if name is None:
            continue
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and m.group(1) in META:
            meta[m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":
                name = None
            continue
        text = line.split(";")[0].strip()
        if not text or meta or text.startswith(".") and not text.startswith((".LBB", ".Lfunc_end")):
            continue
        if text.startswith(".Lfunc_end"):
            meta["_end"] = 1                       # what follows is the kernel descriptor, not code
            continue
        body.append(re.sub(r"\.LBB\d+_", ".LBB_", text))
    return kernels


def mnemonics(body, keep_addr):
    out = [t.split()[0] for t in body if not t.startswith(".LBB")]
    return out if keep_addr else [m for m in out if not ADDR.match(m)]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("-")]
    verbose = "-v" in sys.argv
    maps = [a.split("=", 1) for i, a in enumerate(sys.argv) if sys.argv[i - 1] == "--map"]
    args = [a for a in args if "=" not in a]
    old, new = parse(args[0]), parse(args[1])
    for o, n in maps:
        for k in [k for k in new if n in k and k not in old]:
            cand = [q for q in old if o in q and q not in new]
            if cand:
                new[cand[0]] = new.pop(k)
    tiers = collections.Counter()
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            tiers["only in " + ("old" if k in old else "new")] += 1
            print(f"{'only in old' if k in old else 'only in new':8s} {k}")
            continue
        (bo, mo), (bn, mn) = old[k], new[k]
        mo.pop("_end", None), mn.pop("_end", None)
        if bo == bn and mo == mn:
            tier = "tier 1"
        elif (mnemonics(bo, False) == mnemonics(bn, False) and all(mn[m] <= mo[m] for m in META if m != "Occupancy")
              and mn["Occupancy"] == mo["Occupancy"]):
            tier = "tier 2"
        else:
            tier = "DIFFERS"
        tiers[tier] += 1
        if tier != "tier 1" or verbose:
            co, cn = collections.Counter(mnemonics(bo, True)), collections.Counter(mnemonics(bn, True))
            delta = {m: cn[m] - co[m] for m in sorted(set(co) | set(cn)) if cn[m] != co[m]}
            print(f"{tier:8s} {k}\n         counts {delta}\n         old {mo}\n         new {mn}")
    print("summary:", ", ".join(f"{v} {t}" for t, v in sorted(tiers.items())))
    return 0 if set(tiers) <= {"tier 1", "tier 2"} else 1


if __name__ == "__main__":
    sys.exit(main())
