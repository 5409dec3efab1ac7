"""Parent-against-change table of the compiler's kernel resource remarks (hipcc -Rpass-analysis=kernel-resource-usage).

Usage: python profiles/resource_table.py PARENT.remarks... -- CHANGE.remarks...
Each file is the stderr of one `hipcc <the Makefile's flags> -Rpass-analysis=kernel-resource-usage -S --cuda-device-only file.hip`.
Kernels are matched by mangled name over all files of a side (a kernel may change files); prints the table format of
profiles/live_lists/notes.md s2 and, at the end, the names only one side has and the instances whose figures differ.
Exit status 1 if the name sets differ or an instance's occupancy, scratch, spills or LDS bytes differ."""
import re
import subprocess
import sys

FIELDS = {"TotalSGPRs": "sgpr", "SGPRs": "sgpr", "VGPRs": "vgpr", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occ",
          "SGPRs Spill": "sgpr_spill", "VGPRs Spill": "vgpr_spill", "LDS Size [bytes/block]": "lds"}
MUST = ("occ", "scratch", "sgpr_spill", "vgpr_spill", "lds")


def parse(paths):
    out, cur = {}, None
    for p in paths:
        for line in open(p):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+([^:]+): (\d+)", line)
            if m and cur is not None and m.group(1) in FIELDS:
                cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(names, (re.sub(r"\(dgr::.*\)$", "(...)", s).replace("dgr::(anonymous namespace)::", "") for s in r)))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    sep = sys.argv.index("--")
    parent, change = parse(sys.argv[1:sep]), parse(sys.argv[sep + 1:])
    names = [n for n in parent if n in change]
    pretty = demangle(list(parent) + [n for n in change if n not in parent])
    fmt = lambda r: "{" + ", ".join(f"{k}: {r[k]}" for k in ("sgpr", "vgpr", "scratch", "sgpr_spill", "vgpr_spill", "occ", "lds")) + "}"
    bad, moved = [], []
    for n in names:
        print(f"   {pretty[n]}\n      parent {fmt(parent[n])}\n      change {fmt(change[n])}")
        if any(parent[n][k] != change[n][k] for k in MUST):
            bad.append(pretty[n])
        elif parent[n] != change[n]:
            moved.append(f"{pretty[n]}: vgpr {parent[n]['vgpr']} -> {change[n]['vgpr']}, sgpr {parent[n]['sgpr']} -> {change[n]['sgpr']}")
    only_p, only_c = [pretty[n] for n in parent if n not in change], [pretty[n] for n in change if n not in parent]
    print(f"\n{len(names)} kernels on both sides; only parent: {only_p or 'none'}; only change: {only_c or 'none'}")
    print("occupancy / scratch / spills / LDS differ: " + ("; ".join(bad) or "none"))
    print("register counts moved inside the occupancy step:" + ("".join("\n   " + m for m in moved) or " none"))
    sys.exit(1 if bad or only_p or only_c else 0)


if __name__ == "__main__":
    main()
