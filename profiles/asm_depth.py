"""Instruction counts of a kernel by loop depth, from a gfx950 assembly listing (hipcc -S --cuda-device-only), and the kernel's
register / spill figures from the listing's metadata -- so that a parent and a change can be compared without a GPU.

A blend kernel's cost follows its vector instruction COUNT wherever the instructions stand (profiles/r9/bwd_account.txt), so the
work outside the pair loop matters as much as the loop: this prints it.  The compiler marks every basic block with the loop it
belongs to and that loop's depth; the listing is cut, in order, into
   straight   blocks outside every loop (between two loop nests these are usually one body's prologue or epilogue)
   loop N     a depth-1 loop (a blend kernel's batch loop): its own blocks, and each loop nested inside it on its own line
and every line gives vector / scalar / LDS / memory instruction counts.  v_readlane / v_writelane (scalar-register spills live
in VGPR lanes) and v_mov are also shown on their own.  The pair loop of a body is the child loop that holds `ds_write_b8` (forward)
or `v_permlane32_swap` (backward): it is marked with `<- pair loop`.

Usage: python profiles/asm_depth.py file.s <substring of the kernel's mangled name> [--brief]
       python profiles/asm_depth.py file.s --all <substring>     one summary line per matching kernel"""
import collections
import re
import sys

PAIR_MARKERS = ("ds_write_b8", "v_permlane32_swap")


def kernels(lines):
    """[(name, first line, line of s_endpgm)] of every kernel of the listing"""
    out = []
    for i, l in enumerate(lines):
        m = re.match(r"^(_Z\w+):", l)
        if m:
            end = next((j for j in range(i, len(lines)) if lines[j].strip().startswith(".Lfunc_end")), None)
            if end is not None:  # (a data symbol behind the last function has none)
                out.append((m.group(1), i, end))
    return out


def metadata(lines, name):
    """the kernel's entry of the amdhsa metadata: {key: value}"""
    meta = {}
    idx = next((i for i, l in enumerate(lines) if l.strip() == ".name:           " + name or l.strip() == ".name: " + name
                or re.match(r"^\s*\.name:\s+" + re.escape(name) + r"\s*$", l)), None)
    if idx is None:
        return meta
    # an entry runs from its "- .args:" (or "- .") line to the next one
    lo = idx
    while lo > 0 and not lines[lo].lstrip().startswith("- ."):
        lo -= 1
    hi = idx + 1
    while hi < len(lines) and not lines[hi].lstrip().startswith("- .") and not lines[hi].startswith("amdhsa."):
        hi += 1
    for l in lines[lo:hi]:
        m = re.match(r"^\s*-?\s*\.(\w+):\s+(\S+)\s*$", l)
        if m and m.group(1) in ("sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "private_segment_fixed_size",
                                "group_segment_fixed_size"):
            meta[m.group(1)] = int(m.group(2))
    return meta


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    return "mem"


class Region:
    def __init__(self, title):
        self.title = title
        self.n = collections.Counter()
        self.pair = False

    def add(self, line):
        op = line.split(";")[0].split()[0]
        self.n[classify(op)] += 1
        if op.startswith(("v_readlane", "v_writelane")):
            self.n["lane"] += 1
        if op.startswith(("v_mov_b32", "v_mov_b64", "v_accvgpr")):
            self.n["mov"] += 1
        if op.startswith("s_load") or op.startswith("s_buffer_load"):
            self.n["sload"] += 1
        if any(m in line for m in PAIR_MARKERS):
            self.pair = True

    def row(self):
        n = self.n
        return (f"{self.title:34s} valu {n['valu']:4d}  (v_mov {n['mov']:3d}, lane r/w {n['lane']:3d})   salu {n['salu']:4d} (s_load {n['sload']:2d})"
                f"   lds {n['lds']:3d}   mem {n['mem']:3d}" + ("   <- pair loop" if self.pair else ""))


def by_depth(lines, start, end):
    """the kernel's regions in listing order"""
    body = lines[start + 1:end]
    # pass 1: every loop header's parent (the comment block of a header names them) and depth
    parent, depth_of = {}, {}
    i = 0
    blocks = []  # (first instruction line index, label, comment text)
    while i < len(body):
        l = body[i]
        m = re.match(r"^(?:\.L(BB\d+_\d+)|; %bb\.\d+):(.*)", l)
        if m:
            label, comment = m.group(1), m.group(2)
            j = i + 1
            while j < len(body) and re.match(r"^\s+;", body[j]) and "implicit-def" not in body[j]:
                comment += " " + body[j].strip()
                j += 1
            blocks.append((i, label, comment))
            if label and "Loop Header" in comment:
                d = int(re.search(r"Loop Header: Depth=(\d+)", comment).group(1))
                depth_of[label] = d
                ps = re.findall(r"Parent Loop (BB\d+_\d+) Depth=(\d+)", comment)
                if ps:
                    parent[label] = max(ps, key=lambda p: int(p[1]))[0]
            i = j
        else:
            i += 1

    def chain(h):  # [depth-1 ancestor, ..., h]
        c = [h]
        while c[0] in parent:
            c.insert(0, parent[c[0]])
        return c

    regions, index = [], {}

    def region(key, title):
        if key not in index:
            index[key] = Region(title)
            regions.append(index[key])
        return index[key]

    nstraight = 0
    cur = region(("straight", 0), "straight 0")
    last_was_loop = False
    bi = 0
    for i, l in enumerate(body):
        while bi < len(blocks) and blocks[bi][0] == i:
            _, label, comment = blocks[bi]
            bi += 1
            hdr = None
            if label and "Loop Header" in comment:
                hdr = label
            else:
                m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", comment)
                if m:
                    hdr = m.group(1)
            if hdr is None:
                if last_was_loop:
                    nstraight += 1
                cur = region(("straight", nstraight), f"straight {nstraight}")
                last_was_loop = False
            else:
                c = chain(hdr)
                d = len(c)
                title = ("  " * (d - 1)) + f"loop {c[-1]} depth {d}" + (f" (in {c[0]})" if d > 1 else "")
                # a nested loop is listed behind its depth-1 loop: make sure that one exists first
                region(tuple(c[:1]), f"loop {c[0]} depth 1")
                cur = region(tuple(c), title)
                last_was_loop = True
        if l.startswith("\t") and not l.strip().startswith((".", ";")) and l.split(";")[0].strip():
            cur.add(l)
    return regions


def main():
    path = sys.argv[1]
    lines = open(path).read().splitlines()
    if sys.argv[2] == "--all":
        key = sys.argv[3] if len(sys.argv) > 3 else ""
        for name, s, e in kernels(lines):
            if key not in name:
                continue
            regs = by_depth(lines, s, e)
            md = metadata(lines, name)
            out_v = sum(r.n["valu"] for r in regs if not r.pair)
            pair = [r.n["valu"] for r in regs if r.pair]
            print(f"{name}\n    vgpr {md.get('vgpr_count')} sgpr {md.get('sgpr_count')} sgpr_spill {md.get('sgpr_spill_count')} vgpr_spill {md.get('vgpr_spill_count')}"
                  f" scratch {md.get('private_segment_fixed_size')} lds {md.get('group_segment_fixed_size')}"
                  f" | valu outside pair loops {out_v}, pair loops {pair}, lane r/w {sum(r.n['lane'] for r in regs)}, v_mov outside {sum(r.n['mov'] for r in regs if not r.pair)}")
        return
    key = sys.argv[2]
    brief = "--brief" in sys.argv
    for name, s, e in kernels(lines):
        if key not in name:
            continue
        md = metadata(lines, name)
        print(name)
        print("  " + ", ".join(f"{k} {v}" for k, v in md.items()))
        regs = by_depth(lines, s, e)
        for r in regs:
            if brief and sum(r.n.values()) == 0:
                continue
            print("  " + r.row())
        tot = Region("total (static)")
        for r in regs:
            tot.n.update(r.n)
        print("  " + tot.row())


if __name__ == "__main__":
    main()
