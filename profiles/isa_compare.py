"""Parent-against-change comparison of gfx950 assembly listings (hipcc <the Makefile's flags> -S --cuda-device-only file.hip),
kernel by kernel -- so that a refactor can show, without a GPU, that it moved no instruction.

Kernels are matched by mangled name over all listings of a side (a kernel may change files); a kernel left without a partner
because a parameter's type was renamed is matched by its unqualified name, where that is unambiguous.  A kernel's text is normalised
before it is compared: comments and blank lines dropped, whitespace collapsed, the function number of local labels removed
(.LBB<n>_<m> -> .LBB_<m>: the number counts the functions in front of it in the file).  Per kernel one line, SAME or DIFF; for
a DIFF both instruction counts and the opcodes whose counts differ.

Usage: python profiles/isa_compare.py PARENT CHANGE      two listings, or two directories of *.s listings
Exit status 1 if a kernel differs or the two sides do not hold the same kernels."""
import collections
import glob
import os
import re
import sys


def kernels(path):
    """{mangled name: [normalised lines]} of every function of the listing(s) at `path`"""
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]:
        name, body = None, []
        for l in open(f):
            m = re.match(r"^(_Z\w+):", l)
            if m:
                name, body = m.group(1), []
            elif name is not None and l.strip().startswith(".Lfunc_end"):  # (a data symbol has none: it is dropped)
                out[name], name = body, None
            elif name is not None:
                l = " ".join(l.split(";")[0].split())
                if l:
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", l))
    return out


def unqualified(mangled):
    """seed_apply_kernel of _ZN3dgr12_GLOBAL__N_117seed_apply_kernelE...: the last component of the nested name"""
    m, last = re.match(r"_ZN?", mangled), None
    pos = m.end()
    while (m := re.compile(r"\d+").match(mangled, pos)):
        last = mangled[m.end():m.end() + int(m.group())]
        pos = m.end() + int(m.group())
    return last


def pair_renamed(parent, change):
    """re-keys the kernels of `change` that have no partner to the parent's name of the same unqualified kernel"""
    orphans = lambda a, b: collections.Counter(unqualified(n) for n in a if n not in b)  # noqa: E731
    op, oc = orphans(parent, change), orphans(change, parent)
    names = {unqualified(n): n for n in parent if n not in change}
    for n in [n for n in change if n not in parent]:
        u = unqualified(n)
        if u is not None and op[u] == 1 and oc[u] == 1:
            print(f"(parameter types renamed: {u} matched by name)")
            change[names[u]] = [l.replace(n, names[u]) for l in change.pop(n)]  # (its own name in its directives)


def opcodes(lines):
    return collections.Counter(l.split()[0] for l in lines if not l.startswith(".") and not l.endswith(":"))


def main():
    parent, change = kernels(sys.argv[1]), kernels(sys.argv[2])
    pair_renamed(parent, change)
    same = 0
    for n in parent:
        if n not in change:
            continue
        if parent[n] == change[n]:
            same += 1
            print(f"SAME  {n}  ({sum(opcodes(parent[n]).values())} instructions)")
            continue
        hp, hc = opcodes(parent[n]), opcodes(change[n])
        print(f"DIFF  {n}  ({sum(hp.values())} -> {sum(hc.values())} instructions)")
        delta = [f"{op} {hp[op]} -> {hc[op]}" for op in sorted(set(hp) | set(hc)) if hp[op] != hc[op]]
        print("      " + ("; ".join(delta) if delta else "same opcode histogram: order or operands only"))
    only_p, only_c = [n for n in parent if n not in change], [n for n in change if n not in parent]
    both = len(parent) - len(only_p)
    print(f"\n{both} kernels on both sides, {same} SAME, {both - same} DIFF; only parent: {only_p or 'none'}; only change: {only_c or 'none'}")
    sys.exit(1 if same != both or only_p or only_c else 0)


if __name__ == "__main__":
    main()
