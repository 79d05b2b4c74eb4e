"""Kernel resources of csrc/oz_search.hip before and after the search kernels became one template per family (no GPU needed).

    python tools/search_variants_resources.py PARENT.txt PARENT.s THIS.txt THIS.s > profiles/search_variants_kernel_resources.txt

*.txt: stderr, *.s: the gfx950 assembly (--save-temps) of
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden --cuda-device-only -Rpass-analysis=kernel-resource-usage
          --save-temps -c othellozero_amd/csrc/oz_search.hip
on the parent commit's tree and on this one.  Every suffixed kernel of the parent is set against the instantiation that took its place; every
other kernel against itself.  Exit status 1 where a figure that must hold moved."""
import re
import sys

from proof_play_resources import demangle

FIELDS = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "TotalSGPRs", "SGPRs Spill")
TREE = {"": 0, "_n": 4, "_sel": 8, "_n_sel": 12, "_g": 16}                                   # TV_NOISE, TV_SEL, TV_GUMBEL
ADVANCE = {"": 0, "_v": 8, "_x": 12, "_xs": 28}                                               # AV_EXTRAS, AV_VALUES, AV_SURPRISE
MOVE = {"": 0, "_s": 1, "_c": 3, "_f": 15, "_g": 24, "_fs": 47, "_gs": 56, "_r": 79, "_rs": 111, "_p": 143, "_ps": 175, "_pr": 207, "_prs": 239, "_pa": 128}
READ = {"root_counts": 0, "pruned_counts": 1, "proven_counts": 2, "root_values": 4, "proven_root_values": 6, "sample_moves": 8, "proven_sample_moves": 10}
FAMILIES = [("k_wide_backup_select", TREE), ("k_wide_expand_backup", TREE), ("k_wide_select", TREE), ("k_backup_select", TREE), ("k_expand_backup", TREE),
            ("k_select", TREE), ("k_backup_advance", ADVANCE), ("k_advance", ADVANCE), ("k_sp_move", MOVE), ("k_", READ)]
PER_STEP = {f for f, table in FAMILIES if table is not MOVE and table is not READ}


def parse(path):
    """{mangled kernel: {field: value}} of the remarks (proof_play_resources.parse, for remarks that carry their source position)"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: (?:\S+: )?\s*(.+?): (\S+) \[-Rpass", line)
        if m and m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {})
        elif m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return out


def successor(sig):
    """demangled signature of a parent kernel -> (family, 'family<mask>') of this commit's kernel, or (None, None)"""
    m = re.match(r"(?:void )?(\w+?)(?:<(\d+)u?>)?\(", sig)
    name, signs = m.group(1), int(m.group(2) or 0)
    for family, table in FAMILIES:
        if name.startswith(family) and name[len(family):] in table:
            return family, "%s<%du>" % ("k_root_read" if table is READ else family, table[name[len(family):]] | signs)
    return None, None


def instructions(path):
    """{mangled kernel: instructions between its label and the end of the function}"""
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"(_Z\w+|k_\w+):", line)
        if m:
            cur = m.group(1)
            out[cur] = 0
        elif cur and re.match(r"\s+[a-z]\w+", line) and not line.lstrip().startswith("."):
            out[cur] += 1
        elif line.startswith(".Lfunc_end"):
            cur = None
    return out


def main():
    parent, this = parse(sys.argv[1]), parse(sys.argv[3])
    pins, tins = instructions(sys.argv[2]), instructions(sys.argv[4])
    names = demangle(sorted(set(parent) | set(this)))
    by_name = {re.match(r"(?:void )?([\w<>]+)\(", names[k]).group(1): k for k in this}
    print("# -Rpass-analysis=kernel-resource-usage and the instruction counts of the .s of every kernel of csrc/oz_search.hip, parent against this commit")
    print("# hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fvisibility=hidden --cuda-device-only")
    print("# kernels: parent %d, this commit %d" % (len(parent), len(this)))
    print("# figures: VGPR / AGPR / scratch B/lane / LDS B/block / occupancy waves/SIMD / SGPR / spilled SGPRs / instructions")
    bad, moved, used = [], [], set()
    for k in sorted(parent, key=lambda k: names[k]):
        family, succ = successor(names[k])
        t = by_name.get(succ) if succ else (k if k in this else None)
        old = re.match(r"(?:void )?([\w<>]+)\(", names[k]).group(1)
        if t is None:
            bad.append(old + ": no successor")
            continue
        used.add(t)
        a = [parent[k][f] for f in FIELDS] + [str(pins[k])]
        b = [this[t][f] for f in FIELDS] + [str(tins[t])]
        hard = a[:4] != b[:4] or int(b[4]) < int(a[4]) or (family in PER_STEP and a[5:] != b[5:])
        if hard:
            bad.append(old)
        elif a != b:
            moved.append(old)
        print("%-34s %-28s %s%s" % (old, succ or "(same name)", " / ".join(a), "   unchanged" if a == b else "   this: " + " / ".join(b)))
    extra = sorted(names[k] for k in this if k not in used)
    print("\n# kernels of this commit that took no parent kernel's place: %s" % (", ".join(extra) if extra else "none"))
    print("# figures that moved where they may (move family: SGPRs, spilled SGPRs, instructions; no lower occupancy): %s" % (", ".join(moved) if moved else "none"))
    print("# figures that moved where they must hold (VGPR, AGPR, scratch, LDS, lower occupancy; per-step families: all): %s" % (", ".join(bad) if bad else "none"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
