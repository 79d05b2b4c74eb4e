"""Kernel resources of csrc/oz_search.hip before and after proof play, from the compiler's resource metadata (no GPU needed).

    python tools/proof_play_resources.py PARENT.txt THIS.txt > profiles/proof_play_kernel_resources.txt

PARENT.txt / THIS.txt: stderr of
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Rpass-analysis=kernel-resource-usage -c othellozero_amd/csrc/oz_search.hip
on the parent commit's tree and on this one.  Kernels are keyed by their mangled names; k_value_targets, whose argument list grew by the
exact_proven flag, is matched by its plain name."""
import re
import subprocess
import sys

FIELDS = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
SIBLINGS = {"k_sp_move_p": "k_sp_move_f", "k_sp_move_ps": "k_sp_move_fs", "k_sp_move_pr": "k_sp_move_r", "k_sp_move_prs": "k_sp_move_rs",
            "k_sp_move_pa": "k_sp_move", "k_proven_counts": "k_root_counts", "k_proven_root_values": "k_root_values", "k_proven_sample_moves": "k_sample_moves",
            "k_proof_targets": None}


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1)] = m.group(2)
    return out


def demangle(names):
    r = subprocess.run(["c++filt"] + list(names), capture_output=True, text=True, check=True)
    return dict(zip(names, r.stdout.splitlines()))


def figures(d):
    return " / ".join(d[f] for f in FIELDS)


def plain(sig):
    m = re.match(r"(?:void )?(\w+)", sig)
    return m.group(1)


def main():
    parent, this = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(parent) | set(this)))
    print("# -Rpass-analysis=kernel-resource-usage of every kernel of csrc/oz_search.hip, hipcc --offload-arch=gfx950 -O3 -ffp-contract=off")
    print("# parent = the commit before proof play; this = this commit.  Every kernel of the parent must keep its figures; k_value_targets took")
    print("# one more argument (exact_proven) and is listed on its own.  The new kernels stand against their siblings without proof play.")
    print("# kernel: VGPR / AGPR / SGPR / scratch B/lane / LDS B/block / occupancy waves/SIMD")
    moved = []
    print("\n## kernels of the parent (%d): same mangled name, parent's figures against this commit's" % len(parent))
    for k in sorted(parent, key=lambda k: names[k]):
        if plain(names[k]) == "k_value_targets":
            continue
        if k not in this:
            moved.append(names[k] + " (missing)")
            continue
        same = figures(parent[k]) == figures(this[k])
        if not same:
            moved.append(names[k])
        print("%-90s %s%s" % (names[k][:90], figures(parent[k]), "   unchanged" if same else "   this: " + figures(this[k])))
    print("\n## k_value_targets (one more int argument, one more byte read per lane)")
    for tag, d in (("parent", parent), ("this", this)):
        for k in d:
            if plain(names[k]) == "k_value_targets":
                print("    %-6s %s" % (tag, figures(d[k])))
    print("\n## new kernels, each against its sibling without proof play")
    by_plain = {plain(names[k]): k for k in this}
    for new, sib in SIBLINGS.items():
        print("%-22s %s" % (new, figures(this[by_plain[new]])))
        if sib:
            print("    %-18s %s" % (sib, figures(this[by_plain[sib]])))
    extra = sorted(plain(names[k]) for k in this if k not in parent and plain(names[k]) not in SIBLINGS and plain(names[k]) != "k_value_targets")
    print("\n# kernels of the parent whose figures moved: %s" % (", ".join(moved) if moved else "none"))
    if extra:
        print("# other new kernels: " + ", ".join(extra))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
