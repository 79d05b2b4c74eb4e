"""Kernel resources of csrc/oz_search.hip before and after the selection option, from the compiler's resource metadata (no GPU needed).

    python tools/selection_resources.py PARENT.txt THIS.txt > profiles/selection_kernel_resources.txt

PARENT.txt / THIS.txt: stderr of
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Rpass-analysis=kernel-resource-usage -c othellozero_amd/csrc/oz_search.hip
on the parent commit's tree and on this one.  Kernels are keyed by their mangled names; every new kernel is a *_sel instantiation and stands
against its sibling of the same value signs."""
import re
import sys

from proof_play_resources import demangle, figures, parse


def main():
    parent, this = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(parent) | set(this)))
    print("# -Rpass-analysis=kernel-resource-usage of every kernel of csrc/oz_search.hip, hipcc --offload-arch=gfx950 -O3 -ffp-contract=off")
    print("# parent = the commit before the selection option; this = this commit.  Every kernel of the parent must keep its figures.")
    print("# The new kernels (the *_sel instantiations) stand against their siblings without the option.")
    print("# kernel: VGPR / AGPR / SGPR / scratch B/lane / LDS B/block / occupancy waves/SIMD")
    moved = []
    print("\n## kernels of the parent (%d): same mangled name, parent's figures against this commit's" % len(parent))
    for k in sorted(parent, key=lambda k: names[k]):
        if k not in this:
            moved.append(names[k] + " (missing)")
            continue
        same = figures(parent[k]) == figures(this[k])
        if not same:
            moved.append(names[k])
        print("%-90s %s%s" % (names[k][:90], figures(parent[k]), "   unchanged" if same else "   this: " + figures(this[k])))
    print("\n## new kernels, each against its sibling without the option (<0> reference, <1> sound, <2> proven signs)")
    by_name = {names[k]: k for k in this}
    other = []
    for k in sorted((k for k in this if k not in parent), key=lambda k: names[k]):
        sib = by_name.get(re.sub(r"_sel<", "<", names[k]))
        if "_sel<" not in names[k] or sib is None:
            other.append(names[k])
            continue
        print("%-60s %s" % (names[k][:60], figures(this[k])))
        print("    %-56s %s" % (names[sib][:56], figures(this[sib])))
    print("\n# kernels of the parent whose figures moved: %s" % (", ".join(moved) if moved else "none"))
    if other:
        print("# other new kernels: " + ", ".join(other))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
