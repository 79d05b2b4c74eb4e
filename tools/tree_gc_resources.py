"""Kernel resources of csrc/oz_search.hip before and after the tree collection, from the compiler's resource metadata (no GPU needed).

    python tools/tree_gc_resources.py PARENT.txt THIS.txt > profiles/tree_gc_kernel_resources.txt

PARENT.txt / THIS.txt: stderr of
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Rpass-analysis=kernel-resource-usage -c othellozero_amd/csrc/oz_search.hip
on the parent commit's tree and on this one.  Kernels are keyed by their mangled names; the one new kernel is k_tree_collect."""
import sys

from proof_play_resources import demangle, figures, parse


def main():
    parent, this = parse(sys.argv[1]), parse(sys.argv[2])
    names = demangle(sorted(set(parent) | set(this)))
    print("# -Rpass-analysis=kernel-resource-usage of every kernel of csrc/oz_search.hip, hipcc --offload-arch=gfx950 -O3 -ffp-contract=off")
    print("# parent = the commit before the tree collection; this = this commit.  Every kernel of the parent must keep its figures.")
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
    print("\n## new kernels")
    for k in sorted((k for k in this if k not in parent), key=lambda k: names[k]):
        print("%-90s %s" % (names[k][:90], figures(this[k])))
    print("\n# kernels of the parent whose figures moved: %s" % (", ".join(moved) if moved else "none"))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
