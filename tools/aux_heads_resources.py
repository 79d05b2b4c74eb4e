"""Kernel resources of csrc/oz_replay.hip and csrc/oz_train.hip before and after the auxiliary heads, from the compiler's resource metadata (no GPU
needed).

    python tools/aux_heads_resources.py PARENT_REPLAY.txt THIS_REPLAY.txt PARENT_TRAIN.txt THIS_TRAIN.txt > profiles/aux_heads_kernel_resources.txt

Each .txt: stderr of
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -Rpass-analysis=kernel-resource-usage -c othellozero_amd/csrc/<file>.hip
on the parent commit's tree and on this one.  The trainer's kernels are keyed by their mangled names.  The two append kernels of the replay buffer
took a fourth template argument (AUX) and two more pointer arguments, so their mangled names moved: an instantiation of the parent is matched
with this commit's AUX = false instantiation of the same <N, VISITS, POLICY>; the AUX = true instantiations are the new kernels."""
import re
import sys

from proof_play_resources import demangle, figures, parse


def replay_key(sig):
    """'void k_replay_append<6, true, false>(...)' / '<6, true, false, false>(...)' -> ('k_replay_append', '6, true, false', aux)"""
    m = re.match(r"(?:void )?(\w+)<([^>]*)>", sig)
    if not m:
        return re.match(r"(?:void )?(\w+)", sig).group(1), "", False
    args = [a.strip() for a in m.group(2).split(",")]
    args += ["false"] * (3 - len(args)) if len(args) < 3 else []
    return m.group(1), ", ".join(args[:3]), len(args) > 3 and args[3] == "true"


def main():
    pr, tr, pt, tt = (parse(p) for p in sys.argv[1:5])
    print("# -Rpass-analysis=kernel-resource-usage, hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off; parent = the commit before the")
    print("# auxiliary heads, this = this commit.  Every kernel of the parent must keep its figures.")
    print("# kernel: VGPR / AGPR / SGPR / scratch B/lane / LDS B/block / occupancy waves/SIMD")
    moved = []
    names = demangle(sorted(set(pr) | set(tr)))
    this_by = {replay_key(names[k]): k for k in tr}
    print("\n## csrc/oz_replay.hip: the parent's instantiations (%d) against this commit's AUX = false ones" % len(pr))
    for k in sorted(pr, key=lambda k: names[k]):
        name, args, _ = replay_key(names[k])
        t = this_by.get((name, args, False))
        label = "%s<%s>" % (name, args)
        if t is None:
            moved.append(label + " (missing)")
            continue
        same = figures(pr[k]) == figures(tr[t])
        if not same:
            moved.append(label)
        print("%-44s %s%s" % (label, figures(pr[k]), "   unchanged" if same else "   this: " + figures(tr[t])))
    print("\n## csrc/oz_replay.hip: the new AUX = true instantiations, each under its AUX = false sibling's figures")
    for (name, args, aux), k in sorted(this_by.items()):
        if aux:
            print("%-44s %s   (AUX = false: %s)" % ("%s<%s, true>" % (name, args), figures(tr[k]), figures(tr[this_by[(name, args, False)]])))
    names = demangle(sorted(set(pt) | set(tt)))
    print("\n## csrc/oz_train.hip: kernels of the parent (%d), same mangled name" % len(pt))
    for k in sorted(pt, key=lambda k: names[k]):
        if k not in tt:
            moved.append(names[k] + " (missing)")
            continue
        same = figures(pt[k]) == figures(tt[k])
        if not same:
            moved.append(names[k])
        print("%-90s %s%s" % (names[k].split("(")[0][:90], figures(pt[k]), "   unchanged" if same else "   this: " + figures(tt[k])))
    print("\n## csrc/oz_train.hip: new kernels")
    for k in sorted((k for k in tt if k not in pt), key=lambda k: names[k]):
        print("%-90s %s" % (names[k].split("(")[0][:90], figures(tt[k])))
    print("\n# kernels of the parent whose figures moved: %s" % (", ".join(moved) if moved else "none"))
    return 1 if moved else 0


if __name__ == "__main__":
    sys.exit(main())
