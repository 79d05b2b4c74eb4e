"""The liveness rule of the tree collection, restated (include/othellozero_amd.h, "tree collection"): under a root with D discs a stored
node stays iff it is the root or holds more than D discs."""


def popcount(x):
    return bin(x).count("1")


def tree_keep(root, node):
    """root, node = (own, opp)"""
    return node == root or popcount(node[0] | node[1]) > popcount(root[0] | root[1])


def keep_plan(root, nodes):
    """-> (keep [0 / 1], new_index [-1 where dropped, else the number of kept nodes before it], kept)"""
    keep, new_index, kept = [], [], 0
    for node in nodes:
        k = tree_keep(root, node)
        keep.append(int(k))
        new_index.append(kept if k else -1)
        kept += int(k)
    return keep, new_index, kept


def filter_dump(root, dump):
    """the nodes of a table dump (dicts with k0, k1 = own, opp) that stay under `root`, in order"""
    return [d for d in dump if tree_keep(root, (d["k0"], d["k1"]))]
