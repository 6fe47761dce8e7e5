"""Sequential restatement of the reference's trees and fragment distances:
FragmentDistance::fragment_distance (FragmentDistance.cpp:31-69), GlobalTree's
add_dist and run_impl (GlobalTree.cpp:68-116), is_diagnostic / add_diagnostic
(block_stat.cpp:236-253, ConsensusTree.cpp:294-367), TreeNode's
neighbor_joining, upgma, clone_with_pseudo_leafs and print_newick
(tree.cpp:65-82, 188-258, 285-480), PrintTree::make_tree (PrintTree.cpp:51-67)
and the texts the three processors write.

The reference orders node pairs by address; here nodes are numbered in
creation order (the leaves as added, then each internal node as made),
make_pair(a, b) is (lower number, higher number), and find_min_pair keeps the
first minimum of its (i, j) loop over the current node list (survivors keep
their order, the new node is appended).  The root has no number: parent -1.

Blocks are lists of fragments (seq_index, min, max, ori, row) as
BlockSetEngine.blocks() gives them.  The arithmetic keeps the reference's
order of operations; numpy only evaluates the same float64 operations for many
(i, j) at once (calculate_q) and the column scans for many columns at once
(penalties, diagnostic columns) -- the plain loops fragment_distance and
is_diagnostic are kept beside them and the tests hold them equal.
"""
import numpy as np

NO_BOOTSTRAP, BOOTSTRAP_IN_BRACES, BOOTSTRAP_BEFORE_LENGTH = 0, 1, 2
BOOTSTRAP_PRINT = {"no": NO_BOOTSTRAP, "in-braces": BOOTSTRAP_IN_BRACES, "before-length": BOOTSTRAP_BEFORE_LENGTH}


# ------------------------------------------------------------------ distances
def fragment_distance(a, b):
    """The penalty of two gapped rows: columns c in [1, L - 2] that differ
    while c - 1 and c + 1 are equal and no gap ('-' against '-' is equal)."""
    assert len(a) == len(b)
    penalty = 0
    for c in range(1, len(a) - 1):
        prev_good = a[c - 1] == b[c - 1] and a[c - 1] != "-"
        curr_good = a[c] != b[c]
        next_good = a[c + 1] == b[c + 1] and a[c + 1] != "-"
        if prev_good and curr_good and next_good:
            penalty += 1
    return penalty


def _codes(rows):
    return np.frombuffer("".join(rows).encode(), dtype=np.uint8).reshape(len(rows), len(rows[0]) if rows else 0)


def block_penalties(rows):
    """fragment_distance of every pair (i asc, j asc) of a block's rows."""
    n = len(rows)
    if n < 2:
        return []
    A = _codes(rows)
    L = A.shape[1]
    out = []
    for i in range(n - 1):
        if L < 3:
            out.extend([0] * (n - 1 - i))
            continue
        eq = A[i + 1:] == A[i][None, :]
        good = eq & (A[i][None, :] != 45)
        pen = (good[:, :-2] & ~eq[:, 1:-1] & good[:, 2:]).sum(axis=1)
        out.extend(int(x) for x in pen)
    return out


def pair_distances(blocks):
    """Per block in set order: the penalties of its pairs.  A block of two or
    more fragments without rows raises ValueError (the reference throws
    "Fragment without alignment")."""
    out = []
    for b in blocks:
        if len(b) >= 2 and any(f[4] is None for f in b):
            raise ValueError("Fragment without alignment")
        out.append(block_penalties([f[4] for f in b]) if len(b) >= 2 else [])
    return out


def block_length(b):
    """Block::alignment_length."""
    if not b:
        return 0
    return len(b[0][4]) if b[0][4] is not None else b[0][2] - b[0][1] + 1


def genome_of(name):
    """Sequence::genome (Sequence.cpp:193-202)."""
    parts = name.split("&")
    return parts[0] if len(parts) == 3 and parts[2] in ("c", "l") else ""


def genomes_list(names):
    """genomes_list (block_stat.cpp:255-263): sorted, each once."""
    return sorted({genome_of(n) for n in names})


def stem_blocks(blocks, names):
    """The blocks RemoveNonStem --exact keeps (RemoveNonStem.cpp:29-58)."""
    genomes = genomes_list(names)
    keep = []
    for b in blocks:
        gs = [genome_of(names[f[0]]) for f in b]
        if len(gs) == len(genomes) and sorted(gs) == genomes:
            keep.append(b)
    return keep


def genome_matrix(blocks, names):
    """add_dist over the stem blocks: G x G mutation counts, genomes in
    genomes_list order."""
    genomes = genomes_list(names)
    at = {g: i for i, g in enumerate(genomes)}
    G = len(genomes)
    m = [[0] * G for _ in range(G)]
    for b in stem_blocks(blocks, names):
        pen = iter(pair_distances([b])[0])
        gi = [at[genome_of(names[f[0]])] for f in b]
        for i in range(len(b)):
            for j in range(i + 1, len(b)):
                p = next(pen)
                m[gi[i]][gi[j]] += p
                m[gi[j]][gi[i]] += p
    return m


def is_diagnostic(col, clade, other):
    """is_diagnostic (block_stat.cpp:236-253) on two non-empty lists of rows."""
    first = clade[0][col]
    for r in clade:
        if r[col] != first:
            return False
    for r in other:
        if r[col] == first:
            return False
    return True


def diagnostic_columns(rows, clade_idx):
    """The number of diagnostic columns of the clade rows[i], i in clade_idx,
    against the other rows; 0 when either side is empty (the reference skips
    the pair)."""
    inside = sorted(set(clade_idx))
    outside = [i for i in range(len(rows)) if i not in set(inside)]
    if not inside or not outside or not rows[0]:
        return 0
    A = _codes(rows)
    first = A[inside[0]][None, :]
    ok = (A[inside] == first).all(axis=0) & (A[outside] != first).all(axis=0)
    return int(ok.sum())


# ------------------------------------------------------------------ trees
class Node:
    def __init__(self, leaf=-1):
        self.parent = -1      # -1: the root
        self.leaf = leaf      # leaf index; -2 - index: its pseudo leaf; -1: internal
        self.length = 0.0
        self.bootstrap = 0.0
        self.children = []


class Tree:
    def __init__(self, n=0):
        self.nodes = [Node(i) for i in range(n)]
        self.top = list(range(n))
        self.root_bootstrap = 0.0


def _distances(n, d):
    D = np.zeros((2 * n + 1, 2 * n + 1), dtype=np.float64)
    for i in range(n):
        for j in range(i + 1, n):
            D[i, j] = D[j, i] = d[i][j]
    return D


def _find_min_pair(M, nodes, ties):
    """The first minimum of M over nodes[i], nodes[j], i < j, in loop order."""
    N = len(nodes)
    sub = M[np.ix_(nodes, nodes)]
    iu = np.triu_indices(N, 1)
    vals = sub[iu]
    p = int(np.argmin(vals))
    if ties is not None:
        ties.append(int((vals == vals[p]).sum()) > 1)
    return nodes[int(iu[0][p])], nodes[int(iu[1][p])]


def _join(t, a, b):
    k = len(t.nodes)
    nd = Node()
    nd.children = [a, b]
    t.nodes.append(nd)
    t.nodes[a].parent = k
    t.nodes[b].parent = k
    return k


def upgma(t, d, ties=None):
    """TreeNode::upgma (tree.cpp:311-358)."""
    n = len(t.nodes)
    assert n >= 1
    D = _distances(n, d)
    nodes = list(t.top)
    for _ in range(n - 1):
        a, b = _find_min_pair(D, nodes, ties)
        md = float(D[a, b])
        k = _join(t, a, b)
        t.nodes[a].length = md / 2.0
        t.nodes[b].length = md / 2.0
        for x in nodes:
            if x != a and x != b:
                D[x, k] = D[k, x] = 0.5 * float(D[x, a]) + 0.5 * float(D[x, b])
        nodes = [x for x in nodes if x != a and x != b] + [k]
    t.top = nodes


def _distance_to_first(a, b, D, nodes):
    md = float(D[a, b])
    s = 0.0
    for k in nodes:
        if k != a and k != b:
            s += float(D[a, k])
            s -= float(D[b, k])
    if len(nodes) > 2:
        dist = 0.5 * md + 0.5 * s / float(len(nodes) - 2)
    else:
        dist = 0.5 * md
    if dist < 0.0:
        dist = 0.0
    if dist > md:
        dist = md
    return dist


def _distance_to_pair(a, b, D, k):
    return 0.5 * (float(D[a, k]) + float(D[b, k]) - float(D[a, b]))


def neighbor_joining(t, d, ties=None):
    """TreeNode::neighbor_joining (tree.cpp:360-480)."""
    n = len(t.nodes)
    D = _distances(n, d)
    nodes = list(t.top)
    if n <= 1:
        return
    if n == 2:
        t.nodes[nodes[0]].length = float(D[nodes[0], nodes[1]]) / 2.0
        t.nodes[nodes[1]].length = float(D[nodes[0], nodes[1]]) / 2.0
        return
    for _ in range(n - 3):
        N = len(nodes)
        sub = D[np.ix_(nodes, nodes)]
        q = (N - 2.0) * sub
        for k in range(N):  # calculate_q: -= d(i, k), -= d(j, k) for every k, in this order
            q = q - sub[:, k][:, None]
            q = q - sub[k, :][None, :]
        Q = np.zeros_like(D)
        Q[np.ix_(nodes, nodes)] = q
        a, b = _find_min_pair(Q, nodes, ties)
        k = _join(t, a, b)
        md = float(D[a, b])
        left = _distance_to_first(a, b, D, nodes)
        t.nodes[a].length = left
        t.nodes[b].length = md - left
        for x in nodes:
            if x != a and x != b:
                D[k, x] = D[x, k] = _distance_to_pair(a, b, D, x)
        nodes = [x for x in nodes if x != a and x != b] + [k]
    a, b = nodes[0], nodes[1]
    l0 = _distance_to_first(a, b, D, nodes)
    l1 = float(D[a, b]) - l0
    l2 = _distance_to_pair(a, b, D, nodes[2])
    t.nodes[a].length = l0
    t.nodes[b].length = l1
    t.nodes[nodes[2]].length = l2
    t.top = nodes


def clone_with_pseudo_leafs(t):
    """TreeNode::clone_with_pseudo_leafs (tree.cpp:65-82)."""
    out = Tree()
    out.root_bootstrap = t.root_bootstrap

    def clone(k, parent):
        src = t.nodes[k]
        me = len(out.nodes)
        nd = Node()
        nd.parent, nd.length, nd.bootstrap = parent, src.length, src.bootstrap
        out.nodes.append(nd)
        if src.leaf >= 0:
            for v in (src.leaf, -2 - src.leaf):
                c = Node(v)
                c.parent = me
                nd.children.append(len(out.nodes))
                out.nodes.append(c)
        else:
            for c in src.children:
                nd.children.append(clone(c, me))
        return me

    out.top = [clone(c, -1) for c in t.top]
    return out


def descendants(t):
    """all_descendants of the root: parents before children."""
    out = []

    def go(k):
        out.append(k)
        for c in t.nodes[k].children:
            go(c)

    for c in t.top:
        go(c)
    return out


def leaves_under(t, k):
    out = []

    def go(x):
        if t.nodes[x].leaf >= 0:
            out.append(t.nodes[x].leaf)
        for c in t.nodes[x].children:
            go(c)

    go(k)
    return out


def table(t):
    """The tree in print order: (parent entry, leaf, length, bootstrap), the
    root first."""
    order = descendants(t)
    entry = {k: i + 1 for i, k in enumerate(order)}
    out = [(-1, -1, 0.0, t.root_bootstrap)]
    for k in order:
        nd = t.nodes[k]
        out.append((0 if nd.parent < 0 else entry[nd.parent], nd.leaf, nd.length, nd.bootstrap))
    return out


def fmt(x):
    """ostream << double at the default precision."""
    return "%g" % x


def newick(t, names, lengthes=True, sbs=NO_BOOTSTRAP):
    """TreeNode::newick (tree.cpp:188-258)."""
    o = []

    def go(k, depth):
        root = k < 0
        leaf = -1 if root else t.nodes[k].leaf
        length = 0.0 if root else t.nodes[k].length
        bootstrap = t.root_bootstrap if root else t.nodes[k].bootstrap
        if leaf != -1:
            o.append(names[leaf] if leaf >= 0 else "." + names[-2 - leaf])
            if lengthes:
                o.append(":" + fmt(length))
        else:
            indent = " " * (2 * depth)
            o.append("(")
            first = True
            for c in (t.top if root else t.nodes[k].children):
                if not first:
                    o.append(",")
                first = False
                o.append("\n" + indent + "  ")
                go(c, depth + 1)
            o.append("\n" + indent + ")")
            if lengthes and not root:
                if sbs == BOOTSTRAP_BEFORE_LENGTH:
                    o.append(fmt(bootstrap))
                o.append(":" + fmt(length))
        if sbs == BOOTSTRAP_IN_BRACES:
            o.append("[" + fmt(bootstrap) + "]")

    go(-1, 0)
    return "".join(o) + ";"


def tree_distance(t, a, b):
    """TreeNode::tree_distance_to between the nodes a and b (tree.cpp:164-186)."""
    up = {}
    k, dist = a, 0.0
    while k >= 0:
        up[k] = dist
        dist += t.nodes[k].length
        k = t.nodes[k].parent
    root_a = dist
    k, dist = b, 0.0
    while k >= 0:
        if k in up:
            return up[k] + dist
        dist += t.nodes[k].length
        k = t.nodes[k].parent
    return root_a + dist


# ------------------------------------------------------------------ processors
def clade_counts(t, blocks, names):
    """add_diagnostic with min_block = G over the stem blocks: per node of
    descendants(t) the total of its clade's diagnostic columns."""
    genomes = genomes_list(names)
    at = {g: i for i, g in enumerate(genomes)}
    order = descendants(t)
    clades = [set(leaves_under(t, k)) for k in order]
    totals = [0] * len(order)
    for b in stem_blocks(blocks, names):
        if len(b) < 2:
            continue
        rows = [f[4] for f in b]
        gi = [at[genome_of(names[f[0]])] for f in b]
        for x, clade in enumerate(clades):
            totals[x] += diagnostic_columns(rows, [i for i in range(len(b)) if gi[i] in clade])
    return order, totals


def global_tree_build(blocks, names):
    """GlobalTree::run_impl up to add_diagnostic: (matrix, tree, genomes)."""
    genomes = genomes_list(names)
    m = genome_matrix(blocks, names)
    t = Tree(len(genomes))
    neighbor_joining(t, [[float(x) for x in row] for row in m])
    order, totals = clade_counts(t, blocks, names)
    for k, v in zip(order, totals):
        t.nodes[k].bootstrap = float(v)
    return m, t, genomes


def global_tree_render(t, genomes, bootstrap_print="before-length", pseudo_leafs=False):
    """... and its end: (node table, the file's text)."""
    if pseudo_leafs:
        t = clone_with_pseudo_leafs(t)
    return table(t), newick(t, genomes, True, BOOTSTRAP_PRINT[bootstrap_print]) + "\n"


def global_tree(blocks, names, bootstrap_print="before-length", pseudo_leafs=False):
    """GlobalTree::run_impl: (matrix, node table, text)."""
    m, t, genomes = global_tree_build(blocks, names)
    return (m,) + global_tree_render(t, genomes, bootstrap_print, pseudo_leafs)


def fragment_id(names, f):
    """Fragment::id (Fragment.cpp:173-183)."""
    a, b = (f[1], f[2]) if f[3] == 1 else (f[2], f[1])
    if a == b and f[3] == -1:
        b = -1
    return "%s_%d_%d" % (names[f[0]], a, b)


def block_tree(b, names, method="nj"):
    """PrintTree::make_tree: (node table, newick with print_newick's defaults)."""
    n = len(b)
    pen = iter(pair_distances([b])[0])
    total = block_length(b)
    d = [[0.0] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1, n):
            d[i][j] = d[j][i] = float(next(pen)) / float(total)
    t = Tree(n)
    if method == "nj":
        neighbor_joining(t, d)
    elif method == "upgma":
        upgma(t, d)
    else:
        raise ValueError("Unknown tree construction method: " + method)
    return table(t), newick(t, [fragment_id(names, f) for f in b])


def block_trees(blocks, names, method="nj"):
    return [block_tree(b, names, method) for b in blocks]


def sort_blocks(blocks, block_names):
    """BlocksJobs::sort_blocks (BlocksJobs.cpp:183-193): size descending,
    alignment length descending, name ascending; ties in set order."""
    return sorted(range(len(blocks)), key=lambda k: (-len(blocks[k]), -block_length(blocks[k]), block_names[k]))


def print_tree_text(blocks, names, block_names, method="nj"):
    """PrintTree's file."""
    out = ["block\tnewick_tree\n"]
    for k in sort_blocks(blocks, block_names):
        out.append("%s\t%s\n" % (block_names[k], block_tree(blocks[k], names, method)[1]))
    return "".join(out)


def fragment_distance_text(blocks, names, block_names):
    """FragmentDistance's file."""
    out = ["block\tfr.1\tfr.2\tdistance\n"]
    for k in sort_blocks(blocks, block_names):
        b = blocks[k]
        pen = iter(pair_distances([b])[0])
        total = block_length(b)
        for i in range(len(b)):
            for j in range(i + 1, len(b)):
                out.append("%s\t%s\t%s\t%s\n" % (block_names[k], fragment_id(names, b[i]), fragment_id(names, b[j]),
                                                 fmt(float(next(pen)) / float(total))))
    return "".join(out)
