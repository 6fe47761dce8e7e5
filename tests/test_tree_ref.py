"""Trees and fragment distances without a GPU: the reference's known answers
(src/test/tree.cpp) and hand-made columns against the restatement
(tests/tree_ref.py), the C++ host tree code (npge_amd/csrc/tree.cpp, built into
a stand-alone program) against the restatement bit for bit, and the inputs of
the GPU tests (tests/tree_cases.py): every one of them has work in it."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import tree_cases as tc
import tree_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "npge_amd", "csrc")


def _tree(method, d):
    t = tr.Tree(len(d))
    (tr.neighbor_joining if method == "nj" else tr.upgma)(t, d)
    return t


def _matrix(n, entries):
    d = [[0.0] * n for _ in range(n)]
    for (i, j), v in entries.items():
        d[i][j] = d[j][i] = float(v)
    return d


def _close(a, b):
    return abs(a - b) < 1e-4


KAT3 = _matrix(3, {(0, 1): 2, (0, 2): 5, (1, 2): 7})
KAT4 = _matrix(4, {(0, 1): 7, (0, 2): 11, (0, 3): 14, (1, 2): 6, (1, 3): 9, (2, 3): 7})


# ---------------------------------------------------------------- the reference's known answers
def test_tree_upgma():
    t = _tree("upgma", KAT3)
    assert len(t.top) == 1
    root = t.nodes[t.top[0]]
    assert _close(root.length, 0.0) and len(root.children) == 2
    left, right = root.children
    assert _close(t.nodes[left].length, 3.0) and _close(t.nodes[right].length, 3.0)
    assert 2 in (left, right)
    b12 = right if left == 2 else left
    assert sorted(t.nodes[b12].children) == [0, 1]
    assert _close(t.nodes[0].length, 1.0) and _close(t.nodes[1].length, 1.0)
    # the pinned pair order: the joined pair's lower number first, the new node after the survivor
    assert t.nodes[b12].children == [0, 1] and root.children == [2, 3]


def test_tree_nj():
    t = _tree("nj", KAT3)
    assert len(t.top) == 3
    assert _close(tr.tree_distance(t, 0, 1), 2.0)
    assert _close(tr.tree_distance(t, 0, 2), 5.0)
    assert _close(tr.tree_distance(t, 1, 2), 7.0)


def test_tree_nj_2():
    t = _tree("nj", _matrix(2, {(0, 1): 2}))
    assert len(t.top) == 2 and _close(tr.tree_distance(t, 0, 1), 2.0)


def test_tree_nj_1():
    t = _tree("nj", [[0.0]])
    assert len(t.top) == 1 and _close(t.nodes[0].length, 0.0)
    assert tr.newick(t, ["a1"]) == "(\n  a1:0\n);"


def test_tree_nj_w():
    t = _tree("nj", KAT4)
    for i in range(4):
        for j in range(i + 1, 4):
            assert _close(tr.tree_distance(t, i, j), KAT4[i][j])
    assert t.nodes[0].parent == t.nodes[1].parent >= 0


def test_tree_distance():
    # a1, a2 under a12 (10) under a123 with a3 (20); a123 and a4 under the root
    t = tr.Tree(4)
    a1, a2, a3, a4 = 0, 1, 2, 3
    t.nodes[a1].length, t.nodes[a2].length, t.nodes[a3].length = 1.0, 2.0, 20.0
    a12 = tr._join(t, a1, a2)
    t.nodes[a12].length = 10.0
    a123 = tr._join(t, a12, a3)
    t.top = [a123, a4]
    exp = {(a1, a2): 3, (a2, a1): 3, (a1, a1): 0, (a12, a12): 0, (a1, a12): 1, (a2, a12): 2, (a1, a3): 31,
           (a1, a123): 11, (a2, a3): 32, (a3, a123): 20, (a3, a12): 30, (a3, a3): 0, (a4, a4): 0, (a1, a4): 11,
           (a2, a4): 12, (a3, a4): 20, (a123, a4): 0}
    for (x, y), v in exp.items():
        assert _close(tr.tree_distance(t, x, y), v), (x, y)


def test_newick_forms():
    t = _tree("nj", KAT4)
    for k, v in zip(tr.descendants(t), range(1, 10)):
        t.nodes[k].bootstrap = float(v)
    names = list("abcd")
    # by hand: Q(a,b) = Q(c,d) = -40 (the first wins), a 3.5 + 0.5 * (25 - 15) / 2 = 6, b 1; d(u,c) = 5,
    # d(u,d) = 8; of the last three c 3.5 + 0.5 * (5 - 8) = 2, d 5, u 0.5 * (5 + 8 - 7) = 3
    assert tr.newick(t, names) == "(\n  c:2,\n  d:5,\n  (\n    a:6,\n    b:1\n  ):3\n);"
    assert tr.newick(t, names, True, tr.BOOTSTRAP_BEFORE_LENGTH) == \
        "(\n  c:2,\n  d:5,\n  (\n    a:6,\n    b:1\n  )3:3\n);"
    assert tr.newick(t, names, True, tr.BOOTSTRAP_IN_BRACES) == \
        "(\n  c:2[1],\n  d:5[2],\n  (\n    a:6[4],\n    b:1[5]\n  ):3[3]\n)[0];"
    p = tr.clone_with_pseudo_leafs(t)
    assert tr.newick(p, names, True, tr.BOOTSTRAP_BEFORE_LENGTH).startswith(
        "(\n  (\n    c:0,\n    .c:0\n  )1:2,\n  (\n    d:0,\n    .d:0\n  )2:5,\n  (\n    (\n      a:0,\n      .a:0\n    )4:6,")
    assert [x[1] for x in tr.table(p)] == [-1, -1, 2, -4, -1, 3, -5, -1, -1, 0, -2, -1, 1, -3]


# ---------------------------------------------------------------- fragment_distance, is_diagnostic by hand
@pytest.mark.parametrize("a,b,exp", [
    ("", "", 0), ("A", "C", 0), ("AC", "AG", 0), ("ACA", "AGA", 1), ("A-A", "AGA", 1), ("A-A", "A-A", 0),
    ("-CA", "-GA", 0), ("NCN", "NGN", 1), ("ACCA", "AGGA", 0), ("CAA", "GAA", 0), ("AAC", "AAG", 0),
    ("ACAGA", "ATACA", 2), ("AC-", "AG-", 0)])
def test_fragment_distance_by_hand(a, b, exp):
    assert tr.fragment_distance(a, b) == exp
    assert tr.fragment_distance(b, a) == exp
    if a:
        assert tr.block_penalties([a, b]) == [exp]


def test_is_diagnostic_by_hand():
    #        0: letter split  1: gap split  2: clade with two letters  3: an outside row shares the letter
    rows = ["A-AA",
            "A-CA",
            "CTGA",
            "CGGC"]
    clade, other = rows[:2], rows[2:]
    assert [tr.is_diagnostic(c, clade, other) for c in range(4)] == [True, True, False, False]
    assert tr.diagnostic_columns(rows, [0, 1]) == 2
    # the other side: the letter split and column 2 (G G against A C); in column 1 it holds T and G
    assert tr.diagnostic_columns(rows, [2, 3]) == 2
    assert tr.diagnostic_columns(rows, []) == 0 and tr.diagnostic_columns(rows, [0, 1, 2, 3]) == 0


def test_vector_forms_equal_the_plain_loops():
    rng = np.random.default_rng(3)
    for n, L in [(2, 3), (3, 7), (5, 64), (6, 131)]:
        rows = tc.random_rows(rng, n, L)
        pen = iter(tr.block_penalties(rows))
        for i in range(n):
            for j in range(i + 1, n):
                assert next(pen) == tr.fragment_distance(rows[i], rows[j])
        for mask in range(1, 2 ** n - 1):
            inside = [i for i in range(n) if mask >> i & 1]
            clade = [rows[i] for i in inside]
            other = [rows[i] for i in range(n) if not mask >> i & 1]
            assert tr.diagnostic_columns(rows, inside) == sum(tr.is_diagnostic(c, clade, other) for c in range(L))


# ---------------------------------------------------------------- the C++ host tree code
@pytest.fixture(scope="module")
def tree_program(tmp_path_factory):
    """tree.cpp + tree_main.cpp as a stand-alone executable with build.py's
    flags, under AddressSanitizer and UBSan when the compiler has them."""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the host tree program")
    from npge_amd.build import HOST_FLAGS
    out = str(tmp_path_factory.mktemp("tree") / "tree_main")
    base = ["g++", "-O2", "-std=c++17"] + HOST_FLAGS["tree.cpp"]
    srcs = [os.path.join(CSRC, "tree.cpp"), os.path.join(CSRC, "tree_main.cpp")]
    san = subprocess.run(base + ["-fsanitize=address,undefined", "-o", out] + srcs, capture_output=True, text=True)
    if san.returncode != 0:
        subprocess.run(base + ["-o", out] + srcs, check=True)
    return out


def _run_trees(program, cases):
    """cases: (method, sbs, pseudo, matrix) -> [(node table, newick)]."""
    inp = []
    for method, sbs, pseudo, d in cases:
        inp.append("tree %s %d %d %d\n%s\n" % (method, sbs, pseudo, len(d),
                                               " ".join(float(x).hex() for row in d for x in row)))
    out = subprocess.run([program], input="".join(inp), capture_output=True, text=True, check=True).stdout
    res, pos = [], 0
    for _ in cases:
        end = out.index("\n", pos)
        k = int(out[pos:end].split()[1])
        pos = end + 1
        tb = []
        for _ in range(k):
            end = out.index("\n", pos)
            p = out[pos:end].split()
            tb.append((int(p[0]), int(p[1]), float.fromhex(p[2]), float.fromhex(p[3])))
            pos = end + 1
        end = out.index("\n", pos)
        nbytes = int(out[pos:end].split()[1])
        pos = end + 1
        res.append((tb, out[pos:pos + nbytes]))
        pos += nbytes + 1
    assert pos == len(out)
    return res


def _bits(tb):
    return [(p, leaf, np.float64(a).tobytes(), np.float64(b).tobytes()) for p, leaf, a, b in tb]


def random_matrices():
    """200 integer matrices of 2 to 40 leaves; small value ranges among them,
    so that many minima are tied and the first-minimum and pair-order pins
    decide the tree."""
    rng = random.Random(5)
    cases = []
    for _ in range(200):
        n = rng.randint(2, 40)
        hi = rng.choice([2, 3, 5, 50, 1000])
        d = [[0] * n for _ in range(n)]
        for i in range(n):
            for j in range(i + 1, n):
                d[i][j] = d[j][i] = rng.randint(1, hi)
        cases.append((rng.choice(["nj", "upgma"]), rng.randint(0, 2), rng.randint(0, 1), d))
    return cases


def test_host_tree_code_equals_the_restatement(tree_program):
    cases = [(m, sbs, ps, d) for d in (KAT3, KAT4, _matrix(2, {(0, 1): 2}), [[0.0]])
             for m in ("nj", "upgma") for sbs in (0, 1, 2) for ps in (0, 1)] + random_matrices()
    got = _run_trees(tree_program, cases)
    tied = 0
    for (method, sbs, pseudo, d), (tb, text) in zip(cases, got):
        t, ties = tr.Tree(len(d)), []
        (tr.neighbor_joining if method == "nj" else tr.upgma)(t, d, ties)
        tied += any(ties)
        if pseudo:
            t = tr.clone_with_pseudo_leafs(t)
        assert _bits(tr.table(t)) == _bits(tb), (method, len(d))
        assert tr.newick(t, ["n%d" % i for i in range(len(d))], True, sbs) == text
    print("matrices with a tied minimum in some round:", tied, "of", len(cases))
    assert tied >= len(cases) // 4


def test_host_fragment_penalty_equals_the_restatement(tree_program):
    rng = np.random.default_rng(8)
    for n, L in [(2, 0), (2, 1), (2, 2), (2, 3), (4, 65), (3, 200)]:
        rows = tc.random_rows(rng, n, L) if L else [""] * n
        out = subprocess.run([tree_program], input="pairs %d %d 1\n%s\n" % (n, L, "\n".join(rows)),
                             capture_output=True, text=True, check=True).stdout.split("\n")
        assert out[0] == "pairs %d" % (n * (n - 1) // 2)
        assert [int(x) for x in out[1].split()] == (tr.block_penalties(rows) if L else [0] * (n * (n - 1) // 2))


# ---------------------------------------------------------------- the GPU tests' inputs have work in them
def test_shapes_have_work():
    for (n, L), rows in zip(tc.SHAPES, tc.shape_rows()):
        assert len(rows) == n and all(len(r) == L for r in rows)
        pen = tr.block_penalties(rows)
        assert len(pen) == n * (n - 1) // 2
        assert (max(pen) > 0) == (L >= 3), (n, L)


def test_seams_expected():
    for c, form, rows, exp in tc.seam_rows():
        assert tr.fragment_distance(rows[0], rows[1]) == exp, (c, form)
    assert [e for c, f, r, e in tc.seam_rows() if f == "letter"] == [0] + [1] * 10 + [0]


def test_batches_have_work():
    for seed, count in ((31, 133), (32, 9)):
        for rows in tc.batch_rows(seed, count):
            if len(rows) >= 2 and len(rows[0]) >= 3:
                assert max(tr.block_penalties(rows)) > 0


@pytest.mark.parametrize("G", tc.PLANTED_G)
def test_planted_trees_have_work(G):
    seqs, names, blocks, stem = tc.planted_genomes(G)
    assert [blocks.index(b) for b in tr.stem_blocks(blocks, names)] == stem and len(blocks) > len(stem)
    assert any(len(b[0][4]) == 4097 for b in (blocks[k] for k in stem))
    m, t, genomes = tr.global_tree_build(blocks, names)
    assert genomes == sorted(genomes) and len(genomes) == G
    if G >= 2:
        assert max(max(row) for row in m) > 0
        boot = [t.nodes[k].bootstrap for k in tr.descendants(t)]
        assert max(boot) > 0 and (G == 2 or min(boot) == 0)
    if G == 8:  # the planted clade is a node of the tree (from either side of its branch)
        sets = [sorted(tr.leaves_under(t, k)) for k in tr.descendants(t)]
        assert [0, 1, 2, 3] in sets or [4, 5, 6, 7] in sets
