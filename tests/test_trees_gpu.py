"""Trees and fragment distances on the engine (npgx_blockset_pair_distances /
k_pair_dist, npgx_blockset_genome_distances, npgx_blockset_global_tree /
k_clade_diag, npgx_blockset_block_trees and the GlobalTree, PrintTree and
FragmentDistance processors): exact parity with the sequential restatement
(tests/tree_ref.py) -- integers equal, doubles bit for bit, texts equal -- on
the inputs of tests/tree_cases.py and on real DraftPangenome output."""
import struct

import numpy as np
import pytest

import tree_cases as tc
import tree_ref as tr
from npge_amd import synth
from npge_amd.model import Block, BlockSet, Fragment, Sequence

pytestmark = pytest.mark.gpu

NPGX_ERR_ARG, NPGX_ERR_RANGE, NPGX_ERR_STATE = -1, -4, -5


def _engine(seqs, names, blocks=None):
    from npge_amd import _capi
    from npge_amd.blockset import BlockSetEngine
    eng = BlockSetEngine(_capi.SeqSet(seqs, names))
    if blocks is not None:
        eng.set_blocks(blocks)
    return eng


def _bits(table):
    """A node table with its doubles as bytes: compared bit for bit."""
    return [(p, leaf, struct.pack("<d", a), struct.pack("<d", b)) for p, leaf, a, b in table]


_DRAFT = {}


def _draft(cfg):
    """The engine's DraftPangenome output on a synthetic set (made once)."""
    if cfg not in _DRAFT:
        from npge_amd.anchor_finder import AnchorFinder
        names, seqs = synth.genome_set(cfg)
        eng = _engine(seqs, names)
        eng.apply("DraftPangenome", af=AnchorFinder())
        _DRAFT[cfg] = (seqs, names, eng.blocks())
    return _DRAFT[cfg]


_SHAPES = {}


def _shapes():
    if not _SHAPES:
        _SHAPES["rows"] = tc.shape_rows()
        _SHAPES["set"] = tc.blocks_of(_SHAPES["rows"])
    return _SHAPES["set"]


# ---------------------------------------------------------------- 1: shapes
def test_pair_distances_shapes():
    seqs, names, blocks = _shapes()
    got = _engine(seqs, names, blocks).pair_distances()
    assert len(got) == len(tc.SHAPES)
    for (n, L), b, g in zip(tc.SHAPES, blocks, got):
        assert len(g) == n * (n - 1) // 2
        assert g == tr.pair_distances([b])[0], (n, L)


# ---------------------------------------------------------------- 2: seams
def _check_seams(cases, n):
    seqs, names, blocks = tc.blocks_of([rows for _, _, rows, _ in cases])
    got = _engine(seqs, names, blocks).pair_distances()
    for (c, form, rows, exp), g in zip(cases, got):
        pen = iter(g)
        for i in range(n):
            for j in range(i + 1, n):
                assert next(pen) == (exp if j == n - 1 else 0), (c, form, i, j)


def test_pair_distances_seams():
    """One isolated mismatch at the word seams (63 | 64), the widest tile's
    edge (4095 | 4096) and the row's ends, in the four forms."""
    _check_seams(tc.seam_rows(), 2)


@pytest.mark.parametrize("n", [17, 65])
def test_pair_distances_tile_edges(n):
    """The tile of a block of n rows is narrower than 4096 columns (its rows
    share the LDS): the same forms at that width's edges, read from the
    library."""
    from npge_amd.blockset import pair_dist_tile_columns
    W = pair_dist_tile_columns(n)
    assert W % 64 == 0 and 64 <= W < 4096 and pair_dist_tile_columns(2) == 4096
    L = 2 * W + 70
    _check_seams(tc.seam_rows(L, [W - 2, W - 1, W, W + 1, 2 * W - 1, 2 * W, L - 2, L - 1], n), n)


# ---------------------------------------------------------------- 3: batch
def test_pair_distances_batch():
    rows = tc.batch_rows(31, 133)
    seqs, names, blocks = tc.blocks_of(rows)
    assert sum(len(b) == 1 for b in blocks) >= 10 and max(len(b) for b in blocks) > 64
    eng = _engine(seqs, names, blocks)
    got = eng.pair_distances()
    assert [len(g) for g in got] == [len(b) * (len(b) - 1) // 2 for b in blocks]
    assert got == tr.pair_distances(blocks)
    # a second, smaller set on the same engine: nothing of the first one is left
    small = [blocks[k] for k in (100, 3, 57, 20, 9, 64, 131)]
    eng.set_blocks(small)
    assert eng.pair_distances() == tr.pair_distances(small)


def test_pair_distances_block_without_rows():
    from npge_amd._capi import NpgxError
    seqs, names, blocks = tc.blocks_of(tc.batch_rows(33, 4) + [[None, None]])
    eng = _engine(seqs, names, blocks)
    before = eng.blocks()
    with pytest.raises(NpgxError) as e:
        eng.pair_distances()
    assert e.value.code == NPGX_ERR_STATE
    assert eng.blocks() == before == blocks


# ---------------------------------------------------------------- 4: real output
@pytest.mark.parametrize("cfg", ["tiny", "small", "rtiny"])
def test_global_tree_on_draft(cfg):
    seqs, names, draft = _draft(cfg)
    # DraftPangenome keeps stem blocks only; two blocks made of its own rows stand for what later
    # steps add: a genome missing, and a genome twice (rtiny: a copy of another of its fragments)
    big = max(draft, key=len)
    draft = draft + [big[:-1], big + [big[0]]]
    eng = _engine(seqs, names, draft)
    h, dg = eng.hash(), eng.rows_digest()
    m, t, genomes = tr.global_tree_build(draft, names)
    stem = tr.stem_blocks(draft, names)
    print(cfg, len(draft), "blocks,", len(stem), "stem;", genomes)
    assert 0 < len(stem) == len(draft) - 2
    assert eng.genomes() == genomes
    assert eng.genome_distances() == m
    text, nodes = eng.global_tree()
    exp_nodes, exp_text = tr.global_tree_render(t, genomes)
    assert _bits(nodes) == _bits(exp_nodes)
    assert text == exp_text
    assert eng.hash() == h and eng.rows_digest() == dg and eng.blocks() == draft


# ---------------------------------------------------------------- 5: planted trees
@pytest.mark.parametrize("G", tc.PLANTED_G)
def test_global_tree_planted(G):
    seqs, names, blocks, stem = tc.planted_genomes(G)
    eng = _engine(seqs, names, blocks)
    m, t, genomes = tr.global_tree_build(blocks, names)
    assert eng.genome_distances() == m
    for bp in tc.BOOTSTRAP_PRINTS:
        for pseudo in (False, True):
            text, nodes = eng.global_tree(bootstrap_print=bp, pseudo_leafs=pseudo)
            exp_nodes, exp_text = tr.global_tree_render(t, genomes, bp, pseudo)
            assert _bits(nodes) == _bits(exp_nodes), (bp, pseudo)
            assert text == exp_text, (bp, pseudo)


def _clade_bootstrap(nodes, clade):
    """The bootstrap of the node of a table whose leaves are `clade` (or all
    the others: the same branch seen from its other side)."""
    n = len(nodes)
    under = [set() for _ in range(n)]
    for k in range(n - 1, 0, -1):
        if nodes[k][1] >= 0:
            under[k].add(nodes[k][1])
        under[nodes[k][0]] |= under[k]
    everyone = under[0]
    hits = [nodes[k][3] for k in range(1, n) if under[k] in (set(clade), everyone - set(clade))]
    assert len(hits) == 1
    return hits[0]


def test_global_tree_planted_known_answer():
    """The block of equal rows with PLANTED_COLUMNS set apart for the genomes
    0..3 adds no distance (the planted columns stand in pairs) and exactly its
    four columns -- at the word seam and the tile's edge -- to that clade's
    bootstrap."""
    seqs, names, blocks, stem = tc.planted_genomes(8)
    with_block = _engine(seqs, names, blocks).global_tree()[1]
    k = stem[-1]
    plain_row = blocks[k][7][4]  # a row of the genomes 4..7: the block without its planted columns
    assert "-" not in plain_row
    plain = [(q, mn, mx, o, plain_row) for (q, mn, mx, o, r) in blocks[k]]
    seqs2 = [s[:blocks[k][g][1]] + plain_row + s[blocks[k][g][2] + 1:] if g < 4 else s for g, s in enumerate(seqs)]
    without = _engine(seqs2, names, blocks[:k] + [plain] + blocks[k + 1:]).global_tree()[1]
    a = _clade_bootstrap(with_block, range(4))
    b = _clade_bootstrap(without, range(4))
    assert a - b == float(len(tc.PLANTED_COLUMNS))
    assert [x[:3] for x in with_block] == [x[:3] for x in without]  # the same tree, the same lengths


def test_global_tree_65_genomes():
    from npge_amd._capi import NpgxError
    rows = tc.random_rows(np.random.default_rng(41), 65, 200)
    seqs = [r.replace("-", "") for r in rows]
    names = ["H%02d&chr1&c" % g for g in range(65)]
    blocks = [[(g, 0, len(seqs[g]) - 1, 1, rows[g]) for g in range(65)]]
    eng = _engine(seqs, names, blocks)
    with pytest.raises(NpgxError) as e:
        eng.global_tree()
    assert e.value.code == NPGX_ERR_RANGE
    assert eng.pair_distances() == tr.pair_distances(blocks)
    m = eng.genome_distances()
    assert m == tr.genome_matrix(blocks, names)
    with pytest.raises(NpgxError) as e:
        eng.global_tree(bootstrap_print="sometimes")
    assert e.value.code == NPGX_ERR_ARG


# ---------------------------------------------------------------- 6: PrintTree
@pytest.mark.parametrize("method", ["nj", "upgma"])
def test_block_trees(method):
    from npge_amd._capi import NpgxError
    seqs, names, draft = _draft("small")
    got = _engine(seqs, names, draft).block_trees(method)
    exp = tr.block_trees(draft, names, method)
    assert len(got) == len(draft)
    for (text, nodes), (exp_nodes, exp_text) in zip(got, exp):
        assert _bits(nodes) == _bits(exp_nodes)
        assert text == exp_text
    seqs, names, blocks = _shapes()
    k = tc.SHAPES.index((65, 130))
    (text, nodes), = _engine(seqs, names, [blocks[k]]).block_trees(method)
    exp_nodes, exp_text = tr.block_tree(blocks[k], names, method)
    assert _bits(nodes) == _bits(exp_nodes) and text == exp_text
    with pytest.raises(NpgxError) as e:
        _engine(seqs, names, [blocks[0]]).block_trees("parsimony")
    assert e.value.code == NPGX_ERR_ARG


# ---------------------------------------------------------------- 7: processors
def _model(seqs, names, blocks):
    bs = BlockSet()
    bs.seqs = [Sequence(n, s) for n, s in zip(names, seqs)]
    bnames = ["n%03d" % ((k * 37) % 11) for k in range(len(blocks))]  # names repeat: ties stay in set order
    bs.blocks = [Block([Fragment(bs.seqs[q], mn, mx, o, r) for (q, mn, mx, o, r) in b], name=bn)
                 for b, bn in zip(blocks, bnames)]
    return bs, bnames


def test_processors_write_the_reference_files(tmp_path):
    from npge_amd import script  # noqa: F401  (registers the processors)
    from npge_amd.processor import new_p
    seqs, names, draft = _draft("small")
    bs, bnames = _model(seqs, names, draft)
    before = [[(f.seq.name, f.min_pos, f.max_pos, f.ori, f.row) for f in b.fragments] for b in bs.blocks]

    def run(name, opts):
        p = new_p(name)
        p.set_bs("target", bs)
        p.set_options(opts)
        p.run()
        return p

    m, t, genomes = tr.global_tree_build(draft, names)
    for bp, pseudo in (("before-length", 0), ("in-braces", 1), ("no", 0)):
        path = tmp_path / ("global_%s.tre" % bp)
        run("GlobalTree", "--out-global-tree:=%s --bootstrap-print:=%s --tree-pseudo-leafs:=%d" % (path, bp, pseudo))
        assert path.read_text() == tr.global_tree_render(t, genomes, bp, bool(pseudo))[1]
    for method in ("nj", "upgma"):
        path = tmp_path / ("trees_%s.tsv" % method)
        run("PrintTree", "--tree-file:=%s --tree-method:=%s" % (path, method))
        assert path.read_text() == tr.print_tree_text(draft, names, bnames, method)
    path = tmp_path / "distances.tsv"
    p = run("FragmentDistance", "--distance-file:=%s" % path)
    exp = tr.fragment_distance_text(draft, names, bnames)
    assert path.read_text() == exp == p.text
    assert exp.startswith("block\tfr.1\tfr.2\tdistance\n") and exp.count("\n") > len(draft)
    assert [[(f.seq.name, f.min_pos, f.max_pos, f.ori, f.row) for f in b.fragments] for b in bs.blocks] == before


def test_apply_keeps_results_and_try_smth_refuses():
    from npge_amd._capi import NpgxError
    seqs, names, draft = _draft("tiny")
    eng = _engine(seqs, names, draft)
    h = eng.hash()
    eng.apply("FragmentDistance").apply("PrintTree --tree-method=upgma").apply("GlobalTree --bootstrap-print=no")
    assert eng.hash() == h and eng.blocks() == draft
    assert eng.pair_distances() == tr.pair_distances(draft)
    for name in ("GlobalTree", "PrintTree", "FragmentDistance"):
        with pytest.raises(NpgxError) as e:
            eng.apply("TrySmth --smth-processor:=" + name)
        assert e.value.code == NPGX_ERR_ARG
    with pytest.raises(NpgxError) as e:
        eng.apply("GlobalTree --bootstrap-print=often")
    assert e.value.code == NPGX_ERR_ARG
    assert eng.hash() == h and eng.blocks() == draft
