"""tests/try_smth_ref.py pinned on hand-made cases, and its SmthUnion /
AddingLoopBySize (all names equal) against the oracle's (CPU only)."""
import numpy as np
import pytest

import joiner_ref as jr
import try_smth_cases as tc
import try_smth_ref as tr
from npge_amd import synth
from oracle import oracle as orc

NAMES = ["g0&chr&c", "g1&chr&c"]


def _genomes(n=600, seed=3):
    rng = np.random.default_rng(seed)
    s = "".join("ATGC"[x] for x in rng.integers(0, 4, n))
    return [s, s]


def _block(seqs, a, b):
    return [(q, a, b, 1, seqs[q][a:b + 1]) for q in range(2)]


def test_unique_names():
    seqs = _genomes()
    items = [(tr.NULL, _block(seqs, 0, 199), "x"), ("", _block(seqs, 300, 499), "x"), ("kept", _block(seqs, 200, 299), "x"),
             (tr.NULL, [(0, 500, 599, 1, None)], "x"), (tr.NULL, [(0, 0, 99, 1, None), (0, 200, 299, 1, None)], "x"),
             (tr.NULL, _block(seqs, 0, 99) + [(0, 300, 399, 1, seqs[0][300:400])], "x")]
    got = [n for (n, _, _) in tr.unique_names(items, NAMES)]
    # two s2x200: block_greater puts the one with the larger smallest fragment first, the other gets n1
    assert got == ["s2x200n1", "s2x200", "kept", "u1x100", "r2x100", "r3x100"]


def test_exact_copy_named_wins():
    seqs = _genomes()
    a = _block(seqs, 0, 199)
    pipe = tr.Pipe(seqs, NAMES)
    for other in ([("s2x200", a, "copy"), ("", list(a), "new")], [("", list(a), "new"), ("s2x200", a, "copy")]):
        info = {}
        assert tr.adding_loop(other, pipe, info) == [("s2x200", a, "copy")]
        assert info["cuts"] == [0]  # the unnamed one is cut away whole


def test_one_column_longer_new_wins():
    seqs = _genomes()
    a, n = _block(seqs, 0, 199), _block(seqs, 0, 200)
    assert tr.adding_loop([("s2x200", a, "copy"), ("", n, "new")], tr.Pipe(seqs, NAMES)) == [("", n, "new")]


def test_new_block_over_half_an_original():
    seqs = _genomes()
    a, n = _block(seqs, 0, 199), _block(seqs, 100, 349)
    info = {}
    got = tr.adding_loop([("s2x200", a, "copy"), ("", n, "new")], tr.Pipe(seqs, NAMES), info)
    # positions 100..199 are the new block's: columns 0..99 of the original stay, a new block
    assert got == [("", n, "new"), (tr.NULL, _block(seqs, 0, 99), "piece")]
    assert info == dict(rounds=2, cuts=[1])


def _gapped_case():
    rng = np.random.default_rng(8)
    s0, s1 = ("".join("ATGC"[x] for x in rng.integers(0, 4, 40)) for _ in range(2))
    t1 = jr.revcomp(s1[0:20])
    row0 = s0[5:10] + "--" + s0[10:15] + "-" + s0[15:20] + "---" + s0[20:25]  # letters at 0-4, 7-11, 13-17, 21-25
    row1 = t1[0:3] + "------" + t1[3:20]                                       # letters at 0-2, 9-25
    assert len(row0) == len(row1) == 26
    return [s0, s1], [(0, 5, 24, 1, row0), (1, 0, 19, -1, row1)], row0, row1


@pytest.mark.parametrize("hit", ["direct", "reverse"])
def test_gaps_at_the_overlap_ends(hit):
    """select: the overlap's ends go from sequence positions to letters to
    columns, across gaps, on a direct and on a reverse fragment."""
    seqs, b, row0, row1 = _gapped_case()
    target, s2f = [], tr.FragIndex()
    if hit == "direct":
        # positions 10..19 of sequence 0 = letters 5..14 of row 0 = columns 7..17
        t = [(0, 10, 19, 1, seqs[0][10:20])]
        exp = [[(0, 5, 9, 1, row0[0:7]), (1, 17, 19, -1, row1[0:7])],
               [(0, 20, 24, 1, row0[18:26]), (1, 0, 7, -1, row1[18:26])]]
    else:
        # positions 5..9 of sequence 1, read backwards from 19 = letters 10..14 of row 1 = columns 16..20
        t = [(1, 5, 9, 1, seqs[1][5:10])]
        exp = [[(0, 5, 17, 1, row0[0:16]), (1, 10, 19, -1, row1[0:16])],
               [(0, 20, 24, 1, row0[21:26]), (1, 0, 4, -1, row1[21:26])]]
    s2f.add(t)
    cuts = []
    sub = tr.smth_union([("b", b, "copy")], target, s2f, seqs, cuts)
    assert sub == [(tr.NULL, exp[0], "piece"), (tr.NULL, exp[1], "piece")] and cuts == [2] and target == []
    for piece in exp:  # every row holds its fragment's letters
        for (q, mn, mx, o, row) in piece:
            assert row.replace("-", "") == jr._text(seqs, q, mn, mx, o)


def test_one_letter_reverse_piece_turns_direct():
    """Block::slice of one letter of an ori -1 fragment: set_begin_last makes
    it ori +1, its letter the forward strand's."""
    seqs = ["ACGTACGTAC"]
    row = jr.revcomp(seqs[0][2:6])  # (0, 2, 5, -1)
    got = tr.slice_block([(0, 2, 5, -1, row)], 1, 1, seqs)
    assert got == [(0, 4, 4, 1, seqs[0][4])]


_DRAFT = {}


def _draft(cfg):
    if cfg not in _DRAFT:
        names, seqs = synth.genome_set(cfg)
        o = orc.BlockSetOracle(seqs, names)
        o.apply("DraftPangenome")
        _DRAFT[cfg] = (seqs, names, o.blocks())
    return _DRAFT[cfg]


@pytest.mark.parametrize("overlapping", [False, True])
def test_adding_loop_equals_oracle_on_tiny(overlapping):
    seqs, names, draft = _draft("tiny")
    blocks = tc.overlapping_set(draft, seqs) if overlapping else draft
    pipe = tr.Pipe(seqs, names)
    info = {}
    got = tr.adding_loop([(tr.NULL, b, "x") for b in blocks], pipe, info)
    assert [b for (_, b, _) in got] == pipe.op(blocks, "AddingLoopBySize")
    assert (max(info["cuts"], default=0) >= 2) == overlapping


def test_align_with_names_equals_align():
    seqs, names, draft = _draft("tiny")
    blocks = tc.overlapping_set(draft, seqs)
    pipe = tr.Pipe(seqs, names)
    got = pipe.align([("n%d" % i, b, "x") for i, b in enumerate(blocks)])
    assert [b for (_, b, _) in got] == pipe.op(blocks, "Align")
    # a block Filter keeps whole keeps its name; its slices are new blocks
    assert {n for (n, _, _) in got} <= {"n%d" % i for i in range(len(blocks))} | {tr.NULL}


def test_try_smth_conditions_on_tiny():
    """The parity cases of tests/test_try_smth_gpu.py show a block kept whole
    from the copy, a new block and a piece."""
    seen = set()
    for cfg, inner in (("tiny", "FragmentsExtender"), ("rtiny", "FragmentsExtender")):
        seqs, names, draft = _draft(cfg)
        info = {}
        blocks, bnames = tr.try_smth(draft, seqs, names, inner, info)
        assert len(blocks) == len(bnames) == len(set(bnames))
        seen |= {"whole" if (t == "copy" and b in draft) else t for (t, b) in info["tags"]}
    assert {"whole", "new", "piece"} <= seen
