"""The restatement of LiteFilter, MergeUnique and the JoinerP pipes
(tests/joiner_pipes_ref.py) on the CPU: its properties, the hand-made case
and which synthetic sets give MergeUnique something to merge."""
import pytest

import joiner_pipes_ref as jp
import try_smth_ref as tr
from npge_amd import synth
from oracle import oracle as orc

NULL = jp.NULL


def _rest(seqs, names, blocks):
    return jp.rest(blocks, [NULL] * len(blocks), tr.Pipe(seqs, names))


def _covered_once(blocks, seqs):
    cover = [[0] * len(s) for s in seqs]
    for b in blocks:
        for (q, mn, mx, _, _) in b:
            for p in range(mn, mx + 1):
                cover[q][p] += 1
    return all(c == 1 for row in cover for c in row)


_DRAFT = {}


def _draft(cfg):
    if cfg not in _DRAFT:
        names, seqs = synth.genome_set(cfg)
        o = orc.BlockSetOracle(seqs, names)
        o.apply("DraftPangenome")
        _DRAFT[cfg] = (seqs, names, o.blocks())
    return _DRAFT[cfg]


# ---------------------------------------------------------------- the hand-made case
def test_hand_case_rest_and_merge():
    seqs, names, blocks = jp.hand_case()
    rested, rn = _rest(seqs, names, blocks)
    assert [b for b in rested[2:]] == [[(0, 300, 339, 1, None)], [(1, 300, 339, 1, None)], [(2, 300, 339, 1, None)],
                                       [(3, 300, 339, 1, None)]]
    counts = {}
    got, gn = jp.merge_unique(rested, rn, counts=counts)
    assert gn == [NULL, NULL, NULL, "m3x40"]
    assert got[:2] == blocks and got[2] == [(3, 300, 339, 1, None)]
    # each merged fragment has the ori of its neighbour in block X: the third sequence is reverse-complemented
    assert got[3] == [(0, 300, 339, 1, None), (1, 300, 339, 1, None), (2, 300, 339, -1, None)]
    assert counts == dict(blocks_inspected=2, merges=1, fragments_merged=3)
    assert _covered_once(got, seqs)
    # one neighbour is enough: the fourth sequence's unique fragment, which has no second neighbour, joins them
    got1, gn1 = jp.merge_unique(rested, rn, both=False, counts=counts)
    assert gn1 == [NULL, NULL, "m4x40"] and got1[:2] == blocks
    assert got1[2] == got[3] + [(3, 300, 339, 1, None)]
    assert counts == dict(blocks_inspected=2, merges=1, fragments_merged=4)
    assert _covered_once(got1, seqs)


def test_hand_case_pipes():
    seqs, names, blocks = jp.hand_case(fourth=False)
    got, gn = jp.run("JoinerP", blocks, seqs, names)
    assert len(got) == 1 and gn == [NULL]  # X, m3x40 and Y join into one block
    assert [(q, mn, mx, o) for (q, mn, mx, o, _) in got[0]] == [(0, 0, 639, 1), (1, 0, 639, 1), (2, 0, 639, -1)]
    assert len({len(f[4]) for f in got[0]}) == 1 and _covered_once(got, seqs)
    assert jp.run("MergeAndJoin", blocks, seqs, names) == (got, gn)
    # without Rest, Y is X's neighbour: Joiner aligns the unique fragments as the middle of the pair
    lite, ln = jp.run("LiteJoinerP", blocks, seqs, names)
    assert ln == [NULL] and [[f[:4] for f in b] for b in lite] == [[f[:4] for f in b] for b in got]
    # with the fourth sequence block X has four fragments and joins nothing
    seqs, names, blocks = jp.hand_case()
    got, gn = jp.run("JoinerP", blocks, seqs, names)
    assert sorted(len(b) for b in got) == [1, 3, 4] and _covered_once(got, seqs)


def test_merged_rows():
    """Identity rows of one length stay, the flipped fragment's reverse-complemented."""
    seqs, names, blocks = jp.hand_case()
    pipe = tr.Pipe(seqs, names)
    x = jp.meta_aligner(*_rest(seqs, names, blocks), pipe)
    got, _ = jp.merge_unique(*x)
    assert [f[4] for f in got[3]] == [seqs[0][300:340], seqs[1][300:340], jp.jr.revcomp(seqs[2][300:340])]
    gapped = [[f[:4] + (f[4][:5] + "-" + f[4][5:],) for f in b] if len(b) == 1 else b for b in x[0]]
    with pytest.raises(jp.GappedFlip):
        jp.merge_unique(gapped, x[1])
    # rows of different lengths: the merged block is not aligned
    mixed = [gapped[k] if k == 2 else b for k, b in enumerate(x[0])]
    got, gn = jp.merge_unique(mixed, x[1])
    assert gn[-1] == "m3x41" and all(f[4] is None for f in got[-1])


def test_merge_long():
    seqs, names, blocks = jp.hand_case(ulen=120)
    rested, rn = _rest(seqs, names, blocks)
    assert jp.merge_unique(rested, rn) == (rested, rn)  # 120 >= MIN_LENGTH: not unique enough
    got, gn = jp.merge_unique(rested, rn, merge_long=True)
    assert gn[-1] == "m3x120" and len(got) == len(rested) - 2


def test_lite_filter():
    seqs, names, blocks = jp.hand_case()
    rested, rn = _rest(seqs, names, blocks)
    assert jp.lite_filter(rested, rn) == (blocks, [NULL, NULL])
    assert jp.lite_filter(rested, rn, min_fragment=0, min_block=1) == (rested, rn)
    assert jp.lite_filter(rested, rn, min_fragment=150, min_block=4) == ([blocks[0]], [NULL])


# ---------------------------------------------------------------- the synthetic sets
MERGES = {"tiny": True, "rtiny": True, "small": True}  # does MergeUnique after Rest merge anything?


@pytest.mark.parametrize("cfg", ["tiny", "rtiny", "small"])
def test_properties_on_synth(cfg):
    seqs, names, draft = _draft(cfg)
    rested, rn = _rest(seqs, names, draft)
    assert _covered_once(rested, seqs)
    c2, c1 = {}, {}
    got2, gn2 = jp.merge_unique(rested, rn, counts=c2)
    got1, gn1 = jp.merge_unique(rested, rn, both=False, counts=c1)
    print(cfg, len(draft), "blocks;", c2, c1)
    for got, gn in ((got2, gn2), (got1, gn1)):
        assert _covered_once(got, seqs)  # every base of every sequence is in exactly one fragment
        for b, n in zip(got, gn):
            assert (n == "m%dx%d" % (len(b), jp.aln_len(b))) == (n != NULL)
    merged2 = {f[:3] for b, n in zip(got2, gn2) if n != NULL for f in b}
    merged1 = {f[:3] for b, n in zip(got1, gn1) if n != NULL for f in b}
    assert merged2 <= merged1  # one neighbour merges a superset of what two do
    assert (c2["merges"] > 0) == MERGES[cfg]
