"""The sequential restatement of ReAlign and of the block statistics
(tests/realign_ref.py) pinned with the reference's own known answer
(Block_alignment_stat, src/test/block.cpp:89-143) and shown to take every
branch of ReAlign.cpp:49-59 on this project's own data."""
import realign_ref as rr
from npge_amd import synth
from oracle import oracle as orc

KAT_ROWS = ["TAGTCCG-", "TGTT-CG-", "TG---CG-"]


def test_block_alignment_stat():
    st = rr.stat(KAT_ROWS)
    assert (st["ident_nogap"], st["ident_gap"], st["noident_nogap"], st["noident_gap"]) == (3, 2, 1, 1)
    assert st["pure_gap"] == 1 and st["total"] == 8
    assert st["letters"] == [1, 6, 6, 4, 0]  # A T G C N
    # block_identity: (3 + 2 / 2) / 7 = 0.571428..., truncated to Decimal's four digits
    assert rr.identity_x1e4(st) == 5714
    st5 = rr.stat([r[5:] for r in KAT_ROWS])
    assert (st5["ident_nogap"], st5["ident_gap"], st5["noident_nogap"], st5["noident_gap"]) == (2, 0, 0, 0)
    assert st5["pure_gap"] == 1 and st5["total"] == 3 and st5["letters"] == [0, 0, 3, 3, 0]
    st56 = rr.stat([r[5:7] for r in KAT_ROWS])
    assert (st56["ident_nogap"], st56["ident_gap"], st56["noident_nogap"], st56["noident_gap"]) == (2, 0, 0, 0)
    assert st56["pure_gap"] == 0 and st56["total"] == 2 and st56["letters"] == [0, 0, 3, 3, 0]
    assert rr.identity_x1e4(st56) == 10000


def test_identity_arithmetic():
    """(10000 in + 5000 ig) / total in integer division; 0 without columns."""
    mk = lambda a, b, c, d: dict(ident_nogap=a, ident_gap=b, noident_nogap=c, noident_gap=d)
    assert rr.identity_x1e4(mk(0, 0, 0, 0)) == 0
    assert rr.identity_x1e4(mk(0, 1, 0, 0)) == 5000
    assert rr.identity_x1e4(mk(2, 0, 1, 0)) == 6666   # truncated, not rounded
    assert rr.identity_x1e4(mk(1, 1, 0, 1)) == 5000
    assert rr.identity_x1e4(mk(483, 0, 0, 517)) == 4830
    assert rr.identity_x1e4(rr.stat(["--", "--"])) == 0  # pure-gap columns are not in the total


def test_n_is_an_ordinary_letter():
    """N against N is ident, N against A is not (test_column compares the
    characters; Filter's isColumnGood is another rule)."""
    st = rr.stat(["NNA-", "NAAN"])
    assert (st["ident_nogap"], st["ident_gap"], st["noident_nogap"], st["noident_gap"]) == (2, 1, 1, 0)
    assert st["letters"] == [3, 0, 0, 0, 4]
    assert rr.identity_x1e4(st) == 6250


def test_realign_takes_every_branch_on_small():
    """On the oracle's DraftPangenome output of synth config `small` (99
    blocks): 36 replaced, 3 refused by Filter (the new block is bad, the old one
    good), 5 re-aligned to a lower identity, 15 to other rows of equal
    identity, 40 unchanged.  --force-realign then differs from the default."""
    names, seqs = synth.genome_set("small")
    o = orc.BlockSetOracle(seqs, names)
    o.apply("DraftPangenome")
    draft = o.blocks()
    outcomes = []
    got, counts = rr.realign(draft, seqs, names, outcomes=outcomes)
    tally = {w: outcomes.count(w) for w in set(outcomes)}
    print(len(draft), "blocks:", tally, counts)
    for w in ("replaced", "refused", "lower", "equal"):
        assert tally.get(w, 0) >= 1, (w, tally)
    assert counts["candidates"] == sum(counts[k] for k in ("replaced", "filter_refused", "not_better"))
    assert counts["replaced"] == tally["replaced"] and counts["filter_refused"] == tally["refused"]
    for b, g, w in zip(draft, got, outcomes):
        assert [f[:4] for f in b] == [f[:4] for f in g]
        assert (g != b) == (w == "replaced")
    forced, fcounts = rr.realign(draft, seqs, names, force=True)
    assert forced != got
    assert fcounts["replaced"] == fcounts["candidates"] == sum(1 for b in draft if len(b) >= 2)
