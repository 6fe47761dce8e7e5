"""The sequential restatement of Joiner and OriByMajority (tests/joiner_ref.py)
pinned with the reference's own known answers: every case of
src/test/joiner.cpp, OriByMajority_main of src/test/ori_by_majority.cpp and the
fixture test-script/ori_by_majority/1 (tests/golden/ori_by_majority/1)."""
import os

import pytest

import joiner_cases as jc
import joiner_ref as jr
from npge_amd import io as nio
from npge_amd.model import blockset_hash

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ori_by_majority", "1")


@pytest.mark.parametrize("name", sorted(jc.JOINER_KATS))
def test_joiner_kat(name):
    case = jc.JOINER_KATS[name]
    seqs = case["seqs"]
    blocks = jr.joiner(case["blocks"], seqs)
    if case.get("obm"):
        blocks = jr.ori_by_majority(blocks, jc.names_of(seqs))
    jc.check_kat(case, blocks, lambda b: jr.consensus_string(b, seqs))


def test_joiner_kat_rows():
    """The rows behind two of the consensus checks, written out."""
    case = jc.JOINER_KATS["Joiner_aligner"]
    assert jr.joiner(case["blocks"], case["seqs"]) == [[(0, 0, 6, 1, "ACTGAAT"), (1, 0, 5, 1, "ACT-AAT")]]
    case = jc.JOINER_KATS["Joiner_alignment_rev"]   # b2 is inverted and joined in front of b1
    assert jr.joiner(case["blocks"], case["seqs"]) == [[(0, 0, 4, -1, "CCAGT"), (1, 0, 3, -1, "CCA-T")]]


def test_ori_by_majority_main():
    """ori_by_majority.cpp:16-30."""
    assert jr.ori_by_majority([jc.OBM_TIE], ["s1"])[0][0][3] == 1
    assert jr.ori_by_majority([jc.OBM_MINORITY], ["s1"])[0][0][3] == -1


def test_ori_by_majority_fixture():
    """The tie goes to sequence a (ori 1): nothing is inverted.  The block
    hash ignores orientation, so the exact fragments are compared too."""
    src = nio.read_blockset(open(os.path.join(GOLD, "in.fasta")).read())
    exp = nio.read_blockset(open(os.path.join(GOLD, "out.fasta")).read())
    seqs = []
    for b in src.blocks:
        for f in b.fragments:
            if all(f.seq is not s for s in seqs):
                seqs.append(f.seq)
    names = [s.name for s in seqs]
    blocks = [[(names.index(f.seq.name), f.min_pos, f.max_pos, f.ori, f.row) for f in b.fragments]
              for b in src.blocks]
    got = jr.ori_by_majority(blocks, names)
    assert got == blocks
    ids = sorted(("%s_%d_%d" % ((names[q], mn, mx) if o == 1 else (names[q], mx, mn)), row)
                 for b in got for (q, mn, mx, o, row) in b)
    assert ids == sorted((f.id(), f.row) for b in exp.blocks for f in b.fragments)
    assert blockset_hash(exp.blocks) == blockset_hash(src.blocks)


def test_joiner_empty_middle_and_empty_row():
    """The hand-made case of tests/test_align_batch_gpu.py: a link whose
    between-texts are all empty joins without a middle; a link with one empty
    and one seven-base text gets seven gaps in the empty one's row."""
    from test_align_batch_gpu import SEQS, joiner_case
    st = {}
    got = jr.joiner(joiner_case(), SEQS, st)
    assert st["joins"] == 2 and st["empty_rows"] == 1
    assert got[0] == [(0, 0, 39, 1, SEQS[0][0:40]), (1, 0, 39, 1, SEQS[1][0:40])]
    assert got[1] == [(1, 100, 139, 1, SEQS[1][100:120] + "-" * 7 + SEQS[1][120:140]),
                      (2, 50, 96, 1, SEQS[2][50:97])]


def test_joiner_leaves_failed_partner_inverted():
    """try_join inverts `another` on match -1 before can_join (Joiner.cpp:221-231)
    and does not turn it back when the join then fails."""
    seqs = ["ACGTACGTACGTACGTACGT"] * 2
    one = [(0, 0, 3, 1, None), (1, 0, 3, 1, None)]
    # facing one on sequence 0 only: match -1, can_join fails
    another = [(0, 6, 9, -1, None), (1, 12, 15, -1, None)]
    between = [(1, 6, 9, 1, None), (1, 17, 18, 1, None)]
    st = {}
    got = jr.joiner([one, another, between], seqs, st)
    assert st["joins"] == 0 and st["inverted"] >= 1
    assert got[1] == jr.inverse(another)
