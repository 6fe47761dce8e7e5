"""Joiner and OriByMajority on the engine (npgx_blockset_apply "Joiner" /
"OriByMajority"): the reference's known answers (src/test/joiner.cpp,
src/test/ori_by_majority.cpp, test-script/ori_by_majority), exact parity of
blocks, fragment order, oris and rows with the sequential restatement
(tests/joiner_ref.py) on DraftPangenome results, and the edges of k_join_rows."""
import os

import numpy as np
import pytest

import joiner_cases as jc
import joiner_ref as jr
from helpers import rows_digest
from npge_amd import io as nio
from npge_amd import synth
from npge_amd.model import Block, Fragment, Sequence, blockset_hash

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ori_by_majority", "1")
TILE = 8192  # output bytes per k_join_rows workgroup (PIECE, block_build.hip)


def _engine(seqs, names, blocks=None):
    from npge_amd import _capi
    from npge_amd.blockset import BlockSetEngine
    eng = BlockSetEngine(_capi.SeqSet(seqs, names))
    if blocks is not None:
        eng.set_blocks(blocks)
    return eng


def _model_hash(blocks, names):
    seqs = [Sequence(n, "") for n in names]
    return blockset_hash([Block([Fragment(seqs[q], mn, mx, o) for (q, mn, mx, o, _) in b]) for b in blocks])


def _parity(seqs, names, blocks, stats=None):
    """Joiner on the engine equals the restatement exactly; returns (engine, blocks)."""
    exp = jr.joiner(blocks, seqs, stats)
    eng = _engine(seqs, names, blocks).apply("Joiner")
    got = eng.blocks()
    assert got == exp
    assert eng.hash() == _model_hash(exp, names)
    assert eng.rows_digest() == rows_digest(exp)
    return eng, got


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


def _odd_inverted(blocks):
    return [jr.inverse(b) if i % 2 else b for i, b in enumerate(blocks)]


# ---------------------------------------------------------------- (a) known answers
@pytest.mark.parametrize("name", sorted(jc.JOINER_KATS))
def test_joiner_kat(name):
    case = jc.JOINER_KATS[name]
    seqs, names = case["seqs"], jc.names_of(case["seqs"])
    eng = _engine(seqs, names, case["blocks"]).apply("Joiner")
    if case.get("obm"):
        eng.apply("OriByMajority")
    blocks = eng.blocks()
    cons = eng.conseq()
    jc.check_kat(case, blocks, lambda b: cons[blocks.index(b)])
    exp = jr.joiner(case["blocks"], seqs)
    assert blocks == (jr.ori_by_majority(exp, names) if case.get("obm") else exp)


def test_ori_by_majority_main():
    """ori_by_majority.cpp:16-30."""
    seqs, names = [jc.OBM_SEQ], ["s1"]
    assert _engine(seqs, names, [jc.OBM_TIE]).apply("OriByMajority").blocks() == [jc.OBM_TIE]
    got = _engine(seqs, names, [jc.OBM_MINORITY]).apply("OriByMajority").blocks()
    assert got[0][0][3] == -1
    assert got == [jr.inverse(jc.OBM_MINORITY)]


# ---------------------------------------------------------------- (b) fixture
def test_ori_by_majority_fixture():
    from npge_amd.script import output_hash, run_script
    out = run_script("run_main('Read')\nrun('OriByMajority')\nrun_main('RawWrite', '--skip-rest:=1')\n",
                     open(os.path.join(GOLD, "in.fasta")).read())
    exp = nio.read_blockset(open(os.path.join(GOLD, "out.fasta")).read())
    assert output_hash(out) == blockset_hash(exp.blocks)
    # the block hash ignores orientation: the exact fragments (the tie goes to a, ori 1: nothing inverted)
    assert [(b.name, [(f.id(), f.row) for f in b.fragments]) for b in out.blocks] == \
        [(b.name, [(f.id(), f.row) for f in b.fragments]) for b in exp.blocks]


# ---------------------------------------------------------------- (c) parity on DraftPangenome results
_PARITY_STATS = {}


@pytest.mark.parametrize("cfg", ["tiny", "rtiny"])
def test_joiner_parity_draft(cfg):
    seqs, names, draft = _draft(cfg)
    st = {}
    eng, got = _parity(seqs, names, _odd_inverted(draft), st)
    print(cfg, "blocks %d -> %d" % (len(draft), len(got)), st, eng.stats()["align_jobs"])
    _PARITY_STATS[cfg] = st
    assert st["joins"] >= 3
    if cfg == "rtiny":
        assert st["empty_rows"] >= 1
    assert st["flipped_joins"] >= 1  # match -1: the partner's rows go in as flipped segments
    assert any(len(b[0][4]) > TILE for b in got)
    assert eng.stats()["align_jobs"] >= 1 and eng.stats()["aligned_residues"] > 0


def test_joiner_parity_chain():
    """On at least one set the restatement builds a chain of three blocks or more."""
    for cfg in ("tiny", "rtiny"):
        if cfg not in _PARITY_STATS:
            seqs, _, draft = _draft(cfg)
            _PARITY_STATS[cfg] = {}
            jr.joiner(_odd_inverted(draft), seqs, _PARITY_STATS[cfg])
    assert max(st["max_chain"] for st in _PARITY_STATS.values()) >= 3


def test_second_joiner_changes_nothing():
    seqs, names, draft = _draft("tiny")
    eng = _engine(seqs, names, _odd_inverted(draft)).apply("Joiner")
    once = eng.blocks()
    assert len(once) < len(draft)
    assert eng.apply("Joiner").blocks() == once


# ---------------------------------------------------------------- (d) unaligned and mixed
def test_joiner_unaligned():
    seqs, names, draft = _draft("tiny")
    bare = [[(q, mn, mx, o, None) for (q, mn, mx, o, _) in b] for b in _odd_inverted(draft)]
    st = {}
    _, got = _parity(seqs, names, bare, st)
    assert st["joins"] >= 3 and all(f[4] is None for b in got for f in b)


def test_joiner_rows_on_one_block_only():
    case = jc.JOINER_KATS["Joiner_aligner"]
    seqs, names = case["seqs"], jc.names_of(case["seqs"])
    b1, b2 = case["blocks"]
    mixed = [b1, [(q, mn, mx, o, None) for (q, mn, mx, o, _) in b2]]
    _, got = _parity(seqs, names, mixed)
    assert got == [[(0, 0, 6, 1, None), (1, 0, 5, 1, None)]]


def test_joiner_leaves_failed_partner_inverted():
    """try_join inverts `another` on match -1 and leaves it so when the join
    then fails (Joiner.cpp:221-231): its rows come back reverse-complemented."""
    s = "ACGTTGCAAGCTTAGCCGATATCGGA"
    seqs, names = [s, s], ["p1", "p2"]
    one = [(0, 0, 3, 1, s[0:4]), (1, 0, 3, 1, s[0:4])]
    another = [(0, 6, 9, -1, jr.revcomp(s[6:10])), (1, 12, 15, -1, jr.revcomp(s[12:16]))]  # faces one on p1 only
    between = [(1, 6, 9, 1, s[6:10]), (1, 17, 18, 1, s[17:19] + "--")]
    st = {}
    _, got = _parity(seqs, names, [one, another, between], st)
    assert st["joins"] == 0 and st["inverted"] == 1
    assert got == [one, jr.inverse(another), between]


# ---------------------------------------------------------------- (e) wide
@pytest.mark.parametrize("n", [65, 66])
def test_joiner_wide_middle(n):
    """65 fragments a block, one of them with nothing between: a middle of 65
    rows.  The aligner counts non-empty rows, so the 64 of that job stay with
    the wave kernel; with 66 fragments the 65 non-empty rows are a wide job
    (more than 64: the workgroup-per-problem aligner)."""
    rng = np.random.default_rng(5)
    anc = "".join("ATGC"[x] for x in rng.integers(0, 4, 9))
    left = "".join("ATGC"[x] for x in rng.integers(0, 4, 24))
    right = "".join("ATGC"[x] for x in rng.integers(0, 4, 27))
    seqs, b1, b2 = [], [], []
    for i in range(n):
        g = 0 if i == 7 else 5 + i % 5
        mid = list(anc[:g])
        if g and i % 3 == 0:
            mid[int(rng.integers(0, g))] = "ATGC"[int(rng.integers(0, 4))]
        seqs.append(left + "".join(mid) + right)
        b1.append((i, 0, 23, 1, left))
        b2.append((i, 24 + g, 50 + g, 1, right))
    names = ["w%d" % i for i in range(n)]
    st = {}
    eng, got = _parity(seqs, names, [b1, b2], st)
    assert st["joins"] == 1 and st["empty_rows"] == 1 and len(got) == 1 and len(got[0]) == n
    assert eng.stats()["align_jobs"] == 1
    assert any(k["name"] == "align_wide" for k in eng.kernel_times()) == (n > 65)


def test_join_rows_in_kernel_times(monkeypatch):
    """With every launch timed, kernel_times() shows the decode, the aligner
    and k_join_rows of the last apply."""
    monkeypatch.setenv("NPGX_TIMERS", "2")
    case = jc.JOINER_KATS["Joiner_aligner"]
    eng = _engine(case["seqs"], jc.names_of(case["seqs"]), case["blocks"]).apply("Joiner")
    kt = {k["name"]: k for k in eng.kernel_times()}
    assert {"decode_rows", "align_jobs", "join_rows"} <= set(kt)
    assert kt["join_rows"]["units"] == 2 * len("ACTGAAT")
    st = eng.stats()
    assert st["align_jobs"] == 1 and st["aligned_residues"] == len("TGA") + len("TA") and st["ms_align"] > 0


# ---------------------------------------------------------------- (f) kernel edges
def _pair(rng, n1, gaps, n2, inv2=False):
    """Two blocks of len(gaps) rows that face each other over `gaps` bases;
    rows are the fragments' texts with a shared gap column block inside."""
    seqs, b1, b2 = [], [], []
    for i, g in enumerate(gaps):
        s = "".join("ATGCN"[x] for x in rng.integers(0, 5, n1 + g + n2))
        seqs.append(s)
        a, c = s[:n1], s[n1 + g:]
        b1.append((i, 0, n1 - 1, 1, a[:n1 // 2] + "--" + a[n1 // 2:]))
        b2.append((i, n1 + g, n1 + g + n2 - 1, 1, c[:3] + "-" + c[3:]))
    return seqs, ["e%d" % i for i in range(len(gaps))], [b1, jr.inverse(b2) if inv2 else b2]


@pytest.mark.parametrize("n1,n2,inv2", [(TILE + 900, TILE + 77, False), (2 * TILE + 5, 300, True)])
def test_join_rows_longer_than_a_tile(n1, n2, inv2):
    seqs, names, blocks = _pair(np.random.default_rng(n1), n1, [4, 0, 9], n2, inv2)
    st = {}
    _, got = _parity(seqs, names, blocks, st)
    assert st["joins"] == 1 and len(got[0][0][4]) > 2 * TILE


@pytest.mark.parametrize("n1,gaps,n2", [(37, [5, 3], 21), (16, [1, 1], 15), (3, [0, 2], 50), (31, [0, 0], 33)])
def test_join_rows_length_not_a_multiple_of_16(n1, gaps, n2):
    for inv2 in (False, True):
        seqs, names, blocks = _pair(np.random.default_rng(n2), n1, gaps, n2, inv2)
        st = {}
        _, got = _parity(seqs, names, blocks, st)
        assert st["joins"] == 1 and len(got[0][0][4]) % 16 != 0


def test_ori_by_majority_rows_with_gap_ends():
    """Rows that begin and end with gaps, against Python's reverse complement;
    a block without rows flips only its oris; the majority block stays."""
    rng = np.random.default_rng(3)
    s = ["".join("ATGCN"[x] for x in rng.integers(0, 5, 120)) for _ in range(2)]
    inv = [(0, 10, 59, -1, "---" + jr.revcomp(s[0][10:60]) + "--"),
           (1, 5, 49, -1, "-" + jr.revcomp(s[1][5:50])[:20] + "-----" + jr.revcomp(s[1][5:50])[20:] + "----")]
    keep = [(0, 70, 99, 1, s[0][70:100]), (1, 70, 99, 1, s[1][70:100])]
    bare = [(0, 100, 109, -1, None), (1, 100, 109, -1, None)]
    blocks = [inv, keep, bare]
    names = ["g0", "g1"]
    eng = _engine(s, names, blocks).apply("OriByMajority")
    got = eng.blocks()
    assert got == [jr.inverse(inv), keep, jr.inverse(bare)]
    assert got == jr.ori_by_majority(blocks, names)
    assert eng.rows_digest() == rows_digest(got)


# ---------------------------------------------------------------- (g) errors
def test_joiner_overlapping_facing_fragments():
    from npge_amd import _capi
    seqs = ["ACGTTGCAAGCTTAGCCGATATCGGA" * 2] * 2
    blocks = [[(0, 0, 9, 1, None), (1, 0, 9, 1, None)], [(0, 8, 17, 1, None), (1, 12, 20, 1, None)]]
    with pytest.raises(jr.JoinOverlap):
        jr.joiner(blocks, seqs)
    eng = _engine(seqs, ["o1", "o2"], blocks)
    with pytest.raises(_capi.NpgxError) as e:
        eng.apply("Joiner")
    assert e.value.code == -1 and "o1_0_9" in str(e.value) and "o1_8_17" in str(e.value)  # NPGX_ERR_ARG
    assert eng.blocks() == blocks
