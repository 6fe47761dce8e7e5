"""ReAlign and the block statistics on the engine (npgx_blockset_apply
"ReAlign", npgx_blockset_block_stats / k_col_stat): the reference's known
answer (Block_alignment_stat, src/test/block.cpp:89-143), the kernel's shapes
against the plain-Python statistics, and exact parity of blocks, rows and
outcome counters with the sequential restatement (tests/realign_ref.py)."""
import numpy as np
import pytest

import realign_ref as rr
from helpers import rows_digest
from npge_amd import io as nio
from npge_amd import synth
from npge_amd.model import Block, BlockSet, Fragment, Sequence, blockset_hash

pytestmark = pytest.mark.gpu

STAT_KEYS = ("ident_nogap", "ident_gap", "noident_nogap", "noident_gap", "pure_gap", "total", "letters")


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


def _left_packed(blocks):
    """Every row's letters first, its gaps to the right."""
    return [[(q, mn, mx, o, None if r is None else r.replace("-", "").ljust(len(r), "-"))
             for (q, mn, mx, o, r) in b] for b in blocks]


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


_REF = {}


def _ref(cfg, force=False):
    """The restatement on _draft(cfg), computed once per module."""
    if (cfg, force) not in _REF:
        seqs, names, draft = _draft(cfg)
        outcomes = []
        _REF[(cfg, force)] = rr.realign(draft, seqs, names, force=force, outcomes=outcomes) + (outcomes,)
    return _REF[(cfg, force)]


def _parity(seqs, names, blocks, force=False, exp=None):
    """ReAlign on the engine equals the restatement exactly: blocks in order,
    fragments, rows, hash, row digest and the outcome counters."""
    exp_blocks, exp_counts = exp or rr.realign(blocks, seqs, names, force=force)
    eng = _engine(seqs, names, blocks).apply("ReAlign --force-realign=1" if force else "ReAlign")
    got = eng.blocks()
    assert got == exp_blocks
    assert eng.hash() == _model_hash(exp_blocks, names)
    assert eng.rows_digest() == rows_digest(exp_blocks)
    assert eng.realign_counts() == exp_counts
    return eng, got, exp_counts


# ---------------------------------------------------------------- 1: known answer
def test_block_stats_known_answer():
    rows = ["TAGTCCG-", "TGTT-CG-", "TG---CG-"]
    seqs = ["TAGTCCG", "TGTTCG", "TGCG"]
    blocks = [[(i, 0, len(s) - 1, 1, r) for i, (s, r) in enumerate(zip(seqs, rows))]]
    st = _engine(seqs, ["a", "b", "c"], blocks).block_stats()
    assert st == [dict(ident_nogap=3, ident_gap=2, noident_nogap=1, noident_gap=1, pure_gap=1, total=8,
                       alignment_rows=3, min_fragment_length=4, letters=[1, 6, 6, 4, 0], identity_x1e4=5714)]


# ---------------------------------------------------------------- 2: shapes
SHAPES = [(1, 1), (2, 1), (2, 63), (3, 64), (2, 65), (5, 4096), (5, 4097), (65, 130), (17, 9000)]


def _random_rows(rng, n, L):
    """n gapped rows of L columns over A T G C N: gaps, pure-gap columns where
    the shape has room for them, every row with at least one letter."""
    codes = rng.choice(6, size=(n, L), p=[0.3, 0.2, 0.15, 0.1, 0.05, 0.2])
    # columns agree more often than chance: half of them copy the first row's letter
    same = rng.random((n, L)) < 0.5
    codes = np.where(same & (codes != 5), codes[0][None, :], codes)
    if L >= 3:
        codes[:, rng.choice(L, size=max(1, L // 20), replace=False)] = 5
    for i in range(n):
        if (codes[i] == 5).all():
            free = [c for c in range(L) if not (codes[:, c] == 5).all()] or [0]
            codes[i, free[i % len(free)]] = int(rng.integers(0, 5))
    return ["".join("ATGCN-"[x] for x in row) for row in codes]


def test_block_stats_shapes():
    """One tile and one column past it, a partial word, more rows than lanes, a
    block without rows in the middle: every job's counters against the
    plain-Python statistics."""
    rng = np.random.default_rng(11)
    seqs, blocks = [], []
    for (n, L) in SHAPES:
        rows = _random_rows(rng, n, L)
        if (n, L) == (5, 4097):
            rows = [r[:-1] + "ANN-C"[i] for i, r in enumerate(rows)]  # the lone column of the second tile
        b = []
        for r in rows:
            seqs.append(r.replace("-", ""))
            b.append((len(seqs) - 1, 0, len(seqs[-1]) - 1, 1, r))
        blocks.append(b)
        if (n, L) == (2, 65):
            blocks.append([(0, 0, 0, 1, None), (1, 0, 0, 1, None)])
    names = ["q%d" % i for i in range(len(seqs))]
    got = _engine(seqs, names, blocks).block_stats()
    assert len(got) == len(blocks) == len(SHAPES) + 1
    seen_classes = set()
    for b, g in zip(blocks, got):
        if b[0][4] is None:
            assert g == dict(ident_nogap=0, ident_gap=0, noident_nogap=0, noident_gap=0, pure_gap=0, total=-1,
                             alignment_rows=0, min_fragment_length=1, letters=[0] * 5, identity_x1e4=0)
            continue
        exp = rr.block_stat(b)
        assert g == exp, (len(b), len(b[0][4]))
        seen_classes |= {k for k in STAT_KEYS[:5] if exp[k]}
        assert sum(exp[k] for k in STAT_KEYS[:5]) == exp["total"]
    assert seen_classes == set(STAT_KEYS[:5])


# ---------------------------------------------------------------- 3: parity on small
def test_realign_parity_small():
    seqs, names, draft = _draft("small")
    exp_blocks, exp_counts, outcomes = _ref("small")
    print("small:", len(draft), "blocks", {w: outcomes.count(w) for w in sorted(set(outcomes))}, exp_counts)
    _, got, _ = _parity(seqs, names, draft, exp=(exp_blocks, exp_counts))
    assert exp_counts["replaced"] >= 1 and exp_counts["not_better"] >= 1
    for b, g, w in zip(draft, got, outcomes):
        if w != "replaced":
            assert g == b  # the blocks the restatement leaves alone keep their rows


def test_block_stats_on_small():
    """block_stats() of a natural set: every block against the plain-Python
    statistics, before and after ReAlign (a replaced block's identity grew)."""
    seqs, names, draft = _draft("small")
    exp_blocks, _, outcomes = _ref("small")
    eng = _engine(seqs, names, draft)
    before = eng.block_stats()
    assert before == [rr.block_stat(b) for b in draft]
    after = eng.apply("ReAlign").block_stats()
    assert after == [rr.block_stat(b) for b in exp_blocks]
    for x, y, w in zip(before, after, outcomes):
        assert (y["identity_x1e4"] > x["identity_x1e4"]) == (w == "replaced")


# ---------------------------------------------------------------- 4: left-packed rows
def test_realign_left_packed_tiny():
    seqs, names, draft = _draft("tiny")
    _, _, counts = _parity(seqs, names, _left_packed(draft))
    print("tiny left-packed:", len(draft), "blocks", counts)
    assert counts["replaced"] >= 1


# ---------------------------------------------------------------- 5: wide
def test_realign_wide():
    """One block of 66 fragments (more than 64 non-empty rows: the
    workgroup-per-problem aligner), rows left-packed."""
    rng = np.random.default_rng(66)
    root = rng.integers(0, 4, 300)
    seqs = []
    for i in range(66):
        s = root.copy()
        hit = rng.random(300) < 0.02
        s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        s = list(s)
        if i % 3 == 0:
            at, n = int(rng.integers(10, 280)), int(rng.integers(1, 6))
            del s[at:at + n]
        seqs.append("".join("ATGC"[x] for x in s))
    L = max(len(s) for s in seqs)
    blocks = [[(i, 0, len(s) - 1, 1, s.ljust(L, "-")) for i, s in enumerate(seqs)]]
    names = ["w%d" % i for i in range(66)]
    exp = rr.realign(blocks, seqs, names)
    print("wide: identity", rr.block_stat(blocks[0])["identity_x1e4"], "->",
          rr.block_stat(rr.align_block(blocks[0], seqs))["identity_x1e4"], exp[1])
    eng, _, counts = _parity(seqs, names, blocks, exp=exp)
    assert counts == dict(candidates=1, replaced=1, filter_refused=0, not_better=0)
    assert any(k["name"] == "align_wide" for k in eng.kernel_times())


# ---------------------------------------------------------------- 6: four block kinds
def test_realign_mixed_kinds():
    seqs, names, draft = _draft("tiny")
    packed = _left_packed(draft)
    aligned = next(b for b in packed if len(b) == 3)
    bare3 = next([(q, mn, mx, o, None) for (q, mn, mx, o, _) in b] for b in reversed(draft) if len(b) == 3)
    one_bare = [(0, 5, 204, 1, None)]
    one_row = [(1, 10, 109, -1, rr._text(seqs, 1, 10, 109, -1))]
    assert aligned[0][:4] != bare3[0][:4]
    blocks = [one_bare, one_row, bare3, aligned]
    meta = _engine(seqs, names, blocks).apply("MetaAligner").blocks()
    eng, got, counts = _parity(seqs, names, blocks)
    assert got[:3] == meta[:3] and meta[3] == aligned
    assert got[0][0][4] == seqs[0][5:205] and got[1] == one_row
    assert all(f[4] is not None for f in got[2])
    assert counts["candidates"] == 1
    assert got[3] == rr.realign([aligned], seqs, names)[0][0]


def test_realign_leaves_empty_blocks():
    seqs, names, draft = _draft("tiny")
    blocks = [[], _left_packed(draft[:1])[0], []]
    got = _engine(seqs, names, blocks).apply("ReAlign").blocks()
    assert got == rr.realign(blocks, seqs, names)[0] and got[0] == [] and got[2] == []


# ---------------------------------------------------------------- 7: force
def test_realign_force_small():
    seqs, names, draft = _draft("small")
    exp_blocks, exp_counts, _ = _ref("small", force=True)
    _parity(seqs, names, draft, force=True, exp=(exp_blocks, exp_counts))
    assert exp_blocks != _ref("small")[0]
    assert exp_counts["replaced"] == exp_counts["candidates"] == sum(1 for b in draft if len(b) >= 2)


# ---------------------------------------------------------------- 8: script runner
@pytest.mark.parametrize("opts,force", [("", False), ("--force-realign=1", True)])
def test_realign_script(opts, force):
    from npge_amd.script import run_script
    seqs, names, draft = _draft("tiny")
    packed = _left_packed(draft)
    bs = BlockSet()
    bs.seqs = [Sequence(n, s) for n, s in zip(names, seqs)]
    bs.blocks = [Block([Fragment(bs.seqs[q], mn, mx, o, r) for (q, mn, mx, o, r) in b], name="blk%03d" % i)
                 for i, b in enumerate(packed)]
    call = "run('ReAlign', '%s')" % opts if opts else "run('ReAlign')"
    out = run_script("run_main('Read')\n%s\nrun_main('RawWrite')\n" % call, nio.write_blockset(bs))
    eng = _engine(seqs, names, packed).apply("ReAlign --force-realign=%d" % force)
    got = [[(names.index(f.seq.name), f.min_pos, f.max_pos, f.ori, f.row) for f in b.fragments]
           for b in out.blocks]
    assert got == eng.blocks()
    assert got != packed
    assert [b.name for b in out.blocks] == ["blk%03d" % i for i in range(len(packed))]


# ---------------------------------------------------------------- 9: state, timers
def test_realign_counts_before_any_realign():
    from npge_amd import _capi
    seqs, names, draft = _draft("tiny")
    eng = _engine(seqs, names, draft[:2])
    with pytest.raises(_capi.NpgxError) as e:
        eng.realign_counts()
    assert e.value.code == -5  # NPGX_ERR_STATE
    eng.apply("MetaAligner")
    with pytest.raises(_capi.NpgxError):
        eng.realign_counts()
    assert eng.apply("ReAlign").realign_counts()["candidates"] == 2


def test_realign_unknown_option():
    from npge_amd import _capi
    seqs, names, draft = _draft("tiny")
    eng = _engine(seqs, names, draft[:1])
    with pytest.raises(_capi.NpgxError) as e:
        eng.apply("ReAlign --force-realign=maybe")
    assert e.value.code == -1  # NPGX_ERR_ARG
    assert eng.blocks() == draft[:1]


def test_realign_in_kernel_times(monkeypatch):
    """With every launch timed, kernel_times() shows the decode, the aligner,
    k_refine, k_col_stat and the Filter kernels of the last ReAlign."""
    monkeypatch.setenv("NPGX_TIMERS", "2")
    seqs, names, draft = _draft("tiny")
    packed = _left_packed(draft)
    eng = _engine(seqs, names, packed).apply("ReAlign")
    kt = {k["name"]: k for k in eng.kernel_times()}
    assert {"decode_rows", "align_jobs", "refine_alignment", "col_stat", "filter_columns"} <= set(kt)
    new_len = [len(b[0][4]) for b in rr.realign(packed, seqs, names, force=True)[0]]
    cells = sum(len(b) * (len(b[0][4]) + n) for b, n in zip(packed, new_len))
    assert kt["col_stat"]["units"] == cells  # the old and the new rows of every candidate, once
