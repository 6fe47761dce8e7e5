"""The column kernels behind FixEnds, Filter and ConSeq at the shapes where
they take another path, engine against oracle bit for bit (fragments, rows and
the block count; no tolerances).  The inputs are column_cases.py's;
test_column_cases_ref.py shows on the CPU that they hold what they claim.

* FixEnds: k_fix_ends_small against k_col_bits mode 0 + k_fix_ends on the two
  sides of SMALL_FE_WORDS (4096 columns) and SMALL_FE_ROWS (4 rows), identity
  bits in LDS (262144 columns) and read from global memory (262209), trimmed
  ends of 1, 63, 64, 65 and 128 columns, FeDir::first_good's last admissible
  start L - min_fragment, the best window within sub_frame, an odd number of
  small-path blocks.
* Filter: k_col_bits mode 1, k_fi_scores' gap runs that end at, start at and
  cross a ColTile seam (4096 columns) and touch columns 0 and L-1, runs of 999
  / 1000 / 1001 columns under min_fragment 2000, k_fi_windows' failing frame
  on both sides of a thread's 16 windows and of the tile seam and at
  L - frame_length, k_fi_ends, k_slice_counts over more than one COUNT_PIECE
  (16384 columns), slice_meta with k_set_letter (the orientation flip), job
  indices that differ from block indices.
* ConSeq: k_consensus on both sides of its 256-column tile, ties of every
  pair of letters in both row orders, N majorities, columns of gaps only,
  more rows than a wave has lanes.
* a sweep of random blocks at those lengths with 2 to 70 rows, and the
  buffers reused by a second, smaller set on the same engine.

Not here: ExtendLoopFast's device-planned, grid-stride launches of the same
kernels (elf_device.inc: the ntiles / nlist / dn arguments).  They run only
inside the device loop, on real genome sets (test_elf_device_gpu.py,
test_options_gpu.py::test_draft_pangenome_vector).
"""
import pytest

import column_cases as cc
from test_block_build_gpu import _engine, canon

pytestmark = pytest.mark.gpu


def _eng(S):
    ss, eng = _engine(list(S.seqs), list(S.names), **S.engine_kw())
    eng._ss = ss
    return eng


def _same(S, got, want, what):
    """got == want as sets of blocks and in number; a difference is named by
    the input blocks it comes from."""
    g, w = S.split(got), S.split(want)
    bad = [k for k in sorted(set(g) | set(w), key=lambda k: -1 if k is None else k)
           if canon(g.get(k, [])) != canon(w.get(k, []))]
    assert not bad, "%s: %d input blocks come out otherwise, first %s" % (
        what, len(bad), [(k, S.tags[k] if k is not None else "empty", len(S.blocks[k]) if k is not None else 0)
                         for k in bad[:5]])
    assert len(got) == len(want), what
    assert canon(got) == canon(want), what


def test_fix_ends_edges():
    S = cc.fix_ends_edges()
    want = S.result("FixEnds")
    eng = _eng(S)
    eng.set_blocks(S.input()).apply("FixEnds")
    _same(S, eng.blocks(), want, "FixEnds")


def _filter_counts(S, want):
    """filter_whole and filter_slices as the oracle's output has them: the
    blocks that come out as they went in; the scored blocks (rows, at least
    min_fragment columns and min_block fragments) that do not."""
    got = S.split(want)
    kinds = [cc.outcome(S, k, got) if b else "gone" for k, b in enumerate(S.blocks)]
    mf, mb = S.kw.get("min_fragment", 100), S.kw.get("min_block", 2)
    scored = [bool(b) and b[0][4] is not None and len(b[0][4]) >= mf and len(b) >= mb for b in S.blocks]
    whole = sum(k == "same" for k in kinds)
    sliced = sum(s and k != "same" for s, k in zip(scored, kinds)) if S.kw.get("find_subblocks", 1) else 0
    return whole, sliced, kinds


@pytest.mark.parametrize("name", [n for n, _ in cc.filter_edges()])
def test_filter_edges(name):
    S = dict(cc.filter_edges())[name]
    want = S.result("Filter")
    whole, sliced, kinds = _filter_counts(S, want)
    if name == "default":
        assert whole and "many" in kinds and "one" in kinds
    eng = _eng(S)
    eng.set_blocks(S.input()).apply("Filter")
    _same(S, eng.blocks(), want, "Filter " + name)
    c = eng.stats()["counters"]
    assert (c["filter_whole"], c["filter_slices"]) == (whole, sliced)
    if name == "flip":  # FixEnds' slice is the same column
        eng.set_blocks(S.input()).apply("FixEnds")
        assert eng.blocks() == [cc.FLIP_ANSWER]


def test_filter_edges_show_both_outcomes():
    """(the oracle's output over all groups: blocks that pass whole and blocks
    that are cut, as test_filter_edges compares them)"""
    kinds = []
    for _, S in cc.filter_edges():
        kinds += _filter_counts(S, S.result("Filter"))[2]
    assert kinds.count("same") >= 5 and kinds.count("many") >= 5


@pytest.mark.parametrize("seed", [0, 1])
def test_sweep(seed):
    S = cc.sweep(seed)
    eng = _eng(S)
    for op in ("FixEnds", "Filter"):
        eng.set_blocks(S.input()).apply(op)
        _same(S, eng.blocks(), S.result(op), "%s seed %d" % (op, seed))


def test_buffers_reused_by_a_smaller_set():
    """set_blocks(A), apply, set_blocks(B), apply on one engine: B has fewer,
    shorter blocks in another order; stale bit words, scores, counts or LDS
    would show in B's result."""
    S = cc.sweep(0)
    n = len(S.blocks)
    first = list(range(4 * len(cc.SWEEP_LENGTHS)))           # four rounds of every length
    second = list(range(n - 1, 4 * len(cc.SWEEP_LENGTHS) - 1, -1))  # the last round, backwards: up to 4160 columns
    assert max(len(S.blocks[k][0][4]) for k in second) < 4200 < 33000 == max(len(S.blocks[k][0][4]) for k in first)
    eng = _eng(S)
    for op in ("FixEnds", "Filter"):
        by_input = S.split(S.result(op))
        for part in (first, second):
            eng.set_blocks([list(S.blocks[k]) for k in part]).apply(op)
            want = [b for k in part for b in by_input.get(k, [])]
            _same(S, eng.blocks(), want, op)


def test_consensus_edges():
    S = cc.consensus_edges()
    o = S.oracle()
    o.set_blocks(S.input())
    want = o.conseq()
    eng = _eng(S)
    eng.set_blocks(S.input())
    got = eng.conseq()
    assert got == want
    assert got == [cc.vote([f[4] for f in b]) for b in S.blocks]
