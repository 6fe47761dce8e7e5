"""The MoveGaps / CutGaps kernels and gap_pass at their seams, engine against
oracle bit for bit (fragments, rows, the block count and the block order; no
tolerances), and against the closed forms where gap_cases.py records one.
test_gap_cases_ref.py shows on the CPU that the inputs hold what they claim.

* k_gap_ends: first_col / last_col in 64-column ballot windows that start at
  unaligned columns (first_col(r, t, mp), last_col(r, L - mp, L - t)): tails
  and gap runs of 1, 63, 64, 65, 127, 128, 129, 200 and 201 columns, t + g on
  both sides of L // 2 - 1 at even and odd L, L = 1, 2, 3, max_tail 0 and
  max_tail >= L, rows of letters only and rows that start with a gap.
* k_move_gaps: the hand-made memmove in 64-column chunks; tails of two to
  four chunks, `from` and `to` on a 64-column seam, overlapping moves (gl < tl
  under max-tail-to-gap 5), the right tail behind a long gap run, both ends of
  one row.
* the ratio's truncated division (0.5, 0.3333).
* k_cut_counts: before / after windows up to the seams, the `inside` loop of
  loose rows (CutOp.full) over 1, 63, 64, 65 and 130 columns, rows without a
  letter, erased fragments, one-letter ori -1 fragments, from == to, from > to.
* k_gapless: the first / last gapless column at 0, 1, 63, 64, 65, 128 and
  L - 1 with L % 64 in {0, 1, 63}, one gapless column, none, 1 to 300 rows, the
  early exit `if (!__ballot(ok)) break` in the first window.
* gap_pass: four rows to a workgroup with 1, 2 or 3 rows in the last one,
  which[] against block indices (blocks without fragments among the others),
  buffers reused by a smaller set, the combined move + cut of LiteAlign /
  Align (post[r].lead = gl, post[r].trail = gr) over one and more laps.
* a seeded sweep of 150 blocks of 2 to 70 rows.
"""
import pytest

import gap_cases as gc
from test_block_build_gpu import _engine, canon

pytestmark = pytest.mark.gpu


def _eng(S):
    ss, eng = _engine(list(S.seqs), list(S.names))
    eng._ss = ss
    return eng


def _same(S, got, want, what):
    """got == want, blocks in order; a difference is named by the input
    blocks it comes from."""
    g, w = S.split(got), S.split(want)
    bad = [k for k in sorted(set(g) | set(w), key=lambda k: -1 if k is None else k)
           if (canon(g.get(k, [])) != canon(w.get(k, []))) or (k is None and len(g.get(k, [])) != len(w.get(k, [])))]
    assert not bad, "%s: %d input blocks come out otherwise, first %s" % (
        what, len(bad), [(k, S.tags[k] if k is not None else "empty", len(S.blocks[k]) if k is not None else 0)
                         for k in bad[:5]])
    assert len(got) == len(want), what
    assert got == want, what


def _closed_forms(S, got, what):
    by = S.split(got)
    for k, b in enumerate(S.blocks):
        want = S.expected(k)
        if want is not None and b:
            assert canon(by.get(k, [])) == canon(want), (what, k, S.tags[k])
    if all(e is not None for e in S.expect):
        assert len(by.get(None, [])) == S.cleared(), what


def _run(S, op, eng=None, closed=True):
    eng = eng or _eng(S)
    eng.set_blocks(S.input()).apply(S.engine_op(op))
    got = eng.blocks()
    _same(S, got, S.result(op), op)
    if closed:
        _closed_forms(S, got, op)
    return eng


def test_move_rule_edges():
    """MoveGaps --max-tail=200 --max-tail-to-gap=1: every (t, g) of the rule's
    seams moving at t + g = L // 2 - 1 and staying at L // 2, left, right and
    both ends; t = 201; one end moving while the other fails one condition."""
    S = gc.move_rule_edges()
    assert S.engine_op("MoveGaps") == "MoveGaps --max-tail=200 --max-tail-to-gap=1"
    _run(S, "MoveGaps")


def test_move_max_tail_0():
    _run(gc.move_max_tail_0(), "MoveGaps")


@pytest.mark.parametrize("name", [n for n, _ in gc.move_ratio_edges()])
def test_move_ratio_edges(name):
    """The truncated ratio at 0.5 and 0.3333; under 5 the overlapping moves
    (70, 14), (130, 26), (200, 40), (65, 13): destination over source, two to
    four chunks of k_move_gaps, on both sides."""
    _run(dict(gc.move_ratio_edges())[name], "MoveGaps")


def test_cut_edges():
    """Permissive CutGaps: leads and trails on the seams, from == to, from >
    to, letters outside [from, to], one fragment left, one-letter ori -1."""
    _run(gc.cut_edges(), "CutGaps")


@pytest.mark.parametrize("strict", [False, True])
def test_loose_edges(strict):
    """Loose rows: k_cut_counts' inside loop over 1 to 130 columns, rows
    without a letter."""
    _run(gc.loose_edges(strict), "CutGapsStrict" if strict else "CutGaps")


def test_strict_edges():
    """k_gapless' windows from both ends, 1 to 300 rows, the early exit."""
    _run(gc.strict_edges(), "CutGapsStrict")


@pytest.mark.parametrize("pipe", ["LiteAlign", "Align"])
def test_combined_edges(pipe):
    """The combined move + cut with the default max-tail 3: the moved row
    alone sets from / to; two laps; untouched blocks.  lite_align() is the
    closed form of LiteAlign; Align's Filter is the oracle's.  gap_pass
    rebuilds the blocks it cuts: blocks and fragments stay in input order."""
    _run(gc.combined_edges(), pipe, closed=pipe == "LiteAlign")


@pytest.mark.parametrize("op", ["MoveGaps", "CutGaps", "CutGapsStrict"])
def test_indexing(op):
    """Sets of 4k + 1, 4k + 2, 4k + 3 and 4k rows with blocks without
    fragments inside, then a smaller set, all on one engine: a stale GapEnd,
    MoveOp, CutOp or count of an earlier set would show in a later one."""
    S = gc.indexing()
    by_input = S.result(op)
    eng = _eng(S)
    for part in gc.parts(S):
        eng.set_blocks([list(S.blocks[k]) for k in part]).apply(S.engine_op(op))
        _same(S, eng.blocks(), [by_input[k] for k in part], "%s %s" % (op, part[-1]))


@pytest.mark.parametrize("seed", [0])
def test_sweep(seed):
    S = gc.sweep(seed)
    eng = _eng(S)
    for op in ("MoveGaps", "CutGaps", "CutGapsStrict"):
        _run(S, op, eng=eng, closed=False)
