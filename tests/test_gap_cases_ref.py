"""The oracle alone over gap_cases.py, on the CPU: what keeps
test_gap_shapes_gpu.py from being vacuous.

* every closed form (move_row, the spans handed to add_cut with cut_block,
  lite_align) is the oracle's MoveGaps / CutGaps / CutGapsStrict / LiteAlign;
* every rule edge is there on both sides: each (t, g) moves at t + g =
  L // 2 - 1 and stays at L // 2, and for the conditions on t, on the ratio and
  on t + g a row moves and a row stays for that condition alone (g >= 1 cannot
  fail alone, see gap_cases);
* the cut families hold their cases: every seam as `from` and as `to`, erased
  fragments, one-letter ori -1 fragments, cleared blocks, loose rows whose
  letters inside [from, to] are fewer than their fragment says;
* the sweep's outcome counts, from the oracle's output.
"""
import collections

import pytest

import gap_cases as gc


def canon(blocks):
    return sorted(tuple(sorted(b)) for b in blocks)


def _check(S, op):
    """Every recorded expectation is the oracle's output; the cleared blocks
    are as many as expected.  Returns split(output)."""
    out = S.result(op)
    got = S.split(out)
    known = 0
    for k, b in enumerate(S.blocks):
        want = S.expected(k)
        if want is None or not b:
            continue
        assert canon(got.get(k, [])) == canon(want), (op, k, S.tags[k])
        known += 1
    assert known
    if all(e is not None for e in S.expect):
        assert len(got.get(None, [])) == S.cleared(), op
        assert len(out) == len(S.blocks)  # a cleared block stays in the set
    return got


# ---------------------------------------------------------------- MoveGaps
def _edge_outcomes(S):
    """Per "edge" block: rows 0 (left case) and 1 (right case) move as meta
    says, in the oracle's output."""
    out = S.result("MoveGaps")
    n = collections.Counter()
    for k, m in enumerate(S.meta):
        if not m or m[0] != "edge":
            continue
        _, t, g, moves = m
        rows0, rows1 = [f[4] for f in S.blocks[k]], [f[4] for f in out[k]]
        L = len(rows0[0])
        assert all(gc.conditions(t, g, L, S.max_tail, S.x1e4)) == moves
        left, right = gc.moved_ends([S.blocks[k][:1]], [out[k][:1]]), gc.moved_ends([S.blocks[k][1:2]], [out[k][1:2]])
        assert left == (int(moves), 0) and right == (0, int(moves)), S.tags[k]
        if moves:
            assert rows1[0] == "-" * g + rows0[0][:t] + rows0[0][t + g:]
            assert rows1[1] == rows0[1][:L - t - g] + rows0[1][L - t:] + "-" * g
            if len(rows0) > 3:  # both ends
                assert gc.moved_ends([S.blocks[k][2:3]], [out[k][2:3]]) == (1, 1)
        n[(t, g, moves, L % 2)] += 1
    return n


def test_move_rule_edges():
    """max_tail 200, ratio 1: the closed forms, every (t, g) moving and
    staying at even and odd L on both sides, t = 201 never."""
    S = gc.move_rule_edges()
    _check(S, "MoveGaps")
    n = _edge_outcomes(S)
    for t, g in gc._rule_pairs():
        for odd in (0, 1):
            assert n[(t, g, False, odd)] >= 1
            assert n[(t, g, t <= 200, odd)] >= 1 and (t <= 200 or not n[(t, g, True, odd)])
    assert {t for t, g in gc._rule_pairs()} == set(gc.RULE_T)
    assert {g for t, g in gc._rule_pairs() if g != t} == set(gc.RULE_G)
    # one end moves, the other fails one condition alone
    out = S.result("MoveGaps")
    alone = set()
    for k, m in enumerate(S.meta):
        if not m or m[0] != "one_fails":
            continue
        _, side, i, (t, g) = m
        L = len(S.blocks[k][0][4])
        c = gc.conditions(t, g, L, S.max_tail, S.x1e4)
        assert [j for j in range(4) if not c[j]] == [i], (S.tags[k], c)
        assert gc.moved_ends([S.blocks[k][:1]], [out[k][:1]]) == ((0, 1) if side == "left" else (1, 0)), S.tags[k]
        alone.add((side, i))
    assert alone == {(s, i) for s in ("left", "right") for i in (0, 2, 3)}
    # t = 201 before 201 gaps in a row long enough: the count of letters alone refuses it
    assert any(m and m[0] == "edge" and m[1:3] == (201, 201) and
               gc.conditions(201, 201, len(S.blocks[k][0][4]), 200, 10000) == (False, True, True, True)
               for k, m in enumerate(S.meta))
    tags = set(S.tags)
    assert {"starts with gap", "letters only", "L1", "L2", "L3", "L2 gap", "L3 gap", "max_tail >= L"} <= tags
    k = S.tags.index("max_tail >= L")
    assert [gc.move_row(f[4], 200, 10000)[1:] for f in S.blocks[k]] == [(False, False), (True, False), (False, False),
                                                                        (True, False)]
    assert max(len(b[0][4]) for b in S.blocks) <= 900


def test_move_max_tail_0():
    S = gc.move_max_tail_0()
    _check(S, "MoveGaps")
    assert S.result("MoveGaps") == S.input()


@pytest.mark.parametrize("name", [n for n, _ in gc.move_ratio_edges()])
def test_move_ratio_edges(name):
    """0.5: (32, 64) moves, (33, 64) stays; 0.3333: (1, 3) moves, (2, 5)
    stays; 5: the overlapping moves, tails of two to four 64-column chunks."""
    S = dict(gc.move_ratio_edges())[name]
    _check(S, "MoveGaps")
    n = _edge_outcomes(S)
    moved = {(t, g) for (t, g, moves, _), c in n.items() if moves and c}
    stayed = {(t, g) for (t, g, moves, _), c in n.items() if not moves and c}
    want = {"0.5": ({(32, 64)}, {(33, 64)}), "0.3333": ({(1, 3)}, {(2, 5)}),
            "5": (set(gc.OVERLAPPING), {(71, 14)})}[name]
    assert (moved, stayed) == want
    if name == "5":
        assert all(g < t for t, g in moved) and {(t + 63) // 64 for t, g in moved} == {2, 3, 4}
    assert S.engine_op("MoveGaps") == "MoveGaps --max-tail=200 --max-tail-to-gap=" + name
    assert gc.move_rule_edges().engine_op("MoveGaps") == "MoveGaps --max-tail=200 --max-tail-to-gap=1"


def _chunked_move(row, t, g, descending=True, chunks=None):
    """k_move_gaps' left move restated: the tail copied g columns to the
    right in 64-column chunks from its end backwards, each chunk read before
    it is written, then g gaps.  descending=False and chunks=1 are the two
    ways to get it wrong that the inputs must tell apart."""
    r = list(row)
    his = list(range(t, 0, -64))
    for hi in (his if descending else his[::-1])[:chunks]:
        lo = max(hi - 64, 0)
        r[lo + g:hi + g] = r[lo:hi]
    r[:g] = "-" * g
    return "".join(r)


def test_inputs_tell_a_wrong_memmove_apart():
    """On every moving edge row the chunked copy is the oracle's row, on both
    sides; a copy that stops after one chunk differs for every tail of more
    than 64 letters, and a copy in ascending chunks for every overlapping
    move (gl < tl) of more than one chunk."""
    one_chunk, ascending = set(), set()
    for S in (gc.move_rule_edges(),) + tuple(s for _, s in gc.move_ratio_edges()):
        out = S.result("MoveGaps")
        for k, m in enumerate(S.meta):
            if not m or m[0] != "edge" or not m[3]:
                continue
            _, t, g, _ = m
            for side, i in (("left", 0), ("right", 1)):
                row, want = S.blocks[k][i][4], out[k][i][4]
                if side == "right":
                    row, want = row[::-1], want[::-1]
                assert _chunked_move(row, t, g) == want
                if t > 64:
                    assert _chunked_move(row, t, g, chunks=1) != want
                    one_chunk.add((side, (t + 63) // 64))
                if t > 64 and g < t:
                    assert _chunked_move(row, t, g, descending=False) != want
                    ascending.add((side, t, g))
    assert one_chunk == {(s, n) for s in ("left", "right") for n in (2, 3, 4)}
    assert ascending == {(s, t, g) for s in ("left", "right") for t, g in gc.OVERLAPPING}


# ---------------------------------------------------------------- CutGaps
def _erased(S, got):
    """Fragments erased per block against meta, where meta counts them."""
    n = 0
    for k, m in enumerate(S.meta):
        if isinstance(m, int) and S.expect[k][0] == "cut":
            (b,) = got[k]
            assert len(S.blocks[k]) - len(b) == m, S.tags[k]
            n += m
    return n


def test_cut_edges():
    S = gc.cut_edges()
    got = _check(S, "CutGaps")
    assert _erased(S, got) >= 5
    spans = [e[1:] + (len(b[0][4]),) for b, e in zip(S.blocks, S.expect) if e[0] == "cut"]
    assert {a for a, b, L in spans} >= set(gc.SEAMS) and {L - 1 - b for a, b, L in spans} >= set(gc.SEAMS)
    assert any(a == b for a, b, L in spans)
    assert S.cleared() == 3 and "from > to" in S.tags
    (b,) = got[S.tags.index("outside, one fragment left")]
    assert len(b) == 1
    (b,) = got[S.tags.index("cut down to one fragment")]
    assert len(b) == 1
    (b,) = got[S.tags.index("one letter ori -1")]
    assert sorted((f[3], f[4].replace("-", "")) for f in b if f[1] == f[2]) == [(-1, "G"), (-1, "T")]
    (b,) = got[S.tags.index("outside")]
    assert [f[4] for f in b] == ["CCGATC", "CATGAT"]


@pytest.mark.parametrize("strict", [False, True])
def test_loose_edges(strict):
    S = gc.loose_edges(strict)
    got = _check(S, "CutGapsStrict" if strict else "CutGaps")
    widths = set()
    short = 0
    for k, e in enumerate(S.expect):
        if e[0] != "cut":
            continue
        widths.add(e[2] - e[1] + 1)
        (b,) = got[k]
        for f in b:  # the letters of the row, not the fragment's length less the cut
            assert f[2] - f[1] + 1 == len(f[4].replace("-", ""))
        short += sum(f0[2] - f0[1] + 1 > len(f0[4].replace("-", "")) for f0 in S.blocks[k])
    assert widths >= set(gc.LOOSE_WIDTHS) and short >= 40
    if strict:
        assert S.cleared() == 1
    else:
        assert _erased(S, got) >= 20
        assert sum(not f[4].strip("-") for b in S.blocks for f in b) >= 10  # rows without a letter


def test_strict_edges():
    S = gc.strict_edges()
    _check(S, "CutGapsStrict")
    spans = [(e[1], e[2], len(b[0][4]), len(b)) for b, e in zip(S.blocks, S.expect) if b and e[0] == "cut"]
    for L in (256, 257, 319):
        assert {a for a, b, l, n in spans if l == L} >= {0, 1, 63, 64, 65, 128, L - 1}
        assert {l - 1 - b for a, b, l, n in spans if l == L} >= {0, 1, 63, 64, 65, 128, L - 1}
        assert {a for a, b, l, n in spans if l == L and a == b} >= {0, 1, 63, 64, 65, 128, L - 1}
    assert {256 % 64, 257 % 64, 319 % 64} == {0, 1, 63}
    assert any(a > 63 and n > 64 for a, b, l, n in spans)  # past the first window in a block of more than 64 rows
    assert {len(b) for b in S.blocks if b} >= set(gc.STRICT_ROWS)
    assert max(len(b[0][4]) for b in S.blocks if len(b) == 300) <= 200
    assert S.cleared() == 1 + 4  # the empty block, "strict none" at 2, 64, 65 and 300 rows
    for k, t in enumerate(S.tags):
        if t.startswith("early exit"):
            rows = [f[4] for f in S.blocks[k]]
            L = len(rows[0])
            assert set(rows[0][:64]) == set(rows[0][L - 64:]) == {"-"} and S.expect[k] == ("cut", 70, L - 71)


# ---------------------------------------------------------------- the combined pass
def test_combined_edges():
    """lite_align() is the oracle's LiteAlign; Align (with its Filter) keeps
    the blocks it was given to keep."""
    S = gc.combined_edges()
    _check(S, "LiteAlign")
    laps = collections.Counter(m for m in S.meta if m is not None)
    assert laps[0] >= 2 and laps[1] >= 45 and laps[2] >= 6
    seen = set()
    for t in S.tags:
        if t.startswith("combined"):
            _, side, tt, g = t.split()
            seen.add((side, int(g[1:])))
    assert seen == {(s, g) for s in ("left", "right", "both") for g in gc.COMBINED_G}
    got = S.split(S.result("Align"))
    assert sum(1 for k, b in enumerate(S.blocks) if b and got.get(k)) >= len(S.blocks) // 2
    # both pipes keep blocks and fragments in input order (the GPU file compares the order too); LiteAlign keeps the
    # empty block, Align drops it
    for pipe, n in (("LiteAlign", len(S.blocks)), ("Align", len(S.blocks) - 1)):
        out = S.result(pipe)
        ids = [[f[0] for f in b] for b in out]
        assert len(out) == n and ids == [[f[0] for f in b] for b in S.blocks if b or pipe == "LiteAlign"], pipe


# ---------------------------------------------------------------- indexing
def test_indexing_parts():
    S = gc.indexing()
    ps = gc.parts(S)
    assert {sum(len(S.blocks[k]) for k in p) % 4 for p in ps[:-1]} == {0, 1, 2, 3}
    for p in ps[:-1]:
        empties = [k for k in p if not S.blocks[k]]
        assert empties and empties[0] < p[-1]  # rows after an empty block
    assert len(ps[-1]) < min(len(p) for p in ps[:-1])
    for op in ("MoveGaps", "CutGaps", "CutGapsStrict"):
        out = S.result(op)
        changed = sum(a != b for a, b in zip(S.input(), out))
        assert changed >= len([b for b in S.blocks if b]) - 1, op


# ---------------------------------------------------------------- sweep
def sweep_counts(S):
    left, right = gc.moved_ends(S.input(), S.result("MoveGaps"))
    res = {"moved left": left, "moved right": right}
    for op, name in (("CutGaps", "permissive"), ("CutGapsStrict", "strict")):
        got = S.split(S.result(op))
        cut = [k for k, b in enumerate(S.blocks) if b and got.get(k) and got[k] != [b]]
        res[name + " cut"] = len(cut)
        res[name + " cleared"] = len(got.get(None, [])) - sum(not b for b in S.blocks)
        res[name + " erased"] = sum(len(S.blocks[k]) - len(got[k][0]) for k in cut)
    return res


@pytest.mark.parametrize("seed", [0])
def test_sweep_outcomes(seed):
    """Conditions on the inputs: the seed and the generator's densities are
    chosen so that the oracle meets them."""
    S = gc.sweep(seed)
    assert len(S.blocks) == 150
    assert 2 == min(len(b) for b in S.blocks if b) and max(len(b) for b in S.blocks) == 70
    assert max(len(b[0][4]) for b in S.blocks if b) <= 900
    c = sweep_counts(S)
    for what in ("moved left", "moved right", "permissive cut", "strict cut", "permissive cleared", "strict cleared",
                 "permissive erased"):
        assert c[what] >= 10, c
    assert c["strict erased"] == 0  # (a gapless column holds a letter of every row)
