"""The oracle alone over column_cases.py, on the CPU: what keeps
test_column_shapes_gpu.py from being vacuous.

* every closed-form FixEnds expectation (bad ends come out as [bl, L-1-br];
  the lone window; the best-window choice; the drops) and every literal known
  answer is the oracle's output;
* the plain-Python column vote is BlockSetOracle.conseq() on consensus_edges();
* the Filter cases hold what they are there for: whole passes and cuts, a
  slice longer than COUNT_PIECE, the runs of 999 / 1000 / 1001 columns treated
  alike, the orientation flip;
* the sweep's blocks spread over the outcomes under both processors (bounds on
  the inputs, met by tuning the generator's densities, not measurements).
"""
import collections

import pytest

import column_cases as cc


def canon(blocks):
    return sorted(tuple(sorted(b)) for b in blocks)


def _check_expectations(S, op):
    got = S.split(S.result(op))
    n = 0
    for k in range(len(S.blocks)):
        want = S.expected(k)
        if want is None:
            continue
        key = k if S.blocks[k] else None
        assert canon(got.get(key, [])) == canon(want), (op, k, S.tags[k])
        n += 1
    return n, got


def test_fix_ends_closed_forms():
    S = cc.fix_ends_edges()
    n, got = _check_expectations(S, "FixEnds")
    assert n >= 60
    tags = collections.Counter(t.split()[0] for t in S.tags)
    assert tags["bad_ends"] == 1 + 3 + 3 + 6 * 6, tags
    # the small and the tiled kernels both see every outcome
    for small in (True, False):
        seen = {cc.outcome(S, k, got) for k, b in enumerate(S.blocks) if b and cc.fe_small(b) == small}
        assert seen == {"same", "one", "gone"}, (small, seen)
    assert sum(cc.fe_small(b) for b in S.blocks) % 2 == 1
    assert [k for k, b in enumerate(S.blocks) if not b] not in ([], [len(S.blocks) - 1])
    # the scattered mismatches move the start past the first good column
    moved = 0
    for k, t in enumerate(S.tags):
        if t == "scattered":
            (b,) = got[k]
            row = S.blocks[k][0][4]
            cut = len(row) - len(b[0][4])
            bad = [c for c in range(30) if len({f[4][c] for f in S.blocks[k]}) > 1]
            first_good = min(c for c in range(31) if c not in bad)
            moved += cut > first_good
    assert moved >= 3


def _filter_groups():
    return dict(cc.filter_edges())


@pytest.mark.parametrize("name", ["default", "long_runs", "no_subblocks", "flip"])
def test_filter_known_answers(name):
    S = _filter_groups()[name]
    n, got = _check_expectations(S, "Filter")
    assert n >= 1
    if name == "flip":
        assert S.result("Filter") == [cc.FLIP_ANSWER] == S.result("FixEnds")
        return
    kinds = collections.Counter(cc.outcome(S, k, got) for k, b in enumerate(S.blocks) if b)
    assert kinds["same"] >= 2 and kinds["gone"] >= 1, kinds
    if name == "no_subblocks":
        assert kinds["one"] == kinds["many"] == 0
        return
    assert kinds["many"] >= 1 and kinds["one"] >= 1, kinds


def test_filter_edges_hold_their_cases():
    S = _filter_groups()["default"]
    got = S.split(S.result("Filter"))
    tag = {t: k for k, t in enumerate(S.tags)}
    # the 40,000-column block: slices of 20,000 and 18,999 columns, more than one COUNT_PIECE each, gaps before the cut
    long = got[tag["long 40000"]]
    assert sorted(len(b[0][4]) for b in long) == [18999, 20000]
    first = min(long, key=lambda b: -len(b[0][4]))
    assert sum("-" in f[4] for f in first) >= 3  # fewer letters than columns before the cut
    assert max(len(b[0][4] or "") for b in S.result("Filter")) > 16384
    assert {f[3] for b in long for f in b} == {1, -1}
    # a run of 100 ident-gap columns and more is a cut of its own, at the seam as anywhere
    for ln in cc.GAP_RUNS:
        for where in ("ends_4095", "ends_4096", "starts_4096", "across"):
            k = tag["gap_run %d %s" % (ln, where)]
            assert cc.outcome(S, k, got) == ("same" if ln == 1 else "many"), (ln, where)
    # one failing frame is enough
    for k, t in enumerate(S.tags):
        if t.startswith("isolated frame") or t.startswith("burst"):
            assert cc.outcome(S, k, got) in ("one", "many"), t
    assert cc.outcome(S, tag["unaligned"], got) == "same"
    assert cc.outcome(S, tag["N column"], got) == "same" and cc.outcome(S, tag["pure gap column"], got) == "same"


def test_filter_long_runs_are_capped_alike():
    """999, 1000 and 1001 ident-gap columns under min_fragment 2000: the run's
    length is capped at 999 before it is compared with min_fragment, so all
    three score alike and the blocks are cut at the same distances."""
    S = _filter_groups()["long_runs"]
    got = S.split(S.result("Filter"))
    for ln in (999, 1000, 1001):  # the columns before and after the run, nothing more cut off
        k = S.tags.index("gap_run %d" % ln)
        assert sorted(len(b[0][4]) for b in got[k]) == sorted([2500, 6000 - 2500 - ln])
        k = S.tags.index("gap_run %d ends_4095" % ln)
        assert sorted(len(b[0][4]) for b in got[k]) == sorted([4096 - ln, 7000 - 4096])
    k = S.tags.index("gap_run 2000")  # at min_fragment the run is refused whatever the cap
    assert sorted(len(b[0][4]) for b in got[k]) == [2100, 2900]


@pytest.mark.parametrize("name", cc.INVALID_CASES)
def test_filter_invalid_outcomes(name):
    """(test_filter_steps_gpu.py's inputs: the oracle drops the invalid
    fragment and keeps, slices or loses the rest, as invalid_result asserts)"""
    S, want = cc.invalid_result(name)
    q, mn, mx = S.blocks[0][-1][:3]
    assert (mx >= len(S.seqs[q])) == (name != "all_valid_control")
    assert len(S.blocks[0][-1][4]) == mx - mn + 1 and 300 <= mx - mn + 1 <= 400
    assert all(q != f[0] for b in want for f in b)


def test_consensus_vote():
    S = cc.consensus_edges()
    assert S.blocks == sorted(S.blocks, key=cc.orc.consensus_order)
    o = S.oracle()
    o.set_blocks(S.input())
    got = o.conseq()
    want = [cc.vote([f[4] for f in b]) for b in S.blocks]
    assert got == want
    assert sorted((len(b), len(b[0][4])) for b in S.blocks if len(b[0][4]) not in (9, 22)) == sorted(cc.CONS_SHAPES)
    assert set("".join(want)) == set("ATGCN")
    order = [(x, y) for x in "ATGCN" for y in "ATGCN" if x != y]
    assert got[S.tags.index("pairs")] == "".join(min(p, key="ATGCN".index) for p in order) + "AA"
    assert got[S.tags.index("majorities")] == "NNTTAAAAT"


SWEEP_BOUNDS = {"same": (0.20, 1.0), "changed": (0.20, 1.0), "gone": (0.0, 0.40)}


@pytest.mark.parametrize("seed", [0, 1])
def test_sweep_outcomes(seed):
    S = cc.sweep(seed)
    assert 100 <= len(S.blocks) <= 150
    assert {len(b[0][4]) for b in S.blocks} == set(cc.SWEEP_LENGTHS)
    assert {len(b) for b in S.blocks} == set(cc.SWEEP_ROWS)
    for op, changed in (("FixEnds", "one"), ("Filter", "many")):
        got = S.split(S.result(op))
        kinds = collections.Counter(cc.outcome(S, k, got) for k in range(len(S.blocks)))
        share = {"same": kinds["same"], "changed": kinds[changed], "gone": kinds["gone"]}
        for what, (lo, hi) in SWEEP_BOUNDS.items():
            assert lo <= share[what] / len(S.blocks) <= hi, (op, what, dict(kinds))
