"""The case table of af_cut_cases.py really sits on the edges it names: every
claim of a case is derived again from the oracle's AnchorFinder results
(n_collected, n_found_frags, the used hashes, the blocks), on the CPU alone.
test_af_cut_gpu.py runs the engine over the same table."""
import pytest

import af_cut_cases as cc


@pytest.mark.parametrize("c", cc.CASES, ids=[c["name"] for c in cc.CASES])
def test_case_hits_its_edges(c):
    f, runs = cc.facts(c)
    assert c["tags"] <= f, "claimed but not hit: %s" % sorted(c["tags"] - f)
    assert len(runs) == len(c["runs"])
    if c["name"] != "shorter_than_k":
        assert 2 <= len(c["seqs"]) <= 5
        assert all(300 <= len(s) <= 3000 for s in c["seqs"])


def test_every_edge_has_a_case():
    claimed = set().union(*(c["tags"] for c in cc.CASES))
    assert claimed == cc.REQUIRED_TAGS
    assert len({c["name"] for c in cc.CASES}) == len(cc.CASES)


def test_sharded_cases_are_cases():
    by = {c["name"] for c in cc.CASES}
    assert set(cc.SHARDED) <= by and len(set(cc.SHARDED)) == len(cc.SHARDED)
    # BASE at k = 12: five chunks a sequence, so two ranks split inside sequence 1
    assert cc.n_chunks(next(c for c in cc.CASES if c["name"] == "inside_group")) == 15


@pytest.mark.parametrize("c", cc.SHARD_EXTRA, ids=[c["name"] for c in cc.SHARD_EXTRA])
def test_shard_extra_has_two_chunks(c):
    """Two chunks in all: of three ranks one owns no chunk, of five ranks three."""
    assert [len(s) - c["k"] + 1 for s in c["seqs"]] == [239, 239]
    assert cc.n_chunks(c) == 2
    for world, idle in ((3, [0]), (5, [0, 1, 3])):
        assert [r for r in range(world) if 2 * r // world == 2 * (r + 1) // world] == idle
    (ro,) = cc.oracle_runs(c)
    assert len(ro["block_start"]) - 1 >= 1
    assert ro["n_found_frags"] > 0


@pytest.mark.parametrize("c", cc.EPOCH_CASES, ids=[c["name"] for c in cc.EPOCH_CASES])
def test_epoch_cases_bloom_shapes(c):
    """fp 0.1 gives 3 hash functions (the window masks' path), fp 0.01 gives 7
    (the path without them), and both find something to cut."""
    runs = cc.oracle_runs(c)
    assert len(runs) == len(c["runs"])
    for ro in runs:
        assert ro["hashes"] == cc.EPOCH_HASHES[c["fp"]]
        assert ro["n_found_frags"] > 0


def test_used_set_changes_the_later_runs():
    """Without clearing, the later runs skip the used hashes: fewer collected
    hashes and another cut; with clearing, every run repeats the first."""
    by = {c["name"]: c for c in cc.CASES}
    kept = cc.oracle_runs(by["used_set_kept"])
    assert kept[1]["n_collected"] < kept[0]["n_collected"]
    assert kept[2]["n_collected"] < kept[1]["n_collected"]
    assert len(kept[0]["used"]) < len(kept[1]["used"]) < len(kept[2]["used"])
    cleared = cc.oracle_runs(by["used_set_cleared"])
    for r in cleared[1:]:
        assert r["n_collected"] == cleared[0]["n_collected"]
        assert list(r["used"]) == list(cleared[0]["used"])
        assert list(r["block_start"]) == list(cleared[0]["block_start"])
