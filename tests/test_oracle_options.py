"""The teeth of test_options_gpu.py: on the very inputs the GPU tests use, the
oracle's result with every option vector differs from its result with the
defaults, so an engine that ignored the option (or hard-coded the default)
could not match.  The one exception is stated where it is checked: max_block
alone, which the reference's find_good_subblocks undoes.  CPU only."""
import pytest

import option_cases as oc


def canon(blocks):
    return sorted(tuple(sorted(b)) for b in blocks)


@pytest.mark.parametrize("vector,name", oc.ALIGN_VECTORS, ids=[oc.vid(v) for v, _ in oc.ALIGN_VECTORS])
def test_aligner_vector_bites(vector, name):
    n = oc.changed_jobs(name, vector)
    print("%s on %s: %d of %d jobs change" % (vector, name, n, len(oc.jobs(name))))
    assert n >= 3


@pytest.mark.parametrize("name", ["long", "wide"])
@pytest.mark.parametrize("vector", oc.LEG_VECTORS, ids=oc.vid)
def test_aligner_leg_vector_bites(vector, name):
    """The split / deferred and wide legs: 7 and 5 jobs, at least one moves."""
    n = oc.changed_jobs(name, vector)
    print("%s on %s: %d of %d jobs change" % (vector, name, n, len(oc.jobs(name))))
    assert n >= 1


def test_aligner_restart_legs_bite():
    assert oc.changed_jobs("wide_restart", oc.LEG_VECTORS[0]) == 1
    for v in oc.PREFIX_VECTORS:
        assert oc.changed_jobs("prefix", v) >= 1, v


def test_oracle_kw_maps_every_engine_key():
    from npge_amd.blockset import ALIGN_KEYS, BbOptions
    keys = [k for k, _ in BbOptions._fields_ if k not in ("align", "max_tail", "max_tail_to_gap_x1e4")]
    kw = {k: i for i, k in enumerate(keys + list(ALIGN_KEYS))}
    okw = oc.oracle_kw(kw)
    assert okw["fix_min_fragment"] == okw["filter_min_fragment"] == kw["min_fragment"]
    assert okw["fix_min_identity_x1e4"] == okw["filter_min_identity_x1e4"] == kw["min_identity_x1e4"]
    assert okw["min_identity_x1e4"] == kw["align_min_identity_x1e4"]
    assert okw["min_length"] == kw["align_min_length"]
    assert okw["portion_x1e4"] == kw["extend_portion_x1e4"]
    assert len(okw) == len(kw) + 2


@pytest.mark.parametrize("name,kw", oc.BB_VARIATIONS, ids=[n for n, _ in oc.BB_VARIATIONS])
def test_chain_variation_bites(name, kw):
    base = oc.oracle_chain("tiny", {})
    got = oc.oracle_chain("tiny", kw)
    print(name, [len(s) for s in got], "defaults", [len(s) for s in base])
    assert got[0]
    assert got[-1] != base[-1]


def test_chain_guard_case_returns_no_slice():
    """min_end 60 > min_fragment 40: goodSlices returns nothing, so Filter
    keeps only the blocks that are good whole."""
    kw = dict(oc.BB_VARIATIONS)["guard_min_end_60_min_fragment_40"]
    guard = oc.oracle_chain("tiny", kw)[-1]
    sliced = oc.oracle_chain("tiny", dict(min_fragment=40))[-1]
    before = set(oc.oracle_chain("tiny", kw)[-2])
    assert all(b in before for b in guard)  # whole blocks only (here: none)
    assert len(guard) < len(sliced)


def test_combined_on_small_and_long_block_bites():
    assert oc.oracle_chain("small", oc.COMBINED)[-1] != oc.oracle_chain("small", {})[-1]
    assert any(len(b) > 4 for b in oc.oracle_chain("small", oc.COMBINED)[0])  # past SMALL_FE_ROWS
    fe, fl = oc.oracle_long_block(oc.COMBINED)
    fe0, fl0 = oc.oracle_long_block({})
    assert fe and fl and fe != fe0 and fl != fl0
    assert len(fl) > 1  # the block is cut into slices


@pytest.mark.parametrize("name,kw", oc.BLOCK_SIZE_VARIATIONS, ids=[n for n, _ in oc.BLOCK_SIZE_VARIATIONS])
def test_block_size_variation_bites(name, kw):
    base = oc.oracle_filter_mixed({})
    got = oc.oracle_filter_mixed(kw)
    print(name, len(got), "defaults", len(base), sorted({len(b) for b in got}))
    assert got
    if kw == dict(max_block=2):
        # a block that is good but for its size is one slice, itself: by the
        # reference's rule no input tells max_block 2 from the defaults while
        # find_subblocks is on; the blocks take the other way to the same set
        assert canon(got) == canon(base)
        assert got != oc.oracle_filter_mixed(dict(max_block=2, find_subblocks=0))
    else:
        assert canon(got) != canon(base)


def test_max_block_is_ignored_by_subblocks():
    """find_good_subblocks does not look at max-block (Filter.cpp:176-196):
    with max_block 2 alone the blocks of 3 fragments come back as their own
    sub-blocks; with find_subblocks 0 they are gone."""
    assert any(len(b) == 3 for b in oc.oracle_filter_mixed(dict(max_block=2)))
    assert all(len(b) == 2 for b in oc.oracle_filter_mixed(dict(max_block=2, find_subblocks=0)))
    assert all(len(b) == 3 for b in oc.oracle_filter_mixed(dict(min_block=3)))


@pytest.mark.parametrize("vector", oc.META_VECTORS, ids=oc.vid)
def test_meta_vector_bites(vector):
    assert oc.oracle_meta(vector) != oc.oracle_meta(oc.DEFAULT_VECTOR)


@pytest.mark.parametrize("cfg", ["tiny", "rtiny"])
@pytest.mark.parametrize("name,kw", oc.PIPE_VECTORS, ids=[n for n, _ in oc.PIPE_VECTORS])
def test_pipe_vector_bites(name, kw, cfg):
    blocks, st = oc.oracle_draft(cfg, kw)
    base, _ = oc.oracle_draft(cfg, {})
    assert blocks != base
    assert (len(blocks), st["iterations"]) == oc.PIPE_EXPECTED[cfg, name]
