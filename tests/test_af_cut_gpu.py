"""The AnchorFinder's cut on the engine, over the table of af_cut_cases.py
(test_af_cut_cases_ref.py shows on the CPU that each case sits on its edge).

On one GPU pass 2 looks only at the windows of the
L = min(|H|, max-anchor-fragments + 1) smallest collected hashes, sorts their
keys and cuts: the result, the used hashes and the statistics must be the
oracle's for a plain run (which also counts the FoundFragments of all of H at
once) and for the deferred run DraftPangenome asks for (which counts them when
the statistics are read), first and repeated runs on one handle alike."""
import numpy as np
import pytest

from oracle import oracle as orc

import af_cut_cases as cc
from test_anchor_finder_gpu import _assert_same
from test_block_build_gpu import _engine, canon

pytestmark = pytest.mark.gpu

IDS = [c["name"] for c in cc.CASES]
ARRAYS = ("block_start", "seq", "min_pos", "max_pos", "ori")
STATS = ("members", "bloom_bits", "bloom_hashes", "n_windows", "n_collected_raw", "n_collected", "n_found_frags",
         "n_kept_groups", "n_blocks", "n_fragments", "n_used")


def _af(c):
    from npge_amd.anchor_finder import AnchorFinder
    p = AnchorFinder(bloom_params=c["params"])
    p.set_opt_value("anchor-size", c["k"])
    p.set_opt_value("anchor-fp", c["fp"])
    p.set_opt_value("anchor-similar", c["similar"])
    p.set_opt_value("max-anchor-fragments", c["maxf"])
    p.set_opt_value("bloom-seed", c["seed"])
    return p


@pytest.fixture(scope="module")
def oracle_runs():
    """The oracle's runs of every case, computed once."""
    return {c["name"]: cc.oracle_runs(c) for c in cc.CASES}


@pytest.mark.parametrize("c", cc.CASES, ids=IDS)
def test_plain_run_against_oracle(c, oracle_runs):
    from npge_amd import _capi
    ss = _capi.SeqSet(c["seqs"], c["names"])
    g = _af(c)
    for clear, ro in zip(c["runs"], oracle_runs[c["name"]]):
        if clear:
            g.clear_used()
        rg = g.find(ss)
        _assert_same(rg, ro, g.used_hashes())
        assert g.stats.n_kept_groups == ro["kept_groups"]


def _oracle_blockset(c):
    """The oracle's block set with the case's AnchorFinder options, where it
    can take them (it has no anchor-similar switch and no explicit parameters)."""
    if not c["similar"] or c["params"] is not None:
        return None
    return orc.BlockSetOracle(c["seqs"], c["names"], anchor_size=c["k"],
                              anchor_fp_x1e4=int(round(float(c["fp"]) * 10000)),
                              max_anchor_fragments=c["maxf"], seed=c["seed"])


@pytest.mark.parametrize("c", cc.CASES, ids=IDS)
def test_deferred_engine_run_against_plain_and_oracle(c, oracle_runs):
    """DraftPangenome keeps the anchors on the device and defers the host
    result; what the handle then reports equals the plain run's and the
    oracle's.  The used-set cases make three runs on the handle."""
    ss, eng = _engine(c["seqs"], c["names"])
    af, plain = _af(c), _af(c)
    ob = _oracle_blockset(c)
    for clear, ro in zip(c["runs"], oracle_runs[c["name"]]):
        if clear:
            af.clear_used()
            plain.clear_used()
            ob = _oracle_blockset(c)
        eng.apply("DraftPangenome", af=af)
        blocks = canon(eng.blocks())
        st = eng.stats()
        r = af.result()
        used = af.used_hashes()
        rp = plain.find(ss)
        _assert_same(r, ro, used)
        for key in ARRAYS:
            np.testing.assert_array_equal(r[key], rp[key], err_msg=key)
        np.testing.assert_array_equal(used, plain.used_hashes())
        for key in STATS:
            assert getattr(af.stats, key) == getattr(plain.stats, key), key
        assert list(af.stats.bloom_params) == list(plain.stats.bloom_params)
        assert af.stats.n_kept_groups == ro["kept_groups"]
        assert st["anchor_blocks"] == len(ro["block_start"]) - 1
        if ob is not None:
            ob.apply("DraftPangenome")
            assert blocks == canon(ob.blocks())
            assert st["stem_blocks"] == ob.stats()["stem_blocks"]
    # every run that kept a FoundFragment was deferred and grouped on the host
    # only when result() asked (a plain run groups at once and counts nothing here)
    af.result()
    assert af.stats.host_regroups == sum(1 for ro in oracle_runs[c["name"]] if ro["kept_groups"] > 0)
    assert plain.stats.host_regroups == 0


def test_statistics_without_the_result_first(oracle_runs):
    """The FoundFragment total of a deferred run is counted when the
    statistics are read, whatever was read before; a second run drops the
    first run's pending count with its pending result."""
    from npge_amd import _capi
    import ctypes
    c = next(x for x in cc.CASES if x["name"] == "used_set_kept")
    runs = oracle_runs[c["name"]]
    ss, eng = _engine(c["seqs"], c["names"])
    af = _af(c)
    eng.apply("DraftPangenome", af=af)  # (its result and statistics are never asked for)
    eng.apply("DraftPangenome", af=af)
    st = _capi.AfStats()
    _capi.check(_capi.lib().npgx_af_stats_get(af._h, ctypes.byref(st)))
    assert st.n_found_frags == runs[1]["n_found_frags"]
    assert st.n_collected == runs[1]["n_collected"]
    assert st.n_kept_groups == runs[1]["kept_groups"]
    _assert_same(af.result(), runs[1], af.used_hashes())
