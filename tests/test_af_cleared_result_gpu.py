"""A deferred AnchorFinder result that nobody reads (DraftPangenome keeps the
anchors on the device, anchors_to_device) is dropped by the next run, not
grouped on the host: after npgx_af_clear_used nothing of it is left to do, and
without the clear only its used hashes are added (the hash of every group
after the first), never its fragments.  The result accessors still group on
demand.  npgx_af_stats.host_regroups counts the host groupings of deferred
results; npgx_af_stats_get reports the count from before the grouping it may
trigger itself, so the tests read it before they read a result."""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc
from npge_amd import _capi, synth
from npge_amd.anchor_finder import AnchorFinder

from helpers import rows_digest
from test_block_build_gpu import _engine, canon

pytestmark = pytest.mark.gpu

KEYS = ("block_start", "seq", "min_pos", "max_pos", "ori")


def _regroups(af):
    st = _capi.AfStats()
    _capi.check(_capi.lib().npgx_af_stats_get(af._h, ctypes.byref(st)))
    return int(st.host_regroups)


def _frags(r):
    return [np.asarray(r[k]).tolist() for k in KEYS]


def _env(monkeypatch, anchors_on_device="1"):
    monkeypatch.setenv("NPGX_ELF_DEVICE", "1")
    monkeypatch.setenv("NPGX_ANCHOR_DEVICE", anchors_on_device)


_ORACLE = {}


def _oracle_af(cfg):
    """Two runs of the oracle's AnchorFinder on one instance (the used hashes
    persist): [(fragments, sorted used hashes)] per run; computed once."""
    if cfg not in _ORACLE:
        names, seqs = synth.genome_set(cfg)
        o = orc.AnchorFinder()
        runs = []
        for _ in range(2):
            r = o.run(seqs, names)
            runs.append((_frags(r), sorted(r["used"].tolist())))
        _ORACLE[cfg] = runs
    return _ORACLE[cfg]


@pytest.mark.parametrize("cfg", ["tiny", "small"])
def test_run_clear_run_drops_the_first_result(cfg, monkeypatch):
    _env(monkeypatch)
    names, seqs = synth.genome_set(cfg)
    ss, eng = _engine(seqs, names)
    af = AnchorFinder()
    eng.apply("DraftPangenome", af=af)
    assert eng.stats()["device_iterations"] > 0  # (the anchors stayed on the device)
    af.clear_used()
    eng.apply("DraftPangenome", af=af)
    assert _regroups(af) == 0
    got = (_frags(af.result()), af.used_hashes().tolist())
    ss2, eng2 = _engine(seqs, names)
    fresh = AnchorFinder()
    eng2.apply("DraftPangenome", af=fresh)
    exp = (_frags(fresh.result()), fresh.used_hashes().tolist())
    assert got == exp
    assert len(got[1]) > 0
    assert got[0] == _oracle_af(cfg)[0][0]
    assert sorted(got[1]) == _oracle_af(cfg)[0][1]


@pytest.mark.parametrize("cfg", ["tiny", "small"])
def test_run_run_adds_only_the_used_hashes(cfg, monkeypatch):
    names, seqs = synth.genome_set(cfg)
    res = []
    for anc in ("1", "0"):
        _env(monkeypatch, anc)
        ss, eng = _engine(seqs, names)
        af = AnchorFinder()
        eng.apply("DraftPangenome", af=af)
        eng.apply("DraftPangenome", af=af)
        if anc == "1":
            assert eng.stats()["device_iterations"] > 0
            assert _regroups(af) == 0  # (the first result: no fragment arrays)
        res.append((_frags(af.result()), af.used_hashes().tolist(), canon(eng.blocks()), eng.rows_digest()))
    assert res[0] == res[1]
    exp = _oracle_af(cfg)[1]
    assert res[0][0] == exp[0]
    assert sorted(res[0][1]) == exp[1]
    assert len(exp[1]) > len(_oracle_af(cfg)[0][1])  # (the second run added to the set)


@pytest.mark.parametrize("cfg", ["tiny", "small"])
def test_run_clear_read_groups_on_demand(cfg, monkeypatch):
    _env(monkeypatch)
    names, seqs = synth.genome_set(cfg)
    ss, eng = _engine(seqs, names)
    af = AnchorFinder()
    eng.apply("DraftPangenome", af=af)
    af.clear_used()
    assert _regroups(af) == 0
    r = af.result()
    assert _frags(r) == _oracle_af(cfg)[0][0]
    assert af.used_hashes().tolist() == []
    assert _regroups(af) == 1
    assert _frags(af.result()) == _oracle_af(cfg)[0][0]  # (grouped once)
    assert _regroups(af) == 1


@pytest.mark.parametrize("cfg", ["tiny", "small"])
def test_draft_twice_on_one_engine(cfg, monkeypatch):
    """What BlockBuild.run does every step: clear the used set, DraftPangenome."""
    _env(monkeypatch)
    names, seqs = synth.genome_set(cfg)
    o = orc.BlockSetOracle(seqs, names)
    o.apply("DraftPangenome")
    exp = (o.hash(), rows_digest(o.blocks()))
    ss, eng = _engine(seqs, names)
    af = AnchorFinder()
    for _ in range(2):
        af.clear_used()
        eng.apply("DraftPangenome", af=af)
        assert (eng.hash(), eng.rows_digest()) == exp
    assert _regroups(af) == 0
