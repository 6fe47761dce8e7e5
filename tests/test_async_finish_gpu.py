"""The asynchronous aligner path (align_device with AlignAsync: what the device
ExtendLoopFast calls) without its list and record launches: the wave that
makes a job's status final lists it for the re-run at the proven bound or
writes its rows' record (job_final), and the re-run's launches leave at once
when their device-side count is zero.

DraftPangenome with the device loop against the host loop and the oracle
(hash and rows digest), with the per-slot scratch capped (NPGX_SLOT_BUDGET_MB:
first attempts overflow and re-run) and short segments (NPGX_ALIGN_SPLIT:
split jobs, split sub-jobs and their retry list on flanks a few hundred
columns long); and the aligner alone through npgx_align_batch_async against
npgx_align_batch and the oracle, with and without overflowing jobs."""
import numpy as np
import pytest

from oracle import oracle as orc
from npge_amd import synth
from npge_amd.anchor_finder import AnchorFinder

from helpers import rows_digest
from test_block_build_gpu import _engine
from test_similar_aligner_gpu import _aligner, _family

pytestmark = pytest.mark.gpu

_REF = {}


def _draft(cfg, device, monkeypatch, budget=None, split=None):
    monkeypatch.setenv("NPGX_ELF_DEVICE", "1" if device else "0")
    for k, v in (("NPGX_SLOT_BUDGET_MB", budget), ("NPGX_ALIGN_SPLIT", split)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    names, seqs = synth.genome_set(cfg)
    ss, eng = _engine(seqs, names)
    eng.apply("DraftPangenome", af=AnchorFinder())
    return eng.hash(), eng.rows_digest(), eng.stats()


def _reference(cfg, monkeypatch):
    """(hash, rows digest) of the oracle and of the host loop, once per config."""
    if cfg not in _REF:
        names, seqs = synth.genome_set(cfg)
        o = orc.BlockSetOracle(seqs, names)
        o.apply("DraftPangenome")
        h, d, st = _draft(cfg, False, monkeypatch)
        assert st["device_iterations"] == 0
        _REF[cfg] = ((o.hash(), rows_digest(o.blocks())), (h, d))
    return _REF[cfg]


@pytest.mark.parametrize("split", [None, "64", "128"])
@pytest.mark.parametrize("budget", [None, "1"])
@pytest.mark.parametrize("cfg", ["small", "rsmall"])
def test_draft_device_loop(cfg, budget, split, monkeypatch):
    oracle, host = _reference(cfg, monkeypatch)
    h, d, st = _draft(cfg, True, monkeypatch, budget, split)
    assert st["device_iterations"] > 0 and st["device_sync_iterations"] == 0
    assert (h, d) == host
    assert (h, d) == oracle


def _tail_families():
    rng = np.random.default_rng(61)
    jobs = []
    for i, n in enumerate((2, 3, 4, 5, 7, 9, 11, 13, 16, 17)):
        L = int(rng.integers(600, 2001))
        jobs.append(_family(rng, n, L, 0.05, tail_unrelated=1.0 if i % 2 else 0.0))
    return jobs


def test_async_batch_capped_scratch(monkeypatch):
    """The per-slot scratch capped: families of 600 to 2000 columns, half of
    them with rows unrelated from part-way.  Rows equal npgx_align_batch's
    and the oracle's.  (At these sizes no search outgrows the capped tables:
    the count of re-run jobs reads 0; the re-run is forced below.)"""
    monkeypatch.setenv("NPGX_SLOT_BUDGET_MB", "1")
    jobs = _tail_families()
    exp = [orc.align(job, mode="align_seqs") for job in jobs]
    sync = _aligner().align(jobs)
    al = _aligner()
    got = al.align(jobs, asynchronous=True)
    print("jobs re-run: %d of %d" % (al.retried, len(jobs)))
    for j in range(len(jobs)):
        assert got[j] == sync[j], "job %d differs from npgx_align_batch" % j
        assert got[j] == exp[j], "job %d differs from the oracle" % j


@pytest.mark.parametrize("defer", [None, "1"])
@pytest.mark.parametrize("split", [None, "64"])
def test_async_batch_rerun(split, defer, monkeypatch):
    """NPGX_TEST_FIRST_CAP=1: the first attempt's rooms hold the longest row
    + 1 columns (rounded up to 16), so every family whose alignment is longer
    overflows it -- in the job's own walk, in a split job's chain
    (k_split_post) or in a deferred job's assembly (k_align_finish) -- and
    re-runs at the proven bound from the list the finishing waves made."""
    monkeypatch.setenv("NPGX_TEST_FIRST_CAP", "1")
    for k, v in (("NPGX_ALIGN_SPLIT", split), ("NPGX_ALIGN_DEFER", defer)):
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, v)
    jobs = _tail_families()
    exp = [orc.align(job, mode="align_seqs") for job in jobs]
    must = sum(len(e[0]) > ((max(len(r) for r in job) + 1 + 15) & ~15) for job, e in zip(jobs, exp))
    assert must >= 2
    sync = _aligner().align(jobs)
    al = _aligner()
    got = al.align(jobs, asynchronous=True)
    print("jobs re-run: %d of %d (at least %d)" % (al.retried, len(jobs), must))
    for j in range(len(jobs)):
        assert got[j] == sync[j], "job %d differs from npgx_align_batch" % j
        assert got[j] == exp[j], "job %d differs from the oracle" % j
    assert al.retried >= must
    assert al.align(jobs, asynchronous=True) == sync  # (the handle again: its lists start empty)


def test_draft_device_loop_rerun(monkeypatch):
    """The device loop with first attempts that overflow (NPGX_TEST_FIRST_CAP)."""
    oracle, host = _reference("small", monkeypatch)
    monkeypatch.setenv("NPGX_TEST_FIRST_CAP", "1")
    h, d, st = _draft("small", True, monkeypatch)
    assert st["device_iterations"] > 0 and st["device_sync_iterations"] == 0
    assert (h, d) == host == oracle


def test_async_batch_without_overflows(monkeypatch):
    monkeypatch.delenv("NPGX_SLOT_BUDGET_MB", raising=False)
    rng = np.random.default_rng(62)
    jobs = [_family(rng, n, int(rng.integers(600, 2001)), 0.01) for n in (2, 3, 5, 9, 17)]
    jobs += [["ACGT"], ["", "ACGT", ""], ["", ""]]
    sync = _aligner().align(jobs)
    al = _aligner()
    got = al.align(jobs, asynchronous=True)
    assert al.retried == 0
    assert got == sync
    assert got[:5] == [orc.align(job, mode="align_seqs") for job in jobs[:5]]
