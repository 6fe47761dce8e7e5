"""align_device's launch plan, through the public API: for one batch per path
(plain, split, deferred, the re-run at the proven bound synchronous and
asynchronous, a wide problem) the aligned rows equal the oracle's and the
launches, read as the ordered names of kernel_times() with every launch timed
(NPGX_TIMERS=2), are the ones listed here.  The lists are the host plan's
contract with StageTimer::key_launch and the benches that read the names."""
import numpy as np
import pytest

from oracle import oracle as orc

from test_similar_aligner_gpu import _aligner, _family

pytestmark = pytest.mark.gpu

_KNOBS = ("NPGX_ALIGN_SPLIT", "NPGX_ALIGN_DEFER", "NPGX_ALIGN_DEFER_ROWS", "NPGX_TEST_FIRST_CAP",
          "NPGX_SLOT_BUDGET_MB", "NPGX_UTWINS", "NPGX_JOB_STATS")

_SPLIT_LAUNCHES = ["align_split", "align_jobs", "align_split_chain", "align_split_post", "align_sub_rows",
                   "align_sub_split", "align_sub", "align_sub_post", "align_sub_retry", "align_fin_copy",
                   "align_finish", "gather_rows"]
_DEFER_LAUNCHES = ["align_jobs", "align_sub", "align_fin_copy", "align_finish", "gather_rows"]
_FIRST_CAP = 8


def _run(jobs, env, monkeypatch, asynchronous=False):
    """(aligner, names of its launches in order); the rows are checked against the oracle."""
    monkeypatch.setenv("NPGX_TIMERS", "2")  # read when the handle is made
    for k in _KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    al = _aligner()
    got = al.align(jobs, asynchronous=asynchronous)
    for j, job in enumerate(jobs):
        assert got[j] == orc.align(job, mode="align_seqs"), "job %d differs from the oracle" % j
    return al, [k["name"] for k in al.kernel_times()]


def _rerun_batch():
    """One family without insertions to speak of, and one whose rows each carry
    an insertion of their own: its alignment is longer than the first room of
    NPGX_TEST_FIRST_CAP (the longest row + _FIRST_CAP columns, rounded up to 16)."""
    rng = np.random.default_rng(63)
    calm = _family(rng, 3, 400, 0.01, indel=0.0)
    anc = "".join("ATGC"[x] for x in rng.integers(0, 4, 600))
    ins = ["".join("ATGC"[x] for x in rng.integers(0, 4, 40)) for _ in range(3)]
    grown = [anc[:150 * (i + 1)] + ins[i] + anc[150 * (i + 1):] for i in range(3)]
    jobs = [calm, grown]
    room = lambda job: (max(len(r) for r in job) + _FIRST_CAP + 15) & ~15
    over = [len(orc.align(job, mode="align_seqs")[0]) > room(job) for job in jobs]
    assert over == [False, True]
    return jobs


def test_plain(monkeypatch):
    rng = np.random.default_rng(60)
    jobs = [_family(rng, 3, 60, 0.02) for _ in range(2)]
    assert _run(jobs, {}, monkeypatch)[1] == ["align_jobs", "gather_rows"]


def test_split(monkeypatch):
    rng = np.random.default_rng(61)
    jobs = [_family(rng, 3, 1024, 0.02)]
    assert _run(jobs, {"NPGX_ALIGN_SPLIT": "64"}, monkeypatch)[1] == _SPLIT_LAUNCHES


def test_deferred_unsplit(monkeypatch):
    """Split length 0: the deferred regions' sub-jobs are never split, so no align_sub_split."""
    rng = np.random.default_rng(62)
    jobs = [_family(rng, 4, 600, 0.03)]
    env = {"NPGX_ALIGN_SPLIT": "0", "NPGX_ALIGN_DEFER": "1", "NPGX_ALIGN_DEFER_ROWS": "0"}
    assert _run(jobs, env, monkeypatch)[1] == _DEFER_LAUNCHES


_RERUN_ENV = {"NPGX_TEST_FIRST_CAP": str(_FIRST_CAP), "NPGX_ALIGN_SPLIT": "0", "NPGX_ALIGN_DEFER": "0"}


def test_rerun_synchronous(monkeypatch):
    names = _run(_rerun_batch(), _RERUN_ENV, monkeypatch)[1]
    assert names == ["align_jobs", "align_jobs_retry", "gather_rows"]


def test_rerun_asynchronous(monkeypatch):
    al, names = _run(_rerun_batch(), _RERUN_ENV, monkeypatch, asynchronous=True)
    assert names == ["align_jobs", "align_jobs_retry", "gather_rows"]
    assert al.retried == 1


def test_asynchronous_no_overflow(monkeypatch):
    """The re-run is enqueued whether or not a job overflowed: its count is on the device."""
    rng = np.random.default_rng(64)
    jobs = [_family(rng, 3, 300, 0.02) for _ in range(2)]
    al, names = _run(jobs, {}, monkeypatch, asynchronous=True)
    assert names == ["align_jobs", "align_jobs_retry", "gather_rows"]
    assert al.retried == 0


def test_wide(monkeypatch):
    rng = np.random.default_rng(65)
    jobs = [_family(rng, 65, 40, 0.02), _family(rng, 3, 60, 0.02)]
    assert _run(jobs, {}, monkeypatch)[1] == ["align_jobs", "align_wide", "gather_rows"]
