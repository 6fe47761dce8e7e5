"""The split jobs' chain copies (k_chain_copy into the job's A, k_sub_post into
a split sub-job's output): many workgroups per chain, one part of CHAIN_PART
(512) output columns each, dword stores where a row's place is aligned and
bytes at the ragged ends, the identical-column bits OR-ed into words that
neighbouring parts share.  Families whose alignments end below a part, at
exactly one part, one column past it and several parts on, at columns that
are no multiples of 4 or 64; substitutions only (the alignment is as long as
the rows, so the boundary cases are hit exactly; the segments still start at
arbitrary columns) and with indels (ragged lengths); 2, 3, 17 and 19 rows.
Rows compared with the oracle's exactly."""
import numpy as np
import pytest

from oracle import oracle as orc

from test_similar_aligner_gpu import _aligner, _family

pytestmark = pytest.mark.gpu

LENGTHS = [301, 512, 513, 1023, 1026, 1537, 2051, 4099, 4613]
ROWS = [2, 3, 17, 19]


def _jobs():
    rng = np.random.default_rng(51)
    jobs = []
    for L in LENGTHS:
        for n in ROWS:
            jobs.append(_family(rng, n, L, 0.01, indel=0.0))
    for L in (513, 1537, 4099):
        for n in ROWS:
            jobs.append(_family(rng, n, L, 0.02))
    # unrelated from part-way: low-similarity regions long enough to be split sub-jobs
    for n in ROWS:
        jobs.append(_family(rng, n, 3001, 0.01, tail_unrelated=0.5))
    return jobs


_CACHE = {}


def _expected():
    if not _CACHE:
        jobs = _jobs()
        _CACHE["jobs"] = jobs
        _CACHE["rows"] = [orc.align(job, mode="align_seqs") for job in jobs]
    return _CACHE["jobs"], _CACHE["rows"]


def test_boundary_lengths_are_hit():
    jobs, exp = _expected()
    lens = {len(e[0]) for e in exp}
    for L in LENGTHS:  # (substitutions only: as many columns as the rows are long)
        assert L in lens


@pytest.mark.parametrize("split", ["64", "256"])
def test_chain_copy_part_boundaries(split, monkeypatch):
    monkeypatch.setenv("NPGX_ALIGN_SPLIT", split)
    jobs, exp = _expected()
    got = _aligner().align(jobs)
    for j, (g, e) in enumerate(zip(got, exp)):
        assert g == e, "job %d (%d rows of %d): rows differ from the oracle's" % (j, len(jobs[j]), len(jobs[j][0]))
