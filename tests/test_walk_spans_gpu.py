"""The walk's short spans (sa_device.hpp: the flattened (row, column) forms of
write_tails, cm_reverse, cm_copy and cm_copy_rev, and append_end's narrow
passes) against the oracle's align_seqs, row for row.

The inputs are built so that try_aligned answers with chosen shifts -- the
widths of the child the walk descends into -- at the seams of those forms:
row counts on both sides of VEC_ROWS, of 16 and of the steps of 64 / n, and
child widths around 64 / n, 128 / n and 64.  Two kinds of planted event,
each at a place where all rows are in step, followed by clean columns:

  * sub(m): one row differs from the others at offsets 0, 1, every fourth
    offset and m - 1, so no word of aligned_check letters is shared before
    shift m: every row's shift is m (a child of n rows x m columns);
  * ins(m): one row carries m extra letters: its shift is m, the others' 0;
    or every row but one carries the same m extra letters.  With the default
    gap_check one extra letter is always try_gap's, so the children one column
    wide run with a gap_check above aligned_check (Job.ins).

The letters are chosen so that try_mismatch and try_gap decline the event
(see _avoid), which leaves it to try_aligned.  _word_shifts restates
find_best_word (SimilarAligner.cpp:246-272) on the CPU and every event's
shifts are asserted against it before anything runs on the device; on the
device the jobs' try_aligned calls and scanned shifts (npgx_align_job_stats)
must reach what the planted events need (_check_stats).

A cluster inside a child's prefix (sub(m, inner=q)): the child meets it with
more than aligned_check columns left, try_mismatch and try_gap decline it and
try_aligned is called -- and finds nothing, as it must.  A word shared by all
rows inside the prefixes [0, first_r(best)) would have been complete in the
parent's search at a shift below the one it stopped at (a reversed word is
shared exactly when the forward word is), so a child of process_seqs never
descends again: one stack level is all a walk uses.  _check_events asserts
that for the planted prefixes; the child ends through append_end.
"""
import ctypes

import numpy as np
import pytest

from oracle import oracle as orc

pytestmark = pytest.mark.gpu

AC = 10      # aligned_check
GAP_WIDE = 12  # a gap_check above aligned_check (children one column wide)
CLEAN = 45   # clean columns after an event: the word, and room for the next event's search
ROWS = [2, 3, 8, 9, 16, 17, 21, 22, 32, 33, 63, 64]
LET = "ACGT"


def _widths(n):
    k = 64 // n
    c = -(-128 // n)
    return sorted({m for m in (1, 2, 3, k - 1, k, k + 1, c - 1, c + 1, 63, 64, 65) if m >= 1})


def _avoid(rng, *letters):
    """A letter different from the given ones (at most three)."""
    return str(rng.choice([x for x in LET if x not in letters]))


def _text(rng, length):
    return "".join(LET[x] for x in rng.integers(0, 4, length))


class Job:
    """Rows grown event by event from a shared text."""

    def __init__(self, rng, n):
        self.rng, self.n = rng, n
        self.rows = [""] * n
        self.events = []  # (position of every row, expected shift of every row)
        self.inner = []   # (position, width, offset) of the pairs planted inside a child's prefix
        self.clean(CLEAN)

    def clean(self, length):
        t = _text(self.rng, length)
        self.rows = [r + t for r in self.rows]

    def _mark(self, shifts):
        self.events.append(([len(r) for r in self.rows], shifts))

    def sub(self, m, row, inner=None):
        """m >= 2 columns in which `row` differs densely from the others.
        inner = q: also at offsets q and q + 1, a pair the child (the reversed
        prefix, q + 2 columns from its end) can only hand to try_aligned."""
        o = _text(self.rng, m + 2)
        x = list(o[:m])
        pairs = {0, 1} | ({inner, inner + 1} if inner is not None else set())
        offs = sorted(pairs | {m - 1} | set(range(4, m, 4)))
        for q in offs:
            # (the pairs: neither try_mismatch nor any try_gap variant holds, in either direction)
            nb = q + 1 if q in (0, inner) else q - 1
            x[q] = _avoid(self.rng, o[q], o[nb]) if q in pairs else _avoid(self.rng, o[q])
        self._mark([m] * self.n)
        if inner is not None:
            # (the child meets offset inner + 1 first, after a clean column)
            assert AC < inner + 2 < m - 1 and inner % 4 == 1 and (m - 2) % 4
            self.inner.append((len(self.rows[0]), m, inner))
        self.rows = [r + ("".join(x) if i == row else o[:m]) for i, r in enumerate(self.rows)]
        self.clean(CLEAN)

    def ins(self, m, rows_with):
        """m extra letters in the rows `rows_with` (the same letters in each).
        One extra letter is try_gap's case whenever the gap_check columns
        after it agree, and the word's aligned_check columns must: m = 1 is
        for a gap_check above aligned_check (GAP_WIDE), with one row differing
        at the eleventh column after the event."""
        o0 = str(self.rng.choice(list(LET)))
        o1 = _avoid(self.rng, o0)
        i0 = _avoid(self.rng, o0, o1)
        extra = i0 if m == 1 else i0 + _avoid(self.rng, o0, o1) + _text(self.rng, m - 2)
        self._mark([m if i in rows_with else 0 for i in range(self.n)])
        self.rows = [r + (extra if i in rows_with else "") + o0 + o1 for i, r in enumerate(self.rows)]
        t = _text(self.rng, CLEAN)
        odd = t[:8] + _avoid(self.rng, t[8]) + t[9:]
        spoil = min(set(range(self.n)) - set(rows_with)) if m == 1 else -1
        self.rows = [r + (odd if i == spoil else t) for i, r in enumerate(self.rows)]


def _word_shifts(rows, pos, ac=AC):
    """try_aligned's answer at the state `pos`: the shift of every row, or None."""
    n = len(rows)
    max_shift = min(len(r) - p for r, p in zip(rows, pos)) - ac
    seen, first = {}, {}
    for s in range(max(max_shift, 0)):
        words = [rows[i][pos[i] + s:pos[i] + s + ac] for i in range(n)]
        best = None
        for i, w in enumerate(words):
            seen.setdefault(w, set()).add(i)
            first.setdefault((w, i), s)
            if len(seen[w]) == n:
                best = w
        if best is not None:
            if len(set(words)) == 1:
                return [s] * n
            return [first[(best, i)] for i in range(n)]
    return None


def _check_events(job):
    for pos, shifts in job.events:
        assert _word_shifts(job.rows, pos) == shifts, (job.n, pos[0], shifts[:4])
        assert max(shifts) > 0  # a child descent
    for at, m, q in job.inner:
        # the child's state when it meets the pair: every row q + 2 columns from
        # the prefix's end; its try_aligned is called (max_shift > 0), and no
        # search anywhere in the child can find a word
        child = [r[at:at + m][::-1] for r in job.rows]
        assert q + 2 - AC > 0
        for p in range(m):
            assert _word_shifts(child, [p] * job.n) is None


def _check_stats(job, s):
    """Device statistics of an unsplit job: try_aligned was called for every
    planted event and every pair inside a child, and scanned at least the
    shifts up to each event's answer (an event taken by try_mismatch or
    try_gap instead would leave both short)."""
    assert len(job.events) > 0
    assert s[2] >= len(job.events) + len(job.inner)
    assert s[3] >= sum(max(sh) + 1 for _, sh in job.events)


def _align(jobs, stats=False, gap_check=2):
    from npge_amd import _capi
    from npge_amd.aligner import BatchAligner
    from npge_amd.blockset import JOB_STATS
    al = BatchAligner(gap_check=gap_check)
    got = al.align(jobs)
    if not stats:
        return got, None
    L = _capi.lib()
    L.npgx_align_job_stats.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64,
                                       ctypes.POINTER(ctypes.c_int64)]
    n = ctypes.c_int64(0)
    out = np.zeros((len(jobs), JOB_STATS), dtype=np.int64)
    _capi.check(L.npgx_align_job_stats(al._h, _capi.ptr(out), len(jobs), ctypes.byref(n)))
    assert n.value == len(jobs)
    return got, out


_ORACLE = {}


def _expected(key, jobs, gap_check):
    if key not in _ORACLE:  # computed once, shared by the memory forms
        prm = (1, gap_check) + orc.DEFAULT_SA[2:]
        _ORACLE[key] = [orc.align(j, mode="align_seqs", params=prm) for j in jobs]
    return _ORACLE[key]


def _compare(key, jobs, got, gap_check=2):
    for j, (g, e) in enumerate(zip(got, _expected(key, jobs, gap_check))):
        assert g == e, "job %d of %s (%d rows, lengths %s): %d columns vs %d expected" % (
            j, key, len(jobs[j]), [len(r) for r in jobs[j]][:4], len(g[0]) if g else 0, len(e[0]) if e else 0)


def _width_jobs(n):
    """Equal shifts of every width of _widths(n); extra letters of 1-10 (and
    the seam widths up to 16) columns in one row and in all rows but one."""
    rng = np.random.default_rng(1000 + n)
    a, b, c = Job(rng, n), Job(rng, n), Job(rng, n)
    for i, m in enumerate(w for w in _widths(n) if w >= 2):
        a.sub(m, (n - 1, 0, n // 2)[i % 3])
    short = sorted(set(range(2, 11)) | {m for m in _widths(n) if 2 <= m <= 16})
    for i, m in enumerate(short):
        b.ins(m, {(0, n - 1, n // 2)[i % 3]})
        c.ins(m, set(range(n)) - {(n - 1, 0, n // 2)[i % 3]})
    jobs = [a, b, c]
    for j in jobs:
        _check_events(j)
        assert max(len(r) for r in j.rows) <= 1500
    assert {m for j in jobs for _, sh in j.events for m in sh} >= set(_widths(n)) - {1}
    return jobs


def _one_wide_jobs(n):
    """One extra letter in one row, and in every row but one (GAP_WIDE)."""
    rng = np.random.default_rng(1500 + n)
    a = Job(rng, n)
    for i in range(4):
        a.ins(1, {(0, n - 1, n // 2)[i % 3]} if i < 2 else set(range(n)) - {(n - 1, 0)[i % 2]})
    _check_events(a)
    assert all(max(sh) == 1 for _, sh in a.events)
    return [a]


def _end_jobs(n):
    """Frame ends.  After a shared head row 0 goes on with e letters, the
    other rows with unrelated text of their own and then the same e letters:
    no word is shared within row 0's reach, try_aligned declines and
    append_end walks back over e identical columns (e = 0: row 0 has ended,
    append_all).  Then: a row of length 0, identical rows, a one-letter
    difference in the last aligned_check columns (realing_end runs) and ten
    columns before them (the tail is identical: it does not)."""
    rng = np.random.default_rng(2000 + n)
    k = 64 // n
    jobs = []
    for e in sorted({0, 1, max(k - 1, 0), k, 62, 63, 64}):
        head, tail = _text(rng, CLEAN), _text(rng, e)
        t0, t1 = (tail + "??")[:2]
        rows = [head + tail]
        for _ in range(1, n):
            u = _avoid(rng, t0, t1) + _avoid(rng, t0, t1) + _text(rng, e + 20)
            rows.append(head + u + tail)
        if e > AC:
            assert _word_shifts(rows, [len(head)] * n) is None
        jobs.append(rows)
    body = _text(rng, 120)
    jobs.append([body] * (n - 1) + [""])
    jobs.append([body] * n)
    for at in (len(body) - 3, len(body) - 25):
        odd = body[:at] + _avoid(rng, body[at]) + body[at + 1:]
        jobs.append([body] * (n - 1) + [odd])
    return jobs


@pytest.mark.parametrize("n", ROWS)
def test_child_widths(n, monkeypatch):
    """Short jobs (rows and A|B|C in LDS); every job makes at least as many
    try_aligned calls as events were planted, and none overflows."""
    monkeypatch.setenv("NPGX_JOB_STATS", "1")
    jobs = _width_jobs(n)
    got, st = _align([j.rows for j in jobs], stats=True)
    for j, s in zip(jobs, st):
        _check_stats(j, s)
    _compare(("w", n), [j.rows for j in jobs], got)


@pytest.mark.parametrize("split", [None, "64", "128"])
@pytest.mark.parametrize("n", ROWS)
def test_children_one_column_wide(n, split, monkeypatch):
    if split:
        monkeypatch.setenv("NPGX_ALIGN_SPLIT", split)
    else:
        monkeypatch.setenv("NPGX_JOB_STATS", "1")
    jobs = _one_wide_jobs(n)
    got, st = _align([j.rows for j in jobs], stats=not split, gap_check=GAP_WIDE)
    if st is not None:
        _check_stats(jobs[0], st[0])
    _compare(("1", n), [j.rows for j in jobs], got, gap_check=GAP_WIDE)


@pytest.mark.parametrize("split", ["64", "128"])
@pytest.mark.parametrize("n", ROWS)
def test_child_widths_split(n, split, monkeypatch):
    """The same inputs as segments of split jobs: rows and outputs in global memory."""
    monkeypatch.setenv("NPGX_ALIGN_SPLIT", split)
    jobs = [j.rows for j in _width_jobs(n)]
    _compare(("w", n), jobs, _align(jobs)[0])


@pytest.mark.parametrize("n", ROWS)
def test_child_widths_near_capacity(n, monkeypatch):
    """Rooms of the longest row + 80 columns: near their end col + 64 > cap
    sends fast_run to rows mode, and the jobs with extra letters in all rows
    but one outgrow the room and run again."""
    monkeypatch.setenv("NPGX_TEST_FIRST_CAP", "80")
    jobs = [j.rows for j in _width_jobs(n)]
    _compare(("w", n), jobs, _align(jobs)[0])


@pytest.mark.parametrize("split", [None, "64", "128"])
@pytest.mark.parametrize("n", ROWS)
def test_frame_ends(n, split, monkeypatch):
    """The ways a frame ends (_end_jobs).  By design these inputs plant no
    event that descends -- try_aligned declines, a row has ended or the rows
    are identical -- so no descent or device statistic is asserted here; the
    rows are compared with the oracle's."""
    if split:
        monkeypatch.setenv("NPGX_ALIGN_SPLIT", split)
    jobs = _end_jobs(n)
    _compare(("e", n), jobs, _align(jobs)[0])


def _inner_jobs(n):
    """Children of 24 to 65 columns with a pair of differences inside."""
    rng = np.random.default_rng(3000 + n)
    a = Job(rng, n)
    for i, (m, q) in enumerate(((24, 13), (40, 17), (45, 13), (65, 37), (63, 49))):
        a.sub(m, (n - 1, 0, n // 2)[i % 3], inner=q)
    _check_events(a)
    assert len(a.inner) == 5 and max(len(r) for r in a.rows) <= 1500
    return [a]


@pytest.mark.parametrize("split", [None, "64", "128"])
@pytest.mark.parametrize("n", ROWS)
def test_cluster_inside_child(n, split, monkeypatch):
    if split:
        monkeypatch.setenv("NPGX_ALIGN_SPLIT", split)
    else:
        monkeypatch.setenv("NPGX_JOB_STATS", "1")
    jobs = _inner_jobs(n)
    got, st = _align([j.rows for j in jobs], stats=not split)
    if st is not None:
        _check_stats(jobs[0], st[0])
    _compare(("i", n), [j.rows for j in jobs], got)
