"""Edge-shape inputs of the column kernels behind FixEnds, Filter and ConSeq
(npge_amd/csrc/block_build.hip), shared by test_column_cases_ref.py (the oracle
alone, on the CPU: closed forms, known answers and the spread of outcomes) and
test_column_shapes_gpu.py (engine against oracle, bit for bit).

Blocks are lists of (seq, min, max, ori, row), the form BlockSetEngine and
BlockSetOracle share.  Every row lies on a sequence of its own: the row's
letters wrapped in a few padding letters, so no fragment starts at 0 (the
literal known answers apart); every odd row has ori -1 and its sequence holds
the reverse complement.  A block is therefore known by its sequences, and
split() sorts a processor's output by the input block it came from.

Keyword sets are BlockSetEngine's; option_cases.oracle_kw() translates them.
Everything is seeded, built once per process and handed out unchanged.
"""
import functools

import numpy as np

from oracle import oracle as orc

import option_cases as oc

MIN_FRAGMENT = 100   # the defaults: min_good 90, sub_frame 10 (FixEnds); frame 100, min_end 10 (Filter)
GAP_RUNS = (1, 63, 64, 65, 99, 100, 101)

_COMP = str.maketrans("ATGCN", "TACGN")
_A, _T, _G, _C, _N, _GAP = (ord(x) for x in "ATGCN-")
_LETTERS = np.frombuffer(b"ATGC", dtype=np.uint8)
_ROT = np.arange(256, dtype=np.uint8)  # another letter in the place of each: A -> T -> G -> C -> A
for _x, _y in zip("ATGCN", "TGCAA"):
    _ROT[ord(_x)] = ord(_y)


def revcomp(s):
    return s.translate(_COMP)[::-1]


class Cases:
    """Sequences, names and blocks of one engine / oracle pair, with the
    expectation recorded for each block: None (the oracle alone says),
    ("keep",), ("drop",) or ("slice", first column, last column)."""

    def __init__(self, seed, kw=None, pad=True):
        self.rng = np.random.default_rng(seed)
        self.kw = dict(kw or {})
        self.pad = pad
        self.seqs, self.names, self.blocks, self.expect, self.tags = [], [], [], [], []
        self._results = {}

    def _pad(self):
        if not self.pad:
            return ""
        return "".join("ATGC"[x] for x in self.rng.integers(0, 4, int(self.rng.integers(3, 9))))

    def add(self, rows, expect=None, tag="", oris=None, with_rows=True):
        """rows: strings or one 2-D uint8 array; returns the block's index."""
        if isinstance(rows, np.ndarray):
            rows = [r.tobytes().decode() for r in rows]
        blk = []
        for i, row in enumerate(rows):
            ori = (1 if i % 2 == 0 else -1) if oris is None else oris[i]
            letters = row.replace("-", "")
            assert letters, "a fragment has at least one letter"
            left = self._pad()
            self.seqs.append(left + (letters if ori == 1 else revcomp(letters)) + self._pad())
            self.names.append("g%d&c&c" % len(self.names))
            blk.append((len(self.seqs) - 1, len(left), len(left) + len(letters) - 1, ori, row if with_rows else None))
        self.blocks.append(blk)
        self.expect.append(expect)
        self.tags.append(tag)
        return len(self.blocks) - 1

    def engine_kw(self):
        return dict(self.kw)

    def oracle(self):
        return orc.BlockSetOracle(list(self.seqs), list(self.names), **oc.oracle_kw(self.kw))

    def input(self):
        return [list(b) for b in self.blocks]

    def result(self, op):
        """The oracle's blocks after `op` on the input (computed once)."""
        if op not in self._results:
            o = self.oracle()
            o.set_blocks(self.input())
            o.apply(op)
            self._results[op] = tuple(tuple(b) for b in o.blocks())
        return [list(b) for b in self._results[op]]

    def split(self, out):
        """out's blocks by the input block they came from: {index: [blocks]};
        blocks without fragments under None."""
        owner = {}
        for k, b in enumerate(self.blocks):
            for f in b:
                owner[f[0]] = k
        res = {}
        for b in out:
            ks = {owner[f[0]] for f in b}
            assert len(ks) <= 1, "a block of two input blocks"
            res.setdefault(ks.pop() if ks else None, []).append(b)
        return res

    def expected(self, k):
        """The blocks input block k becomes, where a closed form is recorded."""
        e = self.expect[k]
        if e is None:
            return None
        if e[0] == "keep":
            return [self.blocks[k]]
        if e[0] == "drop":
            return []
        if e[0] == "literal":
            return [list(b) for b in e[1]]
        return [slice_block(self.blocks[k], self.seqs, e[1], e[2])]


def slice_block(blk, seqs, a, b):
    """Block::slice of columns [a, b] in plain Python: a row's letters before
    and inside the columns move its fragment's ends; a fragment without a
    letter there is left out; one letter of an ori -1 fragment becomes ori +1
    and is written as the forward strand's."""
    out = []
    for (q, mn, mx, ori, row) in blk:
        before = a - row.count("-", 0, a)
        cnt = (b + 1 - a) - row.count("-", a, b + 1)
        if not cnt:
            continue
        begin = mn if ori == 1 else mx
        s0, s1 = begin + ori * before, begin + ori * (before + cnt - 1)
        nori = 1 if s0 <= s1 else -1
        r = row[a:b + 1]
        if nori != ori:
            r = "".join(c if c == "-" else seqs[q][min(s0, s1)] for c in r)
        out.append((q, min(s0, s1), max(s0, s1), nori, r))
    return out


def outcome(cases, k, got):
    """'same' | 'one' (one other block: trimmed) | 'many' (2 or more) | 'gone'
    of input block k, got = split(output)."""
    blocks = got.get(k, [])
    if not blocks:
        return "gone"
    if len(blocks) > 1:
        return "many"
    return "same" if sorted(blocks[0]) == sorted(cases.blocks[k]) else "one"


# ---------------------------------------------------------------- row arrays
def fam(rng, n, L):
    """n equal rows of L random letters (uint8, one row a line)."""
    return np.tile(_LETTERS[rng.integers(0, 4, L)], (n, 1))


def mismatch(M, cols, row=-1):
    """Another letter in one row at the columns (given rows equal there)."""
    cols = np.asarray(cols, dtype=np.int64)
    M[row, cols] = _ROT[M[row, cols]]
    return M


def gap(M, a, b, rows=(-1,)):
    """'-' in the rows at columns [a, b)."""
    for r in rows:
        M[r, a:b] = _GAP
    return M


def bad_ends(rng, n, L, bl, br):
    M = fam(rng, n, L)
    mismatch(M, np.r_[0:bl, L - br:L], row=n - 1)
    return M


# ---------------------------------------------------------------- FixEnds
FE_SHAPES = ((2, 99), (2, 100), (2, 101), (2, 128), (4, 4096), (5, 4096), (2, 4097), (4, 4097), (3, 262144),
             (2, 262209))
FE_ENDS = ((0, 0), (1, 0), (0, 1), (63, 64), (64, 63), (65, 128))


def fe_small(blk):
    """FixEnds takes the block through k_fix_ends_small (SMALL_FE_WORDS,
    SMALL_FE_ROWS), not k_col_bits + k_fix_ends."""
    return bool(blk) and blk[0][4] is not None and len(blk) <= 4 and len(blk[0][4]) <= 4096


@functools.lru_cache(maxsize=None)
def fix_ends_edges():
    """One block set for FixEnds with the default options.

    * bad_ends: the first bl and the last br columns differ in one row, the
      rest is identical: the block comes out as columns [bl, L-1-br], at every
      FE_SHAPES x FE_ENDS that leaves 100 columns.  (4, L) and (5, L) put the
      same columns through the small and the tiled kernels; 262144 columns are
      the most whose identity bits k_fix_ends keeps in LDS, 262209 are read
      from global memory.  (2, 99) is shorter than min_fragment: dropped.
    * window: 100 good columns from column s on and nothing else good: the one
      window of full score, kept as it is; s = L-100 is first_good's last
      admissible start.  window90: 90 good columns, found from both ends, the
      middle [s, s+89] is too short: dropped.
    * rising: mismatches at columns 0, 5 and 12 make the starts 1, 6 and 13
      score 98, 99 and 100, each within sub_frame of the best before: 13 wins.
      rising_far: the better window lies 11 past the first: not taken.
      scattered: three random mismatches in the first 30 columns.
    * a gap column in a good window, and at column 0 (cut off: one row keeps
      its coordinates), a block of one fragment, a block without fragments.
      A block with fragments and no rows is not here: the reference asserts
      has_alignment (FixEnds.cpp:123), FixEnds' answer is not defined for it.
    * the small-path blocks are an odd number: the last k_fix_ends_small
      workgroup has an empty half.
    """
    S = Cases(41)
    rng = S.rng
    for n, L in FE_SHAPES:
        if L < MIN_FRAGMENT:
            S.add(fam(rng, n, L), ("drop",), "short")
            continue
        for bl, br in FE_ENDS:
            if L - bl - br >= MIN_FRAGMENT:
                S.add(bad_ends(rng, n, L, bl, br), ("slice", bl, L - 1 - br) if bl + br else ("keep",),
                      "bad_ends %dx%d %d+%d" % (n, L, bl, br))
        if L == 101:
            S.add([], ("keep",), "empty")  # (kept by both sides; among the others, not at the end)

    def window(n, L, s, width):
        M = fam(rng, n, L)
        mismatch(M, np.r_[0:s, s + width:L], row=n - 1)
        return M
    for n, L, s in ((2, 300, 63), (3, 300, 64), (2, 300, 65), (2, 300, 200), (5, 300, 200), (2, 4200, 4100),
                    (5, 4260, 4160), (3, 4196, 4096), (2, 164, 64), (2, 100, 0)):
        S.add(window(n, L, s, 100), ("slice", s, s + 99) if L > 100 else ("keep",), "window %d@%d" % (L, s))
    S.add(window(2, 300, 70, 90), ("drop",), "window90")
    S.add(window(5, 4300, 4090, 90), ("drop",), "window90")
    S.add(mismatch(fam(rng, 2, 300), np.arange(300)), ("drop",), "no_window")
    S.add(mismatch(fam(rng, 5, 4100), np.arange(4100)), ("drop",), "no_window")
    for n in (2, 5):
        S.add(mismatch(fam(rng, n, 300), [0, 5, 12]), ("slice", 13, 299), "rising")
        S.add(mismatch(fam(rng, n, 300), [0, 12]), ("slice", 1, 299), "rising_far")
        S.add(mismatch(fam(rng, n, 300), [295, 299]), ("slice", 0, 294), "rising_reverse")
    for n, L in ((2, 300), (3, 4097), (5, 300), (4, 130), (9, 130)):
        for _ in range(3):
            S.add(mismatch(fam(rng, n, L), rng.choice(30, size=3, replace=False)), None, "scattered")
    S.add(gap(fam(rng, 2, 150), 50, 51), ("keep",), "gap_inside")
    S.add(gap(fam(rng, 5, 150), 50, 51, rows=(1, 3)), ("keep",), "gap_inside")
    S.add(gap(fam(rng, 3, 150), 0, 1, rows=(1,)), ("slice", 1, 149), "gap_at_0")
    S.add(gap(fam(rng, 3, 4160), 4159, 4160, rows=(2,)), ("slice", 0, 4158), "gap_at_end")
    S.add(fam(rng, 1, 150), ("keep",), "one_fragment")
    S.add(fam(rng, 1, 5000), ("keep",), "one_fragment")
    if sum(fe_small(b) for b in S.blocks) % 2 == 0:
        S.add(bad_ends(rng, 3, 200, 7, 0), ("slice", 7, 199), "odd_small")
    return S


# ---------------------------------------------------------------- Filter
def isolated_frame(rng, n, L, i, frame=100):
    """Exactly one frame, the one that starts at column i, misses 90 %: eleven
    mismatches in it, the first and the last of them on its first and last
    column, good columns before and after it."""
    M = fam(rng, n, L)
    inner = i + 5 + 9 * np.arange(9)
    mismatch(M, np.r_[i, inner, i + frame - 1], row=n - 1)
    return M


def burst(rng, n, L, p, k=11):
    """k mismatches from column p on: with 11, the frames that start in
    [p-89, p] fail."""
    return mismatch(fam(rng, n, L), np.arange(p, p + k), row=n - 1)


def sprinkle(M, step=37, margin=12):
    """A mismatch every `step` columns, none near the ends: the block still
    passes whole."""
    L = M.shape[1]
    return mismatch(M, np.arange(margin + step // 2, L - margin, step), row=0)


def _filter_default():
    S = Cases(43)
    rng = S.rng
    for n, L in ((2, 100), (3, 101), (2, 4096), (4, 4097), (3, 8193)):
        S.add(sprinkle(fam(rng, n, L)) if L > 101 else fam(rng, n, L), ("keep",), "whole %d" % L)
    # the first failing frame at f: a burst at f + 89 (f = 0: anywhere up to column 89)
    for n, L, f in ((2, 400, 0), (2, 400, 15), (3, 400, 16), (2, 400, 17), (2, 4400, 4095), (3, 4400, 4096),
                    (2, 400, 300), (2, 4196, 4096), (3, 4195, 4095)):
        p = 50 if f == 0 else min(f + 89, L - 11)
        S.add(burst(rng, n, L, p), None, "burst first failing frame %d of %d" % (f, L))
    # ... and that frame alone failing
    for n, L, i in ((2, 400, 15), (2, 400, 16), (3, 400, 17), (2, 420, 31), (2, 4400, 3855), (2, 4400, 4095),
                    (3, 4400, 4096), (2, 400, 300), (3, 4196, 4096), (2, 8400, 8191), (2, 300, 0)):
        S.add(isolated_frame(rng, n, L, i), None, "isolated frame %d of %d" % (i, L))
    S.add([], ("drop",), "empty")
    # ident-gap runs around the tile seam: the last column 4095, the last column 4096, the first column 4096, across
    for ln in GAP_RUNS:
        for name, a in (("ends_4095", 4096 - ln), ("ends_4096", 4097 - ln), ("starts_4096", 4096),
                        ("across", 4096 - (ln + 1) // 2)):
            n = 2 + (ln + len(name)) % 3
            S.add(gap(fam(rng, n, 4400), a, a + ln), None, "gap_run %d %s" % (ln, name))
    S.add(fam(rng, 2, 150), None, "unaligned", with_rows=False)  # no rows: not scored, kept
    S.add(fam(rng, 3, 50), ("drop",), "too_short")
    for ln in (5, 100):
        S.add(gap(fam(rng, 3, 400), 0, ln, rows=(1,)), None, "gap_run %d at 0" % ln)
        S.add(gap(fam(rng, 3, 4200), 4200 - ln, 4200, rows=(2,)), None, "gap_run %d at L-1" % ln)
    M = fam(rng, 3, 300)
    M[:, 150] = _N
    S.add(M, None, "N column")
    M = fam(rng, 3, 300)
    M[1, 150] = _N
    M[2, 151] = _N
    gap(M, 151, 152, rows=(0,))  # a gap and an N in one column: no ident-gap column
    S.add(M, None, "N letter")
    S.add(gap(fam(rng, 3, 300), 150, 151, rows=(0, 2)), None, "gaps but one")
    S.add(gap(fam(rng, 3, 300), 150, 151, rows=(0, 1, 2)), None, "pure gap column")
    S.add(fam(rng, 2, 99), ("drop",), "too_short")
    # 40,000 columns, an ident-gap run of 1,001 at 20,000: slices of 20,000 and 18,999 columns, each row more than
    # one COUNT_PIECE; single gaps before the cut, so the letters before a slice are fewer than the columns
    M = fam(rng, 4, 40000)
    gap(M, 20000, 21001, rows=(3,))
    for r, c in ((0, 500), (1, 9000), (1, 16384), (2, 16383), (3, 19000), (0, 30000)):
        gap(M, c, c + 1, rows=(r,))
    S.add(M, None, "long 40000")
    S.add(fam(rng, 1, 300), ("drop",), "one_fragment")  # fewer than min_block
    return S


def _filter_long_runs():
    """min_fragment 2000, frame_length 100: runs of 999, 1000 and 1001 columns
    score c_log_score[999] (capped before the comparison with min_fragment)."""
    S = Cases(47, dict(min_fragment=2000, frame_length=100))
    rng = S.rng
    for ln in (999, 1000, 1001):
        S.add(gap(fam(rng, 3, 6000), 2500, 2500 + ln), None, "gap_run %d" % ln)
        S.add(gap(fam(rng, 2, 7000), 4096 - ln, 4096, rows=(0,)), None, "gap_run %d ends_4095" % ln)
    S.add(gap(fam(rng, 2, 7000), 2100, 4100, rows=(0,)), None, "gap_run 2000")
    S.add(sprinkle(fam(rng, 2, 2000)), ("keep",), "whole")
    S.add(fam(rng, 2, 1999), ("drop",), "too_short")
    S.add(burst(rng, 3, 4300, 2100), None, "burst")
    S.add(sprinkle(fam(rng, 3, 4097)), ("keep",), "whole")
    S.add(bad_ends(rng, 2, 2100, 5, 64), None, "bad_ends")
    return S


def _filter_no_subblocks():
    S = Cases(53, dict(find_subblocks=0))
    rng = S.rng
    S.add(sprinkle(fam(rng, 2, 300)), ("keep",), "whole")
    S.add(burst(rng, 2, 400, 200), ("drop",), "burst")
    S.add(fam(rng, 2, 150), ("keep",), "unaligned", with_rows=False)
    S.add(burst(rng, 3, 4400, 4090, k=30), ("drop",), "burst")
    S.add(sprinkle(fam(rng, 3, 4097)), ("keep",), "whole")
    return S


FLIP_KW = dict(min_fragment=1, frame_length=1, min_end=1, min_identity_x1e4=600, min_block=2)
FLIP_ANSWER = [(0, 0, 0, 1, "A"), (1, 9, 9, 1, "T"), (2, 0, 0, 1, "T")]


def _flip():
    """The orientation flip as a known answer, FixEnds' and Filter's alike:
    the slice is column 9 alone, the ori -1 row's one letter there is position
    0 of its sequence, turned to ori +1 and written as the forward strand's
    (k_set_letter).

    A flip inside a slice of two or more columns was looked for with the
    oracle and not found: 6,000 random blocks of 2-4 rows and 2-12 columns,
    rows of one letter among gaps, under four low-identity option sets gave
    2,219 one-column flips and no wider one.  It cannot be reached: both end
    columns of a Filter slice score MAX_COLUMN_SCORE (goodLeftEnd /
    goodRightEnd) and both ends of FixEnds' slice are is_ident_nogap columns,
    so every row of a slice has a letter in its first and in its last column.
    """
    S = Cases(59, FLIP_KW, pad=False)
    S.add(["AAAAAAATTT", "AAATAAATTT", "---------T"], ("literal", [FLIP_ANSWER]), "flip", oris=(-1, 1, 1))
    return S


@functools.lru_cache(maxsize=None)
def filter_edges():
    """(name, Cases) per option group; see the builders."""
    return (("default", _filter_default()), ("long_runs", _filter_long_runs()),
            ("no_subblocks", _filter_no_subblocks()), ("flip", _flip()))


INVALID_CASES = ("drop_then_keep", "drop_then_slice", "drop_then_gone", "drop_no_subblocks", "all_valid_control")


def _invalid_rows(rng, n, L, burst_at=None):
    """n rows of L columns: the last row differs from the first in every
    column (no frame passes with it), the rows before it are equal but for 30
    mismatching columns from burst_at on in the last of them."""
    M = fam(rng, n, L)
    mismatch(M, np.arange(L), row=n - 1)
    if burst_at is not None:
        mismatch(M, np.arange(burst_at, burst_at + 30), row=n - 2)
    return M


@functools.lru_cache(maxsize=None)
def filter_invalid(name):
    """One block whose last fragment is invalid: its sequence ends at its max
    (`at`) or 5 letters before it (`past`), the row keeps max - min + 1
    letters.  Filter drops that fragment and tries the rest again
    (Filter.cpp:230-246).  invalid_result() holds each case's outcome;
    all_valid_control leaves the sequence whole."""
    n, L, burst_at, kw, past = {
        "drop_then_keep": (3, 300, None, {}, 0),
        "drop_then_slice": (3, 400, 185, {}, 5),
        "drop_then_gone": (2, 300, None, {}, 0),
        "drop_no_subblocks": (3, 300, None, dict(find_subblocks=0), 5),
        "all_valid_control": (3, 400, 185, {}, None),
    }[name]
    S = Cases(67, kw)
    k = S.add(_invalid_rows(S.rng, n, L, burst_at), None, name)
    if past is not None:
        q, _, mx = S.blocks[k][-1][:3]
        S.seqs[q] = S.seqs[q][:mx - past]
        assert len(S.seqs[q]) <= mx
    return S


def invalid_result(name):
    """The oracle's Filter output of filter_invalid(name), its outcome
    asserted: a case that degenerates fails here."""
    S = filter_invalid(name)
    want = S.result("Filter")
    blk = S.blocks[0]
    if name in ("drop_then_keep", "drop_no_subblocks"):
        assert len(want) == 1 and sorted(want[0]) == sorted(blk[:2]), name
    elif name == "drop_then_slice":
        assert len(want) == 2 and all(len(b) == 2 and {f[0] for f in b} == {blk[0][0], blk[1][0]} for b in want), name
    elif name == "drop_then_gone":
        assert want == [], name
    else:
        other = filter_invalid("drop_then_slice")
        assert [[f[1:] for f in b] for b in S.blocks] == [[f[1:] for f in b] for b in other.blocks]
        assert sorted(map(sorted, want)) != sorted(map(sorted, other.result("Filter"))), name
    return S, want


# ---------------------------------------------------------------- sweep
SWEEP_LENGTHS = (1, 63, 64, 65, 99, 100, 101, 127, 128, 129, 255, 256, 257, 4031, 4032, 4033, 4095, 4096, 4097,
                 4159, 4160, 8191, 8192, 8193, 16383, 16384, 16385, 33000)
SWEEP_ROWS = (2, 3, 4, 5, 9, 70)
SEAM_ENDS = (1, 2, 15, 16, 17, 63, 64, 65)


def _sweep_block(rng, n, L):
    """One block of the sweep and what was put into it."""
    M = fam(rng, n, L)
    what = []
    u = rng.random()
    if L < MIN_FRAGMENT or u < 0.33:
        if L > 140:
            sprinkle(M, step=int(rng.integers(23, 60)))
        return M, ["clean"]
    if u < 0.38:  # unrelated rows
        M[n - 1] = _LETTERS[rng.integers(0, 4, L)]
        return M, ["noise"]
    room = L - MIN_FRAGMENT
    ends = rng.random() < 0.55
    middle = L >= 255 and (not ends or rng.random() < 0.75)
    if not (ends or middle):
        ends = True
    lo, hi = 0, L
    if ends:
        fit = [e for e in SEAM_ENDS if e <= room // (3 if middle else 1)] or [0]
        bl = int(rng.choice(fit + [0]))
        br = int(rng.choice([e for e in fit if bl + e <= room // (3 if middle else 1)] + [0]))
        if bl + br == 0:
            bl = min(1, room)
        r = int(rng.integers(0, n))
        if rng.random() < 0.3 and n > 2:  # the bad end is a row that starts late: an ident-gap run at the end
            gap(M, 0, bl, rows=(r,))
            gap(M, L - br, L, rows=(r,))
        else:
            mismatch(M, np.r_[0:bl, L - br:L], row=r)
        lo, hi = bl, L - br
        what.append("ends %d+%d" % (bl, br))
    if middle:
        # something bad between two stretches of at least 100 good columns
        kind = rng.choice(["burst", "gap_run", "n_run", "sparse"], p=[0.4, 0.35, 0.15, 0.1])
        free = (hi - lo) - 2 * (MIN_FRAGMENT + 5)
        ln = int(rng.choice(GAP_RUNS)) if kind != "burst" else int(rng.integers(11, 40))
        ln = max(1, min(ln, free))
        if kind == "sparse" and n >= 3:  # a row of few letters: gaps from a column on
            a = lo + MIN_FRAGMENT + 5 + int(rng.integers(0, max(free - ln, 0) + 1))
            gap(M, a, hi, rows=(int(rng.integers(1, n)),))
            what.append("sparse from %d" % a)
        elif free >= 1:
            a = lo + MIN_FRAGMENT + 5 + int(rng.integers(0, free - ln + 1))
            r = int(rng.integers(0, n))
            if kind == "burst":
                mismatch(M, np.arange(a, a + ln), row=r)
            elif kind == "n_run":
                M[:, a:a + ln] = _N
            else:
                gap(M, a, a + ln, rows=(r,))
            what.append("%s %d at %d" % (kind, ln, a))
    return M, what


@functools.lru_cache(maxsize=None)
def sweep(seed):
    """Random blocks at the seam lengths: clean ones with a few mismatches,
    bad ends of seam lengths (mismatches, or a row that starts late), a
    mismatch burst, an ident-gap run (GAP_RUNS), an N run or a sparse row in
    the middle, unrelated rows.  The densities are tuned on the oracle
    (test_column_cases_ref.test_sweep_outcomes): both processors keep, change
    and drop a fair share each."""
    S = Cases(1000 + seed)
    rng = S.rng
    total = 0
    for rnd in range(5):
        for L in SWEEP_LENGTHS:
            if rnd == 4 and L > 4200:
                continue
            rows = [r for r in SWEEP_ROWS if r * L <= (300000 if r < 70 else 100000)]
            n = int(rng.choice(rows))
            if L in (129, 4097, 4160) and rnd == seed % 3:
                n = 70
            M, what = _sweep_block(rng, n, L)
            total += M.size
            S.add(M, None, "%dx%d %s" % (n, L, ", ".join(what)))
    assert 100 <= len(S.blocks) <= 150 and total < 5_000_000, (len(S.blocks), total)
    return S


# ---------------------------------------------------------------- consensus
CONS_SHAPES = ((1, 1), (2, 255), (3, 256), (2, 257), (5, 4097), (65, 130), (300, 70))


def vote(rows):
    """Block::consensus of an aligned block in plain Python: per column the
    counts of A T G C N over the rows, the first maximum wins, a column without
    letters gives A."""
    out = []
    for c in range(len(rows[0])):
        counts = [sum(r[c] == x for r in rows) for x in "ATGCN"]
        out.append("ATGCN"[counts.index(max(counts))])
    return "".join(out)


@functools.lru_cache(maxsize=None)
def consensus_edges():
    """Aligned blocks at CONS_SHAPES (one k_consensus tile is 256 columns) of
    random letters, N and gaps, a block whose columns tie every pair of A T G C
    N in both row orders, columns of gaps only, N majorities and three-way
    ties; the pairs again on the columns around 256.  The blocks are in
    consensus_order."""
    S = Cases(61)
    rng = S.rng
    alphabet = np.frombuffer(b"ATGCN-", dtype=np.uint8)
    for n, L in CONS_SHAPES:
        M = alphabet[rng.choice(6, size=(n, L), p=[0.2, 0.2, 0.2, 0.2, 0.08, 0.12])]
        M[:, 0] = _LETTERS[rng.integers(0, 4, n)]  # (every fragment has a letter)
        if (n, L) == (2, 257):
            pairs = [(x, y) for x in "ATGCN" for y in "ATGCN" if x != y]
            for k, (x, y) in enumerate(pairs):
                M[0, 246 + k % 11], M[1, 246 + k % 11] = ord(x), ord(y)
            M[:, 255] = (_N, _C)
            M[:, 256] = (_C, _N)
            M[:, 245] = _GAP
        S.add(M, None, "%dx%d" % (n, L), oris=[1 if i % 2 == 0 else -1 for i in range(n)])
    pairs = [(x, y) for x in "ATGCN" for y in "ATGCN" if x != y]
    S.add(["".join(x for x, _ in pairs) + "-A", "".join(y for _, y in pairs) + "-C"], None, "pairs")
    # N majority, N against one letter and gaps, gaps only, three-way ties in every rotation, N tie with a gap
    S.add(["NN-TGCA-N", "NN-GCAN-T", "N--CATG--", "A-T------"], None, "majorities")
    order = sorted(range(len(S.blocks)), key=lambda k: orc.consensus_order(S.blocks[k]))
    S.blocks = [S.blocks[k] for k in order]
    S.tags = [S.tags[k] for k in order]
    S.expect = [S.expect[k] for k in order]
    return S
