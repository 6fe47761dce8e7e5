"""Seam and edge inputs of the MoveGaps / CutGaps kernels (k_gap_ends,
k_move_gaps, k_cut_counts, k_gapless and gap_pass around them,
npge_amd/csrc/block_build.hip), shared by test_gap_cases_ref.py (the oracle
alone, on the CPU: the closed forms and the spread of outcomes) and
test_gap_shapes_gpu.py (engine against oracle, bit for bit).

Blocks are column_cases.Cases' : every row on a sequence of its own, every odd
row ori -1, rows of random letters (a wrong copy shows).  GapCases adds
MoveGaps' two options and loose rows: rows given by the caller with fewer
letters than their fragment, or with none.

The rules in plain Python (the ref file holds them against the oracle):

* MoveGaps (MoveGaps.cpp:30-103): the left tail of t letters (counted up to
  max_tail + 1) moves behind the g gaps after it exactly when 1 <= t <=
  max_tail, g >= 1, t * 10000 // g <= max_tail_to_gap_x1e4 and t + g <=
  L // 2 - 1; the row becomes '-' * g + tail + rest.  The right side mirrors
  this with the same L // 2.  g >= 1 cannot fail alone: with t <= max_tail
  the column after the tail is a gap or the row's end, so g = 0 is a row of
  letters only, where t + g = L fails the last condition as well.
* permissive CutGaps (CutGaps.cpp:105-134): from = the largest first-letter
  column, to = the smallest last-letter column over the rows with letters;
  strict (:63-103): the first and the last column without a gap.  from > to
  clears the block (it stays in the set, empty); a row without a letter in
  [from, to] leaves the block; the orientation is kept.
"""
import functools

import numpy as np

from oracle import oracle as orc

import column_cases as cc

SEAMS = (0, 1, 63, 64, 65, 127, 128, 129, 200)
RULE_T = (1, 63, 64, 65, 127, 128, 129, 200, 201)
RULE_G = (63, 64, 65, 128, 130)
OVERLAPPING = ((70, 14), (130, 26), (200, 40), (65, 13))
COMBINED_G = (3, 63, 64, 65, 130)
ENGINE_OP = {"CutGaps": "CutGaps", "CutGapsStrict": "CutGaps --cut-strict=1", "LiteAlign": "LiteAlign",
             "Align": "Align"}


# ---------------------------------------------------------------- the rules
def conditions(t, g, L, max_tail, x1e4):
    """The four conditions of a move, in the order of the module's docstring."""
    return (1 <= t <= max_tail, g >= 1, g >= 1 and t * 10000 // g <= x1e4, t + g <= L // 2 - 1)


def left_end(row, max_tail):
    """(t, g) of the row's left end: letters before the first gap, counted up
    to max_tail + 1, and the gaps after them."""
    t = 0
    while t < len(row) and t <= max_tail and row[t] != "-":
        t += 1
    g = 0
    while t + g < len(row) and row[t + g] == "-":
        g += 1
    return t, g


def move_row(row, max_tail, x1e4):
    """MoveGaps on one row: (the new row, the left tail moved, the right one)."""
    L = len(row)
    tl, gl = left_end(row, max_tail)
    tr, gr = left_end(row[::-1], max_tail)
    ml, mr = all(conditions(tl, gl, L, max_tail, x1e4)), all(conditions(tr, gr, L, max_tail, x1e4))
    if ml:
        row = "-" * gl + row[:tl] + row[tl + gl:]
    if mr:
        row = row[:L - tr - gr] + row[L - tr:] + "-" * gr
    return row, ml, mr


def permissive_span(rows):
    L = len(rows[0])
    a, b = 0, L - 1
    for r in rows:
        s = r.strip("-")
        if s:
            a = max(a, len(r) - len(r.lstrip("-")))
            b = min(b, L - 1 - (len(r) - len(r.rstrip("-"))))
    return a, b


def strict_span(rows):
    L = len(rows[0])
    ok = [all(r[c] != "-" for r in rows) for c in range(L)]
    if not any(ok):
        return L, L - 1
    return ok.index(True), L - 1 - ok[::-1].index(True)


def cut_block(blk, a, b):
    """CutGaps' slice of columns [a, b]: [the block], [[]] when it is cleared."""
    L = len(blk[0][4])
    if (a, b) == (0, L - 1):
        return [list(blk)]
    if b < a:
        return [[]]
    out = []
    for (q, mn, mx, ori, row) in blk:
        before = a - row.count("-", 0, a)
        cnt = (b + 1 - a) - row.count("-", a, b + 1)
        if not cnt:
            continue
        begin = mn if ori == 1 else mx
        s0, s1 = begin + ori * before, begin + ori * (before + cnt - 1)
        out.append((q, min(s0, s1), max(s0, s1), ori, row[a:b + 1]))
    return [out]


def lite_align(blk, max_tail=3, x1e4=10000):
    """LiteAlign on an aligned block of two or more rows: MoveGaps and
    permissive CutGaps until nothing changes; (the block, the laps that
    changed it)."""
    laps = 0
    while blk:
        moved = [f[:4] + (move_row(f[4], max_tail, x1e4)[0],) for f in blk]
        (new,) = cut_block(moved, *permissive_span([f[4] for f in moved]))
        if new == blk:
            break
        blk, laps = new, laps + 1
    return blk, laps


# ---------------------------------------------------------------- rows
def letters(rng, n):
    return "".join("ATGC"[x] for x in rng.integers(0, 4, n))


def tail(rng, t, g):
    """t random letters, each another one than the letter g places before it:
    where a move overlaps its source (g < t), a letter copied from the wrong
    place, or not copied at all, is never right by chance."""
    out = []
    for i in range(t):
        x = "ATGC"[int(rng.integers(0, 4))]
        if i >= g and x == out[i - g]:
            x = "ATGC"[("ATGC".index(x) + 1 + int(rng.integers(0, 3))) % 4]
        out.append(x)
    return "".join(out)


def end_row(rng, L, left=(0, 0), right=(0, 0), inner=0):
    """t letters and g gaps from the left (t 0: the row starts with g gaps),
    the same from the right, letters between them with `inner` single gaps
    away from their ends."""
    (tl, gl), (tr, gr) = left, right
    m = L - tl - gl - tr - gr
    assert m >= 1, (L, left, right)
    mid = list(letters(rng, m))
    if inner and m >= 12:
        for c in rng.integers(m // 3, 2 * m // 3, inner):
            mid[int(c)] = "-"
    return tail(rng, tl, gl) + "-" * gl + "".join(mid) + "-" * gr + tail(rng, tr, gr)[::-1]


class GapCases(cc.Cases):
    """column_cases.Cases with MoveGaps' options, loose rows and the
    expectations ("rows", rows) (the fragments as they are, these rows),
    ("cut", from, to) and ("clear",)."""

    def __init__(self, seed, max_tail=3, x1e4=10000):
        super().__init__(seed)
        self.max_tail, self.x1e4 = max_tail, x1e4
        self.meta = []  # per block what a test wants to know of it

    def oracle(self):
        return orc.BlockSetOracle(list(self.seqs), list(self.names), max_tail=self.max_tail,
                                  max_tail_to_gap_x1e4=self.x1e4)

    def engine_op(self, op):
        """The engine's processor string of the oracle's op."""
        if op != "MoveGaps":
            return ENGINE_OP[op]
        ratio = ("%d.%04d" % divmod(self.x1e4, 10000)).rstrip("0").rstrip(".")
        return "MoveGaps --max-tail=%d --max-tail-to-gap=%s" % (self.max_tail, ratio)

    def add(self, rows, expect=None, tag="", meta=None, **kw):
        k = super().add(rows, expect, tag, **kw)
        self.meta.append(meta)
        return k

    def add_loose(self, rows, extra, expect=None, tag="", meta=None):
        """Rows whose fragments are `extra[i]` letters longer than the row
        says; a row without letters is allowed (its fragment is the extra)."""
        blk = []
        for i, (row, x) in enumerate(zip(rows, extra)):
            ori = 1 if i % 2 == 0 else -1
            text = row.replace("-", "") + letters(self.rng, x)
            assert text
            left = self._pad()
            self.seqs.append(left + (text if ori == 1 else cc.revcomp(text)) + self._pad())
            self.names.append("g%d&c&c" % len(self.names))
            blk.append((len(self.seqs) - 1, len(left), len(left) + len(text) - 1, ori, row))
        self.blocks.append(blk)
        self.expect.append(expect)
        self.tags.append(tag)
        self.meta.append(meta)
        return len(self.blocks) - 1

    def add_moved(self, rows, tag, meta=None):
        """A MoveGaps case: the closed form is move_row on every row."""
        want = [move_row(r, self.max_tail, self.x1e4)[0] for r in rows]
        return self.add(rows, ("rows", want), tag, meta=meta)

    def add_cut(self, rows, span, tag, strict=False, loose=None, meta=None):
        """A CutGaps case that comes out as columns span = (from, to)."""
        assert (strict_span if strict else permissive_span)(rows) == tuple(span), (tag, span)
        L = len(rows[0])
        e = ("keep",) if tuple(span) == (0, L - 1) else ("clear",) if span[1] < span[0] else ("cut",) + tuple(span)
        if loose is None:
            return self.add(rows, e, tag, meta=meta)
        return self.add_loose(rows, loose, e, tag, meta=meta)

    def expected(self, k):
        e = self.expect[k]
        if e is not None and e[0] == "rows":
            return [[f[:4] + (r,) for f, r in zip(self.blocks[k], e[1])]]
        if e is not None and e[0] == "cut":
            return [b for b in cut_block(self.blocks[k], e[1], e[2])]
        if e is not None and e[0] == "clear":
            return []  # (the cleared block is among split()'s None)
        return super().expected(k)

    def cleared(self):
        """How many blocks the closed forms leave empty (the empty inputs too)."""
        return sum(not b or (e is not None and e[0] == "clear") for b, e in zip(self.blocks, self.expect))


# ---------------------------------------------------------------- MoveGaps
def _rule_pairs():
    return [(t, g) for t in RULE_T for g in sorted({t} | set(RULE_G)) if g >= t]


@functools.lru_cache(maxsize=None)
def move_rule_edges():
    """max_tail 200, ratio 1.0.  Every (t, g) of RULE_T x ({t} + RULE_G), g >=
    t, at t + g = L // 2 - 1 (moves) and t + g = L // 2 (stays) with L even
    and odd: a block of a left case (ori +1), a right case (ori -1), and, where
    they move, a row whose both ends move and one of inner gaps.  t = 201
    never moves.  Tails of 65 to 200 letters take k_move_gaps through its
    second, third and fourth chunk, 63 / 64 / 65 and 127 / 128 / 129 put `from`
    and `to` on and beside its 64-column seams; g = 63 / 64 / 65 / 128 / 130
    ends first_col's / last_col's windows there.

    Then: a row that starts / ends with a gap, rows of letters only, L = 1, 2
    and 3, max_tail >= L, and rows where one end moves while the other fails
    one single condition (t = 0, t = max_tail + 1, the ratio, t + g = L // 2).
    meta: ("edge", t, g, moves) per rule block, ("one_fails", side, i) else.
    """
    S = GapCases(71, 200, 10000)
    rng = S.rng
    for t, g in _rule_pairs():
        for half, moves in ((t + g + 1, True), (t + g, False)):
            for L in (2 * half, 2 * half + 1):
                rows = [end_row(rng, L, left=(t, g)), end_row(rng, L, right=(t, g))]
                if moves:
                    rows.append(end_row(rng, L, left=(t, g), right=(t, g)))
                rows.append(end_row(rng, L, inner=3))
                S.add_moved(rows, "edge t%d g%d L%d" % (t, g, L), meta=("edge", t, g, moves and t <= 200))
    S.add_moved([end_row(rng, 300, left=(0, 7)), end_row(rng, 300, right=(0, 7)), end_row(rng, 300)], "starts with gap")
    S.add_moved([letters(rng, 150), letters(rng, 150)], "letters only")
    for L in (1, 2, 3):
        S.add_moved([letters(rng, L), letters(rng, L)], "L%d" % L)
    S.add_moved(["A-", "-T", "G-"], "L2 gap")
    S.add_moved(["A-C", "-TA", "G--", "--C"], "L3 gap")
    # max_tail >= L: the tail is counted to the row's end
    S.add_moved([letters(rng, 40), end_row(rng, 40, left=(2, 5)), end_row(rng, 40, right=(19, 1)),
                 end_row(rng, 40, left=(1, 18))], "max_tail >= L")
    # one end moves (2, 5), the other fails one condition alone (L = 430: L // 2 - 1 = 214; L = 900: 449)
    for side in ("left", "right"):
        for i, bad, L in ((0, (0, 9), 430), (0, (201, 201), 900), (2, (3, 2), 430), (3, (100, 115), 430)):
            row = end_row(rng, L, left=bad, right=(2, 5)) if side == "left" else end_row(rng, L, left=(2, 5), right=bad)
            S.add_moved([row, end_row(rng, L, inner=2)], "one_fails %s %d" % (side, i),
                        meta=("one_fails", side, i, bad))
    return S


@functools.lru_cache(maxsize=None)
def move_max_tail_0():
    """max_tail 0: nothing moves, whatever the rows."""
    S = GapCases(73, 0, 10000)
    rng = S.rng
    S.add_moved([end_row(rng, 200, left=(1, 5)), end_row(rng, 200, right=(1, 64)), end_row(rng, 200, left=(0, 3))],
                "max_tail 0")
    S.add_moved([end_row(rng, 7, left=(1, 1)), end_row(rng, 7)], "max_tail 0 short")
    return S


@functools.lru_cache(maxsize=None)
def move_ratio_edges():
    """(name, GapCases) per ratio: 0.5 -- (32, 64) moves, (33, 64) stays;
    0.3333 -- (1, 3) moves (1 * 10000 // 3 = 3333, truncated), (2, 5) stays
    (4000); 5.0 -- the overlapping moves of OVERLAPPING (gl < tl: the
    destination overlaps the source, the tail spans two to four chunks of
    k_move_gaps) on the left, on the right and on both ends; (71, 14) stays."""
    out = []
    for name, x1e4, yes, no in (("0.5", 5000, [(32, 64)], [(33, 64)]), ("0.3333", 3333, [(1, 3)], [(2, 5)]),
                                ("5", 50000, list(OVERLAPPING), [(71, 14)])):
        S = GapCases(79 + x1e4 % 7, 200, x1e4)
        rng = S.rng
        for moves, pairs in ((True, yes), (False, no)):
            for t, g in pairs:
                for L in (2 * (t + g + 1), 2 * (t + g + 1) + 65):
                    rows = [end_row(rng, L, left=(t, g)), end_row(rng, L, right=(t, g)),
                            end_row(rng, L, left=(t, g), right=(t, g)), end_row(rng, L, inner=2)]
                    S.add_moved(rows, "ratio %s t%d g%d L%d" % (name, t, g, L), meta=("edge", t, g, moves))
        out.append((name, S))
    return tuple(out)


# ---------------------------------------------------------------- CutGaps
def _lead_rows(rng, L, leads, trails, inner=2):
    return [end_row(rng, L, left=(0, a), right=(0, b), inner=inner) for a, b in zip(leads, trails)]


@functools.lru_cache(maxsize=None)
def cut_edges():
    """Permissive CutGaps.  Leads and trails of SEAMS in different rows of
    one block, each seam once the largest lead (= from) and once the largest
    trail (k_cut_counts' before / after windows end on, before and after a
    64-column seam; the row offsets move by from); from == to; from > to (the
    block is cleared and stays in the set); rows whose letters all lie outside
    [from, to] (erased), so that one fragment is left; one-letter ori -1
    fragments (the orientation is kept); blocks nothing cuts.
    meta: the number of fragments erased."""
    S = GapCases(83)
    rng = S.rng
    for j, v in enumerate(SEAMS):
        w = SEAMS[len(SEAMS) - 1 - j]
        leads = [x for x in SEAMS if x <= v]
        trails = [x for x in SEAMS if x <= w]
        n = max(len(leads), len(trails), 2)
        leads = (leads * n)[:n] if v else [0] * n
        trails = (trails[::-1] * n)[:n] if w else [0] * n
        for L in (512 + j, 449):
            rows = _lead_rows(rng, L, leads, trails)
            S.add_cut(rows, (v, L - 1 - w), "seams lead %d trail %d L%d" % (v, w, L), meta=0)
    # from == to: one column
    L = 140
    rows = [end_row(rng, L, left=(0, 70)), end_row(rng, L, right=(0, L - 71)), end_row(rng, L)]
    rows.append(rows[2][:70] + "-" + rows[2][71:])  # no letter in column 70
    S.add_cut(rows, (70, 70), "from == to", meta=1)
    S.add_cut([end_row(rng, 9, left=(0, 4)), end_row(rng, 9, right=(0, 4))], (4, 4), "from == to short", meta=0)
    # from > to
    S.add_cut([end_row(rng, L, left=(0, 80)), end_row(rng, L, right=(0, 90)), end_row(rng, L)], (80, 49), "from > to")
    S.add_cut(["--A", "C--"], (2, 0), "from > to short")
    # letters outside [from, to] only
    S.add_cut(["A--------T", "--CCGATC--", "TCCATGATAG"], (2, 7), "outside", meta=1)
    rows = [letters(rng, 1) + "-" * 198 + letters(rng, 1), end_row(rng, 200, left=(0, 66), right=(0, 129)),
            letters(rng, 65) + "-" * 130 + letters(rng, 5)]
    S.add_cut(rows, (66, 70), "outside, one fragment left", meta=2)
    S.add_cut([end_row(rng, 130, left=(0, 65), right=(0, 10)), letters(rng, 30) + "-" * 95 + letters(rng, 5)],
              (65, 119), "cut down to one fragment", meta=1)
    # one letter of an ori -1 fragment (row 1, row 3) is left
    rows = [end_row(rng, 150, left=(0, 64), right=(0, 21)), letters(rng, 3) + "-" * 97 + "G" + "-" * 45 + letters(rng, 4),
            end_row(rng, 150, inner=3), letters(rng, 2) + "-" * 68 + "T" + "-" * 78 + letters(rng, 1)]
    S.add_cut(rows, (64, 128), "one letter ori -1", meta=0)
    S.add_cut([end_row(rng, 300, inner=4), end_row(rng, 300, inner=2), end_row(rng, 300)], (0, 299), "untouched")
    S.add([], ("keep",), "empty")
    S.add_cut([letters(rng, 1), letters(rng, 1)], (0, 0), "L1")
    S.add_cut([end_row(rng, 64, left=(0, 63)), letters(rng, 64)], (63, 63), "lead L - 1", meta=0)
    return S


LOOSE_WIDTHS = (1, 63, 64, 65, 130)


@functools.lru_cache(maxsize=None)
def loose_edges(strict):
    """Loose rows under CutGaps (strict: CutGapsStrict): rows with fewer
    letters than their fragment, so k_cut_counts counts the letters inside
    [from, to] (CutOp.full) instead of taking them from the fragment's length,
    with [from, to] 1, 63, 64, 65 and 130 columns wide at from = 0, 1, 63 and 64
    (the inside loop's windows start at from); rows without any letter (they
    set nothing and are erased; under strict they leave no gapless column:
    cleared); a loose row beside exact ones.  meta: fragments erased."""
    S = GapCases(89 + strict)
    rng = S.rng
    for w in LOOSE_WIDTHS:
        for a in (0, 1, 63, 64):
            if a == 0 and w == 1:
                continue
            L = a + w + (70 if a % 2 else 3)
            b = a + w - 1
            rows = [end_row(rng, L, left=(0, a), inner=0 if strict else 2),
                    end_row(rng, L, right=(0, L - 1 - b), inner=0 if strict else 2),
                    end_row(rng, L, inner=0 if strict else 3)]
            erased = 0
            if not strict:  # a row without letters and one with letters outside only
                rows.append("-" * L)
                erased = 1
                if a >= 1:
                    rows.append(letters(rng, a) + "-" * (L - a - 1) + letters(rng, 1))
                    erased = 2
            extra = [1 + (i * 7 + w) % 5 for i in range(len(rows))]
            S.add_cut(rows, (a, b), "loose width %d from %d" % (w, a), strict=strict, loose=extra, meta=erased)
    L = 100
    rows = [end_row(rng, L, left=(0, 10)), end_row(rng, L, right=(0, 20)), "-" * L]
    if strict:
        S.add_cut(rows, (L, L - 1), "no letter: no gapless column", strict=True, loose=[2, 0, 5])
    else:
        S.add_cut(rows, (10, 79), "no letter", loose=[2, 0, 5], meta=1)
    rows = [end_row(rng, L, left=(0, 5)), end_row(rng, L), end_row(rng, L, right=(0, 64))]
    S.add_cut(rows, (5, 35), "one loose row", strict=strict, loose=[0, 3, 0], meta=0)
    S.add_cut([end_row(rng, L), end_row(rng, L)], (0, L - 1), "loose untouched", strict=strict, loose=[4, 1])
    return S


def strict_rows(rng, n, L, first, last, block_window=False):
    """n rows of L columns: a gap in every column before `first` and after
    `last` (in one row, or two), none in those two, a few between them.
    block_window: row 0 is gaps over the whole first 64-column window at both
    ends, so k_gapless leaves the row loop early there."""
    M = cc._LETTERS[rng.integers(0, 4, (n, L))]
    cols = np.r_[0:first, last + 1:L]
    M[(cols * 7 + 3) % n, cols] = cc._GAP
    if n > 2:
        M[(cols[::2] * 5 + 1) % n, cols[::2]] = cc._GAP
    if last - first > 4:
        inner = rng.integers(first + 1, last, 3)
        M[rng.integers(0, n, 3), inner] = cc._GAP
    if block_window:
        M[0, :64] = cc._GAP
        M[0, L - 64:] = cc._GAP
    for r in range(n):  # (every fragment has a letter)
        if (M[r] == cc._GAP).all():
            M[r, first] = cc._A
    return [r.tobytes().decode() for r in M]


STRICT_ROWS = (1, 2, 64, 65, 300)


@functools.lru_cache(maxsize=None)
def strict_edges():
    """Strict CutGaps.  The first gapless column at 0, 1, 63, 64, 65, 128 and
    L - 1, the last one mirrored from the row's end, with L % 64 in {0, 1, 63}
    (k_gapless walks 64-column windows from column 0 and from column L - 1);
    exactly one gapless column; none (cleared); 1, 2, 64, 65 and 300 rows (300
    rows of at most 200 columns; more rows than a wave has lanes change
    nothing, the rows are a loop); blocks whose first window at either end is
    refused by row 0 alone (`if (!__ballot(ok)) break`) and whose answer lies
    in the second."""
    S = GapCases(97)
    rng = S.rng
    k = 0
    for L in (256, 257, 319):
        for f in (0, 1, 63, 64, 65, 128, L - 1):
            n = STRICT_ROWS[1 + k % 3]
            k += 1
            if f == L - 1:
                S.add_cut(strict_rows(rng, n, L, f, f), (f, f), "strict first L-1 L%d" % L, strict=True)
                S.add_cut(strict_rows(rng, n, L, 0, 0), (0, 0), "strict last 0 L%d" % L, strict=True)
                continue
            S.add_cut(strict_rows(rng, n, L, f, L - 2 - (k % 2)), (f, L - 2 - (k % 2)), "strict first %d L%d" % (f, L),
                      strict=True)
            S.add_cut(strict_rows(rng, n, L, k % 2, L - 1 - f), (k % 2, L - 1 - f), "strict last L-1-%d L%d" % (f, L),
                      strict=True)
            S.add_cut(strict_rows(rng, n, L, f, f), (f, f), "strict one column %d L%d" % (f, L), strict=True)
    for n in STRICT_ROWS:
        L = 200 if n == 300 else 257
        S.add_cut(strict_rows(rng, n, L, 65, 128), (65, 128), "strict %d rows" % n, strict=True)
        if n > 1:
            rows = [list(r) for r in strict_rows(rng, n, L, 65, 128)]
            for c in range(65, 129):
                rows[(c * 3 + 1) % n][c] = "-"
            S.add_cut(["".join(r) for r in rows], (L, L - 1), "strict none %d rows" % n, strict=True)
    S.add_cut(strict_rows(rng, 1, 130, 0, 129), (0, 129), "strict untouched 1 row", strict=True)
    S.add_cut(strict_rows(rng, 3, 130, 0, 129), (0, 129), "strict untouched", strict=True)
    for L in (200, 257):
        S.add_cut(strict_rows(rng, 5, L, 70, L - 71, block_window=True), (70, L - 71), "early exit L%d" % L, strict=True)
    S.add([], ("keep",), "empty")
    return S


# ---------------------------------------------------------------- combined
@functools.lru_cache(maxsize=None)
def combined_edges():
    """LiteAlign and Align with the default max-tail 3, ratio 1: gap_pass
    moves and cuts in one go and takes the moved rows' first and last letter
    from the move (post[r].lead = gl, post[r].trail = gr) without scanning
    them again.  Equal rows of 300 to 700 random columns (Align's Filter keeps
    them):

    * a tail of 1 to 3 letters moves over g = 3, 63, 64, 65, 130 gaps on the
      left, on the right or on both ends, and the moved row alone then sets
      CutGaps' from / to;
    * more than one lap: the first cut leaves a row of a 2-letter tail before
      a gap run, which moves in the second lap and sets the third's cut;
    * blocks nothing touches.

    The closed form is lite_align(); meta: the laps that change the block."""
    S = GapCases(101)
    rng = S.rng

    def rows_of(n, L):
        return [r.tobytes().decode() for r in cc.fam(rng, n, L)]

    def gapped(row, a, b):
        return row[:a] + "-" * (b - a) + row[b:]

    k = 0
    for g in COMBINED_G:
        for t in (1, 2, 3):
            for side in ("left", "right", "both"):
                n, L = 2 + k % 4, 300 + 2 * (t + g) + 37 * (k % 5)
                k += 1
                rows = rows_of(n, L)
                r = k % n
                if side in ("left", "both"):
                    rows[r] = gapped(rows[r], t, t + g)
                if side in ("right", "both"):
                    rows[r] = gapped(rows[r], L - t - g, L - t)
                S.add(rows, None, "combined %s t%d g%d" % (side, t, g), meta=1)
    for n, L, lead, run in ((3, 400, 10, 9), (2, 500, 64, 70), (4, 333, 63, 5)):
        rows = rows_of(n, L)
        rows[0] = gapped(rows[0], 0, lead)                      # lap 1: from = lead
        rows[1] = gapped(rows[1], lead + 2, lead + 2 + run)     # lap 2: 2 letters move over `run` gaps, from = run
        S.add(rows, None, "laps left %d" % lead, meta=2)
        rows = rows_of(n, L)
        rows[1] = gapped(rows[1], L - lead, L)
        rows[0] = gapped(rows[0], L - lead - 2 - run, L - lead - 2)
        S.add(rows, None, "laps right %d" % lead, meta=2)
    for n, L in ((2, 300), (5, 450)):
        rows = rows_of(n, L)
        rows[1] = gapped(rows[1], L // 2, L // 2 + 3)
        S.add(rows, ("keep",), "untouched", meta=0)
    S.add([], ("keep",), "empty")
    for k, b in enumerate(S.blocks):
        if b and S.expect[k] is None:
            out, laps = lite_align(list(b))
            assert laps == S.meta[k], (S.tags[k], laps)
            S.expect[k] = ("literal", [out])
    return S


# ---------------------------------------------------------------- indexing
@functools.lru_cache(maxsize=None)
def indexing():
    """Blocks of 1 to 5 rows that MoveGaps (max_tail 200), CutGaps and
    CutGapsStrict all change, blocks without fragments among them (gap_pass
    skips those: which[] differs from the block index).  parts(): prefixes of
    4k + 1, 4k + 2, 4k + 3 and 4k rows in all (k_gap_ends, k_move_gaps and
    k_cut_counts pack four rows into a workgroup: the last one is left with 1,
    2 or 3), and a second, smaller set for the same engine."""
    S = GapCases(103, 200, 10000)
    rng = S.rng
    for k, n in enumerate((1, 2, 3, 1, 4, 2, 5, 3, 1, 2, 4, 3)):
        L = (130, 257, 66, 400)[k % 4]
        t, g = ((1, 3), (2, 64), (3, 5), (65, 70))[k % 4]
        rows = []
        for i in range(n):
            if i % 3 == 0:
                rows.append(end_row(rng, L, left=(t, g), right=(0, 1 + i)))
            elif i % 3 == 1:
                rows.append(end_row(rng, L, left=(0, 2 + k), right=(t, g)))
            else:
                rows.append(end_row(rng, L, left=(t, g), right=(t, g), inner=2))
        S.add(rows, None, "indexing %d rows L%d" % (n, L))
        if k % 3 == 1:
            S.add([], None, "empty")
    return S


def parts(S):
    """Index lists into S.blocks: prefixes whose rows are 1, 2, 3 and 0 mod 4
    (each with an empty block inside), then a short one from the end."""
    out, seen, rows = [], set(), 0
    for k, b in enumerate(S.blocks):
        rows += len(b)
        if k >= 3 and rows % 4 not in seen and b:
            seen.add(rows % 4)
            out.append(list(range(k + 1)))
    assert seen == {0, 1, 2, 3}, seen
    out.append(list(range(len(S.blocks) - 1, len(S.blocks) - 4, -1)))
    return out


# ---------------------------------------------------------------- sweep
SWEEP_L = (2, 9, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256, 257, 319, 449, 512, 513, 640, 900)
SWEEP_ROWS = (2, 3, 4, 5, 9, 64, 65, 70)


def _sweep_end(rng, L):
    """One end of a sweep row: nothing, a lead of gaps or a tail (t, g); the
    seam lengths where they fit."""
    u = rng.random()
    room = L // 2 - 1
    if u < 0.3 or room < 2:
        return (0, 0)
    if u < 0.5:
        fit = [x for x in SEAMS[1:] if x <= room] or [1]
        return (0, int(rng.choice(fit)))
    ts = [x for x in (1, 2, 3, 63, 64, 65, 127, 128, 129, 200, 201) if 2 * x <= room + 1] or [1]
    t = int(rng.choice(ts))
    gs = [x for x in (t, 63, 64, 65, 128, 130) if x >= t and t + x <= room + 1] or [max(1, room - t)]
    g = int(rng.choice(gs))
    if rng.random() < 0.15:
        g = max(1, t // 2)  # fails the ratio
    return (t, g)


@functools.lru_cache(maxsize=None)
def sweep(seed):
    """150 random blocks of 2 to 70 rows and 2 to 900 columns mixing the
    families: rows with leads, trails and tails of seam lengths at either end
    (about one in five blocks has only whole rows beside one such row, so the
    block is cut where that row says), rows that do not overlap (cleared),
    rows of letters outside every other row's (erased), blocks with a gap in
    every column but a few (strict), loose blocks, empty blocks.  The same
    blocks go through MoveGaps (max_tail 200), CutGaps and CutGapsStrict."""
    S = GapCases(2000 + seed, 200, 10000)
    rng = S.rng
    for k in range(150):
        L = int(rng.choice(SWEEP_L))
        n = int(rng.choice([r for r in SWEEP_ROWS if r * L <= 20000]))
        u = rng.random()
        if u < 0.03:
            S.add([], None, "empty")
            continue
        if u < 0.15 and L >= 9:  # strict: few gapless columns
            a = int(rng.integers(0, L - 1))
            b = int(rng.integers(a, L))
            S.add(strict_rows(rng, n, L, a, b), None, "%dx%d strict %d %d" % (n, L, a, b))
            continue
        if u < 0.25 and L >= 9:  # two rows that share no column, one whose letters lie at the ends alone
            c = int(rng.integers(2, L - 2))
            rows = [end_row(rng, L, right=(0, L - c)), end_row(rng, L, left=(0, c + 1))]
            rows += [end_row(rng, L, inner=1) for _ in range(min(n, 5) - 2)]
            S.add(rows, None, "%dx%d disjoint at %d" % (len(rows), L, c))
            continue
        rows = []
        for _ in range(n):
            a, b = _sweep_end(rng, L), _sweep_end(rng, L)
            if sum(a) + sum(b) >= L:
                b = (0, 0)
            rows.append(end_row(rng, L, a, b, inner=int(rng.integers(0, 4))))
        if u < 0.45:  # one row decides
            rows = [rows[0]] + [end_row(rng, L, inner=int(rng.integers(0, 3))) for _ in range(n - 1)]
        if u > 0.85 and L >= 9:  # letters at the two ends alone
            rows[-1] = letters(rng, 1) + "-" * (L - 2) + letters(rng, 1)
        if 0.6 < u < 0.7:
            S.add_loose(rows[:-1] + ["-" * L], [int(x) for x in rng.integers(0, 4, n - 1)] + [3], None,
                        "%dx%d loose" % (n, L))
        else:
            S.add(rows, None, "%dx%d" % (n, L))
    return S


def moved_ends(before, after):
    """(left tails, right tails) that moved between two lists of blocks."""
    left = right = 0
    for b0, b1 in zip(before, after):
        for f0, f1 in zip(b0, b1):
            h = len(f0[4]) // 2
            left += f0[4][:h] != f1[4][:h]
            right += f0[4][len(f0[4]) - h:] != f1[4][len(f1[4]) - h:]
    return left, right
