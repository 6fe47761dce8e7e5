"""Sequential restatement of TrySmth, SmthUnion and AddingLoopBySize with block
names.

TEST INFRASTRUCTURE ONLY (the product never imports it).  Blocks are lists of
(seq_index, min_pos, max_pos, ori, row_or_None), the form
BlockSetEngine.blocks() and BlockSetOracle.blocks() share; a named block is an
item (name, block, tag) -- tag says where the block comes from ("copy", "new",
"piece": cut by SmthUnion).  `seqs` are the sequence texts, `names` their
names.

* smth_union / adding_loop: SmthUnion::run_impl and AddingLoopBySize
  (TrySmth.cpp:44-178) with BlockLengthLess's name term (:35-42): the oracle's
  AddingLoopBySize has no names, so it cannot decide the tie between a named
  original and its unnamed equal.  Ties past the name are pinned as DESIGN.md
  "Determinism conventions" says: the smallest fragment, the sorted fragment
  lists, the place in the list.
* align_named: the Align pipe (Align.cpp:36-52) out of the oracle's single
  processors, so that names can follow the blocks: MetaAligner,
  SelfOverlapsResolver, MoveGaps and CutGaps work in place and keep the name;
  Filter keeps a good block as it is and replaces another by its slices, new
  blocks with the null name (Block.cpp:29-34).
* unique_names: UniqueNames.cpp:23-67 with the repo's conventions (repeated
  names numbered in block_greater order, ties in list order).
* the inner step: the oracle's FragmentsExtender, joiner_ref, realign_ref,
  the oracle's AnchorLoopFast.
"""
import bisect
import functools

import joiner_ref as jr
import realign_ref as rr
from oracle import oracle as orc

NULL = "00000000"  # Block::Block (Block.cpp:29-34)


def _begin(f):
    return f[1] if f[3] == 1 else f[2]


def _fkey(f):
    """Fragment::operator< (Fragment.cpp:214-222): min, max, ori, sequence."""
    return (f[1], f[2], f[3], f[0])


def aln_len(b):
    """Block::alignment_length for the blocks met here: the rows' length, or
    the first fragment's without rows."""
    if not b:
        return 0
    return len(b[0][4]) if b[0][4] is not None else b[0][2] - b[0][1] + 1


def genome_of(name):
    p = name.split("&")
    return p[0] if len(p) == 3 and p[2] in ("c", "l") else ""


# ---------------------------------------------------------------- UniqueNames
def unique_names(items, names):
    """UniqueNames on the blocks (the sequences' names are unique already)."""
    gen = [genome_of(n) for n in names]
    genomes = len(set(gen))
    out = []
    for (name, b, tag) in items:
        if name in (NULL, ""):
            g = [gen[f[0]] for f in b]
            t = "u" if len(b) == 1 else "r" if len(set(g)) < len(g) else "s" if len(b) == genomes else "h"
            name = "%s%dx%d" % (t, len(b), aln_len(b))
        out.append([name, b, tag])
    # block_greater (block_hash.cpp:190-215 turned round), ties in list order
    key = [(len(b), aln_len(b), min(_fkey(f) for f in b)) if b else (0,) for (_, b, _) in out]
    order = sorted(range(len(out)), key=lambda i: key[i], reverse=True)
    seen, last = set(), {}
    for i in order:
        n = out[i][0]
        if n in seen:
            k = last.get(n, 0)
            while True:
                k += 1
                if "%sn%d" % (n, k) not in seen:
                    break
            last[n] = k
            out[i][0] = "%sn%d" % (n, k)
        seen.add(out[i][0])
    return [tuple(x) for x in out]


# ---------------------------------------------------------------- Align with names
class Pipe:
    """The oracle's processors over one sequence set."""

    def __init__(self, seqs, names, **params):
        self.seqs, self.names = seqs, names
        self.o = orc.BlockSetOracle(seqs, names, **params)

    def op(self, blocks, name):
        self.o.set_blocks(blocks)
        self.o.apply(name)
        return self.o.blocks()

    def hash(self, blocks):
        self.o.set_blocks(blocks)
        return self.o.hash()

    def in_place(self, items, name):
        got = self.op([b for (_, b, _) in items], name)
        assert len(got) == len(items), name
        return [(n, g, t) for (n, _, t), g in zip(items, got)]

    def filter(self, items):
        """Filter: a block that comes back as it was keeps its name; any other
        is replaced by its slices (one more call tells how many they are)."""
        got = self.op([b for (_, b, _) in items], "Filter")
        out, j = [], 0
        for (n, b, t) in items:
            if j < len(got) and got[j] == b:
                out.append((n, b, t))
                j += 1
                continue
            mine = self.op([b], "Filter")
            assert got[j:j + len(mine)] == mine
            out += [(NULL, s, t) for s in mine]
            j += len(mine)
        assert j == len(got)
        return out

    def align(self, items):
        """Align (Align.cpp:36-52; Pipe.cpp:60-78 for the loop's end)."""
        for name in ("MetaAligner", "SelfOverlapsResolver", "MetaAligner"):
            items = self.in_place(items, name)
        seen = {self.hash([b for (_, b, _) in items])}
        while True:
            items = self.in_place(items, "MoveGaps")
            items = self.in_place(items, "CutGaps")
            items = self.filter(items)
            h = self.hash([b for (_, b, _) in items])
            if h in seen:
                return items
            seen.add(h)


# ---------------------------------------------------------------- SmthUnion
class FragIndex:
    """SetFc (FragmentCollection.hpp:184-364): per sequence, the fragments in
    Fragment::operator< order."""

    def __init__(self):
        self.m = {}

    def add(self, b):
        for f in b:
            bisect.insort(self.m.setdefault(f[0], []), _fkey(f))

    def has_overlap(self, f):
        """has_overlap (:273-297): the lower bound and its predecessor only."""
        c = self.m.get(f[0], [])
        i = bisect.bisect_left(c, _fkey(f))
        for g in c[max(i - 1, 0):i + 1]:
            if max(g[0], f[1]) <= min(g[1], f[2]):
                return True
        return False

    def block_has_overlap(self, b):
        return any(self.has_overlap(f) for f in b)

    def overlaps(self, f):
        """find_overlaps (:319-364): the common part with every fragment of the
        sequence that shares positions with f."""
        return [(max(g[0], f[1]), min(g[1], f[2])) for g in self.m.get(f[0], [])
                if max(g[0], f[1]) <= min(g[1], f[2])]


def _before(x, y):
    """BlockLengthLess (TrySmth.cpp:35-42): size, alignment length and name,
    all descending; then the pinned ties.  x, y: (name, block, tag, index)."""
    for a, b in ((len(x[1]), len(y[1])), (aln_len(x[1]), aln_len(y[1])), (x[0], y[0])):
        if a != b:
            return -1 if a > b else 1
    kx = (min(map(_fkey, x[1])), sorted(map(_fkey, x[1])), x[3]) if x[1] else ((), [], x[3])
    ky = (min(map(_fkey, y[1])), sorted(map(_fkey, y[1])), y[3]) if y[1] else ((), [], y[3])
    return -1 if kx < ky else 1 if kx > ky else 0


def slice_block(b, first, last, seqs):
    """Block::slice (Block.cpp:238-284) of columns [first, last]."""
    out = []
    for (q, mn, mx, o, row) in b:
        before = sum(1 for c in row[:first] if c != "-")
        part = row[first:last + 1]
        inside = sum(1 for c in part if c != "-")
        if not inside:
            continue
        s0 = _begin((q, mn, mx, o)) + o * before
        s1 = s0 + o * (inside - 1)
        no = 1 if s0 <= s1 else -1
        if no != o:  # set_begin_last: a 1-letter ori -1 fragment becomes ori +1, its letter the forward strand's
            part = "".join(c if c == "-" else seqs[q][min(s0, s1)] for c in part)
        out.append((q, min(s0, s1), max(s0, s1), no, part))
    return out


def smth_union(other, target, s2f, seqs, cuts=None):
    """SmthUnion::run_impl (TrySmth.cpp:44-155): other's items in BlockLengthLess
    order; returns the subblocks (the next round's other).  target (a list) and
    s2f (its FragIndex) grow.  cuts (a list) receives the number of pieces of
    every block cut."""
    order = sorted(((n, b, t, i) for i, (n, b, t) in enumerate(other)), key=functools.cmp_to_key(_before))
    sub, subblocks = FragIndex(), []
    for (n, b, t, _) in order:
        if sub.block_has_overlap(b):
            sub.add(b)
            subblocks.append((n, b, t))
            continue
        if not s2f.block_has_overlap(b):
            s2f.add(b)
            target.append((n, b, t))
            continue
        L = aln_len(b)
        good = [True] * L
        for f in b:  # mark_bad (:96-125)
            cols = [k for k, c in enumerate(f[4]) if c != "-"]
            for (a, z) in s2f.overlaps(f):
                fa, fb = (a - _begin(f)) * f[3], (z - _begin(f)) * f[3]
                ba, bb = cols[fa], cols[fb]
                for k in range(min(ba, bb), max(ba, bb) + 1):
                    good[k] = False
        pieces, first = 0, -1
        for k in range(L + 1):  # add_subblocks (:127-147)
            g = k < L and good[k]
            if g and first == -1:
                first = k
            if not g and first != -1:
                x = slice_block(b, first, k - 1, seqs)
                sub.add(x)
                subblocks.append((NULL, x, "piece"))
                pieces += 1
                first = -1
        if cuts is not None:
            cuts.append(pieces)
    return subblocks


def adding_loop(other, pipe, info=None):
    """AddingLoopBySize (TrySmth.cpp:157-178) into an empty target; returns the
    target's items.  info (a dict) receives rounds and cuts."""
    target, s2f, cuts, rounds = [], FragIndex(), [], 0
    while other:
        other = pipe.align(other)
        other = smth_union(other, target, s2f, pipe.seqs, cuts)
        rounds += 1
    if info is not None:
        info.update(rounds=rounds, cuts=cuts)
    return target


# ---------------------------------------------------------------- TrySmth
def run_inner(inner, blocks, seqs, names):
    """The tried processor: `inner` is its option string as apply takes it."""
    tok = inner.split()
    name, opts = tok[0], dict(t.lstrip("-").replace(":=", "=").split("=") for t in tok[1:])
    if name == "FragmentsExtender":
        portion = int(round(float(opts.get("extend-length-portion", 0)) * 10000))
        return Pipe(seqs, names, portion_x1e4=portion).op(blocks, "FragmentsExtender")
    if name == "OriByMajority":
        return jr.ori_by_majority(blocks, names)
    if name == "Joiner":
        return jr.joiner(blocks, seqs)
    if name == "ReAlign":
        return rr.realign(blocks, seqs, names)[0]
    if name == "AnchorLoopFast":
        o = orc.BlockSetOracle(seqs, names)
        o.set_blocks(blocks)
        orc.anchor_loop_fast(o)
        return o.blocks()
    raise ValueError("no restatement of " + name)


def try_smth(blocks, seqs, names, inner, info=None):
    """TrySmth::TrySmth (TrySmth.cpp:184-199) around `inner`; returns (blocks,
    block names).  info (a dict) receives the AddingLoopBySize rounds and cuts,
    `tags` (where each block of the loop's result came from) and `tried` (the
    blocks after the step, ReAlign and Align)."""
    pipe = Pipe(seqs, names)
    copy = unique_names([(NULL, b, "copy") for b in blocks], names)
    new = run_inner(inner, blocks, seqs, names)
    new = rr.realign(new, seqs, names)[0]  # the names are gone: RemoveNames
    new = pipe.align([("", b, "new") for b in new])
    res = adding_loop(copy + new, pipe, info)
    if info is not None:
        info.update(tags=[(t, b) for (_, b, t) in res], tried=[b for (_, b, _) in new])
    res = unique_names(res, names)
    again = rr.realign([b for (_, b, _) in res], seqs, names)[0]
    res = pipe.align([(n, b, t) for (n, _, t), b in zip(res, again)])
    return [b for (_, b, _) in res], [n for (n, _, _) in res]
