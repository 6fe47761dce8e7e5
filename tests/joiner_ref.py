"""Sequential restatement of Joiner::run_impl and OriByMajority.

TEST INFRASTRUCTURE ONLY (the product never imports it): the check that the
engine's batch form of Joiner computes what the reference's sequential loop
computes.  Blocks are lists of (seq_index, min_pos, max_pos, ori, row_or_None),
the form BlockSetEngine.blocks() and BlockSetOracle.blocks() share; `seqs` are
the sequence texts (ATGCN), `names` their names.

Where the reference is not reproducible (Joiner.cpp:238-239 sorts the
std::set<Block*> pointer order with an unstable std::sort) the order is pinned
as DESIGN.md "Determinism conventions" says: blocks by size descending in the
stable order of the input list; a joined block stands where the `one` of its
join stood, so a chain ends up at its head's place.
"""
import bisect

from oracle import oracle as orc

_COMPL = str.maketrans("ATGC", "TACG")


class JoinOverlap(ValueError):
    """The facing fragments of a pair that would be joined overlap: the
    reference concatenates rows that no longer match the joined fragment
    (Joiner.cpp:98-109 leaves the middle empty); the engine refuses."""


def revcomp(s):
    """complement.hpp:19-32 on a gapped row: reversed, A<->T G<->C, '-' and N kept."""
    return s.translate(_COMPL)[::-1]


def inverse(block):
    """Block::inverse (Block.cpp:232-236): every ori flips, every row becomes
    its gapped reverse complement (Fragment::inverse, AlignmentRow::inverse)."""
    return [(q, mn, mx, -o, None if r is None else revcomp(r)) for (q, mn, mx, o, r) in block]


def _text(seqs, q, mn, mx, ori):
    """Fragment::str(0) (Fragment.cpp:163-171): the text read in ori."""
    s = seqs[q][mn:mx + 1]
    return s if ori == 1 else revcomp(s)


def consensus_string(block, seqs):
    """Block::consensus_string (Block.cpp:147-191): unaligned -> the first
    longest fragment's text; aligned -> per column the first of A T G C N with
    the highest count ('A' when the column holds no letter)."""
    if not block:
        return ""
    if block[0][4] is None:
        longest = block[0]
        for f in block:  # Block.cpp:170-177
            if f[2] - f[1] > longest[2] - longest[1]:
                longest = f
        return _text(seqs, longest[0], longest[1], longest[2], longest[3])
    out = []
    for col in zip(*(f[4] for f in block)):
        freq = [sum(1 for c in col if c == x) for x in "ATGCN"]  # test_column, block_stat.cpp:188-210
        out.append("ATGCN"[freq.index(max(freq))])  # Block.cpp:154-164
    return "".join(out)


def ori_by_majority(blocks, names):
    """OriByMajority::process_block_impl (OriByMajority.cpp:35-61) on every block."""
    out = []
    for b in blocks:
        total = sum(mx - mn + 1 for (_, mn, mx, _, _) in b)            # :39-44
        ori_1 = sum(mx - mn + 1 for (_, mn, mx, o, _) in b if o == 1)
        result = False
        if total == 0:                                                  # :45-46
            result = False
        elif ori_1 * 2 < total:                                         # :47-48
            result = True
        elif ori_1 * 2 == total:                                        # :49-56, FragmentCompare3 :25-33
            f = min(b, key=lambda f: (f[1], f[2], names[f[0]]))         # min_element: the first smallest
            result = f[3] == -1
        out.append(inverse(b) if result else list(b))                   # :58-60
    return out


class _S2F:
    """SetFc (FragmentCollection.hpp:184-479) with cycles not allowed
    (Joiner.cpp:235): per sequence the fragments in Fragment::operator< order
    (Fragment.cpp:214-222: min_pos, max_pos, ...).  Keys are (min_pos, max_pos,
    block id, fragment index): two fragments with equal coordinates keep that
    order here (the reference's std::set drops the second)."""

    def __init__(self):
        self.d = {}

    def add(self, seq, key):
        bisect.insort(self.d.setdefault(seq, []), key)

    def remove(self, seq, key):
        lst = self.d[seq]
        lst.pop(bisect.bisect_left(lst, key))

    def neighbor(self, seq, key, ori):
        """next (ori 1) / prev (ori -1), None at the ends (:402-458)."""
        lst = self.d[seq]
        j = bisect.bisect_left(lst, key) + ori
        return lst[j] if 0 <= j < len(lst) else None


def _match(one, another):
    """Block::match (Block.cpp:193-230)."""
    if len(one) != len(another):
        return 0
    c1, c2 = {}, {}
    for f in one:
        c1.setdefault(f[0], {1: 0, -1: 0})[f[3]] += 1
    for f in another:
        c2.setdefault(f[0], {1: 0, -1: 0})[f[3]] += 1
    all_match = all_inv = True
    for seq, n in c1.items():
        if seq not in c2:
            return 0
        for ori in (-1, 1):
            if n[ori] != c2[seq][ori]:
                all_match = False
            if n[ori] != c2[seq][-ori]:
                all_inv = False
        if not all_match and not all_inv:
            return 0
    return 1 if all_match else -1


def joiner(blocks, seqs, stats=None):
    """Joiner::run_impl (Joiner.cpp:234-262).  Returns the blocks after it.
    stats (a dict, optional) receives: joins, max_chain (blocks in the longest
    chain), empty_rows (middles with an empty row next to a non-empty one),
    inverted (blocks try_join left inverted without joining them),
    flipped_joins (joins whose partner was inverted first: match -1)."""
    bs = {}      # block id -> list of [seq, min, max, ori, row]
    pos = {}     # block id -> place in the output
    chain = {}   # block id -> input blocks joined into it
    s2f = _S2F()
    st = dict(joins=0, max_chain=1, empty_rows=0, inverted=0, flipped_joins=0)

    def add_block(k):
        for i, f in enumerate(bs[k]):
            s2f.add(f[0], (f[1], f[2], k, i))

    def remove_block(k):
        for i, f in enumerate(bs[k]):
            s2f.remove(f[0], (f[1], f[2], k, i))

    for k, b in enumerate(blocks):            # :236-237
        bs[k] = [list(f) for f in b]
        pos[k] = k
        chain[k] = 1
        add_block(k)
    next_id = len(blocks)

    def neighbor(k, i, ori):
        f = bs[k][i]
        return s2f.neighbor(f[0], (f[1], f[2], k, i), ori)

    def can_join(one, another):
        """can_join (:51-81): the logical side and, per fragment of one, its
        neighbour's index in another."""
        a, c = bs[one], bs[another]
        if len(a) != len(c) or len(a) < 2:    # :55-63
            return 0, None
        for lo in (1, -1):                    # :65-77
            partner = []
            for i, f in enumerate(a):
                n = neighbor(one, i, f[3] * lo)        # logical_neighbor (FragmentCollection.hpp:461-463)
                if n is None or n[2] != another or c[n[3]][3] != f[3]:   # :68-69, :45-49
                    break
                partner.append(n[3])
            else:
                return lo, partner
        return 0, None

    def try_join(one, another):
        nonlocal next_id
        m = _match(bs[one], bs[another])      # :221
        if m == -1:                           # :222-224
            bs[another] = [list(f) for f in inverse(bs[another])]
            st["inverted"] += 1
        if not m:
            return None
        lo, partner = can_join(one, another)  # :226
        if not lo:
            return None
        if m == -1:
            st["inverted"] -= 1
            st["flipped_joins"] += 1
        a, c = bs[one], bs[another]
        aln = a[0][4] is not None and c[0][4] is not None   # :140
        new, middle = [], []
        for i, f in enumerate(a):
            f1 = c[partner[i]]
            lower, upper = (f, f1) if f[3] * lo == 1 else (f1, f)   # :98-104, :170-173
            if upper[1] <= lower[2]:
                raise JoinOverlap("fragments %r and %r overlap" % (tuple(lower[:3]), tuple(upper[:3])))
            new.append([f[0], min(f[1], f1[1]), max(f[2], f1[2]), f[3], None])   # join, :174-180
            if aln:   # :105-109
                middle.append(_text(seqs, f[0], lower[2] + 1, upper[1] - 1, f[3])
                              if upper[1] - 1 >= lower[2] + 1 else "")
        if aln:
            if any(middle):                   # AbstractAligner::align_seqs (AbstractAligner.cpp:104-143)
                if not all(middle):
                    st["empty_rows"] += 1
                middle = orc.align(middle, mode="align_seqs")
            for i, f in enumerate(a):         # :113-122
                f1 = c[partner[i]]
                new[i][4] = f[4] + middle[i] + f1[4] if lo == 1 else f1[4] + middle[i] + f[4]
        remove_block(one)                     # :248-253
        remove_block(another)
        k = next_id
        next_id += 1
        bs[k] = new
        pos[k] = pos[one]
        chain[k] = chain[one] + chain[another]
        del bs[one], bs[another]
        add_block(k)
        st["joins"] += 1
        st["max_chain"] = max(st["max_chain"], chain[k])
        return k

    order = sorted(range(len(blocks)), key=lambda k: -len(blocks[k]))   # :238-239 (stable)
    for k in order:
        if k not in bs:                       # :241
            continue
        block = k
        for ori in (-1, 1):                   # :242
            while bs[block]:
                n = neighbor(block, 0, ori)   # neighbor_block (:33-43): the front fragment's physical neighbour
                if n is None:
                    break
                new_block = try_join(block, n[2])
                if new_block is None:
                    break
                block = new_block
    if stats is not None:
        stats.update(st)
    return [[tuple(f) for f in bs[k]] for k in sorted(bs, key=lambda k: pos[k])]
