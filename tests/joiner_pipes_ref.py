"""Sequential restatement of LiteFilter, MergeUnique and the JoinerP,
MergeAndJoin and LiteJoinerP pipes, with block names.

TEST INFRASTRUCTURE ONLY (the product never imports it).  Blocks are lists of
(seq_index, min_pos, max_pos, ori, row_or_None), the form
BlockSetEngine.blocks() and BlockSetOracle.blocks() share; every function
takes and returns (blocks, block names).  It sits over joiner_ref (Joiner,
OriByMajority), try_smth_ref's Pipe (the oracle's Rest and MetaAligner) and
try_smth_ref's TrySmth steps.

Where the reference leans on pointer order the order is pinned as DESIGN.md
"Determinism conventions" says:

1. blocks of two or more fragments are taken by size descending, stably in
   the set's order;
2. unique_of's keys (block, ori) are visited in (place of the block in the
   set, -1 before +1) order;
3. a merged block's fragments stand in order of first appearance while
   walking b's fragments;
4. the emptied one-fragment blocks leave the set, the new blocks are appended
   in the order they are made.

Rows: a merged block has rows when all its fragments had rows of one length
(what alignment_needed, AbstractAligner.cpp:162-176, takes for aligned); a
fragment whose ori changed has its gapless row reverse-complemented, and a
gapped one is refused (GappedFlip), as the engine refuses it.
"""
import joiner_ref as jr
import realign_ref as rr
import try_smth_ref as tr

NULL = tr.NULL
MIN_LENGTH = 100
MAX_POS = 1 << 62


class GappedFlip(ValueError):
    """A one-fragment block with a gapped row whose fragment changes its ori."""


def aln_len(b):
    """Block::alignment_length (Block.cpp:133-139)."""
    return max((len(f[4]) if f[4] is not None else f[2] - f[1] + 1 for f in b), default=0)


# ---------------------------------------------------------------- the hand-made case
def hand_case(fourth=True, ulen=40, seed=5):
    """Three sequences X(300) + u_i(ulen, unrelated) + Y(300), the third one
    reverse-complemented; blocks X and Y with rows.  fourth: one more sequence
    X + u_4 that ends after its unique fragment (no second neighbour), its X
    in block X.  Returns (seqs, names, blocks)."""
    import numpy as np
    rng = np.random.default_rng(seed)

    def text(n):
        return "".join("ATGC"[i] for i in rng.integers(0, 4, n))

    X, Y = text(300), text(300)
    us = [text(ulen) for _ in range(4)]
    seqs = [X + us[0] + Y, X + us[1] + Y, jr.revcomp(X + us[2] + Y)]
    end = 600 + ulen - 1
    bx = [(0, 0, 299, 1, X), (1, 0, 299, 1, X), (2, 300 + ulen, end, -1, X)]
    by = [(0, 300 + ulen, end, 1, Y), (1, 300 + ulen, end, 1, Y), (2, 0, 299, -1, Y)]
    if fourth:
        seqs.append(X + us[3])
        bx.append((3, 0, 299, 1, X))
    return seqs, ["s%d" % i for i in range(len(seqs))], [bx, by]


# ---------------------------------------------------------------- LiteFilter
def lite_filter(blocks, names, min_fragment=MIN_LENGTH, min_block=2):
    """LiteFilter::process_block_impl (Filter.cpp:53-64)."""
    keep = [i for i, b in enumerate(blocks) if len(b) >= min_block and aln_len(b) >= min_fragment]
    return [blocks[i] for i in keep], [names[i] for i in keep]


# ---------------------------------------------------------------- MergeUnique
def merge_unique(blocks, names, both=True, merge_long=False, counts=None):
    """MergeUnique::run_impl (MergeUnique.cpp:142-169)."""
    min_length = MAX_POS if merge_long else MIN_LENGTH
    nb = len(blocks)
    frs = [(k, i) for k, b in enumerate(blocks) for i in range(len(b))]     # fragment ids in (block, fragment) order
    gid = {ki: g for g, ki in enumerate(frs)}
    owner = [k for (k, _) in frs]
    ori = [blocks[k][i][3] for (k, i) in frs]
    size = [len(b) for b in blocks]                                        # live; the new blocks follow
    order = {}
    for g, (k, i) in enumerate(frs):
        f = blocks[k][i]
        order.setdefault(f[0], []).append((f[1], f[2], g))
    at = {}
    for lst in order.values():                                              # VectorFc: built once, not updated
        lst.sort()
        for p, (_, _, g) in enumerate(lst):
            at[g] = p

    def nbr(g, d):
        lst = order[blocks[frs[g][0]][frs[g][1]][0]]
        p = at[g] + d
        return lst[p][2] if 0 <= p < len(lst) else None

    def joinable(n):                                                        # isJoinableFragment (:61-77)
        return n is not None and size[owner[n]] == 1 and aln_len(blocks[owner[n]]) < min_length

    news = []

    def merge(ff, b):                                                       # merge_fragments (:36-59)
        for n in ff:
            size[owner[n]] = 0
            owner[n] = nb + len(news)
            p = nbr(n, -1)
            f = p if p is not None and owner[p] == b else nbr(n, 1)
            assert f is not None and owner[f] == b
            ori[n] = ori[f]
        size.append(len(ff))
        news.append(ff)

    def add_group(ff0, b):                                                  # :105-115
        ff = []
        for n in ff0:
            if joinable(n) and n not in ff:
                ff.append(n)
        if len(ff) >= 2:
            merge(ff, b)

    todo = sorted((k for k in range(nb) if len(blocks[k]) >= 2), key=lambda k: -len(blocks[k]))
    for b in todo:
        mine = [gid[(b, i)] for i in range(len(blocks[b]))]
        for d in (-1, 1):
            if both:                                                        # inspect_neighbours2 (:80-117)
                unique_of = {}
                for f in mine:
                    n = nbr(f, ori[f] * d)
                    if not joinable(n):
                        continue
                    in2 = nbr(n, -1) if nbr(n, 1) == f else nbr(n, 1) if nbr(n, -1) == f else None
                    if in2 is None or in2 == f:
                        continue
                    if size[owner[in2]] >= 2:
                        unique_of.setdefault((owner[in2], ori[f] * ori[in2]), []).append(n)
                for key in sorted(unique_of):
                    add_group(unique_of[key], b)
            else:                                                           # inspect_neighbours1 (:120-134)
                add_group([n for n in (nbr(f, ori[f] * d) for f in mine) if joinable(n)], b)
    out, out_names = [], []
    for k, b in enumerate(blocks):
        if not (len(b) == 1 and size[k] == 0):
            out.append(b)
            out_names.append(names[k])
    for ff in news:
        old = [blocks[frs[n][0]][frs[n][1]] for n in ff]
        keep = all(f[4] is not None for f in old) and len({len(f[4]) for f in old}) == 1
        new = []
        for n, f in zip(ff, old):
            row = f[4] if keep else None
            if keep and ori[n] != f[3]:
                if len(row) != f[2] - f[1] + 1:
                    raise GappedFlip("fragment %r" % (f[:3],))
                row = jr.revcomp(row)
            new.append((f[0], f[1], f[2], ori[n], row))
        out.append(new)
        out_names.append("m%dx%d" % (len(new), max(aln_len([f]) for f in old)))
    if counts is not None:
        counts.update(blocks_inspected=len(todo), merges=len(news), fragments_merged=sum(map(len, news)))
    return out, out_names


# ---------------------------------------------------------------- the pipes' other steps
def ori_by_majority(blocks, names, seq_names):
    return jr.ori_by_majority(blocks, seq_names), names


def rest(blocks, names, pipe):
    got = pipe.op(blocks, "Rest")
    assert got[:len(blocks)] == blocks
    return got, names + [NULL] * (len(got) - len(blocks))


def meta_aligner(blocks, names, pipe):
    got = pipe.op(blocks, "MetaAligner")
    assert len(got) == len(blocks)
    return got, names


def joiner(blocks, names, seqs):
    """A block that was not joined keeps its name (it may have been inverted),
    a joined one is a new block."""
    by_coords = {tuple(sorted(f[:3] for f in b)): n for b, n in zip(blocks, names) if b}
    got = jr.joiner(blocks, seqs)
    return got, [by_coords.get(tuple(sorted(f[:3] for f in b)), NULL) if b else NULL for b in got]


def run(name, blocks, seqs, seq_names, names=None, counts=None, **opts):
    """One of the five processors by name; returns (blocks, block names)."""
    names = [NULL] * len(blocks) if names is None else names
    pipe = tr.Pipe(seqs, seq_names)
    if name == "LiteFilter":
        return lite_filter(blocks, names, **opts)
    if name == "MergeUnique":
        return merge_unique(blocks, names, counts=counts, **opts)
    assert not opts
    x = (blocks, names)
    if name in ("JoinerP", "LiteJoinerP"):
        x = lite_filter(*x)
        x = ori_by_majority(*x, seq_names)
    if name in ("JoinerP", "MergeAndJoin"):
        x = rest(*x, pipe)
        x = merge_unique(*x, counts=counts)
        x = meta_aligner(*x, pipe)
    elif name != "LiteJoinerP":
        raise ValueError("no restatement of " + name)
    x = joiner(*x, seqs)
    if name == "JoinerP":
        x = rest(*x, pipe)
    return x


def try_smth(blocks, seqs, seq_names, inner, info=None):
    """TrySmth::TrySmth (TrySmth.cpp:184-199) around one of the processors
    here, by try_smth_ref's steps; returns (blocks, block names)."""
    pipe = tr.Pipe(seqs, seq_names)
    copy = tr.unique_names([(NULL, b, "copy") for b in blocks], seq_names)
    new = run(inner, blocks, seqs, seq_names)[0]
    new = rr.realign(new, seqs, seq_names)[0]  # the names are gone: RemoveNames
    new = pipe.align([("", b, "new") for b in new])
    res = tr.adding_loop(copy + new, pipe, info)
    res = tr.unique_names(res, seq_names)
    again = rr.realign([b for (_, b, _) in res], seqs, seq_names)[0]
    res = pipe.align([(n, b, t) for (n, _, t), b in zip(res, again)])
    return [b for (_, b, _) in res], [n for (n, _, _) in res]
