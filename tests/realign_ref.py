"""Sequential restatement of ReAlign::process_block_impl and of the block
statistics it decides on.

TEST INFRASTRUCTURE ONLY (the product never imports it): the check that the
engine's batch form of ReAlign computes what the reference's per-block loop
computes (ReAlign.cpp:43-63).  Blocks are lists of (seq_index, min_pos,
max_pos, ori, row_or_None), the form BlockSetEngine.blocks() and
BlockSetOracle.blocks() share; `seqs` are the sequence texts, `names` their
names.

* stat / identity_x1e4: make_stat with the six-argument test_column
  (block_stat.cpp:111-154, :188-210) and block_identity (:212-225) in Decimal's
  truncating 4-digit arithmetic (Decimal.hpp:86-125).
* the new rows: oracle.align(texts, "align_block") = align_seqs +
  refine_alignment (AbstractAligner.cpp:51-69).
* is_good_block (Filter.cpp:143-174): the one block in a BlockSetOracle with
  find-subblocks off, "Filter" applied -- it survives iff it is good.

A replaced block keeps its fragments, their order and its place in the list
(DESIGN.md "Determinism conventions"; the reference's set has no order).
"""
from oracle import oracle as orc

_COMPL = str.maketrans("ATGC", "TACG")
LETTERS = "ATGCN"
COUNT_NAMES = ("candidates", "replaced", "filter_refused", "not_better")


def _text(seqs, q, mn, mx, ori):
    """Fragment::str(0): the text read in ori."""
    s = seqs[q][mn:mx + 1]
    return s if ori == 1 else s.translate(_COMPL)[::-1]


def stat(rows):
    """AlignmentStat of gapped rows of one length: the five column classes,
    total and the letter counts A T G C N (char_to_size.hpp:24-36: every
    letter that is not A T G C counts as N)."""
    st = dict(ident_nogap=0, ident_gap=0, noident_nogap=0, noident_gap=0, pure_gap=0,
              total=len(rows[0]) if rows else 0, letters=[0] * 5)
    for col in zip(*rows):
        seen, ident, gap = None, True, False
        for c in col:
            if c == "-":
                gap = True
                continue
            if seen is None:
                seen = c
            elif c != seen:
                ident = False
            st["letters"][LETTERS.index(c) if c in "ATGC" else 4] += 1
        if seen is None:
            st["pure_gap"] += 1
        else:
            st[("ident_" if ident else "noident_") + ("gap" if gap else "nogap")] += 1
    return st


def identity_x1e4(st):
    """block_identity (block_stat.cpp:218-225) x 1e4: accepted = Decimal(in) +
    Decimal(ig) / 2 holds 10000 in + 5000 ig exactly (ig * 1e4 * 1e4 / 2e4), and
    accepted / total is impl * 1e4 / (total * 1e4), truncated."""
    total = st["ident_nogap"] + st["ident_gap"] + st["noident_nogap"] + st["noident_gap"]
    return (10000 * st["ident_nogap"] + 5000 * st["ident_gap"]) // total if total > 0 else 0


def block_stat(block):
    """stat plus alignment_rows, min_fragment_length and identity_x1e4 of an
    aligned block, as npgx_blockset_block_stats reports them."""
    st = stat([f[4] for f in block])
    st["alignment_rows"] = len(block)
    st["min_fragment_length"] = min(mx - mn + 1 for (_, mn, mx, _, _) in block)
    st["identity_x1e4"] = identity_x1e4(st)
    return st


def align_block(block, seqs):
    """remove_alignment + MetaAligner::align_block: the fragments' texts
    aligned and refined; one fragment: its text."""
    texts = [_text(seqs, q, mn, mx, o) for (q, mn, mx, o, _) in block]
    rows = texts if len(block) == 1 else orc.align(texts, "align_block")
    return [(q, mn, mx, o, r) for (q, mn, mx, o, _), r in zip(block, rows)]


def is_good_block(block, seqs, names):
    o = orc.BlockSetOracle(seqs, names, filter_find_subblocks=0)
    o.set_blocks([block])
    o.apply("Filter")
    return len(o.blocks()) == 1


def realign(blocks, seqs, names, force=False, outcomes=None):
    """ReAlign on every block; returns (blocks, counts) with counts keyed by
    COUNT_NAMES.  outcomes (a list) receives one word per block: 'empty',
    'aligned' (no complete alignment before: align_block), 'forced',
    'replaced', 'refused', 'lower', 'equal' (same identity, other rows) or
    'same' (same rows)."""
    out, counts = [], dict.fromkeys(COUNT_NAMES, 0)
    note = outcomes.append if outcomes is not None else (lambda w: None)
    for b in blocks:
        if not b:
            out.append(b)
            note("empty")
            continue
        has_alignment = all(f[4] is not None for f in b)
        if len(b) == 1:
            # alignment_needed's identity row (AbstractAligner.cpp:148-161); a
            # copy of it never has a greater identity
            out.append(b if has_alignment and len(b[0][4]) == b[0][2] - b[0][1] + 1 else align_block(b, seqs))
            note("aligned")
            continue
        if force:
            counts["candidates"] += 1
            counts["replaced"] += 1
            out.append(align_block(b, seqs))
            note("forced")
            continue
        if not has_alignment:
            out.append(align_block(b, seqs))
            note("aligned")
            continue
        counts["candidates"] += 1
        new = align_block(b, seqs)
        i_new = identity_x1e4(stat([f[4] for f in new]))
        i_old = identity_x1e4(stat([f[4] for f in b]))
        if i_new > i_old:
            if is_good_block(new, seqs, names) or not is_good_block(b, seqs, names):
                counts["replaced"] += 1
                out.append(new)
                note("replaced")
            else:
                counts["filter_refused"] += 1
                out.append(b)
                note("refused")
        else:
            counts["not_better"] += 1
            out.append(b)
            note("same" if new == b else ("lower" if i_new < i_old else "equal"))
    return out, counts
