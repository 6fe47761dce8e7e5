"""Inputs shared by the TrySmth / SmthUnion tests (TEST INFRASTRUCTURE ONLY).

Blocks are lists of (seq_index, min_pos, max_pos, ori, row_or_None).
"""
import numpy as np

import try_smth_ref as tr


def overlapping_set(blocks, seqs):
    """Every aligned block of two or more fragments twice, at partly
    overlapping places, in three ways by turn:
    0: its columns [0, 2L/3) and [L/3, L) -- the loser keeps a third;
    1: the block without its first row, and its middle third with every row --
       the middle wins by size and cuts the other into two pieces;
    2: the block and its exact copy."""
    out, k = [], 0
    for b in blocks:
        if len(b) < 2 or b[0][4] is None:
            out.append(b)
            continue
        L = len(b[0][4])
        if k % 3 == 0:
            out += [tr.slice_block(b, 0, 2 * L // 3 - 1, seqs), tr.slice_block(b, L // 3, L - 1, seqs)]
        elif k % 3 == 1:
            out += [b[1:], tr.slice_block(b, L // 3, 2 * L // 3 - 1, seqs)]
        else:
            out += [b, list(b)]
        k += 1
    return out


def wide_case(n=66, length=600, seed=66):
    """(seqs, names, blocks): one block of n rows (more than a wave has lanes)
    without its first row, and its middle third with every row."""
    rng = np.random.default_rng(seed)
    root = rng.integers(0, 4, length)
    seqs = []
    for i in range(n):
        s = root.copy()
        hit = rng.random(length) < 0.0005
        s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        seqs.append("".join("ATGC"[x] for x in s))
    names = ["w%d&chr&c" % i for i in range(n)]
    whole = [(i, 0, length - 1, 1, s) for i, s in enumerate(seqs)]
    return seqs, names, [whole[1:], tr.slice_block(whole, length // 3, 2 * length // 3 - 1, seqs)]
