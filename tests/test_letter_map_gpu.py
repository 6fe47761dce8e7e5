"""k_letter_map (BlockSetEngine.letter_map()) against numpy: one bit a cell, the
letters before each word.  Shapes around the word (64 columns) and the tile
(4096 columns), more rows than a wave has lanes, a row of three tiles; odd
lengths put every row of a block at another alignment."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 63), (2, 64), (3, 65), (17, 4095), (17, 4096), (2, 4097), (70, 130), (1, 12289)]
DENSITY = [0.0, 0.1, 0.5, 1.0]


def _rows(rng, n, L, k0):
    rows = []
    for i in range(n):
        d = DENSITY[(k0 + i) % 4]
        if L > 4096 and n <= 2:  # the rows of more than one tile hold letters: their tile bases are not 0
            d = (0.5, 1.0)[i % 2]
        r = np.where(rng.random(L) < d, ord("A"), ord("-")).astype(np.uint8)
        if i % 5 == 4:  # a gap run across a word border, letters around it
            r[:] = ord("C")
            r[60:70] = ord("-")
        for seam in (4096, 8192):  # a gap run across every tile border the row has, letters on both sides
            if L >= seam + 8:
                r[seam - 12:seam - 6] = ord("G")
                r[seam - 6:seam + 4] = ord("-")
                r[seam + 4:seam + 8] = ord("G")
            elif L > seam:  # one column past the border: the run reaches it, or stops at a lone letter there
                r[seam - 12:seam - 6] = ord("G")
                r[seam - 6:L] = ord("-")
                if i % 2:
                    r[L - 1] = ord("G")
        rows.append(r)
    return rows


def _gap_run_across(r, seam):
    return len(r) >= seam + 8 and (r[seam - 6:seam + 4] == ord("-")).all() and r[seam - 7] != ord("-") \
        and r[seam + 4] != ord("-")


def _expected(r):
    bits = np.zeros((len(r) + 63) // 64 * 64, dtype=np.uint8)
    bits[:len(r)] = r != ord("-")
    words = np.packbits(bits, bitorder="little").view("<u8")
    counts = bits.reshape(-1, 64).sum(axis=1).astype(np.int64)
    return words, np.concatenate([[0], np.cumsum(counts)[:-1]])


def test_letter_map_shapes():
    from npge_amd import _capi
    from npge_amd.blockset import BlockSetEngine
    rng = np.random.default_rng(5)
    seq = "ACGT" * 3100  # every fragment lies on it; the rows' letters are the test's own (loose rows)
    blocks, rows = [], []
    for k, (n, L) in enumerate(SHAPES):
        rs = _rows(rng, n, L, k)
        rows += rs
        blocks.append([(0, 0, max(int((r != ord("-")).sum()), 1) - 1, 1, r.tobytes().decode()) for r in rs])
    blocks.insert(3, [(0, 0, 9, 1, None), (0, 20, 29, 1, None)])  # a block without rows has no map
    assert any((r == ord("-")).all() for r in rows) and any((r != ord("-")).all() and len(r) > 64 for r in rows)
    assert any(len(r) > 70 and (r[60:70] == ord("-")).all() and r[59] != ord("-") and r[70] != ord("-") for r in rows)
    # a row of three tiles with letters in each (non-zero tile bases past the second tile), gap runs across both seams
    long = [r for r in rows if len(r) == 12289]
    assert len(long) == 1 and all((long[0][t * 4096:(t + 1) * 4096] != ord("-")).sum() > 1000 for t in range(3))
    assert _gap_run_across(long[0], 4096) and _gap_run_across(long[0], 8192)
    short = [r for r in rows if len(r) == 4097]  # the second tile is one column: a gap in one row, a letter in the other
    assert len(short) == 2 and all((r[4090:4096] == ord("-")).all() and r[4089] != ord("-") for r in short)
    assert sorted(chr(r[4096]) for r in short) == ["-", "G"]
    eng = BlockSetEngine(_capi.SeqSet([seq], ["s"])).set_blocks(blocks)
    got = eng.letter_map()
    assert len(got) == len(rows) == sum(n for n, _ in SHAPES)
    for r, (words, pre) in zip(rows, got):
        ew, ep = _expected(r)
        assert words.dtype == np.uint64 and np.array_equal(words, ew), len(r)
        assert np.array_equal(pre, ep), len(r)
    assert eng.blocks() == blocks  # (the rows are where they were)


def test_letter_map_of_a_set_without_rows():
    from npge_amd import _capi
    from npge_amd.blockset import BlockSetEngine
    eng = BlockSetEngine(_capi.SeqSet(["ACGTACGTAC"], ["s"])).set_blocks([[(0, 0, 4, 1, None)]])
    assert eng.letter_map() == []
