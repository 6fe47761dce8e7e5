"""The bookkeeping of the processors that send fragment texts to the aligner
(MetaAligner, ReAlign, Joiner): one aligner job per block or link that has
something to align, aligned_residues = the texts that went in, and the kernels
of the batch in kernel_times().  Hand-made blocks on three short sequences;
every expected value comes from the input blocks."""
import numpy as np
import pytest

import joiner_ref as jr
from helpers import rows_digest

pytestmark = pytest.mark.gpu

NAMES = ["a", "b", "c"]


def _seqs():
    """Three related sequences of 300 bases (a root with a few substitutions)."""
    rng = np.random.default_rng(13)
    root = rng.integers(0, 4, 300)
    out = []
    for _ in NAMES:
        s = root.copy()
        hit = rng.random(300) < 0.05
        s[hit] = (s[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        out.append("".join("ATGC"[x] for x in s))
    return out


SEQS = _seqs()


def _engine(blocks):
    from npge_amd import _capi
    from npge_amd.blockset import BlockSetEngine
    eng = BlockSetEngine(_capi.SeqSet(SEQS, NAMES))
    eng.set_blocks(blocks)
    return eng


def _with_rows(frags):
    """A gapless aligned block: every fragment's row is its text."""
    return [(q, mn, mx, o, jr._text(SEQS, q, mn, mx, o)) for (q, mn, mx, o) in frags]


def _residues(blocks):
    return sum(mx - mn + 1 for b in blocks for (_, mn, mx, _, _) in b)


def test_meta_aligner_bookkeeping(monkeypatch):
    monkeypatch.setenv("NPGX_TIMERS", "2")
    unaligned = [(0, 10, 99, 1, None), (1, 12, 110, 1, None), (2, 5, 80, -1, None)]
    assert len({mx - mn for (_, mn, mx, _, _) in unaligned}) == 3
    one = [(0, 150, 199, 1, None)]
    aligned = _with_rows([(0, 200, 229, 1), (1, 200, 229, -1)])
    eng = _engine([unaligned, one, [], aligned]).apply("MetaAligner")
    st = eng.stats()
    assert st["align_jobs"] == 1
    assert st["aligned_residues"] == _residues([unaligned]) == 90 + 99 + 76
    assert st["ms_align"] > 0
    assert {"decode_rows", "align_jobs", "refine_alignment"} <= {k["name"] for k in eng.kernel_times()}
    got = eng.blocks()
    assert [f[:4] for f in got[0]] == [f[:4] for f in unaligned]
    assert [f[4].replace("-", "") for f in got[0]] == [jr._text(SEQS, *f[:4]) for f in unaligned]
    assert len({len(f[4]) for f in got[0]}) == 1
    assert got[1:] == [_with_rows([one[0][:4]]), [], aligned]
    assert eng.rows_digest() == rows_digest(got)


def test_meta_aligner_nothing_to_align():
    blocks = [[(0, 150, 199, 1, None)], _with_rows([(0, 200, 229, 1), (1, 200, 229, -1)]),
              _with_rows([(2, 40, 59, -1)]), [(1, 0, 49, -1, None)]]
    eng = _engine(blocks).apply("MetaAligner")
    st = eng.stats()
    assert st["align_jobs"] == 0 and st["aligned_residues"] == 0
    assert eng.blocks() == [_with_rows([f[:4] for f in b]) for b in blocks]


def test_realign_bookkeeping():
    blocks = [_with_rows([(0, 0, 59, 1), (1, 0, 59, 1), (2, 0, 59, 1)]),
              [(0, 100, 149, 1, None), (1, 100, 160, 1, None)],
              _with_rows([(1, 200, 249, -1), (2, 200, 249, -1)])]
    eng = _engine(blocks).apply("ReAlign")
    st = eng.stats()
    assert st["align_jobs"] == 3  # the unaligned block in meta_align, the two candidates
    assert st["aligned_residues"] == _residues(blocks) == 3 * 60 + 50 + 61 + 2 * 50
    assert eng.realign_counts()["candidates"] == 2
    assert st["ms_align"] > 0


def joiner_case():
    """Link one: both between-texts empty (no job).  Link two: one empty and one
    of seven bases (an empty row inside the one job)."""
    return [_with_rows([(0, 0, 19, 1), (1, 0, 19, 1)]), _with_rows([(0, 20, 39, 1), (1, 20, 39, 1)]),
            _with_rows([(1, 100, 119, 1), (2, 50, 69, 1)]), _with_rows([(1, 120, 139, 1), (2, 77, 96, 1)])]


def test_joiner_bookkeeping():
    blocks = joiner_case()
    st_ref = {}
    exp = jr.joiner(blocks, SEQS, st_ref)
    assert st_ref["joins"] == 2 and len(exp) == 2
    eng = _engine(blocks).apply("Joiner")
    st = eng.stats()
    assert st["align_jobs"] == 1
    assert st["aligned_residues"] == 77 - 70
    assert st["ms_align"] > 0
    got = eng.blocks()
    assert got == exp
    assert eng.rows_digest() == rows_digest(exp)
