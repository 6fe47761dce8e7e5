"""k_pack (the 2-bit store and its N bitmap) and k_decode (fragment text from
them) at their seams, engine against oracle and against plain Python slices,
bit for bit.  The inputs are decode_cases.py's; test_decode_cases_ref.py shows
on the CPU that they hold what they claim.

* 32 bases to a packed word: sequences of 31 / 32 / 33, 63 / 64 / 65, 95 / 96 /
  97, 127 / 128 / 129 letters, fragments from position 0, 1, 31, 32, 33, 63
  (mod 64) of 1 to 16385 letters;
* 64 N bits to an N word, its halves written by two lanes through atomicOr: N
  at 31 | 32 and 63 | 64, at the first and the last base, a sequence of N only;
* the even-word padding of pack_device: 2 to 6 words a sequence, neighbours in
  rank order (not input order) of every other length;
* PIECE = 8192 letters a decode op, the next op at pos + ori * 8192: fragments
  of 8191, 8192, 8193 and 16385 letters in both orientations, N at the seams;
* the complement by code ^= 1, N kept;
* to_atgcn on the way in: lower case, IUPAC letters, dropped characters.

Rows of equal lengths come straight from k_decode (dummy_align refines only
blocks of unequal lengths), so "refine-chunk" must not show in them: the same
rows and the same rows_digest() with it on and off.  The ragged blocks are
decoded into padded rows and refined, the long ones in chunks.
"""
import pytest

import decode_cases as dc
from decode_cases import orc
from helpers import rows_digest
from test_block_build_gpu import _engine

pytestmark = pytest.mark.gpu


def _decoded(chunk=None):
    D = dc.cases()
    ss, eng = _engine(list(D.raw), list(D.names))
    if chunk is not None:
        eng.tune("refine-chunk", chunk)
    eng.set_blocks([list(b) for b in D.blocks]).apply("DummyAligner")
    return D, ss, eng


def _named(D, got, want):
    bad = [k for k in range(len(want)) if k >= len(got) or got[k] != want[k]]
    assert not bad and len(got) == len(want), "%d blocks differ, first %s" % (
        len(bad), [(D.tags[k], [(f[0], f[1], f[3]) for f in D.blocks[k]]) for k in bad[:5]])


def test_pack_layout():
    """Sizes after to_atgcn and the rank order (size descending, name
    ascending) the packed store is laid out in."""
    D = dc.cases()
    ss, _ = _engine(list(D.raw), list(D.names))
    assert [ss.size(i) for i in range(ss.n)] == [len(c) for c in D.clean]
    order = sorted(range(ss.n), key=lambda i: (-len(D.clean[i]), D.names[i], i))
    assert [ss.rank(i) for i in order] == list(range(ss.n))
    assert sum(ss.rank(i) != i for i in range(ss.n)) >= ss.n - 4


def test_decode_seams():
    """Every row is the plain slice of the cleaned text or its reverse
    complement, and the oracle's row."""
    D, ss, eng = _decoded()
    got = eng.blocks()
    _named(D, got, D.want)
    o = orc.BlockSetOracle(list(D.raw), list(D.names))
    o.set_blocks([list(b) for b in D.blocks])
    _named(D, got, o.apply("DummyAligner").blocks())
    assert eng.rows_digest() == rows_digest(D.want)


def test_decode_seams_without_chunks():
    """refine-chunk 0 (the long rows refined whole) gives the same rows and
    the same digest as the default."""
    D, ss, eng = _decoded(0)
    _named(D, eng.blocks(), D.want)
    D, ss1, eng1 = _decoded()
    assert eng.rows_digest() == eng1.rows_digest() == rows_digest(D.want)


@pytest.mark.parametrize("chunk", [256, 0])
def test_decode_ragged(chunk):
    """Fragments of unequal lengths: k_decode into padded rows, then k_refine
    (in chunks of 256 columns, or whole): the oracle's rows, whose letters are
    the slices, and one digest for both settings."""
    D = dc.cases()
    want = [list(b) for b in dc.ragged_rows()]
    ss, eng = _engine(list(D.raw), list(D.names))
    eng.tune("refine-chunk", chunk)
    eng.set_blocks([list(b) for b in D.ragged]).apply("DummyAligner")
    got = eng.blocks()
    assert [[f[4].replace("-", "") for f in b] for b in got] == [[dc.text(D, f) for f in b] for b in D.ragged]
    assert got == want
    assert eng.rows_digest() == rows_digest(want)
    c = eng.refine_counts()
    assert c["jobs"] == len(want) and (c["chunks"] > 0) == bool(chunk)
