"""The oracle alone over decode_cases.py, on the CPU: to_atgcn is the plain
Python rule, DummyAligner's rows of the row-less twin blocks are the plain
slices, and the inputs hold the seams test_decode_seams_gpu.py names."""
import decode_cases as dc
from decode_cases import orc


def test_to_atgcn():
    """Lower case, IUPAC letters (N) and dropped characters."""
    assert orc.to_atgcn(dc.KAT[0]) == dc.KAT[1] == dc.py_atgcn(dc.KAT[0])
    D = dc.cases()
    assert [orc.to_atgcn(r) for r in D.raw] == D.clean == [dc.py_atgcn(r) for r in D.raw]
    raw = "".join(D.raw)
    assert set(dc.IUPAC) <= set(raw.upper()) and set(dc.DROPPED) <= set(raw) and set("atgcn") <= set(raw)
    assert sum(r != c for r, c in zip(D.raw, D.clean)) >= len(D.raw) // 2
    for i, j in enumerate(D.twin):  # the twin holds the same text, spelled another way
        assert D.clean[i] == D.clean[j] and D.names[i] != D.names[j] and (D.raw[i] != D.raw[j] or "N" not in D.raw[i])


def test_sequences_hold_the_seams():
    D = dc.cases()
    assert 36 <= len(D.clean) <= 44
    assert sorted(set(len(c) for c in D.clean)) == sorted(dc.LENGTHS + (dc.LONG, dc.N_ONLY))
    assert "N" * dc.N_ONLY in D.clean
    # rank order (size descending, name ascending) is not input order, twins are no neighbours in name order
    rank = sorted(range(len(D.clean)), key=lambda i: (-len(D.clean[i]), D.names[i], i))
    assert sum(r != i for i, r in enumerate(rank)) >= len(rank) - 4
    assert len(set(D.names)) == len(D.names)
    # every named N position is in some sequence ...
    have = set()
    for c in D.clean:
        have |= {name for name, p in dc.n_positions(len(c)).items() if c[p] == "N"}
    assert have == {"first", "last", "31", "32", "63", "64", "8191", "8192", "16383", "16384"}
    # ... and decoded in both orientations (test_decode_rows_are_slices holds the rows against the slices)
    seen = set()
    for b in D.want:
        for (q, mn, mx, ori, row) in b:
            for name, p in dc.n_positions(len(D.clean[q])).items():
                if mn <= p <= mx and D.clean[q][p] == "N":
                    assert row[p - mn if ori == 1 else mx - p] == "N"
                    seen.add((name, ori))
    assert seen == {(name, ori) for name in have for ori in (1, -1)}


def test_fragments_cover_the_seams():
    D = dc.cases()
    got = {(f[1] % 64, f[2] - f[1] + 1, f[3]) for b in D.blocks for f in b}
    assert got >= {(p, ln, ori) for p in dc.POS for ln in dc.FRAG for ori in (1, -1)}
    whole = {(f[2] + 1) for b in D.blocks for f in b if f[1] == 0 and f[2] + 1 == len(D.clean[f[0]])}
    assert whole == set(len(c) for c in D.clean)
    assert all(len(b) == 2 and b[0][0] == D.twin[b[1][0]] and {b[0][3], b[1][3]} == {1, -1} and b[0][1:3] == b[1][1:3]
               for b in D.blocks)
    assert {b[0][0] < b[1][0] for b in D.blocks} == {True, False}
    # reverse fragments start (at their last base) on every residue a forward one starts on
    assert {f[2] % 64 for b in D.blocks for f in b if f[3] == -1} >= set(dc.POS)
    assert max(f[2] - f[1] + 1 for b in D.blocks for f in b) == dc.LONG <= 16450
    assert sum(f[2] - f[1] + 1 > 8192 for b in D.blocks for f in b) >= 20  # more than one decode op


def test_decode_rows_are_slices():
    """The oracle's DummyAligner on the row-less blocks gives exactly the
    slices, among them (31, 8193, -1), (0, 1, +1), (64, 65, -1) and
    (33, 16385, +1) (pos, length, ori)."""
    D = dc.cases()
    o = orc.BlockSetOracle(list(D.raw), list(D.names))
    o.set_blocks([list(b) for b in D.blocks])
    got = o.apply("DummyAligner").blocks()
    assert got == D.want
    assert all("-" not in f[4] for b in got for f in b)
    assert set("".join(f[4] for b in got for f in b)) == set("ATGCN")
    have = {(f[1] % 64, f[2] - f[1] + 1, f[3]) for b in D.blocks for f in b}
    assert {(31, 8193, -1), (0, 1, 1), (0, 65, -1), (33, 16385, 1)} <= have


def test_ragged_rows_hold_the_slices():
    D = dc.cases()
    got = dc.ragged_rows()
    assert [[f[:4] for f in b] for b in got] == [[f[:4] for f in b] for b in D.ragged]
    for b in got:
        assert len({len(f[4]) for f in b}) == 1 and any("-" in f[4] for f in b)
        for f in b:
            assert f[4].replace("-", "") == dc.text(D, f)
    assert sum(len(b[0][4]) >= 1024 for b in got) >= 6  # long enough for the chunked refinement
