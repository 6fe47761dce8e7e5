"""The cut rule of the chunked refine_alignment on the CPU: the numpy
restatement (tests/refine_chunks_ref.py) with the oracle's refine_alignment
per chunk equals the oracle's refinement of the whole block, on the inputs
the GPU test (tests/test_refine_chunks_gpu.py) uses."""
import pytest

import refine_chunks_ref as rc


def test_tile_cuts_by_hand():
    #          0123456789
    rows = ["AACC-GGTTA",
            "AACCTGGTTA"]
    assert list(rc.solid_letters(rows)) == [ord(x) for x in "AACC"] + [0] + [ord(x) for x in "GGTTA"]
    # cuts: 1|2 (A C), 6|7 (G T), 8|9 (T A); 3|4 and 4|5 have a gap in column 4
    assert rc.tile_cuts(rows, 64) == [2]
    assert rc.tile_cuts(rows, 4) == [2, 7, 9]
    assert rc.chunk_list(rows, 4) == [(0, 2), (2, 7), (7, 9), (9, 10)]
    assert rc.chunk_list(rows, 64) == [(0, 2), (2, 10)]
    # a cut between the last column of a tile and the first of the next belongs to the first
    assert rc.tile_cuts(["AC", "AC"], 1) == [1, -1]
    assert rc.tile_cuts(["AA", "AA"], 1) == [-1, -1]  # one letter: no cut
    assert rc.tile_cuts(["A-", "AC"], 1) == [-1, -1]


@pytest.mark.parametrize("name", ["kats", "random", "homopolymer", "no_cut", "placed", "pure_gap_border", "wide",
                                  "boundary"])
@pytest.mark.parametrize("chunk", [64, 128])
def test_chunks_equal_whole(name, chunk):
    for a, whole in zip(rc.cases()[name], rc.refined(name)):
        assert rc.refine_chunked(a, chunk) == whole


def test_inputs_have_the_shapes_they_are_for():
    cs = rc.cases()
    for a in cs["random"]:
        cuts = rc.tile_cuts(a, 64)
        assert 2 <= len(a) <= 17 and 1500 <= len(a[0])
        assert 2 * sum(c >= 0 for c in cuts) >= len(cuts)  # at least half of the tiles yield a cut
    assert rc.chunk_list(cs["no_cut"][0], 64) == [(0, len(cs["no_cut"][0][0]))]
    h = cs["homopolymer"][0]
    cuts = rc.tile_cuts(h, 64)
    assert 0 < sum(c >= 0 for c in cuts) < len(cuts)  # cuts are rare, not absent
    p = cs["placed"][0]
    L = len(p[0])
    assert rc.chunk_list(p, 128) == [(0, 64), (64, L - 1), (L - 1, L)]  # the first cut of a tile only
    assert rc.chunk_list(p, 64) == [(0, 64), (64, 128), (128, L - 1), (L - 1, L)]
    g = cs["pure_gap_border"][0]
    assert all(set(r[56:72]) == {"-"} for r in g) and len(rc.chunk_list(g, 64)) > 2
    assert len(cs["wide"][0]) == 70 and len(cs["wide"][0][0]) >= 2000
    assert len(cs["boundary"][0][0]) == 300
