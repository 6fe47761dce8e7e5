"""The reference's own known answers for Joiner and OriByMajority
(src/test/joiner.cpp, src/test/ori_by_majority.cpp), shared by the CPU test of
the restatement and the GPU test of the engine.  Sequence texts are given as
the reference's InMemorySequence holds them (to_atgcn: upper case, '-'
dropped: "A-TGG" is the sequence ATGG).  Blocks are lists of
(seq_index, min_pos, max_pos, ori, row_or_None)."""
from joiner_ref import inverse


def _aligner_data(inv1=False, inv2=False):
    """AlignerData (joiner.cpp:238-271)."""
    b1 = [(0, 0, 1, 1, "AC"), (1, 0, 1, 1, "AC")]
    b2 = [(0, 5, 6, 1, "AT"), (1, 4, 5, 1, "AT")]
    return dict(seqs=["ACTGAAT", "ACTAAT"], blocks=[inverse(b1) if inv1 else b1, inverse(b2) if inv2 else b2],
                obm=True, n_blocks=1, size=2, consensus="ACTGAAT")


_S18 = "TGGTCCGAGATGCGGGCC"

# name -> seqs, blocks, obm (OriByMajority after Joiner), and what the reference checks
JOINER_KATS = {
    "Joiner_block": dict(  # joiner.cpp:18-34
        seqs=["TGAGATGCGGGCC", "TGGATGCGGGCC"],
        blocks=[[(0, 0, 0, 1, None), (1, 0, 0, 1, None)], [(0, 3, 4, 1, None), (1, 2, 3, 1, None)]],
        n_blocks=1),
    "Joiner_BlockSet_join": dict(  # :36-64
        seqs=[_S18, _S18],
        blocks=[[(0, 1, 2, 1, None), (1, 1, 2, 1, None)], [(0, 4, 6, -1, None), (1, 4, 6, -1, None)],
                [(0, 7, 8, 1, None), (1, 7, 8, 1, None)]],
        n_blocks=1, size=2, frag_len=8),
    "Joiner_BlockSet_join_wrong": dict(  # :66-92
        seqs=[_S18, _S18],
        blocks=[[(0, 1, 2, 1, None), (1, 1, 2, 1, None)], [(0, 4, 6, -1, None), (1, 4, 6, -1, None)],
                [(0, 7, 8, 1, None), (1, 7, 8, -1, None)]],
        n_blocks=2),
    "Joiner_alternation": dict(  # :94-114
        seqs=["ATATATATATAT"],
        blocks=[[(0, 0, 1, 1, None), (0, 4, 5, 1, None)], [(0, 2, 3, 1, None), (0, 6, 7, 1, None)]],
        n_blocks=1, size=2, aln_len=4, consensus="ATAT"),
    "Joiner_alignment": dict(  # :116-144
        seqs=["ACTGG", "ATGG"],
        blocks=[[(0, 0, 2, 1, "ACT"), (1, 0, 1, 1, "A-T")], [(0, 3, 4, 1, "GG"), (1, 2, 3, 1, "GG")]],
        obm=True, n_blocks=1, size=2, consensus="ACTGG"),
    "Joiner_alignment_2": dict(  # :146-174
        seqs=["ACTGG", "ATGG"],
        blocks=[[(0, 0, 1, 1, "AC"), (1, 0, 0, 1, "A-")], [(0, 2, 4, 1, "TGG"), (1, 1, 3, 1, "TGG")]],
        obm=True, n_blocks=1, size=2, consensus="ACTGG"),
    "Joiner_alignment_rev": dict(  # :176-204
        seqs=["ACTGG", "ATGG"],
        blocks=[[(0, 0, 1, -1, "GT"), (1, 0, 0, -1, "-T")], [(0, 2, 4, 1, "TGG"), (1, 1, 3, 1, "TGG")]],
        obm=True, n_blocks=1, size=2, consensus="ACTGG"),
    "Joiner_alignment_rev_2": dict(  # :206-234
        seqs=["ACTGG", "ATGG"],
        blocks=[[(0, 0, 1, 1, "AC"), (1, 0, 0, 1, "A-")], [(0, 2, 4, -1, "CCA"), (1, 1, 3, -1, "CCA")]],
        obm=True, n_blocks=1, size=2, consensus="ACTGG"),
    "Joiner_aligner": _aligner_data(),                # :273-284
    "Joiner_aligner_2": _aligner_data(inv1=True),     # :286-298
    "Joiner_aligner_3": _aligner_data(inv2=True),     # :300-312
    "Joiner_aligner_4": _aligner_data(True, True),    # :314-327
}

# OriByMajority_main (ori_by_majority.cpp:16-30): the tie leaves f1 at ori 1;
# with a third fragment of ori -1 the block is inverted
OBM_SEQ = "TGGTCCGAGCGGACGGCC"
OBM_TIE = [(0, 2, 6, 1, None), (0, 9, 13, -1, None)]
OBM_MINORITY = OBM_TIE + [(0, 9, 13, -1, None)]


def names_of(seqs):
    return ["s%d" % (i + 1) for i in range(len(seqs))]


def check_kat(case, blocks, consensus):
    """The reference's BOOST_CHECKs of one case on the blocks a Joiner
    (+ OriByMajority) left; consensus: block -> its consensus_string."""
    assert len(blocks) == case["n_blocks"]
    b = blocks[0]
    if "size" in case:
        assert len(b) == case["size"]
    if "frag_len" in case:
        assert b[0][2] - b[0][1] + 1 == case["frag_len"]
    if "aln_len" in case:
        assert (len(b[0][4]) if b[0][4] is not None else b[0][2] - b[0][1] + 1) == case["aln_len"]
    if "consensus" in case:
        assert consensus(b) == case["consensus"]
