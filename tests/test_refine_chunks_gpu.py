"""refine_alignment of a long block in independent chunks (k_refine_cuts, the
chunk jobs of k_refine, the gather by k_join_rows) against the one-wave path
and the oracle; the counts against the numpy restatement of the cut rule
(tests/refine_chunks_ref.py), so a path that falls back to one chunk fails."""
import pytest

import realign_ref as rr
import refine_chunks_ref as rc
import try_smth_ref as tr
from helpers import rows_digest
from npge_amd import synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def _three_ways(name, chunk=64, min_len=0):
    from npge_amd.aligner import refine_batch
    alns, exp = rc.cases()[name], rc.refined(name)
    counts, off = {}, {}
    got = refine_batch(alns, chunk=chunk, min_len=min_len, counts=counts)
    one = refine_batch(alns, chunk=0, min_len=min_len, counts=off)
    want = rc.expected_counts(alns, chunk, min_len, exp)
    print(name, chunk, min_len, counts)
    assert one == exp
    assert got == exp
    assert counts == want
    assert off == rc.expected_counts(alns, 0, min_len, exp)
    return counts


def test_kats():
    c = _three_ways("kats")
    assert c["long_jobs"] == 3


def test_random_long():
    c = _three_ways("random")
    assert c["chunks"] > 100 and c["longest_chunk"] < 1500


def test_homopolymer_runs():
    c = _three_ways("homopolymer")
    assert 1 < c["chunks"] < 24


def test_no_cut_is_one_chunk():
    c = _three_ways("no_cut")
    assert c["chunks"] == 1 and c["longest_chunk"] == len(rc.cases()["no_cut"][0][0])


@pytest.mark.parametrize("chunk,chunks", [(64, 4), (128, 3)])
def test_placed_cuts(chunk, chunks):
    c = _three_ways("placed", chunk=chunk)
    assert c["chunks"] == chunks


def test_pure_gap_columns_across_a_tile_border():
    _three_ways("pure_gap_border")


def test_wide():
    c = _three_ways("wide")
    assert c["chunks"] > 4


@pytest.mark.parametrize("min_len,long_jobs", [(301, 0), (300, 1), (299, 1)])
def test_min_len_boundary(min_len, long_jobs):
    c = _three_ways("boundary", min_len=min_len)
    assert c["long_jobs"] == long_jobs


def test_defaults_are_used():
    from npge_amd.aligner import refine_batch
    alns = [rc.cases()["random"][0], rc.cases()["random"][4]] + rc.cases()["boundary"]
    exp = [rc.refined("random")[0], rc.refined("random")[4]] + rc.refined("boundary")
    counts = {}
    assert refine_batch(alns, counts=counts) == exp
    assert counts == rc.expected_counts(alns, 256, 1024, exp)  # the defaults of "refine-chunk" / "refine-min-len"
    assert counts["long_jobs"] == 2  # 300 columns stay on the one-wave path


@pytest.mark.parametrize("chunk", [100, 32])
def test_bad_chunk(chunk):
    from npge_amd import _capi
    from npge_amd.aligner import refine_batch
    with pytest.raises(_capi.NpgxError) as e:
        refine_batch(rc.KATS, chunk=chunk, min_len=0)
    assert e.value.code == -1 and "chunk" in str(e.value)


# ---------------------------------------------------------------- the engine
def _engine(seqs, names, blocks=None):
    from npge_amd import _capi
    from npge_amd.blockset import BlockSetEngine
    eng = BlockSetEngine(_capi.SeqSet(seqs, names))
    if blocks is not None:
        eng.set_blocks(blocks)
    return eng


def test_tune_keys():
    from npge_amd import _capi
    eng = _engine(["ACGT"], ["a"])
    eng.tune("refine-chunk", 0).tune("refine-chunk", 4096).tune("refine-min-len", 0)
    for key, value in (("refine-chunk", 100), ("refine-chunk", 32), ("refine-chunk", -64), ("refine-min-len", -1)):
        with pytest.raises(_capi.NpgxError) as e:
            eng.tune(key, value)
        assert e.value.code == -1 and key in str(e.value)
    with pytest.raises(_capi.NpgxError) as e:
        eng.tune("refine", 1)
    assert "smth-rows, refine-chunk, refine-min-len)" in str(e.value)


def test_dummy_aligner_unequal_lengths():
    """DummyAligner's rows (letters first, gaps after; remove_pure_gaps first:
    flags bit 1) of fragments of unequal lengths, long enough to be cut."""
    import numpy as np
    rng = np.random.default_rng(91)
    x = "".join("ATGC"[i] for i in rng.integers(0, 4, 700))
    seqs = [x, x[:200] + x[230:], x[:520], x[:300] + "T" + x[300:]]
    names = ["a", "b", "c", "d"]
    blocks = [[(i, 0, len(s) - 1, 1, None) for i, s in enumerate(seqs)]]
    o = orc.BlockSetOracle(seqs, names)
    o.set_blocks(blocks)
    exp = o.apply("DummyAligner").blocks()
    rows = [s.ljust(len(seqs[3]), "-") for s in seqs]
    assert [f[4] for f in exp[0]] == rc.refine(rows)
    for chunk in (64, 0):
        eng = _engine(seqs, names, blocks).tune("refine-chunk", chunk).tune("refine-min-len", 256)
        assert eng.apply("DummyAligner").blocks() == exp
        c = eng.refine_counts()
        assert c == rc.expected_counts([rows], chunk, 256, [[f[4] for f in exp[0]]])
        assert c["chunks"] == (len(rc.chunk_list(rows, 64)) if chunk else 0) and (c["chunks"] > 1) == bool(chunk)


_DRAFT = {}


def _draft(cfg):
    """The engine's DraftPangenome output, then Joiner (made once)."""
    if cfg not in _DRAFT:
        from npge_amd.anchor_finder import AnchorFinder
        names, seqs = synth.genome_set(cfg)
        eng = _engine(seqs, names)
        eng.apply("DraftPangenome", af=AnchorFinder())
        draft = eng.blocks()
        _DRAFT[cfg] = (seqs, names, draft, eng.apply("Joiner").blocks())
    return _DRAFT[cfg]


@pytest.mark.parametrize("cfg", ["tiny", "rtiny"])
def test_realign_after_joiner(cfg):
    seqs, names, _, joined = _draft(cfg)
    exp_blocks, exp_counts = rr.realign(joined, seqs, names)
    for chunk in (64, 0):
        eng = _engine(seqs, names, joined).tune("refine-chunk", chunk).tune("refine-min-len", 256)
        before = eng.block_names()
        eng.apply("ReAlign")
        assert eng.blocks() == exp_blocks
        assert eng.block_names() == before
        assert eng.rows_digest() == rows_digest(exp_blocks)
        assert eng.realign_counts() == exp_counts
        c = eng.refine_counts()
        print(cfg, chunk, c)
        assert c["jobs"] >= exp_counts["candidates"] >= 1
        if chunk:
            assert c["long_jobs"] >= 1 and c["chunks"] > c["long_jobs"]
        else:
            assert c["long_jobs"] == 0 and c["chunks"] == 0


def test_try_smth_joiner_with_chunks():
    seqs, names, draft, _ = _draft("tiny")
    exp_blocks, exp_names = tr.try_smth(draft, seqs, names, "Joiner")
    eng = _engine(seqs, names, draft).tune("refine-chunk", 64).tune("refine-min-len", 256)
    eng.apply("TrySmth --smth-processor:=Joiner")
    assert eng.blocks() == exp_blocks
    assert eng.block_names() == exp_names
    assert eng.rows_digest() == rows_digest(exp_blocks)
    assert eng.refine_counts()["long_jobs"] >= 1
