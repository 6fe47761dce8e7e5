"""Aligner and block-build options off their defaults: the engine (through the
C ABI) against the oracle run with the same options, bit-exact (rows,
fragment coordinates, stats; no tolerances).

The vectors and inputs live in option_cases.py; test_oracle_options.py shows
on the CPU that every one of them moves the oracle's result on these inputs.

* Aligner: every vector on the short or mid set (narrow kernels, vector and
  row-parallel searches), four vectors through the split and deferred forms
  (k_split_post, k_align_sub), the wide aligner and its prefix search, and
  aligned_check 2 / 16 through try_aligned's prefix search.
* Block build: FragmentsExtender -> FixEnds -> FragmentsExtender -> Filter on
  `tiny` once per variation (the goodSlices guard included), the combined
  vector on `small` (blocks past SMALL_FE_ROWS) and on one block of more than
  4,096 columns (past SMALL_FE_WORDS), min_block / max_block on blocks of 2 and
  3 fragments, MetaAligner with two align vectors, and DraftPangenome with
  three vectors on the host loop and the device loop.
"""
import pytest

from npge_amd.processor import Decimal

import option_cases as oc
from test_block_build_gpu import _engine, canon

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- aligner
def _check_align(name, v):
    from npge_amd.aligner import BatchAligner
    jobs = [list(j) for j in oc.jobs(name)]
    al = BatchAligner(mismatch_check=v[0], gap_check=v[1], aligned_check=v[2], min_length=v[3],
                      min_identity=Decimal.raw(v[4]))
    got = al.align(jobs)
    exp = oc.oracle_align(name, v)
    bad = [j for j in range(len(jobs)) if tuple(got[j]) != exp[j]]
    assert not bad, "%s on %s: %d of %d jobs differ, first job %d (%d rows, lengths %s)" % (
        v, name, len(bad), len(jobs), bad[0], len(jobs[bad[0]]), [len(r) for r in jobs[bad[0]]][:8])


@pytest.mark.parametrize("vector,name", oc.ALIGN_VECTORS, ids=[oc.vid(v) for v, _ in oc.ALIGN_VECTORS])
def test_aligner_vector(vector, name):
    _check_align(name, vector)


@pytest.mark.parametrize("defer", [None, "1"])
@pytest.mark.parametrize("split", ["128", "384"])
@pytest.mark.parametrize("vector", oc.LEG_VECTORS, ids=oc.vid)
def test_aligner_vector_split_deferred(vector, split, defer, monkeypatch):
    """Jobs cut at sync states (k_split_post merges the rounds with
    min_length and the weight factor by its own code) and fix_bad_regions'
    re-alignments as sub-jobs (k_align_sub)."""
    monkeypatch.setenv("NPGX_ALIGN_SPLIT", split)
    if defer is None:
        monkeypatch.delenv("NPGX_ALIGN_DEFER", raising=False)
    else:
        monkeypatch.setenv("NPGX_ALIGN_DEFER", defer)
    _check_align("long", vector)


@pytest.mark.parametrize("vector", oc.LEG_VECTORS, ids=oc.vid)
def test_aligner_vector_wide(vector):
    _check_align("wide", vector)


def test_aligner_vector_wide_prefix_search(monkeypatch):
    monkeypatch.setenv("NPGX_WIDE_LONG_HEAD", "4")
    _check_align("wide_restart", oc.LEG_VECTORS[0])


@pytest.mark.parametrize("vector", oc.PREFIX_VECTORS, ids=oc.vid)
def test_aligner_vector_prefix_search(vector):
    _check_align("prefix", vector)


# ---------------------------------------------------------------- block build
def _tiny(cfg="tiny"):
    names, seqs = oc.genome_set(cfg)
    return list(names), list(seqs)


@pytest.mark.parametrize("name,kw", oc.BB_VARIATIONS, ids=[n for n, _ in oc.BB_VARIATIONS])
def test_chain_variation(name, kw):
    _check_chain("tiny", kw)


def _check_chain(cfg, kw):
    names, seqs = _tiny(cfg)
    want = oc.oracle_chain(cfg, kw)
    ss, eng = _engine(seqs, names, **kw)
    cur = oc.thaw(oc.stem_blocks(cfg))
    for step, (op, ordered) in enumerate(zip(oc.CHAIN, oc.CHAIN_ORDERED)):
        if ordered:
            eng.set_blocks(cur)
        eng.apply(op)
        exp = oc.thaw(want[step])
        if ordered:
            assert eng.blocks() == exp, (step, op)
        else:
            assert canon(eng.blocks()) == canon(exp), (step, op)
        cur = exp


def test_chain_combined_small():
    """5-row blocks: past SMALL_FE_ROWS into k_col_bits + k_fix_ends."""
    _check_chain("small", oc.COMBINED)


def test_combined_long_block():
    """One 3-row block of more than 4,096 columns: more than one column tile."""
    names, seqs, blocks = oc.long_block()
    want = oc.oracle_long_block(oc.COMBINED)
    ss, eng = _engine(list(seqs), list(names), **oc.COMBINED)
    for op, exp in zip(("FixEnds", "Filter"), want):
        eng.set_blocks(oc.thaw(blocks)).apply(op)
        assert canon(eng.blocks()) == canon(oc.thaw(exp)), op


@pytest.mark.parametrize("name,kw", oc.BLOCK_SIZE_VARIATIONS, ids=[n for n, _ in oc.BLOCK_SIZE_VARIATIONS])
def test_filter_block_sizes(name, kw):
    names, seqs = _tiny()
    ss, eng = _engine(seqs, names, **kw)
    eng.set_blocks(oc.thaw(oc.mixed_size_blocks())).apply("Filter")
    assert canon(eng.blocks()) == canon(oc.thaw(oc.oracle_filter_mixed(kw)))


@pytest.mark.parametrize("vector", oc.META_VECTORS, ids=oc.vid)
def test_meta_aligner_vector(vector):
    names, seqs = _tiny()
    ss, eng = _engine(seqs, names, **oc.align_kw(vector))
    eng.set_blocks(oc.thaw(oc.meta_blocks())).apply("MetaAligner")
    assert eng.blocks() == oc.thaw(oc.oracle_meta(vector))


@pytest.mark.parametrize("cfg", ["tiny", "rtiny"])
@pytest.mark.parametrize("name,kw", oc.PIPE_VECTORS, ids=[n for n, _ in oc.PIPE_VECTORS])
def test_draft_pangenome_vector(name, kw, cfg, monkeypatch):
    """The host loop and the device loop read the options through different
    code (the host plan and PlanArgs / FiArgs on the device)."""
    from npge_amd.anchor_finder import AnchorFinder
    names, seqs = _tiny(cfg)
    want, ost = oc.oracle_draft(cfg, kw)
    assert want
    digests = []
    for device in ("0", "1"):
        monkeypatch.setenv("NPGX_ELF_DEVICE", device)
        monkeypatch.setenv("NPGX_ELF_CHECK", "1")  # a bad table or flank plan fails loudly instead of faulting
        ss, eng = _engine(seqs, names, **kw)
        eng.apply("DraftPangenome", af=AnchorFinder())
        st = eng.stats()
        for k in ("anchor_blocks", "stem_blocks", "iterations", "aligned_residues"):
            assert st[k] == ost[k], (device, k)
        assert canon(eng.blocks()) == canon(oc.thaw(want)), device
        assert (st["device_iterations"] > 0) == (device == "1")
        digests.append(eng.rows_digest())
    assert digests[0] == digests[1]
