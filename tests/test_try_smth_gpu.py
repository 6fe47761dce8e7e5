"""TrySmth on the engine (npgx_blockset_apply "TrySmth --smth-processor:=NAME")
against its sequential restatement (tests/try_smth_ref.py): fragments, rows,
order and block names; the refusals; a failing step gives the set back."""
import pytest

import try_smth_ref as tr
from helpers import rows_digest
from npge_amd import io as nio
from npge_amd import synth
from npge_amd.model import Block, BlockSet, Fragment, Sequence
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

INNER = ["FragmentsExtender", "FragmentsExtender --extend-length-portion:=0.5", "OriByMajority", "Joiner", "ReAlign",
         "AnchorLoopFast"]
CASES = [(cfg, inner) for cfg in ("tiny", "rtiny") for inner in INNER] + [("small", inner) for inner in INNER[:3]]


def _engine(seqs, names, blocks=None):
    from npge_amd import _capi
    from npge_amd.blockset import BlockSetEngine
    eng = BlockSetEngine(_capi.SeqSet(seqs, names))
    if blocks is not None:
        eng.set_blocks(blocks)
    return eng


_DRAFT = {}


def _draft(cfg):
    if cfg not in _DRAFT:
        names, seqs = synth.genome_set(cfg)
        o = orc.BlockSetOracle(seqs, names)
        o.apply("DraftPangenome")
        _DRAFT[cfg] = (seqs, names, o.blocks())
    return _DRAFT[cfg]


_REF = {}


def _ref(cfg, inner):
    if (cfg, inner) not in _REF:
        seqs, names, draft = _draft(cfg)
        info = {}
        _REF[(cfg, inner)] = tr.try_smth(draft, seqs, names, inner, info) + (info,)
    return _REF[(cfg, inner)]


def _apply(eng, inner):
    from npge_amd.anchor_finder import AnchorFinder
    tok = inner.split()
    call = " ".join(["TrySmth", "--smth-processor:=" + tok[0]] + tok[1:])
    return eng.apply(call, af=AnchorFinder() if tok[0] == "AnchorLoopFast" else None)


def _no_overlaps(blocks):
    per_seq = {}
    for b in blocks:
        for (q, mn, mx, _, _) in b:
            per_seq.setdefault(q, []).append((mn, mx))
    for v in per_seq.values():
        v.sort()
        assert all(a[1] < b[0] for a, b in zip(v, v[1:]))


@pytest.mark.parametrize("cfg,inner", CASES)
def test_try_smth_parity(cfg, inner):
    seqs, names, draft = _draft(cfg)
    exp_blocks, exp_names, info = _ref(cfg, inner)
    eng = _apply(_engine(seqs, names, draft), inner)
    got = eng.blocks()
    counts = eng.try_smth_counts()
    print(cfg, inner, counts)
    assert got == exp_blocks
    assert eng.block_names() == exp_names
    assert eng.rows_digest() == rows_digest(exp_blocks)
    _no_overlaps(got)
    assert counts["blocks_in"] == len(draft) and counts["blocks_out"] == len(got)
    assert counts["blocks_tried"] == len(info["tried"])
    assert counts["rounds"] == info["rounds"]
    assert counts["blocks_cut"] == len(info["cuts"]) and counts["pieces"] == sum(info["cuts"])
    assert counts["row_bytes"] == 0 and (counts["map_bytes"] > 0) == bool(info["cuts"])


def test_try_smth_host_rows_path():
    """smth-rows 0 gives the same set and downloads rows, no maps."""
    cfg, inner = "rtiny", "FragmentsExtender"
    seqs, names, draft = _draft(cfg)
    exp_blocks, exp_names, info = _ref(cfg, inner)
    assert info["cuts"]
    eng = _engine(seqs, names, draft).tune("smth-rows", 0)
    _apply(eng, inner)
    assert eng.blocks() == exp_blocks and eng.block_names() == exp_names
    c = eng.try_smth_counts()
    assert c["map_bytes"] == 0 and c["row_bytes"] > 0


def test_try_smth_script():
    from npge_amd.script import run_script
    seqs, names, draft = _draft("rtiny")
    exp_blocks, exp_names, _ = _ref("rtiny", INNER[1])
    bs = BlockSet()
    bs.seqs = [Sequence(n, s) for n, s in zip(names, seqs)]
    bs.blocks = [Block([Fragment(bs.seqs[q], mn, mx, o, r) for (q, mn, mx, o, r) in b], name="blk%03d" % i)
                 for i, b in enumerate(draft)]
    call = "run('TrySmth', \"--smth-processor:=FragmentsExtender --smth-opts:='--extend-length-portion:=0.5'\")"
    out = run_script("run_main('Read')\n%s\nrun_main('RawWrite')\n" % call, nio.write_blockset(bs))
    got = [[(names.index(f.seq.name), f.min_pos, f.max_pos, f.ori, f.row) for f in b.fragments] for b in out.blocks]
    assert got == exp_blocks
    # (the runner hands the engine fragments and rows, not names: the names are UniqueNames' own)
    assert [b.name for b in out.blocks] == exp_names


@pytest.mark.parametrize("call", ["TrySmth --smth-processor:=NoSuchProcessor", "TrySmth --smth-processor:=TrySmth",
                                  "TrySmth --smth-processor:=DraftPangenome", "TrySmth",
                                  "TrySmth --extend-length-portion:=0.5",
                                  "TrySmth --smth-processor:=FragmentsExtender --no-such-option:=1"])
def test_try_smth_refusals(call):
    from npge_amd import _capi
    seqs, names, draft = _draft("tiny")
    eng = _engine(seqs, names, draft)
    h, d = eng.hash(), eng.rows_digest()
    with pytest.raises(_capi.NpgxError) as e:
        eng.apply(call)
    assert e.value.code == -1  # NPGX_ERR_ARG
    assert eng.hash() == h and eng.rows_digest() == d and eng.blocks() == draft
    assert eng.block_names() == [tr.NULL] * len(draft)
    with pytest.raises(_capi.NpgxError) as e:
        eng.try_smth_counts()
    assert e.value.code == -5  # NPGX_ERR_STATE: no TrySmth has run


def test_joiner_overlap_under_try_smth():
    """Joiner refuses a pair whose facing fragments overlap (the input of
    tests/test_joiner_gpu.py): the error comes out of TrySmth, the set is what
    went in, and the copy is gone -- a following TrySmth on the handle works."""
    from npge_amd import _capi
    seqs = ["ACGTTGCAAGCTTAGCCGATATCGGA" * 2] * 2
    names = ["o1", "o2"]
    blocks = [[(0, 0, 9, 1, None), (1, 0, 9, 1, None)], [(0, 8, 17, 1, None), (1, 12, 20, 1, None)]]
    eng = _engine(seqs, names, blocks)
    h = eng.hash()
    with pytest.raises(_capi.NpgxError) as e:
        eng.apply("TrySmth --smth-processor:=Joiner")
    assert e.value.code == -1 and "o1_0_9" in str(e.value)
    assert eng.blocks() == blocks and eng.hash() == h and eng.block_names() == [tr.NULL] * 2
    exp_blocks, exp_names = tr.try_smth(blocks, seqs, names, "OriByMajority")
    eng.apply("TrySmth --smth-processor:=OriByMajority")
    assert eng.blocks() == exp_blocks and eng.block_names() == exp_names


def test_failure_gives_rows_back():
    """The same failure on aligned blocks: the rows come back too."""
    from npge_amd import _capi
    seqs, names, draft = _draft("tiny")
    a = draft[0]
    L = len(a[0][4])
    # the block cut in two with the halves' facing fragments made to overlap: Joiner matches and refuses them
    left = tr.slice_block(a, 0, L // 2 + 4, seqs)
    right = tr.slice_block(a, L // 2 - 5, L - 1, seqs)
    blocks = [left, right] + draft[1:3]
    eng = _engine(seqs, names, blocks)
    h, d = eng.hash(), eng.rows_digest()
    with pytest.raises(_capi.NpgxError) as e:
        eng.apply("TrySmth --smth-processor:=Joiner")
    assert e.value.code == -1
    assert eng.blocks() == blocks and eng.hash() == h and eng.rows_digest() == d
    _apply(eng, "OriByMajority")
    exp_blocks, exp_names = tr.try_smth(blocks, seqs, names, "OriByMajority")
    assert eng.blocks() == exp_blocks and eng.block_names() == exp_names


def _unchanged_then_works(eng, seqs, names, blocks, h, d):
    """The set is what went in; the copy and the held blocks are gone: a
    following TrySmth on the handle matches the restatement."""
    assert eng.blocks() == blocks and eng.hash() == h and eng.rows_digest() == d
    assert eng.block_names() == [tr.NULL] * len(blocks)
    _apply(eng, "OriByMajority")
    exp_blocks, exp_names = tr.try_smth(blocks, seqs, names, "OriByMajority")
    assert eng.blocks() == exp_blocks and eng.block_names() == exp_names


def test_failure_after_the_loop(monkeypatch):
    """A failure after AddingLoopBySize has aligned and cut its blocks (three
    rounds here): the set comes back from the copy, which the loop never
    touched."""
    from npge_amd import _capi
    seqs, names, draft = _draft("rtiny")
    assert _ref("rtiny", "FragmentsExtender")[2]["rounds"] == 3
    eng = _engine(seqs, names, draft)
    h, d = eng.hash(), eng.rows_digest()
    monkeypatch.setenv("NPGX_TEST_FAIL_TRY_SMTH", "1")
    with pytest.raises(_capi.NpgxError) as e:
        _apply(eng, "FragmentsExtender")
    assert e.value.code == -5 and "injected" in str(e.value)  # NPGX_ERR_STATE
    monkeypatch.delenv("NPGX_TEST_FAIL_TRY_SMTH")
    _unchanged_then_works(eng, seqs, names, draft, h, d)


def test_failure_while_the_step_holds_blocks(monkeypatch):
    """AnchorLoop fails while the set's own blocks wait in its held list."""
    from npge_amd import _capi
    from npge_amd.anchor_finder import AnchorFinder
    seqs, names, draft = _draft("tiny")
    eng = _engine(seqs, names, draft)
    h, d = eng.hash(), eng.rows_digest()
    monkeypatch.setenv("NPGX_TEST_FAIL_ANCHOR_LOOP", "1")
    with pytest.raises(_capi.NpgxError) as e:
        eng.apply("TrySmth --smth-processor:=AnchorLoop", af=AnchorFinder())
    assert e.value.code == -5 and "NPGX_TEST_FAIL_ANCHOR_LOOP" in str(e.value)
    monkeypatch.delenv("NPGX_TEST_FAIL_ANCHOR_LOOP")
    _unchanged_then_works(eng, seqs, names, draft, h, d)
