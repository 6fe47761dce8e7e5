"""LiteFilter, MergeUnique and the JoinerP, MergeAndJoin and LiteJoinerP pipes
on the engine against their sequential restatement
(tests/joiner_pipes_ref.py): blocks, order, block names, rows and
MergeUnique's counts; under TrySmth; through the script runner; refusals."""
import pytest

import joiner_pipes_ref as jp
from helpers import rows_digest
from npge_amd import io as nio
from npge_amd import synth
from npge_amd.model import Block, BlockSet, Fragment, Sequence

pytestmark = pytest.mark.gpu

NULL = jp.NULL
# (the engine's call, the restatement's processor and options); LiteFilter and MergeUnique run after Rest
PROCS = {
    "LiteFilter": ("LiteFilter", {}),
    "LiteFilter --min-fragment=150 --min-block=3": ("LiteFilter", dict(min_fragment=150, min_block=3)),
    "MergeUnique": ("MergeUnique", {}),
    "MergeUnique --both-neighbours=0": ("MergeUnique", dict(both=False)),
    "MergeUnique --merge-long=1": ("MergeUnique", dict(merge_long=True)),
    "JoinerP": ("JoinerP", {}),
    "MergeAndJoin": ("MergeAndJoin", {}),
    "LiteJoinerP": ("LiteJoinerP", {}),
}
INPUTS = ["hand", "hand3", "tiny", "rtiny", "small"]


def _engine(seqs, names, blocks=None):
    from npge_amd import _capi
    from npge_amd.blockset import BlockSetEngine
    eng = BlockSetEngine(_capi.SeqSet(seqs, names))
    if blocks is not None:
        eng.set_blocks(blocks)
    return eng


_IN = {}


def _input(cfg):
    """(seqs, names, blocks, blocks after Rest), made once."""
    if cfg not in _IN:
        if cfg.startswith("hand"):
            seqs, names, blocks = jp.hand_case(fourth=cfg == "hand")
        else:
            from npge_amd.anchor_finder import AnchorFinder
            names, seqs = synth.genome_set(cfg)
            blocks = _engine(seqs, names).apply("DraftPangenome", af=AnchorFinder()).blocks()
        _IN[cfg] = (seqs, names, blocks, _engine(seqs, names, blocks).apply("Rest").blocks())
    return _IN[cfg]


_REF = {}


def _ref(cfg, call):
    if (cfg, call) not in _REF:
        seqs, names, blocks, rested = _input(cfg)
        name, opts = PROCS[call]
        counts = {}
        src = rested if name in ("LiteFilter", "MergeUnique") else blocks
        _REF[(cfg, call)] = jp.run(name, src, seqs, names, counts=counts, **opts) + (counts, src)
    return _REF[(cfg, call)]


@pytest.mark.parametrize("call", list(PROCS))
@pytest.mark.parametrize("cfg", INPUTS)
def test_parity(cfg, call):
    seqs, names, _, _ = _input(cfg)
    exp_blocks, exp_names, exp_counts, src = _ref(cfg, call)
    eng = _engine(seqs, names, src).apply(call)
    assert eng.blocks() == exp_blocks
    assert eng.block_names() == exp_names
    assert eng.rows_digest() == rows_digest(exp_blocks)
    if exp_counts:
        print(cfg, call, exp_counts)
        assert eng.merge_unique_counts() == exp_counts


def test_something_merges():
    """The parity above is not vacuous: the hand-made case and a synthetic set merge."""
    assert _ref("hand", "MergeUnique")[1][-1] == "m3x40" and _ref("hand", "MergeUnique --both-neighbours=0")[1][-1] == "m4x40"
    assert _ref("hand3", "JoinerP")[2] == dict(blocks_inspected=2, merges=1, fragments_merged=3)
    assert len(_ref("hand3", "JoinerP")[0]) == 1
    assert _ref("small", "JoinerP")[2]["merges"] >= 10 and _ref("rtiny", "MergeUnique")[2]["merges"] >= 1
    assert _ref("small", "MergeUnique --merge-long=1")[0] != _ref("small", "MergeUnique")[0]


def test_merged_rows_and_the_gapped_flip():
    """Rows of one length stay (the flipped fragment's reverse-complemented);
    a gapped row that would flip is refused and the set stays as it was."""
    from npge_amd import _capi
    seqs, names, _, rested = _input("hand")
    eng = _engine(seqs, names, rested).apply("MetaAligner")
    aligned = eng.blocks()
    exp_blocks, exp_names = jp.merge_unique(aligned, [NULL] * len(aligned))
    assert [f[4] for f in exp_blocks[-1]] == [seqs[0][300:340], seqs[1][300:340], jp.jr.revcomp(seqs[2][300:340])]
    eng.apply("MergeUnique")
    assert eng.blocks() == exp_blocks and eng.block_names() == exp_names
    assert eng.rows_digest() == rows_digest(exp_blocks)
    gapped = [[f[:4] + (f[4][:5] + "-" + f[4][5:],) for f in b] if len(b) == 1 else b for b in aligned]
    with pytest.raises(jp.GappedFlip):
        jp.merge_unique(gapped, [NULL] * len(gapped))
    eng = _engine(seqs, names, gapped)
    h, d = eng.hash(), eng.rows_digest()
    with pytest.raises(_capi.NpgxError) as e:
        eng.apply("MergeUnique")
    assert e.value.code == -1 and "s2_300_339" in str(e.value)
    assert eng.blocks() == gapped and eng.hash() == h and eng.rows_digest() == d
    mixed = [gapped[k] if k == 2 else b for k, b in enumerate(aligned)]  # rows of 41, 40 and 40 columns: no rows
    exp_blocks, exp_names = jp.merge_unique(mixed, [NULL] * len(mixed))
    eng = _engine(seqs, names, mixed).apply("MergeUnique")
    assert eng.blocks() == exp_blocks and eng.block_names() == exp_names and exp_names[-1] == "m3x41"


@pytest.mark.parametrize("cfg", ["tiny", "rtiny"])
def test_try_smth_joinerp(cfg):
    seqs, names, blocks, _ = _input(cfg)
    exp_blocks, exp_names = jp.try_smth(blocks, seqs, names, "JoinerP")
    eng = _engine(seqs, names, blocks).apply("TrySmth --smth-processor:=JoinerP")
    assert eng.blocks() == exp_blocks
    assert eng.block_names() == exp_names
    assert eng.rows_digest() == rows_digest(exp_blocks)
    assert eng.try_smth_counts()["blocks_in"] == len(blocks)
    assert eng.merge_unique_counts()["blocks_inspected"] >= 1


@pytest.mark.parametrize("inner", ["LiteFilter", "MergeUnique", "MergeAndJoin", "LiteJoinerP"])
def test_try_smth_accepts_the_others(inner):
    seqs, names, blocks, _ = _input("tiny")
    exp_blocks, exp_names = jp.try_smth(blocks, seqs, names, inner)
    eng = _engine(seqs, names, blocks).apply("TrySmth --smth-processor:=" + inner)
    assert eng.blocks() == exp_blocks and eng.block_names() == exp_names


@pytest.mark.parametrize("call,script", [
    ("JoinerP", "run('JoinerP')"), ("MergeAndJoin", "run 'MergeAndJoin'"), ("LiteJoinerP", "run('LiteJoinerP')"),
    ("MergeUnique --both-neighbours=0", "run('MergeUnique', '--both-neighbours:=0')"),
    ("LiteFilter --min-fragment=150 --min-block=3", "run('LiteFilter', '--min-fragment:=150 --min-block:=3')")])
def test_script(call, script):
    from npge_amd.script import run_script
    seqs, names, _, _ = _input("rtiny")
    exp_blocks, exp_names, _, src = _ref("rtiny", call)
    bs = BlockSet()
    bs.seqs = [Sequence(n, s) for n, s in zip(names, seqs)]
    bs.blocks = [Block([Fragment(bs.seqs[q], mn, mx, o, r) for (q, mn, mx, o, r) in b], name="blk%03d" % i)
                 for i, b in enumerate(src)]
    out = run_script("run_main('Read')\n%s\nrun_main('RawWrite')\n" % script, nio.write_blockset(bs))
    got = [[(names.index(f.seq.name), f.min_pos, f.max_pos, f.ori, f.row) for f in b.fragments] for b in out.blocks]
    assert got == exp_blocks
    if call.startswith("LiteFilter"):  # the blocks that stay keep the names they came with
        kept = {tuple(f[:3] for f in b): "blk%03d" % i for i, b in enumerate(src)}
        assert [b.name for b in out.blocks] == [kept[tuple(f[:3] for f in b)] for b in exp_blocks]
    else:  # (the runner hands the engine no names: the engine's own come back)
        assert [b.name for b in out.blocks] == exp_names


@pytest.mark.parametrize("call", ["LiteFilter --max-block=3", "MergeUnique --min-fragment=10", "JoinerP --merge-long=1",
                                  "MergeAndJoin --both-neighbours=0", "LiteJoinerP --min-block=2",
                                  "LiteFilter --min-block=-1", "MergeUnique --merge-long=2"])
def test_unknown_option(call):
    from npge_amd import _capi
    seqs, names, blocks, _ = _input("hand")
    eng = _engine(seqs, names, blocks)
    with pytest.raises(_capi.NpgxError) as e:
        eng.apply(call)
    assert e.value.code == -1  # NPGX_ERR_ARG
    assert eng.blocks() == blocks


def test_counts_before_any_merge_unique():
    from npge_amd import _capi
    seqs, names, blocks, _ = _input("hand")
    eng = _engine(seqs, names, blocks).apply("LiteJoinerP")
    with pytest.raises(_capi.NpgxError) as e:
        eng.merge_unique_counts()
    assert e.value.code == -5  # NPGX_ERR_STATE
