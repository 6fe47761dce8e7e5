"""SmthUnion's cuts from the device letter maps ("smth-rows" 1, the default)
against the host copy of the rows ("smth-rows" 0) and the oracle's
AddingLoopBySize, on sets whose blocks overlap: every block of a DraftPangenome
output twice at partly overlapping places, a block of more than 4096 columns
(tiny's first), a block of more than 64 rows."""
import pytest

import try_smth_cases as tc
import try_smth_ref as tr
from helpers import rows_digest
from npge_amd import synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

_CASES = {}


def _case(name):
    """(seqs, names, blocks, the oracle's AddingLoopBySize, pieces per cut block)."""
    if name not in _CASES:
        if name == "wide":
            seqs, names, blocks = tc.wide_case()
        else:
            names, seqs = synth.genome_set(name)
            o = orc.BlockSetOracle(seqs, names)
            o.apply("DraftPangenome")
            blocks = tc.overlapping_set(o.blocks(), seqs)
        pipe = tr.Pipe(seqs, names)
        info = {}
        ref = tr.adding_loop([(tr.NULL, b, "x") for b in blocks], pipe, info)
        exp = pipe.op(blocks, "AddingLoopBySize")
        assert [b for (_, b, _) in ref] == exp
        _CASES[name] = (seqs, names, blocks, exp, info["cuts"])
    return _CASES[name]


def _run(seqs, names, blocks, smth_rows):
    from npge_amd import _capi
    from npge_amd.blockset import BlockSetEngine
    eng = BlockSetEngine(_capi.SeqSet(seqs, names)).set_blocks(blocks)
    eng.tune("smth-rows", smth_rows)
    return eng.apply("AddingLoopBySize")


@pytest.mark.parametrize("name", ["tiny", "rtiny", "wide"])
def test_both_paths_equal_the_oracle(name):
    seqs, names, blocks, exp, cuts = _case(name)
    assert max(cuts) >= 2  # a block cut into two pieces or more
    if name == "tiny":
        assert any(len(b[0][4]) > 4096 for b in blocks)
    if name == "wide":
        assert any(len(b) > 64 for b in blocks)
    dev, host = _run(seqs, names, blocks, 1), _run(seqs, names, blocks, 0)
    got = dev.blocks()
    assert got == host.blocks()
    assert got == exp
    assert dev.rows_digest() == host.rows_digest() == rows_digest(exp)
    assert dev.hash() == host.hash()
    cd, ch = dev.smth_counts(), host.smth_counts()
    print(name, "device", cd, "host", ch)
    assert cd["row_bytes"] == 0 and cd["map_bytes"] > 0
    assert ch["map_bytes"] == 0 and ch["row_bytes"] > 0
    assert cd["blocks_cut"] == ch["blocks_cut"] == len(cuts)
    assert cd["pieces"] == ch["pieces"] == sum(cuts)
    # 12 bytes a word of 64 cells and 4 a tile against one byte a cell: under
    # half a byte a cell for any row of 32 columns or more (3/16 for long rows)
    assert cd["map_bytes"] < ch["row_bytes"] / 2


def test_smth_rows_key():
    from npge_amd import _capi
    seqs, names, blocks, _, _ = _case("wide")
    eng = _run(seqs, names, blocks[:1], 1)
    with pytest.raises(_capi.NpgxError) as e:
        eng.tune("smth-rows", 2)
    assert e.value.code == -1  # NPGX_ERR_ARG
    with pytest.raises(_capi.NpgxError) as e:
        eng.tune("smth-cols", 1)
    assert e.value.code == -1 and "smth-rows" in str(e.value)


def test_letter_map_in_kernel_times(monkeypatch):
    monkeypatch.setenv("NPGX_TIMERS", "2")
    seqs, names, blocks, _, _ = _case("wide")
    kt = {k["name"]: k for k in _run(seqs, names, blocks, 1).kernel_times()}
    assert "letter_map" in kt and "smth_rows" not in kt
    assert "smth_rows" in {k["name"] for k in _run(seqs, names, blocks, 0).kernel_times()}
