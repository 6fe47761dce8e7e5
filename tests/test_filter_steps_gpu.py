"""Filter's steps that no other test reaches: a block with an invalid fragment
(its max at or past its sequence's end) that does not pass, so Filter drops
the fragment and tries the rest again (Filter.cpp:230-246; the engine's
FilterPass::retry_without_invalid), engine against oracle bit for bit
(fragments, rows and the block count; no tolerances).  The inputs are
column_cases.filter_invalid's, blocks of 2-3 rows and 300-400 columns under
the default options; invalid_result asserts the oracle's outcome of each case
before the engine runs:

* drop_then_keep: the rest passes whole and is kept with the input's rows.
* drop_then_slice: the rest has a burst of 30 mismatches: two slices, their
  letter counts from one pass over each downloaded row.
* drop_then_gone: one fragment is left, fewer than min_block: no block.
* drop_no_subblocks: drop_then_keep under find_subblocks=0.
* all_valid_control: drop_then_slice's rows with the third fragment valid:
  nothing is dropped and the outcome is another.

Not here: a block with an invalid fragment that passes goodSlices whole under
find_subblocks=1.  The engine drops the fragment and keeps the block, the
oracle slices the whole block, and the reference asserts on that input
(Filter.cpp:222-223): the answer is not defined.

The other mode, find_good_subblocks alone (FilterPass::emit_subblocks), runs
only inside AnchorLoop's SplitExtendable:
test_anchor_loop_full_gpu.py::test_anchor_loop asserts split_blocks > 0 and
equal to the oracle's on every set.
"""
import pytest

import column_cases as cc
from test_column_shapes_gpu import _eng, _filter_counts, _same

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", cc.INVALID_CASES)
def test_invalid_fragment(name):
    S, want = cc.invalid_result(name)
    eng = _eng(S)
    eng.set_blocks(S.input()).apply("Filter")
    _same(S, eng.blocks(), want, "Filter " + name)
    whole, sliced, _ = _filter_counts(S, want)
    assert (whole, sliced) == (0, 0 if name == "drop_no_subblocks" else 1)
    c = eng.stats()["counters"]
    assert (c["filter_whole"], c["filter_slices"]) == (whole, sliced)
