"""The stage clock live (npgx_blockset_tune "stage-clock"): DraftPangenome on
the tiny set with the clock off / on and the device / host ExtendLoopFast.
The clock changes no result; off it leaves stats()["ms_gpu"] at 0; on, every
stage the path runs gets GPU time and the stages the path does not run get
none; the stages' sum is contained in the wall time of the apply call (every
event is recorded inside it); and the stats are the last apply's only."""
import os
import time

import pytest

from npge_amd import synth
from npge_amd.blockset import GPU_STAGE_NAMES

from test_block_build_gpu import _engine, canon

pytestmark = pytest.mark.gpu

DEVICE_STAGES = ("anchor_finder", "elf_plan", "flank_decode", "align", "stitch", "fix_ends", "overlapless_union",
                 "elf_download", "filter")
HOST_STAGES = ("anchor_finder", "extend_loop_host", "filter")
LOOP_ONLY = GPU_STAGE_NAMES[2:10]  # elf_upload ... elf_download: the device loop's own marks


def _timed_draft(eng):
    from npge_amd.anchor_finder import AnchorFinder
    af = AnchorFinder()
    t0 = time.perf_counter()
    eng.apply("DraftPangenome", af=af)
    wall_ms = (time.perf_counter() - t0) * 1e3
    return eng.stats(), wall_ms


@pytest.fixture(scope="module")
def runs():
    """(clock, device) -> blocks, rows digest, stats and wall ms of one
    DraftPangenome on a fresh engine, and of a second one on the same engine"""
    saved = {k: os.environ.pop(k, None) for k in ("NPGX_ELF_DEVICE", "NPGX_ANCHOR_DEVICE")}
    try:
        names, seqs = synth.genome_set("tiny")
        out = {}
        for clock in (0, 1):
            for device in (1, 0):
                ss, eng = _engine(seqs, names)
                eng.tune("stage-clock", clock)
                eng.tune("elf-device", device)
                st, wall = _timed_draft(eng)
                r = {"blocks": canon(eng.blocks()), "digest": eng.rows_digest(), "stats": st, "wall_ms": wall}
                if clock:
                    r["stats2"], r["wall2_ms"] = _timed_draft(eng)
                    r["blocks2"], r["digest2"] = canon(eng.blocks()), eng.rows_digest()
                out[(clock, device)] = r
        return out
    finally:
        for k, v in saved.items():
            if v is not None:
                os.environ[k] = v


def test_clock_and_loop_change_no_result(runs):
    first = runs[(0, 1)]
    assert len(first["blocks"]) > 0
    for key, r in runs.items():
        assert r["blocks"] == first["blocks"], key
        assert r["digest"] == first["digest"], key
        assert r["stats"]["iterations"] == first["stats"]["iterations"], key


@pytest.mark.parametrize("device", [1, 0])
def test_clock_off_books_nothing(runs, device):
    ms = runs[(0, device)]["stats"]["ms_gpu"]
    print(ms)
    assert list(ms) == GPU_STAGE_NAMES
    assert all(v == 0 for v in ms.values()), ms


def test_clock_on_device_loop(runs):
    st = runs[(1, 1)]["stats"]
    print(st["ms_gpu"], st["device_iterations"])
    assert st["device_iterations"] > 0
    for k in DEVICE_STAGES:
        assert st["ms_gpu"][k] > 0, (k, st["ms_gpu"])


def test_clock_on_host_loop(runs):
    st = runs[(1, 0)]["stats"]
    print(st["ms_gpu"], st["device_iterations"])
    assert st["device_iterations"] == 0
    for k in LOOP_ONLY:
        assert st["ms_gpu"][k] == 0, (k, st["ms_gpu"])
    for k in HOST_STAGES:
        assert st["ms_gpu"][k] > 0, (k, st["ms_gpu"])


@pytest.mark.parametrize("device", [1, 0])
def test_stages_are_contained_in_the_call(runs, device):
    r = runs[(1, device)]
    total = sum(r["stats"]["ms_gpu"].values())
    print(total, r["wall_ms"])
    assert 0 < total <= r["wall_ms"], (total, r["wall_ms"])


@pytest.mark.parametrize("device", [1, 0])
def test_second_apply_books_its_own_run_only(runs, device):
    """npgx_bb_stats is reset per apply: a second DraftPangenome on the same
    engine reports its own timeline (a sum over both runs would exceed the
    second call's wall time, the first holding the one-off set-up)."""
    r = runs[(1, device)]
    assert r["blocks2"] == r["blocks"] and r["digest2"] == r["digest"]
    st = r["stats2"]
    total = sum(st["ms_gpu"].values())
    print(st["ms_gpu"], total, r["wall2_ms"])
    assert 0 < total <= r["wall2_ms"], (total, r["wall2_ms"])
    for k in (DEVICE_STAGES if device else HOST_STAGES):
        assert st["ms_gpu"][k] > 0, (k, st["ms_gpu"])
    if not device:
        assert all(st["ms_gpu"][k] == 0 for k in LOOP_ONLY)
