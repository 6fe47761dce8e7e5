"""Exactly sharded AnchorFinder (npgx_af_run_sharded) on the GPU:
2 and 3 ranks (processes) share the box's one MI355X, exchanging over gloo with
host staging (RCCL cannot put two ranks on one GPU; the product path binds
the same callbacks to RCCL).  Every rank's result -- SoA anchors, |H|,
FoundFragment count, the persistent used-hash set over two runs -- must equal
the single-GPU npgx_af_run bit for bit, including truncation by
max-anchor-fragments and anchor-similar=false.  The cut's edge cases
(af_cut_cases.py), ranks that own no window and a pass 1 in several epochs
run sharded against the oracle."""
import os
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

KEYS = ("block_start", "seq", "min_pos", "max_pos", "ori")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _af(maxf, similar):
    from npge_amd.anchor_finder import AnchorFinder
    p = AnchorFinder()
    p.set_opt_value("max-anchor-fragments", maxf)
    p.set_opt_value("anchor-similar", similar)
    return p


def _pack(r, used):
    d = {k: np.asarray(r[k]) for k in KEYS}
    d.update(n_collected=r["n_collected"], n_found_frags=r["n_found_frags"], used=used)
    return d


def _worker(rank, world, port, config, maxf, similar, staging, out):
    import torch.distributed as dist
    from npge_amd import _capi, synth
    from npge_amd.comm import TorchComm
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _capi.check(_capi.lib().npgx_set_device(0))
    names, seqs = synth.genome_set(config)
    ss = _capi.SeqSet(seqs, names)
    comm = TorchComm(dist, staging=staging)
    sh = _af(maxf, similar)
    res = []
    for _ in range(2):  # second run: the persistent used-hash set is in play
        r = sh.find_sharded(ss, comm)
        res.append(_pack(r, sh.used_hashes()))
    ref = None
    if rank == 0:
        one = _af(maxf, similar)
        ref = []
        for _ in range(2):
            r = one.find(ss)
            ref.append(_pack(r, one.used_hashes()))
    out[rank] = (res, ref)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,config,maxf,similar,staging", [
    (2, "small", 100000, True, "cpu"),
    (3, "small", 5000, True, "cpu"),
    (2, "tiny", 100000, False, "cpu"),
    (2, "small", 100000, True, "cuda"),   # device staging tensors (the RCCL adapter's path)
    (4, "small", 100000, True, "cpu"),    # rank boundaries inside sequences: the `similar` rule across ranks
    (5, "tiny", 100000, True, "cpu"),
    (4, "tiny", 100000, False, "cpu"),
])
def test_sharded_equals_single(world, config, maxf, similar, staging):
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), config, maxf, similar, staging, out),
             nprocs=world, join=True)
    ref = out[0][1]
    assert len(ref[0]["seq"]) > 0
    for r in range(world):
        res = out[r][0]
        for run in range(2):
            a, b = res[run], ref[run]
            for k in KEYS:
                np.testing.assert_array_equal(a[k], b[k], err_msg="rank %d run %d %s" % (r, run, k))
            assert a["n_collected"] == b["n_collected"]
            assert a["n_found_frags"] == b["n_found_frags"]
            np.testing.assert_array_equal(a["used"], b["used"])


def _cases_worker(rank, world, port, jobs, env, out):
    """Every job (a case of af_cut_cases.py, its bloom-epochs, the oracle's
    runs) on one process group.  A mismatch is recorded, not raised: the ranks
    stay in step through the collectives of the later jobs."""
    os.environ.update(env)  # (before the library loads)
    import torch.distributed as dist
    from npge_amd import _capi
    from npge_amd.anchor_finder import AnchorFinder
    from npge_amd.comm import TorchComm
    from test_anchor_finder_gpu import _assert_same
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _capi.check(_capi.lib().npgx_set_device(0))
    comm = TorchComm(dist, staging="cpu")
    bad = []
    for c, epochs, oracle in jobs:
        ss = _capi.SeqSet(c["seqs"], c["names"])
        p = AnchorFinder(bloom_params=c["params"])
        for key, v in (("anchor-size", c["k"]), ("anchor-fp", c["fp"]), ("anchor-similar", c["similar"]),
                       ("max-anchor-fragments", c["maxf"]), ("bloom-seed", c["seed"]), ("bloom-epochs", epochs)):
            p.set_opt_value(key, v)
        for i, (clear, ro) in enumerate(zip(c["runs"], oracle)):
            if clear:
                p.clear_used()
            r = p.find_sharded(ss, comm)
            try:
                _assert_same(r, ro, p.used_hashes())
                assert p.stats.n_kept_groups == ro["kept_groups"], "n_kept_groups"
            except AssertionError as e:
                bad.append("%s run %d rank %d: %s" % (c["name"], i, rank, e))
    out[rank] = bad
    dist.barrier()
    dist.destroy_process_group()


def _run_cases(world, jobs, env=None):
    import af_cut_cases as cc
    jobs = [(c, epochs, cc.oracle_runs(c)) for c, epochs in jobs]  # the oracle once, here
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_cases_worker, args=(world, _free_port(), jobs, env or {}, out), nprocs=world, join=True)
    assert sorted(out.keys()) == list(range(world))
    assert [b for r in range(world) for b in out[r]] == []
    return jobs


@pytest.mark.parametrize("world", [2, 3])
def test_sharded_cut_cases(world):
    """The edges of the cut (af_cut_cases.py) on the sharded run, the only one
    that cuts by count, scan and scatter: every rank's result, used hashes and
    statistics are the oracle's.  BASE has 15 chunks at k = 12: two ranks split
    inside sequence 1 (the `similar` rule across ranks), three on sequence starts."""
    import af_cut_cases as cc
    by = {c["name"]: c for c in cc.CASES}
    jobs = _run_cases(world, [(by[n], 0) for n in cc.SHARDED])
    assert any(ro["n_found_frags"] > ro["maxf"] for _, _, runs in jobs for ro in runs)


@pytest.mark.parametrize("world", [3, 5])
def test_sharded_rank_without_windows(world):
    """Two chunks over three or five ranks: the ranks that own none still join
    every collective, and all ranks end with the oracle's result."""
    import af_cut_cases as cc
    _run_cases(world, [(c, 0) for c in cc.SHARD_EXTRA])


@pytest.mark.parametrize("fuse", ["1", "0"])
def test_sharded_epochs(fuse):
    """A sharded pass 1 in three epochs: the lower ranks' bits (P0) under every
    epoch, the range's first window reported by the first epoch alone and its
    last by the last, with the window masks (fp 0.1; fused launches or not) and
    without them (fp 0.01)."""
    import af_cut_cases as cc
    _run_cases(2, [(c, 3) for c in cc.EPOCH_CASES], env={"NPGX_AF_EPOCH_FUSE": fuse})


def _bb_worker(rank, world, port, config, out, loop=False):
    import torch.distributed as dist
    from npge_amd import _capi, synth
    from npge_amd.comm import TorchComm
    from npge_amd.pipeline import BlockBuild
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _capi.check(_capi.lib().npgx_set_device(0))
    names, seqs = synth.genome_set(config)
    ss = _capi.SeqSet(seqs, names)
    comm = TorchComm(dist, staging="cpu")
    job = BlockBuild(ss, names, seqs, comm=comm, anchor_loop=loop)
    info = job.run()
    st = job.eng.stats()
    got = (job.eng.hash(), job.eng.blocks(), info["align_jobs"], st["anchor_blocks"])
    ref = None
    if rank == 0:
        one = BlockBuild(ss, names, seqs, anchor_loop=loop)
        one.run()
        ref = (one.eng.hash(), one.eng.blocks(), one.eng.stats()["anchor_blocks"])
    out[rank] = (got, ref)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,config", [(2, "small"), (3, "tiny"), (2, "C4")])
def test_sharded_draft_pangenome_equals_single(world, config):
    """DraftPangenome with the AnchorFinder and every FragmentsExtender batch
    sharded: every rank's block set (fragments and gapped rows) equals one GPU's.
    C4 (32 x 5 Mbp at 2 %) has no anchor in every genome exactly once, so its
    DraftPangenome ends after RemoveNonStem --exact with no blocks: there the
    sharded AnchorFinder's block count is what is compared."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_bb_worker, args=(world, _free_port(), config, out), nprocs=world, join=True)
    ref_hash, ref_blocks, ref_anchors = out[0][1]
    assert ref_anchors > 0
    assert len(ref_blocks) > 0 or config == "C4"
    for r in range(world):
        (h, blocks, n_jobs, anchors) = out[r][0]
        assert n_jobs > 0 or config == "C4"
        assert anchors == ref_anchors, "rank %d" % r
        assert h == ref_hash, "rank %d" % r
        assert blocks == ref_blocks, "rank %d" % r


@pytest.mark.parametrize("world,config", [(2, "small"), (3, "tiny"), (2, "C4")])
def test_sharded_anchor_loop_equals_single(world, config):
    """DraftPangenome then AnchorLoopFast with a comm set: the consensus pipe's
    AnchorFinder runs sharded and its FragmentsExtender batches are split over
    the ranks (C4: whole-genome jobs); every rank ends with one GPU's blocks."""
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_bb_worker, args=(world, _free_port(), config, out, True), nprocs=world, join=True)
    ref_hash, ref_blocks, _ = out[0][1]
    assert len(ref_blocks) > 0
    for r in range(world):
        (h, blocks, _, _) = out[r][0]
        assert h == ref_hash, "rank %d" % r
        assert blocks == ref_blocks, "rank %d" % r
