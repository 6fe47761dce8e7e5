"""bench.py --dump-outputs and the plain (no --full) line.

CPU: the dump's canonical order on a stand-in engine -- the same block set
listed in another block and fragment order gives identical files, float32 /
float64 only, checked against a plain-Python restatement; the seeded sample of
an output over the caps.  GPU: one plain run of the small config writes the
block set its last timed step made and prints a line without the --full
measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("stage_timeline", "pcie_inclusive", "cpu_baseline", "sharded", "replicas", "pairs")


def _arrays(blocks):
    """bench.blockset_arrays()'s form of a list of blocks of (seq, min, max,
    ori, row or None)."""
    frs = [f for b in blocks for f in b]
    bs = np.zeros(len(blocks) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in blocks], out=bs[1:])
    ro = np.zeros(len(frs) + 1, dtype=np.int64)
    np.cumsum([len(f[4] or "") for f in frs], out=ro[1:])
    rows = np.frombuffer("".join(f[4] or "" for f in frs).encode(), dtype=np.uint8)
    col = lambda i, t: np.array([f[i] for f in frs], dtype=t)
    return bs, col(0, np.int32), col(1, np.int64), col(2, np.int64), col(3, np.int8), ro, rows


def _dump(path, blocks):
    bench.dump_blockset(str(path), _arrays(blocks), 0xFEDCBA9876543210, 0x0123456789ABCDEF)


def _canonical(blocks):
    """Plain-Python restatement of the dump's order: fragments sorted inside
    their block, blocks by (first fragment, size, last fragment)."""
    return sorted((tuple(sorted((q, m, x, o, r or "") for q, m, x, o, r in bl)) for bl in blocks),
                  key=lambda bl: (bl[0][:4], len(bl), bl[-1][:4]))


def _blocks(seed=1, n=60):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(n):
        L = int(rng.integers(1, 30))
        blk = []
        for _ in range(int(rng.integers(1, 5))):
            mn = int(rng.integers(0, 100000))
            row = "".join(rng.choice(list("ATGC-"), L)) if b % 7 else None
            blk.append((int(rng.integers(0, 6)), mn, mn + L - 1, int(rng.choice([-1, 1])), row))
        out.append(blk)
    return out


def _shuffled(blocks, seed=2):
    rng = np.random.default_rng(seed)
    return [list(reversed(blocks[i])) for i in rng.permutation(len(blocks))]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d)) if f.endswith(".npy")}


def _assert_dump_is(a, blocks):
    """The (unsampled) dump `a` holds exactly `blocks`."""
    canon = _canonical(blocks)
    flat = [f for bl in canon for f in bl]
    assert a["counts"].tolist() == [len(blocks), len(flat), sum(len(f[4]) for f in flat)]
    assert a["frag_block"].tolist() == [i for i, bl in enumerate(canon) for _ in bl]
    for i, k in enumerate(("frag_seq", "frag_min", "frag_max", "frag_ori")):
        assert a[k].tolist() == [f[i] for f in flat], k
    assert a["frag_row_length"].tolist() == [len(f[4]) for f in flat]
    assert bytes(a["rows"].astype(np.uint8)).decode() == "".join(f[4] for f in flat)


def test_dump_is_order_free_and_exact(tmp_path):
    blocks = _blocks()
    _dump(tmp_path / "a", blocks)
    _dump(tmp_path / "b", _shuffled(blocks))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(b) and len(a) == 10
    for k in a:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
    _assert_dump_is(a, blocks)
    assert a["blockset_hash"].tolist() == [0xFEDCBA98, 0x76543210]
    assert a["rows_digest"].tolist() == [0x01234567, 0x89ABCDEF]


def test_dump_sample_is_fixed(tmp_path, monkeypatch):
    """Over the caps: a sample of the canonical arrays, the same from run to run
    and for either listing order."""
    monkeypatch.setattr(bench, "DUMP_FRAGMENTS", 20)
    monkeypatch.setattr(bench, "DUMP_ROW_CELLS", 100)
    blocks = _blocks()
    _dump(tmp_path / "a", blocks)
    _dump(tmp_path / "b", _shuffled(blocks))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert len(a["frag_seq"]) == 20 and len(a["rows"]) == 100
    assert np.all(np.diff(a["frag_block"]) >= 0)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_dump_empty_blockset(tmp_path):
    _dump(tmp_path, [])
    a = _load(tmp_path)
    assert a["counts"].tolist() == [0, 0, 0] and len(a["rows"]) == 0 and len(a["frag_seq"]) == 0


def test_dump_pairs_records(tmp_path):
    from npge_amd import pairs
    blocks = _blocks()
    recs, sums, want = [], [], []
    for p in (3, 1, 700000):  # (a pair number with the top bit of its field set)
        bl = blocks[p % 5:p % 5 + 10]
        recs.append(pairs.pack_fragments(p, *_arrays(_shuffled(bl, p))[:5]))
        sums.append(np.array([(p << 32) | len(bl), 0xF000000000000001 + p, 77 + p], dtype=np.uint64))
        want.append((p, bl))
    bench.dump_pairs(str(tmp_path), np.concatenate(recs), np.concatenate(sums))
    a = _load(tmp_path)
    assert all(v.dtype == np.float64 for v in a.values())
    assert a["pair_summary"].tolist() == [[p, 10, 0xF0000000, 1 + p, 0, 77 + p] for p in (1, 3, 700000)]
    flat, nb = [], 0
    for p, bl in sorted(want):
        canon = sorted((tuple(sorted(f[:4] for f in b)) for b in bl), key=lambda b: (b[0], len(b), b[-1]))
        flat += [(p, nb + i) + f for i, b in enumerate(canon) for f in b]
        nb += len(canon)
    for i, k in enumerate(("frag_pair", "frag_block", "frag_seq", "frag_min", "frag_max", "frag_ori")):
        assert a[k].tolist() == [f[i] for f in flat], k
    assert a["counts"].tolist() == [3, len(flat)]


@pytest.mark.gpu
def test_plain_run_dumps_its_last_step(tmp_path):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--config", "small",
           "--dump-outputs", str(tmp_path)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "last_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    assert not [k for k in FULL_ONLY if k in d]
    a = _load(tmp_path)
    for k, v in a.items():
        assert v.dtype in (np.float32, np.float64) and np.all(np.isfinite(v)), k
    assert sum(v.nbytes for v in a.values()) <= 64 * 2**20
    nb, nf, cells = (int(x) for x in a["counts"])
    assert nb > 0 and nf >= nb and len(a["frag_seq"]) == nf and len(a["rows"]) == cells
    assert a["frag_block"][0] == 0 and a["frag_block"][-1] == nb - 1
    assert int(a["frag_row_length"].sum()) == cells
    # every row of a block has the block's length, and holds its fragment's residues
    first = np.flatnonzero(np.r_[True, np.diff(a["frag_block"]) > 0])
    assert np.array_equal(a["frag_row_length"], np.repeat(a["frag_row_length"][first], np.diff(np.r_[first, nf])))
    assert set(np.unique(a["rows"]).astype(np.uint8).tobytes().decode()) <= set("ATGCN-")
    start = np.r_[0, np.cumsum(a["frag_row_length"])].astype(np.int64)
    filled = np.r_[0, np.cumsum(a["rows"] != ord("-"))]
    has = a["frag_row_length"] > 0
    assert has.any()
    assert np.array_equal((filled[start[1:]] - filled[start[:-1]])[has], (a["frag_max"] - a["frag_min"] + 1)[has])
    # the dump is the step the line reports: its block count, and block for
    # block the oracle's DraftPangenome on the same seeded set
    assert nb == d["last_step"]["counters"]["blocks_after_filter"]
    from npge_amd import harness, synth
    from oracle import oracle as orc
    names, seqs = synth.genome_set("small", seed=harness.rank_seed(synth.BASE_SEED, 0, "small"))
    assert d["config"]["bp_per_rank"] == synth.total_bp(seqs)
    o = orc.BlockSetOracle(seqs, names, seed=1)
    o.apply("DraftPangenome")
    _assert_dump_is(a, o.blocks())
