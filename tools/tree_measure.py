#!/usr/bin/env python3
"""pair_distances, genome_distances and global_tree timed on one GPU over a
DraftPangenome output, beside the same penalties on one CPU thread (GPU box
diagnostic; measurements, not gates).

  tree_measure.py [CONFIG] [REPEATS]     (C3, 9)

Prints one JSON line.  Call times are host clocks around the computing call
(it ends in a device synchronise), after one warm-up call, the median of the
repeats; kernel times are HIP events on the engine's stream (NPGX_TIMERS=2:
every launch timed), the median too.  The CPU figure is the stand-alone host
program (npge_amd/csrc/tree_main.cpp, built here with build.py's flags) running
fragment_penalty over the rows downloaded from the engine, block after block
on one thread, the median of three runs a block; its penalties are compared
with the GPU's.
"""
import ctypes
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())
os.environ["NPGX_TIMERS"] = "2"


def _kernel(eng, name):
    ks = [k for k in eng.kernel_times() if k["name"] == name]
    return (sum(k["ms"] for k in ks), sum(k["bytes"] for k in ks), sum(int(k["units"]) for k in ks)) if ks else None


def _timed(eng, call, kernels, repeats):
    """call() computes (a size query); -> {wall_ms, kernels: {name: {ms, bytes, units, GBps}}}"""
    walls, ks = [], {k: [] for k in kernels}
    for rep in range(repeats + 1):  # the first is the warm-up
        t = time.perf_counter()
        call()
        w = (time.perf_counter() - t) * 1e3
        if rep == 0:
            continue
        walls.append(w)
        for k in kernels:
            ks[k].append(_kernel(eng, k))
    out = {"wall_ms": round(statistics.median(walls), 4), "wall_ms_min": round(min(walls), 4),
           "wall_ms_max": round(max(walls), 4), "kernels": {}}
    for k, v in ks.items():
        v = [x for x in v if x]
        if v:
            ms = statistics.median(x[0] for x in v)
            out["kernels"][k] = {"ms": round(ms, 5), "bytes": v[0][1], "units": v[0][2],
                                 "GBps": round(v[0][1] / ms / 1e6, 1) if ms > 0 else None}
    return out


def _cpu_pairs(blocks):
    """(penalties per block, total ms) from the stand-alone host program."""
    from npge_amd.build import CSRC, HOST_FLAGS
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "tree_main")
        subprocess.run(["g++", "-O2", "-std=c++17"] + HOST_FLAGS["tree.cpp"] +
                       ["-o", exe, os.path.join(CSRC, "tree.cpp"), os.path.join(CSRC, "tree_main.cpp")], check=True)
        inp = []
        for b in blocks:
            if len(b) >= 2:
                inp.append("pairs %d %d 3\n%s\n" % (len(b), len(b[0][4]), "\n".join(f[4] for f in b)))
        out = subprocess.run([exe], input="".join(inp), capture_output=True, text=True, check=True).stdout.split("\n")
    pens, ms, at = [], 0.0, 0
    for b in blocks:
        if len(b) < 2:
            pens.append([])
            continue
        pens.append([int(x) for x in out[at + 1].split()])
        ms += float(out[at + 2].split()[1])
        at += 3
    return pens, ms


def main(cfg="C3", repeats="9"):
    from npge_amd import _capi, synth
    from npge_amd.anchor_finder import AnchorFinder
    from npge_amd.blockset import BlockSetEngine, _bind
    repeats = int(repeats)
    names, seqs = synth.genome_set(cfg)
    eng = BlockSetEngine(_capi.SeqSet(seqs, names))
    eng.apply("DraftPangenome", af=AnchorFinder())
    L = _bind(_capi.lib())
    i64 = ctypes.c_int64
    nb, npairs, tb, nn, g = i64(), i64(), i64(), i64(), ctypes.c_int32()
    blocks = eng.blocks()
    rec = {"config": cfg, "bases": sum(len(s) for s in seqs), "blocks": len(blocks),
           "rows": sum(len(b) for b in blocks), "row_bytes": sum(len(f[4] or "") for b in blocks for f in b),
           "repeats": repeats, "hash": eng.hash()}
    rec["pair_distances"] = _timed(eng, lambda: _capi.check(L.npgx_blockset_pair_distances(
        eng._h, None, None, 0, ctypes.byref(nb), ctypes.byref(npairs))), ["pair_dist"], repeats)
    rec["pairs"] = npairs.value
    rec["genome_distances"] = _timed(eng, lambda: _capi.check(L.npgx_blockset_genome_distances(
        eng._h, None, 0, ctypes.byref(g), None)), ["pair_dist"], repeats)
    rec["global_tree"] = _timed(eng, lambda: _capi.check(L.npgx_blockset_global_tree(
        eng._h, b"", None, 0, ctypes.byref(tb), None, 0, ctypes.byref(nn))), ["pair_dist", "clade_diag"], repeats)
    rec["genomes"] = g.value
    rec["downloaded_bytes"] = {"pair_distances": 4 * npairs.value, "genome_distances": 8 * g.value * g.value}
    got = eng.pair_distances()
    pens, ms = _cpu_pairs(blocks)
    rec["cpu_one_thread"] = {"fragment_penalty_ms": round(ms, 3), "equal_to_gpu": pens == got}
    rec["text_bytes"] = tb.value
    rec["hash_after"] = eng.hash()
    print(json.dumps(rec))


if __name__ == "__main__":
    main(*sys.argv[1:])
