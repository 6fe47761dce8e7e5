#!/usr/bin/env python3
"""The chunked refine_alignment and the JoinerP pipes timed on one GPU (GPU box
diagnostic; measurements, not gates).

  refine_chunks_measure.py sweep CONFIG [NAME]       TrySmth with the processor NAME (Joiner) on the DraftPangenome
                                                     output, "refine-chunk" 256..4096 with "refine-min-len" 4 x chunk
  refine_chunks_measure.py one CONFIG NAME CHUNK MIN  one such run (CHUNK -1: the library's defaults; 0: chunks off)
  refine_chunks_measure.py realign CONFIG [CHUNK MIN] ReAlign on the DraftPangenome output, three runs after a warm-up
                                                     (run it with NPGX_LIB=<other build> for an A/B)
  refine_chunks_measure.py merge-unique CONFIG       MergeUnique alone after Rest: its host time, two runs after a warm-up

Each prints one JSON line a run.  Wall times are host clocks around calls that
end in a device synchronise; kernel times are HIP events on the engine's
stream (NPGX_TIMERS=2: every launch timed).
"""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())

_SS = {}


def _engine(cfg, chunk, min_len):
    from npge_amd import _capi, synth
    from npge_amd.anchor_finder import AnchorFinder
    from npge_amd.blockset import BlockSetEngine
    if cfg not in _SS:
        names, seqs = synth.genome_set(cfg)
        _SS[cfg] = _capi.SeqSet(seqs, names)
    eng = BlockSetEngine(_SS[cfg])
    if chunk >= 0:
        eng.tune("refine-chunk", chunk).tune("refine-min-len", min_len)
    eng.apply("DraftPangenome", af=AnchorFinder())
    return eng


def _kernels(eng):
    out = {}
    for k in eng.kernel_times():
        e = out.setdefault(k["name"], {"launches": 0, "ms": 0.0, "bytes": 0.0})
        e["launches"] += 1
        e["ms"] += k["ms"]
        e["bytes"] += k["bytes"]
    return {n: {"launches": e["launches"], "ms": round(e["ms"], 4), "bytes": e["bytes"]} for n, e in out.items()}


def one(cfg, inner, chunk, min_len, timers="2"):
    os.environ["NPGX_TIMERS"] = timers
    chunk, min_len = int(chunk), int(min_len)
    eng = _engine(cfg, chunk, min_len)
    n_in = len(eng.fragments()[0]) - 1
    t = time.perf_counter()
    eng.apply("TrySmth --smth-processor:=" + inner)
    wall = (time.perf_counter() - t) * 1e3
    rec = {"config": cfg, "processor": inner, "refine_chunk": chunk, "refine_min_len": min_len, "timers": int(timers),
           "blocks_in": n_in, "wall_ms": round(wall, 3), "refine": eng.refine_counts(),
           "try_smth": eng.try_smth_counts(), "hash": eng.hash(), "rows_digest": eng.rows_digest(),
           "kernels": _kernels(eng)}
    if inner in ("JoinerP", "MergeAndJoin", "MergeUnique"):
        rec["merge_unique"] = eng.merge_unique_counts()
    print(json.dumps(rec), flush=True)


def sweep(cfg, inner="Joiner"):
    for chunk in (256, 512, 1024, 2048, 4096):
        one(cfg, inner, chunk, 4 * chunk)


def realign(cfg, chunk="-1", min_len="-1"):
    os.environ["NPGX_TIMERS"] = "2"
    for rep in range(4):  # the first is the warm-up
        eng = _engine(cfg, int(chunk), int(min_len))
        t = time.perf_counter()
        eng.apply("ReAlign")
        wall = (time.perf_counter() - t) * 1e3
        if rep:
            k = _kernels(eng)
            print(json.dumps({"config": cfg, "lib": os.environ.get("NPGX_LIB", ""), "wall_ms": round(wall, 3),
                              "kernel_ms": round(sum(e["ms"] for e in k.values()), 4), "refine": eng.refine_counts()
                              if hasattr(eng, "refine_counts") and not os.environ.get("NPGX_LIB") else None,
                              "realign": eng.realign_counts(), "rows_digest": eng.rows_digest()}), flush=True)


def merge_unique(cfg):
    """MergeUnique alone (host work) on the DraftPangenome output after Rest."""
    for rep in range(3):  # the first is the warm-up
        eng = _engine(cfg, -1, -1).apply("Rest")
        n_in = len(eng.fragments()[0]) - 1
        t = time.perf_counter()
        eng.apply("MergeUnique")
        wall = (time.perf_counter() - t) * 1e3
        if rep:
            print(json.dumps({"config": cfg, "blocks_in": n_in, "blocks_out": len(eng.fragments()[0]) - 1,
                              "wall_ms": round(wall, 3), "merge_unique": eng.merge_unique_counts()}), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "sweep"
    {"sweep": sweep, "one": one, "realign": realign, "merge-unique": merge_unique}[mode](*(sys.argv[2:] or ["C3"]))
