#!/usr/bin/env python3
"""TrySmth, SmthUnion's two row paths and k_letter_map timed on one GPU (GPU
box diagnostic; measurements, not gates).

  try_smth_measure.py try-smth CONFIG NAME [WARM]  TrySmth with the processor NAME on the DraftPangenome
                                            output: smth-rows 1 and 0, default timers and NPGX_TIMERS=2
                                            (WARM 1, the default: one warm-up run first)
  try_smth_measure.py try-smth-one CONFIG NAME ROWS TIMERS  one such run, no warm-up
  try_smth_measure.py letter-map [CONFIG]   k_letter_map alone over the DraftPangenome output's rows
  try_smth_measure.py anchor-loop [CONFIG]  one DraftPangenome + AnchorLoop, timed after a warm-up one
                                            (run it with NPGX_LIB=<other build> for an A/B)

Each prints one JSON line a run.  Wall times are host clocks around calls that end
in a device synchronise; kernel times are HIP events on the engine's stream
(NPGX_TIMERS=2: every launch timed).
"""
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.getcwd())


_SS = {}


def _engine(cfg):
    """A fresh engine holding the DraftPangenome output; (engine, bases)."""
    from npge_amd import _capi, synth
    from npge_amd.anchor_finder import AnchorFinder
    from npge_amd.blockset import BlockSetEngine
    if cfg not in _SS:
        names, seqs = synth.genome_set(cfg)
        _SS[cfg] = (_capi.SeqSet(seqs, names), sum(len(s) for s in seqs))
    eng = BlockSetEngine(_SS[cfg][0])
    eng.apply("DraftPangenome", af=AnchorFinder())
    return eng, _SS[cfg][1]


def _kernels(eng):
    out = {}
    for k in eng.kernel_times():
        e = out.setdefault(k["name"], {"launches": 0, "ms": 0.0, "bytes": 0.0})
        e["launches"] += 1
        e["ms"] += k["ms"]
        e["bytes"] += k["bytes"]
    return {n: {"launches": e["launches"], "ms": round(e["ms"], 4), "bytes": e["bytes"]} for n, e in out.items()}


def _with_stderr(fn):
    """fn() with the process's stderr (the engine's NPGX_AL_DEBUG lines) kept."""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            fn()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        return f.read().decode(errors="replace").strip().splitlines()


def try_smth_one(cfg, inner, rows, timers, warm_up):
    """One TrySmth on a fresh DraftPangenome output: a JSON record."""
    os.environ["NPGX_AL_DEBUG"] = "1"
    os.environ["NPGX_TIMERS"] = timers
    for rep in range(2 if warm_up else 1):
        eng, bases = _engine(cfg)
        eng.tune("smth-rows", rows)
        n_in = len(eng.fragments()[0]) - 1
        t = time.perf_counter()
        lines = _with_stderr(lambda: eng.apply("TrySmth --smth-processor:=" + inner))
        wall = (time.perf_counter() - t) * 1e3
    st = eng.stats()
    return {"config": cfg, "bases": bases, "blocks_in": n_in, "processor": inner, "smth_rows": rows,
            "timers": int(timers), "warm_up_runs": int(warm_up), "wall_ms": round(wall, 3),
            "counts": eng.try_smth_counts(), "adding_loop": lines, "ms_align": round(st["ms_align"], 3),
            "align_jobs": st["align_jobs"], "aligned_residues": st["aligned_residues"],
            "hash": eng.hash(), "rows_digest": eng.rows_digest(), "kernels": _kernels(eng)}


def try_smth(cfg, inner="FragmentsExtender", warm="1"):
    """Both row paths, default timers and NPGX_TIMERS=2: one JSON line a run."""
    for rows in (1, 0):
        for timers in ("1", "2"):
            print(json.dumps(try_smth_one(cfg, inner, rows, timers, warm == "1" and rows == 1 and timers == "1")),
                  flush=True)


def try_smth_single(cfg, inner, rows, timers):
    print(json.dumps(try_smth_one(cfg, inner, int(rows), timers, False)), flush=True)


def letter_map(cfg):
    """k_letter_map alone: one launch over every row of the DraftPangenome output."""
    os.environ["NPGX_TIMERS"] = "2"
    eng, _ = _engine(cfg)
    best = None
    for _ in range(4):  # the first is the warm-up
        t = time.perf_counter()
        maps = eng.letter_map()
        wall = (time.perf_counter() - t) * 1e3
        k = [x for x in eng.kernel_times() if x["name"] == "letter_map"][0]
        if best is None or k["ms"] < best["kernel_ms"]:
            best = {"kernel_ms": round(k["ms"], 4), "cells": int(k["units"]), "bytes": k["bytes"],
                    "GBps": round(k["bytes"] / k["ms"] / 1e6, 1), "rows": len(maps), "entry_wall_ms": round(wall, 1)}
    print(json.dumps(dict(best, config=cfg)))


def anchor_loop(cfg):
    from npge_amd.anchor_finder import AnchorFinder
    rec = {"config": cfg, "lib": os.environ.get("NPGX_LIB", "")}
    for rep in ("warm-up", "timed"):
        eng, _ = _engine(cfg)
        t = time.perf_counter()
        eng.apply("AnchorLoop", af=AnchorFinder())
        rec["wall_ms"] = round((time.perf_counter() - t) * 1e3, 2)
    rec["hash"], rec["rows_digest"] = eng.hash(), eng.rows_digest()
    rec["blocks"] = len(eng.fragments()[0]) - 1
    rec["rounds"] = eng.stats()["counters"]["spare"]
    print(json.dumps(rec))


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "try-smth"
    {"try-smth": try_smth, "try-smth-one": try_smth_single, "letter-map": letter_map, "anchor-loop": anchor_loop}[mode](*(sys.argv[2:] or ["C3"]))
