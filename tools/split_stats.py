#!/usr/bin/env python3
"""Diagnostic (GPU box): one DraftPangenome with NPGX_SPLIT_DEBUG=1 -- per split
aligner job, the sync states found, the segments that reached one, overflows
and the chain of segments (stderr).

--critical-path [CONFIG]: the same run in a child process, and of its stderr
only the late iterations' critical path: for each of the last four aligner
batches with deferred sub-jobs, per job with sub-jobs when its own walk or its
last segment ended in k_align_jobs and when its sub-jobs started and ended in
k_align_sub (microseconds from the batch's first task; the sub-jobs exist once
the job's chain and regions are known, so their earliest possible start is
the job's own end plus its k_chain_copy / k_split_post), and which job ends
either launch."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

if len(sys.argv) > 1 and sys.argv[1] == "--critical-path":
    cfg = sys.argv[2] if len(sys.argv) > 2 else "C3"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), cfg], stderr=subprocess.PIPE,
                       stdout=subprocess.DEVNULL, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stderr[-2000:])
        sys.exit(p.returncode)
    batches, cur = [], []
    for line in p.stderr.splitlines():
        if line.startswith(("launch:", "sub launch:", "crit job")):
            cur.append(line)
        elif line.startswith("crit launches:"):
            cur.append(line)
            batches.append(cur)
            cur = []
        elif line.startswith("split job") and cur and not cur[-1].startswith("launch:"):
            cur = []  # (a batch without deferred sub-jobs)
    print("%s: %d aligner batches with deferred sub-jobs; the last four:" % (cfg, len(batches)))
    for i, b in enumerate(batches[-4:]):
        print("-- batch %d" % (len(batches) - len(batches[-4:]) + i + 1))
        for line in b:
            print("  " + line)
    sys.exit(0)

sys.path.insert(0, ROOT)
os.environ["NPGX_SPLIT_DEBUG"] = "1"
os.environ["NPGX_JOB_STATS"] = "1"
from npge_amd import _capi, synth  # noqa: E402
from npge_amd.anchor_finder import AnchorFinder  # noqa: E402
from npge_amd.blockset import BlockSetEngine  # noqa: E402

cfg = sys.argv[1] if len(sys.argv) > 1 else "C3"
_capi.check(_capi.lib().npgx_set_device(0))
names, seqs = synth.genome_set(cfg)
ss = _capi.SeqSet(seqs, names)
eng = BlockSetEngine(ss)
eng.apply("DraftPangenome", af=AnchorFinder())

# the longest jobs of the last batch: wall time from the first segment's start,
# and the finishing wave's phases (clock64 cycles at ~2.4 GHz)
os.environ.pop("NPGX_SPLIT_DEBUG", None)
js = eng.job_stats()
if len(js):
    import numpy as np
    o = np.argsort(-js[:, 1])[:8]
    print("cols rows wall_us fin_us ph0_us(chain) ph1_us(regions+realign) ph2_us(realing_end) regions_us nreg")
    for j in o:
        r = js[j]
        print("%6d %3d %8.1f %8.1f %8.1f %8.1f %8.1f %8.1f %d" % (
            r[1], r[6], (r[23] - r[11]) / 100.0, r[0] / 2400.0, r[8] / 2400.0, r[9] / 2400.0, r[10] / 2400.0,
            r[22] / 2400.0, r[5]))
