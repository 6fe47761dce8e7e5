"""Block-set processors on the engine (npgx_blockset_*).

Mirrors the reference's BlockSet + per-block processors of the block build:
RemoveNonStem, DummyAligner, MetaAligner, FragmentsExtender, FixEnds,
OverlaplessUnion, ExtendLoopFast, Filter, MoveGaps, CutGaps,
SelfOverlapsResolver, the Align / LiteAlign pipes (Align.cpp:17-52), Rest,
Joiner (Joiner.cpp:27-262), OriByMajority (OriByMajority.cpp:25-61),
ReAlign (ReAlign.cpp:23-78), TrySmth (TrySmth.cpp:184-199), AnchorLoopFast and
the DraftPangenome driver (lua_lib.lua:1569-1621).
Alignment work goes to the HIP aligner in one batch per processor pass.

ReAlign aligns every block that has all its rows again from its fragments'
texts (one decode launch, one aligner batch, one k_refine launch), takes
Block::identity of the old and the new rows from one k_col_stat launch and
keeps the new rows where the identity grew and Filter does not object
(apply("ReAlign"), apply("ReAlign --force-realign=1"); realign_counts()).
block_stats() gives the same statistics (AlignmentStat) per block.

Joiner plans every chain of collinear neighbouring blocks on the host, aligns
all between-fragments in one batch and writes the joined rows with one
k_join_rows launch; a joined block stands where its chain's head stood.  It
raises NpgxError (NPGX_ERR_ARG) and leaves the set unchanged when the facing
fragments of a pair it would join overlap.

TrySmth (apply("TrySmth --smth-processor:=NAME [NAME's options]")) copies the
set, runs NAME, ReAlign and Align on it, and lets AddingLoopBySize merge the
copy and the new blocks: the larger version of every block wins, a named
original wins a tie, what overlaps the winners is cut into pieces.  A failing
step gives the set back as it came.  try_smth_counts() has the last run's
counts, block_names() the names UniqueNames gave.  SmthUnion reads the rows of
the blocks it cuts through their letter maps (k_letter_map: one bit a cell,
one prefix count a word; tune("smth-rows", 0) for the host copy of the rows);
letter_map() returns the maps of the set's rows, smth_counts() the bytes both
paths downloaded.

LiteFilter (apply("LiteFilter --min-fragment=N --min-block=K")) drops small
blocks; MergeUnique (apply("MergeUnique --both-neighbours=0 --merge-long=1"),
merge_unique_counts()) merges unique fragments with common neighbours into
blocks named "m<size>x<length>"; JoinerP, MergeAndJoin and LiteJoinerP are the
reference's pipes over them, Rest, OriByMajority, MetaAligner and Joiner
(lua_lib.lua:641-668), each one apply and each accepted by TrySmth.

Trees and fragment distances change no block: pair_distances()
(FragmentDistance, k_pair_dist), genome_distances() (GlobalTree's add_dist over
the stem blocks, summed on the device), global_tree() (neighbour joining on
the host, the bootstraps from k_clade_diag's diagnostic columns) and
block_trees() (PrintTree); apply("FragmentDistance"), apply("PrintTree
--tree-method=upgma") and apply("GlobalTree --bootstrap-print=no") keep their
result for those calls and are refused inside TrySmth.

refine_alignment takes a block of at least "refine-min-len" columns in
independent chunks (tune("refine-chunk", N); k_refine_cuts finds the cuts, the
chunks are k_refine jobs, k_join_rows gathers them), bit-identical to one wave
per block; refine_counts() has the last apply's jobs, long jobs and chunks.
"""
import ctypes

import numpy as np

from . import _capi


class BbOptions(ctypes.Structure):
    _fields_ = [("extend_length", ctypes.c_int32), ("max_iterations", ctypes.c_int32),
                ("extend_portion_x1e4", ctypes.c_int64), ("min_fragment", ctypes.c_int32),
                ("frame_length", ctypes.c_int32), ("min_end", ctypes.c_int32),
                ("min_block", ctypes.c_int32), ("max_block", ctypes.c_int32),
                ("find_subblocks", ctypes.c_int32), ("min_identity_x1e4", ctypes.c_int64),
                ("align", _capi.AlignOptions), ("max_tail", ctypes.c_int32),
                ("max_tail_to_gap_x1e4", ctypes.c_int64)]


class BbStats(ctypes.Structure):
    _fields_ = [("iterations", ctypes.c_int64), ("aligned_residues", ctypes.c_int64),
                ("align_jobs", ctypes.c_int64), ("anchor_blocks", ctypes.c_int64),
                ("stem_blocks", ctypes.c_int64), ("ms_align", ctypes.c_double),
                ("ms_host", ctypes.c_double), ("ms_stage", ctypes.c_double * 16),
                ("counters", ctypes.c_int64 * 8), ("loop", ctypes.c_int64 * 8),
                ("ms_loop", ctypes.c_double * 8), ("ms_gpu", ctypes.c_double * 12),
                ("device_iterations", ctypes.c_int64), ("device_sync_iterations", ctypes.c_int64)]


class BlockStat(ctypes.Structure):
    """npgx_block_stat (include/npge_amd.h)."""
    _fields_ = [("ident_nogap", ctypes.c_int32), ("ident_gap", ctypes.c_int32),
                ("noident_nogap", ctypes.c_int32), ("noident_gap", ctypes.c_int32),
                ("pure_gap", ctypes.c_int32), ("total", ctypes.c_int32),
                ("alignment_rows", ctypes.c_int32), ("min_fragment_length", ctypes.c_int32),
                ("letters", ctypes.c_int64 * 5), ("identity_x1e4", ctypes.c_int64)]


class TreeNode(ctypes.Structure):
    """npgx_tree_node (include/npge_amd.h)."""
    _fields_ = [("parent", ctypes.c_int32), ("leaf", ctypes.c_int32), ("length", ctypes.c_double),
                ("bootstrap", ctypes.c_double)]


TRY_SMTH_COUNT_NAMES = ["blocks_in", "blocks_tried", "rounds", "blocks_cut", "pieces", "blocks_out",
                        "map_bytes", "row_bytes"]
SMTH_COUNT_NAMES = ["map_bytes", "row_bytes", "blocks_cut", "pieces"]
MERGE_UNIQUE_COUNT_NAMES = ["blocks_inspected", "merges", "fragments_merged"]
REFINE_COUNT_NAMES = ["jobs", "long_jobs", "chunks", "longest_chunk", "columns_in", "columns_out"]
REALIGN_COUNT_NAMES = ["candidates", "replaced", "filter_refused", "not_better"]
# STAGE_NAMES, GPU_STAGE_NAMES and COUNTER_NAMES name npgx_bb_stats' ms_stage, ms_gpu and counters by
# position: the enums Stage, GpuStage and Counter in csrc/common.hpp are the same lists in the same order,
# and must follow any change here
STAGE_NAMES = ["anchor_finder", "stem_dummy", "move_unchanged", "flank_gather", "align_batch",
               "stitch", "fix_ends", "overlapless_union", "blockset_hash", "filter",
               "align_host_prep", "device_wait", "fix_ends_device", "fix_ends_slice",
               "ou_order", "ou_admit"]
# npgx_bb_stats.ms_gpu: DraftPangenome's GPU timeline by stage ("stage-clock" tuning)
GPU_STAGE_NAMES = ["anchor_finder", "stem_dummy", "elf_upload", "elf_plan", "flank_decode", "align", "stitch",
                   "fix_ends", "overlapless_union", "elf_download", "filter", "extend_loop_host"]
JOB_STATS = 32  # NPGX_JOB_STATS
COUNTER_NAMES = ["blocks_after_extend", "filter_whole", "filter_slices", "blocks_after_filter",
                 "ou_in", "ou_rejected", "hashes", "spare"]
# AnchorLoop's npgx_bb_stats.loop (the oracle's orc_bs_anchor_loop_stats, same order)
ANCHOR_LOOP_NAMES = ["cons_seqs", "cons_anchors", "anchors_left", "split_blocks", "cons_blocks", "dec_blocks",
                     "cons_iterations", "dec_iterations"]
LOOP_NAMES = ["consensus_sequences", "anchors", "cons_blocks", "mapped_blocks", "loop_iterations",
              "unchanged_dropped"]
LOOP_STAGE_NAMES = ["filter_rest", "conseq", "anchor_finder", "move_unchanged_dummy", "extend_and_align",
                    "extend_loop_fast", "deconseq", "align"]


def _bind(L):
    if getattr(L, "_bb_bound", False):
        return L
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    P = ctypes.POINTER
    L.npgx_bb_default_options.argtypes = [P(BbOptions)]
    L.npgx_bb_default_options.restype = None
    L.npgx_blockset_create.argtypes = [vp, P(BbOptions), P(vp)]
    L.npgx_blockset_create_sharing.argtypes = [vp, P(BbOptions), vp, P(vp)]
    L.npgx_blockset_set_blocks.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp]
    L.npgx_blockset_add_anchors.argtypes = [vp, vp]
    L.npgx_blockset_set_comm.argtypes = [vp, vp]
    L.npgx_blockset_apply.argtypes = [vp, ctypes.c_char_p, vp]
    L.npgx_blockset_counts.argtypes = [vp, P(i64), P(i64), P(i64)]
    L.npgx_blockset_copy.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    L.npgx_blockset_hash.argtypes = [vp, P(ctypes.c_uint64)]
    L.npgx_blockset_rows_digest.argtypes = [vp, P(ctypes.c_uint64)]
    if hasattr(L, "npgx_blockset_block_stats"):  # (NPGX_LIB may name an older build)
        L.npgx_blockset_block_stats.argtypes = [vp, P(BlockStat), i64, P(i64)]
        L.npgx_blockset_realign_counts.argtypes = [vp, P(i64 * 4)]
    if hasattr(L, "npgx_blockset_try_smth_counts"):  # (as above)
        L.npgx_blockset_try_smth_counts.argtypes = [vp, P(i64 * 8)]
        L.npgx_blockset_smth_counts.argtypes = [vp, P(i64 * 4)]
        L.npgx_blockset_block_names.argtypes = [vp, vp, i64, P(i64)]
        L.npgx_blockset_letter_map.argtypes = [vp, vp, vp, i64, P(i64)]
    if hasattr(L, "npgx_blockset_refine_counts"):  # (as above)
        L.npgx_blockset_refine_counts.argtypes = [vp, P(i64 * 6)]
        L.npgx_blockset_merge_unique_counts.argtypes = [vp, P(i64 * 3)]
    if hasattr(L, "npgx_blockset_pair_distances"):  # (as above)
        L.npgx_blockset_pair_distances.argtypes = [vp, vp, vp, i64, P(i64), P(i64)]
        L.npgx_blockset_genome_distances.argtypes = [vp, vp, i64, P(ctypes.c_int32), P(i64)]
        L.npgx_blockset_global_tree.argtypes = [vp, ctypes.c_char_p, vp, i64, P(i64), P(TreeNode), i64, P(i64)]
        L.npgx_blockset_block_trees.argtypes = [vp, ctypes.c_char_p, vp, i64, P(i64), vp, vp, P(TreeNode), i64,
                                                P(i64), P(i64)]
        L.npgx_pair_dist_tile_columns.argtypes = [i64]
        L.npgx_pair_dist_tile_columns.restype = ctypes.c_int32
    L.npgx_blockset_conseq.argtypes = [vp, vp, vp, P(i64), P(i64)]
    L.npgx_blockset_deconseq.argtypes = [vp, vp, vp]
    L.npgx_blockset_stats.argtypes = [vp, P(BbStats)]
    L.npgx_blockset_kernel_times.argtypes = [vp, P(_capi.KernelTime), ctypes.c_int32,
                                             P(ctypes.c_int32)]
    L.npgx_blockset_job_stats.argtypes = [vp, vp, i64, P(i64)]
    L.npgx_blockset_reset_loop.argtypes = [vp]
    L.npgx_blockset_free.argtypes = [vp]
    L.npgx_blockset_free.restype = None
    L._bb_bound = True
    return L


ALIGN_KEYS = ("mismatch_check", "gap_check", "aligned_check", "align_min_length",
              "align_min_identity_x1e4")


def pair_dist_tile_columns(rows):
    """The columns of one k_pair_dist tile for a block of `rows` rows."""
    return int(_bind(_capi.lib()).npgx_pair_dist_tile_columns(int(rows)))


def default_options(**kw):
    L = _bind(_capi.lib())
    o = BbOptions()
    L.npgx_bb_default_options(ctypes.byref(o))
    for k, v in kw.items():
        if k in ALIGN_KEYS:
            setattr(o.align, k.replace("align_", ""), v)
        else:
            setattr(o, k, v)
    return o


class BlockSetEngine:
    """One npgx_blockset over a device sequence set."""

    def __init__(self, seqset, options=None, lender=None, **kw):
        """lender: another engine whose aligner this one borrows
        (npgx_blockset_create_sharing): never run the two at the same time."""
        L = _bind(_capi.lib())
        self.ss = seqset
        o = options or default_options(**kw)
        h = ctypes.c_void_p()
        if lender is None:
            _capi.check(L.npgx_blockset_create(seqset.handle, ctypes.byref(o), ctypes.byref(h)))
        else:
            _capi.check(L.npgx_blockset_create_sharing(seqset.handle, ctypes.byref(o), lender._h,
                                                       ctypes.byref(h)))
        self._lender = lender  # freed after this engine
        self._h = h

    def set_comm(self, comm):
        """Shards DraftPangenome / FragmentsExtender over comm's ranks
        (npge_amd.comm.TorchComm); None returns to one GPU."""
        self._comm = comm  # the library keeps a pointer to comm.struct
        _capi.check(_capi.lib().npgx_blockset_set_comm(self._h, comm.pointer() if comm else None))
        return self

    def set_blocks(self, blocks):
        """blocks: list of lists of (seq_index, min, max, ori, row_or_None)."""
        L = _capi.lib()
        frs = [f for b in blocks for f in b]
        bs = np.zeros(len(blocks) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in blocks], out=bs[1:])
        seq = np.array([f[0] for f in frs] or [0], dtype=np.int32)
        mn = np.array([f[1] for f in frs] or [0], dtype=np.int64)
        mx = np.array([f[2] for f in frs] or [0], dtype=np.int64)
        ori = np.array([f[3] for f in frs] or [1], dtype=np.int8)
        has_rows = any(f[4] is not None for f in frs)
        if has_rows:  # per block: rows for every fragment, or none (zero-length rows)
            rows = "".join(f[4] or "" for f in frs).encode()
            ro = np.zeros(len(frs) + 1, dtype=np.int64)
            np.cumsum([len(f[4] or "") for f in frs], out=ro[1:])
            buf = ctypes.create_string_buffer(rows, max(len(rows), 1))
            _capi.check(L.npgx_blockset_set_blocks(self._h, len(blocks), _capi.ptr(bs), _capi.ptr(seq),
                                                   _capi.ptr(mn), _capi.ptr(mx), _capi.ptr(ori),
                                                   _capi.ptr(ro), ctypes.cast(buf, ctypes.c_void_p)))
        else:
            _capi.check(L.npgx_blockset_set_blocks(self._h, len(blocks), _capi.ptr(bs), _capi.ptr(seq),
                                                   _capi.ptr(mn), _capi.ptr(mx), _capi.ptr(ori),
                                                   None, None))
        return self

    def apply(self, processor, af=None):
        L = _capi.lib()
        afh = af._handle() if af is not None else None
        if af is not None:
            af._last_set = self.ss  # (its deferred statistics read the set again)
        _capi.check(L.npgx_blockset_apply(self._h, processor.encode(), afh))
        return self

    def reset_loop(self):
        """Forget AnchorLoopFast's MoveUnchanged hashes (a fresh pipe)."""
        _capi.check(_capi.lib().npgx_blockset_reset_loop(self._h))
        return self

    def blocks(self):
        L = _capi.lib()
        nb, nf, rb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _capi.check(L.npgx_blockset_counts(self._h, ctypes.byref(nb), ctypes.byref(nf), ctypes.byref(rb)))
        n = max(nf.value, 1)
        bs = np.zeros(nb.value + 1, dtype=np.int64)
        seq = np.zeros(n, dtype=np.int32)
        mn = np.zeros(n, dtype=np.int64)
        mx = np.zeros(n, dtype=np.int64)
        ori = np.zeros(n, dtype=np.int8)
        ro = np.zeros(n + 1, dtype=np.int64)
        rows = ctypes.create_string_buffer(max(rb.value, 1))
        _capi.check(L.npgx_blockset_copy(self._h, _capi.ptr(bs), _capi.ptr(seq), _capi.ptr(mn),
                                         _capi.ptr(mx), _capi.ptr(ori), _capi.ptr(ro),
                                         ctypes.cast(rows, ctypes.c_void_p)))
        raw = rows.raw
        out = []
        for b in range(nb.value):
            blk = []
            for i in range(bs[b], bs[b + 1]):
                row = raw[ro[i]:ro[i + 1]].decode() if ro[i + 1] > ro[i] else None
                blk.append((int(seq[i]), int(mn[i]), int(mx[i]), int(ori[i]), row))
            out.append(blk)
        return out

    def fragments(self):
        """Fragment coordinates without rows (no row download): numpy arrays
        (block_start[nb + 1], seq, min, max, ori) in block order."""
        L = _capi.lib()
        nb, nf, rb = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _capi.check(L.npgx_blockset_counts(self._h, ctypes.byref(nb), ctypes.byref(nf), ctypes.byref(rb)))
        n = max(nf.value, 1)
        bs = np.zeros(nb.value + 1, dtype=np.int64)
        seq = np.zeros(n, dtype=np.int32)
        mn = np.zeros(n, dtype=np.int64)
        mx = np.zeros(n, dtype=np.int64)
        ori = np.zeros(n, dtype=np.int8)
        _capi.check(L.npgx_blockset_copy(self._h, _capi.ptr(bs), _capi.ptr(seq), _capi.ptr(mn),
                                         _capi.ptr(mx), _capi.ptr(ori), None, None))
        return bs, seq[:nf.value], mn[:nf.value], mx[:nf.value], ori[:nf.value]

    def conseq(self):
        """ConSeq (ConSeq.cpp:37-50): the text of the sequence each block
        becomes, in block order (consensus of aligned blocks on the GPU)."""
        L = _bind(_capi.lib())
        nb, tot = ctypes.c_int64(), ctypes.c_int64()
        _capi.check(L.npgx_blockset_conseq(self._h, None, None, ctypes.byref(nb), ctypes.byref(tot)))
        buf = ctypes.create_string_buffer(max(tot.value, 1))
        off = np.zeros(nb.value + 1, dtype=np.int64)
        _capi.check(L.npgx_blockset_conseq(self._h, ctypes.cast(buf, ctypes.c_void_p), _capi.ptr(off),
                                           ctypes.byref(nb), ctypes.byref(tot)))
        raw = buf.raw
        return [raw[off[i]:off[i + 1]].decode() for i in range(nb.value)]

    def deconseq(self, cons, source=None):
        """DeConSeq (DeConSeq.cpp:48-96): the blocks of `cons` (an engine over
        the sequences conseq() made of `source`'s blocks, sequence i = block i)
        mapped back onto source's sequences and appended to this engine's
        blocks; source defaults to this engine."""
        L = _bind(_capi.lib())
        src = self if source is None else source
        _capi.check(L.npgx_blockset_deconseq(self._h, src._h, cons._h))
        return self

    def tune(self, key, value):
        """npgx_blockset_tune: "long-head" (the aligner's incremental shifts
        before the prefix search; 0 = never, the low-scratch kernels) or
        "elf-device" (1 / 0 / -1: ExtendLoopFast on the device / host /
        default) or "stage-clock" (1: DraftPangenome fills stats()["ms_gpu"],
        its GPU timeline by stage) or "smth-rows" (1: SmthUnion cuts from
        letter maps, the default; 0: from a host copy of the rows) or
        "refine-chunk" / "refine-min-len" (blocks of at least refine-min-len
        columns are refined in independent chunks cut at the first cut of
        every refine-chunk columns, a multiple of 64; 0: never).  Results do
        not change."""
        _capi.check(_capi.lib().npgx_blockset_tune(self._h, key.encode(), ctypes.c_int64(int(value))))
        return self

    def hash(self):
        h = ctypes.c_uint64()
        _capi.check(_capi.lib().npgx_blockset_hash(self._h, ctypes.byref(h)))
        return h.value

    def rows_digest(self):
        """npgx_blockset_rows_digest: a device-computed 64-bit digest of every
        gapped row bound to its fragment (tests/helpers.py restates it)."""
        h = ctypes.c_uint64()
        _capi.check(_capi.lib().npgx_blockset_rows_digest(self._h, ctypes.byref(h)))
        return h.value

    def block_stats(self):
        """npgx_blockset_block_stats: AlignmentStat of every block in set order
        (k_col_stat on the device), a list of dicts -- the five column classes,
        total, alignment_rows, min_fragment_length, letters (A T G C N) and
        identity_x1e4 (block_identity, truncated to four digits).  A block
        without rows has alignment_rows 0 and total -1."""
        L = _bind(_capi.lib())
        n = ctypes.c_int64()
        _capi.check(L.npgx_blockset_block_stats(self._h, None, 0, ctypes.byref(n)))
        out = (BlockStat * max(n.value, 1))()
        _capi.check(L.npgx_blockset_block_stats(self._h, out, n.value, ctypes.byref(n)))
        res = []
        for s in out[:n.value]:
            d = {k: int(getattr(s, k)) for k, _ in BlockStat._fields_ if k != "letters"}
            d["letters"] = [int(x) for x in s.letters]
            res.append(d)
        return res

    def pair_distances(self):
        """npgx_blockset_pair_distances: FragmentDistance::fragment_distance
        (FragmentDistance.cpp:31-69) of every pair of rows of every block
        (k_pair_dist), a list per block in set order of the penalties of its
        pairs (i ascending, j ascending); Distance.total is the block's
        length.  A block of one fragment has no pairs; NpgxError
        (NPGX_ERR_STATE) when a block of two or more fragments has no rows."""
        L = _bind(_capi.lib())
        nb, npairs = ctypes.c_int64(), ctypes.c_int64()
        _capi.check(L.npgx_blockset_pair_distances(self._h, None, None, 0, ctypes.byref(nb), ctypes.byref(npairs)))
        start = np.zeros(nb.value + 1, dtype=np.int64)
        pen = np.zeros(max(npairs.value, 1), dtype=np.int32)
        _capi.check(L.npgx_blockset_pair_distances(self._h, _capi.ptr(start), _capi.ptr(pen), npairs.value,
                                                   ctypes.byref(nb), ctypes.byref(npairs)))
        return [pen[start[k]:start[k + 1]].tolist() for k in range(nb.value)]

    def genomes(self):
        """genomes_list (block_stat.cpp:255-263): the sequences' genomes
        (Sequence::genome), sorted, each once."""
        from .model import Sequence
        return sorted({Sequence(n, "").genome() for n in self.ss.names})

    def genome_distances(self):
        """npgx_blockset_genome_distances: GlobalTree's add_dist
        (GlobalTree.cpp:68-83) over the blocks RemoveNonStem --exact would
        keep, summed on the device: the G x G matrix (lists of int) of
        mutations between the genomes in genomes() order."""
        L = _bind(_capi.lib())
        g, ns = ctypes.c_int32(), ctypes.c_int64()
        _capi.check(L.npgx_blockset_genome_distances(self._h, None, 0, ctypes.byref(g), ctypes.byref(ns)))
        out = np.zeros(max(g.value * g.value, 1), dtype=np.int64)
        _capi.check(L.npgx_blockset_genome_distances(self._h, _capi.ptr(out), g.value * g.value, ctypes.byref(g),
                                                     ctypes.byref(ns)))
        return out[:g.value * g.value].reshape(g.value, g.value).tolist()

    @staticmethod
    def _table(nodes, a, b):
        return [(int(x.parent), int(x.leaf), float(x.length), float(x.bootstrap)) for x in nodes[a:b]]

    def global_tree(self, bootstrap_print="before-length", pseudo_leafs=False):
        """npgx_blockset_global_tree: GlobalTree::run_impl (GlobalTree.cpp:85-116)
        -- the genome matrix, TreeNode::neighbor_joining (tree.cpp:360-480),
        add_diagnostic (ConsensusTree.cpp:294-367; k_clade_diag), optionally
        clone_with_pseudo_leafs, newick.  Returns (text, nodes): the file's
        text and the node table in print order, (parent entry, leaf, length,
        bootstrap) with the root first; leaf = the genome's index in genomes(),
        -2 - index for its pseudo leaf, -1 for an internal node.  NpgxError
        (NPGX_ERR_RANGE) for more than 64 genomes, (NPGX_ERR_ARG) for another
        bootstrap_print than no / in-braces / before-length."""
        L = _bind(_capi.lib())
        opts = ("--bootstrap-print=%s --tree-pseudo-leafs=%d" % (bootstrap_print, int(bool(pseudo_leafs)))).encode()
        tb, nn = ctypes.c_int64(), ctypes.c_int64()
        _capi.check(L.npgx_blockset_global_tree(self._h, opts, None, 0, ctypes.byref(tb), None, 0, ctypes.byref(nn)))
        text = ctypes.create_string_buffer(max(tb.value, 1))
        nodes = (TreeNode * max(nn.value, 1))()
        _capi.check(L.npgx_blockset_global_tree(self._h, opts, ctypes.cast(text, ctypes.c_void_p), tb.value,
                                                ctypes.byref(tb), nodes, nn.value, ctypes.byref(nn)))
        return text.raw[:tb.value].decode(), self._table(nodes, 0, nn.value)

    def block_trees(self, method="nj"):
        """npgx_blockset_block_trees: PrintTree::make_tree (PrintTree.cpp:51-67)
        of every block in set order, method "nj" or "upgma" (NpgxError
        NPGX_ERR_ARG otherwise): a list of (newick, nodes) -- print_newick's
        text with its defaults and the node table as global_tree's, leaf = the
        fragment's index in its block (named by Fragment::id in the text)."""
        L = _bind(_capi.lib())
        tb, nb, nn = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        _capi.check(L.npgx_blockset_block_trees(self._h, method.encode(), None, 0, ctypes.byref(tb), None, None, None,
                                                0, ctypes.byref(nb), ctypes.byref(nn)))
        text = ctypes.create_string_buffer(max(tb.value, 1))
        nodes = (TreeNode * max(nn.value, 1))()
        ts = np.zeros(nb.value + 1, dtype=np.int64)
        ns = np.zeros(nb.value + 1, dtype=np.int64)
        _capi.check(L.npgx_blockset_block_trees(self._h, method.encode(), ctypes.cast(text, ctypes.c_void_p), tb.value,
                                                ctypes.byref(tb), _capi.ptr(ts), _capi.ptr(ns), nodes, nn.value,
                                                ctypes.byref(nb), ctypes.byref(nn)))
        raw = text.raw
        return [(raw[ts[k]:ts[k + 1]].decode(), self._table(nodes, int(ns[k]), int(ns[k + 1])))
                for k in range(nb.value)]

    def realign_counts(self):
        """Outcomes of the last apply("ReAlign"): candidates, replaced,
        filter_refused (identity grew, Filter kept the old rows), not_better.
        NpgxError (NPGX_ERR_STATE) before any ReAlign."""
        L = _bind(_capi.lib())
        out = (ctypes.c_int64 * 4)()
        _capi.check(L.npgx_blockset_realign_counts(self._h, ctypes.byref(out)))
        return dict(zip(REALIGN_COUNT_NAMES, (int(x) for x in out)))

    def try_smth_counts(self):
        """Counts of the last apply("TrySmth ..."): blocks_in, blocks_tried
        (after the processor, ReAlign and Align), AddingLoopBySize rounds,
        blocks_cut, pieces, blocks_out, map_bytes and row_bytes downloaded by
        SmthUnion.  NpgxError (NPGX_ERR_STATE) before any TrySmth."""
        L = _bind(_capi.lib())
        out = (ctypes.c_int64 * 8)()
        _capi.check(L.npgx_blockset_try_smth_counts(self._h, ctypes.byref(out)))
        return dict(zip(TRY_SMTH_COUNT_NAMES, (int(x) for x in out)))

    def merge_unique_counts(self):
        """The last MergeUnique (alone or inside JoinerP / MergeAndJoin):
        blocks_inspected, merges, fragments_merged.  NpgxError
        (NPGX_ERR_STATE) before any MergeUnique."""
        L = _bind(_capi.lib())
        out = (ctypes.c_int64 * 3)()
        _capi.check(L.npgx_blockset_merge_unique_counts(self._h, ctypes.byref(out)))
        return dict(zip(MERGE_UNIQUE_COUNT_NAMES, (int(x) for x in out)))

    def refine_counts(self):
        """refine_alignment over the last apply: jobs, long_jobs (at least
        "refine-min-len" columns: refined in chunks), chunks, longest_chunk,
        columns_in, columns_out."""
        L = _bind(_capi.lib())
        out = (ctypes.c_int64 * 6)()
        _capi.check(L.npgx_blockset_refine_counts(self._h, ctypes.byref(out)))
        return dict(zip(REFINE_COUNT_NAMES, (int(x) for x in out)))

    def smth_counts(self):
        """SmthUnion's running totals on this set: map_bytes and row_bytes
        downloaded, blocks_cut, pieces."""
        L = _bind(_capi.lib())
        out = (ctypes.c_int64 * 4)()
        _capi.check(L.npgx_blockset_smth_counts(self._h, ctypes.byref(out)))
        return dict(zip(SMTH_COUNT_NAMES, (int(x) for x in out)))

    def block_names(self):
        """The blocks' names in set order ("00000000": a new block's)."""
        L = _bind(_capi.lib())
        n = ctypes.c_int64()
        _capi.check(L.npgx_blockset_block_names(self._h, None, 0, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(max(n.value, 1))
        _capi.check(L.npgx_blockset_block_names(self._h, ctypes.cast(buf, ctypes.c_void_p), n.value, ctypes.byref(n)))
        return buf.raw[:n.value].decode().split("\n")[:-1]

    def letter_map(self):
        """(diagnostic) k_letter_map over every row of every block with rows,
        in set order: a list of (words, prefix) per row -- uint64 words, bit c
        of word w set when column 64 w + c holds a letter, and int64 prefix[w]
        = the row's letters before word w."""
        L = _bind(_capi.lib())
        n = ctypes.c_int64()
        _capi.check(L.npgx_blockset_letter_map(self._h, None, None, 0, ctypes.byref(n)))
        words = np.zeros(max(n.value, 1), dtype=np.uint64)
        pre = np.zeros(max(n.value, 1), dtype=np.int64)
        _capi.check(L.npgx_blockset_letter_map(self._h, _capi.ptr(words), _capi.ptr(pre), n.value, ctypes.byref(n)))
        nf = len(self.fragments()[1])
        out, at = [], 0
        ro = np.zeros(nf + 1, dtype=np.int64)  # the rows' lengths (no row is downloaded)
        _capi.check(L.npgx_blockset_copy(self._h, None, None, None, None, None, _capi.ptr(ro), None))
        for i in range(len(ro) - 1):
            ln = int(ro[i + 1] - ro[i])
            if ln == 0:
                continue
            nw = (ln + 63) // 64
            out.append((words[at:at + nw].copy(), pre[at:at + nw].copy()))
            at += nw
        assert at == n.value
        return out

    def stats(self):
        st = BbStats()
        _capi.check(_capi.lib().npgx_blockset_stats(self._h, ctypes.byref(st)))
        d = {k: getattr(st, k) for k, _ in BbStats._fields_
             if k not in ("ms_stage", "counters", "loop", "ms_loop", "ms_gpu")}
        d["ms_gpu"] = {n: round(st.ms_gpu[i], 3) for i, n in enumerate(GPU_STAGE_NAMES)}
        d["ms_stage"] = {n: round(st.ms_stage[i], 3) for i, n in enumerate(STAGE_NAMES)}
        d["counters"] = {n: int(st.counters[i]) for i, n in enumerate(COUNTER_NAMES)}
        d["loop"] = {n: int(st.loop[i]) for i, n in enumerate(LOOP_NAMES)}
        d["ms_loop"] = {n: round(st.ms_loop[i], 3) for i, n in enumerate(LOOP_STAGE_NAMES)}
        d["loop_raw"] = [int(x) for x in st.loop]  # per pipe: AnchorLoopFast's LOOP_NAMES or AnchorLoop's
        return d

    def anchor_loop_stats(self):
        """Counts of the last AnchorLoop (include/npge_amd.h, npgx_bb_stats.loop)."""
        return dict(zip(ANCHOR_LOOP_NAMES, self.stats()["loop_raw"]))

    def job_stats(self):
        """(n_jobs, NPGX_JOB_STATS) int64 per alignment job of the last apply
        (layout in include/npge_amd.h, npgx_align_job_stats)."""
        L = _capi.lib()
        n = ctypes.c_int64()
        _capi.check(L.npgx_blockset_job_stats(self._h, None, 0, ctypes.byref(n)))
        out = np.zeros((max(n.value, 1), JOB_STATS), dtype=np.int64)
        _capi.check(L.npgx_blockset_job_stats(self._h, _capi.ptr(out), n.value, ctypes.byref(n)))
        return out[:n.value]

    def kernel_times(self):
        return _capi.kernel_times(_capi.lib().npgx_blockset_kernel_times, self._h)

    def __del__(self):
        if getattr(self, "_h", None) is not None:
            try:
                _capi.lib().npgx_blockset_free(self._h)
            except Exception:
                pass
            self._h = None
