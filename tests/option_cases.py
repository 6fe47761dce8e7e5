"""Option vectors off the defaults and the inputs they run on, shared by
test_options_gpu.py (engine against oracle) and test_oracle_options.py (the
oracle's result must move with every vector, so the comparison has teeth).

Aligner vectors are (mismatch_check, gap_check, aligned_check, min_length,
min_identity_x1e4); block-build variations are keyword sets of BlockSetEngine,
mapped to the oracle's keywords by oracle_kw().  Every oracle result is
computed once per process and handed out unchanged.
"""
import functools

import numpy as np

from oracle import oracle as orc
from npge_amd import synth

from test_similar_aligner_gpu import KATS, _family, _random_jobs, _restart_family
from test_block_build_gpu import _stem_blocks

DEFAULT_VECTOR = (1, 2, 10, 100, 9000)

# (vector, input set): the set where the oracle shows the vector biting
ALIGN_VECTORS = [
    ((0, 2, 10, 100, 9000), "short"),
    ((3, 2, 10, 100, 9000), "short"),
    ((4, 2, 10, 100, 9000), "mid"),
    ((1, 1, 10, 100, 9000), "short"),
    ((1, 5, 10, 100, 9000), "short"),
    ((1, 6, 10, 100, 9000), "mid"),
    ((1, 2, 1, 100, 9000), "short"),
    ((1, 2, 2, 100, 9000), "short"),
    ((1, 2, 5, 100, 9000), "short"),
    ((1, 2, 16, 100, 9000), "short"),
    ((1, 2, 10, 30, 9000), "mid"),
    ((1, 2, 10, 20, 9800), "mid"),
    ((1, 2, 10, 100, 9900), "mid"),
    ((1, 2, 10, 100, 7000), "mid"),
    ((2, 3, 4, 20, 8000), "short"),
]

# the vectors of the split / deferred and wide legs
LEG_VECTORS = [(1, 2, 5, 100, 9000), (1, 2, 10, 30, 9000), (2, 3, 4, 20, 8000), (0, 2, 10, 100, 9000)]
PREFIX_VECTORS = [(1, 2, 2, 100, 9000), (1, 2, 16, 100, 9000)]


def vid(v):
    return "-".join(str(x) for x in v)


@functools.lru_cache(maxsize=None)
def jobs(name):
    """The aligner input sets (tuples of tuples of rows; never changed)."""
    if name == "short":
        # rows 1-17: the vector search (<= 8 rows) and the row-parallel search
        # with the LDS word table (> 8)
        out = _random_jobs(101, 60, nmax=17, lmax=300) + KATS
    elif name == "mid":
        # long enough for min_length / min_identity to move FindLowSimilar's regions
        rng = np.random.default_rng(7)
        out = []
        for _ in range(40):
            n = int(rng.integers(2, 18))
            L = int(rng.integers(300, 1500))
            d = float(rng.choice([0.03, 0.08, 0.15]))
            out.append(_family(rng, n, L, d, tail_unrelated=float(rng.choice([0.0, 0.5]))))
    elif name == "long":
        # the split / deferred legs: 2-17 rows x 2,000-4,000 columns
        rng = np.random.default_rng(13)
        out = []
        for n, d, tail in ((2, 0.01, 0.0), (3, 0.05, 0.3), (5, 0.1, 0.0), (8, 0.02, 0.3), (9, 0.05, 0.0),
                           (12, 0.1, 0.3), (17, 0.03, 0.0)):
            out.append(_family(rng, n, int(rng.integers(2000, 4000)), d, tail_unrelated=tail))
    elif name == "wide":
        # more than 64 rows: the workgroup-per-problem aligner
        rng = np.random.default_rng(17)
        out = [_family(rng, n, L, d, tail_unrelated=0.3)
               for n, L, d in ((65, 150, 0.03), (78, 220, 0.08), (90, 300, 0.15))]
        # with 20 and more rows unrelated from a random column on, nearly every
        # column of those three is bad and min_length decides nothing: two
        # families without tails, with bad regions a few columns long
        out.append(_family(np.random.default_rng(17), 70, 280, 0.001))
        out.append(_family(np.random.default_rng(19), 70, 280, 0.003, indel=0.5))
    elif name == "wide_restart":
        out = [_restart_family(np.random.default_rng(19), 70, 200, 1500)]
    elif name == "prefix":
        # insertions of up to 2,000 bases: try_aligned's prefix search, at 3 rows
        # (the vector search) and 12 (the row-parallel one)
        rng = np.random.default_rng(23)
        out = [_restart_family(rng, n, 300, 2000, d=0.03, repeat=rep) for n in (3, 12) for rep in (0.0, 0.5, 1.0)]
    else:
        raise KeyError(name)
    return tuple(tuple(j) for j in out)


@functools.lru_cache(maxsize=None)
def oracle_align(name, vector):
    """The oracle's align_seqs of every job of the set with the vector."""
    return tuple(tuple(orc.align(list(j), "align_seqs", params=vector)) for j in jobs(name))


def changed_jobs(name, vector):
    """How many jobs of the set the vector aligns otherwise than the defaults."""
    return sum(a != b for a, b in zip(oracle_align(name, vector), oracle_align(name, DEFAULT_VECTOR)))


# ---------------------------------------------------------------- block build
_ORACLE_KEYS = {
    "min_fragment": ("fix_min_fragment", "filter_min_fragment"),
    "min_identity_x1e4": ("fix_min_identity_x1e4", "filter_min_identity_x1e4"),
    "frame_length": ("filter_frame_length",),
    "min_end": ("filter_min_end",),
    "min_block": ("filter_min_block",),
    "max_block": ("filter_max_block",),
    "find_subblocks": ("filter_find_subblocks",),
    "extend_portion_x1e4": ("portion_x1e4",),
    "align_min_length": ("min_length",),
    "align_min_identity_x1e4": ("min_identity_x1e4",),
}


def oracle_kw(kw):
    """BlockSetEngine keywords -> BlockSetOracle keywords (the one place the
    two sides' names meet)."""
    out = {}
    for k, v in kw.items():
        for ok in _ORACLE_KEYS.get(k, (k,)):
            assert ok not in out, ok
            out[ok] = v
    assert set(out) <= set(orc.PIPELINE_DEFAULTS), sorted(set(out) - set(orc.PIPELINE_DEFAULTS))
    return out


def align_kw(v):
    return dict(mismatch_check=v[0], gap_check=v[1], aligned_check=v[2], align_min_length=v[3],
                align_min_identity_x1e4=v[4])


COMBINED = dict(min_fragment=40, frame_length=30, min_end=4, min_identity_x1e4=9500)

# the step-by-step chain on `tiny`, once per variation
BB_VARIATIONS = [
    ("extend_length_37", dict(extend_length=37)),
    ("extend_length_250", dict(extend_length=250)),
    ("extend_portion_5000", dict(extend_portion_x1e4=5000)),
    ("min_fragment_30", dict(min_fragment=30)),
    ("min_fragment_250", dict(min_fragment=250)),
    ("min_identity_9900", dict(min_identity_x1e4=9900)),
    ("min_identity_7000", dict(min_identity_x1e4=7000)),
    ("frame_length_20", dict(frame_length=20)),
    ("frame_length_333", dict(frame_length=333)),
    ("min_end_1", dict(min_end=1)),
    ("min_end_40", dict(min_end=40)),
    ("find_subblocks_0", dict(find_subblocks=0)),
    ("combined", COMBINED),
    # goodSlices' guard (goodSlices.cpp: end_length > min_length returns no slice)
    ("guard_min_end_60_min_fragment_40", dict(min_end=60, min_fragment=40)),
]

# Filter alone on blocks of 2 and 3 fragments
BLOCK_SIZE_VARIATIONS = [
    ("min_block_3", dict(min_block=3)),
    ("max_block_2", dict(max_block=2)),
    ("max_block_2_no_subblocks", dict(max_block=2, find_subblocks=0)),
]

META_VECTORS = [(2, 3, 6, 40, 9500), (0, 1, 14, 150, 8000)]

PIPE_VECTORS = [
    ("V1", dict(extend_length=60, min_fragment=40, frame_length=30, min_end=4, min_identity_x1e4=9500,
                **align_kw((2, 3, 6, 40, 9500)))),
    ("V2", dict(extend_length=250, min_fragment=150, frame_length=200, min_end=25, min_identity_x1e4=8500,
                **align_kw((0, 1, 14, 150, 8000)))),
    ("V3", dict(find_subblocks=0, max_iterations=4, aligned_check=3)),
]
# the oracle's DraftPangenome with these vectors: (blocks, iterations)
PIPE_EXPECTED = {("tiny", "V1"): (124, 10), ("tiny", "V2"): (33, 5), ("tiny", "V3"): (9, 4),
                 ("rtiny", "V1"): (119, 10), ("rtiny", "V2"): (38, 5), ("rtiny", "V3"): (12, 4)}

CHAIN = ("FragmentsExtender", "FixEnds", "FragmentsExtender", "Filter")
# test_processors_step_by_step compares the extender's blocks in order (==)
# and the slicing processors' as sets (canon)
CHAIN_ORDERED = (True, False, True, False)


def _freeze(blocks):
    return tuple(tuple(b) for b in blocks)


def thaw(blocks):
    return [list(b) for b in blocks]


@functools.lru_cache(maxsize=None)
def genome_set(cfg):
    names, seqs = synth.genome_set(cfg)
    return tuple(names), tuple(seqs)


@functools.lru_cache(maxsize=None)
def stem_blocks(cfg):
    names, seqs = genome_set(cfg)
    return _freeze(_stem_blocks(list(seqs), list(names)))


def _kw_key(kw):
    return tuple(sorted(kw.items()))


@functools.lru_cache(maxsize=None)
def _oracle_chain(cfg, key):
    names, seqs = genome_set(cfg)
    o = orc.BlockSetOracle(list(seqs), list(names), **oracle_kw(dict(key)))
    cur = thaw(stem_blocks(cfg))
    steps = []
    for op, ordered in zip(CHAIN, CHAIN_ORDERED):
        if ordered:  # the engine's test restarts the extender from the oracle's blocks
            o.set_blocks(cur)
        o.apply(op)
        cur = o.blocks()
        steps.append(_freeze(cur))
    return tuple(steps)


def oracle_chain(cfg, kw):
    """The oracle's blocks after each step of CHAIN, from the stem blocks of
    the set; before an extender step the blocks are set anew (rows kept)."""
    return _oracle_chain(cfg, _kw_key(kw))


@functools.lru_cache(maxsize=None)
def long_block():
    """(names, seqs, blocks): one aligned block of 3 rows and more than 4,096
    columns (more than one column tile of FixEnds / Filter), with an
    unrelated stretch in one row and ragged ends, so the slicing has work."""
    rng = np.random.default_rng(29)
    rows = _family(rng, 3, 6000, 0.03)
    junk = "".join("ATGC"[x] for x in rng.integers(0, 4, 300))
    rows[1] = rows[1][:2500] + junk + rows[1][2800:]
    rows[2] = "".join("ATGC"[x] for x in rng.integers(0, 4, 60)) + rows[2][60:]
    aligned = orc.align(rows, "align_seqs")
    assert len(aligned[0]) > 4096
    names = ("a&chr1&c", "b&chr1&c", "c&chr1&c")
    blocks = [[(i, 0, len(r) - 1, 1, a) for i, (r, a) in enumerate(zip(rows, aligned))]]
    return names, tuple(rows), _freeze(blocks)


@functools.lru_cache(maxsize=None)
def _oracle_long_block(key):
    names, seqs, blocks = long_block()
    o = orc.BlockSetOracle(list(seqs), list(names), **oracle_kw(dict(key)))
    out = []
    for op in ("FixEnds", "Filter"):
        o.set_blocks(thaw(blocks))
        o.apply(op)
        out.append(_freeze(o.blocks()))
    return tuple(out)


def oracle_long_block(kw):
    """The oracle's FixEnds and Filter, each on the long block itself."""
    return _oracle_long_block(_kw_key(kw))


@functools.lru_cache(maxsize=None)
def mixed_size_blocks():
    """The extended `tiny` blocks (the default chain before its Filter) with
    one fragment dropped from every third block: blocks of 2 and of 3
    fragments, which min-block / max-block tell apart."""
    out = []
    for i, b in enumerate(oracle_chain("tiny", {})[2]):
        out.append(tuple(b[:-1]) if i % 3 == 0 and len(b) > 2 else b)
    assert {len(b) for b in out} >= {2, 3}
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _oracle_filter_mixed(key):
    names, seqs = genome_set("tiny")
    o = orc.BlockSetOracle(list(seqs), list(names), **oracle_kw(dict(key)))
    o.set_blocks(thaw(mixed_size_blocks()))
    o.apply("Filter")
    return _freeze(o.blocks())


def oracle_filter_mixed(kw):
    return _oracle_filter_mixed(_kw_key(kw))


@functools.lru_cache(maxsize=None)
def meta_blocks():
    """test_meta_aligner's widened anchors on the first 150 stem blocks of
    `tiny`, single fragments and aligned blocks."""
    names, seqs = genome_set("tiny")
    b0 = thaw(stem_blocks("tiny"))
    rng = np.random.default_rng(3)
    blocks = []
    for b in b0[:150]:
        nb = []
        for s, mn, mx, ori, _ in b:
            a = int(rng.integers(0, 40))
            z = int(rng.integers(0, 40))
            nb.append((s, max(0, mn - a), min(len(seqs[s]) - 1, mx + z), ori, None))
        blocks.append(nb)
    blocks += [[b[0][:4] + (None,)] for b in b0[150:160]]
    blocks += b0[160:170]
    return _freeze(blocks)


@functools.lru_cache(maxsize=None)
def oracle_meta(vector):
    names, seqs = genome_set("tiny")
    o = orc.BlockSetOracle(list(seqs), list(names), **oracle_kw(align_kw(vector)))
    o.set_blocks(thaw(meta_blocks()))
    o.apply("MetaAligner")
    return _freeze(o.blocks())


@functools.lru_cache(maxsize=None)
def _oracle_draft(cfg, key):
    names, seqs = genome_set(cfg)
    o = orc.BlockSetOracle(list(seqs), list(names), **oracle_kw(dict(key)))
    o.apply("DraftPangenome")
    return _freeze(o.blocks()), o.stats()


def oracle_draft(cfg, kw):
    """(blocks, stats) of the oracle's DraftPangenome."""
    return _oracle_draft(cfg, _kw_key(kw))
