"""The cut rule of the chunked refine_alignment, restated in numpy, and the
inputs its CPU and GPU tests share.

A column is solid when every row holds the same letter in it and no row a
gap.  A cut lies between columns c and c+1 when both are solid and their
letters differ.  No move of refine_alignment (refine_alignment.cpp:38-63,
:86-129) reads or writes across such a cut, so refining the pieces between
cuts, each to its own fixpoint, and laying them end to end gives the
refinement of the whole.  The engine uses, per tile of `chunk` columns, the
first cut (c in the tile, the chunk starts at c+1); tiles without a cut merge
into their neighbour.
"""
import numpy as np

from oracle import oracle as orc

GAP = ord("-")


def solid_letters(rows):
    """Per column: the letter's code where the column is solid, else 0."""
    if not rows or not rows[0]:
        return np.zeros(0, dtype=np.uint8)
    a = np.frombuffer("".join(rows).encode(), dtype=np.uint8).reshape(len(rows), len(rows[0]))
    solid = (a == a[0]).all(axis=0) & (a[0] != GAP)
    return np.where(solid, a[0], 0).astype(np.uint8)


def tile_cuts(rows, chunk):
    """One entry per tile: the smallest c+1 with c in the tile and a cut
    between c and c+1, or -1."""
    v = solid_letters(rows)
    L = len(v)
    cut = np.zeros(L, dtype=bool)
    if L > 1:
        cut[:-1] = (v[:-1] != 0) & (v[1:] != 0) & (v[:-1] != v[1:])
    out = []
    for c0 in range(0, L, chunk):
        w = np.flatnonzero(cut[c0:c0 + chunk])
        out.append(int(c0 + w[0] + 1) if len(w) else -1)
    return out


def chunk_list(rows, chunk):
    """[(start, end)] of the chunks of one long alignment."""
    L = len(rows[0])
    starts = [0] + [c for c in tile_cuts(rows, chunk) if c >= 0]
    return list(zip(starts, starts[1:] + [L]))


def refine(rows):
    return orc.align(rows, mode="refine")


def refine_chunked(rows, chunk):
    """The oracle's refine_alignment of every chunk, laid end to end."""
    parts = [refine([r[s:e] for r in rows]) for s, e in chunk_list(rows, chunk)]
    return ["".join(p[i] for p in parts) for i in range(len(rows))]


def expected_counts(alignments, chunk, min_len, refined):
    """What npgx_refine_batch_ex's counts_out holds for the batch."""
    c = dict(jobs=len(alignments), long_jobs=0, chunks=0, longest_chunk=0,
             columns_in=sum(len(a[0]) if a else 0 for a in alignments),
             columns_out=sum(len(r[0]) if r else 0 for r in refined))
    for a in alignments:
        if chunk > 0 and a and len(a[0]) >= min_len and len(a[0]) > 0:
            ch = chunk_list(a, chunk)
            c["long_jobs"] += 1
            c["chunks"] += len(ch)
            c["longest_chunk"] = max(c["longest_chunk"], max(e - s for s, e in ch))
    return c


# ---------------------------------------------------------------- inputs
def family(rng, n, length, d, indel=0.1):
    """n mutated copies of a random ancestor (substitutions, short indels)."""
    anc = rng.integers(0, 4, length)
    rows = []
    for _ in range(n):
        out, i = [], 0
        while i < length:
            r = rng.random()
            if r < d * (1 - indel):
                out.append((int(anc[i]) + int(rng.integers(1, 4))) % 4)
                i += 1
            elif r < d:
                k = int(rng.integers(1, 6))
                if rng.random() < 0.5:
                    out.extend(int(x) for x in rng.integers(0, 4, k))
                else:
                    i += k
            else:
                out.append(int(anc[i]))
                i += 1
        rows.append("".join("ATGC"[x] for x in out))
    return rows


def traded(rng, aln, swaps):
    """Letters and gaps trade places inside each row (test_refine_random)."""
    rows = []
    for r in aln:
        r = list(r)
        for _ in range(int(rng.integers(0, swaps + 1))):
            p, q = int(rng.integers(0, len(r))), int(rng.integers(0, len(r)))
            r[p], r[q] = r[q], r[p]
        rows.append("".join(r))
    return rows


KATS = [["CCGG", "CG-G", "CG-G", "CG-G"], ["CCGGCC", "CGG--C"], ["-CCCCCC", "CCCACCC", "CCCTCCC"]]

RANDOM_SHAPES = [(21, 2, 1500), (22, 5, 3100), (23, 17, 6000), (24, 9, 2047)]


def random_alignments():
    """Aligner output of random families at 2-17 rows x 1500-6000 columns, and
    the same with letters and gaps traded."""
    out = []
    for seed, n, length in RANDOM_SHAPES:
        rng = np.random.default_rng(seed)
        aln = orc.align(family(rng, n, length, float(rng.choice([0.005, 0.02, 0.05]))), mode="similar")
        out += [aln, traded(rng, aln, 12)]
    return out


def homopolymer_alignment(seed=31, n=4, length=1500):
    """Rows over A and T in runs of 1-40, a few gaps scattered into each."""
    rng = np.random.default_rng(seed)
    base, x = [], "A"
    while len(base) < length:
        base += [x] * int(rng.integers(1, 41))
        x = "T" if x == "A" else "A"
    base = base[:length]
    rows = []
    for _ in range(n):
        r = list(base)
        for p in sorted(int(x) for x in rng.integers(0, length, 6)):
            r.insert(p, "-")
        rows.append("".join(r))
    L = max(len(r) for r in rows)
    return [r.ljust(L, "-") for r in rows]


def no_cut_alignment(seed=41, n=4, length=700):
    """Every column holds a gap or a mismatch somewhere."""
    rng = np.random.default_rng(seed)
    a = np.array([list(r) for r in _equal(family(rng, n, length, 0.02, indel=0.0))])
    for c in range(a.shape[1]):
        k = c % n
        if rng.random() < 0.5:
            a[k, c] = "-"
        else:
            a[k, c] = "ATGC"[("ATGC".index(a[(k + 1) % n, c]) + 1) % 4]
    return ["".join(r) for r in a]


def _equal(rows):
    L = min(len(r) for r in rows)
    return [r[:L] for r in rows]


def placed_cuts_alignment(chunk=128, L=64 * 5 + 17):
    """No solid column except those placed: cuts at 63|64, chunk-1|chunk and
    L-2|L-1, and two solid columns of one letter at 2*chunk-1|2*chunk, which
    must not be cut."""
    rows = [list(r) for r in no_cut_alignment(seed=52, n=3, length=L)]
    placed = {63: "A", 64: "C", chunk - 1: "G", chunk: "T", 2 * chunk - 1: "A", 2 * chunk: "A", L - 2: "C", L - 1: "G"}
    for c, x in placed.items():
        for r in rows:
            r[c] = x
    return ["".join(r) for r in rows]


def pure_gap_border_alignment():
    """Pure-gap columns 56..71 (across the border of the first tile of 64) in
    an alignment with cuts on both sides of them."""
    rng = np.random.default_rng(61)
    aln = _equal(family(rng, 3, 400, 0.03, indel=0.0))
    aln = traded(rng, [r[:200] + "-" * 3 + r[200:] for r in aln], 6)
    return [r[:56] + "-" * 16 + r[56:] for r in aln]


def wide_alignment():
    """70 rows x about 2000 columns: aligner output with gaps traded."""
    rng = np.random.default_rng(71)
    aln = orc.align(family(rng, 70, 2000, 0.002), mode="similar")
    return traded(rng, aln, 4)


def boundary_alignment():
    """300 columns (no multiple of 64) for min_len = 299, 300, 301."""
    rng = np.random.default_rng(81)
    aln = orc.align(family(rng, 4, 290, 0.03), mode="similar")
    aln = [r[:300].ljust(300, "-") for r in aln]
    return traded(rng, aln, 6)


_CASES = {}


def cases():
    """name -> list of alignments; made once."""
    if not _CASES:
        _CASES.update({
            "kats": KATS,
            "random": random_alignments(),
            "homopolymer": [homopolymer_alignment()],
            "no_cut": [no_cut_alignment()],
            "placed": [placed_cuts_alignment()],
            "pure_gap_border": [pure_gap_border_alignment()],
            "wide": [wide_alignment()],
            "boundary": [boundary_alignment()],
        })
    return _CASES


_REFINED = {}


def refined(name):
    """The oracle's whole-block refinement of cases()[name]; made once."""
    if name not in _REFINED:
        _REFINED[name] = [refine(a) for a in cases()[name]]
    return _REFINED[name]
