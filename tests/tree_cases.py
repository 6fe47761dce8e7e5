"""Inputs of the tree and fragment-distance tests, shared by the CPU checks
(tests/test_tree_ref.py: every case has work in it) and the GPU parity tests
(tests/test_trees_gpu.py).  Everything is seeded; nothing here needs a GPU."""
import numpy as np

ALPHABET = "ATGCN-"
_LUT = np.frombuffer(ALPHABET.encode(), dtype=np.uint8)

# (rows, columns) of the single-block pair-distance cases
SHAPES = [(2, 1), (2, 2), (2, 3), (2, 63), (2, 64), (2, 65), (3, 66), (2, 129), (5, 4095), (5, 4096), (5, 4097),
          (5, 4098), (17, 9000), (65, 130), (300, 70)]
LENGTHS = [L for _, L in SHAPES]

# the seam cases: one isolated mismatch in two rows of SEAM_L columns
SEAM_L = 4200
SEAM_POS = [0, 1, 62, 63, 64, 65, 4094, 4095, 4096, 4097, 4198, 4199]
SEAM_FORMS = ["letter", "gap", "n-flank", "gap-flank"]

BOOTSTRAP_PRINTS = ["no", "in-braces", "before-length"]
PLANTED_G = [1, 2, 3, 4, 8, 17, 64]
PLANTED_COLUMNS = [63, 64, 4095, 4096]  # of the L = 4097 block of the G = 8 case


def text_of(codes):
    return [_LUT[row].tobytes().decode() for row in codes]


def random_rows(rng, n, L):
    """n gapped rows of L columns over A T G C N -: about 85 % of the cells
    copy the first row, so isolated mismatches are common; with L >= 3 the
    first two rows carry one planted isolated mismatch (columns 0..2), so
    every such block has a pair with a nonzero penalty; every row holds a
    letter."""
    codes = rng.choice(6, size=(n, L), p=[0.25, 0.25, 0.2, 0.15, 0.05, 0.1])
    codes = np.where(rng.random((n, L)) < 0.85, codes[0][None, :], codes)
    if L >= 3 and n >= 2:
        codes[0, 0:3] = [0, 3, 0]
        codes[1, 0:3] = [0, 2, 0]
    for i in range(n):
        if (codes[i] == 5).all():
            codes[i, i % L] = int(rng.integers(0, 5))
    return text_of(codes)


def blocks_of(row_lists):
    """(seqs, names, blocks): every row a fragment covering a sequence of its
    own (the row's letters); a row list of None rows: a block without rows."""
    seqs, blocks = [], []
    for rows in row_lists:
        b = []
        for r in rows:
            seqs.append(r.replace("-", "") if r is not None else "A")
            b.append((len(seqs) - 1, 0, len(seqs[-1]) - 1, 1, r))
        blocks.append(b)
    return seqs, ["q%d" % i for i in range(len(seqs))], blocks


def shape_rows():
    rng = np.random.default_rng(21)
    return [random_rows(rng, n, L) for (n, L) in SHAPES]


def seam_rows(L=SEAM_L, positions=SEAM_POS, n=2):
    """Per (position, form): (rows, expected penalty of every pair with the
    last row).  n rows, all equal but the last one, which carries the mismatch
    at the position: letter against letter; letter against gap; letter against
    letter between N/N flanks (still counted); between '-'/'-' flanks (not
    counted).  A centre at column 0 or L - 1 is never counted."""
    rng = np.random.default_rng(22)
    base = rng.integers(0, 4, size=L)
    out = []
    for c in positions:
        for form in SEAM_FORMS:
            a, b = base.copy(), base.copy()
            a[c] = 0
            b[c] = 5 if form == "gap" else 3
            inner = 0 < c < L - 1
            if form in ("n-flank", "gap-flank"):
                for f in (c - 1, c + 1):
                    if 0 <= f < L:
                        a[f] = b[f] = 4 if form == "n-flank" else 5
            exp = 1 if inner and form != "gap-flank" else 0
            out.append((c, form, text_of([a] * (n - 1) + [b]), exp))
    return out


def batch_rows(seed, count):
    """`count` random blocks: 2 to 70 rows (the long lengths with at most 8),
    the lengths of SHAPES, every tenth block a single fragment."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        L = int(rng.choice(LENGTHS))
        n = 1 if k % 10 == 9 else int(rng.integers(2, 71 if L < 1000 else 9))
        out.append(random_rows(rng, n, L))
    return out


def _evolve(rng, ids, row, rows, p_sub, fixed_split):
    if len(ids) == 1:
        rows[ids[0]] = row
        return
    k = len(ids) // 2 if fixed_split else int(rng.integers(1, len(ids)))
    for part in (ids[:k], ids[k:]):
        child = row.copy()
        L = len(child)
        sub = (rng.random(L) < p_sub) & (child != 5)
        child[sub] = (child[sub] + rng.integers(1, 4, size=int(sub.sum()))) % 4
        for _ in range(int(rng.poisson(L / 400.0))):
            s = int(rng.integers(0, L))
            child[s:s + int(rng.integers(1, 7))] = 5
        _evolve(rng, part, child, rows, p_sub, False)


def planted_genomes(G, seed=None):
    """A set of G genomes "G%02d&chr1&c" with one to three stem blocks whose
    rows evolved along a random binary tree (substitutions and deletions), L
    between 300 and 5000 and one block of 4097 columns, and non-stem blocks
    between them (a genome missing, a genome twice, both at once).  With three
    or more genomes the last two are twins (equal rows), so some clade has no
    diagnostic column; with two, every differing column is diagnostic for
    both.  Returns
    (seqs, names, blocks, stem) with stem = the positions of the stem blocks.
    G = 8: the first split is {0..3} | {4..7} on long branches, and the last
    stem block (4097 columns) has equal rows but for PLANTED_COLUMNS, where
    the rows of the genomes 0..3 hold another letter."""
    rng = np.random.default_rng(100 + G if seed is None else seed)
    names = ["G%02d&chr1&c" % g for g in range(G)]
    text = [[] for _ in range(G)]
    blocks, stem = [], []

    def add_block(genomes, rows):
        b = []
        for g, r in zip(genomes, rows):
            letters = r.replace("-", "")
            at = sum(len(x) for x in text[g])
            text[g].append(letters)
            b.append((g, at, at + len(letters) - 1, 1, r))
        blocks.append(b)

    def evolved(L):
        ids = list(range(G))
        if G != 8:
            rng.shuffle(ids)
        rows = [None] * G
        _evolve(rng, ids, rng.integers(0, 4, size=L), rows, 0.05 if G == 8 else 0.02, G == 8)
        for g in range(G):
            if (rows[g] == 5).all():
                rows[g][0] = 0
        if G >= 3:  # twins: no column sets either of them apart, so their clades count zero
            rows[G - 1] = rows[G - 2].copy()
        return text_of(rows)

    lengths = [4097] + [int(x) for x in rng.integers(300, 5001, size=int(rng.integers(0, 3)))]
    if G == 8:
        lengths = [1500, 4097]
    for k, L in enumerate(lengths):
        rows = evolved(L)
        if G == 8 and k == len(lengths) - 1:
            base = rng.integers(0, 4, size=L)
            codes = [base.copy() for _ in range(G)]
            for g in range(4):
                codes[g][PLANTED_COLUMNS] = (base[PLANTED_COLUMNS] + 1) % 4
            rows = text_of(codes)
        stem.append(len(blocks))
        add_block(list(range(G)), rows)
        # non-stem blocks made of the same rows: they must not count
        if G >= 2:
            add_block(list(range(1, G)), rows[1:])                 # a genome missing
            add_block([0] + list(range(1, G)) + [1], rows + [rows[0]])  # a genome twice
            add_block([1] + list(range(1, G)), rows)               # one missing, one twice: G fragments
        else:
            add_block([0, 0], rows + rows)
    seqs = ["".join(t) for t in text]
    return seqs, names, blocks, stem
