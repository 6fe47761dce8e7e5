"""Inputs around the AnchorFinder's cut (max-anchor-fragments): the table that
test_af_cut_cases_ref.py (CPU, the oracle alone) and test_af_cut_gpu.py share.

The engine's pass 2 on one GPU looks only at the windows of the
L = min(|H|, max-anchor-fragments + 1) smallest collected hashes, sorts their
FoundFragment keys and cuts after max-anchor-fragments of them.  Every case
below sits on one edge of that: where the cut falls in its group, L = |H|,
nothing collected, groups of one FoundFragment (Bloom false positives) under
the cut, a used-hash set from earlier runs, N runs, palindromes, k = 32,
anchor-similar off.  `tags` names the edges a case claims; `facts()` derives
them from the oracle's results (n_collected, n_found_frags, the used hashes,
the blocks), and test_af_cut_cases_ref.py asserts each claim.

Sequences are seeded, 300-3000 bp, 2-5 genomes.
"""
import numpy as np

from oracle import oracle as orc

LETTERS = "ACGT"
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def genomes(seed, n, length, mut=0.03, n_run=0, insert=None, related=True):
    """n mutated copies of one seeded root (related=False: n independent
    sequences); n_run: N runs of that length in every second copy; insert: a
    word put twice into every copy."""
    rng = np.random.default_rng(seed)
    root = rng.integers(0, 4, size=length)
    seqs, names = [], []
    for g in range(n):
        s = root.copy() if related else rng.integers(0, 4, size=length)
        m = rng.random(length) < mut
        s[m] = (s[m] + rng.integers(1, 4, size=int(m.sum()))) % 4
        t = "".join(LETTERS[c] for c in s)
        if insert:
            a, b = length // 5 + 3 * g, 3 * length // 5 + 5 * g
            t = t[:a] + insert + t[a + len(insert):b] + insert + t[b + len(insert):]
        if n_run and g % 2 == 1:
            a = length // 3 + 7 * g
            t = t[:a] + "N" * n_run + t[a + n_run:a + 40] + "N" + t[a + 41:]
        seqs.append(t)
        names.append("g%d&chr&c" % g)
    return seqs, names


def case(name, seqs_names, tags, k=12, fp="0.1", similar=True, maxf=100000, seed=1, params=None, runs=(False,)):
    """runs: one entry per run on the same handle, True = clear the used set first."""
    seqs, names = seqs_names
    return dict(name=name, seqs=seqs, names=names, tags=set(tags), k=k, fp=fp, similar=similar, maxf=maxf,
                seed=seed, params=params, runs=tuple(runs))


PALINDROME = "ACGTTAACGT"  # its own reverse complement (k = 10)
assert revcomp(PALINDROME) == PALINDROME

BASE = genomes(11, 3, 1200)

CASES = [
    case("inside_group", BASE, {"inside"}, maxf=40),
    case("on_boundary", BASE, {"boundary"}, maxf=41),
    case("max1", BASE, {"max1"}, maxf=1),
    case("max2", BASE, {"max2"}, maxf=2),
    case("max_is_total", BASE, {"untruncated", "max_is_total", "L_is_nH"}, maxf=255),
    case("untruncated", genomes(12, 4, 900), {"untruncated", "L_is_nH"}),
    case("nothing_found", genomes(13, 2, 400, related=False), {"nothing"}, k=20, fp="0.001"),
    case("shorter_than_k", (["ACGTACGTAC", "", "ACG"], ["a&c&c", "b&c&c", "c&c&c"]), {"empty"}, k=20),
    case("singles_untruncated", genomes(14, 3, 600), {"singles", "untruncated"}, k=7, fp="0.3"),
    case("singles_truncated", genomes(14, 3, 600), {"singles", "boundary"}, k=7, fp="0.3", maxf=59),
    case("singles_explicit_params", genomes(15, 2, 500), {"singles"}, k=8, fp="0.3", params=[3, 5, 7, 11], maxf=5000),
    case("used_set_kept", BASE, {"used"}, maxf=60, runs=(False, False, False)),
    case("used_set_cleared", BASE, {"used_cleared"}, maxf=60, runs=(False, True, True)),
    case("n_runs", genomes(16, 5, 800, n_run=25), {"N", "inside"}, maxf=100),
    case("palindromes", genomes(17, 3, 700, insert=PALINDROME, related=False), {"palindrome"}, k=10),
    case("k32", genomes(18, 3, 3000, mut=0.01), {"k32", "boundary"}, k=32, fp="0.01", maxf=100),
    case("similar_off", genomes(19, 4, 500), {"similar_off", "inside"}, similar=False, maxf=200),
]

# The sharded run alone (test_af_sharded_gpu.py).  SHARD_EXTRA: two sequences
# of one chunk of 256 windows each, so that with three or five ranks some rank
# owns no chunk and still joins every collective.  SHARDED is the part of
# CASES the sharded run repeats, EPOCH_CASES two of them at the two Bloom
# shapes (fp 0.1: 3 hash functions, window masks; fp 0.01: 7, none) for a
# sharded pass 1 in three epochs.
SHARD_EXTRA = [
    case("two_short", genomes(21, 2, 250), set()),
    case("two_short_off", genomes(21, 2, 250), {"similar_off"}, similar=False, maxf=30),
]

SHARDED = ("inside_group", "on_boundary", "max1", "max_is_total", "nothing_found", "shorter_than_k",
           "singles_truncated", "used_set_kept", "n_runs", "k32", "similar_off")

EPOCH_CASES = [dict(c, name="%s_fp%s" % (c["name"], fp), fp=fp)
               for c in CASES if c["name"] in ("inside_group", "used_set_kept") for fp in ("0.1", "0.01")]
EPOCH_HASHES = {"0.1": 3, "0.01": 7}

WG = 256  # windows per chunk (anchor_finder.hip)


def n_chunks(c):
    """Chunks of the engine's window layout, from the sequence lengths and k."""
    return sum((len(s) - c["k"] + 1 + WG - 1) // WG for s in c["seqs"] if len(s) >= c["k"])


REQUIRED_TAGS = {"inside", "boundary", "max1", "max2", "untruncated", "max_is_total", "L_is_nH", "nothing", "empty",
                 "singles", "used", "used_cleared", "N", "palindrome", "k32", "similar_off"}


def oracle_af(c, maxf=None):
    return orc.AnchorFinder(anchor_size=c["k"], anchor_fp_x1e4=int(round(float(c["fp"]) * 10000)),
                            anchor_similar=c["similar"],
                            max_anchor_fragments=c["maxf"] if maxf is None else maxf, seed=c["seed"],
                            params=c["params"])


def kept_groups(used_before, ro):
    """Hash groups under the cut, from the oracle's counts: every kept group
    but the first adds its hash to the used set (AnchorFinder.cpp:379-381), and
    something is kept whenever anything was found and the limit is not 0."""
    grew = len(ro["used"]) - used_before
    return grew + 1 if ro["n_found_frags"] > 0 and ro["maxf"] > 0 else 0


def oracle_runs(c):
    """The oracle's result of every run of the case, each with `maxf`,
    `used_before` and `kept_groups` added."""
    o = oracle_af(c)
    out, used = [], 0
    for clear in c["runs"]:
        if clear:
            o = oracle_af(c)
            used = 0
        ro = o.run(c["seqs"], c["names"])
        ro["maxf"] = c["maxf"]
        ro["used_before"] = used
        ro["kept_groups"] = kept_groups(used, ro)
        used = len(ro["used"])
        out.append(ro)
    return out


def _first_run(c, maxf):
    ro = oracle_af(c, maxf).run(c["seqs"], c["names"])
    ro["maxf"] = maxf
    return ro


def facts(c):
    """The edges the case's first run sits on (later runs: the used set), from
    the oracle's results alone."""
    runs = oracle_runs(c)
    r0 = runs[0]
    M, total, nH = c["maxf"], r0["n_found_frags"], r0["n_collected"]
    G = r0["kept_groups"]
    n_blocks = len(r0["block_start"]) - 1
    f = set()
    if 0 < M < total:
        # element M opens a new group iff one more kept element means one more group
        G1 = kept_groups(0, _first_run(c, M + 1))
        f.add("boundary" if G1 == G + 1 else "inside")
        assert G1 in (G, G + 1)
    if M == 1 and total > 1:
        f.add("max1")
    if M == 2 and total > 2:
        f.add("max2")
    if total > 0 and M >= total:
        f.add("untruncated")
        assert G == nH
    if total > 0 and M == total:
        f.add("max_is_total")
    if 0 < nH < M + 1:
        f.add("L_is_nH")
    windows = sum(max(0, len(s) - c["k"] + 1) for s in c["seqs"])
    if windows > 0 and nH == 0:
        f.add("nothing")
    if windows == 0:
        f.add("empty")
    # groups of one FoundFragment under the cut (they make no block); with the
    # cut inside a group that group's kept part could be one element too
    if "inside" not in f and G > n_blocks:
        f.add("singles")
    if len(runs) > 1 and all(not x for x in c["runs"][1:]) and all(r["used_before"] > 0 for r in runs[1:]):
        f.add("used")
    if len(runs) > 1 and all(c["runs"][1:]) and len(r0["used"]) > 0:
        f.add("used_cleared")
    if any("N" in s for s in c["seqs"]):
        f.add("N")
    bs = r0["block_start"]
    for b in range(n_blocks):
        i = int(bs[b])
        w = c["seqs"][int(r0["seq"][i])][int(r0["min_pos"][i]):int(r0["max_pos"][i]) + 1]
        if w == revcomp(w) and all(int(o) == 1 for o in r0["ori"][bs[b]:bs[b + 1]]):
            f.add("palindrome")
    if c["k"] == 32:
        f.add("k32")
    if not c["similar"]:
        f.add("similar_off")
    return f, runs

