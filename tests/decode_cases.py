"""Seam inputs of the 2-bit sequence store (k_pack, pack_device,
npge_amd/csrc/seqset.hip) and of the decode of fragment text from it
(k_decode, add_decode, npge_amd/csrc/block_build.hip), shared by
test_decode_cases_ref.py (the oracle alone, on the CPU) and
test_decode_seams_gpu.py (engine against oracle and plain Python slices).

One set of sequences:

* lengths LENGTHS around 32 bases (a packed word), 64 (an N word, written by
  two lanes through atomicOr), 96 and 128 (the even-word padding: 2, 3, 4, 5
  words before the pad word) and 8192 (PIECE, the letters of one decode op),
  and one of LONG letters that holds the long fragments;
* every text twice under names that sort the other way round, in a shuffled
  input order, so a sequence's rank (size descending, name ascending) is not
  its input index and neighbours in the packed store differ in length;
* N at the first base, the last base, 31 | 32 and 63 | 64, and at the PIECE
  seams of the long text; a sequence of N only;
* the input spelled in lower case, with IUPAC letters (they become N) and with
  characters that are dropped, the twin spelled another way.

The blocks have no rows: two fragments of equal length, the same positions of
a text and of its twin in opposite orientations.  DummyAligner returns their
rows; with no gap in either row refine_alignment moves nothing, so every row
is the plain slice of the cleaned text, or its reverse complement (N stays N,
the complement is code ^ 1 on the device, a reverse fragment is read
pos - k).  Fragments start at POS (mod 64) and are FRAG letters long, and every
sequence is taken whole.

The engine lays such equal-length rows out straight from k_decode, without a
refinement.  `ragged` holds a few blocks of fragments of unequal lengths, which
it decodes into padded rows and refines (the long ones in chunks): there the
oracle says where the gaps go, and each row's letters are still the slice.
"""
import functools

import numpy as np

from oracle import oracle as orc

import column_cases as cc

LENGTHS = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 8191, 8192, 8193, 16385)
LONG = 16385 + 64
POS = (0, 1, 31, 32, 33, 63)
FRAG = (1, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193, 16385)
N_ONLY = 70
IUPAC = "RYMKWSBVHD"
DROPPED = "-x*. \n0"
KAT = ("acgtRYn-x*ACGT", "ACGTNNNACGT")


def py_atgcn(raw):
    """Sequence::to_atgcn in plain Python: upper case, A T G C N kept, IUPAC
    letters to N, everything else dropped."""
    out = []
    for c in raw.upper():
        if c in "ATGCN":
            out.append(c)
        elif c in IUPAC:
            out.append("N")
    return "".join(out)


def n_positions(n):
    """The named N positions of a text of n letters: {name: position}."""
    named = {"first": 0, "last": n - 1, "31": 31, "32": 32, "63": 63, "64": 64}
    if n >= LONG:
        named.update({"8191": 8191, "8192": 8192, "16383": 16383, "16384": 16384})
    return {k: p for k, p in named.items() if 0 <= p < n}


def _spell(rng, clean, how):
    """The clean text as an input spelling: 0 as it is, 1 lower case, 2 IUPAC
    letters for N, mixed case and dropped characters in between."""
    if how == 0:
        return clean
    if how == 1:
        return clean.lower()
    out, j = [], 0
    for c in clean:
        if c == "N":
            j += 1
            if j % 4:
                c = IUPAC[j % len(IUPAC)]
        if rng.random() < 0.3:
            c = c.lower()
        out.append(c)
        if rng.random() < 0.02:
            out.append(DROPPED[int(rng.integers(0, len(DROPPED)))])
    return DROPPED[:2] + "".join(out) + DROPPED[2:4]


class Decode:
    """names, raw (the input spellings), clean (after to_atgcn), twin (index
    of the other copy), blocks (row-less) and want (the blocks with their
    rows as plain slices)."""


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(211)
    texts = []
    for k, n in enumerate(LENGTHS + (LONG, N_ONLY)):
        t = list(cc._LETTERS[rng.integers(0, 4, n)].tobytes().decode())
        named = n_positions(n)
        kinds = (("first", "last"), ("31", "32"), ("63", "64"), tuple(named))[k % 4] if n < LONG else tuple(named)
        for name in kinds:
            if name in named:
                t[named[name]] = "N"
        if n == N_ONLY:
            t = ["N"] * n
        texts.append("".join(t))
    D = Decode()
    order = [(k, c) for k in range(len(texts)) for c in (0, 1)]
    order = [order[i] for i in rng.permutation(len(order))]
    D.names, D.raw, D.clean, D.text_of = [], [], [], []
    for k, c in order:
        D.names.append("%s%02d&c&c" % ("zy"[c] if k % 2 else "ab"[c], (len(texts) - k) if c else k))
        D.raw.append(_spell(rng, texts[k], (k + c + 1) % 3))
        D.clean.append(texts[k])
        D.text_of.append(k)
    D.twin = [next(j for j in range(len(order)) if j != i and D.text_of[j] == D.text_of[i]) for i in range(len(order))]
    first = [i for i in range(len(order)) if order[i][1] == 0]
    D.blocks, D.tags = [], []

    def add(i, pos, ln, flip, tag):
        a, b = (i, D.twin[i]) if not flip else (D.twin[i], i)
        D.blocks.append([(a, pos, pos + ln - 1, 1, None), (b, pos, pos + ln - 1, -1, None)])
        D.tags.append(tag)

    k = 0
    for ln in FRAG:
        for p in POS:
            hosts = [i for i in first if len(D.clean[i]) >= p + ln]
            i = hosts[k % len(hosts)] if ln < 8191 else max(hosts, key=lambda i: len(D.clean[i]))
            room = (len(D.clean[i]) - p - ln) // 64
            pos = p + 64 * (k % (room + 1))
            add(i, pos, ln, k % 2 == 1, "pos %d len %d" % (pos, ln))
            k += 1
    for i in first:
        add(i, 0, len(D.clean[i]), i % 2 == 1, "whole %d" % len(D.clean[i]))
    D.want = [[f[:4] + (text(D, f),) for f in b] for b in D.blocks]
    # fragments of unequal lengths: decoded by the same ops into rows that k_refine then fills with gaps (the long
    # ones in chunks); the oracle says where the gaps go, the letters are the slices
    long = max(first, key=lambda i: len(D.clean[i]))
    short = next(i for i in first if len(D.clean[i]) == 129)
    D.ragged = []
    for i, pos, ln, less in ((long, 31, 8193, 3), (long, 33, 16385, 1), (long, 64, 8192, 8191), (short, 63, 65, 64),
                             (short, 32, 33, 1)):
        D.ragged.append([(i, pos, pos + ln - 1, 1, None), (D.twin[i], pos, pos + ln - 1 - less, -1, None)])
        D.ragged.append([(D.twin[i], pos + less, pos + ln - 1, -1, None), (i, pos, pos + ln - 1, -1, None),
                         (i, pos, pos + ln - 1 - less, 1, None)])
    return D


def text(D, f):
    """The fragment's text: the slice, or its reverse complement."""
    s = D.clean[f[0]][f[1]:f[2] + 1]
    return s if f[3] == 1 else cc.revcomp(s)


@functools.lru_cache(maxsize=None)
def ragged_rows():
    """The oracle's DummyAligner on the ragged blocks (computed once)."""
    D = cases()
    o = orc.BlockSetOracle(list(D.raw), list(D.names))
    o.set_blocks([list(b) for b in D.ragged])
    return tuple(tuple(b) for b in o.apply("DummyAligner").blocks())
