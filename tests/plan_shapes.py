"""Barcode-segment shapes that move the model-specialised kernel's plan (tagdust_amd/csrc/td_spec_plan.cpp) onto branches no fixture
and no fuzz seed reaches: two run-time-looped segments, a first-segment trie order with groups of one or none at all, in-sweep label
sums in front of a second looped segment, restarted sweeps whose bridges cross two big barcode segments, a looped segment behind the
read segment, Illumina-style 8 / 10 / 12 nt indices.  Shared by tests/test_plan_shapes.py (CPU: the plan features and the input
conditions), tests/test_plan_shapes_gpu.py (both kernels against the oracle), tests/test_samples_gpu.py and tools/plan_survey.py.
Every generator is seeded; nothing here reads the device."""
import re

import numpy as np

THRESHOLD, MINLEN, DUST = 1.5, 16, 100
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
SPACER = "ACGT"
P5 = "ACGTTGCATCGG"
P3 = "AGATCGGAAGAGC"

# name -> (segments, seed, reads).  A segment is ("B", barcodes, bases[, "suffixes"]), ("S", text), ("F", bases), ("R",), ("P", text).
# "suffixes": the last two bases of the barcodes are pairwise distinct, so no suffix class fills a sharing group (trie order off).
SHAPES = {
    "A": ([("B", 16, 8), ("S", SPACER), ("B", 24, 8), ("R",)], 101, 256),
    "B": ([("B", 48, 6), ("B", 48, 6), ("R",)], 102, 512),
    "C": ([("B", 24, 10), ("F", 8), ("R",), ("P", P3)], 103, 256),
    "D": ([("B", 16, 6, "suffixes"), ("R",)], 104, 256),
    "E": ([("B", 16, 20), ("R",)], 105, 256),
    "F": ([("P", P5), ("B", 24, 8), ("B", 16, 8), ("R",)], 106, 256),
    "G": ([("R",), ("B", 24, 8)], 107, 256),
    "H": ([("B", 16, 8), ("R",), ("B", 16, 8)], 108, 256),
    "I": ([("B", 19, 12), ("R",)], 109, 256),
    "J": ([("B", 32, 8), ("S", "GT"), ("B", 32, 8), ("F", 8), ("R",), ("P", P3)], 110, 512),
}
NAMES = sorted(SHAPES)

# The plan features each shape is there for, under the default knobs (tests/test_plan_shapes.py asserts them).  share: kTrieNShare is
# "none" (0), "all" (kRt[0] / kGroup[0]: every group shares, no left-over slot) or "some" (strictly between).
PLAN = {
    "A": dict(H=45, rt=[16, 0, 24, 0], group=[2, 2, 2, 1], trie=True, share="some", first_n=17, prune_segs=3, restart=1),
    "B": dict(H=99, rt=[48, 48, 0], group=[3, 3, 1], trie=True, share="some", first_n=49, prune_segs=0, restart=0),
    "C": dict(H=28, rt=[24, 0, 0, 0], group=[1, 1, 1, 1], trie=True, share="all", first_n=0, prune_segs=2, restart=1),
    "D": dict(H=18, rt=[15, 0], group=[3, 1], trie=False, share="none", first_n=0, prune_segs=1, restart=1),
    "E": dict(H=18, rt=[16, 0], group=[1, 1], trie=True, share="all", first_n=0, prune_segs=1, restart=1),
    "F": dict(H=44, rt=[0, 24, 16, 0], group=[1, 2, 2, 1], trie=False, share="none", first_n=0, prune_segs=0, restart=0),
    "G": dict(H=26, rt=[0, 24], group=[1, 2], trie=False, share="none", first_n=0, prune_segs=0, restart=0),
    "H": dict(H=35, rt=[16, 0, 16], group=[2, 1, 2], trie=True, share="some", first_n=17, prune_segs=1, restart=1),
    "I": dict(H=21, rt=[19, 0], group=[1, 1], trie=True, share="all", first_n=0, prune_segs=1, restart=1),
    "J": dict(H=71, rt=[32, 0, 32, 0, 0, 0], group=[2, 2, 2, 1, 1, 1], trie=True, share="some", first_n=33, prune_segs=0, restart=0),
}

# Knob variants of the specialised kernel: (shape, environment, the plan features the knob is there to change).  Each gives the bytes
# of the default plan.
KNOB_VARIANTS = [
    ("A", {"TD_SPEC_TRIE_SH": "1"}, dict(trie=True, trie_sh=1, n_share=7)),          # more HMMs share one column than two
    ("A", {"TD_SPEC_TRIE_SH": "3"}, dict(trie=True, trie_sh=3)),
    ("A", {"TD_SPEC_RESTART": "0"}, dict(prune_segs=3, restart=0)),                  # cut sweeps, never restarted
    ("A", {"TD_SPEC_PRUNE": "0"}, dict(prune_segs=0, restart=0, first_n=17)),
    ("H", {"TD_SPEC_RESTART": "0"}, dict(prune_segs=1, restart=0)),
    ("B", {"TD_SPEC_FIRSTSEG": "0"}, dict(first_n=0, rt=[48, 48, 0])),               # 99 labels in the workspace label DP, two loops
    ("C", {"TD_SPEC_GROUPCOLS": "24"}, dict(group=[2, 1, 1, 1], rt=[24, 0, 0, 0], trie=True)),   # groups of two 10-column HMMs
]

# sample assignment on a realistic sheet (tests/test_samples_gpu.py): two 16-barcode indices around a spacer
SAMPLES_SHAPE = ([("B", 16, 8), ("S", "GT"), ("B", 16, 8), ("R",)], 120, 2048)


def _dna(rng, n):
    return "".join("ACGT"[x] for x in rng.randint(0, 4, n))


def _barcodes(rng, n, bases, suffixes=False):
    """n distinct barcodes, any two of them two or more mismatches apart (three from 8 bases on), in the order they were drawn"""
    apart = 3 if bases >= 8 else 2
    bars = []
    while len(bars) < n:
        b = _dna(rng, bases)
        if suffixes:
            b = b[:-2] + "ACGT"[len(bars) // 4] + "ACGT"[len(bars) % 4]
        if all(sum(x != y for x, y in zip(b, o)) >= apart for o in bars):
            bars.append(b)
    return bars


def segments_of(spec, rng):
    """The segment strings of a shape (the reference's -1 .. -k syntax) and the barcode lists of its B segments."""
    segs, bars = [], []
    for s in spec:
        if s[0] == "B":
            bars.append(_barcodes(rng, s[1], s[2], len(s) > 3))
            segs.append("B:" + ",".join(bars[-1]))
        elif s[0] == "F":
            segs.append("F:" + "N" * s[1])
        elif s[0] == "R":
            segs.append("R:N")
        else:
            segs.append(s[0] + ":" + s[1])
    return segs, bars


def make_reads(spec, seed, n_reads, window=None):
    """(segs, reads as text): reads that follow the segments -- the barcodes of every B segment dealt round-robin (the second B
    segment one further every round, so that the pairs vary), one barcode in ten a random k-mer -- through the mutation loop of the
    fuzz tests (substitution 2 %, deletion 1 %, insertion 1 %, N 0.5 %); one read in ten is unrelated random sequence, none shorter
    than segments + 6 bases: no read is without a path.  window = (matchstart, matchend): matchstart random bases in front of every
    read."""
    rng = np.random.RandomState(seed)
    segs, bars = segments_of(spec, rng)
    floor = len(segs) + 6
    reads = []
    for i in range(n_reads):
        parts, nb = [], 0
        for k, s in enumerate(spec):
            if s[0] == "B":
                b = bars[nb][(i + nb * (i // len(bars[nb]))) % len(bars[nb])]
                parts.append(_dna(rng, s[2]) if rng.random_sample() < 0.1 else b)
                nb += 1
            elif s[0] == "S":
                parts.append(s[1])
            elif s[0] == "F":
                parts.append(_dna(rng, s[1]))
            elif s[0] == "R":
                parts.append(_dna(rng, rng.randint(20, 61)))
            elif k == 0:                                                # a 5' linker keeps its end ...
                parts.append(s[1][rng.randint(0, len(s[1])):])
            else:                                                       # ... and a 3' adapter its start
                parts.append(s[1][:rng.randint(0, len(s[1]) + 1)])
        out = []
        for ch in "".join(parts):
            u = rng.random_sample()
            if u < 0.02:
                out.append("ACGT"[rng.randint(4)])
            elif u < 0.03:
                continue
            elif u < 0.04:
                out.append(ch); out.append("ACGT"[rng.randint(4)])
            elif u < 0.045:
                out.append("N")
            else:
                out.append(ch)
        s_ = "".join(out)
        if rng.random_sample() < 0.1 or len(s_) < floor:
            s_ = _dna(rng, rng.randint(floor, 90))
        if window:
            s_ = _dna(rng, window[0]) + s_
        reads.append(s_)
    return segs, reads


def make_case(spec, seed, n_reads, window=None):
    """(segs, seq, offs, md): make_reads as base codes, and the library builder's model for them at -e 0.05 -i 0.1 (its statistics
    taken under the window, if there is one) with the fixed decode parameters of this module."""
    from tagdust_amd import lib as tdlib
    segs, reads = make_reads(spec, seed, n_reads, window)
    reads = [np.array([CODE[ch] for ch in s_], np.uint8) for s_ in reads]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    seq = np.concatenate(reads)
    md, _ = tdlib.build_model(segs, seq, offs, 0.05, 0.1, window=window)
    md.update(threshold=THRESHOLD, minlen=MINLEN, dust=DUST)
    return segs, seq, offs, md


_CASES, _ORACLE = {}, {}
WINDOW = (3, 70)      # the -start / -end case on shape A


def case(name, window=None):
    """make_case of one of the ten shapes, made once"""
    if (name, window) not in _CASES:
        spec, seed, n = SHAPES[name]
        c = make_case(spec, seed, n, window)
        c[1].setflags(write=False); c[2].setflags(write=False)
        _CASES[(name, window)] = c
    return _CASES[(name, window)]


def oracle(name, window=None):
    """(results, labels, rewritten sequences) of the CPU oracle for case(name, window), computed once and read-only"""
    from oracle import pyoracle
    if (name, window) not in _ORACLE:
        segs, seq, offs, md = case(name, window)
        o = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, float(md["threshold"]), int(md["minlen"]), int(md["dust"]), 8,
                                 window=window)
        for a in o:
            a.setflags(write=False)
        _ORACLE[(name, window)] = o
    return _ORACLE[(name, window)]


def plan_features(src):
    """The plan of a model as tdlib.spec_source states it: dict(H, rt, group, trie, trie_sh, n_share, ord, first_n, prune_segs,
    sfx_first, restart, n_hmm, n_col)."""
    def arr(name):
        return [int(x) for x in re.search(r"static constexpr int %s\[\d+\] = \{([^}]*)\};" % name, src).group(1).split(",")]

    def num(name):
        return int(re.search(r"static constexpr int %s = (-?\d+);" % name, src).group(1))
    return dict(H=int(re.search(r"#define TD_H (\d+)", src).group(1)), rt=arr("kRt"), group=arr("kGroup"), n_hmm=arr("kNHmm"), n_col=arr("kNCol"),
                trie=re.search(r"static constexpr bool kTrieOn = (true|false);", src).group(1) == "true", trie_sh=num("kTrieSH"),
                n_share=num("kTrieNShare"), ord=arr("kTrieOrd"), first_n=num("kFirstN"), prune_segs=num("kPruneSegs"),
                sfx_first=num("kSfxFirst"), restart=int(re.search(r"#define TDS_RESTART (\d)", src).group(1)))


def share_class(p):
    """"none", "all" or "some": kTrieNShare against kRt[0] / kGroup[0]"""
    full = p["rt"][0] // p["group"][0] if p["rt"][0] else 0
    return "none" if p["n_share"] == 0 else "all" if p["n_share"] == full else "some"
