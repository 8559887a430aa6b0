"""Generated read pairs for the merge tests (tests/test_merge_reference.py, tests/test_merge_gpu.py) and for the recorded edge
fixtures (tests/golden/make_merge_golden.py).  A pair is ((sequence 1, qualities 1), (sequence 2, qualities 2)), read 2 as it
stands in its file.  Every generator is seeded: the fixtures under tests/golden/merge/ hold exactly these pairs."""
import random

COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
Q60 = "".join(chr(c) for c in range(35, 95))
Q94 = "".join(chr(c) for c in range(33, 127))


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def rand_qual(rng, n, chars):
    return "".join(rng.choice(chars) for _ in range(n))


def overlapping(rng, len_f, len_r, chars, errors=0.03):
    """a pair cut from one fragment (read 2 from its other strand), with a few miscalls"""
    frag_len = rng.randint(max(len_f, len_r), len_f + len_r)
    frag = rand_seq(rng, frag_len)

    def miscalled(s):
        return "".join(rng.choice("ACGT") if rng.random() < errors else c for c in s)
    return (miscalled(frag[:len_f]), rand_qual(rng, len_f, chars)), (miscalled(revcomp(frag[frag_len - len_r:])), rand_qual(rng, len_r, chars))


def names_of(pairs, prefix="p"):
    return ["%s%d" % (prefix, i) for i in range(len(pairs))]


def texts(pairs, names=None):
    """the two FASTQ files (bytes) of a list of pairs"""
    names = names_of(pairs) if names is None else names
    t1 = "".join("@%s\n%s\n+\n%s\n" % (n, a[0], a[1]) for n, (a, b) in zip(names, pairs))
    t2 = "".join("@%s\n%s\n+\n%s\n" % (n, b[0], b[1]) for n, (a, b) in zip(names, pairs))
    return t1.encode(), t2.encode()


def edge_pairs():
    """the shapes named in the kernel's header: group boundaries of the 64-lane candidate sweep, the staging limit, ties, -inf cells"""
    rng = random.Random(7)
    Q = "#5AF"
    pairs = []
    for lf, lr in ((17, 17), (17, 300), (300, 17),                       # one candidate per sweep; one long and one short read
                   (31, 32), (32, 32), (32, 33), (64, 64), (64, 65),     # len_f + len_r = 63, 64, 65, 128, 129
                   (80, 81), (81, 80), (97, 97), (150, 150), (512, 512), (33, 512)):   # 64 and 65 candidates per sweep; the staging limit
        pairs.append(overlapping(rng, lf, lr, Q))
    pairs.append(overlapping(rng, 1000, 150, Q))                         # past the staging room: the host path takes the pair
    pairs.append(overlapping(rng, 150, 513, Q))
    pairs.append((("N" * 70, rand_qual(rng, 70, Q)), (rand_seq(rng, 90), rand_qual(rng, 90, Q))))      # an all-N read
    pairs.append(((rand_seq(rng, 90), rand_qual(rng, 90, Q)), ("N" * 70, rand_qual(rng, 70, Q))))
    pairs.append(((rand_seq(rng, 120), rand_qual(rng, 120, Q)), (rand_seq(rng, 110), rand_qual(rng, 110, Q))))   # unrelated reads
    s = rand_seq(rng, 100)
    pairs.append(((s, "F" * 100), (revcomp(s), "F" * 100)))             # identical reads: d = 0 and d = len_f score the same
    pairs.append((("A" * 40, "~" * 40), ("T" * 40, "~" * 40)))           # every candidate ties at 0.0: d = 0 stays
    pairs.append((("A" * 130, "~" * 130), ("T" * 130, "~" * 130)))       # the same over several 64-lane groups
    s = rand_seq(rng, 60)
    pairs.append(((s, "~" * 60), (revcomp(s), "~" * 60)))               # '~': a mismatching cell is log(0) = -inf
    pairs.append(((rand_seq(rng, 50), "~" * 50), (rand_seq(rng, 50), "~" * 50)))   # ... on every candidate: none wins
    pairs.append(((s, "!" * 60), (revcomp(s), "!" * 60)))               # '!': the called base has probability 0
    pairs.append(((rand_seq(rng, 70), rand_qual(rng, 70, "!~F")), (rand_seq(rng, 75), rand_qual(rng, 75, "!~F"))))
    pairs.append(((rand_seq(rng, 16), "F" * 16), (rand_seq(rng, 40), "F" * 40)))   # too short: no candidate
    return pairs


def random_pairs(n, chars, seed, lo=17, hi=160):
    rng = random.Random(seed)
    return [overlapping(rng, rng.randint(lo, hi), rng.randint(lo, hi), chars) for _ in range(n)]


def n_rich(pairs):
    """every fifth base of both reads replaced by N"""
    def every_fifth(s):
        return "".join("N" if k % 5 == 4 else c for k, c in enumerate(s))
    return [((every_fifth(a[0]), a[1]), (every_fifth(b[0]), b[1])) for a, b in pairs]


# (bases, mismatches, threshold, seed): a full overlap of `bases` cells at quality 'F' of which exactly `mismatches` differ, so that
# id / aligned equals the threshold exactly -- 18/20, 19/20, 15/20, 28/40 -- and the pair is written; and a twin with one mismatch
# more, which is not.  The seeds are such that the full overlap, d = 0, is the best candidate of every one of them.
BOUNDARY = [(20, 2, 0.9, 1), (20, 1, 0.95, 2), (20, 5, 0.75, 3), (40, 12, 0.7, 30)]
THRESHOLDS = [0.0] + [b[2] for b in BOUNDARY]


def boundary_pairs():
    """[at the threshold, one mismatch worse] for each entry of BOUNDARY, in that order"""
    pairs = []
    for bases, mismatches, _, seed in BOUNDARY:
        rng = random.Random(seed)
        s = rand_seq(rng, bases)
        where = rng.sample(range(bases), mismatches + 1)
        for k in (mismatches, mismatches + 1):
            t = list(s)
            for i in where[:k]:
                t[i] = rng.choice([c for c in "ACGT" if c != s[i]])
            pairs.append(((s, "F" * bases), (revcomp("".join(t)), "F" * bases)))
    return pairs


# the sets of the recorded edge fixtures (tests/golden/merge/edge_*), before the filter to the reference's defined domain;
# the names in the files are <set><index in this list>
FIXTURE_SETS = [
    ("edge", edge_pairs),
    ("bound", boundary_pairs),
    ("q3_", lambda: random_pairs(36, "!~F", 31, 17, 90)),
    ("q94_", lambda: random_pairs(36, Q94, 32, 17, 90)),
    ("nrich", lambda: n_rich(random_pairs(36, "#5AF", 33, 17, 90))),
]
# (recorded file, min_overlap, threshold, the reference's options)
EDGE_RUNS = [("edge_merged_default.fq", 16, 0.0, ["-minlen", "16"]), ("edge_merged_Q0.9.fq", 16, 0.9, ["-Q", "0.9"]),
             ("edge_merged_Q0.95.fq", 16, 0.95, ["-Q", "0.95"]), ("edge_merged_Q0.75.fq", 16, 0.75, ["-Q", "0.75"]),
             ("edge_merged_Q0.7.fq", 16, 0.7, ["-Q", "0.7"])]
