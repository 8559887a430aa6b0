"""Regenerates tests/golden/merge/: paired FASTQ inputs and what the reference's `merge -t 1` writes for them.

    python tests/golden/make_merge_golden.py [/path/to/reference]

The reference's `merge` (src/merge.c) is built by oracle/Makefile into oracle/_ref/merge (git-ignored); nothing of it is kept
here.  Only inputs and what `merge -t 1` wrote for them are recorded, and every recorded run is first compared with the plain
restatement of tests/merge_plain.py: the reference must exit 0 and its bytes must equal the restatement's text.

First input pair, two runs: the defaults, and `-Q 0.9 -minlen 20`.  Every pair lies in the reference's defined domain for both
runs: both reads longer than 20 bases, no '.'.

    r1.fq, r2.fq           300 pairs: reads of 21..150 bases, six quality characters, an N in every 17th read 1, an unrelated
                           read 2 in every 50th pair
    r1.fq.gz, r2.fq.gz     the same, compressed
    merged_default.fq      merge -t 1 r1.fq r2.fq
    merged_Q0.9_minlen20.fq  merge -t 1 -Q 0.9 -minlen 20 r1.fq r2.fq

Second input pair: the sets of tests/merge_cases.py FIXTURE_SETS -- the edge shapes of the kernel (sweep boundaries, the 512-base
limit, ties, '~' and '!'), pairs whose id / aligned equals a threshold exactly and their twins one mismatch worse, pairs over
"!~F", over all 94 quality characters, and with every fifth base an N -- filtered to the reference's defined domain by
merge_plain.in_reference_domain (a zero exit status does not mark it: outside it the binary may also write garbage).  A record is
named <set><index in its set>, so the names tell which pairs the filter took out.

    edge_r1.fq, edge_r2.fq   the pairs
    edge_merged_default.fq   merge -t 1 -minlen 16 edge_r1.fq edge_r2.fq
    edge_merged_Q<x>.fq      merge -t 1 -Q <x> edge_r1.fq edge_r2.fq, for x = 0.9, 0.95, 0.75, 0.7: the thresholds of the boundary pairs
"""
import gzip
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import merge_cases  # noqa: E402
import merge_plain  # noqa: E402

OUT = os.path.join(HERE, "merge")
ORACLE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle")
QUALS = "#,5<AF"          # Phred 2, 11, 20, 27, 32, 37
QUAL_WEIGHTS = [1, 2, 3, 4, 5, 5]   # mostly good bases: about 4 % miscalls, so that -Q 0.9 keeps some pairs and drops others
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def build_reference(ref):
    """oracle/_ref/merge by the recipe of oracle/Makefile"""
    subprocess.check_call(["make", "-C", ORACLE, "_ref/merge"] + (["REF=" + ref] if ref else []))
    return os.path.join(ORACLE, "_ref", "merge")


def record(exe, out, args, in1, in2, min_overlap, threshold):
    """runs the reference, holds its bytes against the restatement, and only then writes them"""
    res = subprocess.run([exe, "-t", "1"] + args + [os.path.join(OUT, in1), os.path.join(OUT, in2)], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)
    assert res.returncode == 0, (out, res.returncode)
    recs1 = merge_plain.parse_fastq(open(os.path.join(OUT, in1), "rb").read())
    recs2 = merge_plain.parse_fastq(open(os.path.join(OUT, in2), "rb").read())
    plain = merge_plain.merge_records(recs1, recs2, min_overlap, threshold)
    assert all(merge_plain.in_reference_domain(len(a[1]), len(b[1]), min_overlap, m.best_d) for a, b, m in zip(recs1, recs2, plain)), out
    assert res.stdout == merge_plain.text([r[0] for r in recs1], plain), out + ": the reference and the restatement differ"
    with open(os.path.join(OUT, out), "wb") as f:
        f.write(res.stdout)
    print("%s: %d records, %d bytes" % (out, res.stdout.count(b"\n") // 4, len(res.stdout)))


def edge_fixture():
    """(names, pairs) of the second input pair: FIXTURE_SETS inside the reference's defined domain"""
    names, pairs = [], []
    for prefix, make in merge_cases.FIXTURE_SETS:
        for k, (a, b) in enumerate(make()):
            m = merge_plain.merge_pair(a[0], a[1], b[0], b[1], 16, 0.0)
            if merge_plain.in_reference_domain(len(a[0]), len(b[0]), 16, m.best_d):
                names.append("%s%d" % (prefix, k))
                pairs.append((a, b))
    # the pairs at a threshold and their twins: the full overlap must be the best candidate of each
    for k, (a, b) in enumerate(merge_cases.boundary_pairs()):
        bases, mismatches = merge_cases.BOUNDARY[k // 2][:2]
        m = merge_plain.merge_pair(a[0], a[1], b[0], b[1], 16, 0.0)
        assert (m.best_d, m.id, m.aligned) == (0, bases - mismatches - k % 2, bases) and "bound%d" % k in names, k
    return names, pairs


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def sequenced(rng, s):
    """(read, qualities): every base gets a quality character and is miscalled at that quality's error rate"""
    out, qual = [], []
    for c in s:
        q = rng.choices(QUALS, QUAL_WEIGHTS)[0]
        if rng.random() < 10.0 ** (-(ord(q) - 33) / 10.0):
            c = rng.choice([b for b in "ACGT" if b != c])
        out.append(c)
        qual.append(q)
    return "".join(out), "".join(qual)


def generate(n_pairs=300, seed=20151):
    rng = random.Random(seed)
    r1, r2 = [], []
    for p in range(n_pairs):
        len_f, len_r = rng.randint(21, 150), rng.randint(21, 150)
        frag_len = rng.randint(max(len_f, len_r), len_f + len_r + 10)       # from full containment to no overlap at all
        frag = "".join(rng.choice("ACGT") for _ in range(frag_len))
        s1, q1 = sequenced(rng, frag[:len_f])
        mate = frag[frag_len - len_r:] if (p + 1) % 50 else "".join(rng.choice("ACGT") for _ in range(len_r))
        s2, q2 = sequenced(rng, revcomp(mate))
        if (p + 1) % 17 == 0:
            k = rng.randrange(len_f)
            s1 = s1[:k] + "N" + s1[k + 1:]
        name = "M01:7:FLOWCELL:1:%d:%d:%d" % (1101 + p // 100, 1000 + 13 * p, 2000 + 7 * p)
        r1.append("@%s 1:N:0:1\n%s\n+\n%s\n" % (name, s1, q1))
        r2.append("@%s 2:N:0:1\n%s\n+\n%s\n" % (name, s2, q2))
    return "".join(r1), "".join(r2)


def main():
    exe = build_reference(sys.argv[1] if len(sys.argv) > 1 else None)
    os.makedirs(OUT, exist_ok=True)
    t1, t2 = generate()
    for name, text in (("r1.fq", t1), ("r2.fq", t2)):
        with open(os.path.join(OUT, name), "w") as f:
            f.write(text)
        with open(os.path.join(OUT, name + ".gz"), "wb") as f:
            with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
                g.write(text.encode())
    record(exe, "merged_default.fq", [], "r1.fq", "r2.fq", 16, 0.0)
    record(exe, "merged_Q0.9_minlen20.fq", ["-Q", "0.9", "-minlen", "20"], "r1.fq", "r2.fq", 20, 0.9)
    names, pairs = edge_fixture()
    for name, text in zip(("edge_r1.fq", "edge_r2.fq"), merge_cases.texts(pairs, names)):
        with open(os.path.join(OUT, name), "wb") as f:
            f.write(text)
        print("%s: %d pairs, %d bytes" % (name, len(pairs), len(text)))
    for out, min_overlap, threshold, args in merge_cases.EDGE_RUNS:
        record(exe, out, args, "edge_r1.fq", "edge_r2.fq", min_overlap, threshold)


if __name__ == "__main__":
    main()
