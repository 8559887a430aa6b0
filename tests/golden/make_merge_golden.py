"""Regenerates tests/golden/merge/: paired FASTQ inputs and what the reference's `merge -t 1` writes for them.

    python tests/golden/make_merge_golden.py [/path/to/reference]

The reference's `merge` (src/merge.c) is compiled into a temporary directory with the flags of oracle/Makefile plus -DMERGE; nothing
of it is kept.  Two runs are recorded: the defaults, and `-Q 0.9 -minlen 20`.  Every pair lies in the reference's defined domain
for both runs: both reads longer than 20 bases, no '.'.

    r1.fq, r2.fq           300 pairs: reads of 21..150 bases, six quality characters, an N in every 17th read 1, an unrelated
                           read 2 in every 50th pair
    r1.fq.gz, r2.fq.gz     the same, compressed
    merged_default.fq      merge -t 1 r1.fq r2.fq
    merged_Q0.9_minlen20.fq  merge -t 1 -Q 0.9 -minlen 20 r1.fq r2.fq
"""
import gzip
import os
import random
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "merge")
RFLAGS = ["-O2", "-funroll-loops", "-std=gnu99", "-fcommon", "-w", "-DkslDEBUGLEVEL=0", '-DPACKAGE_NAME="Tagdust"',
          '-DPACKAGE_VERSION="2.33"', '-DPACKAGE_BUGREPORT="timolassmann@gmail.com"', "-DMERGE"]
SOURCES = ["kslib.c", "interface.c", "nuc_code.c", "io.c", "misc.c", "merge.c"]
QUALS = "#,5<AF"          # Phred 2, 11, 20, 27, 32, 37
QUAL_WEIGHTS = [1, 2, 3, 4, 5, 5]   # mostly good bases: about 4 % miscalls, so that -Q 0.9 keeps some pairs and drops others
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


def build_reference(ref, tmp):
    exe = os.path.join(tmp, "merge")
    subprocess.check_call(["gcc"] + RFLAGS + ["-o", exe] + [os.path.join(ref, "src", s) for s in SOURCES] + ["-lpthread", "-lm"])
    return exe


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
    ref = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
    os.makedirs(OUT, exist_ok=True)
    t1, t2 = generate()
    for name, text in (("r1.fq", t1), ("r2.fq", t2)):
        with open(os.path.join(OUT, name), "w") as f:
            f.write(text)
        with open(os.path.join(OUT, name + ".gz"), "wb") as f:
            with gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as g:
                g.write(text.encode())
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_reference(ref, tmp)
        for out, args in (("merged_default.fq", []), ("merged_Q0.9_minlen20.fq", ["-Q", "0.9", "-minlen", "20"])):
            res = subprocess.run([exe, "-t", "1"] + args + [os.path.join(OUT, "r1.fq"), os.path.join(OUT, "r2.fq")],
                                 stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
            with open(os.path.join(OUT, out), "wb") as f:
                f.write(res.stdout)
            print("%s: %d records" % (out, res.stdout.count(b"\n") // 4))


if __name__ == "__main__":
    main()
