"""A plain restatement of the reference's overlap_reads() (src/merge.c:399-688, with prob2scaledprob of misc.c:85-92) for the
tests: per-base profile rows, four products per cell, a log per cell, an ordered float chain per candidate.  It shares nothing
with the code under test: no table of cell scores, no helper of tagdust_amd, and pow / log are the C library's (math.pow, math.log).

    merge_pair(s1, q1, s2, q2, min_overlap, threshold) -> Merged     one pair, read 2 as it stands in its file
    merge_records(recs1, recs2, ...) -> [Merged]                     the records of parse_fastq
    text(names, merged) -> bytes                                     what `merge -t 1` prints
    in_reference_domain(...)                                         where the reference's own behaviour is defined

Where the reference is undefined the restatement follows the project: without a candidate best_d = -1,
nothing is written and the status is NO_CANDIDATE.  Reads beyond 512 bases are computed like any other."""
import collections
import math

import numpy as np

WRITTEN, BELOW, NO_CANDIDATE = 0, 1, 2
REFERENCE_MAX_BASES = 512           # the reference's binary aborts on a read of 513 bases or more
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
F32 = np.float32

Merged = collections.namedtuple("Merged", "best_d out_len id aligned status seq qual")


def parse_fastq(data):
    """[(name, sequence, qualities)] of four-line FASTQ text (bytes); the name is the header line without its '@'"""
    lines = data.decode().split("\n")
    assert lines[-1] == "" and (len(lines) - 1) % 4 == 0
    return [(lines[k][1:], lines[k + 1], lines[k + 3]) for k in range(0, len(lines) - 1, 4)]


def profile_rows(codes, qual):
    """merge.c:426-475: [len, 4] float32"""
    rows = np.empty((len(codes), 4), F32)
    for i, (x, ch) in enumerate(zip(codes, qual)):
        score = F32(1.0 - math.pow(10.0, -(ord(ch) - 33) / 10.0))
        other = F32((1.0 - float(score)) / 3.0)
        rows[i] = [F32(0.25)] * 4 if x > 3 else [score if c == x else other for c in range(4)]
    return rows


def cell_scores(a, b):
    """merge.c:492-497 for every (i, j): sum = 0.0f + a0 b0 + a1 b1 + a2 b2 + a3 b3 in float32, in that order, each product rounded
    before it is added; then (float)log((double)sum), -inf for a sum of zero"""
    s = np.zeros((len(a), len(b)), F32)
    for c in range(4):
        s = s + a[:, None, c] * b[None, :, c]           # float32 * float32 and float32 + float32: one rounding each
    assert s.dtype == F32
    values = np.unique(s)
    logs = np.array([-math.inf if v == 0.0 else math.log(float(v)) for v in values.tolist()], np.float64).astype(F32)
    return logs[np.searchsorted(values, s)]


def merge_pair(s1, q1, s2, q2, min_overlap=16, threshold=0.0):
    f = [CODE[c] for c in s1]
    r = [4 if CODE[c] > 3 else 3 - CODE[c] for c in reversed(s2)]          # merge.c:314-315: read 2 from its other strand
    fq, rq = q1, q2[::-1]
    len_f, len_r = len(f), len(r)
    a, b = profile_rows(f, fq), profile_rows(r, rq)
    cells = cell_scores(a, b)
    # merge.c:478-558: both sweeps in d order, a strict > from -inf
    max_score, best_d, d = F32(-math.inf), -1, 0
    for i in range(len_f):
        if len_f - i > min_overlap and len_r > min_overlap:
            score = np.cumsum(np.diagonal(cells, -i), dtype=F32)[-1]       # an ordered chain from 0.0f: 0.0f + x == x
            if score > max_score:
                max_score, best_d = score, d
        d += 1
    for j in range(len_r):
        if len_f > min_overlap and len_r - j > min_overlap:
            score = np.cumsum(np.diagonal(cells, j), dtype=F32)[-1]
            if score > max_score:
                max_score, best_d = score, d
        d += 1
    if best_d < 0:
        return Merged(-1, 0, 0, 0, NO_CANDIDATE, "", "")
    # merge.c:561-676
    out, qual = [], []
    local_i, local_j = (best_d, 0) if best_d < len_f else (0, best_d - len_f)
    for i in range(local_i):
        out.append("ACGTC"[f[i]])
        qual.append(fq[i])
    for j in range(local_j):
        out.append("ACGTC"[r[j]])
        qual.append(rq[j])
    ident = aligned = 0
    nuc = 0
    while local_i != len_f and local_j != len_r:
        if f[local_i] == r[local_j]:
            out.append("ACGTC"[f[local_i]])
            ident += 1
        else:
            best = F32(-math.inf)
            for c in range(4):
                if a[local_i, c] > best:
                    best, nuc = a[local_i, c], c
                if b[local_j, c] > best:
                    best, nuc = b[local_j, c], c
            out.append("ACGTC"[nuc])
        qual.append(fq[local_i] if fq[local_i] > rq[local_j] else rq[local_j])
        aligned += 1
        local_i += 1
        local_j += 1
    for i in range(local_i, len_f):
        out.append("ACGTC"[f[i]])
        qual.append(fq[i])
    for j in range(local_j, len_r):
        out.append("ACGTC"[r[j]])
        qual.append(rq[j])
    passes = bool(F32(ident) / F32(aligned) >= F32(threshold))              # merge.c:681, in float
    return Merged(best_d, len(out) if passes else 0, ident, aligned, WRITTEN if passes else BELOW, "".join(out), "".join(qual))


def merge_records(recs1, recs2, min_overlap=16, threshold=0.0):
    assert len(recs1) == len(recs2)
    return [merge_pair(x[1], x[2], y[1], y[2], min_overlap, threshold) for x, y in zip(recs1, recs2)]


def text(names, merged):
    """merge.c:329-331: one record per pair with out_len != 0, under the name of read 1"""
    return "".join("@%s\n%s\n+\n%s\n" % (n, m.seq, m.qual) for n, m in zip(names, merged) if m.out_len).encode()


def in_reference_domain(len_f, len_r, min_overlap, best_d):
    """The reference is defined for a pair when both reads are longer than min_overlap (else no candidate exists and it reads
    seq[-1]), neither is longer than 512 bases (its binary aborts), and some candidate has a finite score (best_d >= 0)."""
    return min(len_f, len_r) > min_overlap and max(len_f, len_r) <= REFERENCE_MAX_BASES and best_d >= 0
