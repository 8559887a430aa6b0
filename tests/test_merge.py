"""CPU-side checks of include/tagdust_merge.h: the host path against what the reference's `merge -t 1` wrote for the fixtures
(tests/golden/merge/, made by tests/golden/make_merge_golden.py), the pow() / log() tables against the C library, the tie rule,
the cases the reference leaves undefined, td_merge_stream on the host path, and the command's option check."""
import ctypes
import ctypes.util
import gzip
import os
import subprocess

import numpy as np
import pytest

from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "merge")
RUNS = [("merged_default.fq", 16, 0.0), ("merged_Q0.9_minlen20.fq", 20, 0.9)]


@pytest.fixture(scope="module")
def library():
    tdbuild.build()
    return tdlib.load_library()


def read(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def pairs(library):
    return tdlib.ParsedReads(read("r1.fq")), tdlib.ParsedReads(read("r2.fq"))


def fastq(records):
    """FASTQ text of (name, sequence, qualities) records"""
    return "".join("@%s\n%s\n+\n%s\n" % r for r in records).encode()


def host(text1, text2, **kw):
    r1, r2 = tdlib.ParsedReads(text1), tdlib.ParsedReads(text2)
    return tdlib.merge_batch(r1, r2, None, **kw), r1.names()


@pytest.mark.parametrize("recorded,minlen,threshold", RUNS)
def test_host_equals_reference_output(pairs, recorded, minlen, threshold):
    r1, r2 = pairs
    res = tdlib.merge_batch(r1, r2, None, min_overlap=minlen, threshold=threshold, n_threads=3)
    want = read(recorded)
    assert tdlib.merge_text(res, r1.names()) == want
    assert res["n_written"] == want.count(b"\n") // 4
    assert res["n_written"] + res["n_below"] == len(res["rec"]) and res["n_too_short"] == 0


def test_tables_equal_pow_and_log_of_the_c_library(library):
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    for f in (libm.pow, libm.log):
        f.restype = ctypes.c_double
    libm.pow.argtypes = [ctypes.c_double, ctypes.c_double]
    libm.log.argtypes = [ctypes.c_double]
    chars = bytes(range(33, 127))
    t = tdlib.merge_tables(chars)
    assert t["nq"] == 94 and t["dim"] == 470 and t["qchar"] == chars
    assert [int(t["qindex"][c]) for c in chars] == list(range(94))
    f32 = np.float32
    prof = np.zeros((94, 2), f32)
    for q, c in enumerate(chars):
        score = f32(1.0 - libm.pow(10.0, -(c - 33) / 10.0))
        prof[q] = (score, f32((1.0 - float(score)) / 3.0))
    assert np.array_equal(t["profile"].view(np.uint32), prof.view(np.uint32))
    # the four profile entries of every (quality, base code); sum = 0.0f + f0*r0 + f1*r1 + f2*r2 + f3*r3 in float, in that order
    P = np.zeros((470, 4), f32)
    for q in range(94):
        for x in range(5):
            P[5 * q + x] = [0.25 if x > 3 else (prof[q, 0] if c == x else prof[q, 1]) for c in range(4)]
    s = np.zeros((470, 470), f32)
    for c in range(4):
        s = (s + (P[:, None, c] * P[None, :, c]).astype(f32)).astype(f32)
    logs = {v: (float("-inf") if v == 0.0 else libm.log(float(v))) for v in np.unique(s).tolist()}
    want = np.array([logs[v] for v in s.ravel().tolist()], np.float64).astype(f32).reshape(470, 470)
    assert np.isneginf(want).any()          # '~' against a different '~' base: sum == 0
    assert np.array_equal(t["T"].view(np.uint32), want.view(np.uint32))
    # a batch's tables cover exactly its characters, in ascending order
    t = tdlib.merge_tables(b"FF#A#")
    assert t["nq"] == 3 and t["qchar"] == b"#AF" and t["T"].shape == (15, 15)


def test_identical_homopolymers_take_the_first_of_equal_maxima(library):
    # Read 2 is the reverse complement of read 1.  With quality '~' the profile is exactly (1, 0, 0, 0), a matching cell scores
    # log(1) = 0 and every candidate ties at 0.0, the main diagonal twice (d = 0 and d = len_f): the first one, d = 0, stays.
    res, names = host(fastq([("p", "A" * 40, "~" * 40)]), fastq([("p", "T" * 40, "~" * 40)]))
    assert res["rec"]["best_d"].tolist() == [0]
    assert res["rec"][["out_len", "id", "aligned", "status"]].tolist() == [(40, 40, 40, tdlib.MERGE_WRITTEN)]
    assert tdlib.merge_text(res, names) == b"@p\n" + b"A" * 40 + b"\n+\n" + b"~" * 40 + b"\n"
    # With a quality below that a matching cell scores a little under 0, so the shortest candidate wins: the last of the first sweep
    # (d = 23, 17 cells) ties with the last of the second (d = 40 + 23) and stays.
    res, names = host(fastq([("p", "A" * 40, "F" * 40)]), fastq([("p", "T" * 40, "F" * 40)]))
    assert res["rec"]["best_d"].tolist() == [23]


def test_too_short_pairs_write_nothing_and_are_counted(library):
    recs1 = [("a", "ACGTACGTACGTACGTACGTACGTA", "F" * 25), ("b", "ACGTACGTACGTACGTA", "F" * 17), ("c", "ACGTACGTACGTACGT", "F" * 16)]
    recs2 = [("a", "ACGTACGTACGTACGT", "F" * 16), ("b", "TACGTACGTACGTACGT", "F" * 17), ("c", "ACGTACGTACGTACGTACGTACGTA", "F" * 25)]
    res, names = host(fastq(recs1), fastq(recs2))
    assert res["rec"]["status"].tolist() == [tdlib.MERGE_NO_CANDIDATE, tdlib.MERGE_WRITTEN, tdlib.MERGE_NO_CANDIDATE]
    assert res["rec"]["best_d"].tolist()[0] == -1 and res["rec"]["out_len"].tolist()[0] == 0
    assert (res["n_written"], res["n_below"], res["n_too_short"]) == (1, 0, 2)
    assert tdlib.merge_text(res, names).count(b"\n") == 4
    # with -minlen 30 none of them has a candidate (the reference reads seq[-1] here)
    res, names = host(fastq(recs1), fastq(recs2), min_overlap=30)
    assert res["n_too_short"] == 3 and tdlib.merge_text(res, names) == b""


def test_undefined_inputs_fail_with_messages(library, tmp_path):
    good = fastq([("a", "ACGTACGTACGTACGTACGT", "F" * 20)])
    with pytest.raises(tdlib.TdError, match=r"'\.'"):
        host(fastq([("a", "ACGTACGTAC.TACGTACGT", "F" * 20)]), good)
    with pytest.raises(tdlib.TdError, match="FASTA"):
        host(b">a\nACGTACGTACGTACGTACGT\n", good)
    with pytest.raises(tdlib.TdError, match="number of records"):
        host(good + good, good)
    out = str(tmp_path / "out.fq")

    def stream(t1, t2):
        p1, p2 = str(tmp_path / "x1.fq"), str(tmp_path / "x2.fq")
        open(p1, "wb").write(t1)
        open(p2, "wb").write(t2)
        return tdlib.merge_stream(p1, p2, out, None, n_threads=2)

    with pytest.raises(tdlib.TdError, match="differ in number of entries"):
        stream(good + good, good)
    with pytest.raises(tdlib.TdError, match="different order"):
        stream(good, fastq([("b", "ACGTACGTACGTACGTACGT", "F" * 20)]))
    with pytest.raises(tdlib.TdError, match="FASTA"):
        stream(b">a\nACGTACGTACGTACGTACGT\n", b">a\nACGTACGTACGTACGTACGT\n")
    with pytest.raises(tdlib.TdError, match=r"'\.'"):
        stream(fastq([("a", "ACGTACGTAC.TACGTACGT", "F" * 20)]), good)
    with pytest.raises(tdlib.TdError, match="cannot find"):
        tdlib.merge_stream(str(tmp_path / "missing.fq"), str(tmp_path / "x2.fq"), out, None)


@pytest.mark.parametrize("batch_pairs", [7, 100000])
@pytest.mark.parametrize("suffix", ["", ".gz"])
def test_stream_on_the_host_path(library, tmp_path, batch_pairs, suffix):
    for recorded, minlen, threshold in RUNS:
        out = str(tmp_path / recorded)
        st = tdlib.merge_stream(os.path.join(GOLD, "r1.fq" + suffix), os.path.join(GOLD, "r2.fq" + suffix), out, None,
                                min_overlap=minlen, threshold=threshold, n_threads=2, batch_pairs=batch_pairs)
        want = read(recorded)
        assert open(out, "rb").read() == want
        assert st["n_pairs"] == 300 and st["n_written"] == want.count(b"\n") // 4 and st["bytes_out"] == len(want)
        assert st["n_batches"] == (300 + batch_pairs - 1) // batch_pairs and st["n_too_short"] == 0


def test_gz_fixtures_hold_the_plain_ones():
    for name in ("r1.fq", "r2.fq"):
        assert gzip.decompress(read(name + ".gz")) == read(name)


def test_command_on_the_host_path_and_its_option_check(library, tmp_path):
    exe = tdbuild.MERGE_EXE
    r = subprocess.run([exe, "--host", "-t", "2", "-Q", "0.9", "-minlen", "20", os.path.join(GOLD, "r1.fq"), os.path.join(GOLD, "r2.fq")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == read("merged_Q0.9_minlen20.fq")
    out = str(tmp_path / "m.fq")
    r = subprocess.run([exe, "--host", "--batch-pairs", "64", "--out", out, os.path.join(GOLD, "r1.fq.gz"), os.path.join(GOLD, "r2.fq.gz")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == read("merged_default.fq")
    for bad in (["-join", "x"], ["--frobnicate"], ["-1", "R:N"]):
        r = subprocess.run([exe] + bad + [os.path.join(GOLD, "r1.fq"), os.path.join(GOLD, "r2.fq")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and r.stdout == b"" and ("unknown option " + bad[0]).encode() in r.stderr
    r = subprocess.run([exe, "--host", os.path.join(GOLD, "r1.fq")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 1 and b"two input files" in r.stderr
