"""The fingerprint as bases (td_fingerprint_text, td_writer_set_fingerprint_text of include/tagdust_io.h), no GPU: against a
restatement of the reference's get_finger_seq (src/io.c:1018-1029) in Python, through the host writer, and -- where the reference
binary is built -- against what that binary prints with -show_finger_seq for fingerprints of 4, 12 and 14 bases."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

RBIN = os.path.join(REPO, "oracle", "_ref")
BARCODES = ["ACGTAC", "TTGACA", "GGATCC"]


@pytest.fixture(scope="module", autouse=True)
def library():
    tdbuild.build()
    return tdlib.load_library()


def text_py(fp):
    """get_finger_seq with C's int: & and >> on a Python int behave as on a two's complement int of any width"""
    ln = fp & 0xFF
    key = fp >> 8
    out = []
    for _ in range(ln):
        out.append("ACGT"[key & 3])
        key >>= 2
    return "".join(reversed(out))


def fingerprint_of(word):
    v = 0
    for ch in word:
        v = (v << 2) | "ACGT".index(ch)
    v = (v << 8) | len(word)
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= 1 << 31 else v        # as the reference's int holds it


def test_text_against_the_restatement():
    rng = np.random.default_rng(7)
    assert tdlib.fingerprint_text(27 << 8 | 4) == "ACGT" == text_py(27 << 8 | 4)
    assert tdlib.fingerprint_text(-1) == "T" * 255 == text_py(-1)
    assert tdlib.fingerprint_text(-1253657586) == "TTGTCCCACGGTCA" == text_py(-1253657586)
    assert tdlib.fingerprint_text(0) == ""
    seen_negative = 0
    for ln in (1, 4, 12, 14):
        for _ in range(200):
            word = "".join("ACGT"[b] for b in rng.integers(0, 4, ln))
            fp = fingerprint_of(word)
            seen_negative += fp < 0
            got = tdlib.fingerprint_text(fp)
            assert got == text_py(fp) and len(got) == ln
            if ln <= 12:
                assert got == word                       # 24 bits of bases fit the int
            else:
                assert got[2:] == word[2:]               # the two leading bases were shifted out; what stands there is the sign's
    assert seen_negative > 50
    for fp in rng.integers(-(1 << 31), 1 << 31, 500):
        assert tdlib.fingerprint_text(int(fp)) == text_py(int(fp))


def _fastq_text(g):
    names = bytes(g["names"]).split(b"\n")
    offs = g["offs"]
    alpha = np.frombuffer(b"ACGTN", np.uint8)
    return b"".join(b"@" + names[i] + b"\n" + bytes(alpha[g["seq"][offs[i]:offs[i + 1]]]) + b"\n+\n" + bytes(g["qual"][offs[i]:offs[i + 1]]) + b"\n"
                    for i in range(int(g["n_reads"])))


def _segments_of(g):
    segs = []
    for t, grp in zip(g["seg_type"], str(g["seg_seqs"]).split(";")):
        t = chr(int(t))
        seqs = grp.split(",")
        segs.append("%s:%s" % (t, ",".join(seqs[:-1] if t in "BS" else seqs)))
    return segs


@pytest.mark.parametrize("name", ["umi_f_s_r", "r_s_b_f"])
def test_host_writer_prints_the_text_on_a_fixture_s_results(tmp_path, name):
    """the fixture's own results (the reference's) through td_writer_write, with and without the switch: the files differ in the FP
    tag alone, and the text is td_fingerprint_text of the number"""
    g = load_golden(name)
    pr = tdlib.ParsedReads(_fastq_text(g), 2)
    res = np.zeros(pr.n, tdlib.RESULT_DTYPE)
    for k in ("read_type", "barcode", "fingerprint"):
        res[k] = g[k]
    res["mapq"] = g["mapq"]
    tdlib.write_demultiplexed(str(tmp_path / "num"), _segments_of(g), pr, res, g["seq_after"])
    tdlib.write_demultiplexed(str(tmp_path / "txt"), _segments_of(g), pr, res, g["seq_after"], fingerprint_text=True)
    num = {os.path.basename(f)[3:]: open(f).read() for f in glob.glob(str(tmp_path / "num*.fq"))}
    txt = {os.path.basename(f)[3:]: open(f).read() for f in glob.glob(str(tmp_path / "txt*.fq"))}
    assert num and set(num) == set(txt)
    n_tags = 0
    for k in num:
        a, b = num[k].splitlines(), txt[k].splitlines()
        assert len(a) == len(b)
        for x, y in zip(a, b):
            m = re.search(r";FP:(-?\d+);RQ:", x)
            if m and x.startswith("@"):
                n_tags += 1
                assert y == x.replace(";FP:" + m.group(1) + ";", ";FP:" + tdlib.fingerprint_text(int(m.group(1))) + ";")
                assert re.fullmatch(r"[ACGT]+", tdlib.fingerprint_text(int(m.group(1))))
            else:
                assert x == y
    assert n_tags > 50


def make_reads(L, n=400, seed=3):
    """n FASTQ records barcode + L-base fingerprint + read (a few of them random)"""
    rng = np.random.default_rng(seed + L)
    out = []
    for i in range(n):
        if rng.random() < 0.05:
            s = "".join("ACGT"[b] for b in rng.integers(0, 4, 60))
        else:
            s = BARCODES[int(rng.integers(0, 3))] + "".join("ACGT"[b] for b in rng.integers(0, 4, L + 40))
        out.append("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    return "".join(out)


def _tags(d, prefix):
    """{(file suffix, read name): FP tag} over a run's FASTQ outputs, and the records without their FP tags"""
    tags, rest = {}, {}
    for p in sorted(glob.glob(os.path.join(d, prefix + "*.fq"))):
        lines = open(p).read().splitlines()
        suffix = os.path.basename(p)[len(prefix):]
        for j in range(0, len(lines), 4):
            m = re.fullmatch(r"@(.*?)(?:;FP:([^;]*))?;RQ:(.*)", lines[j])
            assert m, lines[j]
            if m.group(2) is not None:
                tags[(suffix, m.group(1))] = m.group(2)
            rest[(suffix, m.group(1))] = (m.group(3), lines[j + 1], lines[j + 3])
    return tags, rest


@pytest.mark.skipif(not os.path.exists(os.path.join(RBIN, "tagdust_rtest")), reason="oracle/_ref/tagdust_rtest not built")
@pytest.mark.parametrize("L", [4, 12, 14])
def test_against_the_reference_binary(tmp_path, L):
    d = str(tmp_path)
    open(os.path.join(d, "in.fq"), "w").write(make_reads(L))
    args = ["-seed", "42", "-Q", "20", "-1", "B:" + ",".join(BARCODES), "-2", "F:" + "N" * L, "-3", "R:N", "in.fq"]
    for extra, prefix in (([], "num"), (["-show_finger_seq"], "txt")):
        p = subprocess.run([os.path.join(RBIN, "tagdust_rtest")] + args + extra + ["-o", prefix], cwd=d, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, timeout=300)
        assert p.returncode == 0, p.stdout.decode(errors="replace")[-2000:]
    num, num_rest = _tags(d, "num")
    txt, txt_rest = _tags(d, "txt")
    assert num_rest == txt_rest and set(num) == set(txt) and len(num) > 300
    for k in num:
        assert tdlib.fingerprint_text(int(num[k])) == txt[k], (k, num[k], txt[k])
        assert len(txt[k]) == L
    negative = sum(int(v) < 0 for v in num.values())
    print("L", L, "records", len(num), "negative fingerprints", negative)
    assert (negative > 0) == (L >= 12)       # (bases << 8 reaches the int's sign bit from 12 bases on; from 13 on leading bases are lost)
