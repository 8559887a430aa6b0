"""The merge kernel (csrc/td_merge.hip) against the host path, which tests/test_merge.py holds against the reference's output:
every field of every record and every output byte, on the fixtures and on generated pairs that sit where a kernel of this shape
can go wrong.  Then td_merge_stream and the command on the device against the recorded files."""
import os
import random
import subprocess

import numpy as np
import pytest

from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "merge")
RUNS = [("merged_default.fq", 16, 0.0), ("merged_Q0.9_minlen20.fq", 20, 0.9)]
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}


@pytest.fixture(scope="module")
def library():
    tdbuild.build()
    return tdlib.load_library()


def read(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


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


def texts(pairs):
    t1 = "".join("@p%d\n%s\n+\n%s\n" % (i, a[0], a[1]) for i, (a, b) in enumerate(pairs))
    t2 = "".join("@p%d\n%s\n+\n%s\n" % (i, b[0], b[1]) for i, (a, b) in enumerate(pairs))
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


Q60 = "".join(chr(c) for c in range(35, 95))
BATCHES = {
    "edges": edge_pairs,
    "one_pair": lambda: random_pairs(1, "#5AF", 11),
    "q4_193_pairs": lambda: random_pairs(64 * 3 + 1, "#5AF", 12),
    "q60": lambda: random_pairs(40, Q60, 13),
    "q52_wide_staging": lambda: random_pairs(20, Q60[:52], 14),         # 5 * 52 = 260: the first table that needs 16-bit staging
}
_cache = {}


def batch(name, min_overlap=16, threshold=0.0):
    """(read 1, read 2, the host path's result), made once"""
    key = (name, min_overlap, threshold)
    if key not in _cache:
        t1, t2 = texts(BATCHES[name]()) if name in BATCHES else (read("r1.fq"), read("r2.fq"))
        r1, r2 = tdlib.ParsedReads(t1), tdlib.ParsedReads(t2)
        _cache[key] = (r1, r2, tdlib.merge_batch(r1, r2, None, min_overlap=min_overlap, threshold=threshold, n_threads=4))
    return _cache[key]


def assert_same(dev, host):
    for f in ("best_d", "out_len", "id", "aligned", "status"):
        assert np.array_equal(dev["rec"][f], host["rec"][f]), (f, np.nonzero(dev["rec"][f] != host["rec"][f])[0][:8].tolist())
    assert np.array_equal(dev["out_off"], host["out_off"])
    for p in range(len(host["rec"])):
        o, n = int(host["out_off"][p]), int(host["rec"]["out_len"][p])
        assert dev["seq"][o:o + n].tobytes() == host["seq"][o:o + n].tobytes(), p
        assert dev["qual"][o:o + n].tobytes() == host["qual"][o:o + n].tobytes(), p
    for f in ("n_written", "n_below", "n_too_short"):
        assert dev[f] == host[f]


@pytest.mark.parametrize("name,min_overlap,threshold", [("fixtures", 16, 0.0), ("fixtures", 20, 0.9), ("edges", 16, 0.0),
                                                        ("edges", 16, 0.95), ("one_pair", 16, 0.0), ("q52_wide_staging", 16, 0.0)])
def test_device_equals_host(library, name, min_overlap, threshold):
    r1, r2, host = batch(name, min_overlap, threshold)
    dev = tdlib.merge_batch(r1, r2, 0, min_overlap=min_overlap, threshold=threshold)
    assert_same(dev, host)
    if name == "edges":
        # 27 pairs: 3 without a candidate whatever the threshold; the other 24 are all written at threshold 0 (id / aligned >= 0
        # always holds), and at 0.95 the well-matching ones are written and the unrelated / all-N ones fall below
        assert dev["n_on_host"] == 2 and host["n_too_short"] == 3 and host["n_written"] + host["n_below"] == 24
        if threshold == 0.0:
            assert host["n_below"] == 0
        else:
            assert host["n_written"] > 0 and host["n_below"] > 0
        assert int(host["rec"]["best_d"][20]) == 0 and int(host["rec"]["best_d"][21]) == 0      # the all-tie pairs


@pytest.mark.parametrize("name,placement", [("q4_193_pairs", tdlib.MERGE_TABLE_LDS), ("q4_193_pairs", tdlib.MERGE_TABLE_GLOBAL),
                                            ("q4_193_pairs", tdlib.MERGE_TABLE_AUTO), ("q60", tdlib.MERGE_TABLE_GLOBAL),
                                            ("q60", tdlib.MERGE_TABLE_AUTO)])
def test_table_in_lds_and_in_global_memory(library, name, placement):
    r1, r2, host = batch(name)
    dev = tdlib.merge_batch(r1, r2, 0, table_placement=placement)
    assert_same(dev, host)
    fits = name == "q4_193_pairs"
    assert dev["table_in_lds"] == (1 if fits and placement != tdlib.MERGE_TABLE_GLOBAL else 0)


def test_table_that_does_not_fit_lds_is_refused_there(library):
    r1, r2, _ = batch("q60")            # 300 x 300 floats
    with pytest.raises(tdlib.TdError, match="does not fit the LDS budget"):
        tdlib.merge_batch(r1, r2, 0, table_placement=tdlib.MERGE_TABLE_LDS)


@pytest.mark.parametrize("recorded,minlen,threshold", RUNS)
def test_stream_on_the_device_equals_reference_output(library, tmp_path, recorded, minlen, threshold):
    out = str(tmp_path / "m.fq")
    st = tdlib.merge_stream(os.path.join(GOLD, "r1.fq.gz"), os.path.join(GOLD, "r2.fq"), out, 0, min_overlap=minlen, threshold=threshold,
                            n_threads=2, batch_pairs=128)
    want = read(recorded)
    assert open(out, "rb").read() == want
    assert st["n_pairs"] == 300 and st["n_batches"] == 3 and st["n_written"] == want.count(b"\n") // 4 and st["kernel_s"] > 0.0


def test_command_on_the_device_and_on_the_host(library):
    for extra in ([], ["--host"]):
        r = subprocess.run([tdbuild.MERGE_EXE] + extra + ["-Q", "0.9", "-minlen", "20", os.path.join(GOLD, "r1.fq"), os.path.join(GOLD, "r2.fq")],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert r.returncode == 0, r.stderr
        assert r.stdout == read("merged_Q0.9_minlen20.fq")
