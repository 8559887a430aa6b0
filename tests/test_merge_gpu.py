"""The merge kernel (csrc/td_merge.hip): every field of every record and every output byte against the host path on the fixtures
and on generated pairs that sit where a kernel of this shape can go wrong; on the edge shapes and the threshold-boundary pairs
also against the plain restatement of tests/merge_plain.py (which shares no table and no helper with either path) and against
what the reference wrote for them (tests/golden/merge/edge_*); a batch of more than two sweeps of the capped grid; the LDS
budget's edge; a stream whose batches change table placement and staging width.  Then td_merge_stream and the command on the
device against the recorded files.  tests/test_merge_reference.py holds the host path and the restatement against the reference."""
import os
import random
import subprocess

import numpy as np
import pytest
import torch     # before the library is loaded: where torch brings a HIP runtime of its own, only the first one loaded sees the device

import merge_plain as mp
from merge_cases import BOUNDARY, EDGE_RUNS, Q60, THRESHOLDS, boundary_pairs, edge_pairs, names_of, overlapping, random_pairs, texts
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

pytestmark = pytest.mark.gpu

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


BATCHES = {
    "edges": edge_pairs,
    "boundary": boundary_pairs,
    "one_pair": lambda: random_pairs(1, "#5AF", 11),
    "q4_193_pairs": lambda: random_pairs(64 * 3 + 1, "#5AF", 12),
    "q60": lambda: random_pairs(40, Q60, 13),
    "q52_wide_staging": lambda: random_pairs(20, Q60[:52], 14),         # 5 * 52 = 260: the first table that needs 16-bit staging
    "q18_fits_lds": lambda: random_pairs(40, Q60[:18], 15, 17, 90),      # 90 x 90 floats = 32400 bytes: the largest table inside the 32 KiB budget
    "q19_does_not": lambda: random_pairs(40, Q60[:19], 16, 17, 90),      # 95 x 95 floats = 36100 bytes: the first beyond it
}
FIXTURE_PREFIX = {"edges": "edge", "boundary": "bound"}                  # the names of these batches' pairs in tests/golden/merge/edge_*
_cache, _plain, _pairs = {}, {}, {}


def pairs_of(name):
    if name not in _pairs:
        _pairs[name] = BATCHES[name]()
    return _pairs[name]


def plain(name, min_overlap, threshold):
    """the restatement's result for a batch, made once"""
    key = (name, min_overlap, threshold)
    if key not in _plain:
        _plain[key] = [mp.merge_pair(a[0], a[1], b[0], b[1], min_overlap, threshold) for a, b in pairs_of(name)]
    return _plain[key]


def batch(name, min_overlap=16, threshold=0.0):
    """(read 1, read 2, the host path's result), made once"""
    key = (name, min_overlap, threshold)
    if key not in _cache:
        t1, t2 = texts(pairs_of(name)) if name in BATCHES else (read("r1.fq"), read("r2.fq"))
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


def merged(res, p):
    """record p of a merge_batch result as merge_plain.Merged (sequence and qualities as far as they were written)"""
    rec, o = res["rec"][p], int(res["out_off"][p])
    n = int(rec["out_len"])
    return mp.Merged(int(rec["best_d"]), n, int(rec["id"]), int(rec["aligned"]), int(rec["status"]),
                     res["seq"][o:o + n].tobytes().decode(), res["qual"][o:o + n].tobytes().decode())


def assert_equals_plain(res, want, where):
    """pairs `where` of a merge_batch result against the restatement's `want[p]`, every field"""
    for p in where:
        m = want[p]
        assert merged(res, p) == m._replace(seq=m.seq[:m.out_len], qual=m.qual[:m.out_len]), p


def recorded_records(threshold):
    """{name: (sequence, qualities)} of what the reference wrote for the edge fixtures at this threshold"""
    out = [r[0] for r in EDGE_RUNS if r[2] == threshold]
    return {name: (seq, qual) for name, seq, qual in mp.parse_fastq(read(out[0]))}


@pytest.mark.parametrize("name,min_overlap,threshold", [("fixtures", 16, 0.0), ("fixtures", 20, 0.9), ("one_pair", 16, 0.0), ("q52_wide_staging", 16, 0.0)] +
                         [("edges", 16, t) for t in THRESHOLDS] + [("boundary", 16, t) for t in THRESHOLDS])
def test_device_equals_host(library, name, min_overlap, threshold):
    r1, r2, host = batch(name, min_overlap, threshold)
    dev = tdlib.merge_batch(r1, r2, 0, min_overlap=min_overlap, threshold=threshold)
    assert_same(dev, host)
    if name in FIXTURE_PREFIX:
        # host and kernel share td_merge_better / _pick / _passes and the table T: the restatement and the reference's recorded
        # bytes share none of them
        pairs, want = pairs_of(name), plain(name, min_overlap, threshold)
        assert_equals_plain(dev, want, range(len(pairs)))
        recorded, n_recorded = recorded_records(threshold), 0
        for p, ((a, b), m) in enumerate(zip(pairs, want)):
            fixture_name = "%s%d" % (FIXTURE_PREFIX[name], p)
            if mp.in_reference_domain(len(a[0]), len(b[0]), min_overlap, m.best_d) and m.out_len:
                got = merged(dev, p)
                assert recorded[fixture_name] == (got.seq, got.qual), p
                n_recorded += 1
            else:
                assert fixture_name not in recorded         # dropped by the reference too, or outside its defined domain
        assert n_recorded > 0
    if name == "boundary":
        # id / aligned equals the threshold exactly in the first pair of its two, which is written, and not in its twin
        for k, (bases, mismatches, t, _) in enumerate(BOUNDARY):
            at, worse = dev["rec"][2 * k], dev["rec"][2 * k + 1]
            assert (int(at["best_d"]), int(at["id"]), int(at["aligned"])) == (0, bases - mismatches, bases)
            assert (int(worse["best_d"]), int(worse["id"]), int(worse["aligned"])) == (0, bases - mismatches - 1, bases)
            if t == threshold:
                assert at["status"] == tdlib.MERGE_WRITTEN and worse["status"] == tdlib.MERGE_BELOW
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


def test_the_lds_budget_s_edge(library):
    # 18 quality characters: dim 90, 32400 bytes, the largest table inside the budget; 19: dim 95, 36100 bytes, the first beyond
    r1, r2, host = batch("q18_fits_lds")
    assert len(set("".join(a[1] + b[1] for a, b in pairs_of("q18_fits_lds")))) == 18
    for placement in (tdlib.MERGE_TABLE_AUTO, tdlib.MERGE_TABLE_LDS):
        dev = tdlib.merge_batch(r1, r2, 0, table_placement=placement)
        assert dev["table_in_lds"] == 1
        assert_same(dev, host)
    r1, r2, host = batch("q19_does_not")
    assert len(set("".join(a[1] + b[1] for a, b in pairs_of("q19_does_not")))) == 19
    dev = tdlib.merge_batch(r1, r2, 0, table_placement=tdlib.MERGE_TABLE_AUTO)
    assert dev["table_in_lds"] == 0
    assert_same(dev, host)
    with pytest.raises(tdlib.TdError, match="does not fit the LDS budget"):
        tdlib.merge_batch(r1, r2, 0, table_placement=tdlib.MERGE_TABLE_LDS)


def test_more_than_two_sweeps_of_the_capped_grid(library):
    # The grid is capped at 8 blocks of four pairs per CU and strides over the batch.  Two full sweeps and five pairs: every block
    # stages its reads over those of the trip before, and in the last trip block 0 holds four pairs, block 1 one pair and three
    # waves without one, every other block none.
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count          # what the kernel's host side reads
    n = 2 * 32 * n_cu + 5
    rng = random.Random(41)
    pairs, n_long, n_short = [], 0, 0
    for p in range(n):
        lf, lr = rng.randint(17, 40), rng.randint(17, 40)
        kind = rng.randrange(500)
        if kind == 0:                                   # beyond the staging room: skipped by the kernel, done by the host
            lf, lr, n_long = (600, lr, n_long + 1) if p % 2 else (lf, 600, n_long + 1)
        elif kind == 1:                                 # no candidate
            lf, lr, n_short = (16, lr, n_short + 1) if p % 2 else (lf, 16, n_short + 1)
        pairs.append(overlapping(rng, lf, lr, "#5AF"))
    assert n_long > 0 and n_short > 0
    t1, t2 = texts(pairs)
    r1, r2 = tdlib.ParsedReads(t1), tdlib.ParsedReads(t2)
    host = tdlib.merge_batch(r1, r2, None, n_threads=8)
    dev = tdlib.merge_batch(r1, r2, 0)
    print("multi-sweep batch: n_cu = %d, %d pairs, %d on the host, %d without a candidate" % (n_cu, n, n_long, n_short))
    assert_same(dev, host)
    assert dev["n_on_host"] == n_long and dev["n_too_short"] == n_short and dev["table_in_lds"] == 1
    where = sorted(set(range(8)) | set(range(0, n, 97)) | set(range(2 * 32 * n_cu, n)))
    want = {p: mp.merge_pair(pairs[p][0][0], pairs[p][0][1], pairs[p][1][0], pairs[p][1][1], 16, 0.0) for p in where}
    assert_equals_plain(dev, want, where)


def test_stream_whose_batches_change_table_placement_and_staging_width(library, tmp_path):
    # one device handle, batches of 64 pairs: four characters (table in LDS, 8-bit staging); 52 characters and reads twice as long
    # (table in global memory, 16-bit staging, every device buffer regrows); four characters and short reads again; 19 characters
    # (8-bit staging, the first table beyond the LDS budget), a batch that is not full
    Q52 = Q60[:52]
    pairs = random_pairs(64, "#5AF", 51, 17, 80) + random_pairs(64, Q52, 52, 120, 160) + random_pairs(64, "#5AF", 53, 17, 40) + \
        random_pairs(37, Q60[:19], 54, 17, 90)
    assert len(set("".join(a[1] + b[1] for a, b in pairs[64:128]))) == 52 and len(set("".join(a[1] + b[1] for a, b in pairs[192:]))) == 19
    names = names_of(pairs)
    t1, t2 = texts(pairs, names)
    p1, p2 = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")
    for path, text in ((p1, t1), (p2, t2)):
        with open(path, "wb") as f:
            f.write(text)
    out_dev, out_host = str(tmp_path / "dev.fq"), str(tmp_path / "host.fq")
    st = tdlib.merge_stream(p1, p2, out_dev, 0, n_threads=2, batch_pairs=64)
    tdlib.merge_stream(p1, p2, out_host, None, n_threads=2, batch_pairs=64)
    assert st["n_pairs"] == len(pairs) and st["n_batches"] == 4
    with open(out_dev, "rb") as f:
        got = f.read()
    with open(out_host, "rb") as f:
        assert got == f.read()
    assert got == mp.text(names, [mp.merge_pair(a[0], a[1], b[0], b[1], 16, 0.0) for a, b in pairs])


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
