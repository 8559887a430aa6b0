"""The merge's yardsticks, no GPU.  tests/merge_plain.py restates the reference's overlap_reads() without any table or helper of
the code under test.  Here it is held against what the reference's `merge -t 1` wrote (tests/golden/merge/: the 300 pairs and
the edge fixtures, every recorded run), the host path is held against it in every field of every pair -- also where the output
text shows nothing (best_d; id and aligned of dropped pairs) and where the reference is undefined (no candidate, reads beyond
512 bases) -- and, where oracle/_ref/merge is built, host path, restatement and that binary are run on freshly generated pairs."""
import os
import subprocess

import pytest

import merge_cases as mc
import merge_plain as mp
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden", "merge")
REF_MERGE = os.path.join(REPO, "oracle", "_ref", "merge")
RECORDED = [("r1.fq", "r2.fq", "merged_default.fq", 16, 0.0), ("r1.fq", "r2.fq", "merged_Q0.9_minlen20.fq", 20, 0.9)] + \
           [("edge_r1.fq", "edge_r2.fq", out, minlen, threshold) for out, minlen, threshold, _ in mc.EDGE_RUNS]

SETS = {
    "edges": mc.edge_pairs,                                               # with the two pairs beyond 512 bases and the three without a candidate
    "boundary": mc.boundary_pairs,
    "q3": lambda: mc.random_pairs(300, "!~F", 22, 17, 90),                # -inf cells and zero probabilities: 123 pairs have no finite candidate
    "q94": lambda: mc.random_pairs(60, mc.Q94, 23, 17, 90),
    "q94_200": lambda: mc.random_pairs(200, mc.Q94, 25, 17, 90),
    "nrich": lambda: mc.n_rich(mc.random_pairs(200, "#5AF", 24, 17, 90)),
    "short": lambda: mc.random_pairs(200, "#5AF", 26, 1, 60),             # reads from one base up: min_overlap 0, 1 and 30 all cut into them
}
_pairs, _plain = {}, {}


def pairs_of(name):
    if name not in _pairs:
        _pairs[name] = SETS[name]()
    return _pairs[name]


def plain_of(name, min_overlap, threshold):
    """the restatement's result for a set, made once"""
    key = (name, min_overlap, threshold)
    if key not in _plain:
        _plain[key] = [mp.merge_pair(a[0], a[1], b[0], b[1], min_overlap, threshold) for a, b in pairs_of(name)]
    return _plain[key]


@pytest.fixture(scope="module")
def library():
    tdbuild.build()
    return tdlib.load_library()


def read(name):
    with open(os.path.join(GOLD, name), "rb") as f:
        return f.read()


def host_merged(res, p):
    """record p of a merge_batch result as merge_plain.Merged (sequence and qualities as far as they were written)"""
    rec, o = res["rec"][p], int(res["out_off"][p])
    n = int(rec["out_len"])
    return mp.Merged(int(rec["best_d"]), n, int(rec["id"]), int(rec["aligned"]), int(rec["status"]),
                     res["seq"][o:o + n].tobytes().decode(), res["qual"][o:o + n].tobytes().decode())


def assert_equals_plain(res, plain, where=None):
    """every field of every pair (of the pairs `where`): best_d, out_len, id, aligned, status, sequence, qualities"""
    for p in range(len(plain)) if where is None else where:
        m = plain[p]
        assert host_merged(res, p) == m._replace(seq=m.seq[:m.out_len], qual=m.qual[:m.out_len]), p


def test_status_numbers_are_the_library_s():
    assert (mp.WRITTEN, mp.BELOW, mp.NO_CANDIDATE) == (tdlib.MERGE_WRITTEN, tdlib.MERGE_BELOW, tdlib.MERGE_NO_CANDIDATE)


@pytest.mark.parametrize("in1,in2,recorded,minlen,threshold", RECORDED, ids=[r[2] for r in RECORDED])
def test_restatement_equals_recorded_reference_output(in1, in2, recorded, minlen, threshold):
    recs1, recs2 = mp.parse_fastq(read(in1)), mp.parse_fastq(read(in2))
    plain = mp.merge_records(recs1, recs2, minlen, threshold)
    # the recorded runs lie in the reference's defined domain, all of them
    assert all(mp.in_reference_domain(len(a[1]), len(b[1]), minlen, m.best_d) for a, b, m in zip(recs1, recs2, plain))
    assert mp.text([r[0] for r in recs1], plain) == read(recorded)


def test_edge_fixtures_hold_the_generated_sets_inside_the_defined_domain():
    names, pairs = [], []
    for prefix, make in mc.FIXTURE_SETS:
        made = make()
        kept = [k for k, (a, b) in enumerate(made)
                if mp.in_reference_domain(len(a[0]), len(b[0]), 16, mp.merge_pair(a[0], a[1], b[0], b[1], 16, 0.0).best_d)]
        if prefix == "edge":                # all but the two beyond 512 bases and the three without a candidate
            assert [k for k in range(len(made)) if k not in kept] == [14, 15, 23, 25, 26]
        if prefix == "bound":
            assert kept == list(range(8))
        assert 2 * len(kept) >= len(made)
        names += ["%s%d" % (prefix, k) for k in kept]
        pairs += [made[k] for k in kept]
    t1, t2 = mc.texts(pairs, names)
    assert t1 == read("edge_r1.fq") and t2 == read("edge_r2.fq")


def test_boundary_pairs_sit_exactly_at_their_thresholds():
    for k, (a, b) in enumerate(mc.boundary_pairs()):
        bases, mismatches, threshold, _ = mc.BOUNDARY[k // 2]
        m = mp.merge_pair(a[0], a[1], b[0], b[1], 16, threshold)
        assert (m.best_d, m.id, m.aligned) == (0, bases - mismatches - k % 2, bases)
        assert m.status == (mp.WRITTEN if k % 2 == 0 else mp.BELOW)


HOST_CASES = [("edges", 16, t) for t in mc.THRESHOLDS] + [("boundary", 16, t) for t in mc.THRESHOLDS] + \
             [("q3", 16, 0.0), ("q3", 16, 0.9), ("q94", 16, 0.0), ("q94", 20, 0.9), ("nrich", 16, 0.0), ("nrich", 16, 0.7),
              ("short", 0, 0.0), ("short", 1, 0.75), ("short", 30, 0.9), ("edges", 0, 0.0), ("edges", 1, 0.0), ("edges", 30, 0.9)]


@pytest.mark.parametrize("name,min_overlap,threshold", HOST_CASES)
def test_host_equals_restatement_in_every_field(library, name, min_overlap, threshold):
    pairs = pairs_of(name)
    t1, t2 = mc.texts(pairs)
    r1, r2 = tdlib.ParsedReads(t1), tdlib.ParsedReads(t2)
    res = tdlib.merge_batch(r1, r2, None, min_overlap=min_overlap, threshold=threshold, n_threads=2)
    plain = plain_of(name, min_overlap, threshold)
    assert_equals_plain(res, plain)
    assert tdlib.merge_text(res, r1.names()) == mp.text(mc.names_of(pairs), plain)
    status = [m.status for m in plain]
    assert (res["n_written"], res["n_below"], res["n_too_short"]) == tuple(status.count(s) for s in (mp.WRITTEN, mp.BELOW, mp.NO_CANDIDATE))
    # the sets reach what they are there for
    if name == "edges" and min_overlap == 16:
        assert status.count(mp.NO_CANDIDATE) == 3 and plain[20].best_d == 0 and plain[21].best_d == 0 and plain[19].best_d == 0
    if name == "q3":
        assert 100 < status.count(mp.NO_CANDIDATE) < 200
    if name == "short":
        assert (status.count(mp.NO_CANDIDATE) > 0) == (min_overlap > 0) and status.count(mp.NO_CANDIDATE) < len(pairs)
    if threshold > 0.0 and name != "q3":            # (over "!~F" the best candidate is rarely the true overlap)
        assert status.count(mp.WRITTEN) > 0 and status.count(mp.BELOW) > 0


LIVE_CASES = [("edges+boundary", 16, 0.95), ("q3", 16, 0.0), ("q94_200", 20, 0.9), ("q94_200", 30, 0.7), ("nrich", 16, 0.75),
              ("short", 0, 0.0), ("short", 1, 0.0)]


@pytest.mark.parametrize("name,min_overlap,threshold", LIVE_CASES)
def test_host_and_restatement_equal_the_reference_binary(library, tmp_path, name, min_overlap, threshold):
    if not os.path.exists(REF_MERGE):
        pytest.skip("reference binary not built (oracle/_ref is only built where the reference sources exist)")
    made = [pair for part in name.split("+") for pair in pairs_of(part)]
    plain = [m for part in name.split("+") for m in plain_of(part, min_overlap, threshold)]
    kept = [k for k, ((a, b), m) in enumerate(zip(made, plain)) if mp.in_reference_domain(len(a[0]), len(b[0]), min_overlap, m.best_d)]
    # the filter must not hide a failure: at least half of every set is inside the reference's defined domain
    assert 2 * len(kept) >= len(made)
    pairs, names = [made[k] for k in kept], ["p%d" % k for k in kept]
    t1, t2 = mc.texts(pairs, names)
    p1, p2 = str(tmp_path / "r1.fq"), str(tmp_path / "r2.fq")
    for path, text in ((p1, t1), (p2, t2)):
        with open(path, "wb") as f:
            f.write(text)
    r = subprocess.run([REF_MERGE, "-t", "1", "-minlen", str(min_overlap), "-Q", repr(threshold), p1, p2],
                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, timeout=120)
    assert r.returncode == 0
    assert mp.text(names, [plain[k] for k in kept]) == r.stdout
    r1, r2 = tdlib.ParsedReads(t1), tdlib.ParsedReads(t2)
    res = tdlib.merge_batch(r1, r2, None, min_overlap=min_overlap, threshold=threshold, n_threads=2)
    assert tdlib.merge_text(res, r1.names()) == r.stdout
