"""The molecule count on the device (include/tagdust_molecules.h, tagdust_amd/csrc/td_molecules.hip).  The yardstick is td_mol_host
fed with the CPU oracle's labels, outcomes, barcodes and fingerprints for the same reads (oracle/pyoracle.py), never with the
device's own output.  Reads are sampled with replacement from 240 synthetic molecules (a barcode, a UMI, a read) with 2 %
substitutions, 1200 to a batch.  The table has 2^16 slots unless noted: more than 50 times the reads, so the yardstick's
overflow of 0 holds for the device."""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden, golden_artifacts

pytestmark = pytest.mark.gpu

BARCODES = ["TTGTGT", "AAACCC", "AAGGGA", "ACTTCA", "CAGTAC", "CCTAGG", "GATCTC", "GGCATA"]
EXE = os.path.join(REPO, "tagdust_amd", "bin", "tagdust-hip")
RBIN = os.path.join(REPO, "oracle", "_ref")
N_MOL, N_READS = 240, 1200

SHAPES = {
    # barcode of 6 + UMI of 5: the read starts at base 11, a prefix of 32 crosses two 16-base words and the 32-bit N-mask boundary
    "b_f_r": ["B:" + ",".join(BARCODES), "F:NNNNN", "R:N"],
    "r_s_b_f": ["R:N", "S:GTCA", "B:" + ",".join(BARCODES), "F:NNNN"],
    "f_r": ["F:NNNNNN", "R:N"],
    "b_r": ["B:" + ",".join(BARCODES), "R:N"],
}
MINLEN = {"r_s_b_f": 8}
THRESHOLD = {"f_r": 1.0}       # (an architecture without one fixed base tells a read from noise by its length alone: Q is about 3)


def code(s):
    return np.array([b"ACGTN".index(c) for c in s.encode()], np.uint8)


def pairs(entries):
    return [(int(k), int(c)) for k, c in zip(entries["key"], entries["count"])]


def pack(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), offs


def make_reads(shape, seed):
    """N_READS reads drawn with replacement from N_MOL molecules; every base substituted with probability 0.02.  In r_s_b_f the
    read comes first and is 10..40 bases long; one read in twelve there gets an N at read base 3 (inside every prefix) or at read
    base 8 (just behind a prefix of 8)."""
    rng = np.random.default_rng(seed)
    mols = []
    for _ in range(N_MOL):
        bar = code(BARCODES[int(rng.integers(0, len(BARCODES)))])
        if shape == "b_f_r":
            m = [bar, rng.integers(0, 4, 5), rng.integers(0, 4, int(rng.integers(30, 101)))]
        elif shape == "r_s_b_f":
            m = [rng.integers(0, 4, int(rng.integers(10, 41))), code("GTCA"), bar, rng.integers(0, 4, 4)]
        elif shape == "f_r":
            m = [rng.integers(0, 4, 6), rng.integers(0, 4, int(rng.integers(30, 101)))]
        else:
            m = [bar, rng.integers(0, 4, int(rng.integers(30, 101)))]
        mols.append(np.concatenate(m).astype(np.uint8))
    reads = []
    for _ in range(N_READS):
        r = mols[int(rng.integers(0, N_MOL))].copy()
        hit = rng.random(len(r)) < 0.02
        r[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
        if shape == "r_s_b_f" and rng.random() < 1 / 12:
            r[3 if rng.random() < 0.5 else 8] = 4
        reads.append(r)
    return pack(reads)


_CASES = {}


def case(shape, seed=5):
    """(model, seq, offs, threshold, minlen, the oracle's records and labels), computed once"""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    key = (shape, seed)
    if key not in _CASES:
        seq, offs = make_reads(shape, seed)
        md, _ = tdlib.build_model(SHAPES[shape], seq, offs)
        thr, minlen = THRESHOLD.get(shape, 5.0), MINLEN.get(shape, 16)
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, minlen, 100, 2)
        res = {f: np.asarray(ores[f]).copy() for f in ("read_type", "barcode", "fingerprint")}
        _CASES[key] = (md, seq, offs, thr, minlen, res, olab)
    return _CASES[key]


def yardstick(c, P, lo=0, hi=None):
    """td_mol_host over reads lo..hi of a case with the oracle's labels and records"""
    from tagdust_amd import lib as tdlib
    md, seq, offs, _, _, res, lab = c
    hi = len(offs) - 1 if hi is None else hi
    return tdlib.mol_host(md, seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo], {f: v[lo:hi] for f, v in res.items()},
                          lab[offs[lo] + lo:offs[hi] + hi], P)


def check_main_case(c, want, want_tot):
    """what every main case asserts on the oracle's side before the device is compared"""
    n = len(c[2]) - 1
    print("yardstick totals", want_tot)
    assert want_tot["eligible"] >= 0.8 * n
    assert want_tot["molecules"] < 0.7 * want_tot["counted"]
    assert want_tot["overflow"] == 0


def check_identities(ent, tot):
    assert tot["eligible"] == tot["counted"] + tot["skipped_empty"] + tot["skipped_n"] + tot["overflow"]
    assert tot["counted"] == int(ent["count"].sum()) and tot["molecules"] == len(ent)


@pytest.fixture()
def ctx():
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", 0)
    yield c
    c.close()


def start(ctx, c, P, log2_slots=16):
    md, _, _, thr, minlen, _, _ = c
    ctx.upload_model(md)
    ctx.set_params(thr, minlen, 100)
    ctx.mol_enable(P, log2_slots)


def run_batch(ctx, c, lo=0, hi=None):
    _, seq, offs = c[:3]
    hi = len(offs) - 1 if hi is None else hi
    ctx.upload_batch(seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo])
    ctx.run()


# ---- 1, 2, 3: the main cases ----
MAIN = [("b_f_r", 1), ("b_f_r", 16), ("b_f_r", 32), ("r_s_b_f", 8), ("r_s_b_f", 32), ("f_r", 20), ("b_r", 20)]


@pytest.mark.parametrize("shape,P", MAIN, ids=["%s-P%d" % sp for sp in MAIN])
def test_equals_the_yardstick_on_a_ragged_batch(ctx, shape, P):
    c = case(shape)
    want, want_tot = yardstick(c, P)
    check_main_case(c, want, want_tot)
    res = c[5]
    ok = (res["read_type"] & 0xFF) == 0
    if shape == "r_s_b_f":
        assert want_tot["skipped_n"] > 10                      # N at read base 3
        lens = np.diff(c[2])
        assert int((lens - 14 < 32).sum()) > 500 and int((lens - 14 >= 32).sum()) > 100   # read bases 10..40: n < P for most at P = 32
        if P == 8:                                             # N at read base 8 is behind the prefix: such reads count
            n8 = [i for i in np.flatnonzero(ok) if c[1][c[2][i] + 8] == 4 and c[1][c[2][i] + 3] != 4]
            assert len(n8) > 10
    if shape == "f_r":
        assert set(k >> 56 for k, _ in pairs(want)) == {0} and bool((res["barcode"][ok] == -1).all())
    if shape == "b_r":
        assert bool((res["fingerprint"][ok] == -1).all()) and len(set(k >> 56 for k, _ in pairs(want))) > 3
    if shape == "b_f_r":
        assert bool((res["fingerprint"][ok] != -1).all())
    start(ctx, c, P)
    run_batch(ctx, c)
    ent, tot = ctx.mol_entries()
    print(shape, P, "device totals   ", tot)
    assert tot == want_tot
    assert pairs(ent) == pairs(want)
    check_identities(ent, tot)
    dres, labels, _ = ctx.download()                           # the batch itself is what it is without a count
    assert np.array_equal(dres["read_type"], res["read_type"]) and np.array_equal(labels, c[6])
    assert np.array_equal(dres["barcode"], res["barcode"]) and np.array_equal(dres["fingerprint"], res["fingerprint"])
    top, _ = ctx.mol_entries(cap=3)
    assert pairs(top) == pairs(want)[:3]


def test_n_behind_the_prefix_still_counts():
    """(what case 2 is made for, checked on the yardstick alone: a prefix of 8 skips fewer reads for N than a prefix of 32)"""
    c = case("r_s_b_f")
    t8, t32 = yardstick(c, 8)[1], yardstick(c, 32)[1]
    assert 0 < t8["skipped_n"] < t32["skipped_n"] and t8["counted"] > t32["counted"]


# ---- 4: behind the specialised kernel ----
def test_behind_the_specialised_kernel_and_with_length_classes():
    """the b_f_r architecture through its specialised kernel (one compile): the case's batch, then 4096 reads -- the case's reads
    over and over and one 1000-base read among them, so that the long tile gets wave slots of its own geometry while the labels
    keep the stride of the batch's longest read"""
    from oracle import pyoracle
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    c = case("b_f_r")
    md, seq, offs, thr, minlen, res, lab = c
    P = 32
    want, want_tot = yardstick(c, P)
    check_main_case(c, want, want_tot)
    n0 = len(offs) - 1
    rng = np.random.default_rng(9)
    long_read = np.concatenate([code(BARCODES[2]), rng.integers(0, 4, 994, dtype=np.uint8)])
    lseq, loffs = pack([long_read])
    lres, llab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), lseq, loffs, thr, minlen, 100, 2)
    idx = list(np.arange(4095) % n0)
    reads = [seq[offs[i]:offs[i + 1]] for i in idx]
    labs = [lab[offs[i] + i:offs[i + 1] + i + 1] for i in idx]
    recs = {f: [res[f][i] for i in idx] for f in res}
    at = 1700
    reads.insert(at, long_read); labs.insert(at, llab)
    for f in recs:
        recs[f].insert(at, lres[f][0])
    bseq, boffs = pack(reads)
    big_want, big_tot = tdlib.mol_host(md, bseq, boffs, {f: np.array(v) for f, v in recs.items()}, np.concatenate(labs).astype(np.int8), P)
    assert big_tot["overflow"] == 0 and big_tot["eligible"] >= 0.8 * 4096 and big_tot["molecules"] < 0.7 * big_tot["counted"]
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 1)
        ctx.set_option("async_compile", 0)
        start(ctx, c, P)
        assert ctx.get_option("spec_state") >= 0 and ctx.get_option("specialize") == 1
        before = ctx.get_option("spec_batches_generic")
        run_batch(ctx, c)
        assert ctx.get_option("spec_batches_generic") == before     # the specialised kernel decoded it
        ent, tot = ctx.mol_entries()
        assert tot == want_tot and pairs(ent) == pairs(want)
        ctx.mol_reset()
        ctx.upload_batch(bseq, boffs)
        assert ctx.get_option("length_classes") > 0
        ctx.run()
        assert ctx.get_option("spec_batches_generic") == before
        ent, tot = ctx.mol_entries()
        assert tot == big_tot and pairs(ent) == pairs(big_want)
    finally:
        ctx.close()


# ---- 5: accumulation ----
def test_accumulates_over_td_run_and_td_submit_and_resets(ctx):
    from tagdust_amd import RESULT_DTYPE
    c = case("b_f_r")
    _, seq, offs = c[:3]
    n = len(offs) - 1
    P = 16
    start(ctx, c, P)
    whole, whole_tot = yardstick(c, P)
    a, a_tot = yardstick(c, P, 0, 400)
    run_batch(ctx, c, 0, 400)
    ent, tot = ctx.mol_entries()
    assert pairs(ent) == pairs(a) and tot == a_tot
    ctx.counts_reset()                                  # the outcome counters are another matter
    assert ctx.mol_entries()[1] == a_tot
    run_batch(ctx, c, 400, n)
    ent, tot = ctx.mol_entries()
    assert pairs(ent) == pairs(whole) and tot == whole_tot
    # the same molecules again through three tickets in flight: counts add, no key is new
    parts = [(0, 300), (300, 650), (650, n)]
    res = [np.zeros(hi - lo, RESULT_DTYPE) for lo, hi in parts]
    tickets = [ctx.submit(np.ascontiguousarray(seq[offs[lo]:offs[hi]]), np.ascontiguousarray(offs[lo:hi + 1] - offs[lo]), res=r)
               for (lo, hi), r in zip(parts, res)]
    for t in tickets:
        ctx.wait(t)
    ent, tot = ctx.mol_entries()
    assert pairs(ent) == [(k, 2 * v) for k, v in pairs(whole)]
    assert tot == {f: (v if f == "molecules" else 2 * v) for f, v in whole_tot.items()}
    assert np.array_equal(np.concatenate([r["read_type"] for r in res]), c[5]["read_type"])
    ctx.mol_reset()
    ent, tot = ctx.mol_entries()
    assert len(ent) == 0 and not any(tot.values())
    run_batch(ctx, c, 0, 400)
    ent, tot = ctx.mol_entries()
    assert pairs(ent) == pairs(a) and tot == a_tot


# ---- 6: a table of 16 slots ----
def test_overflow_keeps_every_reported_count_exact(ctx):
    c = case("b_f_r")
    P = 16
    want, want_tot = yardstick(c, P)
    assert want_tot["molecules"] >= 64
    start(ctx, c, P, log2_slots=4)
    run_batch(ctx, c)
    run_batch(ctx, c)                                   # a key fails on every attempt or on none
    ent, tot = ctx.mol_entries()
    print("overflow totals", tot)
    assert tot["overflow"] > 0 and 0 < tot["molecules"] <= 16
    check_identities(ent, tot)
    ref = dict(pairs(want))
    assert all(k in ref and v == 2 * ref[k] for k, v in pairs(ent))
    assert tot["eligible"] == 2 * want_tot["eligible"] and tot["skipped_n"] == 2 * want_tot["skipped_n"]
    rows, rtot = ctx.mol_get()
    assert rtot == tot and int(rows["reads"].sum()) == tot["counted"] and int(rows["molecules"].sum()) == tot["molecules"]


# ---- 7: the device's summary ----
@pytest.mark.parametrize("shape", ["b_f_r", "f_r"])
def test_device_summary_equals_the_summary_of_the_entries(ctx, shape):
    from tagdust_amd import lib as tdlib
    c = case(shape)
    P = 16
    want, want_tot = yardstick(c, P)
    start(ctx, c, P)
    for _ in range(12):                                 # counts of 10 and more are met: the last level
        run_batch(ctx, c)
    rows, tot = ctx.mol_get()
    ent, tot2 = ctx.mol_entries()
    assert tot == tot2 and pairs(ent) == [(k, 12 * v) for k, v in pairs(want)]
    from_entries = tdlib.mol_summarise(ent)
    twelve = np.array([(k, 12 * v) for k, v in pairs(want)], tdlib.CENSUS_ENTRY_DTYPE)
    assert np.array_equal(rows, from_entries) and np.array_equal(rows, tdlib.mol_summarise(twelve))
    assert int(rows["levels"][:, 9].sum()) == tot["molecules"] > 0 and int(rows["reads"].sum()) == tot["counted"]
    if shape == "b_f_r":
        assert int((rows["reads"] > 0).sum()) == len(BARCODES) and not rows["reads"][len(BARCODES):].any()
    else:
        assert rows["reads"][0] == tot["counted"] and not rows["reads"][1:].any()
    ctx.mol_reset()
    run_batch(ctx, c)                                   # ... and the lower levels after one batch
    rows, tot = ctx.mol_get()
    assert np.array_equal(rows, tdlib.mol_summarise(want)) and int(rows["levels"][:, 0].sum()) > 0 and int(rows["levels"][:, 1:9].sum()) > 0


# ---- 8: two contexts ----
def test_two_contexts_on_one_device_merge_to_the_whole(ctx):
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    c = case("b_f_r")
    n = len(c[2]) - 1
    P = 32
    other = TagdustHip(0)
    try:
        other.set_option("specialize", 0)
        start(ctx, c, P)
        start(other, c, P)
        run_batch(ctx, c, 0, n // 2)
        run_batch(other, c, n // 2, n)
        a, ta = ctx.mol_entries()
        b, tb = other.mol_entries()
    finally:
        other.close()
    want, want_tot = yardstick(c, P)
    merged = tdlib.census_merge(a, b)
    assert pairs(merged) == pairs(want) and len(a) and len(b) and len(merged) < len(a) + len(b)
    assert all(ta[f] + tb[f] == want_tot[f] for f in tdlib.MOL_TOTALS if f != "molecules")
    assert np.array_equal(tdlib.mol_summarise(merged), tdlib.mol_summarise(want))


# ---- 9: -ref and DUST ----
@pytest.mark.parametrize("name", ["artifacts_b_r", "dust_b_r"])
def test_reads_the_filter_or_dust_rejects_are_not_counted(ctx, name):
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    g = load_golden(name)
    art = golden_artifacts(g)
    if art:
        ctx.set_artifacts(art[0], art[1], art[2], art[3])
    ctx.upload_model(g)
    ctx.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
    ctx.mol_enable(20, 16)
    ctx.upload_batch(g["seq"], g["offs"])
    ctx.run()
    ent, tot = ctx.mol_entries()
    ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(g), g["seq"], g["offs"], float(g["threshold"]), int(g["minlen"]), int(g["dust"]),
                                         art[3] if art else 2, artifacts=(art[0], art[1], art[2]) if art else None)
    assert np.array_equal(ores["read_type"], g["read_type"])
    want, want_tot = tdlib.mol_host(g, g["seq"], g["offs"], ores, olab, 20)
    low = np.asarray(g["read_type"]) & 0xFF
    assert want_tot["eligible"] == int((low == 0).sum()) > 0 and int(np.isin(low, [5, 6]).sum()) > 0
    assert tot == want_tot and pairs(ent) == pairs(want)


# ---- 10: what adds nothing, the refusals, the census beside it ----
def test_other_modes_and_arch_scores_add_nothing(ctx):
    from tagdust_amd import lib as tdlib
    c = case("b_f_r")
    md, seq, offs = c[:3]
    start(ctx, c, 16)
    hi = 200
    sub_seq, sub_offs = seq[:offs[hi]], offs[:hi + 1]
    for mode in (tdlib.MODE_GET_PROB, tdlib.MODE_ARCH_COMP, tdlib.MODE_RNA_DUST):
        ctx.upload_batch(sub_seq, sub_offs)
        ctx.run(mode)
        ctx.sync()
    ctx.arch_scores([md, case("b_r")[0]], sub_seq, sub_offs)
    ent, tot = ctx.mol_entries()
    assert len(ent) == 0 and not any(tot.values())
    run_batch(ctx, c, 0, hi)                            # ... and the count is still alive
    assert ctx.mol_entries()[1] == yardstick(c, 16, 0, hi)[1]


def test_a_context_without_the_count_behaves_as_before(ctx):
    from tagdust_amd import TdError
    c = case("b_f_r")
    md, _, _, thr, minlen, res, lab = c
    ctx.upload_model(md)
    ctx.set_params(thr, minlen, 100)
    assert ctx.get_option("molecules_active") == 0
    run_batch(ctx, c)
    dres, labels, _ = ctx.download()
    assert np.array_equal(dres["read_type"], res["read_type"]) and np.array_equal(labels, lab)
    for call in (ctx.mol_entries, ctx.mol_get, ctx.mol_reset):
        with pytest.raises(TdError, match="molecule count is off"):
            call()
    with pytest.raises(TdError, match="molecule count is off"):
        ctx.get_option("molecules_kernel_us")
    ctx.mol_disable()                                   # (nothing to do)
    ctx.set_window(2, 40)                               # no count: a window is fine
    ctx.set_window(-1, -1)


def test_refusals_and_the_model_upload_that_switches_it_off(ctx):
    from tagdust_amd import TdError
    with pytest.raises(TdError, match="no model uploaded"):
        ctx.mol_enable()
    c = case("b_f_r")
    ctx.upload_model(c[0])
    for bad in (0, 33):
        with pytest.raises(TdError, match="prefix_bases"):
            ctx.mol_enable(bad, 8)
    for bad in (3, 31):
        with pytest.raises(TdError, match="log2_slots"):
            ctx.mol_enable(20, bad)
    ctx.set_window(2, 40)
    with pytest.raises(TdError, match="window"):
        ctx.mol_enable(20, 8)
    ctx.set_window(-1, -1)
    ctx.mol_enable(20, 8)
    assert ctx.get_option("molecules_active") == 1
    with pytest.raises(TdError, match="molecule count is on"):
        ctx.set_window(2, 40)
    ctx.upload_model(c[0])
    assert ctx.get_option("molecules_active") == 0
    ctx.mol_enable(20, 8)
    ctx.mol_disable()
    assert ctx.get_option("molecules_active") == 0


def test_census_and_molecules_together_each_equal_what_they_give_alone(ctx):
    c = case("b_f_r")
    P = 16
    start(ctx, c, P)
    run_batch(ctx, c)
    mol_alone = ctx.mol_entries()
    ctx.mol_disable()
    ctx.census_enable(-1, 0xFF, 16)
    run_batch(ctx, c)
    census_alone = ctx.census()
    ctx.census_disable()
    ctx.mol_enable(P, 16)
    ctx.census_enable(-1, 0xFF, 16)
    run_batch(ctx, c)
    assert ctx.get_option("molecules_kernel_us") >= 0 and ctx.get_option("census_kernel_us") >= 0
    ent, tot = ctx.mol_entries()
    cen, ctot = ctx.census()
    assert pairs(ent) == pairs(mol_alone[0]) and tot == mol_alone[1] and pairs(ent) == pairs(yardstick(c, P)[0])
    assert pairs(cen) == pairs(census_alone[0]) and ctot == census_alone[1] and ctot["counted"] > 0
    # each reset clears its own table and tallies, and nothing of the other's
    ctx.census_reset()
    ent2, tot2 = ctx.mol_entries()
    cen2, ctot2 = ctx.census()
    assert pairs(ent2) == pairs(ent) and tot2 == tot
    assert len(cen2) == 0 and ctot2 and all(v == 0 for v in ctot2.values())
    run_batch(ctx, c)
    ctx.mol_reset()
    ent3, tot3 = ctx.mol_entries()
    cen3, ctot3 = ctx.census()
    assert pairs(cen3) == pairs(census_alone[0]) and ctot3 == census_alone[1]
    assert len(ent3) == 0 and tot3 and all(v == 0 for v in tot3.values())


# ---- 11: the command ----
def fastq_of(seq, offs):
    alpha = np.frombuffer(b"ACGTN", np.uint8)
    return b"".join(b"@r%d\n" % i + bytes(alpha[seq[offs[i]:offs[i + 1]]]) + b"\n+\n" + b"I" * int(offs[i + 1] - offs[i]) + b"\n"
                    for i in range(len(offs) - 1))


def molecules_text(infile, P, tot, rows, labels):
    """<out>_molecules.txt as include/tagdust_run.h describes it, from a yardstick's totals and rows"""
    out = ["# molecules: the extracted reads of %s by barcode, fingerprint and the first bases of the read" % infile,
           "# prefix bases\t%d" % P, "# extracted reads\t%d" % tot["eligible"], "# counted\t%d" % tot["counted"],
           "# molecules\t%d" % tot["molecules"], "# no read base\t%d" % tot["skipped_empty"], "# N in the prefix\t%d" % tot["skipped_n"],
           "# barcode\treads\tmolecules\tduplication\t1\t2\t3\t4\t5\t6\t7\t8\t9\t10+"]

    def line(label, reads, mols, levels):
        dup = 1.0 - mols / reads if reads else 0.0
        return "%s\t%d\t%d\t%0.4f\t%s" % (label, reads, mols, dup, "\t".join(str(int(v)) for v in levels))

    for q, label in enumerate(labels):
        out.append(line(label, int(rows["reads"][q]), int(rows["molecules"][q]), rows["levels"][q]))
    out.append(line("total", int(rows["reads"].sum()), int(rows["molecules"].sum()), rows["levels"].sum(axis=0)))
    return "\n".join(out) + "\n"


def _outputs(d, prefix):
    out = {}
    for p in sorted(glob.glob(os.path.join(d, prefix + "*"))):
        name = os.path.basename(p)[len(prefix):]
        data = open(p, "rb").read()
        if name == "_logfile.txt":    # the messages without their time stamps; the cmd: line repeats the command line as given
            msgs = [l.split(b"]\t", 1)[1] if l.startswith(b"[") and b"]\t" in l else l for l in data.splitlines()]
            data = b"\n".join(m for m in msgs if not m.startswith(b"cmd: "))
        out[name] = data
    return out


def _run(args, d, rc=0):
    env = dict(os.environ, TD_SPECIALIZE="0")
    p = subprocess.run([EXE, "--rtest"] + args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
    assert p.returncode == rc, p.stderr.decode(errors="replace")[-3000:]
    return p.stderr.decode(errors="replace")


def command_case(shape):
    """the case's reads decoded as the command decodes them with -Q 20 (threshold 0, the run's model): (segments, yardstick)"""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    if ("command", shape) not in _CASES:
        _, seq, offs = case(shape)[:3]
        md, _ = tdlib.build_model(SHAPES[shape], seq, offs, e=0.05, d=0.1)
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, 0.0, 16, 100, 8)
        ent, tot = tdlib.mol_host(md, seq, offs, ores, olab, 20)
        _CASES[("command", shape)] = (ent, tot)
    return _CASES[("command", shape)]


@pytest.mark.parametrize("shape", ["b_f_r", "f_r"])
def test_the_command_writes_the_molecules_file(tmp_path, shape):
    from tagdust_amd import lib as tdlib
    _, seq, offs = case(shape)[:3]
    ent, tot = command_case(shape)
    assert tot["molecules"] < 0.7 * tot["counted"] and tot["eligible"] >= 0.8 * (len(offs) - 1)
    d = str(tmp_path)
    open(os.path.join(d, "in.fq"), "wb").write(fastq_of(seq, offs))
    segs = SHAPES[shape]
    base = ["-Q", "20"] + [w for k, s in enumerate(segs) for w in ("-%d" % (k + 1), s)] + ["in.fq"]
    _run(base + ["-o", "plain"], d)
    _run(base + ["--molecules", "--molecules-slots", "16", "-o", "with"], d)
    labels = BARCODES if shape == "b_f_r" else ["-"]
    want = molecules_text("in.fq", 20, tot, tdlib.mol_summarise(ent), labels)
    assert open(os.path.join(d, "with_molecules.txt")).read() == want
    plain, with_opt = _outputs(d, "plain"), _outputs(d, "with")
    assert "_molecules.txt" not in plain and set(with_opt) == set(plain) | {"_molecules.txt"}
    for name in plain:
        assert plain[name] == with_opt[name], name
    assert b"molecule" not in with_opt["_logfile.txt"]


def test_the_run_on_two_devices_equals_the_run_on_one(tmp_path):
    """td_run_execute with one context (td_mol_get's device summary) and with two contexts on one device (entries merged and
    summarised on the host): the same rows, totals and file; a table of 16 slots says so in the file"""
    from tagdust_amd import lib as tdlib
    shape = "b_f_r"
    _, seq, offs = case(shape)[:3]
    ent, tot = command_case(shape)
    d = str(tmp_path)
    fq = os.path.join(d, "in.fq")
    open(fq, "wb").write(fastq_of(seq, offs))
    segs = SHAPES[shape]
    base = ["--rtest", "-Q", "20"] + [w for k, s in enumerate(segs) for w in ("-%d" % (k + 1), s)] + [fq, "--molecules", "--molecules-slots", "14"]
    os.environ["TD_SPECIALIZE"] = "0"
    try:
        one = tdlib.run_execute(base + ["-o", os.path.join(d, "one")])
        two = tdlib.run_execute(base + ["--devices", "0,0", "-o", os.path.join(d, "two")])
        small = tdlib.run_execute(base[:-1] + ["4", "-o", os.path.join(d, "small")])
    finally:
        del os.environ["TD_SPECIALIZE"]
    rows = tdlib.mol_summarise(ent)
    for rep in (one, two):
        assert np.array_equal(rep["molecules"], rows) and rep["molecules_totals"] == tot
    assert open(os.path.join(d, "one_molecules.txt")).read() == open(os.path.join(d, "two_molecules.txt")).read() == \
        molecules_text(fq, 20, tot, rows, BARCODES)
    st = small["molecules_totals"]
    assert st["overflow"] > 0 and st["eligible"] == tot["eligible"] and st["counted"] + st["overflow"] == tot["counted"]
    text = open(os.path.join(d, "small_molecules.txt")).read()
    assert "# the counting table was too small: %d reads were not counted" % st["overflow"] in text and "--molecules-slots 5 or more" in text
    assert tdlib.run_execute(base[:-3] + ["-o", os.path.join(d, "none")])["molecules"] is None


@pytest.mark.parametrize("L", [4, 12])
def test_the_command_prints_fingerprints_as_the_reference_does(tmp_path, L):
    if not os.path.exists(os.path.join(RBIN, "tagdust_rtest")):
        pytest.skip("oracle/_ref/tagdust_rtest not built")
    rng = np.random.default_rng(30 + L)
    words = ["ACGTAC", "TTGACA", "GGATCC"]
    recs = []
    for i in range(400):
        if rng.random() < 0.05:
            s = "".join("ACGT"[b] for b in rng.integers(0, 4, 60))
        else:
            s = words[int(rng.integers(0, 3))] + "".join("ACGT"[b] for b in rng.integers(0, 4, L + 40))
        recs.append("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    d = str(tmp_path)
    open(os.path.join(d, "in.fq"), "w").write("".join(recs))
    args = ["-seed", "42", "-Q", "20", "-1", "B:" + ",".join(words), "-2", "F:" + "N" * L, "-3", "R:N", "in.fq"]
    p = subprocess.run([os.path.join(RBIN, "tagdust_rtest")] + args + ["-show_finger_seq", "-o", "cpu"], cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-2000:]
    _run(args + ["--fingerprint-seq", "-o", "gpu"], d)
    cpu = {k: v for k, v in _outputs(d, "cpu").items() if k != "_logfile.txt"}
    gpu = {k: v for k, v in _outputs(d, "gpu").items() if k != "_logfile.txt"}
    assert cpu and set(cpu) == set(gpu)
    for k in cpu:
        assert cpu[k] == gpu[k], "output file *%s differs" % k
    assert sum(v.count(b";FP:") for v in gpu.values()) > 300 and not any(b";FP:-" in v or b";FP:1" in v for v in gpu.values())
    for spelling in ("-show_finger_seq", "--show_finger_seq"):           # the reference's spelling stays refused
        err = _run(args + [spelling, "-o", "no"], d, rc=1)
        assert "option " + spelling + " of the reference is not implemented by this program" in err
    assert not glob.glob(os.path.join(d, "no*"))
