"""Sample assignment by all 'B' segments on the device (include/tagdust_samples.h, tagdust_amd/csrc/td_samples.hip).  The yardstick is
td_samples_host fed with the CPU oracle's labels and outcomes for the same reads (oracle/pyoracle.py), never with the device's own
output.  The table has 2^16 slots unless noted: a batch has at most 30 distinct tuples, so the yardstick's overflow of 0 holds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B1 = ["ACAGTG", "CTTGTA", "GGCTAC", "TTAGGC"]
B2 = ["AACC", "GGTT", "CATG"]
ARCH = ["B:" + ",".join(B1), "S:GT", "B:" + ",".join(B2), "R:N"]
ARCH_UMI = ["B:" + ",".join(B1), "S:GT", "B:" + ",".join(B2), "F:NNNN", "R:N"]
ARCH_ONE = ["B:" + ",".join(B1), "R:N"]
B3 = ["AGTC", "TCAG", "GACT", "CTGA"]
ARCH_THREE = ["B:" + ",".join(B1), "S:GT", "B:" + ",".join(B2), "S:GT", "B:" + ",".join(B3), "R:N"]
SHEET_THREE = [(a, b, c) for a in range(4) for b in range(3) for c in range(4) if (a + b + c) % 3 == 0]
SHEET = [(0, 0), (1, 1), (2, 2), (3, 0), (0, 1), (1, 2), (3, 2)]
NAMES = ["plate-A1", "plate-A2", None, "x.3", "x_4", "S99", "last"]
SUCCESS, DEMOTED, DUPLICATE = 0, 3, 7


def code(s):
    return np.array([b"ACGTN".index(c) for c in s.encode()], np.uint8)


def pairs(entries):
    return [(int(k), int(c)) for k, c in zip(entries["key"], entries["count"])]


def make_reads(kind="two", n=1000, seed=7):
    """A read that follows the architecture is barcode + GT + barcode (+ four random bases, "umi") + 20..100 random bases; r, drawn
    once per read, decides what changes: < 0.2 the first barcode is a random 6-mer, else < 0.3 the second barcode is a random 4-mer,
    else < 0.35 one base of the first barcode is N, else < 0.45 the whole read is 20..150 random bases.  ("one": barcode + the rest; "three": + GT + a third barcode behind the second.)"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n):
        r = rng.random()
        b1, b2 = code(B1[int(rng.integers(0, 4))]), code(B2[int(rng.integers(0, 3))])
        if r < 0.2:
            b1 = rng.integers(0, 4, 6, dtype=np.uint8)
        elif r < 0.3:
            b2 = rng.integers(0, 4, 4, dtype=np.uint8)
        elif r < 0.35:
            b1[int(rng.integers(0, 6))] = 4
        elif r < 0.45:
            reads.append(rng.integers(0, 4, int(rng.integers(20, 151)), dtype=np.uint8))
            continue
        rest = rng.integers(0, 4, int(rng.integers(20, 101)), dtype=np.uint8)
        if kind == "one":
            reads.append(np.concatenate([b1, rest]))
        elif kind == "three":
            reads.append(np.concatenate([b1, code("GT"), b2, code("GT"), code(B3[int(rng.integers(0, 4))]), rest]))
        elif kind == "umi":
            reads.append(np.concatenate([b1, code("GT"), b2, rng.integers(0, 4, 4, dtype=np.uint8), rest]))
        else:
            reads.append(np.concatenate([b1, code("GT"), b2, rest]))
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), offs


_MODELS, _CASES = {}, {}


def model(kind):
    from tagdust_amd import lib as tdlib
    if kind not in _MODELS:
        seq, offs = make_reads(kind)
        md, _ = tdlib.build_model({"two": ARCH, "umi": ARCH_UMI, "one": ARCH_ONE, "three": ARCH_THREE}[kind], seq, offs)
        _MODELS[kind] = (md, seq, offs)
    return _MODELS[kind]


def case(kind="two", thr=0.5):
    """(model, seq, offs, threshold, the oracle's records as td_read_result, the oracle's labels), computed once"""
    from oracle import pyoracle
    from tagdust_amd import RESULT_DTYPE
    if (kind, thr) not in _CASES:
        md, seq, offs = model(kind)
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, 16, 100, 2)
        res = np.zeros(len(ores), RESULT_DTYPE)
        for f in RESULT_DTYPE.names:
            res[f] = ores["Q" if f == "mapq" else f]
        _CASES[(kind, thr)] = (md, seq, offs, thr, res, olab)
    return _CASES[(kind, thr)]


def sheet_of(kind):
    return {"one": [[0], [2], [3]], "three": SHEET_THREE}.get(kind, SHEET)


def yardstick(c, sheet, lo=0, hi=None):
    """td_samples_host over reads lo..hi of a case with the oracle's labels and records: (rewritten records, entries, totals)"""
    from tagdust_amd import lib as tdlib
    md, _, offs, _, res, lab = c
    hi = len(offs) - 1 if hi is None else hi
    return tdlib.samples_host(md, sheet, offs[lo:hi + 1] - offs[lo], res[lo:hi], lab[offs[lo] + lo:offs[hi] + hi])


@pytest.fixture()
def ctx():
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", 0)
    yield c
    c.close()


def start(ctx, c, sheet=None, log2_slots=16, names=None):
    md, _, _, thr, _, _ = c
    ctx.upload_model(md)
    ctx.set_params(thr, 16, 100)
    if sheet is not None:
        ctx.samples_enable(sheet, names, log2_slots)


def run_batch(ctx, c, lo=0, hi=None):
    _, seq, offs, _, _, _ = c
    hi = len(offs) - 1 if hi is None else hi
    ctx.upload_batch(seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo])
    ctx.run()


def check_identities(ent, tot):
    assert tot["eligible"] == tot["assigned"] + tot["unlisted"] + tot["incomplete"]
    assert int(ent["count"].sum()) == tot["eligible"] - tot["overflow"]


def same_but_for_the_rewrite(got, plain, want):
    """downloads (records, labels, seq_out) with samples on and off: read_type and barcode are the yardstick's, every other byte is equal"""
    assert np.array_equal(got[0]["read_type"], want["read_type"]) and np.array_equal(got[0]["barcode"], want["barcode"])
    for f in got[0].dtype.names:
        if f not in ("read_type", "barcode"):
            assert got[0][f].tobytes() == plain[0][f].tobytes(), f
    assert got[1].tobytes() == plain[1].tobytes() and got[2].tobytes() == plain[2].tobytes()


def test_the_yardstick_meets_what_the_cases_are_made_for():
    """(asserted on the yardstick alone, before the device is asked)"""
    _, _, tot = yardstick(case("two", 0.0), SHEET)
    print("threshold 0.0", tot)
    assert min(tot["assigned"], tot["unlisted"], tot["incomplete"]) >= 10
    _, _, tot = yardstick(case("two", 5.0), SHEET)
    print("threshold 5.0", tot)
    assert tot["incomplete"] == 0 and tot["assigned"] >= 100 and tot["unlisted"] >= 100


@pytest.mark.parametrize("specialize", [0, 1], ids=["generic", "specialised"])
@pytest.mark.parametrize("thr", [0.0, 0.5, 5.0])
def test_whole_batch_equals_the_yardstick(thr, specialize):
    from tagdust_amd import TagdustHip
    c = case("two", thr)
    want, want_ent, want_tot = yardstick(c, SHEET)
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", specialize)
        ctx.set_option("async_compile", 0)
        start(ctx, c)
        before = ctx.get_option("spec_batches_generic")
        run_batch(ctx, c)
        assert (ctx.get_option("spec_batches_generic") == before) == bool(specialize)
        plain = ctx.download()
        assert np.array_equal(plain[0]["read_type"], c[4]["read_type"]) and np.array_equal(plain[1], c[5])
        ctx.samples_enable(SHEET, NAMES, 16)
        assert ctx.get_option("samples") == len(SHEET)
        run_batch(ctx, c)
        got = ctx.download()
        ent, tot = ctx.samples()
        assert ctx.get_option("samples_kernel_us") >= 0
        assert [ctx.samples_name(s) for s in range(len(SHEET))] == ["plate-A1", "plate-A2", "S3", "x.3", "x_4", "S99", "last"]
        assert ctx.samples_name(len(SHEET)) is None and ctx.samples_name(-1) is None
    finally:
        ctx.close()
    print(thr, specialize, "device totals", tot)
    same_but_for_the_rewrite(got, plain, want)
    assert tot == want_tot and pairs(ent) == pairs(want_ent)
    check_identities(ent, tot)
    changed = got[0]["read_type"] != plain[0]["read_type"]
    assert int(changed.sum()) == tot["unlisted"] + tot["incomplete"] and set(got[0]["read_type"][changed]) <= {DEMOTED}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_batch_sizes(ctx, n):
    c = case("two", 0.5)
    start(ctx, c, SHEET)
    lo = 300                                            # (a stretch of the batch with every class in it)
    want, want_ent, want_tot = yardstick(c, SHEET, lo, lo + n)
    run_batch(ctx, c, lo, lo + n)
    res, _, _ = ctx.download()
    ent, tot = ctx.samples()
    assert np.array_equal(res["read_type"], want["read_type"]) and np.array_equal(res["barcode"], want["barcode"])
    assert tot == want_tot and pairs(ent) == pairs(want_ent)
    if n >= 63:
        assert min(tot["assigned"], tot["unlisted"] + tot["incomplete"]) > 0


def test_pipelined_batches_add_up_to_the_whole_and_reset(ctx):
    from tagdust_amd import RESULT_DTYPE
    c = case("two", 0.5)
    _, seq, offs, _, _, _ = c
    n = len(offs) - 1
    want, want_ent, want_tot = yardstick(c, SHEET)
    start(ctx, c, SHEET)
    parts = [(0, 1), (1, 130), (130, 500), (500, 565), (565, n)]
    res = [np.zeros(hi - lo, RESULT_DTYPE) for lo, hi in parts]
    ins = [(np.ascontiguousarray(seq[offs[lo]:offs[hi]]), np.ascontiguousarray(offs[lo:hi + 1] - offs[lo])) for lo, hi in parts]
    tickets = []
    for k, ((s, o), r) in enumerate(zip(ins, res)):     # up to three tickets in flight
        if k >= 3:
            ctx.wait(tickets[k - 3])
        tickets.append(ctx.submit(s, o, res=r))
    for t in tickets[-3:]:
        ctx.wait(t)
    got = np.concatenate(res)
    assert np.array_equal(got["read_type"], want["read_type"]) and np.array_equal(got["barcode"], want["barcode"])
    ent, tot = ctx.samples()
    assert tot == want_tot and pairs(ent) == pairs(want_ent)
    ctx.counts_reset()                                  # the outcome counters are another matter
    assert ctx.samples()[1] == want_tot
    ctx.samples_reset()
    ent, tot = ctx.samples()
    assert len(ent) == 0 and not any(tot.values())
    a, a_ent, a_tot = yardstick(c, SHEET, 0, 400)
    run_batch(ctx, c, 0, 400)
    ent, tot = ctx.samples()
    assert tot == a_tot and pairs(ent) == pairs(a_ent)
    assert ctx.samples_name(0) == "S1"                  # the sheet stays


def test_overflow_leaves_the_rewrite_alone(ctx):
    """three barcode segments: the reads of two have 15 distinct tuples, which a table of 16 slots holds"""
    c = case("three", 0.0)
    want, want_ent, want_tot = yardstick(c, SHEET_THREE)
    assert len(want_ent) > 16 and min(want_tot["assigned"], want_tot["unlisted"], want_tot["incomplete"]) >= 10
    start(ctx, c, SHEET_THREE, log2_slots=4)
    run_batch(ctx, c)
    res, _, _ = ctx.download()
    ent, tot = ctx.samples()
    print("overflow totals", tot)
    assert np.array_equal(res["read_type"], want["read_type"]) and np.array_equal(res["barcode"], want["barcode"])
    assert all(tot[f] == want_tot[f] for f in ("eligible", "assigned", "unlisted", "incomplete"))
    assert tot["overflow"] > 0 and 0 < len(ent) <= 16
    check_identities(ent, tot)
    ref = dict(pairs(want_ent))
    assert all(ref.get(k) == v for k, v in pairs(ent))   # a reported count is exact


def test_census_and_molecule_count_read_the_rewritten_batch(ctx):
    from tagdust_amd import lib as tdlib
    c = case("umi", 0.5)
    md, seq, offs, _, _, lab = c
    want, want_ent, want_tot = yardstick(c, SHEET)
    assert min(want_tot["assigned"], want_tot["unlisted"]) >= 10
    start(ctx, c, SHEET)
    ctx.census_enable(-1, tdlib.CENSUS_DEFAULT_MASK, 16)
    ctx.mol_enable(20, 16)
    run_batch(ctx, c)
    ent, tot = ctx.samples()
    assert tot == want_tot and pairs(ent) == pairs(want_ent)
    cen, cen_tot = ctx.census()
    want_cen, want_cen_tot = tdlib.census_host(md, seq, offs, want["read_type"], lab, -1, tdlib.CENSUS_DEFAULT_MASK)
    assert cen_tot == want_cen_tot and pairs(cen) == pairs(want_cen)
    plain_cen_tot = tdlib.census_host(md, seq, offs, c[4]["read_type"], lab, -1, tdlib.CENSUS_DEFAULT_MASK)[1]
    assert cen_tot["eligible"] == plain_cen_tot["eligible"] + want_tot["unlisted"] + want_tot["incomplete"]   # the demoted reads are in it
    mol, mol_tot = ctx.mol_entries()
    want_mol, want_mol_tot = tdlib.mol_host(md, seq, offs, want, lab, 20)
    assert mol_tot == want_mol_tot and pairs(mol) == pairs(want_mol)
    assert {k >> 56 for k, _ in pairs(mol)} <= set(range(len(SHEET)))       # the bins are samples
    # dedup behind it: the marks of the rewritten records
    ctx.mol_reset()
    ctx.mol_dedup_enable()
    run_batch(ctx, c)
    res, _, _ = ctx.download()
    dup, dup_tot = tdlib.mol_dedup_host(md, seq, offs, want, lab, 20)
    assert ctx.mol_dedup_get() == dup_tot
    assert np.array_equal(res["read_type"] == DUPLICATE, dup)
    assert np.array_equal(res["read_type"][~dup], want["read_type"][~dup]) and np.array_equal(res["barcode"], want["barcode"])


def test_one_barcode_segment(ctx):
    c = case("one", 0.0)
    sheet = sheet_of("one")
    want, want_ent, want_tot = yardstick(c, sheet)
    assert min(want_tot["assigned"], want_tot["unlisted"]) >= 10
    start(ctx, c)
    run_batch(ctx, c)
    plain = ctx.download()
    ctx.samples_enable(sheet)
    run_batch(ctx, c)
    got = ctx.download()
    ent, tot = ctx.samples()
    same_but_for_the_rewrite(got, plain, want)
    assert tot == want_tot and pairs(ent) == pairs(want_ent)
    kept = got[0]["read_type"] == SUCCESS
    assert all(sheet[int(s)][0] == int(b) for s, b in zip(got[0]["barcode"][kept] & 0xFFFF, plain[0]["barcode"][kept] & 0xFFFF))


def test_off_means_off(ctx):
    from tagdust_amd import TdError
    c = case("two", 0.5)
    start(ctx, c)
    assert ctx.get_option("samples") == 0
    run_batch(ctx, c)
    first = ctx.download()
    assert np.array_equal(first[0]["read_type"], c[4]["read_type"]) and np.array_equal(first[0]["barcode"], c[4]["barcode"])
    assert np.array_equal(first[1], c[5])
    for call in (ctx.samples, ctx.samples_reset):
        with pytest.raises(TdError, match="sample assignment is off"):
            call()
    with pytest.raises(TdError, match="samples_kernel_us: sample assignment is off"):
        ctx.get_option("samples_kernel_us")
    ctx.samples_disable()                               # (nothing to do)
    ctx.samples_enable(SHEET)
    run_batch(ctx, c)
    assert not np.array_equal(ctx.download()[0]["read_type"], first[0]["read_type"])
    ctx.samples_disable()
    assert ctx.get_option("samples") == 0 and ctx.samples_name(0) is None
    run_batch(ctx, c)
    again = ctx.download()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    ctx.set_window(2, 40)                               # off: a window is fine
    ctx.set_window(-1, -1)


def test_failures_of_enable_and_the_model_upload_that_switches_it_off(ctx):
    from conftest import load_golden
    from tagdust_amd import RESULT_DTYPE, TdError
    with pytest.raises(TdError, match="td_samples_enable: no model uploaded"):
        ctx.samples_enable(SHEET)
    ctx.upload_model(load_golden("umi_f_s_r"))
    with pytest.raises(TdError, match="td_samples_enable: the model has no 'B' segment"):
        ctx.samples_enable([[0]])
    c = case("two", 0.5)
    md, seq, offs, _, _, _ = c
    start(ctx, c)
    with pytest.raises(TdError, match=r"row 1 of the sheet: barcode 4 of 'B' segment 0 \(column 0\) is out of range"):
        ctx.samples_enable([(0, 0), (4, 0)])
    with pytest.raises(TdError, match="row 2 of the sheet repeats row 0"):
        ctx.samples_enable([(0, 0), (1, 0), (0, 0)])
    with pytest.raises(TdError, match=r"n_samples = 256 \(1..255 supported\)"):
        ctx.samples_enable(np.zeros((256, 2), np.int32))
    with pytest.raises(TdError, match=r"row 1 of the sheet: the name 'a b' holds a character outside"):
        ctx.samples_enable([(0, 0), (1, 0)], ["a", "a b"])
    with pytest.raises(TdError, match=r"row 0 of the sheet: a name has 1..64 characters, this one 65"):
        ctx.samples_enable([(0, 0), (1, 0)], ["x" * 65, "b"])
    with pytest.raises(TdError, match=r"row 0 of the sheet: a name has 1..64 characters, this one 0"):
        ctx.samples_enable([(0, 0), (1, 0)], ["", "b"])
    with pytest.raises(TdError, match=r"row 1 of the sheet: the name 'S1' is taken by an earlier row"):
        ctx.samples_enable([(0, 0), (1, 0)], [None, "S1"])
    for bad in (3, 27):
        with pytest.raises(TdError, match=r"log2_slots = %d \(4..26 supported\)" % bad):
            ctx.samples_enable(SHEET, None, bad)
    ctx.set_window(2, 40)
    with pytest.raises(TdError, match="td_samples_enable: a -start/-end window is set"):
        ctx.samples_enable(SHEET)
    ctx.set_window(-1, -1)
    res = np.zeros(100, RESULT_DTYPE)
    s, o = np.ascontiguousarray(seq[:offs[100]]), np.ascontiguousarray(offs[:101])
    t = ctx.submit(s, o, res=res)
    with pytest.raises(TdError, match="td_samples_enable: td_submit tickets are outstanding"):
        ctx.samples_enable(SHEET)
    ctx.wait(t)
    assert ctx.get_option("samples") == 0               # no failure left anything on
    ctx.samples_enable(SHEET, None, 8)
    with pytest.raises(TdError, match="td_set_window: sample assignment is on"):
        ctx.set_window(2, 40)
    ctx.upload_model(md)
    assert ctx.get_option("samples") == 0
    ctx.set_window(2, 40)
    ctx.set_window(-1, -1)


def test_a_batch_resident_across_the_switch_is_refused(ctx):
    """as the mate filter's: a batch is rewritten under the sheet it was staged under, or not decoded at all"""
    from tagdust_amd import TdError
    c = case("two", 0.5)
    _, seq, offs, _, _, _ = c
    start(ctx, c)
    ctx.upload_batch(seq[:offs[100]], offs[:101])
    ctx.samples_enable(SHEET)
    with pytest.raises(TdError, match="sample assignment is on .* staged while it was off: upload it again"):
        ctx.run()
    assert not any(ctx.samples()[1].values())
    run_batch(ctx, c, 0, 100)
    want, want_ent, want_tot = yardstick(c, SHEET, 0, 100)
    assert ctx.samples()[1] == want_tot
    ctx.samples_enable(SHEET[:3])                       # another sheet: the resident batch belongs to the first
    with pytest.raises(TdError, match="staged under an earlier sheet: upload it again"):
        ctx.run()
    ctx.samples_disable()
    with pytest.raises(TdError, match="sample assignment is off .* staged while it was on: upload it again"):
        ctx.run()
    ctx.run(6)                                          # TD_MODE_RNA_DUST has no labels: it runs whatever the switch says
    run_batch(ctx, c, 0, 100)
    assert np.array_equal(ctx.download()[0]["read_type"], c[4]["read_type"][:100])


def test_other_modes_add_nothing(ctx):
    from tagdust_amd import lib as tdlib
    c = case("two", 0.5)
    _, seq, offs, _, _, _ = c
    start(ctx, c, SHEET)
    for mode in (tdlib.MODE_GET_PROB, tdlib.MODE_ARCH_COMP, tdlib.MODE_RNA_DUST):
        ctx.upload_batch(seq[:offs[200]], offs[:201])
        ctx.run(mode)
        ctx.sync()
    ent, tot = ctx.samples()
    assert len(ent) == 0 and not any(tot.values())


def test_full_sheet_behind_the_specialised_kernel():
    """Two 16-barcode 8-nt indices around a spacer (tests/plan_shapes.py: both segments in the run-time HMM loop, barcodes dealt
    round-robin so that all 256 pairs occur) under a sheet of TD_SAMPLES_MAX = 255 rows in a shuffled order -- every pair but one:
    sample index 254, the binary search over a full row[], and the one pair left out counted as unlisted."""
    import plan_shapes
    from oracle import pyoracle
    from tagdust_amd import TagdustHip, RESULT_DTYPE, lib as tdlib
    segs, seq, offs, md = plan_shapes.make_case(*plan_shapes.SAMPLES_SHAPE)
    thr = float(md["threshold"])
    ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, int(md["minlen"]), int(md["dust"]), 4)
    res = np.zeros(len(ores), RESULT_DTYPE)
    for f in RESULT_DTYPE.names:
        res[f] = ores["Q" if f == "mapq" else f]
    left_out = (5, 9)
    rows = [(a, b) for a in range(16) for b in range(16) if (a, b) != left_out]
    sheet = [rows[k] for k in np.random.RandomState(3).permutation(len(rows))]
    assert len(sheet) == tdlib.SAMPLES_MAX == 255
    want, want_ent, want_tot = tdlib.samples_host(md, sheet, offs, res, olab)
    print("yardstick totals", want_tot, "entries", len(want_ent))
    counts = dict(pairs(want_ent))
    assert counts.get(tdlib.samples_key(list(left_out)), 0) > 0 and want_tot["unlisted"] >= counts[tdlib.samples_key(list(left_out))]
    assert all(counts.get(tdlib.samples_key(list(r)), 0) > 0 for r in sheet)         # every sample has a read ...
    kept = want["read_type"] == SUCCESS
    assert set((want["barcode"][kept] & 0xFF).tolist()) == set(range(255))              # ... index 254 among them
    assert want_tot["assigned"] >= 255 and want_tot["incomplete"] >= 1 and want_tot["overflow"] == 0
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 1)
        ctx.upload_model(md)
        ctx.set_params(thr, int(md["minlen"]), int(md["dust"]))
        ctx.upload_batch(seq, offs)
        ctx.run()
        plain = ctx.download()
        assert np.array_equal(plain[0]["read_type"], res["read_type"]) and np.array_equal(plain[0]["barcode"], res["barcode"])
        assert np.array_equal(plain[1], olab)
        ctx.samples_enable(sheet, None, 16)
        assert ctx.get_option("samples") == 255
        ctx.upload_batch(seq, offs)
        ctx.run()
        got = ctx.download()
        ent, tot = ctx.samples()
        assert ctx.get_option("spec_state") == 3 and ctx.get_option("spec_batches_generic") == 0
        assert ctx.samples_name(254) == "S255" and ctx.samples_name(255) is None
    finally:
        ctx.close()
    print("device totals", tot)
    same_but_for_the_rewrite(got, plain, want)
    assert tot == want_tot and pairs(ent) == pairs(want_ent)
    check_identities(ent, tot)
    unlisted = (plain[0]["read_type"] == SUCCESS) & (got[0]["read_type"] == DEMOTED)
    assert int(unlisted.sum()) == tot["unlisted"] + tot["incomplete"]
    assert dict(pairs(ent))[tdlib.samples_key(list(left_out))] == counts[tdlib.samples_key(list(left_out))]


# ---- the command ----
SAMPLE_NAMES =["s%d" % (k + 1) for k in range(len(SHEET))]


def fastq(seq, offs):
    rows = []
    for i in range(len(offs) - 1):
        s = "".join("ACGTN"[b] for b in seq[offs[i]:offs[i + 1]])
        rows.append("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)))
    return "".join(rows)


def records_by_name(paths):
    """{read name: its four lines} over FASTQ files whose header lines are "@<name>;..." """
    out = {}
    for p in paths:
        lines = open(p).read().splitlines(keepends=True)
        assert len(lines) % 4 == 0
        for k in range(0, len(lines), 4):
            name = lines[k][1:].split(";")[0]
            assert name not in out
            out[name] = "".join(lines[k:k + 4])
    return out


def summary_block(log_path):
    """the controller's summary lines of a log file without their time stamps: {text behind the tab: the number in front of it}"""
    msgs = [l.split("]\t", 1)[1] for l in open(log_path).read().splitlines() if l.startswith("[") and "]\t" in l]
    at = msgs.index("Done.")
    return {m.split("\t", 1)[1]: m.split("\t", 1)[0] for m in msgs[at + 1:] if "\t" in m}


def write_inputs(d):
    import os
    c = case("two", 0.0)          # -Q gives every file threshold 0, and the run builds the model from the same reads with the same rates
    _, seq, offs, _, _, _ = c
    open(os.path.join(d, "in.fq"), "w").write(fastq(seq, offs))
    open(os.path.join(d, "sheet.txt"), "w").write("# name, first barcode, second barcode\n" + "".join(
        "%s\t%s\t%s\n" % (SAMPLE_NAMES[s], B1[a], B2[b]) for s, (a, b) in enumerate(SHEET)))
    return c


def test_the_command_writes_one_file_per_sample(tmp_path):
    import glob
    import os
    import subprocess
    from conftest import REPO
    d = str(tmp_path)
    c = write_inputs(d)
    n = len(c[2]) - 1
    want, want_ent, want_tot = yardstick(c, SHEET)
    exe = os.path.join(REPO, "tagdust_amd", "bin", "tagdust-hip")
    env = dict(os.environ, TD_SPECIALIZE="0")
    base = [exe, "--rtest", "-Q", "0.5"] + [x for k, s in enumerate(ARCH) for x in ("-%d" % (k + 1), s)] + ["in.fq"]
    for extra, prefix in (([], "plain"), (["--samples", "sheet.txt", "--molecules", "--molecules-slots", "16"], "with")):
        p = subprocess.run(base + extra + ["-o", prefix], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    recs = records_by_name(glob.glob(os.path.join(d, "plain*.fq")))
    assert len(recs) == n
    expect = {"with_BC_%s.fq" % s: [] for s in SAMPLE_NAMES}
    expect["with_un.fq"] = []
    for i in range(n):                                  # what the yardstick assigns, in input order
        ok = int(want["read_type"][i]) == SUCCESS
        expect["with_BC_%s.fq" % SAMPLE_NAMES[int(want["barcode"][i]) & 0xFF] if ok else "with_un.fq"].append(recs["r%d" % i])
    got = sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "with*")))
    assert got == sorted(list(expect) + ["with_samples.txt", "with_molecules.txt", "with_logfile.txt"])
    # <out>_molecules.txt labels its rows with the sample names; a row's reads are the sample's
    mol = [l.split("\t") for l in open(os.path.join(d, "with_molecules.txt")).read().splitlines() if not l.startswith("#")]
    assert [(r[0], int(r[1])) for r in mol] == [(s, len(expect["with_BC_%s.fq" % s])) for s in SAMPLE_NAMES] + [("total", want_tot["assigned"])]
    for name, rows in expect.items():
        assert open(os.path.join(d, name)).read() == "".join(rows), name
    assert min(len(rows) for rows in expect.values()) > 0
    # <out>_samples.txt: the totals, one row per sample, the combinations no sample has
    lines = open(os.path.join(d, "with_samples.txt")).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    for text, f in (("extracted reads", "eligible"), ("assigned", "assigned"), ("not in the sheet", "unlisted"), ("incomplete", "incomplete"), ("not counted", "overflow")):
        assert "# %s\t%d" % (text, want_tot[f]) in head
    assert "# samples\t%d" % len(SHEET) in head and "# sheet\tsheet.txt" in head
    assert "# segments\t1 (%s)\t3 (%s)" % (ARCH[0], ARCH[2]) in head
    from tagdust_amd import lib as tdlib
    counts = dict(pairs(want_ent))
    at = lines.index("# combinations not in the sheet")
    rows = [l for l in lines[:at] if not l.startswith("#")]
    assert rows == ["%s\t%s\t%s\t%d\t%0.4f" % (SAMPLE_NAMES[s], B1[a], B2[b], counts[tdlib.samples_key([a, b])], counts[tdlib.samples_key([a, b])] / want_tot["eligible"])
                    for s, (a, b) in enumerate(SHEET)]
    spell = [B1 + ["NNNNNN"], B2 + ["NNNN"]]
    other = [(k, v) for k, v in pairs(want_ent) if tuple(tdlib.samples_key_calls(k)) not in SHEET]
    assert lines[at + 1:] == ["%s\t%s\t%d\t%0.4f" % tuple(["-" if cl < 0 else spell[t][cl] for t, cl in enumerate(tdlib.samples_key_calls(k))] + [v, v / want_tot["eligible"]])
                              for k, v in other]
    assert any("NNNNNN" in l for l in lines[at + 1:])
    # the summary block: the demoted reads have moved from "successfully extracted" to "barcode / UMI not found"
    plain, with_opt = summary_block(os.path.join(d, "plain_logfile.txt")), summary_block(os.path.join(d, "with_logfile.txt"))
    demoted = want_tot["unlisted"] + want_tot["incomplete"]
    assert int(plain["successfully extracted"]) == want_tot["eligible"] and int(with_opt["successfully extracted"]) == want_tot["assigned"]
    assert int(with_opt["barcode / UMI not found"]) == int(plain["barcode / UMI not found"]) + demoted
    for line in ("total input reads", "problems with architecture", "too short", "low complexity"):
        assert with_opt[line] == plain[line], line


def test_two_files_on_two_contexts_give_read1_and_read2_per_sample(tmp_path):
    """a second R:N file: <out>_BC_<name>_READ1/2.fq; two contexts on one device merge their counts"""
    import glob
    import os
    from tagdust_amd import lib as tdlib
    d = str(tmp_path)
    c = write_inputs(d)
    n = len(c[2]) - 1
    want, want_ent, want_tot = yardstick(c, SHEET)
    rng = np.random.default_rng(8)
    mates = [rng.integers(0, 4, 40, dtype=np.uint8) for _ in range(n)]
    moffs = np.arange(n + 1, dtype=np.int64) * 40
    open(os.path.join(d, "in2.fq"), "w").write(fastq(np.concatenate(mates), moffs))
    args = ["--rtest", "--devices", "0,0", "-Q", "0.5"] + [x for k, s in enumerate(ARCH) for x in ("-%d" % (k + 1), s)] + \
        [os.path.join(d, "in.fq"), os.path.join(d, "in2.fq")]
    os.environ["TD_SPECIALIZE"] = "0"
    try:
        plain = tdlib.run_execute(args + ["-o", os.path.join(d, "plain")])
        rep = tdlib.run_execute(args + ["-o", os.path.join(d, "with"), "--samples", os.path.join(d, "sheet.txt")])
    finally:
        del os.environ["TD_SPECIALIZE"]
    assert rep["samples_totals"] == want_tot and pairs(rep["samples"]) == pairs(want_ent) and plain["samples"] is None
    lost = set(records_by_name([os.path.join(d, "plain_un_READ1.fq")]))      # pairs the run without the option did not extract
    demoted = sum(1 for i in range(n) if int(want["read_type"][i]) != int(c[4]["read_type"][i]) and "r%d" % i not in lost)
    assert demoted > 100
    assert rep["counts"][SUCCESS] == plain["counts"][SUCCESS] - demoted and rep["counts"][DEMOTED] == plain["counts"][DEMOTED] + demoted
    for k in (1, 2):
        failed = set(records_by_name([os.path.join(d, "plain_un_READ%d.fq" % k)]))
        recs = records_by_name(glob.glob(os.path.join(d, "plain*_READ%d.fq" % k)))
        assert len(recs) == n
        expect = {"with_BC_%s_READ%d.fq" % (s, k): [] for s in SAMPLE_NAMES}
        expect["with_un_READ%d.fq" % k] = []
        for i in range(n):          # a pair the run without the option did not extract stays where it was (the mate's outcome is not the yardstick's)
            ok = int(want["read_type"][i]) == SUCCESS and "r%d" % i not in failed
            expect["with_BC_%s_READ%d.fq" % (SAMPLE_NAMES[int(want["barcode"][i]) & 0xFF], k) if ok else "with_un_READ%d.fq" % k].append(recs["r%d" % i])
        assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "with*_READ%d.fq" % k))) == sorted(expect)
        for name, rows in expect.items():
            assert open(os.path.join(d, name)).read() == "".join(rows), name
        assert min(len(rows) for rows in expect.values()) > 0
