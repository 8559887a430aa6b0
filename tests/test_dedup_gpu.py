"""Dedup on the device (include/tagdust_molecules.h, td_mol_dedup_enable; tagdust_amd/csrc/td_molecules.hip).  The yardstick is
always td_mol_dedup_host fed with the CPU oracle's labels, outcomes, barcodes and fingerprints for the same reads in the caller's
order, never the device's own output.  The reads are those of tests/test_molecules_gpu.py (1200 from 240 molecules) with one
change: there every read of a molecule has the molecule's length, and the device's stable sort by length then keeps a molecule's
reads in the caller's order -- "the first read in device order" would pass.  So every third read loses bases its key does not
contain (b_f_r: one to three at its end; r_s_b_f: the last base of its read segment), and each case asserts on the yardstick's side
that the device order would give other marks.  The table has 2^16 slots unless noted, so the yardstick's overflow of 0 holds."""
import os

import numpy as np
import pytest

from test_molecules_gpu import MINLEN, SHAPES, THRESHOLD, fastq_of, make_reads, pack, pairs, yardstick, _outputs, _run

pytestmark = pytest.mark.gpu

_CASES = {}


def dedup_reads(shape, seed=5):
    seq, offs = make_reads(shape, seed)
    rng = np.random.default_rng(seed + 100)
    reads = []
    for i in range(len(offs) - 1):
        r = seq[offs[i]:offs[i + 1]]
        if i % 3 == 0:
            if shape == "b_f_r":
                r = r[:len(r) - int(rng.integers(1, 4))]               # (41 bases and more: the prefix of 32 stays whole)
            else:
                cut = len(r) - 14 - 1                                  # r_s_b_f: the read segment's last base, behind a prefix of 8
                r = np.concatenate([r[:cut], r[cut + 1:]])
        reads.append(r)
    return pack(reads)


def case(shape, seed=5):
    """(model, seq, offs, threshold, minlen, the oracle's records and labels) as test_molecules_gpu.case gives them, computed once"""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    key = (shape, seed)
    if key not in _CASES:
        seq, offs = dedup_reads(shape, seed)
        md, _ = tdlib.build_model(SHAPES[shape], seq, offs)
        thr, minlen = THRESHOLD.get(shape, 5.0), MINLEN.get(shape, 16)
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, minlen, 100, 2)
        res = {f: np.asarray(ores[f]).copy() for f in ("read_type", "barcode", "fingerprint")}
        _CASES[key] = (md, seq, offs, thr, minlen, res, olab)
    return _CASES[key]


def in_order(c, order):
    """the case's reads, records and labels in another order"""
    md, seq, offs, thr, minlen, res, lab = c
    rseq, roffs = pack([seq[offs[i]:offs[i + 1]] for i in order])
    rlab = np.concatenate([lab[offs[i] + i:offs[i + 1] + i + 1] for i in order]).astype(np.int8)
    return md, rseq, roffs, thr, minlen, {f: v[order] for f, v in res.items()}, rlab


def marks(c, P):
    """td_mol_dedup_host over a case: (is_duplicate per read, totals)"""
    from tagdust_amd import lib as tdlib
    md, seq, offs, _, _, res, lab = c
    return tdlib.mol_dedup_host(md, seq, offs, res, lab, P)


def check_case(c, P, want, want_tot):
    """what every case asserts on the yardstick's side before the device is compared"""
    mtot = yardstick(c, P)[1]
    print("yardstick", want_tot, mtot)
    assert mtot["overflow"] == 0 and mtot["eligible"] >= 0.8 * (len(c[2]) - 1)
    assert want_tot["duplicates"] >= 0.3 * mtot["eligible"]
    check_identities(want_tot, mtot)
    # the device decodes in the order of a stable sort by length: judged in that order, other reads would stay
    lens = np.diff(c[2])
    dev = np.argsort(lens, kind="stable")
    assert not np.array_equal(dev, np.arange(len(lens)))
    dev_marks = np.zeros(len(lens), bool)
    dev_marks[dev] = marks(in_order(c, dev), P)[0]
    differ = int((dev_marks != want).sum())
    print("reads the device order would mark otherwise:", differ)
    assert differ >= 20 and int(dev_marks.sum()) == int(want.sum())


def check_identities(dtot, mtot):
    assert mtot["eligible"] == dtot["kept"] + dtot["duplicates"]
    assert dtot["kept"] == mtot["molecules"] + mtot["skipped_empty"] + mtot["skipped_n"] + mtot["overflow"]
    assert dtot["unjudged"] == mtot["skipped_empty"] + mtot["skipped_n"] + mtot["overflow"]


def make_ctx(c, P, spec, log2_slots=16, dedup=True):
    from tagdust_amd import TagdustHip
    md, _, _, thr, minlen, _, _ = c
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 1 if spec else 0)
        ctx.set_option("async_compile", 0)
        ctx.upload_model(md)
        ctx.set_params(thr, minlen, 100)
        ctx.mol_enable(P, log2_slots)
        if dedup:
            ctx.mol_dedup_enable()
    except Exception:
        ctx.close()
        raise
    return ctx


def run_batch(ctx, c, lo=0, hi=None):
    """one td_run batch of reads lo..hi: the records as downloaded"""
    _, seq, offs = c[:3]
    hi = len(offs) - 1 if hi is None else hi
    ctx.upload_batch(seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo])
    ctx.run()
    return ctx.download()


def check_records(c, dres, want):
    """the duplicates are the yardstick's, read for read; everything else of every record is as decoded"""
    res = c[5]
    assert np.array_equal(dres["read_type"] == 7, want)
    assert np.array_equal(dres["read_type"][~want], res["read_type"][~want])
    assert np.array_equal(dres["barcode"], res["barcode"]) and np.array_equal(dres["fingerprint"], res["fingerprint"])


# ---- one batch, read for read ----
ONE = [("b_f_r", 16), ("b_f_r", 32), ("r_s_b_f", 8)]


@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
@pytest.mark.parametrize("shape,P", ONE, ids=["%s-P%d" % sp for sp in ONE])
def test_one_batch_marks_the_yardstick_s_duplicates(shape, P, spec):
    c = case(shape)
    want, want_tot = marks(c, P)
    check_case(c, P, want, want_tot)
    if shape == "r_s_b_f":                                # reads with N in the prefix and reads without a read base are kept
        assert want_tot["unjudged"] > 10
    ctx = make_ctx(c, P, spec)
    try:
        assert ctx.get_option("dedup_active") == 1
        before = ctx.get_option("spec_batches_generic")
        dres, labels, _ = run_batch(ctx, c)
        assert (ctx.get_option("spec_batches_generic") == before) == bool(spec)
        check_records(c, dres, want)
        assert np.array_equal(labels, c[6])
        tot = ctx.mol_dedup_get()
        print(shape, P, "device", tot)
        assert tot == want_tot
        ent, mtot = ctx.mol_entries()                     # the count beside it is the count
        mwant, mwant_tot = yardstick(c, P)
        assert mtot == mwant_tot and pairs(ent) == pairs(mwant)
        assert int(ctx.counts()[0]) == mtot["eligible"] and int(ctx.counts()[7]) == 0   # td_counts_get: the outcomes as decoded
        assert ctx.get_option("dedup_kernel_us") >= 0
    finally:
        ctx.close()


# ---- batching does not matter ----
def submit_all(ctx, c, parts, in_flight):
    """the parts through td_submit, `in_flight` tickets outstanding wherever there are that many parts left; the records, joined"""
    from tagdust_amd import RESULT_DTYPE
    _, seq, offs = c[:3]
    bufs = [(np.ascontiguousarray(seq[offs[lo]:offs[hi]]), np.ascontiguousarray(offs[lo:hi + 1] - offs[lo]), np.zeros(hi - lo, RESULT_DTYPE))
            for lo, hi in parts]
    tickets = []
    for k, (s, o, r) in enumerate(bufs):
        if k >= in_flight:
            ctx.wait(tickets[k - in_flight])
        tickets.append(ctx.submit(s, o, res=r))
    for t in tickets[max(0, len(bufs) - in_flight):]:
        ctx.wait(t)
    return np.concatenate([r for _, _, r in bufs])


@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
def test_batching_does_not_matter(spec):
    """Five td_submit batches of 240 with as many tickets in flight as a context holds (four: the fifth is submitted when the first
    has been waited for); four batches of 300 with every ticket in flight before the first td_wait; 1200 reads in one td_submit.
    Behind the specialised kernel neighbouring batches run on the two compute streams."""
    c = case("b_f_r")
    P = 16
    want, want_tot = marks(c, P)
    check_case(c, P, want, want_tot)
    n = len(c[2]) - 1
    ctx = make_ctx(c, P, spec)
    try:
        ctx.set_option("pipeline_depth", 4)
        for parts in ([(k, k + 240) for k in range(0, n, 240)], [(k, k + 300) for k in range(0, n, 300)], [(0, n)]):
            ctx.mol_reset()
            res = submit_all(ctx, c, parts, 4)
            check_records(c, res, want)
            assert ctx.mol_dedup_get() == want_tot
            check_identities(ctx.mol_dedup_get(), ctx.mol_entries()[1])
            assert ctx.get_option("overlap_active") == spec   # (the second stream and workspace exist from the first td_submit on)
        # td_run batches of uneven sizes, the same marks
        ctx.mol_reset()
        got = np.concatenate([run_batch(ctx, c, lo, hi)[0] for lo, hi in ((0, 1), (1, 65), (65, 700), (700, n))])
        check_records(c, got, want)
        assert ctx.mol_dedup_get() == want_tot
    finally:
        ctx.close()


# ---- reset ----
def test_reset_starts_over_and_without_it_every_counted_read_is_a_duplicate():
    c = case("b_f_r")
    P = 16
    want, want_tot = marks(c, P)
    mtot = yardstick(c, P)[1]
    ctx = make_ctx(c, P, 0)
    try:
        check_records(c, run_batch(ctx, c)[0], want)
        ctx.mol_reset()
        assert ctx.mol_dedup_get() == {"kept": 0, "duplicates": 0, "unjudged": 0}
        check_records(c, run_batch(ctx, c)[0], want)      # the same marks, no more
        assert ctx.mol_dedup_get() == want_tot
        dres = run_batch(ctx, c)[0]                       # no reset: the table knows every key with a smaller ordinal
        counted = (c[5]["read_type"] & 0xFF) == 0
        assert mtot["skipped_empty"] + mtot["skipped_n"] == 0 and np.array_equal(dres["read_type"] == 7, counted)
        tot = ctx.mol_dedup_get()
        assert tot == {"kept": want_tot["kept"], "duplicates": want_tot["duplicates"] + mtot["counted"], "unjudged": 0}
        check_identities(tot, ctx.mol_entries()[1])
    finally:
        ctx.close()


# ---- a table of 16 slots ----
def test_a_small_table_keeps_what_it_cannot_judge():
    c = case("b_f_r")
    P = 16
    ctx = make_ctx(c, P, 0, log2_slots=4)
    try:
        dres = run_batch(ctx, c)[0]
        dres2 = run_batch(ctx, c)[0]
        tot = ctx.mol_dedup_get()
        ent, mtot = ctx.mol_entries()
        print("small table", tot, mtot)
        assert mtot["overflow"] > 0 and 0 < mtot["molecules"] <= 16 and tot["unjudged"] == mtot["overflow"]
        check_identities(tot, mtot)
        assert len(ent) == mtot["molecules"] and tot["kept"] == len(ent) + tot["unjudged"]
        assert int((dres["read_type"] == 7).sum()) + int((dres2["read_type"] == 7).sum()) == tot["duplicates"]
    finally:
        ctx.close()


# ---- dedup off ----
def test_after_dedup_was_on_the_count_and_the_census_are_what_they_are_today():
    from tagdust_amd import TdError
    c = case("b_f_r")
    P = 16
    mwant, mwant_tot = yardstick(c, P)
    ctx = make_ctx(c, P, 0, dedup=False)
    try:
        ctx.census_enable(-1, 0xFF, 16)
        dres = run_batch(ctx, c)[0]
        assert np.array_equal(dres["read_type"], c[5]["read_type"])
        census_before = ctx.census()
        assert ctx.get_option("dedup_active") == 0
        with pytest.raises(TdError, match="dedup is off"):
            ctx.mol_dedup_get()
        ctx.mol_dedup_enable()                            # (starts from an empty table)
        ctx.census_reset()
        dres = run_batch(ctx, c)[0]
        assert int((dres["read_type"] == 7).sum()) == marks(c, P)[1]["duplicates"] > 0
        cen, ctot = ctx.census()                          # the census saw the outcomes as decoded
        assert pairs(cen) == pairs(census_before[0]) and ctot == census_before[1] and ctot["counted"] > 0
        ctx.mol_dedup_disable()
        assert ctx.get_option("dedup_active") == 0 and ctx.get_option("molecules_active") == 1
        ctx.mol_reset()
        ctx.census_reset()
        dres = run_batch(ctx, c)[0]
        assert np.array_equal(dres["read_type"], c[5]["read_type"])
        ent, mtot = ctx.mol_entries()
        assert mtot == mwant_tot and pairs(ent) == pairs(mwant)
        cen, ctot = ctx.census()
        assert pairs(cen) == pairs(census_before[0]) and ctot == census_before[1]
        ctx.mol_dedup_enable()
        ctx.mol_disable()                                 # the count goes, dedup with it
        assert ctx.get_option("dedup_active") == 0
        with pytest.raises(TdError, match="molecule count is off"):
            ctx.mol_dedup_enable()
    finally:
        ctx.close()


# ---- the command ----
def records_of(data):
    lines = data.split(b"\n")
    return [b"\n".join(lines[k:k + 4]) for k in range(0, len(lines) - 1, 4)]


def test_the_command_writes_one_read_per_molecule(tmp_path):
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    shape = "b_f_r"
    _, seq, offs = case(shape)[:3]
    n = len(offs) - 1
    # the reads decoded as the command decodes them with -Q 20 (threshold 0, the run's model)
    md, _ = tdlib.build_model(SHAPES[shape], seq, offs, e=0.05, d=0.1)
    ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, 0.0, 16, 100, 8)
    dup, tot = tdlib.mol_dedup_host(md, seq, offs, ores, olab, 20)
    mtot = tdlib.mol_host(md, seq, offs, ores, olab, 20)[1]
    assert tot["duplicates"] >= 0.3 * mtot["eligible"] and mtot["overflow"] == 0
    d = str(tmp_path)
    open(os.path.join(d, "in.fq"), "wb").write(fastq_of(seq, offs))
    head = ["-Q", "20"] + [w for k, s in enumerate(SHAPES[shape]) for w in ("-%d" % (k + 1), s)]
    tail = ["--sync-compile", "--batch-reads", "250", "--molecules-slots", "16"]   # five batches
    base = head + ["in.fq"] + tail
    _run(base + ["--molecules", "-o", "mol"], d)
    _run(base + ["--dedup", "-o", "dd"], d)
    mol, dd = _outputs(d, "mol"), _outputs(d, "dd")
    assert set(mol) == set(dd)
    # every barcode file: the records the yardstick keeps, in input order
    bars = sorted(k for k in dd if k.startswith("_BC_"))
    assert len(bars) == 8
    kept_names = set()
    for k in bars:
        plain = records_of(mol[k])
        ids = [int(r.split(b";", 1)[0][2:]) for r in plain]
        assert ids == sorted(ids) and len(ids) > 0
        want = [r for r, i in zip(plain, ids) if not dup[i]]
        assert records_of(dd[k]) == want, k
        assert len(want) < len(plain)
        kept_names.update(i for i in ids if not dup[i])
    ok = (np.asarray(ores["read_type"]) & 0xFF) == 0
    assert kept_names == set(np.flatnonzero(ok & ~dup).tolist())
    # _un, the log and everything else of the molecules file are those of --molecules alone
    others = [k for k in dd if k not in bars and k != "_molecules.txt"]
    assert any("_un" in k for k in others) and "_logfile.txt" in others
    for k in others:
        assert dd[k] == mol[k], k
    assert b"dedup" not in dd["_logfile.txt"] and b"duplicate" not in dd["_logfile.txt"]
    new = [l for l in dd["_molecules.txt"].split(b"\n") if l not in mol["_molecules.txt"].split(b"\n")]
    assert new == [b"# written\t%d" % tot["kept"], b"# duplicates removed\t%d" % tot["duplicates"]]
    assert [l for l in dd["_molecules.txt"].split(b"\n") if l not in new] == mol["_molecules.txt"].split(b"\n")
    assert b"# extracted reads\t%d" % (tot["kept"] + tot["duplicates"]) in dd["_molecules.txt"].split(b"\n")
    # the report of the library call
    os.environ["TD_SPECIALIZE"] = "0"
    try:
        fq = os.path.join(d, "in.fq")
        rep = tdlib.run_execute(["--rtest"] + head + [fq] + tail + ["--dedup", "-o", os.path.join(d, "rep")])
        two = pytest.raises(tdlib.TdError, tdlib.run_execute, ["--rtest"] + head + [fq] + tail + ["--dedup", "--devices", "0,0", "-o", os.path.join(d, "two")])
    finally:
        del os.environ["TD_SPECIALIZE"]
    assert rep["dedup_totals"] == tot and rep["molecules_totals"] == mtot
    assert "exactly one device" in str(two.value)
