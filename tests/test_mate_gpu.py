"""Mate mode of the molecule count on the device (include/tagdust_molecules.h, tagdust_amd/csrc/td_molecules.hip): the first bases of a
read's mate joined into the key.  The yardstick is always a *_mated host function fed with the CPU oracle's labels and records
(oracle/pyoracle.py), never the device's own output.  1200 reads sampled with replacement from 240 synthetic molecules with 2 %
substitutions, as the neighbouring files use; every molecule has a mate of 35..60 bases, and 40 % of them a second, alternative mate
(two fragments of one barcode and UMI), a read of theirs taking either.  One mate in eight is cut shorter than M (empty included) or
gets an N inside its first M bases or exactly at base M."""
import os

import numpy as np
import pytest

from test_dedup_gpu import records_of
from test_molecules_gpu import BARCODES, MINLEN, SHAPES, THRESHOLD, code, fastq_of, pack, pairs, _outputs, _run

pytestmark = pytest.mark.gpu

N_MOL, N_READS = 240, 1200
MATE_SHAPES = dict(SHAPES, b_f=["B:" + ",".join(BARCODES), "F:NNNNN"])       # the new shape: no read segment at all
_CASES = {}


def make_pairs(shape, M, seed):
    """(seq, offs, mate codes, mate offs) of N_READS pairs.  The reads are ragged in every shape: b_f_r and r_s_b_f by their read
    segments, b_f by one read in five losing its last base."""
    rng = np.random.default_rng(seed)
    mols = []
    for _ in range(N_MOL):
        bar = code(BARCODES[int(rng.integers(0, len(BARCODES)))])
        if shape == "b_f_r":
            m = [bar, rng.integers(0, 4, 5), rng.integers(0, 4, int(rng.integers(30, 101)))]
        elif shape == "r_s_b_f":
            m = [rng.integers(0, 4, int(rng.integers(10, 41))), code("GTCA"), bar, rng.integers(0, 4, 4)]
        else:
            m = [bar, rng.integers(0, 4, 5)]
        mates = [rng.integers(0, 4, int(rng.integers(35, 61)), dtype=np.uint8)]
        if rng.random() < 0.4:
            mates.append(rng.integers(0, 4, int(rng.integers(35, 61)), dtype=np.uint8))
        mols.append((np.concatenate(m).astype(np.uint8), mates))
    reads, mates = [], []
    for _ in range(N_READS):
        r, alt = mols[int(rng.integers(0, N_MOL))]
        r = r.copy()
        hit = rng.random(len(r)) < 0.02
        r[hit] = rng.integers(0, 4, int(hit.sum()), dtype=np.uint8)
        if shape == "b_f" and rng.random() < 0.2:
            r = r[:-1]
        mt = alt[int(rng.integers(0, len(alt)))].copy()
        what = rng.random()
        if what < 1 / 24:
            mt = mt[:0]
        elif what < 2 / 24:
            mt = mt[:int(rng.integers(1, M))] if M > 1 else mt[:0]
        elif what < 3 / 24:
            mt[int(rng.integers(0, M))] = 4
        elif what < 4 / 24:
            mt[M] = 4                                           # the first base behind the mate's prefix: it must not matter
        reads.append(r)
        mates.append(mt)
    return pack(reads) + pack(mates)


def case(shape, M, seed=5):
    """(model, seq, offs, threshold, minlen, the oracle's records, its labels, mate codes, mate offs), computed once"""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    key = (shape, M, seed)
    if key not in _CASES:
        seq, offs, mc, mo = make_pairs(shape, M, seed)
        md, _ = tdlib.build_model(MATE_SHAPES[shape], seq, offs)
        thr, minlen = THRESHOLD.get(shape, 5.0), MINLEN.get(shape, 0 if shape == "b_f" else 16)
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, minlen, 100, 2)
        res = {f: np.asarray(ores[f]).copy() for f in ("read_type", "barcode", "fingerprint")}
        _CASES[key] = (md, seq, offs, thr, minlen, res, olab, mc, mo)
    return _CASES[key]


def part(c, lo, hi):
    """reads lo..hi of a case with their mates, every array its own"""
    md, seq, offs, thr, minlen, res, lab, mc, mo = c
    return (md, np.ascontiguousarray(seq[offs[lo]:offs[hi]]), np.ascontiguousarray(offs[lo:hi + 1] - offs[lo]), thr, minlen,
            {f: v[lo:hi] for f, v in res.items()}, lab[offs[lo] + lo:offs[hi] + hi], np.ascontiguousarray(mc[mo[lo]:mo[hi]]),
            np.ascontiguousarray(mo[lo:hi + 1] - mo[lo]))


def host_args(c, M):
    md, seq, offs, _, _, res, lab, mc, mo = c
    return (md, seq, offs, res, lab, (mc, mo, M) if M else None)


def yardstick(c, P, M):
    from tagdust_amd import lib as tdlib
    return tdlib.mol_host_mated(*host_args(c, M), P)


def check_data(c, P, M):
    """what the data must be, asserted on the yardstick's side before the device is compared"""
    md, seq, offs, _, _, res, lab, mc, mo = c
    from tagdust_amd import lib as tdlib
    n = len(offs) - 1
    want, tot = yardstick(c, P, M)
    plain, ptot = yardstick(c, P, 0)
    print("yardstick mated", tot, "unmated", ptot)
    assert tot["overflow"] == 0 and tot["eligible"] >= 0.7 * n and tot["eligible"] == ptot["eligible"]
    assert tot["molecules"] < 0.7 * tot["counted"]
    assert tot["skipped_n"] > ptot["skipped_n"] and tot["counted"] > 0.7 * tot["eligible"]
    if any(int(t) == ord("R") for t in md["seg_type"]):
        assert tot["molecules"] >= 1.1 * ptot["molecules"] > 0          # the alternative mates are molecules of their own
    else:
        assert ptot["skipped_empty"] == ptot["eligible"] and tot["molecules"] > 100     # b_f: nothing to count without the mate
    lens = np.diff(offs)
    dev = np.argsort(lens, kind="stable")                     # the device decodes in this order
    assert not np.array_equal(dev, np.arange(n))
    inv = np.empty(n, np.int64)
    inv[dev] = np.arange(n)
    wrong_c, wrong_o = pack([mc[mo[k]:mo[k + 1]] for k in inv])  # read i with the mate at its device position
    wrong, _ = tdlib.mol_host_mated(md, seq, offs, res, lab, (wrong_c, wrong_o, M), P)
    differ = len(set(pairs(wrong)) ^ set(pairs(want)))
    print("entries that differ when the mates are taken in device order:", differ)
    assert differ >= 20
    return want, tot


def make_ctx(c, P, M, spec=0, log2_slots=16, dedup=False, collapse=False):
    from tagdust_amd import TagdustHip
    md, _, _, thr, minlen = c[:5]
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 1 if spec else 0)
        ctx.set_option("async_compile", 0)
        ctx.upload_model(md)
        ctx.set_params(thr, minlen, 100)
        ctx.mol_enable(P, log2_slots)
        if collapse:
            ctx.mol_collapse_enable()
        if dedup:
            ctx.mol_dedup_enable()
        if M:
            ctx.mol_mate_enable(M)
    except Exception:
        ctx.close()
        raise
    return ctx


def run_batch(ctx, c, mate=True):
    """one td_run batch of a case (or a part of one) with its mates: the records as downloaded"""
    _, seq, offs = c[:3]
    if mate:
        ctx.mol_mate_next(c[7], c[8])
    ctx.upload_batch(seq, offs)
    ctx.run()
    return ctx.download()


def submit_all(ctx, c, cuts, in_flight=4):
    """the parts between the cuts through td_submit, each behind its own td_mol_mate_next, `in_flight` tickets outstanding wherever
    there are that many parts left; the records, joined"""
    from tagdust_amd import RESULT_DTYPE
    parts = [part(c, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    outs = [np.zeros(len(p[2]) - 1, RESULT_DTYPE) for p in parts]
    tickets = []
    for k, (p, r) in enumerate(zip(parts, outs)):
        if k >= in_flight:
            ctx.wait(tickets[k - in_flight])
        ctx.mol_mate_next(p[7], p[8])
        tickets.append(ctx.submit(p[1], p[2], res=r))
    for t in tickets[max(0, len(parts) - in_flight):]:
        ctx.wait(t)
    return np.concatenate(outs)


# ---- the count ----
MAIN = [("b_f_r", 12, 20), ("b_f_r", 1, 31), ("r_s_b_f", 8, 8), ("b_f", 12, 20)]


@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
@pytest.mark.parametrize("shape,P,M", MAIN, ids=["%s-P%d-M%d" % s for s in MAIN])
def test_the_count_equals_the_yardstick(shape, P, M, spec):
    c = case(shape, M)
    want, want_tot = check_data(c, P, M)
    ctx = make_ctx(c, P, M, spec)
    try:
        assert ctx.get_option("mate_bases") == M and ctx.get_option("molecules_active") == 1
        before = ctx.get_option("spec_batches_generic")
        dres, labels, _ = run_batch(ctx, c)
        assert (ctx.get_option("spec_batches_generic") == before) == bool(spec)
        ent, tot = ctx.mol_entries()
        print(shape, P, M, "device", tot)
        assert tot == want_tot
        assert pairs(ent) == pairs(want)
        assert tot["eligible"] == tot["counted"] + tot["skipped_empty"] + tot["skipped_n"] + tot["overflow"]
        assert tot["counted"] == int(ent["count"].sum()) and tot["molecules"] == len(ent)
        # the batch itself is what it is without a mate
        assert np.array_equal(dres["read_type"], c[5]["read_type"]) and np.array_equal(labels, c[6])
        assert np.array_equal(dres["barcode"], c[5]["barcode"]) and np.array_equal(dres["fingerprint"], c[5]["fingerprint"])
        assert ctx.get_option("mate_kernel_us") >= 0 and ctx.get_option("molecules_kernel_us") >= 0
        rows, rtot = ctx.mol_get()
        from tagdust_amd import lib as tdlib
        assert rtot == tot and np.array_equal(rows, tdlib.mol_summarise(want))
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 64, 65])
def test_batches_of_one_wave_and_one_read_more_or_less(n):
    P, M = 12, 20
    c = case("b_f_r", M)
    ctx = make_ctx(c, P, M)
    try:
        for lo in (0, 700):
            p = part(c, lo, lo + n)
            want, want_tot = yardstick(p, P, M)
            ctx.mol_reset()
            run_batch(ctx, p)
            ent, tot = ctx.mol_entries()
            assert tot == want_tot and pairs(ent) == pairs(want) and tot["eligible"] > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
def test_five_submitted_batches_of_uneven_size_each_with_its_own_mates(spec):
    from tagdust_amd import lib as tdlib
    P, M = 12, 20
    c = case("b_f_r", M)
    want, want_tot = yardstick(c, P, M)
    dup, dtot = tdlib.mol_dedup_host_mated(*host_args(c, M), P)
    assert dtot["duplicates"] >= 0.2 * want_tot["eligible"]
    n = len(c[2]) - 1
    ctx = make_ctx(c, P, M, spec, dedup=True)
    try:
        ctx.set_option("pipeline_depth", 4)
        res = submit_all(ctx, c, [0, 1, 130, 131, 700, n])
        ent, tot = ctx.mol_entries()
        assert tot == want_tot and pairs(ent) == pairs(want)
        assert np.array_equal(res["read_type"] == 7, dup) and ctx.mol_dedup_get() == dtot
        assert np.array_equal(res["read_type"][~dup], c[5]["read_type"][~dup])
        assert ctx.get_option("overlap_active") == spec
    finally:
        ctx.close()


# ---- dedup, the collapse, freeze and replay ----
@pytest.mark.parametrize("shape,P,M", [("b_f_r", 12, 20), ("r_s_b_f", 8, 8), ("b_f", 12, 20)])
def test_dedup_marks_the_yardstick_s_duplicates_read_for_read(shape, P, M):
    from tagdust_amd import lib as tdlib
    c = case(shape, M)
    want, want_tot = tdlib.mol_dedup_host_mated(*host_args(c, M), P)
    mtot = yardstick(c, P, M)[1]
    plain = tdlib.mol_dedup_host(*host_args(c, 0)[:5], P)[0]
    assert want_tot["duplicates"] >= 0.2 * mtot["eligible"] and int((plain != want).sum()) >= 20     # the mate changes who is a duplicate
    assert want_tot["unjudged"] == mtot["skipped_empty"] + mtot["skipped_n"] > 10
    ctx = make_ctx(c, P, M, dedup=True)
    try:
        dres = run_batch(ctx, c)[0]
        assert np.array_equal(dres["read_type"] == 7, want)
        assert np.array_equal(dres["read_type"][~want], c[5]["read_type"][~want])
        assert ctx.mol_dedup_get() == want_tot
        assert mtot["eligible"] == want_tot["kept"] + want_tot["duplicates"]
        assert want_tot["kept"] == mtot["molecules"] + mtot["skipped_empty"] + mtot["skipped_n"]
    finally:
        ctx.close()


def test_collapse_entries_and_origins():
    from tagdust_amd import lib as tdlib
    P, M = 12, 20
    c = case("b_f_r", M)
    want, worg, want_tot = tdlib.mol_host_origins_mated(*host_args(c, M), P)
    roots, rorg, ctot = tdlib.mol_collapse_host(want, worg)
    assert ctot["absorbed"] > 5 and int(worg["n"].max()) == P + M and int(worg["n"].min()) < P + M
    ctx = make_ctx(c, P, M, collapse=True)
    try:
        run_batch(ctx, c)
        ent, org, tot = ctx.mol_origins()
        assert tot == want_tot and pairs(ent) == pairs(want) and np.array_equal(org, worg)
        cent, corg, dtot = ctx.mol_collapse_entries()
        assert pairs(cent) == pairs(roots) and np.array_equal(corg, rorg) and dtot == ctot
    finally:
        ctx.close()


@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
def test_freeze_and_replay(spec):
    from tagdust_amd import lib as tdlib
    P, M = 12, 20
    c = case("b_f_r", M)
    want, want_tot, want_ctot = tdlib.mol_dedup_collapsed_host_mated(*host_args(c, M), P)
    exact = tdlib.mol_dedup_host_mated(*host_args(c, M), P)[0]
    assert int((want != exact).sum()) > 5 and want_ctot["absorbed"] > 5
    n = len(c[2]) - 1
    ctx = make_ctx(c, P, M, spec, dedup=True, collapse=True)
    try:
        ctx.set_option("pipeline_depth", 4)
        survey = submit_all(ctx, c, [0, 500, n])
        assert np.array_equal(survey["read_type"] == 7, exact)
        mtot = ctx.mol_entries()[1]
        assert ctx.mol_dedup_freeze() == want_ctot
        replay = submit_all(ctx, c, [0, 65, 300, 900, n])
        assert np.array_equal(replay["read_type"] == 7, want) and ctx.mol_dedup_get() == want_tot
        assert ctx.mol_entries()[1] == mtot == yardstick(c, P, M)[1]       # the table stays as the survey left it
        assert mtot["eligible"] == want_tot["kept"] + want_tot["duplicates"]
        assert want_tot["kept"] == want_ctot["molecules_after"] + mtot["skipped_empty"] + mtot["skipped_n"]
        with pytest.raises(tdlib.TdError, match="no mate batch is named"):        # the replay needs its mates as the survey did
            ctx.submit(c[1], c[2], res=np.zeros(n, tdlib.RESULT_DTYPE))
        assert ctx.mol_dedup_get() == want_tot
    finally:
        ctx.close()


# ---- the failures, the other modes, off again ----
def test_failures_leave_the_totals_and_a_correct_batch_works_afterwards():
    from tagdust_amd import RESULT_DTYPE, TdError
    from tagdust_amd import lib as tdlib
    P, M = 12, 20
    c = case("b_f_r", M)
    a, b = part(c, 0, 400), part(c, 400, 800)
    ctx = make_ctx(c, P, M)
    try:
        run_batch(ctx, a)
        ent0, tot0 = ctx.mol_entries()
        assert tot0 == yardstick(a, P, M)[1] and tot0["counted"] > 0

        def unchanged():
            ent, tot = ctx.mol_entries()
            return tot == tot0 and pairs(ent) == pairs(ent0)

        # a missing mate: td_run and td_submit
        ctx.upload_batch(b[1], b[2])
        with pytest.raises(TdError, match="td_run: mate mode is on.*without a mate"):
            ctx.run()
        assert unchanged()
        r = np.zeros(400, RESULT_DTYPE)
        with pytest.raises(TdError, match="td_submit: mate mode is on.*no mate batch is named"):
            ctx.submit(b[1], b[2], res=r)
        assert unchanged()
        # a mate batch of another n_reads: td_submit and td_run; the wrong batch is dropped, not kept for the next one
        short = part(c, 400, 799)
        ctx.mol_mate_next(short[7], short[8])
        with pytest.raises(TdError, match="the named mate batch has 399 reads, the batch 400"):
            ctx.submit(b[1], b[2], res=r)
        with pytest.raises(TdError, match="no mate batch is named"):
            ctx.submit(short[1], short[2], res=r[:399])
        ctx.mol_mate_next(short[7], short[8])
        ctx.upload_batch(b[1], b[2])
        with pytest.raises(TdError, match="td_run: mate mode is on"):
            ctx.run()
        assert unchanged()
        # enable with a ticket out, and P + M > 32
        ctx.mol_mate_next(b[7], b[8])
        t = ctx.submit(b[1], b[2], res=r)
        with pytest.raises(TdError, match="td_mol_mate_enable: td_submit tickets are outstanding"):
            ctx.mol_mate_enable(M)
        with pytest.raises(TdError, match="td_mol_mate_disable: td_submit tickets are outstanding"):
            ctx.mol_mate_disable()
        ctx.wait(t)
        both = part(c, 0, 800)
        want, want_tot = yardstick(both, P, M)
        ent, tot = ctx.mol_entries()
        assert tot == want_tot and pairs(ent) == pairs(want)               # ... and the correct batch after all of it worked
        for bad in (0, -1, 21, 32):
            with pytest.raises(TdError, match="td_mol_mate_enable: mate_bases = %d with prefix_bases = 12" % bad):
                ctx.mol_mate_enable(bad)
        ent, tot = ctx.mol_entries()
        assert tot == want_tot and pairs(ent) == pairs(want) and ctx.get_option("mate_bases") == M
        # mate mode needs the count; a new model and td_mol_disable switch it off
        ctx.mol_disable()
        assert ctx.get_option("mate_bases") == 0
        with pytest.raises(TdError, match="td_mol_mate_enable: the molecule count is off"):
            ctx.mol_mate_enable(M)
        with pytest.raises(TdError, match="td_mol_mate_next: mate mode is off"):
            ctx.mol_mate_next(b[7], b[8])
        with pytest.raises(TdError, match="mate_kernel_us: mate mode is off"):
            ctx.get_option("mate_kernel_us")
        ctx.mol_enable(P, 16)
        ctx.mol_mate_enable(M)
        ctx.upload_model(c[0])
        assert ctx.get_option("mate_bases") == 0 and ctx.get_option("molecules_active") == 0
    finally:
        ctx.close()


def test_other_modes_neither_need_nor_consume_a_mate():
    from tagdust_amd import RESULT_DTYPE
    from tagdust_amd import lib as tdlib
    P, M = 12, 20
    c = case("b_f_r", M)
    a = part(c, 0, 300)
    ctx = make_ctx(c, P, M)
    try:
        ctx.upload_batch(a[1], a[2])                        # no mate named at all
        ctx.run(tdlib.MODE_GET_PROB)
        ctx.sync()
        ctx.mol_mate_next(a[7], a[8])
        r = np.zeros(300, RESULT_DTYPE)
        ctx.wait(ctx.submit(a[1], a[2], mode=tdlib.MODE_GET_PROB, res=r))
        assert not any(ctx.mol_entries()[1].values())
        ctx.wait(ctx.submit(a[1], a[2], res=r))             # the mate named before the other mode's batch is still there
        want, want_tot = yardstick(a, P, M)
        ent, tot = ctx.mol_entries()
        assert tot == want_tot and pairs(ent) == pairs(want)
    finally:
        ctx.close()


def test_mate_mode_off_again_equals_the_unmated_yardstick_on_a_fresh_table():
    P, M = 12, 20
    c = case("b_f_r", M)
    ctx = make_ctx(c, P, M, dedup=True)
    try:
        run_batch(ctx, c)
        assert ctx.mol_entries()[1] == yardstick(c, P, M)[1]
        ctx.mol_mate_disable()
        assert ctx.get_option("mate_bases") == 0
        ent, tot = ctx.mol_entries()
        assert len(ent) == 0 and not any(tot.values())      # the table is empty: it never mixes keys of two kinds
        dres = run_batch(ctx, c, mate=False)[0]
        want, want_tot = yardstick(c, P, 0)
        ent, tot = ctx.mol_entries()
        assert tot == want_tot and pairs(ent) == pairs(want)
        from tagdust_amd import lib as tdlib
        dup, dtot = tdlib.mol_dedup_host(*host_args(c, 0)[:5], P)
        assert np.array_equal(dres["read_type"] == 7, dup) and ctx.mol_dedup_get() == dtot
        ctx.mol_mate_enable(8)                              # ... and on again with another M
        assert not any(ctx.mol_entries()[1].values())
        run_batch(ctx, c)
        want, want_tot = yardstick(c, P, 8)
        ent, tot = ctx.mol_entries()
        assert tot == want_tot and pairs(ent) == pairs(want)
    finally:
        ctx.close()


# ---- the command ----
def test_the_command_on_two_fastq_files(tmp_path):
    """tagdust-hip on read 1 (barcode, UMI, read) and read 2 (the mate) with --mate-bases 20 --dedup, five batches: the _READ1 and
    _READ2 files of every barcode hold the same names in the same order, exactly those of the yardstick's kept reads"""
    import re
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    shape, P, M = "b_f_r", 12, 20
    seq, offs, mc, mo = make_pairs(shape, M, seed=8)
    mates = [mc[mo[i]:mo[i + 1]] for i in range(len(mo) - 1)]
    mc, mo = pack([m if len(m) else code("AC") for m in mates])     # (a FASTQ record has at least one base; two are still short of M)
    n = len(offs) - 1
    # the reads decoded as the command decodes them with -Q 20 and -dust 0 (threshold 0, the run's model)
    md, _ = tdlib.build_model(MATE_SHAPES[shape], seq, offs, e=0.05, d=0.1)
    ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, 0.0, 16, 0, 8)
    dup, tot = tdlib.mol_dedup_host_mated(md, seq, offs, ores, olab, (mc, mo, M), P)
    mtot = tdlib.mol_host_mated(md, seq, offs, ores, olab, (mc, mo, M), P)[1]
    plain_dup = tdlib.mol_dedup_host(md, seq, offs, ores, olab, P)[0]
    assert tot["duplicates"] >= 0.2 * mtot["eligible"] and mtot["overflow"] == 0 and int((plain_dup != dup).sum()) >= 20
    d = str(tmp_path)
    open(os.path.join(d, "r1.fq"), "wb").write(fastq_of(seq, offs))
    open(os.path.join(d, "r2.fq"), "wb").write(fastq_of(mc, mo))
    head = ["-Q", "20"] + [w for k, s in enumerate(MATE_SHAPES[shape]) for w in ("-%d" % (k + 1), s)]
    tail = ["-dust", "0", "--sync-compile", "--batch-reads", "250", "--molecules-slots", "16", "--molecules-prefix", str(P), "--mate-bases", str(M)]
    base = head + ["r1.fq", "r2.fq"] + tail
    _run(base + ["-o", "mol"], d)
    _run(base + ["--dedup", "-o", "dd"], d)
    mol, dd = _outputs(d, "mol"), _outputs(d, "dd")
    assert set(mol) == set(dd)
    first = sorted(k for k in dd if k.startswith("_BC_") and "_READ1" in k)
    assert len(first) == 8 and all(k.replace("_READ1", "_READ2") in dd for k in first)
    name = lambda r: int(re.match(rb"@r(\d+)", r).group(1))
    kept_names = set()
    for k in first:
        one = [name(r) for r in records_of(dd[k])]
        two = [name(r) for r in records_of(dd[k.replace("_READ1", "_READ2")])]
        assert one == two and one == sorted(one) and len(one) > 0, k
        plain = [name(r) for r in records_of(mol[k])]
        assert one == [i for i in plain if not dup[i]] and len(one) < len(plain), k
        assert records_of(dd[k]) == [r for r in records_of(mol[k]) if not dup[name(r)]]
        kept_names.update(one)
    ok = (np.asarray(ores["read_type"]) & 0xFF) == 0
    assert kept_names == set(np.flatnonzero(ok & ~dup).tolist())
    # <out>_molecules.txt carries the yardstick's totals and names the mate
    lines = dd["_molecules.txt"].split(b"\n")
    for want in (b"# molecules: the extracted reads of r1.fq by barcode, fingerprint and the first bases of the read", b"# prefix bases\t%d" % P,
                 b"# mate bases\t%d" % M, b"# mate file\tr2.fq", b"# extracted reads\t%d" % mtot["eligible"], b"# counted\t%d" % mtot["counted"],
                 b"# molecules\t%d" % mtot["molecules"], b"# no read base\t%d" % mtot["skipped_empty"], b"# N in the prefix\t%d" % mtot["skipped_n"],
                 b"# written\t%d" % tot["kept"], b"# duplicates removed\t%d" % tot["duplicates"]):
        assert want in lines, want
    assert lines.index(b"# mate bases\t%d" % M) == lines.index(b"# prefix bases\t%d" % P) + 1
    new = [l for l in lines if l not in mol["_molecules.txt"].split(b"\n")]
    assert new == [b"# written\t%d" % tot["kept"], b"# duplicates removed\t%d" % tot["duplicates"]]
    # the log -- its extracted count among it --, the _un files and everything else are those of the run without --dedup
    others = [k for k in dd if not k.startswith("_BC_") and k != "_molecules.txt"]
    assert any("_un" in k for k in others) and "_logfile.txt" in others
    for k in others:
        assert dd[k] == mol[k], k
    extracted = [l for l in dd["_logfile.txt"].split(b"\n") if b"extracted" in l]
    assert extracted and any(b"%d" % mtot["eligible"] in l for l in dd["_logfile.txt"].split(b"\n"))
    # the report of the library call; without the option the two files are refused as ever
    os.environ["TD_SPECIALIZE"] = "0"
    try:
        fq = [os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")]
        rep = tdlib.run_execute(["--rtest"] + head + fq + tail + ["--dedup", "-o", os.path.join(d, "rep")])
        no = pytest.raises(tdlib.TdError, tdlib.run_execute, ["--rtest"] + head + fq + ["-dust", "0", "--molecules", "-o", os.path.join(d, "no")])
    finally:
        del os.environ["TD_SPECIALIZE"]
    assert rep["dedup_totals"] == tot and rep["molecules_totals"] == mtot
    assert int(rep["counts"][0]) == mtot["eligible"] and int(rep["counts"][7]) == 0
    assert "--molecules needs exactly one input file (2 given)" in str(no.value)
