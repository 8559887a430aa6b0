"""One read per collapsed molecule on the device (include/tagdust_molecules.h: survey, td_mol_dedup_freeze, replay;
tagdust_amd/csrc/td_molecules.hip).  The yardstick is td_mol_dedup_collapsed_host fed with the CPU oracle's labels, outcomes,
barcodes and fingerprints for the same reads in the caller's order (oracle/pyoracle.py), never the device's own output -- but for
the table of 16 slots, where which keys overflow is the device's to say: there the restatement of tests/test_dedup_collapsed.py is
given the device's td_mol_origins.  Compared read for read on read_type; every other field of every record, the labels and the
rewritten sequences must equal a plain decode of the same reads; the three tallies are compared as well.  The table has 2^16
slots unless noted, so the yardstick's overflow of 0 holds.  Helpers of tests/test_molecules_gpu.py and tests/test_collapse_gpu.py
are used as they are."""
import gzip
import os

import numpy as np
import pytest

from test_collapse_gpu import ARCH, begin, exact_case, noise_case
from test_dedup_collapsed import check_identities, classify, hand_ordered, replay_py
from test_molecules_gpu import BARCODES, code, fastq_of, pack, _outputs, _run

pytestmark = pytest.mark.gpu

_CASES = {}


# ---- the cases ----
def decoded_by(md, seq, offs, thr=5.0, minlen=16):
    """a case as test_collapse_gpu.decoded gives it, under a model that another case already has (one compile serves both)"""
    from oracle import pyoracle
    ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, minlen, 100, 2)
    return (md, seq, offs, thr, minlen, {f: np.asarray(ores[f]).copy() for f in ("read_type", "barcode", "fingerprint")}, olab)


def hand_ordered_case():
    """the hand-ordered molecules of tests/test_dedup_collapsed.py as reads a decoder sees: barcode, UMI of 4, 50 read bases.  The
    read without a read base is no extracted read to a decoder (the architecture does not match): here it is a failed record in the
    middle of the wave, and the empty class is the host test's."""
    if "hand" not in _CASES:
        read = np.random.default_rng(44).integers(0, 4, 50, dtype=np.uint8)
        reads = []
        for b, umi, _, special in hand_ordered():
            r = read.copy()
            if special == "n":
                r[3] = 4
            reads.append(np.concatenate([code(BARCODES[b]), code(umi), r[:0] if special == "empty" else r]))
        _CASES["hand"] = decoded_by(exact_case(4)[0][0], *pack(reads))
    return _CASES["hand"]


def ragged_case():
    """the noise case with every third read one to three bases shorter at its end, behind every prefix: the batch is sorted by
    length on the device, and a molecule's reads no longer stay in the caller's order there"""
    if "ragged" not in _CASES:
        _, seq, offs = noise_case()[:3]
        rng = np.random.default_rng(105)
        reads = []
        for i in range(len(offs) - 1):
            r = seq[offs[i]:offs[i + 1]]
            reads.append(r[:len(r) - int(rng.integers(1, 4))] if i % 3 == 0 else r)
        _CASES["ragged"] = decoded_by(noise_case()[0], *pack(reads))
    return _CASES["ragged"]


def part(c, lo, hi):
    """reads lo..hi of a case as a case"""
    md, seq, offs, thr, minlen, res, lab = c
    return md, seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo], thr, minlen, {f: v[lo:hi] for f, v in res.items()}, lab[offs[lo] + lo:offs[hi] + hi]


def in_order(c, order):
    """the case's reads, records and labels in another order"""
    md, seq, offs, thr, minlen, res, lab = c
    rseq, roffs = pack([seq[offs[i]:offs[i + 1]] for i in order])
    rlab = np.concatenate([lab[offs[i] + i:offs[i + 1] + i + 1] for i in order]).astype(np.int8)
    return md, rseq, roffs, thr, minlen, {f: v[order] for f, v in res.items()}, rlab


def want_of(c, P):
    """td_mol_dedup_collapsed_host over a case: (is_duplicate per read, dedup totals, collapse totals)"""
    from tagdust_amd import lib as tdlib
    md, seq, offs, _, _, res, lab = c
    return tdlib.mol_dedup_collapsed_host(md, seq, offs, res, lab, P)


def classes_of(c, P):
    md, seq, offs, _, _, res, lab = c
    return classify(md, seq, offs, res, lab, P)


# ---- the device ----
def make_ctx(c, P, spec=0, log2_slots=16):
    """a context with the case's model and count, dedup and collapse on: it surveys"""
    from tagdust_amd import TagdustHip
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 1 if spec else 0)
        ctx.set_option("async_compile", 0)
        ctx.set_option("pipeline_depth", 4)
        begin(ctx, c, P, log2_slots)
        ctx.mol_dedup_enable()
        assert ctx.get_option("dedup_frozen") == 0
    except Exception:
        ctx.close()
        raise
    return ctx


def run_batch(ctx, c, lo=0, hi=None):
    """one td_run batch of reads lo..hi: records, labels and rewritten sequences as downloaded"""
    _, seq, offs = c[:3]
    hi = len(offs) - 1 if hi is None else hi
    ctx.upload_batch(seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo])
    ctx.run()
    return ctx.download()


def run_all(ctx, c, parts):
    return np.concatenate([run_batch(ctx, c, lo, hi)[0] for lo, hi in parts])


def submit_all(ctx, c, parts, in_flight=4):
    """the parts through td_submit with as many tickets in flight as a context holds (four); the records, joined"""
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


def plain_decode(c, name, spec=0):
    """(records, labels, rewritten sequences) of the case on a context without a count, by the same kernel variant, computed once"""
    from tagdust_amd import TagdustHip
    if ("plain", name, spec) not in _CASES:
        md, _, _, thr, minlen, _, _ = c
        ctx = TagdustHip(0)
        try:
            ctx.set_option("specialize", 1 if spec else 0)
            ctx.set_option("async_compile", 0)
            ctx.upload_model(md)
            ctx.set_params(thr, minlen, 100)
            _CASES[("plain", name, spec)] = run_batch(ctx, c)
        finally:
            ctx.close()
    return _CASES[("plain", name, spec)]


def check_records(c, name, got, want, lo=0, hi=None, spec=0):
    """the duplicates are the yardstick's, read for read; everything else of every record is the plain decode's, which carries the
    oracle's outcomes, barcodes and fingerprints"""
    hi = len(c[2]) - 1 if hi is None else hi
    plain = plain_decode(c, name, spec)[0][lo:hi]
    res = c[5]
    assert np.array_equal(plain["read_type"], res["read_type"][lo:hi]) and np.array_equal(plain["barcode"], res["barcode"][lo:hi])
    assert np.array_equal(plain["fingerprint"], res["fingerprint"][lo:hi])
    assert np.array_equal((got["read_type"] & 0xFF) == 7, want)
    assert np.array_equal(got["read_type"], np.where(want, (plain["read_type"] & ~0xFF) | 7, plain["read_type"]))
    for f in got.dtype.names:
        if f != "read_type":
            assert np.array_equal(got[f].view(np.uint32), plain[f].view(np.uint32)), f


# ---- one batch, read for read: fewer than 64 reads, one partial wave ----
CORE = {"hand-ordered": (hand_ordered_case, 20), "exact-4": (lambda: exact_case(4)[0], 20), "exact-8": (lambda: exact_case(8)[0], 20)}


@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
@pytest.mark.parametrize("name", sorted(CORE))
def test_one_wave_keeps_the_yardstick_s_read_of_every_tree(name, spec):
    from tagdust_amd import lib as tdlib
    c, P = CORE[name][0](), CORE[name][1]
    md, seq, offs, _, _, res, lab = c
    n = len(offs) - 1
    want, want_tot, want_ctot = want_of(c, P)
    classes = classes_of(c, P)
    # the yardstick's side first
    print(name, want_tot, want_ctot)
    assert 0 < n < 64 and want_ctot["absorbed"] > 0 and want_ctot["longest_chain"] == 2
    check_identities(classes, want_tot, want_ctot)
    exact, exact_tot = tdlib.mol_dedup_host(md, seq, offs, res, lab, P)
    assert exact_tot["duplicates"] + want_ctot["absorbed"] == want_tot["duplicates"] and not np.array_equal(exact, want)
    if name == "hand-ordered":                            # the root's first read, not the tree's
        assert not want[2] and want[0] and want[1] and classes.count("n") == 1 and classes.count(None) == 1
        assert not np.array_equal(replay_py(classes, rule="min")[0], want)
    ctx = make_ctx(c, P, spec)
    try:
        before = ctx.get_option("spec_batches_generic")
        surveyed, _, _ = run_batch(ctx, c)
        assert np.array_equal((surveyed["read_type"] & 0xFF) == 7, exact)          # the survey is today's exact dedup
        assert ctx.mol_dedup_freeze() == want_ctot and ctx.get_option("dedup_frozen") == 1
        assert ctx.mol_dedup_get() == {"kept": 0, "duplicates": 0, "unjudged": 0}
        got, labels, seq_out = run_batch(ctx, c)
        assert (ctx.get_option("spec_batches_generic") == before) == bool(spec)
        check_records(c, name, got, want, spec=spec)
        plain = plain_decode(c, name, spec)
        assert np.array_equal(labels, plain[1]) and np.array_equal(labels, lab) and np.array_equal(seq_out, plain[2])
        assert ctx.mol_dedup_get() == want_tot
        assert ctx.get_option("dedup_replay_kernel_us") >= 0
        # every written judged read spells an entry of td_mol_collapse_entries
        roots = set(int(k) for k in ctx.mol_collapse_entries()[0]["key"])
        kept = [classes[i][0] for i in range(n) if isinstance(classes[i], tuple) and not want[i]]
        assert sorted(kept) == sorted(roots)
    finally:
        ctx.close()


# ---- 1200 reads, a partial last wave: neither pass's batching matters ----
@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
def test_neither_pass_s_batching_matters(spec):
    """Surveyed in one td_run and replayed in five td_submit batches with as many tickets in flight as a context holds (four: the
    fifth is submitted when the first has been waited for); surveyed in four td_submit batches, all in flight, and replayed in
    uneven td_run batches, one of them with no read; a replay of the first 500 reads alone.  Behind the specialised kernel
    neighbouring batches run on the two compute streams."""
    c = noise_case()
    P = 16
    n = len(c[2]) - 1
    want, want_tot, want_ctot = want_of(c, P)
    classes = classes_of(c, P)
    print("noise", want_tot, want_ctot)
    assert n == 1200 and n % 64 != 0 and want_ctot["absorbed"] > 40 and want_tot["duplicates"] > 0.5 * n
    check_identities(classes, want_tot, want_ctot)
    ctx = make_ctx(c, P, spec)
    try:
        run_batch(ctx, c)
        assert ctx.mol_dedup_freeze() == want_ctot
        got = submit_all(ctx, c, [(k, k + 240) for k in range(0, n, 240)])
        check_records(c, "noise", got, want, spec=spec)
        assert ctx.mol_dedup_get() == want_tot
        assert ctx.get_option("overlap_active") == spec

        ctx.mol_reset()
        assert ctx.get_option("dedup_frozen") == 0
        submit_all(ctx, c, [(k, k + 300) for k in range(0, n, 300)])
        assert ctx.mol_dedup_freeze() == want_ctot
        got = run_all(ctx, c, [(0, 1), (1, 65), (65, 65), (65, 700), (700, n)])
        check_records(c, "noise", got, want, spec=spec)
        assert ctx.mol_dedup_get() == want_tot

        assert ctx.mol_dedup_freeze() == want_ctot                 # again: the ordinals start over
        got = run_all(ctx, c, [(0, 130), (130, 500)])
        check_records(c, "noise", got, want[:500], 0, 500, spec=spec)
        tot = ctx.mol_dedup_get()
        assert tot["duplicates"] == int(want[:500].sum()) and tot["kept"] + tot["duplicates"] == sum(x is not None for x in classes[:500])
    finally:
        ctx.close()


# ---- reads of differing lengths: the caller's order, not the device's ----
@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
def test_the_ordinal_is_the_caller_s_not_the_device_s(spec):
    c = ragged_case()
    P = 16
    n = len(c[2]) - 1
    want, want_tot, want_ctot = want_of(c, P)
    check_identities(classes_of(c, P), want_tot, want_ctot)
    # the device decodes in the order of a stable sort by length: judged in that order, other reads would stay
    lens = np.diff(c[2])
    dev = np.argsort(lens, kind="stable")
    assert not np.array_equal(dev, np.arange(n))
    dev_marks = np.zeros(n, bool)
    dev_marks[dev] = want_of(in_order(c, dev), P)[0]
    differ = int((dev_marks != want).sum())
    print("reads the device order would mark otherwise:", differ)
    assert differ >= 20 and int(dev_marks.sum()) == int(want.sum())
    ctx = make_ctx(c, P, spec)
    try:
        run_batch(ctx, c)
        assert ctx.mol_dedup_freeze() == want_ctot
        got, labels, _ = run_batch(ctx, c)
        check_records(c, "ragged", got, want, spec=spec)
        assert np.array_equal(labels, c[6]) and ctx.mol_dedup_get() == want_tot
        assert ctx.mol_dedup_freeze() == want_ctot
        check_records(c, "ragged", submit_all(ctx, c, [(0, 500), (500, 501), (501, n)]), want, spec=spec)
        assert ctx.mol_dedup_get() == want_tot
    finally:
        ctx.close()


# ---- a table of 16 slots ----
def test_a_table_of_sixteen_slots_keeps_what_it_does_not_hold():
    """which keys overflow is the device's to say: the restatement is given the device's td_mol_origins and treats every read whose
    key is not among them as unjudged"""
    c, _ = exact_case(4, extra=12)
    P = 20
    classes = classes_of(c, P)
    assert len({x[0] for x in classes if isinstance(x, tuple)}) == 27
    ctx = make_ctx(c, P, 0, log2_slots=4)
    try:
        run_batch(ctx, c)
        ent, org, mtot = ctx.mol_origins()
        held = {int(k): (int(v), o) for (k, v), o in zip(ent.tolist(), org.tolist())}
        want, want_tot, want_ctot = replay_py(classes, held=held)
        ctot = ctx.mol_dedup_freeze()
        assert mtot["overflow"] > 0 and len(held) == 16 and {k: ctot[k] for k in want_ctot} == want_ctot
        got, _, _ = run_batch(ctx, c)
        check_records(c, "sixteen", got, want)
        tot = ctx.mol_dedup_get()
        print("sixteen slots", tot, mtot, ctot)
        assert tot == want_tot and tot["unjudged"] == mtot["overflow"] + mtot["skipped_empty"] + mtot["skipped_n"]
        assert tot["kept"] == ctot["molecules_after"] + mtot["skipped_empty"] + mtot["skipped_n"] + mtot["overflow"]
        assert mtot["eligible"] == tot["kept"] + tot["duplicates"] and ctx.mol_origins()[2] == mtot
    finally:
        ctx.close()


# ---- state ----
def test_freeze_is_refused_without_its_three_parts_and_with_a_ticket_outstanding():
    from tagdust_amd import RESULT_DTYPE, TagdustHip, TdError
    from test_molecules_gpu import start
    c = noise_case()
    _, seq, offs = c[:3]
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 0)
        ctx.upload_model(c[0])
        with pytest.raises(TdError, match="td_mol_dedup_freeze: the molecule count is off"):
            ctx.mol_dedup_freeze()
        start(ctx, c, 16)
        ctx.mol_collapse_enable()
        with pytest.raises(TdError, match="td_mol_dedup_freeze: dedup is off"):
            ctx.mol_dedup_freeze()
        ctx.mol_collapse_disable()
        ctx.mol_dedup_enable()
        with pytest.raises(TdError, match="td_mol_dedup_freeze: the collapse is off"):
            ctx.mol_dedup_freeze()
        ctx.mol_collapse_enable()
        res = np.zeros(300, RESULT_DTYPE)
        t = ctx.submit(np.ascontiguousarray(seq[:offs[300]]), np.ascontiguousarray(offs[:301]), res=res)
        with pytest.raises(TdError, match="td_mol_dedup_freeze: td_submit tickets are outstanding"):
            ctx.mol_dedup_freeze()
        ctx.wait(t)
        assert ctx.get_option("dedup_frozen") == 0
        with pytest.raises(TdError, match="not frozen"):
            ctx.get_option("dedup_replay_kernel_us")
        ctx.mol_dedup_freeze()
        assert ctx.get_option("dedup_frozen") == 1
    finally:
        ctx.close()


def same_tables(a, b):
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v


def tables(ctx):
    return [ctx.mol_entries(), ctx.mol_origins(), ctx.mol_collapse_entries(), ctx.mol_get(), ctx.mol_collapse_get()]


def test_the_frozen_table_stays_and_a_reset_surveys_again():
    from tagdust_amd import lib as tdlib
    c = noise_case()
    md, seq, offs, _, _, res, lab = c
    P = 16
    want, want_tot, want_ctot = want_of(c, P)
    exact, exact_tot = tdlib.mol_dedup_host(md, seq, offs, res, lab, P)
    counted = np.array([isinstance(x, tuple) for x in classes_of(c, P)])
    ctx = make_ctx(c, P)
    try:
        run_batch(ctx, c)
        surveyed = tables(ctx)
        ctx.mol_dedup_freeze()
        same_tables(tables(ctx), surveyed)
        check_records(c, "noise", run_batch(ctx, c)[0], want)
        same_tables(tables(ctx), surveyed)                       # keys, counts, origins and the count's totals: the survey's
        same_tables(tables(ctx), surveyed)                       # ... as often as asked
        # the same reads once more without a freeze: their ordinals go on from 1200, no read is anybody's keeper
        again = run_batch(ctx, c)[0]
        assert np.array_equal((again["read_type"] & 0xFF) == 7, counted)
        assert ctx.mol_dedup_get() == {"kept": want_tot["kept"], "duplicates": want_tot["duplicates"] + int(counted.sum()), "unjudged": want_tot["unjudged"]}
        # freeze again: the ordinals start over, the tallies with them
        assert ctx.mol_dedup_freeze() == want_ctot
        check_records(c, "noise", run_batch(ctx, c)[0], want)
        assert ctx.mol_dedup_get() == want_tot
        same_tables(tables(ctx), surveyed)
        ctx.mol_reset()
        assert ctx.get_option("dedup_frozen") == 0 and len(ctx.mol_entries()[0]) == 0
        check_records(c, "noise", run_batch(ctx, c)[0], exact)   # it surveys again: exact dedup, as td_mol_dedup_host says
        assert ctx.mol_dedup_get() == exact_tot
        ctx.mol_dedup_freeze()
        for disable in (ctx.mol_dedup_disable, ctx.mol_collapse_disable):
            assert ctx.get_option("dedup_frozen") == 1
            disable()                                            # the frozen state ends with an empty table
            assert ctx.get_option("dedup_frozen") == 0 and len(ctx.mol_entries()[0]) == 0 and ctx.get_option("molecules_active") == 1
            ctx.mol_dedup_enable()
            ctx.mol_collapse_enable()
            run_batch(ctx, c, 0, 300)
            ctx.mol_dedup_freeze()
        ctx.upload_model(md)                                     # a new model: the count goes, the state with it
        assert ctx.get_option("dedup_frozen") == 0 and ctx.get_option("molecules_active") == 0
    finally:
        ctx.close()


def test_a_replay_of_reads_never_surveyed_keeps_them_unjudged():
    c = noise_case()
    P = 16
    n = len(c[2]) - 1
    classes = classes_of(c, P)
    want, want_tot, _ = replay_py(classes[:600], classes)        # the first half surveyed, the whole replayed
    held = {x[0] for x in classes[:600] if isinstance(x, tuple)}
    fresh = sum(isinstance(x, tuple) and x[0] not in held for x in classes)
    assert fresh > 20 and want_tot["unjudged"] == fresh
    ctx = make_ctx(c, P)
    try:
        run_batch(ctx, c, 0, 600)
        ctx.mol_dedup_freeze()
        check_records(c, "noise", run_batch(ctx, c)[0], want)
        assert ctx.mol_dedup_get() == want_tot
    finally:
        ctx.close()


def test_two_contexts_on_one_device_are_independent():
    c = noise_case()
    P = 16
    n = len(c[2]) - 1
    half = part(c, 0, 600)
    want_a, tot_a, ctot_a = want_of(half, P)
    want_b, tot_b, ctot_b = want_of(c, P)
    assert not np.array_equal(want_a, want_b[:600])
    a, b = make_ctx(c, P), make_ctx(c, P, spec=1)
    try:
        run_batch(a, c, 0, 600)
        run_batch(b, c)
        assert a.mol_dedup_freeze() == ctot_a
        assert b.get_option("dedup_frozen") == 0 and a.get_option("dedup_frozen") == 1
        got_a = run_batch(a, c, 0, 600)[0]
        assert b.mol_dedup_freeze() == ctot_b
        got_b = submit_all(b, c, [(0, 400), (400, n)])
        check_records(c, "noise", got_a, want_a, 0, 600)
        check_records(c, "noise", got_b, want_b, spec=1)
        assert a.mol_dedup_get() == tot_a and b.mol_dedup_get() == tot_b
    finally:
        a.close()
        b.close()


# ---- the command ----
def records_of(data):
    lines = data.split(b"\n")
    return [b"\n".join(lines[k:k + 4]) for k in range(0, len(lines) - 1, 4)]


def command_case():
    """The noise case with 80 reads among its 1200 that are not extracted -- 40 with a read of one base (low complexity at -dust
    10), 30 with a barcode that is not listed, 10 too short -- so that the log's counters and the census of --unknown-barcodes have
    something to say; decoded as the command decodes with -Q 20 -dust 10: threshold 0, the run's model."""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    if "command" not in _CASES:
        _, seq, offs = noise_case()[:3]
        rng = np.random.default_rng(23)
        reads = [seq[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
        umi = lambda: rng.integers(0, 4, 8, dtype=np.uint8)
        extra = [np.concatenate([code(BARCODES[q % 8]), umi(), np.full(50, q & 3, np.uint8)]) for q in range(40)]
        extra += [np.concatenate([code(["GGGGGG", "CTCTCT", "TATATA"][q % 3]), umi(), rng.integers(0, 4, 50, dtype=np.uint8)]) for q in range(30)]
        extra += [np.concatenate([code(BARCODES[q % 8]), umi(), rng.integers(0, 4, 6, dtype=np.uint8)]) for q in range(10)]
        for p, e in zip(sorted(rng.choice(len(reads), len(extra), replace=False).tolist(), reverse=True), extra):
            reads.insert(p, e)
        seq, offs = pack(reads)
        md, _ = tdlib.build_model(ARCH[8], seq, offs, e=0.05, d=0.1)
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, 0.0, 16, 10, 8)
        res = {f: np.asarray(ores[f]).copy() for f in ("read_type", "barcode", "fingerprint")}
        _CASES["command"] = (md, seq, offs, 0.0, 16, res, olab)
    return _CASES["command"]


@pytest.mark.parametrize("infile", ["in.fq", "in.fq.gz"])
def test_the_command_writes_one_read_per_collapsed_molecule(tmp_path, infile):
    from tagdust_amd import lib as tdlib
    c = command_case()
    md, seq, offs, _, _, res, lab = c
    P = 20
    dup, tot, ctot = want_of(c, P)
    exact, exact_tot = tdlib.mol_dedup_host(md, seq, offs, res, lab, P)
    outcomes = np.bincount(res["read_type"] & 0xFF, minlength=8)
    print("command", outcomes.tolist(), tot, ctot)
    assert outcomes[0] >= 1100 and outcomes[6] >= 30 and outcomes[1] + outcomes[3] >= 20 and ctot["absorbed"] > 40
    d = str(tmp_path)
    text = fastq_of(seq, offs)
    open(os.path.join(d, infile), "wb").write(gzip.compress(text) if infile.endswith(".gz") else text)
    base = ["-Q", "20", "-dust", "10"] + [w for k, s in enumerate(ARCH[8]) for w in ("-%d" % (k + 1), s)]
    base += [infile, "--sync-compile", "--batch-reads", "250", "--molecules-slots", "14", "--unknown-barcodes", "5"]   # six batches
    _run(base + ["--dedup", "--collapse-umis", "-o", "two"], d)
    _run(base + ["--dedup-collapsed", "-o", "one"], d)
    two, one = _outputs(d, "two"), _outputs(d, "one")
    assert set(two) == set(one) and "_unknown_barcodes.txt" in one
    # the barcode files: exactly the reads the yardstick keeps, in input order.  (The read a tree keeps is the first of its root's
    # own key, so it is among the reads exact dedup keeps: the other run's files hold every record that is wanted here.)
    assert not (exact & ~dup).any()
    bars = sorted(k for k in one if k.startswith("_BC_"))
    assert len(bars) == 8
    kept_ids = []
    for k in bars:
        records = records_of(two[k])
        ids = [int(r.split(b";", 1)[0][2:]) for r in records]
        assert ids == sorted(ids) and len(ids) > 0
        assert records_of(one[k]) == [r for r, i in zip(records, ids) if not dup[i]], k
        kept_ids += [int(r.split(b";", 1)[0][2:]) for r in records_of(one[k])]
    ok = (res["read_type"] & 0xFF) == 0
    assert sorted(kept_ids) == np.flatnonzero(ok & ~dup).tolist() and len(kept_ids) == tot["kept"] < exact_tot["kept"]
    # the log, _un and the census report one pass: byte for byte those of the run that reads the file once
    others = [k for k in one if k not in bars and k != "_molecules.txt"]
    assert "_logfile.txt" in others and any("_un" in k for k in others)
    for k in others:
        assert one[k] == two[k], k
    assert b"%d\ttotal input reads" % (len(offs) - 1) in one["_logfile.txt"] and b"%d\tlow complexity" % outcomes[6] in one["_logfile.txt"]
    assert len(one["_unknown_barcodes.txt"].splitlines()) > 8
    # <out>_molecules.txt: two values and one new line
    a, b = two["_molecules.txt"].split(b"\n"), one["_molecules.txt"].split(b"\n")
    assert b"# written\t%d" % exact_tot["kept"] in a and b"# duplicates removed\t%d" % exact_tot["duplicates"] in a
    at = b.index(b"# dedup\tcollapsed molecules")
    assert b[at + 1:at + 3] == [b"# written\t%d" % tot["kept"], b"# duplicates removed\t%d" % tot["duplicates"]]
    assert a[at:at + 2] == [b"# written\t%d" % exact_tot["kept"], b"# duplicates removed\t%d" % exact_tot["duplicates"]]
    assert b[:at] + b[at + 3:] == a[:at] + a[at + 2:]
    assert tot["kept"] == ctot["molecules_after"] + tot["unjudged"]
    assert b"# molecules after collapse\t%d" % ctot["molecules_after"] in b    # the files agree with the table
    if infile == "in.fq":                                        # the report of the library call
        os.environ["TD_SPECIALIZE"] = "0"
        try:
            rep = tdlib.run_execute(["--rtest"] + base[:base.index(infile)] + [os.path.join(d, infile)] + base[base.index(infile) + 1:]
                                    + ["--dedup-collapsed", "-o", os.path.join(d, "rep")])
        finally:
            del os.environ["TD_SPECIALIZE"]
        assert rep["dedup_collapsed"] and rep["dedup_totals"] == tot and rep["collapse_totals"] == ctot and rep["survey_s"] > 0
        assert rep["counts"][:8].tolist() == outcomes.tolist() and rep["stream"]["n_reads"] == len(offs) - 1
