"""The base-quality filter on the device (include/tagdust_quality.h, tagdust_amd/csrc/td_quality.hip).  The yardstick is always
td_qual_host over what the same context returns with the filter off -- records and labels -- never the filtered output itself.
Batches hold at most 260 reads of 20..100 bases; the generic kernel decodes them except where a test says otherwise."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B1 = ["ACAGTG", "CTTGTA", "GGCTAC", "TTAGGC"]
ARCH = ["B:" + ",".join(B1), "F:NNNNNN", "R:N"]
SUCCESS, TOO_SHORT, LOW_COMPLEXITY, DUPLICATE, LOW_QUALITY = 0, 2, 6, 7, 8
B, F, BF = 1, 2, 3
Q, OFFSET = 20, 33
THR = OFFSET + Q
FIRST = 13                                     # bases in front of the ragged batch: its offs[0]


def code(s):
    return np.array([b"ACGTN".index(c) for c in s.encode()], np.uint8)


def structured(rng, length):
    """barcode, six UMI bases, then random bases up to `length`; now and then the barcode is a random 6-mer"""
    b = code(B1[int(rng.integers(0, 4))]) if rng.random() > 0.1 else rng.integers(0, 4, 6, dtype=np.uint8)
    return np.concatenate([b, rng.integers(0, 4, 6, dtype=np.uint8), rng.integers(0, 4, length - 12, dtype=np.uint8)])


def offsets(reads, first=0):
    offs = np.full(len(reads) + 1, first, np.int64)
    offs[1:] += np.cumsum([len(r) for r in reads])
    return offs


def generated_qualities(n_bases, seed):
    """each base low with probability 0.05"""
    rng = np.random.default_rng(seed)
    low = rng.random(n_bases) < 0.05
    return np.where(low, THR - 1 - rng.integers(0, 15, n_bases), THR + rng.integers(0, 40, n_bases)).astype(np.uint8)


_MODEL = []


def model():
    """the builder's model of ARCH over 600 structured reads, made once"""
    from tagdust_amd import lib as tdlib
    if not _MODEL:
        rng = np.random.default_rng(5)
        reads = [structured(rng, int(rng.integers(31, 101))) for _ in range(600)]
        _MODEL.append(tdlib.build_model(ARCH, np.concatenate(reads), offsets(reads))[0])
    return _MODEL[0]


_RAGGED = []


def ragged():
    """130 reads behind FIRST other bases: 64 of 20..29 bases -- with minlen 30 none of them is extracted (too short, or no match at all), and sorted by length they
    are the first tile --, 66 structured ones of 31..100 bases with 31, 32, 33, 63, 64 and 65 among them, in a shuffled order; the
    last read ends on bit 31 of the last word of low flags.  (seq, offs, qual): seq and qual hold the FIRST bytes in front as well;
    reads 100.. have three low barcode bases each and reads 115.. three low UMI bases as well, so that K = 2 has reads to fail."""
    if not _RAGGED:
        rng = np.random.default_rng(17)
        lens = [31, 32, 33, 63, 64, 65] + [int(x) for x in rng.integers(31, 101, 59)]
        reads = [rng.integers(0, 4, int(rng.integers(20, 30)), dtype=np.uint8) for _ in range(64)] + [structured(rng, ln) for ln in lens]
        order = rng.permutation(len(reads))
        reads = [reads[k] for k in order]
        total = sum(len(r) for r in reads)
        last = structured(rng, 40 + (-(total + 40)) % 32)
        reads.append(last)
        offs = offsets(reads, FIRST)
        assert len(reads) == 130 and (int(offs[-1]) - FIRST) % 32 == 0 and FIRST % 32 != 0
        seq = np.concatenate([rng.integers(0, 4, FIRST, dtype=np.uint8)] + reads)
        qual = generated_qualities(len(seq), 23)
        for i in range(100, 130):
            if offs[i + 1] - offs[i] >= 31:
                qual[offs[i] + 1:offs[i] + 4] = THR - 1
                if i >= 115:
                    qual[offs[i] + 7:offs[i] + 10] = THR - 1
        _RAGGED.append((seq, offs, qual))
    return _RAGGED[0]


@pytest.fixture()
def ctx():
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", 0)
    yield c
    c.close()


def start(ctx, minlen=30, dust=100):
    ctx.upload_model(model())
    ctx.set_params(0.5, minlen, dust)


def run_plain(ctx, seq, offs):
    """the batch through a context whose filter is off: (records, labels, seq_out)"""
    ctx.upload_batch(seq, offs)
    ctx.run()
    return ctx.download()


def run_judged(ctx, seq, offs, qual):
    ctx.qual_next(qual, len(offs) - 1)
    ctx.upload_batch(seq, offs)
    ctx.run()
    return ctx.download()


def yardstick(md, offs, plain, qual, max_low, segments, q=Q, offset=OFFSET):
    """td_qual_host over a context's own unfiltered download; the batch's first byte is offs[0] of qual"""
    from tagdust_amd import lib as tdlib
    rel = offs - offs[0]
    return tdlib.qual_host(md, rel, plain[0], plain[1][:int(rel[-1]) + len(rel) - 1], qual[int(offs[0]):int(offs[-1])], q, offset, max_low, segments)


def same_but_for_the_outcome(got, plain, want):
    assert np.array_equal(got[0]["read_type"], want["read_type"])
    for f in got[0].dtype.names:
        if f != "read_type":
            assert got[0][f].tobytes() == plain[0][f].tobytes(), f
    assert got[1].tobytes() == plain[1].tobytes() and got[2].tobytes() == plain[2].tobytes()


# ---- 1. a ragged, length-sorted batch ----
@pytest.mark.parametrize("max_low", [0, 2])
@pytest.mark.parametrize("segments", [B, F, BF], ids=["B", "F", "BF"])
def test_ragged_sorted_batch_equals_the_host(ctx, segments, max_low):
    seq, offs, qual = ragged()
    start(ctx)
    plain = run_plain(ctx, seq, offs)
    lens = np.diff(offs)
    first_tile = np.argsort(lens, kind="stable")[:64]
    assert lens[first_tile].max() < 30 and SUCCESS not in set(plain[0]["read_type"][first_tile])        # one tile without an eligible read
    want, want_tot = yardstick(model(), offs, plain, qual, max_low, segments)
    print(segments, max_low, "host totals", want_tot)
    assert want_tot["failed"] >= 1 and want_tot["passed"] >= 1
    ctx.qual_enable(Q, OFFSET, max_low, segments)
    assert ctx.get_option("quality_filter") == 1
    got = run_judged(ctx, seq, offs, qual)
    tot = ctx.qual_totals()
    assert ctx.get_option("quality_kernel_us") >= 0
    same_but_for_the_outcome(got, plain, want)
    assert tot == want_tot and tot["eligible"] == tot["passed"] + tot["failed"]
    changed = got[0]["read_type"] != plain[0]["read_type"]
    assert int(changed.sum()) == tot["failed"] and set(got[0]["read_type"][changed]) == {LOW_QUALITY}
    # the decode kernel's own tally does not know the verdicts
    assert ctx.counts()[SUCCESS] == 2 * int((plain[0]["read_type"] == SUCCESS).sum())
    # the tallies add up over batches and go back to zero
    got2 = run_judged(ctx, seq, offs, qual)
    assert np.array_equal(got2[0]["read_type"], want["read_type"])
    assert ctx.qual_totals() == {k: 2 * v for k, v in want_tot.items()}
    ctx.qual_reset()
    assert not any(ctx.qual_totals().values())


def test_offset_64(ctx):
    seq, offs, qual = ragged()
    q64 = (qual.astype(np.int32) + 31).astype(np.uint8)
    start(ctx)
    plain = run_plain(ctx, seq, offs)
    want, want_tot = yardstick(model(), offs, plain, q64, 1, BF, Q, 64)
    assert want_tot["failed"] >= 1 and want_tot["passed"] >= 1
    ctx.qual_enable(Q, 64, 1, BF)
    got = run_judged(ctx, seq, offs, q64)
    same_but_for_the_outcome(got, plain, want)
    assert ctx.qual_totals() == want_tot


# ---- 2. td_run and td_submit, three tickets in flight ----
def submit_in_parts(ctx, seq, offs, qual, parts):
    """every part with a quality array of its own -- zeros, which are low, wherever another part's bytes would be --, wiped as soon as
    td_submit has returned; at most three tickets in flight; the records in input order"""
    from tagdust_amd import RESULT_DTYPE
    res = [np.zeros(hi - lo, RESULT_DTYPE) for lo, hi in parts]
    offs_of = [np.ascontiguousarray(offs[lo:hi + 1]) for lo, hi in parts]
    tickets = []
    for k, (lo, hi) in enumerate(parts):
        if k >= 3:
            ctx.wait(tickets[k - 3])
        own = np.zeros(len(qual), np.uint8)
        own[offs[lo]:offs[hi]] = qual[offs[lo]:offs[hi]]
        ctx.qual_next(own, hi - lo)
        tickets.append(ctx.submit(seq, offs_of[k], res=res[k]))
        own[:] = 0                                  # the bytes were packed while the batch was staged
    for t in tickets[-3:]:
        ctx.wait(t)
    return np.concatenate(res)


def test_submit_with_three_tickets_in_flight_equals_td_run(ctx):
    seq, offs, qual = ragged()
    start(ctx)
    plain = run_plain(ctx, seq, offs)
    want, want_tot = yardstick(model(), offs, plain, qual, 0, BF)
    ctx.qual_enable(Q, OFFSET, 0, BF)
    got = run_judged(ctx, seq, offs, qual)
    assert np.array_equal(got[0]["read_type"], want["read_type"])
    ctx.qual_reset()
    parts = [(0, 50), (50, 51), (51, 100), (100, 129), (129, 130)]
    res = submit_in_parts(ctx, seq, offs, qual, parts)
    assert np.array_equal(res["read_type"], want["read_type"])
    for f in res.dtype.names:
        if f != "read_type":
            assert res[f].tobytes() == plain[0][f].tobytes(), f
    assert ctx.qual_totals() == want_tot


def test_submit_under_the_specialised_kernel():
    """the reference's F-B-F-R fixture, whose kernel the parity tests compile: 240 reads as three batches in flight"""
    from conftest import load_golden
    from tagdust_amd import TagdustHip, lib as tdlib
    g = load_golden("f_b_f_r")
    seq, offs = g["seq"].astype(np.uint8), g["offs"].astype(np.int64)
    qual = generated_qualities(len(seq), 29)
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 1)
        ctx.set_option("async_compile", 0)
        ctx.upload_model(g)
        ctx.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
        plain = run_plain(ctx, seq, offs)
        want, want_tot = tdlib.qual_host(g, offs, plain[0], plain[1], qual, Q, OFFSET, 0, BF)
        assert want_tot["failed"] >= 1 and want_tot["passed"] >= 1
        ctx.qual_enable(Q, OFFSET, 0, BF)
        res = submit_in_parts(ctx, seq, offs, qual, [(0, 80), (80, 160), (160, 240)])
        assert ctx.get_option("spec_state") == 3 and ctx.get_option("spec_batches_generic") == 0
        assert np.array_equal(res["read_type"], want["read_type"]) and ctx.qual_totals() == want_tot
    finally:
        ctx.close()


# ---- 3. composition ----
def pairs(entries):
    return [(int(k), int(c)) for k, c in zip(entries["key"], entries["count"])]


def test_census_molecule_count_and_dedup_read_the_verdicts(ctx):
    from tagdust_amd import lib as tdlib
    md = model()
    seq, offs, qual = ragged()
    seq, qual, offs = seq[FIRST:], qual[FIRST:], offs - FIRST
    start(ctx)
    plain = run_plain(ctx, seq, offs)
    lab = plain[1][:int(offs[-1]) + len(offs) - 1]
    want, want_tot = yardstick(md, offs, plain, qual, 0, BF)
    assert want_tot["failed"] >= 10 and want_tot["passed"] >= 10
    ctx.qual_enable(Q, OFFSET, 0, BF)
    ctx.census_enable(-1, 0xFF, 16)                 # every outcome 0..7: a dropped read has outcome 8 and is in no census
    ctx.mol_enable(20, 16)
    run_judged(ctx, seq, offs, qual)
    cen, cen_tot = ctx.census()
    want_cen, want_cen_tot = tdlib.census_host(md, seq, offs, want["read_type"], lab, -1, 0xFF)
    assert cen_tot == want_cen_tot and pairs(cen) == pairs(want_cen)
    assert cen_tot["eligible"] == len(offs) - 1 - want_tot["failed"]
    mol, mol_tot = ctx.mol_entries()
    want_mol, want_mol_tot = tdlib.mol_host(md, seq, offs, want, lab, 20)
    assert mol_tot == want_mol_tot and pairs(mol) == pairs(want_mol) and mol_tot["eligible"] == want_tot["passed"]
    ctx.mol_reset()
    ctx.mol_dedup_enable()
    twice = np.concatenate([seq, seq]), np.concatenate([offs, offs[1:] + offs[-1]]), np.concatenate([qual, qual])
    plain2_type = np.concatenate([want["read_type"], want["read_type"]])
    res = run_judged(ctx, *twice)[0]
    rec2 = np.concatenate([want, want])
    lab2 = np.concatenate([lab, lab])
    dup, dup_tot = tdlib.mol_dedup_host(md, twice[0], twice[1], rec2, lab2, 20)
    assert ctx.mol_dedup_get() == dup_tot and dup_tot["duplicates"] >= 10
    assert np.array_equal(res["read_type"] == DUPLICATE, dup) and np.array_equal(res["read_type"][~dup], plain2_type[~dup])


def test_samples_count_no_failed_read(ctx):
    from tagdust_amd import lib as tdlib
    md = model()
    seq, offs, qual = ragged()
    seq, qual, offs = seq[FIRST:], qual[FIRST:], offs - FIRST
    sheet = [[0], [2], [3]]
    start(ctx)
    plain = run_plain(ctx, seq, offs)
    lab = plain[1][:int(offs[-1]) + len(offs) - 1]
    want_q, want_tot = yardstick(md, offs, plain, qual, 0, BF)
    want, want_ent, want_s = tdlib.samples_host(md, sheet, offs, want_q, lab)
    ctx.qual_enable(Q, OFFSET, 0, BF)
    ctx.samples_enable(sheet)
    got = run_judged(ctx, seq, offs, qual)
    ent, tot = ctx.samples()
    assert tot == want_s and pairs(ent) == pairs(want_ent) and tot["eligible"] == want_tot["passed"]
    assert np.array_equal(got[0]["read_type"], want["read_type"]) and np.array_equal(got[0]["barcode"], want["barcode"])
    assert int((got[0]["read_type"] == LOW_QUALITY).sum()) == want_tot["failed"] >= 10


def test_a_pair_whose_mate_fails_keeps_the_joined_outcome(ctx):
    from tagdust_amd import lib as tdlib
    md = model()
    seq, offs, qual = ragged()
    seq, offs = seq[FIRST:], offs - FIRST
    n = len(offs) - 1
    qual = np.full(len(seq), OFFSET, np.uint8)      # every base low: every read that is still eligible fails
    rng = np.random.default_rng(3)
    mates = [np.zeros(40, np.uint8) if i % 3 == 0 else rng.integers(0, 4, 40, dtype=np.uint8) for i in range(n)]   # every third mate is poly-A
    mseq, moffs = np.concatenate(mates), offsets(mates)
    start(ctx)
    ctx.mol_enable(20, 16)
    ctx.mol_mate_enable(8)
    ctx.mol_mate_filter_enable()
    ctx.mol_mate_next(mseq, moffs)
    plain = run_plain(ctx, seq, offs)
    joined = plain[0]["read_type"]
    poly_a = np.arange(n) % 3 == 0
    assert set(joined[poly_a & (np.diff(offs) >= 30)]) == {LOW_COMPLEXITY} and int((joined == SUCCESS).sum()) >= 10
    want, want_tot = yardstick(md, offs, plain, qual, 0, BF)
    ctx.mol_reset()
    ctx.qual_enable(Q, OFFSET, 0, BF)
    ctx.mol_mate_next(mseq, moffs)
    got = run_judged(ctx, seq, offs, qual)
    assert np.array_equal(got[0]["read_type"], want["read_type"])
    assert np.array_equal(got[0]["read_type"][joined != SUCCESS], joined[joined != SUCCESS])       # the joined outcome, not 8
    assert set(got[0]["read_type"][joined == SUCCESS]) == {LOW_QUALITY}
    tot = ctx.qual_totals()
    assert tot == want_tot and tot["eligible"] == int((joined == SUCCESS).sum()) == tot["failed"]
    assert ctx.mol_entries()[1]["eligible"] == 0


# ---- 4. refusals ----
def test_refusals_leave_the_context_usable(ctx):
    from conftest import load_golden
    from tagdust_amd import RESULT_DTYPE, TdError, lib as tdlib
    seq, offs, qual = ragged()
    n = len(offs) - 1
    with pytest.raises(TdError, match="td_qual_enable: no model uploaded"):
        ctx.qual_enable(Q)
    ctx.upload_model(load_golden("c3_b6_s_r_p"))
    with pytest.raises(TdError, match="td_qual_enable: the model has no 'F' segment"):
        ctx.qual_enable(Q, OFFSET, 0, F)
    start(ctx)
    plain = run_plain(ctx, seq, offs)
    for args, msg in (((0,), "min_quality = 0"), ((94,), "min_quality = 94"), ((Q, 50), "offset = 50"), ((Q, OFFSET, -1), "max_low = -1"),
                      ((Q, OFFSET, 0, 0), "segments = 0"), ((Q, OFFSET, 0, 4), "segments = 4")):
        with pytest.raises(TdError, match="td_qual_enable: " + msg):
            ctx.qual_enable(*args)
    ctx.set_window(2, 40)
    with pytest.raises(TdError, match="td_qual_enable: a -start/-end window is set"):
        ctx.qual_enable(Q)
    ctx.set_window(-1, -1)
    with pytest.raises(TdError, match="td_qual_next: the base-quality filter is off"):
        ctx.qual_next(qual, n)
    res = np.zeros(n, RESULT_DTYPE)
    t = ctx.submit(seq, offs, res=res)
    with pytest.raises(TdError, match="td_qual_enable: td_submit tickets are outstanding"):
        ctx.qual_enable(Q)
    ctx.wait(t)
    assert ctx.get_option("quality_filter") == 0 and np.array_equal(res["read_type"], plain[0]["read_type"])
    # a resident batch staged before the enable
    ctx.upload_batch(seq, offs)
    ctx.qual_enable(Q, OFFSET, 0, BF)
    with pytest.raises(TdError, match="the base-quality filter is on .* staged without qualities named for as many reads: td_qual_next first, then td_batch_upload"):
        ctx.run()
    with pytest.raises(TdError, match="td_set_window: the base-quality filter is on"):
        ctx.set_window(2, 40)
    # no qualities named, and qualities named for another n_reads
    with pytest.raises(TdError, match="td_submit: the base-quality filter is on .* no qualities are named for this batch of 130 reads"):
        ctx.submit(seq, offs, res=res)
    ctx.qual_next(qual, n - 1)
    with pytest.raises(TdError, match="td_submit: the named qualities are those of 129 reads, the batch has 130"):
        ctx.submit(seq, offs, res=res)
    with pytest.raises(TdError, match="no qualities are named"):            # (the wrong name was dropped)
        ctx.submit(seq, offs, res=res)
    ctx.qual_next(qual, n - 1)
    ctx.upload_batch(seq, offs)
    with pytest.raises(TdError, match="staged without qualities named for as many reads"):
        ctx.run()
    assert not any(ctx.qual_totals().values())                              # nothing was decoded
    got = run_judged(ctx, seq, offs, qual)                                  # the next correct call succeeds
    want, want_tot = yardstick(model(), offs, plain, qual, 0, BF)
    assert np.array_equal(got[0]["read_type"], want["read_type"]) and ctx.qual_totals() == want_tot
    # other parameters: the resident batch belongs to the earlier enable
    ctx.qual_enable(Q, OFFSET, 2, BF)
    with pytest.raises(TdError, match="staged under an earlier td_qual_enable"):
        ctx.run()
    ctx.run(tdlib.MODE_GET_PROB)                                            # no other mode is judged, or refused
    ctx.qual_next(qual, n)
    t = ctx.submit(seq, offs, res=res)
    ctx.wait(t)
    assert int((res["read_type"] == LOW_QUALITY).sum()) == ctx.qual_totals()["failed"] >= 1
    # a new model switches the filter off
    ctx.upload_model(model())
    assert ctx.get_option("quality_filter") == 0


# ---- 5. the off state ----
def test_off_means_off(ctx):
    from tagdust_amd import TagdustHip, TdError
    seq, offs, qual = ragged()
    fresh = TagdustHip(0)
    try:
        fresh.set_option("specialize", 0)
        start(fresh)
        first = run_plain(fresh, seq, offs)
    finally:
        fresh.close()
    start(ctx)
    assert ctx.get_option("quality_filter") == 0
    for call in (ctx.qual_totals, ctx.qual_reset):
        with pytest.raises(TdError, match="the base-quality filter is off"):
            call()
    with pytest.raises(TdError, match="quality_kernel_us: the base-quality filter is off"):
        ctx.get_option("quality_kernel_us")
    ctx.qual_disable()                                  # (nothing to do)
    ctx.qual_enable(Q, OFFSET, 0, BF)
    judged = run_judged(ctx, seq, offs, qual)
    assert not np.array_equal(judged[0]["read_type"], first[0]["read_type"])
    ctx.qual_disable()
    assert ctx.get_option("quality_filter") == 0
    with pytest.raises(TdError, match="the base-quality filter is off .* staged while it was on: upload it again"):
        ctx.run()
    with pytest.raises(TdError, match="quality_kernel_us: the base-quality filter is off"):
        ctx.get_option("quality_kernel_us")
    again = run_plain(ctx, seq, offs)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, again))
    ctx.set_window(2, 40)                               # off: a window is fine
    ctx.set_window(-1, -1)


# ---- 6. the command ----
def fastq(seq, offs, qual):
    rows = []
    for i in range(len(offs) - 1):
        s = "".join("ACGTN"[b] for b in seq[offs[i]:offs[i + 1]])
        rows.append("@r%d\n%s\n+\n%s\n" % (i, s, bytes(qual[offs[i]:offs[i + 1]]).decode()))
    return "".join(rows)


def records_by_file(paths):
    """{read name: (file, its four lines)} over FASTQ files whose header lines are "@<name>;..." """
    out = {}
    for p in paths:
        lines = open(p).read().splitlines(keepends=True)
        assert len(lines) % 4 == 0
        for k in range(0, len(lines), 4):
            name = lines[k][1:].split(";")[0].strip()
            assert name not in out
            out[name] = (os.path.basename(p), "".join(lines[k:k + 4]))
    return out


def summary_lines(log_text):
    msgs = [l.split("]\t", 1)[1] for l in log_text.splitlines() if l.startswith("[") and "]\t" in l]
    return msgs[msgs.index("Done."):]


_COMMAND = []


def command_reads():
    """300 reads of 31..100 bases with printable qualities; reads 200.. have three low barcode bases"""
    if not _COMMAND:
        rng = np.random.default_rng(41)
        reads = [structured(rng, int(rng.integers(31, 101))) if rng.random() > 0.1 else rng.integers(0, 4, int(rng.integers(31, 101)), dtype=np.uint8)
                 for _ in range(300)]
        seq, offs = np.concatenate(reads), offsets(reads)
        qual = generated_qualities(len(seq), 43)
        for i in range(200, 300):
            qual[offs[i] + 1:offs[i] + 4] = THR - 1
        qual[qual == ord("@")] += 1                     # (no quality line starts like a header or a separator line)
        qual[qual == ord("+")] += 1
        _COMMAND.append((seq, offs, qual))
    return _COMMAND[0]


def command_yardstick(dust, max_low, segments):
    """What the run decodes: -Q gives every file threshold 0, and the run builds its model from the same reads with the same rates.
    (the unfiltered records, td_qual_host's records, its totals)"""
    from tagdust_amd import TagdustHip, lib as tdlib
    seq, offs, qual = command_reads()
    md = tdlib.build_model(ARCH, seq, offs)[0]
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 0)
        c.upload_model(md)
        c.set_params(0.0, 16, dust)
        plain = run_plain(c, seq, offs)
    finally:
        c.close()
    want, tot = tdlib.qual_host(md, offs, plain[0], plain[1], qual, Q, OFFSET, max_low, segments)
    return plain[0], want, tot


def run_both(d, extra_args, quality_args):
    from tagdust_amd import lib as tdlib
    base = ["--rtest", "--batch-reads", "128", "-Q", "0.5"] + [x for k, s in enumerate(ARCH) for x in ("-%d" % (k + 1), s)] + extra_args
    os.environ["TD_SPECIALIZE"] = "0"
    try:
        plain = tdlib.run_execute(base + ["-o", os.path.join(d, "plain")])
        rep = tdlib.run_execute(base + ["-o", os.path.join(d, "with")] + quality_args)
    finally:
        del os.environ["TD_SPECIALIZE"]
    return plain, rep


def check_files(d, suffix, n, failed_names):
    """every file of the run with the option is the plain run's minus the failed reads, which are in _un, in input order"""
    plain = records_by_file(glob.glob(os.path.join(d, "plain*%s.fq" % suffix)))
    assert len(plain) == n
    expect = {}
    for i in range(n):
        f, rec = plain["r%d" % i]
        f = "with" + f[len("plain"):]
        expect.setdefault(f, [])
        expect.setdefault("with_un%s.fq" % suffix, [])
        expect["with_un%s.fq" % suffix if "r%d" % i in failed_names else f].append(rec)
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "with*%s.fq" % suffix))) == sorted(expect)
    for name, rows in expect.items():
        assert open(os.path.join(d, name)).read() == "".join(rows), name
    return expect


def test_the_command_on_one_file(tmp_path):
    d = str(tmp_path)
    seq, offs, qual = command_reads()
    n = len(offs) - 1
    open(os.path.join(d, "in.fq"), "w").write(fastq(seq, offs, qual))
    unfiltered, want, tot = command_yardstick(100, 1, BF)
    print("host totals", tot)
    assert tot["failed"] >= 20 and tot["passed"] >= 20
    plain, rep = run_both(d, [os.path.join(d, "in.fq")], ["--min-base-quality", str(Q), "--max-low-bases", "1"])
    assert plain["quality_totals"] is None and rep["quality_totals"] == tot
    failed = {"r%d" % i for i in range(n) if want["read_type"][i] == LOW_QUALITY}
    expect = check_files(d, "", n, failed)
    assert len(expect["with_un.fq"]) == int((unfiltered["read_type"] != SUCCESS).sum()) + tot["failed"]
    # the log: the same summary, the failed reads moved, one line more
    a, b = summary_lines(plain["log"]), summary_lines(rep["log"])
    assert b[-1] == "%d\tlow base quality in barcode / UMI (Q < %d, more than 1 bases)" % (tot["failed"], Q) and len(b) == len(a) + 1
    assert "low base quality" not in plain["log"]
    assert rep["counts"][SUCCESS] == plain["counts"][SUCCESS] - tot["failed"] and rep["counts"][3] == plain["counts"][3] + tot["failed"]
    assert "%d\tsuccessfully extracted" % (plain["counts"][SUCCESS] - tot["failed"]) in b
    assert rep["counts"][:8].sum() == plain["counts"][:8].sum() == n


def test_the_command_on_a_pair_with_mate_bases(tmp_path):
    d = str(tmp_path)
    seq, offs, qual = command_reads()
    n = len(offs) - 1
    rng = np.random.default_rng(8)
    mates = [rng.integers(0, 4, 40, dtype=np.uint8) for _ in range(n)]
    open(os.path.join(d, "in.fq"), "w").write(fastq(seq, offs, qual))
    open(os.path.join(d, "in2.fq"), "w").write(fastq(np.concatenate(mates), offsets(mates), np.full(40 * n, ord("#"), np.uint8)))   # the mate's qualities are not judged
    unfiltered, want, tot = command_yardstick(0, 0, B)
    assert tot["failed"] >= 20 and tot["passed"] >= 20
    plain, rep = run_both(d, [os.path.join(d, "in.fq"), os.path.join(d, "in2.fq"), "--mate-bases", "8", "-dust", "0"],
                          ["--min-base-quality", str(Q), "--quality-segments", "B"])
    assert rep["quality_totals"] == tot
    failed = {"r%d" % i for i in range(n) if want["read_type"][i] == LOW_QUALITY}
    for k in (1, 2):
        expect = check_files(d, "_READ%d" % k, n, failed)
        assert len(expect["with_un_READ%d.fq" % k]) == int((unfiltered["read_type"] != SUCCESS).sum()) + tot["failed"]
    assert rep["counts"][SUCCESS] == plain["counts"][SUCCESS] - tot["failed"] and rep["counts"][3] == plain["counts"][3] + tot["failed"]
    assert summary_lines(rep["log"])[-1] == "%d\tlow base quality in barcode / UMI (Q < %d, more than 0 bases)" % (tot["failed"], Q)
    assert rep["molecules_totals"]["eligible"] == tot["passed"]               # the count behind the filter sees the verdicts


def test_the_command_refuses_fasta(tmp_path):
    from tagdust_amd import TdError, lib as tdlib
    d = str(tmp_path)
    seq, offs, _ = command_reads()
    rows = [">r%d\n%s\n" % (i, "".join("ACGTN"[b] for b in seq[offs[i]:offs[i + 1]])) for i in range(len(offs) - 1)]
    open(os.path.join(d, "in.fa"), "w").write("".join(rows))
    args = ["--rtest", "-Q", "0.5"] + [x for k, s in enumerate(ARCH) for x in ("-%d" % (k + 1), s)] + [os.path.join(d, "in.fa"), "-o", os.path.join(d, "fa")]
    os.environ["TD_SPECIALIZE"] = "0"
    try:
        with pytest.raises(TdError, match=r'the base-quality filter is on and record "r0" of .*in\.fa has no quality line \(FASTA\)'):
            tdlib.run_execute(args + ["--min-base-quality", str(Q)])
        tdlib.run_execute(args + ["--force"])                                  # without the option the file runs
    finally:
        del os.environ["TD_SPECIALIZE"]
