"""The UMI collapse on the device (include/tagdust_molecules.h, td_mol_collapse_*; tagdust_amd/csrc/td_molecules.hip).  The yardstick
is td_mol_collapse_host over td_mol_host_origins fed with the CPU oracle's labels, outcomes, barcodes and fingerprints for the same
reads (oracle/pyoracle.py), never with the device's own output -- but for the table of 16 slots, where which keys overflow is the
device's to say and the yardstick is given the device's td_mol_origins.  Compared entry for entry, origin for origin, totals for
totals.  Helpers of tests/test_molecules_gpu.py are used as they are."""
import os

import numpy as np
import pytest

from test_molecules_gpu import BARCODES, code, fastq_of, molecules_text, pack, run_batch, start, _outputs, _run

pytestmark = pytest.mark.gpu

ARCH = {4: ["B:" + ",".join(BARCODES), "F:NNNN", "R:N"], 8: ["B:" + ",".join(BARCODES), "F:NNNNNNNN", "R:N"]}
_CASES = {}


def i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def fingerprint_of(umi):
    v = 0
    for ch in umi:
        v = (v << 2) | "ACGT".index(ch)
    return i32((v << 8) | len(umi))


def decoded(segs, seq, offs, thr=5.0, minlen=16, threads=2, **model_kw):
    """a case as tests/test_molecules_gpu.py's helpers take it: (model, seq, offs, threshold, minlen, the oracle's records and labels)"""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    md, _ = tdlib.build_model(segs, seq, offs, **model_kw)
    ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, minlen, 100, threads)
    return (md, seq, offs, thr, minlen, {f: np.asarray(ores[f]).copy() for f in ("read_type", "barcode", "fingerprint")}, olab)


def exact_molecules(L):
    """[(barcode index, UMI, read index, copies)]: the chain, the threshold pair on either side, the singleton ties, the cross-bin
    pair and a pair that differs in the read; UMIs of 8 get a fixed head in front of the four bases that vary"""
    head = "" if L == 4 else "GTCA"
    mols = [(0, "AAAA", 0, 10), (0, "AAAC", 0, 5), (0, "AACC", 0, 3),          # 10 <- 5 <- 3, the 3 two mismatches from the 10
            (1, "ACGT", 0, 5), (1, "ACGA", 0, 8),                              # 8 < 2 * 5 - 1: two roots
            (2, "ACGT", 0, 5), (2, "ACGA", 0, 9),                              # 9: one root
            (3, "GGGG", 0, 1), (3, "GGGT", 0, 1),                              # the smaller key is the root
            (4, "TTTA", 0, 1), (4, "TTTC", 0, 1), (4, "TTTG", 0, 1),           # one root with 3
            (5, "CACA", 0, 10), (6, "CACC", 0, 1),                             # neighbours in different bins stay apart
            (5, "CACC", 1, 1)]                                                 # ... and so do neighbours with different reads
    return [(b, head + u, r, k) for b, u, r, k in mols]


def exact_case(L, extra=0):
    """error-free reads, every molecule repeated as often as its count says; `extra` more molecules of one read each, barcode 7"""
    if ("exact", L, extra) not in _CASES:
        rng = np.random.default_rng(40 + L)
        reads_of = [rng.integers(0, 4, 50, dtype=np.uint8) for _ in range(2)]
        reads = []
        for b, umi, r, copies in exact_molecules(L):
            reads += [np.concatenate([code(BARCODES[b]), code(umi), reads_of[r]])] * copies
        for q in range(extra):
            reads.append(np.concatenate([code(BARCODES[7]), np.array([q & 3, q >> 2, 2, 1], np.uint8)[:L], reads_of[1]]))
        order = rng.permutation(len(reads))
        seq, offs = pack([reads[i] for i in order])
        _CASES[("exact", L, extra)] = decoded(ARCH[L], seq, offs), reads_of
    return _CASES[("exact", L, extra)]


def noise_case():
    """1200 reads from 240 molecules (a barcode, a UMI of 8, a read), 2 % substitutions in the UMI only"""
    if "noise" not in _CASES:
        rng = np.random.default_rng(7)
        mols = [(code(BARCODES[int(rng.integers(0, len(BARCODES)))]), rng.integers(0, 4, 8, dtype=np.uint8),
                 rng.integers(0, 4, int(rng.integers(30, 101)), dtype=np.uint8)) for _ in range(240)]
        reads = []
        for _ in range(1200):
            bar, umi, read = mols[int(rng.integers(0, 240))]
            umi = umi.copy()
            hit = rng.random(8) < 0.02
            umi[hit] = (umi[hit] + rng.integers(1, 4, int(hit.sum()), dtype=np.uint8)) & 3
            reads.append(np.concatenate([bar, umi, read]))
        _CASES["noise"] = decoded(ARCH[8], *pack(reads))
    return _CASES["noise"]


def yardstick(c, P, lo=0, hi=None):
    """((entries, origins, totals) of td_mol_host_origins, (roots, origins, totals) of td_mol_collapse_host over them), reads lo..hi"""
    from tagdust_amd import lib as tdlib
    md, seq, offs, _, _, res, lab = c
    hi = len(offs) - 1 if hi is None else hi
    raw = tdlib.mol_host_origins(md, seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo], {f: v[lo:hi] for f, v in res.items()},
                                 lab[offs[lo] + lo:offs[hi] + hi], P)
    return raw, tdlib.mol_collapse_host(raw[0], raw[1])


def same(got, want):
    """entries, origins and totals of two results"""
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]


def check_identities(raw, col):
    t = col[2]
    assert t["molecules_after"] + t["absorbed"] == t["molecules_before"] == len(raw[0]) and t["molecules_after"] == len(col[0])
    assert int(col[0]["count"].sum()) == int(raw[0]["count"].sum()) == raw[2]["counted"]


def check_device(ctx, raw, col):
    """origins, collapsed entries and rows of the device against the yardstick; the count's own results stay what they are"""
    from tagdust_amd import lib as tdlib
    same(ctx.mol_origins(), raw)
    same(ctx.mol_collapse_entries(), col)
    rows, tot = ctx.mol_collapse_get()
    assert tot == col[2] and np.array_equal(rows, tdlib.mol_summarise(col[0]))
    plain_rows, plain_tot = ctx.mol_get()
    assert np.array_equal(rows["reads"], plain_rows["reads"]) and plain_tot == raw[2]
    ent, tot = ctx.mol_entries()
    assert np.array_equal(ent, raw[0]) and tot == raw[2] and np.array_equal(plain_rows, tdlib.mol_summarise(raw[0]))
    top = ctx.mol_collapse_entries(cap=3)
    assert np.array_equal(top[0], col[0][:3]) and np.array_equal(top[1], col[1][:3]) and top[2] == col[2]


@pytest.fixture()
def ctx():
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", 0)
    yield c
    c.close()


def begin(ctx, c, P, log2_slots=16):
    start(ctx, c, P, log2_slots)
    ctx.mol_collapse_enable()
    assert ctx.get_option("collapse_active") == 1


# ---- exact counts ----
@pytest.mark.parametrize("L", [4, 8])
def test_exact_counts_the_chain_the_threshold_the_ties_and_the_bins(ctx, L):
    from tagdust_amd import lib as tdlib
    c, reads_of = exact_case(L)
    P = 20
    raw, col = yardstick(c, P)
    # the yardstick's side first: the raw entries have the intended counts ...
    w = [int("".join(str(b) for b in r[:P]), 4) for r in reads_of]
    intended = {tdlib.mol_key(b, fingerprint_of(u), w[r], P): k for b, u, r, k in exact_molecules(L)}
    assert {int(k): int(v) for k, v in raw[0].tolist()} == intended and raw[2]["counted"] == len(c[2]) - 1
    key = lambda b, u, r=0: tdlib.mol_key(b, fingerprint_of(("" if L == 4 else "GTCA") + u), w[r], P)
    roots = {int(k): int(v) for k, v in col[0].tolist()}
    print("exact", L, col[2])
    assert col[2]["longest_chain"] == 2 and col[2]["absorbed"] == 6 > 0 and col[2]["molecules_after"] == 9
    assert roots[key(0, "AAAA")] == 18 and roots[key(1, "ACGT")] == 5 and roots[key(1, "ACGA")] == 8 and roots[key(2, "ACGA")] == 14
    assert roots[min(key(3, "GGGG"), key(3, "GGGT"))] == 2 and roots[min(key(4, "TTT" + x) for x in "ACG")] == 3
    assert roots[key(5, "CACA")] == 10 and roots[key(6, "CACC")] == 1 and roots[key(5, "CACC", 1)] == 1
    check_identities(raw, col)
    begin(ctx, c, P)
    run_batch(ctx, c)
    check_device(ctx, raw, col)
    assert ctx.get_option("collapse_origin_kernel_us") >= 0


# ---- noise, and the table's shapes ----
@pytest.mark.parametrize("log2_slots", [16, 10])
def test_noise_in_the_umi_is_collapsed_as_the_yardstick_does(ctx, log2_slots):
    c = noise_case()
    P = 16
    raw, col = yardstick(c, P)
    print("noise", raw[2], col[2])
    assert raw[2]["eligible"] >= 0.8 * 1200 and col[2]["absorbed"] > 40 and col[2]["molecules_after"] >= 200
    assert col[2]["molecules_after"] % 64 != 0 and col[2]["molecules_before"] % 64 != 0        # a partial last wave in every pass
    check_identities(raw, col)
    begin(ctx, c, P, log2_slots)
    run_batch(ctx, c)
    check_device(ctx, raw, col)
    again = ctx.mol_collapse_get()                                                             # twice in a row
    assert np.array_equal(again[0], ctx.mol_collapse_get()[0]) and again[1] == col[2]


def test_a_table_of_sixteen_slots(ctx):
    """the window is the whole table, probes wrap, some keys overflow -- which ones is the device's to say: an overflowed key is in
    nobody's neighbourhood, so the device equals the yardstick over what the device holds"""
    from tagdust_amd import lib as tdlib
    c, _ = exact_case(4, extra=12)
    P = 20
    raw, _ = yardstick(c, P)
    assert len(raw[0]) == 27
    begin(ctx, c, P, log2_slots=4)
    run_batch(ctx, c)
    run_batch(ctx, c)                                                                          # a key fails on every attempt or on none
    held = ctx.mol_origins()
    print("sixteen slots", held[2])
    assert held[2]["overflow"] > 0 and len(held[0]) == 16
    ref = {int(k): (int(v), o) for (k, v), o in zip(raw[0].tolist(), raw[1].tolist())}
    for (k, v), o in zip(held[0].tolist(), held[1].tolist()):
        assert ref[int(k)] == (v // 2, o) and v % 2 == 0
    col = tdlib.mol_collapse_host(held[0], held[1])
    same(ctx.mol_collapse_entries(), col)
    rows, tot = ctx.mol_collapse_get()
    assert tot == col[2] and np.array_equal(rows, tdlib.mol_summarise(col[0])) and int(rows["reads"].sum()) == held[2]["counted"]
    assert set(int(k) for k in col[0]["key"]) <= set(ref)


def test_a_full_table_of_sixteen_slots_with_overflow(ctx):
    """the noise case into 16 slots: the table is full, every probe of an absent neighbour walks the whole wrapped window"""
    from tagdust_amd import lib as tdlib
    c = noise_case()
    begin(ctx, c, 16, log2_slots=4)
    run_batch(ctx, c)
    held = ctx.mol_origins()
    assert held[2]["overflow"] > 0 and len(held[0]) == 16
    col = tdlib.mol_collapse_host(held[0], held[1])
    same(ctx.mol_collapse_entries(), col)
    assert ctx.mol_collapse_get()[1] == col[2]


def origins_with_cap(ctx, cap):
    """td_mol_origins itself: (n as it reports it, the first min(cap, n) entries, their origins)"""
    import ctypes as C
    from tagdust_amd import lib as tdlib
    n = C.c_int64(-1)
    e, o = np.zeros(max(cap, 1), tdlib.CENSUS_ENTRY_DTYPE), np.zeros(max(cap, 1), tdlib.MOL_ORIGIN_DTYPE)
    ctx._chk(tdlib._mol_lib().td_mol_origins(ctx.h, e.ctypes.data if cap else None, o.ctypes.data if cap else None, cap, C.byref(n), None))
    return n.value, e[:min(cap, n.value)], o[:min(cap, n.value)]


@pytest.mark.parametrize("log2_slots", [10, 4])
def test_origins_with_a_cap_are_the_head_of_all_of_them(ctx, log2_slots):
    """td_mol_origins with room for none, for three and for all: the same n each time, the three are the head of the whole, and the
    whole is td_mol_host_origins over the oracle's labels -- in 16 slots, where the table is full, over the keys the device holds"""
    c, _ = exact_case(4, extra=12 if log2_slots == 4 else 0)
    P = 20
    raw, _ = yardstick(c, P)
    begin(ctx, c, P, log2_slots)
    run_batch(ctx, c)
    n0, e0, o0 = origins_with_cap(ctx, 0)
    n3, e3, o3 = origins_with_cap(ctx, 3)
    n, e, o = origins_with_cap(ctx, n0)
    assert n0 == n3 == n == len(e) and len(e0) == len(o0) == 0 and len(e3) == len(o3) == 3
    assert np.array_equal(e3, e[:3]) and np.array_equal(o3, o[:3])
    if log2_slots == 4:
        assert n == 16 < len(raw[0]) and ctx.mol_origins()[2]["overflow"] > 0
        held = np.isin(raw[0]["key"], e["key"])
        assert held.sum() == 16 and np.array_equal(e, raw[0][held]) and np.array_equal(o, raw[1][held])
    else:
        assert n == len(raw[0]) == 15 and np.array_equal(e, raw[0]) and np.array_equal(o, raw[1])


# ---- paths and state ----
def test_behind_the_specialised_kernel_and_with_length_classes():
    from oracle import pyoracle
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    c = noise_case()
    md, seq, offs, thr, minlen, res, lab = c
    P = 16
    raw, col = yardstick(c, P)
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
    big = (md, bseq, boffs, thr, minlen, {f: np.array(v) for f, v in recs.items()}, np.concatenate(labs).astype(np.int8))
    big_raw, big_col = yardstick(big, P)
    assert big_col[2]["absorbed"] > 0
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 1)
        ctx.set_option("async_compile", 0)
        begin(ctx, c, P)
        before = ctx.get_option("spec_batches_generic")
        run_batch(ctx, c)
        assert ctx.get_option("spec_batches_generic") == before     # the specialised kernel decoded it
        check_device(ctx, raw, col)
        ctx.mol_reset()
        ctx.upload_batch(bseq, boffs)
        assert ctx.get_option("length_classes") > 0
        ctx.run()
        assert ctx.get_option("spec_batches_generic") == before
        check_device(ctx, big_raw, big_col)
    finally:
        ctx.close()


def test_over_td_run_and_tickets_in_mid_run_and_after_a_reset(ctx):
    from tagdust_amd import RESULT_DTYPE, TdError
    c = noise_case()
    _, seq, offs = c[:3]
    n = len(offs) - 1
    P = 16
    begin(ctx, c, P)
    part_raw, part_col = yardstick(c, P, 0, 400)
    whole_raw, whole_col = yardstick(c, P)
    run_batch(ctx, c, 0, 400)
    check_device(ctx, part_raw, part_col)                        # in mid-run ...
    run_batch(ctx, c, 400, n)
    check_device(ctx, whole_raw, whole_col)                      # ... more batches, then again
    # the same reads again through three tickets in flight: every count doubles, no key is new
    parts = [(0, 300), (300, 650), (650, n)]
    res = [np.zeros(hi - lo, RESULT_DTYPE) for lo, hi in parts]
    tickets = [ctx.submit(np.ascontiguousarray(seq[offs[lo]:offs[hi]]), np.ascontiguousarray(offs[lo:hi + 1] - offs[lo]), res=r)
               for (lo, hi), r in zip(parts, res)]
    with pytest.raises(TdError, match="tickets are outstanding"):
        ctx.mol_collapse_enable()
    for t in tickets:
        ctx.wait(t)
    from tagdust_amd import lib as tdlib
    twice = whole_raw[0].copy()
    twice["count"] *= 2
    twice_col = tdlib.mol_collapse_host(twice, whole_raw[1])
    assert twice_col[2]["absorbed"] > 0
    same(ctx.mol_collapse_entries(), twice_col)
    got = ctx.mol_origins()
    assert np.array_equal(got[0], twice) and np.array_equal(got[1], whole_raw[1])
    ctx.mol_reset()
    empty = ctx.mol_collapse_entries()
    assert len(empty[0]) == 0 and not any(empty[2].values()) and not ctx.mol_collapse_get()[0]["reads"].any()
    run_batch(ctx, c, 0, 400)
    check_device(ctx, part_raw, part_col)
    ctx.mol_collapse_disable()
    assert ctx.get_option("collapse_active") == 0 and ctx.get_option("molecules_active") == 1
    for call in (ctx.mol_collapse_get, ctx.mol_collapse_entries, ctx.mol_origins):
        with pytest.raises(TdError, match="collapse is off"):
            call()
    assert np.array_equal(ctx.mol_entries()[0], part_raw[0])     # table and count stay
    ctx.mol_collapse_enable()                                    # ... and enabling starts from an empty table
    assert len(ctx.mol_entries()[0]) == 0
    ctx.mol_disable()
    assert ctx.get_option("collapse_active") == 0


def test_refusals(ctx):
    from tagdust_amd import TdError
    from test_molecules_gpu import case
    c = noise_case()
    ctx.upload_model(c[0])
    with pytest.raises(TdError, match="molecule count is off"):
        ctx.mol_collapse_enable()
    ctx.mol_enable(16, 10)
    ctx.mol_collapse_enable()
    ctx.upload_model(c[0])                                       # a new model switches it off with the count
    assert ctx.get_option("collapse_active") == 0 and ctx.get_option("molecules_active") == 0
    ctx.upload_model(case("b_r")[0])                             # no 'F' segment
    ctx.mol_enable(16, 10)
    with pytest.raises(TdError, match="no 'F' segment"):
        ctx.mol_collapse_enable()


def test_with_dedup_the_marks_are_those_without_the_collapse(ctx):
    c = noise_case()
    P = 16
    raw, col = yardstick(c, P)
    start(ctx, c, P)
    ctx.mol_dedup_enable()
    run_batch(ctx, c)
    alone, _, _ = ctx.download()
    alone_tot = ctx.mol_dedup_get()
    ctx.mol_collapse_enable()                                    # (an empty table again, dedup's first ordinals with it)
    run_batch(ctx, c)
    both, _, _ = ctx.download()
    assert np.array_equal(both["read_type"], alone["read_type"]) and ctx.mol_dedup_get() == alone_tot and alone_tot["duplicates"] > 0
    same(ctx.mol_origins(), raw)
    same(ctx.mol_collapse_entries(), col)


def test_two_contexts_concatenated_equal_one_fed_both(ctx):
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    c = noise_case()
    n = len(c[2]) - 1
    P = 16
    other = TagdustHip(0)
    try:
        other.set_option("specialize", 0)
        begin(ctx, c, P)
        begin(other, c, P)
        run_batch(ctx, c, 0, n // 2)
        run_batch(other, c, n // 2, n)
        a, b = ctx.mol_origins(), other.mol_origins()
        run_batch(ctx, c, n // 2, n)
        one = ctx.mol_collapse_entries()
    finally:
        other.close()
    merged = tdlib.mol_collapse_host(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]))
    same(merged, one)
    same(merged, yardstick(c, P)[1])
    assert len(a[0]) and len(b[0]) and merged[2]["molecules_before"] < len(a[0]) + len(b[0])


# ---- the command ----
def collapse_text(plain, rows, crows, ctot):
    """<out>_molecules.txt with --collapse-umis from the file without it: three lines in front of the column header, two columns"""
    lines = plain.splitlines()
    at = next(i for i, l in enumerate(lines) if l.startswith("# barcode\t"))
    head = lines[:at] + ["# UMI collapse\tfingerprints one mismatch apart, directional rule",
                         "# molecules after collapse\t%d" % ctot["molecules_after"], "# absorbed\t%d" % ctot["absorbed"],
                         lines[at] + "\tcollapsed\tduplication_collapsed"]
    body = []
    for q, l in enumerate(lines[at + 1:]):
        last = q == len(lines) - at - 2
        reads = int(rows["reads"].sum()) if last else int(rows["reads"][q])
        mols = int(crows["molecules"].sum()) if last else int(crows["molecules"][q])
        body.append(l + "\t%d\t%0.4f" % (mols, 1.0 - mols / reads if reads else 0.0))
    return "\n".join(head + body) + "\n"


def test_the_command_with_and_without_the_option(tmp_path):
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    _, seq, offs = noise_case()[:3]
    if "command" not in _CASES:                                  # as the command decodes with -Q 20: threshold 0, the run's model
        _CASES["command"] = decoded(ARCH[8], seq, offs, thr=0.0, minlen=16, threads=8, e=0.05, d=0.1)
    c = _CASES["command"]
    raw, col = yardstick(c, 20)
    assert col[2]["absorbed"] > 40
    d = str(tmp_path)
    fq = os.path.join(d, "in.fq")
    open(fq, "wb").write(fastq_of(seq, offs))
    base = ["-Q", "20"] + [w for k, s in enumerate(ARCH[8]) for w in ("-%d" % (k + 1), s)] + ["in.fq", "--molecules-slots", "14"]
    _run(base + ["--molecules", "-o", "plain"], d)
    _run(base + ["--collapse-umis", "-o", "with"], d)
    # --molecules alone: the file in the format it had before the option existed, from td_mol_get of a context fed the same reads
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 0)
        start(ctx, c, 20, 14)
        run_batch(ctx, c)
        rows, tot = ctx.mol_get()
    finally:
        ctx.close()
    assert tot == raw[2] and np.array_equal(rows, tdlib.mol_summarise(raw[0]))
    plain_want = molecules_text("in.fq", 20, tot, rows, BARCODES)
    assert open(os.path.join(d, "plain_molecules.txt")).read() == plain_want
    crows = tdlib.mol_summarise(col[0])
    want = collapse_text(plain_want, rows, crows, col[2])
    assert open(os.path.join(d, "with_molecules.txt")).read() == want
    assert "\tcollapsed\tduplication_collapsed\n" in want and "# absorbed\t%d\n" % col[2]["absorbed"] in want
    plain, with_opt = _outputs(d, "plain"), _outputs(d, "with")
    assert set(plain) == set(with_opt)
    for name in plain:                                           # every other output is what it is without the option
        if name != "_molecules.txt":
            assert plain[name] == with_opt[name], name
    # one context (the device's collapse) and two contexts on one device (their origins collapsed on the host): the same report
    args = ["--rtest"] + base[:-3] + [fq, "--molecules-slots", "14", "--collapse-umis"]
    os.environ["TD_SPECIALIZE"] = "0"
    try:
        one = tdlib.run_execute(args + ["-o", os.path.join(d, "one")])
        two = tdlib.run_execute(args + ["--devices", "0,0", "-o", os.path.join(d, "two")])
        none = tdlib.run_execute(args[:-1] + ["--molecules", "-o", os.path.join(d, "none")])
    finally:
        del os.environ["TD_SPECIALIZE"]
    for rep in (one, two):
        assert rep["collapse_totals"] == col[2] and np.array_equal(rep["molecules_collapsed"], crows) and np.array_equal(rep["molecules"], rows)
    assert open(os.path.join(d, "one_molecules.txt")).read() == open(os.path.join(d, "two_molecules.txt")).read() == want.replace("in.fq", fq, 1)
    assert none["collapse_totals"] is None and none["molecules_collapsed"] is None and np.array_equal(none["molecules"], rows)
