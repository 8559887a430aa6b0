"""The join of barcode calls across input files on the device (include/tagdust_samples.h, tagdust_amd/csrc/td_samples.hip): an
exporter context's words and a primary context's assignment.  The yardsticks are td_samples_export_host and td_samples_join_host
fed with the CPU oracle's labels and outcomes for the same reads (oracle/pyoracle.py), never with the device's own output; the
primary is fed the yardstick's words, so a wrong export cannot hide a wrong join."""
import numpy as np
import pytest

from test_samples_gpu import B1, B2, B3, case, code, model, pairs

pytestmark = pytest.mark.gpu

SUCCESS, DEMOTED = 0, 3
FAILED = 0xFFFFFFFF
LO = 300                                                # (a stretch of the cases' batches with every class in it)
N_HMM = {"one": [5], "two": [5, 4], "three": [5, 4, 5]}
_UNIFORM = {}


def uniform_case(kind, thr, n=300, seed=11):
    """as test_samples_gpu.case, with reads of ONE length (the slot is not sorted: device order is the caller's)"""
    from oracle import pyoracle
    from tagdust_amd import RESULT_DTYPE
    if (kind, thr) not in _UNIFORM:
        md, _, _ = model(kind)
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
            rest = rng.integers(0, 4, 40, dtype=np.uint8)
            parts = {"one": [b1, rest], "two": [b1, code("GT"), b2, rest],
                     "three": [b1, code("GT"), b2, code("GT"), code(B3[int(rng.integers(0, 4))]), rest]}[kind]
            read = np.concatenate(parts)
            if 0.35 <= r < 0.45:
                read = rng.integers(0, 4, len(read), dtype=np.uint8)
            reads.append(read)
        assert len({len(r) for r in reads}) == 1
        offs = np.zeros(n + 1, np.int64)
        offs[1:] = np.cumsum([len(r) for r in reads])
        seq = np.concatenate(reads).astype(np.uint8)
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, 16, 100, 2)
        res = np.zeros(len(ores), RESULT_DTYPE)
        for f in RESULT_DTYPE.names:
            res[f] = ores["Q" if f == "mapq" else f]
        _UNIFORM[(kind, thr)] = (md, seq, offs, thr, res, olab)
    return _UNIFORM[(kind, thr)]


THR_PRIMARY, THR_EXPORTER = 0.0, 0.5                    # (at 0.0 reads with a missing or decoy call are extracted; at 0.5 some reads are not)


def data(kind, uniform, thr):
    """(the case, the first read of the stretch the tests use: the exporter's reads are others than the primary's, whose barcodes
    test_samples_gpu.make_reads draws from the same stream for every kind)"""
    lo = {THR_PRIMARY: 0, THR_EXPORTER: 40} if uniform else {THR_PRIMARY: LO, THR_EXPORTER: 100}
    return (uniform_case(kind, thr) if uniform else case(kind, thr)), lo[thr]


def cut(c, lo, hi):
    """reads lo..hi of a case as a batch of their own: (seq, offs, oracle records, oracle labels)"""
    _, seq, offs, _, res, lab = c
    return (np.ascontiguousarray(seq[offs[lo]:offs[hi]]), np.ascontiguousarray(offs[lo:hi + 1] - offs[lo]), res[lo:hi],
            lab[offs[lo] + lo:offs[hi] + hi])


def layout(primary, exporter, primary_first):
    """(first column of the primary, of the exporter, column_hmms, a sheet over all columns that lists about half of the tuples)"""
    mp, me = len(N_HMM[primary]), len(N_HMM[exporter])
    first_p, first_e = (0, mp) if primary_first else (me, 0)
    hm = N_HMM[primary] + N_HMM[exporter] if primary_first else N_HMM[exporter] + N_HMM[primary]
    grid = np.stack(np.meshgrid(*[np.arange(h - 1) for h in hm], indexing="ij"), -1).reshape(-1, len(hm))
    sheet = [tuple(int(b) for b in row) for row in grid if int(row.sum()) % 2 == 0]
    return first_p, first_e, hm, sheet


def new_ctx(c, specialize):
    from tagdust_amd import TagdustHip
    ctx = TagdustHip(0)
    ctx.set_option("specialize", specialize)
    ctx.set_option("async_compile", 0)
    ctx.upload_model(c[0])
    ctx.set_params(c[3], 16, 100)
    return ctx


def export_by_run(ctx, batch, sorted_expected):
    seq, offs, _, _ = batch
    n = len(offs) - 1
    words = np.full(n, 0xDEADBEEF, np.uint32)
    ctx.samples_export_next(words, n)
    ctx.upload_batch(seq, offs)
    ctx.run()
    assert ctx.get_option("batch_sorted") == int(sorted_expected)
    return words


def join_by_run(ctx, batch, words, sorted_expected):
    seq, offs, _, _ = batch
    n = len(offs) - 1
    w = np.array(words, np.uint32)
    ctx.samples_join_next(w, n)
    ctx.upload_batch(seq, offs)
    w[:] = 0x01010101                                   # (the words were taken when the batch was staged)
    ctx.run()
    assert ctx.get_option("batch_sorted") == int(sorted_expected)
    return ctx.download()[0]


def yard(primary_c, exporter_c, lo_p, lo_e, n, names):
    """the yardsticks over n reads of both cases: (the exporter's words, rewritten records, entries, totals)"""
    from tagdust_amd import lib as tdlib
    primary, exporter, primary_first = names
    first_p, first_e, hm, sheet = layout(primary, exporter, primary_first)
    _, eo, er, el = cut(exporter_c, lo_e, lo_e + n)
    words = tdlib.samples_export_host(exporter_c[0], first_e, eo, er, el)
    _, po, pr, pl = cut(primary_c, lo_p, lo_p + n)
    want, ent, tot = tdlib.samples_join_host(primary_c[0], sheet, first_p, hm, words, po, pr, pl)
    return words, want, ent, tot


SHAPES = [("two", "one", True), ("one", "three", False), ("two", "two", False), ("one", "two", True), ("three", "one", True)]


@pytest.mark.parametrize("names", SHAPES, ids=lambda s: "%s+%s%s" % (s[0], s[1], "" if s[2] else "-exporter-first"))
def test_the_yardsticks_meet_what_the_cases_are_made_for(names):
    """(asserted on the yardsticks alone, before the device is asked)"""
    for uniform in (False, True):
        (pc, lo_p), (ec, lo_e) = data(names[0], uniform, THR_PRIMARY), data(names[1], uniform, THR_EXPORTER)
        words, want, ent, tot = yard(pc, ec, lo_p, lo_e, 257, names)
        print(names, uniform, tot)
        assert min(tot["assigned"], tot["unlisted"], tot["incomplete"], tot["partner_failed"]) >= 3
        assert tot["eligible"] == tot["assigned"] + tot["unlisted"] + tot["incomplete"]
        assert int((pc[4]["read_type"][lo_p:lo_p + 257] == SUCCESS).sum()) == tot["eligible"] + tot["partner_failed"]
        lengths = np.diff(pc[2][lo_p:lo_p + 258])
        assert (len(set(lengths)) == 1) == uniform


CASES = [(n, u, 0) for n in (1, 63, 64, 65, 257) for u in (True, False)] + [(n, u, 1) for n in (65, 257) for u in (True, False)]


@pytest.mark.parametrize("n,uniform,specialize", CASES,
                         ids=["%d-%s-%s" % (n, "uniform" if u else "mixed", "specialised" if s else "generic") for n, u, s in CASES])
@pytest.mark.parametrize("names", SHAPES[:3], ids=lambda s: "%s+%s%s" % (s[0], s[1], "" if s[2] else "-exporter-first"))
def test_export_and_join_equal_the_yardsticks(names, n, uniform, specialize):
    primary, exporter, primary_first = names
    first_p, first_e, hm, sheet = layout(*names)
    (pc, lo_p), (ec, lo_e) = data(primary, uniform, THR_PRIMARY), data(exporter, uniform, THR_EXPORTER)
    words, want, want_ent, want_tot = yard(pc, ec, lo_p, lo_e, n, names)
    p_batch, e_batch = cut(pc, lo_p, lo_p + n), cut(ec, lo_e, lo_e + n)
    # a batch of one length is not sorted; one read never is; reads of several lengths are
    sorted_p, sorted_e = (len(set(np.diff(b[1]))) > 1 for b in (p_batch, e_batch))
    assert uniform == (not sorted_p) or n == 1
    ex = new_ctx(ec, specialize)
    try:
        ex.samples_export_enable(first_e)
        assert ex.get_option("samples_export") == 1 and ex.get_option("samples_join") == 0
        before = ex.get_option("spec_batches_generic")
        got_words = export_by_run(ex, e_batch, sorted_e)
        assert (ex.get_option("spec_batches_generic") == before) == bool(specialize)
        assert ex.get_option("samples_export_kernel_us") >= 0
        e_res = ex.download()[0]
    finally:
        ex.close()
    assert np.array_equal(e_res["read_type"], e_batch[2]["read_type"])       # the export changes nothing of its batch
    assert np.array_equal(got_words, words)
    pr = new_ctx(pc, specialize)
    try:
        pr.samples_join_enable(sheet, hm, first_p)
        assert pr.get_option("samples_join") == len(sheet) and pr.get_option("samples_export") == 0
        got = join_by_run(pr, p_batch, words, sorted_p)
        ent, tot = pr.samples_join()
        assert pr.get_option("samples_join_kernel_us") >= 0
        assert pr.samples()[1] == {k: v for k, v in tot.items() if k != "partner_failed"}
    finally:
        pr.close()
    print(names, n, uniform, specialize, tot)
    assert got.tobytes() == want.tobytes()
    assert tot == want_tot and pairs(ent) == pairs(want_ent)


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform", "mixed"])
def test_two_tickets_in_flight(uniform):
    from tagdust_amd import RESULT_DTYPE
    names = ("two", "one", False)
    first_p, first_e, hm, sheet = layout(*names)
    (pc, lo_p), (ec, lo_e) = data("two", uniform, THR_PRIMARY), data("one", uniform, THR_EXPORTER)
    words, want, want_ent, want_tot = yard(pc, ec, lo_p, lo_e, 257, names)
    parts = [(0, 130), (130, 257)]
    ex = new_ctx(ec, 0)
    try:
        ex.samples_export_enable(first_e)
        ins = [cut(ec, lo_e + a, lo_e + b) for a, b in parts]
        outs = [np.full(b - a, 0xDEADBEEF, np.uint32) for a, b in parts]
        e_res = [np.zeros(b - a, RESULT_DTYPE) for a, b in parts]
        tickets = []
        for (seq, offs, _, _), w, r in zip(ins, outs, e_res):
            ex.samples_export_next(w, len(w))
            tickets.append(ex.submit(seq, offs, res=r))
        for t in tickets:
            ex.wait(t)
    finally:
        ex.close()
    assert np.array_equal(np.concatenate(outs), words)
    assert np.array_equal(np.concatenate(e_res)["read_type"], ec[4]["read_type"][lo_e:lo_e + 257])
    pr = new_ctx(pc, 0)
    try:
        pr.samples_join_enable(sheet, hm, first_p)
        ins = [cut(pc, lo_p + a, lo_p + b) for a, b in parts]
        res = [np.zeros(b - a, RESULT_DTYPE) for a, b in parts]
        tickets = []
        for (seq, offs, _, _), r, (a, b) in zip(ins, res, parts):
            w = np.array(words[a:b], np.uint32)
            pr.samples_join_next(w, b - a)
            tickets.append(pr.submit(seq, offs, res=r))
            w[:] = 0                                    # (taken when the batch was staged)
        for t in tickets:
            pr.wait(t)
        ent, tot = pr.samples_join()
    finally:
        pr.close()
    assert np.concatenate(res).tobytes() == want.tobytes()
    assert tot == want_tot and pairs(ent) == pairs(want_ent)


def test_failures_leave_the_context_usable():
    from tagdust_amd import TdError
    from tagdust_amd import RESULT_DTYPE
    names = ("two", "one", True)
    first_p, first_e, hm, sheet = layout(*names)
    (pc, lo_p), (ec, lo_e) = data("two", False, THR_PRIMARY), data("one", False, THR_EXPORTER)
    n = 65
    words, want, want_ent, want_tot = yard(pc, ec, lo_p, lo_e, n, names)
    p_batch, e_batch = cut(pc, lo_p, lo_p + n), cut(ec, lo_e, lo_e + n)
    ex = new_ctx(ec, 0)
    try:
        with pytest.raises(TdError, match=r"td_samples_export_next: the export is off"):
            ex.samples_export_next(np.zeros(n, np.uint32), n)
        ex.samples_enable([[0], [1]])
        with pytest.raises(TdError, match=r"td_samples_export_enable: sample assignment is on in this context \(td_samples_disable first\)"):
            ex.samples_export_enable(first_e)
        ex.samples_disable()
        with pytest.raises(TdError, match=r"first_column = 4 \(0..3\)"):
            ex.samples_export_enable(4)
        ex.samples_export_enable(first_e)
        with pytest.raises(TdError, match=r"td_samples_enable: the context exports its barcode calls"):
            ex.samples_enable([[0], [1]])
        with pytest.raises(TdError, match=r"td_samples_join_enable: the context exports its barcode calls"):
            ex.samples_join_enable(sheet, hm, first_p)
        with pytest.raises(TdError, match=r"td_set_window: the context exports its barcode calls"):
            ex.set_window(2, 20)
        # no array named: td_run refuses the batch, td_submit refuses it before anything is staged
        ex.upload_batch(e_batch[0], e_batch[1])
        with pytest.raises(TdError, match=r"td_run: the context exports its barcode calls .* staged without an array named for as many words"):
            ex.run()
        with pytest.raises(TdError, match=r"td_submit: the context exports its barcode calls and no words are named for this batch of 65 reads"):
            ex.submit(e_batch[0], e_batch[1])
        # an array named for another number of reads
        w = np.zeros(n + 1, np.uint32)
        ex.samples_export_next(w, n + 1)
        with pytest.raises(TdError, match=r"td_submit: the named words are those of 66 reads, the batch has 65"):
            ex.submit(e_batch[0], e_batch[1])
        ex.samples_export_next(w, n + 1)
        ex.upload_batch(e_batch[0], e_batch[1])
        with pytest.raises(TdError, match=r"td_run: the context exports"):
            ex.run()
        with pytest.raises(TdError, match=r"td_samples_export_next: no array of words for a batch of 65 reads"):
            ex.samples_export_next(None, n)
        assert np.array_equal(export_by_run(ex, e_batch, True), words)      # a good batch behind all of them
        ex.samples_export_disable()
        assert ex.get_option("samples_export") == 0
        ex.upload_batch(e_batch[0], e_batch[1])
        ex.run()                                        # ... and without the export the context decodes as ever
        assert np.array_equal(ex.download()[0]["read_type"], e_batch[2]["read_type"])
    finally:
        ex.close()
    pr = new_ctx(pc, 0)
    try:
        with pytest.raises(TdError, match=r"td_samples_join_next: the join is off"):
            pr.samples_join_next(words, n)
        with pytest.raises(TdError, match=r"column_hmms\[0\] = 7, 'B' segment 0 of the model"):
            pr.samples_join_enable(sheet, [7] + hm[1:], first_p)
        pr.samples_join_enable(sheet, hm, first_p)
        with pytest.raises(TdError, match=r"td_samples_export_enable: the join is on in this context"):
            pr.samples_export_enable(0)
        pr.upload_batch(p_batch[0], p_batch[1])
        with pytest.raises(TdError, match=r"td_run: the context joins its partners' barcode calls .* td_samples_join_next first"):
            pr.run()
        r = np.zeros(n, RESULT_DTYPE)
        with pytest.raises(TdError, match=r"td_submit: the context joins its partners' barcode calls and no words are named"):
            pr.submit(p_batch[0], p_batch[1], res=r)
        pr.samples_join_next(words[:-1], n - 1)
        with pytest.raises(TdError, match=r"td_submit: the named words are those of 64 reads, the batch has 65"):
            pr.submit(p_batch[0], p_batch[1], res=r)
        ent, tot = pr.samples_join()
        assert len(ent) == 0 and not any(tot.values())  # nothing of the refused batches was counted
        got = join_by_run(pr, p_batch, words, True)
        ent, tot = pr.samples_join()
        assert got.tobytes() == want.tobytes() and tot == want_tot and pairs(ent) == pairs(want_ent)
        # a batch staged under the join is refused once the join is off, and a new model switches the join off
        pr.samples_join_next(words, n)
        pr.upload_batch(p_batch[0], p_batch[1])
        pr.samples_disable()
        with pytest.raises(TdError, match=r"td_run: sample assignment is off .* staged while it was on"):
            pr.run()
        pr.samples_join_enable(sheet, hm, first_p)
        pr.upload_model(pc[0])
        assert pr.get_option("samples_join") == 0 and pr.get_option("samples") == 0
    finally:
        pr.close()


# ---- td_stream_run_multi: the barcodes of one sample in two (three) index files ----
I_BARS = [["ACAGTG", "CTTGTA", "GGCTAC", "TTAGGC"], ["AAGGTC", "CCTTGA", "GTGTAC", "TGCACG"], ["ATATCG", "CGCGAT", "GACTTA", "TCAGCC"]]
I_SECOND = ["AACC", "GGTT", "CATG", "TCGA"]            # index file 1 has a second barcode behind a spacer: two columns of its own
I_ARCH = [["B:" + ",".join(I_BARS[0])], ["B:" + ",".join(I_BARS[1]), "S:GT", "B:" + ",".join(I_SECOND)], ["B:" + ",".join(I_BARS[2])]]
I_COLUMNS = [1, 2, 1]
I_THR = [0.5, 0.0, 0.5]                                # (at 0.0 file 1's reads with a decoy first barcode are extracted by their second)
N_STREAM = 600


def index_reads(t, seed):
    """600 index reads of file t: a barcode of its list (file 1: + GT + a second barcode); one in twelve has two bases (it is not
    extracted), one in twenty is all N, and in file 1 one in eight has a first barcode that is none of the list: the decode calls
    the decoy there and still extracts the read by its last barcode, which is what gives the join incomplete reads"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(N_STREAM):
        r = rng.random()
        read = code(I_BARS[t][int(rng.integers(0, 4))])
        if t == 1:
            if r > 0.875:
                read = code("TTTTTT")
            read = np.concatenate([read, code("GT"), code(I_SECOND[int(rng.integers(0, 4))])])
        if r < 1 / 12:
            read = read[:2]
        elif r < 1 / 12 + 0.05:
            read = np.full(len(read), 4, np.uint8)
        reads.append(read)
    offs = np.zeros(N_STREAM + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), offs


_STREAM = {}


def stream_inputs():
    """three index files' reads with their models, two read files' reads; built once"""
    from tagdust_amd import lib as tdlib
    if not _STREAM:
        idx = []
        for t in range(3):
            seq, offs = index_reads(t, 60 + t)
            md, _ = tdlib.build_model(I_ARCH[t], seq, offs)
            idx.append((md, seq, offs))
        rng = np.random.default_rng(70)
        reads = [(rng.integers(0, 4, N_STREAM * 50, dtype=np.uint8), np.arange(N_STREAM + 1, dtype=np.int64) * 50) for _ in range(2)]
        _STREAM.update(idx=idx, reads=reads)
    return _STREAM["idx"], _STREAM["reads"]


def stream_ctx(t, thr=None):
    from tagdust_amd import TagdustHip
    ctx = TagdustHip(0)
    ctx.set_option("specialize", 0)
    ctx.upload_model(stream_inputs()[0][t][0])
    ctx.set_params(I_THR[t] if thr is None else thr, 16, 100)
    return ctx


def stream_sheet(order):
    """(sample names, the sheet in the call order's columns, column_hmms, the first column of every file of `order`): a row is
    written by index FILE 0, 1, 2 whatever the call order, so the same barcodes name the same samples in every order"""
    files = sorted(order)
    m = sum(I_COLUMNS[t] for t in files)
    at = {t: sum(I_COLUMNS[u] for u in files if u < t) for t in files}
    grid = np.stack(np.meshgrid(*[np.arange(4)] * m, indexing="ij"), -1).reshape(-1, m)
    by_file = [tuple(int(b) for b in row) for row in grid if int(row.sum()) % 2 == 0]
    names = ["s" + "".join(str(b) for b in row) for row in by_file]
    sheet = [tuple(row[at[t] + u] for t in order for u in range(I_COLUMNS[t])) for row in by_file]
    first = list(np.cumsum([0] + [I_COLUMNS[t] for t in order])[:-1])
    return names, sheet, [5] * m, [int(f) for f in first]


def stream_expectation(order, ctxs):
    """per-file td_run decodes on `ctxs` plus td_samples_export_host / td_samples_join_host: (rewritten records of the primary,
    entries, totals, every record's final outcome)"""
    from tagdust_amd import lib as tdlib
    idx, _ = stream_inputs()
    names, sheet, hm, first = stream_sheet(order)
    decoded = []
    for ctx, t in zip(ctxs, order):
        ctx.upload_batch(idx[t][1], idx[t][2])
        ctx.run()
        res, lab, _ = ctx.download()
        decoded.append((res, lab))
    word = np.zeros(N_STREAM, np.uint32)
    for q in range(1, len(order)):
        t = order[q]
        word |= tdlib.samples_export_host(idx[t][0], first[q], idx[t][2], decoded[q][0], decoded[q][1])
    p = order[0]
    want, ent, tot = tdlib.samples_join_host(idx[p][0], sheet, 0, hm, word, idx[p][2], decoded[0][0], decoded[0][1])
    final = want["read_type"].copy()
    for q in range(1, len(order)):
        final = np.maximum(final, decoded[q][0]["read_type"])
    return want, ent, tot, final


def expected_files(names, want, final):
    expect = {name: [] for name in names + ["un"]}
    for i in range(N_STREAM):
        ok = int(final[i]) == SUCCESS
        expect[names[int(want["barcode"][i]) & 0xFF] if ok else "un"].append("r%d" % i)
    return expect


def write_stream_files(d, order, n_read_files):
    import os
    from test_samples_gpu import fastq
    idx, reads = stream_inputs()
    for t in order:
        p = os.path.join(d, "I%d.fq" % t)
        if not os.path.exists(p):
            open(p, "w").write(fastq(idx[t][1], idx[t][2]))
    for k in range(n_read_files):
        p = os.path.join(d, "R%d.fq" % k)
        if not os.path.exists(p):
            open(p, "w").write(fastq(*reads[k]))


def check_output_files(d, prefix, names, expect, n_read_files):
    import glob
    import os
    from test_samples_gpu import records_by_name
    suffixes = [""] if n_read_files == 1 else ["_READ%d" % (k + 1) for k in range(n_read_files)]
    want_files = sorted(["%s_BC_%s%s.fq" % (prefix, s, x) for s in names for x in suffixes] + ["%s_un%s.fq" % (prefix, x) for x in suffixes])
    assert sorted(os.path.basename(f) for f in glob.glob(os.path.join(d, prefix + "_*.fq"))) == want_files
    for x in suffixes:
        for s in names + ["un"]:
            f = os.path.join(d, "%s_%s%s.fq" % (prefix, "un" if s == "un" else "BC_" + s, x))
            assert list(records_by_name([f])) == expect[s], f


def run_join_stream(d, prefix, order, n_read_files, thr=None):
    """Index files `order` (the first is the primary) and n_read_files read files through td_stream_run_multi with the join;
    the expectation from per-file td_run decodes and td_samples_join_host.  Returns {sample name or "un": [record names]}."""
    import os
    from tagdust_amd import lib as tdlib
    idx, reads = stream_inputs()
    names, sheet, hm, first = stream_sheet(order)
    write_stream_files(d, order, n_read_files)
    ctxs = [stream_ctx(t, thr) for t in order]
    try:
        want, ent, tot, final = stream_expectation(order, ctxs)
        print(prefix, order, tot)
        # (file 1, with its two barcodes, is the one whose reads can be extracted with a decoy call: single-barcode index files
        # give no incomplete read, the decode does not extract a read whose only barcode is the decoy)
        assert min(tot["assigned"], tot["unlisted"], tot["partner_failed"]) >= 10 and (tot["incomplete"] >= 10 or 1 not in order)
        ctxs[0].samples_join_enable(sheet, hm, 0, names)
        for q in range(1, len(order)):
            ctxs[q].samples_export_enable(first[q])
        files = [(os.path.join(d, "I%d.fq" % t), I_ARCH[t], [ctx]) for t, ctx in zip(order, ctxs)]
        files += [(os.path.join(d, "R%d.fq" % k), ["R:N"], None) for k in range(n_read_files)]
        st, cnt = tdlib.stream_run_multi(files, os.path.join(d, prefix), n_devices=1, dust=100, batch_reads=128, n_threads=2)
        dev_ent, dev_tot = ctxs[0].samples_join()
    finally:
        for ctx in ctxs:
            ctx.close()
    assert st["n_reads"] == N_STREAM and st["n_batches"] == 5
    assert dev_tot == tot and pairs(dev_ent) == pairs(ent)
    expect = expected_files(names, want, final)
    assert int(cnt[0]) == tot["assigned"] == sum(len(v) for k, v in expect.items() if k != "un")
    assert [int(c) for c in cnt[8:8 + len(names)]] == [len(expect[s]) for s in names] and int(cnt[:8].sum()) == N_STREAM
    check_output_files(d, prefix, names, expect, n_read_files)
    assert len(expect["un"]) > 0 and sum(1 for s in names if expect[s]) >= len(names) // 2
    return expect


def test_stream_two_index_files_in_both_call_orders_and_a_second_read_file(tmp_path):
    d = str(tmp_path)
    a = run_join_stream(d, "ab", [0, 1], 1)
    b = run_join_stream(d, "ba", [1, 0], 1)              # primary and exporter swapped, and the sheet's columns with them
    assert a == b
    c = run_join_stream(d, "four", [0, 1], 2)           # a fourth file: READ1 and READ2 per sample
    assert a == c


def test_stream_three_index_files_or_their_words(tmp_path):
    run_join_stream(str(tmp_path), "three", [0, 1, 2], 1)


def test_stream_refusals(tmp_path):
    """without both sides of the join the old refusal stands, word for word; mate mode and the quality filter are named"""
    import os
    from test_samples_gpu import fastq
    from tagdust_amd import TdError
    from tagdust_amd import lib as tdlib
    d = str(tmp_path)
    idx, reads = stream_inputs()
    for t in (0, 1):
        open(os.path.join(d, "I%d.fq" % t), "w").write(fastq(idx[t][1], idx[t][2]))
    open(os.path.join(d, "R0.fq"), "w").write(fastq(*reads[0]))
    old = r"td_stream_run_multi: barcodes seem to be in both architectures \(barcode_hmm.c:140-145\)"
    ctxs = [stream_ctx(t) for t in (0, 1)]
    files = [(os.path.join(d, "I%d.fq" % t), I_ARCH[t], [ctxs[t]]) for t in (0, 1)] + [(os.path.join(d, "R0.fq"), ["R:N"], None)]
    sheet = [(0, 0, 0), (1, 1, 1)]
    try:
        def run():
            return tdlib.stream_run_multi(files, os.path.join(d, "x"), n_devices=1, dust=100, batch_reads=128, n_threads=2)
        with pytest.raises(TdError, match=old):
            run()                                       # neither side
        ctxs[0].samples_join_enable(sheet, [5, 5, 5], 0)
        with pytest.raises(TdError, match=old):
            run()                                       # a primary without its exporter
        ctxs[0].samples_disable()
        ctxs[1].samples_export_enable(1)
        with pytest.raises(TdError, match=old):
            run()                                       # an exporter without a primary
        ctxs[0].samples_export_enable(0)
        with pytest.raises(TdError, match=old):
            run()                                       # two exporters
        ctxs[0].samples_export_disable()
        ctxs[0].samples_join_enable(sheet, [5, 5, 5], 0)
        ctxs[1].qual_enable(20)
        with pytest.raises(TdError, match=r"barcode calls are joined across input files \(td_samples_join_enable\) and the base-quality filter is on"):
            run()
        ctxs[1].qual_disable()
        ctxs[1].mol_enable(4, 16)                       # mate mode in a barcode file's context
        ctxs[1].mol_mate_enable(8)
        with pytest.raises(TdError, match=r"barcode calls are joined across input files \(td_samples_join_enable\) and mate mode is on in the contexts of .*I1.fq: "
                                          r"the join and mate mode do not go together yet"):
            run()
        ctxs[1].mol_mate_disable()
        ctxs[1].mol_disable()
        st, _ = run()                                   # ... and with both sides it runs
        assert st["n_reads"] == N_STREAM
    finally:
        for c in ctxs:
            c.close()


def test_the_command_joins_two_index_files(tmp_path):
    """tagdust-hip -arch ... I0 I2 R0 --samples sheet --join-barcodes: the files, <out>_samples.txt and the log's extracted count
    are those of the library run over the same files.  (Index files 0 and 2: lists of equal length without a shared spelling, so
    that -arch chooses each file's own candidate.  For file 1, with its two barcodes around a spacer, -arch prefers R:N, so the
    incomplete class is the streaming tests' above, not this one's.)"""
    import os
    import subprocess
    from conftest import REPO
    from test_samples_gpu import records_by_name, summary_block
    d = str(tmp_path)
    order = [0, 2]
    # (-Q makes the run decode every file with threshold 0, as test_samples_gpu's command test notes: so does the library run here)
    lib_expect = run_join_stream(d, "lib", order, 1, thr=0.0)
    idx, _ = stream_inputs()
    names, sheet, hm, first = stream_sheet(order)
    ctxs = [stream_ctx(t, 0.0) for t in order]
    try:
        want, ent, tot, final = stream_expectation(order, ctxs)
    finally:
        for c in ctxs:
            c.close()
    # the candidates: two lists of 6-nt barcodes without a shared spelling, and a read
    arch_text = [" ".join("-%d %s" % (k + 1, seg) for k, seg in enumerate(a)) for a in (I_ARCH[order[0]], I_ARCH[order[1]], ["R:N"])]
    open(os.path.join(d, "arch.txt"), "w").write("".join("tagdust %s\n" % a for a in arch_text))
    spell = [I_BARS[order[0]], I_BARS[order[1]]]
    m = len(spell)
    open(os.path.join(d, "sheet.txt"), "w").write("# name i7 i5\n" + "".join(
        "%s\t%s\n" % (n, "\t".join(spell[t][b] for t, b in enumerate(row))) for n, row in zip(names, sheet)))
    exe = os.path.join(REPO, "tagdust_amd", "bin", "tagdust-hip")
    args = [exe, "--rtest", "-Q", "0.5", "--batch-reads", "128", "-arch", "arch.txt", "I0.fq", "I2.fq", "R0.fq", "-o", "cmd", "--samples", "sheet.txt", "--join-barcodes"]
    p = subprocess.run(args, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=dict(os.environ, TD_SPECIALIZE="0"))
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-3000:]
    log = open(os.path.join(d, "cmd_logfile.txt")).read()
    using = [l.split("Using: ", 1)[1].strip() for l in log.splitlines() if "Using: " in l]
    assert using == arch_text                            # the chosen architectures, before anything else
    check_output_files(d, "cmd", names, lib_expect, 1)
    for s in names + ["un"]:
        f = "%s.fq" % ("un" if s == "un" else "BC_" + s)
        assert list(records_by_name([os.path.join(d, "cmd_" + f)])) == list(records_by_name([os.path.join(d, "lib_" + f)]))
    assert int(summary_block(os.path.join(d, "cmd_logfile.txt"))["successfully extracted"]) == tot["assigned"]
    lines = open(os.path.join(d, "cmd_samples.txt")).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    for text, f in (("extracted reads", "eligible"), ("assigned", "assigned"), ("not in the sheet", "unlisted"), ("incomplete", "incomplete"),
                    ("not counted", "overflow"), ("partner failed", "partner_failed")):
        assert "# %s\t%d" % (text, tot[f]) in head, text
    assert "# segments\t1 of I0.fq (%s)\t1 of I2.fq (%s)" % (I_ARCH[0][0], I_ARCH[2][0]) in head
    counts = dict(pairs(ent))
    at = lines.index("# combinations not in the sheet")
    rows = [l.split("\t") for l in lines[:at] if not l.startswith("#")]
    assert [(r[0], tuple(r[1:1 + m]), int(r[1 + m])) for r in rows] == [
        (n, tuple(spell[t][b] for t, b in enumerate(row)), counts.get((m << 56) | sum((b + 1) << (8 * t) for t, b in enumerate(row)), 0))
        for n, row in zip(names, sheet)]
    assert sum(int(l.split("\t")[m]) for l in lines[at + 1:]) == tot["unlisted"] + tot["incomplete"]
