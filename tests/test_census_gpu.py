"""The census of barcode spellings on the device (include/tagdust_census.h, tagdust_amd/csrc/td_census.hip).  The yardstick is
td_census_host fed with the CPU oracle's labels and outcomes for the same reads (oracle/pyoracle.py), never with the device's own
output.  The table has 2^16 slots unless noted: at least 16 times the reads, so the yardstick's overflow of 0 holds for the device."""
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden, golden_artifacts

pytestmark = pytest.mark.gpu

DEFAULT = (1 << 1) | (1 << 3)
ALPHA = np.frombuffer(b"ACGTN", np.uint8)
BARCODES = ["TTGTGT", "AAACCC", "AAGGGA", "ACTTCA", "CAGTAC", "CCTAGG", "GATCTC", "GGCATA"]
LINKER30 = "GTCAGTTACGGATCCAGTCTTGCAAGCTAG"          # 30 bases: the barcode behind it lies at bases 30..35, across base 32
EXE = os.path.join(REPO, "tagdust_amd", "bin", "tagdust-hip")


def code(s):
    return np.array([b"ACGTN".index(c) for c in s.encode()], np.uint8)


def pairs(entries):
    return [(int(k), int(c)) for k, c in zip(entries["key"], entries["count"])]


def pack(reads):
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    return np.concatenate(reads).astype(np.uint8), offs


def mutate(rng, word):
    """a barcode as a sequencer may leave it: a substitution, a single-base insertion or deletion, or an N"""
    w = list(word)
    r = rng.random()
    p = int(rng.integers(0, len(w)))
    if r < 0.15:
        w[p] = int(rng.integers(0, 4))
    elif r < 0.25:
        w.insert(p, int(rng.integers(0, 4)))
    elif r < 0.35:
        del w[p]
    elif r < 0.45:
        w[p] = 4
    return np.array(w, np.uint8)


SHAPES = {
    "b_r": ["B:" + ",".join(BARCODES), "R:N"],
    "r_s_b_f": ["R:N", "S:GTCA", "B:" + ",".join(BARCODES), "F:NNNN"],
    "b_at_base_30": ["S:" + LINKER30, "B:" + ",".join(BARCODES), "R:N"],
}


def make_reads(shape, n, seed):
    """n reads of 20..150 bases: nine in ten follow the architecture (barcodes listed and not listed, mutated), one in ten is uniformly random"""
    rng = np.random.default_rng(seed)
    words = [code(b) for b in BARCODES] + [code("CGCGAT"), code("TCATGA")]
    reads = []
    for _ in range(n):
        ln = int(rng.integers(20, 151))
        if rng.random() < 0.1:
            reads.append(rng.integers(0, 4, ln, dtype=np.uint8))
            continue
        bar = mutate(rng, words[int(rng.integers(0, len(words)))])
        if shape == "b_r":
            r = np.concatenate([bar, rng.integers(0, 4, max(ln - len(bar), 14), dtype=np.uint8)])
        elif shape == "r_s_b_f":
            r = np.concatenate([rng.integers(0, 4, max(ln - 14, 16), dtype=np.uint8), code("GTCA"), bar, rng.integers(0, 4, 4, dtype=np.uint8)])
        else:
            r = np.concatenate([code(LINKER30), bar, rng.integers(0, 4, max(ln - 36, 16), dtype=np.uint8)])
        reads.append(r.astype(np.uint8))
    return pack(reads)


_CASES = {}


def case(shape, n=1000, seed=5):
    """(model, seq, offs, threshold, the oracle's outcomes and labels), computed once"""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    key = (shape, n, seed)
    if key not in _CASES:
        seq, offs = make_reads(shape, n, seed)
        md, _ = tdlib.build_model(SHAPES[shape], seq, offs)
        thr = 5.0
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, 16, 100, 2)
        _CASES[key] = (md, seq, offs, thr, ores["read_type"].copy(), olab)
    return _CASES[key]


def yardstick(c, mask, segment=-1, lo=0, hi=None):
    """td_census_host over reads lo..hi of a case with the oracle's labels and outcomes"""
    from tagdust_amd import lib as tdlib
    md, seq, offs, _, rt, lab = c
    hi = len(offs) - 1 if hi is None else hi
    return tdlib.census_host(md, seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo], rt[lo:hi], lab[offs[lo] + lo:offs[hi] + hi], segment, mask)


@pytest.fixture()
def ctx():
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", 0)
    yield c
    c.close()


def start(ctx, c, mask, log2_slots=16, segment=-1):
    md, _, _, thr, _, _ = c
    ctx.upload_model(md)
    ctx.set_params(thr, 16, 100)
    ctx.census_enable(segment, mask, log2_slots)


def run_batch(ctx, c, lo=0, hi=None):
    _, seq, offs, _, _, _ = c
    hi = len(offs) - 1 if hi is None else hi
    ctx.upload_batch(seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo])
    ctx.run()


def check_identities(ent, tot):
    assert tot["eligible"] == tot["counted"] + tot["skipped_empty"] + tot["skipped_long"] + tot["skipped_n"] + tot["overflow"]
    assert tot["counted"] == int(ent["count"].sum()) and tot["distinct"] == len(ent)


@pytest.mark.parametrize("shape", sorted(SHAPES))
@pytest.mark.parametrize("mask", [DEFAULT, 1 << 0], ids=["default-mask", "assigned"])
def test_equals_the_yardstick_on_a_ragged_batch(ctx, shape, mask):
    c = case(shape)
    want, want_tot = yardstick(c, mask)
    print(shape, mask, "yardstick totals", want_tot)
    assert want_tot["counted"] > 50 and want_tot["distinct"] > 5 and want_tot["overflow"] == 0
    if mask == DEFAULT or shape != "r_s_b_f":
        assert want_tot["skipped_n"] > 0      # N inside the barcode is met
    start(ctx, c, mask)
    run_batch(ctx, c)
    ent, tot = ctx.census()
    print(shape, mask, "device totals   ", tot)
    assert tot == want_tot
    assert pairs(ent) == pairs(want)
    check_identities(ent, tot)
    res, labels, _ = ctx.download()               # the batch itself is what it is without a census
    assert np.array_equal(res["read_type"], c[4]) and np.array_equal(labels, c[5])
    top, _ = ctx.census(cap=3)
    assert pairs(top) == pairs(want)[:3]


def test_lengths_of_the_words_cover_indels_and_the_word_boundary():
    """(what the cases above are made for, checked on the yardstick alone)"""
    ent, _ = yardstick(case("b_at_base_30"), 0xFF)
    lens = {k >> 56 for k, _ in pairs(ent)}
    assert {5, 6, 7} <= lens


def _c3_case():
    from oracle import pyoracle
    if "c3" not in _CASES:
        g = load_golden("c3_b6_s_r_p")
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(g), g["seq"], g["offs"], float(g["threshold"]), int(g["minlen"]), int(g["dust"]), 2)
        assert np.array_equal(olab, g["labels"])
        _CASES["c3"] = (g, np.asarray(g["seq"], np.uint8), np.asarray(g["offs"], np.int64), float(g["threshold"]), ores["read_type"].copy(), olab)
    return _CASES["c3"]


def test_behind_the_specialised_kernel():
    """config-3 architecture, whose specialised kernel the smoke test and the parity tests compile too (the disk cache serves it)"""
    from tagdust_amd import TagdustHip
    c = _c3_case()
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 1)
        ctx.set_option("async_compile", 0)
        for mask in (DEFAULT, 1 << 0):
            start(ctx, c, mask)
            assert ctx.get_option("spec_state") >= 0 and ctx.get_option("specialize") == 1
            before = ctx.get_option("spec_batches_generic")
            run_batch(ctx, c)
            assert ctx.get_option("spec_batches_generic") == before     # the specialised kernel decoded it
            ent, tot = ctx.census()
            want, want_tot = yardstick(c, mask)
            assert tot == want_tot and pairs(ent) == pairs(want) and tot["counted"] > 0
    finally:
        ctx.close()


def test_behind_the_specialised_kernel_with_length_classes():
    """4096 reads (64 tiles): the config-3 fixture's reads over and over, and six 1000-base reads among them -- the long tiles get
    wave slots of their own geometry, the labels keep the stride of the batch's longest read"""
    from oracle import pyoracle
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    g, seq, offs, thr, rt, lab = _c3_case()
    n0 = len(offs) - 1
    rng = np.random.default_rng(9)
    longs = []
    for _ in range(6):
        r = rng.integers(0, 4, 1000, dtype=np.uint8)
        r[:6] = code("CGCGAT")
        longs.append(r)
    lseq, loffs = pack(longs)
    lres, llab, _ = pyoracle.label_batch(pyoracle.OracleModel(g), lseq, loffs, thr, int(g["minlen"]), int(g["dust"]), 2)
    reps = (4096 - 6) // n0
    short_n = 4096 - 6
    idx = np.arange(short_n) % n0
    reads = [seq[offs[i]:offs[i + 1]] for i in idx]
    labs = [lab[offs[i] + i:offs[i + 1] + i + 1] for i in idx]
    types = [rt[i] for i in idx]
    at = [100, 900, 1700, 2500, 3300, 4000]
    for k, p in enumerate(at):
        reads.insert(p, longs[k]); labs.insert(p, llab[loffs[k] + k:loffs[k + 1] + k + 1]); types.insert(p, lres["read_type"][k])
    assert len(reads) == 4096 and reps >= 1
    bseq, boffs = pack(reads)
    blab = np.concatenate(labs).astype(np.int8)
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 1)
        ctx.set_option("async_compile", 0)
        ctx.upload_model(g)
        ctx.set_params(thr, int(g["minlen"]), int(g["dust"]))
        ctx.census_enable(-1, 0xFF, 16)
        ctx.upload_batch(bseq, boffs)
        assert ctx.get_option("length_classes") > 0
        ctx.run()
        ent, tot = ctx.census()
    finally:
        ctx.close()
    want, want_tot = tdlib.census_host(g, bseq, boffs, np.array(types), blab, -1, 0xFF)
    assert tot == want_tot and pairs(ent) == pairs(want) and tot["eligible"] == 4096


def test_heavy_hitter_counts_are_exact(ctx):
    """4096 reads that spell one barcode the architecture does not list and 64 that each spell another one, in two batches of 2080
    with the rare ones spread among the others: one key takes 64 lanes of most waves"""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    md, _, _, thr, _, _ = case("b_r")
    rng = np.random.default_rng(21)
    body = rng.integers(0, 4, 44, dtype=np.uint8)
    others = set()
    while len(others) < 64:
        w = "".join("ACGT"[b] for b in rng.integers(0, 4, 6))
        if w not in BARCODES and w != "CGCGAT":
            others.add(w)
    kinds = [np.concatenate([code("CGCGAT"), body])] + [np.concatenate([code(w), body]) for w in sorted(others)]
    kseq, koffs = pack(kinds)
    kres, klab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), kseq, koffs, thr, 16, 100, 2)
    which = np.zeros(4160, np.int64)
    which[np.arange(64) * 65 + 7] = np.arange(1, 65)
    reads = [kinds[k] for k in which]
    labs = np.concatenate([klab[koffs[k] + k:koffs[k + 1] + k + 1] for k in which]).astype(np.int8)
    bseq, boffs = pack(reads)
    want, want_tot = tdlib.census_host(md, bseq, boffs, kres["read_type"][which], labs, -1, 0xFF)
    assert pairs(want)[0] == (tdlib.census_key("CGCGAT"), 4096) and len(want) == 65 and all(c == 1 for _, c in pairs(want)[1:])
    ctx.upload_model(md)
    ctx.set_params(thr, 16, 100)
    ctx.census_enable(-1, 0xFF, 16)
    for lo, hi in ((0, 2080), (2080, 4160)):
        ctx.upload_batch(bseq[boffs[lo]:boffs[hi]], boffs[lo:hi + 1] - boffs[lo])
        ctx.run()
    ent, tot = ctx.census()
    assert pairs(ent) == pairs(want) and tot == want_tot


def test_accumulates_over_td_run_and_td_submit_and_resets(ctx):
    from tagdust_amd import RESULT_DTYPE
    c = case("b_r")
    _, seq, offs, _, _, _ = c
    n = len(offs) - 1
    mask = 0xFF
    start(ctx, c, mask)
    whole, whole_tot = yardstick(c, mask)
    a, a_tot = yardstick(c, mask, lo=0, hi=400)
    run_batch(ctx, c, 0, 400)
    ent, tot = ctx.census()
    assert pairs(ent) == pairs(a) and tot == a_tot
    ctx.counts_reset()                                  # the outcome counters are another matter
    assert ctx.census()[1] == a_tot
    run_batch(ctx, c, 400, n)
    ent, tot = ctx.census()
    assert pairs(ent) == pairs(whole) and tot == whole_tot
    # three tickets in flight on top of it
    parts = [(0, 300), (300, 650), (650, n)]
    res = [np.zeros(hi - lo, RESULT_DTYPE) for lo, hi in parts]
    tickets = [ctx.submit(np.ascontiguousarray(seq[offs[lo]:offs[hi]]), np.ascontiguousarray(offs[lo:hi + 1] - offs[lo]), res=r)
               for (lo, hi), r in zip(parts, res)]
    for t in tickets:
        ctx.wait(t)
    ent, tot = ctx.census()
    assert pairs(ent) == [(k, 2 * v) for k, v in pairs(whole)]
    assert tot == {f: (v if f == "distinct" else 2 * v) for f, v in whole_tot.items()}
    assert np.array_equal(np.concatenate([r["read_type"] for r in res]), c[4])
    ctx.census_reset()
    ent, tot = ctx.census()
    assert len(ent) == 0 and not any(tot.values())
    run_batch(ctx, c, 0, 400)
    ent, tot = ctx.census()
    assert pairs(ent) == pairs(a) and tot == a_tot


def test_overflow_keeps_every_reported_count_exact(ctx):
    c = case("b_r")
    mask = 0xFF
    want, want_tot = yardstick(c, mask)
    assert want_tot["distinct"] >= 64
    start(ctx, c, mask, log2_slots=4)
    run_batch(ctx, c)
    run_batch(ctx, c)                                   # a key fails on every attempt or on none
    ent, tot = ctx.census()
    print("overflow totals", tot)
    assert tot["overflow"] > 0 and 0 < tot["distinct"] <= 16
    check_identities(ent, tot)
    ref = dict(pairs(want))
    assert all(k in ref and v == 2 * ref[k] for k, v in pairs(ent))
    assert tot["eligible"] == 2 * want_tot["eligible"] and tot["skipped_n"] == 2 * want_tot["skipped_n"]


def test_other_modes_and_arch_scores_add_nothing(ctx):
    from tagdust_amd import lib as tdlib
    c = case("b_r")
    md, seq, offs, _, _, _ = c
    start(ctx, c, 0xFF)
    hi = 200
    sub_seq, sub_offs = seq[:offs[hi]], offs[:hi + 1]
    for mode in (tdlib.MODE_GET_PROB, tdlib.MODE_ARCH_COMP, tdlib.MODE_RNA_DUST):
        ctx.upload_batch(sub_seq, sub_offs)
        ctx.run(mode)
        ctx.sync()
    ctx.arch_scores([md, case("r_s_b_f")[0]], sub_seq, sub_offs)
    ent, tot = ctx.census()
    assert len(ent) == 0 and not any(tot.values())
    run_batch(ctx, c, 0, hi)                            # ... and the census is still alive
    assert ctx.census()[1] == yardstick(c, 0xFF, lo=0, hi=hi)[1]


def test_a_context_without_a_census_behaves_as_before(ctx):
    from tagdust_amd import TdError
    c = case("b_r")
    md, _, _, thr, rt, lab = c
    ctx.upload_model(md)
    ctx.set_params(thr, 16, 100)
    assert ctx.get_option("census_active") == 0
    run_batch(ctx, c)
    res, labels, _ = ctx.download()
    assert np.array_equal(res["read_type"], rt) and np.array_equal(labels, lab)
    for call in (ctx.census, ctx.census_reset):
        with pytest.raises(TdError, match="census is off"):
            call()
    ctx.census_disable()                                # (nothing to do)
    ctx.set_window(2, 40)                               # no census: a window is fine
    ctx.set_window(-1, -1)


def test_refusals_and_the_model_upload_that_switches_it_off(ctx):
    from tagdust_amd import TdError
    with pytest.raises(TdError, match="no model uploaded"):
        ctx.census_enable()
    g = load_golden("umi_f_s_r")
    ctx.upload_model(g)
    with pytest.raises(TdError, match="no 'B' segment"):
        ctx.census_enable()
    c = case("r_s_b_f")
    ctx.upload_model(c[0])
    with pytest.raises(TdError, match="not a 'B' segment"):
        ctx.census_enable(segment=0)
    for bad in (3, 27):
        with pytest.raises(TdError, match="log2_slots"):
            ctx.census_enable(log2_slots=bad)
    for bad in (0, 0x100):
        with pytest.raises(TdError, match="outcome_mask"):
            ctx.census_enable(mask=bad)
    ctx.set_window(2, 40)
    with pytest.raises(TdError, match="window"):
        ctx.census_enable(log2_slots=8)
    ctx.set_window(-1, -1)
    ctx.census_enable(segment=2, log2_slots=8)
    assert ctx.get_option("census_active") == 1
    with pytest.raises(TdError, match="census is on"):
        ctx.set_window(2, 40)
    ctx.upload_model(c[0])
    assert ctx.get_option("census_active") == 0
    ctx.census_enable(log2_slots=8)
    ctx.census_disable()
    assert ctx.get_option("census_active") == 0


@pytest.mark.parametrize("name", ["artifacts_b_r", "dust_b_r"])
def test_follows_the_final_outcomes_of_filter_and_dust(ctx, name):
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    g = load_golden(name)
    art = golden_artifacts(g)
    mask = DEFAULT | (1 << 5) | (1 << 6)
    if art:
        ctx.set_artifacts(art[0], art[1], art[2], art[3])
    ctx.upload_model(g)
    ctx.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
    ctx.census_enable(-1, mask, 16)
    ctx.upload_batch(g["seq"], g["offs"])
    ctx.run()
    ent, tot = ctx.census()
    ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(g), g["seq"], g["offs"], float(g["threshold"]), int(g["minlen"]), int(g["dust"]),
                                         art[3] if art else 2, artifacts=(art[0], art[1], art[2]) if art else None)
    assert np.array_equal(ores["read_type"], g["read_type"])
    want, want_tot = tdlib.census_host(g, g["seq"], g["offs"], ores["read_type"], olab, -1, mask)
    low = np.asarray(g["read_type"]) & 0xFF
    assert want_tot["eligible"] == int(np.isin(low, [1, 3, 5, 6]).sum()) and int(np.isin(low, [5, 6]).sum()) > 0
    assert tot == want_tot and pairs(ent) == pairs(want)


def test_two_contexts_on_one_device_merge_to_the_whole(ctx):
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    c = case("b_at_base_30")
    n = len(c[2]) - 1
    other = TagdustHip(0)
    try:
        other.set_option("specialize", 0)
        start(ctx, c, DEFAULT)
        start(other, c, DEFAULT)
        run_batch(ctx, c, 0, n // 2)
        run_batch(other, c, n // 2, n)
        a, ta = ctx.census()
        b, tb = other.census()
    finally:
        other.close()
    want, want_tot = yardstick(c, DEFAULT)
    assert pairs(tdlib.census_merge(a, b)) == pairs(want) and len(a) and len(b)
    assert all(ta[f] + tb[f] == want_tot[f] for f in tdlib.CENSUS_TOTALS if f != "distinct")


# ---- the command ----
def levenshtein(a, b):
    row = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        prev, row[0] = row[0], i
        for j in range(1, len(b) + 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (a[i - 1] != b[j - 1]))
    return row[len(b)]


def command_case(seed=42, n=3000):
    """td_simreads with eight barcodes and no errors, decoded with the first seven: (FASTQ text, segments, the yardstick's rows)"""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    if ("command", seed, n) in _CASES:
        return _CASES[("command", seed, n)]
    text = tdlib.simreads(BARCODES, seed=seed, rng=1, barnum=8, readlen=40, numseq=n, random_frac=0.1, error_rate=0.0)
    pr = tdlib.ParsedReads(text, 0)
    seq, offs = pr.codes.copy(), pr.offs.copy()
    pr.close()
    listed = BARCODES[:7]
    segs = ["B:" + ",".join(listed), "R:N"]
    md, _ = tdlib.build_model(segs, seq, offs, e=0.05, d=0.1)        # as the run builds it when -Q is given (threshold 0)
    ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, 0.0, 16, 100, 8)
    ent, tot = tdlib.census_host(md, seq, offs, ores["read_type"], olab, -1, DEFAULT)
    rows = []
    for k, cnt in pairs(ent)[:10]:
        w = tdlib.census_key_text(k)
        d = [levenshtein(w, b) for b in listed]
        rows.append("%d\t%s\t%s\t%d" % (cnt, w, listed[int(np.argmin(d))], min(d)))
    _CASES[("command", seed, n)] = (text, segs, rows, tot, pairs(ent))
    return _CASES[("command", seed, n)]


def test_the_command_writes_the_top_unknown_barcodes(tmp_path):
    text, segs, rows, tot, _ = command_case()
    omitted = BARCODES[7]
    d0 = [levenshtein(omitted, b) for b in BARCODES[:7]]
    assert rows[0].split("\t")[1:] == [omitted, BARCODES[int(np.argmin(d0))], str(min(d0))] and int(rows[0].split("\t")[0]) > 100
    d = str(tmp_path)
    open(os.path.join(d, "in.fq"), "wb").write(text)
    env = dict(os.environ, TD_SPECIALIZE="0")
    base = [EXE, "--rtest", "-Q", "10", "-1", segs[0], "-2", segs[1], "in.fq"]

    def run(extra, prefix, rc=0):
        p = subprocess.run(base + extra + ["-o", prefix], cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
        assert p.returncode == rc, p.stderr.decode(errors="replace")[-3000:]
        return p.stderr.decode(errors="replace")

    run([], "plain")
    run(["--unknown-barcodes", "10"], "with")
    lines = open(os.path.join(d, "with_unknown_barcodes.txt")).read().splitlines()
    head = [l for l in lines if l.startswith("#")]
    assert [l for l in lines if not l.startswith("#")] == rows
    assert "# eligible reads\t%d" % tot["eligible"] in head and "# counted\t%d" % tot["counted"] in head
    assert not any("too small" in l for l in head) and head[-1] == "# count\tsequence\tnearest\tdistance"

    def outputs(prefix):
        out = {}
        for p in sorted(glob.glob(os.path.join(d, prefix + "*"))):
            name = os.path.basename(p)[len(prefix):]
            data = open(p, "rb").read()
            if name == "_logfile.txt":    # the messages without their time stamps; the cmd: line repeats the command line as given
                msgs = [l.split(b"]\t", 1)[1] if l.startswith(b"[") and b"]\t" in l else l for l in data.splitlines()]
                data = b"\n".join(m for m in msgs if not m.startswith(b"cmd: "))
            out[name] = data
        return out

    plain, with_opt = outputs("plain"), outputs("with")
    assert "_unknown_barcodes.txt" not in plain and set(with_opt) == set(plain) | {"_unknown_barcodes.txt"}
    for name in plain:
        assert plain[name] == with_opt[name], name
    kept = open(os.path.join(d, "with_unknown_barcodes.txt")).read()
    err = run(["--unknown-barcodes", "10"], "with", rc=1)        # a second run without --force
    assert "already exists" in err and open(os.path.join(d, "with_unknown_barcodes.txt")).read() == kept
    for p in glob.glob(os.path.join(d, "with*")):
        if not p.endswith("_unknown_barcodes.txt"):
            os.remove(p)
    err = run(["--unknown-barcodes", "10"], "with", rc=1)        # ... also when that file is the only one left: it is named
    assert "with_unknown_barcodes.txt" in err


def test_the_run_reports_the_merged_census_of_two_devices(tmp_path):
    """td_run_execute with two contexts on one device: the report holds every spelling, merged, and the totals"""
    from tagdust_amd import lib as tdlib
    text, segs, rows, tot, want = command_case()
    d = str(tmp_path)
    open(os.path.join(d, "in.fq"), "wb").write(text)
    os.environ["TD_SPECIALIZE"] = "0"
    try:
        rep = tdlib.run_execute(["--rtest", "--devices", "0,0", "-Q", "10", "-1", segs[0], "-2", segs[1], os.path.join(d, "in.fq"),
                                 "-o", os.path.join(d, "two"), "--unknown-barcodes", "3", "--unknown-barcodes-slots", "12"])
    finally:
        del os.environ["TD_SPECIALIZE"]
    assert pairs(rep["unknown"]) == want and rep["unknown_totals"] == tot
    lines = [l for l in open(os.path.join(d, "two_unknown_barcodes.txt")).read().splitlines() if not l.startswith("#")]
    assert lines == rows[:3]
