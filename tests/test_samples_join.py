"""The join of barcode calls across input files (include/tagdust_samples.h) on the host, no GPU: td_samples_export_host and
td_samples_join_host over labels written by hand and over the reference's own labels (tests/golden), against the definition
restated here in plain Python; the tie to td_samples_host, which existing tests pin; the OR of several exporters' words."""
import os

import numpy as np
import pytest

from conftest import load_golden
from tagdust_amd import TdError
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib
from test_samples import BSBR_SHEET, DEMOTED, SUCCESS, as_pairs, b_segments, hand, hmms, records, samples_py

FAILED = 0xFFFFFFFF


@pytest.fixture(scope="module", autouse=True)
def library():
    tdbuild.build()
    return tdlib.load_library()


def own_calls_py(md, offs, labels, i):
    """read i's calls for the model's own 'B' segments, -1 = no position (samples_py's rule: the last position wins)"""
    segs = b_segments(md)
    o, ln = int(offs[i]), int(offs[i + 1] - offs[i])
    lab = labels[o + i:o + i + ln + 1]
    calls = [-1] * len(segs)
    for p in range(ln):
        v = int(md["label"][int(lab[p + 1])])
        if (v & 0xFFFF) in segs:
            calls[segs.index(v & 0xFFFF)] = (v >> 16) & 0x7FFF
    return calls


def export_py(md, first_column, offs, res, labels):
    """The definition of an exporter's words."""
    words = np.zeros(len(offs) - 1, np.uint32)
    for i in range(len(words)):
        if int(res["read_type"][i]) != SUCCESS:
            words[i] = FAILED
        else:
            words[i] = sum((c + 1) << (8 * (first_column + u)) for u, c in enumerate(own_calls_py(md, offs, labels, i)))
    return words


def join_py(md, sheet, first_column, column_hmms, words, offs, res, labels):
    """The definition of the join: (rewritten records, entries by count descending then key ascending, totals)."""
    segs = b_segments(md)
    m = len(column_hmms)
    rows = {tuple(int(b) for b in np.atleast_1d(r)): s for s, r in enumerate(sheet)}
    out = res.copy()
    tot = dict.fromkeys(tdlib.SAMPLES_TOTALS + ("partner_failed",), 0)
    counts = {}
    for i in range(len(offs) - 1):
        if int(res["read_type"][i]) != SUCCESS:
            continue
        if int(words[i]) == FAILED:
            tot["partner_failed"] += 1
            continue
        tot["eligible"] += 1
        word = int(words[i]) | sum((c + 1) << (8 * (first_column + u)) for u, c in enumerate(own_calls_py(md, offs, labels, i)))
        key = (m << 56) | word
        counts[key] = counts.get(key, 0) + 1
        calls = [((word >> (8 * t)) & 0xFF) - 1 for t in range(m)]
        if any(c == -1 or c == int(column_hmms[t]) - 1 for t, c in enumerate(calls)):
            tot["incomplete"] += 1
            out["read_type"][i] = DEMOTED
        elif tuple(calls) in rows:
            tot["assigned"] += 1
            out["barcode"][i] = (segs[-1] << 16) | rows[tuple(calls)]
        else:
            tot["unlisted"] += 1
            out["read_type"][i] = DEMOTED
    return out, sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])), tot


def random_batch(md, n, rng, p_missing=0.08, p_decoy=0.08, p_failed=0.1):
    """n reads with labels written by hand: a 'B' segment has no position / the decoy now and then, some reads were not extracted"""
    segs = b_segments(md)
    paths = []
    for _ in range(n):
        p = []
        for j in range(int(md["S"])):
            if j in segs and rng.random() < p_missing:
                continue
            hs = hmms(md, j)
            if j in segs:
                hs = hs[-1:] if rng.random() < p_decoy else hs[:-1]
            p += [hs[int(rng.integers(0, len(hs)))]] * int(rng.integers(1, 5))
        paths.append(p)
    offs, res, labels = hand(md, paths)
    res["read_type"] = np.where(rng.random(n) < p_failed, rng.choice([1, 2, 3, 5, 1 << 8], n), SUCCESS)
    return offs, res, labels


def column_hmms_of(models):
    return [int(md["n_hmm"][j]) for md in models for j in b_segments(md)]


def a_sheet(column_hmms, rng, fraction=0.5):
    """about `fraction` of all complete tuples, at most 255, in random order"""
    grid = np.stack(np.meshgrid(*[np.arange(h - 1) for h in column_hmms], indexing="ij"), -1).reshape(-1, len(column_hmms))
    pick = rng.permutation(len(grid))[:max(1, min(255, int(len(grid) * fraction)))]
    return [tuple(int(b) for b in grid[k]) for k in pick]


@pytest.fixture(scope="module")
def three_segments():
    """B / S / B / S / B / R with two barcodes each, built by the library's own model builder"""
    rng = np.random.default_rng(13)
    bars = [["ACGT", "TGCA"], ["AAGG", "CCTT"], ["GATC", "CTAG"]]
    reads = []
    for _ in range(40):
        parts = []
        for t in range(3):
            parts += [bars[t][int(rng.integers(0, 2))], "GT"]
        reads.append(np.array([b"ACGT".index(c) for c in "".join(parts[:-1]).encode()] + list(rng.integers(0, 4, 30)), np.uint8))
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    segs = ["B:" + ",".join(bars[0]), "S:GT", "B:" + ",".join(bars[1]), "S:GT", "B:" + ",".join(bars[2]), "R:N"]
    md, _ = tdlib.build_model(segs, np.concatenate(reads), offs)
    assert len(b_segments(md)) == 3
    return md


def check_join(models, primary, seed, n=400):
    """models in column order, models[primary] holds the sheet; every class must occur.  Returns the library's totals."""
    rng = np.random.default_rng(seed)
    first = np.concatenate([[0], np.cumsum([len(b_segments(md)) for md in models])])
    hm = column_hmms_of(models)
    sheet = a_sheet(hm, rng)
    batches = [random_batch(md, n, rng) for md in models]
    word = np.zeros(n, np.uint32)
    for k, md in enumerate(models):
        if k == primary:
            continue
        offs, res, labels = batches[k]
        w = tdlib.samples_export_host(md, int(first[k]), offs, res, labels)
        assert w.dtype == np.uint32 and np.array_equal(w, export_py(md, int(first[k]), offs, res, labels))
        own = sum(0xFF << (8 * t) for t in range(int(first[k]), int(first[k + 1])))
        assert all(int(x) == FAILED or int(x) & ~own == 0 for x in w)        # all other bytes are 0
        word |= w                                                            # all-ones absorbs
    md = models[primary]
    offs, res, labels = batches[primary]
    got, ent, tot = tdlib.samples_join_host(md, sheet, int(first[primary]), hm, word, offs, res, labels)
    want, want_ent, want_tot = join_py(md, sheet, int(first[primary]), hm, word, offs, res, labels)
    assert got.tobytes() == want.tobytes()
    assert as_pairs(ent) == want_ent and tot == want_tot
    assert tot["eligible"] == tot["assigned"] + tot["unlisted"] + tot["incomplete"] and tot["overflow"] == 0
    assert int((res["read_type"] == SUCCESS).sum()) == tot["eligible"] + tot["partner_failed"]
    assert int(ent["count"].sum()) == tot["eligible"] and all(k >> 56 == len(hm) for k, _ in as_pairs(ent))
    # every class is there: assigned, unlisted, incomplete by a missing call and by the decoy, partner_failed
    assert min(tot["assigned"], tot["unlisted"], tot["partner_failed"]) >= 5
    keys = [k for k, _ in as_pairs(ent)]
    missing = [k for k in keys if any((k >> (8 * t)) & 0xFF == 0 for t in range(len(hm)))]
    decoy = [k for k in keys if all((k >> (8 * t)) & 0xFF != 0 for t in range(len(hm))) and any((k >> (8 * t)) & 0xFF == hm[t] for t in range(len(hm)))]
    assert missing and decoy
    # a failed partner leaves the read alone
    pf = (res["read_type"] == SUCCESS) & (word == FAILED)
    assert got[pf].tobytes() == res[pf].tobytes()
    assert set(got["barcode"][(got["read_type"] == SUCCESS) & ~pf & (res["read_type"] == SUCCESS)] >> 16) == {b_segments(md)[-1]}
    return tot


def test_two_columns_partner_behind_and_in_front():
    a, b = load_golden("casava_index"), load_golden("c3_b6_s_r_p")
    check_join([a, b], 0, 21)            # first_column == 0: the partner's column behind the own one
    check_join([a, b], 1, 22)            # first_column == 1: ... in front of it
    check_join([b, a], 0, 23)


def test_three_columns():
    g, c = load_golden("b_s_b_r"), load_golden("casava_index")
    check_join([g, c], 0, 31)            # 2 + 1, the primary first
    check_join([g, c], 1, 32)            # the primary last: its own column is 2
    check_join([c, g], 1, 33)            # 1 + 2, own columns 1..2
    check_join([c, g, ], 0, 34)


def test_four_columns_one_plus_three_and_two_plus_two(three_segments):
    g, c = load_golden("b_s_b_r"), load_golden("c3_b6_s_r_p")
    check_join([c, three_segments], 0, 41)
    check_join([c, three_segments], 1, 42)
    check_join([three_segments, c], 0, 43)
    check_join([g, g], 0, 44)
    check_join([g, g], 1, 45)


def test_the_or_of_two_exporters_and_an_all_ones_word():
    """three files of one, two and one columns: the words of two exporters OR-ed, one of them all ones for some reads"""
    c, g, d = load_golden("casava_index"), load_golden("b_s_b_r"), load_golden("c3_b6_s_r_p")
    for primary, seed in ((0, 51), (1, 52), (2, 53)):
        tot = check_join([c, g, d], primary, seed)
        assert tot["partner_failed"] >= 10
    # all ones absorbs whatever the other exporter says, and a word of 0 contributes nothing
    rng = np.random.default_rng(54)
    offs, res, labels = random_batch(c, 50, rng, p_failed=0.0)
    hm = column_hmms_of([c, d])
    sheet = a_sheet(hm, rng)
    w1 = np.full(50, FAILED, np.uint32)
    w2 = np.full(50, 3 << 8, np.uint32)
    got, ent, tot = tdlib.samples_join_host(c, sheet, 0, hm, w1 | w2, offs, res, labels)
    assert got.tobytes() == res.tobytes() and len(ent) == 0 and tot["partner_failed"] == 50 and tot["eligible"] == 0
    got, ent, tot = tdlib.samples_join_host(c, sheet, 0, hm, np.zeros(50, np.uint32), offs, res, labels)
    assert tot["partner_failed"] == 0 and tot["incomplete"] == tot["eligible"] == 50      # column 1 has no call
    assert got.tobytes() == join_py(c, sheet, 0, hm, np.zeros(50, np.uint32), offs, res, labels)[0].tobytes()


def test_without_a_partner_column_the_join_is_the_pinned_definition():
    g = load_golden("b_s_b_r")
    res = records(g)
    offs, labels = np.asarray(g["offs"], np.int64), g["labels"]
    hm = column_hmms_of([g])
    want, want_ent, want_tot = tdlib.samples_host(g, BSBR_SHEET, offs, res, labels)
    got, ent, tot = tdlib.samples_join_host(g, BSBR_SHEET, 0, hm, np.zeros(len(res), np.uint32), offs, res, labels)
    assert got.tobytes() == want.tobytes() and ent.tobytes() == want_ent.tobytes()
    assert tot == dict(want_tot, partner_failed=0)
    assert (tot["eligible"], tot["assigned"], tot["unlisted"], tot["incomplete"]) == (185, 109, 76, 0)
    assert got.tobytes() == samples_py(g, BSBR_SHEET, offs, res, labels)[0].tobytes()
    # the export words of the model over its eligible reads are the low words of those entries
    words = tdlib.samples_export_host(g, 0, offs, res, labels)
    elig = res["read_type"] == SUCCESS
    assert np.all(words[~elig] == FAILED) and np.all(words[elig] != FAILED)
    hist = {}
    for w in words[elig]:
        hist[int(w)] = hist.get(int(w), 0) + 1
    assert hist == {k & 0xFFFFFFFF: n for k, n in as_pairs(want_ent)}


def test_every_failure_has_its_message(three_segments):
    g, c = load_golden("b_s_b_r"), load_golden("casava_index")
    offs, res, labels = hand(g, [[0]])
    w = np.zeros(1, np.uint32)

    def join(md, sheet, first, hm):
        return tdlib.samples_join_host(md, sheet, first, hm, w, offs, res, labels)

    with pytest.raises(TdError, match=r"td_samples_join_host: m_total = 1 \(2..4 columns supported\)"):
        join(c, [(0,)], 0, [13])
    with pytest.raises(TdError, match=r"m_total = 5 \(2..4 columns supported\)"):
        join(g, [(0,) * 5], 0, [5, 4, 13, 13, 13])
    with pytest.raises(TdError, match=r"the model's 2 'B' segments from column 2 on do not fit into 3 columns"):
        join(g, [(0, 0, 0)], 2, [13, 5, 4])
    with pytest.raises(TdError, match=r"column_hmms\[1\] = 7, 'B' segment 0 of the model \(that column\) has 5 HMMs"):
        join(g, [(0, 0, 0)], 1, [13, 7, 4])
    with pytest.raises(TdError, match=r"column_hmms\[0\] = 1 \(a barcode and the decoy at least, 127 at most\)"):
        join(g, [(0, 0, 0)], 1, [1, 5, 4])
    with pytest.raises(TdError, match=r"row 1 of the sheet: barcode 12 of column 0 \(another file's\) is out of range \(0..11; the last HMM is the all-N decoy\)"):
        join(g, [(0, 0, 0), (12, 0, 0)], 1, [13, 5, 4])
    with pytest.raises(TdError, match=r"row 0 of the sheet: barcode 4 of 'B' segment 0 \(column 1\) is out of range \(0..3;"):
        join(g, [(0, 4, 0)], 1, [13, 5, 4])
    with pytest.raises(TdError, match="row 2 of the sheet repeats row 0"):
        join(g, [(1, 0, 0), (0, 0, 0), (1, 0, 0)], 1, [13, 5, 4])
    u = load_golden("umi_f_s_r")
    with pytest.raises(TdError, match="td_samples_export_host: the model has no 'B' segment"):
        tdlib.samples_export_host(u, 0, u["offs"], records(u), u["labels"])
    with pytest.raises(TdError, match=r"td_samples_export_host: the model's 3 'B' segments from column 2 on do not fit into 4 columns"):
        tdlib.samples_export_host(three_segments, 2, offs, res, labels)
    with pytest.raises(TdError, match=r"td_samples_export_host: first_column = 4 \(0..3\)"):
        tdlib.samples_export_host(c, 4, offs, res, labels)


# ---- the command: --samples FILE --join-barcodes ----
I1, I2, I3 = ["ACAGTG", "CTTGTA", "GGCTAC"], ["AAGGTC", "CCTTGA"], ["ATATCG", "CGCGAT"]


@pytest.fixture()
def run_dir(tmp_path):
    d = str(tmp_path)
    for name in ("I1.fq", "I2.fq", "R1.fq"):
        open(os.path.join(d, name), "w").write("@r\nACGTAC\n+\nIIIIII\n")
    open(os.path.join(d, "sheet.txt"), "w").write("# name i7 i5\ns1 ACAGTG AAGGTC\ns2\tCTTGTA\tCCTTGA\n")
    open(os.path.join(d, "arch.txt"), "w").write("tagdust -1 B:%s -2 R:N\n" % ",".join(I2))
    return d


def plan_args(d, *extra, files=("I1.fq", "I2.fq")):
    return ["-1", "B:" + ",".join(I1), "-arch", os.path.join(d, "arch.txt"), "-o", os.path.join(d, "out")] + list(extra) + [os.path.join(d, f) for f in files]


ARCHS = ["-1 B:" + ",".join(I1), "-1 B:" + ",".join(I2), "-1 R:N"]


def test_the_plan_of_a_two_barcode_file_run(run_dir):
    d = run_dir
    sheet = os.path.join(d, "sheet.txt")
    plan = tdlib.run_plan(plan_args(d, "--samples", sheet, "--join-barcodes")).splitlines()
    assert "join: files 0,1; columns 1 = segment 1 of file 0, 2 = segment 1 of file 1; file 0 holds the sheet, a read whose partner in another " \
           "barcode file is not extracted goes to _un" in plan
    assert "samples: %s: 2 samples by segments 1, 1 of the joined files; a read whose barcodes are incomplete or name no sample goes to _un" % sheet in plan
    assert "barcode file: 0" in plan and "output reads: 1" in plan
    out = os.path.join(d, "out")
    assert [l for l in plan if l.startswith("output file: ")] == ["output file: " + out + s for s in ("_BC_s1.fq", "_BC_s2.fq", "_un.fq", "_samples.txt")]
    # without the option the old refusal stands, word for word -- the plan's and td_run_output_files_describe's
    old = ("Barcodes seem to be in both architectures... (--samples: barcodes spread over several input files are not joined; the controller's rule of "
           "one barcode file stays, and a sheet lists the barcode segments of that one file.)")
    with pytest.raises(TdError) as e:
        tdlib.run_plan(plan_args(d, "--samples", sheet))
    assert str(e.value) == old
    with pytest.raises(TdError) as e:
        tdlib.run_output_files(["--samples", sheet, "-o", out], ARCHS)
    assert str(e.value) == old
    with pytest.raises(TdError) as e:
        tdlib.run_output_files(["-o", out], ARCHS)
    assert str(e.value) == "Barcodes seem to be in both architectures... "
    # three barcode files and two read files: READ1 / READ2 per sample, three columns
    open(os.path.join(d, "sheet3.txt"), "w").write("a ACAGTG AAGGTC ATATCG\nb ACAGTG AAGGTC CGCGAT\n")
    got = tdlib.run_output_files(["--samples", os.path.join(d, "sheet3.txt"), "--join-barcodes", "-o", out], ARCHS[:2] + ["-1 B:" + ",".join(I3), "-1 R:N", "-1 R:N"])
    assert sorted(got) == sorted(out + s for s in ("_BC_a_READ1.fq", "_BC_a_READ2.fq", "_BC_b_READ1.fq", "_BC_b_READ2.fq", "_un_READ1.fq", "_un_READ2.fq",
                                                   "_samples.txt"))


def test_every_refusal_of_the_option_has_its_message(run_dir):
    d = run_dir
    sheet, out = os.path.join(d, "sheet.txt"), os.path.join(d, "out")

    def refused(args, text, archs=None):
        with pytest.raises(TdError) as e:
            tdlib.run_plan(args) if archs is None else tdlib.run_output_files(args, archs)
        assert text in str(e.value), str(e.value)

    refused(plan_args(d, "--join-barcodes"), "--join-barcodes needs --samples: the sheet names the barcodes of every file that are joined.")
    refused(plan_args(d, "--samples", sheet, "--join-barcodes", "--devices", "0,1"), "--join-barcodes needs exactly one device (2 given)")
    refused(plan_args(d, "--samples", sheet, "--join-barcodes", "--unknown-barcodes", "10"), "--join-barcodes cannot be combined with --unknown-barcodes")
    refused(plan_args(d, "--samples", sheet, "--join-barcodes", "-start", "2"), "--join-barcodes cannot be combined with -start / -end")
    refused(plan_args(d, "--samples", sheet, "--join-barcodes", "-end", "20"), "--join-barcodes cannot be combined with -start / -end")
    five = ["-1 B:AC,GT -2 S:A -3 B:AC,GT -4 S:A -5 B:AC,GT", "-1 B:AC,GT -2 S:A -3 B:AC,GT", "-1 R:N"]
    refused(["--samples", sheet, "--join-barcodes", "-o", out], "--join-barcodes: the barcode files have 5 barcode segments together (at most 4).", five)
    refused(["--samples", sheet, "--join-barcodes", "-o", out], "--join-barcodes: only one input file (-) has barcode segments: there is nothing to join, "
            "drop the option", [ARCHS[0], "-1 R:N"])
    refused(["-1", "B:" + ",".join(I1), "--samples", sheet, "--join-barcodes", "-o", out, os.path.join(d, "I1.fq"), os.path.join(d, "R1.fq")],
            "--join-barcodes: only one input file (%s) has barcode segments" % os.path.join(d, "I1.fq"))
    # the rules of other options for two decoded files stay their own
    refused(plan_args(d, "--samples", sheet, "--join-barcodes", "--molecules"), "--molecules needs exactly one input file (2 given)")
    refused(plan_args(d, "--samples", sheet, "--join-barcodes", "--mate-bases", "8", "-dust", "0"), "--mate-bases: exactly one input file may have an architecture other than R:N (2 have)")
    refused(plan_args(d, "--samples", sheet, "--join-barcodes", "--min-base-quality", "20"), "--min-base-quality: exactly one input file may have an architecture other than R:N (2 have)")


def test_every_error_of_a_joined_sheet_names_file_and_segment(run_dir):
    d = run_dir
    out = os.path.join(d, "out")

    def sheet_error(text):
        p = os.path.join(d, "bad.txt")
        open(p, "w").write(text)
        with pytest.raises(TdError) as e:
            tdlib.run_plan(plan_args(d, "--samples", p, "--join-barcodes"))
        return str(e.value).replace(p, "SHEET").replace(d + os.sep, "")

    assert sheet_error("s1 ACAGTG\n") == "--samples: SHEET line 1: 2 columns, need 3 (the name and one barcode per barcode segment of every barcode file, files first)."
    assert sheet_error("s1 ACAGTG AAGGTC\ns2 ACAGTG ACAGTG\n") == "--samples: SHEET line 2: 'ACAGTG' (column 2) is not a barcode of segment 1 of file 1 (I2.fq)."
    assert sheet_error("s1 AAGGTC AAGGTC\n") == "--samples: SHEET line 1: 'AAGGTC' (column 1) is not a barcode of segment 1 of file 0 (I1.fq)."
    assert sheet_error("s1 ACAGTG AAGGTC\n\ns2 ACAGTG AAGGTC\n") == "--samples: SHEET line 3: the barcodes repeat those of line 1."
    assert sheet_error("s1 ACAGTG AAGGTC\ns1 ACAGTG CCTTGA\n") == "--samples: SHEET line 2: the name 's1' is taken by line 1."
    assert sheet_error("# nothing\n") == "--samples: SHEET lists no sample."
    assert sheet_error("s1 ACAGTG NNNNNN\n") == "--samples: SHEET line 1: 'NNNNNN' (column 2) is not a barcode of segment 1 of file 1 (I2.fq)."


def test_the_option_is_in_the_usage_text_and_the_structures(library):
    import ctypes as C
    library.td_run_usage.restype = C.c_char_p
    assert "--join-barcodes " in library.td_run_usage().decode()
    assert tdlib._RunOptsJoin._fields_[-2:] == [("quality_offset", C.c_int32), ("join_barcodes", C.c_int32)]
    assert [f for f, _ in tdlib._RunReportJoin._fields_[-2:]] == ["quality_totals", "partner_failed"]
    o = tdlib.RunOpts(["--join-barcodes"])
    assert o.o.join_barcodes == 1 and tdlib.RunOpts([]).o.join_barcodes == 0
