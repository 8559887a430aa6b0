"""Sample assignment by all 'B' segments (include/tagdust_samples.h) on the host, no GPU: td_samples_host over the reference's own
labels and records (tests/golden) and over labels written by hand, against the definition restated here in plain Python; keys in
both directions and their merge; every failure of a sheet with its message."""
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from tagdust_amd import TdError
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

BSBR_SHEET = [(0, 0), (1, 1), (2, 2), (3, 0), (0, 1), (1, 2), (3, 2)]
SUCCESS, DEMOTED = 0, 3


@pytest.fixture(scope="module", autouse=True)
def library():
    tdbuild.build()
    return tdlib.load_library()


def b_segments(md):
    return [j for j in range(int(md["S"])) if int(md["seg_type"][j]) == ord("B")]


def records(g):
    """the fixture's per-read records as td_read_result"""
    res = np.zeros(int(g["n_reads"]), tdlib.RESULT_DTYPE)
    for f in ("f_score", "b_score", "r_score", "bar_prob", "mapq", "read_type", "barcode", "fingerprint"):
        res[f] = np.asarray(g[f])
    return res


def samples_py(md, sheet, offs, res, labels):
    """The definition: (rewritten records, entries [(key, count)] by count descending then key ascending, totals)."""
    segs = b_segments(md)
    m = len(segs)
    rows = {tuple(int(b) for b in np.atleast_1d(r)): s for s, r in enumerate(sheet)}
    out = res.copy()
    tot = dict.fromkeys(tdlib.SAMPLES_TOTALS, 0)
    counts = {}
    for i in range(len(offs) - 1):
        if int(res["read_type"][i]) != SUCCESS:
            continue
        tot["eligible"] += 1
        o, ln = int(offs[i]), int(offs[i + 1] - offs[i])
        lab = labels[o + i:o + i + ln + 1]
        calls = [-1] * m
        for p in range(ln):
            v = int(md["label"][int(lab[p + 1])])
            if (v & 0xFFFF) in segs:
                calls[segs.index(v & 0xFFFF)] = (v >> 16) & 0x7FFF
        key = (m << 56) | sum((c + 1) << (8 * t) for t, c in enumerate(calls))
        counts[key] = counts.get(key, 0) + 1
        if any(c == -1 or c == int(md["n_hmm"][segs[t]]) - 1 for t, c in enumerate(calls)):
            tot["incomplete"] += 1
            out["read_type"][i] = DEMOTED
        elif tuple(calls) in rows:
            tot["assigned"] += 1
            out["barcode"][i] = (segs[-1] << 16) | rows[tuple(calls)]
        else:
            tot["unlisted"] += 1
            out["read_type"][i] = DEMOTED
    return out, sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])), tot


def as_pairs(entries):
    return [(int(k), int(c)) for k, c in zip(entries["key"], entries["count"])]


def check_against_the_definition(md, sheet, offs, res, labels):
    got, ent, tot = tdlib.samples_host(md, sheet, offs, res, labels)
    want, want_ent, want_tot = samples_py(md, sheet, offs, res, labels)
    assert got.tobytes() == want.tobytes()
    assert as_pairs(ent) == want_ent and tot == want_tot
    assert tot["eligible"] == tot["assigned"] + tot["unlisted"] + tot["incomplete"] and tot["overflow"] == 0
    assert int(ent["count"].sum()) == tot["eligible"]
    return got, ent, tot


def test_the_reference_s_fixture_with_two_barcode_segments():
    g = load_golden("b_s_b_r")
    assert b_segments(g) == [0, 2]
    res = records(g)
    got, ent, tot = check_against_the_definition(g, BSBR_SHEET, g["offs"], res, g["labels"])
    assert tot == {"eligible": 185, "assigned": 109, "unlisted": 76, "incomplete": 0, "overflow": 0}
    assert len(ent) == 12
    changed = got["read_type"] != res["read_type"]
    assert int(changed.sum()) == 76 and set(got["read_type"][changed]) == {DEMOTED} and set(res["read_type"][changed]) == {SUCCESS}
    assert np.array_equal(got["barcode"][changed], res["barcode"][changed])
    kept = (got["read_type"] == SUCCESS)
    assert int(kept.sum()) == 109 and set(got["barcode"][kept] >> 16) == {2} and set(got["barcode"][kept] & 0xFFFF) <= set(range(7))
    for f in ("f_score", "b_score", "r_score", "bar_prob", "mapq", "fingerprint"):
        assert got[f].tobytes() == res[f].tobytes()
    # the pair names the sample: the reference's own barcode is the last segment's call alone
    last = res["barcode"][kept] & 0xFFFF
    assert all(BSBR_SHEET[int(s)][1] == int(b) for s, b in zip(got["barcode"][kept] & 0xFFFF, last))


def hand(md, paths):
    """reads whose labels are written by hand: paths = one list of HMM indices per read; every read is extracted"""
    offs = np.zeros(len(paths) + 1, np.int64)
    offs[1:] = np.cumsum([len(p) for p in paths])
    labels = np.concatenate([np.array([0] + list(p), np.int8) for p in paths])
    res = np.zeros(len(paths), tdlib.RESULT_DTYPE)
    res["barcode"] = -1
    return offs, res, labels


def hmms(md, seg):
    """the HMM indices of a segment in the order of their calls"""
    hs = [h for h in range(int(md["H"])) if int(md["label"][h]) & 0xFFFF == seg]
    return sorted(hs, key=lambda h: int(md["label"][h]) >> 16)


def test_labels_written_by_hand():
    g = load_golden("b_s_b_r")
    b0, s1, b2, r3 = (hmms(g, j) for j in range(4))
    assert len(b0) == 5 and len(b2) == 4
    tail = [r3[0]] * 5
    paths = [
        [b0[1]] * 6 + [s1[0]] * 2 + [b2[1]] * 4 + tail,      # (1, 1): listed
        [b0[2]] * 6 + [s1[0]] * 2 + [b2[0]] * 4 + tail,      # (2, 0): complete, not listed
        [s1[0]] * 2 + [b2[1]] * 4 + tail,                    # the first segment without a position
        [b0[1]] * 6 + [s1[0]] * 2 + tail,                    # the last segment without a position
        [b0[4]] * 6 + [s1[0]] * 2 + [b2[1]] * 4 + tail,      # the decoy in the first segment
        [b0[1]] * 6 + [s1[0]] * 2 + [b2[3]] * 4 + tail,      # the decoy in the last
        [b0[0]] * 3 + [b0[1]] * 3 + [s1[0]] * 2 + [b2[0]] * 2 + [b2[1]] * 2 + tail,   # visited twice with two HMMs: the last position wins
        [b0[4]] * 3 + [b0[0]] * 3 + [s1[0]] * 2 + [b2[0]] * 4 + tail,   # ... also over the decoy
        tail,                                                # no barcode at all
        [],                                                  # no base at all
    ]
    offs, res, labels = hand(g, paths)
    got, ent, tot = check_against_the_definition(g, BSBR_SHEET, offs, res, labels)
    assert list(got["read_type"]) == [0, 3, 3, 3, 3, 3, 0, 0, 3, 3]
    assert list(got["barcode"]) == [(2 << 16) | 1, -1, -1, -1, -1, -1, (2 << 16) | 1, (2 << 16) | 0, -1, -1]
    key = tdlib.samples_key
    assert dict(as_pairs(ent)) == {key([1, 1]): 2, key([2, 0]): 1, key([-1, 1]): 1, key([1, -1]): 1, key([4, 1]): 1, key([1, 3]): 1, key([0, 0]): 1,
                                   key([-1, -1]): 2}
    assert tot == {"eligible": 10, "assigned": 3, "unlisted": 1, "incomplete": 6, "overflow": 0}
    # a read that is not eligible is untouched, whatever its labels say
    res2 = res.copy()
    res2["read_type"] = [1, 2, 3, 5, 6, 7, 1, 1 << 8, -1, 2]
    got2, ent2, tot2 = check_against_the_definition(g, BSBR_SHEET, offs, res2, labels)
    assert got2.tobytes() == res2.tobytes() and len(ent2) == 0 and tot2["eligible"] == 0


def test_one_segment_and_a_sheet_that_lists_a_subset():
    g = load_golden("c2_b4_r")
    segs = b_segments(g)
    assert len(segs) == 1
    n_bar = int(g["n_hmm"][segs[0]]) - 1
    sheet = [[b] for b in range(n_bar) if b % 2 == 0][::-1]          # every other barcode, in descending order
    res = records(g)
    got, ent, tot = check_against_the_definition(g, sheet, g["offs"], res, g["labels"])
    assert tot["assigned"] > 0 and tot["unlisted"] > 0
    kept = got["read_type"] == SUCCESS
    # m = 1: the reference's own call is the one call, a sample is a renumbering of it
    assert all(sheet[int(s)][0] == int(b) for s, b in zip(got["barcode"][kept] & 0xFFFF, res["barcode"][kept] & 0xFFFF))
    assert all(k >> 56 == 1 for k, _ in as_pairs(ent))


@pytest.fixture(scope="module")
def four_segments():
    """B / S / B / S / B / S / B / R with two barcodes each, built by the library's own model builder"""
    rng = np.random.default_rng(3)
    bars = [["ACGT", "TGCA"], ["AAGG", "CCTT"], ["GATC", "CTAG"], ["AGAG", "TCTC"]]
    reads = []
    for _ in range(40):
        parts = []
        for t in range(4):
            parts += [bars[t][int(rng.integers(0, 2))], "GT"]
        reads.append(np.array([b"ACGT".index(c) for c in "".join(parts[:-1]).encode()] + list(rng.integers(0, 4, 30)), np.uint8))
    offs = np.zeros(len(reads) + 1, np.int64)
    offs[1:] = np.cumsum([len(r) for r in reads])
    segs = ["B:" + ",".join(bars[0]), "S:GT", "B:" + ",".join(bars[1]), "S:GT", "B:" + ",".join(bars[2]), "S:GT", "B:" + ",".join(bars[3]), "R:N"]
    md, _ = tdlib.build_model(segs, np.concatenate(reads), offs)
    return md


def test_four_segments(four_segments):
    md = four_segments
    segs = b_segments(md)
    assert segs == [0, 2, 4, 6] and all(int(md["n_hmm"][j]) == 3 for j in segs)
    rng = np.random.default_rng(4)
    paths = []
    for _ in range(200):
        p = []
        for j in range(int(md["S"])):
            if j in segs and rng.random() < 0.05:
                continue                                     # a segment without a position
            hs = hmms(md, j)
            if j in segs and rng.random() >= 0.05:
                hs = hs[:-1]                                 # (the decoy in one segment of twenty)
            p += [hs[int(rng.integers(0, len(hs)))]] * int(rng.integers(1, 5))
        paths.append(p)
    offs, res, labels = hand(md, paths)
    sheet = [(a, b, c, d) for a in range(2) for b in range(2) for c in range(2) for d in range(2) if (a + b + c + d) % 2 == 0]
    got, ent, tot = check_against_the_definition(md, sheet, offs, res, labels)
    assert min(tot["assigned"], tot["unlisted"], tot["incomplete"]) >= 10
    assert all(k >> 56 == 4 for k, _ in as_pairs(ent))
    assert set(got["barcode"][got["read_type"] == SUCCESS] >> 16) == {6}


def test_keys_in_both_directions():
    rng = np.random.default_rng(5)
    for m in (1, 2, 3, 4) * 20:
        calls = [int(c) for c in rng.integers(-1, 127, m)]
        k = tdlib.samples_key(calls)
        assert k != 0 and k >> 56 == m and tdlib.samples_key_calls(k) == calls
    assert tdlib.samples_key([1, 4]) == (2 << 56) | 2 | (5 << 8)
    assert tdlib.samples_key([-1]) == 1 << 56                # no call at all is still a key
    for bad in ([], [0] * 5, [127], [-2, 0]):
        with pytest.raises(TdError, match="no calls"):
            tdlib.samples_key(bad)
    for bad in (0, 5 << 56, (1 << 56) | (1 << 8), (2 << 56) | 0x81, 7):
        with pytest.raises(TdError, match="no key"):
            tdlib.samples_key_calls(bad)


def test_merge_of_two_halves_is_the_whole():
    g = load_golden("b_s_b_r")
    res, offs, lab = records(g), np.asarray(g["offs"], np.int64), g["labels"]
    _, whole, tot = tdlib.samples_host(g, BSBR_SHEET, offs, res, lab)
    cut = len(res) // 3
    ra, a, ta = tdlib.samples_host(g, BSBR_SHEET, offs[:cut + 1], res[:cut], lab[:offs[cut] + cut])
    rb, b, tb = tdlib.samples_host(g, BSBR_SHEET, offs[cut:] - offs[cut], res[cut:], lab[offs[cut] + cut:])
    assert as_pairs(tdlib.census_merge(a, b)) == as_pairs(whole) and len(a) > 3 and len(b) > 3
    assert all(ta[f] + tb[f] == tot[f] for f in tdlib.SAMPLES_TOTALS)
    assert np.concatenate([ra, rb]).tobytes() == tdlib.samples_host(g, BSBR_SHEET, offs, res, lab)[0].tobytes()


def test_every_failure_of_a_sheet_has_its_message(four_segments):
    g = load_golden("b_s_b_r")
    res = records(g)

    def host(md, sheet):
        return tdlib.samples_host(md, sheet, g["offs"], res, g["labels"])

    u = load_golden("umi_f_s_r")
    with pytest.raises(TdError, match="td_samples_host: the model has no 'B' segment"):
        tdlib.samples_host(u, [[0]], u["offs"], records(u), u["labels"])
    with pytest.raises(TdError, match=r"n_samples = 0 \(1..255 supported\)"):
        host(g, np.zeros((0, 2), np.int32))
    with pytest.raises(TdError, match=r"n_samples = 256 \(1..255 supported\)"):
        host(g, np.zeros((256, 2), np.int32))
    with pytest.raises(TdError, match=r"row 1 of the sheet: barcode 4 of 'B' segment 0 \(column 0\) is out of range \(0..3; the last HMM is the all-N decoy\)"):
        host(g, [(0, 0), (4, 0)])                            # the decoy cannot be listed
    with pytest.raises(TdError, match=r"row 2 of the sheet: barcode 3 of 'B' segment 2 \(column 1\) is out of range \(0..2;"):
        host(g, [(0, 0), (1, 0), (0, 3)])
    with pytest.raises(TdError, match=r"row 0 of the sheet: barcode -1 of 'B' segment 0"):
        host(g, [(-1, 0)])
    with pytest.raises(TdError, match="row 3 of the sheet repeats row 1"):
        host(g, [(0, 0), (1, 2), (2, 2), (1, 2)])
    # five 'B' segments: the four-segment model with its 'R' segment called a barcode segment
    five = dict(four_segments)
    five["seg_type"] = np.array([ord("B") if j == 7 else int(t) for j, t in enumerate(four_segments["seg_type"])], np.int32)
    offs, res5, labels = hand(five, [[0]])
    with pytest.raises(TdError, match=r"the model has 5 'B' segments \(at most 4\)"):
        tdlib.samples_host(five, [(0, 0, 0, 0, 0)], offs, res5, labels)
    # what needs a context is written into td_samples_enable (tests/test_samples_gpu.py runs it)
    src = open(os.path.join(REPO, "tagdust_amd", "csrc", "td_samples.hip")).read()
    for text in ("td_samples_enable: no model uploaded", "td_samples_enable: td_submit tickets are outstanding", "log2_slots < 4 || log2_slots > 26",
                 "td_samples_enable: a -start/-end window is set"):
        assert text in src


def test_names_are_checked_by_the_unit_the_context_uses():
    src = open(os.path.join(REPO, "tagdust_amd", "csrc", "td_samples_host.cpp")).read()
    for text in ("a name has 1..%d characters", "holds a character outside [A-Za-z0-9._-]", "is taken by an earlier row"):
        assert text in src


def test_the_host_unit_builds_and_agrees_without_hip(tmp_path):
    """td_samples_host.cpp with the host compiler alone, and the stand-alone program over it (tools/host_checks.sh runs it under the sanitizers)"""
    import shutil
    import subprocess
    cxx = os.environ.get("CXX", "").split() or (["g++"] if shutil.which("g++") else None)
    as_cxx = []
    if not cxx:
        for d in (os.path.dirname(os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))), "/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin"):
            if not cxx and os.path.exists(os.path.join(d, "clang++")):
                cxx, as_cxx = [os.path.join(d, "clang++")], ["-x", "c++"]
    assert cxx, "no host C++ compiler: set CXX, or install g++"
    exe = str(tmp_path / "samples_host_check")
    sources = [os.path.join(REPO, "tagdust_amd", "csrc", u) for u in ("td_census_host.cpp", "td_samples_host.cpp")] + \
        [os.path.join(REPO, "tools", "samples_host_check.cpp")]
    for cmd in (cxx + ["-std=c++17", "-O1", "-Wall"] + as_cxx + sources + ["-o", exe], [exe]):
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert done.returncode == 0, " ".join(cmd) + "\n" + done.stdout
    assert "samples_host_check: ok" in done.stdout.splitlines()
    script = open(os.path.join(REPO, "tools", "host_checks.sh")).read()
    assert "tools/samples_host_check.cpp -o $OUT/samples_host_check" in script and "\n$OUT/samples_host_check &&" in script


def test_header_symbols_are_exported_and_bound(library):
    hdr = open(os.path.join(REPO, "include", "tagdust_samples.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = set(re.findall(r"\b(td_[a-z_0-9]+)\s*\(", hdr))
    assert found == set(tdlib.SAMPLES_ABI_SYMBOLS)
    for name in sorted(found):
        assert hasattr(library, name), name


def test_the_kernel_is_plain_hip_in_front_of_the_counts():
    """where the step stands in launch_end: behind the mate join and the -ref hits, in front of the census and the molecule count"""
    src = open(os.path.join(REPO, "tagdust_amd", "csrc", "td_batch.hip")).read()
    body = src[src.index("static int launch_end("):]
    order = [body.index(w) for w in ("mol_mate_join(", "slot_count_hits(", "samples_slot(", "census_count_slot(", "mol_slot_decoded(")]
    assert order == sorted(order)
    kernel = open(os.path.join(REPO, "tagdust_amd", "csrc", "td_samples.hip")).read()
    assert "asm" not in kernel and "kt_walk_tile(" in kernel and "kt_wave_add(" in kernel and "kt_launch_slot(" in kernel


# ---- the command: --samples FILE ----
B1 = ["ACAGTG", "CTTGTA", "GGCTAC", "TTAGGC"]
B2 = ["AACC", "GGTT", "CATG"]
TWO = ["-1", "B:" + ",".join(B1), "-2", "S:GT", "-3", "B:" + ",".join(B2), "-4", "R:N"]
GOOD_SHEET = "# plate 7\nA1\tACAGTG\tAACC\n\nA2  CTTGTA  GGTT\n  # a comment behind white space\nB-1.x_y\tTTAGGC\tCATG\n"


def _touch(d, name, text="@r\nACGT\n+\nIIII\n"):
    p = os.path.join(str(d), name)
    open(p, "w").write(text)
    return p


def test_the_option_parses_and_is_in_the_usage_text():
    import ctypes as C
    assert tdlib.RunOpts(["in.fq"]).o.samples_file is None
    assert tdlib.RunOpts(["in.fq", "--samples", "sheet.txt"]).o.samples_file == b"sheet.txt"
    with pytest.raises(TdError, match="unknown option -samples"):    # own options take two dashes
        tdlib.RunOpts(["in.fq", "-samples", "sheet.txt"])
    with pytest.raises(TdError, match="requires an argument"):
        tdlib.RunOpts(["in.fq", "--samples"])
    lib = tdlib.load_library()
    lib.td_run_usage.restype = C.c_char_p
    assert b"--samples FILE" in lib.td_run_usage()
    assert tdlib._RunOptsSamples._fields_[-1] == ("samples_file", C.c_char_p)


def test_the_plan_line_and_the_file_names(tmp_path):
    fq = _touch(tmp_path, "in.fq")
    sheet = _touch(tmp_path, "sheet.txt", GOOD_SHEET)
    out = str(tmp_path / "o")
    base = TWO + [fq, "-o", out]
    without = tdlib.run_plan(base)
    assert "samples:" not in without and "output file: %s_BC_ACAGTG.fq\n" % out in without
    plan = tdlib.run_plan(base + ["--samples", sheet])
    assert "samples: %s: 3 samples by segments 1, 3 of file 0; a read whose barcodes are incomplete or name no sample goes to _un\n" % sheet in plan
    want = [out + "_BC_A1.fq", out + "_BC_A2.fq", out + "_BC_B-1.x_y.fq", out + "_un.fq", out + "_samples.txt"]
    assert [l[len("output file: "):] for l in plan.splitlines() if l.startswith("output file: ")] == want
    assert tdlib.run_output_files(["in.fq", "-o", out, "--samples", sheet], [" ".join(TWO)]) == want
    # two files: one set per read segment of the run, the sample names in front of the read's number
    fq2 = _touch(tmp_path, "in2.fq")
    names = tdlib.run_output_files(["in.fq", "in2.fq", "-o", out, "--samples", sheet], [" ".join(TWO), "-1 R:N"])
    assert names == [out + "_BC_%s_READ%d.fq" % (s, k) if s else out + "_un_READ%d.fq" % k for k in (1, 2) for s in ("A1", "A2", "B-1.x_y", None)] + \
        [out + "_samples.txt"]
    assert "file 1 architecture: default: -1 R:N" in tdlib.run_plan(TWO + [fq, fq2, "-o", out, "--samples", sheet])
    # one barcode segment: "segment", and a one-column sheet
    one = _touch(tmp_path, "one.txt", "x CTTGTA\ny ACAGTG\n")
    plan = tdlib.run_plan(["-1", "B:" + ",".join(B1), "-2", "R:N", fq, "-o", out, "--samples", one])
    assert "samples: %s: 2 samples by segment 1 of file 0;" % one in plan and "output file: %s_BC_x.fq\noutput file: %s_BC_y.fq\n" % (out, out) in plan
    # the existing-file check and --force use the new names
    open(out + "_BC_A2.fq", "w").write("old\n")
    assert tdlib.run_plan(base) == without
    with pytest.raises(TdError, match="already exists.*_BC_A2.fq"):
        tdlib.run_plan(base + ["--samples", sheet])
    assert "samples:" in tdlib.run_plan(base + ["--samples", sheet, "--force"])
    os.remove(out + "_BC_A2.fq")
    open(out + "_samples.txt", "w").write("old\n")
    with pytest.raises(TdError, match="already exists.*_samples.txt"):
        tdlib.run_plan(base + ["--samples", sheet])


def test_the_sheet_is_resolved_once_the_arch_file_s_choice_is_made(tmp_path):
    fq = _touch(tmp_path, "in.fq")
    sheet = _touch(tmp_path, "sheet.txt", GOOD_SHEET)
    arch = _touch(tmp_path, "arch.txt", "tagdust " + " ".join(TWO) + "\ntagdust -1 R:N\n")
    out = str(tmp_path / "o")
    plan = tdlib.run_plan(["-arch", arch, fq, "-o", out, "--samples", sheet])
    assert "samples: %s: resolved once the arch file's choice is made\n" % sheet in plan
    one = _touch(tmp_path, "one.txt", "tagdust " + " ".join(TWO) + "\n")      # one candidate: nothing to choose
    plan = tdlib.run_plan(["-arch", one, fq, "-o", out, "--samples", sheet])
    assert "3 samples by segments 1, 3 of file 0" in plan and "output file: %s_BC_A1.fq\n" % out in plan


@pytest.mark.parametrize("text, message", [
    ("A1 ACAGTG AACC\nA2 CTTGTA\n", r"line 2: 2 columns, need 3 \(the name and one barcode per barcode segment\)"),
    ("A1 ACAGTG AACC GGTT\n", r"line 1: 4 columns, need 3"),
    ("# x\n\nA1 ACAGTG AACC\nA2 CTTGTT GGTT\n", r"line 4: 'CTTGTT' is not a barcode of segment 1"),
    ("A1 ACAGTG AACC\nA2 CTTGTA ACAGTG\n", r"line 2: 'ACAGTG' is not a barcode of segment 3"),
    ("A1 NNNNNN AACC\n", r"line 1: 'NNNNNN' is not a barcode of segment 1"),            # the decoy cannot be listed
    ("A1 ACAGTG AACC\nA2 CTTGTA GGTT\n\nA3 ACAGTG AACC\n", r"line 4: the barcodes repeat those of line 1"),
    ("A1 ACAGTG AACC\nA2 CTTGTA GGTT\nA1 GGCTAC CATG\n", r"line 3: the name 'A1' is taken by line 1"),
    ("A/1 ACAGTG AACC\n", r"line 1: the name 'A/1' is not 1..64 characters of \[A-Za-z0-9._-\]"),
    ("%s ACAGTG AACC\n" % ("x" * 65), r"line 1: the name 'x{65}' is not 1..64 characters"),
    ("# nothing\n\n", r"lists no sample"),
])
def test_the_sheet_parser_names_the_line(tmp_path, text, message):
    fq = _touch(tmp_path, "in.fq")
    sheet = _touch(tmp_path, "sheet.txt", text)
    with pytest.raises(TdError, match="--samples: .*sheet.txt " + message):
        tdlib.run_plan(TWO + [fq, "-o", str(tmp_path / "o"), "--samples", sheet])


def test_the_option_is_refused_without_a_barcode_with_a_window_and_across_files(tmp_path):
    fq = _touch(tmp_path, "in.fq")
    fq2 = _touch(tmp_path, "in2.fq")
    sheet = _touch(tmp_path, "sheet.txt", GOOD_SHEET)
    out = str(tmp_path / "o")
    for arch in (["-1", "R:N"], ["-1", "F:NNNN", "-2", "R:N"]):
        with pytest.raises(TdError, match="--samples: no input file's architecture has a barcode segment"):
            tdlib.run_plan(arch + [fq, "-o", out, "--samples", sheet])
    for window in (["-start", "3"], ["-end", "30"], ["-start", "3", "-end", "30"]):
        with pytest.raises(TdError, match="--samples cannot be combined with -start / -end"):
            tdlib.run_plan(TWO + [fq, "-o", out, "--samples", sheet] + window)
    with pytest.raises(TdError, match="--samples: the sample sheet .*missing.txt does not exist"):
        tdlib.run_plan(TWO + [fq, "-o", out, "--samples", str(tmp_path / "missing.txt")])
    # barcodes in two files: the controller's one-barcode-file rule stays, and with a sheet the refusal says so
    with pytest.raises(TdError, match="Barcodes seem to be in both architectures.*--samples: barcodes spread over several input files are not joined"):
        tdlib.run_output_files(["in.fq", "in2.fq", "-o", out, "--samples", sheet], [" ".join(TWO), "-1 B:AAAA,CCCC -2 R:N"])
    with pytest.raises(TdError, match=r"Barcodes seem to be in both architectures\.\.\. $"):
        tdlib.run_output_files(["in.fq", "in2.fq", "-o", out], [" ".join(TWO), "-1 B:AAAA,CCCC -2 R:N"])
    five = ["-%d" % (k + 1) for k in range(6)]
    segs = ["B:AC,GT", "B:AC,GT", "B:AC,GT", "B:AC,GT", "B:AC,GT", "R:N"]
    with pytest.raises(TdError, match=r"--samples: the architecture has 5 barcode segments \(at most 4\)"):
        tdlib.run_plan([x for pair in zip(five, segs) for x in pair] + [fq, "-o", out, "--samples", sheet])
