"""The base-quality filter (include/tagdust_quality.h) on the host, no GPU: td_qual_pack against a numpy restatement, td_qual_host
over the reference's own labels and records (tests/golden) with generated and planted qualities against the definition restated here
in plain Python, every refusal of the parameters, the command's options, plan line and refusals, and the stand-alone program over
the host unit."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden
from tagdust_amd import TdError
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

SUCCESS, LOW_QUALITY = 0, 8
B, F, BF = tdlib.QUAL_SEG_B, tdlib.QUAL_SEG_F, tdlib.QUAL_SEG_B | tdlib.QUAL_SEG_F
Q, OFFSET = 20, 33
THR = OFFSET + Q
WITH_F = ["umi_f_s_r", "f_b_f_r", "c5_b96_f_r_p"]
WITHOUT_F = "c3_b6_s_r_p"


@pytest.fixture(scope="module", autouse=True)
def library():
    tdbuild.build()
    return tdlib.load_library()


# ---- td_qual_pack ----
def pack_np(qual, thr):
    """the definition: bit g & 31 of words[g >> 5] is qual[g] < thr; (n + 31) // 32 + 1 words, every other bit zero"""
    q = np.asarray(qual, np.uint8)
    n_words = (len(q) + 31) // 32 + 1
    bits = np.zeros(n_words * 32, np.uint8)
    bits[:len(q)] = q.astype(np.int32) < thr
    return np.packbits(bits, bitorder="little").view("<u4")


@pytest.mark.parametrize("n", [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000])
def test_pack_against_numpy(n):
    rng = np.random.default_rng(100 + n)
    q = rng.integers(0, 256, n).astype(np.uint8)          # bytes of 128 and more among them
    for thr in (THR, 64 + 40, 1, 255):
        if n:
            q[rng.integers(0, n)] = thr                    # equal to thr: not low
            q[rng.integers(0, n)] = thr - 1                # one below: low
        words = tdlib.qual_pack(q, thr)
        assert words.dtype == np.uint32 and len(words) == (n + 31) // 32 + 1
        assert np.array_equal(words, pack_np(q, thr))
        assert words[-1] == 0                              # the spare word


def test_pack_is_unsigned_and_exact_at_the_threshold():
    q = np.array([THR, THR - 1, 128, 255, 0, 127, THR + 1], np.uint8)
    words = tdlib.qual_pack(q, THR)
    assert [int(words[0] >> k) & 1 for k in range(7)] == [0, 1, 0, 0, 1, 0, 0] and words[0] >> 7 == 0 and words[1] == 0
    q = np.full(70, 200, np.uint8)                         # as signed chars these would all be negative
    assert not tdlib.qual_pack(q, THR).any()
    q = np.full(70, THR - 1, np.uint8)
    assert np.array_equal(tdlib.qual_pack(q, THR), np.array([0xFFFFFFFF, 0xFFFFFFFF, 0x3F, 0], np.uint32))
    with pytest.raises(TdError, match="thr"):
        tdlib.qual_pack(q, 300)


# ---- td_qual_host ----
def records(g):
    res = np.zeros(int(g["n_reads"]), tdlib.RESULT_DTYPE)
    for f in ("f_score", "b_score", "r_score", "bar_prob", "mapq", "read_type", "barcode", "fingerprint"):
        res[f] = np.asarray(g[f])
    return res


def judged_positions(md, offs, labels, i, segments):
    """the positions p of read i whose label's segment is of a chosen type"""
    o, ln = int(offs[i]), int(offs[i + 1] - offs[i])
    lab = labels[o + i:o + i + ln + 1]
    want = [ord(c) for c, bit in (("B", B), ("F", F)) if segments & bit]
    return [p for p in range(ln) if int(md["seg_type"][int(md["label"][int(lab[p + 1])]) & 0xFFFF]) in want]


def qual_py(md, offs, res, labels, qual, min_quality, offset, max_low, segments):
    """The definition: (rewritten records, totals)."""
    out = res.copy()
    tot = dict.fromkeys(tdlib.QUALITY_TOTALS, 0)
    thr = offset + min_quality
    for i in range(len(offs) - 1):
        if int(res["read_type"][i]) != SUCCESS:
            continue
        tot["eligible"] += 1
        n_low = sum(1 for p in judged_positions(md, offs, labels, i, segments) if int(qual[int(offs[i]) + p]) < thr)
        tot["low_bases"] += n_low
        if n_low > max_low:
            tot["failed"] += 1
            out["read_type"][i] = LOW_QUALITY
        else:
            tot["passed"] += 1
    return out, tot


def generated_qualities(n_bases, seed):
    """each base low with probability 0.05"""
    rng = np.random.default_rng(seed)
    low = rng.random(n_bases) < 0.05
    return np.where(low, THR - 1 - rng.integers(0, 15, n_bases), THR + rng.integers(0, 40, n_bases)).astype(np.uint8)


def planted(md, offs, res, labels, qual, max_low, segments):
    """qualities with four reads written by hand; returns (qual, {what: read})"""
    qual = qual.copy()
    elig = [i for i in range(len(offs) - 1) if int(res["read_type"][i]) == SUCCESS and
            len(judged_positions(md, offs, labels, i, segments)) >= max_low + 1]
    other = [i for i in range(len(offs) - 1) if int(res["read_type"][i]) != SUCCESS]
    assert len(elig) >= 3 and other
    where = {"outside": elig[0], "exactly_k": elig[1], "k_plus_1": elig[2], "not_eligible": other[0]}
    for what, i in where.items():
        o, ln = int(offs[i]), int(offs[i + 1] - offs[i])
        j = judged_positions(md, offs, labels, i, segments)
        if what == "outside":                  # low bases only in positions that are not judged: the read passes
            qual[o:o + ln] = THR - 1
            qual[o + np.array(j, np.int64)] = THR
            assert ln > len(j)
        elif what == "not_eligible":           # full of low bases, and untouched
            qual[o:o + ln] = OFFSET
        else:
            qual[o:o + ln] = THR + 5
            qual[o + np.array(j[:max_low + (what == "k_plus_1")], np.int64)] = THR - 1
    return qual, where


def has_type(md, segments):
    types = {int(t) for t in md["seg_type"]}
    return bool((segments & B and ord("B") in types) or (segments & F and ord("F") in types))


@pytest.mark.parametrize("max_low", [0, 2])
@pytest.mark.parametrize("segments", [B, F, BF], ids=["B", "F", "BF"])
@pytest.mark.parametrize("name", WITH_F + [WITHOUT_F])
def test_host_against_the_definition(name, segments, max_low):
    g = load_golden(name)
    offs, labels, res = g["offs"].astype(np.int64), g["labels"], records(g)
    qual = generated_qualities(int(offs[-1]), 7)
    if not has_type(g, segments):              # (umi_f_s_r has no 'B' segment, c3_b6_s_r_p no 'F': the definition refuses)
        with pytest.raises(TdError, match="no '[BF]' segment"):
            tdlib.qual_host(g, offs, res, labels, qual, Q, OFFSET, max_low, segments)
        return
    qual, where = planted(g, offs, res, labels, qual, max_low, segments)
    got, tot = tdlib.qual_host(g, offs, res, labels, qual, Q, OFFSET, max_low, segments)
    want, want_tot = qual_py(g, offs, res, labels, qual, Q, OFFSET, max_low, segments)
    assert got.tobytes() == want.tobytes() and tot == want_tot
    assert tot["failed"] >= 1 and tot["passed"] >= 1 and tot["eligible"] == tot["passed"] + tot["failed"]
    assert got["read_type"][where["outside"]] == SUCCESS and got["read_type"][where["exactly_k"]] == SUCCESS
    assert got["read_type"][where["k_plus_1"]] == LOW_QUALITY
    assert got["read_type"][where["not_eligible"]] == res["read_type"][where["not_eligible"]] != SUCCESS
    changed = got["read_type"] != res["read_type"]
    assert int(changed.sum()) == tot["failed"] and set(res["read_type"][changed]) == {SUCCESS}
    for f in ("f_score", "b_score", "r_score", "bar_prob", "mapq", "barcode", "fingerprint"):
        assert got[f].tobytes() == res[f].tobytes()


def test_host_with_offset_64_and_a_batch_that_does_not_start_at_zero():
    g = load_golden("f_b_f_r")
    offs, labels, res = g["offs"].astype(np.int64), g["labels"], records(g)
    qual = (generated_qualities(int(offs[-1]), 11).astype(np.int32) + 31).astype(np.uint8)
    whole, tot = tdlib.qual_host(g, offs, res, labels, qual, Q, 64, 1, BF)
    want, want_tot = qual_py(g, offs, res, labels, qual, Q, 64, 1, BF)
    assert whole.tobytes() == want.tobytes() and tot == want_tot and tot["failed"] >= 1 and tot["passed"] >= 1
    # reads 100.. as a batch of their own: the caller's offsets stay, the labels move by the reads in front
    lo = 100
    part, ptot = tdlib.qual_host(g, offs[lo:], res[lo:], labels[lo:], qual, Q, 64, 1, BF)
    assert part.tobytes() == whole[lo:].tobytes()
    head, htot = tdlib.qual_host(g, offs[:lo + 1], res[:lo], labels, qual, Q, 64, 1, BF)
    assert {k: htot[k] + ptot[k] for k in tot} == tot


def test_host_argument_checks():
    g = load_golden("f_b_f_r")
    offs, labels, res = g["offs"].astype(np.int64), g["labels"], records(g)
    qual = generated_qualities(int(offs[-1]), 3)
    for kw, msg in ((dict(min_quality=0), "min_quality"), (dict(min_quality=94), "min_quality"), (dict(offset=32), "offset"),
                    (dict(offset=0), "offset"), (dict(max_low=-1), "max_low"), (dict(segments=0), "segments"), (dict(segments=4), "segments")):
        a = dict(min_quality=Q, offset=OFFSET, max_low=0, segments=BF)
        a.update(kw)
        with pytest.raises(TdError, match="td_qual_host: " + msg):
            tdlib.qual_host(g, offs, res, labels, qual, **a)
    bad = offs.copy()
    bad[5] = bad[4] - 1
    with pytest.raises(TdError, match="td_qual_host: read 4 has length -1"):
        tdlib.qual_host(g, bad, res, labels, qual, Q)
    lib = tdlib._qual_lib()
    desc, keep = tdlib.make_model_desc(g)
    p, tot = tdlib._QualParams(Q, OFFSET, 0, BF), tdlib._QualTotals()
    assert lib.td_qual_host(None, C.byref(p), offs.ctypes.data, 1, res.ctypes.data, labels.ctypes.data, qual.ctypes.data, C.byref(tot)) != 0
    assert lib.td_qual_host(C.byref(desc), None, offs.ctypes.data, 1, res.ctypes.data, labels.ctypes.data, qual.ctypes.data, C.byref(tot)) != 0
    assert lib.td_qual_host(C.byref(desc), C.byref(p), None, 1, res.ctypes.data, labels.ctypes.data, qual.ctypes.data, C.byref(tot)) != 0
    assert lib.td_qual_host(C.byref(desc), C.byref(p), offs.ctypes.data, 1, res.ctypes.data, labels.ctypes.data, None, C.byref(tot)) != 0
    assert b"bad arguments" in lib.td_last_error(None)
    assert lib.td_qual_host(C.byref(desc), C.byref(p), offs.ctypes.data, 0, None, None, None, C.byref(tot)) == 0 and tot.eligible == 0


# ---- the ABI ----
def test_header_symbols_are_exported_and_bound(library):
    hdr = open(os.path.join(REPO, "include", "tagdust_quality.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = set(re.findall(r"\b(td_[a-z_0-9]+)\s*\(", hdr))
    assert found == set(tdlib.QUALITY_ABI_SYMBOLS)
    for name in sorted(found):
        assert hasattr(library, name), name
    main = open(os.path.join(REPO, "include", "tagdust_hip.h")).read()
    assert re.search(r"#define\s+TD_EXTRACT_FAIL_LOW_BASE_QUALITY\s+8\b", main) and tdlib.EXTRACT_FAIL_LOW_BASE_QUALITY == 8
    assert C.sizeof(tdlib._QualParams) == 16 and C.sizeof(tdlib._QualTotals) == 32
    # the options and the report's fields are appended: what earlier tests pin stays where it is
    assert [f for f, _ in tdlib._RunOptsQuality._fields_[-5:]] == ["samples_file", "min_base_quality", "max_low_bases", "quality_segments", "quality_offset"]
    assert [f for f, _ in tdlib._RunReportQuality._fields_[-3:]] == ["samples_totals", "quality", "quality_totals"]


# ---- the command ----
ARCH = ["-1", "B:ACGT,TTGA", "-2", "F:NNNNNN", "-3", "R:N"]


@pytest.fixture
def files(tmp_path):
    a, b = tmp_path / "a.fq", tmp_path / "b.fq"
    a.write_text("@r\nACGT\n+\nIIII\n")
    b.write_text("@r\nACGT\n+\nIIII\n")
    return str(a), str(b), str(tmp_path / "out")


def test_option_parsing():
    o = tdlib.RunOpts(["x.fq"]).o
    assert (o.min_base_quality, o.max_low_bases, o.quality_segments, o.quality_offset) == (0, 0, BF, 33)
    ro = tdlib.RunOpts(["--min-base-quality", "20", "--max-low-bases", "2", "--quality-segments", "F", "--quality-offset", "64", "x.fq"])
    assert (ro.o.min_base_quality, ro.o.max_low_bases, ro.o.quality_segments, ro.o.quality_offset) == (20, 2, F, 64)
    ro = tdlib.RunOpts(["--quality-segments", "B", "--min-base-quality", "93", "x.fq"])
    assert (ro.o.min_base_quality, ro.o.quality_segments) == (93, B)
    ro = tdlib.RunOpts(["--quality-segments", "BF", "--min-base-quality", "1", "x.fq"])
    assert (ro.o.min_base_quality, ro.o.quality_segments) == (1, BF)
    for bad, msg in ((["--min-base-quality", "0"], "1..93"), (["--min-base-quality", "94"], "1..93"), (["--min-base-quality", "x"], "1..93"),
                     (["--min-base-quality", "20", "--max-low-bases", "-1"], "K >= 0"), (["--min-base-quality", "20", "--quality-segments", "R"], "B, F or BF"),
                     (["--min-base-quality", "20", "--quality-offset", "50"], "33 or 64"), (["--max-low-bases", "1"], "need --min-base-quality"),
                     (["--quality-segments", "B"], "need --min-base-quality"), (["--quality-offset", "64"], "need --min-base-quality"),
                     (["-min-base-quality", "20"], "unknown option"), (["--min-base-quality"], "requires an argument")):
        with pytest.raises(TdError, match=msg):
            tdlib.RunOpts(bad + ["x.fq"] if bad != ["--min-base-quality"] else ["x.fq"] + bad)


def test_the_plan_s_quality_line(files):
    a, b, out = files
    plan = tdlib.run_plan(ARCH + [a, "-o", out, "--min-base-quality", "20"])
    line = [ln for ln in plan.splitlines() if ln.startswith("quality: ")]
    assert line == ["quality: an extracted read with more than 0 bases below Q20 (offset 33) in its barcode or fingerprint segments goes to _un "
                    "and is neither assigned, counted nor kept by --dedup"]
    plan = tdlib.run_plan(ARCH + [a, "-o", out, "--min-base-quality", "30", "--max-low-bases", "2", "--quality-segments", "F", "--quality-offset", "64"])
    assert "quality: an extracted read with more than 2 bases below Q30 (offset 64) in its fingerprint segments goes to _un" in plan
    assert "quality:" not in tdlib.run_plan(ARCH + [a, "-o", out])
    # pair mode is in: barcode and UMI in read 1, the cDNA in read 2
    plan = tdlib.run_plan(ARCH + [a, b, "-o", out, "--min-base-quality", "20", "--mate-bases", "8", "-dust", "0"])
    assert "quality: " in plan and "mate: 8 bases" in plan


def test_the_plan_s_refusals(files):
    a, b, out = files
    q = ["--min-base-quality", "20"]
    with pytest.raises(TdError, match="--min-base-quality cannot be combined with -start / -end"):
        tdlib.run_plan(ARCH + [a, "-o", out, "-start", "2", "-end", "30"] + q)
    with pytest.raises(TdError, match="--min-base-quality needs exactly one device"):
        tdlib.run_plan(ARCH + [a, "-o", out, "--devices", "0,1"] + q)
    with pytest.raises(TdError, match="--min-base-quality: the architecture is a single read segment"):
        tdlib.run_plan(["-1", "R:N", a, "-o", out] + q)
    # two decoded files (the second takes its architecture from a one-candidate arch file)
    arch = os.path.join(os.path.dirname(a), "arch.txt")
    open(arch, "w").write("tagdust -1 S:GGGG -2 R:N\n")
    with pytest.raises(TdError, match="--min-base-quality: exactly one input file may have an architecture other than R:N \\(2 have\\)"):
        tdlib.run_plan(ARCH + [a, b, "-o", out, "-arch", arch] + q)
    with pytest.raises(TdError, match="--min-base-quality: the architecture has no segment of the types --quality-segments names"):
        tdlib.run_plan(["-1", "B:ACGT,TTGA", "-2", "R:N", a, "-o", out, "--quality-segments", "F"] + q)
    assert "quality: " in tdlib.run_plan(["-1", "B:ACGT,TTGA", "-2", "R:N", a, "-o", out] + q)      # BF over a B-only architecture judges the barcode


def test_usage_names_the_options(library):
    library.td_run_usage.restype = C.c_char_p
    usage = library.td_run_usage().decode()
    for opt in ("--min-base-quality Q", "--max-low-bases K", "--quality-segments B|F|BF", "--quality-offset 33|64"):
        assert opt in usage, opt


def test_the_summary_s_extra_line():
    rep = tdlib._RunReportQuality()
    for k, v in {0: 700, 1: 100, 3: 90}.items():
        rep.counts[k] = v
    rep.quality = 1
    rep.quality_totals.failed = 50
    lib = tdlib._run_lib()

    def summary(args):
        o = tdlib.RunOpts(args)
        n = lib.td_run_format_summary(o.p, C.byref(rep), None, 0)
        buf = C.create_string_buffer(n + 1)
        lib.td_run_format_summary(o.p, C.byref(rep), buf, n + 1)
        return buf.value.decode()
    with_it = summary(["a.fq", "--min-base-quality", "20", "--max-low-bases", "1"])
    without = summary(["a.fq"])
    assert with_it == without + "50\tlow base quality in barcode / UMI (Q < 20, more than 1 bases)\n"
    assert without.endswith("0\tmatch artifacts:\n")


# ---- the stand-alone program over the host unit ----
def host_compiler():
    """$CXX, else g++, else the clang++ beside hipcc; with what makes it read its inputs as plain C++"""
    if os.environ.get("CXX"):
        return os.environ["CXX"].split(), []
    if shutil.which("g++"):
        return ["g++"], []
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for d in (os.path.dirname(os.path.realpath(hipcc)), "/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, "clang++")):
            return [os.path.join(d, "clang++")], ["-x", "c++"]
    return None, None


def test_the_host_unit_builds_and_agrees_without_hip(tmp_path):
    cxx, as_cxx = host_compiler()
    assert cxx, "no host C++ compiler: set CXX, or install g++"
    exe = str(tmp_path / "quality_host_check")
    srcs = [os.path.join(REPO, "tagdust_amd", "csrc", "td_quality_host.cpp"), os.path.join(REPO, "tools", "quality_host_check.cpp")]
    done = subprocess.run(cxx + ["-std=c++17", "-O1", "-Wall"] + as_cxx + srcs + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, done.stdout
    done = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0 and "quality_host_check: ok" in done.stdout.splitlines(), done.stdout


def test_the_sanitizer_script_builds_and_runs_the_program():
    script = open(os.path.join(REPO, "tools", "host_checks.sh")).read()
    assert "tools/quality_host_check.cpp -o $OUT/quality_host_check" in script
    assert "\n$OUT/quality_host_check &&" in script
