"""The census of barcode spellings (include/tagdust_census.h) on the host, no GPU: td_census_host over the reference's own labels,
outcomes and reads (tests/golden) against the definition restated here in plain Python; the refusals; key text and merge; the two
options of the whole-run driver (include/tagdust_run.h) and what they add to the plan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from tagdust_amd import TdError
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

DEFAULT = (1 << 1) | (1 << 3)
FIXTURES = ["c3_b6_s_r_p", "r_s_b_f", "b_s_b_r", "c2_indel_varlen", "casava_index"]


@pytest.fixture(scope="module", autouse=True)
def library():
    tdbuild.build()
    return tdlib.load_library()


def b_segments(g):
    return [j for j in range(int(g["S"])) if int(g["seg_type"][j]) == ord("B")]


def census_py(g, seq, offs, read_type, labels, segment, mask):
    """The definition: entries [(key, count)] by count descending then key ascending, and the seven totals."""
    seg_of = [int(v) & 0xFFFF for v in g["label"]]
    if segment == -1:
        segment = b_segments(g)[-1]
    tot = dict.fromkeys(tdlib.CENSUS_TOTALS, 0)
    counts = {}
    for i in range(len(offs) - 1):
        if not (mask >> (int(read_type[i]) & 0xFF)) & 1:
            continue
        tot["eligible"] += 1
        o, ln = int(offs[i]), int(offs[i + 1] - offs[i])
        lab = labels[o + i:o + i + ln + 1]
        word = [int(seq[o + p]) for p in range(ln) if seg_of[int(lab[p + 1])] == segment]
        if not word:
            tot["skipped_empty"] += 1
        elif len(word) > 28:
            tot["skipped_long"] += 1
        elif any(b > 3 for b in word):
            tot["skipped_n"] += 1
        else:
            key = len(word) << 56
            for k, b in enumerate(word):
                key |= b << (2 * (len(word) - 1 - k))
            counts[key] = counts.get(key, 0) + 1
            tot["counted"] += 1
    tot["distinct"] = len(counts)
    return sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])), tot


def as_pairs(entries):
    return [(int(k), int(c)) for k, c in zip(entries["key"], entries["count"])]


def listed_barcodes(g, segment):
    """the spellings the architecture lists for a segment (without the all-N wildcard)"""
    segs = [s for s in str(g["cmdline"]).split() if re.match(r"^[BRGOPSF]:", s)]
    return [w for w in segs[segment][2:].split(",")]


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("mask", [DEFAULT, 1 << 0], ids=["default-mask", "assigned"])
def test_host_census_is_the_definition_on_the_reference_s_fixtures(name, mask):
    g = load_golden(name)
    for segment in [-1] + b_segments(g):
        ent, tot = tdlib.census_host(g, g["seq"], g["offs"], g["read_type"], g["labels"], segment, mask)
        want, want_tot = census_py(g, g["seq"], g["offs"], g["read_type"], g["labels"], segment, mask)
        assert as_pairs(ent) == want, (name, segment)
        assert tot == want_tot, (name, segment)
        assert tot["eligible"] == tot["counted"] + tot["skipped_empty"] + tot["skipped_long"] + tot["skipped_n"] + tot["overflow"]
        assert tot["counted"] == int(ent["count"].sum()) and tot["overflow"] == 0
    if mask == 1:
        assert tot["eligible"] == int((np.asarray(g["read_type"]) == 0).sum()) > 0


def test_minus_one_is_the_last_b_segment():
    g = load_golden("b_s_b_r")
    assert b_segments(g) == [0, 2]
    last = tdlib.census_host(g, g["seq"], g["offs"], g["read_type"], g["labels"], -1, 1)
    assert as_pairs(last[0]) == as_pairs(tdlib.census_host(g, g["seq"], g["offs"], g["read_type"], g["labels"], 2, 1)[0])
    first = tdlib.census_host(g, g["seq"], g["offs"], g["read_type"], g["labels"], 0, 1)
    assert as_pairs(first[0]) != as_pairs(last[0])
    # (an indel makes a word one base longer or shorter; the most frequent spelling has the segment's own length)
    assert as_pairs(first[0])[0][0] >> 56 == int(g["seg_len"][0]) and as_pairs(last[0])[0][0] >> 56 == int(g["seg_len"][2])


@pytest.mark.parametrize("name", ["c3_b6_s_r_p", "r_s_b_f", "casava_index"])
def test_assigned_reads_mostly_spell_listed_barcodes(name):
    """mask 1 << 0 on a fixture without indels: the keys with the largest counts are listed barcodes of the architecture"""
    g = load_golden(name)
    seg = b_segments(g)[-1]
    listed = {tdlib.census_key(w) for w in listed_barcodes(g, seg) if set(w) <= set("ACGT")}
    assert listed
    ent, _ = tdlib.census_host(g, g["seq"], g["offs"], g["read_type"], g["labels"], -1, 1)
    top = as_pairs(ent)[:min(len(listed), 3)]
    assert top and all(k in listed for k, _ in top), [tdlib.census_key_text(k) for k, _ in top]


def test_refusals():
    g = load_golden("umi_f_s_r")
    assert not b_segments(g)
    with pytest.raises(TdError, match="no 'B' segment"):
        tdlib.census_host(g, g["seq"], g["offs"], g["read_type"], g["labels"])
    g = load_golden("c3_b6_s_r_p")
    not_b = [j for j in range(int(g["S"])) if j not in b_segments(g)][0]
    with pytest.raises(TdError, match="not a 'B' segment"):
        tdlib.census_host(g, g["seq"], g["offs"], g["read_type"], g["labels"], not_b)
    with pytest.raises(TdError, match="out of range"):
        tdlib.census_host(g, g["seq"], g["offs"], g["read_type"], g["labels"], int(g["S"]))
    for mask in (0, 1 << 8, 0x1FF):
        with pytest.raises(TdError, match="outcome_mask"):
            tdlib.census_host(g, g["seq"], g["offs"], g["read_type"], g["labels"], -1, mask)
    # log2_slots belongs to the device table: its range is written into td_census_enable, which needs a context (tests/test_census_gpu.py)
    src = open(os.path.join(REPO, "tagdust_amd", "csrc", "td_census.hip")).read()
    assert "log2_slots < 4 || log2_slots > 26" in src


def test_header_symbols_are_exported_and_bound(library):
    hdr = open(os.path.join(REPO, "include", "tagdust_census.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = set(re.findall(r"\b(td_[a-z_0-9]+)\s*\(", hdr))
    assert found == set(tdlib.CENSUS_ABI_SYMBOLS)
    for name in sorted(found):
        assert hasattr(library, name), name


def test_key_text_round_trip():
    rng = np.random.default_rng(3)
    for ln in list(range(1, 29)) * 3:
        w = "".join("ACGT"[b] for b in rng.integers(0, 4, ln))
        k = tdlib.census_key(w)
        assert k != 0 and k >> 56 == ln and tdlib.census_key_text(k) == w
    assert tdlib.census_key_text((6 << 56) | 0b000110111110) == "ACGTTG"
    for bad in (0, 29 << 56, (2 << 56) | (1 << 4), 5):
        with pytest.raises(TdError, match="no key"):
            tdlib.census_key_text(bad)


def test_merge_of_two_halves_is_the_whole_and_the_order_is_stable():
    g = load_golden("c3_b6_s_r_p")
    n = int(g["n_reads"])
    seq, offs, lab, rt = g["seq"], np.asarray(g["offs"], np.int64), g["labels"], np.asarray(g["read_type"])
    mask = 0xFF
    whole, tot = tdlib.census_host(g, seq, offs, rt, lab, -1, mask)
    cut = n // 2 + 1
    a, ta = tdlib.census_host(g, seq[:offs[cut]], offs[:cut + 1], rt[:cut], lab[:offs[cut] + cut], -1, mask)
    b, tb = tdlib.census_host(g, seq[offs[cut]:], offs[cut:] - offs[cut], rt[cut:], lab[offs[cut] + cut:], -1, mask)
    merged = tdlib.census_merge(a, b)
    assert as_pairs(merged) == as_pairs(whole) and len(whole) > 3
    assert all(ta[f] + tb[f] == tot[f] for f in tdlib.CENSUS_TOTALS if f != "distinct")
    # round trip: nothing added, nothing lost; the order does not depend on the order of the input
    empty = np.zeros(0, tdlib.CENSUS_ENTRY_DTYPE)
    assert as_pairs(tdlib.census_merge(whole, empty)) == as_pairs(whole) == as_pairs(tdlib.census_merge(empty, whole))
    rng = np.random.default_rng(11)
    for _ in range(5):
        both = np.concatenate([a, b])
        rng.shuffle(both)
        k = int(rng.integers(0, len(both) + 1))
        assert as_pairs(tdlib.census_merge(both[:k], both[k:])) == as_pairs(whole)
    pairs = as_pairs(whole)
    assert pairs == sorted(pairs, key=lambda kv: (-kv[1], kv[0]))


# ---- the run's options and plan ----
def _touch(d, name):
    p = os.path.join(str(d), name)
    open(p, "w").write("@r\nACGT\n+\nIIII\n")
    return p


def test_the_two_options_parse():
    o = tdlib.RunOpts(["in.fq"]).o
    assert (o.unknown_barcodes, o.unknown_slots_log2) == (0, 20)
    o = tdlib.RunOpts(["in.fq", "--unknown-barcodes", "10", "--unknown-barcodes-slots", "16"]).o
    assert (o.unknown_barcodes, o.unknown_slots_log2) == (10, 16)
    with pytest.raises(TdError, match="unknown option -unknown-barcodes"):   # own options take two dashes
        tdlib.RunOpts(["in.fq", "-unknown-barcodes", "10"])
    with pytest.raises(TdError, match="requires an argument"):
        tdlib.RunOpts(["in.fq", "--unknown-barcodes"])
    with pytest.raises(TdError, match="K >= 1"):
        tdlib.RunOpts(["in.fq", "--unknown-barcodes", "0"])
    for bad in ("3", "27"):
        with pytest.raises(TdError, match="4..26"):
            tdlib.RunOpts(["in.fq", "--unknown-barcodes-slots", bad])
    lib = tdlib.load_library()
    lib.td_run_usage.restype = C.c_char_p
    assert b"--unknown-barcodes K" in lib.td_run_usage() and b"--unknown-barcodes-slots N" in lib.td_run_usage()


def test_the_plan_with_and_without_the_option(tmp_path):
    fq = _touch(tmp_path, "in.fq")
    out = str(tmp_path / "o")
    base = ["-1", "B:ACGT,TTGA", "-2", "R:N", fq, "-o", out]
    without = tdlib.run_plan(base)
    with_opt = tdlib.run_plan(base + ["--unknown-barcodes", "5"])
    assert "unknown_barcodes" not in without
    assert with_opt == without + "output file: " + out + "_unknown_barcodes.txt\n"
    # the file joins the existing-output check
    open(out + "_unknown_barcodes.txt", "w").write("old\n")
    assert tdlib.run_plan(base) == without
    with pytest.raises(TdError, match="already exists.*_unknown_barcodes.txt"):
        tdlib.run_plan(base + ["--unknown-barcodes", "5"])
    assert tdlib.run_plan(base + ["--unknown-barcodes", "5", "--force"]) == with_opt


def test_the_option_is_refused_without_a_barcode_or_with_a_window(tmp_path):
    fq = _touch(tmp_path, "in.fq")
    out = str(tmp_path / "o")
    with pytest.raises(TdError, match="--unknown-barcodes.*no input file's architecture has a barcode segment"):
        tdlib.run_plan(["-1", "R:N", fq, "-o", out, "--unknown-barcodes", "5"])
    with pytest.raises(TdError, match="--unknown-barcodes.*no input file's architecture has a barcode segment"):
        tdlib.run_plan(["-1", "F:NNNN", "-2", "R:N", fq, "-o", out, "--unknown-barcodes", "5"])
    base = ["-1", "B:ACGT,TTGA", "-2", "R:N", fq, "-o", out, "--unknown-barcodes", "5"]
    for window in (["-start", "3"], ["-end", "30"], ["-start", "3", "-end", "30"]):
        with pytest.raises(TdError, match="--unknown-barcodes cannot be combined with -start / -end"):
            tdlib.run_plan(base + window)
    assert "_unknown_barcodes.txt" in tdlib.run_plan(base)
