"""The molecule count (include/tagdust_molecules.h) on the host, no GPU: td_mol_host over the reference's own labels, outcomes,
barcodes, fingerprints and reads (tests/golden) against the definition restated here in plain Python, key function included;
td_mol_summarise against Python; merging; the refusals; the options of the whole-run driver and what they add to the plan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from tagdust_amd import TdError
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

M64 = (1 << 64) - 1
FIXTURES = ["umi_f_s_r", "r_s_b_f", "f_b_f_r", "c5_b96_f_r_p", "c3_b6_s_r_p", "c2_indel_varlen"]


@pytest.fixture(scope="module", autouse=True)
def library():
    tdbuild.build()
    return tdlib.load_library()


def mix(k):
    k ^= k >> 30
    k = (k * 0xBF58476D1CE4E5B9) & M64
    k ^= k >> 27
    k = (k * 0x94D049BB133111EB) & M64
    k ^= k >> 31
    return k


def key_py(barcode, fingerprint, w, n):
    a = mix((((fingerprint & 0xFFFFFFFF) << 8) | n) & M64)
    low = mix(w ^ a) & 0x00FFFFFFFFFFFFFF
    if low == 0:
        low = 1
    b = 0 if barcode == -1 else barcode & 0xFF
    return (b << 56) | low


def mol_py(g, seq, offs, res, labels, P):
    """The definition: entries [(key, count)] by count descending then key ascending, and the six totals."""
    is_r = [int(g["seg_type"][int(v) & 0xFFFF]) == ord("R") for v in g["label"]]
    tot = dict.fromkeys(tdlib.MOL_TOTALS, 0)
    counts = {}
    for i in range(len(offs) - 1):
        if int(res["read_type"][i]) & 0xFF != 0:
            continue
        tot["eligible"] += 1
        o, ln = int(offs[i]), int(offs[i + 1] - offs[i])
        lab = labels[o + i:o + i + ln + 1]
        bases = [int(seq[o + p]) for p in range(ln) if is_r[int(lab[p + 1])]][:P]
        if not bases:
            tot["skipped_empty"] += 1
        elif any(b > 3 for b in bases):
            tot["skipped_n"] += 1
        else:
            w = 0
            for b in bases:
                w = (w << 2) | b
            k = key_py(int(res["barcode"][i]), int(res["fingerprint"][i]), w, len(bases))
            counts[k] = counts.get(k, 0) + 1
            tot["counted"] += 1
    tot["molecules"] = len(counts)
    return sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])), tot


def summarise_py(pairs):
    rows = np.zeros(256, tdlib.MOL_ROW_DTYPE)
    for k, c in pairs:
        r = rows[k >> 56]
        r["reads"] += c
        r["molecules"] += 1
        r["levels"][min(c, 10) - 1] += 1
    return rows


def as_pairs(entries):
    return [(int(k), int(c)) for k, c in zip(entries["key"], entries["count"])]


def results_of(g):
    return {f: np.asarray(g[f]) for f in ("read_type", "barcode", "fingerprint")}


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("P", [1, 16, 20, 32])
def test_host_count_is_the_definition_on_the_reference_s_fixtures(name, P):
    g = load_golden(name)
    res = results_of(g)
    ent, tot = tdlib.mol_host(g, g["seq"], g["offs"], res, g["labels"], P)
    want, want_tot = mol_py(g, g["seq"], g["offs"], res, g["labels"], P)
    assert as_pairs(ent) == want, name
    assert tot == want_tot, name
    assert tot["eligible"] == tot["counted"] + tot["skipped_empty"] + tot["skipped_n"] + tot["overflow"] and tot["overflow"] == 0
    assert tot["counted"] == int(ent["count"].sum()) and tot["molecules"] == len(ent)
    assert tot["eligible"] == int(((res["read_type"] & 0xFF) == 0).sum()) > 0 and tot["counted"] > 0
    has_f = any(int(t) == ord("F") for t in g["seg_type"])
    assert bool((res["fingerprint"][(res["read_type"] & 0xFF) == 0] != -1).all()) == has_f
    assert all(k != 0 and tdlib.mol_key_bin(k) == k >> 56 for k, _ in want)


def test_the_key_function():
    rng = np.random.default_rng(5)
    for _ in range(300):
        n = int(rng.integers(1, 33))
        w = int(rng.integers(0, 1 << 62)) & ((1 << (2 * n)) - 1) if n < 32 else int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        fp = int(rng.integers(-(1 << 31), 1 << 31))
        bar = int(rng.integers(-1, 300))
        k = tdlib.mol_key(bar, fp, w, n)
        assert k == key_py(bar, fp, w, n) and k & 0x00FFFFFFFFFFFFFF != 0
        assert tdlib.mol_key_bin(k) == (0 if bar == -1 else bar & 0xFF)
    # the prefix length belongs to the key: "A" and "AA" are different molecules; so does the fingerprint, so does the barcode
    assert len({tdlib.mol_key(0, -1, 0, 1), tdlib.mol_key(0, -1, 0, 2), tdlib.mol_key(0, 0x1B04, 0, 1), tdlib.mol_key(1, -1, 0, 1)}) == 4
    assert tdlib.mol_key(-1, 7, 9, 4) == tdlib.mol_key(0, 7, 9, 4)       # no barcode segment: the writer's file 0


def test_summarise_against_python_with_ten_and_eleven_in_the_last_level():
    pairs = [((3 << 56) | 5, 10), ((3 << 56) | 6, 11), ((3 << 56) | 7, 9), ((3 << 56) | 8, 1), ((0 << 56) | 9, 1), ((255 << 56) | 1, 2),
             ((3 << 56) | 9, 1000000)]
    e = np.array(pairs, tdlib.CENSUS_ENTRY_DTYPE)
    rows = tdlib.mol_summarise(e)
    want = summarise_py(pairs)
    assert np.array_equal(rows, want)
    assert list(rows[3]["levels"]) == [1, 0, 0, 0, 0, 0, 0, 0, 1, 3] and rows[3]["reads"] == 1000031 and rows[3]["molecules"] == 5
    assert rows[255]["levels"][1] == 1 and rows[0]["molecules"] == 1
    assert not tdlib.mol_summarise(np.zeros(0, tdlib.CENSUS_ENTRY_DTYPE))["reads"].any()
    g = load_golden("c5_b96_f_r_p")
    ent, tot = tdlib.mol_host(g, g["seq"], g["offs"], results_of(g), g["labels"], 20)
    rows = tdlib.mol_summarise(ent)
    assert np.array_equal(rows, summarise_py(as_pairs(ent)))
    assert int(rows["reads"].sum()) == tot["counted"] and int(rows["molecules"].sum()) == tot["molecules"]
    assert int(rows["levels"].sum()) == tot["molecules"] and int((rows["reads"] > 0).sum()) > 1


def test_merge_of_two_halves_is_the_whole():
    g = load_golden("c5_b96_f_r_p")
    n = int(g["n_reads"])
    seq, offs, lab = g["seq"], np.asarray(g["offs"], np.int64), g["labels"]
    res = results_of(g)
    whole, tot = tdlib.mol_host(g, seq, offs, res, lab, 20)
    cut = n // 2 + 1
    a, ta = tdlib.mol_host(g, seq[:offs[cut]], offs[:cut + 1], {f: v[:cut] for f, v in res.items()}, lab[:offs[cut] + cut], 20)
    b, tb = tdlib.mol_host(g, seq[offs[cut]:], offs[cut:] - offs[cut], {f: v[cut:] for f, v in res.items()}, lab[offs[cut] + cut:], 20)
    merged = tdlib.census_merge(a, b)
    assert as_pairs(merged) == as_pairs(whole) and len(a) and len(b)
    assert all(ta[f] + tb[f] == tot[f] for f in tdlib.MOL_TOTALS if f != "molecules")
    assert np.array_equal(tdlib.mol_summarise(merged), tdlib.mol_summarise(whole))


def test_refusals():
    g = load_golden("umi_f_s_r")
    for bad in (0, 33, -1):
        with pytest.raises(TdError, match="prefix_bases"):
            tdlib.mol_host(g, g["seq"], g["offs"], results_of(g), g["labels"], bad)
    # log2_slots belongs to the device table: its range is written into td_mol_enable, which needs a context (tests/test_molecules_gpu.py)
    src = open(os.path.join(REPO, "tagdust_amd", "csrc", "td_molecules.hip")).read()
    assert "log2_slots < 4 || log2_slots > 30" in src


def test_one_table_implementation():
    """the census and the molecule count include the same device header; neither unit has a probe loop or a compaction of its own:
    both count through the header's one tail (kt_wave_add: kt_wave_merge, then kt_probe_add) and read their table through the
    shared unit's kt_table_entries; the key's arithmetic and the cursor pattern are each written once, and the host units are
    plain C++"""
    csrc = os.path.join(REPO, "tagdust_amd", "csrc")
    header = open(os.path.join(csrc, "td_keytable.h")).read()
    for unit in ("td_census.hip", "td_molecules.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert "atomicCAS" not in text and "kt_wave_add(" in text and "kt_table_entries(" in text
        assert "compact_kernel" not in text and not re.search(r"__global__[^;{]*compact", text)
    at = header.index("KtWaveAdded kt_wave_add(")
    tail = header[at:header.index("\n}\n", at)]
    assert "kt_wave_merge(" in tail and "kt_probe_add(" in tail
    assert header.count("atomicCAS") == 1 and "__global__" not in header
    assert open(os.path.join(csrc, "td_keytable.hip")).read().count("__global__") == 1
    # the key's arithmetic is written once, in the header both sides read; the cursor pattern once, in the device header; and the host
    # units with the header they include are plain C++
    shared, host_units = "td_count_key.h", ("td_census_host.cpp", "td_molecules_host.cpp")
    for unit in ("td_census.hip", "td_molecules.hip", "td_keytable.hip", "td_keytable.h") + host_units:
        text = open(os.path.join(csrc, unit)).read()
        assert not re.search(r"\b(kt_mix|mol_key)\s*\([^;{]*\)\s*\{", text), unit
        assert ("atomicAdd(cursor" in text) == (unit == "td_keytable.h"), unit
    text = open(os.path.join(csrc, shared)).read()
    assert len(re.findall(r"\bkt_mix\s*\([^;{]*\)\s*\{", text)) == 1 and len(re.findall(r"\bmol_key\s*\([^;{]*\)\s*\{", text)) == 1
    for unit in host_units + (shared,):
        text = open(os.path.join(csrc, unit)).read()
        assert "hip/" not in text and "__global__" not in text and "atomicAdd(cursor" not in text, unit
        assert not re.search(r'#include\s*"(td_ctx|td_device|td_keytable)\.h"', text), unit


def test_header_symbols_are_exported_and_bound(library):
    hdr = open(os.path.join(REPO, "include", "tagdust_molecules.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    found = set(re.findall(r"\b(td_[a-z_0-9]+)\s*\(", hdr))
    assert found == set(tdlib.MOL_ABI_SYMBOLS)
    for name in sorted(found) + ["td_fingerprint_text", "td_writer_set_fingerprint_text"]:
        assert hasattr(library, name), name


# ---- the run's options and plan ----
def _touch(d, name):
    p = os.path.join(str(d), name)
    open(p, "w").write("@r\nACGT\n+\nIIII\n")
    return p


def test_the_options_parse():
    o = tdlib.RunOpts(["in.fq"]).o
    assert (o.molecules, o.molecules_prefix, o.molecules_slots_log2, o.fingerprint_seq) == (0, 20, 26, 0)
    o = tdlib.RunOpts(["in.fq", "--molecules", "--molecules-prefix", "32", "--molecules-slots", "12", "--fingerprint-seq"]).o
    assert (o.molecules, o.molecules_prefix, o.molecules_slots_log2, o.fingerprint_seq) == (1, 32, 12, 1)
    assert (o.unknown_barcodes, o.unknown_slots_log2) == (0, 20)
    for own in ("-molecules", "-fingerprint-seq"):                       # own options take two dashes
        with pytest.raises(TdError, match="unknown option " + own):
            tdlib.RunOpts(["in.fq", own])
    with pytest.raises(TdError, match="requires an argument"):
        tdlib.RunOpts(["in.fq", "--molecules-prefix"])
    for bad in ("0", "33"):
        with pytest.raises(TdError, match="--molecules-prefix: need 1..32"):
            tdlib.RunOpts(["in.fq", "--molecules-prefix", bad])
    for bad in ("3", "31"):
        with pytest.raises(TdError, match="--molecules-slots: need 4..30"):
            tdlib.RunOpts(["in.fq", "--molecules-slots", bad])
    for spelling in ("-show_finger_seq", "--show_finger_seq"):           # the reference's spelling stays refused
        with pytest.raises(TdError, match="option " + spelling + " of the reference is not implemented"):
            tdlib.RunOpts(["in.fq", spelling])
    lib = tdlib.load_library()
    lib.td_run_usage.restype = C.c_char_p
    usage = lib.td_run_usage()
    assert b"--molecules " in usage and b"--molecules-prefix P" in usage and b"--molecules-slots N" in usage and b"--fingerprint-seq" in usage


def test_the_plan_with_and_without_the_option(tmp_path):
    fq = _touch(tmp_path, "in.fq")
    out = str(tmp_path / "o")
    base = ["-1", "B:ACGT,TTGA", "-2", "F:NNNN", "-3", "R:N", fq, "-o", out]
    without = tdlib.run_plan(base)
    with_opt = tdlib.run_plan(base + ["--molecules"])
    assert "molecules" not in without
    assert with_opt == without + "output file: " + out + "_molecules.txt\n"
    assert tdlib.run_plan(base + ["--fingerprint-seq"]) == without
    both = tdlib.run_plan(base + ["--molecules", "--unknown-barcodes", "5"])
    assert both == without + "output file: " + out + "_unknown_barcodes.txt\n" + "output file: " + out + "_molecules.txt\n"
    # the file joins the existing-output check
    open(out + "_molecules.txt", "w").write("old\n")
    assert tdlib.run_plan(base) == without
    with pytest.raises(TdError, match="already exists.*_molecules.txt"):
        tdlib.run_plan(base + ["--molecules"])
    assert tdlib.run_plan(base + ["--molecules", "--force"]) == with_opt
    # no barcode segment is fine: the file has the one row "-"
    nobar = ["-1", "F:NNNN", "-2", "R:N", fq, "-o", str(tmp_path / "p")]
    assert tdlib.run_plan(nobar + ["--molecules"]) == tdlib.run_plan(nobar) + "output file: " + str(tmp_path / "p") + "_molecules.txt\n"


def test_the_three_refusals_of_the_run(tmp_path):
    fq, fq2 = _touch(tmp_path, "in.fq"), _touch(tmp_path, "in2.fq")
    out = str(tmp_path / "o")
    base = ["-1", "B:ACGT,TTGA", "-2", "F:NNNN", "-3", "R:N", "-o", out, "--molecules"]
    with pytest.raises(TdError, match="--molecules needs exactly one input file"):
        tdlib.run_plan(base + [fq, fq2])
    for window in (["-start", "3"], ["-end", "30"], ["-start", "3", "-end", "30"]):
        with pytest.raises(TdError, match="--molecules cannot be combined with -start / -end"):
            tdlib.run_plan(base + [fq] + window)
    with pytest.raises(TdError, match="--molecules: the architecture is a single read segment"):
        tdlib.run_plan(["-1", "R:N", fq, "-o", out, "--molecules"])
    assert "_molecules.txt" in tdlib.run_plan(base + [fq])
