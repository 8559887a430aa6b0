"""The mate filter (include/tagdust_molecules.h, td_mol_mate_filter_enable) on the host, no GPU.  The filter needs no host function
of its own: its definition is the join  read_type[i] = max(read_type[i] as decoded, t2[i])  followed by the four *_mated host
functions on the joined records.  Here that is restated in plain Python over the reference's own labels and records (tests/golden)
with mate types drawn by hand, the case the filter exists for is pinned, and the run's option, plan line and refusals are checked,
with the unit's source."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import REPO, load_golden
from tagdust_amd import TdError
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib
from test_dedup_collapsed import check_identities as check_frozen_identities
from test_dedup_collapsed import replay_py
from test_mate import FIXTURES, as_origins, as_pairs, classify_mated, count_py, dedup_py, mates_for, repeated

PM = [(12, 20), (8, 8), (1, 31)]


@pytest.fixture(scope="module", autouse=True)
def library():
    tdbuild.build()
    return tdlib.load_library()


def draw_types(n, seed, n_art=5):
    """mate types drawn by hand: 0 for three in five, DUST's 6, and (1-based sequence << 8) | 5 for sequences 1..n_art"""
    rng = np.random.default_rng(seed)
    what = rng.random(n)
    t2 = np.zeros(n, np.int32)
    t2[what < 0.2] = 6
    hit = what >= 0.8
    t2[hit] = (rng.integers(1, n_art + 1, int(hit.sum())).astype(np.int32) << 8) | 5
    return t2


def joined(res, t2):
    """the join: whole signed words, the reference's HMMER3_MAX (src/barcode_hmm.c:344-350); every other field as decoded"""
    out = dict(res)
    out["read_type"] = np.array([max(int(a), int(b)) for a, b in zip(res["read_type"], t2)], np.asarray(res["read_type"]).dtype)
    return out


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("P,M", PM, ids=["P%d-M%d" % pm for pm in PM])
def test_the_join_then_the_mated_host_functions_is_the_definition(name, P, M):
    g = load_golden(name)
    seq, offs, res, labels, source = repeated(g, seed=11)
    n = len(offs) - 1
    mc, mo, _ = mates_for(n, M, seed=7 + M, source=source)
    mate = (mc, mo, M)
    t2 = draw_types(n, seed=3 + P)
    assert {0, 6} <= set(t2.tolist()) and any((int(t) & 0xFF) == 5 and int(t) >> 8 >= 1 for t in t2)
    jres = joined(res, t2)
    # the join itself: never below either side, 261 = (1 << 8) | 5 beats DUST's 6, the other fields stay
    own = np.asarray(res["read_type"])
    assert (jres["read_type"] >= own).all() and (jres["read_type"] >= t2).all()
    assert all(int(j) in (int(a), int(b)) for j, a, b in zip(jres["read_type"], own, t2))
    assert max(6, (1 << 8) | 5) == 261
    assert jres["barcode"] is res["barcode"] and jres["fingerprint"] is res["fingerprint"]
    was = (own & 0xFF) == 0
    now = (jres["read_type"] & 0xFF) == 0
    assert np.array_equal(now, was & (t2 == 0)) and 0 < int(now.sum()) < int(was.sum())
    # the four host functions on joined records against the restated definition on joined records
    classes = classify_mated(g, seq, offs, jres, labels, P, mate)
    want, want_origin, want_tot = count_py(classes)
    ent, tot = tdlib.mol_host_mated(g, seq, offs, jres, labels, mate, P)
    assert as_pairs(ent) == want and tot == want_tot
    ent2, org, tot2 = tdlib.mol_host_origins_mated(g, seq, offs, jres, labels, mate, P)
    assert as_pairs(ent2) == want and tot2 == want_tot and as_origins(ent2, org) == want_origin
    assert tot["eligible"] == int(now.sum()) == tot["counted"] + tot["skipped_empty"] + tot["skipped_n"] + tot["overflow"]
    assert tot["counted"] == int(ent["count"].sum()) and tot["molecules"] == len(ent)
    dup, dtot = tdlib.mol_dedup_host_mated(g, seq, offs, jres, labels, mate, P)
    want_dup, want_dtot = dedup_py(classes)
    assert np.array_equal(dup, want_dup) and dtot == want_dtot
    assert tot["eligible"] == dtot["kept"] + dtot["duplicates"]
    assert dtot["kept"] == tot["molecules"] + tot["skipped_empty"] + tot["skipped_n"]
    assert not dup[~now].any()                                  # a read whose mate failed is no duplicate: it is not judged at all
    cdup, ctot, coll = tdlib.mol_dedup_collapsed_host_mated(g, seq, offs, jres, labels, mate, P)
    want_cdup, want_ctot, want_coll = replay_py(classes)
    assert np.array_equal(cdup, want_cdup) and ctot == want_ctot and {k: coll[k] for k in want_coll} == want_coll
    check_frozen_identities(classes, ctot, coll)
    # every t2 zero: bit for bit the unjoined result
    zres = joined(res, np.zeros(n, np.int32))
    assert np.array_equal(zres["read_type"], own)
    a, ta = tdlib.mol_host_mated(g, seq, offs, zres, labels, mate, P)
    b, tb = tdlib.mol_host_mated(g, seq, offs, res, labels, mate, P)
    assert as_pairs(a) == as_pairs(b) and ta == tb


@pytest.mark.parametrize("name", FIXTURES)
def test_a_molecule_whose_first_read_has_a_failing_mate_keeps_a_later_read(name):
    """The case the filter exists for.  Judged with the join in front, the molecule's later read with a passing mate is kept; judged
    without it and combined behind the count, as the run did before, the molecule leaves the output altogether."""
    P, M = 12, 20
    g = load_golden(name)
    seq, offs, res, labels, source = repeated(g, seed=11)
    n = len(offs) - 1
    mc, mo, _ = mates_for(n, M, seed=7 + M, source=source)
    mate = (mc, mo, M)
    plain = classify_mated(g, seq, offs, res, labels, P, mate)
    first, pairs_ij = {}, []
    for i, c in enumerate(plain):                               # (i, j): the first two reads of a molecule
        if isinstance(c, tuple):
            if c[0] not in first:
                first[c[0]] = [i]
            elif len(first[c[0]]) == 1:
                first[c[0]].append(i)
                pairs_ij.append(tuple(first[c[0]]))
    assert len(pairs_ij) >= 10, len(pairs_ij)
    t2 = np.zeros(n, np.int32)
    for i, _ in pairs_ij[::2]:
        t2[i] = 6                                               # the first read's mate fails DUST
    for i, _ in pairs_ij[1::2]:
        t2[i] = (2 << 8) | 5                                    # ... or matches the second artifact sequence
    jres = joined(res, t2)
    # on the yardstick's inputs first: the failing mates are those of first reads, their molecules' second reads pass
    assert all(t2[i] != 0 and t2[j] == 0 and i < j for i, j in pairs_ij)
    dup_j = tdlib.mol_dedup_host_mated(g, seq, offs, jres, labels, mate, P)[0]
    kept_j = ((jres["read_type"] & 0xFF) == 0) & ~dup_j
    assert all(kept_j[j] and not kept_j[i] for i, j in pairs_ij)                   # the later read is the molecule's one kept read
    # judged without the join the first read is the keeper and the later one a duplicate ...
    dup_p = tdlib.mol_dedup_host_mated(g, seq, offs, res, labels, mate, P)[0]
    assert all(dup_p[j] and not dup_p[i] for i, j in pairs_ij)
    # ... and the combination behind the count then sends the keeper to _un: no read of the molecule is written
    written_p = ((jres["read_type"] & 0xFF) == 0) & ~dup_p
    keys = {plain[i][0] for i, _ in pairs_ij}
    assert not any(written_p[k] for k, c in enumerate(plain) if isinstance(c, tuple) and c[0] in keys and k in {x for p in pairs_ij for x in p})
    assert int(kept_j.sum()) >= int(written_p.sum()) + len(pairs_ij)


# ---- the header, the mirror, the unit's source ----
def test_header_symbols_and_the_mirror(library):
    hdr = open(os.path.join(REPO, "include", "tagdust_molecules.h")).read()
    for name in ("td_mol_mate_filter_enable", "td_mol_mate_filter_disable", "td_mol_mate_types"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in tdlib.MOL_ABI_SYMBOLS and hasattr(library, name), name
    assert "int td_mol_mate_next   (td_ctx* ctx, const uint8_t* codes, const int64_t* offs, int64_t n_reads);" in hdr
    assert "typedef struct td_mol_mate { const uint8_t* codes; const int64_t* offs; int32_t bases; } td_mol_mate;" in hdr
    assert "td_counts_get does not" in hdr and "the yardstick of the device path" in hdr
    for m in ("mol_mate_filter_enable", "mol_mate_filter_disable", "mol_mate_types"):
        assert hasattr(tdlib.TagdustHip, m)
    assert tdlib._RunOptsMate._fields_[-2:] == [("mate_bases", C.c_int32), ("mate_filter", C.c_int32)]


def test_the_filter_unit_shares_the_arithmetic_of_the_rna_dust_kernel():
    csrc = os.path.join(REPO, "tagdust_amd", "csrc")
    unit = open(os.path.join(csrc, "td_mate_filter.hip")).read()
    rna = open(os.path.join(csrc, "td_rnadust.hip")).read()
    inner = open(os.path.join(csrc, "td_rnadust_inner.h")).read()
    code = lambda text: "\n".join(l.split("//")[0] for l in text.splitlines())
    for text in (unit, rna):
        assert '#include "td_rnadust_inner.h"' in text
        # no Myers column, text scan, best-hit rule or DUST body of its own: they are called, never defined
        for name in ("rd_step", "rd_step_chk", "rd_scan_text", "rd_best", "rd_build_masks", "rd_match", "rd_dust_low"):
            assert not re.search(r"\b(void|int|bool)\s+%s\s*\(" % name, code(text)), name
        assert "VP + (X & VP)" not in code(text)
        assert "rd_match(" in code(text) and "rd_dust_low(" in code(text)
    for name in ("rd_step", "rd_step_chk", "rd_scan_text", "rd_best", "rd_build_masks", "rd_match", "rd_dust_low"):
        assert len(re.findall(r"\b(?:void|int|bool)\s+%s\s*\(" % name, code(inner))) == 1, name
    from tagdust_amd import build
    assert "td_mate_filter.hip" in build.SOURCES and "td_rnadust_inner.h" in build.HEADERS and "td_mate_filter.h" in build.HEADERS
    assert "LDS per workgroup" in unit


# ---- the run's option, plan and refusals ----
def _touch(d, name):
    p = os.path.join(str(d), name)
    open(p, "w").write("@r\nACGT\n+\nIIII\n")
    return p


def test_the_option_parses():
    off = tdlib.RunOpts(["a.fq", "b.fq", "--mate-bases", "20"])
    assert off.o.mate_filter == 0
    on = tdlib.RunOpts(["a.fq", "b.fq", "--mate-bases", "20", "--mate-filter"])     # (kept alive: .o points into it)
    assert (on.o.mate_bases, on.o.mate_filter, on.o.molecules, on.o.dust) == (20, 1, 1, 100)
    with pytest.raises(TdError, match="unknown option -mate-filter"):
        tdlib.RunOpts(["a.fq", "-mate-filter"])
    lib = tdlib.load_library()
    lib.td_run_usage.restype = C.c_char_p
    assert b"--mate-filter" in lib.td_run_usage() and b"--mate-bases M" in lib.td_run_usage()


def test_the_plan_line_and_every_refusal(tmp_path):
    fq1, fq2, fq3 = _touch(tmp_path, "r1.fq"), _touch(tmp_path, "r2.fq"), _touch(tmp_path, "r3.fq")
    out = str(tmp_path / "o")
    segs = ["-1", "B:ACGT,TTGA", "-2", "F:NNNN", "-3", "R:N"]
    base = segs + ["-o", out, "--molecules-prefix", "12"]
    ref = os.path.join(str(tmp_path), "ref.fa")
    open(ref, "w").write(">a\nACGTACGTACGTACGTACGT\n")
    mate = ["--mate-bases", "20"]
    # without --mate-filter the refusal stands, with it the default DUST of 100 and a -ref file are accepted for two files
    with pytest.raises(TdError, match="run with -dust 0 and without -ref"):
        tdlib.run_plan(base + [fq1, fq2] + mate)
    plan = tdlib.run_plan(base + [fq1, fq2] + mate + ["--mate-filter"])
    line = [l for l in plan.splitlines() if l.startswith("mate: ")]
    assert len(line) == 1 and "mate filter on" in line[0] and "dust 100" in line[0] and "-ref none" in line[0]
    assert "takes no part" not in line[0] and "file 0 is decoded, file 1 is its mate" in line[0]
    assert "dust: 100\n" in plan and "ref: off\n" in plan
    plan = tdlib.run_plan(base + [fq1, fq2, "-ref", ref, "-dust", "50", "--dedup"] + mate + ["--mate-filter"])
    line = [l for l in plan.splitlines() if l.startswith("mate: ")][0]
    assert "dust 50" in line and "-ref " + ref in line and "ref: on\n" in plan
    off = tdlib.run_plan(base + [fq1, fq2, "-dust", "0"] + mate)
    assert "takes no part" in off and "mate filter" not in off
    on0 = tdlib.run_plan(base + [fq1, fq2, "-dust", "0"] + mate + ["--mate-filter"])
    assert [l for l in on0.splitlines() if not l.startswith("mate: ")] == [l for l in off.splitlines() if not l.startswith("mate: ")]
    # the refusals
    with pytest.raises(TdError, match="--mate-filter needs --mate-bases"):
        tdlib.run_plan(segs + ["-o", out, fq1, "--mate-filter"])
    with pytest.raises(TdError, match=r"--mate-filter with DUST or -ref takes exactly two input files \(3 given\): the outcome of .*r3\.fq"):
        tdlib.run_plan(base + [fq1, fq2, fq3] + mate + ["--mate-filter"])
    with pytest.raises(TdError, match=r"--mate-filter with DUST or -ref takes exactly two input files \(3 given\): the outcome of .*r3\.fq"):
        tdlib.run_plan(base + [fq1, fq2, fq3, "-dust", "0", "-ref", ref] + mate + ["--mate-filter"])
    assert "mate filter on" in tdlib.run_plan(base + [fq1, fq2, fq3, "-dust", "0"] + mate + ["--mate-filter"])     # nothing can fail: three are fine
    with pytest.raises(TdError, match="--mate-bases.*one device"):
        tdlib.run_plan(base + [fq1, fq2, "--devices", "0,0"] + mate + ["--mate-filter"])
    with pytest.raises(TdError, match="--mate-bases.*--dedup-collapsed.*the survey reads one file"):
        tdlib.run_plan(base + [fq1, fq2, "--dedup-collapsed"] + mate + ["--mate-filter"])
    with pytest.raises(TdError, match="--mate-bases: exactly one input file may have an architecture other than R:N"):
        tdlib.run_plan(["-1", "R:N", "-o", out, "--molecules-prefix", "12", fq1, fq2] + mate + ["--mate-filter"])
