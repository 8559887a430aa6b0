"""Dedup -- one read per molecule (include/tagdust_molecules.h) -- on the host, no GPU: td_mol_dedup_host over the reference's own
labels, outcomes, barcodes, fingerprints and reads (tests/golden) against the definition restated here in plain Python (walk the
reads in order, a set of keys decides); the writer, which writes a duplicate to no file; the options of the whole-run driver, what
they add to the plan and where they are refused; the enable rule."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from conftest import REPO, load_golden
from tagdust_amd import TdError
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

M64 = (1 << 64) - 1
FIXTURES = ["umi_f_s_r", "r_s_b_f", "f_b_f_r", "c3_b6_s_r_p"]


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
    return ((0 if barcode == -1 else barcode & 0xFF) << 56) | (low or 1)


def dedup_py(g, seq, offs, res, labels, P):
    """The definition: (per read: its key, None when it is not counted; which reads are duplicates; kept, duplicates, unjudged;
    eligible, molecules, not counted)."""
    is_r = [int(g["seg_type"][int(v) & 0xFFFF]) == ord("R") for v in g["label"]]
    n = len(offs) - 1
    keys, dup = [None] * n, np.zeros(n, bool)
    seen = set()
    tot = {"kept": 0, "duplicates": 0, "unjudged": 0}
    eligible = 0
    for i in range(n):
        if int(res["read_type"][i]) & 0xFF != 0:
            continue
        eligible += 1
        o, ln = int(offs[i]), int(offs[i + 1] - offs[i])
        lab = labels[o + i:o + i + ln + 1]
        bases = [int(seq[o + p]) for p in range(ln) if is_r[int(lab[p + 1])]][:P]
        if not bases or any(b > 3 for b in bases):
            tot["unjudged"] += 1
            tot["kept"] += 1
            continue
        w = 0
        for b in bases:
            w = (w << 2) | b
        k = key_py(int(res["barcode"][i]), int(res["fingerprint"][i]), w, len(bases))
        keys[i] = k
        if k in seen:
            dup[i] = True
            tot["duplicates"] += 1
        else:
            seen.add(k)
            tot["kept"] += 1
    return keys, dup, tot, eligible, len(seen)


def results_of(g):
    return {f: np.asarray(g[f]) for f in ("read_type", "barcode", "fingerprint")}


def reversed_batch(g):
    """the same reads, the last one first: (seq, offs, res, labels)"""
    offs = np.asarray(g["offs"], np.int64)
    n = len(offs) - 1
    order = range(n - 1, -1, -1)
    seq = np.concatenate([g["seq"][offs[i]:offs[i + 1]] for i in order]).astype(np.uint8)
    lab = np.concatenate([g["labels"][offs[i] + i:offs[i + 1] + i + 1] for i in order]).astype(np.int8)
    roffs = np.zeros(n + 1, np.int64)
    roffs[1:] = np.cumsum(np.diff(offs)[::-1])
    return seq, roffs, {f: v[::-1].copy() for f, v in results_of(g).items()}, lab


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("P", [1, 16, 32])
def test_host_decision_is_the_definition_on_the_reference_s_fixtures(name, P):
    g = load_golden(name)
    res = results_of(g)
    dup, tot = tdlib.mol_dedup_host(g, g["seq"], g["offs"], res, g["labels"], P)
    keys, want, want_tot, eligible, molecules = dedup_py(g, g["seq"], g["offs"], res, g["labels"], P)
    assert np.array_equal(dup, want) and tot == want_tot, name
    # the identities, with the count's own totals
    _, mt = tdlib.mol_host(g, g["seq"], g["offs"], res, g["labels"], P)
    assert mt["eligible"] == eligible == tot["kept"] + tot["duplicates"] > 0
    assert tot["kept"] == mt["molecules"] + mt["skipped_empty"] + mt["skipped_n"] + mt["overflow"] and mt["molecules"] == molecules
    assert tot["unjudged"] == mt["skipped_empty"] + mt["skipped_n"] and mt["overflow"] == 0
    assert not dup[(res["read_type"] & 0xFF) != 0].any()
    # reversed, the other end of every molecule stays: the last read of a key in the given order
    n = len(keys)
    rseq, roffs, rres, rlab = reversed_batch(g)
    rdup, rtot = tdlib.mol_dedup_host(g, rseq, roffs, rres, rlab, P)
    assert rtot == tot
    last = {}
    for i, k in enumerate(keys):
        if k is not None:
            last[k] = i
    want_back = np.array([k is not None and last[k] != i for i, k in enumerate(keys)])
    assert np.array_equal(rdup[::-1], want_back)
    if name == "c3_b6_s_r_p" and P == 1:                  # (no UMI, a prefix of one base: a few molecules of many reads each)
        assert tot["duplicates"] > 0 and not np.array_equal(want_back, want)


def _fastq(names, g, keep):
    offs = g["offs"]
    alpha = np.frombuffer(b"ACGTN", np.uint8)
    return b"".join(b"@" + names[i] + b"\n" + bytes(alpha[g["seq"][offs[i]:offs[i + 1]]]) + b"\n+\n" + bytes(g["qual"][offs[i]:offs[i + 1]]) + b"\n"
                    for i in keep)


def _files(prefix):
    return {os.path.basename(f)[len(os.path.basename(prefix)):]: open(f, "rb").read() for f in glob.glob(prefix + "*")}


def test_the_writer_writes_a_duplicate_to_no_file(tmp_path):
    from oracle import pyoracle
    from test_io import segments_of
    g = load_golden("c3_b6_s_r_p")
    n = int(g["n_reads"])
    names = bytes(g["names"]).split(b"\n")
    pr = tdlib.ParsedReads(_fastq(names, g, range(n)), 2)
    ores, _, oseq = pyoracle.label_batch(pyoracle.OracleModel(g), pr.codes, pr.offs, float(g["threshold"]), int(g["minlen"]), int(g["dust"]), 2)
    res = np.zeros(n, tdlib.RESULT_DTYPE)
    for k in ("f_score", "b_score", "r_score", "bar_prob", "read_type", "barcode", "fingerprint"):
        res[k] = ores[k]
    res["mapq"] = ores["Q"]
    ok = np.flatnonzero(res["read_type"] == 0)
    assert len(ok) > 10 and len(ok) < n                   # some reads fail: the _un file is not empty
    marked = [int(ok[0]), int(ok[len(ok) // 2]), int(ok[-1])]
    segs = segments_of(g)
    tdlib.write_demultiplexed(str(tmp_path / "plain"), segs, pr, res, oseq)
    plain = _files(str(tmp_path / "plain"))
    for i in marked:                                      # as decoded, each of them is in a barcode file
        assert sum(v.count(b"@" + names[i] + b";") for k, v in plain.items() if "_un" not in k) == 1
    dres = res.copy()
    dres["read_type"][marked] = tdlib.EXTRACT_DUPLICATE
    tdlib.write_demultiplexed(str(tmp_path / "dup"), segs, pr, dres, oseq)
    # the same batch with those records taken out
    keep = [i for i in range(n) if i not in marked]
    pr2 = tdlib.ParsedReads(_fastq(names, g, keep), 2)
    offs = np.asarray(pr.offs)
    seq2 = np.concatenate([oseq[offs[i]:offs[i + 1]] for i in keep]).astype(np.uint8)
    tdlib.write_demultiplexed(str(tmp_path / "removed"), segs, pr2, res[keep], seq2)
    dup, removed = _files(str(tmp_path / "dup")), _files(str(tmp_path / "removed"))
    assert set(dup) == set(removed) == set(plain) and any("_un" in k for k in dup)
    for k in dup:
        assert dup[k] == removed[k], k
        for i in marked:
            assert b"@" + names[i] + b";" not in dup[k], k
    un = [k for k in dup if "_un" in k]
    assert all(dup[k] == plain[k] for k in un) and any(len(dup[k]) for k in un)
    assert sum(len(v) for v in dup.values()) < sum(len(v) for v in plain.values())


def _touch(d, name):
    p = os.path.join(str(d), name)
    open(p, "w").write("@r\nACGT\n+\nIIII\n")
    return p


def test_the_option_the_plan_and_the_refusals(tmp_path):
    def parsed(args):
        ro = tdlib.RunOpts(args)                          # (.o is the library's structure: read it while ro holds it)
        try:
            return ro.o.dedup, ro.o.molecules, ro.o.molecules_prefix, ro.o.molecules_slots_log2
        finally:
            ro.close()

    assert parsed(["in.fq"]) == (0, 0, 20, 26)
    assert parsed(["in.fq", "--molecules"]) == (0, 1, 20, 26)
    assert parsed(["in.fq", "--dedup"]) == (1, 1, 20, 26)  # alone, it turns the count on
    with pytest.raises(TdError, match="unknown option -dedup"):   # own options take two dashes
        tdlib.RunOpts(["in.fq", "-dedup"])
    lib = tdlib.load_library()
    lib.td_run_usage.restype = C.c_char_p
    assert b"--dedup " in lib.td_run_usage()
    fq, fq2 = _touch(tmp_path, "in.fq"), _touch(tmp_path, "in2.fq")
    out = str(tmp_path / "o")
    base = ["-1", "B:ACGT,TTGA", "-2", "F:NNNN", "-3", "R:N", "-o", out]
    with_mol = tdlib.run_plan(base + [fq, "--molecules"])
    with_dedup = tdlib.run_plan(base + [fq, "--dedup"])
    assert "dedup" not in with_mol
    line = [l for l in with_dedup.splitlines() if l.startswith("dedup: ")]
    assert len(line) == 1 and "one read per molecule" in line[0]
    assert with_dedup.replace(line[0] + "\n", "") == with_mol            # ... and the molecules file is an output file
    assert "output file: " + out + "_molecules.txt\n" in with_dedup
    assert tdlib.run_plan(base + [fq, "--dedup", "--molecules"]) == with_dedup
    with pytest.raises(TdError, match="--dedup needs exactly one device.*survive twice"):
        tdlib.run_plan(base + [fq, "--dedup", "--devices", "0,1"])
    assert tdlib.run_plan(base + [fq, "--molecules", "--devices", "0,1"])   # (the count alone merges its devices)
    with pytest.raises(TdError, match="needs exactly one input file"):
        tdlib.run_plan(base + [fq, fq2, "--dedup"])
    for window in (["-start", "3"], ["-end", "30"]):
        with pytest.raises(TdError, match="cannot be combined with -start / -end"):
            tdlib.run_plan(base + [fq, "--dedup"] + window)
    with pytest.raises(TdError, match="the architecture is a single read segment"):
        tdlib.run_plan(["-1", "R:N", fq, "-o", out, "--dedup"])


def test_enable_needs_the_count():
    """td_mol_dedup_enable fails with a message unless td_mol_enable came first.  A context needs a device, so here: the call
    without one fails with a message, and the refusal is in the source (tests/test_dedup_gpu.py runs into it)."""
    src = open(os.path.join(REPO, "tagdust_amd", "csrc", "td_molecules.hip")).read()
    at = src.index('extern "C" int td_mol_dedup_enable(')
    body = src[at:src.index("\n}\n", at)]
    assert 'if (!z.on) return fail(c, "td_mol_dedup_enable: the molecule count is off (td_mol_enable first)' in body
    assert 'if (tickets_outstanding(c)) return fail(c, "td_mol_dedup_enable: td_submit tickets are outstanding' in body
    lib = tdlib._mol_lib()
    assert lib.td_mol_dedup_enable(None) != 0
    assert b"td_mol_dedup_enable" in lib.td_last_error(None)
