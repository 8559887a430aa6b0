"""Mate mode of the molecule count (include/tagdust_molecules.h) on the host, no GPU: the four *_mated host functions over the
reference's own labels and records (tests/golden) against the definition restated here in plain Python, key function included;
mate == NULL against the unmated functions; the identities; the refusals; the run's option, its plan line and its refusals.

Mates come from a seeded pool, their lengths 0..50 and independent of the reads': shorter than M, empty, an N inside the first M
bases, and an N exactly at base M, where it must not matter."""
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

M64 = (1 << 64) - 1
FIXTURES = ["umi_f_s_r", "c3_b6_s_r_p", "b_f"]
PM = [(1, 31), (12, 20), (8, 8), (20, 1), (16, 16)]


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


def results_of(g):
    return {f: np.asarray(g[f]) for f in ("read_type", "barcode", "fingerprint")}


def mates_for(n, M, seed, pool=40, source=None):
    """n mates drawn from a pool of `pool` sequences of 0..50 bases: one in eight empty, one in eight shorter than M, one in eight
    with an N inside the first M bases, one in eight with an N exactly at base M (the first base behind the prefix).  source
    (None: every mate is drawn freely): read j is a copy of read source[j], and all copies of a read share two alternative mates.
    Returns (codes, offs, the kinds drawn)."""
    rng = np.random.default_rng(seed)
    seqs, kinds = [], []
    for q in range(pool):
        kind = ("empty", "short", "n_inside", "n_at_M")[q % 8] if q % 8 < 4 else "plain"
        if kind == "empty":
            s = np.zeros(0, np.uint8)
        elif kind == "short":
            s = rng.integers(0, 4, int(rng.integers(1, M)) if M > 1 else 0, dtype=np.uint8)
        else:
            s = rng.integers(0, 4, int(rng.integers(M + 1, 51)), dtype=np.uint8)
        if kind == "n_inside":
            s[int(rng.integers(0, M))] = 4 + int(rng.integers(0, 3)) * 60      # (any byte above 3 is an N)
        if kind == "n_at_M":
            s[M] = 4
        seqs.append(s)
        kinds.append(kind)
    pick = rng.integers(0, pool, n)
    if source is not None:
        pick = (np.asarray(source) * 7 + rng.integers(0, 2, n)) % pool
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(seqs[p]) for p in pick])
    codes = np.concatenate([seqs[p] for p in pick] + [np.zeros(0, np.uint8)]).astype(np.uint8)
    return codes, offs, [kinds[p] for p in pick]


def repeated(g, seed):
    """(seq, offs, res, labels, source) of twice as many reads as the fixture has, drawn from it with replacement: the fixtures'
    own reads are nearly all molecules of their own, copies give dedup and the collapse something to find"""
    rng = np.random.default_rng(seed)
    offs0, lab0, res0 = np.asarray(g["offs"], np.int64), np.asarray(g["labels"]), results_of(g)
    n0 = len(offs0) - 1
    source = rng.integers(0, n0, 2 * n0)
    offs = np.zeros(len(source) + 1, np.int64)
    offs[1:] = np.cumsum(np.diff(offs0)[source])
    seq = np.concatenate([g["seq"][offs0[i]:offs0[i + 1]] for i in source])
    lab = np.concatenate([lab0[offs0[i] + i:offs0[i + 1] + i + 1] for i in source])
    return seq, offs, {f: v[source] for f, v in res0.items()}, lab, source


def classify_mated(md, seq, offs, res, labels, P, mate):
    """The definition.  What every read is to the count: None (not eligible), "empty", "n", or (key, (w, fingerprint, n)); mate:
    None or (codes, offs, M)."""
    is_r = [int(md["seg_type"][int(v) & 0xFFFF]) == ord("R") for v in md["label"]]
    out = []
    for i in range(len(offs) - 1):
        if int(res["read_type"][i]) & 0xFF != 0:
            out.append(None)
            continue
        o, ln = int(offs[i]), int(offs[i + 1] - offs[i])
        lab = labels[o + i:o + i + ln + 1]
        bases = [int(seq[o + p]) for p in range(ln) if 0 <= int(lab[p + 1]) < len(is_r) and is_r[int(lab[p + 1])]][:P]
        if mate is not None:
            mc, mo, M = mate
            bases += [int(b) for b in mc[int(mo[i]):int(mo[i + 1])][:M]]
        if not bases:
            out.append("empty")
        elif any(b > 3 for b in bases):
            out.append("n")
        else:
            w = 0
            for b in bases:
                w = (w << 2) | b
            fp = int(res["fingerprint"][i])
            out.append((key_py(int(res["barcode"][i]), fp, w, len(bases)), (w, fp, len(bases))))
    return out


def count_py(classes):
    """entries [(key, count)] in the order of td_census_get, {key: origin}, the six totals"""
    tot = dict.fromkeys(tdlib.MOL_TOTALS, 0)
    counts, origin = {}, {}
    for c in classes:
        if c is None:
            continue
        tot["eligible"] += 1
        if c == "empty":
            tot["skipped_empty"] += 1
        elif c == "n":
            tot["skipped_n"] += 1
        else:
            counts[c[0]] = counts.get(c[0], 0) + 1
            origin.setdefault(c[0], c[1])
            tot["counted"] += 1
    tot["molecules"] = len(counts)
    return sorted(counts.items(), key=lambda kv: (-kv[1], kv[0])), origin, tot


def dedup_py(classes):
    dup = np.zeros(len(classes), bool)
    tot = dict.fromkeys(tdlib.MOL_DEDUP_TOTALS, 0)
    seen = set()
    for i, c in enumerate(classes):
        if c is None:
            continue
        if not isinstance(c, tuple):
            tot["unjudged"] += 1
            tot["kept"] += 1
        elif c[0] in seen:
            dup[i] = True
            tot["duplicates"] += 1
        else:
            seen.add(c[0])
            tot["kept"] += 1
    return dup, tot


def as_pairs(entries):
    return [(int(k), int(c)) for k, c in zip(entries["key"], entries["count"])]


def as_origins(entries, origins):
    return {int(k): (int(o["w"]), int(o["fingerprint"]), int(o["n"])) for k, o in zip(entries["key"], origins)}


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("P,M", PM, ids=["P%d-M%d" % pm for pm in PM])
def test_the_four_mated_host_functions_are_the_definition(name, P, M):
    g = load_golden(name)
    seq, offs, res, labels, source = repeated(g, seed=11)
    n = len(offs) - 1
    mc, mo, kinds = mates_for(n, M, seed=7 + M, source=source)
    mate = (mc, mo, M)
    assert {"empty", "n_inside", "n_at_M", "plain"} <= set(kinds) and (M == 1 or "short" in kinds)
    assert int(np.diff(mo).min()) == 0 and int(np.diff(mo).max()) > M
    classes = classify_mated(g, seq, offs, res, labels, P, mate)
    want, want_origin, want_tot = count_py(classes)
    # the count, with and without origins
    ent, tot = tdlib.mol_host_mated(g, seq, offs, res, labels, mate, P)
    assert as_pairs(ent) == want and tot == want_tot, name
    ent2, org, tot2 = tdlib.mol_host_origins_mated(g, seq, offs, res, labels, mate, P)
    assert as_pairs(ent2) == want and tot2 == want_tot and as_origins(ent2, org) == want_origin
    assert all(tdlib.mol_key(int(res["barcode"][i]), c[1][1], c[1][0], c[1][2]) == c[0] for i, c in enumerate(classes) if isinstance(c, tuple))
    # the identities of the count
    assert tot["eligible"] == tot["counted"] + tot["skipped_empty"] + tot["skipped_n"] + tot["overflow"] and tot["overflow"] == 0
    assert tot["counted"] == int(ent["count"].sum()) > 0 and tot["molecules"] == len(ent)
    assert tot["eligible"] == int(((res["read_type"] & 0xFF) == 0).sum())
    # every kind of mate is met by an eligible read, and does what the definition says
    ok = [i for i in range(n) if classes[i] is not None]
    assert tot["skipped_n"] >= sum(kinds[i] == "n_inside" for i in ok) > 0
    assert sum(kinds[i] == "n_at_M" and isinstance(classes[i], tuple) for i in ok) > 0
    assert max(c[1][2] for c in classes if isinstance(c, tuple)) <= P + M <= 32
    assert np.array_equal(tdlib.mol_summarise(ent)["reads"].sum(), tot["counted"])
    # dedup and its identities
    dup, dtot = tdlib.mol_dedup_host_mated(g, seq, offs, res, labels, mate, P)
    want_dup, want_dtot = dedup_py(classes)
    assert np.array_equal(dup, want_dup) and dtot == want_dtot
    assert tot["eligible"] == dtot["kept"] + dtot["duplicates"]
    assert dtot["kept"] == tot["molecules"] + tot["skipped_empty"] + tot["skipped_n"] and dtot["duplicates"] > 0
    # survey, freeze, replay and the identities of the frozen state
    cdup, ctot, coll = tdlib.mol_dedup_collapsed_host_mated(g, seq, offs, res, labels, mate, P)
    want_cdup, want_ctot, want_coll = replay_py(classes)
    assert np.array_equal(cdup, want_cdup) and ctot == want_ctot and {k: coll[k] for k in want_coll} == want_coll
    check_frozen_identities(classes, ctot, coll)


def test_b_f_has_no_read_segment_unmated_everything_is_empty_mated_it_is_counted():
    g = load_golden("b_f")
    res = results_of(g)
    assert not any(int(t) == ord("R") for t in g["seg_type"])
    _, tot = tdlib.mol_host(g, g["seq"], g["offs"], res, g["labels"], 12)
    assert tot["eligible"] == tot["skipped_empty"] > 100 and tot["counted"] == 0
    rng = np.random.default_rng(3)
    n = len(g["offs"]) - 1
    mo = np.arange(n + 1, dtype=np.int64) * 30
    mc = rng.integers(0, 4, 30 * n, dtype=np.uint8)
    ent, mtot = tdlib.mol_host_mated(g, g["seq"], g["offs"], res, g["labels"], (mc, mo, 20), 12)
    assert mtot["eligible"] == tot["eligible"] == mtot["counted"] == mtot["molecules"] and mtot["skipped_empty"] == 0
    assert as_pairs(ent) == count_py(classify_mated(g, g["seq"], g["offs"], res, g["labels"], 12, (mc, mo, 20)))[0]


def test_the_split_between_own_and_mate_bases_is_not_in_the_key():
    """the limit the header states: own ACG + mate T and own AC + mate GT share a word -- and the word is (w1 << 2 * n2) | w2"""
    from test_dedup_collapsed import Synthetic
    syn = Synthetic()
    a = syn.read(3, 0x1B04, 0b000110, 3)            # own ACG
    b = syn.read(3, 0x1B04, 0b0001, 2)              # own AC
    seq, offs, res, lab = syn.case([a, b])
    mc, mo = np.array([3, 2, 3], np.uint8), np.array([0, 1, 3], np.int64)      # mates T and GT
    ent, org, tot = tdlib.mol_host_origins_mated(syn.md, seq, offs, res, lab, (mc, mo, 4), 8)
    assert tot["counted"] == 2 and tot["molecules"] == 1
    assert (int(org[0]["w"]), int(org[0]["n"])) == (0b00011011, 4) and int(ent[0]["key"]) == key_py(3, 0x1B04, 0b00011011, 4)


@pytest.mark.parametrize("name", FIXTURES)
def test_no_mate_is_the_unmated_function_entry_for_entry(name):
    g = load_golden(name)
    res = results_of(g)
    args = (g, g["seq"], g["offs"], res, g["labels"])
    for P in (1, 12, 32):
        a, ta = tdlib.mol_host(*args, P)
        b, tb = tdlib.mol_host_mated(*args, None, P)
        assert as_pairs(a) == as_pairs(b) and ta == tb
        a, ao, ta = tdlib.mol_host_origins(*args, P)
        b, bo, tb = tdlib.mol_host_origins_mated(*args, None, P)
        assert as_pairs(a) == as_pairs(b) and np.array_equal(ao, bo) and ta == tb
        a, ta = tdlib.mol_dedup_host(*args, P)
        b, tb = tdlib.mol_dedup_host_mated(*args, None, P)
        assert np.array_equal(a, b) and ta == tb
        a, ta, ca = tdlib.mol_dedup_collapsed_host(*args, P)
        b, tb, cb = tdlib.mol_dedup_collapsed_host_mated(*args, None, P)
        assert np.array_equal(a, b) and ta == tb and ca == cb
        assert as_pairs(tdlib.mol_host(*args, P)[0]) == count_py(classify_mated(*args, P, None))[0]


def test_refusals_of_the_host_functions():
    g = load_golden("umi_f_s_r")
    res = results_of(g)
    n = len(g["offs"]) - 1
    mc, mo, _ = mates_for(n, 8, seed=1)
    calls = (tdlib.mol_host_mated, tdlib.mol_host_origins_mated, tdlib.mol_dedup_host_mated, tdlib.mol_dedup_collapsed_host_mated)
    for call in calls:
        for bad in (0, -3):
            with pytest.raises(TdError, match=call.__name__.replace("mol_", "td_mol_") + ": mate bases = %d" % bad):
                call(g, g["seq"], g["offs"], res, g["labels"], (mc, mo, bad), 12)
        with pytest.raises(TdError, match=r"prefix_bases \+ mate bases = 12 \+ 21"):
            call(g, g["seq"], g["offs"], res, g["labels"], (mc, mo, 21), 12)
        with pytest.raises(TdError, match=r"prefix_bases \+ mate bases = 32 \+ 1"):
            call(g, g["seq"], g["offs"], res, g["labels"], (mc, mo, 1), 32)
        with pytest.raises(TdError, match="prefix_bases = 33"):
            call(g, g["seq"], g["offs"], res, g["labels"], (mc, mo, 1), 33)
        call(g, g["seq"], g["offs"], res, g["labels"], (mc, mo, 20), 12)           # 32 together is fine
        bad_offs = mo.copy()
        bad_offs[5] = bad_offs[4] - 1
        with pytest.raises(TdError, match="mate 4 has a negative length"):
            call(g, g["seq"], g["offs"], res, g["labels"], (mc, bad_offs, 8), 12)
    with pytest.raises(ValueError, match="the mate batch has"):
        tdlib.mol_host_mated(g, g["seq"], g["offs"], res, g["labels"], (mc, mo[:-1], 8), 12)


def test_header_symbols_and_the_mirror(library):
    hdr = open(os.path.join(REPO, "include", "tagdust_molecules.h")).read()
    for name in ("td_mol_mate_enable", "td_mol_mate_disable", "td_mol_mate_next", "td_mol_host_mated", "td_mol_host_origins_mated",
                 "td_mol_dedup_host_mated", "td_mol_dedup_collapsed_host_mated"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in tdlib.MOL_ABI_SYMBOLS and hasattr(library, name), name
    assert "typedef struct td_mol_mate { const uint8_t* codes; const int64_t* offs; int32_t bases; } td_mol_mate;" in hdr
    assert C.sizeof(tdlib._MolMate) == 24
    import tagdust_amd
    assert tagdust_amd.mol_host_mated is tdlib.mol_host_mated
    for m in ("mol_mate_enable", "mol_mate_disable", "mol_mate_next"):
        assert hasattr(tdlib.TagdustHip, m)
    # the host unit keeps one walk over a read, and the four unmated names are calls with no mate
    src = open(os.path.join(REPO, "tagdust_amd", "csrc", "td_molecules_host.cpp")).read()
    assert len(re.findall(r"\bint host_read_class\(", src)) == 1
    for name in ("td_mol_host", "td_mol_host_origins", "td_mol_dedup_host", "td_mol_dedup_collapsed_host"):
        body = src[src.index('extern "C" int %s(' % name):]
        body = body[body.index("{"):body.index("\n}\n")]
        assert "return %s_mated(" % name in body and "nullptr" in body and body.count(";") == 1, name


# ---- the run's option, plan and refusals ----
def _touch(d, name):
    p = os.path.join(str(d), name)
    open(p, "w").write("@r\nACGT\n+\nIIII\n")
    return p


def test_the_option_parses():
    o = tdlib.RunOpts(["in.fq"]).o
    assert (o.mate_bases, o.molecules) == (0, 0)
    o = tdlib.RunOpts(["a.fq", "b.fq", "--mate-bases", "20"]).o
    assert (o.mate_bases, o.molecules, o.molecules_prefix) == (20, 1, 20)           # implies --molecules
    for bad in ("0", "32", "-1", "x"):
        with pytest.raises(TdError, match="--mate-bases: need 1..31"):
            tdlib.RunOpts(["a.fq", "b.fq", "--mate-bases", bad])
    with pytest.raises(TdError, match="requires an argument"):
        tdlib.RunOpts(["a.fq", "--mate-bases"])
    with pytest.raises(TdError, match="unknown option -mate-bases"):
        tdlib.RunOpts(["a.fq", "-mate-bases", "4"])
    lib = tdlib.load_library()
    lib.td_run_usage.restype = C.c_char_p
    assert b"--mate-bases M" in lib.td_run_usage()


def test_the_plan_line_and_every_refusal(tmp_path):
    fq1, fq2, fq3 = _touch(tmp_path, "r1.fq"), _touch(tmp_path, "r2.fq"), _touch(tmp_path, "r3.fq")
    out = str(tmp_path / "o")
    segs = ["-1", "B:ACGT,TTGA", "-2", "F:NNNN", "-3", "R:N"]
    base = segs + ["-o", out, "-dust", "0", "--molecules-prefix", "12"]
    # without the option two files stay refused, word for word
    with pytest.raises(TdError, match=re.escape("--molecules needs exactly one input file (2 given): a read and its fingerprint in different "
                                                "files are not joined")):
        tdlib.run_plan(base + ["--molecules", fq1, fq2])
    plain = tdlib.run_plan(base + [fq1, fq2])
    plan = tdlib.run_plan(base + [fq1, fq2, "--mate-bases", "20"])
    assert "mate: " not in plain
    assert "mate: 20 bases" in plan and "output file: " + out + "_molecules.txt\n" in plan
    assert [l for l in plan.splitlines() if not l.startswith("mate: ") and "_molecules.txt" not in l] == plain.splitlines()
    assert "mate: 20 bases" in tdlib.run_plan(base + [fq1, fq2, fq3, "--mate-bases", "20", "--dedup"])
    with pytest.raises(TdError, match=r"--molecules-prefix.*--mate-bases|--mate-bases.*--molecules-prefix"):
        tdlib.run_plan(base + [fq1, fq2, "--mate-bases", "21"])
    with pytest.raises(TdError, match=r"--molecules-prefix.*--mate-bases|--mate-bases.*--molecules-prefix"):
        tdlib.run_plan(segs + ["-o", out, "-dust", "0", fq1, fq2, "--mate-bases", "13"])     # the default prefix of 20
    with pytest.raises(TdError, match="--mate-bases needs two or more input files"):
        tdlib.run_plan(base + [fq1, "--mate-bases", "20"])
    with pytest.raises(TdError, match="run with -dust 0 and without -ref"):
        tdlib.run_plan(segs + ["-o", out, "--molecules-prefix", "12", fq1, fq2, "--mate-bases", "20"])      # the default DUST of 100
    ref = os.path.join(str(tmp_path), "ref.fa")
    open(ref, "w").write(">a\nACGTACGTACGTACGTACGT\n")
    with pytest.raises(TdError, match="run with -dust 0 and without -ref"):
        tdlib.run_plan(base + [fq1, fq2, "--mate-bases", "20", "-ref", ref])
    with pytest.raises(TdError, match="--mate-bases.*one device"):
        tdlib.run_plan(base + [fq1, fq2, "--mate-bases", "20", "--devices", "0,0"])
    with pytest.raises(TdError, match="--mate-bases.*--dedup-collapsed.*the survey reads one file"):
        tdlib.run_plan(base + [fq1, fq2, "--mate-bases", "20", "--dedup-collapsed"])
