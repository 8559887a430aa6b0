"""The UMI collapse (include/tagdust_molecules.h) on the host, no GPU: td_mol_collapse_host against the definition restated here in
plain Python, neighbour keys through td_mol_key, on hand-built tables and on the reference's fixtures; td_mol_host_origins against
a restatement over the reference's own labels and records; the option of the whole-run driver, its plan line and its refusals."""
import os

import numpy as np
import pytest

from conftest import load_golden
from tagdust_amd import TdError
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

FIXTURES = ["umi_f_s_r", "r_s_b_f", "f_b_f_r", "c5_b96_f_r_p"]


@pytest.fixture(scope="module", autouse=True)
def library():
    tdbuild.build()
    return tdlib.load_library()


def i32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v & 0x80000000 else v


def fingerprint_of(umi):
    """the reference's int of (bases << 8 | length): the leading bases of more than 12 fall out of it"""
    v = 0
    for ch in umi:
        v = (v << 2) | "ACGT".index(ch)
    return i32((v << 8) | len(umi))


def collapse_py(items):
    """The definition.  items: [(key, count, (w, fingerprint, n))], keys may repeat.  Returns (the roots [(key, collapsed, origin)]
    by collapsed descending then key ascending, totals dict)."""
    count, origin = {}, {}
    for k, c, o in items:
        count[k] = count.get(k, 0) + c
        origin.setdefault(k, o)
    before = lambda a, b: (-count[a], a) < (-count[b], b)   # (count, key) of a comes strictly before that of b
    parent = {}
    for u in count:
        w, fp, n = origin[u]
        m = 0 if fp == -1 else min(fp & 0xFF, 12)
        best = None
        for i in range(m):
            for d in (1, 2, 3):
                v = tdlib.mol_key(u >> 56, i32((fp & 0xFFFFFFFF) ^ (d << (8 + 2 * i))), w, n)
                if v in count and count[v] >= 2 * count[u] - 1 and before(v, u) and (best is None or before(v, best)):
                    best = v
        parent[u] = u if best is None else best
    collapsed = dict.fromkeys(count, 0)
    longest = 0
    for u in count:
        r, steps = u, 0
        while parent[r] != r:
            r, steps = parent[r], steps + 1
        collapsed[r] += count[u]
        longest = max(longest, steps)
    roots = sorted(((k, collapsed[k], origin[k]) for k in count if parent[k] == k), key=lambda t: (-t[1], t[0]))
    tot = {"molecules_before": len(count), "molecules_after": len(roots), "absorbed": len(count) - len(roots), "longest_chain": longest}
    return roots, tot


def arrays(items):
    e = np.array([(k, c) for k, c, _ in items], tdlib.CENSUS_ENTRY_DTYPE)
    o = np.array([o for _, _, o in items], tdlib.MOL_ORIGIN_DTYPE)
    return e, o


def as_items(entries, origins):
    return [(int(k), int(c), (int(w), int(f), int(n))) for (k, c), (w, f, n) in zip(entries.tolist(), origins.tolist())]


def collapse_both(items):
    """td_mol_collapse_host held against the restatement and both identities; returns (roots {key: collapsed}, totals)"""
    ent, org, tot = tdlib.mol_collapse_host(*arrays(items))
    want, want_tot = collapse_py(items)
    assert as_items(ent, org) == want and tot == want_tot
    assert tot["molecules_after"] + tot["absorbed"] == tot["molecules_before"] == len({k for k, _, _ in items})
    assert int(ent["count"].sum()) == sum(c for _, c, _ in items)
    return {int(k): int(c) for k, c in ent.tolist()}, tot


def mol(umi, count, bin_=3, w=0x1B2D, n=20):
    fp = fingerprint_of(umi)
    return (tdlib.mol_key(bin_, fp, w, n), count, (w, fp, n))


# ---- hand-built tables ----
def test_a_chain_of_ten_five_three_has_one_root():
    a, b, c = mol("AAAA", 10), mol("AAAC", 5), mol("AACC", 3)   # the 3 is two mismatches from the 10
    roots, tot = collapse_both([c, a, b])
    assert roots == {a[0]: 18} and tot["longest_chain"] == 2 and tot["absorbed"] == 2


def test_the_threshold_for_a_child_of_five():
    child = mol("ACGT", 5)
    roots, tot = collapse_both([child, mol("ACGA", 8)])
    assert len(roots) == 2 and tot["absorbed"] == 0 and tot["longest_chain"] == 0
    parent = mol("ACGA", 9)
    roots, tot = collapse_both([child, parent])
    assert roots == {parent[0]: 14} and tot["longest_chain"] == 1


def test_singletons_the_smaller_key_is_the_root():
    a, b = mol("GGGG", 1), mol("GGGT", 1)
    roots, _ = collapse_both([a, b])
    assert roots == {min(a[0], b[0]): 2}
    three = [mol("TTTA", 1), mol("TTTC", 1), mol("TTTG", 1)]   # mutually one mismatch apart
    roots, tot = collapse_both(three)
    assert roots == {min(k for k, _, _ in three): 3} and tot["longest_chain"] == 1


def test_a_child_with_two_qualifying_parents():
    child, p5, p7 = mol("CAAA", 1), mol("CAAC", 5), mol("CAAG", 7)   # (7 < 2 * 5 - 1: the two parents stay apart)
    roots, _ = collapse_both([child, p5, p7])
    assert roots == {p5[0]: 5, p7[0]: 8}
    q5 = mol("CAAG", 5)
    roots, _ = collapse_both([child, p5, q5])
    lo, hi = sorted([p5[0], q5[0]])
    assert roots == {lo: 6, hi: 5}


def test_other_bins_prefixes_and_prefix_lengths_stay_apart():
    big = mol("ACAC", 10)
    for other in (mol("ACAA", 1, bin_=4), mol("ACAA", 1, w=0x1B2E), mol("ACAA", 1, n=19)):
        roots, tot = collapse_both([big, other])
        assert len(roots) == 2 and tot["absorbed"] == 0
    roots, _ = collapse_both([big, mol("ACAA", 1)])
    assert roots == {big[0]: 11}


def test_umis_of_twelve_and_fourteen_bases():
    # 12 bases: the first base sits in bits 30..31 of the int, a mismatch there crosses the sign bit
    a, b = mol("ACGTACGTACGT", 10), mol("TCGTACGTACGT", 2)
    assert a[2][1] > 0 > b[2][1]
    roots, _ = collapse_both([a, b])
    assert roots == {a[0]: 12}
    # 14 bases: only the last 12 are in the fingerprint -- a mismatch in base 2 (the first it still holds) collapses, and UMIs
    # that differ in base 0 alone are one fingerprint
    a, b = mol("GGACGTACGTACGT", 10), mol("GGTCGTACGTACGT", 2)
    roots, _ = collapse_both([a, b])
    assert roots == {a[0]: 12}
    assert fingerprint_of("GGACGTACGTACGT") == fingerprint_of("TGACGTACGTACGT") and (a[2][1] & 0xFF) == 14


def test_repeated_keys_are_added_first():
    parent, child = mol("GATC", 8), mol("GATA", 5)
    halves = [parent, (child[0], 2, child[2]), (child[0], 3, child[2])]      # 2 and 3 alone would each be absorbed by the 8
    roots, tot = collapse_both(halves)
    assert roots == {parent[0]: 8, child[0]: 5} and tot["molecules_before"] == 2


def test_entries_without_a_fingerprint_are_never_merged():
    w, n = 77, 9
    none = (tdlib.mol_key(2, -1, w, n), 1, (w, -1, n))
    near = i32(0xFFFFFFFF ^ (1 << 8))                                         # one "mismatch" from -1 by the bare formula
    big = (tdlib.mol_key(2, near, w, n), 10, (w, near, n))
    roots, tot = collapse_both([none, big, (tdlib.mol_key(2, -1, w + 1, n), 1, (w + 1, -1, n))])
    assert none[0] in roots and roots[none[0]] == 1 and tot["molecules_after"] == 3
    assert collapse_both([])[1] == {"molecules_before": 0, "molecules_after": 0, "absorbed": 0, "longest_chain": 0}


def test_a_random_table_with_many_neighbours():
    rng = np.random.default_rng(11)
    items = []
    for _ in range(600):                                                      # 4-nt UMIs, two bins, two prefixes: dense neighbourhoods
        umi = "".join("ACGT"[b] for b in rng.integers(0, 4, 4))
        items.append(mol(umi, int(rng.choice([1, 1, 1, 2, 3, 5, 9, 17, 40])), bin_=int(rng.integers(0, 2)), w=int(rng.integers(0, 2))))
    roots, tot = collapse_both(items)
    assert tot["absorbed"] > 50 and tot["longest_chain"] >= 2 and tot["molecules_after"] > 4


# ---- the reference's fixtures ----
def origins_py(g, P):
    """mol_host's definition with what every key was made of: ([(key, count, origin)] in the order of td_census_get, totals)"""
    is_r = [int(g["seg_type"][int(v) & 0xFFFF]) == ord("R") for v in g["label"]]
    seq, offs, labels = g["seq"], g["offs"], g["labels"]
    tot = dict.fromkeys(tdlib.MOL_TOTALS, 0)
    counts, origin = {}, {}
    for i in range(len(offs) - 1):
        if int(g["read_type"][i]) & 0xFF != 0:
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
            fp = int(g["fingerprint"][i])
            k = tdlib.mol_key(int(g["barcode"][i]), fp, w, len(bases))
            counts[k] = counts.get(k, 0) + 1
            assert origin.setdefault(k, (w, fp, len(bases))) == (w, fp, len(bases))
            tot["counted"] += 1
    tot["molecules"] = len(counts)
    return [(k, c, origin[k]) for k, c in sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))], tot


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("P", [1, 20, 32])
def test_host_origins_and_collapse_on_the_reference_s_fixtures(name, P):
    g = load_golden(name)
    res = {f: np.asarray(g[f]) for f in ("read_type", "barcode", "fingerprint")}
    ent, org, tot = tdlib.mol_host_origins(g, g["seq"], g["offs"], res, g["labels"], P)
    want, want_tot = origins_py(g, P)
    assert as_items(ent, org) == want and tot == want_tot and len(want) > 0
    plain, plain_tot = tdlib.mol_host(g, g["seq"], g["offs"], res, g["labels"], P)
    assert np.array_equal(plain, ent) and plain_tot == tot
    assert all(tdlib.mol_key(k >> 56, o[1], o[0], o[2]) == k for k, _, o in want)      # an origin is what its key was made of
    roots, ctot = collapse_both(want)
    assert ctot["molecules_before"] == tot["molecules"]
    if P == 1 and name in ("umi_f_s_r", "r_s_b_f"):                                    # (few prefixes: UMIs meet their neighbours)
        assert ctot["absorbed"] > 0
    # the two halves' molecules concatenated collapse to the whole's
    n = int(g["n_reads"])
    offs = np.asarray(g["offs"], np.int64)
    cut = n // 2
    a = tdlib.mol_host_origins(g, g["seq"][:offs[cut]], offs[:cut + 1], {f: v[:cut] for f, v in res.items()}, g["labels"][:offs[cut] + cut], P)
    b = tdlib.mol_host_origins(g, g["seq"][offs[cut]:], offs[cut:] - offs[cut], {f: v[cut:] for f, v in res.items()}, g["labels"][offs[cut] + cut:], P)
    both = tdlib.mol_collapse_host(np.concatenate([a[0], b[0]]), np.concatenate([a[1], b[1]]))
    whole = tdlib.mol_collapse_host(ent, org)
    assert np.array_equal(both[0], whole[0]) and np.array_equal(both[1], whole[1]) and both[2] == whole[2]


def test_bad_arguments_fail_with_a_message():
    lib = tdlib._mol_lib()
    assert lib.td_mol_collapse_host(None, None, 1, None, None, None, None) != 0
    assert b"td_mol_collapse_host" in lib.td_last_error(None)
    for call in (lib.td_mol_collapse_enable, lib.td_mol_collapse_disable):
        assert call(None) != 0
    g = load_golden("umi_f_s_r")
    with pytest.raises(TdError, match="prefix_bases"):
        tdlib.mol_host_origins(g, g["seq"], g["offs"], {f: np.asarray(g[f]) for f in ("read_type", "barcode", "fingerprint")}, g["labels"], 33)


# ---- the run's option, plan and refusals ----
def _touch(d, name):
    p = os.path.join(str(d), name)
    open(p, "w").write("@r\nACGT\n+\nIIII\n")
    return p


def test_the_option_the_plan_and_the_refusals(tmp_path):
    def parsed(args):
        ro = tdlib.RunOpts(args)
        try:
            return ro.o.collapse_umis, ro.o.molecules, ro.o.dedup
        finally:
            ro.close()

    assert parsed(["in.fq"]) == (0, 0, 0)
    assert parsed(["in.fq", "--molecules"]) == (0, 1, 0)
    assert parsed(["in.fq", "--collapse-umis"]) == (1, 1, 0)                 # alone, it turns the count on
    assert parsed(["in.fq", "--collapse-umis", "--dedup"]) == (1, 1, 1)
    with pytest.raises(TdError, match="unknown option -collapse-umis"):      # own options take two dashes
        tdlib.RunOpts(["in.fq", "-collapse-umis"])
    lib = tdlib._run_lib()
    lib.td_run_usage.restype = tdlib.C.c_char_p
    assert b"--collapse-umis " in lib.td_run_usage()
    fq, fq2 = _touch(tmp_path, "in.fq"), _touch(tmp_path, "in2.fq")
    out = str(tmp_path / "o")
    base = ["-1", "B:ACGT,TTGA", "-2", "F:NNNN", "-3", "R:N", "-o", out]
    with_mol = tdlib.run_plan(base + [fq, "--molecules"])
    with_col = tdlib.run_plan(base + [fq, "--collapse-umis"])
    assert "collapse" not in with_mol and "collapse" not in tdlib.run_plan(base + [fq])
    line = [l for l in with_col.splitlines() if l.startswith("collapse: ")]
    assert len(line) == 1 and "one mismatch apart" in line[0]
    assert with_col.replace(line[0] + "\n", "") == with_mol and "output file: " + out + "_molecules.txt\n" in with_col
    both = tdlib.run_plan(base + [fq, "--collapse-umis", "--dedup"])
    assert both.replace(line[0] + "\n", "") == tdlib.run_plan(base + [fq, "--dedup"])
    assert tdlib.run_plan(base + [fq, "--collapse-umis", "--devices", "0,1"])        # (the devices' molecules are collapsed on the host)
    with pytest.raises(TdError, match="--collapse-umis: the architecture has no fingerprint"):
        tdlib.run_plan(["-1", "B:ACGT,TTGA", "-2", "R:N", fq, "-o", out, "--collapse-umis"])
    with pytest.raises(TdError, match="needs exactly one input file"):
        tdlib.run_plan(base + [fq, fq2, "--collapse-umis"])
    for window in (["-start", "3"], ["-end", "30"]):
        with pytest.raises(TdError, match="cannot be combined with -start / -end"):
            tdlib.run_plan(base + [fq, "--collapse-umis"] + window)
    with pytest.raises(TdError, match="the architecture is a single read segment"):
        tdlib.run_plan(["-1", "R:N", fq, "-o", out, "--collapse-umis"])
