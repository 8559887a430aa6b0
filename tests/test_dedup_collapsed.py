"""One read per collapsed molecule (include/tagdust_molecules.h: survey, freeze, replay) on the host, no GPU:
td_mol_dedup_collapsed_host against the definition restated here in plain Python -- neighbour keys through td_mol_key -- on the
hand-built tables of tests/test_collapse.py spelled out as reads, on the reference's fixture with an F segment and on a hand-ordered
case built for this test; the option of the whole-run driver, its plan line and its refusals.

The restatement (replay_py) and the hand-ordered case's molecules are also what tests/test_dedup_collapsed_gpu.py uses."""
import os

import numpy as np
import pytest

from conftest import load_golden
from tagdust_amd import TdError
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib
from test_collapse import fingerprint_of, i32, mol


@pytest.fixture(scope="module", autouse=True)
def library():
    tdbuild.build()
    return tdlib.load_library()


# ---- the definition ----
def classify(md, seq, offs, res, labels, P):
    """what every read is to the count: None (not eligible), "empty", "n", or (key, (w, fingerprint, n)) of a counted read"""
    is_r = [int(md["seg_type"][int(v) & 0xFFFF]) == ord("R") for v in md["label"]]
    out = []
    for i in range(len(offs) - 1):
        if int(res["read_type"][i]) & 0xFF != 0:
            out.append(None)
            continue
        o, ln = int(offs[i]), int(offs[i + 1] - offs[i])
        lab = labels[o + i:o + i + ln + 1]
        bases = [int(seq[o + p]) for p in range(ln) if 0 <= int(lab[p + 1]) < len(is_r) and is_r[int(lab[p + 1])]][:P]
        if not bases:
            out.append("empty")
        elif any(b > 3 for b in bases):
            out.append("n")
        else:
            w = 0
            for b in bases:
                w = (w << 2) | b
            fp = int(res["fingerprint"][i])
            out.append((tdlib.mol_key(int(res["barcode"][i]), fp, w, len(bases)), (w, fp, len(bases))))
    return out


def forest_py(count, origin):
    """{key: the root of its tree} by the collapse's definition: the parent is the qualifying neighbour that comes first"""
    before = lambda a, b: (-count[a], a) < (-count[b], b)
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
    root = {}
    for u in count:
        r = u
        while parent[r] != r:
            r = parent[r]
        root[u] = r
    return root


def replay_py(survey, replay=None, held=None, rule="root"):
    """The definition.  survey, replay: what classify gives for the surveyed and for the replayed reads (None: the same reads); read
    i has ordinal i in either.  held: {key: (count, origin)} of the keys the table holds after the survey (None: every key of the
    survey, no overflow).  rule "root": keeper = the first ordinal of the root's own key; "min": the minimum over the tree, which
    the definition rules out.  Returns (is_duplicate, dedup totals, collapse totals without the chain)."""
    replay = survey if replay is None else replay
    first, count, origin = {}, {}, {}
    for i, c in enumerate(survey):
        if isinstance(c, tuple):
            first.setdefault(c[0], i)
            count[c[0]] = count.get(c[0], 0) + 1
            origin.setdefault(c[0], c[1])
    if held is not None:
        count = {k: v[0] for k, v in held.items()}
        origin = {k: v[1] for k, v in held.items()}
    root = forest_py(count, origin)
    if rule == "root":
        keeper = {u: first[root[u]] for u in count}
    else:
        keeper = {u: min(first[v] for v in count if root[v] == root[u]) for u in count}
    dup = np.zeros(len(replay), bool)
    tot = dict.fromkeys(tdlib.MOL_DEDUP_TOTALS, 0)
    for i, c in enumerate(replay):
        if c is None:
            continue
        if not isinstance(c, tuple) or c[0] not in keeper:
            tot["unjudged"] += 1
            tot["kept"] += 1
        elif keeper[c[0]] == i:
            tot["kept"] += 1
        else:
            dup[i] = True
            tot["duplicates"] += 1
    n_roots = len(set(root.values()))
    return dup, tot, {"molecules_before": len(count), "molecules_after": n_roots, "absorbed": len(count) - n_roots}


def check_identities(classes, tot, ctot, overflow=0):
    """eligible(survey) == kept + duplicates and kept == molecules_after + skipped_empty + skipped_n + overflow"""
    eligible = sum(c is not None for c in classes)
    skipped = sum(c in ("empty", "n") for c in classes)
    assert eligible == tot["kept"] + tot["duplicates"]
    assert tot["kept"] == ctot["molecules_after"] + skipped + overflow and tot["unjudged"] == skipped + overflow


# ---- reads without a decoder: a fixture's model, labels and records written by hand ----
class Synthetic:
    """reads whose labels say "four bases of something else, then read bases" over the model of the fixture umi_f_s_r"""

    def __init__(self):
        self.md = load_golden("umi_f_s_r")
        seg = [int(self.md["seg_type"][int(v) & 0xFFFF]) for v in self.md["label"]]
        self.h_read = seg.index(ord("R"))
        self.h_other = next(h for h, t in enumerate(seg) if t != ord("R"))

    def read(self, bin_, fp, w, n, n_at=None, tail=3):
        """one extracted read of barcode bin_ and fingerprint fp whose first n read bases spell w (n = 0: no read base at all);
        n_at: that read base is an N"""
        body = [(w >> (2 * (n - 1 - p))) & 3 for p in range(n)] + ([1, 2, 3][:tail] if n >= 20 else [])
        if n_at is not None:
            body[n_at] = 4
        seq = np.array([0, 1, 2, 3] + body, np.uint8)
        lab = np.array([self.h_other] * 5 + [self.h_read] * len(body), np.int8)
        return seq, lab, (0, bin_, fp)

    def case(self, reads):
        """(seq, offs, res, labels) of a list of read() results"""
        offs = np.zeros(len(reads) + 1, np.int64)
        offs[1:] = np.cumsum([len(s) for s, _, _ in reads])
        res = {"read_type": np.array([r[0] for _, _, r in reads], np.int32), "barcode": np.array([r[1] for _, _, r in reads], np.int32),
               "fingerprint": np.array([r[2] for _, _, r in reads], np.int32)}
        return np.concatenate([s for s, _, _ in reads]), offs, res, np.concatenate([l for _, l, _ in reads])

    def of_items(self, items, seed):
        """a table of test_collapse.py -- [(key, count, (w, fingerprint, n))] -- as reads, every molecule as often as its count says,
        in a shuffled order"""
        reads = []
        for key, count, (w, fp, n) in items:
            reads += [self.read(key >> 56, fp, w, n)] * count
        order = np.random.default_rng(seed).permutation(len(reads))
        return self.case([reads[i] for i in order])


@pytest.fixture(scope="module")
def syn():
    return Synthetic()


def host_and_py(md, seq, offs, res, labels, P):
    """td_mol_dedup_collapsed_host held against the restatement, flags and totals, and both identities; (classes, flags, totals)"""
    dup, tot, ctot = tdlib.mol_dedup_collapsed_host(md, seq, offs, res, labels, P)
    classes = classify(md, seq, offs, res, labels, P)
    want, want_tot, want_ctot = replay_py(classes)
    assert np.array_equal(dup, want) and tot == want_tot
    assert {k: ctot[k] for k in want_ctot} == want_ctot
    check_identities(classes, tot, ctot)
    return classes, dup, tot, ctot


# the tables of tests/test_collapse.py
no_fp = lambda w, n=9: (tdlib.mol_key(2, -1, w, n), 1, (w, -1, n))
HAND_BUILT = {
    "chain": lambda: [mol("AACC", 3), mol("AAAA", 10), mol("AAAC", 5)],
    "threshold-8": lambda: [mol("ACGT", 5), mol("ACGA", 8)],
    "threshold-9": lambda: [mol("ACGT", 5), mol("ACGA", 9)],
    "singletons-2": lambda: [mol("GGGG", 1), mol("GGGT", 1)],
    "singletons-3": lambda: [mol("TTTA", 1), mol("TTTC", 1), mol("TTTG", 1)],
    "two-parents-5-7": lambda: [mol("CAAA", 1), mol("CAAC", 5), mol("CAAG", 7)],
    "two-parents-5-5": lambda: [mol("CAAA", 1), mol("CAAC", 5), mol("CAAG", 5)],
    "other-bin": lambda: [mol("ACAC", 10), mol("ACAA", 1, bin_=4)],
    "other-prefix": lambda: [mol("ACAC", 10), mol("ACAA", 1, w=0x1B2E)],
    "other-prefix-length": lambda: [mol("ACAC", 10), mol("ACAA", 1, n=19)],
    "same-bin-and-prefix": lambda: [mol("ACAC", 10), mol("ACAA", 1)],
    "twelve-bases": lambda: [mol("ACGTACGTACGT", 10), mol("TCGTACGTACGT", 2)],
    "fourteen-bases": lambda: [mol("GGACGTACGTACGT", 10), mol("GGTCGTACGTACGT", 2)],
    "repeated-keys": lambda: [mol("GATC", 8), mol("GATA", 2), mol("GATA", 3)],
    "no-fingerprint": lambda: [no_fp(77), (tdlib.mol_key(2, i32(0xFFFFFFFF ^ (1 << 8)), 77, 9), 10, (77, i32(0xFFFFFFFF ^ (1 << 8)), 9)), no_fp(78)],
    "nothing": lambda: [],
}


@pytest.mark.parametrize("name", sorted(HAND_BUILT))
def test_the_hand_built_tables_as_reads(syn, name):
    items = HAND_BUILT[name]()
    seq, offs, res, labels = syn.of_items(items, 3) if items else (np.zeros(0, np.uint8), np.zeros(1, np.int64),
                                                                  {f: np.zeros(0, np.int32) for f in ("read_type", "barcode", "fingerprint")}, np.zeros(0, np.int8))
    classes, dup, tot, ctot = host_and_py(syn.md, seq, offs, res, labels, 20)
    assert tot["kept"] + tot["duplicates"] == sum(c for _, c, _ in items) and tot["unjudged"] == 0
    assert ctot["molecules_before"] == len({k for k, _, _ in items})
    # every kept read spells a root of td_mol_collapse_host over the same table
    if items:
        e = np.array([(k, c) for k, c, _ in items], tdlib.CENSUS_ENTRY_DTYPE)
        o = np.array([o for _, _, o in items], tdlib.MOL_ORIGIN_DTYPE)
        roots, _, rtot = tdlib.mol_collapse_host(e, o)
        assert sorted(classes[i][0] for i in np.flatnonzero(~dup)) == sorted(int(k) for k in roots["key"]) and rtot == ctot
    if name == "chain":
        assert tot["kept"] == 1 and ctot["longest_chain"] == 2
    if name == "threshold-8":
        assert tot["kept"] == 2


def test_a_random_table_with_many_neighbours(syn):
    rng = np.random.default_rng(11)
    items = []
    for _ in range(300):
        umi = "".join("ACGT"[b] for b in rng.integers(0, 4, 4))
        items.append(mol(umi, int(rng.choice([1, 1, 1, 2, 3, 5, 9])), bin_=int(rng.integers(0, 2)), w=int(rng.integers(0, 2))))
    seq, offs, res, labels = syn.of_items(items, 5)
    classes, dup, tot, ctot = host_and_py(syn.md, seq, offs, res, labels, 20)
    exact = tdlib.mol_dedup_host(syn.md, seq, offs, res, labels, 20)[1]
    assert ctot["absorbed"] > 50 and ctot["longest_chain"] >= 2 and tot["duplicates"] == exact["duplicates"] + ctot["absorbed"]


# ---- the hand-ordered case ----
# (barcode index, UMI, read index, what is special) per read, in input order: the chain 10 <- 5 <- 3 with a copy of the grandchild
# first, then a copy of the child, and the root's first read behind both; a singleton tie; neighbours in two bins; a read with an N
# in its prefix; a read without a read base
def hand_ordered():
    chain = [(0, "AACC", 0, None), (0, "AAAC", 0, None), (0, "AAAA", 0, None)]
    rest = [(0, "AAAA", 0, None)] * 9 + [(0, "AAAC", 0, None)] * 4 + [(0, "AACC", 0, None)] * 2
    order = np.random.default_rng(17).permutation(len(rest))
    tie = [(3, "GGGT", 0, None), (3, "GGGG", 0, None)]
    bins = [(5, "CACA", 0, None)] * 3 + [(6, "CACC", 0, None)]
    return chain + [rest[i] for i in order[:8]] + tie + [(1, "ACGT", 0, "n")] + bins + [rest[i] for i in order[8:]] + [(1, "ACGT", 0, "empty")]


def test_the_hand_ordered_case_pins_the_root_s_first_read(syn):
    W, P = 0x1B2D, 20
    reads = []
    for b, umi, _, special in hand_ordered():
        reads.append(syn.read(b, fingerprint_of(umi), W, 0 if special == "empty" else P, n_at=3 if special == "n" else None))
    seq, offs, res, labels = syn.case(reads)
    classes, dup, tot, ctot = host_and_py(syn.md, seq, offs, res, labels, P)
    assert classes.count("n") == 1 and classes.count("empty") == 1 and None not in classes and len(reads) < 64
    key = lambda b, umi: tdlib.mol_key(b, fingerprint_of(umi), W, P)
    keys = [c[0] if isinstance(c, tuple) else None for c in classes]
    # the chain: reads 0 and 1 are the grandchild's and the child's first, read 2 the root's -- the one that stays
    assert keys[:3] == [key(0, "AACC"), key(0, "AAAC"), key(0, "AAAA")]
    chain = [i for i, k in enumerate(keys) if k in keys[:3]]
    assert len(chain) == 18 and [i for i in chain if not dup[i]] == [2]
    # "the minimum over the tree" would keep read 0 instead: the definition is the root's first
    by_min = replay_py(classes, rule="min")[0]
    assert [i for i in chain if not by_min[i]] == [0] and not np.array_equal(by_min, dup)
    # the tie: the smaller key is the root, whichever came first; the bins stay apart
    tie = [i for i, k in enumerate(keys) if k in (key(3, "GGGG"), key(3, "GGGT"))]
    assert [keys[i] for i in tie if not dup[i]] == [min(key(3, "GGGG"), key(3, "GGGT"))]
    assert sum(not dup[i] for i, k in enumerate(keys) if k in (key(5, "CACA"), key(6, "CACC"))) == 2
    # exact dedup marks fewer: the feature shows
    exact, exact_tot = tdlib.mol_dedup_host(syn.md, seq, offs, res, labels, P)
    assert exact_tot["duplicates"] < tot["duplicates"] == exact_tot["duplicates"] + ctot["absorbed"] and ctot["absorbed"] == 3
    assert tot == {"kept": 4 + 2, "duplicates": len(reads) - 6, "unjudged": 2}
    assert ctot == {"molecules_before": 7, "molecules_after": 4, "absorbed": 3, "longest_chain": 2}


# ---- the reference's fixture with an F segment ----
@pytest.mark.parametrize("P", [1, 20, 32])
def test_on_the_reference_s_fixture(P):
    g = load_golden("umi_f_s_r")
    res = {f: np.asarray(g[f]) for f in ("read_type", "barcode", "fingerprint")}
    classes, dup, tot, ctot = host_and_py(g, g["seq"], g["offs"], res, g["labels"], P)
    assert tot["kept"] > 0 and ctot["molecules_before"] == tdlib.mol_host(g, g["seq"], g["offs"], res, g["labels"], P)[1]["molecules"]
    exact, exact_tot = tdlib.mol_dedup_host(g, g["seq"], g["offs"], res, g["labels"], P)
    assert tot["duplicates"] == exact_tot["duplicates"] + ctot["absorbed"]
    if P == 1:
        assert ctot["absorbed"] > 0 and not np.array_equal(exact, dup)
    # a record that is no success is no duplicate either, and never judged
    assert not dup[(np.asarray(g["read_type"]) & 0xFF) != 0].any()


def test_bad_arguments_fail_with_a_message():
    lib = tdlib._mol_lib()
    assert lib.td_mol_dedup_collapsed_host(None, 20, None, None, 0, None, None, None, None, None) != 0
    assert b"td_mol_dedup_collapsed_host" in lib.td_last_error(None)
    assert lib.td_mol_dedup_freeze(None, None) != 0
    g = load_golden("umi_f_s_r")
    with pytest.raises(TdError, match="prefix_bases"):
        tdlib.mol_dedup_collapsed_host(g, g["seq"], g["offs"], {f: np.asarray(g[f]) for f in ("read_type", "barcode", "fingerprint")}, g["labels"], 0)


# ---- the run's option, plan and refusals ----
def _touch(d, name):
    p = os.path.join(str(d), name)
    open(p, "w").write("@r\nACGT\n+\nIIII\n")
    return p


def test_the_option_the_plan_and_the_refusals(tmp_path):
    def parsed(args):
        ro = tdlib.RunOpts(args)
        try:
            return ro.o.dedup_collapsed, ro.o.dedup, ro.o.collapse_umis, ro.o.molecules
        finally:
            ro.close()

    assert parsed(["in.fq"]) == (0, 0, 0, 0)
    assert parsed(["in.fq", "--dedup", "--collapse-umis"]) == (0, 1, 1, 1)
    assert parsed(["in.fq", "--dedup-collapsed"]) == (1, 1, 1, 1)            # alone, it sets the three it implies
    with pytest.raises(TdError, match="unknown option -dedup-collapsed"):    # own options take two dashes
        tdlib.RunOpts(["in.fq", "-dedup-collapsed"])
    lib = tdlib._run_lib()
    lib.td_run_usage.restype = tdlib.C.c_char_p
    assert b"--dedup-collapsed " in lib.td_run_usage()
    fq, fq2 = _touch(tmp_path, "in.fq"), _touch(tmp_path, "in2.fq")
    out = str(tmp_path / "o")
    base = ["-1", "B:ACGT,TTGA", "-2", "F:NNNN", "-3", "R:N", "-o", out]
    both = tdlib.run_plan(base + [fq, "--dedup", "--collapse-umis"])
    # without the new option the plan is what it is today, text for text
    assert "dedup-collapsed" not in both
    assert [l for l in both.splitlines() if l.startswith(("dedup", "collapse"))] == [
        "dedup: one read per molecule is written (barcode, fingerprint and the start of the read)",
        "collapse: fingerprints one mismatch apart are counted as one molecule (directional rule; the count and --dedup stay exact)"]
    plan = tdlib.run_plan(base + [fq, "--dedup-collapsed"])
    line = [l for l in plan.splitlines() if l.startswith("dedup-collapsed: ")]
    assert len(line) == 1 and "read twice" in line[0] and "one read per collapsed molecule" in line[0]
    assert plan.replace(line[0] + "\n", "") == both and "output file: " + out + "_molecules.txt\n" in plan
    assert tdlib.run_plan(base + [fq, "--dedup-collapsed", "--dedup", "--collapse-umis", "--molecules"]) == plan
    with pytest.raises(TdError, match="needs exactly one input file"):
        tdlib.run_plan(base + [fq, fq2, "--dedup-collapsed"])
    for window in (["-start", "3"], ["-end", "30"]):
        with pytest.raises(TdError, match="cannot be combined with -start / -end"):
            tdlib.run_plan(base + [fq, "--dedup-collapsed"] + window)
    with pytest.raises(TdError, match="the architecture is a single read segment"):
        tdlib.run_plan(["-1", "R:N", fq, "-o", out, "--dedup-collapsed"])
    with pytest.raises(TdError, match="the architecture has no fingerprint"):
        tdlib.run_plan(["-1", "B:ACGT,TTGA", "-2", "R:N", fq, "-o", out, "--dedup-collapsed"])
    with pytest.raises(TdError, match="needs exactly one device"):
        tdlib.run_plan(base + [fq, "--dedup-collapsed", "--devices", "0,1"])
    with pytest.raises(TdError, match="cannot read the input from stdin"):
        tdlib.run_plan(base + ["-", "--dedup-collapsed"])
    assert tdlib.run_plan(base + ["-", "--dedup", "--collapse-umis"])        # (stdin stays fine for one pass)


def test_the_abi_mirror_has_the_new_names_and_fields():
    assert {"td_mol_dedup_freeze", "td_mol_dedup_collapsed_host"} <= set(tdlib.MOL_ABI_SYMBOLS) and "td_stream_survey" in tdlib.IO_ABI_SYMBOLS
    lib = tdlib.load_library()
    for name in ("td_mol_dedup_freeze", "td_mol_dedup_collapsed_host", "td_stream_survey"):
        assert getattr(lib, name)
    assert tdlib._RunOpts._fields_[-1][0] == "dedup_collapsed" and [f for f, _ in tdlib._RunReport._fields_[-2:]] == ["dedup_collapsed", "survey_s"]
