"""The barcode-segment shapes of tests/plan_shapes.py (CPU side): each shape still puts the specialised kernel's plan on the branch
it was made for, and its reads -- judged by the oracle alone -- still call every HMM of every barcode segment, so that a later edit of
the generator or of the plan's heuristics (tagdust_amd/csrc/td_spec_plan.cpp) cannot silently move a case off its branch.  These
are conditions on the inputs of tests/test_plan_shapes_gpu.py, not on the code under test."""
import numpy as np
import pytest

import plan_shapes
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib


@pytest.fixture(scope="module", autouse=True)
def _built():
    tdbuild.build()


def _calls(md, offs, ores, olab):
    """per B segment: how many extracted reads call each of its HMMs, read from the oracle's labels (test_free_order._seg_of_labels)"""
    label = np.asarray(md["label"]).astype(np.int64)
    calls = {j: np.zeros(int(md["n_hmm"][j]), np.int64) for j in range(int(md["S"])) if chr(int(md["seg_type"][j])) == "B"}
    for i in np.flatnonzero(ores["read_type"] == 0):
        lab = label[olab[int(offs[i]) + i + 1:int(offs[i + 1]) + i + 1]]
        for j in calls:
            at = (lab & 0xFFFF) == j
            if at.any():
                calls[j][int(((lab >> 16) & 0x7FFF)[at][0])] += 1
    return calls


@pytest.mark.parametrize("name", plan_shapes.NAMES)
def test_shape_reaches_its_plan_state(name):
    segs, seq, offs, md = plan_shapes.case(name)
    assert 256 <= len(offs) - 1 <= 512
    assert (float(md["threshold"]), int(md["minlen"]), int(md["dust"])) == (plan_shapes.THRESHOLD, plan_shapes.MINLEN, plan_shapes.DUST)
    p = plan_shapes.plan_features(tdlib.spec_source(md))
    want = plan_shapes.PLAN[name]
    print(name, segs[0][:20], p)
    for k in ("H", "rt", "group", "trie", "first_n", "prune_segs", "restart"):
        assert p[k] == want[k], (name, k, p[k], want[k])
    assert plan_shapes.share_class(p) == want["share"], (name, p["n_share"], p["rt"][0], p["group"][0])
    assert p["trie_sh"] == (2 if p["trie"] else 1)                      # (the default TD_SPEC_TRIE_SH)


def test_shapes_between_them_reach_every_state():
    """what the ten are there for, stated on the table itself"""
    P = plan_shapes.PLAN
    two_rt = [n for n in P if sum(r > 0 for r in P[n]["rt"]) >= 2]
    assert len(two_rt) >= 4
    assert any(P[n]["trie"] and P[n]["group"][0] == 1 for n in P)                                  # kGroup[0] == 1
    assert any(P[n]["rt"][0] > 0 and not P[n]["trie"] for n in P)                                  # looped, no sharing group
    assert any(P[n]["first_n"] > 0 and any(r > 0 for r in P[n]["rt"][1:]) for n in P)              # label sums + a later loop
    assert any(P[n]["first_n"] > 0 and P[n]["H"] - P[n]["first_n"] > 32 for n in P)                # pruning off behind label sums
    assert any(P[n]["prune_segs"] >= 3 and P[n]["restart"] and n in two_rt for n in P)             # bridges across two big segments
    assert any(P[n]["rt"][-1] > 0 for n in P)                                                      # a looped segment last
    assert any(P[n]["rt"][0] == 0 and sum(r > 0 for r in P[n]["rt"]) >= 2 for n in P)              # two loops, none first
    # shape D: the last real barcode and the decoy are left to the unrolled code behind the run-time prefix
    assert P["D"]["rt"][0] == 15 and len(plan_shapes.SHAPES["D"][0][0]) == 4 and plan_shapes.SHAPES["D"][0][0][1] == 16
    assert plan_shapes.SHAPES["I"][0][0][1] == 19                                                  # an odd count with groups of one


@pytest.mark.parametrize("name", plan_shapes.NAMES)
def test_oracle_outcomes_cover_every_hmm(name):
    segs, seq, offs, md = plan_shapes.case(name)
    ores, olab, _ = plan_shapes.oracle(name)
    hist = np.bincount(ores["read_type"] & 0xFF, minlength=8)
    calls = _calls(md, offs, ores, olab)
    print(name, hist.tolist(), {j: (int(c[:-1].min()), int(c[-1])) for j, c in calls.items()})
    assert np.isfinite(ores["b_score"]).all(), "a read without a path"
    assert (hist >= 5).sum() >= 2, hist
    p = plan_shapes.plan_features(tdlib.spec_source(md))
    for j, c in calls.items():
        assert len(c) == p["n_hmm"][j] and (c[:-1] >= 2).all(), (name, j, c.tolist())   # the last HMM of a B segment is its decoy
        assert p["rt"][j] <= len(c) - 1                                                   # (the left-overs at index >= kRt[j] among them)
    if p["trie"]:
        G, first = p["group"][0], calls[min(calls)]
        shared, left = p["ord"][:p["n_share"] * G], p["ord"][p["n_share"] * G:]
        assert sorted(p["ord"]) == list(range(p["rt"][0]))
        assert first[shared].sum() >= 1
        if plan_shapes.PLAN[name]["share"] == "some":
            assert len(left) >= 1 and first[left].sum() >= 1
        else:
            assert not left


@pytest.mark.parametrize("name,env,want", plan_shapes.KNOB_VARIANTS, ids=["%s-%s" % (v[0], "-".join("%s=%s" % kv for kv in v[1].items())) for v in plan_shapes.KNOB_VARIANTS])
def test_knob_variant_changes_its_plan_feature(name, env, want, monkeypatch):
    md = plan_shapes.case(name)[3]
    base = plan_shapes.plan_features(tdlib.spec_source(md))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = plan_shapes.plan_features(tdlib.spec_source(md))
    for k, v in want.items():
        assert p[k] == v, (name, env, k, p[k])
    assert any(p[k] != base[k] for k in want), (name, env)


def test_reference_made_fixture_of_shape_a():
    """plan_a_b16_s_b24_r (tests/golden/make_golden.py): the reference's own model and outputs for 240 reads of shape A's generator;
    its plan is shape A's, every real barcode of both segments is called, outcome 0 and two more have five reads each."""
    import os
    from conftest import GOLDEN_DIR, load_golden
    g = load_golden("plan_a_b16_s_b24_r")
    segs, reads = plan_shapes.make_reads(plan_shapes.SHAPES["A"][0], plan_shapes.SHAPES["A"][1], 240)
    assert int(g["n_reads"]) == 240 and "".join(chr(int(t)) for t in g["seg_type"]) == "BSBR" and list(g["n_hmm"]) == [17, 2, 25, 1]
    for j in (0, 2):                                                    # (the reference appends the decoy to a B segment's list)
        assert str(g["seg_seqs"]).split(";")[j] == segs[j][2:] + ",NNNNNNNN", j
    assert np.array_equal(g["seq"], np.array([plan_shapes.CODE[ch] for s_ in reads for ch in s_], np.uint8))
    hist = np.bincount(g["read_type"] & 0xFF, minlength=8)
    print(float(g["threshold"]), hist.tolist())
    assert hist[0] >= 5 and (hist[1:] >= 5).sum() >= 2
    p = plan_shapes.plan_features(tdlib.spec_source(g))
    want = plan_shapes.PLAN["A"]
    for k in ("H", "rt", "group", "trie", "first_n", "prune_segs", "restart"):
        assert p[k] == want[k], (k, p[k])
    ores = np.zeros(240, [("read_type", "<i4")])
    ores["read_type"] = g["read_type"]
    for j, c in _calls(g, g["offs"], ores, g["labels"]).items():
        assert (c[:-1] >= 2).all(), (j, c.tolist())
    assert os.path.getsize(os.path.join(GOLDEN_DIR, "plan_a_b16_s_b24_r.npz")) <= 32 * 1024


def test_windowed_case_and_samples_shape():
    """the -start / -end case on shape A keeps the plan of shape A; the sheet shape of tests/test_samples_gpu.py loops both segments"""
    segs, seq, offs, md = plan_shapes.case("A", plan_shapes.WINDOW)
    p = plan_shapes.plan_features(tdlib.spec_source(md))
    assert p["rt"] == [16, 0, 24, 0] and p["first_n"] == 17
    ores, _, _ = plan_shapes.oracle("A", plan_shapes.WINDOW)
    hist = np.bincount(ores["read_type"] & 0xFF, minlength=8)
    print("A windowed", hist.tolist())
    assert np.isfinite(ores["b_score"]).all() and (hist >= 5).sum() >= 2 and hist[0] >= 100
    segs, seq, offs, md = plan_shapes.make_case(*plan_shapes.SAMPLES_SHAPE)
    p = plan_shapes.plan_features(tdlib.spec_source(md))
    assert p["rt"] == [16, 0, 16, 0] and p["n_hmm"] == [17, 2, 17, 1]
