#!/usr/bin/env python
"""Which states of the model-specialised kernel's plan (tagdust_amd/csrc/td_spec_plan.cpp) the GPU suite reaches: the plan features of
every model a GPU test uploads -- the fixtures of tests/golden (and those test_runtime_hmm_loop_path forces into the run-time loop),
the committed seeds of the tag fuzz, the free-order fuzz, the windowed fuzz and the many-label architectures, the bench workloads, the
shapes of tests/plan_shapes.py with their knob variants -- read from tdlib.spec_source, then each plan state with the models that
reach it.  CPU only; run it after a change to the plan's heuristics and look for a state that lost its last model.
usage: tools/plan_survey.py [--states]     (--states: the second table only; exit status 1 if a state is reached by no model)"""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tagdust_amd import lib as tdlib

for k in [k for k in os.environ if k.startswith("TD_SPEC_") and k != "TD_SPEC_CACHE_DIR"]:
    del os.environ[k]

# state -> (what it is, predicate over the plan features and the segment types of a model)
STATES = [
    ("two-loops", "two or more run-time-looped segments", lambda p, ty: sum(r > 0 for r in p["rt"]) >= 2),
    ("loops-none-first", "two looped segments, the first segment not among them", lambda p, ty: p["rt"][0] == 0 and sum(r > 0 for r in p["rt"]) >= 2),
    ("trie-group1", "trie order with kGroup[0] == 1 (every HMM shares, no left-over)", lambda p, ty: p["trie"] and p["group"][0] == 1),
    ("trie-leftovers", "trie order with sharing groups and left-over slots", lambda p, ty: p["trie"] and 0 < p["n_share"] < p["rt"][0] // p["group"][0]),
    ("loop-no-trie", "first segment looped, trie order off", lambda p, ty: p["rt"][0] > 0 and not p["trie"]),
    ("trie-sh-other", "a TD_SPEC_TRIE_SH other than 2", lambda p, ty: p["trie"] and p["trie_sh"] != 2),
    ("left-over-hmm", "a real barcode behind the run-time prefix (kRt[j] < n_hmm - 1)", lambda p, ty: any(0 < r < n - 1 for r, n in zip(p["rt"], p["n_hmm"]))),
    ("sums+later-loop", "kFirstN > 0 and a later segment looped", lambda p, ty: p["first_n"] > 0 and any(r > 0 for r in p["rt"][1:])),
    ("sums-no-prune", "kFirstN > 0 and H - kFirstN > 32 (pruning off)", lambda p, ty: p["first_n"] > 0 and p["H"] - p["first_n"] > 32),
    ("many-labels+two-loops", "kFirstN == 0, H > 32, two looped segments", lambda p, ty: p["first_n"] == 0 and p["H"] > 32 and sum(r > 0 for r in p["rt"]) >= 2),
    ("restart-two-big", "restarted sweeps bridging two looped segments", lambda p, ty: p["restart"] == 1 and sum(r > 0 for r in p["rt"][:p["prune_segs"]]) >= 2),
    ("cut-two-big-no-restart", "pruned, not restarted, two looped leading segments", lambda p, ty: p["restart"] == 0 and sum(r > 0 for r in p["rt"][:p["prune_segs"]]) >= 2),
    ("loop-last", "a looped segment last, behind the read segment", lambda p, ty: p["rt"][-1] > 0 and "R" in ty[:-1]),
    ("generic-wide-multi", "a multi-HMM segment of more than 16 columns (generic kernel: workspace rows)", lambda p, ty: any(n > 1 and c > 16 for n, c in zip(p["n_hmm"], p["n_col"]))),
    ("index-8nt+", "a barcode segment of 16 or more HMMs and 8 or more columns", lambda p, ty: any(t == "B" and n >= 16 and c >= 8 for t, n, c in zip(ty, p["n_hmm"], p["n_col"]))),
]


def models():
    """(source of the model, name, model mapping, environment) of every model the GPU suite uploads"""
    import bench
    import plan_shapes
    import test_parity_gpu as tp
    from conftest import GOLDEN_NAMES, load_golden
    for name in GOLDEN_NAMES:
        yield "fixture", name, load_golden(name), {}
    for name in ("c2_b4_r", "c3_b6_s_r_p", "casava_index", "scen1_b_r", "o_b_s_r", "b_s_b_r"):      # test_runtime_hmm_loop_path
        yield "fixture", name + " RT_MIN=3", load_golden(name), {"TD_SPEC_RT_MIN": "3"}
    for seed in tp._FUZZ_SEEDS:
        yield "fuzz", "seed %d" % seed, tp._random_case(seed)[3], {}
    for seed in tp._FREE_ORDER_SEEDS:
        yield "free-order", "seed %d" % seed, tp._free_order_case(seed)[3], {}
    for case in tp._WINDOW_CASES:
        yield "window", "%s %d %d-%d" % (case[0], case[1], case[2][0], case[2][1]), tp._windowed_case(case)[3], {}
    for case in tp._MANY_LABEL_CASES:
        yield "many-label", "b%d%s%s" % (case[0], " 5'P" if case[1] else "", " umi" if case[2] else ""), tp._many_label_case(*case)[3], {}
    for w in ("c2", "c3", "c5"):
        bench.select_workload(w)
        yield "bench", w, bench.load_model(), {}
    bench.select_workload("c3")
    for name in plan_shapes.NAMES:
        yield "shape", name, plan_shapes.case(name)[3], {}
    yield "shape", "A window", plan_shapes.case("A", plan_shapes.WINDOW)[3], {}
    for name, env, _ in plan_shapes.KNOB_VARIANTS:
        yield "shape", name + " " + " ".join("%s=%s" % (k[8:], v) for k, v in env.items()), plan_shapes.case(name)[3], env
    yield "shape", "samples sheet", plan_shapes.make_case(*plan_shapes.SAMPLES_SHAPE)[3], {}


def main():
    import plan_shapes
    rows = []
    for src, name, md, env in models():
        os.environ.update(env)
        p = plan_shapes.plan_features(tdlib.spec_source(md))
        for k in env:
            del os.environ[k]
        ty = "".join(chr(int(t)) for t in md["seg_type"])
        rows.append((src, name, ty, p))
    if "--states" not in sys.argv[1:]:
        print("%-10s %-28s %-7s %3s  %-18s %-14s %-12s %6s %5s %7s" % ("source", "model", "types", "H", "kRt", "kGroup", "trie", "firstN", "prune", "restart"))
        for src, name, ty, p in rows:
            trie = "on sh%d %d/%d" % (p["trie_sh"], p["n_share"], p["rt"][0] // p["group"][0]) if p["trie"] else "off"
            print("%-10s %-28s %-7s %3d  %-18s %-14s %-12s %6d %5d %7d" % (src, name, ty, p["H"], ",".join(map(str, p["rt"])), ",".join(map(str, p["group"])),
                                                                           trie, p["first_n"], p["prune_segs"], p["restart"]))
        print()
    missing = 0
    for key, text, pred in STATES:
        hit = ["%s %s" % (src, name) for src, name, ty, p in rows if pred(p, ty)]
        missing += not hit
        print("%-24s %-72s %s" % (key, text, "; ".join(hit[:8]) + (" (+%d)" % (len(hit) - 8) if len(hit) > 8 else "") if hit else "-- NO MODEL --"))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
