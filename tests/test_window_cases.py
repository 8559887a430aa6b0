"""-start / -end on architectures other than "B R" (CPU side): the two reference-made windowed fixtures meet the conditions
they were generated for (tests/golden/make_golden.py asserts the same before it writes them), and the committed cases of the
windowed fuzz (test_parity_gpu.test_windowed_architectures_against_oracle), recomputed with the oracle, still cover what each
was chosen for -- a later edit of a generator must not silently empty the fuzz."""
import numpy as np
import pytest

from conftest import golden_artifacts, golden_window, load_golden

WINDOW_FIXTURES = ["win_r_s_b_r", "win_b_f_r_ref"]


def _types(g):
    return "".join(chr(int(t)) for t in g["seg_type"])


def _kept_behind(seq_after, offs, i, matchend):
    """bases of read i at or behind matchend that the rewrite kept"""
    return int((seq_after[int(offs[i]) + matchend:int(offs[i + 1])] != 65).sum()) if offs[i + 1] - offs[i] > matchend else 0


def check_win_r_s_b_r(g):
    """A read segment first: 240 reads, -Q given, -dust 30 given (which the reference switches off again for two read segments,
    interface.c:441-445); outcome 0 and two other outcomes with five reads each; at least 20
    extracted reads keep a base at or behind matchend, and a read whose first segment is a read segment keeps all of them."""
    ms, me = golden_window(g)
    assert _types(g) == "RSBR" and (ms, me) == (2, 58) and int(g["q_given"]) == 1
    assert "-dust 30" in str(g["cmdline"]) and int(g["dust"]) == 0
    assert int(g["n_reads"]) == 240 and (g["lens"] >= me).all()
    hist = np.bincount(g["read_type"] & 0xFF, minlength=8)
    assert hist[0] >= 5 and (hist[1:] >= 5).sum() >= 2, hist
    ok = np.flatnonzero(g["read_type"] == 0)
    tails = [_kept_behind(g["seq_after"], g["offs"], i, me) for i in ok]
    assert sum(t > 0 for t in tails) >= 20, tails
    assert all(t == int(g["lens"][i]) - me for t, i in zip(tails, ok))
    assert any(int(g["lens"][i]) == me for i in ok)                        # ... and reads that end with the window have none
    return hist


def check_win_b_f_r_ref(g):
    """B F R under a window with -ref on three threads (243 reads: ranges of 81 with one left-over read each): at least 10
    artifact hits, one or more of them on a left-over position; 5 low-complexity reads; 5 successes, with fingerprints; 5 reads
    whose mismatch follows from the window cutting the barcode (nothing in front of it) -- they succeed under a window that
    starts where their architecture does."""
    from oracle import pyoracle
    ms, me = golden_window(g)
    art = golden_artifacts(g)
    assert _types(g) == "BFR" and (ms, me) == (3, 40) and int(g["q_given"]) == 0 and int(g["dust"]) == 30 and art[3] == 3
    n = int(g["n_reads"])
    assert n == 243 and (g["lens"] >= me).all()
    rt = g["read_type"] & 0xFF
    hist = np.bincount(rt, minlength=8)
    assert hist[5] >= 10 and hist[6] >= 5 and hist[0] >= 5, hist
    interval = n // 3
    left_over = [t * interval + (interval // 4) * 4 + k for t in range(3) for k in range(interval % 4)]
    assert left_over == [80, 161, 242] and (rt[left_over] == 5).any(), rt[left_over]
    ok = g["read_type"] == 0
    assert (g["fingerprint"][ok] & 0xFF == 5).all() and len(set(g["fingerprint"][ok].tolist())) >= 5
    for i in np.flatnonzero(ok):                                            # behind the window the first segment is B: nothing kept
        assert _kept_behind(g["seq_after"], g["offs"], i, me) == 0
    names = bytes(g["names"]).split(b"\n")
    cut = np.array([nm.endswith(b";CUT") for nm in names])
    assert (cut & (rt == 1)).sum() >= 5, (int(cut.sum()), rt[cut])
    moved, _, _ = pyoracle.label_batch(pyoracle.OracleModel(g), g["seq"], g["offs"], float(g["threshold"]), int(g["minlen"]),
                                       int(g["dust"]), 1, window=(0, me - ms))
    assert ((moved["read_type"] == 0) & cut & (rt == 1)).sum() >= 5, moved["read_type"][cut & (rt == 1)]
    return hist


FIXTURE_CHECKS = {"win_r_s_b_r": check_win_r_s_b_r, "win_b_f_r_ref": check_win_b_f_r_ref}


@pytest.mark.parametrize("name", WINDOW_FIXTURES)
def test_windowed_fixture_meets_its_conditions(name):
    import os
    from conftest import GOLDEN_DIR
    g = load_golden(name)
    print(name, float(g["threshold"]), FIXTURE_CHECKS[name](g).tolist())
    assert os.path.getsize(os.path.join(GOLDEN_DIR, name + ".npz")) <= 32 * 1024


def _case_stats(case):
    """What one case of the windowed fuzz covers, from the generator and the oracle alone."""
    from test_parity_gpu import _windowed_oracle
    segs, seq, offs, md, artifacts, nthreads, ores, olab, oseq = _windowed_oracle(case)
    ms, me = case[2]
    lens = np.diff(offs)
    ty = [s_[0] for s_ in segs]
    rt = ores["read_type"] & 0xFF
    ok = np.flatnonzero(ores["read_type"] == 0)
    return dict(
        segs=segs, ty="".join(ty), H=int(md["H"]), hist=np.bincount(rt, minlength=8),
        tail_kept=sum(_kept_behind(oseq, offs, i, me) > 0 for i in ok),
        fingerprints=int((ores["fingerprint"][ok] != -1).sum()) if "F" in ty else 0,
        inside=int(((lens > ms) & (lens < me) & np.isfinite(ores["b_score"])).sum()),
        nothing=int((np.isneginf(ores["b_score"]) | (lens <= ms)).sum()),
        p3=ty[-1] == "P" and len(ty) > 1, nbar=max([s_.count(",") + 1 for s_ in segs if s_[0] == "B"] or [0]),
        art=artifacts is not None)


def test_windowed_fuzz_cases_cover_what_they_were_chosen_for():
    from test_parity_gpu import _WINDOW_CASES
    assert 8 <= len(_WINDOW_CASES) <= 10
    stats = [_case_stats(c) for c in _WINDOW_CASES]
    for c, st in zip(_WINDOW_CASES, stats):
        print(c, st["ty"], "H", st["H"], st["hist"].tolist(), {k: st[k] for k in ("tail_kept", "fingerprints", "inside", "nothing")})
        assert c[2][0] in (0, 2, 5, 9)
        assert (st["hist"] >= 5).sum() >= 2, c
        assert st["inside"] >= 20 and st["nothing"] >= 8, c
    n = lambda f: sum(1 for st in stats if f(st))
    assert n(lambda st: st["ty"][0] == "R" and st["tail_kept"] >= 10) >= 2
    assert n(lambda st: st["ty"].count("R") == 2) >= 1
    assert n(lambda st: "F" in st["ty"] and st["fingerprints"] >= 20) >= 1
    assert n(lambda st: st["p3"]) >= 1
    assert n(lambda st: st["nbar"] >= 20 and st["H"] > 32) >= 1
    assert n(lambda st: "R" not in st["ty"]) >= 1
    assert n(lambda st: st["art"]) >= 2
    assert n(lambda st: st["art"] and st["hist"][5] >= 5 and st["hist"][6] >= 5) >= 1
