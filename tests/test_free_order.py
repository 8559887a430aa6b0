"""Segment orders away from "tags, one read segment, optional 3' linker" (CPU side): the five reference-made fixtures reach the
branches of extract_reads (barcode_hmm.c:3172-3313) they were made for, and the committed seeds of the free-order fuzz
(test_parity_gpu.test_free_order_architectures_against_oracle) still cover what they were chosen to cover -- a later edit of the
generator must not silently empty the fuzz."""
import numpy as np
import pytest

from conftest import load_golden

FREE_ORDER_FIXTURES = ["b_s_b_r", "r_s_b_f", "f_b_f_r", "b_f", "r_g_b_r"]


def _types(g):
    return "".join(chr(int(t)) for t in g["seg_type"])


def _seg_of_labels(g, i):
    """segment index per base of read i, from the reference's labels"""
    o = int(g["offs"][i])
    lab = g["labels"][o + i + 1:int(g["offs"][i + 1]) + i + 1]
    return np.asarray(g["label"]).astype(np.int64)[lab] & 0xFFFF


@pytest.mark.parametrize("name", FREE_ORDER_FIXTURES)
def test_fixture_outcomes(name):
    """240 reads; outcome 0 and two more outcomes with five reads each."""
    g = load_golden(name)
    assert int(g["n_reads"]) == 240
    hist = np.bincount(g["read_type"] & 0xFF)
    print(name, float(g["threshold"]), hist.tolist())
    assert hist[0] >= 5 and (hist[1:] >= 5).sum() >= 2


def test_fixtures_reach_their_branches():
    ok = lambda g: g["read_type"] == 0
    # two B segments: the barcode reported is the last one's, every barcode of both occurs, the decoy is hit in the second
    g = load_golden("b_s_b_r")
    assert _types(g) == "BSBR" and list(g["n_hmm"]) == [5, 2, 4, 1]
    assert ((g["barcode"][ok(g)] >> 16) == 2).all() and set((g["barcode"][ok(g)] & 0xFFFF).tolist()) == {0, 1, 2}
    pairs = set()
    label = np.asarray(g["label"]).astype(np.int64)
    for i in np.flatnonzero(ok(g)):
        lab = label[g["labels"][int(g["offs"][i]) + i + 1:int(g["offs"][i + 1]) + i + 1]]
        pairs.add((int(((lab >> 16) & 0x7FFF)[(lab & 0xFFFF) == 0][0]), int(g["barcode"][i]) & 0xFFFF))
    assert len({a for a, b in pairs}) == 4 and any(a != b for a, b in pairs)
    # the read segment first, tags behind it: reads whose read segment ends too short in front of the tags
    g = load_golden("r_s_b_f")
    assert _types(g) == "RSBF"
    short = np.flatnonzero(g["read_type"] == 2)
    assert len(short) >= 5
    for i in short[:5]:
        seg = _seg_of_labels(g, i)
        assert seg[0] == 0 and (seg == 0).sum() < int(g["minlen"]) and (seg != 0).any()
    assert (g["fingerprint"][ok(g)] & 0xFF == 5).all()
    # two F segments: 16 fingerprint bases fill the 32-bit key, (key << 8) drops its top byte
    g = load_golden("f_b_f_r")
    assert _types(g) == "FBFR" and int(g["seg_len"][0]) + int(g["seg_len"][2]) == 16
    fp = g["fingerprint"][ok(g)].astype(np.int64) & 0xFFFFFFFF
    assert (fp & 0xFF == 16).all() and len(set(fp.tolist())) > 100
    keys = []
    for i in np.flatnonzero(ok(g)):
        seg = _seg_of_labels(g, i)
        b = g["seq"][int(g["offs"][i]):int(g["offs"][i + 1])][(seg == 0) | (seg == 2)].astype(np.int64) & 3
        key = 0
        for x in b:
            key = (key << 2) | int(x)
        assert len(b) == 16
        keys.append(key)
    keys = np.array(keys, np.int64)
    assert ((keys >> 24) != 0).sum() > 50                                # bits the shift loses ...
    assert np.array_equal(fp, ((keys << 8) & 0xFFFFFFFF) | 16)           # ... and it loses them
    assert (g["fingerprint"][ok(g)] < 0).any()                           # (as int32: the sign bit is in use)
    # no read segment: nothing of an extracted read is kept
    g = load_golden("b_f")
    assert _types(g) == "BF"
    for i in np.flatnonzero(ok(g))[:20]:
        assert (g["seq_after"][int(g["offs"][i]):int(g["offs"][i + 1])] == 65).all()
    # two read segments around G and a barcode: four or more label runs in a read
    g = load_golden("r_g_b_r")
    assert _types(g) == "RGBR"
    runs = [1 + int((np.diff(_seg_of_labels(g, i)) != 0).sum()) for i in np.flatnonzero(ok(g))]
    assert max(runs) >= 4 and (g["read_type"] == 2).sum() >= 5


@pytest.fixture(scope="module")
def fuzz_cases():
    from oracle import pyoracle
    from test_parity_gpu import _FREE_ORDER_SEEDS, _free_order_case
    out = []
    for seed in _FREE_ORDER_SEEDS:
        segs, seq, offs, md = _free_order_case(seed)
        ores, _, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, float(md["threshold"]), int(md["minlen"]), int(md["dust"]), 4)
        out.append((seed, segs, ores))
    return out


def test_free_order_seeds_cover_what_they_were_chosen_for(fuzz_cases):
    n = dict(two_b=0, r_not_last=0, no_r=0, two_f=0, f13=0, two_r=0)
    for seed, segs, ores in fuzz_cases:
        print(seed, segs, np.bincount(ores["read_type"] & 0xFF).tolist())
        assert np.isfinite(ores["b_score"]).all(), (seed, "a read without a path")
        assert (np.bincount(ores["read_type"] & 0xFF) >= 5).sum() >= 2, (seed, segs)
        ty = [s_[0] for s_ in segs]
        assert not any(a == "R" and b == "R" for a, b in zip(ty, ty[1:]))
        n["two_b"] += ty.count("B") == 2
        n["r_not_last"] += "R" in ty and ty[-1] != "R"
        n["no_r"] += "R" not in ty
        n["two_f"] += ty.count("F") == 2
        n["f13"] += sum(len(s_) - 2 for s_ in segs if s_[0] == "F") >= 13
        n["two_r"] += ty.count("R") == 2
    assert n["two_b"] >= 2 and n["r_not_last"] >= 2 and n["no_r"] >= 1 and n["two_f"] >= 1 and n["f13"] >= 1 and n["two_r"] >= 1, n
