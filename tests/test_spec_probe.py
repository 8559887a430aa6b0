"""The probe reads (td_spec_probe, include/tagdust_hip.h): what a freshly loaded specialised kernel is compared with the generic
kernel on before it takes over.  Host only: they must be reproducible, leave the C library's rand() alone (threshold calibration
is bound to its sequence) and exercise the model -- several outcomes, several barcodes -- under the probe's fixed parameters."""
import ctypes as C
import ctypes.util

import numpy as np
import pytest

from conftest import load_golden, GOLDEN_NAMES

N_PROBE = 256


@pytest.fixture(scope="module")
def probes():
    """name -> (fixture, codes, offs): made once, shared, never modified."""
    from tagdust_amd import lib
    out = {}
    for name in GOLDEN_NAMES:
        g = load_golden(name)
        codes, offs = lib.spec_probe(g)
        codes.setflags(write=False)
        offs.setflags(write=False)
        out[name] = (g, codes, offs)
    return out


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_probe_is_reproducible_and_well_formed(probes, name):
    from tagdust_amd import lib
    g, codes, offs = probes[name]
    codes2, offs2 = lib.spec_probe(g)
    assert codes.tobytes() == codes2.tobytes() and offs.tobytes() == offs2.tobytes()
    assert len(offs) == N_PROBE + 1 and offs[0] == 0 and offs[-1] == len(codes)
    lens = np.diff(offs)
    assert (lens >= 1).all()
    assert codes.min() >= 0 and codes.max() <= 4
    assert (codes == 4).any(), "no N among the probe reads"
    for t in range(N_PROBE // 64):
        assert len(set(lens[t * 64:(t + 1) * 64].tolist())) > 1, "tile %d is not ragged" % t


def test_probe_leaves_rand_alone(probes):
    from tagdust_amd import lib
    libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")
    libc.rand.restype = C.c_int
    libc.srand.argtypes = [C.c_uint]
    libc.srand(1)
    want = libc.rand()
    for name in GOLDEN_NAMES:
        libc.srand(1)
        lib.spec_probe(probes[name][0])
        assert libc.rand() == want, name


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_probe_exercises_the_model(probes, name):
    """Decoded by the oracle under the probe's fixed parameters: at least two outcomes, and for a model with a barcode segment
    at least min(number of barcodes, 8) different barcodes among the extracted reads -- of the LAST barcode segment, the one
    whose barcode extract_reads reports ((segment << 16) | barcode, hence the mask)."""
    from oracle import pyoracle
    from tagdust_amd import lib
    g, codes, offs = probes[name]
    p = lib.spec_probe_params()
    assert p["minlen"] == 16 and p["dust"] == 100
    res, labels, seq = pyoracle.label_batch(pyoracle.OracleModel(g), codes, offs, p["threshold"], p["minlen"], p["dust"], 4)
    outcomes = set((res["read_type"] & 0xFF).tolist())
    print(name, "outcomes", np.bincount(res["read_type"] & 0xFF).tolist())
    assert len(outcomes) >= 2
    seg_type = np.asarray(g["seg_type"]).astype(np.int64)
    bsegs = [j for j in range(int(g["S"])) if seg_type[j] == ord("B")]
    if bsegs:
        n_barcodes = int(np.asarray(g["n_hmm"])[bsegs[-1]]) - 1      # (the last HMM of a barcode segment is the all-N decoy)
        ok = (res["read_type"] == 0) & (res["barcode"] >= 0)
        assert ((res["barcode"][ok] >> 16) == bsegs[-1]).all()
        found = set((res["barcode"][ok] & 0xFFFF).tolist())
        print(name, "barcodes", len(found), "of", n_barcodes)
        assert len(found) >= min(n_barcodes, 8)


def test_probe_combines_the_barcodes_of_two_segments():
    """Two barcode segments of equal size: were both to take HMM k % nh for the k-th architecture-following read, only the pairs
    (i, i) would ever be probed.  Later barcode segments step through the combinations instead; decoded by the oracle, the
    extracted architecture-following reads show at least min(nh1 * nh2, 8) different (first, second) barcode pairs -- the second
    as extract_reads reports it, the first read off the labels."""
    from oracle import pyoracle
    from tagdust_amd import lib
    rng = np.random.RandomState(5)
    bars1, bars2 = ["ACAGTG", "CTTGTA", "GGCTAC"], ["TTAGGC", "CATGCA", "AGTCAA"]
    segs = ["B:" + ",".join(bars1), "S:GT", "B:" + ",".join(bars2), "R:N"]
    reads = []
    for i in range(200):
        s_ = bars1[rng.randint(3)] + "GT" + bars2[rng.randint(3)] + "".join("ACGT"[x] for x in rng.randint(0, 4, rng.randint(20, 50)))
        reads.append(np.array(["ACGT".index(ch) for ch in s_], np.uint8))
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    md, _ = lib.build_model(segs, np.concatenate(reads), offs, 0.05, 0.1)
    nh1, nh2 = int(md["n_hmm"][0]), int(md["n_hmm"][2])
    assert nh1 == nh2 == 4
    codes, offs = lib.spec_probe(md)
    p = lib.spec_probe_params()
    res, labels, _ = pyoracle.label_batch(pyoracle.OracleModel(md), codes, offs, p["threshold"], p["minlen"], p["dust"], 4)
    label = np.asarray(md["label"]).astype(np.int64)
    pairs = set()
    for r in range(N_PROBE):
        if (r & 7) == 7 or res["read_type"][r] != 0:       # (one read in eight ignores the architecture)
            continue
        lab = label[labels[offs[r] + r + 1:offs[r + 1] + r + 1]]
        first = set(((lab >> 16) & 0x7FFF)[(lab & 0xFFFF) == 0].tolist())
        assert len(first) == 1 and int(res["barcode"][r]) >> 16 == 2
        pairs.add((first.pop(), int(res["barcode"][r]) & 0xFFFF))
    print("pairs", sorted(pairs))
    assert len(pairs) >= min(nh1 * nh2, 8)
