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
    at least min(number of barcodes, 8) different barcodes among the extracted reads."""
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
        n_barcodes = int(np.asarray(g["n_hmm"])[bsegs[0]]) - 1      # (the last HMM of a barcode segment is the all-N decoy)
        ok = (res["read_type"] == 0) & (res["barcode"] >= 0)
        found = set(res["barcode"][ok].tolist())
        print(name, "barcodes", len(found), "of", n_barcodes)
        assert len(found) >= min(n_barcodes, 8)
