"""Parity tests proper: the HIP path (through the C-ABI, tagdust_amd/libtagdust_hip.so) against
 (a) the committed fixtures produced by the reference itself (tests/golden/*.npz) and
 (b) the CPU oracle on fresh seeded inputs.
Bit-exact for labels / outcomes / barcodes / fingerprints / extracted sequences and for the float
scores (f, b, r, bar_prob); Q within 1e-4 (BASELINE.json north_star) -- in practice also bit-exact."""
import os

import numpy as np
import pytest

from conftest import load_golden, golden_artifacts, golden_window, GOLDEN_NAMES

pytestmark = pytest.mark.gpu

Q_TOL = 1e-4


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module", params=[1, 0], ids=["specialised", "generic"])
def ctx(request):
    """Both device paths: the model-specialised kernel (hiprtc, default) and the generic ahead-of-time kernel."""
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", request.param)
    c.set_option("poison_workspace", 1)      # stale workspace contents must never reach a result
    yield c
    c.close()


def _run(ctx, g, seq=None, offs=None, threshold=None):
    art = golden_artifacts(g)
    if art:
        ctx.set_artifacts(art[0], art[1], art[2], art[3])
    else:
        ctx.set_artifacts(None)
    ctx.upload_model(g)
    ctx.set_params(float(g["threshold"]) if threshold is None else threshold, int(g["minlen"]), int(g["dust"]))
    win = golden_window(g) if seq is None else None        # a fixture run with -start / -end
    ctx.set_window(*(win or (-1, -1)))
    try:
        ctx.upload_batch(g["seq"] if seq is None else seq, g["offs"] if offs is None else offs)
        ctx.counts_reset()
        ctx.run()
        return ctx.download()
    finally:
        ctx.set_window(-1, -1)


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_hip_vs_reference_fixture(ctx, name):
    g = load_golden(name)
    res, labels, seq_after = _run(ctx, g)
    assert np.array_equal(_bits(res["b_score"]), _bits(g["b_score"]))
    assert np.array_equal(_bits(res["f_score"]), _bits(g["f_score"]))
    assert np.array_equal(_bits(res["r_score"]), _bits(g["r_score"]))
    assert np.array_equal(_bits(res["bar_prob"]), _bits(g["bar_prob"].astype(np.float32)))
    assert np.array_equal(labels, g["labels"])
    assert np.allclose(res["mapq"], g["mapq"], rtol=0, atol=Q_TOL)
    assert np.array_equal(res["read_type"], g["read_type"])
    assert np.array_equal(res["barcode"], g["barcode"])
    assert np.array_equal(res["fingerprint"], g["fingerprint"])
    assert np.array_equal(seq_after, g["seq_after"])
    # device-side outcome counters == serial counting (barcode_hmm.c:354-384)
    cnt = ctx.counts()
    for code in range(8):
        assert cnt[code] == int(((g["read_type"] & 0xFF) == code).sum())   # an artifact hit is (sequence << 8) | 5
    ok = g["read_type"] == 0
    bins = np.bincount((g["barcode"][ok & (g["barcode"] >= 0)] & 0xFF), minlength=256)
    assert np.array_equal(cnt[8:], bins)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["c3_b6_s_r_p", "c2_b4_r", "c5_b96_f_r_p"])
def test_tiles_of_tiny_reads(ctx, name):
    """Tiles whose longest read is a handful of bases: S + 1 .. S + 12, 64 reads of each length, so that every tile's position
    loops end inside their first block (the request rings of the light sweep groups, the label DP and the traceback run in
    blocks of 2-4 positions and finish with a partial one).  HIP == oracle."""
    from oracle import pyoracle
    g = load_golden(name)
    S = int(g["S"])
    lens = np.repeat(np.arange(S + 1, S + 13), 64)
    rng = np.random.RandomState(77)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seq = rng.randint(0, 4, int(offs[-1])).astype(np.uint8)
    seq[rng.random_sample(len(seq)) < 0.02] = 4
    src_off = g["offs"]
    for i in range(0, len(lens), 2):   # prefixes of real reads, so that barcodes are found
        k = i % int(g["n_reads"])
        s_ = g["seq"][src_off[k]:src_off[k + 1]][:lens[i]]
        seq[offs[i]:offs[i] + len(s_)] = s_
    ores, olab, oseq = pyoracle.label_batch(pyoracle.OracleModel(g), seq, offs, float(g["threshold"]), int(g["minlen"]), int(g["dust"]), 4)
    res, labels, seq_after = _run(ctx, g, seq, offs)
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), k
    assert np.array_equal(labels, olab)
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL)
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), k
    assert np.array_equal(seq_after, oseq)


@pytest.mark.parametrize("name", ["c2_b4_r", "c3_b6_s_r_p", "scen2_endloss", "umi_f_s_r"])
def test_hip_vs_oracle_fresh_reads(ctx, name):
    """Fresh seeded reads (uniform random with occasional N, ragged lengths incl. 1-base reads) through
    the fixture's model: HIP == oracle."""
    from oracle import pyoracle
    g = load_golden(name)
    rng = np.random.RandomState(1234)
    n = 700
    lens = rng.randint(int(g["S"]) + 1, int(g["lens"].max()) + 1, n)
    lens[:5] = int(g["lens"].max())
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seq = rng.randint(0, 4, int(offs[-1])).astype(np.uint8)
    seq[rng.random_sample(len(seq)) < 0.01] = 4
    # plant real reads too so that successes occur
    src_off = g["offs"]
    for i in range(0, n, 3):
        k = i % int(g["n_reads"])
        s = g["seq"][src_off[k]:src_off[k + 1]]
        m = min(len(s), lens[i])
        seq[offs[i]:offs[i] + m] = s[:m]
    model = pyoracle.OracleModel(g)
    ores, olab, oseq = pyoracle.label_batch(model, seq, offs, float(g["threshold"]), int(g["minlen"]), int(g["dust"]), 4)
    res, labels, seq_after = _run(ctx, g, seq, offs)
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), k
    assert np.array_equal(labels, olab)
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL)
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), k
    assert np.array_equal(seq_after, oseq)


def test_empty_batch(ctx):
    g = load_golden("c2_b4_r")
    res, labels, seq_after = _run(ctx, g, np.zeros(0, np.uint8), np.zeros(1, np.int64))
    assert len(res) == 0 and len(labels) == 0 and len(seq_after) == 0


def test_long_segment_fallback_matches_oracle(ctx):
    """A 20-column partial segment exercises the workspace-row path (segments > 16 columns)."""
    from oracle import pyoracle
    g = load_golden("scen2_p_b_r_p")
    # widen the trailing P segment by repeating its middle column -- tables only, the oracle and the
    # HIP path see the same flattened model, which is all this test needs
    S, ncol, nh = int(g["S"]), g["n_col"].copy(), g["n_hmm"].copy()
    last = S - 1
    c0 = int((nh[:last] * ncol[:last]).sum())
    old = int(ncol[last])
    new = 20
    rep = [0] + [1] * (new - old + 1) + list(range(2, old))
    idx = list(range(c0)) + [c0 + r for r in rep]
    g2 = dict(g)
    for k in ("trans", "eM", "eI", "sM", "sI"):
        g2[k] = g[k][idx]
    ncol[last] = new
    g2["n_col"] = ncol
    g2["C"] = len(idx)
    seg_len = g["seg_len"].copy(); seg_len[last] = new
    g2["seg_len"] = seg_len
    model = pyoracle.OracleModel(g2)
    ores, olab, oseq = pyoracle.label_batch(model, g["seq"], g["offs"], float(g["threshold"]), int(g["minlen"]), int(g["dust"]), 4)
    res, labels, seq_after = _run(ctx, g2)
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), k
    assert np.array_equal(labels, olab)
    assert np.array_equal(res["read_type"], ores["read_type"])
    assert np.array_equal(seq_after, oseq)


@pytest.mark.parametrize("name", ["c2_b4_r", "scen2_endloss", "o_b_s_r"])
def test_backward_only_mode(ctx, name):
    """TD_MODE_ARCH_COMP (do_arch_comparison, barcode_hmm.c:2111-2148): backward() alone, b_score bit-exact."""
    from tagdust_amd import MODE_ARCH_COMP
    g = load_golden(name)
    ctx.upload_model(g)
    ctx.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
    ctx.upload_batch(g["seq"], g["offs"])
    ctx.run(MODE_ARCH_COMP)
    res, _, _ = ctx.download(labels=False, seq=False)
    assert np.array_equal(_bits(res["b_score"]), _bits(g["b_score"]))


def test_ascii_upload_and_large_ragged_batch(ctx):
    """td_batch_upload_ascii (nuc_code mapping incl. lower case, U, IUPAC -> N) on a ragged batch large enough to use the
    threaded host packing; HIP == oracle.  (1094 tiles: on a chip with 2048 wave slots or more every wave still gets one tile --
    waves that decode several tiles are tests/test_wave_reuse_gpu.py's.)"""
    from oracle import pyoracle
    g = load_golden("c2_b4_r")
    rng = np.random.RandomState(99)
    n = 70000
    lens = rng.randint(20, 101, n)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    codes = rng.randint(0, 4, int(offs[-1])).astype(np.uint8)
    codes[rng.random_sample(len(codes)) < 0.003] = 4
    src = g["offs"]
    for i in range(0, n, 2):   # plant real reads (prefixes) so that barcodes are found
        k = i % int(g["n_reads"])
        s_ = g["seq"][src[k]:src[k + 1]][:lens[i]]
        codes[offs[i]:offs[i] + len(s_)] = s_
    alphabet = np.frombuffer(b"ACGTN", np.uint8)
    ascii_ = alphabet[codes].copy()
    lower = rng.random_sample(len(ascii_)) < 0.1
    ascii_[lower] = np.frombuffer(b"acgtn", np.uint8)[codes[lower]]
    tu = (codes == 3) & (rng.random_sample(len(codes)) < 0.05)
    ascii_[tu] = ord("U")
    amb = (codes == 4) & (rng.random_sample(len(codes)) < 0.5)
    ascii_[amb] = ord("R")
    ctx.upload_model(g)
    ctx.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
    ctx.upload_batch_ascii(ascii_, offs)
    ctx.run()
    res, labels, seq_after = ctx.download()
    ores, olab, oseq = pyoracle.label_batch(pyoracle.OracleModel(g), codes, offs, float(g["threshold"]), int(g["minlen"]), int(g["dust"]), 16)
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), k
    assert np.array_equal(labels, olab)
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL)
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), k
    assert np.array_equal(seq_after, oseq)


@pytest.mark.parametrize("name", ["c2_b4_r", "c3_b6_s_r_p", "casava_index", "scen1_b_r", "o_b_s_r", "b_s_b_r"])
def test_runtime_hmm_loop_path(name, monkeypatch):
    """The specialised kernel's run-time HMM loop (normally only for segments with >= 16 HMMs, e.g. 96 barcodes) forced
    onto small barcode segments: same bits as the reference."""
    from tagdust_amd import TagdustHip, lib as tdlib
    monkeypatch.setenv("TD_SPEC_RT_MIN", "3")
    g = load_golden(name)
    assert "kRt[%d] = {0" % int(g["S"]) not in tdlib.spec_source(g) or name == "o_b_s_r"
    c = TagdustHip(0)
    try:
        res, labels, seq_after = _run(c, g)
    finally:
        c.close()
    for k in ("b_score", "f_score", "r_score"):
        assert np.array_equal(_bits(res[k]), _bits(g[k])), k
    assert np.array_equal(_bits(res["bar_prob"]), _bits(g["bar_prob"].astype(np.float32)))
    assert np.array_equal(labels, g["labels"])
    assert np.allclose(res["mapq"], g["mapq"], rtol=0, atol=Q_TOL)
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], g[k]), k
    assert np.array_equal(seq_after, g["seq_after"])


def test_long_linkers_from_host_model_builder(ctx):
    """Architecture with a 20-nt 5' linker and a 34-nt 3' adapter (segments longer than the register-row limit of the
    generic kernel), model built by the library's own host builder (include/tagdust_model.h) from the reads' statistics;
    HIP == oracle on reads carrying partial linkers."""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    rng = np.random.RandomState(7)
    five, three = "ACGTTGCATCGGATCCTAGA", "AGATCGGAAGAGCACACGTCTGAACTCCAGTCAC"
    bars = ["ACAGTG", "CTTGTA", "GGCTAC", "TAGCTT"]
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    reads = []
    for i in range(900):
        k5, k3 = rng.randint(0, len(five) + 1), rng.randint(0, len(three) + 1)
        s_ = five[len(five) - k5:] + bars[rng.randint(4)] + "".join("ACGT"[x] for x in rng.randint(0, 4, rng.randint(25, 60))) + three[:k3]
        s_ = "".join(("ACGT"[rng.randint(4)] if rng.random_sample() < 0.02 else ch) for ch in s_)
        if rng.random_sample() < 0.1:
            s_ = "".join("ACGT"[x] for x in rng.randint(0, 4, len(s_)))
        reads.append(np.array([code[ch] for ch in s_], np.uint8))
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    seq = np.concatenate(reads)
    segs = ["P:" + five, "B:" + ",".join(bars), "R:N", "P:" + three]
    md, st = tdlib.build_model(segs, seq, offs, 0.05, 0.1)
    assert list(md["n_col"]) == [20, 6, 1, 34]
    md.update(threshold=2.0, minlen=16, dust=100)
    model = pyoracle.OracleModel(md)
    ores, olab, oseq = pyoracle.label_batch(model, seq, offs, 2.0, 16, 100, 8)
    assert (ores["read_type"] == 0).sum() > 300
    res, labels, seq_after = _run(ctx, md, seq, offs, threshold=2.0)
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), k
    assert np.array_equal(labels, olab)
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL)
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), k
    assert np.array_equal(seq_after, oseq)


def test_abi_error_paths(ctx):
    """Misuse is reported as TD_FAIL with a message (never a crash, never a silent fallback)."""
    from tagdust_amd import TdError, TagdustHip
    g = load_golden("c2_b4_r")
    fresh = TagdustHip(0)
    try:
        with pytest.raises(TdError, match="no model"):
            fresh.upload_batch(g["seq"], g["offs"])
        with pytest.raises(TdError, match="no model"):
            fresh.run()
        bad = dict(g)
        bad["A"] = g["A"] * 0.5
        with pytest.raises(TdError, match="not 0/1|diagonal"):
            fresh.upload_model(bad)
        odd = dict(g)
        odd["n_hmm"] = g["n_hmm"] + 1          # sizes that do not add up to H / C
        with pytest.raises(TdError, match="inconsistent"):
            fresh.upload_model(odd)
        fresh.upload_model(g)
        with pytest.raises(TdError, match="unsupported mode"):
            fresh.upload_batch(g["seq"], g["offs"])
            fresh.run(3)
        with pytest.raises(TdError, match="unknown option"):
            fresh.set_option("no_such_option", 1)
    finally:
        fresh.close()


def test_model_reupload_uses_kernel_cache(ctx):
    """Uploading the same architecture again must not recompile (the code object is cached by source hash)."""
    import time
    g = load_golden("c3_b6_s_r_p")
    ctx.upload_model(g)
    t0 = time.perf_counter()
    ctx.upload_model(g)
    dt = time.perf_counter() - t0
    assert dt < 1.0, "re-upload took %.2f s" % dt


def test_long_reads(ctx):
    """400-bp reads (workspace and row strides scale with the batch's longest read); HIP == oracle."""
    from oracle import pyoracle
    g = load_golden("c2_b4_r")
    rng = np.random.RandomState(3)
    n = 200
    lens = rng.randint(250, 401, n)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seq = rng.randint(0, 4, int(offs[-1])).astype(np.uint8)
    src = g["offs"]
    for i in range(0, n, 2):
        seq[offs[i]:offs[i] + 4] = g["seq"][src[i]:src[i] + 4]     # a real barcode in front
    ores, olab, oseq = pyoracle.label_batch(pyoracle.OracleModel(g), seq, offs, float(g["threshold"]), 16, 100, 8)
    res, labels, seq_after = _run(ctx, g, seq, offs)
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), k
    assert np.array_equal(labels, olab) and np.array_equal(res["read_type"], ores["read_type"]) and np.array_equal(seq_after, oseq)


def test_read_without_valid_path_is_a_mismatch(ctx):
    """A read shorter than the number of mandatory segments has no valid path: b_score = -inf.  The reference then indexes
    its logsum table with NaN and crashes; the device reports ARCHITECTURE_MISMATCH with Q = 0 and the
    other reads of the batch are unaffected."""
    g = load_golden("c2_b4_r")
    n_good = 70
    good = [g["seq"][g["offs"][i]:g["offs"][i + 1]] for i in range(n_good)]
    reads = good[:35] + [np.array([2], np.uint8)] + good[35:]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    res, labels, seq_after = _run(ctx, g, np.concatenate(reads), offs)
    assert res["read_type"][35] == 1 and res["mapq"][35] == 0.0 and np.isneginf(res["b_score"][35])
    keep = np.r_[0:35, 36:n_good + 1]
    assert np.array_equal(res["read_type"][keep], g["read_type"][:n_good])
    assert np.array_equal(_bits(res["f_score"][keep]), _bits(g["f_score"][:n_good]))


def test_probe_reads_without_a_path(ctx):
    """The probe reads of a model with four mandatory segments (b_s_b_r): the generator pads its reads to 4 bases whatever the
    model, and a read of four bases or fewer has no path through four mandatory segments.  Decoded under the probe's fixed
    parameters, with reads of 1 .. 4 bases behind the 256 probe reads so that the rule is met whatever the generator drew: a read
    the oracle reports as without a path (its guard, oracle/td_oracle.c; the reference is undefined there) comes
    back as a mismatch with Q = 0 and b_score = -inf from both kernels; every other read agrees with the oracle in full."""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    g = load_golden("b_s_b_r")
    codes, offs = tdlib.spec_probe(g)
    n_probe = len(offs) - 1
    extra = [np.array([2, 0, 3, 1][:k], np.uint8) for k in (1, 2, 3, 4)]
    seq = np.concatenate([codes] + extra)
    offs = np.concatenate([offs, offs[-1] + np.cumsum([len(e) for e in extra])]).astype(np.int64)
    p = tdlib.spec_probe_params()
    ores, olab, oseq = pyoracle.label_batch(pyoracle.OracleModel(g), seq, offs, p["threshold"], p["minlen"], p["dust"], 4)
    nopath = np.isneginf(ores["b_score"])
    print("probe reads without a path:", int(nopath[:n_probe].sum()), "of", n_probe)
    assert nopath[:n_probe].sum() <= 8 and nopath[n_probe:].all()
    assert (ores["read_type"][nopath] == 1).all() and (ores["Q"][nopath] == 0.0).all()
    g2 = dict(g)
    g2.update(minlen=p["minlen"], dust=p["dust"])
    res, labels, seq_after = _run(ctx, g2, seq, offs, threshold=p["threshold"])
    assert (res["read_type"][nopath] == 1).all() and (res["mapq"][nopath] == 0.0).all() and np.isneginf(res["b_score"][nopath]).all()
    assert np.array_equal(seq_after, oseq)          # (a read without a path keeps its sequence)
    keep = ~nopath
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k][keep]), _bits(ores[k][keep])), k
    assert np.allclose(res["mapq"][keep], ores["Q"][keep], rtol=0, atol=Q_TOL)
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k][keep], ores[k][keep]), k
    lab_keep = np.concatenate([np.full(int(offs[i + 1] - offs[i]) + 1, keep[i]) for i in range(len(keep))])
    assert np.array_equal(labels[lab_keep], olab[lab_keep])


def test_long_reads_switch_to_clamped_logsum(monkeypatch):
    """The clamp-free logsum of the specialised kernel is only used while parameters x read length bound every score
    difference below the point where its LDS byte address would wrap; beyond that td_batch_upload reloads the kernel
    with the clamped form.  Forced here through the limit knob; results stay bit-exact either way."""
    from tagdust_amd import TagdustHip
    g = load_golden("c2_indel_varlen")
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 1)
        res0, labels0, seq0 = _run(c, g)
        assert c.get_option("spec_lsum_clamped") == 0
        c.set_option("spec_lsum_limit", 1)      # (TD_SPEC_LSUM_LIMIT is read when a context is created)
        res1, labels1, seq1 = _run(c, g)
        assert c.get_option("spec_lsum_clamped") == 1
    finally:
        c.close()
    for k in ("b_score", "f_score", "r_score", "bar_prob", "mapq"):
        assert np.array_equal(_bits(res0[k]), _bits(res1[k]))
    assert np.array_equal(labels0, labels1) and np.array_equal(labels0, g["labels"])
    assert np.array_equal(seq0, seq1) and np.array_equal(seq0, g["seq_after"])


def test_arch_scores_one_launch_for_all_candidates():
    """td_arch_scores: several candidate models over one (ragged) batch in a single launch of the generic kernel must give,
    per model, exactly the b_scores of a TD_MODE_ARCH_COMP run with that model alone -- and of the oracle."""
    from oracle import pyoracle
    from tagdust_amd import TagdustHip, MODE_ARCH_COMP
    names = ["c2_b4_r", "umi_f_s_r", "o_b_s_r", "scen2_endloss", "c3_b6_s_r_p", "b_intp_g_r", "c5_b96_f_r_p"]
    models = [load_golden(n_) for n_ in names]
    g = load_golden("c2_indel_varlen")
    seq, offs = g["seq"], g["offs"]
    c = TagdustHip(0)
    try:
        got = c.arch_scores(models, seq, offs)
        assert got.shape == (len(models), int(g["n_reads"]))
        c.set_option("specialize", 0)
        for k, m in enumerate(models):
            c.upload_model(m)
            c.set_params(0.0, 16, 100)
            c.upload_batch(seq, offs)
            c.run(MODE_ARCH_COMP)
            res, _, _ = c.download(labels=False, seq=False)
            assert np.array_equal(_bits(got[k]), _bits(res["b_score"])), names[k]
        ores = pyoracle.label_batch(pyoracle.OracleModel(models[0]), seq, offs, 0.0, 16, 100, 4)[0]
        assert np.array_equal(_bits(got[0]), _bits(ores["b_score"]))
        # many copies of one candidate: more models than fit the chip's wave slots at full width
        many = c.arch_scores([models[1]] * 40, seq, offs)
        assert all(np.array_equal(_bits(many[k]), _bits(got[1])) for k in range(40))
    finally:
        c.close()


def test_start_end_window_against_oracle(ctx):
    """-start / -end: do_label_thread / do_probability_estimation decode seq + matchstart for matchend - matchstart bases
    (barcode_hmm.c:2195-2210, :2290-2313) and the rewrite then walks the whole read (:3325-3356).  With td_set_window the
    device does the same in every mode; results equal the oracle's window path (itself pinned by the reference fixture
    window_b_r) bit for bit, for uniform and ragged batches -- a read that ends inside the window is decoded on what it has
    there (the reference's behaviour for such reads is undefined)."""
    from oracle import pyoracle
    from tagdust_amd import MODE_GET_PROB, MODE_ARCH_COMP
    g = load_golden("c2_b4_r")
    om = pyoracle.OracleModel(g)
    rng = np.random.RandomState(21)
    n = 500
    for ragged in (False, True):
        lens = rng.randint(40, 101, n) if ragged else np.full(n, 100)
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        seq = rng.randint(0, 4, int(offs[-1])).astype(np.uint8)
        seq[rng.random_sample(len(seq)) < 0.004] = 4
        src = g["offs"]
        for i in range(0, n, 2):
            k = i % int(g["n_reads"])
            s_ = g["seq"][src[k]:src[k + 1]][:lens[i] - 3]
            seq[offs[i] + 3:offs[i] + 3 + len(s_)] = s_                     # the architecture starts at base 3
        start, end = 3, 63
        ores, olab, oseq = pyoracle.label_batch(om, seq, offs, float(g["threshold"]), 16, 100, 8, window=(start, end))
        assert len(set(ores["read_type"].tolist())) >= 2
        ctx.upload_model(g)
        ctx.set_params(float(g["threshold"]), 16, 100)
        ctx.set_window(start, end)
        try:
            ctx.upload_batch(seq, offs)
            ctx.run()
            res, labels, seq_after = ctx.download()
            for k in ("b_score", "f_score", "r_score", "bar_prob"):
                assert np.array_equal(_bits(res[k]), _bits(ores[k])), (k, ragged)
            assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL)
            assert np.array_equal(labels, olab), ragged
            for k in ("read_type", "barcode", "fingerprint"):
                assert np.array_equal(res[k], ores[k]), (k, ragged)
            assert np.array_equal(seq_after, oseq), ragged
            ctx.run(MODE_GET_PROB)
            res2, _, _ = ctx.download(labels=False, seq=False)
            assert np.array_equal(_bits(res2["f_score"]), _bits(ores["f_score"])) and np.allclose(res2["mapq"], ores["Q"], rtol=0, atol=Q_TOL)
            ctx.run(MODE_ARCH_COMP)
            res3, _, _ = ctx.download(labels=False, seq=False)
            assert np.array_equal(_bits(res3["b_score"]), _bits(ores["b_score"]))
        finally:
            ctx.set_window(-1, -1)
    ctx.upload_batch(g["seq"], g["offs"])          # back to whole reads
    ctx.run()
    res, labels, _ = ctx.download()
    assert np.array_equal(labels, g["labels"])


def test_logsum_selfcheck_falls_back_to_clamped_form(monkeypatch, capfd):
    """Every load of a compiled kernel runs lsum() over the operand pairs that matter (-inf operands, gaps around the 15.7
    cut, huge gaps) against the reference's formula; a failing clamp-free form must be replaced by the clamped one, with a
    message, and the results stay bit-exact.  The failure is forced through TD_SPEC_SELFCHECK_FAIL."""
    from tagdust_amd import TagdustHip
    g = load_golden("c2_b4_r")
    monkeypatch.setenv("TD_SPEC_EXTRA_OPTS", "-DTD_TEST_UNIQUE_KEY=1")   # a cache key of its own: not served from the in-memory cache
    monkeypatch.setenv("TD_SPEC_SELFCHECK_FAIL", "1")
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 1)
        res, labels, seq = _run(c, g)
        assert c.get_option("spec_lsum_clamped") == 1
    finally:
        c.close()
    assert "self-check" in capfd.readouterr().err
    assert np.array_equal(labels, g["labels"]) and np.array_equal(seq, g["seq_after"])
    assert np.array_equal(_bits(res["f_score"]), _bits(g["f_score"]))
    monkeypatch.delenv("TD_SPEC_SELFCHECK_FAIL")
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 1)
        _run(c, g)
        assert c.get_option("spec_lsum_clamped") == 0      # the real self-check passes on gfx950
    finally:
        c.close()


@pytest.mark.parametrize("workload,n", [("c3", 1 << 20), ("c2", 1 << 20), ("c5", 1 << 19)], ids=["config3", "config2", "config5"])
def test_full_size_batch_properties(workload, n):
    """BASELINE.json's shapes at full batch size (2^20 reads; 2^19 for the 100-HMM architecture of configs[4], whose
    workspace is 42 MiB per wave): the oracle cannot cover a million reads in seconds, so the batch is checked through
    properties that do not depend on its size -- a batch decodes like its permutation, like its halves, and like itself
    a second time (through the pipelined calls as well); the device counters add up -- and, since round 4, the WHOLE batch is
    compared with the oracle (all 2^20 reads of configs 2 and 3, 2^15 of config 5)."""
    import bench
    from oracle import pyoracle
    from tagdust_amd import TagdustHip, RESULT_DTYPE
    bench.select_workload(workload)
    model = bench.load_model()
    L = bench.READ_LEN
    reads = bench.synth_batch(n, 20240607).reshape(n, L)
    offs = np.arange(n + 1, dtype=np.int64) * L
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 1)
        c.upload_model(model)
        c.set_params(float(model["threshold"]), int(model["minlen"]), int(model["dust"]))

        def decode(r):
            c.upload_batch(r.reshape(-1), np.arange(len(r) + 1, dtype=np.int64) * L)
            c.counts_reset()
            c.run()
            return c.download() + (c.counts(),)

        res, labels, seq, cnt = decode(reads)
        # the fast paths this model / batch is meant to get are the ones it got
        assert c.get_option("prune_active") == 1 and c.get_option("spec_lsum_clamped") == 0
        # counters == serial counting over the results
        assert int(cnt[:8].sum()) == n
        for code in range(8):
            assert cnt[code] == int(((res["read_type"] & 0xFF) == code).sum())
        ok = (res["read_type"] == 0) & (res["barcode"] >= 0)
        assert np.array_equal(cnt[8:], np.bincount(res["barcode"][ok] & 0xFF, minlength=256))
        assert 0.75 * n < cnt[0] < 0.97 * n                                 # ~90 % of the synthetic reads carry the architecture
        # idempotence, and the pipelined calls give the same bytes
        res2 = np.zeros(n, RESULT_DTYPE)
        labels2 = np.zeros(n * (L + 1), np.int8)
        seq2 = np.zeros(n * L, np.uint8)
        c.wait(c.submit(np.ascontiguousarray(reads.reshape(-1)), offs, res=res2, labels=labels2, seq_out=seq2))
        if workload != "c5":      # (config 5 at this size: HBM holds one 150 GB workspace, not two)
            c.wait(c.submit(np.ascontiguousarray(reads.reshape(-1)), offs, res=res2, labels=labels2, seq_out=seq2))   # second stream
            assert c.get_option("overlap_active") == 1
        assert res.tobytes() == res2.tobytes() and np.array_equal(labels, labels2) and np.array_equal(seq, seq2)
        # permutation: tiles hold 64 neighbours; a read must not care who they are
        perm = np.random.default_rng(5).permutation(n)
        resp, labelsp, seqp, cntp = decode(reads[perm])
        assert resp.tobytes() == res[perm].tobytes()
        assert np.array_equal(labelsp.reshape(n, L + 1), labels.reshape(n, L + 1)[perm])
        assert np.array_equal(seqp.reshape(n, L), seq.reshape(n, L)[perm])
        assert np.array_equal(cntp, cnt)
        # halves
        h = n // 2
        ra, la, sa, ca = decode(reads[:h])
        rb, lb, sb, cb = decode(reads[h:])
        assert ra.tobytes() + rb.tobytes() == res.tobytes()
        assert np.array_equal(np.concatenate([la, lb]), labels) and np.array_equal(np.concatenate([sa, sb]), seq)
        assert np.array_equal(ca + cb, cnt)
    finally:
        c.close()
        bench.select_workload("c3")
    # ... and against the oracle, bit for bit, on EVERY read of the batch for configs 2 and 3 (the restatement decodes ~65 k
    # config-3 reads a second on the box's 16 host threads: 16 s), on the first 2^15 reads for the 100-HMM architecture (eight times
    # the work per read).  The pruning and restart fall-backs are rare, data-dependent events: a sample does not meet them, the
    # whole batch does.  Counters == serial counting over the oracle's outcomes (barcode_hmm.c:354-384).
    no = n if workload != "c5" else 1 << 15
    om = pyoracle.OracleModel(model)
    ores, olab, oseq = pyoracle.label_batch(om, reads[:no].reshape(-1), offs[:no + 1], float(model["threshold"]),
                                            int(model["minlen"]), int(model["dust"]), n_threads=16)
    for k, ok_ in (("b_score", "b_score"), ("f_score", "f_score"), ("r_score", "r_score"), ("bar_prob", "bar_prob"), ("mapq", "Q")):
        assert np.array_equal(_bits(res[k][:no]), _bits(ores[ok_])), k
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k][:no], ores[k]), k
    assert np.array_equal(labels[:no * (L + 1)], olab)
    assert np.array_equal(seq[:no * L], oseq)
    if no == n:
        for code in range(8):
            assert cnt[code] == int(((ores["read_type"] & 0xFF) == code).sum())
        oko = (ores["read_type"] == 0) & (ores["barcode"] >= 0)
        assert np.array_equal(cnt[8:], np.bincount(ores["barcode"][oko] & 0xFF, minlength=256))


def test_disk_cache_of_compiled_kernels(tmp_path, monkeypatch):
    """TD_SPEC_CACHE_DIR: the code object of an architecture is written once (atomically) and a later process -- here a
    second context after the in-memory cache has been bypassed by a different directory -- loads it instead of compiling."""
    import os
    from tagdust_amd import TagdustHip
    g = load_golden("umi_f_s_r")
    monkeypatch.setenv("TD_SPEC_CACHE_DIR", str(tmp_path))
    monkeypatch.setenv("TD_SPEC_EXTRA_OPTS", "-DTD_TEST_UNIQUE_KEY=2")   # a cache key no other test compiled: not in the
                                                                          # in-memory cache of this process
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 1)
        res, labels, seq = _run(c, g)
    finally:
        c.close()
    files = [f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]
    assert len(files) == 1 and not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]
    assert np.array_equal(labels, g["labels"])
    # the file alone must be enough: same bytes through a copy in another directory, in-memory cache has this key already,
    # so check the loader by reading the file back and comparing with what a fresh compile would produce
    blob = open(os.path.join(tmp_path, files[0]), "rb").read()
    assert blob[:4] == b"\x7fELF" and len(blob) > 10000


def _random_arch(rng):
    """A random read architecture in the reference's -1 .. -k segment syntax, with reads that (mostly) follow it."""
    def dna(n):
        return "".join("ACGT"[x] for x in rng.randint(0, 4, n))
    segs, parts = [], []            # parts: callables producing the segment's text for one read
    if rng.random_sample() < 0.3:
        segs.append("O:N"); parts.append(lambda: dna(rng.randint(0, 4)))
    if rng.random_sample() < 0.4:
        p5 = dna(rng.randint(4, 16)); segs.append("P:" + p5); parts.append(lambda p5=p5: p5[rng.randint(0, len(p5)):])
    nb = int(rng.choice([0, 2, 5, 9, 20, 30]))          # 20 / 30: run-time HMM loop and the H > 32 label path
    if nb:
        L = int(rng.randint(4, 8))
        bars = sorted({dna(L) for _ in range(nb)})
        segs.append("B:" + ",".join(bars)); parts.append(lambda bars=bars: bars[rng.randint(len(bars))])
    if rng.random_sample() < 0.4:
        nf = int(rng.randint(4, 9)); segs.append("F:" + "N" * nf); parts.append(lambda nf=nf: dna(nf))
    if rng.random_sample() < 0.4:
        sp = dna(rng.randint(2, 5)); segs.append("S:" + sp); parts.append(lambda sp=sp: sp)
    if rng.random_sample() < 0.2:
        segs.append("G:G"); parts.append(lambda: "G" * rng.randint(0, 4))
    segs.append("R:N"); parts.append(lambda: dna(rng.randint(18, 70)))
    if rng.random_sample() < 0.5:
        p3 = dna(rng.randint(5, 24)); segs.append("P:" + p3); parts.append(lambda p3=p3: p3[:rng.randint(0, len(p3) + 1)])
    return segs, parts


_FUZZ_SEEDS = list(range(20))
if os.environ.get("TD_FUZZ_SEEDS"):      # e.g. TD_FUZZ_SEEDS=100:180 for a longer one-off run
    _a, _b = os.environ["TD_FUZZ_SEEDS"].split(":")
    _FUZZ_SEEDS = list(range(int(_a), int(_b)))


def _random_case(seed):
    """Segments, 400 reads, the builder's model with its decode parameters, artifact filter (or None) and thread count of one seed
    of the tag fuzz (also read by tools/plan_survey.py)."""
    from tagdust_amd import lib as tdlib
    rng = np.random.RandomState(1000 + seed)
    segs, parts = _random_arch(rng)
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
    reads = []
    for i in range(400):
        s_ = "".join(p() for p in parts)
        out = []
        for ch in s_:
            u = rng.random_sample()
            if u < 0.02:
                out.append("ACGT"[rng.randint(4)])
            elif u < 0.03:
                continue
            elif u < 0.04:
                out.append(ch); out.append("ACGT"[rng.randint(4)])
            elif u < 0.045:
                out.append("N")
            else:
                out.append(ch)
        s_ = "".join(out)
        # (reads too short to have any path through the model are left out: the reference -- and with it the oracle --
        # indexes its logsum table with a NaN there and crashes; the device's own rule for them is tested separately)
        if rng.random_sample() < 0.1 or len(s_) < 12:
            s_ = "".join("ACGT"[x] for x in rng.randint(0, 4, rng.randint(12, 90)))
        reads.append(np.array([code[ch] for ch in s_], np.uint8))
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    seq = np.concatenate(reads)
    md, _ = tdlib.build_model(segs, seq, offs, 0.05, 0.1)
    thr = float(rng.choice([0.0, 1.5, 8.0]))
    md.update(threshold=thr, minlen=int(rng.choice([8, 16])), dust=int(rng.choice([0, 100, 20])))
    art, nthreads = None, 8
    if seed % 3 == 1:   # an artifact filter on top: random sequences (some of them windows of reads), -fe, thread count
        texts = []
        for j in range(int(rng.randint(1, 5))):
            if rng.random_sample() < 0.5:
                r0 = reads[rng.randint(len(reads))]
                texts.append(np.minimum(r0[-40:], 3))
            else:
                texts.append(rng.randint(0, 4, rng.randint(20, 120)).astype(np.uint8))
        a_index = np.concatenate([[0], np.cumsum([len(t_) + 1 for t_ in texts])]).astype(np.int32)
        a_string = np.concatenate([np.concatenate([[ord("X")], t_]) for t_ in texts]).astype(np.uint8)
        nthreads = int(rng.randint(1, 6))
        art = (a_string, a_index, int(rng.randint(2, 14)))
        md["art_n"], md["art_string"], md["art_index"] = len(texts), a_string, a_index
        md["art_filter_error"], md["art_threads"] = art[2], nthreads
    return segs, seq, offs, md, art, nthreads


@pytest.mark.parametrize("seed", _FUZZ_SEEDS)
def test_random_architectures_against_oracle(ctx, seed):
    """Model shapes beyond the fixtures: random segment lists (optional / partial / barcode / fingerprint / spacer / G /
    read segments of random sizes), models from the library's own builder, reads with substitutions, indels, Ns and a
    share of unrelated sequences; both kernels must equal the oracle bit for bit."""
    from oracle import pyoracle
    segs, seq, offs, md, art, nthreads = _random_case(seed)
    thr = float(md["threshold"])
    ores, olab, oseq = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, int(md["minlen"]), int(md["dust"]),
                                            nthreads, artifacts=art)
    res, labels, seq_after = _run(ctx, md, seq, offs, threshold=thr)
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), (k, segs)
    assert np.array_equal(labels, olab), segs
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL), segs
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), (k, segs)
    assert np.array_equal(seq_after, oseq), segs


def _free_order_arch(rng):
    """A random architecture whose segments come in ANY order (beside _random_arch, whose tags all sit in front of its one read
    segment and whose random stream the committed seeds are bound to): 0-2 read segments, 0-2 barcode segments, 0-2 fingerprints,
    spacer / partial / optional / G segments, shuffled -- two B, two F (up to 32 fingerprint bases: the 32-bit key wraps), tags 3'
    of the read segment, no read segment at all, two read segments around tags.  (segs, parts): parts[j](rng-driven) gives the
    text of segment j for one read."""
    def dna(n):
        return "".join("ACGT"[x] for x in rng.randint(0, 4, n))
    segs, parts = [], []
    for _ in range(int(rng.choice(3, p=[0.2, 0.6, 0.2]))):
        segs.append("R:N"); parts.append(lambda: dna(rng.randint(10, 46)))
    for _ in range(int(rng.choice(3, p=[0.25, 0.5, 0.25]))):
        L = int(rng.randint(4, 8))
        bars = sorted({dna(L) for _ in range(int(rng.choice([2, 3, 5, 9])))})
        # a random k-mer in place of the barcode in one read in ten
        segs.append("B:" + ",".join(bars))
        parts.append(lambda bars=bars, L=L: dna(L) if rng.random_sample() < 0.1 else bars[rng.randint(len(bars))])
    for _ in range(int(rng.choice(3, p=[0.5, 0.25, 0.25]))):
        nf = int(rng.choice([4, 6, 8, 12, 13, 16]))
        # a UMI one base off in 15 % of the reads
        segs.append("F:" + "N" * nf)
        parts.append(lambda nf=nf: dna(nf + (int(rng.choice([-1, 1])) if rng.random_sample() < 0.15 else 0)))
    if rng.random_sample() < 0.5:
        sp = dna(rng.randint(2, 7)); segs.append("S:" + sp); parts.append(lambda sp=sp: sp)
    if rng.random_sample() < 0.4:
        pp = dna(rng.randint(5, 17)); segs.append("P:" + pp)
        parts.append(lambda pp=pp: pp[rng.randint(0, len(pp)):] if rng.random_sample() < 0.5 else pp[:rng.randint(0, len(pp) + 1)])
    if rng.random_sample() < 0.2:
        segs.append("O:N"); parts.append(lambda: dna(rng.randint(0, 4)))
    if rng.random_sample() < 0.2:
        segs.append("G:G"); parts.append(lambda: "G" * rng.randint(0, 4))
    if not segs:
        bars = sorted({dna(6) for _ in range(5)})
        segs.append("B:" + ",".join(bars)); parts.append(lambda bars=bars: bars[rng.randint(len(bars))])
    while True:
        order = rng.permutation(len(segs))
        if not any(segs[order[i]] == "R:N" and segs[order[i + 1]] == "R:N" for i in range(len(order) - 1)):
            break
    return [segs[i] for i in order], [parts[i] for i in order]


def _free_order_case(seed):
    """Segments, 200 reads, the builder's model and the decode parameters of one free-order fuzz seed.  Reads follow the
    segments, go through the mutation loop of test_random_architectures_against_oracle, and are replaced by a uniform random read
    of floor .. 89 bases (floor = number of segments + 6) with p = 0.1 or when they came out shorter than floor: no read is
    without a path through the model (those have a test of their own, test_probe_reads_without_a_path)."""
    from tagdust_amd import lib as tdlib
    rng = np.random.RandomState(20000 + seed)
    segs, parts = _free_order_arch(rng)
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
    floor = len(segs) + 6
    reads = []
    for i in range(200):
        s_ = "".join(p() for p in parts)
        out = []
        for ch in s_:
            u = rng.random_sample()
            if u < 0.02:
                out.append("ACGT"[rng.randint(4)])
            elif u < 0.03:
                continue
            elif u < 0.04:
                out.append(ch); out.append("ACGT"[rng.randint(4)])
            elif u < 0.045:
                out.append("N")
            else:
                out.append(ch)
        s_ = "".join(out)
        if rng.random_sample() < 0.1 or len(s_) < floor:
            s_ = "".join("ACGT"[x] for x in rng.randint(0, 4, rng.randint(floor, 90)))
        reads.append(np.array([code[ch] for ch in s_], np.uint8))
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    seq = np.concatenate(reads)
    md, _ = tdlib.build_model(segs, seq, offs, 0.05, 0.1)
    thr = float(rng.choice([0.0, 1.5, 8.0]))
    md.update(threshold=thr, minlen=int(rng.choice([8, 16])), dust=int(rng.choice([0, 100, 20])))
    return segs, seq, offs, md


# chosen on the CPU (generator + oracle) so that the conditions of tests/test_free_order.py hold: two outcomes with five reads each
# for every seed; between them two B segments, tags behind the read segment, no read segment, two F, 13 or more fingerprint
# bases, two read segments
_FREE_ORDER_SEEDS = [7, 11, 13, 17, 34, 36]
if os.environ.get("TD_FREE_ORDER_SEEDS"):      # e.g. TD_FREE_ORDER_SEEDS=100:180 for a longer one-off run
    _a, _b = os.environ["TD_FREE_ORDER_SEEDS"].split(":")
    _FREE_ORDER_SEEDS = list(range(int(_a), int(_b)))


@pytest.mark.parametrize("seed", _FREE_ORDER_SEEDS)
def test_free_order_architectures_against_oracle(ctx, seed):
    """Segment lists in any order (_free_order_arch): the specialised kernel's plan -- first-segment labels, label runs, pruned
    leading and trailing segments, restarts -- and both kernels' restatement of extract_reads on orders no fixture follows.
    Both kernels equal the oracle bit for bit; the device counters equal serial counting."""
    from oracle import pyoracle
    segs, seq, offs, md = _free_order_case(seed)
    thr = float(md["threshold"])
    ores, olab, oseq = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, int(md["minlen"]), int(md["dust"]), 8)
    assert np.isfinite(ores["b_score"]).all(), segs
    res, labels, seq_after = _run(ctx, md, seq, offs, threshold=thr)
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), (k, segs)
    assert np.array_equal(labels, olab), segs
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL), segs
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), (k, segs)
    assert np.array_equal(seq_after, oseq), segs
    cnt = ctx.counts()
    for c_ in range(8):
        assert cnt[c_] == int(((ores["read_type"] & 0xFF) == c_).sum()), (c_, segs)
    ok = (ores["read_type"] == 0) & (ores["barcode"] >= 0)
    assert np.array_equal(cnt[8:], np.bincount(ores["barcode"][ok] & 0xFF, minlength=256)), segs


# The windowed fuzz: (generator, seed, (matchstart, matchend), artifact filter (thread count, -fe) or None), chosen on the CPU
# (generator + oracle) so that the conditions of tests/test_window_cases.py hold -- per case two outcomes with five reads each, 20
# reads that end inside the window, 8 reads without a path or without a base in the window; between them what each is there for:
_WINDOW_CASES = [
    ("free", 5, (0, 70), (3, 20)),    # R B R: a read segment first (the tail is kept), two read segments, artifact filter on 3 threads
    ("free", 13, (5, 75), None),      # R P F F: a read segment first, 24 fingerprint bases inside the window
    ("free", 17, (5, 104), None),     # R B P S F R: six segments, two read segments, F behind an internal P
    ("free", 10, (5, 15), None),      # S B: no read segment, a window of 10 bases
    ("tags", 15, (5, 37), None),      # B F S R: the window ends inside the read segment of most reads
    ("tags", 14, (5, 60), None),      # P B S R with 30 barcodes: more than 32 labels, 5' P pruned
    ("tags", 9, (5, 48), (2, 14)),    # B R: artifact filter on 2 threads, DUST
    ("tags", 2, (9, 60), (5, 24)),    # B F R P: a 3' P segment that the window cuts, artifact filter on 5 threads, matchstart 9
]


def _windowed_case(case):
    """Segments, reads, the builder's model (its statistics taken under the window, as the reference takes them), decode parameters
    and artifact filter of one case of the windowed fuzz.  200 reads follow the segments behind `matchstart` random bases and go
    through the mutation loop of the other fuzz tests with N at 0.5 % of the positions; one in ten is replaced by an unrelated read,
    one in sixteen turns low-complexity behind its first 12 bases; about a third is cut to end inside the window and about a third
    padded to run past matchend, none shorter than matchstart + segments + 2.  12 more reads of 1, matchstart, matchstart + 1, ..
    matchstart + segments + 1 bases are spread over the batch: no base in the window, or no path through the model."""
    from tagdust_amd import lib as tdlib
    gen, seed, (ms, me), art = case
    rng = np.random.RandomState(30000 + seed)
    segs, parts = (_random_arch if gen == "tags" else _free_order_arch)(rng)

    def dna(n):
        return "".join("ACGT"[x] for x in rng.randint(0, 4, n))
    floor = ms + len(segs) + 2
    assert floor < me
    reads = []
    for i in range(200):
        s_ = "".join(p() for p in parts)
        out = []
        for ch in s_:
            u = rng.random_sample()
            if u < 0.02:
                out.append("ACGT"[rng.randint(4)])
            elif u < 0.03:
                continue
            elif u < 0.04:
                out.append(ch); out.append("ACGT"[rng.randint(4)])
            elif u < 0.045:
                out.append("N")
            else:
                out.append(ch)
        s_ = dna(ms) + "".join(out)
        if rng.random_sample() < 0.1:
            s_ = dna(len(s_))
        if rng.random_sample() < 1.0 / 16:
            s_ = s_[:12] + (dna(int(rng.randint(1, 4))) * 100)[:max(len(s_) - 12, 30)]
        u = rng.random_sample()
        if u < 1.0 / 3:      # ends inside the window
            s_ = (s_ + dna(me))[:int(rng.randint(floor, me))]
        elif u < 2.0 / 3:    # runs past matchend
            s_ = s_ + dna(max(0, int(rng.randint(me + 1, me + 31)) - len(s_)))
        elif len(s_) < floor:
            s_ = s_ + dna(floor - len(s_))
        reads.append(s_)
    short = [n_ for n_ in [1] + list(range(ms, floor)) if n_ >= 1]
    for k in range(12):
        reads.insert(int(rng.randint(0, len(reads) + 1)), dna(short[k % len(short)]))
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
    reads = [np.array([code[ch] for ch in s_], np.uint8) for s_ in reads]
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    seq = np.concatenate(reads)
    md, _ = tdlib.build_model(segs, seq, offs, 0.05, 0.1, window=(ms, me))
    md.update(threshold=float(rng.choice([0.0, 1.5, 8.0])), minlen=int(rng.choice([8, 16])), dust=int(rng.choice([0, 100, 20])))
    artifacts, nthreads = None, 8
    if art:                  # texts partly cut from the reads (as the filter sees them: the start of a read), -fe, thread count; DUST on
        nthreads, fe = art
        texts = []
        for j in range(4):
            r0 = reads[int(rng.randint(len(reads)))]
            texts.append(np.minimum(r0[:60], 3) if j < 3 else rng.randint(0, 4, 80).astype(np.uint8))
        a_index = np.concatenate([[0], np.cumsum([len(t_) + 1 for t_ in texts])]).astype(np.int32)
        a_string = np.concatenate([np.concatenate([[ord("X")], t_]) for t_ in texts]).astype(np.uint8)
        artifacts = (a_string, a_index, fe)
        md.update(dust=20)
    return segs, seq, offs, md, artifacts, nthreads


_WINDOW_ORACLE = {}


def _windowed_oracle(case):
    """_windowed_case(case) and the oracle's results for it, computed once for both kernels (and for tests/test_window_cases.py)"""
    from oracle import pyoracle
    if case not in _WINDOW_ORACLE:
        segs, seq, offs, md, artifacts, nthreads = _windowed_case(case)
        o = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, float(md["threshold"]), int(md["minlen"]), int(md["dust"]),
                                 nthreads, artifacts=artifacts, window=case[2])
        for a in o:
            a.setflags(write=False)
        _WINDOW_ORACLE[case] = (segs, seq, offs, md, artifacts, nthreads) + o
    return _WINDOW_ORACLE[case]


@pytest.mark.parametrize("case", _WINDOW_CASES, ids=["%s%d-%d-%d" % (c[0], c[1], c[2][0], c[2][1]) for c in _WINDOW_CASES])
def test_windowed_architectures_against_oracle(ctx, case):
    """-start / -end (td_set_window) over architecture shapes: the specialised kernel's TDS_WINDOW variant -- unpack loop, random
    model, zeroed labels behind the window, label runs, extraction and everything behind it on the whole read -- and the generic
    kernel's window branches, on read segments first (the tail behind matchend is kept), F / P / S / G / O segments, pruned
    segments, more than 32 labels, two read segments, no read segment, an artifact filter; reads that end inside the window, reads
    without a base in it and reads without a path (for which the oracle's guard states the device's rule: mismatch, Q = 0,
    b_score = -inf, the sequence as it was).  The window is set before the model is uploaded: one specialised kernel per case.
    Label run, then MODE_GET_PROB and MODE_ARCH_COMP on the resident batch.  Both kernels equal the oracle bit for bit; the device
    counters equal td_count_outcomes over the oracle's results."""
    from tagdust_amd import lib as tdlib, MODE_GET_PROB, MODE_ARCH_COMP, RESULT_DTYPE
    segs, seq, offs, md, artifacts, nthreads, ores, olab, oseq = _windowed_oracle(case)
    if artifacts:
        ctx.set_artifacts(artifacts[0], artifacts[1], artifacts[2], nthreads)
    else:
        ctx.set_artifacts(None)
    ctx.set_window(*case[2])
    try:
        ctx.upload_model(md)
        ctx.set_params(float(md["threshold"]), int(md["minlen"]), int(md["dust"]))
        ctx.upload_batch(seq, offs)
        ctx.counts_reset()
        ctx.run()
        res, labels, seq_after = ctx.download()
        cnt = ctx.counts()
        ctx.run(MODE_GET_PROB)
        res2, _, _ = ctx.download(labels=False, seq=False)
        ctx.run(MODE_ARCH_COMP)
        res3, _, _ = ctx.download(labels=False, seq=False)
    finally:
        ctx.set_window(-1, -1)
        ctx.set_artifacts(None)
    nopath = np.isneginf(ores["b_score"])
    keep = ~nopath
    assert np.array_equal(_bits(res["b_score"]), _bits(ores["b_score"])), segs
    for k in ("f_score", "r_score", "bar_prob"):      # (a read without a path has b_score = -inf; its other scores mean nothing)
        assert np.array_equal(_bits(res[k][keep]), _bits(ores[k][keep])), (k, segs)
    assert (res["mapq"][nopath] == 0.0).all()
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL), segs
    lab_keep = np.repeat(keep, np.diff(offs) + 1)
    assert np.array_equal(labels[lab_keep], olab[lab_keep]), segs
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), (k, segs)
    assert np.array_equal(seq_after, oseq), segs
    as_res = np.zeros(len(ores), RESULT_DTYPE)
    for k in ("read_type", "barcode", "fingerprint"):
        as_res[k] = ores[k]
    assert np.array_equal(cnt, tdlib.count_outcomes(as_res, np.diff(offs))), segs
    assert np.array_equal(_bits(res2["f_score"][keep]), _bits(ores["f_score"][keep])), segs
    assert np.allclose(res2["mapq"], ores["Q"], rtol=0, atol=Q_TOL), segs
    assert np.array_equal(_bits(res3["b_score"]), _bits(ores["b_score"])), segs


_MANY_LABEL_CASES = [(60, False, True), (96, False, True), (96, True, False), (62, True, True), (97, False, False)]


def _many_label_case(nb, linker_first, umi):
    """Segments, 330 reads and the builder's model (threshold 1.0, minlen 16, dust 100) of one many-label architecture (also read by
    tools/plan_survey.py)."""
    from tagdust_amd import lib as tdlib
    rng = np.random.RandomState(4000 + nb + 7 * linker_first)

    def dna(n):
        return "".join("ACGT"[x] for x in rng.randint(0, 4, n))
    bars = sorted({dna(6) for _ in range(4 * nb)})[:nb]
    assert len(bars) == nb
    five = "ACGTTGCATCGG"
    three = "AGATCGGAAGAGC"
    segs = (["P:" + five] if linker_first else []) + ["B:" + ",".join(bars)] + (["F:NNNNNNNN"] if umi else []) + ["R:N"]
    if nb != 97:
        segs.append("P:" + three)
    code = {"A": 0, "C": 1, "G": 2, "T": 3, "N": 4}
    reads = []
    for i in range(330):
        kind = rng.randint(10)
        b = bars[rng.randint(nb)] if kind != 1 else dna(6)
        u = dna(8 if kind != 2 else int(rng.choice([6, 7, 9]))) if umi else ""
        ins = dna(int(rng.randint(20, 70)) if kind != 3 else int(rng.randint(2, 14)))
        s_ = (five[rng.randint(0, len(five)):] if linker_first else "") + b + u + ins
        if nb != 97:
            s_ += three[:rng.randint(0, len(three) + 1)] if kind != 3 else three
        out = []
        for ch in s_:
            v = rng.random_sample()
            if v < 0.02:
                out.append("ACGT"[rng.randint(4)])
            elif v < 0.025:
                continue
            elif v < 0.03:
                out.append(ch); out.append("ACGT"[rng.randint(4)])
            elif v < 0.033:
                out.append("N")
            else:
                out.append(ch)
        s_ = "".join(out)
        if kind == 4:
            s_ = dna(int(rng.randint(20, 100)))
        reads.append(np.array([code[ch] for ch in s_], np.uint8))
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    seq = np.concatenate(reads)
    md, _ = tdlib.build_model(segs, seq, offs, 0.05, 0.1)
    assert int(md["H"]) == nb + 1 + (1 if umi else 0) + 1 + (1 if nb != 97 else 0) + (1 if linker_first else 0)
    md.update(threshold=1.0, minlen=16, dust=100)
    return segs, seq, offs, md


@pytest.mark.parametrize("nb,linker_first,umi", _MANY_LABEL_CASES,
                         ids=["H64-first", "H100-first", "H100-behind-5p-linker", "H67-behind-5p-linker", "H99-b97-r"])
def test_many_label_architectures_against_oracle(ctx, nb, linker_first, umi):
    """Architectures at and near the reference's limit of 100 HMMs (total_prob[100], barcode_hmm.c:4186): the run-time HMM
    loop, the workspace label DP (:4447-4472 over > 32 labels) and -- with the big segment first -- the in-sweep label sums,
    and with a 5' linker in front of it the run-wise label DP.  Models from the library's own builder; reads with
    substitutions, indels, Ns, wrong-length UMIs, non-barcodes, short inserts and unrelated sequences; both kernels equal the
    oracle bit for bit."""
    from oracle import pyoracle
    segs, seq, offs, md = _many_label_case(nb, linker_first, umi)
    thr = 1.0
    ores, olab, oseq = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, 16, 100, 16)
    assert len(set(ores["read_type"].tolist())) >= 3
    res, labels, seq_after = _run(ctx, md, seq, offs, threshold=thr)
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), (k, segs[0][:12])
    assert np.array_equal(labels, olab)
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL)
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), k
    assert np.array_equal(seq_after, oseq)


@pytest.mark.parametrize("name", ["c2_b4_r", "c3_b6_s_r_p", "scen2_p_b_r_p", "c2_indel_varlen", "b_r_s_r"])
def test_first_segment_label_sums_forced(name, monkeypatch):
    """The forward sweep can sum the posteriors of predecessor-free first-segment labels itself (used automatically for
    models with more than 32 labels, e.g. config 5); forced on here for small models so that the scheme is covered on
    the register path of the label DP as well."""
    from tagdust_amd import TagdustHip
    monkeypatch.setenv("TD_SPEC_FIRSTSEG", "1")
    g = load_golden(name)
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 1)
        res, labels, seq_after = _run(c, g)
    finally:
        c.close()
    assert np.array_equal(labels, g["labels"])
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], g[k]), k
    assert np.array_equal(seq_after, g["seq_after"])
    assert np.array_equal(_bits(res["f_score"]), _bits(g["f_score"]))
