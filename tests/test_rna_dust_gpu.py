"""run_rna_dust on the device (TD_MODE_RNA_DUST, td_rnadust.hip) and -ref in multi-file runs (td_stream_run_multi).

The reference's controller hands its -ref FASTA to every file's step: run_pHMM for a decoded file, run_rna_dust for an R:N file
(src/barcode_hmm.c:209-214, :313-325).  do_rna_dust (:2370-2395) sets EXTRACT_SUCCESS, runs match_to_reference over the thread
ranges of the batch, then DUST, which overwrites the outcome.  These tests hold the device path against the unmodified reference
binary, against the host path it replaces, and against the oracle's restatement of match_to_reference."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden

RBIN = os.path.join(REPO, "oracle", "_ref")
ALPHA = np.frombuffer(b"ACGTN", np.uint8)
COMP = np.array([3, 2, 1, 0, 4], np.uint8)


def _files(d, prefix):
    return {os.path.basename(p)[len(prefix):]: open(p, "rb").read() for p in sorted(glob.glob(os.path.join(d, prefix + "*.fq")))}


def _log_counts(path):
    out = {}
    for line in open(path).read().splitlines():
        f = line.split("\t")
        if len(f) >= 3 and f[1].strip().isdigit():      # (the percentage lines have other names)
            out[f[2].strip()] = int(f[1].strip())
    return out


def _artifacts(rng, n=12):
    """Seeded random artifact sequences of 90-160 nt, plus one (AC)50: (FASTA text, list of code arrays)."""
    seqs = [rng.integers(0, 4, int(rng.integers(90, 161)), dtype=np.uint8) for _ in range(n)]
    seqs.append(np.tile(np.array([0, 1], np.uint8), 50))
    text = b"".join(b">art%d some words\n" % j + bytes(ALPHA[s]) + b"\n" for j, s in enumerate(seqs))
    return text, seqs


def _fasta(text):
    from tagdust_amd import lib as tdlib
    string, s_index, _ = tdlib.parse_fasta(text)
    return np.ascontiguousarray(string, np.uint8), np.ascontiguousarray(s_index, np.int32)


def _window(rng, seqs, L, subs=True):
    """An L-nt window of a random artifact (L <= its length), forward or reverse complement, with 0-3 substitutions."""
    s = seqs[int(rng.integers(0, len(seqs)))]
    if len(s) < L:
        s = seqs[0]
    p = int(rng.integers(0, len(s) - L + 1))
    w = s[p:p + L].copy()
    if rng.integers(0, 2):
        w = COMP[w[::-1]]
    for _ in range(int(rng.integers(0, 4)) if subs else 0):
        q = int(rng.integers(0, L))
        w[q] = (w[q] + int(rng.integers(1, 4))) & 3
    return w


def _leftovers(n, T):
    """Indices of a batch of n reads that match_to_reference scores with bpm_check_error (thread ranges of run_pHMM)."""
    out = []
    interval = n // T
    for t in range(T):
        lo = t * interval
        hi = n if t == T - 1 else lo + interval
        out.extend(range(lo + (hi - lo) // 4 * 4, hi))
    return out


def _fastq(names, seqs):
    return b"".join(b"@" + nm + b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n" for nm, s in zip(names, seqs))


def _plant(path, rng, seqs, positions):
    """Replace the reads at `positions` of a 76-nt FASTQ file by planted artifact windows."""
    lines = open(path, "rb").read().split(b"\n")
    for i in positions:
        lines[4 * i + 1] = bytes(ALPHA[_window(rng, seqs, 76)])
    open(path, "wb").write(b"\n".join(lines))


def _need_ref():
    if not os.path.exists(os.path.join(RBIN, "tagdust_rtest")):
        pytest.skip("oracle/_ref binaries not built")


@pytest.mark.gpu
@pytest.mark.parametrize("T,n_ctx", [(1, 1), (3, 2)], ids=["t1-one-context", "t3-two-contexts"])
def test_multi_file_ref_equals_the_reference_binary(tmp_path, T, n_ctx):
    """The CASAVA three-read shape with -ref: the index file decoded, reads 1 and 3 through TD_MODE_RNA_DUST, 1000-record
    batches as in the -DRTEST build (four batches and a tail) == the reference binary's files and counts."""
    _need_ref()
    import bench
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    d = str(tmp_path)
    n = 4321
    r1, r2, r3, segs = bench.write_casava_files(d, n)
    rng = np.random.default_rng(5 + T)
    text, seqs = _artifacts(rng)
    open(os.path.join(d, "art.fa"), "wb").write(text)
    # planted reads: some in groups of four, some on the left-over positions of every batch's thread ranges
    left = [b0 + i for b0 in range(0, n, 1000) for i in _leftovers(min(1000, n - b0), T)]
    _plant(r1, rng, seqs, sorted(set(list(rng.choice(n, 60, replace=False)) + left[::2])))
    _plant(r3, rng, seqs, sorted(set(list(rng.choice(n, 60, replace=False)) + left[1::2])))
    g = load_golden("casava_index")
    args = str(g["cmdline"]).split()
    subprocess.run([os.path.join(RBIN, "tagdust_rtest")] + args + ["-ref", os.path.join(d, "art.fa"), "-fe", "2", "-t", str(T),
                   r2, r1, r3, "-o", os.path.join(d, "cpu")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    string, s_index = _fasta(text)
    head = b"".join(open(r2, "rb").readlines()[:4000])   # the reference's statistics come from its first batch
    pr = tdlib.ParsedReads(head, 1)
    ctx2 = [TagdustHip(0) for _ in range(n_ctx)]
    ctx1 = [TagdustHip(0) for _ in range(n_ctx)]
    ctx3 = [TagdustHip(0) for _ in range(n_ctx)]
    try:
        thr = tdlib.estimate_threshold(ctx2[0], segs, pr.codes, pr.offs, float(g["d"]), seed=42, n_reads=4000, rng=1)
        model, _ = tdlib.build_model(segs, pr.codes, pr.offs, 0.05, float(g["d"]))
        for c in ctx2:
            c.upload_model(model)
            c.set_params(thr, 16, 100)
        for c in ctx1 + ctx3:                 # no model: run_rna_dust
            c.set_params(0.0, 16, 100)
        for c in ctx1 + ctx2 + ctx3:
            c.set_artifacts(string, s_index, 2, T)
        st, cnt = tdlib.stream_run_multi([(r2, segs, ctx2), (r1, ["R:N"], ctx1), (r3, ["R:N"], ctx3)], os.path.join(d, "gpu"),
                                         n_devices=n_ctx, dust=100, batch_reads=1000, n_threads=4)
    finally:
        pr.close()
        for c in ctx1 + ctx2 + ctx3:
            c.close()
    assert st["n_reads"] == n and st["n_batches"] == 5
    a, b = _files(d, "cpu"), _files(d, "gpu")
    assert len(a) == 26 and set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        assert a[k] == b[k], "output file *%s differs" % k
    log = _log_counts(os.path.join(d, "cpu_logfile.txt"))
    assert log["successfully extracted"] == cnt[0] and log["problems with architecture"] == cnt[1]
    assert log["low complexity"] == cnt[6] and log["total input reads"] == n == int(cnt[:8].sum())
    assert log["match artifacts:"] == cnt[5] > 0


@pytest.mark.gpu
def test_single_rn_file_ref_equals_the_reference_binary(tmp_path):
    """`-1 R:N -ref` on one file: read lengths around the 63-character cap of bmp_single and the mod-64 shifts of
    bpm_check_error (left-over reads of the 3 thread ranges), planted windows and random reads."""
    _need_ref()
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    d = str(tmp_path)
    rng = np.random.default_rng(3)
    text, seqs = _artifacts(rng)
    open(os.path.join(d, "art.fa"), "wb").write(text)
    lens = [1, 2, 3, 4, 5, 31, 32, 63, 64, 65, 100, 150]
    n = 2400
    reads = []
    for i in range(n):
        L = lens[i % len(lens)]
        s = _window(rng, seqs, L) if (i % 3 == 0 and L <= 90) else rng.integers(0, 4, L, dtype=np.uint8)
        reads.append(bytes(ALPHA[s]))
    path = os.path.join(d, "in.fq")
    open(path, "wb").write(_fastq([b"r%d" % i for i in range(n)], reads))
    subprocess.run([os.path.join(RBIN, "tagdust_rtest"), "-1", "R:N", "-ref", os.path.join(d, "art.fa"), "-fe", "2", "-t", "3", path,
                    "-o", os.path.join(d, "cpu")], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
    string, s_index = _fasta(text)
    c = TagdustHip(0)
    try:
        c.set_params(0.0, 16, 100)
        c.set_artifacts(string, s_index, 2, 3)
        st, cnt = tdlib.stream_run_multi([(path, ["R:N"], [c])], os.path.join(d, "gpu"), n_devices=1, dust=100, batch_reads=1000,
                                         n_threads=2)
    finally:
        c.close()
    a, b = _files(d, "cpu"), _files(d, "gpu")
    assert a and set(a) == set(b), (sorted(a), sorted(b))
    for k in a:
        assert a[k] == b[k], "output file *%s differs" % k
    log = _log_counts(os.path.join(d, "cpu_logfile.txt"))
    assert log["total input reads"] == n == int(cnt[:8].sum()) and log["match artifacts:"] == cnt[5] > 0
    assert log["successfully extracted"] == cnt[0] and log["low complexity"] == cnt[6]


@pytest.mark.gpu
@pytest.mark.parametrize("dust", [100, 20])
def test_device_path_equals_host_path_without_filter(tmp_path, dust):
    """R:N files without -ref: device contexts (TD_MODE_RNA_DUST) == the host path (contexts None), '.' and N included."""
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    d = str(tmp_path)
    rng = np.random.default_rng(dust)
    alpha = np.frombuffer(b"ACGTN.", np.uint8)
    reads = []
    for i in range(6000):
        L = [1, 2, 3, 4, 5][i % 5] if i % 7 == 0 else int(rng.integers(6, 160))
        p = rng.random()
        if p < 0.1:
            s = np.tile(rng.integers(0, 4, int(rng.integers(1, 4)), dtype=np.uint8), L)[:L]        # low complexity
        else:
            s = rng.integers(0, 4, L, dtype=np.uint8)
        w = rng.random(L)
        s = np.where(w < 0.03, 4, np.where(w > 0.97, 5, s)).astype(np.uint8)                      # N and '.'
        reads.append(bytes(alpha[s]))
    paths = [os.path.join(d, "a.fq"), os.path.join(d, "b.fq")]
    for k, p in enumerate(paths):
        open(p, "wb").write(_fastq([b"r%d" % i for i in range(len(reads))], reads if k == 0 else reads[::-1]))
    ctxs = [TagdustHip(0), TagdustHip(0)]
    try:
        for c in ctxs:
            c.set_params(0.0, 16, dust)
        out = {}
        for tag, cx in (("dev", ctxs), ("host", None)):
            out[tag] = tdlib.stream_run_multi([(paths[0], ["R:N"], [cx[0]] if cx else None), (paths[1], ["R:N"], [cx[1]] if cx else None)],
                                              os.path.join(d, tag), n_devices=1, dust=dust, batch_reads=1500, n_threads=2)[1]
    finally:
        for c in ctxs:
            c.close()
    a, b = _files(d, "host"), _files(d, "dev")
    assert a and set(a) == set(b)
    for k in a:
        assert a[k] == b[k], "output file *%s differs" % k
    assert np.array_equal(out["dev"], out["host"]) and out["dev"][6] > 0


def _dust_low(s, cut):
    """rna_dust_low (td_stream.cpp) / dust_sequences on a raw read, restated."""
    L = len(s)
    if L < 1:
        return False
    at = lambda k: int(s[k]) if k < L else 0
    key = ((at(0) & 3) << 2) | (at(1) & 3)
    trip = np.zeros(64, np.int64)
    c = 2
    for j in range(2, min(L, 64)):
        key = ((key << 2) | (at(j) & 3)) & 63
        trip[key] += 1
        c += 1
    with np.errstate(divide="ignore", invalid="ignore"):
        sc = np.float64((trip * (trip - 1) // 2).sum()) / np.float64(c - 3) * 10.0
    return bool(sc > cut)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 3, 7])
def test_mode_equals_the_oracle(T):
    """td_multi_decode(TD_MODE_RNA_DUST) over two contexts == tdo_match_artifacts per thread range + DUST restated."""
    from oracle import pyoracle
    from tagdust_amd import RESULT_DTYPE
    from tagdust_amd import lib as tdlib
    rng = np.random.default_rng(100 + T)
    text, seqs = _artifacts(rng)
    string, s_index = _fasta(text)
    n = 20003                                  # (left-over reads in every thread range for T = 1, 3, 7)
    left = set(_leftovers(n, T))
    rl = []
    for i in range(n):
        if i in left:                          # bpm_check_error starts its score at the read length: it finds short reads
            L = int(rng.integers(8, 32))
            s = _window(rng, seqs, L, subs=False)
        else:
            L = int(rng.integers(1, 160)) if i % 5 else int(rng.integers(8, 32))
            s = _window(rng, seqs, L) if rng.random() < 0.05 and L <= 90 else rng.integers(0, 4, L, dtype=np.uint8)
        if rng.random() < 0.02:
            s = np.tile(np.array([0, 1], np.uint8), L)[:L].copy()
        if rng.random() < 0.05:
            s[int(rng.integers(0, L))] = 4
        rl.append(s.astype(np.uint8))
    lens = np.array([len(s) for s in rl], np.int64)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum(lens)
    codes = np.concatenate(rl)
    dust = 100
    m = tdlib.TagdustMulti([0, 0])
    try:
        m.set_params(0.0, 16, dust)
        m.set_artifacts(string, s_index, 2, T)
        m.counts_reset()
        res, lab, sq = m.decode(codes, offs, mode=tdlib.MODE_RNA_DUST, labels=False, seq=True)
        dev_counts = m.counts()
    finally:
        m.close()
    # the oracle: match_to_reference per thread range, then DUST
    L = pyoracle.lib()
    L.tdo_match_artifacts.restype = None
    L.tdo_match_artifacts.argtypes = [C.POINTER(pyoracle._Artifacts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
    art = pyoracle._Artifacts(string.ctypes.data, s_index.ctypes.data, len(s_index) - 1, 2)
    ores = np.zeros(n, pyoracle.RESULT_DTYPE)
    work = codes.copy()
    interval = n // T
    for t in range(T):
        lo = t * interval
        hi = n if t == T - 1 else lo + interval
        L.tdo_match_artifacts(C.byref(art), work.ctypes.data, offs.ctypes.data, ores.ctypes.data, lo, hi)
    assert np.array_equal(work, codes)
    want = ores["read_type"].copy()
    for i in range(n):
        if _dust_low(rl[i], dust):
            want[i] = 6
    got = res["read_type"]
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    hits = (want & 0xFF) == 5
    assert hits[sorted(left)].any() and hits[[i for i in range(n) if i not in left]].any()
    assert (res["f_score"] == 0).all() and (res["b_score"] == 0).all() and (res["r_score"] == 0).all() and (res["bar_prob"] == 0).all()
    assert (res["mapq"] == -1).all() and (res["barcode"] == -1).all() and (res["fingerprint"] == -1).all()
    assert np.array_equal(sq, codes)
    assert np.array_equal(dev_counts, tdlib.count_outcomes(res, lens))
    assert res.dtype == RESULT_DTYPE


@pytest.mark.gpu
def test_refusals(tmp_path):
    """A filter on the index file with an R:N file that has no contexts, a dust mismatch, labels in the new mode."""
    import bench
    from tagdust_amd import TagdustHip, TdError
    from tagdust_amd import lib as tdlib
    d = str(tmp_path)
    r1, r2, r3, segs = bench.write_casava_files(d, 200)
    text, _ = _artifacts(np.random.default_rng(0), 3)
    string, s_index = _fasta(text)
    ci, cr = TagdustHip(0), TagdustHip(0)
    try:
        ci.set_artifacts(string, s_index, 2, 1)
        with pytest.raises(TdError, match="r1.fq.*no contexts"):
            tdlib.stream_run_multi([(r2, segs, [ci]), (r1, ["R:N"], None)], os.path.join(d, "x"), dust=100, batch_reads=100)
        cr.set_params(0.0, 16, 100)
        with pytest.raises(TdError, match="dust"):
            tdlib.stream_run_multi([(r1, ["R:N"], [cr])], os.path.join(d, "y"), dust=50, batch_reads=100)
        offs = np.array([0, 3, 7], np.int64)
        codes = np.array([0, 1, 2, 3, 0, 1, 2], np.uint8)
        res = np.zeros(2, tdlib.RESULT_DTYPE)
        with pytest.raises(TdError, match="no labels"):
            cr.submit(codes, offs, mode=tdlib.MODE_RNA_DUST, res=res, labels=np.zeros(9, np.int8))
        t = cr.submit(codes, offs, mode=tdlib.MODE_RNA_DUST, res=res)   # the context still works
        cr.wait(t)
        assert (res["read_type"] == 0).all() and (res["mapq"] == -1).all()
    finally:
        ci.close()
        cr.close()
