"""Background compile of the model-specialised kernel (option "async_compile") and the whole-kernel probe every freshly loaded
specialised kernel has to pass (include/tagdust_hip.h: td_spec_wait, td_spec_probe).  A model is usable as soon as its tables are
up -- the generic kernel decodes until the compiled one is handed over -- and a kernel that does not reproduce the generic
kernel's output on the probe reads never takes over.  Every output is compared with the reference's fixtures bit for bit.

A fresh compile (6-8 s for the small models) comes from a TD_TEST_UNIQUE_KEY define of the test's own in TD_SPEC_EXTRA_OPTS plus
a cache directory of its own."""
import os
import time

import numpy as np
import pytest

from conftest import load_golden, golden_artifacts, golden_window, GOLDEN_NAMES

pytestmark = pytest.mark.gpu

RES_FIELDS = ("f_score", "b_score", "r_score", "bar_prob", "mapq", "read_type", "barcode", "fingerprint")


@pytest.fixture(scope="module")
def goldens():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = load_golden(name)
        return cache[name]
    return get


def _fresh(monkeypatch, tmp_path, key, extra=""):
    monkeypatch.setenv("TD_SPEC_CACHE_DIR", str(tmp_path))
    monkeypatch.setenv("TD_SPEC_EXTRA_OPTS", ("-DTD_TEST_UNIQUE_KEY=%d %s" % (key, extra)).strip())


def _golden_res(g):
    from tagdust_amd import RESULT_DTYPE
    r = np.zeros(int(g["n_reads"]), RESULT_DTYPE)
    for k in RES_FIELDS:
        r[k] = g[k]
    return r


def _assert_golden(g, res, labels, seq):
    want = _golden_res(g)
    for k in RES_FIELDS:
        a, b = np.ascontiguousarray(res[k]).view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)
        assert np.array_equal(a, b), k
    assert np.array_equal(labels, g["labels"])
    assert np.array_equal(seq, g["seq_after"])


def _ctx(g, async_compile, **opts):
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", 1)
    c.set_option("async_compile", async_compile)
    for k, v in opts.items():
        c.set_option(k, v)
    c.upload_model(g)
    c.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
    return c


def _decode(c, g):
    c.upload_batch(g["seq"], g["offs"])
    c.run()
    return c.download()


def _expected_counts(g, times=1):
    cnt = np.zeros(264, np.int64)
    for code in range(8):
        cnt[code] = int(((g["read_type"] & 0xFF) == code).sum())
    ok = (g["read_type"] == 0) & (g["barcode"] >= 0)
    cnt[8:] = np.bincount(g["barcode"][ok] & 0xFF, minlength=256)
    return cnt * times


def test_async_upload_decodes_before_the_kernel_is_ready(goldens, monkeypatch, tmp_path):
    _fresh(monkeypatch, tmp_path, 101)
    g = goldens("umi_f_s_r")
    c = _ctx(g, 1)            # (without the feature: TdError "unknown option async_compile")
    try:
        assert c.get_option("async_compile") == 1
        assert c.get_option("spec_state") == 1
        res, labels, seq = _decode(c, g)
        _assert_golden(g, res, labels, seq)
        assert c.get_option("spec_batches_generic") >= 1
        c.spec_wait()
        assert c.get_option("spec_state") == 3
        n_generic = c.get_option("spec_batches_generic")
        res2, labels2, seq2 = _decode(c, g)
        assert c.get_option("spec_batches_generic") == n_generic       # the compiled kernel ran this one
        assert res2.tobytes() == res.tobytes() and labels2.tobytes() == labels.tobytes() and seq2.tobytes() == seq.tobytes()
    finally:
        c.close()


def test_pipelined_batches_across_the_hand_over(goldens, monkeypatch, tmp_path):
    from tagdust_amd import RESULT_DTYPE
    _fresh(monkeypatch, tmp_path, 102)
    g = goldens("c2_b4_r")
    c = _ctx(g, 1, pipeline_depth=3, poison_workspace=1)
    try:
        n = int(g["n_reads"])
        offs = np.ascontiguousarray(g["offs"], np.int64)
        seq = np.ascontiguousarray(g["seq"], np.uint8)
        c.counts_reset()
        n_batches, after, first_spec = 0, 0, -1
        deadline = time.monotonic() + 120.0
        while after < 3:
            assert time.monotonic() < deadline, "no hand-over within 120 s (spec_state %d)" % c.get_option("spec_state")
            res = np.zeros(n, RESULT_DTYPE)
            lab = np.zeros(int(offs[-1]) + n, np.int8)
            sq = np.zeros(int(offs[-1]), np.uint8)
            c.wait(c.submit(seq, offs, res=res, labels=lab, seq_out=sq))
            n_batches += 1
            _assert_golden(g, res, lab, sq)
            if c.get_option("spec_state") == 3:
                if first_spec < 0:
                    first_spec = n_batches
                after += 1
        print("hand-over after %d batches of %d" % (first_spec, n_batches))
        assert c.get_option("spec_batches_generic") >= 1
        assert np.array_equal(c.counts(), _expected_counts(g, n_batches))
    finally:
        c.close()


def test_streaming_run_async_equals_sync(goldens, monkeypatch, tmp_path):
    import glob
    from tagdust_amd import lib as tdlib
    g = goldens("umi_f_s_r")
    a = str(g["cmdline"]).split()
    segs = [a[i + 1] for i in range(len(a) - 1) if a[i].startswith("-") and a[i][1:].isdigit()]
    n_src, offs, n = int(g["n_reads"]), g["offs"], 1 << 16
    letters = np.frombuffer(b"ACGTN", np.uint8)
    recs = []
    for i in range(n_src):
        s = bytes(letters[g["seq"][offs[i]:offs[i + 1]]])
        recs.append(b"\n" + s + b"\n+\n" + b"I" * len(s) + b"\n")
    fq = str(tmp_path / "in.fq")
    with open(fq, "wb") as fh:
        fh.write(b"".join(b"@r%d" % i + recs[i % n_src] for i in range(n)))
    out = {}
    for mode in ("async", "sync"):
        if mode == "async":
            _fresh(monkeypatch, tmp_path / "cache", 103)
            os.makedirs(str(tmp_path / "cache"), exist_ok=True)
        else:
            monkeypatch.delenv("TD_SPEC_EXTRA_OPTS")
        c = _ctx(g, 1 if mode == "async" else 0)
        try:
            st = tdlib.stream_run(c, fq, segs, str(tmp_path / mode), batch_reads=4096, n_threads=3)
            assert st["n_reads"] == n
            if mode == "async":
                assert c.get_option("spec_batches_generic") >= 1
            else:
                assert c.get_option("spec_state") == 3 and c.get_option("spec_batches_generic") == 0
        finally:
            c.close()
        out[mode] = {os.path.basename(p)[len(mode):]: open(p, "rb").read() for p in sorted(glob.glob(str(tmp_path / (mode + "*"))))
                     if os.path.isfile(p)}
    assert out["sync"] and set(out["sync"]) == set(out["async"])
    for k in out["sync"]:
        assert out["sync"][k] == out["async"][k], "output file *%s differs" % k


@pytest.mark.parametrize("async_compile", [0, 1], ids=["sync", "async"])
@pytest.mark.parametrize("wrong", [1, 2])
def test_probe_rejects_a_wrong_kernel(goldens, monkeypatch, tmp_path, capfd, wrong, async_compile):
    """TDS_TEST_WRONG_RESULT makes the compiled kernel compute wrong values (one b_score bit per tile / one label of every read
    of odd length): the probe must keep it from ever decoding a batch."""
    _fresh(monkeypatch, tmp_path, 110 + 2 * wrong + async_compile, "-DTDS_TEST_WRONG_RESULT=%d" % wrong)
    g = goldens("umi_f_s_r")
    c = _ctx(g, async_compile)          # the upload succeeds
    try:
        c.spec_wait()
        assert c.get_option("spec_state") == 4
        res, labels, seq = _decode(c, g)
        _assert_golden(g, res, labels, seq)
        assert c.get_option("spec_state") == 4
        assert c.get_option("prune_active") == 0 and c.get_option("overlap_active") == 0
        assert c.get_option("spec_batches_generic") >= 1
    finally:
        c.close()
    err = capfd.readouterr().err
    assert "probe" in err.lower() and "read" in err


@pytest.mark.parametrize("name", GOLDEN_NAMES)
def test_probe_accepts_every_shipped_model(goldens, name):
    from tagdust_amd import TagdustHip
    g = goldens(name)
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 1)
        art = golden_artifacts(g)
        if art:
            c.set_artifacts(*art)
        c.upload_model(g)
        assert c.get_option("spec_probe") == 1
        assert c.get_option("spec_state") == 3
        assert not c.counts().any()         # the probe counted on scratch counters
        win = golden_window(g)
        if win:                             # the window variant is loaded -- and probed -- with the first batch through a window
            c.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
            c.set_window(*win)
            res, labels, seq = _decode(c, g)
            assert c.get_option("spec_state") == 3
            _assert_golden(g, res, labels, seq)
    finally:
        c.close()


def test_async_selfcheck_falls_back_through_a_second_job(goldens, monkeypatch):
    """A background compile whose clamp-free logsum fails the self-check at the hand-over (forced through
    TD_SPEC_SELFCHECK_FAIL, which a context reads when it is created) is not loaded: the clamped form goes to the background as a
    second job, the generic kernel decodes meanwhile, and td_spec_wait returns only when that second kernel has taken over.  The
    ordinary cache directory serves: both code objects are usually there already."""
    monkeypatch.setenv("TD_SPEC_SELFCHECK_FAIL", "1")
    g = goldens("umi_f_s_r")
    c = _ctx(g, 1)
    try:
        assert c.get_option("spec_state") in (1, 2)
        res, labels, seq = _decode(c, g)
        _assert_golden(g, res, labels, seq)
        c.spec_wait()
        assert c.get_option("spec_state") == 3
        assert c.get_option("spec_lsum_clamped") == 1
        n_generic = c.get_option("spec_batches_generic")
        res2, labels2, seq2 = _decode(c, g)
        assert res2.tobytes() == res.tobytes() and labels2.tobytes() == labels.tobytes() and seq2.tobytes() == seq.tobytes()
        assert c.get_option("spec_batches_generic") == n_generic       # the clamped kernel ran this one
    finally:
        c.close()


def test_concurrent_uploads_share_one_compile(goldens, monkeypatch, tmp_path):
    from tagdust_amd import TagdustHip
    _fresh(monkeypatch, tmp_path, 120)
    g = goldens("umi_f_s_r")
    a, b = TagdustHip(0), TagdustHip(0)
    try:
        before = a.get_option("spec_compiles_started")
        for c in (a, b):
            c.set_option("async_compile", 1)
            c.upload_model(g)
            c.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
        a.spec_wait()
        b.spec_wait()
        assert a.get_option("spec_compiles_started") - before == 1
        assert a.get_option("spec_state") == 3 and b.get_option("spec_state") == 3
        for c in (a, b):
            _assert_golden(g, *_decode(c, g))
    finally:
        a.close()
        b.close()


def test_superseded_upload_is_never_loaded(goldens, monkeypatch, tmp_path):
    """Model A async, then model B at once: A's compile may finish and land in the caches, the context decodes under B."""
    ga, gb = goldens("umi_f_s_r"), goldens("scen1_b_r")
    _fresh(monkeypatch, tmp_path, 121)
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    try:
        c.set_option("async_compile", 1)
        c.upload_model(ga)
        assert c.get_option("spec_state") == 1
        c.upload_model(gb)
        c.set_params(float(gb["threshold"]), int(gb["minlen"]), int(gb["dust"]))
        c.spec_wait()
        assert c.get_option("spec_state") == 3
        _assert_golden(gb, *_decode(c, gb))
        # A's reads under this context are decoded under B: not what A's model makes of them
        c.set_params(float(ga["threshold"]), int(ga["minlen"]), int(ga["dust"]))
        res, labels, seq = _decode(c, ga)
        assert not np.array_equal(labels, ga["labels"])
        assert not np.array_equal(np.ascontiguousarray(res["f_score"]).view(np.uint32), np.ascontiguousarray(ga["f_score"]).view(np.uint32))
    finally:
        c.close()


def test_destroy_while_compiling(goldens, monkeypatch, tmp_path):
    _fresh(monkeypatch, tmp_path, 122)
    g = goldens("umi_f_s_r")
    c = _ctx(g, 1)
    assert c.get_option("spec_state") == 1
    c.close()                               # returns, after the worker has finished: the code object is on disk
    files = [f for f in os.listdir(str(tmp_path)) if f.endswith(".hsaco")]
    assert len(files) == 1 and not [f for f in os.listdir(str(tmp_path)) if f.endswith(".tmp")]
    c2 = _ctx(g, 0)
    try:
        assert c2.get_option("spec_state") == 3
        _assert_golden(g, *_decode(c2, g))
    finally:
        c2.close()


def test_compile_failure_is_reported(goldens, monkeypatch, tmp_path):
    """A compile failure stays an error: at once from a synchronous upload; from td_spec_wait and from the next staging call
    after a background one."""
    from tagdust_amd import TagdustHip, TdError
    monkeypatch.setenv("TD_SPEC_CACHE_DIR", str(tmp_path))
    monkeypatch.setenv("TD_SPEC_EXTRA_OPTS", "-DTD_TEST_UNIQUE_KEY=130 --td-no-such-compiler-option")
    g = goldens("umi_f_s_r")
    c = TagdustHip(0)
    try:
        with pytest.raises(TdError, match="did not compile"):
            c.upload_model(g)
        assert c.get_option("spec_state") == 5
        c.set_option("async_compile", 1)
        c.upload_model(g)                   # the tables are up, the compile is on its way to failing
        with pytest.raises(TdError, match="did not compile"):
            c.spec_wait()
        assert c.get_option("spec_state") == 5
        with pytest.raises(TdError, match="did not compile"):
            c.upload_batch(g["seq"], g["offs"])
    finally:
        c.close()
