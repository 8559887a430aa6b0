"""Per-artifact hit counts (td_artifact_hits_get, td_multi_artifact_hits): the reference's reference_fasta->mer_hash
(src/barcode_hmm.c:381), the `count<TAB>name` lines of its log -- reads whose outcome is ((index + 1) << 8) | 5, counted on the
device behind every batch while a -ref filter is set.  Held against a host count over the downloaded read_type values."""
import numpy as np
import pytest

from conftest import load_golden, golden_artifacts

pytestmark = pytest.mark.gpu

ALPHA = np.frombuffer(b"ACGTN", np.uint8)


def _want(read_type, n_seq):
    rt = np.asarray(read_type)
    hit = (rt & 0xFF) == 5
    return np.bincount((rt[hit] >> 8) - 1, minlength=n_seq).astype(np.int64)


@pytest.fixture()
def ctx():
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", 0)
    yield c
    c.close()


def _fixture_ctx(ctx):
    g = load_golden("artifacts_b_r")
    string, s_index, fe, T = golden_artifacts(g)
    ctx.set_artifacts(string, s_index, fe, T)
    ctx.upload_model(g)
    ctx.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
    return g, len(s_index) - 1


def test_fixture_hits_accumulate_and_reset(ctx):
    g, n_seq = _fixture_ctx(ctx)
    want = _want(g["read_type"], n_seq)
    assert want.sum() > 0
    assert not ctx.artifact_hits(n_seq).any()
    ctx.upload_batch(g["seq"], g["offs"])
    ctx.run()
    res, _, _ = ctx.download()
    assert np.array_equal(res["read_type"], g["read_type"])
    assert np.array_equal(ctx.artifact_hits(n_seq), want)
    half = int(g["n_reads"]) // 2          # a second, different batch
    ctx.upload_batch(g["seq"][:g["offs"][half]], g["offs"][:half + 1])
    ctx.run()
    res2, _, _ = ctx.download()
    assert np.array_equal(ctx.artifact_hits(n_seq + 3), np.concatenate([want + _want(res2["read_type"], n_seq), [0, 0, 0]]))
    assert ctx.counts()[5] == want.sum() + _want(res2["read_type"], n_seq).sum()
    ctx.counts_reset()
    assert not ctx.artifact_hits(n_seq).any()
    from tagdust_amd import TdError
    with pytest.raises(TdError, match="room for"):
        ctx.artifact_hits(n_seq - 1)


def test_fixture_hits_through_submit_and_wait(ctx):
    from tagdust_amd import RESULT_DTYPE
    g, n_seq = _fixture_ctx(ctx)
    n = int(g["n_reads"])
    seq, offs = np.ascontiguousarray(g["seq"], np.uint8), np.ascontiguousarray(g["offs"], np.int64)
    cut = n // 3
    parts = [(0, cut), (cut, n), (0, n)]
    res = [np.zeros(b - a, RESULT_DTYPE) for a, b in parts]
    tickets = [ctx.submit(seq, np.ascontiguousarray(offs[a:b + 1]), res=r) for (a, b), r in zip(parts, res)]
    for t in tickets:
        ctx.wait(t)
    # (thread ranges of the filter are taken per batch, so the pieces are counted as they were decoded)
    want = sum(_want(r["read_type"], n_seq) for r in res)
    assert want.sum() > 0 and np.array_equal(res[2]["read_type"], g["read_type"])
    assert np.array_equal(ctx.artifact_hits(n_seq), want)
    ctx.counts_reset()
    assert not ctx.artifact_hits(n_seq).any()


def _filter(rng, n_seq, L=20):
    from tagdust_amd import lib as tdlib
    seqs = [rng.integers(0, 4, L, dtype=np.uint8) for _ in range(n_seq)]
    text = b"".join(b">a%d\n" % j + bytes(ALPHA[s]) + b"\n" for j, s in enumerate(seqs))
    string, s_index, _ = tdlib.parse_fasta(text)
    return seqs, np.ascontiguousarray(string, np.uint8), np.ascontiguousarray(s_index, np.int32)


@pytest.mark.parametrize("n_seq", [300, 1100], ids=["300", "1100-beyond-the-lds-bins"])
def test_one_read_per_sequence_in_rna_dust_mode(ctx, n_seq):
    """A filter of n_seq sequences of 20 bases and one read equal to each, through TD_MODE_RNA_DUST (no model): n_seq ones."""
    from tagdust_amd import RESULT_DTYPE
    from tagdust_amd import lib as tdlib
    seqs, string, s_index = _filter(np.random.default_rng(n_seq), n_seq)
    ctx.set_params(0.0, 16, 0)
    ctx.set_artifacts(string, s_index, 2, 1)
    offs = (np.arange(n_seq + 1, dtype=np.int64) * 20)
    codes = np.concatenate(seqs)
    res = np.zeros(n_seq, RESULT_DTYPE)
    ctx.wait(ctx.submit(codes, offs, mode=tdlib.MODE_RNA_DUST, res=res))
    hits = ctx.artifact_hits(n_seq)
    assert np.array_equal(hits, _want(res["read_type"], n_seq))
    assert np.array_equal(hits, np.ones(n_seq, np.int64))


def test_two_contexts_on_one_device_sum(ctx):
    from tagdust_amd import lib as tdlib
    rng = np.random.default_rng(8)
    seqs, string, s_index = _filter(rng, 40, L=60)
    n = 5003
    reads = []
    for i in range(n):
        if i % 3 == 0:
            s = seqs[int(rng.integers(0, 40))]
            p = int(rng.integers(0, 20))
            reads.append(s[p:p + 40])
        else:
            reads.append(rng.integers(0, 4, int(rng.integers(20, 80)), dtype=np.uint8))
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in reads])
    codes = np.concatenate(reads)
    m = tdlib.TagdustMulti([0, 0])
    try:
        m.set_params(0.0, 16, 100)
        m.set_artifacts(string, s_index, 2, 3)
        m.counts_reset()
        res, _, _ = m.decode(codes, offs, mode=tdlib.MODE_RNA_DUST, labels=False, seq=False)
        hits = m.artifact_hits(40)
        m.counts_reset()
        assert not m.artifact_hits(40).any()
    finally:
        m.close()
    want = _want(res["read_type"], 40)
    assert want.sum() > 1000 and np.array_equal(hits, want)


def test_without_a_filter_nothing_changes(ctx):
    g = load_golden("c2_b4_r")
    ctx.upload_model(g)
    ctx.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
    ctx.upload_batch(g["seq"], g["offs"])
    ctx.counts_reset()
    ctx.run()
    res, labels, seq_after = ctx.download()
    assert ctx.get_option("artifacts_active") == 0
    assert not ctx.artifact_hits(5).any()
    ms = ctx.last_kernel_ms()
    assert np.isfinite(ms) and ms > 0.0
    assert np.array_equal(res["read_type"], g["read_type"]) and np.array_equal(res["barcode"], g["barcode"])
    assert np.array_equal(labels, g["labels"]) and np.array_equal(seq_after, g["seq_after"])
    assert np.array_equal(res["b_score"].view(np.uint32), np.asarray(g["b_score"], np.float32).view(np.uint32))
