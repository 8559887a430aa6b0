"""The barcode-segment shapes of tests/plan_shapes.py on the device: every shape through the model-specialised kernel and the generic
kernel against the CPU oracle, by the standing rule -- scores bit for bit, Q within 1e-4, labels / outcomes / barcodes / fingerprints /
rewritten sequences equal, device counters equal to serial counting over the oracle's outcomes -- then the knob variants of the
specialised kernel, a -start / -end window over two run-time-looped segments, and a pipelined pass.  tests/test_plan_shapes.py pins
(on the CPU) which plan state each shape reaches.  A specialised context must really have decoded with its own kernel: the load-time
probe would otherwise hand a rejected kernel's batches to the generic one."""
import numpy as np
import pytest

import plan_shapes
from test_parity_gpu import Q_TOL, _bits

pytestmark = pytest.mark.gpu

_DEFAULT = {}      # shape -> the specialised kernel's downloads under the default knobs


@pytest.fixture(scope="module", params=[1, 0], ids=["specialised", "generic"])
def ctx(request):
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    c.set_option("specialize", request.param)
    c.set_option("poison_workspace", 1)      # stale workspace contents must never reach a result
    yield c
    c.close()


def _decode(c, name, window=None, modes=True):
    """case(name, window) through context c: (records, labels, sequences, counters, records of MODE_GET_PROB, of MODE_ARCH_COMP)"""
    from tagdust_amd import MODE_GET_PROB, MODE_ARCH_COMP
    segs, seq, offs, md = plan_shapes.case(name, window)
    c.set_artifacts(None)
    c.set_window(*(window or (-1, -1)))
    try:
        c.upload_model(md)
        c.set_params(float(md["threshold"]), int(md["minlen"]), int(md["dust"]))
        c.upload_batch(seq, offs)
        c.counts_reset()
        c.run()
        out = c.download() + (c.counts(),)
        if modes:
            c.run(MODE_GET_PROB)
            out += (c.download(labels=False, seq=False)[0],)
            c.run(MODE_ARCH_COMP)
            out += (c.download(labels=False, seq=False)[0],)
        if c.get_option("specialize"):
            assert c.get_option("spec_state") == 3 and c.get_option("spec_batches_generic") == 0, (name, "the specialised kernel did not decode")
        else:
            assert c.get_option("spec_batches_generic") >= 1
    finally:
        c.set_window(-1, -1)
    return out


def _differing(name, window, res, labels, ores, olab):
    """which reads differ, and where their labels do: segment, HMM and side of kRt -- for the message of a failing comparison"""
    segs, seq, offs, md = plan_shapes.case(name, window)
    label = np.asarray(md["label"]).astype(np.int64)
    out = []
    for i in range(len(offs) - 1):
        a, b = labels[int(offs[i]) + i:int(offs[i + 1]) + i + 1], olab[int(offs[i]) + i:int(offs[i + 1]) + i + 1]
        fields = [k for k, o in (("b_score", "b_score"), ("f_score", "f_score"), ("r_score", "r_score"), ("bar_prob", "bar_prob"))
                  if _bits(res[k][i:i + 1])[0] != _bits(ores[o][i:i + 1])[0]]
        fields += [k for k in ("read_type", "barcode", "fingerprint") if res[k][i] != ores[k][i]]
        if fields or not np.array_equal(a, b):
            at = np.flatnonzero(a != b)[:3]
            out.append((i, fields, [(int(p), "seg %d hmm %d" % (label[a[p]] & 0xFFFF, (label[a[p]] >> 16) & 0x7FFF),
                                     "oracle seg %d hmm %d" % (label[b[p]] & 0xFFFF, (label[b[p]] >> 16) & 0x7FFF)) for p in at]))
    return len(out), out[:6]


def _check(name, window, got, want):
    from tagdust_amd import lib as tdlib, RESULT_DTYPE
    segs, seq, offs, md = plan_shapes.case(name, window)
    ores, olab, oseq = want
    res, labels, seq_after, cnt = got[:4]
    why = lambda: (name, segs[0][:24], _differing(name, window, res, labels, ores, olab))
    for k in ("b_score", "f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k]), _bits(ores[k])), (k,) + why()
    assert np.array_equal(labels, olab), why()
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL), name
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), (k,) + why()
    assert np.array_equal(seq_after, oseq), name
    as_res = np.zeros(len(ores), RESULT_DTYPE)
    for k in ("read_type", "barcode", "fingerprint"):
        as_res[k] = ores[k]
    assert np.array_equal(cnt, tdlib.count_outcomes(as_res, np.diff(offs))), name
    for c_ in range(8):
        assert cnt[c_] == int(((ores["read_type"] & 0xFF) == c_).sum()), (name, c_)
    if len(got) > 4:
        assert np.array_equal(_bits(got[4]["f_score"]), _bits(ores["f_score"])), (name, "MODE_GET_PROB")
        assert np.allclose(got[4]["mapq"], ores["Q"], rtol=0, atol=Q_TOL), (name, "MODE_GET_PROB")
        assert np.array_equal(_bits(got[5]["b_score"]), _bits(ores["b_score"])), (name, "MODE_ARCH_COMP")


def _same_bytes(a, b, what):
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]), what


@pytest.mark.parametrize("name", plan_shapes.NAMES)
def test_shape_against_oracle(ctx, name):
    """Label run, then MODE_GET_PROB and MODE_ARCH_COMP on the resident batch; both kernels equal the oracle."""
    got = _decode(ctx, name)
    if ctx.get_option("specialize"):
        _DEFAULT[name] = got
    _check(name, None, got, plan_shapes.oracle(name))


def test_windowed_shape_a_against_oracle(ctx):
    """-start 3 -end 70 on shape A, three random bases in front of the architecture: the TDS_WINDOW variant of the specialised kernel
    (and the generic kernel's window branches) over two run-time-looped segments, in-sweep label sums and restarted sweeps."""
    w = plan_shapes.WINDOW
    _check("A", w, _decode(ctx, "A", w), plan_shapes.oracle("A", w))


def _default(name):
    """the specialised kernel's bytes under the default knobs: test_shape_against_oracle's, or (this test run alone) made here"""
    from tagdust_amd import TagdustHip
    if name not in _DEFAULT:
        c = TagdustHip(0)
        try:
            c.set_option("specialize", 1)
            c.set_option("poison_workspace", 1)
            _DEFAULT[name] = _decode(c, name)
        finally:
            c.close()
    return _DEFAULT[name]


@pytest.mark.parametrize("name,env,want", plan_shapes.KNOB_VARIANTS,
                         ids=["%s-%s" % (v[0], "-".join("%s=%s" % kv for kv in v[1].items())) for v in plan_shapes.KNOB_VARIANTS])
def test_knob_variant_gives_the_bytes_of_the_default(name, env, want, monkeypatch):
    """The TD_SPEC_* knobs are read when a model is uploaded: a fresh context per variant.  The knob moved the plan feature it is
    there for; the bytes are the default plan's and the oracle's."""
    from tagdust_amd import TagdustHip, lib as tdlib
    base = _default(name)
    md = plan_shapes.case(name)[3]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    p = plan_shapes.plan_features(tdlib.spec_source(md))
    for k, v in want.items():
        assert p[k] == v, (name, env, k, p[k])
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 1)
        c.set_option("poison_workspace", 1)
        got = _decode(c, name, modes=False)
    finally:
        c.close()
    _check(name, None, got, plan_shapes.oracle(name))
    _same_bytes(got, base, (name, env))


def test_pipelined_pass_on_shape_j():
    """Three td_submit tickets of the same batch in flight, compact egress (the default): the bytes of the synchronous path."""
    from tagdust_amd import TagdustHip, RESULT_DTYPE
    segs, seq, offs, md = plan_shapes.case("J")
    base = _default("J")
    n = len(offs) - 1
    seq, offs = np.ascontiguousarray(seq, np.uint8), np.ascontiguousarray(offs, np.int64)
    c = TagdustHip(0)
    try:
        c.set_option("specialize", 1)
        c.upload_model(md)
        c.set_params(float(md["threshold"]), int(md["minlen"]), int(md["dust"]))
        assert c.get_option("compact_egress") == 1
        outs = [(np.zeros(n, RESULT_DTYPE), np.zeros(int(offs[-1]) + n, np.int8), np.zeros(int(offs[-1]), np.uint8)) for _ in range(3)]
        tickets = [c.submit(seq, offs, res=r, labels=l, seq_out=s) for r, l, s in outs]
        for t in tickets:
            c.wait(t)
        assert c.get_option("spec_state") == 3 and c.get_option("spec_batches_generic") == 0
    finally:
        c.close()
    for k, (r, l, s) in enumerate(outs):
        assert r.tobytes() == base[0].tobytes() and np.array_equal(l, base[1]) and np.array_equal(s, base[2]), k
