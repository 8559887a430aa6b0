"""Waves that decode several tiles ("Slot reuse").

Both decode kernels run persistent waves: a wave slot owns one region of the workspace and decodes tile after tile in it.  The chip
has thousands of slots and the plan clips the slot count to the tile count, so a batch of fewer than 131 072 reads (generic kernel)
or 262 144 reads (specialised kernel) gives every wave exactly one tile, and nothing that only happens on a wave's second tile is
reached: the previous tile's finite scores, path words and posterior masks in the workspace (not the NaNs and all-ones masks of
"poison_workspace"), the adaptive state a wave of the specialised kernel carries from tile to tile, the shared tile counter, a
big-geometry slot that goes on with short tiles, and the candidates of td_arch_scores on a few slots each.  TD_WAVE_SLOTS (read when
a context is created) forces the slot count; here 8 or 16 slots decode 41 .. 165 tiles.  Every case shows that it is not vacuous:
batch_info()[2] is the forced slot count and the batch has at least 5 tiles per slot.

Reads without a path through the model (fewer bases than mandatory segments) are part of every batch.  For them the oracle's guard
states the device's rule (oracle/td_oracle.c: mismatch, Q = 0, b_score = -inf, the sequence as it was; "the other scores mean
nothing"), so f_score, r_score, bar_prob and the labels are compared on the reads that have a path and everything else on all reads,
as tests/test_parity_gpu.py::test_windowed_architectures_against_oracle does."""
import numpy as np
import pytest
import torch     # before the library is loaded: where torch brings a HIP runtime of its own, only the first one loaded sees the device

from conftest import load_golden, golden_window, GOLDEN_NAMES
from test_parity_gpu import _bits, Q_TOL
from test_prune import _same

pytestmark = pytest.mark.gpu

SLOTS = 8
N_RAGGED = 2600          # 41 tiles: at least 5 per slot on 8 slots
SEED_A, SEED_B, SEED_C = 11, 12, 13


def _ragged_batch(g, n, seed):
    """n reads for fixture g whose lengths run from 1 to the fixture's longest read, so that tiles sorted by length differ in tmax
    from one to the next: 45 % prefixes of the fixture's own reads (barcodes and UMIs are found), 25 % uniform random reads, 15 %
    reads with about 20 % N (on either kind), 8 % reads too short for any path (fewer bases than segments, behind the window's
    start when the fixture has one), 7 % 1-base reads; five whole fixture reads of the longest length in front."""
    rng = np.random.RandomState(seed)
    src, n0 = g["offs"], int(g["n_reads"])
    lmax = int(g["lens"].max())
    win = golden_window(g)
    ms = win[0] if win else 0
    longest = [k for k in range(n0) if int(g["lens"][k]) == lmax]
    reads = []
    for i in range(n):
        u = rng.random_sample()
        L = int(rng.randint(1, lmax + 1))
        k = int(rng.randint(n0))
        own = np.array(g["seq"][src[k]:src[k + 1]][:L], np.uint8)
        if i < 5:
            k = longest[i % len(longest)]
            r = np.array(g["seq"][src[k]:src[k + 1]], np.uint8)
        elif u < 0.45:
            r = own
        elif u < 0.70:
            r = rng.randint(0, 4, L).astype(np.uint8)
        elif u < 0.85:
            r = own if rng.random_sample() < 0.5 else rng.randint(0, 4, L).astype(np.uint8)
            r[rng.random_sample(len(r)) < 0.2] = 4
        elif u < 0.93:
            r = own[:ms + int(rng.randint(1, max(2, int(g["S"]))))]
        else:
            r = own[:1]
        reads.append(r)
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(np.int64)
    return np.concatenate(reads).astype(np.uint8), offs


_CASES = {}


def _case(name, seed, n=N_RAGGED):
    """(fixture, seq, offs, oracle results, oracle labels, oracle sequences) of one ragged batch: computed once, shared by both
    kernels and by the parts below, read-only.  The oracle is the restatement _windowed_oracle uses, under the fixture's window."""
    from oracle import pyoracle
    key = (name, seed, n)
    if key not in _CASES:
        g = load_golden(name)
        seq, offs = _ragged_batch(g, n, seed)
        o = pyoracle.label_batch(pyoracle.OracleModel(g), seq, offs, float(g["threshold"]), int(g["minlen"]), int(g["dust"]), 8,
                                 window=golden_window(g))
        for a in (seq, offs) + o:
            a.setflags(write=False)
        _CASES[key] = (g, seq, offs) + o
    return _CASES[key]


def _assert_mix(offs, ores, lmax):
    """the batch is what the docstrings say: every length class, reads without a path, and at least two outcomes"""
    lens = np.diff(offs)
    assert lens.min() == 1 and lens.max() == lmax
    assert (lens == 1).sum() >= 64 and len(np.unique(lens)) >= min(lmax, 60)
    assert np.isneginf(ores["b_score"]).sum() >= 64
    assert (ores["read_type"] == 0).sum() >= 64 and len(set(ores["read_type"].tolist())) >= 2


def _assert_oracle(got, offs, ores, olab, oseq, what=""):
    res, labels, seq_after = got
    nopath = np.isneginf(ores["b_score"])
    keep = ~nopath
    assert np.array_equal(_bits(res["b_score"]), _bits(ores["b_score"])), ("b_score", what)
    for k in ("f_score", "r_score", "bar_prob"):
        assert np.array_equal(_bits(res[k][keep]), _bits(ores[k][keep])), (k, what)
    assert (res["mapq"][nopath] == 0.0).all(), what
    assert np.allclose(res["mapq"], ores["Q"], rtol=0, atol=Q_TOL), what
    lab_keep = np.repeat(keep, np.diff(offs) + 1)
    assert np.array_equal(labels[lab_keep], olab[lab_keep]), ("labels", what)
    for k in ("read_type", "barcode", "fingerprint"):
        assert np.array_equal(res[k], ores[k]), (k, what)
    assert np.array_equal(seq_after, oseq), ("sequence", what)


def _assert_counters(cnt, ores, what=""):
    """device counters == serial counting over the oracle's outcomes (barcode_hmm.c:354-384)"""
    for code in range(8):
        assert cnt[code] == int(((ores["read_type"] & 0xFF) == code).sum()), (code, what)
    ok = (ores["read_type"] == 0) & (ores["barcode"] >= 0)
    assert np.array_equal(cnt[8:], np.bincount(ores["barcode"][ok] & 0xFF, minlength=256)), what


def _open(g, specialize, poison=1):
    """a context for fixture g under the environment as it stands now (TD_WAVE_SLOTS, TD_SPEC_*), its window set before the upload"""
    from tagdust_amd import TagdustHip
    c = TagdustHip(0)
    try:
        c.set_option("specialize", specialize)
        c.set_option("poison_workspace", poison)
        c.set_window(*(golden_window(g) or (-1, -1)))
        c.upload_model(g)
        c.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
    except Exception:
        c.close()
        raise
    return c


def _decode(c, seq, offs):
    c.upload_batch(seq, offs)
    c.counts_reset()
    c.run()
    return c.download()


# ---------------------------------------------------------------------------------------------------------------------
# 1. ragged batches on 8 wave slots, both kernels, against the oracle
# ---------------------------------------------------------------------------------------------------------------------
# c3_b6_s_r_p: leading and trailing segments, pruning and restarts; c2_b4_r; c5_b96_f_r_p: 100 labels, byte path and the label-DP
# row; b_r_s_r: two read segments; r_s_b_f: free order, ends in a UMI; plan_a_b16_s_b24_r; win_r_s_b_r: the TDS_WINDOW variant,
# where lenF / tmaxF differ from len / tmax
_ARCHS = ["c3_b6_s_r_p", "c2_b4_r", "c5_b96_f_r_p", "b_r_s_r", "r_s_b_f", "plan_a_b16_s_b24_r", "win_r_s_b_r"]


@pytest.mark.parametrize("specialize", [1, 0], ids=["specialised", "generic"])
@pytest.mark.parametrize("name", _ARCHS)
def test_ragged_batches_on_eight_wave_slots(name, specialize, monkeypatch):
    """41 tiles of lengths 1 .. the fixture's longest read on 8 wave slots: every wave decodes five tiles or so in one workspace
    region, the generic kernel shortest first (rows beyond the previous tile's tmax hold older tiles' values), the specialised one
    longest first (rows beyond the current tmax hold a longer tile's values).  The first batch starts on a poisoned workspace, the
    second -- other reads, the lengths drawn again -- on what the first left behind ("poison_workspace" 0).  Both equal the oracle
    bit for bit (Q within Q_TOL), and the device counters equal serial counting over the oracle's outcomes."""
    monkeypatch.setenv("TD_WAVE_SLOTS", str(SLOTS))
    g, seq_a, offs_a, ores_a, olab_a, oseq_a = _case(name, SEED_A)
    _, seq_b, offs_b, ores_b, olab_b, oseq_b = _case(name, SEED_B)
    assert (golden_window(g) is not None) == (name == "win_r_s_b_r")
    _assert_mix(offs_a, ores_a, int(g["lens"].max()))
    _assert_mix(offs_b, ores_b, int(g["lens"].max()))
    assert not np.array_equal(np.diff(offs_a), np.diff(offs_b))
    tiles = (N_RAGGED + 63) // 64
    assert tiles >= 5 * SLOTS
    c = _open(g, specialize, poison=1)
    try:
        got_a = _decode(c, seq_a, offs_a)
        cnt_a = c.counts()
        assert c.batch_info()[2] == SLOTS
        c.set_option("poison_workspace", 0)
        got_b = _decode(c, seq_b, offs_b)
        cnt_b = c.counts()
        assert c.batch_info()[2] == SLOTS
        assert c.get_option("spec_batches_generic") == (0 if specialize else 2)      # the kernel the case names decoded both
    finally:
        c.close()
    _assert_oracle(got_a, offs_a, ores_a, olab_a, oseq_a, (name, "first batch"))
    _assert_counters(cnt_a, ores_a, (name, "first batch"))
    _assert_oracle(got_b, offs_b, ores_b, olab_b, oseq_b, (name, "second batch"))
    _assert_counters(cnt_b, ores_b, (name, "second batch"))


# ---------------------------------------------------------------------------------------------------------------------
# 2. carried adaptive state of the specialised kernel
# ---------------------------------------------------------------------------------------------------------------------
def _spec_run(monkeypatch, env, g, seq, offs):
    """One batch through a fresh specialised context compiled under `env` on 8 wave slots: (res, labels, seq, diagnostic words
    -- td_diag_get, word k = slot 192 + k --, wave slots used)."""
    with monkeypatch.context() as m:
        m.setenv("TD_WAVE_SLOTS", str(SLOTS))
        for k in ("TD_SPEC_PRUNE", "TD_SPEC_PRUNE_STATS", "TD_SPEC_RESTART", "TD_SPEC_EXTRA_OPTS"):
            m.delenv(k, raising=False)
        for k, v in env.items():
            m.setenv(k, v)
        c = _open(g, 1, poison=1)
        try:
            got = _decode(c, seq, offs)
            return got + (c.diag(), c.batch_info()[2])
        finally:
            c.close()


_DENSE = {}


def _dense(monkeypatch):
    """the ragged batch of part 1 through a context that does not prune (TD_SPEC_PRUNE=0), once for all knob sets"""
    if "c3" not in _DENSE:
        g, seq, offs = _case("c3_b6_s_r_p", SEED_A)[:3]
        _DENSE["c3"] = _spec_run(monkeypatch, {"TD_SPEC_PRUNE": "0", "TD_SPEC_PRUNE_STATS": "0"}, g, seq, offs)
    return _DENSE["c3"]


_KNOBS = {
    # the window of the backward bridges widens on the first tiles; later tiles of the same wave restart with the widened window
    "backward-window": {"TD_SPEC_RESTART": "1", "TD_SPEC_EXTRA_OPTS": "-DTDS_RESTART_W=2"},
    # the restarts are given up (restart_on = false); later tiles of the wave are pruned without them
    "backward-given-up": {"TD_SPEC_RESTART": "1", "TD_SPEC_EXTRA_OPTS": "-DTDS_RESTART_W=2 -DTDS_RESTART_WMAX=2"},
    # the forward window widens once (w.rWf += 12) and is then given up (n_fwd_fail, restart_fwd_on = false)
    "forward-window": {"TD_SPEC_RESTART": "1", "TD_SPEC_EXTRA_OPTS": "-DTDS_RESTART_WF=2"},
    # bgap grows by 40 per miss; later tiles guess their spill cut with the grown value
    "spill-cut": {"TD_SPEC_EXTRA_OPTS": "-DTDS_PRUNE_BGAP=-150.0f -DTDS_PRUNE_MARGIN=0"},
    # n_fallback * 4 > n_tiles_done + 4 switches pruning off from a wave's third tile on
    "total-prob": {"TD_SPEC_EXTRA_OPTS": "-DTDS_PRUNE_TT=1000.0f"},
}


@pytest.mark.parametrize("knobs", list(_KNOBS), ids=list(_KNOBS))
def test_carried_state_acts_on_later_tiles(knobs, monkeypatch):
    """A wave of the specialised kernel carries a widened backward window (w.rW), restart_on = false, a widened forward window
    (w.rWf), restart_fwd_on = false, a grown bgap and prune_on = false from tile to tile.  The forced-knob tests of tests/test_prune.py
    trigger each event with one tile per wave, so no tile is decoded under the changed state; here 8 waves decode the 41 ragged tiles
    of part 1 (config-3 architecture: leading segments, so the backward bridges exist, and a 3' adapter, so the forward ones do).
    Every knob set gives the bytes of a context that does not prune, and the oracle's; the diagnostic words show that the changed
    state acted on later tiles.  Which tiles a wave gets after its first is decided by an atomic counter: bounds, not counts."""
    g, seq, offs, ores, olab, oseq = _case("c3_b6_s_r_p", SEED_A)
    tiles = (len(offs) - 1 + 63) // 64
    assert tiles >= 5 * SLOTS
    env = dict(_KNOBS[knobs], TD_SPEC_PRUNE="1", TD_SPEC_PRUNE_STATS="1")
    dense = _dense(monkeypatch)
    got = _spec_run(monkeypatch, env, g, seq, offs)
    assert dense[4] == SLOTS and got[4] == SLOTS
    d = {k: int(got[3][k - 192]) for k in (198, 199, 206, 207, 224, 226, 232, 234, 235, 236, 238)}
    print("diagnostic words (%s): %s" % (knobs, d))
    assert _same(dense, got)
    _assert_oracle(got[:3], offs, ores, olab, oseq, knobs)
    assert d[236] == tiles                  # every tile took the pruning decision (word 236 is counted once per tile)
    if knobs == "backward-window":
        # Word 206 counts every restarted backward pass, word 207 those a bridge left open.  W = 2 cannot close a bridge, so the first
        # restarted tile of a wave is left open: at least 1.  Every open pass is followed by another pass of the same tile; while
        # w.rW + 8 <= TDS_RESTART_WMAX that pass restarts again with the wider window, and once the bridges close it is counted in
        # 206 alone -- as is every later tile of the wave, which starts from the widened w.rW: open < restarted.  A wave whose
        # window had stayed at 2 would have every restarted pass open (206 == 207).  No tile needs the dense second pass.
        assert d[207] >= 1
        assert d[207] < d[206]
        assert d[238] == 0
    elif knobs == "backward-given-up":
        # TDS_RESTART_WMAX = 2: the first open bridge sets restart_on = false (w.rW + 8 > WMAX), so a wave leaves exactly one pass
        # open -- its first tile is one of the batch's 8 longest, where the bridges fit in front of the cut: at least the slot
        # count -- and never restarts again: at most one per wave, fewer than the tiles (5 per wave).
        assert d[207] >= SLOTS
        assert d[207] < tiles
    elif knobs == "forward-window":
        # Word 199 counts forward bridges that did not close.  From a window of 2 the first one of a wave cannot: at least 1.  The
        # first failure widens w.rWf by 12, the second sets restart_fwd_on = false: at most two per wave.
        assert d[199] >= 1
        assert d[199] <= 2 * SLOTS
    elif knobs == "spill-cut":
        # Word 234 / 226 count spill cuts / stops guessed too short; each costs a dense pass and adds 40 to bgap.  A fall-back at a
        # wave's d-th tile needs pruning still on: 4 (f - 1) <= (d - 1) + 4, so a wave of t tiles falls back at most t / 4 + 2
        # times -- over all waves fewer than the tiles.
        assert d[234] + d[226] >= 1
        assert d[234] + d[226] <= tiles // 4 + 2 * SLOTS < tiles
    else:
        # Every pruned pass fails its total_prob check (word 235) and is repeated densely (word 238).  A wave's first tile -- given
        # by slot number -- fails: at least the slot count.  After two failures n_fallback * 4 = 8 > n_tiles_done + 4 = 6, prune_on
        # is false and the wave's later tiles are dense from the start, without a failed check: two per wave, fewer than the tiles.
        assert d[238] == tiles
        assert d[235] >= SLOTS
        assert d[235] < tiles


# ---------------------------------------------------------------------------------------------------------------------
# 3. tickets in flight on few slots
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [1, 0], ids=["two-workspaces", "one-workspace"])
def test_three_tickets_in_flight_on_eight_slots(overlap, monkeypatch):
    """Three tickets of three different ragged batches (41 tiles each) are submitted before the first wait, on 8 wave slots: with
    "overlap_decode" they use both workspaces and both tile counters, and the third lands on the first workspace and its counter
    again -- which the launch must have reset.  Every ticket equals the synchronous upload / run / download of its batch, and the
    third one the oracle."""
    from tagdust_amd import RESULT_DTYPE
    monkeypatch.setenv("TD_WAVE_SLOTS", str(SLOTS))
    cases = [_case("c3_b6_s_r_p", s) for s in (SEED_A, SEED_B, SEED_C)]
    g = cases[0][0]
    c, ref = _open(g, 1, poison=0), _open(g, 1, poison=0)
    try:
        c.set_option("pipeline_depth", 3)
        c.set_option("overlap_decode", overlap)
        outs = []
        for _, seq, offs, _, _, _ in cases:
            n = len(offs) - 1
            assert (n + 63) // 64 >= 5 * SLOTS
            res, lab, sq = np.zeros(n, RESULT_DTYPE), np.full(int(offs[-1]) + n, 99, np.int8), np.full(int(offs[-1]), 99, np.uint8)
            outs.append((res, lab, sq, c.submit(seq, offs, res=res, labels=lab, seq_out=sq)))
        for o in outs:
            c.wait(o[3])
            assert c.batch_info()[2] == SLOTS
        assert c.get_option("overlap_active") == overlap
        for (_, seq, offs, _, _, _), o in zip(cases, outs):
            want = _decode(ref, seq, offs)
            assert ref.batch_info()[2] == SLOTS
            assert _same(want, o[:3])
    finally:
        c.close()
        ref.close()
    _, _, offs, ores, olab, oseq = cases[2]
    _assert_oracle(outs[2][:3], offs, ores, olab, oseq, "third ticket")


# ---------------------------------------------------------------------------------------------------------------------
# 4. a big-geometry slot that goes on with short tiles
# ---------------------------------------------------------------------------------------------------------------------
def test_big_slot_goes_on_with_short_tiles(monkeypatch):
    """Length classes on 16 wave slots: 165 tiles of 30 .. 100 bases and 20 reads of 200 bases -- under 1 % of the batch, twice the
    99 % mark -- make one long tile, which gets slot 0 with the geometry of the longest read (lay_big / lmax_big).  With ten tiles
    per slot that slot takes further, short tiles from the counter after its long one and decodes them in the big geometry: by
    construction, not observed -- the kernel does not report which slot decoded a tile.  The bytes equal one geometry for all
    (TD_NO_LENGTH_CLASSES=1) and the oracle on every read."""
    from oracle import pyoracle
    slots = 16
    g = load_golden("c3_b6_s_r_p")
    rng = np.random.RandomState(41)
    src, n0 = g["offs"], int(g["n_reads"])
    n, n_long = 165 * 64, 20
    reads = []
    for i in range(n):
        k = int(rng.randint(n0))
        own = np.array(g["seq"][src[k]:src[k + 1]], np.uint8)
        if i % (n // n_long) == 7:          # the fixture's read with 50 more bases in its read segment (which starts at position 9)
            r = np.concatenate([own[:20], rng.randint(0, 4, 50).astype(np.uint8), own[20:]])
        else:
            r = own[:int(rng.randint(30, 101))]
            u = rng.random_sample()
            if u < 0.2:
                r = rng.randint(0, 4, len(r)).astype(np.uint8)
            elif u < 0.3:
                r[rng.random_sample(len(r)) < 0.2] = 4
        reads.append(r)
    lens = np.array([len(r) for r in reads])
    assert (lens == 200).sum() == n_long and lens[lens < 200].max() == 100 and lens.min() == 30
    assert n_long * 100 < n and 200 * 2 >= 3 * np.sort(lens)[int(0.99 * n)]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    seq = np.concatenate(reads).astype(np.uint8)
    tiles = (n + 63) // 64
    assert tiles >= 160 and tiles >= 5 * slots
    ores, olab, oseq = pyoracle.label_batch(pyoracle.OracleModel(g), seq, offs, float(g["threshold"]), int(g["minlen"]), int(g["dust"]), 8)
    monkeypatch.setenv("TD_WAVE_SLOTS", str(slots))

    def run(no_classes):
        if no_classes:
            monkeypatch.setenv("TD_NO_LENGTH_CLASSES", "1")
        else:
            monkeypatch.delenv("TD_NO_LENGTH_CLASSES", raising=False)
        c = _open(g, 1, poison=1)
        try:
            return _decode(c, seq, offs), c.get_option("length_classes"), c.batch_info()[2]
        finally:
            c.close()

    one, k1, s1 = run(True)
    two, k2, s2 = run(False)
    assert k1 == 0 and k2 >= 1                  # (one long tile: n_long x 4 <= slots holds, and it keeps its geometry)
    assert s1 == slots and s2 == slots
    assert _same(one, two)
    _assert_oracle(two, offs, ores, olab, oseq, "length classes")


# ---------------------------------------------------------------------------------------------------------------------
# 5. td_arch_scores: distinct candidates, more tiles than slots per candidate
# ---------------------------------------------------------------------------------------------------------------------
def test_arch_scores_distinct_candidates_reuse_their_slots():
    """td_decode_multi_kernel gives each candidate wave_budget / n_candidates slots: with a quarter as many candidates as the chip
    has CUs that is at most 32, and a ragged batch of 97 tiles makes every slot decode three tiles.  The candidates are all fixture
    models in a shuffled order, repeated: neighbours differ in S, H, C and workspace layout, so an argument block, workspace offset
    or output row taken from a neighbour shows.  Each row equals, bit for bit, a TD_MODE_ARCH_COMP run of that model alone on the
    generic kernel, and three of the models the oracle's b_score."""
    from oracle import pyoracle
    from tagdust_amd import TagdustHip, MODE_ARCH_COMP
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n_models = max(1, -(-n_cu // 4))
    per = (n_cu * 2 * 4 // n_models) // 4 * 4
    assert 4 <= per <= 32
    g, seq, offs = _case("c3_b6_s_r_p", SEED_C, 6200)[:3]
    tiles = (len(offs) - 1 + 63) // 64
    assert tiles >= 3 * per
    order = list(np.random.RandomState(5).permutation(len(GOLDEN_NAMES)))
    names = [GOLDEN_NAMES[order[k % len(order)]] for k in range(n_models)]
    distinct = {n_: load_golden(n_) for n_ in set(names)}
    assert all(a != b for a, b in zip(names, names[1:]))
    assert len({(int(m["S"]), int(m["H"]), int(m["C"])) for m in distinct.values()}) >= 10
    c = TagdustHip(0)
    try:
        got = c.arch_scores([distinct[n_] for n_ in names], seq, offs)
        assert got.shape == (n_models, len(offs) - 1)
        c.set_option("specialize", 0)
        alone = {}
        for n_, m in distinct.items():
            c.upload_model(m)
            c.set_params(0.0, 16, 100)
            c.upload_batch(seq, offs)
            c.run(MODE_ARCH_COMP)
            alone[n_] = c.download(labels=False, seq=False)[0]["b_score"].copy()
    finally:
        c.close()
    for k, n_ in enumerate(names):
        assert np.array_equal(_bits(got[k]), _bits(alone[n_])), (k, n_)
    for n_ in ("c3_b6_s_r_p", "r_s_b_f", "plan_a_b16_s_b24_r"):
        ores = pyoracle.label_batch(pyoracle.OracleModel(distinct[n_]), seq, offs, 0.0, 16, 100, 8)[0]
        assert np.array_equal(_bits(got[names.index(n_)]), _bits(ores["b_score"])), n_
