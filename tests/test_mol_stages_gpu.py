"""The stages behind the molecule count (tagdust_amd/csrc/td_molecules.hip: count, origin pass, dedup's two passes, replay, mate
kernel) over the smallest batches -- none, one read (a partial wave), 65 reads (a full wave and one lane) -- on the generic kernel:
what every "*_kernel_us" option of td_get_option refuses with and answers, and dedup's and the frozen state's totals against
td_mol_dedup_host / td_mol_dedup_collapsed_host fed with the CPU oracle's records for the same reads in the same order
(oracle/pyoracle.py), never the device's own output.

The shape is b_r of tests/test_molecules_gpu.py wherever the stage allows it.  The collapse refuses a model without an 'F' segment
(td_mol_collapse_enable), so everything that needs the collapse on -- its origin pass, the freeze, the replay -- runs on b_f_r, the
same reads with a UMI of 5 behind the barcode.  The refusals' texts are written out here in full, not taken from the library."""
import numpy as np
import pytest

from test_molecules_gpu import MINLEN, SHAPES, THRESHOLD, make_reads, pack

pytestmark = pytest.mark.gpu

N = 66                      # reads of a case: batches of 1 (read 0) and of 65 (reads 1..65)
BATCHES = [(0, 1), (1, N)]
P = {"b_r": 20, "b_f_r": 16}
M = 8                       # mate bases (P + M <= 32)

OFF = {"molecules_kernel_us": "td_get_option: molecules_kernel_us: the molecule count is off",
       "dedup_kernel_us": "td_get_option: dedup_kernel_us: dedup is off",
       "collapse_origin_kernel_us": "td_get_option: collapse_origin_kernel_us: the collapse is off",
       "dedup_replay_kernel_us": "td_get_option: dedup_replay_kernel_us: the context is not frozen (td_mol_dedup_freeze)",
       "mate_kernel_us": "td_get_option: mate_kernel_us: mate mode is off"}
NONE_YET = {"molecules_kernel_us": "td_get_option: molecules_kernel_us: no batch has been counted yet",
            "dedup_kernel_us": "td_get_option: dedup_kernel_us: no batch has been judged yet",
            "collapse_origin_kernel_us": "td_get_option: collapse_origin_kernel_us: no batch has left its origins yet",
            "dedup_replay_kernel_us": "td_get_option: dedup_replay_kernel_us: no batch has been replayed yet",
            "mate_kernel_us": "td_get_option: mate_kernel_us: no mate batch has been staged yet"}
# Two events recorded back to back on an idle stream, no launch between them: a few microseconds at the most.  A millisecond is
# hundreds of times that, and still says that nothing was waited for inside the bracket.
EMPTY_BRACKET_US = 1000

_CASES = {}


def case(shape):
    """(model, seq, offs, threshold, minlen, the oracle's records and labels, mate codes, mate offs) of the first N reads of
    test_molecules_gpu.make_reads under the model of all of them; a mate of 40 random bases per read.  Computed once."""
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    if shape not in _CASES:
        seq, offs = make_reads(shape, 5)
        md, _ = tdlib.build_model(SHAPES[shape], seq, offs)
        seq, offs = seq[:offs[N]].copy(), offs[:N + 1].copy()
        thr, minlen = THRESHOLD.get(shape, 5.0), MINLEN.get(shape, 16)
        ores, olab, _ = pyoracle.label_batch(pyoracle.OracleModel(md), seq, offs, thr, minlen, 100, 2)
        res = {f: np.asarray(ores[f]).copy() for f in ("read_type", "barcode", "fingerprint")}
        mates = np.random.default_rng(77).integers(0, 4, (N, 40), dtype=np.uint8)
        _CASES[shape] = (md, seq, offs, thr, minlen, res, olab) + pack(list(mates))
    return _CASES[shape]


def in_order(c, order):
    """(md, seq, offs, res, labels) as the host yardsticks take them: the case's reads, records and labels in `order`"""
    md, seq, offs, _, _, res, lab = c[:7]
    rseq, roffs = pack([seq[offs[i]:offs[i + 1]] for i in order])
    rlab = np.concatenate([lab[offs[i] + i:offs[i + 1] + i + 1] for i in order]).astype(np.int8)
    return md, rseq, roffs, {f: v[order] for f, v in res.items()}, rlab


def make_ctx(c, prefix, dedup=False, collapse=False, count=True):
    from tagdust_amd import TagdustHip
    md, _, _, thr, minlen = c[:5]
    ctx = TagdustHip(0)
    try:
        ctx.set_option("specialize", 0)
        ctx.upload_model(md)
        ctx.set_params(thr, minlen, 100)
        if count:
            ctx.mol_enable(prefix, 16)
        if collapse:
            ctx.mol_collapse_enable()
        if dedup:
            ctx.mol_dedup_enable()
    except Exception:
        ctx.close()
        raise
    return ctx


def run_batch(ctx, c, lo, hi, mate=False):
    """one td_run batch of reads lo..hi (lo == hi: no reads), behind its mates when mate mode is on: the records as downloaded"""
    _, seq, offs = c[:3]
    if mate:
        mc, mo = c[7], c[8]
        ctx.mol_mate_next(mc[mo[lo]:mo[hi]], mo[lo:hi + 1] - mo[lo])
    ctx.upload_batch(seq[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo])
    ctx.run()
    return ctx.download()[0]


def refusal(ctx, name):
    from tagdust_amd import TdError
    with pytest.raises(TdError) as e:
        ctx.get_option(name)
    return str(e.value)


# ---- the refusals, word for word ----
def test_every_option_refuses_in_its_own_words_while_off_and_before_any_batch():
    ctx = make_ctx(case("b_r"), P["b_r"], count=False)
    try:
        for name in OFF:                                  # no count: every stage is off
            assert refusal(ctx, name) == OFF[name]
        ctx.mol_enable(P["b_r"], 16)
        assert refusal(ctx, "molecules_kernel_us") == NONE_YET["molecules_kernel_us"]
        for name in ("dedup_kernel_us", "collapse_origin_kernel_us", "dedup_replay_kernel_us", "mate_kernel_us"):
            assert refusal(ctx, name) == OFF[name]
        ctx.mol_dedup_enable()
        ctx.mol_mate_enable(M)
        for name in ("molecules_kernel_us", "dedup_kernel_us", "mate_kernel_us"):
            assert refusal(ctx, name) == NONE_YET[name]
        for name in ("collapse_origin_kernel_us", "dedup_replay_kernel_us"):
            assert refusal(ctx, name) == OFF[name]
    finally:
        ctx.close()
    ctx = make_ctx(case("b_f_r"), P["b_f_r"], dedup=True, collapse=True)
    try:
        for name in ("molecules_kernel_us", "dedup_kernel_us", "collapse_origin_kernel_us"):
            assert refusal(ctx, name) == NONE_YET[name]
        assert refusal(ctx, "dedup_replay_kernel_us") == OFF["dedup_replay_kernel_us"]
        ctx.mol_dedup_freeze()                            # (of an empty table)
        assert refusal(ctx, "dedup_replay_kernel_us") == NONE_YET["dedup_replay_kernel_us"]
        ctx.mol_collapse_disable()                        # ends the frozen state with it
        assert refusal(ctx, "dedup_replay_kernel_us") == OFF["dedup_replay_kernel_us"]
        assert refusal(ctx, "collapse_origin_kernel_us") == OFF["collapse_origin_kernel_us"]
        assert refusal(ctx, "dedup_kernel_us") == NONE_YET["dedup_kernel_us"]
    finally:
        ctx.close()


# ---- what the options answer after a batch, and after an empty one ----
def check_answers(ctx, names, run_65, run_empty):
    run_65()
    before = {name: ctx.get_option(name) for name in names}
    print("after 65 reads", before)
    assert all(v >= 0 for v in before.values())
    run_empty()
    after = {name: ctx.get_option(name) for name in names}
    print("after no reads", after)
    for name in names:
        if name == "dedup_kernel_us":                     # an empty batch does not record dedup's pair: the 65 reads' figure stands
            assert after[name] == before[name]
        else:                                             # ... and no other pair has a launch between its events
            assert 0 <= after[name] <= EMPTY_BRACKET_US
    # The mate kernel's pair is recorded by the staging, launch or none.  The pairs on the compute stream are not recorded at all:
    # td_run returns from a batch without tiles before it reaches the count's launches, so their figures stand like dedup's.
    for name in names:
        if name != "mate_kernel_us":
            assert after[name] == before[name]


def test_the_options_answer_after_a_batch_and_after_an_empty_one():
    c = case("b_r")
    ctx = make_ctx(c, P["b_r"], dedup=True)
    try:
        ctx.mol_mate_enable(M)
        check_answers(ctx, ["molecules_kernel_us", "dedup_kernel_us", "mate_kernel_us"], lambda: run_batch(ctx, c, 1, N, mate=True),
                      lambda: run_batch(ctx, c, 0, 0, mate=True))
        tot = ctx.mol_dedup_get()
        assert tot["kept"] + tot["duplicates"] == ctx.mol_entries()[1]["eligible"] > 0
    finally:
        ctx.close()
    c = case("b_f_r")
    ctx = make_ctx(c, P["b_f_r"], dedup=True, collapse=True)
    try:
        check_answers(ctx, ["molecules_kernel_us", "dedup_kernel_us", "collapse_origin_kernel_us"], lambda: run_batch(ctx, c, 1, N),
                      lambda: run_batch(ctx, c, 0, 0))
        ctx.mol_dedup_freeze()
        check_answers(ctx, ["dedup_replay_kernel_us"], lambda: run_batch(ctx, c, 1, N), lambda: run_batch(ctx, c, 0, 0))
    finally:
        ctx.close()


# ---- dedup, then the frozen state, over the small batches ----
def test_dedup_and_the_replay_over_one_read_and_65_equal_the_yardsticks():
    from tagdust_amd import lib as tdlib
    c = case("b_f_r")
    prefix = P["b_f_r"]
    parts = BATCHES + [BATCHES[1]]                        # one read, 65 reads, the 65 again
    w = in_order(c, np.concatenate([np.arange(lo, hi) for lo, hi in parts]))
    want, want_tot = tdlib.mol_dedup_host(*w, prefix)
    fwant, fwant_tot, fwant_ctot = tdlib.mol_dedup_collapsed_host(*w, prefix)
    mtot = tdlib.mol_host(*w, prefix)[1]
    print("yardsticks", mtot, want_tot, fwant_tot, fwant_ctot)
    assert mtot["overflow"] == 0 and mtot["counted"] >= 0.7 * len(want)
    assert want_tot["duplicates"] >= 0.4 * mtot["eligible"] and want_tot["kept"] > 0   # (the second 65 are duplicates wherever counted)
    assert fwant_tot["duplicates"] > 0 and fwant_tot["kept"] > 0
    lens = np.diff(c[2])[1:N]
    assert not np.array_equal(np.argsort(lens, kind="stable"), np.arange(N - 1))   # the device sorts the 65: read_at is in use
    ctx = make_ctx(c, prefix, dedup=True, collapse=True)
    try:
        got = np.concatenate([run_batch(ctx, c, lo, hi) for lo, hi in parts])
        assert np.array_equal((got["read_type"] & 0xFF) == 7, want)
        assert ctx.mol_dedup_get() == want_tot
        assert ctx.mol_entries()[1] == mtot
        assert ctx.mol_dedup_freeze() == fwant_ctot
        got = np.concatenate([run_batch(ctx, c, lo, hi) for lo, hi in parts])
        assert np.array_equal((got["read_type"] & 0xFF) == 7, fwant)
        assert ctx.mol_dedup_get() == fwant_tot
        assert ctx.mol_entries()[1] == mtot               # the table is read-only: the count's tallies stay the survey's
    finally:
        ctx.close()
