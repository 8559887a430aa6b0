"""The mate filter on the device (include/tagdust_molecules.h, td_mol_mate_filter_enable; tagdust_amd/csrc/td_mate_filter.hip): the
mates of a TD_MODE_GET_LABEL batch judged as TD_MODE_RNA_DUST judges a batch, and the verdict joined to the read's outcome in front
of everything that reads a batch's outcomes.

The yardsticks are never the filter's own output: the mate types come from the CPU oracle's match_to_reference per thread range and
DUST restated in Python (tests/test_rna_dust_gpu.py), and from TD_MODE_RNA_DUST over the same mates in a second context; everything
behind the join comes from the *_mated host functions over the oracle's records with read_type replaced by the joined value."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_dedup_gpu import records_of
from test_mate_gpu import MATE_SHAPES, make_ctx, part, run_batch
from test_mate_gpu import case as mate_case
from test_molecules_gpu import code, fastq_of, pack, pairs, _outputs, _run
from test_rna_dust_gpu import COMP, RBIN, _artifacts, _dust_low, _fasta, _leftovers, _window

pytestmark = pytest.mark.gpu

P, M = 12, 20
LENS = [0, 1, 2, 3, 30, 31, 32, 62, 63, 64, 65, 100, 127, 128, 130, 200]
ONE = np.zeros(1, np.uint8)
_ART = {}
_JOIN = {}


def artifacts(seed=41):
    """(FASTA text, code arrays, string, s_index) of 13 artifact sequences, made once"""
    if seed not in _ART:
        text, seqs = _artifacts(np.random.default_rng(seed))
        _ART[seed] = (text, seqs) + _fasta(text)
    return _ART[seed]


# ---- t2: the yardsticks ----
def t2_restated(mates, art, T, dust, first=0, total=0):
    """What TD_MODE_RNA_DUST leaves in read_type for these mates as reads first.. of a batch of `total` (0: the batch is these):
    tdo_match_artifacts per thread range, then DUST restated.  Returns (types, usable): an empty mate is no FASTQ record, the oracle
    is not asked about it (usable False) unless there is no filter -- then it is 0."""
    from oracle import pyoracle
    n = len(mates)
    N = total if total else n
    want = np.zeros(n, np.int32)
    usable = np.ones(n, bool)
    if art is not None:
        L = pyoracle.lib()
        L.tdo_match_artifacts.restype = None
        L.tdo_match_artifacts.argtypes = [C.POINTER(pyoracle._Artifacts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]
        string, s_index = art
        usable = np.array([len(m) > 0 for m in mates])
        full = [ONE] * first + [m if len(m) else ONE for m in mates] + [ONE] * (N - first - n)
        codes, offs = pack(full)
        codes = np.minimum(codes, 4).astype(np.uint8)            # (the reference knows one N, 4: any byte above 3 is an N here)
        a = pyoracle._Artifacts(string.ctypes.data, s_index.ctypes.data, len(s_index) - 1, 2)
        ores = np.zeros(N, pyoracle.RESULT_DTYPE)
        work = codes.copy()
        interval = N // T
        for t in range(T):
            lo = t * interval
            hi = N if t == T - 1 else lo + interval
            L.tdo_match_artifacts(C.byref(a), work.ctypes.data, offs.ctypes.data, ores.ctypes.data, lo, hi)
        assert np.array_equal(work, codes)
        want = ores["read_type"][first:first + n].astype(np.int32)
    for i, m in enumerate(mates):
        if dust and _dust_low(m, dust):
            want[i] = 6
    return want, usable


def t2_mode(ctx, mates, art, T, dust, first=0, total=0):
    """TD_MODE_RNA_DUST over the mates as a batch of their own, given as codes, in a context without a model"""
    from tagdust_amd import lib as tdlib
    mc, mo = pack(list(mates) + [np.zeros(0, np.uint8)])
    mo = mo[:-1]
    ctx.set_params(0.0, 16, dust)
    if art is None:
        ctx.set_artifacts(None)
    else:
        ctx.set_artifacts(art[0], art[1], 2, T)
    ctx.set_batch_window(first, total)
    res = np.zeros(len(mates), tdlib.RESULT_DTYPE)
    mc = mc if len(mc) else np.zeros(1, np.uint8)
    ctx.wait(ctx.submit(mc, mo, mode=tdlib.MODE_RNA_DUST, res=res))
    return res["read_type"].astype(np.int32)


def t2_filter(ctx, c, mates, art, T, dust, first=0, total=0):
    """td_mol_mate_types of a resident batch of len(mates) reads of case c with these mates"""
    p = part(c, 0, len(mates))
    mc, mo = pack(list(mates) + [np.zeros(0, np.uint8)])
    ctx.set_params(c[3], c[4], dust)
    if art is None:
        ctx.set_artifacts(None)
    else:
        ctx.set_artifacts(art[0], art[1], 2, T)
    ctx.set_batch_window(first, total)
    ctx.mol_mate_next(mc, mo[:-1])
    ctx.upload_batch(p[1], p[2])
    return ctx.mol_mate_types()


def mate_batch(rng, seqs, n, left):
    """n mates: every length of LENS, an N inside the first 64 bases, an N in the last 63, all-N mates, poly-A and a dinucleotide
    repeat, artifact windows of both strands at the head and at the tail; short exact windows on the positions `left`, where
    bpm_check_error finds them"""
    pool = [rng.integers(0, 4, L, dtype=np.uint8) for L in LENS]
    s = rng.integers(0, 4, 100, dtype=np.uint8); s[10] = 4; pool.append(s)                  # an N inside the first 64 bases
    s = rng.integers(0, 4, 130, dtype=np.uint8); s[130 - 20] = 4; pool.append(s)            # ... in the last 63
    s = rng.integers(0, 4, 64, dtype=np.uint8); s[63] = 9; s[0] = 7; pool.append(s)         # ... at both ends of a 64-base mate
    pool.append(np.full(80, 4, np.uint8))                                                   # all N
    pool.append(np.full(3, 7, np.uint8))                                                    # all N, another byte (7 & 3 = 3)
    pool.append(np.zeros(150, np.uint8))                                                    # poly-A
    pool.append(np.tile(np.array([2, 3], np.uint8), 40))                                    # (GT)40
    s = rng.integers(0, 4, 64, dtype=np.uint8); s[30:] = 0; s[40] = 4; pool.append(s)       # low complexity with an N inside
    for L in (76, 63, 70, 90):
        pool.append(_window(rng, seqs, L))                                                  # a window, either strand, 0-3 substitutions
        w = _window(rng, seqs, L, subs=False)
        pool.append(np.concatenate([rng.integers(0, 4, 20, dtype=np.uint8), COMP[w[::-1]]]))   # behind 20 other bases: the last 63 match
        pool.append(np.concatenate([w, rng.integers(0, 4, 30, dtype=np.uint8)]))            # in front of 30 other bases: the first 63 match
    order = rng.permutation(len(pool))
    mates = [pool[order[i % len(pool)]].copy() for i in range(n)]
    for k, i in enumerate(left):
        if k % 3 != 2:
            mates[i] = _window(rng, seqs, int(rng.integers(8, 32)), subs=False)
    return mates


SETTINGS = [("dust", 100, False), ("ref", 0, True), ("both", 100, True), ("both-dust20", 20, True)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_the_mate_types_equal_rna_dust_mode_and_the_oracle(n):
    from tagdust_amd import TagdustHip
    _, seqs, string, s_index = artifacts()
    c = mate_case("b_f_r", M)
    fctx = make_ctx(c, P, M)
    mctx = TagdustHip(0)
    seen = {"dust": 0, "art": 0, "art_left": 0, "art_four": 0, "left": 0, "empty": 0}
    try:
        fctx.mol_mate_filter_enable()
        assert fctx.get_option("mate_filter") == 1
        windows = [(T, 0, 0) for T in (1, 3, 8)] + [(3, 13, n + 37), (8, 5, n + 5)]
        for T, first, total in windows:
            N = total if total else n
            left = [g - first for g in _leftovers(N, T) if first <= g < first + n]
            rng = np.random.default_rng(1000 * n + 10 * T + first)
            mates = mate_batch(rng, seqs, n, left)
            for tag, dust, with_art in SETTINGS:
                art = (string, s_index) if with_art else None
                want, usable = t2_restated(mates, art, T, dust, first, total)
                mode = t2_mode(mctx, mates, art, T, dust, first, total)
                got = t2_filter(fctx, c, mates, art, T, dust, first, total)
                where = (n, T, first, total, tag)
                assert got.dtype == np.int32 and len(got) == n
                assert np.array_equal(got, mode), (where, np.flatnonzero(got != mode)[:10])
                assert np.array_equal(got[usable], want[usable]), (where, np.flatnonzero((got != want) & usable)[:10])
                assert fctx.get_option("mate_filter_kernel_us") >= 0
                hit = (got & 0xFF) == 5
                assert ((got == 0) | (got == 6) | (hit & (got >> 8 >= 1) & (got >> 8 <= 13))).all()
                is_left = np.zeros(n, bool)
                is_left[left] = True
                seen["dust"] += int((got == 6).sum()); seen["art"] += int(hit.sum()); seen["left"] += len(left)
                seen["art_left"] += int((hit & is_left & usable).sum()); seen["art_four"] += int((hit & ~is_left).sum())
                seen["empty"] += int((~usable).sum())
        print(n, seen)
        assert seen["left"] > 0                                 # every batch size has left-over reads under some n_threads
        assert seen["art_left"] > 0                             # ... and bpm_check_error finds the short windows planted there
        if n >= 63:
            assert seen["dust"] > 0 and seen["art_four"] > 0 and seen["empty"] > 0
    finally:
        fctx.close()
        mctx.close()


def test_neither_dust_nor_artifacts_launches_nothing_and_every_type_is_zero():
    from tagdust_amd import TdError
    _, seqs, string, s_index = artifacts()
    c = mate_case("b_f_r", M)
    ctx = make_ctx(c, P, M)
    try:
        ctx.mol_mate_filter_enable()
        mates = mate_batch(np.random.default_rng(2), seqs, 257, [])
        got = t2_filter(ctx, c, mates, None, 1, 0)
        assert len(got) == 257 and not got.any()
        ctx.run()
        ctx.download()
        for name in ("mate_filter_kernel_us", "mate_join_kernel_us"):        # neither kernel has ever been launched
            with pytest.raises(TdError, match=name + ": no .* yet"):
                ctx.get_option(name)
        assert ctx.get_option("mate_kernel_us") >= 0
        got = t2_filter(ctx, c, mates, (string, s_index), 3, 100)             # ... and with something to judge by they are
        assert got.any()
        ctx.run()
        ctx.download()
        assert ctx.get_option("mate_filter_kernel_us") >= 0 and ctx.get_option("mate_join_kernel_us") >= 0
    finally:
        ctx.close()


# ---- the join and everything behind it ----
T_JOIN = 3


def join_case(shape):
    """The case of tests/test_mate_gpu.py with mates that can fail: one in eleven keeps its first M bases -- the molecule -- in
    front of a poly-A tail (DUST), one in sixteen in front of the reverse complement of an artifact window (its last 63 bases
    match); no mate is empty.  Returns (case with those mates, (string, s_index))."""
    if shape not in _JOIN:
        _, seqs, string, s_index = artifacts()
        c = mate_case(shape, M)
        mc, mo = c[7], c[8]
        rng = np.random.default_rng(77)
        mates = []
        for i in range(len(mo) - 1):
            m = mc[mo[i]:mo[i + 1]]
            m = m if len(m) else code("AC")
            u = rng.random()
            if u < 0.09:
                m = np.concatenate([m[:M], np.zeros(50, np.uint8)])
            elif u < 0.15:
                a = seqs[int(rng.integers(0, len(seqs)))]
                at = int(rng.integers(0, len(a) - 70 + 1))
                m = np.concatenate([m[:M], COMP[a[at:at + 70][::-1]]])       # (the reverse complement of the last 63 bases is in the text)
            mates.append(m.astype(np.uint8))
        nmc, nmo = pack(mates)
        _JOIN[shape] = (c[:7] + (nmc, nmo), (string, s_index))
    return _JOIN[shape]


def judged(shape, cuts):
    """The yardstick's records of a join case submitted in the batches between `cuts` (thread ranges are a batch's): per batch the
    oracle's decode with the read's own -ref and DUST, and the restated types of its mates.  Returns (own records, labels, t2,
    joined records)."""
    from oracle import pyoracle
    key = (shape, tuple(cuts))
    if key not in _JOIN:
        c, art = join_case(shape)
        om = pyoracle.OracleModel(c[0])
        own, labs, t2s = [], [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            p = part(c, lo, hi)
            ores, olab, _ = pyoracle.label_batch(om, p[1], p[2], p[3], p[4], 100, T_JOIN, artifacts=(art[0], art[1], 2))
            own.append({f: np.asarray(ores[f]).copy() for f in ("read_type", "barcode", "fingerprint")})
            labs.append(olab)
            mates = [p[7][p[8][i]:p[8][i + 1]] for i in range(hi - lo)]
            want, usable = t2_restated(mates, art, T_JOIN, 100)
            assert usable.all()
            t2s.append(want)
        res = {f: np.concatenate([o[f] for o in own]) for f in own[0]}
        t2 = np.concatenate(t2s)
        jres = dict(res)
        jres["read_type"] = np.maximum(res["read_type"], t2.astype(res["read_type"].dtype))
        _JOIN[key] = (res, np.concatenate(labs), t2, jres)
    return _JOIN[key]


def check_join_data(shape, cuts):
    """asserted on the yardstick first: enough mates fail, and the join changes which read of a molecule is kept"""
    from tagdust_amd import lib as tdlib
    c, _ = join_case(shape)
    res, lab, t2, jres = judged(shape, cuts)
    n = len(t2)
    args = lambda r: (c[0], c[1], c[2], r, lab, (c[7], c[8], M))
    assert int((t2 == 6).sum()) >= 0.05 * n and int(((t2 & 0xFF) == 5).sum()) >= 0.02 * n, (int((t2 == 6).sum()), int(((t2 & 0xFF) == 5).sum()))
    dup_j = tdlib.mol_dedup_host_mated(*args(jres), P)[0]
    dup_p = tdlib.mol_dedup_host_mated(*args(res), P)[0]
    changed = int((dup_p & ~dup_j & ((jres["read_type"] & 0xFF) == 0)).sum())     # kept now, a duplicate of a read whose mate fails before
    print(shape, "mates failing DUST", int((t2 == 6).sum()), "matching an artifact", int(((t2 & 0xFF) == 5).sum()), "molecules whose kept read changes", changed)
    assert changed >= 10
    return c, res, lab, t2, jres, args


def filter_ctx(c, art, spec, **kw):
    ctx = make_ctx(c, P, M, spec, **kw)
    try:
        ctx.set_artifacts(art[0], art[1], 2, T_JOIN)
        ctx.mol_mate_filter_enable()
    except Exception:
        ctx.close()
        raise
    return ctx


def expected_types(jres, dup):
    want = jres["read_type"].copy()
    want[dup] = 7
    return want


def hits_of(types, n_seq):
    t = np.asarray(types)
    return np.bincount((t[(t & 0xFF) == 5] >> 8) - 1, minlength=n_seq)[:n_seq].astype(np.int64)


@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
@pytest.mark.parametrize("shape", ["b_f_r", "b_f"])
def test_a_batch_and_everything_behind_the_join_equal_the_yardstick(shape, spec):
    from tagdust_amd import RESULT_DTYPE
    from tagdust_amd import lib as tdlib
    n = len(mate_case(shape, M)[2]) - 1
    c, res, lab, t2, jres, args = check_join_data(shape, [0, n])
    _, art = join_case(shape)
    n_seq = len(art[1]) - 1
    want, worg, want_tot = tdlib.mol_host_origins_mated(*args(jres), P)
    dup, dtot = tdlib.mol_dedup_host_mated(*args(jres), P)
    roots, rorg, ctot = tdlib.mol_collapse_host(want, worg)
    plain_tot = tdlib.mol_host_mated(*args(res), P)[1]
    assert want_tot["eligible"] < plain_tot["eligible"] and want_tot["molecules"] > 50
    ctx = filter_ctx(c, art, spec, dedup=True, collapse=True)
    try:
        with_census = any(int(t) == ord("B") for t in c[0]["seg_type"])
        if with_census:
            ctx.census_enable()
        ctx.counts_reset()
        dres, labels, _ = run_batch(ctx, c)
        assert np.array_equal(ctx.mol_mate_types(), t2)
        assert np.array_equal(labels, lab)
        got = dres["read_type"]
        assert np.array_equal(got, expected_types(jres, dup)), np.flatnonzero(got != expected_types(jres, dup))[:10]
        assert np.array_equal(dres["barcode"], res["barcode"]) and np.array_equal(dres["fingerprint"], res["fingerprint"])
        ent, org, tot = ctx.mol_origins()
        assert tot == want_tot and pairs(ent) == pairs(want) and np.array_equal(org, worg)
        assert ctx.mol_dedup_get() == dtot and want_tot["eligible"] == dtot["kept"] + dtot["duplicates"]
        cent, corg, cdtot = ctx.mol_collapse_entries()
        assert pairs(cent) == pairs(roots) and np.array_equal(corg, rorg) and cdtot == ctot
        # the -ref hit count is made from the combined type, the census sees it, td_counts_get stays as decoded
        assert np.array_equal(ctx.artifact_hits(n_seq), hits_of(jres["read_type"], n_seq)) and hits_of(jres["read_type"], n_seq).sum() > 0
        if with_census:
            cen, cen_tot = ctx.census()
            wcen, wcen_tot = tdlib.census_host(c[0], c[1], c[2], jres["read_type"], lab)
            assert cen_tot == wcen_tot and pairs(cen) == pairs(wcen)
        own = np.zeros(n, RESULT_DTYPE)
        own["read_type"], own["barcode"] = res["read_type"], res["barcode"]
        assert np.array_equal(ctx.counts(), tdlib.count_outcomes(own, np.diff(c[2])))
        assert ctx.get_option("mate_filter_kernel_us") >= 0 and ctx.get_option("mate_join_kernel_us") >= 0
    finally:
        ctx.close()


def submit_parts(ctx, c, cuts, in_flight=4):
    """test_mate_gpu.submit_all: the parts between the cuts through td_submit, each behind its own td_mol_mate_next"""
    from test_mate_gpu import submit_all
    return submit_all(ctx, c, cuts, in_flight)


@pytest.mark.parametrize("spec", [0, 1], ids=["generic", "specialised"])
def test_five_submitted_batches_then_freeze_and_replay(spec):
    from tagdust_amd import lib as tdlib
    shape = "b_f_r"
    n = len(mate_case(shape, M)[2]) - 1
    cuts = [0, 1, 130, 131, 700, n]
    c, res, lab, t2, jres, args = check_join_data(shape, cuts)
    _, art = join_case(shape)
    want, want_tot = tdlib.mol_host_mated(*args(jres), P)
    dup, dtot = tdlib.mol_dedup_host_mated(*args(jres), P)
    cdup, cdtot, ctot = tdlib.mol_dedup_collapsed_host_mated(*args(jres), P)
    assert int((cdup != dup).sum()) > 0
    ctx = filter_ctx(c, art, spec, dedup=True, collapse=True)
    try:
        ctx.set_option("pipeline_depth", 4)
        survey = submit_parts(ctx, c, cuts)
        assert np.array_equal(survey["read_type"], expected_types(jres, dup))
        ent, tot = ctx.mol_entries()
        assert tot == want_tot and pairs(ent) == pairs(want) and ctx.mol_dedup_get() == dtot
        assert np.array_equal(ctx.artifact_hits(len(art[1]) - 1), hits_of(jres["read_type"], len(art[1]) - 1))
        assert ctx.mol_dedup_freeze() == ctot
        replay = submit_parts(ctx, c, cuts)
        assert np.array_equal(replay["read_type"], expected_types(jres, cdup)) and ctx.mol_dedup_get() == cdtot
        assert ctx.mol_entries()[1] == want_tot                  # the table stays as the survey left it
        assert want_tot["eligible"] == cdtot["kept"] + cdtot["duplicates"]
        assert ctx.get_option("overlap_active") == spec
    finally:
        ctx.close()


def test_filter_on_without_dust_and_artifacts_is_the_filter_off_result_bit_for_bit():
    from tagdust_amd import TdError
    c, _ = join_case("b_f_r")
    out = {}
    for on in (0, 1):
        ctx = make_ctx(c, P, M, dedup=True, collapse=True)
        try:
            ctx.set_params(c[3], c[4], 0)
            if on:
                ctx.mol_mate_filter_enable()
            assert ctx.get_option("mate_filter") == on
            ctx.counts_reset()
            dres, labels, seq = run_batch(ctx, c)
            out[on] = (dres.tobytes(), labels.tobytes(), seq.tobytes(), ctx.mol_origins(), ctx.mol_dedup_get(), ctx.mol_collapse_entries(),
                       ctx.counts().tobytes())
            if on:
                assert not ctx.mol_mate_types().any()
                with pytest.raises(TdError, match="no mate batch has been judged yet"):
                    ctx.get_option("mate_filter_kernel_us")
        finally:
            ctx.close()
    a, b = out[0], out[1]
    assert a[:3] == b[:3] and a[6] == b[6] and a[4] == b[4]
    assert pairs(a[3][0]) == pairs(b[3][0]) and np.array_equal(a[3][1], b[3][1]) and a[3][2] == b[3][2]
    assert pairs(a[5][0]) == pairs(b[5][0]) and np.array_equal(a[5][1], b[5][1]) and a[5][2] == b[5][2]


def test_failures_leave_the_totals_and_a_correct_batch_works_afterwards():
    from tagdust_amd import RESULT_DTYPE, TdError
    from tagdust_amd import lib as tdlib
    n = len(mate_case("b_f_r", M)[2]) - 1
    cuts = [0, 400, 800]
    c, art = join_case("b_f_r")
    res, lab, t2, jres = judged("b_f_r", cuts)
    a, b = part(c, 0, 400), part(c, 400, 800)
    first = {f: v[:400] for f, v in jres.items()}
    # enable without mate mode: the count alone
    ctx = make_ctx(c, P, 0)
    try:
        with pytest.raises(TdError, match="td_mol_mate_filter_enable: mate mode is off"):
            ctx.mol_mate_filter_enable()
        with pytest.raises(TdError, match="td_mol_mate_filter_disable: mate mode is off"):
            ctx.mol_mate_filter_disable()
        with pytest.raises(TdError, match="td_mol_mate_types: the mate filter is off"):
            ctx.mol_mate_types()
        assert ctx.get_option("mate_filter") == 0
        with pytest.raises(TdError, match="mate_filter_kernel_us: the mate filter is off"):
            ctx.get_option("mate_filter_kernel_us")
    finally:
        ctx.close()
    ctx = filter_ctx(c, art, 0)
    try:
        run_batch(ctx, a)
        ent0, tot0 = ctx.mol_entries()
        want0, want_tot0 = tdlib.mol_host_mated(a[0], a[1], a[2], first, lab[:a[2][-1] + 400], (a[7], a[8], M), P)
        assert tot0 == want_tot0 and pairs(ent0) == pairs(want0) and tot0["counted"] > 0
        # the switch with a ticket out
        r = np.zeros(400, RESULT_DTYPE)
        ctx.mol_mate_next(b[7], b[8])
        t = ctx.submit(b[1], b[2], res=r)
        for call, name in ((ctx.mol_mate_filter_enable, "enable"), (ctx.mol_mate_filter_disable, "disable")):
            with pytest.raises(TdError, match="td_mol_mate_filter_%s: td_submit tickets are outstanding" % name):
                call()
        ctx.wait(t)
        assert ctx.get_option("mate_filter") == 1
        both = {f: v[:800] for f, v in jres.items()}
        ab = part(c, 0, 800)
        want, want_tot = tdlib.mol_host_mated(ab[0], ab[1], ab[2], both, lab[:ab[2][-1] + 800], (ab[7], ab[8], M), P)
        ent, tot = ctx.mol_entries()
        assert tot == want_tot and pairs(ent) == pairs(want)        # the totals are those of the two correct batches
        assert np.array_equal(r["read_type"], both["read_type"][400:])
        # a batch that is resident across the switch was judged under the other state: td_run says so, nothing is counted
        ctx.mol_mate_next(a[7], a[8])
        ctx.upload_batch(a[1], a[2])
        ctx.mol_mate_filter_disable()
        assert ctx.get_option("mate_filter") == 0 and not any(ctx.mol_entries()[1].values())       # (an empty table, as td_mol_reset leaves it)
        with pytest.raises(TdError, match="td_run: the mate filter is off .* staged while it was on"):
            ctx.run()
        assert not any(ctx.mol_entries()[1].values())
        ctx.mol_mate_filter_enable()
        run_batch(ctx, a)
        ent, tot = ctx.mol_entries()
        assert tot == want_tot0 and pairs(ent) == pairs(want0)
        # td_mol_mate_disable, td_mol_disable and a new model switch the filter off as well
        ctx.mol_mate_disable()
        assert ctx.get_option("mate_filter") == 0
        ctx.mol_mate_enable(M)
        ctx.mol_mate_filter_enable()
        ctx.mol_disable()
        assert ctx.get_option("mate_filter") == 0
        ctx.mol_enable(P, 16)
        ctx.mol_mate_enable(M)
        ctx.mol_mate_filter_enable()
        ctx.upload_model(c[0])
        assert ctx.get_option("mate_filter") == 0 and ctx.get_option("mate_bases") == 0
    finally:
        ctx.close()


# ---- the command against the reference binary ----
def _log_lines(d, prefix):
    out = []
    for line in open(os.path.join(d, prefix + "_logfile.txt")).read().splitlines():
        out.append(line.split("]\t", 1)[1] if line.startswith("[") and "]\t" in line else line)
    return out


def _summary(d, prefix):
    lines = _log_lines(d, prefix)
    at = [i for i, l in enumerate(lines) if l.endswith("\ttotal input reads")]
    assert at, lines
    return lines[at[0]:]


@pytest.mark.parametrize("T", [1, 3], ids=["t1", "t3"])
def test_the_command_equals_the_reference_binary_and_dedup_keeps_the_yardstick_s_reads(tmp_path, T):
    """tagdust-hip r1.fq r2.fq --mate-bases 20 --mate-filter with the default -dust 100 and a -ref file of two sequences: the output
    files and the log's summary block of the unmodified reference binary on the same files and options; with --dedup the _READ1 and
    _READ2 files of every barcode hold exactly the yardstick's kept reads, and no written record has a failing mate."""
    import subprocess
    from oracle import pyoracle
    from tagdust_amd import lib as tdlib
    if not os.path.exists(os.path.join(RBIN, "tagdust_rtest")):
        pytest.skip("oracle/_ref/tagdust_rtest not built")
    shape = "b_f_r"
    c, _ = join_case(shape)
    seq, offs, mc, mo = c[1], c[2], c[7], c[8]
    n = len(offs) - 1
    _, seqs, _, _ = artifacts()
    two = [seqs[0], seqs[1]]
    text = b"".join(b">art%d\n" % j + bytes(np.frombuffer(b"ACGTN", np.uint8)[s]) + b"\n" for j, s in enumerate(two))
    string, s_index = _fasta(text)
    # the mates of join_case match windows of all thirteen sequences: those of the first two are hits here
    d = str(tmp_path)
    open(os.path.join(d, "r1.fq"), "wb").write(fastq_of(seq, offs))
    open(os.path.join(d, "r2.fq"), "wb").write(fastq_of(mc, mo))
    open(os.path.join(d, "art.fa"), "wb").write(text)
    head = [w for k, s in enumerate(MATE_SHAPES[shape]) for w in ("-%d" % (k + 1), s)] + ["-ref", "art.fa", "-fe", "2", "-t", str(T), "-seed", "42"]
    p = subprocess.run([os.path.join(RBIN, "tagdust_rtest")] + head + ["r1.fq", "r2.fq", "-o", "cpu"], cwd=d, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-2000:]
    tail = ["--sync-compile", "--molecules-slots", "16", "--molecules-prefix", str(P), "--mate-bases", str(M), "--mate-filter"]
    _run(head + ["r1.fq", "r2.fq"] + tail + ["-o", "gpu"], d)
    cpu = {k: v for k, v in _outputs(d, "cpu").items() if k != "_logfile.txt"}
    gpu = {k: v for k, v in _outputs(d, "gpu").items() if k not in ("_logfile.txt", "_molecules.txt")}
    assert cpu and set(cpu) == set(gpu), (sorted(cpu), sorted(gpu))
    for k in cpu:
        assert cpu[k] == gpu[k], "output file *%s differs" % k
    assert _summary(d, "cpu") == _summary(d, "gpu")
    assert b"# mate filter\tdust 100, -ref art.fa" in _outputs(d, "gpu")["_molecules.txt"].split(b"\n")
    # --dedup through the library call, which reports the threshold the run estimated
    os.environ["TD_SPECIALIZE"] = "0"
    try:
        rep = tdlib.run_execute(["--rtest"] + [os.path.join(d, w) if w == "art.fa" else w for w in head] + [os.path.join(d, "r1.fq"), os.path.join(d, "r2.fq")] + tail +
                                ["--dedup", "-o", os.path.join(d, "dd")])
    finally:
        del os.environ["TD_SPECIALIZE"]
    thr = rep["thresholds"][0]
    picked = [float(l.split("::")[1]) for l in _log_lines(d, "cpu") if l.startswith("Selected Threshold::")]
    assert len(picked) == 2 and abs(picked[0] - thr) < 1e-4, (picked, thr)           # (the reference chose the same one for read 1)
    # the yardstick: the reads decoded as the command decodes them, batch for batch (1000 records), the mates judged batch for batch
    md, _ = tdlib.build_model(MATE_SHAPES[shape], seq, offs, e=0.05, d=0.1)
    om = pyoracle.OracleModel(md)
    own, labs, t2s = [], [], []
    for lo in range(0, n, 1000):
        hi = min(n, lo + 1000)
        pr = part(c, lo, hi)
        ores, olab, _ = pyoracle.label_batch(om, pr[1], pr[2], thr, 16, 100, T, artifacts=(string, s_index, 2))
        own.append({f: np.asarray(ores[f]).copy() for f in ("read_type", "barcode", "fingerprint")})
        labs.append(olab)
        t2s.append(t2_restated([pr[7][pr[8][i]:pr[8][i + 1]] for i in range(hi - lo)], (string, s_index), T, 100)[0])
    res = {f: np.concatenate([o[f] for o in own]) for f in own[0]}
    t2 = np.concatenate(t2s)
    jres = dict(res)
    jres["read_type"] = np.maximum(res["read_type"], t2.astype(res["read_type"].dtype))
    assert int((t2 == 6).sum()) >= 0.05 * n and int(((t2 & 0xFF) == 5).sum()) > 0
    dup, tot = tdlib.mol_dedup_host_mated(md, seq, offs, jres, np.concatenate(labs), (mc, mo, M), P)
    dd = _outputs(d, "dd")
    first = sorted(k for k in dd if k.startswith("_BC_") and "_READ1" in k)
    assert len(first) == 8 and all(k.replace("_READ1", "_READ2") in dd for k in first)
    name = lambda r: int(re.match(rb"@r(\d+)", r).group(1))
    kept_names = set()
    for k in first:
        one = [name(r) for r in records_of(dd[k])]
        twos = [name(r) for r in records_of(dd[k.replace("_READ1", "_READ2")])]
        assert one == twos and one == sorted(one) and len(one) > 0, k
        kept_names.update(one)
    ok = (jres["read_type"] & 0xFF) == 0
    assert kept_names == set(np.flatnonzero(ok & ~dup).tolist())
    assert not any(t2[i] != 0 for i in kept_names)               # no written record has a failing mate
    lines = dd["_molecules.txt"].split(b"\n")
    assert b"# written\t%d" % tot["kept"] in lines and b"# duplicates removed\t%d" % tot["duplicates"] in lines
    assert rep["dedup_totals"] == tot and sum(rep["artifact_hits"].values()) == int(((jres["read_type"] & 0xFF) == 5).sum())
