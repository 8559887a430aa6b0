"""Measures the molecule count (include/tagdust_molecules.h) on 2^20 config-3-shaped reads with an 8-nt fingerprint, drawn with
replacement from 2^18 molecules.

    python tools/molecules_bench.py [--reads 1048576] [--molecules 262144] [--out profiles/molecules.json]        # on the MI355X

The architecture is the flagship's with an F segment behind the barcode: B:<8 barcodes> F:NNNNNNNN S:GTA R:N P:<adapter>; a
molecule is a barcode, a UMI and an insert, a read is a molecule with the 3' adapter's prefix at its end and 2 % substitutions in
barcode, spacer and adapter (the flagship's generator; UMI and insert are copied as they are, so the molecules of a batch are
known: the distinct draws).

Measured: the count kernel's time from HIP events (option "molecules_kernel_us": events around its launch) beside the decode
kernel's time of the same batch (td_last_kernel_ms), median of 5 batches, the table reset before each so that every batch claims
its slots anew; the totals of one batch; the device summary's time (td_mol_get, 2^22 slots); and host-to-host reads/s of the batch
through td_submit / td_wait with the count on and off in turn (on, off, on, off).  The yardstick is the run with the count off:
the path without this feature.

Dedup (td_mol_dedup_enable) gets a row of its own on the same workload: the two passes' time from HIP events (option
"dedup_kernel_us": events around both launches of a td_run batch, nothing else in flight), median of 5 batches with the table
reset before each, the totals of one batch, and a third state "dedup" in the host-to-host rotation (on, off, dedup, on, off,
dedup), to be held against "on" -- the count alone -- of the same process.  Expectation, written down before the first run: pass
1 walks the labels again as the count does and adds a probe (a load that mostly hits the key's first slot) and one 8-byte atomic
minimum at a random address, so it should cost about what the count kernel costs; pass 2 reads 12 bytes per read in order and one
random 8-byte word: less than half of that.  The table's random traffic bounds both.

Expectation, written down before the first run, from the bytes the count kernel touches per read: the outcome, length, barcode
and fingerprint (16 B), a label byte per position up to the 20th read base (the read starts at base 17: 37 B), three 2-bit words
and two N-mask words (20 B) -- 73 B streamed -- and the table: a load of the key, a CAS on it for a new key, an add on the
count, three touches of 8 B that each move a 64-byte sector or more at a random address, 200-400 B.  Under 0.5 KB against the
56 KB a read costs the decode kernel: about one percent of the decode kernel's time, and no visible change host to host, where
the count runs behind the decode kernel on its stream while the copies of the neighbouring batches are under way.

The UMI collapse (td_mol_collapse_enable) has a mode of its own, --collapse, which adds a "collapse" section to the same file and
measures nothing else:

    python tools/molecules_bench.py --collapse

The same workload with 0.5 % substitutions per UMI base on top, so that there is something to collapse.  Per batch: the origin
pass from HIP events (option "collapse_origin_kernel_us") beside the count kernel and the decode kernel of the same batch, median
of 5 batches with the table reset before each.  End of run: td_mol_collapse_get from the call to the rows on the host, the first
call (it allocates the parent and collapsed arrays) and the second.  Host to host: td_submit / td_wait with the collapse on and
with the count alone in turn in one process, two passes of each after a first pass of the process that is discarded (the first
pass pays for the first touches of every buffer).  The yardstick is the count alone in the same process.  Expectation, written
down before the first run: the origin pass is dedup's pass 1 with a 16-byte store for a key's first read in place of the atomic
minimum -- a walk, a probe, at most one store --, so it should cost about what dedup's pass 1 costs, which is about what the count
kernel costs; the collapse touches 3 * m + 2 = 26 random words per molecule for an 8-nt UMI (24 probes that mostly end at an empty
or a foreign slot, the parent's count, the root's add) besides two sweeps over the table's keys, so at the 60-100 ns a random
touch of a quarter-full 64 MiB table costs a lane and some ten thousand lanes in flight, 2.8 * 10^5 molecules should take well
under 10 ms, less than the host's sort of the entries; host to host nothing visible.

One read per collapsed molecule (td_mol_dedup_freeze: survey, freeze, replay) has a mode of its own, --dedup-collapsed, which adds
a "dedup_collapsed" section to the same file and measures nothing else:

    python tools/molecules_bench.py --dedup-collapsed [--with-command | --command-only]

The collapse's workload (0.5 % substitutions per UMI base).  Per iteration, the table reset before each: one td_run batch surveyed
(count, origin pass, exact dedup's two passes: option "dedup_kernel_us", the yardstick of measurement 1 on the same visit),
td_mol_collapse_get from call to return (the yardstick of measurement 2), td_mol_dedup_freeze from call to return -- the first call
of the process allocates the keepers --, then the same batch replayed by td_run (option "dedup_replay_kernel_us"); medians of 5
iterations behind a first one.  Host to host: td_submit / td_wait in the frozen state (one batch surveyed, the freeze, then the
timed steps: their ordinals run on, so hardly a read is its tree's keeper, which is the same work -- key, probe, load, compare --
with more stores), with exact dedup and with the count alone in turn in one process, two passes of each after a first pass that
is discarded.  --with-command: the whole command on a FASTQ of the batch, --dedup-collapsed against --dedup --collapse-umis of
the same build (a path this mode does not touch), same file, same box: a first run that is discarded (it compiles the model kernel,
the later ones find it in the cache), then the two in turn, twice each, seconds on the wall.  Expectations, written down before the first run:
  1. the replay kernel takes at most what exact dedup's two passes take on the same visit (0.30 ms per 2^20 reads on an earlier
     visit): one launch in place of two, one walk and one probe as pass 1 has, one random 8-byte load, no atomic on the table;
  2. td_mol_dedup_freeze takes about what td_mol_collapse_get takes (1.2 ms on an earlier visit): the same three launches without
     the summary sweep, plus one sweep over the occupied list and, the first time, one allocation of 8 bytes per slot (32 MiB);
  3. host to host: no expectation set in advance;
  4. the command: up to twice the streaming seconds -- the survey decodes everything a second time --, expected and accepted.

Mate mode (td_mol_mate_enable: the first bases of a read's mate joined into the key) has a mode of its own, --mate, which adds a
"mate" section to the same file and measures nothing else:

    python tools/molecules_bench.py --mate

The same workload plus a mate of 150 bases per read (one mate per molecule, copied as it is), P = 12 own bases and M = 20 of the
mate.  Per batch: the mate kernel from HIP events (option "mate_kernel_us") beside the count kernel with the mate on and the decode
kernel of the same batch, median of 5 batches with the table reset before each; the count kernel with mate mode off (P = 12) the
same way.  Host to host: td_submit / td_wait with mate mode on and off in turn in one process, two passes of each after a first pass
that is discarded; the state with mate mode off is the yardstick.  Nobody has measured what the second upload costs.  Expectation,
written down before the first run:
  1. 150 B more host to device per read beside the 150 B of the read itself and its 8-byte offset: the upload roughly doubles
     (158 -> 316 B per read), and so does the host's staging copy of pageable input;
  2. about 9 B more per eligible lane in each of the kernels over mol_lane_key (an 8-byte word and a byte at the read's index in
     the caller's order -- the batch is of one length here, so that index is the lane's own and the loads are coalesced): beside
     the 73 B streamed and 200-400 B of table traffic per read, a few percent of the count kernel at most;
  3. the mate kernel touches one or two 64-byte lines of its mate per read (20 bytes at a stride of 150) and writes 9 B: 2^20 reads
     move 64-128 MiB, some tens of microseconds at HBM rate -- the same order as the count kernel, far below the decode kernel;
  4. host to host: no expectation set in advance.  The decode kernel bounds the pipeline and the upload runs beside it, so the
     doubled copy may not show at all; if the loss is more than the extra copy's bytes explain, the next step is to copy only the
     first M bytes of each mate (not built here).

The mate filter (td_mol_mate_filter_enable: the mate judged by DUST and -ref, its outcome joined to the read's in front of the count)
has a mode of its own, --mate-filter, which adds a "mate_filter" section to the same file and measures nothing else:

    python tools/molecules_bench.py --mate-filter

The mate workload above (2^20 reads with a 150-base mate, P = 12, M = 20) with -dust 100 and 16 artifact sequences of 100 nt
(tools/rna_dust_bench.py's), n_threads 16, set on the context in both states, so that the read's own filter costs the same in both
and the difference is the mate's.  Per batch: the filter kernel (option "mate_filter_kernel_us") and the join kernel
("mate_join_kernel_us") from HIP events, median and range of 5 batches behind one that is discarded; beside them td_rna_dust_kernel
over the same mates as a batch of their own in a second context of the same process (td_last_kernel_ms), the same way -- that kernel
does the same arithmetic from packed tiles and is the yardstick.  Host to host: td_submit / td_wait with the filter off and on in
turn in one process, two passes of each after a first pass that is discarded.  Expectation, written down before the first run:
  1. the filter kernel runs td_rna_dust_kernel's columns -- 16 sequences x 101 characters x 2 strands per mate, 2.7 ms per 2^20 reads
     when that kernel was measured on this filter -- and stages 150 B per mate through LDS (157 MB as coalesced dwords: 40-50 us at
     HBM rate) where that kernel reads 56 B of packed words: within 10 % of the yardstick, 2.7-3.0 ms.  It holds 93 VGPRs and
     32 KiB of LDS per workgroup (5 waves per SIMD, the yardstick 8); the columns are VALU-bound, so that should not show;
  2. the join kernel moves 12 B per read (two loads, one store, the batch is of one length: all coalesced): 12 MiB, 5-10 us, the
     price of a launch;
  3. host to host: the filter kernel runs on the slot's high-priority aux stream beside the decode kernel of the batch before, whose
     compute units it takes while it runs: a loss of up to filter / decode kernel time, no more.  No threshold is set.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (the flagship workload's barcodes, spacer, adapter and read length)

UMI = 8
PREFIX = 20
LOG2_SLOTS = 22


def code(s):
    return np.array(["ACGT".index(c) for c in s], np.uint8)


MATE_PREFIX, MATE_BASES, MATE_LEN = 12, 20, 150


def make_batch(n, n_mol, seed=1, sub=0.02, umi_sub=0.0, with_mates=False):
    rng = np.random.default_rng(seed)
    L = bench.READ_LEN
    bar = np.array([code(b) for b in bench.BARCODES], np.uint8)
    mol = rng.integers(0, 4, size=(n_mol, L), dtype=np.uint8)
    mol[:, :6] = bar[rng.integers(0, len(bar), n_mol)]
    mol[:, 6 + UMI:6 + UMI + len(bench.SPACER)] = code(bench.SPACER)
    draw = rng.integers(0, n_mol, n)
    y = mol[draw]
    ad = code(bench.ADAPTER)
    keep = rng.integers(0, len(ad) + 1, n)
    t0 = L - len(ad)
    pos = np.arange(t0, L)[None, :]
    start = (L - keep)[:, None]
    in_ad = pos >= start
    y[:, t0:] = np.where(in_ad, ad[np.clip(pos - start, 0, len(ad) - 1)], y[:, t0:])
    structured = np.zeros((n, L), bool)
    structured[:, :6] = True
    structured[:, 6 + UMI:6 + UMI + len(bench.SPACER)] = True
    structured[:, t0:] |= in_ad
    structured &= rng.random((n, L)) < sub
    np.copyto(y, rng.integers(0, 4, size=(n, L), dtype=np.uint8), where=structured)
    if umi_sub > 0:                                                # misread UMI bases: always another base
        hit = rng.random((n, UMI)) < umi_sub
        y[:, 6:6 + UMI] = np.where(hit, (y[:, 6:6 + UMI] + rng.integers(1, 4, size=(n, UMI), dtype=np.uint8)) & 3, y[:, 6:6 + UMI])
    batch = (np.ascontiguousarray(y.reshape(-1)), np.arange(n + 1, dtype=np.int64) * L, int(len(np.unique(draw))))
    if with_mates:                                                 # one mate per molecule, copied as it is
        mates = rng.integers(0, 4, size=(n_mol, MATE_LEN), dtype=np.uint8)[draw]
        batch += (np.ascontiguousarray(mates.reshape(-1)), np.arange(n + 1, dtype=np.int64) * MATE_LEN)
    return batch


def measure(ctx, seq, offs, n):
    from tagdust_amd import RESULT_DTYPE
    out = {}
    ctx.mol_enable(PREFIX, LOG2_SLOTS)
    dec, cnt = [], []
    for it in range(6):
        ctx.mol_reset()
        ctx.upload_batch(seq, offs)
        ctx.run()
        dec.append(ctx.last_kernel_ms())
        cnt.append(ctx.get_option("molecules_kernel_us") / 1000.0)
        if it == 0:
            t0 = time.perf_counter()
            rows, tot = ctx.mol_get()
            out["device_summary_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
            out["totals_of_one_batch"] = tot
            out["rows_of_one_batch"] = [[int(r["reads"]), int(r["molecules"])] for r in rows[:len(bench.BARCODES)]]
    out["decode_kernel_ms_runs"] = [round(v, 3) for v in dec[1:]]
    out["count_kernel_ms_runs"] = [round(v, 3) for v in cnt[1:]]
    d, c = statistics.median(dec[1:]), statistics.median(cnt[1:])
    out["decode_kernel_ms_median"], out["count_kernel_ms_median"] = round(d, 3), round(c, 3)
    out["count_share_of_decode"] = round(c / d, 5)
    out["count_kernel_reads_per_s"] = round(n / (c * 1e-3)) if c > 0 else None
    # dedup's two passes behind the count
    ctx.mol_dedup_enable()
    dd = []
    for it in range(6):
        ctx.mol_reset()
        ctx.upload_batch(seq, offs)
        ctx.run()
        dd.append(ctx.get_option("dedup_kernel_us") / 1000.0)
        if it == 0:
            out["dedup_totals_of_one_batch"] = ctx.mol_dedup_get()
    out["dedup_passes"] = 2
    out["dedup_kernel_ms_runs"] = [round(v, 3) for v in dd[1:]]
    out["dedup_kernel_ms_median"] = round(statistics.median(dd[1:]), 3)
    out["dedup_share_of_decode"] = round(statistics.median(dd[1:]) / d, 5)
    ctx.mol_disable()
    # host to host through td_submit / td_wait: the count on, off, and on with dedup, in turn
    res = [np.zeros(n, RESULT_DTYPE) for _ in range(2)]
    rates = {"on": [], "off": [], "dedup": []}
    for state in ("on", "off", "dedup", "on", "off", "dedup"):
        if state != "off":
            ctx.mol_enable(PREFIX, LOG2_SLOTS)
        if state == "dedup":
            ctx.mol_dedup_enable()
        steps = 4
        for t in [ctx.submit(seq, offs, res=r) for r in res]:      # warm-up: both slots, both result buffers
            ctx.wait(t)
        t0 = time.perf_counter()
        tickets = []
        for s in range(steps):
            tickets.append(ctx.submit(seq, offs, res=res[s & 1]))
            if len(tickets) == 2:
                ctx.wait(tickets.pop(0))
        for t in tickets:
            ctx.wait(t)
        rates[state].append(round(steps * n / (time.perf_counter() - t0)))
        if state != "off":
            ctx.mol_disable()
    out["host_to_host_reads_per_s"] = rates
    return out


def measure_collapse(ctx, seq, offs, n):
    from tagdust_amd import RESULT_DTYPE
    out = {"umi_substitution_rate": 0.005}
    ctx.mol_enable(PREFIX, LOG2_SLOTS)
    ctx.mol_collapse_enable()
    dec, cnt, org = [], [], []
    for it in range(6):
        ctx.mol_reset()
        ctx.upload_batch(seq, offs)
        ctx.run()
        dec.append(ctx.last_kernel_ms())
        cnt.append(ctx.get_option("molecules_kernel_us") / 1000.0)
        org.append(ctx.get_option("collapse_origin_kernel_us") / 1000.0)
        if it == 0:
            for name in ("collapse_get_ms_first_call", "collapse_get_ms_second_call"):
                t0 = time.perf_counter()
                rows, tot = ctx.mol_collapse_get()
                out[name] = round((time.perf_counter() - t0) * 1e3, 3)
            out["collapse_totals_of_one_batch"] = tot
            out["rows_of_one_batch_collapsed"] = [[int(r["reads"]), int(r["molecules"])] for r in rows[:len(bench.BARCODES)]]
    d, c, o = statistics.median(dec[1:]), statistics.median(cnt[1:]), statistics.median(org[1:])
    out["decode_kernel_ms_median"], out["count_kernel_ms_median"], out["origin_kernel_ms_median"] = round(d, 3), round(c, 3), round(o, 3)
    out["origin_kernel_ms_runs"] = [round(v, 3) for v in org[1:]]
    out["origin_share_of_decode"], out["origin_over_count"] = round(o / d, 5), round(o / c, 3) if c > 0 else None
    ctx.mol_disable()
    # host to host: the first pass of the process is discarded, then the collapse and the count alone in turn, twice each
    res = [np.zeros(n, RESULT_DTYPE) for _ in range(2)]
    rates = {"discarded_first_pass": [], "collapse": [], "count_alone": []}
    for k, state in enumerate(("count_alone", "collapse", "count_alone", "collapse", "count_alone")):
        ctx.mol_enable(PREFIX, LOG2_SLOTS)
        if state == "collapse":
            ctx.mol_collapse_enable()
        steps = 4
        for t in [ctx.submit(seq, offs, res=r) for r in res]:      # warm-up: both slots, both result buffers
            ctx.wait(t)
        t0 = time.perf_counter()
        tickets = []
        for s in range(steps):
            tickets.append(ctx.submit(seq, offs, res=res[s & 1]))
            if len(tickets) == 2:
                ctx.wait(tickets.pop(0))
        for t in tickets:
            ctx.wait(t)
        rates["discarded_first_pass" if k == 0 else state].append(round(steps * n / (time.perf_counter() - t0)))
        ctx.mol_disable()
    out["host_to_host_reads_per_s"] = rates
    return out


def measure_dedup_collapsed(ctx, seq, offs, n):
    from tagdust_amd import RESULT_DTYPE
    out = {"umi_substitution_rate": 0.005}
    ctx.mol_enable(PREFIX, LOG2_SLOTS)
    ctx.mol_dedup_enable()
    ctx.mol_collapse_enable()
    dec, exact, rep, frz, col = [], [], [], [], []
    for it in range(6):
        ctx.mol_reset()
        ctx.upload_batch(seq, offs)
        ctx.run()                                                  # the survey
        dec.append(ctx.last_kernel_ms())
        exact.append(ctx.get_option("dedup_kernel_us") / 1000.0)
        if it == 0:
            out["exact_dedup_totals_of_one_batch"] = ctx.mol_dedup_get()
        ctx.mol_collapse_get()                                     # (the first of the process allocates parent and collapsed)
        t0 = time.perf_counter()
        ctx.mol_collapse_get()
        col.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ctot = ctx.mol_dedup_freeze()
        frz.append((time.perf_counter() - t0) * 1e3)
        ctx.upload_batch(seq, offs)
        ctx.run()                                                  # the replay
        rep.append(ctx.get_option("dedup_replay_kernel_us") / 1000.0)
        if it == 0:
            out["freeze_ms_first_call"] = round(frz[0], 3)
            out["collapse_totals_of_one_batch"] = ctot
            out["replay_totals_of_one_batch"] = ctx.mol_dedup_get()
            out["count_totals_of_one_batch"] = ctx.mol_get()[1]
    med = statistics.median
    out["decode_kernel_ms_median"] = round(med(dec[1:]), 3)
    out["exact_dedup_two_passes_ms_runs"], out["exact_dedup_two_passes_ms_median"] = [round(v, 3) for v in exact[1:]], round(med(exact[1:]), 3)
    out["replay_kernel_ms_runs"], out["replay_kernel_ms_median"] = [round(v, 3) for v in rep[1:]], round(med(rep[1:]), 3)
    out["replay_over_exact_dedup"] = round(med(rep[1:]) / med(exact[1:]), 3) if med(exact[1:]) > 0 else None
    out["freeze_ms_runs"], out["freeze_ms_median"] = [round(v, 3) for v in frz[1:]], round(med(frz[1:]), 3)
    out["collapse_get_ms_runs"], out["collapse_get_ms_median"] = [round(v, 3) for v in col[1:]], round(med(col[1:]), 3)
    ctx.mol_disable()
    # host to host: the first pass of the process is discarded, then the three states in turn, twice each
    res = [np.zeros(n, RESULT_DTYPE) for _ in range(2)]
    rates = {"discarded_first_pass": [], "frozen": [], "exact_dedup": [], "count_alone": []}
    for k, state in enumerate(("count_alone", "frozen", "exact_dedup", "count_alone", "frozen", "exact_dedup", "count_alone")):
        ctx.mol_enable(PREFIX, LOG2_SLOTS)
        if state != "count_alone":
            ctx.mol_dedup_enable()
        if state == "frozen":
            ctx.mol_collapse_enable()
            ctx.upload_batch(seq, offs)
            ctx.run()
            ctx.mol_dedup_freeze()
        steps = 4
        for t in [ctx.submit(seq, offs, res=r) for r in res]:      # warm-up: both slots, both result buffers
            ctx.wait(t)
        t0 = time.perf_counter()
        tickets = []
        for s in range(steps):
            tickets.append(ctx.submit(seq, offs, res=res[s & 1]))
            if len(tickets) == 2:
                ctx.wait(tickets.pop(0))
        for t in tickets:
            ctx.wait(t)
        rates["discarded_first_pass" if k == 0 else state].append(round(steps * n / (time.perf_counter() - t0)))
        ctx.mol_disable()
    out["host_to_host_reads_per_s"] = rates
    return out


def measure_mate(ctx, seq, offs, n, mseq, moffs):
    from tagdust_amd import RESULT_DTYPE
    out = {"prefix_bases": MATE_PREFIX, "mate_bases": MATE_BASES, "mate_len": MATE_LEN,
           "upload_bytes_per_read": {"mate_off": int(offs[1] - offs[0]) + 8, "mate_on": int(offs[1] - offs[0]) + 8 + MATE_LEN + 8}}
    med = statistics.median
    for state in ("mate_on", "mate_off"):
        ctx.mol_enable(MATE_PREFIX, LOG2_SLOTS)
        if state == "mate_on":
            ctx.mol_mate_enable(MATE_BASES)
        dec, cnt, mk = [], [], []
        for it in range(6):
            ctx.mol_reset()
            if state == "mate_on":
                ctx.mol_mate_next(mseq, moffs)
            ctx.upload_batch(seq, offs)
            ctx.run()
            dec.append(ctx.last_kernel_ms())
            cnt.append(ctx.get_option("molecules_kernel_us") / 1000.0)
            if state == "mate_on":
                mk.append(ctx.get_option("mate_kernel_us") / 1000.0)
            if it == 0:
                out["totals_of_one_batch_" + state] = ctx.mol_get()[1]
        out["decode_kernel_ms_median_" + state] = round(med(dec[1:]), 3)
        out["count_kernel_ms_runs_" + state], out["count_kernel_ms_median_" + state] = [round(v, 3) for v in cnt[1:]], round(med(cnt[1:]), 3)
        if mk:
            out["mate_kernel_ms_runs"], out["mate_kernel_ms_median"] = [round(v, 3) for v in mk[1:]], round(med(mk[1:]), 3)
            out["mate_kernel_share_of_decode"] = round(med(mk[1:]) / med(dec[1:]), 5)
        ctx.mol_disable()
    out["count_kernel_mate_on_over_off"] = round(out["count_kernel_ms_median_mate_on"] / out["count_kernel_ms_median_mate_off"], 3) \
        if out["count_kernel_ms_median_mate_off"] > 0 else None
    # host to host: the first pass of the process is discarded, then mate mode on and off in turn, twice each
    res = [np.zeros(n, RESULT_DTYPE) for _ in range(2)]
    rates = {"discarded_first_pass": [], "mate_on": [], "mate_off": []}
    for k, state in enumerate(("mate_off", "mate_on", "mate_off", "mate_on", "mate_off")):
        ctx.mol_enable(MATE_PREFIX, LOG2_SLOTS)
        if state == "mate_on":
            ctx.mol_mate_enable(MATE_BASES)

        def submit(r):
            if state == "mate_on":
                ctx.mol_mate_next(mseq, moffs)
            return ctx.submit(seq, offs, res=r)

        steps = 4
        for t in [submit(r) for r in res]:                         # warm-up: both slots, both result buffers
            ctx.wait(t)
        t0 = time.perf_counter()
        tickets = []
        for s in range(steps):
            tickets.append(submit(res[s & 1]))
            if len(tickets) == 2:
                ctx.wait(tickets.pop(0))
        for t in tickets:
            ctx.wait(t)
        rates["discarded_first_pass" if k == 0 else state].append(round(steps * n / (time.perf_counter() - t0)))
        ctx.mol_disable()
    out["host_to_host_reads_per_s"] = rates
    out["host_to_host_mate_on_over_off"] = round(max(rates["mate_on"]) / max(rates["mate_off"]), 4)
    return out


def measure_mate_filter(ctx, seq, offs, n, mseq, moffs, device):
    """the mate filter: its two kernels per batch beside td_rna_dust_kernel over the same mates, then host to host on against off"""
    from tagdust_amd import RESULT_DTYPE, TagdustHip
    from tagdust_amd import lib as tdlib
    import rna_dust_bench
    string, s_index, _ = tdlib.parse_fasta(rna_dust_bench.artifact_fasta(16))
    T = 16
    out = {"prefix_bases": MATE_PREFIX, "mate_bases": MATE_BASES, "mate_len": MATE_LEN, "dust": 100, "n_artifacts": 16, "artifact_len": 100,
           "n_threads": T, "box_to_box_spread": "+-7 % between machines of the pool: a ratio below that is no finding"}
    med = statistics.median
    spread = lambda v: {"runs": [round(x, 3) for x in v], "median": round(med(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
    ctx.set_artifacts(string, s_index, 2, T)
    ctx.mol_enable(MATE_PREFIX, LOG2_SLOTS)
    ctx.mol_mate_enable(MATE_BASES)
    ctx.mol_mate_filter_enable()
    dec, cnt, mk, fk, jk = [], [], [], [], []
    for it in range(6):
        ctx.mol_reset()
        ctx.mol_mate_next(mseq, moffs)
        ctx.upload_batch(seq, offs)
        ctx.run()
        dec.append(ctx.last_kernel_ms())
        cnt.append(ctx.get_option("molecules_kernel_us") / 1000.0)
        mk.append(ctx.get_option("mate_kernel_us") / 1000.0)
        fk.append(ctx.get_option("mate_filter_kernel_us") / 1000.0)
        jk.append(ctx.get_option("mate_join_kernel_us") / 1000.0)
        if it == 0:
            t2 = ctx.mol_mate_types()
            out["mate_types_of_one_batch"] = {"passed": int((t2 == 0).sum()), "low_complexity": int((t2 == 6).sum()),
                                              "matches_artifact": int(((t2 & 0xFF) == 5).sum())}
            out["totals_of_one_batch"] = ctx.mol_get()[1]
    out["decode_kernel_ms"], out["count_kernel_ms"], out["mate_kernel_ms"] = spread(dec[1:]), spread(cnt[1:]), spread(mk[1:])
    out["filter_kernel_ms"], out["join_kernel_ms"] = spread(fk[1:]), spread(jk[1:])
    ctx.mol_disable()
    # the yardstick: td_rna_dust_kernel over the same mates as a batch of their own, same settings, same process
    rd = TagdustHip(device)
    try:
        rd.set_params(0.0, 16, 100)
        rd.set_artifacts(string, s_index, 2, T)
        res = np.zeros(n, RESULT_DTYPE)
        ms = []
        for it in range(6):
            rd.wait(rd.submit(mseq, moffs, mode=tdlib.MODE_RNA_DUST, res=res))
            ms.append(rd.last_kernel_ms())
        out["rna_dust_kernel_ms_same_mates"] = spread(ms[1:])
        out["rna_dust_mode_equals_mate_types"] = bool(np.array_equal(res["read_type"], t2))
    finally:
        rd.close()
    out["filter_over_rna_dust_kernel"] = round(out["filter_kernel_ms"]["median"] / out["rna_dust_kernel_ms_same_mates"]["median"], 3)
    out["filter_kernel_share_of_decode"] = round(out["filter_kernel_ms"]["median"] / out["decode_kernel_ms"]["median"], 4)
    # host to host: the first pass of the process is discarded, then the filter off and on in turn, twice each
    res = [np.zeros(n, RESULT_DTYPE) for _ in range(2)]
    rates = {"discarded_first_pass": [], "filter_on": [], "filter_off": []}
    for k, state in enumerate(("filter_off", "filter_on", "filter_off", "filter_on", "filter_off")):
        ctx.mol_enable(MATE_PREFIX, LOG2_SLOTS)
        ctx.mol_mate_enable(MATE_BASES)
        if state == "filter_on":
            ctx.mol_mate_filter_enable()

        def submit(r):
            ctx.mol_mate_next(mseq, moffs)
            return ctx.submit(seq, offs, res=r)

        steps = 4
        for t in [submit(r) for r in res]:                         # warm-up: both slots, both result buffers
            ctx.wait(t)
        t0 = time.perf_counter()
        tickets = []
        for s in range(steps):
            tickets.append(submit(res[s & 1]))
            if len(tickets) == 2:
                ctx.wait(tickets.pop(0))
        for t in tickets:
            ctx.wait(t)
        rates["discarded_first_pass" if k == 0 else state].append(round(steps * n / (time.perf_counter() - t0)))
        ctx.mol_disable()
    out["host_to_host_reads_per_s"] = rates
    out["host_to_host_filter_on_over_off"] = round(max(rates["filter_on"]) / max(rates["filter_off"]), 4)
    return out


def measure_command(segs, seq, offs):
    """the whole command once each way on a FASTQ of the batch: seconds on the wall and the report's streaming seconds"""
    import shutil
    import subprocess
    import tempfile
    from tagdust_amd import build as tdbuild
    d = tempfile.mkdtemp(prefix="td_molecules_bench_")
    try:
        n, L = len(offs) - 1, bench.READ_LEN
        alpha = np.frombuffer(b"ACGT", np.uint8)
        bases = alpha[seq].reshape(n, L)
        rec = np.empty((n, 12 + 1 + L + 3 + L + 1), np.uint8)
        names = np.char.zfill(np.arange(n).astype("S11"), 11)
        rec[:, 0] = ord("@")
        rec[:, 1:12] = np.frombuffer(names.tobytes(), np.uint8).reshape(n, 11)
        rec[:, 12] = 10
        rec[:, 13:13 + L] = bases
        rec[:, 13 + L:16 + L] = np.frombuffer(b"\n+\n", np.uint8)
        rec[:, 16 + L:16 + 2 * L] = ord("I")
        rec[:, 16 + 2 * L] = 10
        fq = os.path.join(d, "in.fq")
        rec.tofile(fq)
        base = [tdbuild.EXE, "-Q", "20"] + [w for k, s in enumerate(segs) for w in ("-%d" % (k + 1), s)] + [fq, "--molecules-slots", str(LOG2_SLOTS)]
        out = {"fastq_bytes": os.path.getsize(fq), "dedup_and_collapse_umis": {"wall_s_runs": []}, "dedup_collapsed": {"wall_s_runs": []}}
        runs = [("discarded_first_run", ["--dedup", "--collapse-umis"])]   # (it compiles the model kernel; the later runs find it cached)
        runs += [("dedup_and_collapse_umis", ["--dedup", "--collapse-umis"]), ("dedup_collapsed", ["--dedup-collapsed"])] * 2
        for name, opts in runs:
            t0 = time.perf_counter()
            p = subprocess.run(base + opts + ["--force", "-o", os.path.join(d, name)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            wall = time.perf_counter() - t0
            if p.returncode != 0:
                raise RuntimeError(p.stderr.decode(errors="replace")[-2000:])
            if name == "discarded_first_run":
                out[name] = {"wall_s": round(wall, 3)}
                continue
            text = open(os.path.join(d, name + "_molecules.txt")).read().splitlines()
            out[name]["wall_s_runs"].append(round(wall, 3))
            out[name]["molecules_file_head"] = [l for l in text if l.startswith("# ") and not l.startswith("# molecules:")][:13]
        out["wall_ratio"] = round(min(out["dedup_collapsed"]["wall_s_runs"]) / min(out["dedup_and_collapse_umis"]["wall_s_runs"]), 3)
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--molecules", type=int, default=1 << 18)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "molecules.json"))
    ap.add_argument("--collapse", action="store_true", help="measure the UMI collapse alone and add a \"collapse\" section to --out")
    ap.add_argument("--dedup-collapsed", action="store_true", help="measure survey, freeze and replay alone and add a \"dedup_collapsed\" section to --out")
    ap.add_argument("--mate", action="store_true", help="measure mate mode alone and add a \"mate\" section to --out")
    ap.add_argument("--mate-filter", action="store_true", help="measure the mate filter alone and add a \"mate_filter\" section to --out")
    ap.add_argument("--with-command", action="store_true", help="with --dedup-collapsed: the whole command each way on a FASTQ of the batch")
    ap.add_argument("--command-only", action="store_true", help="with --dedup-collapsed: the whole command alone, into the section that --out already has")
    args = ap.parse_args()
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    segs = ["B:" + ",".join(bench.BARCODES), "F:" + "N" * UMI, "S:" + bench.SPACER, "R:N", "P:" + bench.ADAPTER]
    seq, offs, drawn, *mates = make_batch(args.reads, args.molecules, umi_sub=0.005 if args.collapse or args.dedup_collapsed else 0.0,
                                          with_mates=args.mate or args.mate_filter)
    head = min(args.reads, 100000)
    md, _ = tdlib.build_model(segs, seq[:offs[head]], offs[:head + 1])
    if args.dedup_collapsed and args.command_only:
        doc = json.load(open(args.out))
        doc["dedup_collapsed"]["command"] = measure_command(segs, seq, offs)
        json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
        print(json.dumps(doc["dedup_collapsed"]["command"], sort_keys=True))
        return
    ctx = TagdustHip(args.device)
    doc = {"reads": args.reads, "read_len": bench.READ_LEN, "molecules_drawn_from": args.molecules, "molecules_in_the_batch": drawn,
           "architecture": " ".join(segs), "prefix_bases": PREFIX, "table_log2_slots": LOG2_SLOTS, "threshold": 5.0}
    try:
        ctx.set_option("async_compile", 0)
        ctx.upload_model(md)
        ctx.set_params(5.0, 16, 100)
        if args.collapse:
            section = dict(doc, **measure_collapse(ctx, seq, offs, args.reads))
        elif args.dedup_collapsed:
            section = dict(doc, **measure_dedup_collapsed(ctx, seq, offs, args.reads))
        elif args.mate:
            section = dict(doc, **measure_mate(ctx, seq, offs, args.reads, *mates))
        elif args.mate_filter:
            section = dict(doc, **measure_mate_filter(ctx, seq, offs, args.reads, *mates, args.device))
        else:
            doc.update(measure(ctx, seq, offs, args.reads))
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    if args.dedup_collapsed and args.with_command:                 # (the context is closed: the command has the device to itself)
        section["command"] = measure_command(segs, seq, offs)
    if args.collapse or args.dedup_collapsed or args.mate or args.mate_filter:         # the file's other figures stay what they are
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["collapse" if args.collapse else "dedup_collapsed" if args.dedup_collapsed else "mate" if args.mate else "mate_filter"] = section
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
