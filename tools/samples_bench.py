"""Measures sample assignment by all 'B' segments (include/tagdust_samples.h) on 2^20 config-3-shaped reads with a second barcode
segment of four barcodes behind the spacer: B:<8 barcodes> / S:GTA / B:<4 barcodes> / R:N / P:<adapter>.

    python tools/samples_bench.py [--reads 1048576] [--out profiles/samples.json]        # on the MI355X

The kernel's time is taken from the pair of HIP events around its launch (option "samples_kernel_us") beside the decode kernel's
time of the same batch (td_last_kernel_ms) and, in the same process on the same batch, the census count kernel's
("census_kernel_us", every outcome eligible), median of 5 batches each.  Host to host: reads/s of that batch through td_submit /
td_wait with samples off and on, two passes of each state in one process, the first pass of a state discarded.

What was expected before the first run (written here before it, not a threshold): the same walk over the labels as the census's,
shorter where the labels' segments are ordered (it ends behind the second barcode, at base 13 of 150), plus an LDS lookup and two
stores per eligible read: about the census's 0.41 ms per 2^20 reads, a few per cent of the decode kernel.  Host to host the pool's
+-7 % between machines makes a smaller difference no finding.
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

import bench  # noqa: E402  (the flagship workload's read generator)

SECOND = ["AACC", "GGTT", "CATG", "TCGA"]
EXPECTED = {"samples_kernel_ms": "about the census's 0.41 ms per 2^20 reads", "share_of_decode": "a few per cent",
            "host_to_host": "inside the pool's +-7 % between machines"}


def make_batch(n, seed=1):
    """config-3 reads with one of SECOND behind the spacer (2 % substitutions there too); one read in ten stays fully random"""
    x = bench.synth_batch_c3(n, seed, random_frac=0.0)
    rng = np.random.default_rng(seed + 1)
    at = len(bench.BARCODES[0]) + len(bench.SPACER)
    bar = np.array([["ACGT".index(c) for c in b] for b in SECOND], np.uint8)
    x[:, at:at + 4] = bar[rng.integers(0, len(SECOND), n)]
    mut = rng.random((n, 4)) < 0.02
    np.copyto(x[:, at:at + 4], rng.integers(0, 4, size=(n, 4), dtype=np.uint8), where=mut)
    rand = rng.random(n) < 0.1
    x[rand] = rng.integers(0, 4, size=(int(rand.sum()), x.shape[1]), dtype=np.uint8)
    return np.ascontiguousarray(x.reshape(-1)), np.arange(n + 1, dtype=np.int64) * x.shape[1]


def median_of_batches(ctx, seq, offs, option):
    dec, own = [], []
    for _ in range(6):
        ctx.upload_batch(seq, offs)
        ctx.run()
        dec.append(ctx.last_kernel_ms())
        own.append(ctx.get_option(option) / 1000.0)
    return [round(v, 3) for v in dec[1:]], [round(v, 3) for v in own[1:]]


def host_to_host(ctx, seq, offs, n, sheet):
    from tagdust_amd import RESULT_DTYPE
    res = [np.zeros(n, RESULT_DTYPE) for _ in range(2)]
    rates = {"off": [], "on": []}
    for state in ("off", "on", "off", "on"):
        if state == "on":
            ctx.samples_enable(sheet, None, 16)
        for keep in (False, True):                       # two passes, the first discarded
            steps = 4
            t0 = time.perf_counter()
            tickets = []
            for s in range(steps):
                tickets.append(ctx.submit(seq, offs, res=res[s & 1]))
                if len(tickets) == 2:
                    ctx.wait(tickets.pop(0))
            for t in tickets:
                ctx.wait(t)
            if keep:
                rates[state].append(round(steps * n / (time.perf_counter() - t0)))
        if state == "on":
            ctx.samples_disable()
    return rates


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "samples.json"))
    args = ap.parse_args()
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    n = args.reads
    seq, offs = make_batch(n)
    segs = ["B:" + ",".join(bench.BARCODES), "S:" + bench.SPACER, "B:" + ",".join(SECOND), "R:N", "P:" + bench.ADAPTER]
    head = min(n, 100000)
    md, _ = tdlib.build_model(segs, seq[:offs[head]], offs[:head + 1])
    sheet = [(a, b) for a in range(len(bench.BARCODES)) for b in range(len(SECOND)) if (a + b) % 2 == 0]      # 16 of the 32 pairs
    doc = {"reads": n, "read_len": bench.READ_LEN, "architecture": " ".join(segs), "samples": len(sheet), "table_log2_slots": 16,
           "expected_before_the_first_run": EXPECTED}
    ctx = TagdustHip(args.device)
    try:
        ctx.set_option("async_compile", 0)
        ctx.upload_model(md)
        ctx.set_params(0.5, 16, 100)
        ctx.census_enable(-1, 0xFF, 20)
        dec, cen = median_of_batches(ctx, seq, offs, "census_kernel_us")
        ctx.census_disable()
        doc["census_kernel_ms_runs"], doc["census_kernel_ms_median"] = cen, statistics.median(cen)
        ctx.samples_enable(sheet, None, 16)
        dec, smp = median_of_batches(ctx, seq, offs, "samples_kernel_us")
        ent, tot = ctx.samples()
        ctx.samples_disable()
        doc["decode_kernel_ms_runs"], doc["decode_kernel_ms_median"] = dec, statistics.median(dec)
        doc["samples_kernel_ms_runs"], doc["samples_kernel_ms_median"] = smp, statistics.median(smp)
        doc["samples_share_of_decode"] = round(statistics.median(smp) / statistics.median(dec), 5)
        doc["samples_over_census"] = round(statistics.median(smp) / statistics.median(cen), 3) if statistics.median(cen) > 0 else None
        doc["totals_of_five_batches_and_one"] = tot
        doc["distinct_combinations"] = len(ent)
        doc["host_to_host_reads_per_s"] = host_to_host(ctx, seq, offs, n, sheet)
        r = doc["host_to_host_reads_per_s"]
        doc["host_to_host_on_over_off"] = round(statistics.mean(r["on"]) / statistics.mean(r["off"]), 4)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
