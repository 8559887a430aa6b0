"""Measures the census of barcode spellings (include/tagdust_census.h) on 2^20 config-3 reads of which one in ten spells a
barcode outside the list -- once a long tail of random spellings, once a single heavy hitter.

    python tools/census_bench.py [--reads 1048576] [--out profiles/census.json]        # on the MI355X

Per input: the count kernel's time from HIP events (option "census_kernel_us": events around its launch) beside the decode kernel's
time of the same batch (td_last_kernel_ms), median of 5 batches; the census of the batch (eligible, counted, distinct, the top
count); and host-to-host reads/s of that batch through td_submit / td_wait with the census on and off in turn (on, off, on, off).
The census counts every outcome here (mask 0xFF), so that all reads go through the table whatever the threshold makes of them.
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

import bench  # noqa: E402  (the flagship workload's read generator and model)

UNKNOWN = "CGCGAT"          # the heavy hitter: not in bench.BARCODES


def make_batch(n, kind, seed=1):
    """config-3 reads without fully random ones; one in ten gets another barcode: a random 6-mer (tail) or UNKNOWN (heavy)"""
    x = bench.synth_batch_c3(n, seed, random_frac=0.0)
    rng = np.random.default_rng(seed + 1)
    pick = rng.random(n) < 0.1
    k = int(pick.sum())
    if kind == "tail":
        x[pick, :6] = rng.integers(0, 4, size=(k, 6), dtype=np.uint8)
    else:
        x[pick, :6] = np.array(["ACGT".index(c) for c in UNKNOWN], np.uint8)
    return np.ascontiguousarray(x.reshape(-1)), np.arange(n + 1, dtype=np.int64) * x.shape[1]


def measure(ctx, seq, offs, n):
    from tagdust_amd import RESULT_DTYPE
    out = {}
    ctx.census_enable(-1, 0xFF, 20)
    dec, cen = [], []
    for it in range(6):
        ctx.upload_batch(seq, offs)
        ctx.run()
        dec.append(ctx.last_kernel_ms())
        cen.append(ctx.get_option("census_kernel_us") / 1000.0)
        if it == 0:
            ent, tot = ctx.census(cap=3)
            out["census_of_one_batch"] = dict(tot, top=[[int(e["key"]), int(e["count"])] for e in ent])
    out["decode_kernel_ms_runs"] = [round(v, 3) for v in dec[1:]]
    out["count_kernel_ms_runs"] = [round(v, 3) for v in cen[1:]]
    d, c = statistics.median(dec[1:]), statistics.median(cen[1:])
    out["decode_kernel_ms_median"], out["count_kernel_ms_median"] = round(d, 3), round(c, 3)
    out["count_share_of_decode"] = round(c / d, 5)
    out["count_kernel_reads_per_s"] = round(n / (c * 1e-3)) if c > 0 else None
    ctx.census_disable()
    # host to host through td_submit / td_wait, the census on and off in turn
    res = [np.zeros(n, RESULT_DTYPE) for _ in range(2)]
    rates = {"on": [], "off": []}
    for state in ("on", "off", "on", "off"):
        if state == "on":
            ctx.census_enable(-1, 0xFF, 20)
        steps = 4
        ctx.wait(ctx.submit(seq, offs, res=res[0]))      # warm-up
        t0 = time.perf_counter()
        tickets = []
        for s in range(steps):
            tickets.append(ctx.submit(seq, offs, res=res[s & 1]))
            if len(tickets) == 2:
                ctx.wait(tickets.pop(0))
        for t in tickets:
            ctx.wait(t)
        rates[state].append(round(steps * n / (time.perf_counter() - t0)))
        if state == "on":
            ctx.census_disable()
    out["host_to_host_reads_per_s"] = rates
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "census.json"))
    args = ap.parse_args()
    from tagdust_amd import TagdustHip
    g = bench.load_model()
    ctx = TagdustHip(args.device)
    doc = {"reads": args.reads, "read_len": bench.READ_LEN, "workload": "config3, one read in ten spells a barcode outside the list",
           "table_log2_slots": 20, "outcome_mask": 0xFF}
    try:
        ctx.set_option("async_compile", 0)
        ctx.upload_model(g)
        ctx.set_params(float(g["threshold"]), int(g["minlen"]), int(g["dust"]))
        for kind in ("tail", "heavy"):
            seq, offs = make_batch(args.reads, kind)
            doc[kind] = measure(ctx, seq, offs, args.reads)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
