"""Measures sample assignment by all 'B' segments (include/tagdust_samples.h) on 2^20 config-3-shaped reads with a second barcode
segment of four barcodes behind the spacer: B:<8 barcodes> / S:GTA / B:<4 barcodes> / R:N / P:<adapter>.

    python tools/samples_bench.py [--reads 1048576] [--out profiles/samples.json]        # on the MI355X
    python tools/samples_bench.py --join-stream [--out profiles/samples.json]   # ... and td_stream_run_multi over three files, join against the one-column shape
    python tools/samples_bench.py --join [--out profiles/samples.json]   # the join across input files: export and join kernel beside td_samples_kernel

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


def median_with_words(ctx, seq, offs, option, name_words):
    """as median_of_batches, with the words of the join named in front of every batch"""
    own = []
    for _ in range(6):
        name_words()
        ctx.upload_batch(seq, offs)
        ctx.run()
        own.append(ctx.get_option(option) / 1000.0)
    return [round(v, 3) for v in own[1:]]


def join_kernels(ctx, seq, offs, n, sheet):
    """--join: the exporter's and the primary's kernels of the join across input files beside td_samples_kernel, one process, the
    same model and batch: the export of the model's own two columns; the join of them with a third column of four barcodes whose
    words are drawn here (one partner in twenty failed, one in twenty the decoy)."""
    rng = np.random.default_rng(3)
    ctx.samples_enable(sheet, None, 16)
    _, smp = median_of_batches(ctx, seq, offs, "samples_kernel_us")
    ctx.samples_disable()
    ctx.samples_export_enable(0)
    out = np.zeros(n, np.uint32)
    exp = median_with_words(ctx, seq, offs, "samples_export_kernel_us", lambda: ctx.samples_export_next(out, n))
    ctx.samples_export_disable()
    words = ((rng.integers(0, 4, n).astype(np.uint32) + 1) << 16)
    r = rng.random(n)
    words[r < 0.05] = 5 << 16
    words[r > 0.95] = 0xFFFFFFFF
    sheet3 = [(a, b, c) for a, b in sheet for c in range(4) if (a + c) % 2 == 0]
    hm = [len(bench.BARCODES) + 1, len(SECOND) + 1, 5]
    ctx.samples_join_enable(sheet3, hm, 0, None, 16)
    join = median_with_words(ctx, seq, offs, "samples_join_kernel_us", lambda: ctx.samples_join_next(words, n))
    _, tot = ctx.samples_join()
    ctx.samples_disable()
    return {"samples_kernel_ms_runs": smp, "samples_kernel_ms_median": statistics.median(smp),
            "export_kernel_ms_runs": exp, "export_kernel_ms_median": statistics.median(exp),
            "join_kernel_ms_runs": join, "join_kernel_ms_median": statistics.median(join),
            "join_samples": len(sheet3), "join_columns": 3, "join_totals_of_six_batches": tot}


I7 = ["AACCGGTT", "ACGTTGCA", "CATGGTAC", "GGATCCAA", "TTGACGTC", "CGTAATGC", "GTCAGTCA", "TAGCTAGG"]
I5 = ["ATATCGCG", "CCGGAATT", "GACTGACT", "TGCATGCA", "AGGTCCTA", "CTAGAGCT", "GTTAACCG", "TCCGTTAG"]


def write_fastq_fixed(path, codes):
    """n reads of one length as FASTQ, names r0000000.."""
    n, ln = codes.shape
    rec = np.empty((n, 10 + ln + 3 + ln + 1), np.uint8)
    rec[:, 0] = ord("@")
    rec[:, 1] = ord("r")
    digits = np.arange(n)
    for k in range(7):
        rec[:, 8 - k] = ord("0") + digits % 10
        digits = digits // 10
    rec[:, 9] = 10
    rec[:, 10:10 + ln] = np.frombuffer(b"ACGTN", np.uint8)[codes]
    rec[:, 10 + ln:13 + ln] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 13 + ln:13 + 2 * ln] = ord("I")
    rec[:, 13 + 2 * ln] = 10
    rec.tofile(path)


def join_stream(n, device, workdir):
    """--join-stream: td_stream_run_multi records/s over three files -- two 8-nt index files and one 150-base read file -- with the
    join (file 0 joins, file 1 exports, a two-column sheet), against the same three files with the second index file declared R:N
    and a one-column sheet (td_samples_enable), the shape that needs no join.  The two layouts alternate, three runs each in one
    process after one discarded run of each; batches of 2^18 records."""
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    rng = np.random.default_rng(5)
    bars = [np.array([["ACGT".index(c) for c in b] for b in lst], np.uint8) for lst in (I7, I5)]
    idx = []
    for t in range(2):
        x = bars[t][rng.integers(0, 8, n)]
        mut = rng.random((n, 8)) < 0.02
        np.copyto(x, rng.integers(0, 4, size=(n, 8), dtype=np.uint8), where=mut)
        idx.append(np.ascontiguousarray(x))
    reads = rng.integers(0, 4, size=(n, 150), dtype=np.uint8)
    paths = [os.path.join(workdir, f) for f in ("I1.fq", "I2.fq", "R1.fq")]
    for p, x in zip(paths, idx + [reads]):
        write_fastq_fixed(p, x)
    segs = [["B:" + ",".join(I7)], ["B:" + ",".join(I5)]]
    head = min(n, 100000)
    mds = [tdlib.build_model(segs[t], idx[t][:head].reshape(-1), np.arange(head + 1, dtype=np.int64) * 8)[0] for t in range(2)]
    sheet2 = [(a, b) for a in range(8) for b in range(8) if (a + b) % 2 == 0]
    sheet1 = [(a,) for a in range(8)]
    ctxs = [TagdustHip(device) for _ in range(2)]
    rates = {"join": [], "one_column": []}
    try:
        for t in range(2):
            ctxs[t].upload_model(mds[t])
            ctxs[t].set_params(0.5, 16, 100)
        for rep in range(4):
            for layout in ("join", "one_column"):
                if layout == "join":
                    ctxs[0].samples_join_enable(sheet2, [9, 9], 0)
                    ctxs[1].samples_export_enable(1)
                    files = [(paths[0], segs[0], [ctxs[0]]), (paths[1], segs[1], [ctxs[1]]), (paths[2], ["R:N"], None)]
                else:
                    ctxs[0].samples_enable(sheet1, None, 16)
                    files = [(paths[0], segs[0], [ctxs[0]]), (paths[1], ["R:N"], None), (paths[2], ["R:N"], None)]
                t0 = time.perf_counter()
                st, cnt = tdlib.stream_run_multi(files, os.path.join(workdir, "out_" + layout), n_devices=1, dust=100, batch_reads=1 << 18)
                dt = time.perf_counter() - t0
                assert st["n_reads"] == n
                if rep:
                    rates[layout].append(round(n / dt))
                ctxs[0].samples_disable()
                if layout == "join":
                    ctxs[1].samples_export_disable()
    finally:
        for c in ctxs:
            c.close()
    return {"records": n, "batch_reads": 1 << 18, "files": "two 8-nt index files (8 barcodes each, 2 % substitutions), one 150-base read file (R:N, no contexts)",
            "records_per_s_join_runs": rates["join"], "records_per_s_one_column_runs": rates["one_column"],
            "records_per_s_join_median": statistics.median(rates["join"]), "records_per_s_one_column_median": statistics.median(rates["one_column"]),
            "join_over_one_column": round(statistics.median(rates["join"]) / statistics.median(rates["one_column"]), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--join", action="store_true", help="measure only the kernels of the join across input files; the result goes under the key "
                    "\"join\" of the --out file, whose other keys stay")
    ap.add_argument("--join-stream", action="store_true", help="measure only td_stream_run_multi over three files with the join against the one-column "
                    "shape; the result goes under the key \"join_stream\" of the --out file")
    ap.add_argument("--workdir", default=None, help="--join-stream: where the three input files and the outputs are written [a temporary directory]")
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "samples.json"))
    args = ap.parse_args()
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    n = args.reads
    if args.join_stream:
        import tempfile
        with tempfile.TemporaryDirectory(dir=args.workdir) as wd:
            res = join_stream(n, args.device, wd)
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["join_stream"] = res
        json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
        print(json.dumps(res, sort_keys=True))
        return
    seq, offs = make_batch(n)
    segs = ["B:" + ",".join(bench.BARCODES), "S:" + bench.SPACER, "B:" + ",".join(SECOND), "R:N", "P:" + bench.ADAPTER]
    head = min(n, 100000)
    md, _ = tdlib.build_model(segs, seq[:offs[head]], offs[:head + 1])
    sheet = [(a, b) for a in range(len(bench.BARCODES)) for b in range(len(SECOND)) if (a + b) % 2 == 0]      # 16 of the 32 pairs
    doc = {"reads": n, "read_len": bench.READ_LEN, "architecture": " ".join(segs), "samples": len(sheet), "table_log2_slots": 16,
           "expected_before_the_first_run": EXPECTED}
    ctx = TagdustHip(args.device)
    if args.join:
        try:
            ctx.set_option("async_compile", 0)
            ctx.upload_model(md)
            ctx.set_params(0.5, 16, 100)
            res = dict(join_kernels(ctx, seq, offs, n, sheet), reads=n)
        finally:
            ctx.close()
        doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
        doc["join"] = res
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
        print(json.dumps(res, sort_keys=True))
        return
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
