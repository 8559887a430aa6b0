"""Measures the base-quality filter (include/tagdust_quality.h) on the molecules workload: 2^20 config-3-shaped reads with an 8-nt
UMI (tools/molecules_bench.py's generator), B:<8 barcodes> / F:NNNNNNNN / S:GTA / R:N / P:<adapter>, and qualities in which
each base is low with probability 0.05.

    python tools/quality_bench.py [--reads 1048576] [--stream-reads 1048576] [--stream-copies 4] [--out profiles/quality.json]        # on the MI355X

The judge kernel's time is taken from the pair of HIP events around its launch (option "quality_kernel_us") beside the decode
kernel's time of the same batch (td_last_kernel_ms) and, in the same process on the same batch, the census count kernel's
("census_kernel_us", every outcome eligible), median of 5 batches each; once more with qualities without a low base, where every
block of labels is skipped.  The host pack pass: td_qual_pack over the batch's bytes on one thread, seconds per batch.  Host to
host: reads/s of that batch through td_submit / td_wait with the filter off and on, two passes of each state in one process, the
first pass of a state discarded.  Streaming: td_stream_run over a FASTQ file of --stream-reads of the same reads, --stream-copies
times over (4.2 M reads, 1.3 GB), without the filter, with a filter that fails no read (max_low 1000: the same files) and with the
filter as above, the better of the last two of three runs each.

What was expected before the first run (written here before it, not a threshold): the kernel walks the same label bytes as the
census's and adds an eighth of a byte per base, so no more than the census's time per 2^20 reads; host to host the mate row's
-10 % was for a doubled upload, this one adds an eighth of the batch's bytes, so a loss beyond the pool's +-7 % between machines
would need an explanation.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import bench  # noqa: E402  (the flagship workload's barcodes, spacer, adapter and read length)
import molecules_bench  # noqa: E402  (the molecules workload's read generator)

Q, OFFSET, MAX_LOW = 20, 33, 0
EXPECTED = {"quality_kernel_ms": "no more than the census's time per 2^20 reads", "host_to_host": "inside the pool's +-7 % between machines",
            "pack": "a flat SIMD pass: a small part of the staging copy it rides on"}


def qualities(n_bases, p_low, seed=3):
    rng = np.random.default_rng(seed)
    low = rng.random(n_bases) < p_low
    q = np.where(low, OFFSET + Q - 1 - rng.integers(0, 15, n_bases), OFFSET + Q + rng.integers(0, 20, n_bases)).astype(np.uint8)
    q[(q == ord("@")) | (q == ord("+"))] += 1                # (no quality line of the streaming file starts like a header or a separator)
    return q


def median_of_batches(ctx, seq, offs, option, qual=None):
    dec, own = [], []
    for _ in range(6):
        if qual is not None:
            ctx.qual_next(qual, len(offs) - 1)
        ctx.upload_batch(seq, offs)
        ctx.run()
        dec.append(ctx.last_kernel_ms())
        own.append(ctx.get_option(option) / 1000.0)
    return [round(v, 3) for v in dec[1:]], [round(v, 3) for v in own[1:]]


def host_to_host(ctx, seq, offs, n, qual):
    from tagdust_amd import RESULT_DTYPE
    res = [np.zeros(n, RESULT_DTYPE) for _ in range(2)]
    rates = {"off": [], "on": []}
    for state in ("off", "on", "off", "on"):
        if state == "on":
            ctx.qual_enable(Q, OFFSET, MAX_LOW)
        for keep in (False, True):                       # two passes, the first discarded
            steps = 4
            t0 = time.perf_counter()
            tickets = []
            for s in range(steps):
                if state == "on":
                    ctx.qual_next(qual, n)
                tickets.append(ctx.submit(seq, offs, res=res[s & 1]))
                if len(tickets) == 2:
                    ctx.wait(tickets.pop(0))
            for t in tickets:
                ctx.wait(t)
            if keep:
                rates[state].append(round(steps * n / (time.perf_counter() - t0)))
        if state == "on":
            ctx.qual_disable()
    return rates


def write_fastq(path, seq, offs, qual, n, copies):
    """the first n reads, `copies` times over"""
    L = int(offs[1] - offs[0])
    text = np.frombuffer(b"ACGTN", np.uint8)[seq[:n * L]].reshape(n, L)
    rows = []
    for i in range(n):
        rows.append(b"@r%d\n%s\n+\n%s\n" % (i, text[i].tobytes(), qual[i * L:(i + 1) * L].tobytes()))
    once = b"".join(rows)
    with open(path, "wb") as f:
        for _ in range(copies):
            f.write(once)


def streaming(ctx, segs, seq, offs, qual, n, copies):
    """off; on with max_low 1000, where no read fails and the files are those of the off run: what judging costs; on with MAX_LOW,
    where the failed reads move to the _un file: what the run the user asked for costs"""
    import glob
    from tagdust_amd import lib as tdlib
    out = {"reads": n * copies}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fq")
        write_fastq(path, seq, offs, qual, n, copies)
        out["file_bytes"] = os.path.getsize(path)
        for state, max_low in (("off", None), ("on_nothing_fails", 1000), ("on", MAX_LOW)):
            if max_low is not None:
                ctx.qual_enable(Q, OFFSET, max_low)
            walls = []
            for k in range(3):                               # the first run of a state is discarded
                st = tdlib.stream_run(ctx, path, segs, os.path.join(d, "out"))
                walls.append(round(float(st["wall_s"]), 4))
                for f in glob.glob(os.path.join(d, "out*")):
                    os.remove(f)
            out[state + "_wall_s_runs"] = walls
            out[state + "_reads_per_s"] = round(n * copies / min(walls[1:]))
            if max_low is not None:
                out[state + "_totals_of_three_runs"] = ctx.qual_totals()
                ctx.qual_disable()
    for state in ("on_nothing_fails", "on"):
        out[state + "_over_off"] = round(out[state + "_reads_per_s"] / out["off_reads_per_s"], 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--stream-reads", type=int, default=1 << 20, help="reads of the batch that the streaming file holds (0: no streaming run)")
    ap.add_argument("--stream-copies", type=int, default=4, help="... this many times over")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "quality.json"))
    args = ap.parse_args()
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    n = args.reads
    seq, offs, _ = molecules_bench.make_batch(n, max(1, n // 4))
    qual = qualities(len(seq), 0.05)
    clean = qualities(len(seq), 0.0)
    segs = ["B:" + ",".join(bench.BARCODES), "F:" + "N" * molecules_bench.UMI, "S:" + bench.SPACER, "R:N", "P:" + bench.ADAPTER]
    head = min(n, 100000)
    md, _ = tdlib.build_model(segs, seq[:offs[head]], offs[:head + 1])
    doc = {"reads": n, "read_len": bench.READ_LEN, "architecture": " ".join(segs), "min_quality": Q, "max_low": MAX_LOW, "segments": "BF",
           "low_base_share": 0.05, "expected_before_the_first_run": EXPECTED}
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        tdlib.qual_pack(qual, OFFSET + Q)
        t.append(round(time.perf_counter() - t0, 5))
    doc["pack_one_thread_s_runs"], doc["pack_bytes"] = t, int(len(qual))
    ctx = TagdustHip(args.device)
    try:
        ctx.set_option("async_compile", 0)
        ctx.upload_model(md)
        ctx.set_params(0.5, 16, 100)
        ctx.census_enable(-1, 0xFF, 20)
        dec, cen = median_of_batches(ctx, seq, offs, "census_kernel_us")
        ctx.census_disable()
        doc["census_kernel_ms_runs"], doc["census_kernel_ms_median"] = cen, statistics.median(cen)
        ctx.qual_enable(Q, OFFSET, MAX_LOW)
        dec, own = median_of_batches(ctx, seq, offs, "quality_kernel_us", qual)
        doc["totals_of_five_batches_and_one"] = ctx.qual_totals()
        _, own_clean = median_of_batches(ctx, seq, offs, "quality_kernel_us", clean)
        ctx.qual_disable()
        doc["decode_kernel_ms_runs"], doc["decode_kernel_ms_median"] = dec, statistics.median(dec)
        doc["quality_kernel_ms_runs"], doc["quality_kernel_ms_median"] = own, statistics.median(own)
        doc["quality_kernel_ms_no_low_base_runs"], doc["quality_kernel_ms_no_low_base_median"] = own_clean, statistics.median(own_clean)
        doc["quality_share_of_decode"] = round(statistics.median(own) / statistics.median(dec), 5)
        doc["quality_over_census"] = round(statistics.median(own) / statistics.median(cen), 3) if statistics.median(cen) > 0 else None
        doc["host_to_host_reads_per_s"] = host_to_host(ctx, seq, offs, n, qual)
        r = doc["host_to_host_reads_per_s"]
        doc["host_to_host_on_over_off"] = round(statistics.mean(r["on"]) / statistics.mean(r["off"]), 4)
        if args.stream_reads > 0:
            doc["streaming"] = streaming(ctx, segs, seq, offs, qual, min(n, args.stream_reads), args.stream_copies)
    finally:
        ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
