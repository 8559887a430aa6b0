"""Measures the read-pair merger (include/tagdust_merge.h) on generated pairs of 2 x 150 bp with 40 % overlap.

    python tools/merge_bench.py --gpu  [--pairs 1048576] [--out profiles/merge.json]     # on the MI355X
    python tools/merge_bench.py --cpu  [--reference-src DIR] [--out profiles/merge.json]  # anywhere: host path, reference binary

--gpu: kernel time from HIP events (median of 5 over one batch of 2^18 pairs, table in LDS and in global memory), achieved
cells/s against the LDS-gather rate DESIGN.md section 4 quotes, and td_merge_stream files -> file (pairs/s, seconds per stage).
--cpu: td_merge_host with 16 threads on a 2^16-pair slice and, when the reference's sources are given, its `merge -t 16 >
/dev/null` on the same slice (compiled into a temporary directory by tests/golden/make_merge_golden.py's recipe).
Results are merged into the JSON file under the keys "gpu" and "cpu".
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

READ_LEN, OVERLAP, MIN_OVERLAP = 150, 60, 16
QUALS = np.frombuffer(b",5AF", np.uint8)            # a binned instrument: Phred 11, 20, 32, 37
QUAL_P = [0.05, 0.10, 0.25, 0.60]
LDS_GATHER_NS_PER_CU = 1.7                         # one wave64 ds_read_b32 gather per 1.7 ns per CU
N_CU = 256


def cells_per_pair(lf=READ_LEN, lr=READ_LEN, m=MIN_OVERLAP):
    a = sum(min(lf - i, lr) for i in range(lf) if lf - i > m and lr > m)
    b = sum(min(lf, lr - j) for j in range(lr) if lf > m and lr - j > m)
    return a + b


def generate(n, seed=1):
    """FASTQ text of n pairs: a fragment of 2 x 150 - 60 bases, read 1 its head, read 2 the reverse complement of its tail"""
    rng = np.random.default_rng(seed)
    frag_len = 2 * READ_LEN - OVERLAP
    frag = rng.integers(0, 4, size=(n, frag_len), dtype=np.uint8)
    letters = np.frombuffer(b"ACGT", np.uint8)
    out = []
    for which in (1, 2):
        codes = frag[:, :READ_LEN] if which == 1 else (3 - frag[:, frag_len - READ_LEN:])[:, ::-1]
        qual = QUALS[rng.choice(4, size=(n, READ_LEN), p=QUAL_P)]
        err = rng.random((n, READ_LEN)) < 10.0 ** (-(qual.astype(np.float64) - 33.0) / 10.0)
        codes = np.where(err, (codes + rng.integers(1, 4, size=codes.shape, dtype=np.uint8)) % 4, codes).astype(np.uint8)
        names = np.char.add(np.char.add("@M01:7:FC:1:1101:", np.arange(n).astype(str)), ":%d %d:N:0:1" % (2000, which)).astype("S")
        w = names.dtype.itemsize
        rec = np.full((n, w + 1 + READ_LEN + 3 + READ_LEN + 1), ord("\n"), np.uint8)
        rec[:, :w] = np.frombuffer(names.tobytes(), np.uint8).reshape(n, w)
        rec[:, w + 1:w + 1 + READ_LEN] = letters[codes]
        rec[:, w + 2 + READ_LEN] = ord("+")
        rec[:, w + 4 + READ_LEN:w + 4 + 2 * READ_LEN] = qual
        text = rec.tobytes().replace(b"\x00", b"")          # (names are padded with NULs to one width)
        out.append(text)
    return out


def write_files(tmp, n, tag):
    t1, t2 = generate(n)
    p1, p2 = os.path.join(tmp, "r1_%s.fq" % tag), os.path.join(tmp, "r2_%s.fq" % tag)
    open(p1, "wb").write(t1)
    open(p2, "wb").write(t2)
    return p1, p2, t1, t2


def run_gpu(args, tmp):
    from tagdust_amd import lib as tdlib
    res = {"pairs": args.pairs, "read_len": READ_LEN, "overlap": OVERLAP, "cells_per_pair": cells_per_pair()}
    nb = min(args.pairs, 1 << 18)
    _, _, t1, t2 = write_files(tmp, nb, "batch")
    r1, r2 = tdlib.ParsedReads(t1), tdlib.ParsedReads(t2)
    host = None
    for key, placement in (("lds", tdlib.MERGE_TABLE_LDS), ("global", tdlib.MERGE_TABLE_GLOBAL)):
        ms = []
        for _ in range(6):
            r = tdlib.merge_batch(r1, r2, args.device, table_placement=placement)
            ms.append(r["kernel_ms"])
        med = statistics.median(ms[1:])
        cells = nb * cells_per_pair() / (med * 1e-3)
        bound = N_CU * 64 / (LDS_GATHER_NS_PER_CU * 1e-9)
        res["kernel_" + key] = {"batch_pairs": nb, "kernel_ms_runs": [round(x, 3) for x in ms[1:]], "kernel_ms_median": round(med, 3),
                                "pairs_per_s": round(nb / (med * 1e-3)), "cells_per_s": cells,
                                "lds_gather_bound_cells_per_s": bound, "fraction_of_bound": round(cells / bound, 3)}
        if host is None:
            host = r["n_written"]
    res["batch_written"] = host
    p1, p2, _, _ = write_files(tmp, args.pairs, "all")
    out = os.path.join(tmp, "merged.fq")
    runs = []
    for _ in range(3):
        st = tdlib.merge_stream(p1, p2, out, args.device, n_threads=8)
        runs.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in st.items()})
    best = min(runs, key=lambda s: s["wall_s"])
    res["stream"] = {"runs": runs, "pairs_per_s_best": round(best["n_pairs"] / best["wall_s"]), "host_threads": 8}
    return res


def run_cpu(args, tmp):
    from tagdust_amd import lib as tdlib
    n = 1 << 16
    p1, p2, t1, t2 = write_files(tmp, n, "slice")
    r1, r2 = tdlib.ParsedReads(t1), tdlib.ParsedReads(t2)
    t0 = time.time()
    r = tdlib.merge_batch(r1, r2, None, n_threads=16)
    dt = time.time() - t0
    res = {"slice_pairs": n, "cpus": os.cpu_count(), "td_merge_host_16_threads": {"seconds": round(dt, 3), "pairs_per_s": round(n / dt), "written": r["n_written"]}}
    if args.reference_src:
        sys.path.insert(0, os.path.join(REPO, "tests", "golden"))
        import make_merge_golden
        exe = make_merge_golden.build_reference(args.reference_src, tmp)
        t0 = time.time()
        with open(os.devnull, "wb") as null:
            subprocess.run([exe, "-t", "16", p1, p2], stdout=null, stderr=null, check=True)
        dt = time.time() - t0
        res["reference_merge_t16"] = {"seconds": round(dt, 3), "pairs_per_s": round(n / dt)}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--reference-src", default=None, help="directory of the reference package (its src/merge.c is compiled into a temporary directory)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "merge.json"))
    args = ap.parse_args()
    if not (args.gpu or args.cpu):
        ap.error("give --gpu and/or --cpu")
    doc = {}
    if os.path.exists(args.out):
        doc = json.load(open(args.out))
    with tempfile.TemporaryDirectory() as tmp:
        if args.gpu:
            doc["gpu"] = run_gpu(args, tmp)
        if args.cpu:
            doc["cpu"] = run_cpu(args, tmp)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(doc, open(args.out, "w"), indent=1, sort_keys=True)
    print(json.dumps(doc, sort_keys=True))


if __name__ == "__main__":
    main()
