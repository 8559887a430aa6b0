"""Measurements of run_rna_dust on the device (TD_MODE_RNA_DUST, td_rnadust.hip) and of -ref in multi-file runs.

  (a) kernel:  milliseconds of td_rna_dust_kernel per 2^20 reads (HIP events around the launch, td_last_kernel_ms) for reads of
               76 and 150 nt and 1, 16, 64 artifact sequences of 100 nt, against the VALU issue bound: steps x VALU per step
               (from the kernel's ISA) over 1.229e12 wave-instructions/s.  A `rocprofv3 --kernel-trace --stats` run of
               `--only kernel` is the cross-check.
  (b) e2e:     the CASAVA three-read shape through td_stream_run_multi, --records records, with 16 artifact sequences and without
               a filter, both with batch_reads 1 000 001; the two alternate in one process and the warm second run of each counts.
  (c) cpu:     the unmodified reference (oracle/_ref/tagdust -t 16 -ref) on a 2^20-record slice of the same files.

Prints one JSON line per measurement and, with --out, writes them all to a JSON file."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# VALU instructions per text character of the kernel's inner loop, both strands together: the 16-character unrolled body of
# td_rna_dust_kernel for waves whose reads all have >= 63 bases (864 VALU / 16), read off the gfx950 ISA (hipcc -save-temps)
VALU_PER_CHAR = 54
WAVE_INSTR_PER_S = 1.229e12


def artifact_fasta(n_seq, length=100, seed=7):
    rng = np.random.default_rng(seed)
    return b"".join(b">a%d\n" % j + bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, length)]) + b"\n" for j in range(n_seq))


def kernel_times(reps=5):
    from tagdust_amd import TagdustHip, RESULT_DTYPE
    from tagdust_amd import lib as tdlib
    out = []
    n = 1 << 20
    ctx = TagdustHip(0)
    try:
        ctx.set_params(0.0, 16, 100)
        for L in (76, 150):
            rng = np.random.default_rng(L)
            codes = tdlib.PinnedArray((n * L,), np.uint8)
            codes.array[:] = rng.integers(0, 4, n * L, dtype=np.uint8)
            offs = np.arange(n + 1, dtype=np.int64) * L
            res = tdlib.PinnedArray((n,), RESULT_DTYPE)
            for n_seq in (1, 16, 64):
                string, s_index, _ = tdlib.parse_fasta(artifact_fasta(n_seq))
                ctx.set_artifacts(string, s_index, 2, 16)
                ms = []
                for r in range(reps + 1):
                    ctx.wait(ctx.submit(codes.array, offs, mode=tdlib.MODE_RNA_DUST, res=res.array))
                    if r:
                        ms.append(ctx.last_kernel_ms())
                chars = int(s_index[-1])                        # 'X' bytes included: the kernel scans them too
                wave_instr = (n / 64) * chars * VALU_PER_CHAR
                bound_ms = wave_instr / WAVE_INSTR_PER_S * 1e3
                med = float(np.median(ms))
                rec = {"what": "kernel", "read_len": L, "n_artifacts": n_seq, "artifact_len": 100, "reads": n, "kernel_ms_median": med,
                       "kernel_ms_min": float(min(ms)), "valu_bound_ms": bound_ms, "share_of_valu_bound": bound_ms / med,
                       "hits": int(((res.array["read_type"] & 0xFF) == 5).sum()), "low_complexity": int((res.array["read_type"] == 6).sum())}
                print(json.dumps(rec), flush=True)
                out.append(rec)
            codes.free()
            res.free()
    finally:
        ctx.close()
    return out


def e2e(records, n_threads=0):
    import bench
    from tagdust_amd import TagdustHip
    from tagdust_amd import lib as tdlib
    z = np.load(os.path.join(REPO, "tests", "golden", "casava_index.npz"))
    model = {k: z[k] for k in z.files}
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.time()
        r1, r2, r3, segs = bench.write_casava_files(tmp, records)
        print(json.dumps({"what": "files", "records": records, "seconds": time.time() - t0}), flush=True)
        open(os.path.join(tmp, "art.fa"), "wb").write(artifact_fasta(16))
        string, s_index, _ = tdlib.parse_fasta(artifact_fasta(16))
        cx = {k: TagdustHip(0) for k in ("idx", "idx_ref", "r1", "r3")}
        try:
            for k in ("idx", "idx_ref"):
                cx[k].upload_model(model)
                cx[k].set_params(float(model["threshold"]), int(model["minlen"]), int(model["dust"]))
            for k in ("r1", "r3"):
                cx[k].set_params(0.0, 16, int(model["dust"]))
            for k in ("idx_ref", "r1", "r3"):
                cx[k].set_artifacts(string, s_index, 2, 16)
            runs = {"no_filter": [(r2, segs, [cx["idx"]]), (r1, ["R:N"], None), (r3, ["R:N"], None)],
                    "ref_16": [(r2, segs, [cx["idx_ref"]]), (r1, ["R:N"], [cx["r1"]]), (r3, ["R:N"], [cx["r3"]])]}
            got = {}
            for rep in range(2):
                for name, files in runs.items():
                    # (one output directory per run: the two runs' files must not meet on disk)
                    st, cnt = tdlib.stream_run_multi(files, os.path.join(tmp, "o_" + name), dust=int(model["dust"]), batch_reads=1000001,
                                                     n_threads=n_threads)
                    for p in os.listdir(tmp):
                        if p.startswith("o_" + name):
                            os.unlink(os.path.join(tmp, p))
                    if rep == 1:
                        got[name] = {"what": "e2e", "run": name, "records": st["n_reads"], "batches": st["n_batches"], "wall_s": st["wall_s"],
                                     "records_per_s": st["n_reads"] / st["wall_s"], "read_s": st["read_s"], "parse_busy_s": st["parse_s"],
                                     "decode_thread_busy_s": st["decode_s"], "write_busy_s": st["write_s"], "artifact_hits": int(cnt[5]),
                                     "low_complexity": int(cnt[6]), "extracted": int(cnt[0])}
                        print(json.dumps(got[name]), flush=True)
            ratio = got["ref_16"]["records_per_s"] / got["no_filter"]["records_per_s"]
            rec = {"what": "e2e_ratio", "ref_16_over_no_filter": ratio}
            print(json.dumps(rec), flush=True)
            out += [got["no_filter"], got["ref_16"], rec]
        finally:
            for c in cx.values():
                c.close()
    return out


def cpu_baseline(records):
    import bench
    exe = os.path.join(REPO, "oracle", "_ref", "tagdust")
    if not os.path.exists(exe):
        return []
    z = np.load(os.path.join(REPO, "tests", "golden", "casava_index.npz"))
    args = str(z["cmdline"]).split()
    with tempfile.TemporaryDirectory() as tmp:
        r1, r2, r3, segs = bench.write_casava_files(tmp, records)
        open(os.path.join(tmp, "art.fa"), "wb").write(artifact_fasta(16))
        t0 = time.time()
        subprocess.run([exe] + args + ["-ref", os.path.join(tmp, "art.fa"), "-fe", "2", "-t", "16", r2, r1, r3, "-o", os.path.join(tmp, "cpu")],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=1500)
        dt = time.time() - t0
    rec = {"what": "cpu_reference", "records": records, "threads": 16, "n_artifacts": 16, "wall_s": dt, "records_per_s": records / dt}
    print(json.dumps(rec), flush=True)
    return [rec]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--only", choices=["kernel", "e2e", "cpu"], action="append", help="run only these parts (repeatable)")
    ap.add_argument("--records", type=int, default=1 << 23, help="records of the e2e runs (default 2^23)")
    ap.add_argument("--cpu-records", type=int, default=1 << 20, help="records of the reference run (default 2^20)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", help="write all results to this JSON file")
    a = ap.parse_args()
    parts = a.only or ["kernel", "e2e", "cpu"]
    res = []
    if "kernel" in parts:
        res += kernel_times(a.reps)
    if "e2e" in parts:
        res += e2e(a.records)
    if "cpu" in parts:
        res += cpu_baseline(a.cpu_records)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
