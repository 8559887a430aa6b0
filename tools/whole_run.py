#!/usr/bin/env python3
"""Measurements of the whole-run driver, as one JSON document:

  statistics   td_sequence_stats (host) against td_sequence_stats_device (upload included) on 1 000 001 config-3 reads with the
               trailing adapter: five runs each, alternating, medians -- and the two results compared byte for byte;
  whole run    the 2^20-read config-3 FASTQ of tools/e2e_pipeline.py through the command (tagdust_amd/bin/tagdust-hip, release
               constants, -seed 42): default (decode while the model kernel compiles, statistics on the device), --sync-compile,
               --stats-on-host; wall seconds of the process and the driver's own phase seconds from an in-process run.  With
               --reference PATH the reference binary runs on the same file and the output files are compared.

usage: tools/whole_run.py [n_reads] [--reference PATH] [--skip-stats] [--skip-run]"""
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np

import bench
import e2e_pipeline
from tagdust_amd import TagdustHip
from tagdust_amd import build as tdbuild
from tagdust_amd import lib as tdlib

SEGS = ["B:" + ",".join(bench.BARCODES), "S:" + bench.SPACER, "R:N", "P:" + bench.ADAPTER]


def measure_stats():
    n = 1000001
    reads = bench.synth_batch(n, 99)
    codes = np.ascontiguousarray(reads.reshape(-1), np.uint8)
    offs = np.arange(n + 1, dtype=np.int64) * reads.shape[1]
    c = TagdustHip(0)
    try:
        tdlib.sequence_stats_device(c, SEGS, codes[:offs[1000]], offs[:1001])      # (first launch: module load)
        host, dev = [], []
        for _ in range(5):
            t = time.perf_counter(); h = tdlib.sequence_stats(SEGS, codes, offs); host.append(time.perf_counter() - t)
            t = time.perf_counter(); d = tdlib.sequence_stats_device(c, SEGS, codes, offs); dev.append(time.perf_counter() - t)
            assert bytes(h) == bytes(d), "device statistics differ from the host's"
    finally:
        c.close()
    return {"reads": n, "bases": int(offs[-1]), "host_s": [round(x, 4) for x in host], "device_s": [round(x, 4) for x in dev],
            "host_median_s": round(statistics.median(host), 4), "device_median_s": round(statistics.median(dev), 4), "identical": True,
            "mean_3_len": h.mean_3_len, "stdev_3_len": h.stdev_3_len}


def measure_run(n, reference):
    out = {"reads": n, "arch": " ".join("-%d %s" % (k + 1, s) for k, s in enumerate(SEGS))}
    cores = min(len(os.sched_getaffinity(0)), 16)
    arch = [a for k, s in enumerate(SEGS) for a in ("-%d" % (k + 1), s)]
    with tempfile.TemporaryDirectory() as tmp:
        fq = os.path.join(tmp, "in.fq")
        e2e_pipeline.write_fastq(fq, bench.synth_batch(n, 99))
        out["fastq_bytes"] = os.path.getsize(fq)
        files = {}
        for tag, extra in (("default", []), ("sync_compile", ["--sync-compile"]), ("stats_on_host", ["--stats-on-host"])):
            cmd = [tdbuild.EXE] + extra + ["-t", str(cores), "-seed", "42"] + arch + [fq, "-o", os.path.join(tmp, tag)]
            t = time.perf_counter()
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
            out[tag] = {"wall_s": round(time.perf_counter() - t, 3), "rc": p.returncode}
            if p.returncode:
                out[tag]["stderr"] = p.stderr.decode(errors="replace")[-500:]
            files[tag] = {os.path.basename(f)[len(tag):]: open(f, "rb").read() for f in glob.glob(os.path.join(tmp, tag + "*.fq"))}
        out["cases_identical"] = bool(files["default"]) and files["default"] == files["sync_compile"] == files["stats_on_host"]
        rep = tdlib.run_execute(["-t", str(cores), "-seed", "42"] + arch + [fq, "-o", os.path.join(tmp, "inproc")])   # (kernel cached by now)
        out["in_process_phases_s"] = {k: round(v, 3) for k, v in rep["seconds"].items()}
        out["in_process_stream"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in rep["stream"].items()}
        out["threshold"] = rep["thresholds"][0]
        if reference and os.path.exists(reference):
            t = time.perf_counter()
            p = subprocess.run([reference, "-t", str(cores), "-seed", "42"] + arch + [fq, "-o", os.path.join(tmp, "ref")], stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, timeout=1100)
            out["reference"] = {"wall_s": round(time.perf_counter() - t, 3), "threads": cores, "rc": p.returncode}
            ref = {os.path.basename(f)[3:]: open(f, "rb").read() for f in glob.glob(os.path.join(tmp, "ref*.fq"))}
            out["identical_output_files"] = bool(ref) and ref == files["default"]
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 1 << 20
    reference = sys.argv[sys.argv.index("--reference") + 1] if "--reference" in sys.argv else None
    out = {}
    if "--skip-stats" not in sys.argv:
        out["statistics"] = measure_stats()
    if "--skip-run" not in sys.argv:
        out["whole_run"] = measure_run(n, reference)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
