"""What the first calls on a new context cost (config 3, 2^20 reads).

  python tools/first_call.py              the cold-cache leg: a fresh TD_SPEC_CACHE_DIR and a cache key of its own per leg, so that
                                          every leg really compiles.  Seconds from td_model_upload to the first complete batch with
                                          the synchronous compile against option "async_compile" (the generic kernel decodes until
                                          the compiled one is handed over), the batch index of the hand-over, and what the load-time
                                          probe costs ("spec_probe" 1 against 0).  One JSON line at the end.
  python tools/first_call.py --workspace  the workspace-placement leg (TD_WS_CANDIDATES 3 against 1)

A library without the "async_compile" option (an older build, TD_LIB_PATH) runs the synchronous leg alone."""
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tagdust_amd import TagdustHip, RESULT_DTYPE, TdError  # noqa: E402

N = 1 << 20


def workspace_leg(model, reads, offs):
    for cand in ("3", "1"):
        os.environ["TD_WS_CANDIDATES"] = cand
        t = time.perf_counter(); c = TagdustHip(0); t_ctx = time.perf_counter() - t
        t = time.perf_counter(); c.upload_model(model); t_model = time.perf_counter() - t
        c.set_params(float(model["threshold"]), 16, 100)
        t = time.perf_counter(); c.upload_batch(reads, offs); t_up = time.perf_counter() - t
        t = time.perf_counter(); c.run(); c.sync(); t_run = time.perf_counter() - t
        res = np.zeros(N, RESULT_DTYPE); sq = np.zeros(N * 150, np.uint8)
        t = time.perf_counter(); tk = c.submit(reads, offs, res=res, seq_out=sq); tk2 = c.submit(reads, offs, res=res, seq_out=sq); c.wait(tk); c.wait(tk2); t_sub = time.perf_counter() - t
        t = time.perf_counter(); c.close(); t_close = time.perf_counter() - t
        print("candidates %s: ctx %.2f s, model upload %.2f s, first upload_batch %.2f s (workspace), first run %.3f s, first two submits (second workspace) %.2f s, close %.2f s" % (cand, t_ctx, t_model, t_up, t_run, t_sub, t_close), flush=True)


def cold_leg(model, reads, offs, leg, async_compile, probe):
    """One context, one fresh compile: returns the timings of the leg."""
    os.environ["TD_SPEC_EXTRA_OPTS"] = "-DTD_FIRST_CALL_LEG=%d" % leg
    c = TagdustHip(0)
    out = {"async": async_compile, "probe": probe}
    try:
        have = True
        try:
            c.set_option("async_compile", async_compile)
            c.set_option("spec_probe", probe)
        except TdError:
            have = False
            if async_compile or not probe:
                return None
        c.set_option("pipeline_depth", 3)
        res = np.zeros(N, RESULT_DTYPE)
        sq = np.zeros(int(offs[-1]), np.uint8)
        t0 = time.perf_counter()
        c.upload_model(model)
        out["upload_s"] = time.perf_counter() - t0
        c.set_params(float(model["threshold"]), 16, 100)
        c.wait(c.submit(reads, offs, res=res, seq_out=sq))
        out["first_batch_s"] = time.perf_counter() - t0
        first = res["read_type"].copy()
        n_batches, handover = 1, (1 if not have or c.get_option("spec_state") == 3 else 0)
        while have and not handover and time.perf_counter() - t0 < 120.0:
            c.wait(c.submit(reads, offs, res=res, seq_out=sq))
            n_batches += 1
            if c.get_option("spec_state") == 3:
                handover = n_batches
                out["handover_s"] = time.perf_counter() - t0
        assert np.array_equal(first, res["read_type"])
        out["handover_batch"] = handover
        if have:
            out["state"] = c.get_option("spec_state")
            out["batches_generic"] = c.get_option("spec_batches_generic")
            out["probe_ms"] = c.get_option("spec_probe_us") / 1000.0
        c.wait(c.submit(reads, offs, res=res, seq_out=sq))
        out["steady_kernel_ms"] = c.last_kernel_ms()
    finally:
        t = time.perf_counter()
        c.close()
        out["close_s"] = time.perf_counter() - t
    return out


def main():
    bench.select_workload("c3")
    model = bench.load_model()
    reads, offs = bench.synth_host_batch(N, 5)
    if "--workspace" in sys.argv:
        workspace_leg(model, reads, offs)
        return
    with tempfile.TemporaryDirectory() as d:
        os.environ["TD_SPEC_CACHE_DIR"] = d
        legs = {}
        for leg, (name, a, p) in enumerate((("sync", 0, 1), ("sync_noprobe", 0, 0), ("async", 1, 1))):
            r = cold_leg(model, reads, offs, leg + 1, a, p)
            if r is None:
                continue
            legs[name] = r
            print("%-12s upload %.2f s, first complete batch %.2f s after the upload began, hand-over at batch %s, probe %s ms, close %.2f s" % (
                name, r["upload_s"], r["first_batch_s"], r["handover_batch"], r.get("probe_ms", "-"), r["close_s"]), flush=True)
    print(json.dumps({"tool": "first_call", "workload": "c3", "n_reads": N, "legs": legs}))


if __name__ == "__main__":
    main()
