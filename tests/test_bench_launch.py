"""bench.py's own launcher (no GPU needed): `python bench.py --gpus N` with WORLD_SIZE unset must start its N ranks itself --
the driver types exactly that -- relay rank 0's single JSON line and exit non-zero when a rank fails.  Beside it the host side
of --dump-outputs and the fixed inputs it relies on."""
import json
import os
import subprocess
import sys

import numpy as np

from conftest import REPO


def _bench(args, env):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, os.path.join(REPO, "bench.py")] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          env=e, timeout=600)


def test_bare_command_spawns_its_ranks_and_relays_one_line():
    p = _bench(["--gpus", "3", "--steps", "2", "--warmup", "1"], {"TD_BENCH_DRYRUN": "1"})
    assert p.returncode == 0, p.stderr.decode()[-1500:]
    lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["dryrun"] and d["n_gpus"] == 3 and d["rank_sum"] == 6 and d["local_ranks_seen"] == "3"


def test_a_failing_rank_fails_the_command():
    """Without a GPU every rank stops at "no GPU visible" (there is no CPU fallback): the parent must exit non-zero and print no
    result line."""
    p = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0", "--extras", "0", "--cpu-sample", "0"], {"HIP_VISIBLE_DEVICES": "-1", "CUDA_VISIBLE_DEVICES": ""})
    assert p.returncode != 0
    assert not [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert "no GPU visible" in p.stderr.decode()


def test_under_a_launcher_the_world_must_match():
    p = _bench(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0", "TD_BENCH_DRYRUN": "1"})
    assert p.returncode != 0 and "WORLD_SIZE=1" in p.stderr.decode()


def test_bench_input_is_pinned():
    """The bench workload's host batches are fixed by their seeds: two builds compared with --dump-outputs see the same reads.
    Digests of the generator's output for a small batch and for the third host batch of a default run (seed 1000 + 2)."""
    import hashlib
    import bench
    bench.select_workload("c3")
    for n, seed, digest in ((4096, 1000, "9760c9149c8e51ca34615f41766c0ef3"), (1 << 20, 1002, "c7779b896f4319ea7aec5f72b70d450e")):
        codes, offs = bench.synth_host_batch(n, seed)
        assert codes.dtype == np.uint8 and np.array_equal(offs, np.arange(n + 1) * bench.READ_LEN)
        assert hashlib.sha256(codes.tobytes()).hexdigest()[:32] == digest


def test_dump_outputs_layout(tmp_path):
    """--dump-outputs: every record field of every read, and the sequences and labels (read i at offs[i] + i, len_i + 1) of a
    fixed sample of reads, all as float32 / float64, within 64 MB."""
    import bench
    from tagdust_amd import RESULT_DTYPE
    rng = np.random.default_rng(5)
    n = 20000
    lens = rng.integers(1, 40, n)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    res = np.zeros(n, RESULT_DTYPE)
    for f in RESULT_DTYPE.names:
        res[f] = rng.integers(-5, 1 << 20, n)
    seq = rng.integers(0, 5, int(offs[-1])).astype(np.uint8)
    lab = rng.integers(-1, 100, int(offs[-1]) + n).astype(np.int8)
    total = bench.dump_outputs(str(tmp_path / "a"), offs, (res, seq, lab))
    bench.dump_outputs(str(tmp_path / "b"), offs, (res, seq, lab))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(["record_" + f + ".npy" for f in RESULT_DTYPE.names] +
                           ["sample_index.npy", "sample_seq_offsets.npy", "sample_seq.npy", "sample_labels.npy"])
    d = {k[:-4]: np.load(tmp_path / "a" / k) for k in names}
    assert sum(a.nbytes for a in d.values()) == total <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in d.values())
    for k in names:
        assert np.array_equal(d[k[:-4]], np.load(tmp_path / "b" / k))
    for f in RESULT_DTYPE.names:
        assert np.array_equal(d["record_" + f], res[f])
    idx = d["sample_index"].astype(np.int64)
    so = d["sample_seq_offsets"].astype(np.int64)
    assert len(idx) == bench.DUMP_SAMPLE_READS and np.all(np.diff(idx) > 0)
    lab_off = np.concatenate([[0], np.cumsum(lens[idx] + 1)])
    for j in (0, 17, len(idx) - 1):
        i = idx[j]
        assert np.array_equal(d["sample_seq"][so[j]:so[j + 1]], seq[offs[i]:offs[i + 1]])
        assert np.array_equal(d["sample_labels"][lab_off[j]:lab_off[j + 1]], lab[offs[i] + i:offs[i + 1] + i + 1])
