"""The command (tagdust_amd/bin/tagdust-hip over include/tagdust_run.h) against the unmodified reference binary
(oracle/_ref/tagdust_rtest): the same set of output files with the same bytes, the same summary block in the log.  Both run with
the -DRTEST constants (--rtest: 1000-record batches, 4000 calibration reads on the private generator).  One child process at a
time, each with a time limit."""
import glob
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import REPO, load_golden

pytestmark = pytest.mark.gpu

RBIN = os.path.join(REPO, "oracle", "_ref")
EXE = os.path.join(REPO, "tagdust_amd", "bin", "tagdust-hip")
ALPHA = np.frombuffer(b"ACGTN", np.uint8)


def _need_ref():
    if not os.path.exists(os.path.join(RBIN, "tagdust_rtest")):
        pytest.skip("oracle/_ref/tagdust_rtest not built")


def _write_fastq(g, path):
    names = bytes(g["names"]).split(b"\n")
    offs = g["offs"]
    with open(path, "wb") as fh:
        for i in range(int(g["n_reads"])):
            s = bytes(ALPHA[g["seq"][offs[i]:offs[i + 1]]])
            q = bytes(g["qual"][offs[i]:offs[i + 1]])
            fh.write(b"@" + names[i] + b"\n" + s + b"\n+\n" + q + b"\n")


def _ref(args, cwd):
    p = subprocess.run([os.path.join(RBIN, "tagdust_rtest")] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert p.returncode == 0, p.stdout.decode(errors="replace")[-2000:]


def _hip(args, cwd, specialize=False, timeout=120, rc=0):
    env = dict(os.environ)
    if specialize:
        env.pop("TD_SPECIALIZE", None)
    else:
        env["TD_SPECIALIZE"] = "0"          # (keeps hiprtc compiles out of the cases that are not about them)
    p = subprocess.run([EXE, "--rtest"] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, env=env)
    err = p.stderr.decode(errors="replace")
    assert p.returncode == rc, err[-3000:]
    return err


def _outputs(d, prefix):
    return {os.path.basename(p)[len(prefix):]: open(p, "rb").read() for p in sorted(glob.glob(os.path.join(d, prefix + "*")))
            if not p.endswith("_logfile.txt")}


def _log(d, prefix):
    """The log's messages without their time stamps."""
    out = []
    for line in open(os.path.join(d, prefix + "_logfile.txt")).read().splitlines():
        out.append(line.split("]\t", 1)[1] if line.startswith("[") and "]\t" in line else line)
    return out


def _summary(d, prefix):
    lines = _log(d, prefix)
    at = [i for i, l in enumerate(lines) if l.endswith("\ttotal input reads")]
    assert at, lines
    return lines[at[0]:]


def _same_files(d):
    cpu, gpu = _outputs(d, "cpu"), _outputs(d, "gpu")
    assert cpu and set(cpu) == set(gpu), (sorted(cpu), sorted(gpu))
    for k in cpu:
        assert cpu[k] == gpu[k], "output file *%s differs" % k
    return cpu


# ---- G3 ----
CASES = [(n, [], False) for n in ("c2_b4_r", "c3_b6_s_r_p", "umi_f_s_r", "b_r_s_r", "dust_b_r", "window_b_r", "win_r_s_b_r", "c5_big_b96_f_r_p")]
CASES += [("c5_big_b96_f_r_p", ["--stats-on-host"], False), ("c3_b6_s_r_p", ["--sync-compile"], True)]


@pytest.mark.parametrize("name,extra,specialize", CASES, ids=[n + "".join(e) + ("-specialised" if s else "") for n, e, s in CASES])
def test_command_equals_the_reference_binary(tmp_path, name, extra, specialize):
    _need_ref()
    g = load_golden(name)
    d = str(tmp_path)
    _write_fastq(g, os.path.join(d, "in.fq"))
    args = str(g["cmdline"]).split()
    _ref(args + ["in.fq", "-o", "cpu"], d)
    # (the specialised case waits for one hiprtc compile of this architecture: README's times for it are 5-19 s)
    _hip(extra + args + ["in.fq", "-o", "gpu"], d, specialize=specialize, timeout=240 if specialize else 120)
    _same_files(d)
    assert _summary(d, "cpu") == _summary(d, "gpu")
    if name == "c5_big_b96_f_r_p":      # 1100 reads: more than one RTEST batch, all of them in the statistics
        assert _summary(d, "gpu")[0] == "1100\ttotal input reads"


# ---- G4 ----
@pytest.mark.parametrize("threads", [1, 3])
def test_ref_filter_through_the_command(tmp_path, threads):
    _need_ref()
    g = load_golden("artifacts_b_r")
    d = str(tmp_path)
    _write_fastq(g, os.path.join(d, "in.fq"))
    open(os.path.join(d, "art.fa"), "wb").write(bytes(g["art_fasta_text"]))
    args = str(g["cmdline"]).split() + ["-t", str(threads)]
    _ref(args + ["in.fq", "-o", "cpu"], d)
    _hip(args + ["in.fq", "-o", "gpu"], d)
    _same_files(d)
    cpu, gpu = _summary(d, "cpu"), _summary(d, "gpu")
    assert cpu == gpu
    arts = [l for l in gpu[gpu.index([l for l in gpu if l.endswith("\tmatch artifacts:")][0]) + 1:] if l]
    assert len(arts) == 3 and all(int(l.split("\t")[0]) > 0 for l in arts)


# ---- G5 ----
@pytest.mark.parametrize("devices", ["0", "0,0"])
def test_three_files_with_an_arch_file(tmp_path, devices):
    _need_ref()
    import bench
    d = str(tmp_path)
    bench.write_casava_files(d, 3000)
    g = load_golden("casava_index")
    with open(os.path.join(d, "arch.txt"), "w") as fh:
        fh.write("tagdust " + " ".join(str(g["cmdline"]).split()[2:]) + "\n")
        fh.write("tagdust -1 R:N\n")
    args = ["-seed", "42", "-arch", "arch.txt", "r1.fq", "r2.fq", "r3.fq"]
    _ref(args + ["-o", "cpu"], d)
    _hip(["--devices", devices] + args + ["-o", "gpu"], d, timeout=180)
    assert len(_same_files(d)) == 26
    assert _summary(d, "cpu") == _summary(d, "gpu")
    pick = lambda p: [l for l in _log(d, p) if l.startswith("Using:") or "Confidence" in l]
    assert pick("cpu") == pick("gpu") and len(pick("cpu")) == 6


# ---- G6 ----
def test_read_only_architecture(tmp_path):
    _need_ref()
    d = str(tmp_path)
    tags = os.path.join(REPO, "tests", "golden", "EDITTAG_6nt_ed_4_first4.txt")
    p = subprocess.run([os.path.join(RBIN, "simreads_rtest"), tags, "-seed", "42", "-sim_barnum", "0", "-sim_readlen", "50", "-sim_readlen_mod", "0",
                        "-sim_numseq", "3000", "-sim_endloss", "0", "-sim_random_frac", "0.1", "-sim_error_rate", "0.02", "-o", "c0.fq"],
                       cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    assert p.returncode == 0
    _ref(["-seed", "42", "-1", "R:N", "c0.fq", "-o", "cpu"], d)
    _hip(["-seed", "42", "-1", "R:N", "c0.fq", "-o", "gpu"], d)
    _same_files(d)
    assert _summary(d, "cpu") == _summary(d, "gpu")


# ---- G7 ----
def test_errors_exit_with_status_one(tmp_path):
    g = load_golden("c2_b4_r")
    d = str(tmp_path)
    _write_fastq(g, os.path.join(d, "r1.fq"))
    args = str(g["cmdline"]).split()
    text = open(os.path.join(d, "r1.fq"), "rb").read()
    # a truncated .gz as the second file: the decompressor's status ends the run, and it is named
    packed = gzip.compress(text)
    open(os.path.join(d, "r2.fq.gz"), "wb").write(packed[:len(packed) // 2])
    err = _hip(args + ["r1.fq", "r2.fq.gz", "-o", "trunc"], d, rc=1)
    assert "zcat" in err and not _outputs(d, "trunc")
    # input files with different record counts: the controller's message (barcode_hmm.c:262)
    lines = text.split(b"\n")
    open(os.path.join(d, "short.fq"), "wb").write(b"\n".join(lines[:4 * 100]) + b"\n")
    err = _hip(args + ["r1.fq", "short.fq", "-o", "count"], d, rc=1)
    assert "Input File:r1.fq and short.fq differ in number of entries." in err
    assert "differ in number of entries" in open(os.path.join(d, "count_logfile.txt")).read()
    # existing outputs: nothing is touched
    first = args[args.index("-1") + 1].split(":")[1].split(",")[0]
    keep = os.path.join(d, "have_BC_%s.fq" % first)
    open(keep, "w").write("keep me\n")
    err = _hip(args + ["r1.fq", "-o", "have"], d, rc=1)
    assert "already exists" in err and open(keep).read() == "keep me\n"
    assert sorted(_outputs(d, "have")) == ["_BC_%s.fq" % first]
