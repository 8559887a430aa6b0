"""The plain C++ host units of the two counts (tagdust_amd/csrc/td_census_host.cpp, td_molecules_host.cpp), of the batch geometry
(td_batch_plan.cpp) and of the model path (td_model.cpp, td_model_flat.cpp, td_spec_plan.cpp, td_spec_bounds.cpp) build with the host
compiler alone -- no hipcc, no HIP header, no HIP runtime -- and the stand-alone programs
over them (tools/*_host_check.cpp, the ones tools/host_checks.sh runs under the sanitizers) agree with their restatements.  No GPU,
no sanitizer here."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

CSRC = os.path.join(REPO, "tagdust_amd", "csrc")
# the program, and what it links beside the two host units of the counts (td_fingerprint_text is td_fastq.cpp's); the batch plan's
# links its own unit alone, the worker pool's (td_workers.h) nothing at all, the model path's its four units
COUNT_UNITS = ("td_census_host.cpp", "td_molecules_host.cpp")
WITHOUT_COUNT_UNITS = ("batch_plan_host_check", "workers_host_check", "model_host_check")
PROGRAMS = [("census_host_check", []), ("molecules_host_check", ["td_fastq.cpp"]), ("dedup_host_check", []), ("collapse_host_check", []),
            ("dedup_collapsed_host_check", []), ("mate_host_check", []), ("batch_plan_host_check", ["td_batch_plan.cpp"]), ("workers_host_check", []),
            ("model_host_check", ["td_model.cpp", "td_model_flat.cpp", "td_spec_plan.cpp", "td_spec_bounds.cpp"]),
            ("run_host_check", ["td_run_opts.cpp", "td_run_plan.cpp", "td_run_report.cpp", "td_model.cpp", "td_model_flat.cpp", "td_fastq.cpp", "td_samples_host.cpp"])]


def host_compiler():
    """$CXX, else g++, else the clang++ beside hipcc; with what makes it read its inputs as plain C++"""
    if os.environ.get("CXX"):
        return os.environ["CXX"].split(), []
    if shutil.which("g++"):
        return ["g++"], []
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for d in (os.path.dirname(os.path.realpath(hipcc)), "/opt/rocm/lib/llvm/bin", "/opt/rocm/llvm/bin"):
        if os.path.exists(os.path.join(d, "clang++")):
            return [os.path.join(d, "clang++")], ["-x", "c++"]
    return None, None


def run(cmd):
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert done.returncode == 0, " ".join(cmd) + "\n" + done.stdout
    return done.stdout


def compiled(cxx, as_cxx, source, out_dir):
    obj = os.path.join(out_dir, os.path.basename(source) + ".o")
    run(cxx + ["-std=c++17", "-O1", "-Wall"] + as_cxx + ["-c", source, "-o", obj])
    return obj


@pytest.fixture(scope="module")
def host_objects(tmp_path_factory):
    """the two host units of the counts, compiled once for the programs over them"""
    cxx, as_cxx = host_compiler()
    assert cxx, "no host C++ compiler: set CXX, or install g++"
    d = str(tmp_path_factory.mktemp("host_units"))
    return [compiled(cxx, as_cxx, os.path.join(CSRC, u), d) for u in COUNT_UNITS]


@pytest.mark.parametrize("name,extra", PROGRAMS, ids=[p[0] for p in PROGRAMS])
def test_the_host_units_build_and_agree_without_hip(tmp_path, host_objects, name, extra):
    cxx, as_cxx = host_compiler()
    d = str(tmp_path)
    objs = [compiled(cxx, as_cxx, s, d) for s in [os.path.join(CSRC, e) for e in extra] + [os.path.join(REPO, "tools", name + ".cpp")]]
    exe = os.path.join(d, name)
    run(cxx + ([] if name in WITHOUT_COUNT_UNITS else host_objects) + objs + ["-o", exe, "-lpthread"])
    assert (name + ": ok") in run([exe]).splitlines()


def test_the_sanitizer_script_builds_and_runs_every_program():
    script = open(os.path.join(REPO, "tools", "host_checks.sh")).read()
    for name, _ in PROGRAMS:
        assert ("tools/%s.cpp -o $OUT/%s" % (name, name)) in script, name
        assert ("\n$OUT/%s &&" % name) in script, name
