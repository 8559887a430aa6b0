"""tools/mate_host_check.cpp, the stand-alone program over the *_mated host functions of tagdust_amd/csrc/td_molecules_host.cpp
that tools/host_checks.sh runs under the sanitizers, builds with the host compiler alone and agrees with its restatement.  No GPU,
no sanitizer here."""
import os

from conftest import REPO
from test_host_units import COUNT_UNITS, CSRC, compiled, host_compiler, run


def test_the_mate_host_check_builds_and_agrees_without_hip(tmp_path):
    cxx, as_cxx = host_compiler()
    assert cxx, "no host C++ compiler: set CXX, or install g++"
    d = str(tmp_path)
    objs = [compiled(cxx, as_cxx, s, d) for s in [os.path.join(CSRC, u) for u in COUNT_UNITS] + [os.path.join(REPO, "tools", "mate_host_check.cpp")]]
    exe = os.path.join(d, "mate_host_check")
    run(cxx + objs + ["-o", exe])
    assert "mate_host_check: ok" in run([exe]).splitlines()
    script = open(os.path.join(REPO, "tools", "host_checks.sh")).read()
    assert "tools/mate_host_check.cpp -o $OUT/mate_host_check" in script and "$OUT/mate_host_check &&" in script
