"""The host entry points of the plant analysis (csrc/abi_analysis.cpp) under
AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program
(tests/cpp/analysis_asan.cpp, analysis_asan.mk).  No device is needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_analysis_entry_points_under_sanitizers():
    """cmpc_plant_equilibrium_host, cmpc_plant_target_host, cmpc_plant_gains_host,
    cmpc_plant_modes_host and cmpc_eig_host on B = 3 scenarios at both plants'
    default operating point, on heap arrays of exactly the documented sizes,
    then cmpc_target_check, cmpc_gain_check and the host forms with one bad
    argument of every kind: no memory or UB error, every refusal with its
    message."""
    here = os.path.join(ROOT, "tests", "cpp")
    subprocess.check_call(["make", "-s", "-C", here, "-f", "analysis_asan.mk", "analysis_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([os.path.join(here, "analysis_asan")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("analysis_asan ok"), r.stdout
    assert "runtime error" not in r.stderr, r.stderr[-2000:]
