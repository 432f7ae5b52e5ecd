"""DevScratch's sticky error (gk_internal.h) and the `.bin` framing helpers (gk_binstream.h), checked on the host: a program of
its own (tests/host/scratch_check.hip) with a counting, failing pool of malloc / free, built with AddressSanitizer and
UndefinedBehaviorSanitizer and run.  No device, nothing loaded into Python.  The failure paths of the entry points that use these
helpers are not reachable from a GPU test (no test makes a device allocation fail): this program is where they are covered.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "scratch_check.hip")


def test_scratch_and_binstream_under_sanitizers(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "scratch_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                            SRC, "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr[-4000:]
    # where a device is present the first runtime call initialises the HIP / HSA runtime, whose own allocations live until the
    # process ends: not this program's leaks (its pool counts its own frees)
    supp = tmp_path / "lsan.supp"
    supp.write_text("leak:libhsa-runtime64\nleak:libamdhip64\nleak:libhsakmt\nleak:libdrm\n")
    env = dict(os.environ)
    env["UBSAN_OPTIONS"] = "print_stacktrace=1"
    env["LSAN_OPTIONS"] = f"suppressions={supp}:print_suppressions=0"
    run = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    report = run.stdout + run.stderr
    assert run.returncode == 0, report[-4000:]
    assert "runtime error:" not in report and "AddressSanitizer" not in report and "LeakSanitizer" not in report, report[-4000:]
    assert "scratch_check ok" in run.stdout
