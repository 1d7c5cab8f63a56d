"""One AddressSanitizer + UndefinedBehaviorSanitizer pass over ed25519_cosi.cuh's host build: tests/cosi_harness.cpp
compiled as a stand-alone program (-DCOSI_HARNESS_MAIN) with -fsanitize=address,undefined and run on the CPU.  Its main
runs the aggregation and the verification over rosters at every group edge of both table widths, masks of both
polarities with stray bits at the exact stride and at an odd one (the last mask ends its buffer), and messages at the
padding edges, all in exactly sized heap buffers: the table slots picked by the mask's digits, the partial last group
and the byte-wise mask and message reads are where an overrun would later fault a GPU, and here a byte read or written
past a buffer is the sanitizer's to report.
(shift-base is off as in tests/test_host_harness_sanitizers.py: the signed-limb field code shifts negative values left.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_build", "cosi_sanitize_main")


def test_cosi_headers_are_clean_under_asan_and_ubsan():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DCOSI_HARNESS_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize=shift-base", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", EXE,
                           os.path.join(ROOT, "tests", "cosi_harness.cpp")])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
