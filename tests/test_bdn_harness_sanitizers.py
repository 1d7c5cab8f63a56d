"""One AddressSanitizer + UndefinedBehaviorSanitizer pass over blake2xs.cuh's and bdn.cuh's host build:
tests/bdn_harness.cpp compiled as a stand-alone program (-DBDN_HARNESS_MAIN) with -fsanitize=address,undefined and run on
the CPU.  Its main runs NewMask's lanes and the masked sums for all six (suite, group) pairs over rosters at every group
edge of both table widths, every slice count from 1 to the number of groups, masks of both polarities with stray bits at
the exact stride and at an odd one (the last mask ends its buffer), a roster with a rejected key, and hashes at the
block edges, all in exactly sized heap buffers: the table slots picked by the mask's digits, the partial last group, the
slices' ranges, the in-place fold and the byte-wise mask and message reads are where an overrun would later fault a GPU,
and here a byte read or written past a buffer is the sanitizer's to report.  Nothing is loaded into python.
(shift-base is off as in tests/test_host_harness_sanitizers.py.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_build", "bdn_sanitize_main")


def test_bdn_headers_are_clean_under_asan_and_ubsan():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DBDN_HARNESS_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize=shift-base", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", EXE,
                           os.path.join(ROOT, "tests", "bdn_harness.cpp")])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=900,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
