"""One AddressSanitizer + UndefinedBehaviorSanitizer pass over ed25519_proof.cuh's host build: tests/proof_harness.cpp
compiled as a stand-alone program (-DPROOF_HARNESS_MAIN) with -fsanitize=address,undefined and run on the CPU.  Its main
runs the linear combination for every (ko, ks) and both flag values and the challenge at every name and data length of
the tests, all in exactly sized heap buffers: the interleaved digit columns, the table slots picked by address and the
partial-block byte loops of the hash are where an overrun would later fault a GPU, and here a byte read or written past
a buffer is the sanitizer's to report.
(shift-base is off as in tests/test_host_harness_sanitizers.py: the signed-limb field code shifts negative values left.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_build", "proof_sanitize_main")


def test_proof_headers_are_clean_under_asan_and_ubsan():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DPROOF_HARNESS_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize=shift-base", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", EXE,
                           os.path.join(ROOT, "tests", "proof_harness.cpp")])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
