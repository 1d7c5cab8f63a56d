"""One AddressSanitizer + UndefinedBehaviorSanitizer pass over ed25519_eddsa.cuh's host build: tests/eddsa_harness.cpp
compiled as a stand-alone program (-DEDDSA_HARNESS_MAIN) with -fsanitize=address,undefined and run on the CPU.  Its main
expands keys and signs over exactly sized heap buffers: message lengths on either side of every block and padding
boundary of SHA-512(prefix || msg) and SHA-512(R || A || msg), an odd byte offset in front of an empty first message,
the last message ending its buffer, one key for the batch and one per element.  The byte-wise message reads of the two
hashes are where an overrun would later fault a GPU, and here a byte read past a buffer is the sanitizer's to report.
Nothing is loaded into Python under a sanitizer.
(shift-base is off as in tests/test_host_harness_sanitizers.py: the signed-limb field code shifts negative values left.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_build", "eddsa_sanitize_main")


def test_eddsa_headers_are_clean_under_asan_and_ubsan():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DEDDSA_HARNESS_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize=shift-base", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", EXE,
                           os.path.join(ROOT, "tests", "eddsa_harness.cpp")])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
