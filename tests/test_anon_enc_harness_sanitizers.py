"""One AddressSanitizer + UndefinedBehaviorSanitizer pass over ed25519_anonenc.cuh's host build: tests/anon_enc_harness.cpp
compiled as a stand-alone program (-DANON_ENC_HARNESS_MAIN) with -fsanitize=address,undefined and run on the CPU.  Its main
runs sign/anon's seal and open over exactly sized heap buffers: every message length of the keystream's and the MAC's
block edges, an odd byte offset in front of an empty first element, the last message and the last ciphertext ending
their buffers, ciphertexts cut at every boundary of Decrypt's length checks (each in a buffer it ends), both values of
the key stride and of the private-key stride.  The byte-wise message and ciphertext accesses, the 48 + 32 ring bytes a
ciphertext is longer than its message and the per-lane slab slots are where an overrun would later fault a GPU, and here
a byte read or written past a buffer is the sanitizer's to report.
(shift-base is off as in tests/test_host_harness_sanitizers.py: the signed-limb field code shifts negative values left.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "_build", "anon_enc_sanitize_main")


def test_anon_enc_headers_are_clean_under_asan_and_ubsan():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DANON_ENC_HARNESS_MAIN", "-fsanitize=address,undefined",
                           "-fno-sanitize=shift-base", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", EXE,
                           os.path.join(ROOT, "tests", "anon_enc_harness.cpp")])
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])
    assert r.stdout.strip() == "ok"
