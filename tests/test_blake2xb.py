"""util/blake2xb.py, the host BLAKE2Xb behind Scalar.Pick, against the two outputs the reference prints and against
hashlib where hashlib can build the node -- no GPU."""
import hashlib

from kyber_amd.group import edwards25519 as ed
from kyber_amd.util import blake2xb as X
from oracle import ed25519 as O


def test_diffie_hellman_example_pins_the_unkeyed_stream_and_the_rejection_loop():
    """examples/dh_test.go:19-48: blake2xb.New(nil), two picks, the shared secret a*b*B"""
    rng = X.New(None)
    a, da = X.pick_int(rng.Read)
    b, db = X.pick_int(rng.Read)
    assert (da, db) == (3, 3)  # both picks reject twice: the loop is pinned, not only the first draw
    assert O.encode(O.mul_int(a * b % O.L, O.B)).hex() == "80ea238cacfdab279626970bba18c69083c7751865dec4c6434bff4351282847"


def test_rep2_example_pins_the_keyed_stream():
    """proof/proof_test.go:89-117: the stream keyed "example"; the proof's first 32 bytes are v*B of the second pick"""
    rng = X.New(b"example")
    X.pick_int(rng.Read)
    v, _ = X.pick_int(rng.Read)
    assert O.encode(O.mul_int(v, O.B)).hex() == "e9a2daf49d7ce22535be0a15789ceacaa71e6ed626c340ed0d3d71d4a9ef553b"


def test_root_node_matches_hashlib_keyed_and_unkeyed():
    for key in (b"", b"k" * 32, bytes(range(64)), b"example"):
        for msg in (b"", b"abc", bytes(range(200)), bytes(300)):
            want = hashlib.blake2b(msg, digest_size=64, key=key, fanout=1, depth=1, node_offset=0xFFFFFFFF << 32).digest()
            assert X.root_hash(key, msg) == want
    assert X.blake2b_param(b"abc", X.param_block(64, 0, 1, 1, 0, 0, 0, 0, 0)) == hashlib.blake2b(b"abc").digest()


def test_xof_interface_long_seeds_clone_reseed_and_keystream():
    long_seed = bytes(range(100))  # the first 64 bytes key the hash, the rest is written (blake.go:20-36)
    a = X.New(long_seed)
    assert a.Read(96) == X.output_node(X.root_hash(long_seed[:64], long_seed[64:]), 0) + X.output_node(X.root_hash(long_seed[:64], long_seed[64:]), 1)[:32]
    b = X.New(long_seed)
    assert b.Read(10) + b.Read(86) == X.New(long_seed).Read(96)  # reads continue inside a node
    c = b.Clone()
    assert c.Read(50) == b.Read(50)
    d = X.New(b"seed")
    key = X.New(b"seed").Read(128)
    d.Reseed()
    assert d.Read(40) == X.New(key).Read(40)
    e = X.New(b"ks")
    assert e.XORKeyStream(bytes(33)) == X.New(b"ks").Read(33)
    try:
        e.Write(b"x")
    except ValueError:
        pass
    else:
        raise AssertionError("a write after a read must fail, as in the reference")


def test_scalar_pick_takes_the_xof_as_its_stream():
    assert ed.Scalar().Pick(X.New(b"example")).v == X.pick(X.New(b"example").Read)
    assert len(ed.Scalar().Pick(lambda n: bytes(n)).v) == 32  # a plain callable still works
