"""Labelled cases of the two sign/dss engine calls, shared by the CPU test (tests/test_dss_host.py: the lane programs
compiled for the host) and the GPU test (tests/test_gpu_dss.py).  A World is one roster, one long-term key and a few
sessions with their honest partial signatures; a case is one partial signature handed to kyb_ed25519_dss_check with the
status its label promises by construction -- the oracle (tests/_dss_oracle.py) must agree before any engine is asked."""
import hashlib

from oracle import ed25519 as O
from tests import _dkg_cases as DC
from tests import _dss_oracle as D
from tests import _vss_oracle as VO

L = O.L
OK, BAD_POINT, NONCANONICAL, SMALL_ORDER = 0, 1, 5, 6
INDEX, SIG, SESSION, PARTIAL = D.ST_DSS_INDEX, D.ST_DSS_SIG, D.ST_DSS_SESSION, D.ST_DSS_PARTIAL
# the padding edges of 64 + len under SHA-512 (one block holds 111 bytes of data: 47 of message), and the empty message
MSG_LENGTHS = (0, 47, 48, 63, 64, 111, 112)
HONEST = 7  # participants 0 .. 6 hold keys and shares; 7, 8, 9 are the special encodings; 10 is honest again
SPECIAL = {7: DC.ORDER8, 8: DC.UNDECODABLE, 9: DC.NONCANONICAL}
NP = 11


def _scalar(tag: bytes) -> int:
    return DC.scalar(b"dss cases " + tag)


class World:
    """np = 11 participants, a long-term polynomial of tl coefficients, one random polynomial of tr per session"""

    def __init__(self, name: str, tl: int, tr: int, lengths, torsion: bool = False, bad_session=None):
        tag = name.encode()
        self.name, self.tl, self.tr, self.ns, self.torsion = name, tl, tr, len(lengths), torsion
        self.privs = [_scalar(tag + b" priv %d" % i) for i in range(NP)]
        self.participants = [SPECIAL.get(i) or O.mul_base(DC.le(self.privs[i])) for i in range(NP)]
        self.long_coeffs = [_scalar(tag + b" long %d" % k) for k in range(tl)]
        self.rand_coeffs = [[_scalar(tag + b" rand %d %d" % (b, k)) for k in range(tr)] for b in range(self.ns)]
        self.long_commits = [O.mul_base(DC.le(c)) for c in self.long_coeffs]
        self.rand_commits = [[O.mul_base(DC.le(c)) for c in row] for row in self.rand_coeffs]
        if torsion:  # commitments with a torsion component: the fold must stay exact off the prime-order subgroup
            t8 = O.decode(DC.ORDER8)
            self.long_commits[-1] = O.encode(O.add(O.decode(self.long_commits[-1]), t8))
            self.rand_commits[0][0] = O.encode(O.add(O.decode(self.rand_commits[0][0]), O.mul_int(3, t8)))
        if bad_session is not None:
            self.rand_commits[bad_session][tr - 1] = DC.UNDECODABLE
        self.msgs = [hashlib.shake_128(tag + b" msg %d" % b).digest(n) for b, n in enumerate(lengths)]
        self.sids = [D.session_id(self.long_commits, rc) for rc in self.rand_commits]
        self.h = [D.hash_sig(rc[0], self.long_commits[0], m) for rc, m in zip(self.rand_commits, self.msgs)]

    def alpha(self, i: int) -> int:
        return DC.eval_scalar(self.long_coeffs, i)

    def beta(self, b: int, i: int) -> int:
        return DC.eval_scalar(self.rand_coeffs[b], i)

    def nonce(self, b: int, i: int) -> bytes:
        return DC.le(_scalar(self.name.encode() + b" nonce %d %d" % (b, i)))

    def honest(self, b: int, i: int):
        """(V, sid, sig) participant i issues in session b"""
        return D.partial(DC.le(self.privs[i]), i, DC.le(self.alpha(i)), DC.le(self.beta(b, i)), self.nonce(b, i), self.long_commits,
                         self.rand_commits[b], self.msgs[b])

    def signed(self, b: int, i: int, v: bytes, sid: bytes, key: int = None):
        """a partial with these V and session id, signed by participant i's key (or another) under its usual nonce"""
        key = self.privs[i] if key is None else key
        return v, sid, VO.schnorr_sign(self.nonce(b, i), DC.le(key), D.partial_hash(v, i, sid))

    def expected(self, b: int, i: int, v: bytes, sid: bytes, sig: bytes):
        return D.check(self.participants, self.long_commits, self.rand_commits[b], self.msgs[b], i, v, sid, sig)

    def sess_status(self):
        return [BAD_POINT if D.folded(self.long_commits, rc, m) is None else OK for rc, m in zip(self.rand_commits, self.msgs)]


def worlds():
    return [
        World("main", 4, 4, MSG_LENGTHS[:3]),
        World("short long-term", 2, 5, MSG_LENGTHS[3:5]),          # tl + tr odd: the session id ends inside a block
        World("short random", 5, 2, MSG_LENGTHS[5:7]),
        World("one each", 1, 1, (5,)),                             # tl + tr = 2: the session id ends ON a block
        World("torsion", 3, 3, (9, 0), torsion=True),
        World("bad session", 3, 3, (1, 2, 3), bad_session=1),      # an undecodable commitment between two good sessions
    ]


def _flip(b: bytes, pos: int = 0) -> bytes:
    return b[:pos] + bytes([b[pos] ^ 1]) + b[pos + 1:]


def cases(w: World):
    """[(label, session, index, V, sid, sig, status by construction)]"""
    out = []

    def add(label, b, i, part, want):
        out.append((label, b, i) + tuple(part) + (want,))

    bad = set(b for b, s in enumerate(w.sess_status()) if s)

    def honest_want(b, i):
        """an honest share's verdict: V B lies in the prime-order subgroup, so in the torsion world it holds only where
        the right side's torsion component -- 3 t8 from R_0 of session 0, h x^(tl - 1) t8 from the last A -- cancels"""
        if b in bad:
            return BAD_POINT
        if w.torsion and ((3 if b == 0 else 0) + w.h[b] * (i + 1) ** (w.tl - 1)) % 8:
            return PARTIAL
        return OK

    for b in range(w.ns):
        for i in (0, 3, 6, NP - 1):  # idx = np - 1 is the last honest key
            add("honest", b, i, w.honest(b, i), honest_want(b, i))
    b = 0 if 0 not in bad else 2
    v, sid, sig = w.honest(b, 2)
    other_sid = _flip(sid, 31)
    vi = int.from_bytes(v, "little")
    # each status alone
    add("index = np", b, NP, (v, sid, sig), INDEX)
    add("index = 2^32 - 1", b, 2**32 - 1, (v, sid, sig), INDEX)
    add("S + 1", b, 2, (v, sid, sig[:32] + DC.le((int.from_bytes(sig[32:], "little") + 1) % L)), SIG)
    add("signed by another key", b, 2, w.signed(b, 2, v, sid, key=w.privs[3]), SIG)
    add("R no point", b, 2, (v, sid, DC.UNDECODABLE + sig[32:]), SIG)  # R's decoding is the equation's (status of verify: 0)
    add("wrong session id", b, 2, w.signed(b, 2, v, other_sid), SESSION)
    add("V + 1", b, 2, w.signed(b, 2, DC.le((vi + 1) % L), sid), PARTIAL)
    if max(w.tl, w.tr) > 1:  # (constant polynomials give every signer the same share)
        add("another signer's V", b, 2, w.signed(b, 2, w.honest(b, 4)[0], sid), PARTIAL)
    # each adjacent pair of the precedence
    add("index = np, bad signature", b, NP, (v, sid, _flip(sig, 40)), INDEX)
    add("bad signature, wrong session id", b, 2, (v, other_sid, sig), SIG)  # (the hash covers the id: the signature fails)
    add("S >= l, wrong session id", b, 2, (v, other_sid, sig[:32] + DC.le(L)), NONCANONICAL)
    add("wrong session id, V + 1", b, 2, w.signed(b, 2, DC.le((vi + 1) % L), other_sid), SESSION)
    # V's range: the 32 bytes are never reduced
    add("V = 0", b, 2, w.signed(b, 2, bytes(32), sid), PARTIAL)
    add("V + l", b, 2, w.signed(b, 2, DC.le(vi + L), sid), honest_want(b, 2))  # the same scalar mod l, the same point
    add("V + 2^255", b, 2, w.signed(b, 2, DC.le(vi + 2**255), sid), PARTIAL)
    add("V all ones", b, 2, w.signed(b, 2, b"\xff" * 32, sid), PARTIAL)
    # the signature's byte-level checks, as kyb_ed25519_verify reports them
    add("S = l", b, 2, (v, sid, sig[:32] + DC.le(L)), NONCANONICAL)
    add("S = 2^256 - 1", b, 2, (v, sid, sig[:32] + b"\xff" * 32), NONCANONICAL)
    add("R of small order", b, 2, (v, sid, DC.ORDER8 + sig[32:]), SMALL_ORDER)
    add("R not canonical", b, 2, (v, sid, DC.NONCANONICAL + sig[32:]), NONCANONICAL)
    add("key of small order", b, 7, (v, sid, sig), SMALL_ORDER)
    add("key that does not decode", b, 8, (v, sid, sig), BAD_POINT)
    add("key not canonical", b, 9, (v, sid, sig), NONCANONICAL)
    if bad:
        s = min(bad)
        hv, hsid, _ = w.honest(s, 2)
        add("bad session: wrong id first", s, 2, w.signed(s, 2, hv, _flip(hsid)), SESSION)
        add("bad session: bad signature first", s, 2, (hv, hsid, _flip(w.honest(s, 2)[2], 33)), SIG)
    return out
