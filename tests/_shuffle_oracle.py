"""shuffle/ (pair.go, simple.go, sequences.go) and proof/hash.go restated sequentially in Python, element by element, on
oracle/ed25519.py and the pure-Python BLAKE2Xb (no GPU, no engine): the checker of kyb_ed25519_theta_check and of
kyber_amd/shuffle + kyber_amd/proof/hash.py, never the thing shipped, and written from the reference's text without
looking at the batched implementation.

Points and scalars are 32 wire bytes; G or H None is the standard base (Point.Mul(s, nil), point.go:243).  Scalars the
protocol computes are Python integers modulo l; scalars read off the wire are kept as their bytes and multiply as such
(UnmarshalBinary copies them unreduced, scalar.go:226-232).  The wire layout is what suite.Write produces, read off the
call sites: a struct is its fields in order, a slice its elements, no length prefixes.  Errors are ShuffleError with the
reference's message.

The reference's own shuffle tests print no bytes and there is no Go toolchain to run them, so no transcript of the Go
program is pinned anywhere: this restatement is the yardstick."""
from kyber_amd.util import blake2xb
from oracle import ed25519 as O

L = O.L
NULL = O.encode(O.IDENTITY)
ERR_POINT = "invalid Ed25519 curve point"  # point.go:67
ERR_SIMPLE, ERR_PAIR, ERR_MALFORMED = "incorrect SimpleShuffleProof", "invalid PairShuffleProof", "malformed SimpleShuffleProof"
ERR_SHORT = "unexpected EOF"  # io.ReadFull on the proof's buffer


class ShuffleError(Exception):
    pass


def le(b) -> int:
    return int.from_bytes(bytes(b), "little")


def sc(v: int) -> bytes:
    return (v % L).to_bytes(32, "little")


def pmul(s: bytes, P) -> bytes:
    """Point.Mul(s, P) on wire bytes; P None: the base-point multiplication"""
    out = O.mul_base(bytes(s)) if P is None else O.mul(bytes(s), bytes(P))
    assert out is not None
    return out


def _pmul_each(scalars, points):
    return [pmul(s, P) for s, P in zip(scalars, points)]


# The products of one loop of a verifier, element by element.  many_products() swaps in a batched multiplication (the C
# restatement of the same oracle, tests/_oracle_c.py) for the one test whose k makes 41 000 big-integer products too slow;
# additions, comparisons and the order of the checks stay as they are.
pmul_many = _pmul_each


class many_products:
    def __init__(self, fn):
        self.fn = fn

    def __enter__(self):
        global pmul_many
        pmul_many = self.fn

    def __exit__(self, *exc):
        global pmul_many
        pmul_many = _pmul_each


_DECODED = {}  # encoding -> point, for the encodings this module has itself produced or already decoded


def _dec(e):
    e = bytes(e)
    if e not in _DECODED:
        if len(_DECODED) > 200000:
            _DECODED.clear()
        _DECODED[e] = O.decode(e)
    return _DECODED[e]


def _enc(pt) -> bytes:
    e = O.encode(pt)
    _DECODED.setdefault(e, pt)
    return e


def padd(a: bytes, b: bytes) -> bytes:
    return _enc(O.add(_dec(a), _dec(b)))


def psub(a: bytes, b: bytes) -> bytes:
    return _enc(O.add(_dec(a), O.neg(_dec(b))))


def pequal(a: bytes, b: bytes) -> bool:
    """Point.Equal: on re-encodings (point.go:81-96)"""
    return O.encode(_dec(a)) == O.encode(_dec(b))


def pick(stream) -> int:
    return blake2xb.pick_int(stream)[0]


def inv(v: int) -> int:
    return pow(v % L, L - 2, L)  # scalar.go:157-175: an exponentiation, so Inv(0) = 0


# ---------------------------------------------------------------------------------------------------- proof/hash.go
class HashProver:
    """hash.go:12-89.  random_stream(n) -> n bytes: suite.RandomStream()"""

    def __init__(self, protocol: bytes, random_stream):
        self.pubrand = blake2xb.New(protocol)
        self.prirand = random_stream
        self.msg = b""
        self.proof = b""

    def Put(self, *fields):
        for f in fields:
            self.msg += bytes(f) if isinstance(f, (bytes, bytearray)) else b"".join(bytes(e) for e in f)

    def _consume(self):
        if self.msg:
            self.pubrand.Reseed()
            self.pubrand.Write(self.msg)
            self.proof += self.msg
            self.msg = b""

    def PubRand(self, n: int):
        self._consume()
        return [pick(self.pubrand.Read) for _ in range(n)]

    def PriRand(self, n: int):
        return [pick(self.prirand) for _ in range(n)]

    def Proof(self) -> bytes:
        self._consume()
        return self.proof


class HashVerifier:
    """hash.go:91-142"""

    def __init__(self, protocol: bytes, proof: bytes):
        self.buf = bytes(proof)
        self.read = 0  # bytes the Gets have taken
        self.stirred = 0  # bytes already written into the public randomness
        self.pubrand = blake2xb.New(protocol)

    def Get(self, kinds: str):
        """one element per character of kinds: 'P' a point (must decode), 'S' a scalar (copied raw)"""
        out = []
        for kind in kinds:
            if len(self.buf) - self.read < 32:
                raise ShuffleError(ERR_SHORT)
            e = self.buf[self.read:self.read + 32]
            self.read += 32
            if kind == "P" and O.decode(e) is None:
                raise ShuffleError(ERR_POINT)
            out.append(e)
        return out

    def PubRand(self, n: int):
        if self.read > self.stirred:
            self.pubrand.Reseed()
            self.pubrand.Write(self.buf[self.stirred:self.read])
            self.stirred = self.read
        return [pick(self.pubrand.Read) for _ in range(n)]


def hash_prove(protocol: bytes, prover, random_stream) -> bytes:
    ctx = HashProver(protocol, random_stream)
    prover(ctx)
    return ctx.Proof()


def hash_verify(protocol: bytes, verifier, proof: bytes):
    """None, or the error's message"""
    try:
        verifier(HashVerifier(protocol, proof))
    except ShuffleError as e:
        return str(e)
    return None


# -------------------------------------------------------------------------------------------------------- simple.go
def thenc(G, a, b, c, d) -> bytes:
    ab = a * b % L if a is not None else 0
    cd = (c * d % L if d is not None else c) if c is not None else 0
    return pmul(sc(ab - cd), G)


def simple_prove(G, gamma: int, x, y, ctx):
    k = len(x)
    assert k > 1 and k == len(y)
    ctx.Put([pmul(sc(v), G) for v in x], [pmul(sc(v), G) for v in y])
    t = ctx.PubRand(1)[0]
    gamma_t = gamma * t % L
    xhat = [(v - t) % L for v in x]
    yhat = [(v - gamma_t) % L for v in y]
    thlen = 2 * k - 1
    theta = ctx.PriRand(thlen)
    Theta = [thenc(G, None, None, theta[0], yhat[0])]
    for i in range(1, k):
        Theta.append(thenc(G, theta[i - 1], xhat[i], theta[i], yhat[i]))
    for i in range(k, thlen):
        Theta.append(thenc(G, theta[i - 1], gamma, theta[i], None))
    Theta.append(thenc(G, theta[thlen - 1], gamma, None, None))
    ctx.Put(Theta)
    c = ctx.PubRand(1)[0]
    alpha = [0] * thlen
    runprod = c
    for i in range(k):
        runprod = runprod * xhat[i] % L
        runprod = runprod * inv(yhat[i]) % L
        alpha[i] = (theta[i] + runprod) % L
    gammainv = inv(gamma)
    rungamma = c
    for i in range(1, k):
        rungamma = rungamma * gammainv % L
        alpha[thlen - i] = (theta[thlen - i] + rungamma) % L
    ctx.Put([sc(v) for v in alpha])


def simple_verify(G, Gamma: bytes, k: int, ctx):
    thlen = 2 * k - 1
    if k <= 1:
        raise ShuffleError(ERR_MALFORMED)
    X, Y = (lambda v: (v[:k], v[k:]))(ctx.Get("P" * (2 * k)))
    t = ctx.PubRand(1)[0]
    Theta = ctx.Get("P" * (thlen + 1))
    c = sc(ctx.PubRand(1)[0])
    alpha = ctx.Get("S" * thlen)
    negt = sc(-t)
    U, W = pmul(negt, G), pmul(negt, Gamma)
    Xhat = [padd(X[i], U) for i in range(k)]
    Yhat = [padd(Y[i], W) for i in range(k)]
    # thver(A, B, T, a, b) for the 2k rows: (Xhat_i, Yhat_i) with (c | alpha_{i-1}, alpha_i), then (Gamma, G) with
    # (alpha_{i-1}, alpha_i | c)
    As, Bs = Xhat + [Gamma] * k, Yhat + [G] * k
    a_s = [c] + alpha[:thlen]
    b_s = alpha[:thlen] + [c]
    P = pmul_many(a_s, As)
    Q = pmul_many([sc(-le(b)) for b in b_s], Bs)
    good = True
    for i in range(thlen + 1):
        good = good and pequal(padd(P[i], Q[i]), Theta[i])
    if not good:
        raise ShuffleError(ERR_SIMPLE)


# ---------------------------------------------------------------------------------------------------------- pair.go
def pair_prove(pi, G, H, beta, X, Y, ctx):
    k = len(pi)
    assert k > 1 and k == len(beta) == len(X) == len(Y)
    piinv = [0] * k
    for i in range(k):
        piinv[pi[i]] = i
    u, w, a = ctx.PriRand(k), ctx.PriRand(k), ctx.PriRand(k)
    tau0, nu, gamma = ctx.PriRand(1)[0], ctx.PriRand(1)[0], ctx.PriRand(1)[0]
    Gamma = pmul(sc(gamma), G)
    wbetasum = tau0
    Lambda1, Lambda2 = NULL, NULL
    A, C, U, W = [], [], [], []
    for i in range(k):
        A.append(pmul(sc(a[i]), G))
        C.append(pmul(sc(gamma * a[pi[i]]), G))
        U.append(pmul(sc(u[i]), G))
        W.append(pmul(sc(gamma * w[i]), G))
        wbetasum = (wbetasum + w[i] * beta[pi[i]]) % L
        wu = sc(w[piinv[i]] - u[i])
        Lambda1 = padd(Lambda1, pmul(wu, X[i]))
        Lambda2 = padd(Lambda2, pmul(wu, Y[i]))
    Lambda1 = padd(Lambda1, pmul(sc(wbetasum), G))
    Lambda2 = padd(Lambda2, pmul(sc(wbetasum), H))
    ctx.Put(Gamma, A, C, U, W, Lambda1, Lambda2)
    rho = ctx.PubRand(k)
    b = [(rho[i] - u[i]) % L for i in range(k)]
    d = [gamma * b[pi[i]] % L for i in range(k)]
    ctx.Put([pmul(sc(v), G) for v in d])
    lam = ctx.PubRand(1)[0]
    r = [(a[i] + lam * b[i]) % L for i in range(k)]
    s = [gamma * r[pi[i]] % L for i in range(k)]
    tau = -tau0 % L
    sigma = []
    for i in range(k):
        sigma.append((w[i] + b[pi[i]]) % L)
        tau = (tau + b[i] * beta[i]) % L
    ctx.Put([sc(v) for v in sigma], sc(tau))
    simple_prove(G, gamma, r, s, ctx)


def pair_verify(G, H, X, Y, Xbar, Ybar, ctx):
    k = len(X)
    assert k > 1 and len(Y) == k and len(Xbar) == k and len(Ybar) == k
    p1 = ctx.Get("P" * (4 * k + 3))
    Gamma, W = p1[0], p1[1 + 3 * k:1 + 4 * k]
    Lambda1, Lambda2 = p1[4 * k + 1], p1[4 * k + 2]
    rho = [sc(v) for v in ctx.PubRand(k)]
    D = ctx.Get("P" * k)
    ctx.PubRand(1)
    p5 = ctx.Get("S" * (k + 1))
    sigma, tau = p5[:k], p5[k]
    simple_verify(G, Gamma, k, ctx)
    Phi1, Phi2 = NULL, NULL
    sX, rX = pmul_many(sigma, Xbar), pmul_many(rho, X)
    sY, rY = pmul_many(sigma, Ybar), pmul_many(rho, Y)
    sG = pmul_many(sigma, [Gamma] * k)
    for i in range(k):
        Phi1 = padd(Phi1, sX[i])  # (31)
        Phi1 = psub(Phi1, rX[i])
        Phi2 = padd(Phi2, sY[i])  # (32)
        Phi2 = psub(Phi2, rY[i])
        if not pequal(sG[i], padd(W[i], D[i])):  # (33)
            raise ShuffleError(ERR_PAIR)
    if not pequal(padd(Lambda1, pmul(tau, G)), Phi1) or not pequal(padd(Lambda2, pmul(tau, H)), Phi2):
        raise ShuffleError(ERR_PAIR)


def shuffle(G, H, X, Y, rand):
    """Shuffle (pair.go:318-361): (Xbar, Ybar, prover); rand(n) -> n stream bytes"""
    k = len(X)
    assert k == len(Y)
    pi = list(range(k))
    for i in range(k - 1, 0, -1):
        j = int.from_bytes(rand(8), "big") % (i + 1)  # randUint64: Bits(64, false, rand), big-endian
        if j != i:
            pi[j], pi[i] = pi[i], pi[j]
    beta = [pick(rand) for _ in range(k)]
    Xbar = [padd(pmul(sc(beta[pi[i]]), G), X[pi[i]]) for i in range(k)]
    Ybar = [padd(pmul(sc(beta[pi[i]]), H), Y[pi[i]]) for i in range(k)]
    return Xbar, Ybar, lambda ctx: pair_prove(pi, G, H, beta, X, Y, ctx)


def verifier(G, H, X, Y, Xbar, Ybar):
    return lambda ctx: pair_verify(G, H, X, Y, Xbar, Ybar, ctx)


# ----------------------------------------------------------------------------------------------------- sequences.go
def random_int(mod: int, rand) -> int:
    """random.Int (rand.go:19-46): Bits(BitLen(mod), false), big-endian, redrawn until below mod"""
    bits = mod.bit_length()
    while True:
        b = bytearray(rand((bits + 7) // 8))
        if bits & 7:
            b[0] &= 0xFF >> (8 - (bits & 7))
        v = int.from_bytes(b, "big")
        if v < mod:
            return v


def get_sequence_verifiable(X, Y, Xbar, Ybar, e):
    """(XUp, YUp, XDown, YDown) of sequences.go:155-190; X[j][i], e[j] as wire bytes"""
    NQ, k = len(X), len(X[0])

    def fold(M):
        out = []
        for i in range(k):
            acc = pmul(e[0], M[0][i])
            for j in range(1, NQ):
                acc = padd(acc, pmul(e[j], M[j][i]))
            out.append(acc)
        return out

    return fold(X), fold(Y), fold(Xbar), fold(Ybar)


def sequences_shuffle(G, H, X, Y, rand):
    """SequencesShuffle (sequences.go:36-124): (xBar, yBar, getProver); getProver(e) -> prover, e as integers"""
    NQ, k = len(X), len(X[0])
    pi = list(range(k))
    for i in range(k - 1, 0, -1):
        j = random_int(i + 1, rand)
        if j != i:
            pi[i], pi[j] = pi[j], pi[i]
    beta = [[pick(rand) for _ in range(k)] for _ in range(NQ)]
    xbar = [[padd(pmul(sc(beta[j][pi[i]]), G), X[j][pi[i]]) for i in range(k)] for j in range(NQ)]
    ybar = [[padd(pmul(sc(beta[j][pi[i]]), H), Y[j][pi[i]]) for i in range(k)] for j in range(NQ)]

    def get_prover(e):
        assert len(e) == NQ
        beta2 = [sum(e[j] * beta[j][i] for j in range(NQ)) % L for i in range(k)]
        XUp, YUp, _, _ = get_sequence_verifiable(X, Y, xbar, ybar, [sc(v) for v in e])
        return lambda ctx: pair_prove(pi, G, H, beta2, XUp, YUp, ctx)

    return xbar, ybar, get_prover
