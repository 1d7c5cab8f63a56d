"""proof/dleq (dleq.go) and share/pvss (pvss.go) restated in Python on oracle/ed25519.py, hashlib and the host BLAKE2Xb
(no GPU, no engine): the checker of kyb_ed25519_dleq_challenge / kyb_ed25519_dleq_verify and of kyber_amd/share/pvss.py,
never the thing shipped.  Points and scalars are 32 wire bytes; a share is (I, V, (C, R, VG, VH)).  Errors are returned by
the reference's names (pvss.go:34-39)."""
import hashlib

from kyber_amd.util import blake2xb
from oracle import ed25519 as O

ErrTooFewShares, ErrEncVerification, ErrDecVerification = "ErrTooFewShares", "ErrEncVerification", "ErrDecVerification"
ErrGlobalChallengeVerification, ErrDecShareChallengeVerification = "ErrGlobalChallengeVerification", "ErrDecShareChallengeVerification"
ST_OK, ST_BAD_POINT, ST_DLEQ_CHALLENGE = 0, 1, 7  # include/kyber_hip.h
BASE = O.encode(O.B)


def le(b) -> int:
    return int.from_bytes(bytes(b), "little")


def sc(v: int) -> bytes:
    return (v % O.L).to_bytes(32, "little")


def canon(enc: bytes):
    """MarshalBinary(UnmarshalBinary(enc)), or None where UnmarshalBinary fails"""
    pt = O.decode(bytes(enc))
    return None if pt is None else O.encode(pt)


def pick(seed: bytes) -> bytes:
    """suite.Scalar().Pick(suite.XOF(seed)) (scalar.go:180-184 over xof/blake2xb)"""
    return blake2xb.pick(blake2xb.New(seed).Read)


def mul(s: bytes, p: bytes) -> bytes:
    out = O.mul(bytes(s), bytes(p))
    assert out is not None
    return out


# ------------------------------------------------------------------------------------------------- proof/dleq
def dleq_challenge(xG, xH, vG, vH) -> bytes:
    """dleq.go:57-76: the four points are hashed as MarshalTo writes them"""
    return pick(hashlib.sha256(b"".join(canon(p) for p in (xG, xH, vG, vH))).digest())


def dleq_verify(G, H, xG, xH, C, R, VG, VH, vartime=False) -> bool:
    """Proof.Verify (dleq.go:160-172) on wire bytes; a point that does not decode makes the proof invalid.  Scalars are
    used as UnmarshalBinary leaves them (unreduced), through the oracle's Mul."""
    vg, vh = canon(VG), canon(VH)
    parts = [O.mul(bytes(R), bytes(G), vartime), O.mul(bytes(C), bytes(xG), vartime), O.mul(bytes(R), bytes(H), vartime),
             O.mul(bytes(C), bytes(xH), vartime)]
    if vg is None or vh is None or any(p is None for p in parts):
        return False
    a = O.encode(O.add(O.decode(parts[0]), O.decode(parts[1])))
    b = O.encode(O.add(O.decode(parts[2]), O.decode(parts[3])))
    return a == vg and b == vh


def abi_status(G, H, xG, xH, C, expect_c=None, fs_with=None) -> int:
    """status[i] of kyb_ed25519_dleq_verify: the challenge first, then the four points the equations decode.
    fs_with: (VG, VH) when KYB_F_DLEQ_FS is set"""
    if expect_c is not None and bytes(C) != bytes(expect_c):
        return ST_DLEQ_CHALLENGE
    if fs_with is not None and bytes(C) != device_challenge(xG, xH, *fs_with):
        return ST_DLEQ_CHALLENGE
    return ST_BAD_POINT if any(O.decode(bytes(p)) is None for p in (G, H, xG, xH)) else ST_OK


def canon_bytes_rule(enc: bytes) -> bytes:
    """the canonical bytes the device derives WITHOUT decoding (csrc/ed25519_dleq.cuh): y mod p, sign cleared where x = 0"""
    v = le(enc)
    y, sign = v & ((1 << 255) - 1), v >> 255
    if y >= O.P:
        y -= O.P
    if y in (1, O.P - 1):
        sign = 0
    return (y | sign << 255).to_bytes(32, "little")


def device_challenge(xG, xH, vG, vH) -> bytes:
    """kyb_ed25519_dleq_challenge: dleq_challenge wherever the four encodings decode, defined on every input"""
    return pick(hashlib.sha256(b"".join(canon_bytes_rule(p) for p in (xG, xH, vG, vH))).digest())


def new_proof(G, H, x: bytes, rand):
    """NewDLEQProof (dleq.go:41-82): ((C, R, VG, VH), xG, xH); rand is the suite's random stream"""
    xG, xH = mul(x, G), mul(x, H)
    v = blake2xb.pick(rand)
    vG, vH = mul(v, G), mul(v, H)
    c = dleq_challenge(xG, xH, vG, vH)
    return (c, sc(le(v) - le(c) * le(x)), vG, vH), xG, xH


def new_proof_batch(G, H, secrets, rand):
    """NewDLEQProofBatch (dleq.go:87-154): one collective challenge"""
    assert len(G) == len(H) == len(secrets)
    xG, xH, v, vG, vH = [], [], [], [], []
    for i, x in enumerate(secrets):
        xG.append(mul(x, G[i]))
        xH.append(mul(x, H[i]))
        v.append(blake2xb.pick(rand))
        vG.append(mul(v[i], G[i]))
        vH.append(mul(v[i], H[i]))
    c = pick(hashlib.sha256(b"".join(xG + xH + vG + vH)).digest())
    return [(c, sc(le(v[i]) - le(c) * le(x)), vG[i], vH[i]) for i, x in enumerate(secrets)], xG, xH


# ------------------------------------------------------------------------------------------------- share/pvss
def enc_shares(H, X, secret: bytes, t: int, rand):
    """EncShares (pvss.go:51-92): (shares, commits, coeffs); NewPriPoly keeps the secret and picks t - 1 coefficients"""
    n = len(X)
    coeffs = [le(secret)] + [le(blake2xb.pick(rand)) for _ in range(t - 1)]
    values = [sc(sum(c * pow(i + 1, j, O.L) for j, c in enumerate(coeffs))) for i in range(n)]  # PriPoly.Eval
    commits = [mul(sc(c), H) for c in coeffs]
    proofs, _, sX = new_proof_batch([H] * n, X, values, rand)
    return [(i, sX[i], proofs[i]) for i in range(n)], commits, coeffs


def compute_commitments(n: int, commits, coeffs=None, H=None):
    """computeCommitments (pvss.go:94-114), the Horner loop.  With the dealer's coefficients at hand the same points are
    p(i) * H (a PubPoly evaluates to the commitment of its PriPoly's value): the n = 1000 round uses that, the Horner
    loop there being 5 x 10^5 oracle multiplications."""
    if coeffs is not None:
        return [mul(sc(sum(c * pow(i + 1, j, O.L) for j, c in enumerate(coeffs))), H) for i in range(n)]
    out = []
    for i in range(n):
        acc = O.IDENTITY
        for j in range(len(commits) - 1, 0, -1):
            acc = O.mul_int(i + 1, O.add(acc, O.decode(commits[j])))
        out.append(O.encode(O.add(acc, O.decode(commits[0]))))
    return out


def global_challenge(coms, shares) -> bytes:
    """computeGlobalChallenge (pvss.go:116-149)"""
    return pick(hashlib.sha256(b"".join(list(coms) + [s[1] for s in shares] + [s[2][2] for s in shares] + [s[2][3] for s in shares])).digest())


def verify_enc_share(H, X, sH, exp_c, share):
    """VerifyEncShare (pvss.go:154-163): None or the error's name"""
    _, V, (C, R, VG, VH) = share
    if bytes(C) != bytes(exp_c):
        return ErrGlobalChallengeVerification
    return None if dleq_verify(H, X, sH, V, C, R, VG, VH) else ErrEncVerification


def dec_share(H, X, sH, x: bytes, exp_c, share, rand):
    """DecShare (pvss.go:199-217): (decrypted share, None) or (None, error)"""
    err = verify_enc_share(H, X, sH, exp_c, share)
    if err:
        return None, err
    V = mul(sc(pow(le(x), O.L - 2, O.L)), share[1])
    proof, _, _ = new_proof(BASE, V, x, rand)
    return (share[0], V, proof), None


def verify_dec_share(G, X, enc, dec):
    """VerifyDecShare (pvss.go:248-277): None or the error's name"""
    _, V, (C, R, VG, VH) = dec
    pts = [canon(p) for p in (X, enc[1], VG, VH)]
    if any(p is None for p in pts):
        return ErrDecVerification  # (the reference could not have unmarshalled such a share)
    if bytes(C) != pick(hashlib.sha256(b"".join(pts)).digest()):
        return ErrDecShareChallengeVerification
    return None if dleq_verify(G, V, X, enc[1], C, R, VG, VH) else ErrDecVerification


def recover_secret(G, X, encs, decs, t: int, n: int):
    """RecoverSecret (pvss.go:303-323): (point bytes, None) or (None, ErrTooFewShares); RecoverCommit interpolates over
    the first t valid shares by index (share/poly.go:418-476)"""
    D = [d for x, e, d in zip(X, encs, decs) if verify_dec_share(G, x, e, d) is None]
    if len(D) < t:
        return None, ErrTooFewShares
    use = sorted(D, key=lambda d: d[0])[:t]
    acc = O.IDENTITY
    for d in use:
        num = den = 1
        for o in use:
            if o[0] != d[0]:
                num = num * (o[0] + 1) % O.L
                den = den * (o[0] - d[0]) % O.L
        acc = O.add(acc, O.mul_int(num * pow(den, O.L - 2, O.L) % O.L, O.decode(d[1])))
    return O.encode(acc), None
