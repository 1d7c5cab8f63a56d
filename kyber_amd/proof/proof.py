"""Host-side mirror of the reference's proof predicates (proof/proof.go), function for function, over the contexts of
kyber_amd/proof/hash.py and the engine's linear combination:

  Rep, And, Or, String                     proof.go:147-193, 341-361, 449-469   -> Rep, And, Or, Predicate.String
  enumVars, makeScalars, send/getResponses proof.go:195-201, 652-719            -> _scalar_vars, the r lists below
  repPred / andPred / orPred commit, respond   proof.go:203-272, 370-397, 478-576 -> _commit, _respond
  getCommits, verify                       proof.go:274-322, 399-429, 578-624   -> _get_commits, _verify
  Prover, Verifier                         proof.go:721-783                     -> Predicate.Prover, Predicate.Verifier
  HashProve / HashVerify over n proofs of ONE predicate                          -> HashProveBatch, HashVerifyBatch

A Rep's commitment V = w P + v_1 B_1 + ... and its check V == c P + r_1 B_1 + ... are ONE kyb_ed25519_lincomb each
(edwards25519.batch_lincomb); the challenge of a batch is ONE kyb_ed25519_fs_challenge.  Scalars are Python integers
on the prover's side (r = v - c x, the sub-challenge sums); what a verifier reads off the wire stays the raw 32 bytes
(scalar.go:226-232) and multiplies as such, Add reduces, Equal compares bytes.

Point values are 32 bytes, a Point, None (the standard base, Mul(s, nil): point.go:243) or, in the batch calls, an (n, 32)
array; secrets are integers, 32 bytes, a Scalar or an (n, 32) array.  In a lincomb, points given once go in `shared`,
None as a nil term, per-proof arrays in `own`; a Rep with more than four of either kind is composed from batch_mul and
batch_add instead."""
from __future__ import annotations

import numpy as np

from ..group import edwards25519 as ed
from . import hash as PH
from .hash import ProofError

L = ed.ORDER
ErrOrInAnd = "can't have OR predicates within AND predicates"
ErrOrNested = "OR predicates can't be nested in anything else"
ErrOrNestedVerify = "OR predicates can't be in anything else"  # proof.go:592
ErrNoChoice = "no choice of proof branch for OR-predicate "
ErrCommit = "invalid proof: commit mismatch"
ErrSubChallenges = "invalid proof: bad sub-challenges"
_PREC_NONE, _PREC_OR, _PREC_AND = 0, 1, 2


class Predicate:
    def String(self) -> str:
        return self._str(_PREC_NONE)

    def Prover(self, suite, secrets, points, choice=None):
        """a callable over a ProverContext (proof.go:768-775)"""
        return lambda ctx: _prove(self, secrets, points, choice or {}, ctx)

    def Verifier(self, suite, points):
        """a callable over a VerifierContext (proof.go:778-783)"""
        return lambda ctx: _verify_ctx(self, points, ctx)


class _Rep(Predicate):
    def __init__(self, P, T):
        self.P, self.T = P, T

    def _str(self, prec):
        return self.P + "=" + "+".join(s + "*" + b for s, b in self.T)


class _Group(Predicate):
    def __init__(self, sub):
        self.sub = tuple(sub)

    def _str(self, prec):
        s = self.SEP.join(q._str(self.PREC) for q in self.sub)
        return "(" + s + ")" if prec not in (_PREC_NONE, self.PREC) else s


class _And(_Group):
    SEP, PREC = " && ", _PREC_AND


class _Or(_Group):
    SEP, PREC = " || ", _PREC_OR


def Rep(P: str, *SB: str) -> Predicate:
    if len(SB) & 1:
        raise ValueError("mismatched Scalar")
    return _Rep(P, tuple((SB[i], SB[i + 1]) for i in range(0, len(SB), 2)))


def And(*sub: Predicate) -> Predicate:
    return _And(sub)


def Or(*sub: Predicate) -> Predicate:
    return _Or(sub)


def _scalar_vars(p, sidx=None):
    """name -> index from 1 in enumVars' order"""
    sidx = {} if sidx is None else sidx
    if isinstance(p, _Rep):
        for s, _ in p.T:
            sidx.setdefault(s, len(sidx) + 1)
    else:
        for q in p.sub:
            _scalar_vars(q, sidx)
    return sidx


def _reps(p, out=None):
    """the Rep predicates in the order getCommits reads their commitments"""
    out = [] if out is None else out
    if isinstance(p, _Rep):
        out.append(p)
    else:
        for q in p.sub:
            _reps(q, out)
    return out


def _int(x) -> int:
    if isinstance(x, int):
        return x % L
    if hasattr(x, "MarshalBinary"):
        x = x.MarshalBinary()
    return int.from_bytes(bytes(x), "little") % L


def _sc(v: int) -> bytes:
    return (v % L).to_bytes(32, "little")


def _pt(x):
    """a point value as None, 32 bytes or an (n, 32) array"""
    if x is None or isinstance(x, np.ndarray):
        return x
    return x.MarshalBinary() if hasattr(x, "MarshalBinary") else bytes(x)


# ------------------------------------------------------------------------------------------ the engine's part
def lincomb(n: int, terms, expect=None):
    """(out or None, ok or None, status) of sum_j s_j * B_j over n elements.  terms: [(scalars (n, 32) uint8, point)], a
    point being None, 32 bytes or an (n, 32) array.  With expect ((n, 32)) the verdict alone is returned."""
    own, shared = [], []
    for s, B in terms:
        (own if isinstance(B, np.ndarray) else shared).append((s, B))
    while len(shared) > 4 and len(own) < 4:  # a point too many for the batch's tables rides with the elements
        s, B = shared.pop()
        own.append((s, np.tile(np.frombuffer(ed._BASE_ENC if B is None else B, dtype=np.uint8), (n, 1))))
    if len(own) > 4 or len(shared) > 4:
        return _composed(n, terms, expect)
    scalars = np.stack([s for s, _ in own + shared], axis=1)
    pts = np.stack([B for _, B in own], axis=1) if own else None
    return ed.batch_lincomb(np.ascontiguousarray(scalars), pts, [B for _, B in shared], expect, want_out=expect is None)


def _composed(n: int, terms, expect):
    """the same value from batch_mul / batch_mul_base / batch_add, for a Rep with more terms than one lincomb takes"""
    acc, bad = None, np.zeros(n, dtype=np.uint8)
    for s, B in terms:
        if B is None:
            t = np.asarray(ed.batch_mul_base(s))
        else:
            t, st = ed.batch_mul(s, B if isinstance(B, np.ndarray) else np.tile(np.frombuffer(B, dtype=np.uint8), (n, 1)))
            bad |= np.asarray(st) != 0
            t = np.where(bad[:, None] != 0, np.frombuffer(ed._NULL_ENC, dtype=np.uint8), np.asarray(t))
        acc = t if acc is None else np.asarray(ed.batch_add(acc, np.ascontiguousarray(t))[0])
    acc = np.where(bad[:, None] != 0, 0, acc).astype(np.uint8)
    if expect is None:
        return acc, None, bad
    canon, st = ed.batch_unmarshal(expect)
    return None, ((np.asarray(canon) == acc).all(axis=1) & (np.asarray(st) == 0) & (bad == 0)).astype(np.uint8), bad


def _rows(x, n: int) -> np.ndarray:
    """a scalar or scalars as (n, 32) bytes"""
    if isinstance(x, np.ndarray):
        return x
    return np.tile(np.frombuffer(_sc(x) if isinstance(x, int) else bytes(x), dtype=np.uint8), (n, 1))


# ------------------------------------------------------------------------------------------------------- prover
class _Prover:
    """the prover's walk for ONE proof with the point arithmetic handed out: draw() is PriRand of one scalar,
    commit(rep, w, v) is told the scalars of a commitment when the reference would Put it"""

    def __init__(self, pred, sval, choice, draw, commit):
        self.sidx = _scalar_vars(pred)
        self.sval, self.choice, self.draw, self.commit_cb = sval, choice, draw, commit
        self.pp = {}

    def _scalars(self, pr):
        return [None] * (len(self.sidx) + 1) if pr is None else pr

    def commit(self, p, w, pv):
        if isinstance(p, _Rep):
            v = self._scalars(pv)
            self.pp[p] = (w, v, None)
            for s, _B in p.T:
                if v[self.sidx[s]] is None:  # a blinding secret the first time a variable is met
                    v[self.sidx[s]] = self.draw()
            self.commit_cb(p, w, [v[self.sidx[s]] for s, _B in p.T])
        elif isinstance(p, _And):
            v = self._scalars(pv)
            for q in p.sub:
                self.commit(q, w, v)
        else:
            if pv is not None:
                raise ProofError(ErrOrInAnd)
            wi = [None] * len(p.sub)
            self.pp[p] = (w, None, wi)
            if w is None:  # proof-obligated: pre-challenges for the other branches only
                choice = self.choice.get(p)
                if choice is None or not 0 <= choice < len(p.sub):
                    raise ProofError(ErrNoChoice + p.String())
                for i in range(len(p.sub)):
                    if i != choice:
                        wi[i] = self.draw()
            else:  # pre-challenges that add up to w
                wl = w
                for i in range(len(p.sub) - 1):
                    wi[i] = self.draw()
                    wl = (wl - wi[i]) % L
                wi[-1] = wl
            for q, x in zip(p.sub, wi):
                self.commit(q, x, None)

    def respond(self, p, c, pr, put):
        """put(list of scalars) is ProverContext.Put of one message"""
        if isinstance(p, _Rep):
            w, v, _ = self.pp[p]
            r = self._scalars(pr)
            for s, _B in p.T:
                i = self.sidx[s]
                if r[i] is None:
                    r[i] = v[i] if w is not None else (v[i] - c * self.sval[s]) % L
            self._send(pr, r, put)
        elif isinstance(p, _And):
            r = self._scalars(pr)
            for q in p.sub:
                self.respond(q, c, r, put)
            self._send(pr, r, put)
        else:
            if pr is not None:
                raise ProofError(ErrOrNested)
            w, _, ci = self.pp[p]
            if w is None:
                choice = self.choice[p]
                ci[choice] = (c - sum(x for i, x in enumerate(ci) if i != choice)) % L
            if len(p.sub) > 1:
                put(ci)
            for q, x in zip(p.sub, ci):
                self.respond(q, x, None, put)

    @staticmethod
    def _send(pr, r, put):
        if pr is None:  # once per OR-domain, the variables it used
            for x in r:
                if x is not None:
                    put([x])


def _commit_terms(p, w, v, pval, n):
    """the terms of V = w P + v_1 B_1 + ... (w = 0 on the obligated branch: Null plus the terms encodes the same bytes)"""
    return [(_rows(w, n), _pt(pval[p.P]))] + [(_rows(x, n), _pt(pval[B])) for x, (_s, B) in zip(v, p.T)]


def _prove(pred, secrets, points, choice, ctx):
    sval = {k: _int(x) for k, x in secrets.items()}

    def commit(p, w, v):
        out, _, st = lincomb(1, _commit_terms(p, w or 0, v, points, 1))
        if np.asarray(st).any():
            raise ProofError(PH.ErrPoint)
        ctx.Put(np.asarray(out))

    pr = _Prover(pred, sval, choice, lambda: _int(ctx.PriRand(1)[0][0].tobytes()), commit)
    pr.commit(pred, None, None)
    c = _int(ctx.PubRand(1)[0].tobytes())
    pr.respond(pred, c, None, lambda xs: ctx.Put(b"".join(_sc(x) for x in xs)))


# ----------------------------------------------------------------------------------------------------- verifier
class _Verifier:
    """the verifier's walk over n proofs at once: get(kind, count) returns a (n, count, 32) array of the next field,
    check(rep, c, r, V) receives a Rep's scalars as (n, 32) arrays, fail(mask, message) the proofs a host check rejects"""

    def __init__(self, pred, get, check, fail):
        self.sidx = _scalar_vars(pred)
        self.get, self.check, self.fail = get, check, fail
        self.vp = {}

    def _scalars(self, pr):
        return [None] * (len(self.sidx) + 1) if pr is None else pr

    def get_commits(self, p, pr):
        if isinstance(p, _Rep):
            r = self._scalars(pr)
            self.vp[p] = (self.get("P", 1)[:, 0], r)
            for s, _B in p.T:
                if r[self.sidx[s]] is None:
                    r[self.sidx[s]] = ()  # a response to read
        elif isinstance(p, _And):
            r = self._scalars(pr)
            self.vp[p] = (None, r)
            for q in p.sub:
                self.get_commits(q, r)
        else:
            for q in p.sub:
                self.get_commits(q, None)

    def _get_responses(self, pr, r):
        if pr is None:
            for i, x in enumerate(r):
                if x is not None:
                    r[i] = self.get("S", 1)[:, 0]

    def verify(self, p, c, pr):
        if isinstance(p, _Rep):
            V, r = self.vp[p]
            self._get_responses(pr, r)
            self.check(p, c, [r[self.sidx[s]] for s, _B in p.T], V)
        elif isinstance(p, _And):
            _, r = self.vp[p]
            self._get_responses(pr, r)
            for q in p.sub:
                self.verify(q, c, r)
        else:
            if pr is not None:
                raise ProofError(ErrOrNestedVerify)
            if len(p.sub) > 1:
                ci = self.get("S", len(p.sub))
                total = [_sc(sum(int.from_bytes(ci[i, j].tobytes(), "little") for j in range(len(p.sub)))) for i in range(ci.shape[0])]
                self.fail(np.array([t != c[i].tobytes() for i, t in enumerate(total)]), ErrSubChallenges)
                subs = [np.ascontiguousarray(ci[:, j]) for j in range(len(p.sub))]
            else:
                subs = [c]
            for q, x in zip(p.sub, subs):
                self.verify(q, x, None)


def _verify_ctx(pred, points, ctx):
    def get(kind, count):
        return ctx.Get((kind, count))[0][None]

    def check(p, c, r, V):
        terms = [(c, _pt(points[p.P]))] + [(x, _pt(points[B])) for x, (_s, B) in zip(r, p.T)]
        _, ok, st = lincomb(1, terms, expect=V)
        if np.asarray(st).any():
            raise ProofError(PH.ErrPoint)
        if not np.asarray(ok)[0]:
            raise ProofError(ErrCommit)

    def fail(mask, message):
        if mask.any():
            raise ProofError(message)

    v = _Verifier(pred, get, check, fail)
    v.get_commits(pred, None)
    if hasattr(ctx, "CheckPoints"):
        ctx.CheckPoints()
    v.verify(pred, np.asarray(ctx.PubRand(1)).reshape(1, 32), None)


# -------------------------------------------------------------------------------------------------------- batches
def _names(protocolNames, n: int):
    if isinstance(protocolNames, (str, bytes, bytearray)):
        return protocolNames.encode() if isinstance(protocolNames, str) else bytes(protocolNames)
    if len(protocolNames) != n:
        raise ValueError("protocolNames: one name or one per proof")
    return [x.encode() if isinstance(x, str) else bytes(x) for x in protocolNames]


def _name_of(names, i: int) -> bytes:
    return names if isinstance(names, bytes) else names[i]


def _row(x, i: int):
    return x[i].tobytes() if isinstance(x, np.ndarray) else x


def _challenges(names, data: np.ndarray) -> np.ndarray:
    c, st = ed.batch_fs_challenge(names, data)
    if np.asarray(st).any():
        raise ProofError("Scalar.Pick found no scalar in 128 draws")
    return np.asarray(c)


def HashProveBatch(protocolNames, pred, secrets, points, choices, rands):
    """n proofs of ONE predicate, proof i byte for byte HashProve(Suite(rands[i]), name_i, pred.Prover(...)).  secrets and
    points: a value shared by the batch or an (n, 32) array; choices: None, one choice map for all proofs or one per
    proof; rands: one BLAKE2Xb stream per proof.  The private draws are read proof by proof on the host, in the
    reference's order; the commitments are ONE lincomb per Rep, the challenges ONE fs_challenge, the responses host
    integers.  Returns a list of n byte strings."""
    n = len(rands)
    names = _names(protocolNames, n)
    points = {k: _pt(v) for k, v in points.items()}
    if choices is None or isinstance(choices, dict):
        choices = [choices or {}] * n
    reps = _reps(pred)
    walks, recorded = [], []
    for i in range(n):
        sval = {k: _int(_row(v, i)) for k, v in secrets.items()}
        rec = {}
        read = PH._reader(rands[i])
        w = _Prover(pred, sval, choices[i], lambda read=read: PH.blake2xb.pick_int(read)[0],
                    lambda p, w_, v, rec=rec: rec.__setitem__(p, (w_ or 0, v)))
        w.commit(pred, None, None)
        walks.append(w)
        recorded.append(rec)
    commits = np.zeros((n, len(reps), 32), dtype=np.uint8)
    for k, p in enumerate(reps):
        col = lambda f: np.frombuffer(b"".join(_sc(f(recorded[i][p])) for i in range(n)), dtype=np.uint8).reshape(n, 32).copy()
        terms = [(col(lambda e: e[0]), points[p.P])] + [(col(lambda e, j=j: e[1][j]), points[B]) for j, (_s, B) in enumerate(p.T)]
        out, _, st = lincomb(n, terms)
        if np.asarray(st).any():
            raise ProofError(PH.ErrPoint)
        commits[:, k] = np.asarray(out)
    c = _challenges(names, commits.reshape(n, -1))
    proofs = []
    for i in range(n):
        msg = [commits[i].tobytes()]
        walks[i].respond(pred, _int(c[i].tobytes()), None, lambda xs: msg.append(b"".join(_sc(x) for x in xs)))
        proofs.append(b"".join(msg))
    return proofs


def HashVerifyBatch(protocolNames, pred, points, proofs):
    """n proofs of ONE predicate: a list with None, or the ProofError the sequential HashVerify raises for that proof.
    The batch's work is one batch_unmarshal over all commitments, one fs_challenge and one lincomb per Rep; a proof
    that fails anything there -- and a proof too short for the predicate -- is then verified on its own, so that the
    first failure in the reference's order decides its message.  Trailing bytes are ignored."""
    n = len(proofs)
    names = _names(protocolNames, n)
    points = {k: _pt(v) for k, v in points.items()}
    reps = _reps(pred)
    # the proof's length: the commitments, then what verify reads (a dry walk over an empty batch counts the fields)
    count = [0]
    dry = _Verifier(pred, lambda kind, cnt: (count.__setitem__(0, count[0] + cnt), np.zeros((0, cnt, 32), dtype=np.uint8))[1],
                    lambda *a: None, lambda *a: None)
    dry.get_commits(pred, None)
    dry.verify(pred, np.zeros((0, 32), dtype=np.uint8), None)
    size = 32 * count[0]
    full = [i for i in range(n) if len(proofs[i]) >= size]
    bad = np.zeros(n, dtype=bool)
    bad[[i for i in range(n) if len(proofs[i]) < size]] = True
    if full:
        m = len(full)
        buf = np.frombuffer(b"".join(bytes(proofs[i])[:size] for i in full), dtype=np.uint8).reshape(m, size // 32, 32)
        sel = lambda v: v[full] if isinstance(v, np.ndarray) else v
        pts = {k: sel(v) for k, v in points.items()}
        failed = np.zeros(m, dtype=bool)
        pos = [0]

        def get(kind, cnt):
            a = buf[:, pos[0]:pos[0] + cnt]
            pos[0] += cnt
            return a

        def check(p, c, r, V):
            terms = [(np.ascontiguousarray(c), pts[p.P])] + [(np.ascontiguousarray(x), pts[B]) for x, (_s, B) in zip(r, p.T)]
            _, ok, st = lincomb(m, terms, expect=np.ascontiguousarray(V))
            failed[:] |= (np.asarray(ok) == 0) | (np.asarray(st) != 0)

        def fail(mask, message):
            failed[:] |= mask

        v = _Verifier(pred, get, check, fail)
        v.get_commits(pred, None)
        commits = np.ascontiguousarray(buf[:, :len(reps)])
        _, st = ed.batch_unmarshal(commits.reshape(-1, 32))
        failed |= (np.asarray(st).reshape(m, len(reps)) != 0).any(axis=1)
        nm = names if isinstance(names, bytes) else [names[i] for i in full]
        v.verify(pred, _challenges(nm, commits.reshape(m, -1)), None)
        bad[np.array(full)[failed]] = True
    out = [None] * n
    for i in np.nonzero(bad)[0]:
        one = {k: _row(v, i) for k, v in points.items()}
        try:
            PH.HashVerify(PH.Suite(), _name_of(names, i), pred.Verifier(None, one), proofs[i])
            out[i] = ProofError("the batch rejected a proof its own verification accepts")  # never: both run the same checks
        except ProofError as e:
            out[i] = e
    return out
