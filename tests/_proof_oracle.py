"""CPU ORACLE (test infrastructure) -- the reference's proof/proof.go and shuffle/biffle.go restated sequentially in
Python integers over oracle/ed25519.py and the HashProver / HashVerifier of tests/_shuffle_oracle.py.  The checker of the
predicate tests, never the thing shipped.

A predicate is a tuple: ("rep", P, ((s, B), ...)), ("and", subs), ("or", subs); an Or's branch choice is keyed by the
predicate's id(), as the reference keys its map by the pointer.  Point values are 32 wire bytes, None the standard
base (Mul(s, nil), point.go:243); secrets are integers.  Responses and sub-challenges read off the wire stay the raw 32
bytes (scalar.go:226-232) and multiply as such; Add reduces; Equal compares bytes."""
from oracle import ed25519 as O
from tests import _anon_oracle as AO
from tests import _shuffle_oracle as SO

L = O.L
IDENT = O.encode(O.IDENTITY)
ERR_OR_IN_AND = "can't have OR predicates within AND predicates"
ERR_OR_NESTED = "OR predicates can't be nested in anything else"
ERR_OR_NESTED_V = "OR predicates can't be in anything else"
ERR_NO_CHOICE = "no choice of proof branch for OR-predicate "
ERR_COMMIT = "invalid proof: commit mismatch"
ERR_SUB = "invalid proof: bad sub-challenges"


class ProofError(SO.ShuffleError):
    pass


def Rep(P, *SB):
    if len(SB) & 1:
        raise ValueError("mismatched Scalar")
    return ("rep", P, tuple((SB[i], SB[i + 1]) for i in range(0, len(SB), 2)))


def And(*sub):
    return ("and", tuple(sub))


def Or(*sub):
    return ("or", tuple(sub))


PREC_NONE, PREC_OR, PREC_AND = 0, 1, 2


def string(p, prec=PREC_NONE) -> str:
    if p[0] == "rep":
        return p[1] + "=" + "+".join(s + "*" + b for s, b in p[2])
    mine, sep = (PREC_AND, " && ") if p[0] == "and" else (PREC_OR, " || ")
    s = sep.join(string(q, mine) for q in p[1])
    return "(" + s + ")" if prec not in (PREC_NONE, mine) else s


def scalar_vars(p, sidx=None):
    """name -> index from 1, in enumVars' order (proof.go:195-201, 652-673)"""
    sidx = {} if sidx is None else sidx
    if p[0] == "rep":
        for s, _ in p[2]:
            sidx.setdefault(s, len(sidx) + 1)
    else:
        for q in p[1]:
            scalar_vars(q, sidx)
    return sidx


class _State:
    def __init__(self, pred, pval, ctx, sval=None, choice=None):
        self.sidx = scalar_vars(pred)
        self.n = len(self.sidx) + 1
        self.pval, self.sval, self.choice, self.ctx = pval, sval, choice or {}, ctx
        self.pp, self.vp = {}, {}

    def scalars(self, pr):
        return [None] * self.n if pr is None else pr


def _pmul(s: bytes, B):
    return SO.pmul(s, B)


# ------------------------------------------------------------------------------------------------------------ prover
def _commit(st, p, w, pv):
    if p[0] == "rep":
        v = st.scalars(pv)
        st.pp[id(p)] = (w, v, None)
        V = _pmul(SO.sc(w), st.pval[p[1]]) if w is not None else IDENT
        for s, B in p[2]:
            i = st.sidx[s]
            if v[i] is None:
                v[i] = st.ctx.PriRand(1)[0]
            V = SO.padd(V, _pmul(SO.sc(v[i]), st.pval[B]))
        st.ctx.Put(V)
    elif p[0] == "and":
        v = st.scalars(pv)
        for q in p[1]:
            _commit(st, q, w, v)
    else:
        if pv is not None:
            raise ProofError(ERR_OR_IN_AND)
        sub = p[1]
        wi = [None] * len(sub)
        st.pp[id(p)] = (w, None, wi)
        if w is None:
            choice = st.choice.get(id(p))
            if choice is None or not 0 <= choice < len(sub):
                raise ProofError(ERR_NO_CHOICE + string(p))
            for i in range(len(sub)):
                if i != choice:
                    wi[i] = st.ctx.PriRand(1)[0]
        else:
            wl = w
            for i in range(len(sub) - 1):
                wi[i] = st.ctx.PriRand(1)[0]
                wl = (wl - wi[i]) % L
            wi[-1] = wl
        for q, x in zip(sub, wi):
            _commit(st, q, x, None)


def _send(st, pr, r):
    if pr is None:
        for x in r:
            if x is not None:
                st.ctx.Put(SO.sc(x))


def _respond(st, p, c, pr):
    if p[0] == "rep":
        w, v, _ = st.pp[id(p)]
        r = st.scalars(pr)
        for s, _B in p[2]:
            i = st.sidx[s]
            if r[i] is None:
                r[i] = v[i] if w is not None else (v[i] - c * st.sval[s]) % L
        _send(st, pr, r)
    elif p[0] == "and":
        r = st.scalars(pr)
        for q in p[1]:
            _respond(st, q, c, r)
        _send(st, pr, r)
    else:
        if pr is not None:
            raise ProofError(ERR_OR_NESTED)
        w, _, ci = st.pp[id(p)]
        sub = p[1]
        if w is None:
            choice = st.choice[id(p)]
            ci[choice] = (c - sum(x for i, x in enumerate(ci) if i != choice)) % L
        if len(sub) > 1:
            st.ctx.Put([SO.sc(x) for x in ci])
        for q, x in zip(sub, ci):
            _respond(st, q, x, None)


def prover(pred, sval, pval, choice=None):
    """choice: {id(or predicate): branch}"""
    def run(ctx):
        st = _State(pred, pval, ctx, sval, choice)
        _commit(st, pred, None, None)
        c = ctx.PubRand(1)[0]
        _respond(st, pred, c, None)
    return run


# ---------------------------------------------------------------------------------------------------------- verifier
def _get_commits(st, p, pr):
    if p[0] == "rep":
        r = st.scalars(pr)
        V = st.ctx.Get("P")[0]
        st.vp[id(p)] = (V, r)
        for s, _B in p[2]:
            if r[st.sidx[s]] is None:
                r[st.sidx[s]] = b""  # a slot to fill
    elif p[0] == "and":
        r = st.scalars(pr)
        st.vp[id(p)] = (None, r)
        for q in p[1]:
            _get_commits(st, q, r)
    else:
        for q in p[1]:
            _get_commits(st, q, None)


def _get_responses(st, pr, r):
    if pr is None:
        for i, x in enumerate(r):
            if x is not None:
                r[i] = st.ctx.Get("S")[0]


def _verify(st, p, c: bytes, pr):
    if p[0] == "rep":
        V0, r = st.vp[id(p)]
        _get_responses(st, pr, r)
        V = _pmul(c, st.pval[p[1]])
        for s, B in p[2]:
            V = SO.padd(V, _pmul(r[st.sidx[s]], st.pval[B]))
        if not SO.pequal(V, V0):
            raise ProofError(ERR_COMMIT)
    elif p[0] == "and":
        _, r = st.vp[id(p)]
        _get_responses(st, pr, r)
        for q in p[1]:
            _verify(st, q, c, r)
    else:
        if pr is not None:
            raise ProofError(ERR_OR_NESTED_V)
        sub = p[1]
        if len(sub) > 1:
            ci = st.ctx.Get("S" * len(sub))
            if SO.sc(sum(SO.le(x) for x in ci)) != c:
                raise ProofError(ERR_SUB)
        else:
            ci = [c]
        for q, x in zip(sub, ci):
            _verify(st, q, x, None)


def verifier(pred, pval):
    def run(ctx):
        st = _State(pred, pval, ctx)
        _get_commits(st, pred, None)
        c = SO.sc(ctx.PubRand(1)[0])
        _verify(st, pred, c, None)
    return run


def hash_prove(name: bytes, pred, sval, pval, choice, rand) -> bytes:
    return SO.hash_prove(name, prover(pred, sval, pval, choice), rand.Read)


def hash_verify(name: bytes, pred, pval, proof: bytes):
    """None, or the error's message"""
    return SO.hash_verify(name, verifier(pred, pval), proof)


# ------------------------------------------------------------------------------------------------------ biffle.go
def biffle_pred():
    and0 = And(Rep("Xbar0-X0", "beta0", "G"), Rep("Ybar0-Y0", "beta0", "H"), Rep("Xbar1-X1", "beta1", "G"), Rep("Ybar1-Y1", "beta1", "H"))
    and1 = And(Rep("Xbar0-X1", "beta1", "G"), Rep("Ybar0-Y1", "beta1", "H"), Rep("Xbar1-X0", "beta0", "G"), Rep("Ybar1-Y0", "beta0", "H"))
    return Or(and0, and1)


def biffle_points(G, H, X, Y, Xbar, Ybar):
    pts = {"G": G, "H": H}
    for i in range(2):
        for j in range(2):
            pts[f"Xbar{i}-X{j}"] = SO.psub(Xbar[i], X[j])
            pts[f"Ybar{i}-Y{j}"] = SO.psub(Ybar[i], Y[j])
    return pts


def biffle(G, H, X, Y, rand):
    """(Xbar, Ybar, prover): biffle.go:49-81; rand: a BLAKE2Xb stream"""
    bit = rand.XORKeyStream(bytes(1))[0] & 1  # random.Bytes
    beta = [SO.pick(rand.Read) for _ in range(2)]
    Xbar, Ybar = [None, None], [None, None]
    for i in range(2):
        pi = i ^ bit
        Xbar[i] = SO.padd(_pmul(SO.sc(beta[pi]), G), X[pi])
        Ybar[i] = SO.padd(_pmul(SO.sc(beta[pi]), H), Y[pi])
    pred = biffle_pred()
    return Xbar, Ybar, prover(pred, {"beta0": beta[0], "beta1": beta[1]}, biffle_points(G, H, X, Y, Xbar, Ybar), {id(pred): bit})


def biffle_verifier(G, H, X, Y, Xbar, Ybar):
    return verifier(biffle_pred(), biffle_points(G, H, X, Y, Xbar, Ybar))


point_pick = AO.point_pick
BASE = O.encode(O.B)


def rep_case():
    """TestRep's setup (proof_test.go:13-56): (predicate, secrets, points, choice, the stream after the two picks)"""
    from kyber_amd.util import blake2xb

    rand = blake2xb.New(b"seed")
    x, y = SO.pick(rand.Read), SO.pick(rand.Read)
    Xp = _pmul(SO.sc(x), None)
    Yp = _pmul(SO.sc(y), Xp)
    Rp = SO.padd(Xp, Yp)
    andx = And(And(Rep("X", "x", "B"), Rep("R", "x", "B", "y", "X")))
    false_and = And(Rep("Y", "x", "B"), Rep("R", "x", "B", "y", "B"))
    or1 = Or(false_and, andx)
    or1x = Or(or1)
    or2x = Or(Or(Rep("B", "y", "X"), Rep("R", "x", "R")))
    pred = Or(or1x, or2x)
    return pred, {"x": x, "y": y}, {"B": BASE, "X": Xp, "Y": Yp, "R": Rp}, {id(or1): 1, id(or1x): 0, id(pred): 0}, rand
