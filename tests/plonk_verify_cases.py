"""The reference model, a small prover and the cases of the PLONK verifier tests (test_plonk_verify.py on the emulation,
test_plonk_verify_gpu.py on the device); every case takes the context it runs on.

  * model_rows / model_verify: backend/plonk/bn254/verify.go:36-323 restated over pyref's integers, points and pairing_check, with the
    reference's conventions (the inverse of 0 is 0 in fr.Inverse, BatchInvert and Div).
  * prove: backend/plonk/bn254/prove.go over pyref (plonk_synthetic_instance, plonk_build_z, plonk_quotient, the linearised polynomial
    of prove.go:1352-1460, kzg.Open / BatchOpenSinglePoint) with an SRS from a KNOWN tau, so a commitment is [p(tau)]G1.
  * The challenges come from a SHA-256 transcript of THIS module, shared by its prover and its verifiers.  It is NOT gnark's
    (gnark-crypto's fiatshamir package, kzg.FoldProof's transcript and the crypto/rand draw of BatchVerifyMultiPoints are not
    restated): the device takes the six values as inputs, and so does the model.
  * Public inputs as gnark makes them: row i < nb_public carries x_i in the prover's Qk and 0 in the key's; the BSB22 hash of
    commitment t sits in the prover's Qk at row nb_public + CommitmentConstraintIndexes[t]."""
import ctypes as C
import functools
import hashlib

import numpy as np

import pyref
from gnark_amd import _lib
from gnark_amd import plonk_verify as pv
from helpers import arr_to_fr, fr_to_arr, g1_to_arr, g2_to_arr

CURVES = (pyref.BN254, pyref.BLS12_381)
TAU = 0x1D2C3B4A59687766554433221100FFEEDDCCBBAA99887766554433221100F1E2
BSB22_DST = b"BSB22-Plonk"
NP_FIXED = 9


def finv(x, r):
    """fr.Inverse: the inverse of 0 is 0"""
    return pow(x % r, r - 2, r)


def challenge(c, label, *parts):
    h = hashlib.sha256(label.encode())
    for p in parts:
        h.update(p if isinstance(p, bytes) else int(p).to_bytes(64, "big"))
    return int.from_bytes(h.digest(), "big") % c.r


def point_bytes(c, P):
    return b"\x00" * (2 * c.fp_bytes) if P is None else pyref.g1_marshal_uncompressed(c, P)


class Key:
    """plonk.VerifyingKey over pyref's points"""

    def __init__(self, c, n, nb_public, cci, S, Ql, Qr, Qm, Qo, Qk, Qcp, g1, g2):
        self.c, self.n, self.nb_public, self.cci = c, n, nb_public, list(cci)
        self.S, self.Ql, self.Qr, self.Qm, self.Qo, self.Qk, self.Qcp, self.g1, self.g2 = S, Ql, Qr, Qm, Qo, Qk, list(Qcp), g1, g2

    def device(self, ctx=None):
        """the package's VerifyingKey over the same points (pinned when a context is given)"""
        c = self.c
        one = lambda P: g1_to_arr(c, [P])[0]
        size_inv, gen, shift = pv.domain_constants(c.cid, self.n)
        vk = pv.VerifyingKey(c.cid, self.n, size_inv, gen, self.nb_public, shift, g1_to_arr(c, self.S), one(self.Ql), one(self.Qr), one(self.Qm),
                             one(self.Qo), one(self.Qk), g1_to_arr(c, self.Qcp).reshape(len(self.Qcp), 2 * c.fp_limbs), one(self.g1),
                             g2_to_arr(c, self.g2), list(self.cci))
        return vk.Pin(ctx) if ctx is not None else vk


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def model_pi(c, n, nb_public, cci, zeta, pub, hashes):
    """verify.go:136-188"""
    r = c.r
    w, ninv = c.fr_root_of_unity(n), pow(n, -1, r)
    zh = (pow(zeta, n, r) - 1) % r
    pi = 0
    for i, x in enumerate(pub):                               # BatchInvert leaves a zero denominator zero
        wi = pow(w, i, r)
        pi = (pi + zh * finv(zeta - wi, r) % r * ninv % r * wi % r * x) % r
    for t, h in zip(cci, hashes):                             # Div by a zero denominator gives zero
        wi = pow(w, nb_public + t, r)
        pi = (pi + zh * wi % r * finv(zeta - wi, r) % r * ninv % r * h) % r
    return pi


def model_scalars(c, n, nb_public, cci, evals, chal, pub, hashes):
    """verify.go:124-277: (relation_ok, the scalars of the linearised digest by name)"""
    r = c.r
    nb = len(cci)
    gamma, beta, alpha, zeta, v, u = chal
    cv = evals[:6 + nb]
    zu = evals[6 + nb]
    _, l, ro, o, s1, s2 = cv[:6]
    zn = pow(zeta, n, r)
    zh = (zn - 1) % r
    l1 = finv(zeta - 1, r) * zh % r * pow(n, -1, r) % r
    pi = model_pi(c, n, nb_public, cci, zeta, pub, hashes)
    a2l1 = l1 * alpha % r * alpha % r
    const_lin = (beta * s1 + gamma + l) % r * ((s2 * beta + gamma + ro) % r) % r * ((o + gamma) % r) % r * alpha % r * zu % r
    const_lin = (-(const_lin - a2l1 + pi)) % r
    relation_ok = const_lin == cv[0] % r
    _s1 = (beta * s1 + l + gamma) % r * ((beta * s2 + ro + gamma) % r) % r * beta % r * alpha % r * zu % r
    g = c.fr_gen
    _s2 = (beta * zeta + gamma + l) % r * ((beta * g % r * zeta + gamma + ro) % r) % r * ((beta * g % r * g % r * zeta + o + gamma) % r) % r * alpha % r
    _s2 = (-_s2) % r
    zn2 = pow(zeta, n + 2, r)
    sc = dict(l=l, r=ro, rl=l * ro % r, o=o, one=1, s1=_s1, coeff_z=(a2l1 + _s2) % r, zh=(-zh) % r, zh1=(-(zn2 * zh)) % r,
              zh2=(-(zn2 * zn2 % r * zh)) % r, qc=[x % r for x in cv[6:]])
    return relation_ok, sc


def model_rows(c, n, nb_public, cci, evals, chal, pub, hashes):
    """The coefficient row of the whole KZG check, as ga_plonk_verify_scalars defines it: key columns G1 Ql Qr Qm Qo Qk S1 S2 S3 Qcp..,
    proof columns L R O Z H0 H1 H2 W_zeta W_zeta_omega Bsb.., then (-1, -u)."""
    r = c.r
    nb = len(cci)
    _, _, _, zeta, v, u = chal
    ok, sc = model_scalars(c, n, nb_public, cci, evals, chal, pub, hashes)
    cv, zu = evals[:6 + nb], evals[6 + nb]
    E = sum(pow(v, k, r) * cv[k] for k in range(6 + nb)) % r
    w = c.fr_root_of_unity(n)
    key = [(-(E + u * zu)) % r, sc["l"], sc["r"], sc["rl"], sc["o"], 1, pow(v, 4, r), pow(v, 5, r), sc["s1"]] + [pow(v, 6 + t, r) for t in range(nb)]
    proof = [v % r, pow(v, 2, r), pow(v, 3, r), (sc["coeff_z"] + u) % r, sc["zh"], sc["zh1"], sc["zh2"], zeta % r, u * w % r * zeta % r] + sc["qc"]
    return ok, key + proof + [(-1) % r, (-u) % r]


def model_verify(c, key: Key, proof, pub, chal, hashes=None):
    """plonk.Verify (verify.go:36-323) with the challenges given -> (accepted, relation_ok or None when an earlier check rejects).
    proof: dict with LRO, Z, H, Bsb, Wz, Wzw (points), cv (6 + nb_bsb values), zu."""
    r, G1 = c.r, pyref.g1_group(c)
    nb = len(key.Qcp)
    if len(key.cci) != nb or len(proof["Bsb"]) != nb or len(proof["cv"]) != 6 + nb or len(pub) != key.nb_public:   # :45-59
        return False, None
    for P in proof["LRO"] + [proof["Z"]] + proof["H"] + proof["Bsb"] + [proof["Wz"], proof["Wzw"]]:                  # :61-85
        if not (G1.on_curve(P) and G1.mul(P, r) is None):
            return False, None
    if hashes is None:
        hashes = [pyref.fr_hash(c, point_bytes(c, P), BSB22_DST, 1)[0] for P in proof["Bsb"]]                        # :162-175
    gamma, beta, alpha, zeta, v, u = chal
    evals = list(proof["cv"]) + [proof["zu"]]
    ok, sc = model_scalars(c, key.n, key.nb_public, key.cci, evals, chal, pub, hashes)
    if not ok:
        return False, False
    points = proof["Bsb"] + [key.Ql, key.Qr, key.Qm, key.Qo, key.Qk, key.S[2], proof["Z"]] + proof["H"]                # :263-280
    scalars = sc["qc"] + [sc["l"], sc["r"], sc["rl"], sc["o"], 1, sc["s1"], sc["coeff_z"], sc["zh"], sc["zh1"], sc["zh2"]]
    lin = G1.msm(points, scalars)
    digests = [lin] + proof["LRO"] + [key.S[0], key.S[1]] + key.Qcp                                                   # :283-297: kzg.FoldProof
    vs = [pow(v, k, r) for k in range(6 + nb)]
    folded_digest = G1.msm(digests, vs)
    folded_value = sum(a * b for a, b in zip(vs, proof["cv"])) % r
    # kzg.BatchVerifyMultiPoints (:305-318) over (folded, Z) at (zeta, w zeta) with the scalars (1, u)
    w = c.fr_root_of_unity(key.n)
    lam, ds, hs = [1, u % r], [folded_digest, proof["Z"]], [proof["Wz"], proof["Wzw"]]
    ys, zs = [folded_value, proof["zu"] % r], [zeta % r, zeta * w % r]
    fd = G1.msm(ds, lam)
    fe = G1.mul(key.g1, sum(a * b for a, b in zip(lam, ys)) % r)
    fq = G1.msm(hs, lam)
    fzq = G1.msm(hs, [a * b % r for a, b in zip(lam, zs)])
    left = G1.add(G1.add(fd, G1.neg(fe)), fzq)
    return pyref.pairing_check(c, [(left, key.g2[0]), (G1.neg(fq), key.g2[1])]), True


# ---- the prover ------------------------------------------------------------------------------------------------------------------------
def _canonical(c, n, v):
    w0, ninv = c.fr_root_of_unity(n), pow(n, -1, c.r)
    return [x * ninv % c.r for x in pyref._ntt_natural(list(v), pow(w0, -1, c.r), c.r)]


def _blinded(c, n, coeffs, b):
    """p + b(X) (X^n - 1) (getBlindedCoefficients)"""
    out = list(coeffs) + [0] * len(b)
    for i, bi in enumerate(b):
        out[i] = (out[i] - bi) % c.r
        out[n + i] = (out[n + i] + bi) % c.r
    return out


def _commit(c, poly):
    return pyref.g1_group(c).mul(c.g1, pyref._poly_eval(poly, TAU, c.r))


def _open(c, poly, z):
    """kzg.Open over the known tau: (p(z), [(p(tau) - p(z)) / (tau - z)]G1)"""
    r = c.r
    val = pyref._poly_eval(poly, z, r)
    return val, pyref.g1_group(c).mul(c.g1, (pyref._poly_eval(poly, TAU, r) - val) * pow(TAU - z, -1, r) % r)


def srs_g2(c):
    return [c.g2, pyref.g2_group(c).mul(c.g2, TAU)]


class Circuit:
    """a satisfying synthetic trace with its key: everything that does not depend on a proof's blinding"""

    def __init__(self, c, n, nb_bsb, nb_public, seed=5):
        r = c.r
        self.c, self.n, self.nb_bsb, self.nb_public = c, n, nb_bsb, nb_public
        lag, qcp, pi2, perm, rng = pyref.plonk_synthetic_instance(c, n, seed, nb_bsb)
        self.lag, self.perm, self.rng = lag, perm, rng
        self.cci = list(range(nb_bsb))                                    # the hash of commitment t sits at row nb_public + t
        can = functools.partial(_canonical, c, n)
        self.can = {k: can(v) for k, v in lag.items()}
        self.qcp, self.pi2 = [can(q) for q in qcp], [can(p) for p in pi2]
        self.bsb = [_commit(c, p) for p in self.pi2]
        self.hashes = [pyref.fr_hash(c, point_bytes(c, P), BSB22_DST, 1)[0] for P in self.bsb]
        self.pub = [lag["Qk"][i] for i in range(nb_public)]               # x_i: what the gate of row i needs of Qk
        qk_key = list(lag["Qk"])
        for i in range(nb_public):
            qk_key[i] = 0
        for t, h in zip(self.cci, self.hashes):
            qk_key[nb_public + t] = (qk_key[nb_public + t] - h) % r
        self.qk_key = can(qk_key)
        cm = lambda k: _commit(c, self.can[k])
        self.key = Key(c, n, nb_public, self.cci, [cm("S1"), cm("S2"), cm("S3")], cm("Ql"), cm("Qr"), cm("Qm"), cm("Qo"), _commit(c, self.qk_key),
                       [_commit(c, q) for q in self.qcp], c.g1, srs_g2(c))

    def prove(self, seed):
        """one proof (prove.go): its blinding and therefore its commitments, challenges and openings depend on `seed`"""
        c, n, r = self.c, self.n, self.c.r
        rng = pyref.Xoshiro(1000 + seed)
        bp = {k: [rng.field(r) for _ in range(3 if k == "Bz" else 2)] for k in ("Bl", "Br", "Bo", "Bz")}
        bl = {k: _blinded(c, n, self.can[k], bp["B" + k.lower()]) for k in ("L", "R", "O")}
        LRO = [_commit(c, bl[k]) for k in ("L", "R", "O")]
        key = self.key
        bind = [point_bytes(c, P) for P in key.S + [key.Ql, key.Qr, key.Qm, key.Qo, key.Qk] + key.Qcp] + list(self.pub)
        gamma = challenge(c, "gamma", *bind, *[point_bytes(c, P) for P in LRO])
        beta = challenge(c, "beta", gamma)
        Zl = pyref.plonk_build_z(c, n, self.lag["L"], self.lag["R"], self.lag["O"], self.perm, beta, gamma)
        zc = _canonical(c, n, Zl)
        zb = _blinded(c, n, zc, bp["Bz"])
        Z = _commit(c, zb)
        alpha = challenge(c, "alpha", beta, *[point_bytes(c, P) for P in self.bsb + [Z]])
        x = dict(self.can, Z=zc)
        h = pyref.plonk_quotient(c, n, x, self.qcp, self.pi2, bp, alpha, beta, gamma)
        assert not any(h[3 * (n + 2):]), "the quotient does not fit three shards of n + 2"
        hs = [h[i * (n + 2):(i + 1) * (n + 2)] for i in range(3)]
        H = [_commit(c, s) for s in hs]
        zeta = challenge(c, "zeta", alpha, *[point_bytes(c, P) for P in H])
        lin, evals, zu, Wzw = self.linearise(bl, zb, hs, (gamma, beta, alpha, zeta))
        polys = [lin, bl["L"], bl["R"], bl["O"], self.can["S1"], self.can["S2"]] + self.qcp
        cv = [pyref._poly_eval(p, zeta, r) for p in polys]
        assert cv[1:4] == evals
        v = challenge(c, "fold", zeta, zu, *cv)                          # (this module's stand-in for kzg.FoldProof's transcript)
        folded = [0] * max(len(p) for p in polys)
        for k, p in enumerate(polys):
            vk = pow(v, k, r)
            for i, a in enumerate(p):
                folded[i] = (folded[i] + vk * a) % r
        _, Wz = _open(c, folded, zeta)
        u = challenge(c, "batch", v, point_bytes(c, Wz), point_bytes(c, Wzw))   # (stand-in for crypto/rand in BatchVerifyMultiPoints)
        proof = dict(LRO=LRO, Z=Z, H=H, Bsb=list(self.bsb), Wz=Wz, Wzw=Wzw, cv=cv, zu=zu)
        return proof, (gamma, beta, alpha, zeta, v, u)

    def linearise(self, bl, zb, hs, chal):
        """the openings at zeta and w zeta and the linearised polynomial of prove.go:1352-1460 -> (lin, [l, r, o](zeta), zu, W_zeta_omega)"""
        c, n, r = self.c, self.n, self.c.r
        gamma, beta, alpha, zeta = chal
        ev = lambda p: pyref._poly_eval(p, zeta, r)
        zu, Wzw = _open(c, zb, zeta * c.fr_root_of_unity(n) % r)
        l, ro, o = ev(bl["L"]), ev(bl["R"]), ev(bl["O"])
        s1 = (ev(self.can["S1"]) * beta + l + gamma) % r * ((ev(self.can["S2"]) * beta + ro + gamma) % r) % r * zu % r * beta % r * alpha % r
        g = c.fr_gen
        s2 = (beta * zeta + l + gamma) % r * ((beta * zeta % r * g + ro + gamma) % r) % r * ((beta * zeta % r * g % r * g + o + gamma) % r) % r
        s2 = (-s2) * alpha % r
        zn = pow(zeta, n, r)
        zn2, zh = zn * zeta % r * zeta % r, (zn - 1) % r
        a2l1 = zh * finv(zeta - 1, r) % r * alpha % r * alpha % r * pow(n, -1, r) % r
        qz = [ev(q) for q in self.qcp]
        lin = []
        for i in range(len(zb)):
            t = zb[i] * s2 % r
            if i < n:
                t += self.can["S3"][i] * s1 + self.can["Qm"][i] * l % r * ro + self.can["Ql"][i] * l + self.can["Qr"][i] * ro + self.can["Qo"][i] * o + self.qk_key[i]
                t += sum(p[i] * q for p, q in zip(self.pi2, qz))
            t = (t + zb[i] * a2l1) % r
            if i < len(hs[2]):
                t = (t - ((hs[2][i] * zn2 + hs[1][i]) % r * zn2 + hs[0][i]) % r * zh) % r
            lin.append(t)
        return lin, [l, ro, o], zu, Wzw


@functools.lru_cache(maxsize=None)
def circuit(cname, n, nb_bsb, nb_public):
    return Circuit(pyref.CURVES[cname], n, nb_bsb, nb_public)


@functools.lru_cache(maxsize=None)
def proven(cname, n, nb_bsb, nb_public, seed=0):
    """(circuit, proof, challenges): made once per session and shared; callers copy what they change"""
    cir = circuit(cname, n, nb_bsb, nb_public)
    proof, chal = cir.prove(seed)
    return cir, proof, chal


# ---- to and from the package's arrays ----------------------------------------------------------------------------------------------------
def to_proof(c, proof) -> pv.Proof:
    one = lambda P: g1_to_arr(c, [P])[0]
    return pv.Proof(g1_to_arr(c, proof["LRO"]), one(proof["Z"]), g1_to_arr(c, proof["H"]),
                    g1_to_arr(c, proof["Bsb"]).reshape(len(proof["Bsb"]), 2 * c.fp_limbs), one(proof["Wz"]), fr_to_arr(c, proof["cv"]),
                    one(proof["Wzw"]), fr_to_arr(c, [proof["zu"]])[0])


def chal_arr(c, chals):
    """challenge tuples -> (N, 6, 4)"""
    return np.array([fr_to_arr(c, list(ch)) for ch in chals], dtype=np.uint64).reshape(len(chals), 6, 4)


def copy_proof(proof):
    return {k: (list(v) if isinstance(v, list) else v) for k, v in proof.items()}


def run_scalars(ctx, vk, c, evals, chals, pubs, hashes, on_device=False):
    """ga_plonk_verify_scalars on integer inputs -> (rows as integers [N][W], relation_ok [N]); operands on the host or the device"""
    N, nb, npub = len(evals), vk.nb_bsb, vk.NbPublicVariables
    W = 2 * (NP_FIXED + nb) + 2
    ev = fr_to_arr(c, [x for e in evals for x in e])
    ch = fr_to_arr(c, [x for e in chals for x in e])
    pub = fr_to_arr(c, [x for e in pubs for x in e]) if npub else np.zeros((0, 4), np.uint64)
    hs = fr_to_arr(c, [x for e in hashes for x in e]) if nb else np.zeros((0, 4), np.uint64)
    pts = np.zeros((N * (NP_FIXED + nb), 2 * c.fp_limbs), dtype=np.uint64)     # (not read by the scalar side, but never null)
    a = _lib.PlonkProofs()
    lib = ctx.lib
    rows = np.zeros((N * W, 4), dtype=np.uint64)
    rel = np.zeros(N, dtype=np.uint8)
    if not on_device:
        a.points, a.evals, a.challenges = pts.ctypes.data, ev.ctypes.data, ch.ctypes.data
        a.public_inputs = pub.ctypes.data if npub else None
        a.bsb_hashes = hs.ctypes.data if nb else None
        lib.check(lib.ga_plonk_verify_scalars(vk.handle, C.byref(a), N, 0, rows.ctypes.data_as(C.c_void_p), rel.ctypes.data_as(C.c_void_p)))
    else:
        bufs = [ctx.to_device(x) for x in (pts, ev, ch, pub if npub else np.zeros((1, 4), np.uint64), hs if nb else np.zeros((1, 4), np.uint64))]
        d_rows, d_rel = ctx.malloc(rows.nbytes), ctx.malloc(max(N, 8))
        try:
            a.points, a.evals, a.challenges, a.public_inputs, a.bsb_hashes = (b.ptr for b in bufs)
            lib.check(lib.ga_plonk_verify_scalars(vk.handle, C.byref(a), N, _lib.PLONK_ON_DEVICE, C.c_void_p(d_rows.ptr), C.c_void_p(d_rel.ptr)))
            rows, rel = d_rows.to_host((N * W, 4)), d_rel.to_host((N,), dtype=np.uint8)
        finally:
            for b in bufs + [d_rows, d_rel]:
                b.free()
    got = arr_to_fr(c, rows)
    return [got[j * W:(j + 1) * W] for j in range(N)], [bool(x) for x in rel]


def random_inputs(c, n, nb_bsb, nb_public, count, seed):
    rng = pyref.Xoshiro(seed)
    f = lambda k: [rng.field(c.r) for _ in range(k)]
    return [f(7 + nb_bsb) for _ in range(count)], [f(6) for _ in range(count)], [f(nb_public) for _ in range(count)], [f(nb_bsb) for _ in range(count)]


def blank_key(c, n, nb_bsb, nb_public, cci=None):
    """a key whose points are all the generator: the scalar side reads none of them"""
    return Key(c, n, nb_public, list(range(nb_bsb)) if cci is None else cci, [c.g1] * 3, c.g1, c.g1, c.g1, c.g1, c.g1, [c.g1] * nb_bsb, c.g1, srs_g2(c))


def check_rows(ctx, c, n, nb_bsb, nb_public, evals, chals, pubs, hashes, on_device=False, cci=None):
    """the rows and relation_ok of the device against the model, bit for bit"""
    key = blank_key(c, n, nb_bsb, nb_public, cci)
    vk = key.device(ctx)
    try:
        rows, rel = run_scalars(ctx, vk, c, evals, chals, pubs, hashes, on_device)
    finally:
        vk.close()
    for j in range(len(evals)):
        ok, want = model_rows(c, n, nb_public, key.cci, evals[j], chals[j], pubs[j], hashes[j])
        assert rows[j] == want, (c.name, n, nb_bsb, nb_public, j, [i for i, (a, b) in enumerate(zip(rows[j], want)) if a != b])
        assert rel[j] == ok, (c.name, n, nb_bsb, nb_public, j)
    return rows, rel


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def rows_combos(n, nb_bsb):
    """(nb_public, count, operands on the device): every nb_public of {0, 1, 3, n - nb_bsb} and every count of {1, 3, 65, 257} (a wave and
    a block are crossed) with host and with device operands"""
    full = n - nb_bsb
    return [(0, 257, False), (1, 65, True), (3, 3, False), (full, 1, True), (3, 257, True), (full, 65, False), (1, 1, False), (0, 3, True),
            (full, 3, False), (1, 257, True), (3, 65, False), (0, 1, True), (0, 65, False), (1, 3, True), (3, 1, True), (full, 257, False)]


def case_rows(ctx, c, n, nb_bsb):
    for k, (nb_public, count, on_device) in enumerate(rows_combos(n, nb_bsb)):
        if nb_public == n - nb_bsb and count == 257:
            count_inputs = random_inputs(c, n, nb_bsb, nb_public, 5, 77 + k)      # (a full row of public inputs: five distinct proofs tiled)
            inputs = tuple([v[j % 5] for j in range(count)] for v in count_inputs)
        else:
            inputs = random_inputs(c, n, nb_bsb, nb_public, count, 77 + k)
        check_rows(ctx, c, n, nb_bsb, nb_public, *inputs, on_device=on_device)


def case_edges(ctx, c):
    """zeta on and off the domain's special points, zero challenges, a zero public input: n = 8, three public inputs, one BSB22 hash at
    row 3 + 2 = 5; rows 0-2 carry public terms, row 5 the hash, row 7 nothing"""
    n, nb_bsb, nb_public, cci = 8, 1, 3, [2]
    w = c.fr_root_of_unity(n)
    ev, ch, pub, hs = random_inputs(c, n, nb_bsb, nb_public, 10, 4242)
    G, B, A, Zt, V, U = range(6)
    ch[0][Zt] = 1
    ch[1][Zt] = w                      # a public row
    ch[2][Zt] = pow(w, 5, c.r)         # the BSB22 row
    ch[3][Zt] = pow(w, 7, c.r)         # a row that carries no term
    ch[4][Zt] = 0
    ch[5][A] = 0
    ch[6][V] = 0
    ch[7][U] = 0
    pub[8] = [0, 0, 0]
    ch[9][Zt], ch[9][A], ch[9][V], ch[9][U] = pow(w, 2, c.r), 0, 0, 0
    for on_device in (False, True):
        check_rows(ctx, c, n, nb_bsb, nb_public, ev, ch, pub, hs, on_device=on_device, cci=cci)


def case_acceptance(ctx, cname, n, nb_bsb, nb_public):
    c = pyref.CURVES[cname]
    cir, proof, chal = proven(cname, n, nb_bsb, nb_public)
    assert model_verify(c, cir.key, proof, cir.pub, chal) == (True, True)
    vk = cir.key.device(ctx)
    try:
        assert pv.Verify(ctx, vk, to_proof(c, proof), cir.pub, chal_arr(c, [chal])[0])
        assert np.array_equal(pv.BsbHashes(c.cid, to_proof(c, proof).Bsb22Commitments, lib=ctx.lib).reshape(-1, 4), fr_to_arr(c, cir.hashes).reshape(-1, 4))
    finally:
        vk.close()


def tampered(c, cir, proof, chal):
    """(name, proof, public inputs, challenges, hashes) with each field changed in turn: every point replaced by another point of the
    subgroup, every evaluation, one public input, one hash, every challenge"""
    G1 = pyref.g1_group(c)
    out = []
    shift = lambda P: G1.add(P, c.g1)
    for name in ("LRO", "H", "Bsb"):
        for i in range(len(proof[name])):
            p = copy_proof(proof)
            p[name][i] = shift(p[name][i])
            out.append(("%s[%d]" % (name, i), p, cir.pub, chal, cir.hashes))
    for name in ("Z", "Wz", "Wzw"):
        p = copy_proof(proof)
        p[name] = shift(p[name])
        out.append((name, p, cir.pub, chal, cir.hashes))
    for i in range(len(proof["cv"])):
        p = copy_proof(proof)
        p["cv"][i] = (p["cv"][i] + 1) % c.r
        out.append(("cv[%d]" % i, p, cir.pub, chal, cir.hashes))
    p = copy_proof(proof)
    p["zu"] = (p["zu"] + 1) % c.r
    out.append(("zu", p, cir.pub, chal, cir.hashes))
    if cir.pub:
        out.append(("public", proof, [(cir.pub[0] + 1) % c.r] + cir.pub[1:], chal, cir.hashes))
    if cir.hashes:
        out.append(("hash", proof, cir.pub, chal, [(cir.hashes[0] + 1) % c.r] + cir.hashes[1:]))
    for i, name in enumerate(("gamma", "beta", "alpha", "zeta", "v", "u")):
        ch = list(chal)
        ch[i] = (ch[i] + 1) % c.r
        out.append((name, proof, cir.pub, tuple(ch), cir.hashes))
    return out


def verify_list(ctx, vk, c, items, **kw):
    """VerifyMany over (proof, public inputs, challenges, hashes) tuples -> (verdicts, relation_ok)"""
    nb = vk.nb_bsb
    hashes = [fr_to_arr(c, h) if nb else np.zeros((0, 4), np.uint64) for _, _, _, h in items]
    return pv.VerifyMany(ctx, vk, [to_proof(c, p) for p, _, _, _ in items], [pub for _, pub, _, _ in items], chal_arr(c, [ch for _, _, ch, _ in items]),
                         hashes, detail=True, **kw)


def case_tamper(ctx, cname, full_model):
    """n = 16, two BSB22 commitments, three public inputs: 11 points, 9 evaluations, a public input, a hash, 6 challenges"""
    c = pyref.CURVES[cname]
    cir, proof, chal = proven(cname, 16, 2, 3)
    cases = tampered(c, cir, proof, chal)
    assert len(cases) == 11 + 9 + 1 + 1 + 6
    vk = cir.key.device(ctx)
    try:
        items = [(proof, cir.pub, chal, cir.hashes)] + [t[1:] for t in cases]
        ok, rel = verify_list(ctx, vk, c, items)
    finally:
        vk.close()
    assert ok[0] and rel[0]
    for k, (name, p, pub, ch, hs) in enumerate(cases, 1):
        if name == "u":
            # u is the scalar kzg.BatchVerifyMultiPoints draws from crypto/rand to batch the two openings: both openings of a valid
            # proof hold on their own, so the batched check holds for EVERY u and the reference accepts.  Another u cannot reject a
            # valid proof; the verdict must be the model's, which is to accept.
            assert model_verify(c, cir.key, p, pub, ch, hs) == (True, True) and ok[k] and rel[k]
            continue
        assert not ok[k], name
        want_rel, _ = model_scalars(c, cir.n, cir.nb_public, cir.cci, list(p["cv"]) + [p["zu"]], ch, pub, hs)
        assert bool(rel[k]) == want_rel, name
        if full_model:
            assert model_verify(c, cir.key, p, pub, ch, hs) == (False, want_rel), name


def distinct_proofs(cname, k, n=16, nb_bsb=1, nb_public=3):
    cir = circuit(cname, n, nb_bsb, nb_public)
    return cir, [proven(cname, n, nb_bsb, nb_public, seed)[1:] for seed in range(k)]


def off_curve(c, P):
    return (P[0], (P[1] + 1) % c.p)


def case_verify_many(ctx, cname, total):
    """`total` proofs, 8 distinct ones tiled, bad ones at known places (the first and the last among them): the verdict vector is exact"""
    c = pyref.CURVES[cname]
    cir, ps = distinct_proofs(cname, 8)
    items = [(ps[j % 8][0], cir.pub, ps[j % 8][1], cir.hashes) for j in range(total)]
    bad = {0: "cv", total // 2: "point", total // 2 + 3: "off", total - 1: "public"}
    for j, kind in bad.items():
        p, pub, ch, hs = items[j]
        p = copy_proof(p)
        if kind == "cv":
            p["cv"][1] = (p["cv"][1] + 1) % c.r
        elif kind == "point":
            p["Wz"] = pyref.g1_group(c).add(p["Wz"], c.g1)
        elif kind == "off":
            p["H"][1] = off_curve(c, p["H"][1])
        else:
            pub = [(pub[0] + 5) % c.r] + pub[1:]
        items[j] = (p, pub, ch, hs)
    vk = cir.key.device(ctx)
    try:
        ok, rel = verify_list(ctx, vk, c, items)
    finally:
        vk.close()
    assert [j for j in range(total) if not ok[j]] == sorted(bad)
    assert [j for j in range(total) if not rel[j]] == [0, total - 1]          # the relation fails for the evaluation and the public input


def case_batch(ctx, cname):
    c = pyref.CURVES[cname]
    G1 = pyref.g1_group(c)
    cir, ps = distinct_proofs(cname, 4)
    good = [to_proof(c, p) for p, _ in ps]
    chs = chal_arr(c, [ch for _, ch in ps])
    pubs = [cir.pub] * 4
    vk = cir.key.device(ctx)
    try:
        rng = np.random.default_rng(11)
        assert pv.BatchVerify(ctx, vk, good, pubs, chs, rng)
        badp = copy_proof(ps[2][0])
        badp["Wz"] = G1.add(badp["Wz"], c.g1)                   # the relation holds, the pairing does not
        bad = good[:2] + [to_proof(c, badp)] + good[3:]
        assert not pv.BatchVerify(ctx, vk, bad, pubs, chs, rng)
        assert pv.BatchVerify(ctx, vk, bad, pubs, chs, rng, weights=[3, 5, 0, 7])
        assert not pv.BatchVerify(ctx, vk, bad, pubs, chs, rng, weights=[3, 5, 1, 7])
        # two proofs with equal v whose L commitments are off by +T and -T: the sum with weights (1, 1) cancels T, (1, 2) does not
        T = G1.mul(c.g1, 12345)
        plus, minus = copy_proof(ps[0][0]), copy_proof(ps[0][0])
        plus["LRO"][0], minus["LRO"][0] = G1.add(plus["LRO"][0], T), G1.add(minus["LRO"][0], G1.neg(T))
        pair, ch2 = [to_proof(c, plus), to_proof(c, minus)], chal_arr(c, [ps[0][1]] * 2)
        assert pv.BatchVerify(ctx, vk, pair, pubs[:2], ch2, rng, weights=[1, 1])
        assert not pv.BatchVerify(ctx, vk, pair, pubs[:2], ch2, rng, weights=[1, 2])
        assert list(pv.VerifyMany(ctx, vk, pair, pubs[:2], ch2)) == [False, False]
    finally:
        vk.close()


def cofactor_point(c):
    """a point of E(Fp) of order prime to r (BLS12-381: the cofactor of G1 is not 1): [r]R for a curve point R"""
    G1 = pyref.g1_group(c)
    x = 3
    while True:
        y = pyref._sqrt_fp((x * x * x + c.b) % c.p, c.p)
        if y is not None and G1.on_curve((x, y)):
            T = G1.mul((x, y), c.r)
            if T is not None:
                return T
        x += 1


def case_point_checks(ctx, cname):
    c = pyref.CURVES[cname]
    G1 = pyref.g1_group(c)
    cir, ps = distinct_proofs(cname, 3)
    items = [(p, cir.pub, ch, cir.hashes) for p, ch in ps] * 2
    p = copy_proof(items[1][0])
    p["LRO"][2] = off_curve(c, p["LRO"][2])
    items[1] = (p,) + items[1][1:]
    want = [True, False, True, True, True, True]
    if c.name == "bls12-381":
        T = cofactor_point(c)
        assert G1.on_curve(T) and G1.mul(T, c.r) is not None
        p = copy_proof(items[4][0])
        p["Z"] = G1.add(p["Z"], T)                              # on the curve, outside the subgroup
        items[4] = (p,) + items[4][1:]
        want[4] = False
    vk = cir.key.device(ctx)
    try:
        ok, rel = verify_list(ctx, vk, c, items)
        assert list(ok) == want and all(rel)
        if c.name == "bls12-381":
            # Without the point check the shifted point goes through the point stage.  e(P + T, Q) = e(P, Q) for T of order prime to r
            # (the value lies in mu_r and its order divides that of T), so the other proofs keep their verdicts and this one passes
            sub = [items[0], items[4], items[2]]
            ok2, rel2 = verify_list(ctx, vk, c, sub, point_check=False)
            assert all(rel2) and ok2[0] and ok2[2], list(ok2)
            assert ok2[1]
    finally:
        vk.close()


def case_key_files(ctx, c):
    """tests/golden/vk_blank_plonk_*.bin: every byte is decoded, the points are on the curve and in the subgroup, and Size, SizeInv,
    Generator and CosetShift are those of the library's own domain of that size"""
    import os
    from gnark_amd import ecc, fft
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    for name, nq in (("nocommit", 0), ("commit", 1)):
        raw = open(os.path.join(gold, "vk_blank_plonk_%s_%s.bin" % (c.name.replace("-", ""), name)), "rb").read()
        vk, used = pv.VerifyingKey.ReadFrom(c.cid, raw, lib=ctx.lib)
        assert used == len(raw) and vk.nb_bsb == nq == len(vk.CommitmentConstraintIndexes)
        assert len(vk.Lines) % (4 * 4 * c.fp_bytes) == 0 and len(vk.Lines) > 0      # [2][2][k] lines of two Fp2 values each
        g1 = np.concatenate([vk.S, [vk.Ql, vk.Qr, vk.Qm, vk.Qo, vk.Qk], vk.Qcp, [vk.KzgG1]])
        assert ecc.CheckPoints(ctx, c.cid, 0, g1)[3] == ecc.NONE_BAD and ecc.CheckPoints(ctx, c.cid, 1, vk.KzgG2)[3] == ecc.NONE_BAD
        assert np.array_equal(vk.KzgG1, g1_to_arr(c, [c.g1])[0]) and np.array_equal(vk.KzgG2[0], g2_to_arr(c, [c.g2])[0])
        n = vk.Size
        assert n == (8 if name == "nocommit" else 16)
        d = fft.Domain(ctx, c.name, n)
        try:
            e = [0] * n
            e[n // 2] = 1                                                           # bitrev(1)
            assert arr_to_fr(c, d.FFT(fr_to_arr(c, e), fft.DIT))[1] == vk.Generator
            e = [0] * n
            e[1] = 1
            assert arr_to_fr(c, d.FFT(fr_to_arr(c, e), fft.DIF, True))[0] == vk.CosetShift
            assert arr_to_fr(c, d.FFTInverse(fr_to_arr(c, [1] + [0] * (n - 1)), fft.DIF))[0] == vk.SizeInv
        finally:
            d.close()
        vk.Pin(ctx)          # the key of the file is accepted by the device
        vk.close()
        for cut in (len(raw) - 1, 100):
            try:
                pv.VerifyingKey.ReadFrom(c.cid, raw[:cut], lib=ctx.lib)
            except (ValueError, _lib.GnarkAmdError):
                continue
            raise AssertionError("a truncated key was read")


def case_errors(ctx, c):
    """every GA_ERR_INVALID of the header, each followed by a successful call; count = 0; a BLS12-377 domain; an allocation failure"""
    import os
    from gnark_amd import fft
    lib = ctx.lib
    cir, proof, chal = proven(c.name, 4, 1, 0)
    vk = cir.key.device(ctx)
    items = [(proof, cir.pub, chal, cir.hashes)]

    def good():
        ok, rel = verify_list(ctx, vk, c, items)
        assert ok[0] and rel[0]

    def refused(rc, word="ga_plonk"):
        assert rc == -1 and word in lib.ga_last_error().decode(), (rc, lib.ga_last_error())
        good()

    try:
        good()
        w1 = 2 * c.fp_limbs
        pts, ev, ch, pub, hs, _ = pv._pack(vk, [to_proof(c, proof)], [cir.pub], chal_arr(c, [chal]), [fr_to_arr(c, cir.hashes)], lib)
        a = _lib.PlonkProofs()
        a.points, a.evals, a.challenges, a.bsb_hashes = pts.ctypes.data, ev.ctypes.data, ch.ctypes.data, np.ascontiguousarray(hs).ctypes.data
        ok, rel, out2 = np.zeros(1, np.uint8), np.zeros(1, np.uint8), (C.c_uint64 * 2)()
        okp, relp = ok.ctypes.data_as(C.c_void_p), rel.ctypes.data_as(C.c_void_p)
        rows = np.zeros((2 * 10 + 2, 4), np.uint64)
        rowsp = rows.ctypes.data_as(C.c_void_p)
        # null pointers
        refused(lib.ga_plonk_verify(None, C.byref(a), 1, 0, None, okp, relp, out2))
        refused(lib.ga_plonk_verify(vk.handle, None, 1, 0, None, okp, relp, out2))
        refused(lib.ga_plonk_verify(vk.handle, C.byref(a), 1, 0, None, None, relp, out2))
        refused(lib.ga_plonk_verify(vk.handle, C.byref(a), 1, 0, None, okp, relp, None), "out2")
        refused(lib.ga_plonk_verify_scalars(vk.handle, C.byref(a), 1, 0, None, relp))
        refused(lib.ga_plonk_verify_scalars(vk.handle, C.byref(a), 1, 0, rowsp, None))
        b = _lib.PlonkProofs()
        for fld in ("points", "evals", "challenges", "bsb_hashes"):
            for f2 in ("points", "evals", "challenges", "bsb_hashes"):
                setattr(b, f2, None if f2 == fld else getattr(a, f2))
            refused(lib.ga_plonk_verify(vk.handle, C.byref(b), 1, 0, None, okp, relp, out2))
            refused(lib.ga_plonk_verify_scalars(vk.handle, C.byref(b), 1, 0, rowsp, relp))
        # combined mode without weights
        refused(lib.ga_plonk_verify(vk.handle, C.byref(a), 1, _lib.PLONK_VERIFY_COMBINED, None, okp, relp, out2), "weights")
        # count = 0 touches nothing, whatever else is passed
        assert lib.ga_plonk_verify(vk.handle, None, 0, 0, None, None, None, None) == 0
        assert lib.ga_plonk_verify_scalars(vk.handle, None, 0, 0, None, None) == 0
        # the key's own refusals
        d = fft.Domain(ctx, c.name, 8)
        pt = g1_to_arr(c, [c.g1])
        g2 = g2_to_arr(c, srs_g2(c))
        qcp = g1_to_arr(c, [c.g1] * 17)

        def make(nb_public, nb_bsb, cci, null=None, dom=None):
            k = _lib.PlonkVkIn()
            k.nb_public, k.nb_bsb = nb_public, nb_bsb
            idx = np.array(list(cci) + [0], dtype=np.uint64)
            k.commitment_constraint_indexes = idx.ctypes.data
            for f in ("ql", "qr", "qm", "qo", "qk", "s1", "s2", "s3", "kzg_g1"):
                setattr(k, f, pt.ctypes.data)
            k.qcp, k.kzg_g2 = qcp.ctypes.data, g2.ctypes.data
            if null:
                setattr(k, null, None)
            h = C.c_void_p()
            rc = lib.ga_plonk_vk_create((dom or d).handle, C.byref(k), C.byref(h))
            if rc == 0:
                lib.ga_plonk_vk_destroy(h)
            return rc

        try:
            assert make(3, 2, [0, 4]) == 0
            refused(make(3, 17, list(range(17))), "nb_bsb")
            refused(make(7, 2, [0, 0]), "nb_public")
            refused(make(9, 0, []), "nb_public")
            refused(make(3, 2, [0, 5]), "commitment_constraint_indexes")
            for f in ("ql", "s3", "kzg_g1", "kzg_g2", "qcp", "commitment_constraint_indexes"):
                refused(make(3, 1, [0], null=f))
            assert make(3, 0, [], null="qcp") == 0
            refused(lib.ga_plonk_vk_create(None, None, None))
        finally:
            d.close()
        d377 = fft.Domain(ctx, "bls12-377", 8)
        try:
            rc = make(0, 0, [], dom=d377)
            assert rc == -1 and "ga_plonk_vk_create" in lib.ga_last_error().decode() and "bls12-377" in lib.ga_last_error().decode()
            good()
        finally:
            d377.close()
        # an allocation failure deep inside the call: an error code, then the same call gives the same result
        os.environ["GA_FAULT_THROW"] = "ga_plonk_verify"
        try:
            rc = lib.ga_plonk_verify(vk.handle, C.byref(a), 1, 0, None, okp, relp, out2)
        finally:
            del os.environ["GA_FAULT_THROW"]
        assert rc == -3 and "ga_plonk_verify" in lib.ga_last_error().decode()
        assert lib.ga_plonk_verify(vk.handle, C.byref(a), 1, 0, None, okp, relp, out2) == 0
        assert ok[0] == 1 and rel[0] == 1 and (out2[0], out2[1]) == (0, 0xFFFFFFFFFFFFFFFF)
        good()
    finally:
        vk.close()


def case_device_loop(ctx, cname):
    """One proof whose every polynomial step is a DEVICE call -- ga_plonk_build_z, ga_plonk_quotient, the table MSM for every commitment,
    ga_fr_poly_evaluate, ga_fr_linear_combination (the linearised and the folded polynomial), ga_kzg_open (both openings) -- accepted by
    the model and by the device verifier: blinding, the order of ClaimedValues and the n + 2 shards of h agree between the calls."""
    from gnark_amd import ecc, fft, plonk
    from helpers import arr_to_g1_affine
    c = pyref.CURVES[cname]
    r, n = c.r, 16
    cir = circuit(cname, n, 1, 3)
    key, G1 = cir.key, pyref.g1_group(c)
    M = n + 3                                                  # the longest polynomial: the blinded Z and the linearised one
    srs = [G1.mul(c.g1, pow(TAU, i, r)) for i in range(M)]
    table = ecc.PrecomputedBases(ctx, c.name, 0, g1_to_arr(c, srs))
    d0, d1 = fft.Domain(ctx, c.name, n), fft.Domain(ctx, c.name, pyref.plonk_rho(n) * n)
    pad = lambda p: fr_to_arr(c, list(p) + [0] * (M - len(p)))
    to_pt = lambda jac: arr_to_g1_affine(c, ecc.jac_to_affine(c.cid, 0, jac, lib=ctx.lib))
    commit = lambda p: to_pt(table.MultiExp(pad(p)))
    fr1 = lambda x: fr_to_arr(c, [x])
    ev_at = lambda p, z: arr_to_fr(c, plonk.Evaluate(ctx, c.name, pad(p), fr1(z)))[0]
    try:
        rng = pyref.Xoshiro(31337)
        bp = {k: [rng.field(r) for _ in range(3 if k == "Bz" else 2)] for k in ("Bl", "Br", "Bo", "Bz")}
        bl = {k: _blinded(c, n, cir.can[k], bp["B" + k.lower()]) for k in ("L", "R", "O")}
        LRO = [commit(bl[k]) for k in ("L", "R", "O")]
        assert LRO[0] == _commit(c, bl["L"])
        bind = [point_bytes(c, P) for P in key.S + [key.Ql, key.Qr, key.Qm, key.Qo, key.Qk] + key.Qcp] + list(cir.pub)
        gamma = challenge(c, "gamma", *bind, *[point_bytes(c, P) for P in LRO])
        beta = challenge(c, "beta", gamma)
        Zl = arr_to_fr(c, plonk.BuildRatioCopyConstraint(d0, fr_to_arr(c, cir.lag["L"]), fr_to_arr(c, cir.lag["R"]), fr_to_arr(c, cir.lag["O"]), cir.perm,
                                                         fr1(beta), fr1(gamma)))
        zc = _canonical(c, n, Zl)
        zb = _blinded(c, n, zc, bp["Bz"])
        Z = commit(zb)
        alpha = challenge(c, "alpha", beta, *[point_bytes(c, P) for P in cir.bsb + [Z]])
        polys = {k: fr_to_arr(c, v) for k, v in dict(cir.can, Z=zc).items()}
        h = arr_to_fr(c, plonk.ComputeQuotient(d0, d1, polys, [fr_to_arr(c, q) for q in cir.qcp], [fr_to_arr(c, p) for p in cir.pi2],
                                               bp={k: fr_to_arr(c, v) for k, v in bp.items()}, alpha=fr1(alpha), beta=fr1(beta), gamma=fr1(gamma)))
        assert not any(h[3 * (n + 2):])
        hs = [h[i * (n + 2):(i + 1) * (n + 2)] for i in range(3)]
        H = [commit(s) for s in hs]
        zeta = challenge(c, "zeta", alpha, *[point_bytes(c, P) for P in H])
        # the openings and the scalars of the linearised polynomial (prove.go:1352-1460)
        zu_arr, wzw = table.KzgOpen(pad(zb), fr1(zeta * c.fr_root_of_unity(n) % r))
        zu, Wzw = arr_to_fr(c, zu_arr)[0], to_pt(wzw)
        l, ro, o = ev_at(bl["L"], zeta), ev_at(bl["R"], zeta), ev_at(bl["O"], zeta)
        s1z, s2z, qz = ev_at(cir.can["S1"], zeta), ev_at(cir.can["S2"], zeta), [ev_at(q, zeta) for q in cir.qcp]
        g = c.fr_gen
        s1 = (s1z * beta + l + gamma) % r * ((s2z * beta + ro + gamma) % r) % r * zu % r * beta % r * alpha % r
        s2 = (beta * zeta + l + gamma) % r * ((beta * zeta % r * g + ro + gamma) % r) % r * ((beta * zeta % r * g % r * g + o + gamma) % r) % r
        s2 = (-s2) * alpha % r
        zn = pow(zeta, n, r)
        zn2, zh = zn * zeta % r * zeta % r, (zn - 1) % r
        a2l1 = zh * finv(zeta - 1, r) % r * alpha % r * alpha % r * pow(n, -1, r) % r
        terms = [((s2 + a2l1) % r, zb), (s1, cir.can["S3"]), (l * ro % r, cir.can["Qm"]), (l, cir.can["Ql"]), (ro, cir.can["Qr"]), (o, cir.can["Qo"]),
                 (1, cir.qk_key), ((-zh) % r, hs[0]), ((-zh * zn2) % r, hs[1]), ((-zh * zn2 % r * zn2) % r, hs[2])] + list(zip(qz, cir.pi2))
        lin = arr_to_fr(c, plonk.LinearCombination(ctx, c.name, fr_to_arr(c, [s for s, _ in terms]), [pad(p) for _, p in terms]))
        assert lin == cir.linearise(bl, zb, hs, (gamma, beta, alpha, zeta))[0]
        opened = [lin, bl["L"], bl["R"], bl["O"], cir.can["S1"], cir.can["S2"]] + cir.qcp
        cv = [ev_at(p, zeta) for p in opened]
        v = challenge(c, "fold", zeta, zu, *cv)
        folded = plonk.LinearCombination(ctx, c.name, fr_to_arr(c, [pow(v, k, r) for k in range(len(opened))]), [pad(p) for p in opened])
        _, wz = table.KzgOpen(folded, fr1(zeta))
        Wz = to_pt(wz)
        u = challenge(c, "batch", v, point_bytes(c, Wz), point_bytes(c, Wzw))
    finally:
        table.free()
        d0.close()
        d1.close()
    proof, chal = dict(LRO=LRO, Z=Z, H=H, Bsb=list(cir.bsb), Wz=Wz, Wzw=Wzw, cv=cv, zu=zu), (gamma, beta, alpha, zeta, v, u)
    assert model_verify(c, key, proof, cir.pub, chal) == (True, True)
    vk = key.device(ctx)
    try:
        assert pv.Verify(ctx, vk, to_proof(c, proof), cir.pub, chal_arr(c, [chal])[0])      # (the hashes: BsbHashes on the device library's host code)
        bad = copy_proof(proof)
        bad["H"][2] = G1.add(bad["H"][2], c.g1)
        assert not pv.Verify(ctx, vk, to_proof(c, bad), cir.pub, chal_arr(c, [chal])[0])
    finally:
        vk.close()
