"""plonk.Verify on the device (backend/plonk/bn254/verify.go:36-323): the verifying key as gnark writes it, and three verifiers over
ga_plonk_verify -- Verify (one proof), VerifyMany (N proofs under one key, one exact verdict each, one pairing pass of N groups) and
BatchVerify (the randomised check of N proofs: two MSMs, two Miller loops and one final exponentiation).

NOT computed here: the Fiat-Shamir challenges.  gamma, beta, alpha and zeta come from gnark-crypto's fiatshamir transcript, v from
kzg.FoldProof's, u from crypto/rand inside kzg.BatchVerifyMultiPoints; the caller supplies the six values per proof, the same division
as on the prover side (Fiat-Shamir, folding and linearisation stay in Go).  The BSB22 hashes of verify.go:162-175 are BsbHashes."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .device import Context, _ptr, affine_words, as_u64, curve_id
from .ecc import G1, G2
from .fft import Domain
from .g16_setup import FR_MODULUS
from .groth16 import HashToField, MarshalG1

BSB22_DST = b"BSB22-Plonk"                                   # verify.go:163
KEY_VERSION_MARKER = 0                                      # marshal.go: a versioned key starts with the marker, then the version
FR_DOMAIN = {_lib.BN254: (5, 28), _lib.BLS12_381: (7, 32)}   # fft.Domain's FrMultiplicativeGen and the 2-adicity of r - 1
FIXED_POINTS = 9                                             # L R O Z H0 H1 H2 W_zeta W_zeta_omega, then the BSB22 commitments
NB_CHALLENGES = 6                                            # gamma beta alpha zeta v u


def domain_constants(cid: int, n: int):
    """(SizeInv, Generator, CosetShift) of fft.NewDomain(n), canonical integers"""
    r = FR_MODULUS[cid]
    gen, adicity = FR_DOMAIN[cid]
    wmax = pow(gen, (r - 1) >> adicity, r)
    return pow(n, -1, r), pow(wmax, (1 << adicity) // n, r), gen


def fr_mont(cid: int, values) -> np.ndarray:
    """canonical integers -> (n, 4) fr.Element images (Montgomery)"""
    r = FR_MODULUS[cid]
    out = np.zeros((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        m = (int(v) % r << 256) % r
        out[i] = [(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
    return out


@dataclass
class VerifyingKey:
    """plonk.VerifyingKey (backend/plonk/bn254/setup.go): affine images, Montgomery limbs; field elements as canonical integers"""
    curve: int
    Size: int
    SizeInv: int
    Generator: int
    NbPublicVariables: int
    CosetShift: int
    S: np.ndarray                     # (3, 2 fp)
    Ql: np.ndarray
    Qr: np.ndarray
    Qm: np.ndarray
    Qo: np.ndarray
    Qk: np.ndarray
    Qcp: np.ndarray                   # (nb_bsb, 2 fp)
    KzgG1: np.ndarray
    KzgG2: np.ndarray                 # (2, 4 fp)
    CommitmentConstraintIndexes: list = field(default_factory=list)
    Lines: bytes = b""                # vk.Kzg.Lines as written: the precomputed lines of gnark-crypto's fixed-argument pairing, not used here
    version: int = 0                  # 0: the legacy layout without the marker
    domain: Domain = None
    handle: C.c_void_p = None

    @classmethod
    def ReadFrom(cls, curve, data: bytes, lib=None):
        """VerifyingKey.ReadFrom (marshal.go:177-203 / :229-300), compressed or raw points, with or without the version marker: Size,
        SizeInv, Generator, NbPublicVariables, CosetShift, S[0..2], Ql, Qr, Qm, Qo, Qk, u32 len + Qcp, Kzg.G1, Kzg.G2[0], Kzg.G2[1],
        Kzg.Lines, u32 len + CommitmentConstraintIndexes.  Kzg.Lines is kept as bytes: it is what lies between G2[1] and the indexes,
        whose number is len(Qcp) (verify.go:45).  Returns (key, bytes read).  The domain fields must be fft.NewDomain(Size)'s."""
        lib = lib or _lib.load()
        cid = curve_id(curve)
        if cid not in FR_DOMAIN:
            raise ValueError("plonk verifying key: bn254 and bls12-381 only (no pairing for this curve)")
        data = bytes(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        off = 0

        def uint(nbytes):
            nonlocal off
            if off + nbytes > len(data):
                raise ValueError("plonk verifying key: truncated")
            v = int.from_bytes(data[off:off + nbytes], "big")
            off += nbytes
            return v

        def point(group):
            nonlocal off
            out = np.zeros(affine_words(cid, group), dtype=np.uint64)
            used = C.c_size_t()
            lib.check(lib.ga_point_unmarshal(cid, group, C.c_void_p(buf.ctypes.data + off), len(data) - off, _ptr(out), C.byref(used)))
            off += used.value
            return out

        version, size = 0, uint(8)
        if size == KEY_VERSION_MARKER:
            version, size = uint(8), uint(8)
            if version != 1:
                raise ValueError(f"plonk verifying key: unsupported serialization version {version}")
        size_inv, gen, nb_public, shift = uint(32), uint(32), uint(8), uint(32)
        if size == 0 or size & (size - 1) or size > (1 << FR_DOMAIN[cid][1]) or (size_inv, gen, shift) != domain_constants(cid, size):
            raise ValueError("plonk verifying key: Size, SizeInv, Generator or CosetShift is not fft.NewDomain(Size)'s")
        S = np.array([point(G1) for _ in range(3)], dtype=np.uint64)
        ql, qr, qm, qo, qk = (point(G1) for _ in range(5))
        nq = uint(4)
        qcp = np.array([point(G1) for _ in range(nq)], dtype=np.uint64).reshape(nq, affine_words(cid, G1))
        g1 = point(G1)
        g2 = np.array([point(G2), point(G2)], dtype=np.uint64)
        tail = 4 + 8 * nq
        if len(data) - off < tail:
            raise ValueError("plonk verifying key: truncated")
        lines = data[off:len(data) - tail]
        off = len(data) - tail
        if uint(4) != nq:
            raise ValueError("plonk verifying key: len(CommitmentConstraintIndexes) != len(Qcp)")
        cci = [uint(8) for _ in range(nq)]
        return cls(cid, size, size_inv, gen, nb_public, shift, S, ql, qr, qm, qo, qk, qcp, g1, g2, cci, lines, version), off

    @property
    def nb_bsb(self) -> int:
        return int(self.Qcp.shape[0])

    def Pin(self, ctx: Context):
        """the key on the device (ga_plonk_vk_create) with its own size-n domain; close() frees both"""
        if self.handle:
            return self
        w1 = affine_words(self.curve, G1)
        self.domain = Domain(ctx, self.curve, self.Size)
        keep = {k: as_u64(np.asarray(v).reshape(-1, w1), w1) for k, v in
                (("ql", self.Ql), ("qr", self.Qr), ("qm", self.Qm), ("qo", self.Qo), ("qk", self.Qk), ("s1", self.S[0]), ("s2", self.S[1]),
                 ("s3", self.S[2]), ("kzg_g1", self.KzgG1))}
        keep["qcp"] = as_u64(np.asarray(self.Qcp).reshape(-1, w1), w1)
        keep["kzg_g2"] = as_u64(np.asarray(self.KzgG2).reshape(2, -1), affine_words(self.curve, G2))
        cci = np.array(list(self.CommitmentConstraintIndexes) or [0], dtype=np.uint64)
        a = _lib.PlonkVkIn()
        a.nb_public, a.nb_bsb = self.NbPublicVariables, len(self.CommitmentConstraintIndexes)
        a.commitment_constraint_indexes = cci.ctypes.data
        for k, v in keep.items():
            setattr(a, k, v.ctypes.data if v.size else None)
        if len(self.CommitmentConstraintIndexes) != self.nb_bsb:      # verify.go:45
            self.domain.close()
            raise ValueError("plonk verifying key: len(CommitmentConstraintIndexes) != len(Qcp)")
        h = C.c_void_p()
        try:
            ctx.lib.check(ctx.lib.ga_plonk_vk_create(self.domain.handle, C.byref(a), C.byref(h)))
        except Exception:
            self.domain.close()
            self.domain = None
            raise
        self.handle = h
        return self

    def close(self):
        if self.handle:
            self.domain.ctx.lib.ga_plonk_vk_destroy(self.handle)
            self.handle = None
        if self.domain:
            self.domain.close()
            self.domain = None


@dataclass
class Proof:
    """plonk.Proof (backend/plonk/bn254/prove.go:55-75) as arrays: G1Affine images and fr.Element images (Montgomery)"""
    LRO: np.ndarray                   # (3, 2 fp)
    Z: np.ndarray
    H: np.ndarray                     # (3, 2 fp)
    Bsb22Commitments: np.ndarray      # (nb_bsb, 2 fp)
    BatchedProofH: np.ndarray         # BatchedProof.H: the opening proof at zeta
    ClaimedValues: np.ndarray         # (6 + nb_bsb, 4): BatchedProof.ClaimedValues
    ZShiftedH: np.ndarray             # ZShiftedOpening.H
    ZShiftedClaimedValue: np.ndarray  # (4,)

    def points(self, w1: int) -> np.ndarray:
        rows = [np.asarray(self.LRO).reshape(3, w1), np.asarray(self.Z).reshape(1, w1), np.asarray(self.H).reshape(3, w1),
                np.asarray(self.BatchedProofH).reshape(1, w1), np.asarray(self.ZShiftedH).reshape(1, w1),
                np.asarray(self.Bsb22Commitments, dtype=np.uint64).reshape(-1, w1)]
        return np.concatenate(rows).astype(np.uint64)

    def evals(self) -> np.ndarray:
        return np.concatenate([np.asarray(self.ClaimedValues, dtype=np.uint64).reshape(-1, 4), np.asarray(self.ZShiftedClaimedValue, dtype=np.uint64).reshape(1, 4)])


def BsbHashes(curve, commitments, lib=None) -> np.ndarray:
    """verify.go:162-175: fr.Hash(commitment.Marshal(), "BSB22-Plonk", 1) of every BSB22 commitment -> (nb_bsb, 4) fr images"""
    cid = curve_id(curve)
    com = np.asarray(commitments, dtype=np.uint64).reshape(-1, affine_words(cid, G1))
    out = np.zeros((com.shape[0], 4), dtype=np.uint64)
    for i in range(com.shape[0]):
        out[i] = HashToField(cid, MarshalG1(cid, com[i], lib=lib), BSB22_DST, 1, lib=lib)[0]
    return out


def _pack(vk: VerifyingKey, proofs, public_witnesses, challenges, hashes, lib):
    """the five arrays of ga_plonk_proofs; None where a proof has the wrong shape (verify.go:45-59)"""
    cid = vk.curve
    w1, nb, npub = affine_words(cid, G1), vk.nb_bsb, vk.NbPublicVariables
    N = len(proofs)
    pts = np.zeros((N, FIXED_POINTS + nb, w1), dtype=np.uint64)
    ev = np.zeros((N, 7 + nb, 4), dtype=np.uint64)
    pub = np.zeros((N, max(npub, 1), 4), dtype=np.uint64)
    hs = np.zeros((N, max(nb, 1), 4), dtype=np.uint64)
    shaped = np.ones(N, dtype=bool)
    for i, p in enumerate(proofs):
        pp, pe = p.points(w1), p.evals()
        if pp.shape[0] != FIXED_POINTS + nb or pe.shape[0] != 7 + nb or len(public_witnesses[i]) != npub:
            shaped[i] = False
            continue
        pts[i], ev[i] = pp, pe
        if npub:
            pub[i, :npub] = fr_mont(cid, public_witnesses[i])
        if nb:
            hs[i, :nb] = BsbHashes(cid, p.Bsb22Commitments, lib=lib) if hashes is None else np.asarray(hashes[i], dtype=np.uint64).reshape(nb, 4)
    ch = as_u64(np.asarray(challenges, dtype=np.uint64).reshape(N, NB_CHALLENGES, 4).reshape(N * NB_CHALLENGES, 4), 4)
    return pts, ev, ch, pub[:, :npub], hs[:, :nb], shaped


def _run(ctx: Context, vk: VerifyingKey, arrays, flags: int, weights=None):
    pts, ev, ch, pub, hs = (np.ascontiguousarray(a) for a in arrays)
    N = pts.shape[0]
    a = _lib.PlonkProofs()
    a.points, a.evals, a.challenges = pts.ctypes.data, ev.ctypes.data, ch.ctypes.data
    a.public_inputs = pub.ctypes.data if pub.size else None
    a.bsb_hashes = hs.ctypes.data if hs.size else None
    ok = np.zeros(N, dtype=np.uint8)
    rel = np.zeros(N, dtype=np.uint8)
    out2 = (C.c_uint64 * 2)()
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.uint64)
    ctx.lib.check(ctx.lib.ga_plonk_verify(vk.handle, C.byref(a), N, flags, None if w is None else _ptr(w), _ptr(ok), _ptr(rel), out2))
    return ok, rel, (int(out2[0]), int(out2[1]))


def Scalars(ctx: Context, vk: VerifyingKey, proofs, public_witnesses, challenges, hashes=None):
    """ga_plonk_verify_scalars: (rows (N, 2 (9 + nb_bsb) + 2, 4), relation_ok (N,)) -- the coefficient row of every proof's KZG check"""
    vk.Pin(ctx)
    pts, ev, ch, pub, hs, shaped = _pack(vk, proofs, public_witnesses, challenges, hashes, ctx.lib)
    if not shaped.all():
        raise ValueError("Scalars: a proof or a public witness has the wrong shape for this key")
    N = len(proofs)
    a = _lib.PlonkProofs()
    keep = [np.ascontiguousarray(x) for x in (pts, ev, ch, pub, hs)]
    a.points, a.evals, a.challenges = keep[0].ctypes.data, keep[1].ctypes.data, keep[2].ctypes.data
    a.public_inputs = keep[3].ctypes.data if keep[3].size else None
    a.bsb_hashes = keep[4].ctypes.data if keep[4].size else None
    rows = np.zeros((N, 2 * (FIXED_POINTS + vk.nb_bsb) + 2, 4), dtype=np.uint64)
    rel = np.zeros(N, dtype=np.uint8)
    ctx.lib.check(ctx.lib.ga_plonk_verify_scalars(vk.handle, C.byref(a), N, 0, _ptr(rows), _ptr(rel)))
    return rows, rel.astype(bool)


def VerifyMany(ctx: Context, vk: VerifyingKey, proofs, public_witnesses, challenges, hashes=None, point_check: bool = True, detail: bool = False):
    """N proofs under one key: one exact verdict per proof (what N calls of plonk.Verify return as nil / error); with `detail`
    (verdicts, relation_ok): whether the algebraic relation of verify.go:206-223 held, False too for a proof of the wrong shape.

    proofs: Proof objects; public_witnesses: per proof the public inputs as canonical integers; challenges: (N, 6, 4) fr images
    gamma beta alpha zeta v u; hashes: per proof the (nb_bsb, 4) hashed commitments, or None to compute them (BsbHashes)."""
    N = len(proofs)
    verdict, relation = np.zeros(N, dtype=bool), np.zeros(N, dtype=bool)
    if N:
        vk.Pin(ctx)
        pts, ev, ch, pub, hs, shaped = _pack(vk, proofs, public_witnesses, challenges, hashes, ctx.lib)
        live = np.flatnonzero(shaped)
        if live.size:
            chl = ch.reshape(N, NB_CHALLENGES, 4)[live].reshape(-1, 4)
            flags = 0 if point_check else _lib.PLONK_VERIFY_NO_POINT_CHECK
            ok, rel, _ = _run(ctx, vk, (pts[live], ev[live], chl, pub[live], hs[live]), flags)
            verdict[live], relation[live] = ok.astype(bool), rel.astype(bool)
    return (verdict, relation) if detail else verdict


def Verify(ctx: Context, vk: VerifyingKey, proof, public_witness, challenges, hashes=None) -> bool:
    """plonk.Verify (verify.go:36-323) with the challenges given: False where the reference returns an error"""
    return bool(VerifyMany(ctx, vk, [proof], [public_witness], np.asarray(challenges, dtype=np.uint64).reshape(1, NB_CHALLENGES, 4),
                           None if hashes is None else [hashes])[0])


def BatchVerify(ctx: Context, vk: VerifyingKey, proofs, public_witnesses, challenges, rng, hashes=None, weights=None) -> bool:
    """The randomised check of N proofs under one key: sum_j rho_j (P_j, Q_j) with 128-bit rho_j drawn from `rng` (a numpy Generator: a
    caller that keeps the seed can replay them) unless `weights` (canonical integers) are given.  True means every proof is valid
    up to a probability of about 2^-128; False that at least one is not (VerifyMany says which)."""
    N = len(proofs)
    if N == 0:
        return True
    vk.Pin(ctx)
    pts, ev, ch, pub, hs, shaped = _pack(vk, proofs, public_witnesses, challenges, hashes, ctx.lib)
    if not shaped.all():
        return False
    if weights is None:
        words = rng.integers(0, 1 << 64, size=(N, 2), dtype=np.uint64)
        weights = [int(lo) | (int(hi) << 64) for lo, hi in words]
    ok, _, _ = _run(ctx, vk, (pts, ev, ch, pub, hs), _lib.PLONK_VERIFY_COMBINED, fr_mont(vk.curve, weights))
    return bool(ok[0])
