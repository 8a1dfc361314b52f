"""groth16.Verify on the device (backend/groth16/bn254/verify.go:38-145): the verifying key as gnark writes it, and three verifiers
over ecc.PairingCheck -- Verify (one proof, the reference's steps), VerifyMany (N proofs under one key, one exact verdict each, one
pairing call) and BatchVerify (the randomised check of N proofs with N + 3 Miller loops and one final exponentiation).  The points
around the pairings come from CheckPoints, ScalePoints, MultiExp and SparsePointSums; the commitment hashes are HashToField."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib, ecc
from .device import Context, _ptr, affine_words, as_u64, curve_id
from .ecc import G1, G2
from .g16_setup import FR_MODULUS
from .groth16 import COMMITMENT_DST, FOLD_DST, HashToField, MarshalG1

FP_MODULUS = {
    _lib.BN254: 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47,
    _lib.BLS12_381: 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB,
}


def _int(words) -> int:
    return sum(int(w) << (64 * i) for i, w in enumerate(words))


def _words(k: int, n: int):
    return [(k >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(n)]


def _neg(cid: int, group: int, pt: np.ndarray) -> np.ndarray:
    """-P of one affine image: every Fp coordinate of y becomes p - y (Montgomery images negate like the values); (0,0) stays"""
    p, wa = FP_MODULUS[cid], affine_words(cid, group)
    nw = wa // (2 if group == G1 else 4)
    out = np.array(pt, dtype=np.uint64).reshape(wa).copy()
    for lo in range(wa // 2, wa, nw):
        y = _int(out[lo:lo + nw])
        out[lo:lo + nw] = _words((p - y) % p, nw)
    return out


def _fr_from_mont(cid: int, words) -> int:
    r = FR_MODULUS[cid]
    return _int(words) * pow(1 << 256, -1, r) % r


def _scalars(ks) -> np.ndarray:
    return np.array([_words(int(k), 4) for k in ks], dtype=np.uint64).reshape(-1, 4)


@dataclass
class VerifyingKey:
    """backend/groth16/bn254/verify.go / setup.go:58-73: affine images, Montgomery limbs"""
    curve: int
    alpha1: np.ndarray
    beta2: np.ndarray
    gamma2: np.ndarray
    delta2: np.ndarray
    K: np.ndarray                                            # (nb_public + nb_commitments, 2 fp) G1Affine
    CommitmentKeys: list = field(default_factory=list)       # per commitment (G, GSigmaNeg), G2Affine each (pedersen.VerifyingKey)
    PublicAndCommitmentCommitted: list = field(default_factory=list)
    e: np.ndarray = None                                     # e(alpha, beta) in the library's normalisation (Precompute)
    beta1: np.ndarray = None                                 # [beta]1, [delta]1: in the file, not used by the verifier
    delta1: np.ndarray = None

    @classmethod
    def ReadFrom(cls, curve, data: bytes, lib=None):
        """VerifyingKey.ReadFrom (marshal.go:151-230), compressed or raw points: [alpha]1 [beta]1 [beta]2 [gamma]2 [delta]1 [delta]2,
        u32 len + [K]1, then -- when present -- PublicAndCommitmentCommitted (u32 count, per row u32 len + u64s), u32 nbCommitments and
        per commitment a pedersen.VerifyingKey (G, GSigmaNeg).  Returns (key, bytes read); reading stops behind the last field, as
        the Go decoder's does."""
        lib = lib or _lib.load()
        cid = curve_id(curve)
        data = bytes(data)
        buf = np.frombuffer(data, dtype=np.uint8)
        off = 0

        def point(group):
            nonlocal off
            out = np.zeros(affine_words(cid, group), dtype=np.uint64)
            used = C.c_size_t()
            lib.check(lib.ga_point_unmarshal(cid, group, C.c_void_p(buf.ctypes.data + off), len(data) - off, _ptr(out), C.byref(used)))
            off += used.value
            return out

        def uint(nbytes):
            nonlocal off
            if off + nbytes > len(data):
                raise ValueError("verifying key: truncated")
            v = int.from_bytes(data[off:off + nbytes], "big")
            off += nbytes
            return v

        alpha1, beta1, beta2, gamma2, delta1, delta2 = point(G1), point(G1), point(G2), point(G2), point(G1), point(G2)
        nk = uint(4)
        K = np.array([point(G1) for _ in range(nk)], dtype=np.uint64).reshape(nk, affine_words(cid, G1))
        pacc, keys = [], []
        if off < len(data):
            for _ in range(uint(4)):
                pacc.append([uint(8) for _ in range(uint(4))])
            for _ in range(uint(4)):
                g = point(G2)
                keys.append((g, point(G2)))
        return cls(cid, alpha1, beta2, gamma2, delta2, K, keys, pacc, None, beta1, delta1), off

    def Precompute(self, ctx: Context):
        """vk.Precompute (verify.go:70-73 reads its result): e = e(alpha, beta), the group value of one PairingCheck"""
        _, gt, _, _ = ecc.PairingCheck(ctx, self.curve, self.alpha1[None, :], self.beta2[None, :], want_gt=True)
        self.e = gt[0]
        return self.e

    @property
    def nb_commitments(self) -> int:
        return len(self.PublicAndCommitmentCommitted)


def _proof_points(cid, proofs):
    """(Ar, Bs, Krs, commitments (N, ncom, 2 fp), poks) of a list of proofs as arrays; the number of commitments must agree"""
    w1, w2 = affine_words(cid, G1), affine_words(cid, G2)
    ar = as_u64(np.array([np.asarray(p.Ar).reshape(w1) for p in proofs]).reshape(-1, w1), w1)
    bs = as_u64(np.array([np.asarray(p.Bs).reshape(w2) for p in proofs]).reshape(-1, w2), w2)
    krs = as_u64(np.array([np.asarray(p.Krs).reshape(w1) for p in proofs]).reshape(-1, w1), w1)
    coms = [np.zeros((0, w1), np.uint64) if p.Commitments is None else np.asarray(p.Commitments, dtype=np.uint64).reshape(-1, w1) for p in proofs]
    poks = [np.zeros(w1, np.uint64) if p.CommitmentPok is None else np.asarray(p.CommitmentPok, dtype=np.uint64).reshape(w1) for p in proofs]
    return ar, bs, krs, coms, poks


def _shape_ok(vk: VerifyingKey, ncom: int, npub: int) -> bool:
    """verify.go:46-58: the counts of commitments and of public inputs (without the constant-one wire)"""
    nb_public = vk.K.shape[0] - vk.nb_commitments
    return len(vk.CommitmentKeys) == vk.nb_commitments and ncom == vk.nb_commitments and npub == nb_public - 1


def _commitment_wires(vk: VerifyingKey, pw: list, coms: np.ndarray, lib):
    """solveCommitmentWire (verify.go:86-103): the hash of every commitment joins the public witness; and the fold challenge"""
    cid = vk.curve
    ser = b""
    for i, idx in enumerate(vk.PublicAndCommitmentCommitted):
        msg = MarshalG1(cid, coms[i], lib=lib) + b"".join(int(pw[j - 1]).to_bytes(32, "big") for j in idx)
        h = _fr_from_mont(cid, HashToField(cid, msg, COMMITMENT_DST, 1, lib=lib)[0])
        pw.append(h)
        ser += h.to_bytes(32, "big")
    return _fr_from_mont(cid, HashToField(cid, ser, FOLD_DST, 1, lib=lib)[0]) if ser else 0


def VerifyMany(ctx: Context, vk: VerifyingKey, proofs, public_witnesses) -> np.ndarray:
    """N proofs under one key: one exact verdict per proof (what N calls of groth16.Verify return as nil / error), from one CheckPoints
    call per group of points, one SparsePointSums call for the N kSums (rows: the proofs, columns: vk.K and the commitments), one
    ScalePoints call for the folded commitments and ONE PairingCheck call of N groups (2N with commitments).

    proofs: objects with Ar, Bs, Krs, Commitments, CommitmentPok (groth16.Proof); public_witnesses: per proof the public inputs as
    canonical integers, without the constant-one wire."""
    cid, lib = vk.curve, ctx.lib
    r = FR_MODULUS[cid]
    N = len(proofs)
    verdict = np.zeros(N, dtype=bool)
    if N == 0:
        return verdict
    w1 = affine_words(cid, G1)
    ar, bs, krs, coms, poks = _proof_points(cid, proofs)
    live = [i for i in range(N) if _shape_ok(vk, coms[i].shape[0], len(public_witnesses[i]))]
    if not live:
        return verdict
    ncom, nk, L = vk.nb_commitments, vk.K.shape[0], len(live)
    ar, bs, krs = ar[live], bs[live], krs[live]
    com = np.concatenate([coms[i] for i in live]).reshape(L * ncom, w1)
    pok = np.array([poks[i] for i in live], dtype=np.uint64).reshape(L, w1)

    # proof.isValid (verify.go:63-65): on the curve and in the subgroups
    g1_pts = np.concatenate([ar, krs, com, pok] if ncom else [ar, krs])
    st1 = ecc.CheckPoints(ctx, cid, G1, g1_pts)[0]
    st2 = ecc.CheckPoints(ctx, cid, G2, bs)[0]
    valid = (st1[:L] == 0) & (st1[L:2 * L] == 0) & (st2 == 0)
    if ncom:
        valid &= (st1[2 * L:2 * L + L * ncom].reshape(L, ncom) == 0).all(axis=1) & (st1[2 * L + L * ncom:] == 0)

    pws, challenges = [], []
    for k, i in enumerate(live):
        pw = [int(x) % r for x in public_witnesses[i]]
        challenges.append(_commitment_wires(vk, pw, com[k * ncom:(k + 1) * ncom], lib))
        pws.append(pw)

    # kSum_i = K[0] + sum_j pw_ij K[j] + sum_k C_ik (verify.go:115-123): row i of a sparse matrix over [K | commitments]
    coeffs = _scalars([1] + [x for pw in pws for x in pw])
    terms = np.zeros((L, nk + ncom, 2), dtype=np.uint32)
    terms[:, 1:nk, 0] = 1 + np.arange(L * (nk - 1), dtype=np.uint32).reshape(L, nk - 1)
    terms[:, :nk, 1] = np.arange(nk, dtype=np.uint32)
    terms[:, nk:, 1] = nk + np.arange(L * ncom, dtype=np.uint32).reshape(L, ncom)
    row_start = np.arange(L + 1, dtype=np.uint64) * (nk + ncom)
    ksum, _ = ecc.SparsePointSums(ctx, cid, G1, np.concatenate([vk.K, com]), row_start, terms.reshape(-1, 2), coeffs)

    neg_alpha, neg_gamma, neg_delta = _neg(cid, G1, vk.alpha1), _neg(cid, G2, vk.gamma2), _neg(cid, G2, vk.delta2)
    P, Q, gs = [], [], [0]
    if ncom:
        # pedersen.BatchVerifyMultiVk (verify.go:104-112): prod_k e(ch^k C_k, GSigmaNeg_k) e(pok, G) = 1
        folded, _ = ecc.ScalePoints(ctx, cid, G1, com, _scalars([pow(ch, k, r) for ch in challenges for k in range(ncom)]))
        sneg = np.array([s for _, s in vk.CommitmentKeys], dtype=np.uint64)
    for k in range(L):
        if ncom:
            P += [folded[k * ncom:(k + 1) * ncom], pok[k][None, :]]
            Q += [sneg, vk.CommitmentKeys[0][0][None, :]]
            gs.append(gs[-1] + ncom + 1)
        # e(Krs, -delta) e(Ar, Bs) e(kSum, -gamma) e(-alpha, beta) = 1 (verify.go:128-139)
        P += [krs[k][None, :], ar[k][None, :], ksum[k][None, :], neg_alpha[None, :]]
        Q += [neg_delta[None, :], bs[k][None, :], neg_gamma[None, :], vk.beta2[None, :]]
        gs.append(gs[-1] + 4)
    ok, _, _ = ecc.PairingCheck(ctx, cid, np.concatenate(P), np.concatenate(Q), gs)
    per = ok.reshape(L, 2 if ncom else 1).all(axis=1)
    verdict[live] = valid & per
    return verdict


def Verify(ctx: Context, vk: VerifyingKey, proof, public_witness) -> bool:
    """groth16.Verify (verify.go:38-145): proof.isValid through CheckPoints, the commitment hashes through HashToField, kSum on the
    device through MultiExp, and the Pedersen batch check and the main equation as the two groups of one PairingCheck call.  False
    where the reference returns an error."""
    cid, lib = vk.curve, ctx.lib
    r = FR_MODULUS[cid]
    ar, bs, krs, coms, poks = _proof_points(cid, [proof])
    com, ncom = coms[0], vk.nb_commitments
    if not _shape_ok(vk, com.shape[0], len(public_witness)):
        return False
    g1_pts = np.concatenate([ar, krs, com, poks[0][None, :]] if ncom else [ar, krs])
    if ecc.CheckPoints(ctx, cid, G1, g1_pts, status=False)[3] != ecc.NONE_BAD or ecc.CheckPoints(ctx, cid, G2, bs, status=False)[3] != ecc.NONE_BAD:
        return False
    pw = [int(x) % r for x in public_witness]
    ch = _commitment_wires(vk, pw, com, lib)
    # kSum = K[0] + sum_j pw_j K[j] + sum_k C_k (verify.go:115-123) as one MSM
    ksum = ecc.jac_to_affine(cid, G1, ecc.MultiExp(ctx, cid, G1, np.concatenate([vk.K, com]), _scalars([1] + pw + [1] * ncom), montgomery=False), lib=lib)
    P, Q, gs = [], [], [0]
    if ncom:
        folded, _ = ecc.ScalePoints(ctx, cid, G1, com, powers=(1, ch))
        P += [folded, poks[0][None, :]]
        Q += [np.array([s for _, s in vk.CommitmentKeys], dtype=np.uint64), vk.CommitmentKeys[0][0][None, :]]
        gs.append(ncom + 1)
    P += [krs, ar, ksum[None, :], _neg(cid, G1, vk.alpha1)[None, :]]
    Q += [_neg(cid, G2, vk.delta2)[None, :], bs, _neg(cid, G2, vk.gamma2)[None, :], vk.beta2[None, :]]
    gs.append(gs[-1] + 4)
    ok, _, _ = ecc.PairingCheck(ctx, cid, np.concatenate(P), np.concatenate(Q), gs)
    return bool(ok.all())


def BatchVerify(ctx: Context, vk: VerifyingKey, proofs, public_witnesses, rng) -> bool:
    """The randomised check of N proofs under one key without commitments, with 128-bit r_i drawn from `rng` (a numpy Generator: a
    caller that keeps the seed can replay them):

        prod_i e(r_i A_i, B_i) . e(sum_i r_i Krs_i, -delta) . e(sum_i r_i kSum_i, -gamma) . e(-(sum_i r_i) alpha, beta) = 1

    N + 3 Miller loops and one final exponentiation; a false statement passes with probability about 2^-128.  True means every
    proof is valid; False that at least one is not (VerifyMany says which)."""
    cid = vk.curve
    if vk.nb_commitments or vk.CommitmentKeys:
        raise ValueError("BatchVerify: keys with commitments are not supported (each proof has its own Pedersen check): use VerifyMany")
    r = FR_MODULUS[cid]
    N = len(proofs)
    if N == 0:
        return True
    ar, bs, krs, coms, _ = _proof_points(cid, proofs)
    if not all(_shape_ok(vk, coms[i].shape[0], len(public_witnesses[i])) for i in range(N)):
        return False
    if ecc.CheckPoints(ctx, cid, G1, np.concatenate([ar, krs]), status=False)[3] != ecc.NONE_BAD:
        return False
    if ecc.CheckPoints(ctx, cid, G2, bs, status=False)[3] != ecc.NONE_BAD:
        return False
    words = rng.integers(0, 1 << 64, size=(N, 2), dtype=np.uint64)
    ri = [int(lo) | (int(hi) << 64) for lo, hi in words]
    rs = _scalars(ri)
    nk = vk.K.shape[0]
    # sum_i r_i kSum_i = [sum_i r_i] K[0] + sum_j [sum_i r_i pw_ij] K[j]
    ks = [sum(ri) % r] + [sum(x * (int(pw[j]) % r) for x, pw in zip(ri, public_witnesses)) % r for j in range(nk - 1)]
    scaled_a, _ = ecc.ScalePoints(ctx, cid, G1, ar, rs)
    lib = ctx.lib
    affine = lambda jac: ecc.jac_to_affine(cid, G1, jac, lib=lib)
    sum_krs = affine(ecc.MultiExp(ctx, cid, G1, krs, rs, montgomery=False))
    sum_k = affine(ecc.MultiExp(ctx, cid, G1, vk.K, _scalars(ks), montgomery=False))
    neg_alpha, _ = ecc.ScalePoints(ctx, cid, G1, vk.alpha1[None, :], scalar=(r - ks[0]) % r)
    P = np.concatenate([scaled_a, sum_krs[None, :], sum_k[None, :], neg_alpha])
    Q = np.concatenate([bs, _neg(cid, G2, vk.delta2)[None, :], _neg(cid, G2, vk.gamma2)[None, :], vk.beta2[None, :]])
    ok, _, _ = ecc.PairingCheck(ctx, cid, P, Q)
    return bool(ok[0])
