"""RedJubjub (RedDSA on Jubjub) for the binding signature of `SaplingProvingContext::binding_sig`
(/root/reference/masp_proofs/src/sapling/prover.rs:279-326), restated from
/root/reference/masp_primitives/src/sapling/redjubjub.rs:36-38,138-160,166-169,191-239 and
masp_primitives/src/sapling/util.rs:9-15.  Host-side and tiny: it closes the `TxProver` surface around the GPU prover;
group arithmetic goes through libmasp_host's Jubjub (`host.jubjub_mul / jubjub_add`).

Signing in batches: `sign_batch` and `spend_sigs` run `spend_sig_internal` (masp_primitives/src/sapling.rs:167-195) for many items in one
call, on the GPU (masp_hip_redjubjub_sign_batch) or on host threads (masp_host_redjubjub_sign_batch)."""
import hashlib
import os
import secrets

import numpy as np

from . import host as H

RJ = H.JUBJUB_ORDER


def h_star(a, b):
    """H*(a || b) = BLAKE2b-512(personal "MASP__RedJubjubH") reduced into the Jubjub scalar field (`from_bytes_wide`)."""
    h = hashlib.blake2b(digest_size=64, person=b"MASP__RedJubjubH")
    h.update(a)
    h.update(b)
    return int.from_bytes(h.digest(), "little") % RJ


def public_key(sk, generator):
    """PublicKey::from_private: [sk] P_G."""
    return H.jubjub_mul(generator, sk % RJ)


def sign(sk, msg, generator, rng=secrets.token_bytes):
    """PrivateKey::sign -> 64 bytes Rbar || Sbar.  T = 80 random bytes, r = H*(T || M), R = [r] P_G, S = r + H*(Rbar || M) sk."""
    t = rng(80)
    r = h_star(t, msg)
    rbar = H.jubjub_mul(generator, r)
    s = (r + h_star(rbar, msg) * (sk % RJ)) % RJ
    return rbar + s.to_bytes(32, "little")


def verify(vk, msg, sig, generator):
    """PublicKey::verify (ZIP 216 rules: canonical R): [8]( -[S] P_G + R + [c] vk ) == identity."""
    if len(sig) != 64:
        return False
    rbar, sbar = sig[:32], sig[32:]
    s = int.from_bytes(sbar, "little")
    if s >= RJ:
        return False
    try:
        c = h_star(rbar, msg)
        acc = H.jubjub_add(H.jubjub_add(rbar, H.jubjub_mul(vk, c)), H.jubjub_mul(generator, s), subtract=True)
        return H.jubjub_mul(acc, 8) == H.JUBJUB_IDENTITY
    except (H.HostError, ValueError):
        return False            # R or vk is not a canonical point encoding


def sign_batch(items, ctx, threads=None, rng=os.urandom):
    """items: (sk, alpha or None, sighash, kind) each -> one entry per item, in order: (vk, sig), 32 and 64 bytes, or None where the item is
    refused (sk or alpha not below r_J).  Per item rsk = sk + alpha, vk = [rsk] G_kind and sig = PrivateKey::sign(rsk, vk || sighash): what
    spend_sig_internal returns next to the rk it signs under.  kind: 0 spend authorisation, 1 binding.  sk, alpha: 32 bytes or an int;
    rng(80) draws each item's T, and everything below that is a function of its inputs.  ctx: a masp_amd.Context, the items are signed on
    its GPU (masp_hip_redjubjub_sign_batch); None: on `threads` host threads."""
    items = list(items)
    if not items:
        return []
    cat = lambda f: np.frombuffer(b"".join(f(it) for it in items), dtype=np.uint8)
    alphas = None if all(it[1] is None for it in items) else cat(lambda it: bytes(32) if it[1] is None else H._b(it[1]))
    arrays = (cat(lambda it: H._b(it[0])), alphas, cat(lambda it: H._b(it[2])), np.array([int(it[3]) for it in items], dtype=np.uint8),
              cat(lambda it: H._b(rng(80), 80)))
    status, vks, sigs = H.redjubjub_sign_batch(*arrays, threads=threads) if ctx is None else ctx.redjubjub_sign_batch(*arrays)
    return [None if s else (vk.tobytes(), sig.tobytes()) for s, vk, sig in zip(status.tolist(), vks, sigs)]


def spend_sigs(asks, ars, sighash, ctx, threads=None, rng=os.urandom):
    """The loop a builder runs over its spends: one sighash, spend i signed with ask_i randomised by ar_i -> (rk, spend_auth_sig) per spend,
    or None where ask_i or ar_i is not below r_J.  ctx, threads, rng: as sign_batch."""
    return sign_batch([(ask, ar, sighash, 0) for ask, ar in zip(asks, ars)], ctx, threads=threads, rng=rng)
