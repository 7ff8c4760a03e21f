"""Node-side validation of MASP bundles: the verifier half of the `masp_proofs` API.

    SaplingVerificationContextInner   masp_proofs/src/sapling/verifier.rs:20-204
    SaplingVerificationContext        masp_proofs/src/sapling/verifier/single.rs
    BatchValidator                    masp_proofs/src/sapling/verifier/batch.rs:40-239

Types cross this API in their wire encodings, as in prover.py: Jubjub points as 32-byte `to_bytes()` encodings, field elements as
ints or 32-byte little-endian values, proofs as 192 bytes, RedJubjub signatures as 64 bytes Rbar || Sbar.  A cv, rk or epk that does
not decode (ZIP 216 rules) makes its bundle invalid, as the reference's deserialisation of the bundle would.  The consensus checks are
host-side; `BatchValidator.validate` makes one RedJubjub batch call on the GPU (masp_hip_redjubjub_verify_batch) and one Groth16 batch
call per non-empty circuit batch (masp_hip_verify_batch).  `BatchValidator.validate_each` says WHICH bundle is bad: the same queues
through the per-item calls (masp_hip_redjubjub_verify_each, masp_hip_verify_each), one verdict per check_bundle call.
"""
import secrets
from dataclasses import dataclass

from . import host as H
from . import redjubjub as RJS
from .hip import BINDING, SPEND_AUTH

I128_MIN, I128_MAX = -(1 << 127), (1 << 127) - 1


@dataclass
class SpendDescription:
    cv: bytes
    anchor: object            # bls12_381::Scalar: int or 32 bytes LE
    nullifier: bytes
    rk: bytes
    zkproof: bytes
    spend_auth_sig: bytes


@dataclass
class ConvertDescription:
    cv: bytes
    anchor: object
    zkproof: bytes


@dataclass
class OutputDescription:
    cv: bytes
    cmu: object               # bls12_381::Scalar: int or 32 bytes LE
    ephemeral_key: bytes
    zkproof: bytes


@dataclass
class Bundle:
    spends: list
    converts: list
    outputs: list
    value_balance: list       # [(asset identifier[32], i128)]: the components of the reference's I128Sum, as binding_sig takes them
    binding_sig: bytes


def spending_key_generator():
    return H.point_bytes(*H.generator_uv(4))


def value_commitment_randomness_generator():
    return H.point_bytes(*H.generator_uv(3))


def _int(x):
    return x if isinstance(x, int) else int.from_bytes(bytes(x), "little")


def decodes(p):
    """ExtendedPoint::from_bytes succeeds (canonical v, u^2 a square, no negative zero)."""
    try:
        H.point_uv(bytes(p))
        return True
    except ValueError:
        return False


def is_small_order(p):
    return H.jubjub_mul(bytes(p), 8) == H.JUBJUB_IDENTITY


def spend_public_inputs(cv, anchor, nullifier, rk):
    """verifier.rs:71-95: rk.u, rk.v, cv.u, cv.v, anchor, the nullifier multipacked into two 254-bit chunks."""
    return list(H.point_uv(bytes(rk))) + list(H.point_uv(bytes(cv))) + [_int(anchor)] + H.multipack(bytes(nullifier))


def convert_public_inputs(cv, anchor):
    """verifier.rs:120-128: cv.u, cv.v, anchor."""
    return list(H.point_uv(bytes(cv))) + [_int(anchor)]


def output_public_inputs(cv, cmu, epk):
    """verifier.rs:151-165: cv.u, cv.v, epk.u, epk.v, cmu."""
    return list(H.point_uv(bytes(cv))) + list(H.point_uv(bytes(epk))) + [_int(cmu)]


def _le32(x):
    return x.to_bytes(32, "little") if isinstance(x, int) else bytes(x)


def _device_shaped(bundle):
    """Every field of the bundle has the length its wire encoding has (a scalar given as an int is below 2^256): BatchValidator.check_bundles
    sends such a bundle to the device; any other goes through check_bundle."""
    def raw(x, n=32):        # a point, a nullifier, a proof
        return not isinstance(x, int) and len(bytes(x)) == n

    def scalar(x):
        return 0 <= x < 1 << 256 if isinstance(x, int) else len(bytes(x)) == 32
    try:
        return (all(raw(d.cv) and scalar(d.anchor) and raw(d.nullifier) and raw(d.rk) and raw(d.zkproof, 192) for d in bundle.spends) and
                all(raw(d.cv) and scalar(d.anchor) and raw(d.zkproof, 192) for d in bundle.converts) and
                all(raw(d.cv) and scalar(d.cmu) and raw(d.ephemeral_key) and raw(d.zkproof, 192) for d in bundle.outputs) and
                all(raw(a) and int(v) == v for a, v in bundle.value_balance))
    except (TypeError, ValueError):
        return False


def _rows_as_ints(a):
    """uint8[n, k, 32] of little-endian scalars -> n lists of k ints"""
    n, k = a.shape[0], a.shape[1]
    data = a.tobytes()
    return [[int.from_bytes(data[32 * (i * k + j):32 * (i * k + j) + 32], "little") for j in range(k)] for i in range(n)]


class _Inner:
    """SaplingVerificationContextInner (verifier.rs:20-204): cv_sum and the consensus checks; the signature and proof checks are the
    caller's callbacks, as in the reference."""

    def __init__(self):
        self.cv_sum = H.JUBJUB_IDENTITY

    def check_spend(self, cv, anchor, nullifier, rk, sighash, spend_auth_sig, zkproof, sig_check, proof_check):
        if is_small_order(cv) or is_small_order(rk):
            return False
        self.cv_sum = H.jubjub_add(self.cv_sum, cv)
        if not sig_check(rk, bytes(rk) + bytes(sighash), spend_auth_sig):
            return False
        return proof_check(zkproof, spend_public_inputs(cv, anchor, nullifier, rk))

    def check_convert(self, cv, anchor, zkproof, proof_check):
        if is_small_order(cv):
            return False
        self.cv_sum = H.jubjub_add(self.cv_sum, cv)
        return proof_check(zkproof, convert_public_inputs(cv, anchor))

    def check_output(self, cv, cmu, epk, zkproof, proof_check):
        if is_small_order(cv) or is_small_order(epk):
            return False
        self.cv_sum = H.jubjub_add(self.cv_sum, cv, subtract=True)
        return proof_check(zkproof, output_public_inputs(cv, cmu, epk))

    def bvk(self, value_balance):
        """cv_sum - sum of [value] value_commitment_generator(asset) (masp_compute_value_balance, sapling/mod.rs:14-38); None when a
        value has no absolute value in i128 (i128::MIN) or an asset identifier has no generator."""
        bvk = self.cv_sum
        for asset, value in value_balance:
            value = int(value)
            if not I128_MIN < value <= I128_MAX:
                return None
            try:
                vb = H.jubjub_mul(H.jubjub_mul(H.asset_generator(asset), 8), abs(value))
            except ValueError:
                return None
            bvk = H.jubjub_add(bvk, vb, subtract=value >= 0)
        return bvk

    def final_check(self, value_balance, sighash, binding_sig, sig_check):
        bvk = self.bvk(value_balance)
        if bvk is None:
            return False
        return sig_check(bvk, bvk + bytes(sighash), binding_sig)


class SaplingVerificationContext:
    """= SaplingVerificationContext (verifier/single.rs), ZIP 216 on: signatures by `redjubjub.verify` and proofs by a verifying key's
    `verify(proof, public_inputs)` (host.PreparedVerifyingKey), one at a time on the host.  Points that do not decode are refused."""

    def __init__(self):
        self._inner = _Inner()

    @property
    def cv_sum(self):
        return self._inner.cv_sum

    def check_spend(self, cv, anchor, nullifier, rk, sighash, spend_auth_sig, zkproof, verifying_key):
        if not (decodes(cv) and decodes(rk)):
            return False
        g = spending_key_generator()
        return self._inner.check_spend(cv, anchor, nullifier, rk, sighash, spend_auth_sig, zkproof,
                                       lambda vk, msg, sig: RJS.verify(vk, msg, bytes(sig), g),
                                       lambda proof, pi: verifying_key.verify(proof, pi))

    def check_convert(self, cv, anchor, zkproof, verifying_key):
        if not decodes(cv):
            return False
        return self._inner.check_convert(cv, anchor, zkproof, lambda proof, pi: verifying_key.verify(proof, pi))

    def check_output(self, cv, cmu, epk, zkproof, verifying_key):
        if not (decodes(cv) and decodes(epk)):
            return False
        return self._inner.check_output(cv, cmu, epk, zkproof, lambda proof, pi: verifying_key.verify(proof, pi))

    def final_check(self, value_balance, sighash, binding_sig):
        g = value_commitment_randomness_generator()
        return self._inner.final_check(value_balance, sighash, binding_sig, lambda vk, msg, sig: RJS.verify(vk, msg, bytes(sig), g))


_EMPTY_BUNDLE = Bundle([], [], [], [], b"")     # what check_bundles sends in the place of a bundle that check_bundle decides


class BatchValidator:
    """= BatchValidator (verifier/batch.rs:40-239) over one `hip.Context`: check_bundle runs the consensus checks on the host and queues
    proofs (per circuit) and signatures; validate verifies everything queued in one RedJubjub batch and one Groth16 batch per circuit on
    the GPU.  Several validators may share a context and run in different threads.  check_bundles is check_bundle over a block's bundles
    with the per-description work in one device call; the two may be mixed."""

    def __init__(self, context):
        self._ctx = context
        self._bundles_added = False
        self._proofs = {"spend": ([], []), "convert": ([], []), "output": ([], [])}
        self._signatures = []            # (vk, sig, sighash, kind)
        self._bundles = []               # per check_bundle call: (what it returned, where its items start in the four queues)

    def _queue_marks(self):
        return (len(self._signatures),) + tuple(len(self._proofs[k][0]) for k in ("spend", "convert", "output"))

    def _queue_proof(self, kind, proof, public_inputs):
        self._proofs[kind][0].append(bytes(proof))
        self._proofs[kind][1].append(public_inputs)
        return True

    def _queue_sig(self, vk, sig, sighash, kind):
        self._signatures.append((bytes(vk), bytes(sig), bytes(sighash), kind))
        return True

    def check_bundle(self, bundle, sighash):
        """batch.rs:78-193.  False if the bundle breaks a consensus rule checked here (a proof `Proof::read` refuses, a cv / rk / epk that
        does not decode or has small order, a bad value balance); what was queued before that stays queued, as in the reference."""
        self._bundles_added = True
        start = self._queue_marks()
        ok = self._check_bundle(bundle, sighash)
        self._bundles.append((ok, start))
        return ok

    def _check_bundle(self, bundle, sighash):
        sighash = bytes(sighash)
        ctx = _Inner()
        for d in bundle.spends:
            if not (decodes(d.cv) and decodes(d.rk)) or not H.proof_read(d.zkproof):
                return False
            if not ctx.check_spend(d.cv, d.anchor, d.nullifier, d.rk, sighash, d.spend_auth_sig, d.zkproof,
                                   lambda vk, msg, sig: self._queue_sig(vk, sig, sighash, SPEND_AUTH),
                                   lambda proof, pi: self._queue_proof("spend", proof, pi)):
                return False
        for d in bundle.converts:
            if not decodes(d.cv) or not H.proof_read(d.zkproof):
                return False
            if not ctx.check_convert(d.cv, d.anchor, d.zkproof, lambda proof, pi: self._queue_proof("convert", proof, pi)):
                return False
        for d in bundle.outputs:
            if not (decodes(d.cv) and decodes(d.ephemeral_key)) or not H.proof_read(d.zkproof):
                return False
            if not ctx.check_output(d.cv, d.cmu, d.ephemeral_key, d.zkproof, lambda proof, pi: self._queue_proof("output", proof, pi)):
                return False
        return ctx.final_check(bundle.value_balance, sighash, bundle.binding_sig,
                               lambda vk, msg, sig: self._queue_sig(vk, sig, sighash, BINDING))

    def check_bundles(self, bundles, sighashes):
        """check_bundle over a whole block: one bool per bundle, and the validator's queues and marks exactly as check_bundle leaves them
        bundle after bundle, with the per-description work (decoding cv / rk / epk, the small-order tests, `Proof::read`, the public
        inputs, bvk) done for all bundles in ONE device call (Context.check_bundles).  The queues are then rebuilt from the statuses in
        the reference's order.  A bundle with a field of the wrong length goes through check_bundle itself, in its place; a value outside
        i128 is sent as i128::MIN, which is refused where check_bundle refuses it."""
        bundles, sighashes = list(bundles), [bytes(s) for s in sighashes]
        assert len(bundles) == len(sighashes)
        if not bundles:
            return []
        on_device = [_device_shaped(b) for b in bundles]
        sent = [b if dev else _EMPTY_BUNDLE for b, dev in zip(bundles, on_device)]
        spends, converts, outputs = ([d for b in sent for d in getattr(b, k)] for k in ("spends", "converts", "outputs"))
        entries = [(a, int(v)) for b in sent for a, v in b.value_balance]
        join = lambda items, field: b"".join(_le32(getattr(d, field)) for d in items)      # noqa: E731
        res = self._ctx.check_bundles(
            [(len(b.spends), len(b.converts), len(b.outputs), len(b.value_balance)) for b in sent],
            [join(spends, f) for f in ("cv", "anchor", "nullifier", "rk", "zkproof")],
            [join(converts, f) for f in ("cv", "anchor", "zkproof")],
            [join(outputs, f) for f in ("cv", "cmu", "ephemeral_key", "zkproof")],
            [b"".join(bytes(a) for a, _ in entries),
             b"".join((v if I128_MIN <= v <= I128_MAX else I128_MIN).to_bytes(16, "little", signed=True) for _, v in entries)])
        inputs = [_rows_as_ints(a) for a in (res.spend_inputs, res.convert_inputs, res.output_inputs)]
        status = [a.tolist() for a in (res.spend_status, res.convert_status, res.output_status)]
        bundle_status, bvks = res.bundle_status.tolist(), res.bvk.tobytes()
        at, verdicts = [0, 0, 0], []
        for k, (bundle, sighash, dev) in enumerate(zip(bundles, sighashes, on_device)):
            if not dev:
                verdicts.append(self.check_bundle(bundle, sighash))
                continue
            self._bundles_added = True
            start = self._queue_marks()
            ok = True
            for q, (kind, items) in enumerate((("spend", bundle.spends), ("convert", bundle.converts), ("output", bundle.outputs))):
                first = at[q]
                at[q] += len(items)
                for i, d in enumerate(items, first):
                    if not ok or status[q][i]:
                        ok = False             # refused at this description: what came before stays queued, nothing after it is
                        break
                    if q == 0:
                        self._queue_sig(d.rk, d.spend_auth_sig, sighash, SPEND_AUTH)
                    self._queue_proof(kind, d.zkproof, inputs[q][i])
            if ok and bundle_status[k] == 0:
                self._queue_sig(bvks[32 * k:32 * k + 32], bundle.binding_sig, sighash, BINDING)
            else:
                ok = False
            self._bundles.append((ok, start))
            verdicts.append(ok)
        return verdicts

    def validate(self, spend_vk, convert_vk, output_vk, rng=None):
        """batch.rs:201-239.  The vks are hip.GpuVerifyingKey objects; rng(k) -> k random bytes (default: secrets.token_bytes).  True when
        no bundle was added; otherwise True iff every queued signature and proof verifies."""
        if not self._bundles_added:
            return True
        rng = rng or secrets.token_bytes
        if self._signatures and not self._ctx.redjubjub_verify_batch(self._signatures, randomness=rng(16 * len(self._signatures))):
            return False
        for kind, vk in (("spend", spend_vk), ("convert", convert_vk), ("output", output_vk)):
            proofs, inputs = self._proofs[kind]
            if proofs and not vk.verify_batch(proofs, inputs, randomness=rng(16 * len(proofs))):
                return False
        return True

    def validate_each(self, spend_vk, convert_vk, output_vk):
        """One bool per check_bundle call, in order: True iff that call returned True and every signature and proof it queued verifies
        on its own (Context.redjubjub_verify_each, GpuVerifyingKey.verify_each: no randomness, the answer is exact).  A mempool calls
        this instead of `validate`; a block validator calls it once `validate` has said False, to name the transaction.  What a refused
        bundle had queued before it was refused is not verified and counts against no other bundle.  `validate` is unaffected."""
        ends = [start for _, start in self._bundles[1:]] + [self._queue_marks()]
        spans = [(ok, start, end) for (ok, start), end in zip(self._bundles, ends)]
        queues = [self._signatures] + [list(zip(*self._proofs[k])) for k in ("spend", "convert", "output")]
        verdicts = []
        for q, items in enumerate(queues):
            # the items of the bundles check_bundle accepted, and where each sits in its queue
            wanted = [i for ok, start, end in spans if ok for i in range(start[q], end[q])]
            sel = [items[i] for i in wanted]
            if not sel:
                got = []
            elif q == 0:
                got = [bool(v) for v in self._ctx.redjubjub_verify_each(sel)]
            else:
                vk = (spend_vk, convert_vk, output_vk)[q - 1]
                got = [v == 1 for v in vk.verify_each([p for p, _ in sel], [pi for _, pi in sel])]
            assert len(got) == len(sel)
            verdicts.append(dict(zip(wanted, got)))
        return [ok and all(verdicts[q][i] for q in range(4) for i in range(start[q], end[q])) for ok, start, end in spans]
