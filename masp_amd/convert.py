"""masp_primitives::convert: AllowedConversion, and the allowed conversions of a whole conversion tree in one call.

`AllowedConversion` is host.AllowedConversion.  `batch` computes many of them at once: on a masp_amd.Context's GPU
(masp_hip_sapling_allowed_conversions), or with ctx=None on host threads (masp_host_allowed_conversions).  A conversion tree is then two
device calls, the leaves and FrozenCommitmentTree's; fusing them so that the leaves never leave the device is not built."""
import numpy as np

from . import host as H
from .host import AllowedConversion  # noqa: F401
from .merkle_tree import FrozenCommitmentTree

STATUS = {1: "an asset identifier has no generator", 2: "a value is i128::MIN: invalid conversion"}


def _merge(sum_):
    """a value sum (a dict or pairs of identifier and value) merged as AllowedConversion.__init__ merges it: equal identifiers added,
    zeros dropped, in identifier order"""
    merged = {}
    for ident, value in (sum_.items() if isinstance(sum_, dict) else sum_):
        ident = H._b(ident)
        merged[ident] = merged.get(ident, 0) + int(value)
    merged = {k: v for k, v in sorted(merged.items()) if v != 0}
    for v in merged.values():
        if not -(1 << 127) <= v < (1 << 127):
            raise OverflowError("value does not fit an i128")
    return merged


def _run(merged, ctx, threads):
    """one call over the merged sums -> (status, generators, cmus)"""
    off = np.zeros(len(merged) + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in merged])
    ids = np.frombuffer(b"".join(k for m in merged for k in m), dtype=np.uint8).reshape(-1, 32)
    vals = np.frombuffer(b"".join(v.to_bytes(16, "little", signed=True) for m in merged for v in m.values()), dtype=np.uint8).reshape(-1, 16)
    if ctx is None:
        return H.allowed_conversions(off, ids, vals, threads=threads)
    return ctx.allowed_conversions(off, ids, vals)


def _refusal(status):
    e = ValueError("invalid conversion: " + STATUS.get(int(status), "status %d" % status))
    e.status = int(status)
    return e


class batch:
    """many allowed conversions per call"""

    @staticmethod
    def allowed_conversions(sums, ctx=None, threads=None):
        """AllowedConversion(sum) for every value sum of the list (each a dict or an iterable of (identifier, value)) in one call: on
        ctx's GPU, or with ctx=None on `threads` host threads.  One entry per sum, in order: the AllowedConversion, its leaf already known,
        or a ValueError instance with .status (1: an identifier has no generator, 2: a value is i128::MIN) where the call refused."""
        merged = [_merge(s) for s in sums]
        if not merged:
            return []
        status, gens, cmus = _run(merged, ctx, threads)
        return [AllowedConversion.from_parts(m, gens[i].tobytes(), cmus[i].tobytes()) if status[i] == 0 else _refusal(status[i])
                for i, m in enumerate(merged)]

    @staticmethod
    def read_allowed_conversions(blobs, ctx=None, threads=None):
        """AllowedConversion.read for every serialised conversion of the list, the generators recomputed in one call and compared.  One
        entry per blob, in order: the AllowedConversion, or a ValueError instance for what the checked read refuses."""
        out, parsed, where = [None] * len(blobs), [], []
        for i, blob in enumerate(blobs):
            try:
                parsed.append(AllowedConversion.parse(blob, check_identifiers=False))   # (the call below finds a bad identifier)
                where.append(i)
            except ValueError as e:
                out[i] = e
        if parsed:
            status, gens, cmus = _run([assets for assets, _ in parsed], ctx, threads)
            for k, (i, (assets, generator)) in enumerate(zip(where, parsed)):
                if status[k] != 0:
                    out[i] = _refusal(status[k])
                elif gens[k].tobytes() != generator:
                    out[i] = ValueError("allowed conversion: the generator is not the value sum's")
                else:
                    out[i] = AllowedConversion.from_parts(assets, generator, cmus[k].tobytes())
        return out

    @staticmethod
    def conversion_tree(conversions, ctx=None):
        """The tree of allowed conversions: a FrozenCommitmentTree over the conversions' commitment()s, built on ctx's GPU or with ctx=None
        on the host."""
        return FrozenCommitmentTree([c.commitment() for c in conversions], ctx)
