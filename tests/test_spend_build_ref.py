"""spend_build_ref, the other side of the spend-building and signing tests, against what pins it: the reference's ZIP 32 key vectors
(tests/golden/zip32_key_vectors.json: ak = [ask] G_spend, nk = [nsk] G_pgk), the product's Python signer and verifier, and the public
inputs of the Spend circuit's witness synthesis.  CPU only; every comparison is of bytes."""
import masp_amd
import spend_build_ref as R
from masp_amd import host as H
from masp_amd import redjubjub as RJS
from test_circuits import spend_instance


def _b(x):
    return x if isinstance(x, (bytes, bytearray)) else R._le(x)


def test_the_fixture_pins_both_basepoints():
    vectors = R.key_vectors()
    assert len(vectors) == 3
    for v in vectors:
        ask, nsk, ak, nk = (bytes.fromhex(v[f]) for f in ("ask", "nsk", "ak", "nk"))
        assert H.jubjub_mul(R.G_SPEND, ask) == ak and H.jubjub_mul(R.G_PGK, nsk) == nk
        status, vk, _ = R.sign_reference(dict(sk=ask, alpha=None, sighash=bytes(32), kind=0, T=bytes(80)))
        assert (status, vk) == (0, ak)                                # PublicKey::from_private on the spend authorisation basepoint
        spend = dict(R.good_spend(1), ak=ak, nsk=nsk)
        assert R.reference(spend)[5] == nk
        assert R.reference(dict(spend, ar=bytes(32)))[2] == ak        # rk with ar = 0


def test_reference_signatures_verify_and_equal_the_python_signer():
    items, want = R.references("edge_items", R.edge_items, R.sign_reference)
    items, want = items + R.sign_batch(6)[0], want + R.sign_batch(6)[1]
    seen = 0
    for it, (status, vk, sig) in zip(items, want):
        if status:
            continue
        seen += 1
        msg, g = vk + it["sighash"], R.BASE[it["kind"]]
        assert RJS.verify(vk, msg, sig, g)
        # the verification equation once more, through the host's point calls alone: [8] (R + [c] vk - [S] G) = O
        c = R.h_star(sig[:32], msg)
        acc = H.jubjub_sum([sig[:32], H.jubjub_mul(vk, c), H.jubjub_mul(g, sig[32:])], subtract=[False, False, True])
        assert H.jubjub_mul(acc, 8) == H.JUBJUB_IDENTITY
        assert not RJS.verify(vk, msg, sig[:32] + R._le((R._int(sig[32:]) + 1) % R.RJ), g)
        rsk = (R._int(it["sk"]) + (R._int(it["alpha"]) if it["alpha"] is not None else 0)) % R.RJ
        assert RJS.public_key(rsk, g) == vk
        assert RJS.sign(rsk, msg, g, rng=lambda n, T=it["T"]: T[:n]) == sig
    assert seen >= 30
    zero = [w for it, w in zip(items, want) if w[0] == 0 and (R._int(it["sk"]) + R._int(it["alpha"] or bytes(32))) % R.RJ == 0]
    assert len(zero) >= 2 and all(w[1] == H.JUBJUB_IDENTITY for w in zero)     # rsk = 0 is signed with: vk is the identity


def test_a_built_spend_carries_the_spend_circuits_public_inputs():
    assert masp_amd.note_encryption.BUILD_SPEND_STATUS.keys() == set(range(1, 10))
    for seed in (1, 2):
        inst, cmu, pk_d = spend_instance(seed, value=seed * 1000 + 9)
        inputs, _, cv, rk, nf = H.spend_assignment(check=True, **inst)
        spend = dict(asset=inst["asset_identifier"], value=inst["value"], d=inst["diversifier"], pk_d=pk_d, lead=1, rseed=_b(inst["rcm"]),
                     ak=inst["ak"], nsk=_b(inst["nsk"]), ar=_b(inst["ar"]), rcv=_b(inst["rcv"]), position=inst["position"])
        status, cv_r, rk_r, nf_r, cmu_r, nk_r = R.reference(spend)
        assert (status, cv_r, rk_r, nf_r, cmu_r) == (0, bytes(cv), bytes(rk), bytes(nf), bytes(cmu))
        pub = [int.from_bytes(inputs[i].tobytes(), "little") for i in range(8)]
        assert pub[1:3] == list(H.point_uv(rk_r)) and pub[3:5] == list(H.point_uv(cv_r))
        assert pub[5] == R._int(H.merkle_root(cmu_r, inst["path_siblings"], inst["position"])) == R._int(_b(inst["anchor"]))
        assert pub[6:8] == H.multipack(nf_r)
