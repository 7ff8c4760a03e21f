"""The test-only shim tests/native/output_build_dev.hip (device/output_build.hpp on the host, and the product's output-building
kernels on the GPU, one alone or all), with the product's flags as native_build.py reads them from the Makefile."""
import ctypes as C

import numpy as np

import native_build

UNIT = native_build.unit("output_build_dev")
STAGES = ("parse", "memo", "commit", "cv", "ladder", "seal", "rows")     # stage k + 1 is kernel k_ob_<name>
PARTS = ("state", "status", "cv", "cmu", "epk", "memo", "cols", "enc", "cout")
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = native_build.load(UNIT)
        _lib.obd_block_bytes.restype = C.c_size_t
        _lib.obd_block_bytes.argtypes = [C.c_uint32]
        _lib.obd_block_layout.argtypes = [C.c_uint32, C.c_void_p]
        _lib.obd_table_mul_host.argtypes = [C.c_char_p, C.c_char_p]
        _lib.obd_seal_host.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int] + [C.c_char_p] * 9
        for f in (_lib.obd_stage_host, _lib.obd_stage_gpu):
            f.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 13
    return _lib


def table_mul(k):
    """[k] G_vcr from the device's fixed-base table, on the host -> 32 bytes"""
    out = C.create_string_buffer(32)
    assert load().obd_table_mul_host(int(k).to_bytes(32, "little"), out) == 0
    return out.raw


def seal(k_enc, plaintext, ovk, cv, cmu, epk, pk_d, esk, out_random=None, use_memo=True):
    """the seal step alone on the host, from K_enc on -> (enc_ciphertext[612], out_ciphertext[80]); ovk None: out_random's 96 bytes"""
    enc, cout = C.create_string_buffer(612), C.create_string_buffer(80)
    rc = load().obd_seal_host(bytes(k_enc), bytes(plaintext), int(use_memo), int(ovk is not None), bytes(ovk or bytes(32)), bytes(cv), bytes(cmu),
                              bytes(epk), bytes(pk_d), bytes(esk), None if out_random is None else bytes(out_random), enc, cout)
    assert rc == 0, rc
    return enc.raw, cout.raw


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def new_block(n):
    """the zeroed block of n outputs: everything the kernels hand each other"""
    return np.zeros(load().obd_block_bytes(n), np.uint8)


def parts(block, n):
    """{name: the part's bytes} of a block, the state as [n_pad, sizeof(ObState)] and the rest flat"""
    lay = np.zeros(11, np.uint64)
    load().obd_block_layout(n, _p(lay))
    at = [int(x) for x in lay[:9]] + [block.size]
    return {name: block[at[i]:at[i + 1]] for i, name in enumerate(PARTS)}


def results(block, n):
    """(status, cvs, cmus, epks, encs, couts) of a block that went through every stage"""
    p = parts(block, n)
    return (p["status"][:n].copy(), p["cv"][:32 * n].reshape(n, 32), p["cmu"][:32 * n].reshape(n, 32), p["epk"][:32 * n].reshape(n, 32),
            p["enc"][:612 * n].reshape(n, 612), p["cout"][:80 * n].reshape(n, 80))


def stage_host(stage, arrays, block):
    """stage 1..7 (STAGES) of the header's steps on the CPU over a copy of `block`, 0: all of them -> the block after it"""
    out = block.copy()
    rc = load().obd_stage_host(int(stage), arrays[0].shape[0], *[_p(a) for a in arrays], _p(out))
    assert rc == 0, rc
    return out


def stage_gpu(stage, arrays, block):
    """the product's kernel `stage` alone (1..7), or all seven (0), on the GPU over a copy of `block` -> the block after it"""
    out = block.copy()
    rc = load().obd_stage_gpu(int(stage), arrays[0].shape[0], *[_p(a) for a in arrays], _p(out))
    assert rc == 0, rc
    return out
