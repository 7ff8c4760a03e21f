"""The test-only shim tests/native/spend_build_dev.hip (device/spend_build.hpp on the host, and the product's spend-building and
signing kernels on the GPU, one alone or all), with the product's flags as native_build.py reads them from the Makefile."""
import ctypes as C

import numpy as np

import native_build

UNIT = native_build.unit("spend_build_dev")
SIGN_STAGES = ("key", "nonce_hash", "nonce_point", "finish")     # stage k + 1 is kernel k_rs_<name>
SIGN_PARTS = ("state", "status", "vk", "sig")
SPEND_STAGES = ("parse", "keys", "commit", "cv", "finish")       # stage k + 1 is kernel k_sb_<name>
SPEND_PARTS = ("state", "status", "cv", "rk", "nf", "cmu", "nk")
TABLES = {"spend": 0, "pgk": 1, "vcr": 2}
_lib = None


def load():
    global _lib
    if _lib is None:
        _lib = native_build.load(UNIT)
        for f in (_lib.sbd_sign_block_bytes, _lib.sbd_spend_block_bytes):
            f.restype = C.c_size_t
            f.argtypes = [C.c_uint32]
        _lib.sbd_sign_block_layout.argtypes = _lib.sbd_spend_block_layout.argtypes = [C.c_uint32, C.c_void_p]
        _lib.sbd_table_mul_host.argtypes = [C.c_int, C.c_char_p, C.c_char_p]
        _lib.sbd_reduce_wide_host.argtypes = [C.c_char_p, C.c_char_p]
        _lib.sbd_reduce_wide_host.restype = None
        _lib.sbd_mul_add_host.argtypes = [C.c_char_p] * 4
        _lib.sbd_mul_add_host.restype = None
        for f in (_lib.sbd_sign_stage_host, _lib.sbd_sign_stage_gpu):
            f.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 6
        for f in (_lib.sbd_spend_stage_host, _lib.sbd_spend_stage_gpu):
            f.argtypes = [C.c_int, C.c_uint32] + [C.c_void_p] * 12
    return _lib


def table_mul(table, k):
    """[k] G from the device's fixed-base table ("spend", "pgk" or "vcr"), on the host -> 32 bytes"""
    out = C.create_string_buffer(32)
    assert load().sbd_table_mul_host(TABLES[table], int(k).to_bytes(32, "little"), out) == 0
    return out.raw


def reduce_wide(x):
    """the header's wide reduction of an integer below 2^512 -> an integer"""
    out = C.create_string_buffer(32)
    load().sbd_reduce_wide_host(int(x).to_bytes(64, "little"), out)
    return int.from_bytes(out.raw, "little")


def mul_add(r, c, k):
    """the header's r + c k mod r_J of three integers below r_J -> an integer"""
    out = C.create_string_buffer(32)
    load().sbd_mul_add_host(*[int(x).to_bytes(32, "little") for x in (r, c, k)], out)
    return int.from_bytes(out.raw, "little")


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class _Kind:
    def __init__(self, name, part_names, n_layout):
        self.name, self.part_names, self.n_layout = name, part_names, n_layout

    def new_block(self, n):
        """the zeroed block of n items: everything the kernels hand each other"""
        return np.zeros(getattr(load(), "sbd_%s_block_bytes" % self.name)(n), np.uint8)

    def parts(self, block, n):
        """{name: the part's bytes} of a block, and the state's item size"""
        lay = np.zeros(self.n_layout, np.uint64)
        getattr(load(), "sbd_%s_block_layout" % self.name)(n, _p(lay))
        k = len(self.part_names)
        at = [int(x) for x in lay[:k]] + [block.size]
        return {name: block[at[i]:at[i + 1]] for i, name in enumerate(self.part_names)}, int(lay[k])

    def _run(self, where, stage, arrays, block):
        out = block.copy()
        rc = getattr(load(), "sbd_%s_stage_%s" % (self.name, where))(int(stage), arrays[0].shape[0], *[_p(a) for a in arrays], _p(out))
        assert rc == 0, rc
        return out

    def stage_host(self, stage, arrays, block):
        """stage k >= 1 of the header's steps on the CPU over a copy of `block`, 0: all of them -> the block after it"""
        return self._run("host", stage, arrays, block)

    def stage_gpu(self, stage, arrays, block):
        """the product's kernel `stage` alone, or all of them (0), on the GPU over a copy of `block` -> the block after it"""
        return self._run("gpu", stage, arrays, block)


sign = _Kind("sign", SIGN_PARTS, 6)
spend = _Kind("spend", SPEND_PARTS, 9)


def sign_results(block, n):
    """(status, vks, sigs) of a block that went through every stage"""
    p, _ = sign.parts(block, n)
    return p["status"][:n].copy(), p["vk"][:32 * n].reshape(n, 32), p["sig"][:64 * n].reshape(n, 64)


def spend_results(block, n):
    """(status, cvs, rks, nfs, cmus, nks) of a block that went through every stage"""
    p, _ = spend.parts(block, n)
    return (p["status"][:n].copy(),) + tuple(p[f][:32 * n].reshape(n, 32) for f in ("cv", "rk", "nf", "cmu", "nk"))
