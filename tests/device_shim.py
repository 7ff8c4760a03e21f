"""Build of the test-only shim tests/native/device_math_host.hip, shared by the modules that load it.  The shim is compiled with
the product's own flags (FLAGS of masp_amd/csrc/Makefile, read from the Makefile), so that the device code it tests is the code
as it ships, and it is rebuilt whenever it or any header it includes is newer than the library."""
import ctypes as C
import glob
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "native", "device_math_host.hip")
SO = os.path.join(HERE, "native", "_device_math_host.so")
MAKEFILE = os.path.join(ROOT, "masp_amd", "csrc", "Makefile")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"


def makefile_flags():
    """FLAGS of masp_amd/csrc/Makefile as a list, $(ARCH) replaced by the Makefile's ARCH"""
    text = open(MAKEFILE).read()
    var = {}
    for name in ("ARCH", "FLAGS"):
        m = re.search(r"^%s\s*\?=\s*(.*)$" % name, text, re.M)
        assert m, "no %s in %s" % (name, MAKEFILE)
        var[name] = m.group(1).strip()
    flags = var["FLAGS"].replace("$(ARCH)", var["ARCH"])
    assert "$(" not in flags, flags
    return flags.split()


def build_command(out=SO):
    flags = makefile_flags()
    return [HIPCC] + flags + [f for f in ("-fPIC",) if f not in flags] + ["-shared", SRC, "-o", out]


def asm_command(out):
    """the shim's device assembly, as the Makefile's `asm` target makes the product's (input of tools/check_codeobj.py)"""
    return [HIPCC] + makefile_flags() + ["-w", "-S", "--cuda-device-only", SRC, "-o", out]


def dependencies():
    dev = os.path.join(ROOT, "masp_amd", "csrc", "device")
    return sorted(glob.glob(os.path.join(dev, "*.hpp")) + glob.glob(os.path.join(dev, "*.h"))) + \
        [os.path.join(ROOT, "tools", "fp28.hpp"), SRC, MAKEFILE]


_lib = None


def load():
    """the shim as a ctypes library, rebuilt first if missing or older than any of its sources"""
    global _lib
    if _lib is None:
        newest = max(os.path.getmtime(p) for p in dependencies())
        if not os.path.exists(SO) or os.path.getmtime(SO) < newest:
            tmp = SO + ".%d.tmp" % os.getpid()
            subprocess.check_call(build_command(tmp))
            os.replace(tmp, SO)
        _lib = C.CDLL(SO)
    return _lib
