"""The test-only shim tests/native/device_math_host.hip, shared by the modules that load it.  The shim is compiled with the product's
own flags (FLAGS of masp_amd/csrc/Makefile, as native_build.py reads them from the Makefile), so that the device code it tests is the code
as it ships."""
import native_build
from native_build import HIPCC, ROOT, makefile_flags

UNIT = native_build.unit("device_math_host")


def asm_command(out):
    """the shim's device assembly, as the Makefile's `asm` target makes the product's (input of tools/check_codeobj.py)"""
    return [HIPCC] + makefile_flags() + ["-w", "-S", "--cuda-device-only", UNIT.src, "-o", out]


def load():
    return native_build.load(UNIT)
