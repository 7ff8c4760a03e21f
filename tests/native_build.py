"""How the tests' native units (tests/native/*.hip, a shared library each) get built and loaded: the only place in tests/ that knows.
A unit is compiled with the product's own flags (FLAGS of masp_amd/csrc/Makefile, read from the Makefile), so that the device code it tests
is the code as it ships.  The compiler writes the unit's dependencies (-MD: those of the host pass, and no unit includes a file in its
device pass alone); the files of them that lie in the repository are kept next to the library, as _<name>.so.d, relative to the
repository's root.  A unit is rebuilt when its library or that list is missing, when a file
on the list is gone, or when the library is older than a file on the list, than the list or than the Makefile.
`python tests/native_build.py` builds whatever is stale of the units the *_shim modules declare, at most JOBS compilers at a time."""
import collections
import concurrent.futures
import ctypes as C
import glob
import importlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MAKEFILE = os.path.join(ROOT, "masp_amd", "csrc", "Makefile")
HIPCC = "/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else "hipcc"
JOBS = 8        # the -j8 of tests/conftest.py
UNITS = []      # every unit declared through unit(), in the order of declaration
_libs = {}


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


class Unit(collections.namedtuple("Unit", "src so defines")):
    def command(self, out=None):
        out = out or self.so
        return [HIPCC] + makefile_flags() + list(self.defines) + ["-shared", self.src, "-o", out, "-MD", "-MF", out + ".d"]

    def dependencies(self):
        """the in-tree files the library was built from, relative to the repository's root, as its build recorded them"""
        return open(self.so + ".d").read().splitlines()


def unit(name, suffix="", defines=()):
    """tests/native/<name>.hip -> tests/native/_<name><suffix>.so"""
    u = Unit(os.path.join(HERE, "native", name + ".hip"), os.path.join(HERE, "native", "_%s%s.so" % (name, suffix)), tuple(defines))
    UNITS.append(u)
    return u


def stale(u):
    if not os.path.exists(u.so) or not os.path.exists(u.so + ".d"):
        return True
    deps = [os.path.join(ROOT, p) for p in u.dependencies()] + [u.so + ".d", MAKEFILE]
    return not all(os.path.exists(p) for p in deps) or os.path.getmtime(u.so) < max(os.path.getmtime(p) for p in deps)


def _in_tree(depfile):
    """the compiler's dependency file (make rules) -> the files under ROOT, relative to it, sorted"""
    root = os.path.realpath(ROOT)
    rules = open(depfile).read().replace("\\\n", " ").splitlines()
    rel = {os.path.relpath(os.path.realpath(p), root) for rule in rules if ": " in rule for p in rule.split(": ", 1)[1].split()}
    return sorted(p for p in rel if not p.startswith(".."))


def _compile(u):
    tmp = u.so + ".%d.tmp" % os.getpid()
    try:
        r = subprocess.run(u.command(tmp), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode:
            raise RuntimeError("%s failed (%d):\n%s" % (" ".join(u.command(tmp)), r.returncode, r.stdout))
        sys.stderr.write(r.stdout)
        deps = _in_tree(tmp + ".d")
        with open(tmp + ".d", "w") as f:
            f.write("\n".join(deps) + "\n")
        os.utime(tmp)       # the library is no older than the list written after it
        os.replace(tmp + ".d", u.so + ".d")
        os.replace(tmp, u.so)
    finally:
        for p in (tmp, tmp + ".d"):
            if os.path.exists(p):
                os.remove(p)


def build(units, jobs=JOBS):
    """compile the stale ones of `units`, at most `jobs` side by side -> those it compiled"""
    todo = [u for u in units if stale(u)]
    if todo:
        with concurrent.futures.ThreadPoolExecutor(min(jobs, len(todo))) as pool:
            list(pool.map(_compile, todo))
    return todo


def load_all(units):
    """the units as ctypes libraries (one per process), the stale ones built side by side first"""
    units = list(units)
    build([u for u in units if u.so not in _libs])
    for u in units:
        if u.so not in _libs:
            _libs[u.so] = C.CDLL(u.so)
    return [_libs[u.so] for u in units]


def load(u):
    return load_all([u])[0]


def declared_units():
    """the units of all *_shim modules"""
    for path in sorted(glob.glob(os.path.join(HERE, "*_shim.py"))):
        importlib.import_module(os.path.basename(path)[:-3])
    return list(UNITS)


def main():
    sys.path.insert(0, ROOT)
    units = declared_units()
    built = build(units)
    for u in built:
        print("built", os.path.relpath(u.so, ROOT))
    print("%d of %d units were stale" % (len(built), len(units)))


if __name__ == "__main__":
    import native_build     # the module the shims import, not a second copy of it under the name __main__
    native_build.main()
