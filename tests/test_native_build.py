"""tests/native_build.py on a throw-away unit: a .hip with one empty kernel that includes one local header, in a directory that stands in
for the repository (with a copy of the Makefile, so that the test sets every mtime the rule looks at).  No GPU: hipcc cross-compiles."""
import ctypes as C
import glob
import os
import shutil
import time

import pytest

import native_build

SOURCE = '#include <hip/hip_runtime.h>\n#include "inc/local.hpp"\n__global__ void k_empty() {}\nextern "C" int tnb_value() { return TNB_VALUE; }\n'


class Tree:
    def __init__(self, root, monkeypatch):
        self.root = str(root)
        os.makedirs(os.path.join(self.root, "inc"))
        self.header = self.write("inc/local.hpp", "#define TNB_VALUE 7\n")
        self.other = self.write("inc/other.hpp", "#define TNB_OTHER 1\n")
        self.makefile = os.path.join(self.root, "Makefile")
        shutil.copy(native_build.MAKEFILE, self.makefile)
        self.unit = native_build.Unit(self.write("unit.hip", SOURCE), os.path.join(self.root, "_unit.so"), ())
        self.compiles = 0
        run = native_build.subprocess.run

        def counted(*args, **kw):
            self.compiles += 1
            return run(*args, **kw)

        monkeypatch.setattr(native_build, "ROOT", self.root)
        monkeypatch.setattr(native_build, "MAKEFILE", self.makefile)
        monkeypatch.setattr(native_build, "_libs", {})
        monkeypatch.setattr(native_build.subprocess, "run", counted)

    def write(self, name, text):
        path = os.path.join(self.root, name)
        with open(path, "w") as f:
            f.write(text)
        return path

    def settle(self):
        """every file of the tree as old as every other, well in the past: whatever is touched afterwards is the newer one"""
        t = time.time() - 1000
        for dirpath, _, names in os.walk(self.root):
            for n in names:
                os.utime(os.path.join(dirpath, n), (t, t))

    def loads(self):
        """load the unit -> how many compilers that started"""
        before = self.compiles
        native_build.load(self.unit)
        return self.compiles - before


@pytest.fixture
def tree(tmp_path, monkeypatch):
    return Tree(tmp_path, monkeypatch)


def test_one_staleness_rule_from_the_compilers_own_dependencies(tree):
    unit = tree.unit
    assert native_build.stale(unit)
    assert tree.loads() == 1 and native_build.load(unit).tnb_value() == 7
    # source and header recorded, relative to the root, and nothing from outside it (the HIP headers are)
    deps = unit.dependencies()
    assert deps == ["inc/local.hpp", "unit.hip"]
    assert not any(os.path.isabs(d) or d.startswith("..") for d in deps)
    assert tree.loads() == 0
    native_build._libs.clear()                      # a later process
    tree.settle()
    assert not native_build.stale(unit) and tree.loads() == 0
    os.utime(tree.other)
    assert not native_build.stale(unit) and tree.loads() == 0
    os.utime(tree.header)
    native_build._libs.clear()
    assert native_build.stale(unit) and tree.loads() == 1 and not native_build.stale(unit)
    tree.settle()
    os.utime(tree.makefile)
    assert native_build.stale(unit)
    tree.settle()
    os.remove(unit.so + ".d")
    native_build._libs.clear()
    assert native_build.stale(unit) and tree.loads() == 1 and unit.dependencies() == deps
    tree.settle()
    os.remove(tree.header)
    assert native_build.stale(unit)


def test_a_failed_compile_keeps_the_previous_library(tree):
    unit = tree.unit
    native_build.build([unit])
    before = open(unit.so, "rb").read(), open(unit.so + ".d").read()
    tree.settle()
    tree.write("unit.hip", SOURCE + "#error not today\n")
    with pytest.raises(RuntimeError, match="not today"):
        native_build.load(unit)
    assert (open(unit.so, "rb").read(), open(unit.so + ".d").read()) == before
    assert C.CDLL(unit.so).tnb_value() == 7
    assert not glob.glob(os.path.join(tree.root, "*.tmp*"))
    assert native_build.stale(unit)
