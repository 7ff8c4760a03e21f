import os
import subprocess
import sys

import pytest

# The HIP runtime reads GPU_MAX_HW_QUEUES once, at the process's first HIP call — which in this process may be a test-side HIP unit
# (tests/native) loaded before libmasp_hip.so: say it here (round 5: the contexts' measured masp_hip_options::hw_queues showed the whole
# GPU suite running on the runtime's default of four).  Set, not defaulted: the suite asserts 16 (a context's 15 streams a queue each), and a
# launcher that exports a smaller value of its own would otherwise leave every context of the suite short of queues
os.environ["GPU_MAX_HW_QUEUES"] = "16"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session", autouse=True)
def _native_libraries_built():
    """Build the product libraries and the oracle if a fresh checkout has not been built yet (same as
    __graft_entry__.build(), minus the code-object audit).  hipcc cross-compiles without a GPU."""
    need = [os.path.join(ROOT, "masp_amd", "libmasp_host.so"), os.path.join(ROOT, "masp_amd", "libmasp_hip.so")]
    if not all(os.path.exists(p) for p in need):
        env = dict(os.environ)
        env["PATH"] = "/opt/rocm/bin:" + env.get("PATH", "")
        subprocess.check_call(["make", "-s", "-j8", "-C", os.path.join(ROOT, "masp_amd", "csrc")], env=env)
    if not os.path.exists(os.path.join(ROOT, "oracle", "_build", "liboracle.so")):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
