"""GPU: build() and smoke() of __graft_entry__ in one process.

`python __graft_entry__.py smoke` runs both in one interpreter.  build() ends
by loading the engine; if that happens before torch is imported, the process
holds the system's HIP runtime (librsmi.so's) and then the one a torch wheel
brings along, and smoke() fails at rs_new with "HIP device error".  A child
process runs build() with its make steps left out (the tree is built: the
suite could not run otherwise) and then smoke().
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
if not torch.cuda.is_available():
    pytest.skip("no GPU", allow_module_level=True)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = """
import subprocess, sys
sys.path.insert(0, {root!r})
import __graft_entry__ as g
assert "torch" not in sys.modules and "rsmi" not in sys.modules
subprocess.run = lambda *a, **k: None   # the make steps: everything is built
g.build()
assert "rsmi" in sys.modules
g.smoke()
"""


def test_build_then_smoke_in_one_process():
    run = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT)], capture_output=True, text=True, timeout=120,
                         cwd=ROOT)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "smoke ok" in run.stdout
