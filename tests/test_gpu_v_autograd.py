"""pygsp_amd.nn on the GPU: torch tensors through the engine and back, forward and backward, in ONE fresh child process
(tests/autograd_child.py).  This process has libgspx loaded already, so importing torch here would put two HIP runtimes
into it; the child imports pygsp_amd.nn - and so torch - first."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "autograd_child.py")


def test_torch_tensors_through_the_engine_in_a_fresh_process():
    run = subprocess.run(["timeout", "-k", "10", "120", sys.executable, CHILD], capture_output=True, text=True)
    print(run.stdout)
    print(run.stderr, file=sys.stderr)
    assert run.returncode == 0, "the child ended with status {}:\n{}".format(run.returncode, run.stderr[-4000:])
    lines = [ln for ln in run.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, run.stdout
    record = json.loads(lines[0])
    if "skip" in record:
        pytest.skip(record["skip"])
    assert record["path"] in ("zero_copy", "staged")
    assert (record["path"] == "zero_copy") == bool(record["ptr_found"]), record
    assert record["torch"] and record["hip_runtimes"], record
    assert all(e < 1e-10 for e in record["errors"].values()), record
    assert all(b < a for a, b in zip(record["losses"], record["losses"][1:])), record
