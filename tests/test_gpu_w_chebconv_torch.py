"""pygsp_amd.nn.cheby_conv and ChebConv on the GPU: torch tensors through the engine and back, forward and backward, in
ONE fresh child process (tests/chebconv_child.py) - this process has libgspx loaded already, and the child imports
pygsp_amd.nn, and so torch, first."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chebconv_child.py")


def test_chebconv_on_torch_tensors_in_a_fresh_process():
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
    assert all(e < 1e-10 for e in record["errors"].values()), record
    assert all(b < a for a, b in zip(record["losses"], record["losses"][1:])), record
