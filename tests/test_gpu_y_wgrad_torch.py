"""nn.WeightedGraph and nn.cheby_filter's weight gradient on the GPU: torch tensors through the engine and back in ONE
fresh child process (tests/wgrad_child.py).  This process has libgspx loaded already, so importing torch here would put
two HIP runtimes into it; the child imports pygsp_amd.nn - and so torch - first."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "wgrad_child.py")


def test_weighted_graph_through_the_engine_in_a_fresh_process():
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
    for lap_type in ("combinatorial", "normalized"):
        assert all(e < 1e-10 for e in record["errors"][lap_type].values()), record
    assert all(b < a for a, b in zip(record["dense_losses"], record["dense_losses"][1:])), record
    assert all(b < a for a, b in zip(record["losses"], record["losses"][1:])), record
