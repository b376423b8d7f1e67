"""Two data-parallel ranks on the box's one GPU over gloo (tests/parallel_two_ranks_worker.py): what a one-rank collective cannot show,
that W ranks with B / W pairs each do what one rank does with all B — state broadcast, one reduced gradient against float64 autograd of
the oracle on the whole batch, the head's BatchNorm over the whole batch, bit-identical replicas after two full steps.  The children
are started with subprocess before they touch the GPU (never an exec of this process); three processes use the card at once."""
import json
import os
import subprocess
import sys

import pytest

from tests.gpu_guard import record_dir

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_train_as_one_rank_on_the_whole_batch():
    port = str(29400 + os.getpid() % 150)
    record = os.path.join(record_dir(), "parallel_parity.json")
    if os.path.exists(record):
        os.remove(record)
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, SWF_PARITY_LOG="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(REPO, "tests", "parallel_two_ranks_worker.py")], cwd=REPO, env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for rank, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0 and f"rank {rank} ok" in out, f"rank {rank} rc={p.returncode}\n{out[-3000:]}"
    with open(record) as f:
        rec = json.load(f)
    assert rec["world_size"] == 2 and 0.0 <= rec["worst_gradient_distance"] <= 5e-3, rec
