"""Two-rank synchronised batch norm on real GPUs over RCCL (skipped on machines with fewer than two devices; the one-rank RCCL form is
tests/test_sync_bn.py, the two-rank gloo form tests/test_sync_bn_gloo.py).  The ranks are separate processes started by
torch.distributed.run.  This file's name carries ``test_two_rank_rccl_training_step`` on purpose: tests/conftest.py moves the tests
whose id contains it to the front of the session, before anything has initialised the GPU in this process -- a process that has
must not start other GPU programs."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_two_rank_rccl_sync_bn():
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs; one-rank RCCL coverage is in test_sync_bn.py, two-rank gloo coverage in test_sync_bn_gloo.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29537", os.path.join(HERE, "helpers", "sync_bn_gpu_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [json.loads(l.split("SYNCBNRESULT ", 1)[1]) for l in out.stdout.splitlines() if "SYNCBNRESULT " in l]
    assert len(res) == 2
    for r in res:
        assert r["same_params"] and r["same_buffers"] and r["buffers_moved"], r
        assert r["worlds"] == [2] * 4 and not r["warnings"], r
        assert all(n > 0 and n % 2 == 0 for n in r["all_gathers"]) and len(set(r["all_gathers"])) == 1, r
