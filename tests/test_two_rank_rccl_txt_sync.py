"""Two-rank text encoder over the ranks' union on real GPUs over RCCL (skipped on machines with fewer than two devices; the one-rank
RCCL form and the virtual ranks on one device are in tests/test_txt_group.py, the layout identities in tests/test_txt_regroup.py).
The ranks are separate processes started by torch.distributed.run.  The test's name carries ``test_two_rank_rccl_training_step`` on
purpose: tests/conftest.py moves the tests whose id contains it to the front of the session, before anything has initialised the GPU
in this process -- a process that has must not start other GPU programs."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def test_two_rank_rccl_training_step_txt_sync():
    """2 ranks x 3 sentences, eval mode: every rank's mu / logvar / style gradient match its rows of the single-process emulation
    (``group=None`` on the 6 samples) within 1e-4 of the emulation's scale -- launches of different batch size, the bound of
    tests/test_txt_group.py --, with one all-gather in the forward and one in the backward."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs >= 2 GPUs; one-rank RCCL and virtual-rank coverage is in test_txt_group.py")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(HERE, "helpers", "txt_sync_gpu_worker.py")]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    res = [json.loads(l.split("TXTSYNCRESULT ", 1)[1]) for l in out.stdout.splitlines() if "TXTSYNCRESULT " in l]
    assert len(res) == 2
    for r in res:
        print(r)
        assert r["world"] == 2 and r["all_gathers"] == 2 and r["finite"], r
        assert all(e <= 1e-4 for e in r["errs"]), r
