"""bench.py --dump-outputs without a GPU: what dump_outputs writes from a trainer-shaped object (every loss, the G / D
weights and their moving averages), the dtypes, the seeded sample of a large network and the 64 MB cap."""
import os
import types

import numpy as np
import torch

import bench


def _trainer():
    torch.manual_seed(0)
    big = torch.nn.Linear(3000, 700)        # 2 100 700 elements: more than DUMP_SAMPLE, so it is sampled
    small = torch.nn.Sequential(torch.nn.Linear(10, 4), torch.nn.InstanceNorm2d(4, affine=True, track_running_stats=True))
    return types.SimpleNamespace(gen=big, dis=small, gen_copy=big, dis_copy=small,
                                 loss_dis_all=torch.tensor(1.25), loss_gen_total=torch.tensor([0.5]),
                                 loss_gen_vgg=0, loss_ds=0.75, loss_flag=True, not_a_loss=torch.tensor(3.0))


def _flat(module):
    return torch.cat([t.detach().reshape(-1).float() for t in module.state_dict().values() if t.is_floating_point()]).numpy()


def test_dump_outputs_files_dtypes_and_sample(tmp_path):
    tr = _trainer()
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(tr, str(a))
    bench.dump_outputs(tr, str(b))
    names = sorted(os.listdir(a))
    assert names == sorted(["loss_dis_all.npy", "loss_ds.npy", "loss_gen_total.npy", "loss_gen_vgg.npy"] +
                           [n + "_state.npy" for n in bench.DUMP_NETS])
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == (np.float64 if n.startswith("loss_") else np.float32), n
        np.testing.assert_array_equal(x, y)           # the same sample positions every run
    assert np.load(a / "loss_dis_all.npy").tolist() == [1.25]
    assert np.load(a / "loss_ds.npy").tolist() == [0.75]
    assert np.load(a / "loss_gen_vgg.npy").tolist() == [0.0]

    full = _flat(tr.gen)
    gen = np.load(a / "gen_state.npy")
    assert full.size > bench.DUMP_SAMPLE and gen.size == bench.DUMP_SAMPLE
    idx = np.sort(np.random.default_rng(1234).choice(full.size, bench.DUMP_SAMPLE, replace=False))
    np.testing.assert_array_equal(gen, full[idx])
    np.testing.assert_array_equal(np.load(a / "dis_state.npy"), _flat(tr.dis))   # small enough to be written whole


def test_dump_outputs_stay_under_64_mb():
    # losses are a few bytes each; every network contributes at most DUMP_SAMPLE float32 values
    assert len(bench.DUMP_NETS) * bench.DUMP_SAMPLE * 4 + 4096 <= 64 << 20
