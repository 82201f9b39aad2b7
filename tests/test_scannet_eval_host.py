"""Host side of ScanNet validation / whole-room testing: the multi-step schedule against the values the reference's own
MultiStepLRScheduler returned (tests/golden/scannet_eval.npz, tests/tools/gen_golden_scannet_eval.py), the factory on the
ScanNet config's keys, the benchmark's label ids, and the numpy restatements of tests/scannet_eval_ref.py -- which the GPU
tests use where the reference leaves an order unspecified -- pinned to what the reference's own code returned."""
import bisect

import numpy as np
import pytest
import torch

import amcontrast3d_amd
import scannet_eval_ref as ref
from conftest import load_golden

amcontrast3d_amd.activate()

from openpoints.scheduler import CosineLRScheduler, MultiStepLRScheduler, build_scheduler_from_cfg  # noqa: E402
from openpoints.utils import EasyConfig  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return load_golden("scannet_eval")


def _opt(lr=0.001, groups=1):
    return torch.optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr * (j + 1)} for j in range(groups)], lr=lr)


@pytest.mark.parametrize("tag", ["plain", "warmup"])
def test_multistep_values_equal_the_reference_run(g, tag):
    """same Python floats, same operations: exactly equal, epochs 0..100, through get_epoch_values and through step()"""
    s = g["meta"]["sched"]
    warm = s["warmup_epochs"] if tag == "warmup" else 0
    opt = _opt(s["lr"])
    sched = MultiStepLRScheduler(opt, decay_t=s["decay_epochs"], decay_rate=s["decay_rate"], warmup_t=warm,
                                 warmup_lr_init=s["warmup_lr"])
    assert opt.param_groups[0]["lr"] == float(g[f"sched/{tag}/initial"])
    want = g[f"sched/{tag}/lr"]
    assert want.shape == (101,)
    got = [sched.get_epoch_values(t)[0] for t in range(101)]
    assert got == want.tolist()
    for t in range(101):
        sched.step(t)
        assert opt.param_groups[0]["lr"] == want[t]
    # the boundary of bisect_right(decay_t, t + 1): the value set at the end of epoch 69 (for epoch 70) is the decayed one
    assert got[68] == s["lr"] and got[69] == s["lr"] * s["decay_rate"] and got[88] == got[69]
    assert got[89] == s["lr"] * s["decay_rate"] ** 2 == got[100]
    assert sched.get_curr_decay_steps(68) == 0 and sched.get_curr_decay_steps(69) == 1 == bisect.bisect_right([70, 90], 70)
    assert sched.get_update_values(10) is None
    if warm:
        assert got[0] == s["warmup_lr"] and got[:warm] == [s["warmup_lr"] + t * (s["lr"] - s["warmup_lr"]) / warm for t in range(warm)]


def test_multistep_param_groups_state_and_noise():
    opt = _opt(0.002, groups=2)
    opt.param_groups[1]["lr_scale"] = 0.5
    sched = MultiStepLRScheduler(opt, decay_t=[3, 5], decay_rate=0.1)
    sched.step(2)
    assert [grp["lr"] for grp in opt.param_groups] == [0.002 * 0.1, 0.004 * 0.1 * 0.5]
    state = sched.state_dict()
    assert "optimizer" not in state
    other = MultiStepLRScheduler(_opt(0.002, groups=2), decay_t=[100], decay_rate=0.5)
    other.load_state_dict(state)
    assert other.get_epoch_values(4) == sched.get_epoch_values(4) == [0.002 * 0.1 ** 2, 0.004 * 0.1 ** 2]
    per_update = MultiStepLRScheduler(_opt(), decay_t=[3], decay_rate=0.1, t_in_epochs=False)
    assert per_update.get_epoch_values(5) is None and per_update.get_update_values(5) == [0.001 * 0.1]
    with pytest.raises(NotImplementedError):
        MultiStepLRScheduler(_opt(), decay_t=[3], noise_range_t=10)


def test_build_scheduler_from_cfg_on_the_scannet_keys(g):
    """cfgs/scannet/default.yaml:70-81: sched multistep, decay_epochs [70, 90], decay_rate 0.1, warmup_epochs 0"""
    cfg = EasyConfig()
    cfg.update({"lr": 0.001, "epochs": 100, "sched": "multistep", "decay_epochs": [70, 90], "decay_rate": 0.1, "warmup_epochs": 0,
                "min_lr": None})
    opt = _opt(cfg.lr)
    sched, epochs = build_scheduler_from_cfg(cfg, opt, return_epochs=True)
    assert type(sched) is MultiStepLRScheduler and epochs == 100
    assert [sched.get_epoch_values(t)[0] for t in range(101)] == g["sched/plain/lr"].tolist()
    cfg.update({"warmup_epochs": 5, "warmup_lr": 1.0e-6})
    sched = build_scheduler_from_cfg(cfg, _opt(cfg.lr))
    assert [sched.get_epoch_values(t)[0] for t in range(101)] == g["sched/warmup/lr"].tolist()
    # scheduler_factory.py:19: without decay_rate, final_decay_rate ** (1 / epochs)
    bare = EasyConfig()
    bare.update({"lr": 0.001, "epochs": 100, "sched": "multistep", "decay_epochs": [70, 90]})
    assert build_scheduler_from_cfg(bare, _opt()).decay_rate == 0.01 ** (1 / 100)
    # the other schedules keep their behaviour
    cos = EasyConfig()
    cos.update({"lr": 0.01, "epochs": 100, "sched": "cosine", "min_lr": 1e-5})
    assert type(build_scheduler_from_cfg(cos, _opt(0.01))) is CosineLRScheduler
    for name in ("step", "tanh", "poly", "plateau"):
        cos.sched = name
        with pytest.raises(NotImplementedError):
            build_scheduler_from_cfg(cos, _opt(0.01))
    cfg.update({"lr_noise": [0.5, 0.9]})
    with pytest.raises(NotImplementedError):
        build_scheduler_from_cfg(cfg, _opt())


def test_scannet_benchmark_ids():
    from amcontrast3d_amd import evaluate
    ids = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39]  # the benchmark's VALID_CLASS_IDS
    assert list(evaluate.SCANNET_VALID_CLASS_IDS) == ids
    pred = np.array([0, 19, 12, 13, 11, 0], dtype=np.int64)
    got = evaluate.scannet_benchmark_ids(pred)
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.tolist() == [1, 39, 14, 16, 12, 1]
    got_t = evaluate.scannet_benchmark_ids(torch.from_numpy(pred))
    assert torch.is_tensor(got_t) and got_t.dtype == torch.int64 and got_t.tolist() == got.tolist()
    assert evaluate.scannet_benchmark_ids(np.arange(20)).tolist() == ids
    for bad in ([20], [-1], [-100]):
        with pytest.raises(ValueError):
            evaluate.scannet_benchmark_ids(np.array(bad))
        with pytest.raises(ValueError):
            evaluate.scannet_benchmark_ids(torch.tensor(bad))


@pytest.mark.parametrize("tag", ["a", "b"])
def test_restatement_equals_the_reference_run(g, tag):
    """sub-clouds of the test route and the val item, bit for bit on the reference's own picks; the fixture's own claims"""
    room = ref.fixture_room(g, tag)
    shifted = room["coord"] - room["coord"].min(0)
    count = room["count"]
    P = int(count.max())
    assert room["parts"].shape == (P, len(count))
    assert (count == 1).any() and (count == 2).any() and (count >= 3).any() and (P % count != 0).any()
    perm, start = ref.fixture_perm(room)
    for i in range(P):
        assert np.array_equal(room["idx_sort"][start[perm[i]] + i % count[perm[i]]], room["parts"][i])
        pos, x, heights, inp = ref.fixture_part(room, g["meta"]["rows"], i)
        got = ref.sub_cloud(shifted, room["feat"], room["parts"][i], "test")
        for a, b in zip(got, (pos, x, heights)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert np.array_equal(ref.assemble(*got), inp)
    got = ref.sub_cloud(shifted, room["feat"], room["val/idx_unique"], "val")
    for a, k in zip(got, ("val/pos", "val/x", "val/heights")):
        assert np.array_equal(a, room[k])
    assert np.array_equal(ref.assemble(*got), room["val/input"])
    assert np.array_equal(room["label"][room["val/idx_unique"]], room["val/y"]) and (room["val/y"] == -100).any()
    raw_max = ((room["feat"][room["val/idx_unique"]] + 1) * 127.5).max()
    assert (raw_max > 1) == (tag == "a")  # the / 255 branch taken (a) and not taken (b)
    # a stable sort orders the voxels as the reference's sort does; only the order inside a voxel is its own
    idx_sort, voxel_idx, st, ct = ref.stable_tables(shifted)
    assert np.array_equal(ct, count) and np.array_equal(voxel_idx, room["voxel_idx"]) and np.array_equal(st, start)
    assert np.array_equal(np.sort(idx_sort), np.arange(len(shifted)))


def test_vote_restatement_is_the_mean():
    rng = np.random.default_rng(0)
    room = ref.make_room(920, 300, 3, 5)
    shifted = room[0] - room[0].min(0)
    idx_sort, voxel_idx, start, count = ref.stable_tables(shifted)
    P, nvox, C = int(count.max()), len(count), 5
    perm = np.stack([rng.permutation(nvox) for _ in range(P)])
    where = np.argsort(perm, axis=1)
    parts = np.stack([idx_sort[start[perm[i]] + i % count[perm[i]]] for i in range(P)])
    logits = rng.standard_normal((P, C, nvox)).astype(np.float32)
    got, mag, k = ref.vote(logits, where, start, count, idx_sort, voxel_idx, np.float64)
    flat = logits.transpose(0, 2, 1).reshape(-1, C).astype(np.float64)
    want = np.zeros((len(shifted), C))
    np.add.at(want, parts.reshape(-1), flat)
    cnt = np.bincount(parts.reshape(-1), minlength=len(shifted))
    assert np.array_equal(cnt, k) and cnt.min() >= 1 and len(set(cnt.tolist())) > 1
    np.testing.assert_allclose(got, want / cnt[:, None], rtol=1e-13, atol=1e-15)
    f32 = ref.vote(logits, where, start, count, idx_sort, voxel_idx)[0]
    assert f32.dtype == np.float32 and (np.abs(f32 - got) <= ref.vote_bound(mag, k)).all()
