"""policyNN and the RL train step against goldens produced by the reference's network.py / train_RL.py arithmetic
(tests/golden/network_golden.npz, train_loss_golden.npz), and the data-parallel gradient sync on 2 gloo ranks (CPU)."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import sigma_zero_amd as sz
from sigma_zero_amd import train_rl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_policynn_reproduces_reference_init_and_forward(golden_dir):
    z = np.load(os.path.join(golden_dir, "network_golden.npz"))
    torch.manual_seed(0)
    net = sz.policyNN({}).eval()
    assert list(net.state_dict().keys()) == [str(k) for k in z["keys"]]           # the 252 keys, same order
    assert sum(p.numel() for p in net.parameters()) == int(z["n_params"]) == 22809420
    sd = net.state_dict()
    for k in ("conv1.weight", "conv_p2.bias", "fc_v1.weight", "fc_v2.bias", "resnet_blocks.0.conv1.weight", "resnet_blocks.18.conv2.weight"):
        assert np.array_equal(sd[k].flatten()[:4].numpy(), z["probe_" + k.replace(".", "_")]), k   # same RNG consumption order
    x = torch.from_numpy(z["x"].astype(np.float32))
    torch.set_num_threads(1)
    with torch.no_grad():
        p, v = net(x, inference=True)
        logits, _ = net(x, inference=False)
    assert np.allclose(p.numpy(), z["policy_softmax"], rtol=1e-5, atol=1e-8)
    assert np.allclose(logits.numpy(), z["policy_logits"], rtol=1e-4, atol=1e-6)
    assert np.allclose(v.numpy(), z["value"], rtol=1e-4, atol=1e-6)


def test_train_loss_matches_reference(golden_dir):
    z = np.load(os.path.join(golden_dir, "train_loss_golden.npz"))
    torch.manual_seed(0)
    net = sz.policyNN({})
    net.train()
    torch.set_num_threads(1)
    batch = {"states": torch.from_numpy(z["x"].astype(np.float32)), "actions": torch.from_numpy(z["p_target"]), "rewards": torch.from_numpy(z["v_target"])}
    loss, mse, ce = train_rl.loss_fn(net, batch, "cpu")
    assert abs(float(mse.detach()) - float(z["mse"])) < 1e-5 and abs(float(ce.detach()) - float(z["ce"])) < 1e-4


def test_collate_unpacks_like_reference():
    rng = np.random.RandomState(0)
    planes = rng.rand(5, 119, 8, 8) < 0.2
    packed = (planes.astype(np.uint8) * (1 << np.arange(8)).astype(np.uint8)).sum(-1).astype(np.uint8)     # generate_training_supervised.py:91
    ds = train_rl.SelfPlayDataset(list(packed), [np.array([3, 77])] * 5, [np.array([0.25, 0.75])] * 5, [1, -1, 0, 1, -1])
    batch = train_rl.SelfPlayDataset.collate([ds[i] for i in range(5)])
    assert batch["states"].shape == (5, 119, 8, 8) and np.array_equal(batch["states"].numpy().astype(bool), planes)
    assert float(batch["actions"][0, 77]) == 0.75 and float(batch["actions"].sum()) == 5.0
    assert batch["rewards"].tolist() == [1, -1, 0, 1, -1]


def test_device_batches_equal_dataloader_with_collate():
    """DeviceBatches (gather + bit unpack + scatter on the training device) yields the DataLoader + collatefn batches bit for bit"""
    rng = np.random.RandomState(1)
    n = 37
    planes = rng.rand(n, 119, 8, 8) < 0.2
    packed = list((planes.astype(np.uint8) * (1 << np.arange(8)).astype(np.uint8)).sum(-1).astype(np.uint8))
    aidx = [np.sort(rng.choice(4672, size=rng.randint(1, 40), replace=False)) for _ in range(n)]
    aprob = [(lambda v: v / v.sum())(rng.rand(len(a))) for a in aidx]
    rew = [float(rng.choice([-1, 0, 1])) for _ in range(n)]
    ds = train_rl.SelfPlayDataset(packed, aidx, aprob, rew)
    dl = torch.utils.data.DataLoader(ds, batch_size=8, shuffle=False, drop_last=True, collate_fn=train_rl.SelfPlayDataset.collate)
    db = train_rl.DeviceBatches(packed, aidx, aprob, rew, batch_size=8, device="cpu", shuffle=False)
    assert len(db) == len(dl) == 4
    for a, b in zip(dl, db):
        for k in ("states", "actions", "rewards"):
            assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    # shuffled: a permutation of the same samples, every sample at most once per pass, last partial batch dropped
    g = torch.Generator().manual_seed(3)
    seen = torch.cat([b["rewards"] for b in train_rl.DeviceBatches(packed, aidx, aprob, rew, batch_size=8, device="cpu", shuffle=True, generator=g)])
    assert seen.numel() == 32


def _make_batch(seed, n):
    g = torch.Generator().manual_seed(seed)
    return {"states": (torch.rand(n, 119, 8, 8, generator=g) < 0.15).float(),
            "actions": torch.softmax(torch.randn(n, 4672, generator=g) * 3, 1), "rewards": torch.randint(-1, 2, (n,), generator=g).float()}


def _ddp_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    torch.manual_seed(0)
    net = sz.policyNN({})
    net.eval()                                   # frozen BN statistics: DP must then equal large-batch training exactly
    opt, sched = train_rl.make_optimiser(net)
    sync = train_rl.GradSync(net, n_buckets=4)
    full = _make_batch(7, 4)
    mine = {k: v[rank * 2:(rank + 1) * 2] for k, v in full.items()}
    sync.zero(); sync.begin_step()
    loss, _, _ = train_rl.loss_fn(net, mine, "cpu")
    loss.backward()
    sync.finish_step()
    out[rank] = sync.flat.clone().numpy()
    opt.step()
    dist.barrier()
    dist.destroy_process_group()


def test_gradient_allreduce_two_ranks_equals_big_batch(tmp_path):
    world = 2
    port = 29500 + (os.getpid() % 2000)
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_ddp_worker, args=(world, port, out), nprocs=world, join=True)
    # single process, batch of 4
    torch.manual_seed(0)
    torch.set_num_threads(4)
    net = sz.policyNN({})
    net.eval()
    loss, _, _ = train_rl.loss_fn(net, _make_batch(7, 4), "cpu")
    loss.backward()
    ref = torch.cat([p.grad.flatten() for p in net.parameters()]).numpy()
    assert np.array_equal(out[0], out[1])                                   # both ranks hold the same averaged gradient
    assert np.allclose(out[0], ref, rtol=1e-4, atol=1e-7), float(np.abs(out[0] - ref).max())


def _agg_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out[rank] = train_rl.aggregate_throughput([100 * (rank + 1), 90 * (rank + 1)], 1.0 + rank)
    dist.destroy_process_group()


def test_bench_aggregation_two_ranks():
    """bench.py's multi-rank contract: value = units of ALL ranks / MAX wall time over ranks (weak scaling, no data-path collective)."""
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_agg_worker, args=(2, 31500 + (os.getpid() % 2000), out), nprocs=2, join=True)
    assert out[0] == out[1] == ([300.0, 270.0], 2.0)
    assert train_rl.aggregate_throughput([5, 4], 0.5) == ([5.0, 4.0], 0.5)


class _TinyNet(torch.nn.Module):
    """policyNN's (policy logits, value) surface with a handful of parameters: the multi-rank training loop is the subject, not the net"""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Linear(119 * 64, 4672)
        self.v = torch.nn.Linear(119 * 64, 1)

    def forward(self, x, inference=False):
        x = x.flatten(1)
        return self.p(x), torch.tanh(self.v(x))


def _fake_records(n, seed):
    rng = np.random.RandomState(seed)
    packed = [rng.randint(0, 256, size=(119, 8)).astype(np.uint8) for _ in range(n)]
    aidx = [np.sort(rng.choice(4672, size=rng.randint(1, 30), replace=False)) for _ in range(n)]
    aprob = [rng.dirichlet(np.ones(len(a))) for a in aidx]
    rew = rng.choice([-1, 0, 1], size=n).tolist()
    return packed, aidx, aprob, rew


def _uneven_worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(1)
    torch.manual_seed(0)
    net = _TinyNet()
    train_rl.sync_module_state(net, average_buffers=False)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    sync = train_rl.GradSync(net, n_buckets=3)
    # rank 0 holds 3 batches of 8, rank 1 holds 5 (+ a remainder): game lengths differ per rank in real self-play
    n = [3 * 8 + 2, 5 * 8 + 5][rank]
    dl = train_rl.DeviceBatches(*_fake_records(n, 10 + rank), batch_size=8, device="cpu", shuffle=True, generator=torch.Generator().manual_seed(rank))
    hist = train_rl.train(net, dl, opt, total_steps=2, sync=sync, device=torch.device("cpu"))
    out[rank] = (len(dl), len(hist), torch.cat([p.detach().flatten() for p in net.parameters()]).numpy())
    # a rank without a single full batch must not hang its peers either: MIN is 0, nobody steps
    dl0 = train_rl.DeviceBatches(*_fake_records([3, 40][rank], 20 + rank), batch_size=8, device="cpu")
    out[10 + rank] = len(train_rl.train(net, dl0, opt, total_steps=1, sync=sync, device=torch.device("cpu")))
    dist.barrier()
    dist.destroy_process_group()


def test_multi_rank_training_with_unequal_batch_counts_does_not_deadlock():
    """train_RL.py:219-264 on N ranks: every rank trains on its own games, so per-rank batch counts differ; every rank must run the
    same number of all-reduced steps (MIN over ranks) and end with identical parameters"""
    world = 2
    mgr = mp.get_context("spawn").Manager()
    out = mgr.dict()
    mp.spawn(_uneven_worker, args=(world, 33500 + (os.getpid() % 2000), out), nprocs=world, join=True)
    assert out[0][0] == 3 and out[1][0] == 5                      # local batch counts differ ...
    assert out[0][1] == out[1][1] == 3 * 3                        # ... both ranks ran MIN(3,5) batches in each of the 3 passes
    assert np.array_equal(out[0][2], out[1][2])                   # and hold the same parameters (same averaged gradients every step)
    assert out[10] == out[11] == 0


def test_optimiser_state_resume(tmp_path):
    """train_RL.py:189-197 by intent: RL_{n}.pt -> model, RL_opt_{n}.pt -> optimiser; a missing pair leaves both untouched"""
    torch.manual_seed(1)
    net = _TinyNet()
    opt = torch.optim.Adam(net.parameters(), lr=1e-4, weight_decay=1e-4)
    dl = train_rl.DeviceBatches(*_fake_records(16, 3), batch_size=8, device="cpu", shuffle=False)
    train_rl.train(net, dl, opt, total_steps=0)
    train_rl.save_cycle(net, opt, 4, str(tmp_path))
    net2 = _TinyNet()
    opt2 = torch.optim.Adam(net2.parameters(), lr=1e-4, weight_decay=1e-4)
    assert not train_rl.load_cycle(net2, opt2, 3, str(tmp_path))
    assert train_rl.load_cycle(net2, opt2, 4, str(tmp_path))
    for a, b in zip(net.parameters(), net2.parameters()):
        assert torch.equal(a, b)
    s1, s2 = opt.state_dict()["state"], opt2.state_dict()["state"]
    assert s1.keys() == s2.keys() and len(s1) > 0
    for k in s1:
        assert torch.equal(s1[k]["exp_avg"], s2[k]["exp_avg"]) and torch.equal(s1[k]["exp_avg_sq"], s2[k]["exp_avg_sq"]) and s1[k]["step"] == s2[k]["step"]
    # one more identical step on both: identical parameters afterwards (the Adam moments were really restored)
    train_rl.train(net, dl, opt, total_steps=0)
    train_rl.train(net2, dl, opt2, total_steps=0)
    for a, b in zip(net.parameters(), net2.parameters()):
        assert torch.equal(a, b)


def test_split_convs_refuse_weights_beyond_the_f16_range():
    """the train convolutions pack w * 2^10 into f16: a weight of 64 or more would become inf, so switching them on refuses such a model (ValueError) and leaves
    its forwards untouched; weights just below the limit are accepted"""
    from sigma_zero_amd.trainconv import enable_split_convs, disable_split_convs
    torch.manual_seed(0)
    net = sz.policyNN({})
    with torch.no_grad():
        net.resnet_blocks[3].conv2.weight[5, 7, 1, 1] = 63.9
    assert enable_split_convs(net) == 38
    disable_split_convs(net)
    with torch.no_grad():
        net.resnet_blocks[3].conv2.weight[5, 7, 1, 1] = -64.0
    with pytest.raises(ValueError, match="resnet_blocks.3.conv2"):
        enable_split_convs(net)
    assert not any(hasattr(m, "_sz_orig_forward") for m in net.modules())
