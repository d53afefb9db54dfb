"""bench.py's launcher contract, the part that needs no GPU: a --gpus / WORLD_SIZE mismatch is refused before anything touches a device."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)


def test_gpus_flag_must_match_the_launchers_world_size():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "1"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], {"RANK": "0", "LOCAL_RANK": "0", "WORLD_SIZE": "4"})
    assert r.returncode != 0 and "WORLD_SIZE=4" in r.stderr
    r = _run(["--gpus", "0"], {})
    assert r.returncode != 0


def test_without_a_gpu_the_bench_fails_loudly():
    import torch
    if torch.cuda.is_available():
        return
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], {})
    assert r.returncode != 0 and "no CPU fallback" in r.stderr


def test_dump_outputs_needs_a_timed_step():
    r = _run(["--gpus", "1", "--steps", "0", "--warmup", "0", "--dump-outputs", "unused"], {})
    assert r.returncode != 0 and "--dump-outputs needs --steps >= 1" in r.stderr


def test_dump_outputs_writes_float32_within_the_budget(tmp_path):
    """bench.dump_outputs on a synthetic ply record: every array lands as float32 .npy, all boards while they fit, a seeded board
    subset (the same one every time) once they do not, and never more than the byte budget"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench

    def last(B):
        g = np.random.RandomState(B)
        rec = dict(packed=g.randint(0, 256, (B, 119, 8)).astype(np.uint8), action=g.randint(0, 4672, (B, 218)).astype(np.int32),
                   visits=g.randint(0, 800, (B, 218)).astype(np.int32), n_child=np.full(B, 20, np.int32), colour=np.ones(B, np.uint8),
                   chosen=np.zeros(B, np.int32), game_over=np.zeros(B, np.uint8), result=np.zeros(B, np.int8), active=np.ones(B, np.uint8))
        return rec, dict(rec=rec, policy=torch.from_numpy(g.rand(B, 4672).astype(np.float32)), value=torch.from_numpy(g.rand(B).astype(np.float32)))

    def load(d):
        return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}

    rec, small = last(40)
    bench.dump_outputs(str(tmp_path / "small"), small)
    z = load(str(tmp_path / "small"))
    assert all(v.dtype == np.float32 for v in z.values())
    assert np.array_equal(z["visits"], rec["visits"]) and np.array_equal(z["packed"], rec["packed"]) and np.array_equal(z["board_index"], np.arange(40))
    assert np.array_equal(z["policy"], small["policy"].numpy()) and np.array_equal(z["value"], small["value"].numpy())

    limit = 8 << 20
    rec, big = last(1000)
    for d in ("big1", "big2"):
        bench.dump_outputs(str(tmp_path / d), big, limit=limit)
    z, z2 = load(str(tmp_path / "big1")), load(str(tmp_path / "big2"))
    assert sum(os.path.getsize(str(tmp_path / "big1" / f)) for f in os.listdir(str(tmp_path / "big1"))) <= limit
    idx = z["board_index"].astype(np.int64)
    assert 256 < len(idx) < 1000 and len(z["policy"]) == 256 and np.array_equal(z["visits"], rec["visits"][idx])
    pol = z["policy_board_index"].astype(np.int64)
    assert set(pol.tolist()) <= set(idx.tolist()) and np.array_equal(z["policy"], big["policy"].numpy()[pol])
    assert all(np.array_equal(z[k], z2[k]) for k in z)


def test_side_measurements_wait_for_full():
    """a plain run measures the headline only; the side measurements that take runs of their own are asked for with --full"""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1"]).full is False
    assert bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full"]).full is True
