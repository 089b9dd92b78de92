"""bench.py's host-side choices (no GPU)."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_auto_partition_keeps_model_sharding_and_takes_the_grid_the_table_projects():
    b = _bench()
    # BASELINE.json north_star: "partition across the 8 GPUs of one node by sharding the model database" -- the DB stays
    # sharded (G >= 2) for every N > 1; a DB too small for N shards gets frame groups beside them
    assert b.choose_partition(20, 1) == (1, 1)
    assert b.choose_partition(20, 2) == (2, 1)
    assert b.choose_partition(20, 4) == (2, 2)
    assert b.choose_partition(20, 8) == (2, 4)
    assert b.choose_partition(200, 8) == (8, 1) and b.choose_partition(200, 4) == (4, 1) and b.choose_partition(200, 2) == (2, 1)
    for n_models, world in ((20, 8), (200, 8), (50, 4), (20, 2), (3, 8)):
        G, R = b.choose_partition(n_models, world)
        assert G >= 2 and G * R == world
    # the projections the choice rests on (profiles/per_rank_load.json): north_star's >= 6x at 8 GPUs for both DBs
    assert b.projected_speedup(20, 2, 4) >= 6.0 and b.projected_speedup(200, 8, 1) >= 6.0
    assert b.projected_speedup(20, 8, 1) < 3.5          # why pure sharding of the small DB is not what auto runs
    # the explicit forms
    assert b.choose_partition(20, 8, "models") == (8, 1) and b.choose_partition(20, 8, "frames") == (1, 8)
    assert b.choose_partition(20, 8, "grid", "4x2") == (4, 2)
    import pytest
    with pytest.raises(SystemExit):
        b.choose_partition(20, 8, "grid", "3x2")


def test_per_rank_table_interpolates():
    b = _bench()
    t = {"10": 20000.0, "20": 10000.0}
    assert abs(b.per_rank_us(10, t) - 50.0) < 1e-9 and abs(b.per_rank_us(20, t) - 100.0) < 1e-9
    assert abs(b.per_rank_us(15, t) - 75.0) < 1e-9
    assert abs(b.per_rank_us(5, t) - 50.0) < 1e-9       # below the table: the smallest shard's cost (it does not shrink further)
    assert abs(b.per_rank_us(40, t) - 200.0) < 1e-9     # beyond: the last slope


def test_scaling_and_partition_labels():
    b = _bench()
    assert b.scaling_label(1, 1) == "n/a"                                       # nothing scales at N = 1
    assert b.scaling_label(8, 1) == "strong" and b.scaling_label(1, 8) == "weak" and b.scaling_label(2, 4) == "weak"
    assert b.partition_label(1, 1) == "single GPU" and b.partition_label(8, 1) == "model-shard x8"
    assert b.partition_label(1, 4).startswith("frame-parallel x4") and b.partition_label(2, 4) == "grid: 2 model shards x 4 frame groups"


def test_gpus_n_without_a_launcher_never_prints_a_line_for_ranks_that_did_not_run():
    """`python bench.py --gpus 2` on a host with fewer than 2 devices (this container has none): non-zero exit, no JSON
    line -- never `"n_gpus": 2` from one process."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MH_BENCH_REHEARSE")}
    import torch
    if torch.cuda.device_count() >= 2:
        return   # (a multi-GPU host really runs it: covered by tests/test_gpu_bench_rehearsal.py)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert "--gpus 2" in r.stderr


def test_default_batch_follows_the_partition():
    b = _bench()
    from moped_amd import capi
    a = b.parse(["--gpus", "8"])
    assert b.default_batch(a, True) == capi.MAX_BATCH      # 2.5 models per rank: as many frames per launch as the library takes
    assert b.default_batch(a, True, 2) == capi.MAX_BATCH   # a 2 x 4 grid: 10 models per rank
    a200 = b.parse(["--gpus", "8", "--models", "200"])
    assert b.default_batch(a200, True, 2) == 16            # 100 models per rank
    a = b.parse(["--gpus", "8", "--models", "200"])
    assert b.default_batch(a, True) == 16                  # configs[3]: 25 models per rank, MATCH fills the chip
    a = b.parse([])
    assert b.default_batch(a, False) == 16
    a = b.parse(["--depth-kind", "1"])
    assert b.default_batch(a, False) == 16                 # depth attributes travel with a merged batch (round 4)
    a = b.parse(["--depth-kind", "1", "--moped3d-frontend"])
    assert b.default_batch(a, False) == 16                 # a depth map per frame travels with a merged batch too (round 4)


def test_a_plain_run_times_the_headline_alone_and_full_keeps_every_leg():
    b = _bench()
    a = b.parse(["--steps", "7", "--warmup", "2"])
    assert not a.full and a.steps == 7 and a.warmup == 2
    assert a.no_secondary and a.no_cpu_baseline and a.no_roofline and a.h2d_steps == 0
    a = b.parse(["--full"])
    assert not (a.no_secondary or a.no_cpu_baseline or a.no_roofline) and a.h2d_steps == 3
    a = b.parse(["--full", "--no-roofline", "--h2d-steps", "0"])     # each leg can still be left out on its own
    assert a.no_roofline and a.h2d_steps == 0 and not a.no_secondary and not a.no_cpu_baseline


def _records(n):
    from moped_amd import capi
    r = np.zeros(n, capi.frame_block_dtype(32))
    rng = np.random.default_rng(5)
    r["head"]["n_objects"] = np.arange(n) % 4
    r["head"]["n_objects"][0] = 40                                # more than a record carries: all 32 slots are valid
    r["head"]["counts"] = rng.integers(0, 3000, (n, 4))
    r["objects"]["model"] = rng.integers(0, 20, (n, 32))            # stale values beyond n_objects too
    r["objects"]["pose"] = rng.standard_normal((n, 32, 7))
    r["objects"]["score"] = rng.random((n, 32))
    r["objects"]["n_points"] = rng.integers(7, 300, (n, 32))
    return r


def test_dump_outputs_writes_every_frame_in_order_and_masks_the_slots_past_n_objects(tmp_path):
    b = _bench()
    r = _records(48)
    b.dump_outputs(str(tmp_path / "out"), r)
    got = {f[:-4]: np.load(str(tmp_path / "out" / f)) for f in os.listdir(str(tmp_path / "out"))}
    assert set(got) == {"frame_index", "n_objects", "counts", "object_model", "object_pose", "object_score", "object_n_points"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["frame_index"], np.arange(48)) and np.array_equal(got["n_objects"], r["head"]["n_objects"])
    assert np.array_equal(got["counts"], r["head"]["counts"])
    n = np.minimum(r["head"]["n_objects"], 32)
    for f in range(48):
        k = n[f]
        assert np.array_equal(got["object_model"][f, :k], r["objects"]["model"][f, :k]) and (got["object_model"][f, k:] == -1).all()
        assert np.array_equal(got["object_pose"][f, :k], r["objects"]["pose"][f, :k]) and (got["object_pose"][f, k:] == 0).all()
        assert np.array_equal(got["object_score"][f, :k], r["objects"]["score"][f, :k]) and (got["object_score"][f, k:] == 0).all()
        assert np.array_equal(got["object_n_points"][f, :k], r["objects"]["n_points"][f, :k])


def test_dump_outputs_of_a_large_step_is_a_fixed_sample_within_64_mb(tmp_path):
    b = _bench()
    r = _records(b.DUMP_MAX_FRAMES + 1000)
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), r)
    size = sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a")))
    assert size <= 64 * 2 ** 20
    ia, ib = np.load(str(tmp_path / "a" / "frame_index.npy")), np.load(str(tmp_path / "b" / "frame_index.npy"))
    assert len(ia) == b.DUMP_MAX_FRAMES and np.array_equal(ia, ib) and (np.diff(ia) > 0).all()
    assert np.array_equal(np.load(str(tmp_path / "a" / "n_objects.npy")), r["head"]["n_objects"][ia.astype(np.int64)])


def test_dump_outputs_is_refused_where_it_would_not_be_the_single_gpu_path():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MH_BENCH_REHEARSE")}
    for extra in (["--gpus", "2"], ["--force-exchange"], ["--steps", "0"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--dump-outputs", "unused"] + extra,
                           capture_output=True, text=True, env=env, timeout=300, cwd=ROOT)
        assert r.returncode != 0 and "--dump-outputs" in r.stderr and not os.path.exists(os.path.join(ROOT, "unused"))
