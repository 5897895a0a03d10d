"""Multi-rank runs of the REAL HIP engine: two torch.distributed ranks, one engine
each over its slice of the base, candidates exchanged and merged by ShardedGGNN.  The test box has
one GPU, so both ranks use device 0 and the gloo backend (RCCL refuses two ranks on one device);
the exchange + device merge code is the one the RCCL run uses, only the collective differs.

Checked against a single handle over the same base with set_shard_size (the reference's
multi-shard mode) and against the oracle's ResultMerger:
  * bf_query: bit-identical to the single handle (exact search, deterministic),
  * query: the merged result equals orc.merge_results of the per-rank rows that were exchanged
    (id offset rank * shards_per_rank * N_shard, result_merger.cpp:115-116), recall >= 0.97.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import make_int_data

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("world,spg", [(2, 1), (2, 2)])
def test_two_ranks_real_engine(orc, tmp_path, world, spg):
    import ggnn_amd as ggnn
    shard, D, K = 3000, 64, 10
    out = str(tmp_path / "merged.npz")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29500 + (os.getpid() % 500) + 7 * spg
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(ROOT, "tests", "tools", "dist_engine_check.py"), out, str(shard), str(spg)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    N = shard * spg * world
    base, q = make_int_data(N, D, 871), make_int_data(200, D, 872)
    # single handle, same partition: the reference's multi-shard mode on one GPU
    eng = ggnn.GGNN()
    eng.set_base(base)
    gt, gt_d = eng.bf_query(q, K)
    assert np.array_equal(z["gt"], gt.numpy()) and np.array_equal(z["gt_d"], gt_d.numpy())
    # merged == ResultMerger over the rows the ranks exchanged
    parts_i = [z["parts_ids"][r_] for r_ in range(world)]
    parts_d = [z["parts_d"][r_] for r_ in range(world)]
    m_ids, m_d = orc.merge_results(parts_i, parts_d, K, spg, shard)
    assert np.array_equal(z["d"], m_d)
    uniq = np.ones_like(m_d, bool)                 # ids at tied distances may swap between parts
    uniq[:, 1:] &= m_d[:, 1:] != m_d[:, :-1]
    uniq[:, :-1] &= m_d[:, :-1] != m_d[:, 1:]
    assert np.array_equal(z["ids"][uniq], m_ids[uniq])
    rec = np.mean([len(set(a) & set(b)) / K for a, b in zip(z["ids"], z["gt"])])
    assert rec >= 0.97, rec
    assert z["ids"].max() >= shard * spg          # ids of the second rank's slice are offset


def _json_line(stdout):
    import json
    lines = [ln for ln in stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


def test_bench_two_ranks_strong_scaling_line(tmp_path):
    """bench.py --gpus 2 --full as the driver launches it (torch.distributed.run, one rank per GPU),
    here with both ranks on GPU 0 over gloo and a small base: the strong-scaling line must carry
    queries/s on the fixed 8-shard base, the one-GPU point of the same base and the speed-up."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    port = 29500 + (os.getpid() % 400) + 57
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", "2", "--steps", "3", "--warmup", "1", "--backend", "gloo", "--single-device",
           "--n-base", "20000", "--n-query", "600", "--tau-query", "1.0", "--max-iters", "400",
           "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 2 and d["steps"] == 3 and d["warmup"] == 1
    assert d["unit"] == "queries/s" and d["scaling"] == "strong" and d["higher_is_better"] is True
    assert abs(d["value"] - 600 / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    assert "8 shards x 20000" in d["config"]["workload"]
    assert "x 96 f32" in d["config"]["workload"]          # BASELINE configs[3]: the DEEP100M shape
    assert d["secondary_base"] is None or d["secondary_base"]["dim"] == 128
    assert d["recall_at_10"] > 0.95
    pip = d["pipelined_batches"]
    assert pip.get("results_equal_blocking") is True and pip["queries_per_s"] > 0, pip
    one = d["one_gpu_same_base"]
    assert one["recall_at_10"] > 0.95 and one["queries_per_s"] > 0
    assert abs(d["speedup_vs_one_gpu_same_base"] - d["value"] / one["queries_per_s"]) < 1e-9


def test_bench_single_gpu_line_small():
    """the --full N=1 line on a small base: contract fields, roofline and cpu_baseline objects, the
    dataset block and the one-GPU point of the strong-scaling series"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "3", "--warmup", "1",
           "--n-base", "20000", "--n-query", "600", "--tau-query", "1.0", "--max-iters", "400"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = _json_line(r.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline",
                "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["vs_baseline"] is None and d["dtype"] == "f32"
    assert d["recall_at_10"] > 0.95 and d["recall_at_10_heldout_queries"] > 0.95
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "valu") and 0 < rf["frac"] and "secondary" in rf
    assert rf["without_prescreen"]["results"].startswith("bit-identical")
    cb = d["cpu_baseline"]
    assert cb["kind"] in ("port", "reference") and cb["value"] > 0 and cb["cores"] >= 1
    res = d["recall_targets"]["results"]
    assert set(res) >= {"lowrank16", "lowrank24", "lowrank32", "lowrankf16"}
    for kind, r in res.items():
        assert r["same_settings_as_headline"]["queries_per_s"] > 0
        at = r["at_recall_0.99"]
        assert (at is None and "not_reached_best" in r) or at["recall_at_10"] >= 0.99, kind
    one = d["strong_scaling_one_gpu"]
    assert one["queries_per_s"] > 0 and "pipelined_batches" in one
    for kname in ("merge_kernel", "sym_kernel"):
        b = d["build"][kname]
        assert b["launches"] > 0 and b["kernel_ms_sum"] > 0 and b["float_rows"] > 0
        rl = b["roofline"]
        # the binding roof is NAMED (fabric bytes vs HBM, own bytes vs the L2s, VALU issue; hbm and
        # valu need committed counter passes of the workload) and no fraction exceeds 1
        assert rl["bound"] in ("hbm", "l2", "valu") and 0 < rl["frac"] <= 1.0
        assert rl["frac"] == max(rl["candidates"].values()) and rl["own_bytes_over_hbm_peak"] > 0
        assert b["roofline"]["bytes"] <= b["reference_algorithm"]["bytes"]
    for kind, r in res.items():
        assert 1.0 < r["local_intrinsic_dimension"]["mle_k20"] < 128.0, kind


def test_sharded_engine_over_rccl_one_rank_world():
    """The process-per-GPU path with the backend the driver uses (`nccl` = RCCL): a one-rank world
    on the one GPU of the test box -- `all_gather_into_tensor` of the packed CUDA candidates, the
    device merge, blocking and pipelined queries -- against a plain single handle."""
    code = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["GGNN_ROOT"])
import ggnn_amd as ggnn
from ggnn_amd.distributed import ShardedGGNN
from bench import synthetic
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", device_id=dev)
base = synthetic("lowrank16", 60000, 64, 1, dev)
q = synthetic("lowrank16", 500, 64, 2, dev)
s = ShardedGGNN()
s.set_base(base)
s.set_shard_size(20000)           # three resident shards on the one rank
s.build(24, 0.5, 1)
ids, d = s.query(q, 10, 0.9, 200)
gt, gd = s.bf_query(q, 10)
t = s.query_async(q, 10, 0.9, 200, slot=1)
ids2, d2 = s.finish(t)
assert ids.is_cuda and tuple(ids.shape) == (500, 10)
assert torch.equal(ids, ids2) and torch.equal(d, d2)
assert s.last_query_parts == 1
s.split_blocking = True           # two half-batches in flight (default from 4096 queries)
ids3, d3 = s.query(q, 10, 0.9, 200)
assert s.last_query_parts == 2 and torch.equal(ids, ids3) and torch.equal(d, d3)
ref = ggnn.GGNN(); ref.set_base_reference(base); ref.set_shard_size(20000)
ref.set_return_results_on_gpu(True); ref.build(24, 0.5, 1)
rg, rd = ref.bf_query(q, 10)
assert torch.equal(gd, rd[:, :10]) and torch.equal(gt, rg[:, :10])
rec = (ids.unsqueeze(2) == gt.unsqueeze(1)).any(2).float().mean().item()
assert rec > 0.95, rec
dist.destroy_process_group()
print("OK", rec)
'''
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(29500 + (os.getpid() % 300) + 101),
               RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", GGNN_ROOT=ROOT,
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0 and "OK" in r.stdout, r.stdout[-1000:] + r.stderr[-3000:]
