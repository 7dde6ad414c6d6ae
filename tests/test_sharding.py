"""Multi-GPU layout of the path on CPU: image sharding is a static partition, and the one
start-up collective (flat weight broadcast) leaves every rank with rank 0's weights.
World size 2 over gloo (the GPU run uses the same code over RCCL)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from centernet_amd import sharding, synth
from centernet_amd.model import create_model


def test_shard_range_is_a_partition():
    for n in (0, 1, 7, 32, 255, 256):
        for world in (1, 2, 3, 8):
            spans = [sharding.shard_range(n, r, world) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
                assert a1 == b0 and a0 <= a1
            sizes = [b - a for a, b in spans]
            assert max(sizes) - min(sizes) <= 1
            assert sizes == [len(c) for c in np.array_split(np.arange(n), world)]


def test_flatten_roundtrip():
    m = create_model("resdcn_18", {"hm": 80, "wh": 2, "reg": 2}, 64)
    synth.fill_state_dict_(m, 1)
    flat, layout = sharding.flatten_state(m)
    assert flat.numel() == sum(int(np.prod(s)) for _, s in layout)
    m2 = create_model("resdcn_18", {"hm": 80, "wh": 2, "reg": 2}, 64)
    sharding.unflatten_state_(m2, flat, layout)
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        if a.is_floating_point():
            assert torch.equal(a, b), k


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = create_model("res_18", {"hm": 80, "wh": 2, "reg": 2}, 64)
    synth.fill_state_dict_(m, 100 + rank)          # ranks start with DIFFERENT weights
    nbytes = sharding.broadcast_weights(m, src=0)
    flat, _ = sharding.flatten_state(m)
    lo, hi = sharding.shard_range(5, rank, world)   # 5 images over 2 ranks: 3 + 2
    dets = torch.full((hi - lo, 4, 6), float(rank))
    # uneven shards: pad to the max shard for the all_gather, as a caller would
    pad = torch.zeros((3 - (hi - lo), 4, 6))
    allg = sharding.gather_detections(torch.cat([dets, pad], 0))
    q.put((rank, nbytes, float(flat.double().sum()), (lo, hi), tuple(allg.shape),
           float(allg[3:, 0, 0].max())))
    dist.barrier()
    dist.destroy_process_group()


def test_weight_broadcast_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    ref = create_model("res_18", {"hm": 80, "wh": 2, "reg": 2}, 64)
    synth.fill_state_dict_(ref, 100)
    want = float(sharding.flatten_state(ref)[0].double().sum())
    assert res[0][2] == pytest.approx(want, rel=0, abs=0)
    assert res[1][2] == res[0][2], "rank 1 must hold rank 0's weights after the broadcast"
    assert res[0][1] == res[1][1] > 50e6            # ~63 MB for res_18
    assert res[0][3] == (0, 3) and res[1][3] == (3, 5)
    assert res[0][4] == (6, 4, 6) and res[0][5] == 1.0


def test_launch_ranks_spawns_world(tmp_path):
    """bench.py --gpus N without a launcher starts N ranks itself through
    sharding.launch_ranks: here a 2-rank gloo job whose rank 0 reports the world it saw."""
    import subprocess
    import sys
    import textwrap
    script = tmp_path / "probe.py"
    out = tmp_path / "seen.txt"
    script.write_text(textwrap.dedent("""
        import os, sys
        import torch, torch.distributed as dist
        dist.init_process_group("gloo")
        t = torch.tensor([float(dist.get_rank() + 1)])
        dist.all_reduce(t)
        if dist.get_rank() == 0:
            open(sys.argv[1], "w").write("%d %d %s" % (dist.get_world_size(), int(t.item()), sys.argv[2]))
        dist.destroy_process_group()
    """))
    cmd = sharding.launch_command(str(script), [str(out), "--flag"], 2)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "127.0.0.1" in cmd
    assert cmd[cmd.index("--nproc-per-node") + 1] == "2"
    rc = sharding.launch_ranks(str(script), [str(out), "--flag"], 2)
    assert rc == 0
    assert out.read_text() == "2 3 --flag"


def test_bench_refuses_world_mismatch():
    """bench.py under a launcher whose world size differs from --gpus must fail loudly (the
    round-1 defect: --gpus was parsed and ignored)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "bench.py")).read()
    assert "launch_ranks" in src and "world != a.gpus" in src
    sys.path.insert(0, root)
    import bench
    a = bench.parse(["--gpus", "8", "--config", "3"])
    assert (a.gpus, a.task, a.arch, a.batch, a.fp16) == (8, "multi_pose", "dla_34", 32, False)
    a = bench.parse(["--config", "4"])
    assert (a.arch, a.batch, a.fp16) == ("hourglass", 8, True)
    a = bench.parse([])
    assert (a.gpus, a.task, a.arch, a.batch, a.fp16, a.res) == (1, "ctdet", "resdcn_18", 32, False, 512)


def _run_bench_stub(args, env_extra=None):
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BENCH_STUB="1", OMP_NUM_THREADS="2")
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + args, env=env,
                       capture_output=True, text=True, timeout=600)
    return p, [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]


def test_bench_rank_logic_end_to_end_two_ranks_gloo():
    """`python bench.py --gpus 2` end to end on CPU: the file's own control flow -- self-spawned
    ranks (torchrun, 127.0.0.1), process group, ONE flat weight broadcast, warm-up, barrier,
    K timed steps, barrier, max-over-ranks clock, exactly one JSON line from rank 0 -- with the
    detector replaced by bench._StubDetector (BENCH_STUB=1; gloo instead of RCCL).  What an 8-GPU
    lease runs differs only in the backend string and the detector."""
    p, lines = _run_bench_stub(["--gpus", "2", "--steps", "6", "--warmup", "2", "--batch", "4",
                                "--res", "64", "--full"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1, "exactly one JSON line, from rank 0"
    r = lines[0]
    assert r["n_gpus"] == 2 and r["world_size_seen"] == 2 and r["backend"] == "gloo"
    assert r["steps"] == 6 and r["warmup"] == 2 and r["scaling"] == "weak" and r["data"] == "stub"
    assert r["config"]["global_batch"] == 8 and r["config"]["parallelism"] == "image-sharded x2"
    assert r["weight_broadcast_bytes"] == 4 * (64 * 64 + 64) and r["weight_broadcast_ms"] > 0
    # one shared batch through every replica behind the broadcast: same results on every rank
    assert r["cross_rank_agreement"]["ok"] and r["cross_rank_agreement"]["ranks"] == 2
    assert r["cross_rank_agreement"]["max_score_diff"] <= 1e-4
    # every rank's own rate is in the line (a straggler GPU is visible); the headline is the slowest's clock
    assert len(r["per_rank_img_s"]) == 2 and all(v > 0 for v in r["per_rank_img_s"])
    assert r["value"] <= sum(r["per_rank_img_s"]) * (1 + 1e-6)
    # whole-job rate = images of ALL ranks / the slowest rank's time
    assert abs(r["value"] - 8 * 6 / (r["ms_per_step"] * 6e-3)) <= 1e-6 * r["value"]
    assert r["metric"].startswith("images/sec whole-node") and r["higher_is_better"] is True
    # every rank says which device it sits on; the line carries one distinct identity per rank
    assert [d["rank"] for d in r["rank_devices"]] == [0, 1]
    assert len({d["uuid"] for d in r["rank_devices"]}) == 2
    assert r["rccl_ranks_seen"] is None      # gloo here; an RCCL run reports the world it really formed


def test_bench_plain_run_is_headline_only_and_dumps_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps, prints the headline fields and none of the
    --full figures, and --dump-outputs writes the last timed step's result as float32 .npy."""
    import numpy as np
    out = tmp_path / "dump"
    p, lines = _run_bench_stub(["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--res", "64",
                                "--dump-outputs", str(out)])
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1
    r = lines[0]
    assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["higher_is_better"] is True
    assert r["metric"].startswith("images/sec whole-node") and r["unit"] == "img/s" and r["dtype"] == "f32s"
    assert abs(r["value"] - 2 * 3 / (r["ms_per_step"] * 3e-3)) <= 1e-6 * r["value"]
    for k in ("roofline", "time_share", "box_calibration", "cross_rank_agreement", "cpu_baseline"):
        assert k not in r, k
    d = np.load(out / "detections.npy")
    assert d.dtype == np.float32 and d.shape == (64, 64)
    p, _ = _run_bench_stub(["--gpus", "1", "--steps", "1", "--per-op"])
    assert p.returncode != 0 and "--per-op needs --full" in p.stderr


def test_bench_refuses_two_ranks_on_one_device():
    """Two ranks that report the SAME device identity (a wrong LOCAL_RANK -> device mapping on a real node):
    no JSON line, non-zero exit, a message that names the cause -- a scaling number can never come from
    ranks that shared a GPU."""
    p, lines = _run_bench_stub(["--gpus", "2", "--steps", "2", "--warmup", "1", "--batch", "2", "--res", "64"],
                               {"BENCH_FAKE_UUID": "GPU-same"})
    assert p.returncode != 0
    assert not lines
    assert "two ranks share a GPU" in (p.stderr + p.stdout)


def test_bench_config2_over_eight_ranks_is_global_batch_256():
    """BASELINE configs[2]: dla_34, batch 256 sharded over 8 GPUs = 32 per rank -- the line of an
    8-rank run says so (stub detector, 8 CPU ranks over gloo)."""
    p, lines = _run_bench_stub(["--gpus", "8", "--config", "2", "--steps", "2", "--warmup", "1",
                                "--res", "64"], {"OMP_NUM_THREADS": "1"})
    assert p.returncode == 0, p.stderr[-2000:]
    assert len(lines) == 1
    r = lines[0]
    assert r["n_gpus"] == 8 and r["world_size_seen"] == 8
    assert r["config"]["global_batch"] == 256 and "dla_34" in r["config"]["workload"]
    assert "batch 32 per GPU" in r["config"]["workload"]


def test_bench_under_a_launcher_with_the_wrong_world_fails(tmp_path):
    """torchrun --nproc-per-node 2 bench.py --gpus 4: refused (an N > 1 line can never come from a
    different world than it claims)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = sharding.launch_command(os.path.join(root, "bench.py"),
                                  ["--gpus", "4", "--steps", "1", "--warmup", "1", "--batch", "2", "--res", "64"], 2)
    p = subprocess.run(cmd, env=dict(os.environ, BENCH_STUB="1", OMP_NUM_THREADS="1"),
                       capture_output=True, text=True, timeout=600)
    assert p.returncode != 0
    assert "--gpus 4 but the process group has 2" in (p.stderr + p.stdout)


def test_cross_rank_agreement_rule():
    """bench.cross_rank_agreement: replicas agree when scores are within 1e-4 and rows sit in
    place; a class change, a moved box or a larger score difference is a disagreement."""
    import sys
    import torch
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import bench
    g = torch.Generator().manual_seed(0)
    d = torch.rand((2, 10, 6), generator=g)
    d[..., 5] = torch.randint(0, 80, (2, 10), generator=g).float()
    ok = bench.cross_rank_agreement([d, d + 0, d + torch.tensor([0, 0, 0, 0, 5e-5, 0])])
    assert ok["ok"] and ok["ranks"] == 3 and abs(ok["max_score_diff"] - 5e-5) < 1e-6
    bad = d.clone(); bad[0, 0, 4] += 1e-3
    assert not bench.cross_rank_agreement([d, bad])["ok"]
    bad = d.clone(); bad[:, :, 5] += 1
    assert not bench.cross_rank_agreement([d, bad])["ok"]
    y = torch.rand((64, 64), generator=g)
    assert bench.cross_rank_agreement([y, y.clone()])["ok"]
    assert not bench.cross_rank_agreement([y, y + 1e-3])["ok"]
