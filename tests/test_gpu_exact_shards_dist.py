"""dist.ExactShardedTracer and `cli --deterministic --ranks N` on the GPU box's one device: the ranks share it over gloo (the rehearsal of the
N > 1 path; RCCL sums int64 the same way) and rank 0 must end up with the image bytes and landed weight of ONE process with ONE handle."""
import hashlib
import json
import os
import re
import socket
import subprocess
import sys

import pytest

from ice_halo_sim_amd import scenes
from tests.test_gpu_exact_shards import RAY_BASE, SEED, _fisheye, _one, _prism

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = os.path.join(ROOT, "tests", "golden", "exact_shards_config.json")
N = (1 << 17) + 5
WLS = ((530.0, 1.0), (610.0, 0.8), (450.0, 2.0))   # weights that give the landed integer the scales 27, 28 and 26
STEPS = 2


def _scene():
    return _one(_prism(0.7), scenes.stochastic_prism_entry(), hits=8)   # (the sampled entry's proportion is 100: most rays, cut at shapes)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    from ice_halo_sim_amd.dist import ExactShardedTracer
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    tr = ExactShardedTracer(_scene(), _fisheye(), seed=SEED, device=0, rank=rank, world=world, ray_base=RAY_BASE)
    roots = 0
    for _ in range(STEPS):
        for l, w in WLS:
            roots += int(tr.trace_session(scenes.wl_discrete(l, w), N).root_count)
    img, landed = tr.readback()
    assert (img is None) == (rank != 0)
    rec = {"roots": roots, "exchanges": tr.exchanges, "landed": landed, "sha": hashlib.sha256(img.tobytes()).hexdigest() if rank == 0 else None}
    with open(os.path.join(out_dir, "rank%d.json" % rank), "w") as f:
        json.dump(rec, f)
    tr.backend.close()
    dist.barrier()
    dist.destroy_process_group()


_ONE = {}


def _one_handle():
    """The same sequence on one process's one handle: traced once, shared by the cases."""
    if not _ONE:
        from ice_halo_sim_amd.backend import HipTraceBackend
        from tests._oracle_backend import run_session
        hb = HipTraceBackend(device=0, seed=SEED)
        hb.set_option("deterministic", 1)
        hb.set_option("ray_base", RAY_BASE)
        for _ in range(STEPS):
            for l, w in WLS:
                run_session(hb, _scene(), _fisheye(), scenes.wl_discrete(l, w), N)
        img, landed = hb.ReadbackXyzAccum()
        hb.close()
        assert landed > 0
        _ONE.update(sha=hashlib.sha256(img.tobytes()).hexdigest(), landed=landed)
    return _ONE


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_over_gloo_give_one_ranks_bytes(world, tmp_path):
    import torch.multiprocessing as mp
    want = _one_handle()
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    recs = [json.load(open(tmp_path / ("rank%d.json" % r))) for r in range(world)]
    assert recs[0]["sha"] == want["sha"]
    assert recs[0]["landed"] == want["landed"]
    assert sum(r["roots"] for r in recs) == STEPS * len(WLS) * N and all(r["roots"] > 0 for r in recs)
    assert all(r["exchanges"] == STEPS * len(WLS) for r in recs)          # before every change of wavelength, and at the readback
    assert all(r["landed"] == 0.0 and r["sha"] is None for r in recs[1:])


def _cli(extra, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    e.update(env)
    return subprocess.run([sys.executable, "-m", "ice_halo_sim_amd.cli", "-f", CONFIG, "--render", "1", "--deterministic", "--seed", "7"] + extra,
                          capture_output=True, text=True, cwd=ROOT, env=e, timeout=600)


def test_cli_ranks_print_the_one_rank_sha256():
    one = _cli([])
    assert one.returncode == 0, one.stdout + one.stderr
    three = _cli(["--ranks", "3"], HALO_DIST_BACKEND="gloo")               # (one after the other: this process and three ranks hold the GPU at most)
    assert three.returncode == 0, three.stdout + three.stderr
    sha = lambda out: re.findall(r"^xyz sha256: ([0-9a-f]{64})$", out, re.M)
    assert len(sha(one.stdout)) == 1 and sha(three.stdout) == sha(one.stdout), (one.stdout, three.stdout)
    landed = lambda out: re.findall(r"landed intensity (\S+)", out)
    assert landed(three.stdout) == landed(one.stdout) and len(landed(one.stdout)) == 1


def test_cli_ranks_need_deterministic_and_refuse_what_sharding_refuses(tmp_path):
    r = subprocess.run([sys.executable, "-m", "ice_halo_sim_amd.cli", "-f", CONFIG, "--render", "1", "--ranks", "2"], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and "--deterministic" in r.stderr
    doc = json.load(open(CONFIG))
    doc["scene"]["scattering"] = [{"prob": 0.5, "entries": [{"crystal": 3}]}, {"prob": 0.0, "entries": [{"crystal": 3}]}]
    doc["scene"]["ray_num"] = 20000
    cfg = tmp_path / "two_layers.json"
    cfg.write_text(json.dumps(doc))
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    r = subprocess.run([sys.executable, "-m", "ice_halo_sim_amd.cli", "-f", str(cfg), "--render", "1", "--deterministic", "--ranks", "2"],
                       capture_output=True, text=True, cwd=ROOT, env=dict(e, HALO_DIST_BACKEND="gloo"), timeout=600)
    assert r.returncode != 0
    assert "refused:" in r.stderr and "a multi-layer scene is not supported" in r.stderr, r.stderr[-2000:]
