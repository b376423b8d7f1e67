"""N>1 path on CPU: two gloo ranks shard a batch, run the (oracle) forward on their shard and all-gather.
Correctness contract: the gathered output equals the unsharded forward, row for row."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from swin_unet_image_fusion_amd.shard import ShardedFusion, shard_bounds

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_shard_bounds_cover_batch_exactly():
    for batch in (0, 1, 5, 16, 17, 128):
        for world in (1, 2, 3, 8):
            got = []
            for r in range(world):
                a, b, per = shard_bounds(batch, world, r)
                assert 0 <= a <= b <= batch and b - a <= per
                got += list(range(a, b))
            assert got == list(range(batch))
    with pytest.raises(ValueError):
        shard_bounds(4, 2, 2)


def _worker(rank, world, port, batch, q):
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import swin_fusion_oracle as O
        from swin_unet_image_fusion_amd.config import CONFIGS, synthetic_pair
        from tests import golden_util as G
        torch.set_num_threads(2)
        cfg = CONFIGS["tiny"]
        sd = G.recipe_state(dict(weight_seed=0, flavor="stress", keys_file="state_keys_tiny.json"))
        ir, vis = (torch.from_numpy(a) for a in synthetic_pair(batch, 16, 16))
        fwd = lambda a, b: O.model_forward(sd, cfg, a, b)
        runner = ShardedFusion(world_size=world, rank=rank, forward_fn=fwd)
        with torch.no_grad():
            full = runner.fuse_global(ir, vis)
            ref = fwd(ir, vis)
        ok = full.shape == ref.shape and torch.allclose(full, ref, rtol=0, atol=1e-6)
        # weak-scaling step API: equal shards, rank-major order
        a, b, per = shard_bounds(batch - batch % world, world, rank)
        with torch.no_grad():
            g = runner.step(ir[a:b], vis[a:b])
        ok = ok and torch.allclose(g, ref[: g.shape[0]], rtol=0, atol=1e-6)
        # pipelined steps (bench.py's loop): the gather of step i is waited for after step i+1 has been issued; results
        # stay valid for two steps (double-buffered) and each equals its own step's unsharded rows
        if b > a:
            with torch.no_grad():
                flipped = fwd(vis, ir)
                h0 = runner.step_async(ir[a:b], vis[a:b])
                h1 = runner.step_async(vis[a:b], ir[a:b])
                g0, g1 = h0.wait(), h1.wait()
            ok = ok and g0.data_ptr() != g1.data_ptr()
            ok = ok and torch.allclose(g0, ref[: g0.shape[0]], rtol=0, atol=1e-6) and torch.allclose(g1, flipped[: g1.shape[0]], rtol=0, atol=1e-6)
        q.put((rank, bool(ok)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("batch", [4, 5])
def test_two_rank_gloo_matches_unsharded(batch):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29600 + batch + (os.getpid() % 200)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, batch, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(180)
        assert p.exitcode == 0
    res = dict(q.get(timeout=5) for _ in range(2))
    assert res == {0: True, 1: True}


def test_runner_runs_every_forward_without_grad():
    """ShardedFusion is an inference runner: step, step_async, local_forward and fuse_global call forward_fn under no_grad even when the
    caller has grad enabled, so a model whose parameters require grad takes its fused forward there."""
    seen = []

    def fwd(a, b):
        seen.append(torch.is_grad_enabled())
        return a * b

    runner = ShardedFusion(world_size=1, rank=0, forward_fn=fwd)
    a, b = torch.rand(2, 1, 4, 4, requires_grad=True), torch.rand(2, 1, 4, 4)
    assert torch.is_grad_enabled()
    outs = [runner.step(a, b), runner.step_async(a, b).wait(), runner.local_forward(a, b), runner.fuse_global(a, b)]
    assert seen == [False] * 4
    assert torch.is_grad_enabled()
    for o in outs:
        assert o.grad_fn is None and not o.requires_grad
        assert torch.equal(o, (a * b).detach())
