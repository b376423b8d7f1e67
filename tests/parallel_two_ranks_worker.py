"""Worker of tests/test_gpu_parallel_two_ranks.py: one of two ranks that SHARE the box's one GPU, gloo as the process group (RCCL cannot
put two ranks on one device; this rehearses the control flow, not RCCL).  Each rank trains the `tiny` model on two pairs of its own;
together they must do what one rank does on all four: the same state after broadcast_state, one reduced gradient that equals float64
autograd of the oracle on the whole batch, head statistics over the whole batch, and bit-identical replicas after two full steps."""
import datetime
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
from torch import nn

# Rank r's images are scaled by 1 - SCALE r, so that the two halves of the head's batch have different means.  The blocks' LayerNorms
# take most of a scale away again: on the CPU oracle the halves' means differ by 0.008 at SCALE 0.5 (0.005-0.006 from 0.75 to 0.99),
# below the 1e-2 asked for below, and by 0.057 at -3 (rank 1's images are four times rank 0's).
SCALE = -3.0


def shard(rank, step=0):
    from swin_unet_image_fusion_amd import synthetic_pair
    ir, vis = (torch.from_numpy(a) for a in synthetic_pair(2, 16, 16, seed_ir=100 + rank + 10 * step, seed_vis=200 + rank + 10 * step))
    return ir * (1.0 - SCALE * rank), vis * (1.0 - SCALE * rank)


def gathered(t, world):
    """Every rank's copy of `t`, on the CPU."""
    mine = t.detach().cpu().contiguous()
    out = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(out, mine)
    return out


def main():
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    from oracle import swin_fusion_oracle as O
    from swin_unet_image_fusion_amd import CONFIGS, DataParallelStep, FusedAdam, MyLoss, MyModel, TorchCollective, load_recipe_into
    from tests.gpu_guard import record_dir
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))   # a peer that failed ends this rank soon
    cfg = CONFIGS["tiny"]
    new_model = lambda: MyModel(**cfg.model_kwargs(nn.ELU(inplace=True)))
    m = new_model()
    load_recipe_into(m, seed=10 + rank, flavor="stress")          # differently seeded replicas
    if rank == 1:
        m.final_layer[1].num_batches_tracked += 7
    m.to(dev).train()
    opt = FusedAdam(m.parameters(), lr=1e-3, max_grad_norm=1.0)
    coll = TorchCollective()
    dp = DataParallelStep(m, MyLoss(), opt, group=coll)

    # 1. broadcast_state: both replicas hold rank 0's state
    ref = new_model()
    load_recipe_into(ref, seed=10, flavor="stress")
    sd0 = {k: v.detach().clone() for k, v in ref.state_dict().items()}
    key_before = m.graph_key() if hasattr(m, "graph_key") else None
    dp.broadcast_state(src=0)
    got = m.state_dict()
    assert got.keys() == sd0.keys()
    for k, v in sd0.items():
        assert got[k].dtype == v.dtype and torch.equal(got[k].cpu(), v), f"rank {rank}: {k} differs from rank 0's after broadcast_state"
    if rank == 1 and key_before is not None:
        assert m.graph_key() != key_before, "graph_key() did not follow the broadcast"

    # the oracle on the whole batch of four, in float64
    shards = [shard(r) for r in range(world)]
    ir_all, vis_all = torch.cat([s[0] for s in shards]), torch.cat([s[1] for s in shards])
    as64 = lambda grad: {k: (v.double().requires_grad_(grad and "running" not in k) if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    means = []
    for ir, vis in shards:                                       # the halves' head-batch means, from the oracle's running-mean update
        sd = as64(False)
        rm0 = sd["final_layer.1.running_mean"].clone()
        with torch.no_grad():
            O.model_forward(sd, cfg, ir.double(), vis.double(), training=True)
        means.append((sd["final_layer.1.running_mean"] - 0.9 * rm0) / 0.1)
    assert float((means[0] - means[1]).abs().max()) > 1e-2, f"the halves' head-batch means are too close: {means}"
    sd = as64(True)
    out_ref = O.model_forward(sd, cfg, ir_all.double(), vis_all.double(), training=True)
    tgt_all = torch.maximum(ir_all, vis_all)
    (out_ref - tgt_all.double()).square().mean().backward()

    # 2. one forward / backward under head_sync, one reduced gradient
    ir, vis = (t.to(dev) for t in shards[rank])
    tgt = torch.maximum(ir, vis)
    with dp.head_sync():
        out = m(ir, vis)
        (out - tgt).square().mean().backward()
    dp.reduce_gradients()
    flats = gathered(dp._grads.flat, world)
    assert torch.equal(flats[0], flats[1]), "the reduced flat gradient differs between the ranks"
    mine = out_ref.detach()[2 * rank:2 * rank + 2]
    fwd = float((out.detach().cpu().double() - mine).abs().max() / out_ref.detach().abs().max())
    assert fwd <= 2e-3, f"rank {rank}: forward rel-max {fwd}"
    gmax = max(float(v.grad.abs().max()) for v in sd.values() if v.requires_grad and v.grad is not None)
    worst, worst_key = 0.0, None
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        g, r = p.grad.detach().cpu().double(), sd[k].grad
        err = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-3 * gmax)
        if err > worst:
            worst, worst_key = err, k
    print(f"rank {rank}: forward rel-max {fwd:.3e}, worst gradient distance {worst:.3e} at {worst_key}", flush=True)
    assert worst <= 5e-3, (worst, worst_key)
    now = m.state_dict()
    for k in ("final_layer.1.running_mean", "final_layer.1.running_var"):
        assert torch.allclose(now[k].cpu().double(), sd[k], rtol=2e-3, atol=1e-6), (k, now[k].cpu(), sd[k])
    assert int(now["final_layer.1.num_batches_tracked"]) == 1
    if rank == 0:
        os.makedirs(record_dir(), exist_ok=True)
        with open(os.path.join(record_dir(), "parallel_parity.json"), "w") as f:
            json.dump({"config": "tiny", "world_size": world, "pairs_per_rank": 2, "shape": [16, 16], "transport": "gloo, two ranks on one GPU",
                       "forward_rel_max": fwd, "worst_gradient_distance": worst, "worst_parameter": worst_key, "limit": 5e-3}, f, indent=1)

    # 3. sync_head_bn=False: every rank normalises with its own half, and the running statistics part ways
    local = DataParallelStep(m, MyLoss(), opt, group=coll, sync_head_bn=False)
    m.zero_grad(set_to_none=True)
    with local.head_sync():
        m(ir, vis)
    rms = gathered(m.final_layer[1].running_mean, world)
    assert not torch.equal(rms[0], rms[1]), "sync_head_bn=False left the running statistics equal: the switch does nothing"

    # 4. two full steps from one state: the replicas stay bit-identical
    dp.broadcast_state(src=0)
    m.zero_grad(set_to_none=True)
    for i in range(2):
        a, b = shard(rank, step=i + 1)
        loss, detail = dp.step(a.to(dev), b.to(dev))
        assert torch.isfinite(loss).all()
    torch.cuda.synchronize()
    pieces = [p.detach().reshape(-1) for p in m.parameters()]
    pieces += [opt.state[p][k].reshape(-1) for p in m.parameters() for k in ("exp_avg", "exp_avg_sq")]
    pieces += [opt.last_grad_norm.reshape(-1)]
    pieces += [b.detach().reshape(-1).float() for b in m.final_layer[1].buffers()]
    both = gathered(torch.cat(pieces), world)
    assert torch.equal(both[0], both[1]), "the replicas differ after two data-parallel steps"
    assert float(opt.last_grad_norm) > 0
    dist.barrier()
    dist.destroy_process_group()
    print(f"rank {rank} ok", flush=True)


if __name__ == "__main__":
    main()
