#!/usr/bin/env python
"""Cross-replica BatchNorm groups (config.batch_norm_group_size > 0) on ONE GPU: a torchrun worker for tests/test_gpu_syncbn_dp.py.

SYNCBN_MODE=generator (2 ranks, gloo: RCCL refuses two ranks per device), SYNCBN_DUMP=<dir>: float32, per-device batch 2, one group
  of both ranks.  Each rank runs Generator.forward(train=True) and backward on its inputs and its slice of one fixed cotangent
  (tests/syncbn_reference.py) and writes images, new batch_stats and gradients to <dir>/generator_<group>_rank<r>.pt -- once with
  batch_norm_group_size = 4 and once with -1 (the control: per-replica statistics).
SYNCBN_MODE=step (2 ranks, gloo), SYNCBN_DTYPE=float32|bfloat16: one train_step with GradSync(schedule="exclusive") and groups on;
  everything finite, G's and D's parameters and G's batch_stats identical across the ranks; the overlapped schedule is refused.
SYNCBN_MODE=graph (1 rank, backend nccl = RCCL): batch_norm_group_size = the per-device batch, so the group is this one rank and
  its collectives run inside the captured graph.  One eager step + three replays of GraphedTrainStep must be BIT-equal to four
  eager steps of the same configuration and to four eager steps with batch_norm_group_size = -1 (one row: 0 + 1 * x).
usage: python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port <port> tools/dp_syncbn_one_gpu.py"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from xmcgan_image_generation_amd import dp, synthetic, train_utils, xmc_gan  # noqa: E402
from xmcgan_image_generation_amd.configs import coco_xmc  # noqa: E402


def _fresh(cfg):
    gp, gs = synthetic.init_generator(cfg, seed=42, bias_scale=0.05)
    dp_, ds = synthetic.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    return gen, disc, train_utils.load_flax_params(state, gp, gs, dp_, ds)


def _same_on_all_ranks(t, world):
    mine = t.detach().float().cpu().contiguous()
    others = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(others, mine)
    return all(torch.equal(o, others[0]) for o in others) and bool(torch.isfinite(mine).all())


def generator_mode(rank, world):
    from tests import syncbn_reference as S
    assert world == S.WORLD
    for group in (S.PER_DEVICE * S.WORLD, -1):
        out = S.run_rank(S.config(group), rank, "cuda")
        torch.save(out, os.path.join(os.environ["SYNCBN_DUMP"], f"generator_{group}_rank{rank}.pt"))
    if rank == 0:
        print("syncbn generator OK")


def step_mode(rank, world):
    cfg = coco_xmc.get_test_config()
    cfg.dtype = os.environ.get("SYNCBN_DTYPE", "bfloat16")
    cfg.batch_size = 2 * world
    cfg.batch_norm_group_size = 2 * world
    gen, disc, state = _fresh(cfg)
    groups = gen(train=True).bn_groups
    assert groups.ranks == list(range(world)) and groups.group is not None
    try:
        dp.GradSync(schedule="overlapped", bn_groups=groups)
        raise AssertionError("the overlapped schedule was accepted with BatchNorm groups")
    except ValueError as e:
        assert "deadlock" in str(e)
    sync = dp.GradSync(schedule="exclusive", bn_groups=groups)
    batch = {k: torch.as_tensor(v).cuda() for k, v in synthetic.make_batch(cfg, per_device_batch=2, rank=rank).items()}
    state, metrics = train_utils.train_step(0, state, batch, xmc_gan, gen, disc, cfg, {}, grad_sync=sync)
    torch.cuda.synchronize()
    assert all(math.isfinite(float(v)) for v in metrics.values()), metrics
    assert _same_on_all_ranks(state.g_optimizer.arena.params, world), "G parameters"
    assert _same_on_all_ranks(state.d_optimizer.arena.params, world), "D parameters"
    for path, t in synthetic.tree_leaves(state.generator_state["batch_stats"]):
        assert _same_on_all_ranks(t, world), path
    if rank == 0:
        print(f"syncbn step OK {cfg.dtype}", {k: round(float(v), 4) for k, v in metrics.items()})


def graph_mode(rank, world):
    assert world == 1
    dtype = os.environ.get("SYNCBN_DTYPE", "bfloat16")

    def cfg_of(group):
        cfg = coco_xmc.get_test_config()
        cfg.dtype = dtype
        cfg.batch_size = 2
        cfg.batch_norm_group_size = group
        return cfg
    batches = [{k: torch.as_tensor(v).cuda() for k, v in synthetic.make_batch(cfg_of(-1), per_device_batch=2, rank=r).items()}
               for r in range(4)]

    def run(group, graph):
        cfg = cfg_of(group)
        gen, disc, state = _fresh(cfg)
        groups = gen(train=True).bn_groups
        assert (groups is None) == (group <= 0) and (groups is None or groups.group is not None)
        sync = dp.GradSync(schedule="exclusive", bn_groups=groups)
        metrics = []
        state, m = train_utils.train_step(0, state, batches[0], xmc_gan, gen, disc, cfg, {}, grad_sync=sync)
        metrics.append(m)
        if graph:
            graphed = train_utils.GraphedTrainStep(state, batches[1], xmc_gan, gen, disc, cfg, {}, grad_sync=sync)
            state = graphed.state
            for tb in batches[1:]:
                state, m = graphed(state, tb)
                metrics.append({k: v.clone() for k, v in m.items()})
        else:
            for tb in batches[1:]:
                state, m = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {}, grad_sync=sync)
                metrics.append(m)
        torch.cuda.synchronize()
        state = xmc_gan._flush(state)
        assert all(math.isfinite(float(v)) for m in metrics for v in m.values())
        return dict(g=state.g_optimizer.arena.params.clone(), d=state.d_optimizer.arena.params.clone(),
                    bn=[(p, t.clone()) for p, t in synthetic.tree_leaves(state.generator_state["batch_stats"])],
                    g_loss=[float(m["g_loss"]) for m in metrics])

    graphed, eager, default = run(2, True), run(2, False), run(-1, False)
    for name, other in (("eager steps with the group", eager), ("eager steps with batch_norm_group_size = -1", default)):
        for key in ("g", "d"):
            same = torch.equal(graphed[key], other[key])
            print(f"graph replay vs {name}: {key} parameters identical={same}"
                  + ("" if same else f" (fraction differing {float((graphed[key] != other[key]).float().mean()):.3e})"))
            assert same, (name, key)
        for (p, a), (_, b) in zip(graphed["bn"], other["bn"]):
            assert torch.equal(a, b), (name, p)
        assert graphed["g_loss"] == other["g_loss"], (name, graphed["g_loss"], other["g_loss"])
    print(f"syncbn graph OK {dtype}", graphed["g_loss"])


def main():
    mode = os.environ.get("SYNCBN_MODE", "generator")
    torch.cuda.set_device(0)
    if mode == "graph":
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    {"generator": generator_mode, "step": step_mode, "graph": graph_mode}[mode](rank, world)
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
