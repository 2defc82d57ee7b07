#!/usr/bin/env python
"""config.ada_target, config.lecam_weight and config.skip_nonfinite_updates with data-parallel replicas on ONE
GPU: a torchrun worker for tests/test_gpu_replica_controllers_dp.py.

DPC_MODE=step (2 ranks, gloo: RCCL refuses two ranks per device): float32, eager, get_test_config(), per-device batch 2, all three
  switches on, GradSync(schedule="exclusive").  Three train_steps; after each, G's and D's parameters, ada.state, lecam.state and
  guard.counters are bit-identical on the two ranks; p > 0 and the anchors are non-zero at the end.  Then the same run with a NaN in
  rank 1's z in step 2: both ranks keep the parameters of step 1, both count the two skipped half steps, step 3 proceeds.
DPC_MODE=graph (1 rank, backend nccl = RCCL), bfloat16: one eager step + three replays of GraphedTrainStep with the switches on and
  the exclusive exchange -- the all-gathers are inside the captured graph, and with one row the ``_rows`` kernels reduce to the
  single-process ones -- must be BIT-equal to four eager steps with grad_sync=None: parameters, moments, EMA, ada.state,
  lecam.state, guard.counters and the metrics.
usage: python -m torch.distributed.run --nproc-per-node 2 --master-addr 127.0.0.1 --master-port <port> tools/dp_controllers_one_gpu.py"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from xmcgan_image_generation_amd import dp, synthetic, train_utils, xmc_gan  # noqa: E402
from xmcgan_image_generation_amd.configs import coco_xmc  # noqa: E402
from xmcgan_image_generation_amd.libml import ada as ada_lib  # noqa: E402
from xmcgan_image_generation_amd.libml import diff_augment  # noqa: E402
from xmcgan_image_generation_amd.libml import lecam as lecam_lib  # noqa: E402

B = 2
POLICY = "color,translation,cutout"


def _cfg(dtype):
    cfg = coco_xmc.get_test_config()
    cfg.dtype, cfg.batch_size, cfg.pretrained_image_contrastive = dtype, B, False
    cfg.update(dict(diff_augment=POLICY, ada_target=0.6, ada_interval=1, ada_kimg=0.05, lecam_weight=0.3, lecam_start=0,
                    skip_nonfinite_updates=True))
    return cfg


def _fresh(cfg):
    gp, gs = synthetic.init_generator(cfg, seed=42, bias_scale=0.05)
    dp_, ds = synthetic.init_discriminator(cfg, seed=43, bias_scale=0.05)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    return gen, disc, train_utils.load_flax_params(state, gp, gs, dp_, ds)


def _batch(cfg, step, rank):
    tb = {k: torch.as_tensor(v).cuda() for k, v in synthetic.make_batch(cfg, per_device_batch=B, rank=rank, seed=1234 + step).items()}
    rows = B * cfg.d_step_per_g_step
    tb["d_aug"] = torch.from_numpy(diff_augment.draw_plan(11, step, rank, rows, cfg.image_size, cfg.image_size, POLICY))
    tb["d_aug_u"] = torch.from_numpy(ada_lib.draw_gates(11, step, rank, rows))
    return tb


def _small(state):
    return dict(ada=state.ada.state, lecam=state.lecam.state, counters=state.guard.counters)


def _bits(t):
    return t.detach().contiguous().view(torch.int32).reshape(-1).cpu()


def _same_bits_on_all_ranks(t, world):
    mine = _bits(t)
    others = [torch.empty_like(mine) for _ in range(world)]
    dist.all_gather(others, mine)
    return all(torch.equal(o, others[0]) for o in others)


def step_mode(rank, world):
    assert world == 2
    cfg = _cfg("float32")
    runs = {}
    for scenario in ("clean", "nan"):
        gen, disc, state = _fresh(cfg)
        ops = gen(train=True).ops
        assert all(hasattr(ops, name) for name in ("ada_update_rows", "lecam_rows", "verdict_merge"))
        sync = dp.GradSync(schedule="exclusive")
        snaps = []
        for step in (1, 2, 3):
            batch = _batch(cfg, step, rank)
            if scenario == "nan" and step == 2 and rank == 1:
                batch["z"][:, 0] = float("nan")       # every half step of this rank's step 2
            state, metrics = train_utils.train_step(step, state, batch, xmc_gan, gen, disc, cfg, {}, grad_sync=sync)
            torch.cuda.synchronize()
            tensors = dict(_small(state), g=state.g_optimizer.arena.params, d=state.d_optimizer.arena.params)
            for name, t in tensors.items():
                assert _same_bits_on_all_ranks(t, world), (scenario, step, name)
            snaps.append(dict({k: t.clone() for k, t in tensors.items()}, metrics={k: float(v) for k, v in metrics.items()}))
        train_utils.check_replica_drift(_small(state), sync)
        runs[scenario] = snaps
    last = runs["clean"][-1]
    assert all(math.isfinite(v) for s in runs["clean"] for v in s["metrics"].values()), runs["clean"]
    assert last["counters"].tolist() == [0, 0, 0, 0]
    assert float(last["ada"][ada_lib.P]) > 0 and float(last["ada"][ada_lib.ADJUSTMENTS]) == 6, last["ada"]
    assert float(last["lecam"][lecam_lib.ANCHOR_REAL]) != 0 and float(last["lecam"][lecam_lib.ANCHOR_FAKE]) != 0, last["lecam"]
    assert float(last["lecam"][lecam_lib.UPDATES]) == 6 and last["metrics"][lecam_lib.METRIC_KEY] > 0
    s1, s2, s3 = runs["nan"]
    assert torch.equal(s1["g"], runs["clean"][0]["g"]) and torch.equal(s1["d"], runs["clean"][0]["d"])
    assert torch.equal(s2["g"], s1["g"]) and torch.equal(s2["d"], s1["d"]), "a rank applied the half steps of the NaN batch"
    assert s2["counters"].tolist() == [2, 2, 2, 0] and s3["counters"].tolist() == [2, 0, 2, 0], (s2["counters"], s3["counters"])
    assert not torch.equal(s3["g"], s2["g"]) and not torch.equal(s3["d"], s2["d"])
    assert bool(torch.isfinite(s3["g"]).all()) and bool(torch.isfinite(s3["d"]).all())
    # (the anchors are forward values outside the verdict: they tick through the skipped step, and they move in it wherever a
    # max(x, 0) of the generator turned the NaN into finite images and logits)
    assert float(s2["lecam"][lecam_lib.TICKS]) == 4 and float(s3["lecam"][lecam_lib.TICKS]) == 6
    if rank == 0:
        print("controllers step OK", "p", float(last["ada"][ada_lib.P]), "anchors", last["lecam"][:2].tolist(), "skipped", s3["counters"].tolist())


def graph_mode(rank, world):
    assert world == 1
    cfg = _cfg("bfloat16")
    batches = [_batch(cfg, step, 0) for step in range(4)]

    def run(replicas):
        gen, disc, state = _fresh(cfg)
        sync = dp.GradSync(schedule="exclusive") if replicas else None
        metrics = []
        if replicas:
            state, m = train_utils.train_step(0, state, batches[0], xmc_gan, gen, disc, cfg, {}, grad_sync=sync)
            metrics.append({k: float(v) for k, v in m.items()})
            graphed = train_utils.GraphedTrainStep(state, batches[1], xmc_gan, gen, disc, cfg, {}, grad_sync=sync)
            state = graphed.state
            for tb in batches[1:]:
                state, m = graphed(state, tb)
                metrics.append({k: float(v) for k, v in m.items()})
        else:
            for tb in batches:
                state, m = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {})
                metrics.append({k: float(v) for k, v in m.items()})
        torch.cuda.synchronize()
        state = xmc_gan._flush(state)
        out = {f"{n}.{k}": getattr(a, k).clone() for n, a in (("d", state.d_optimizer.arena), ("g", state.g_optimizer.arena))
               for k in ("params", "m", "v")}
        out.update(ema=state.ema_buffer.clone(), verdict=state.guard.verdict.clone(), **{k: t.clone() for k, t in _small(state).items()})
        return out, metrics

    (got, got_m), (want, want_m) = run(True), run(False)
    for name in want:
        same = torch.equal(_bits(got[name]), _bits(want[name]))
        print(f"graph replay with the exclusive exchange vs eager steps without replicas: {name} identical={same}")
        assert same, name
    assert got_m == want_m, (got_m, want_m)
    assert all(math.isfinite(v) for m in want_m for v in m.values()), want_m
    assert float(want["ada"][ada_lib.ADJUSTMENTS]) == 8 and float(want["lecam"][lecam_lib.UPDATES]) == 8
    assert want["counters"].tolist() == [0, 0, 0, 0] and want_m[-1][lecam_lib.METRIC_KEY] > 0
    print("controllers graph OK", "p", float(want["ada"][ada_lib.P]), "anchors", want["lecam"][:2].tolist())


def main():
    mode = os.environ.get("DPC_MODE", "step")
    torch.cuda.set_device(0)
    if mode == "graph":
        dist.init_process_group("nccl", device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo")
    {"step": step_mode, "graph": graph_mode}[mode](dist.get_rank(), dist.get_world_size())
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
