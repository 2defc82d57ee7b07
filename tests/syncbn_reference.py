"""Shared by the two-rank tests of cross-replica BatchNorm groups (tests/test_syncbn_gloo.py on the mock operator table,
tests/test_gpu_syncbn_dp.py + tools/dp_syncbn_one_gpu.py on the HIP backend): the fixed inputs of the generator-level case, what
one rank runs, the float64 oracle on the CONCATENATED batch and the per-leaf comparison.

The case: get_test_config(), two ranks of per-device batch 2 (config.batch_size = 4), batch_norm_group_size = 4 -> one group of
both ranks; parameters syn.init_generator(cfg, 42, bias_scale=0.05); rank r's inputs are the first two samples of
syn.make_batch(cfg, per_device_batch=2, rank=r); the cotangent is one fixed random image batch, rank r takes rows [2r, 2r + 2)."""
import functools

import torch

from oracle import torch_ref as R
from xmcgan_image_generation_amd import synthetic as syn
from xmcgan_image_generation_amd.configs import coco_xmc

COND_KEYS = ("sentence_embedding", "embedding", "max_len")
PER_DEVICE, WORLD = 2, 2


def config(group, dtype="float32"):
    cfg = coco_xmc.get_test_config()
    cfg.dtype = dtype
    cfg.batch_size = PER_DEVICE * WORLD
    cfg.batch_norm_group_size = group
    return cfg


def rank_inputs(cfg, rank):
    batch = syn.make_batch(cfg, per_device_batch=PER_DEVICE, rank=rank)
    return {k: torch.as_tensor(batch[k][:PER_DEVICE]) for k in COND_KEYS + ("z",)}


def cotangent(cfg):
    """One fixed random cotangent, U[0, 1) like the images of syn.make_batch.  Not white noise around zero: under an N(0, 1)
    cotangent every parameter gradient is a sum of random-signed terms that cancel to a small fraction of their mass, and the
    float32 ORACLE is then 2.1e-3 (worst leaf, norm-relative) from the float64 oracle on this very case -- above the gates,
    whatever the implementation.  With the positive cotangent the float32 oracle is 4.1e-4 from the float64 one."""
    g = torch.Generator().manual_seed(7)
    return torch.rand((PER_DEVICE * WORLD, cfg.image_size, cfg.image_size, 3), generator=g)


def run_rank(cfg, rank, device="cpu"):
    """What one rank runs (torch.distributed initialised, operator table chosen by the caller): create_train_state, the fixed
    parameters, Generator.forward(train=True, need_tape=True) and backward -> CPU tensors: images, the new batch_stats leaves
    and the gradient leaves, in tree order."""
    from xmcgan_image_generation_amd import train_utils
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    gen, _, state = train_utils.create_train_state(cfg, 0)
    state = train_utils.load_flax_params(state, gp, gs)
    inp = {k: v.to(device) for k, v in rank_inputs(cfg, rank).items()}
    g = gen(train=True)
    arena = state.g_optimizer.arena
    img, new_stats, tape = g.forward(state.g_optimizer.target, state.generator_state["batch_stats"],
                                     {k: inp[k] for k in COND_KEYS}, inp["z"], train=True, need_tape=True)
    dimg = cotangent(cfg)[rank * PER_DEVICE:(rank + 1) * PER_DEVICE].contiguous().to(device=device, dtype=img.dtype)
    arena.zero_grads()
    g.backward(tape, dimg)
    if device != "cpu":
        torch.cuda.synchronize()
    cpu = lambda t: t.detach().float().cpu().clone()
    return dict(img=cpu(img), bn=[(p, cpu(t)) for p, t in syn.tree_leaves(new_stats)],
                grads=[(p, cpu(t)) for p, t in syn.tree_leaves(arena.tree(arena.grads))])


@functools.lru_cache(maxsize=None)
def reference(dtype=torch.float64):
    """the oracle generator (training mode) on the concatenated batch of 4 with autograd -> the same dict as run_rank, images of
    all four samples, gradients of the whole batch's cotangent.

    float64 is the reference of every comparison; ``errors`` also prints the distance of the gradients from the float32 oracle."""
    cfg = config(-1)
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    inps = [rank_inputs(cfg, r) for r in range(WORLD)]
    cat = {k: torch.cat([i[k] for i in inps]).to(dtype) for k in COND_KEYS + ("z",)}
    params = R.to_torch(gp, dtype, requires_grad=True)
    img, new, _ = R.generator(params, R.to_torch(gs, dtype), {k: cat[k] for k in COND_KEYS}, cat["z"], cfg, True)
    leaves = R.leaves(params)
    grads = torch.autograd.grad(img, [t for _, t in leaves], cotangent(cfg).to(dtype))
    return dict(img=img.detach(), bn=[(p, t.detach()) for p, t in R.leaves(new)],
                grads=[(p, g) for (p, _), g in zip(leaves, grads)])


def _rel(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / max(float(b.norm()), 1e-12))


def errors(ranks, ref=None):
    """-> dict(img, bn, bn_leaf, grad, grad_leaf): worst norm-relative error per leaf of the two ranks' dumps against the
    oracle on the concatenated batch: images per rank against their slice, every batch_stats leaf of every rank, and the SUM
    of the ranks' parameter gradients (= the gradient of the whole batch's cotangent).  Gradient leaves whose true value is
    analytically zero (biases that only feed a BatchNorm) hold round-off on both sides, so the gradient error's denominator is
    max(||ref leaf||, 1e-2 x the network's RMS gradient x sqrt(numel)) -- the floor of tests/test_host_logic.py::
    test_gradients_match.  That is looser than plain norm-relative for every leaf whose true gradient is small, not only for the
    zero ones."""
    ref = ref or reference()
    out = dict(img=0.0, bn=0.0, bn_leaf=None, grad=0.0, grad_leaf=None, grad_vs_float32_oracle=0.0)
    for r, d in enumerate(ranks):
        out["img"] = max(out["img"], _rel(d["img"], ref["img"][r * PER_DEVICE:(r + 1) * PER_DEVICE]))
        assert [p for p, _ in d["bn"]] == [p for p, _ in ref["bn"]]
        for (p, a), (_, b) in zip(d["bn"], ref["bn"]):
            e = _rel(a, b)
            if e > out["bn"]:
                out["bn"], out["bn_leaf"] = e, p
    for key, rg in (("grad", ref["grads"]), ("grad_vs_float32_oracle", reference(torch.float32)["grads"])):
        rms = (sum(float(b.double().pow(2).sum()) for _, b in rg) / sum(b.numel() for _, b in rg)) ** 0.5
        assert [p for p, _ in ranks[0]["grads"]] == [p for p, _ in rg]
        for k, (p, b) in enumerate(rg):
            total = sum(d["grads"][k][1].double() for d in ranks)
            e = float((total - b.double()).norm()) / max(float(b.double().norm()), 1e-2 * rms * b.numel() ** 0.5)
            if e > out[key]:
                out[key] = e
                if key == "grad":
                    out["grad_leaf"] = p
    return out
