"""What ``TrainStatistics`` must report for one ``train_step``, from the oracle (oracle/torch_ref.py) in float64 -- shared by
tests/test_train_statistics.py (CPU operator table) and tests/test_gpu_train_statistics.py.

``reference(b)`` picks the data seed on the oracle: the first seed whose ten logit / similarity matrices of the train_g_d half
(five heads, both directions) have, in EVERY row, a gap between the two largest entries above 1e-3 of the row's largest
magnitude -- the step tests hold the logits to 1e-3 relative, so with such a seed every argmax, i.e. every accuracy, is decided.
The oracle's step on that seed is computed once per batch size and shared.

No seed qualifies at C0 with ``synthetic``'s initialisation and uniform-noise images: the discriminator's pooled features are
nearly the same for every image, so each matrix is nearly constant along its image axis (image_contrastive at B = 4, seed 0:
rows like [9.9804, 9.9804, 9.9812, 9.9806]).  Smallest gaps measured on the oracle, seeds 0-3: B = 4: 2.7e-06, 8.1e-06, 2.1e-06,
7.6e-07; B = 2: 1.8e-06, 8.3e-06, 8.8e-06, 3.5e-05 (the last digits move with the host's thread count) -- against the 1e-3 the
comparison would need to be safe against a 1e-3 logit error.  ``reference`` then keeps the scanned seed with the LARGEST smallest
gap (B = 4: seed 1, B = 2: seed 3), and ``check_accuracies`` still compares every accuracy exactly, no row excluded: what decides
it is then the float32 error of the step under test against a gap of ~1e-4 absolute (rows of magnitude ~10), not the 1e-3 bar."""
import numpy as np
import torch

from oracle import torch_ref as R
from xmcgan_image_generation_amd import synthetic as syn
from xmcgan_image_generation_amd.configs import coco_xmc
from xmcgan_image_generation_amd.xmc_gan import METRIC_KEYS

HEADS = ("fake_word", "real_word", "fake_sentence", "real_sentence", "image_contrastive")
LOGIT_TOL = 1e-3                     # tests/test_gpu_step.py: contrastive logits within 1e-3 of the matrix's largest magnitude
GAP = 1e-3
MAX_SEEDS = 4                        # "among the first few"
_CACHE = {}


def matrices(aux):
    """{head: (matrix, matrix of the other direction)} of the oracle's train_g_d half, float64; None for a switched-off head"""
    out = {}
    for head, key in (("fake_sentence", "fake_sentence_logits"), ("real_sentence", "real_sentence_logits"),
                      ("image_contrastive", "image_contrastive_logits")):
        out[head] = None if aux[key] is None else tuple(m.detach().double() for m in aux[key])
    for head, key in (("fake_word", "fake_word_sim"), ("real_word", "real_word_sim")):
        out[head] = None if aux[key] is None else (aux[key].detach().double(), aux[key].detach().double().t())
    return out


def get_statistics(logits):
    """reference attention_lib.get_statistics (:36-43) with labels = eye, float64 -> (accuracy, entropy)"""
    prob = torch.softmax(logits, dim=-1)
    entropy = -(prob * torch.log(prob + 1e-8)).sum(-1).mean()
    acc = (logits.argmax(-1) == torch.arange(logits.shape[0])).double().mean()
    return float(acc), float(entropy)


def head_statistics(mats):
    """{"<head>_loss" | "_acc" | "_entropy": float} (0 for a switched-off head, reference xmc_net.py:60-64)"""
    out = {}
    for head in HEADS:
        if mats[head] is None:
            out.update({f"{head}_loss": 0.0, f"{head}_acc": 0.0, f"{head}_entropy": 0.0})
            continue
        m1, m2 = mats[head]
        (a1, e1), (a2, e2) = get_statistics(m1), get_statistics(m2)
        out[f"{head}_loss"] = float(R.xent_rows(m1) + R.xent_rows(m2))
        out[f"{head}_acc"] = 0.5 * (a1 + a2)
        out[f"{head}_entropy"] = 0.5 * (e1 + e2)
    return out


def min_row_gap(mats):
    """smallest (largest - second largest) / (largest magnitude) over every row of every matrix"""
    worst = np.inf
    for pair in mats.values():
        for m in pair or ():
            top = m.topk(2, dim=-1).values
            worst = min(worst, float(((top[:, 0] - top[:, 1]) / m.abs().max(dim=-1).values).min()))
    return worst


def entropy_tolerances(mats):
    """per head: ten times the largest change of the head's entropy when its matrices move by the logit tolerance (every entry
    by +-LOGIT_TOL * the matrix's largest magnitude: a few random sign patterns, and the two patterns that sharpen / flatten
    every row -- the largest entry one way, the others the other way)"""
    gen = torch.Generator().manual_seed(7)
    tol = {}
    for head in HEADS:
        if mats[head] is None:
            tol[head] = 0.0
            continue
        base = 0.5 * sum(get_statistics(m)[1] for m in mats[head])
        patterns = []
        for _ in range(6):
            patterns.append([torch.randint(0, 2, m.shape, generator=gen).double() * 2 - 1 for m in mats[head]])
        sharpen = [torch.nn.functional.one_hot(m.argmax(-1), m.shape[-1]).double() * 2 - 1 for m in mats[head]]
        patterns += [sharpen, [-s for s in sharpen]]
        worst = 0.0
        for signs in patterns:
            moved = 0.5 * sum(get_statistics(m + LOGIT_TOL * float(m.abs().max()) * s)[1] for m, s in zip(mats[head], signs))
            worst = max(worst, abs(moved - base))
        tol[head] = 10.0 * worst
    return tol


def _sq_norm(tree):
    return sum(float(t.detach().double().pow(2).sum()) for _, t in R.leaves(tree))


def reference(b, cfg_update=None):
    """-> dict(cfg, seed, gp, gs, dp, ds, batch, expect {name: float}, entropy_tol {head: float}, logit (2B,), ref_metrics)"""
    key = (b, tuple(sorted((cfg_update or {}).items())))
    if key in _CACHE:
        return _CACHE[key]
    cfg = coco_xmc.get_test_config()
    cfg.batch_size = b
    cfg.update(cfg_update or {})
    gp, gs = syn.init_generator(cfg, seed=42, bias_scale=0.05)
    dp, ds = syn.init_discriminator(cfg, seed=43, bias_scale=0.05)
    assert cfg.d_step_per_g_step == 2
    best = None
    for seed in range(MAX_SEEDS):
        batch = syn.make_batch(cfg, per_device_batch=b, seed=seed)
        parts = R._split(R.batch_to_torch(batch), 2)
        mid, _ = R.train_d(R.make_state(gp, gs, dp, ds, torch.float32), parts[0], cfg)       # train_step = train_d, then train_g_d
        ref_new, ref_metrics, dbg = R.train_g_d(mid, parts[1], cfg)
        mats = matrices(dbg["aux"])
        gap = min_row_gap(mats)
        print(f"stats_reference: B = {b}, seed {seed}: smallest top-two gap {gap:.3e}")
        if best is None or gap > best[0]:
            best = (gap, seed, batch, mid, ref_metrics, dbg, mats)
        if gap > GAP:
            break
    gap, seed, batch, mid, ref_metrics, dbg, mats = best
    expect = head_statistics(mats)
    logit = dbg["aux"]["logit"].detach().double().view(-1)
    real, fake = logit[:b], logit[b:]
    expect.update(real_logit_mean=float(real.mean()), fake_logit_mean=float(fake.mean()),
                  real_margin_frac=float((real < 1).double().mean()), fake_margin_frac=float((fake > -1).double().mean()),
                  d_grad_norm=_sq_norm(dbg["d_grad"]) ** 0.5, g_grad_norm=_sq_norm(dbg["g_grad"]) ** 0.5,
                  d_param_norm=_sq_norm(mid["d_params"]) ** 0.5, g_param_norm=_sq_norm(mid["g_params"]) ** 0.5)
    out = dict(cfg=cfg, seed=seed, gap=gap, gp=gp, gs=gs, dp=dp, ds=ds, batch=batch, expect=expect, entropy_tol=entropy_tolerances(mats),
               logit=logit, ref_metrics=ref_metrics)
    _CACHE[key] = out
    return out


def check_values(got, ref, loss_tol, grad_tol, param_tol):
    """``got``: {name: float} of TrainStatistics.vec after ONE train_step on ref's batch.  Prints every figure, then asserts.
    loss_tol: relative to max(1, |want|); grad_tol / param_tol: relative."""
    b = ref["cfg"].batch_size
    expect, logit = ref["expect"], ref["logit"]
    lmax = float(logit.abs().max())
    rows = []
    for head in HEADS:
        rows.append((f"{head}_loss", loss_tol * max(1.0, abs(expect[f"{head}_loss"]))))
        rows.append((f"{head}_entropy", ref["entropy_tol"][head]))
    rows += [("real_logit_mean", LOGIT_TOL * lmax), ("fake_logit_mean", LOGIT_TOL * lmax)]
    # a logit closer to its margin than the logit tolerance may fall on either side of it: each such logit allows 1 / B
    rows.append(("real_margin_frac", float(((logit[:b] - 1).abs() <= LOGIT_TOL * lmax).sum()) / b))
    rows.append(("fake_margin_frac", float(((logit[b:] + 1).abs() <= LOGIT_TOL * lmax).sum()) / b))
    rows += [(k, grad_tol * expect[k]) for k in ("d_grad_norm", "g_grad_norm")]
    rows += [(k, param_tol * expect[k]) for k in ("d_param_norm", "g_param_norm")]
    failed = []
    for name, tol in rows:
        err = abs(got[name] - expect[name])
        print(f"  {name:28s} got {got[name]: .9e} want {expect[name]: .9e} |diff| {err:.3e} allowed {tol:.3e}")
        if not err <= tol:
            failed.append((name, got[name], expect[name], err, tol))
    assert not failed, failed


def check_accuracies(got, ref):
    """the five accuracies equal ``get_statistics`` of the oracle's matrices EXACTLY, no row excluded, on the seed ``reference``
    chose (module docstring: the first that separates every row's two largest entries by GAP, else the best of those scanned)"""
    print(f"  seed {ref['seed']}: smallest top-two gap {ref['gap']:.3e} ({'above' if ref['gap'] > GAP else 'BELOW'} {GAP})")
    for head in HEADS:
        print(f"  {head}_acc got {got[f'{head}_acc']!r} want {ref['expect'][f'{head}_acc']!r}")
    for head in HEADS:
        assert got[f"{head}_acc"] == ref["expect"][f"{head}_acc"], head


def snapshot(state, metrics):
    """everything a step leaves behind, by name: parameters, both Adam moments, EMA, batch_stats, u0 and the five metrics"""
    out = {}
    for name, arena in (("g", state.g_optimizer.arena), ("d", state.d_optimizer.arena)):
        out.update({f"{name}/params": arena.params, f"{name}/m": arena.m, f"{name}/v": arena.v})
    for name, tree in (("batch_stats", state.generator_state["batch_stats"]),
                       ("u0", state.discriminator_state["spectral_norm_stats"])):
        out.update({f"{name}/{p}": t for p, t in syn.tree_leaves(tree)})
    out.update({f"metrics/{k}": torch.as_tensor(metrics[k]).reshape(-1) for k in METRIC_KEYS})
    out["ema"] = state.ema_buffer
    return out
