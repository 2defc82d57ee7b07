"""In-graph training statistics (``config.train_statistics``): what ``train_g_d`` knows about a step beyond its five metrics.

``TrainStatistics`` owns static device buffers.  ``xmc_gan.train_g_d`` fills them -- one ``xmc_segment_sumsq`` launch per arena
buffer in front of each optimiser update (``leaf_pass``), one ``xmc_train_stats`` launch at the end of the half step
(``finish``) -- and the training loop reads them only where it writes scalars (``read`` / ``reset``).  Nothing is read on the
host in between, so a captured step (``train_utils.GraphedTrainStep``) replays the launches with everything else.

Per step, ``NAMES`` in one float32 vector (``vec``; summed in float64 in ``sums``):

* the reference discriminator's 15-key ``statistic_dict`` (xmc_net.py:126-141): loss, accuracy and entropy of the five
  contrastive heads, from the discriminator forward whose losses ``train_g_d`` reports; a switched-off head reports 0;
* ``real_logit_mean``, ``fake_logit_mean``, ``real_margin_frac`` (share of real logits < 1), ``fake_margin_frac`` (share of
  generated logits > -1);
* ``d_grad_norm``, ``g_grad_norm``, ``d_param_norm``, ``g_param_norm``: L2 norms over the arenas at the moment the optimiser
  update of ``train_g_d`` starts -- gradients after the data-parallel exchange and times the update's ``grad_scale``,
  parameters before the update.  With ``ops.fuse_opt`` the gradient through sigma of a spectrally-normalised weight is applied
  inside the optimiser kernel: such a layer's entry is the gradient as the arena stores it, without that term;
* ``d_sigma_min``, ``d_sigma_max`` over the spectral bank's ``scal`` pairs of the step.

Per physical tensor of each arena (``leaves``: every ``ParamArena`` spec with its own offset and each merged ``<module>/GB``,
D's before G's, in arena order): the sum of squares of its gradient and of its parameters and the number of non-finite gradient
elements, per step (``leaf_gsq`` / ``leaf_psq`` / ``leaf_bad``) and summed over the window (``win_*``).

The statistics are those of THIS replica: nothing is averaged over replicas.  On an operator table without the two entry points
(the tests' CPU table) both launches are restated in float64 torch."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from .nets.xmc_net import LOSS_SLOTS, STAT_KEYS


def arena_leaves(arena):
    """[(path, offset, number of elements)] of the physical tensors of a ``ParamArena``, in arena order"""
    out = [(p, sp[0], int(np.prod(sp[1]))) for p, sp in arena.specs.items() if sp[0] is not None]
    out += [(p, off, int(np.prod(shape))) for p, (off, shape) in arena.merged.items()]
    return sorted(out, key=lambda e: e[1])


class TrainStatistics:
    NAMES = tuple(STAT_KEYS) + ("real_logit_mean", "fake_logit_mean", "real_margin_frac", "fake_margin_frac",
                                "d_grad_norm", "g_grad_norm", "d_param_norm", "g_param_norm", "d_sigma_min", "d_sigma_max")

    def __init__(self):
        self._arenas = None
        self._fwd = None
        self.leaves = []

    # ----------------------------------------------------------------------------------------------------------- buffers
    def bind(self, ops, d_arena, g_arena):
        """allocate the static buffers for this pair of arenas (once: a captured graph owns their addresses)"""
        if self._arenas is not None and self._arenas[0] is d_arena and self._arenas[1] is g_arena:
            return self
        self._arenas = (d_arena, g_arena)
        dev = d_arena.params.device
        self.native = hasattr(ops, "segment_sumsq") and hasattr(ops, "train_stats")
        per = {"d": arena_leaves(d_arena), "g": arena_leaves(g_arena)}
        self.leaves = [(w, p, off, n) for w in ("d", "g") for p, off, n in per[w]]
        self.leaf_names = [f"{w}/{p}" for w, p, _, _ in self.leaves]
        self.n_d, nl = len(per["d"]), len(self.leaves)
        self._range = {"d": (0, self.n_d), "g": (self.n_d, nl)}
        self._scale = {"d": 1.0, "g": 1.0}
        z = lambda n, dt: torch.zeros((n,), dtype=dt, device=dev)
        self.vec, self.sums, self.info = z(len(self.NAMES), torch.float32), z(len(self.NAMES), torch.float64), z(4, torch.int32)
        self.leaf_gsq, self.leaf_psq, self.leaf_bad = z(nl, torch.float64), z(nl, torch.float64), z(nl, torch.int32)
        self.leaf_pbad = z(nl, torch.int32)                                  # (the parameter pass's count: not reported)
        self.win_gsq, self.win_psq, self.win_bad = z(nl, torch.float64), z(nl, torch.float64), z(nl, torch.int64)
        self._segs, self._segs_host, self._ws = {}, {}, {}
        for w in ("d", "g"):
            flat = [v for _, off, n in per[w] for v in (off, n)]
            self._segs[w] = torch.tensor(flat, dtype=torch.int64).view(-1, 2).to(dev)
            self._segs_host[w] = (C.c_int64 * len(flat))(*flat)
            if self.native:
                nbytes = ops.segment_sumsq_ws_bytes(self._segs_host[w], len(per[w]))
                # one workspace per launch of a step: D's pair may run beside the generator's backward pass
                self._ws[w] = [torch.empty((nbytes,), dtype=torch.uint8, device=dev) for _ in range(2)]
        return self

    # -------------------------------------------------------------------------------------------------------- per step
    def leaf_pass(self, ops, which, arena, grad_scale=1.0):
        """per-tensor sums of ``arena``'s gradients and parameters, on the current stream (xmc_gan._apply_adam calls this in
        front of the update it is about to issue)"""
        lo, hi = self._range[which]
        self._scale[which] = float(grad_scale)
        if self.native:
            segs, host, ws = self._segs[which], self._segs_host[which], self._ws[which]
            ops.segment_sumsq(arena.grads, segs, host, self.leaf_gsq[lo:hi], self.leaf_bad[lo:hi], ws[0])
            ops.segment_sumsq(arena.params, segs, host, self.leaf_psq[lo:hi], self.leaf_pbad[lo:hi], ws[1])
            return
        for i, (_, _, off, n) in enumerate(self.leaves[lo:hi], start=lo):
            g, p = arena.grads[off:off + n].double(), arena.params[off:off + n].double()
            self.leaf_gsq[i] = (g * g).sum()
            self.leaf_psq[i] = (p * p).sum()
            self.leaf_bad[i] = int((~torch.isfinite(arena.grads[off:off + n])).sum())

    def note_forward(self, logit, loss_vec, head_stats, scal):
        """the discriminator forward whose losses the half step reports (xmc_gan._forward)"""
        self._fwd = (logit, loss_vec, head_stats, scal)

    def finish(self, ops):
        """gather the step's vector and add it, and the per-tensor tables, to the window sums: one launch on the current stream"""
        logit, loss_vec, head_stats, scal = self._fwd
        self._fwd = None
        b = logit.numel() // 2
        n_sigma = scal.numel() // 2 if scal is not None else 0
        if self.native:
            from ._lib import TrainStatsArgs
            ptr = lambda t: t.data_ptr() if t is not None else None
            assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (logit, loss_vec, head_stats))
            assert loss_vec.numel() == len(LOSS_SLOTS) and head_stats.numel() == 2 * len(LOSS_SLOTS)
            args = TrainStatsArgs(ptr(logit), ptr(scal), ptr(loss_vec), ptr(head_stats), ptr(self.leaf_gsq), ptr(self.leaf_psq),
                                  ptr(self.leaf_bad), ptr(self.vec), ptr(self.sums), ptr(self.info), ptr(self.win_gsq),
                                  ptr(self.win_psq), ptr(self.win_bad), b, n_sigma, len(self.leaves), self.n_d,
                                  self._scale["d"], self._scale["g"])
            ops.train_stats(args)
            return
        f64 = torch.float64
        v = torch.zeros((len(self.NAMES),), dtype=f64)
        v[0:15:3], v[1:15:3], v[2:15:3] = loss_vec.to(f64), head_stats.view(-1, 2)[:, 0].to(f64), head_stats.view(-1, 2)[:, 1].to(f64)
        real, fake = logit[:b].to(f64), logit[b:].to(f64)
        v[15], v[16] = real.mean(), fake.mean()
        v[17], v[18] = (logit[:b] < 1).to(f64).mean(), (logit[b:] > -1).to(f64).mean()
        nd = self.n_d
        v[19], v[20] = self.leaf_gsq[:nd].sum().sqrt() * abs(self._scale["d"]), self.leaf_gsq[nd:].sum().sqrt() * abs(self._scale["g"])
        v[21], v[22] = self.leaf_psq[:nd].sum().sqrt(), self.leaf_psq[nd:].sum().sqrt()
        if n_sigma:
            sigma = scal.view(-1, 2)[:, 0]
            v[23], v[24] = sigma.min(), sigma.max()
        self.vec.copy_(v.to(torch.float32))
        self.sums += self.vec.to(f64)
        sc = torch.cat([torch.full((nd,), self._scale["d"] ** 2, dtype=f64), torch.full((len(self.leaves) - nd,), self._scale["g"] ** 2, dtype=f64)])
        self.win_gsq += self.leaf_gsq * sc
        self.win_psq += self.leaf_psq
        self.win_bad += self.leaf_bad.to(torch.int64)
        self.info[0] += 1
        bad = torch.nonzero(self.leaf_bad)
        if int(self.info[1]) == 0 and bad.numel():
            self.info[1], self.info[2] = self.info[0], int(bad[0])

    # ------------------------------------------------------------------------------------------------------- the loop
    def read(self):
        """the only host synchronisation -> dict(count, sums {name: float64 window sum}, leaves {"d/<path>" | "g/<path>":
        (window sum of the gradient's squares, ... of the parameters' squares, non-finite gradient elements)},
        first_bad (1-based call of the window whose gradients first held a non-finite value, that leaf's name) or None)"""
        if self._arenas is None:
            return dict(count=0, sums={k: 0.0 for k in self.NAMES}, leaves={}, first_bad=None)
        count, call, leaf, _ = self.info.cpu().tolist()
        sums = dict(zip(self.NAMES, self.sums.cpu().tolist()))
        rows = zip(self.win_gsq.cpu().tolist(), self.win_psq.cpu().tolist(), self.win_bad.cpu().tolist())
        return dict(count=count, sums=sums, leaves=dict(zip(self.leaf_names, rows)),
                    first_bad=(call, self.leaf_names[leaf]) if call else None)

    def reset(self):
        if self._arenas is not None:
            for t in (self.sums, self.info, self.win_gsq, self.win_psq, self.win_bad):
                t.zero_()
