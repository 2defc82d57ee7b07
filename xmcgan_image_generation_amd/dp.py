"""Data-parallel replicas: gradient averaging over RCCL / xGMI.

The reference's only parallelism is ``jax.pmap`` replicas with ``lax.pmean`` of the G and D gradient
pytrees (``xmcgan/xmc_gan.py:170-171,251``; ``train_utils.py:378-388``): BatchNorm statistics,
spectral-norm vectors and contrastive negatives stay per-replica.  Here: one process
per GPU, ``torch.distributed`` (backend "nccl" == RCCL on ROCm), and each network's gradients are ONE
flat float32 arena, all-reduced in a few large buckets (xGMI is point-to-point, ~153 GB/s per link:
large messages, few launches) issued from a SIDE stream so the exchange of the discriminator
gradients overlaps the generator's backward pass.  The sum is turned into the mean by the 1/world
factor folded into the Adam kernel (``grad_scale``).
"""
from __future__ import annotations

import torch
import torch.distributed as dist


def check_schedule(schedule, bn_groups):
    """Cross-replica BatchNorm groups (``BNGroups``) need the exclusive gradient schedule."""
    if bn_groups is not None and schedule != "exclusive":
        raise ValueError(
            "batch_norm_group_size > 0 needs GradSync(schedule='exclusive'): under the overlapped schedule the gradient "
            "exchange runs on a side stream beside the generator's passes, so the kernels of two communicators (gradient "
            "group, BatchNorm group) sit in parallel branches and nothing makes every rank run them in the same order -- a "
            "deadlock hazard")


def logit_rows(logit, b, replicas=None, rows=None):
    """-> (rows, rank): the (world, 2b) float32 rows that config.ada_target and config.lecam_weight are decided from, and the
    row that is this replica's own.  ``replicas`` (the step's exclusive ``GradSync``): ``GradSync.logit_rows``.  Without: the
    discriminator's (2b,) logit vector ``logit`` itself as ONE row -- a view, no copy and no launch"""
    if replicas is not None:
        return replicas.logit_rows(logit, b, rows), replicas.rank
    assert logit.dtype == torch.float32 and logit.dim() == 1 and logit.is_contiguous()
    return logit.detach()[:2 * int(b)].view(1, 2 * int(b)), 0


class BNGroups:
    """The replica groups that share BatchNorm statistics (``config.batch_norm_group_size > 0``; flax
    ``nn.BatchNorm(axis_name="batch", axis_index_groups=get_device_groups(...))``, reference xmc_net.py:192-201).

    Every rank creates EVERY group with ``dist.new_group`` in the same order (the call is collective over the world) and keeps
    its own: process groups of their own, never the gradient group, even where a group is the whole world.  Without
    ``torch.distributed`` a group of one replica needs no exchange (the split kernels run with a single row); a larger one
    cannot exist.  With it the collectives run even for a group of one: the only way a one-GPU machine exercises them.

    ``gather_rows`` is an all-gather followed -- in the caller -- by a fixed-order sum (ops.bn_finalize_rows / ops.rows_mean),
    not a sum all-reduce: a backend is free to add in any order, and here every rank of a group must compute the same bits
    from the same rows, under gloo and RCCL alike."""

    def __init__(self, config, world=None, rank=None):
        from .utils.device_utils import config_groups
        distributed = dist.is_available() and dist.is_initialized()
        world, self.device_batch, self.groups = config_groups(config, world)
        if rank is None:
            rank = dist.get_rank() if distributed else 0
        self.ranks = next(g for g in self.groups if rank in g)
        self.size = len(self.ranks)
        self.group = None
        if distributed:
            if world != dist.get_world_size():
                raise ValueError(f"BNGroups: world ({world}) is not the initialised process group's size ({dist.get_world_size()})")
            for g in self.groups:
                pg = dist.new_group(g)
                if rank in g:
                    self.group = pg
        elif self.size > 1:
            raise ValueError(f"batch_norm_group_size ({config.batch_norm_group_size}) spans {self.size} replicas of batch "
                             f"{self.device_batch}: that needs torch.distributed to be initialised")

    def check_batch(self, b):
        if int(b) != self.device_batch:
            raise ValueError(f"the BatchNorm groups were built for a per-device batch of {self.device_batch} "
                             f"(batch_norm_group_size {self.size * self.device_batch}), this generator call sees {int(b)}")

    def gather_rows(self, row):
        """row (n,) float32 -> (G, n): the rows of the group's replicas in rank order.  Issued on -- and synchronous with respect
        to -- the current stream (the one the generator runs on); capturable like GradSync's exchanges."""
        row = row.contiguous().view(-1)
        if self.group is None:
            return row.view(1, -1)
        out = torch.empty((self.size, row.numel()), dtype=row.dtype, device=row.device)
        dist.all_gather_into_tensor(out.view(-1), row, group=self.group)      # (the concatenated form: gloo takes no other)
        return out


class GradSync:
    """``transport="bf16"`` (optional, off by default: it changes the numerics the parity tests pin): the gradients travel
    as bfloat16 -- half the bytes on the xGMI links -- and are summed by RCCL in bfloat16; the
    float32 arena is rewritten with the widened sum when the exchange is waited for.  ``transport="float32"`` is the
    reference's ``lax.pmean`` of float32 gradients.

    ``schedule``: WHEN the half steps issue their exchanges (same sums, same parameters -- bit for bit -- either way):
      "overlapped" (default)  sliced from inside the backward passes on the side stream: D's exchange of train_d under the next
                              generator forward, D's of train_g_d under G's backward pass, G's in three buckets behind its slices;
      "exclusive"             each arena in one piece AFTER the backward passes of its half step have finished, waited for before
                              the optimiser kernels start: nothing runs beside the RCCL kernels.  Cost = bytes / link bandwidth,
                              with no contention term (a resident neighbour costs the convolution kernels 18-28 %, profiles/
                              r05_cu_contention.txt): the schedule that cannot lose to the overlap going wrong on real xGMI links."""

    def __init__(self, bucket_elems=32 * 1024 * 1024, group=None, transport="float32", schedule="overlapped", bn_groups=None):
        if not dist.is_initialized():
            raise RuntimeError("GradSync needs torch.distributed to be initialised")
        if transport not in ("float32", "bf16"):
            raise ValueError("transport is 'float32' or 'bf16'")
        if schedule not in ("overlapped", "exclusive"):
            raise ValueError("schedule is 'overlapped' or 'exclusive'")
        self.bn_groups = bn_groups          # the BNGroups of the generator this exchange serves, or None
        check_schedule(schedule, bn_groups)
        self.schedule = schedule
        self.group = group
        self.world = dist.get_world_size(group)
        self.rank = dist.get_rank(group)
        self.bucket = int(bucket_elems)
        self.transport = transport
        self._works = {}
        self._half = {}             # tag -> [(float32 slice, bf16 copy)] to widen back in wait()
        self._side = None

    def require_groups(self, bn_groups):
        """train_step's check: this exchange was built for the generator's BatchNorm groups and (still) runs the exclusive schedule"""
        check_schedule(self.schedule, bn_groups)
        if bn_groups is not self.bn_groups:
            raise ValueError("the generator has BatchNorm groups: build GradSync(schedule='exclusive', bn_groups=generator(train=True).bn_groups)")

    @property
    def exclusive(self) -> bool:
        return self.schedule == "exclusive"

    def _side_stream(self, device):
        if device.type != "cuda":
            return None
        if self._side is None:
            self._side = torch.cuda.Stream(device=device)
        return self._side

    def all_reduce(self, flat: torch.Tensor, tag: str, append: bool = False) -> float:
        """Start the (asynchronous) sum all-reduce of ``flat``; returns the scale (1/world) the
        consumer must apply.  ``flat`` must not be written until ``wait(tag)``.  ``append``: add this exchange to the
        ones already in flight under ``tag`` (bucketed exchange of one arena, issued slice by slice as the backward
        pass completes them)."""
        works = list(self._works.get(tag, [])) if append else []
        side = self._side_stream(flat.device)
        if not append:
            self._half[tag] = []
        if self.transport == "bf16":
            # precision: RCCL then SUMS in bfloat16 across the ranks (8 mantissa bits: an 8-rank sum carries ~3 more bits of
            # rounding than the reference's float32 pmean) -- the price of half the xGMI bytes; off by default
            half = flat.to(torch.bfloat16)                       # one cast pass on the producer stream
            if side is not None:
                half.record_stream(side)                         # allocated on the producer stream, reduced on the side stream
            self._half.setdefault(tag, []).append((flat, half))
            flat = half
        chunks = [flat[i:i + self.bucket] for i in range(0, flat.numel(), self.bucket)]
        if side is not None:
            side.wait_stream(torch.cuda.current_stream())        # gradients are complete
            with torch.cuda.stream(side):
                for c in chunks:
                    works.append(dist.all_reduce(c, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        else:
            for c in chunks:
                works.append(dist.all_reduce(c, op=dist.ReduceOp.SUM, group=self.group, async_op=True))
        self._works[tag] = works
        return 1.0 / self.world

    def wait(self, tag: str):
        """Make the current stream (GPU) / the host (gloo) wait for the exchange tagged ``tag``."""
        for w in self._works.pop(tag, []):
            w.wait()
        for dst, half in self._half.pop(tag, []):
            if half.is_cuda:
                half.record_stream(torch.cuda.current_stream())  # ... and widened on the consumer's stream
            dst.copy_(half)                                      # widen the summed bf16 gradients back into the arena

    def gather_rows(self, row):
        """row (n,) float32 or int32 -> (world, n): the rows of all replicas in rank order.  Issued on -- and synchronous with
        respect to -- the current stream; capturable like ``BNGroups.gather_rows``.  What the controllers that must agree on
        every rank are decided from (ADA's p, the LeCam anchors, the non-finite guard's verdict): an all-gather
        followed -- in the caller -- by one fixed-order kernel over all rows, never a sum all-reduce, so that every rank
        computes the same bits under gloo and RCCL alike.

        Exclusive schedule only (ValueError otherwise), and that is why the GRADIENT communicator may be reused here: under it
        every exchange has been waited for before the next collective is issued, so nothing is in flight on this group beside
        the gather, and every rank issues the same collectives in the same (program) order.  Under the overlapped schedule a
        sliced gradient exchange would be running on the side stream, and the order in which the two reach the communicator
        would be decided by the streams of each rank: a deadlock hazard."""
        if not self.exclusive:
            raise ValueError("GradSync.gather_rows needs GradSync(schedule='exclusive'): under the overlapped schedule gradient "
                             "slices are in flight on this communicator beside the caller's stream")
        if row.dtype not in (torch.float32, torch.int32):
            raise ValueError(f"GradSync.gather_rows takes float32 or int32 rows, got {row.dtype}")
        row = row.contiguous().view(-1)
        out = torch.empty((self.world, row.numel()), dtype=row.dtype, device=row.device)
        dist.all_gather_into_tensor(out.view(-1), row, group=self.group)      # (the concatenated form: gloo takes no other)
        return out

    def logit_rows(self, logit, b, rows=None):
        """-> the all-gathered (world, 2b) float32 rows, in rank order, of the discriminator's (2b,) logit vector ``logit``.
        ``rows``: the rows when another controller of the same half step has gathered them already -- one gather serves ADA
        and LeCam."""
        if rows is None:
            rows = self.gather_rows(logit.detach().float().reshape(-1)[:2 * int(b)])
        return rows

    def mean_metrics(self, metrics: dict) -> dict:
        """TrainMetrics.gather_from_model_output (xmc_gan.py:185-190): mean over replicas."""
        keys = sorted(metrics)
        v = torch.stack([metrics[k].reshape(()).float() for k in keys])
        dist.all_reduce(v, group=self.group)
        v = v / self.world
        return {k: v[i] for i, k in enumerate(keys)}
