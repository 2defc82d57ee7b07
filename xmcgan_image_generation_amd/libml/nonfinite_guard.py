"""``config.skip_nonfinite_updates``: a half step whose gradients are not finite is not applied.

``NonfiniteGuard`` owns the device buffers of the decision: ``verdict`` (int32[4]: any bad value, how many, the first segment that
held one, 0) written once per half step by ``judge``, and the persistent ``counters`` (int32[4]: half steps skipped in total, the
current run of skipped ones, the longest run, padding) that travel in the checkpoint.  On ``HipOps`` ``judge`` is
``xmc_nonfinite_verdict`` (two launches, no host read: a captured step replays it) and ``commit`` is ``xmc_commit_if``; on an operator
table without those ops the same arithmetic runs in torch.  Nothing here reads the verdict on the host -- ``read`` (the training loop,
at a logging boundary) is the only synchronisation."""
from __future__ import annotations

import torch

MAX_SEGMENTS = 8                     # XMC_NONFINITE_MAX_SEGMENTS
_WS_BYTES = 16 * 1024                # the largest workspace xmc_nonfinite_verdict asks for: 1024 workgroups x 16 bytes
_INT32_MAX = 2147483647


def enabled(config):
    return bool(config.get("skip_nonfinite_updates", False))


def max_consecutive(config):
    """``config.nonfinite_max_consecutive``: the run of skipped half steps at which ``train`` gives up (a policy default, not a
    measurement: a NaN that persists means the parameters or the data are bad, and skipping cannot help)"""
    return int(config.get("nonfinite_max_consecutive", 100))


class NonfiniteGuard:
    def __init__(self, device):
        self.verdict = torch.zeros((4,), dtype=torch.int32, device=device)
        self.counters = torch.zeros((4,), dtype=torch.int32, device=device)
        self._ws = torch.zeros((_WS_BYTES,), dtype=torch.uint8, device=device)

    # ------------------------------------------------------------------------------------------------ device side
    def judge(self, ops, segments):
        """one verdict over the flat float32 tensors ``segments`` (everything the half step is about to commit) -> ``verdict``"""
        segments = [t.reshape(-1) for t in segments]
        if not 1 <= len(segments) <= MAX_SEGMENTS:
            raise ValueError(f"NonfiniteGuard.judge takes 1 to {MAX_SEGMENTS} segments")
        for t in segments:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("NonfiniteGuard.judge scans contiguous float32 buffers")
        if hasattr(ops, "nonfinite_verdict"):
            if ops.nonfinite_verdict_ws_bytes([t.numel() for t in segments]) > self._ws.numel():
                raise ValueError("NonfiniteGuard: the verdict's workspace is too small")
            ops.nonfinite_verdict(segments, self.verdict, self.counters, self._ws)
            return self.verdict
        # the same arithmetic in torch (operator tables without the op)
        bad, first = 0, -1
        for i, t in enumerate(segments):
            k = int((~torch.isfinite(t)).sum())
            if k and first < 0:
                first = i
            bad += k
        self.verdict.copy_(torch.tensor([int(bad > 0), min(bad, _INT32_MAX), first, 0], dtype=torch.int32))
        c = self.counters.tolist()
        if bad:
            c[0] = min(c[0] + 1, _INT32_MAX)
            c[1] = min(c[1] + 1, _INT32_MAX)
            c[2] = max(c[2], c[1])
        else:
            c[1] = 0
        self.counters.copy_(torch.tensor(c, dtype=torch.int32))
        return self.verdict

    def commit(self, ops, dst, src):
        """dst = src unless the verdict is bad"""
        if dst.data_ptr() == src.data_ptr():
            return dst
        if hasattr(ops, "commit_if"):
            return ops.commit_if(dst, src.contiguous(), self.verdict)
        if int(self.verdict[0]) == 0:
            dst.copy_(src)
        return dst

    # -------------------------------------------------------------------------------------------------- host side
    def read(self):
        """-> dict(skipped=half steps skipped in total, run=the current run of skipped half steps, longest=the longest run since
        ``reset_longest``).  A host synchronisation."""
        total, run, longest, _ = self.counters.cpu().tolist()
        return dict(skipped=total, run=run, longest=longest)

    def reset_longest(self):
        """start a new window: the longest run restarts from the run that is still going on"""
        self.counters[2:3].copy_(self.counters[1:2])

    def state_dict(self):
        import numpy as np
        return {"counters": self.counters.cpu().numpy().astype(np.int32)}

    def load_state_dict(self, d):
        import numpy as np
        self.counters.copy_(torch.from_numpy(np.asarray(d["counters"], dtype=np.int32).reshape(4).copy()))
