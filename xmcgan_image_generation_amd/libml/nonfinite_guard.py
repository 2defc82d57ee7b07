"""``config.skip_nonfinite_updates``: a half step whose gradients are not finite is not applied.

``NonfiniteGuard`` owns the device buffers of the decision: ``verdict`` (int32[4]: any bad value, how many, the first segment that
held one, 0) written once per half step by ``judge``, and the persistent ``counters`` (int32[4]: half steps skipped in total, the
current run of skipped ones, the longest run, padding) that travel in the checkpoint.  On ``HipOps`` ``judge`` is
``xmc_nonfinite_verdict`` (two launches, no host read: a captured step replays it) and ``commit`` is ``xmc_commit_if``.  Nothing here
reads the verdict on the host -- ``read`` (the training loop, at a logging boundary) is the only synchronisation.

With data-parallel replicas (``judge(..., replicas=)``) the scan writes a local verdict, the ranks' verdicts are
all-gathered and ``merge_rows`` -- the specification of ``xmc_verdict_merge`` -- turns the same rows into the same verdict and the
same counters on every rank."""
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


def advance_counters(counters, bad):
    """the persistent counters behind a verdict (the rule of ``xmc_nonfinite_verdict``): [0] += 1 and [1] += 1 (saturating) and
    [2] = max([2], [1]) on a bad one, [1] = 0 on a clean one; [3] is not touched.  -> a new list of four ints"""
    c = [int(v) for v in counters]
    if bad:
        c[0] = min(c[0] + 1, _INT32_MAX)
        c[1] = min(c[1] + 1, _INT32_MAX)
        c[2] = max(c[2], c[1])
    else:
        c[1] = 0
    return c


def merge_rows(rows, counters):
    """The specification of ``xmc_verdict_merge``: ``rows`` is int32 (w, 4), the LOCAL verdicts of all w ranks in rank order.
    -> (verdict, counters), lists of four ints.  With r* the lowest rank whose ``rows[r][0] != 0``: verdict = [is there an r*,
    the saturating sum of ``rows[r][1]``, ``rows[r*][2]`` or -1, r* or 0]; the counters advance from the merged verdict[0]
    (``advance_counters``).  Integers only: every rank computes the same bits from the same rows."""
    import numpy as np
    rows = np.asarray(rows, np.int32)
    if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] != 4:
        raise ValueError(f"nonfinite_guard.merge_rows: rows must be (w, 4) with w >= 1, got {rows.shape}")
    bad = [r for r in range(rows.shape[0]) if rows[r, 0] != 0]
    total = min(int(rows[:, 1].astype(np.int64).sum()), _INT32_MAX)
    verdict = [1, total, int(rows[bad[0], 2]), bad[0]] if bad else [0, total, -1, 0]
    return verdict, advance_counters(counters, bool(bad))


class NonfiniteGuard:
    def __init__(self, device):
        self.verdict = torch.zeros((4,), dtype=torch.int32, device=device)
        self.counters = torch.zeros((4,), dtype=torch.int32, device=device)
        self._ws = torch.zeros((_WS_BYTES,), dtype=torch.uint8, device=device)
        # replicas only: this rank's verdict row and the scratch counters its scan advances (never read)
        self._local = torch.zeros((2, 4), dtype=torch.int32, device=device)

    # ------------------------------------------------------------------------------------------------ device side
    def judge(self, ops, segments, replicas=None):
        """one verdict over the flat float32 tensors ``segments`` (everything the half step is about to commit) -> ``verdict``.
        ``replicas`` (the step's ``dp.GradSync``, exclusive schedule): the scan writes a LOCAL verdict (and scratch counters),
        the ranks' rows are all-gathered, and the merge writes ``verdict`` and the persistent ``counters`` -- the same on
        every rank, so that all of them apply the half step or none does"""
        segments = [t.reshape(-1) for t in segments]
        if not 1 <= len(segments) <= MAX_SEGMENTS:
            raise ValueError(f"NonfiniteGuard.judge takes 1 to {MAX_SEGMENTS} segments")
        for t in segments:
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError("NonfiniteGuard.judge scans contiguous float32 buffers")
        if replicas is None:
            return self._scan(ops, segments, self.verdict, self.counters)
        rows = replicas.gather_rows(self._scan(ops, segments, self._local[0], self._local[1]))
        ops.verdict_merge(rows, self.verdict, self.counters)
        return self.verdict

    def _scan(self, ops, segments, verdict, counters):
        """``xmc_nonfinite_verdict`` over ``segments`` into ``verdict`` / ``counters`` (int32[4] each) -> ``verdict``"""
        if ops.nonfinite_verdict_ws_bytes([t.numel() for t in segments]) > self._ws.numel():
            raise ValueError("NonfiniteGuard: the verdict's workspace is too small")
        ops.nonfinite_verdict(segments, verdict, counters, self._ws)
        return verdict

    def commit(self, ops, dst, src):
        """dst = src unless the verdict is bad"""
        if dst.data_ptr() == src.data_ptr():
            return dst
        return ops.commit_if(dst, src.contiguous(), self.verdict)

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
