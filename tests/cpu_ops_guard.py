"""The mock operator table (tests/cpu_ops.py) with the device-decided entry points of config.skip_nonfinite_updates restated in
torch -- ``xmc_metrics_accum(_if)`` and ``xmc_adam_ema_dev(_guarded)`` with its device-side step counter, and
``xmc_nonfinite_verdict`` by the kernel's bit mask -- so that the DEVICE-decided path of the host logic (guarded launches that read
the verdict themselves, Adam's t in ``ParamArena.step_state``, ``sync_opt_step``) runs on the host.  The plain ``CpuOps`` has the
verdict by ``torch.isfinite`` and ``commit_if`` only: with it ``_apply_adam`` reads the verdict on the host.  Also the helpers the
guard tests share."""
import numpy as np
import torch

from tests.cpu_ops import CpuOps
from xmcgan_image_generation_amd import synthetic as syn


class CpuOpsGuard(CpuOps):
    name = "cpu-mock-guard"

    def nonfinite_verdict(self, segments, verdict, counters, ws):
        bits = [t.reshape(-1).view(torch.int32) for t in segments]
        bad = [int(((b & 0x7f800000) == 0x7f800000).sum()) for b in bits]
        total = sum(bad)
        first = next((i for i, k in enumerate(bad) if k), -1)
        verdict.copy_(torch.tensor([int(total > 0), min(total, 2 ** 31 - 1), first, 0], dtype=torch.int32))
        c = counters.tolist()
        if total:
            c[0], c[1] = c[0] + 1, c[1] + 1
            c[2] = max(c[2], c[1])
        else:
            c[1] = 0
        counters.copy_(torch.tensor(c, dtype=torch.int32))

    def metrics_accum(self, vals, sums, info):
        v = torch.cat([t.reshape(-1) for t in vals])
        for i in range(v.numel()):
            sums[i] += v[i].double()
        info[0] += 1
        if not bool(torch.isfinite(v).all()) and int(info[1]) == 0:
            info[1] = info[0]

    def metrics_accum_if(self, vals, sums, info, verdict):
        if int(verdict[0]) == 0:
            self.metrics_accum(vals, sums, info)

    def adam_ema_dev(self, p, g, m, v, ema, step_state, *, lr, beta1, beta2, eps=1e-8, grad_scale=1.0, ema_decay=0.0, verdict=None):
        if verdict is not None and int(verdict[0]) != 0:
            return                                   # p, m, v, ema and the counter stay as they are
        t = int(step_state.view(torch.int32)[0]) + 1
        step_state.view(torch.int32)[0] = t
        self.adam_ema(p, g, m, v, ema, lr=lr, beta1=beta1, beta2=beta2, step=t, eps=eps, grad_scale=grad_scale, ema_decay=ema_decay)


# ------------------------------------------------------------------------------------------------ helpers of the guard tests
def poison(batch, cfg, halves, how="z"):
    """a copy of ``batch`` with one bad VALUE in the rows of the given half steps (0 = train_d, 1 = train_g_d at
    d_step_per_g_step = 2): ``how`` = "z" puts a NaN into z[row, 0], "image" a +inf into one pixel"""
    out = {k: torch.as_tensor(v).clone() for k, v in batch.items()}
    rows = out["z"].shape[0] // cfg.d_step_per_g_step
    for h in halves:
        if how == "z":
            out["z"][h * rows, 0] = float("nan")
        else:
            out["image"][h * rows, 1, 2, 0] = float("inf")
    return out


def leaves(state):
    """every persistent leaf of a TrainState as host int32 bit patterns (bit-equality also holds NaN to NaN)"""
    ga, da = state.g_optimizer.arena, state.d_optimizer.arena
    ga.sync_opt_step()
    da.sync_opt_step()
    out = {"g/params": ga.params, "g/m": ga.m, "g/v": ga.v, "d/params": da.params, "d/m": da.m, "d/v": da.v, "ema": state.ema_buffer}
    for name, tree in (("bn", state.generator_state["batch_stats"]), ("sn", state.discriminator_state["spectral_norm_stats"])):
        for path, t in syn.tree_leaves(tree):
            out[f"{name}/{path}"] = t
    out = {k: t.detach().float().cpu().contiguous().view(torch.int32).numpy().copy() for k, t in out.items()}
    out["g/t"] = np.asarray(ga.opt_step)
    out["d/t"] = np.asarray(da.opt_step)
    return out


def assert_same(got, want, skip=()):
    assert sorted(got) == sorted(want)
    for k in want:
        if k not in skip:
            assert np.array_equal(got[k], want[k]), k


def counters(state):
    return state.guard.counters.cpu().tolist()[:3]
