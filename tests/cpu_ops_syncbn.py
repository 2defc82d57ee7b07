"""The mock operator table (tests/cpu_ops.py) with the group-aware BatchNorm methods of ops.py: bn_batch_sums,
bn_finalize_rows, rows_mean and the ``reduce_s`` hook of cbn_act_bwd (cross-replica BatchNorm groups,
config.batch_norm_group_size > 0)."""
import torch

from tests.cpu_ops import CpuOps


class CpuOpsSyncBN(CpuOps):
    name = "cpu-mock-syncbn"

    def bn_batch_sums(self, x):
        return self.bn_stats(x)

    def bn_finalize_rows(self, rows, pixels_per_row, run_mean, run_var, update, eps=1e-5, momentum=0.9):
        total = rows[0].clone()
        for r in range(1, rows.shape[0]):        # index order, as the kernel
            total = total + rows[r]
        return self.bn_finalize(total, rows.shape[0] * pixels_per_row, run_mean, run_var, update, eps, momentum)

    def rows_mean(self, rows):
        total = rows[0].clone()
        for r in range(1, rows.shape[0]):
            total = total + rows[r]
        return total / rows.shape[0]

    def cbn_act_bwd(self, dy, x, mean, rstd, gb, hc, relu=True, dgb_out=None, reduce_s=None):
        if reduce_s is None:
            return super().cbn_act_bwd(dy, x, mean, rstd, gb, hc, relu, dgb_out)
        n, h, w, c = x.shape
        f = h // hc
        g2 = gb.reshape(-1, 2 * c)
        gamma, beta = g2[:, :c], g2[:, c:]
        a = self._up(gamma, n, hc, h, c) + 1
        xh = (x - mean) * rstd
        u = xh * a + self._up(beta, n, hc, h, c)
        g = torch.where(u > 0, dy, torch.zeros_like(dy)) if relu else dy
        pool = lambda t: t.view(n, hc, f, hc, f, c).sum((2, 4)).reshape(-1, c)
        dgb = torch.cat([pool(g * xh), pool(g)], dim=1)                  # dgamma | dbeta per cell: local
        if dgb_out is not None:
            dgb_out.reshape(-1, 2 * c).copy_(dgb) if dgb_out.is_contiguous() else dgb_out.copy_(dgb)
            dgb = dgb_out
        else:
            dgb = dgb.reshape(gb.shape).contiguous()
        dxh = g * a
        # s[0:C] = sum (gamma + 1) dbeta, s[C:2C] = sum (gamma + 1) dgamma (xmc_cbn_bwd_sums), exchanged, / LOCAL pixels
        s = reduce_s(torch.cat([dxh.sum((0, 1, 2)), (dxh * xh).sum((0, 1, 2))]).contiguous())
        p = n * h * w
        dx = rstd * (dxh - s[:c] / p - xh * s[c:] / p)
        return dx.contiguous(), dgb
