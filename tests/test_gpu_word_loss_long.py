"""word_loss at Localized Narratives' caption length: the fused kernels (csrc/word_loss_fused.hip) and the GEMM + column-kernel
chain (``wl_*`` of csrc/losses.hip) at T = 64 and T = 33 against the float64 specification, forward and gradient, with the gates
of tests/test_gpu_word_loss_fused.py.  B * T = 192 and 512 are whole 64-column tiles; 3 * 33 = 99 leaves the second tile ragged and
puts caption boundaries inside a tile.  max_len covers 1, T and both sides of 32."""
import numpy as np
import pytest
import torch

from tests.test_gpu_word_loss_fused import WL_GRAD_TOL, _case, _ops

pytestmark = pytest.mark.gpu

CASES = [(3, 64, [64, 1, 33]), (3, 33, [33, 1, 32]), (8, 64, [64, 1, 33, 32, 47, 2, 17, 60])]


@pytest.mark.parametrize("b,t,max_len", CASES, ids=[f"{b}-{t}" for b, t, _ in CASES])
def test_word_loss_long_vs_spec(b, t, max_len):
    from oracle import np_spec as S
    from oracle import torch_ref as R
    from xmcgan_image_generation_amd.libml import attention_lib as A
    ops = _ops()
    r, e = 256, 768
    feat, words = _case(b, r, t, e, 131 + b + t)
    ml = torch.tensor(max_len, dtype=torch.float32).view(b, 1)
    wn = A.normalize_words(ops, words.cuda())

    def run(fused):
        ops.wl_fused = fused
        loss = torch.zeros(1, device="cuda")
        stats = torch.zeros(2, device="cuda")
        tape = A.word_loss_fwd(ops, feat.cuda(), wn, ml.cuda(), loss, stats=stats)
        assert bool(tape.get("fused")) == fused
        dx = A.word_loss_bwd(ops, tape)
        return float(loss), tape["sim_t"].double().cpu(), dx.double().cpu()

    loss_f, sim_f, dx_f = run(True)
    loss_g, sim_g, dx_g = run(False)
    ref_loss, _, _, ref_sims = S.word_loss(feat.double().numpy(), words.double().numpy(), ml.double().numpy(), return_logits=True)
    x = feat.double().clone().requires_grad_(True)
    l_ref, _ = R.word_loss(x, words.double(), ml.double())
    (gref,) = torch.autograd.grad(l_ref, x)
    err_f = float((dx_f - gref).norm() / gref.norm())
    err_g = float((dx_g - gref).norm() / gref.norm())
    for name, sim, loss in (("fused", sim_f, loss_f), ("GEMM path", sim_g, loss_g)):
        serr = np.abs(sim.numpy().T - ref_sims).max() / np.abs(ref_sims).max()
        print(f"word_loss {name} B={b} T={t}: loss {loss:.6f} vs float64 {ref_loss:.6f}; similarities max err / max {serr:.2e}")
        assert serr <= 2e-2, (name, serr)
        assert abs(loss - ref_loss) <= 2e-2 * max(1.0, abs(ref_loss)), (name, loss, ref_loss)
    print(f"word_loss B={b} T={t}: gradient norm-relative fused {err_f:.2e}, GEMM path {err_g:.2e}")
    assert err_f <= WL_GRAD_TOL, (err_f, err_g)
    assert err_g <= WL_GRAD_TOL, (err_f, err_g)
    assert err_f <= 1.5 * err_g + 5e-3, (err_f, err_g)            # no worse than the path it replaces
    assert abs(loss_f - loss_g) <= 5e-3 * max(1.0, abs(loss_g))
    assert float((sim_f - sim_g).abs().max()) <= 1e-2 * float(sim_g.abs().max())
