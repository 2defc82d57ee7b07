"""attention_for_g on the matrix cores for 32 < T <= 64 (attn_mfma.hip, the two-word-block kernels; Localized Narratives'
64-token captions) against the oracle, with the bars of ``test_gpu_kernels.test_attention_for_g_on_mfma``:

(a) the float64 oracle on the SAME bf16-rounded words within the bf16 tolerance (``_close``): probabilities, context, gradient;
(b) probabilities < 4e-2 from the oracle on the exact words; argmax agreement with the VALU kernel > 0.97;
(c) the backward within 3e-2 (norm-relative) of the VALU kernel.

What (b) leaves to the reference alone, on the CPU at (3, 256, 64, 768): the oracle on bf16-rounded words is 2.0e-4 in
probability from the exact-word oracle and agrees in 0.9987 of the argmax positions.  max_len covers both ends, the word-block
boundary (32, 33) and a length inside the second block; T = 33 and 48 leave the second block partly / half padded."""
import pytest
import torch

from tests.test_gpu_kernels import _close, _ops, _rnd

pytestmark = pytest.mark.gpu

MAX_LEN = [64.0, 33.0, 32.0, 1.0, 47.0]
CASES = [(5, 256, 64, 768), (2, 128, 33, 768), (3, 256, 48, 768), (2, 128, 64, 128)]
BF16 = torch.bfloat16


def _inputs(b, r, t, e):
    ops = _ops(BF16)
    g = torch.Generator().manual_seed(164 + r + t)
    region, rr = _rnd((b, r, e), BF16, g)
    words = torch.randn((b, t, e), generator=g)
    max_len = torch.tensor(MAX_LEN[:b]).clamp(max=float(t)).view(b, 1)
    wn, _ = ops.l2norm_fwd(words.reshape(b * t, e).cuda())
    return ops, g, region, rr, words, max_len, wn.view(b, t, e)


def run_case(b, r, t, e):
    from oracle import torch_ref as R
    ops, g, region, rr, words, max_len, wn = _inputs(b, r, t, e)
    assert ops._attn_mfma(region, b, r, t, e), "the long MFMA kernel must be what runs"
    ml = max_len.cuda().view(-1)
    ctx, attn, rinv = ops.attn_g_fwd(region, wn, ml, 15.0)
    ops.attn_mfma = False
    ctx_v, attn_v, rinv_v = ops.attn_g_fwd(region, wn, ml, 15.0)
    ops.attn_mfma = True
    mask = (torch.arange(t, dtype=torch.float64)[None, :] >= max_len.double()).double()[:, None, :].expand(-1, r, -1)

    def oracle(words_hat):
        rq = rr.clone().requires_grad_(True)
        c, a = R.attention_for_g(rq, words_hat, 15.0, mask)
        return rq, c, a
    rq, ctx_ref, attn_ref = oracle(wn.bfloat16().double().cpu())          # what the kernel multiplies
    _close(rinv, 1.0 / rr.norm(dim=-1), torch.float32, "rinv", scale=float((1.0 / rr.norm(dim=-1)).max()))
    _close(attn, attn_ref, BF16, "attn probs (bf16 words)", scale=1.0)
    _close(ctx, ctx_ref, BF16, "attn ctx (bf16 words)")
    masked = mask.bool().cuda()
    assert not attn[masked].any(), "a word at or beyond max_len has probability exactly 0"
    _, _, attn_x = oracle(words.double())
    perr = float((attn.double().cpu() - attn_x.detach()).abs().max())
    agree = float((attn.argmax(-1) == attn_v.argmax(-1)).float().mean())
    print(f"long MFMA attention {(b, r, t, e)}: probs vs exact-word oracle {perr:.3e}, argmax agreement with VALU {agree:.4f}")
    assert perr < 4e-2 and agree > 0.97, (perr, agree)
    dctx, dcr = _rnd((b, r, e), BF16, g)
    dreg = ops.attn_g_bwd(dctx, region, wn, attn, rinv, 15.0)
    (ref,) = torch.autograd.grad(ctx_ref, rq, dcr)
    _close(dreg, ref, BF16, "attn bwd (bf16 words)", scale=2.0 * float(ref.abs().max()))
    ops.attn_mfma = False
    dreg_v = ops.attn_g_bwd(dctx, region, wn, attn_v, rinv_v, 15.0)
    rel = float((dreg.float() - dreg_v.float()).norm() / dreg_v.float().norm())
    print(f"long MFMA attention backward {(b, r, t, e)} vs VALU kernel: norm-relative difference {rel:.3e}")
    assert rel < 3e-2, rel


@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_attention_for_g_long_on_mfma(case):
    run_case(*case)


def run_sliced(b, r, t, e):
    """the row-pitch forms: ctx written into / dctx read from a column slice of a wider tensor -- bit-equal to the dense forms,
    and no element outside the slice changes"""
    ops, g, region, _, _, max_len, wn = _inputs(b, r, t, e)
    ml = max_len.cuda().view(-1)
    assert ops.attn_g_sliced(region, t)
    ctx, attn, rinv = ops.attn_g_fwd(region, wn, ml, 15.0)
    lo, wide = 64, 64 + e + 136
    sentinel = (torch.randn((b, r, wide), generator=g) * 3).to(BF16).cuda()
    full = sentinel.clone()
    ctx_s, attn_s, rinv_s = ops.attn_g_fwd(region, wn, ml, 15.0, ctx_out=full[:, :, lo:lo + e])
    assert torch.equal(full[:, :, lo:lo + e], ctx) and torch.equal(attn_s, attn) and torch.equal(rinv_s, rinv)
    assert torch.equal(full[:, :, :lo], sentinel[:, :, :lo]) and torch.equal(full[:, :, lo + e:], sentinel[:, :, lo + e:])
    dfull = (torch.randn((b, r, wide), generator=g)).to(BF16).cuda()
    dslice = dfull[:, :, lo:lo + e]
    dreg_s = ops.attn_g_bwd(dslice, region, wn, attn, rinv, 15.0)
    dreg = ops.attn_g_bwd(dslice.contiguous(), region, wn, attn, rinv, 15.0)
    assert torch.equal(dreg_s, dreg)


@pytest.mark.parametrize("case", [(2, 128, 33, 768), (2, 128, 64, 128)], ids=["2-128-33-768", "2-128-64-128"])
def test_sliced_context_forms(case):
    run_sliced(*case)


def test_supported_domain():
    lib = _ops(BF16).lib
    assert lib.xmc_attn_g_mfma_supported(3, 256, 64, 768) == 1
    assert lib.xmc_attn_g_mfma_supported(3, 256, 33, 768) == 1 and lib.xmc_attn_g_mfma_supported(3, 256, 17, 768) == 1
    assert lib.xmc_attn_g_mfma_supported(3, 256, 65, 768) == 0 and lib.xmc_attn_g_mfma_supported(3, 192, 64, 768) == 0
    assert lib.xmc_attn_g_mfma_supported(3, 256, 64, 1152) == 0          # 144 e bytes of LDS would pass 160 KiB
