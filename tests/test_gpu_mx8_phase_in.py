"""The "in" phase form of the MX-fp8 mode (``ops.fp8_phase_in_mx`` / ``config.conv_fp8_phase_in``) on the MI355X:
avg_pool2(conv3x3(x)) as four 2x2 convolutions on the low-resolution output grid, one per parity of the input pixel, multiplied
by the block-scaled MFMA (conv_phase_in_mx8_kernel) -- against float64 ``F.avg_pool2d(F.conv2d(.))`` on operands whose
quantisation is exact, against the bf16 "in" phase kernel on generic data, through producer packets, split-K, the training
step, its overlapped schedule and hipGraph replay.

Measured on one MI355X (profiles/r08_mx8_phase_in_parity.txt): exact operands 5.9e-8 .. 3.8e-7 of the magnitude (gate 2e-4),
device-quantised Gaussian activations 7.2e-7 .. 2.6e-5; against the bf16 "in" phase kernel 3.75e-2 forward, 2.75e-2 with
relu_in, 3.76e-2 at 1e-4-sized gradients (gate 6e-2); 12 launches of the kernel in one C1 step (8 forward, 4 data gradient)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_mx8 import e4m3_decode_table, lossless_mx
from tests.test_gpu_mx8_phase import RND, bits_of, exact_master

pytestmark = pytest.mark.gpu


def _ops(phase_in_mx=True, phase_mx=False):
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=torch.bfloat16)
    ops.fp8 = True
    ops.fp8_phase_mx = phase_mx
    ops.fp8_phase_in_mx = phase_in_mx
    return ops


# rows (columns) of the 3x3 kernel summed by (parity a of the input pixel, window position tu):
#   avg_pool2(conv3x3(x))[i] = 1/4 sum_a sum_tu F_a[tu] x[2 (i - a + tu) + a]
IN_SETS = {(0, 0): (1, 0), (0, 1): (2,), (1, 0): (0,), (1, 1): (2, 1)}


def in_taps(w):
    """(rows, 9, k) float64 launch weight -> (rows, 16, k) "in"-form tap sums, tap = (2a + b) * 4 + tu * 2 + tv"""
    w9 = w.reshape(w.shape[0], 3, 3, w.shape[2])
    out = np.zeros((w.shape[0], 16, w.shape[2]))
    for a in range(2):
        for b in range(2):
            for tu in range(2):
                for tv in range(2):
                    t = (2 * a + b) * 4 + tu * 2 + tv
                    for dy in IN_SETS[(a, tu)]:
                        for dx in IN_SETS[(b, tv)]:
                            out[:, t] += w9[:, dy, dx]
    return out


def in_form_by_parity(x, f16):
    """the identity the kernel computes, literally: x (n, 2h, 2w, c) float64, f16 (rows, 16, c) = in_taps(w) -> (n, h, w, rows).
    Parity (a, b) of the input is a 2x2 convolution on x[a::2, b::2] with window origin (i - a, j - b); outside the map = 0."""
    n, hh, ww, c = x.shape
    h, w = hh // 2, ww // 2
    out = torch.zeros((n, h, w, f16.shape[0]), dtype=torch.float64)
    f = torch.from_numpy(f16)
    for a in range(2):
        for b in range(2):
            sub = x[:, a::2, b::2]                                    # sub[u][v] = x[2u + a][2v + b]
            # window origin (i - a, j - b): pad one row / column in front for parity 1, behind for parity 0
            sp = F.pad(sub, (0, 0, b, 1 - b, a, 1 - a))               # sp[u'][v'] = sub[u' - a][v' - b]
            for tu in range(2):
                for tv in range(2):
                    t = (2 * a + b) * 4 + tu * 2 + tv
                    out += sp[:, tu:tu + h, tv:tv + w] @ f[:, t].T
    return out / 4


def assert_in_fixture_is_lossless(wl):
    """CPU emulation of the weight path: the "in"-form tap sums are exact in bf16, and exact in e4m3 under BOTH scale rules
    (mx_scale_byte + pack_fp8x4 of csrc/conv_stream_mx8.hip).  Returns the largest quantised magnitude."""
    f16 = in_taps(wl)
    t = torch.from_numpy(f16).float()
    assert torch.equal(t.bfloat16().float().double(), torch.from_numpy(f16)), "tap sums not exact in bf16"
    rows, _, k = f16.shape
    blocks = f16.reshape(rows, 16, k // 32, 32)
    amax = np.abs(blocks).max(-1).astype(np.float32)
    codes = np.unique(np.abs(e4m3_decode_table()[:0x7F]))
    qmax = 0.0
    for rnd in RND.values():
        sb = ((((amax.view(np.uint32).astype(np.int64) + rnd) >> 23) & 0xFF) - 8).clip(0, None)
        q = np.abs(blocks) * 2.0 ** (127.0 - sb)[..., None]
        q = np.where(amax[..., None] > 0, q, 0.0)
        assert q.max() <= 448.0
        qmax = max(qmax, float(q.max()))
        err = np.abs(q[..., None] - codes).min(-1).max()
        assert err == 0.0, ("weight fixture is not exact in e4m3", err)
    return qmax


def ref_pooled(x64, w9, bands):
    """float64 avg_pool2(conv3x3 SAME (x)) of ``x64`` (n, H, W, c) with ``w9`` (rows, 9, c) on the OUTPUT row ranges ``bands``
    (None: all rows) -> list of (r0, r1, (n, r1 - r0, W / 2, rows))"""
    rows, _, c = w9.shape
    wt = torch.from_numpy(w9).reshape(rows, 3, 3, c).permute(0, 3, 1, 2).contiguous()
    H = x64.shape[1]
    xp = F.pad(x64.permute(0, 3, 1, 2), (1, 1, 1, 1))
    out = []
    for r0, r1 in (bands if bands is not None else [(0, H // 2)]):
        out.append((r0, r1, F.avg_pool2d(F.conv2d(xp[:, :, 2 * r0:2 * r1 + 2], wt), 2).permute(0, 2, 3, 1)))
    return out


def check_against_float64(tag, y, x64, wl, bands, alpha=1.0, bias=None, res=None, res_scale=1.0):
    """the project's gate for this instruction and accumulator: max |got - ref| / (conv(|x|, |w|) + |ref|) < 2e-4"""
    got = y.double().cpu()
    worst = 0.0
    for (r0, r1, ref), (_, _, mag) in zip(ref_pooled(x64, wl, bands), ref_pooled(x64.abs(), np.abs(wl), bands)):
        ref = ref * alpha
        if bias is not None:
            ref = ref + bias.double().cpu()
        if res is not None:
            ref = ref + res_scale * res.double().cpu()[:, r0:r1]
        mag = mag * abs(alpha) + ref.abs()
        worst = max(worst, float(((got[:, r0:r1] - ref).abs() / mag.clamp_min(1e-30)).max()))
    print("conv_phase_in_mx8", tag, "max |error| / magnitude:", worst)
    assert worst < 2e-4, (tag, worst)
    return worst


def _desc(ops, n, hin, k, rows):
    from xmcgan_image_generation_amd._lib import XMC_CONV_PACKED, XMC_CONV_PHASE, ConvDesc
    return ConvDesc(n, hin, hin, k, rows, 3, 0, 0, 0, 0, ops.code, 1.0, 1.0, XMC_CONV_PACKED | XMC_CONV_PHASE, 1, 0, 0, 0, 0, None)


# OUTPUT grid, n, reduction length K, rows, form, split-K, options.  Images per tile: 16 at 4^2, 4 at 8^2, 1 from 16^2 on.
# The float64 reference of the largest grid covers bands of output rows (map edges, tile seams, the middle).
# Every case runs its launch with float32 output (gated against float64) AND with bf16 output (= that result rounded).
CASES = [
    (4, 17, 1536, 128, "d", True, {}),
    (4, 3, 1024, 96, "g", False, {}),
    (4, 21, 1536, 192, "g", True, {}),
    (8, 3, 1024, 256, "d", False, {}),
    (8, 5, 1536, 96, "g", True, {}),
    (8, 6, 768, 320, "d", True, {}),
    (16, 2, 192, 96, "g", False, {}),
    (16, 3, 384, 256, "d", False, {}),
    (16, 2, 384, 320, "d", False, {}),
    (32, 1, 384, 96, "g", False, {}),
    (32, 1, 192, 192, "d", False, {}),
    (64, 1, 192, 96, "g", False, dict(bands=[(0, 5), (29, 35), (59, 64)])),
]


def run_case(ops, xb, h, n, k, rows, form, opts, gen, tgen):
    """one launch of the discriminator-forward form (forward weight of an avg_pool2(conv3x3(.)) layer: bias, shortcut at
    res_scale, device alpha, relu_in, (y > 0) bits and packets for the next convolution) or of the generator-dgrad form
    (data-gradient weight of a conv3x3(upsample2(.)) layer: alpha = 4, no bias)"""
    master, wl = exact_master(rows, k, gen, "fwd" if form == "d" else "dgrad")
    assert_in_fixture_is_lossless(wl)
    wf, wd = ops.prep_conv_weight(torch.from_numpy(master).cuda(), None, True, phase="pool" if form == "d" else "ups")
    w = wf if form == "d" else wd
    assert w.phase is not None and w.phase[0] == "in" and w.phase_mx8 is not None
    assert ops.can_pool_out(xb, w)
    if form == "d":
        bias = torch.randn(rows, generator=tgen).cuda()
        res = torch.randn((n, h, h, rows), generator=tgen).bfloat16().cuda()
        alpha_dev = torch.full((1,), 0.75, device="cuda")
        kw = dict(res=res, res_scale=0.5, alpha_dev=alpha_dev, relu_in=True)
        ref_kw = dict(alpha=0.75, bias=bias, res=res, res_scale=0.5)
    else:
        bias = None
        kw = dict(alpha=4.0)
        ref_kw = dict(alpha=4.0)
    y = ops.conv(xb, w, bias, ks=3, pool_out=True, out_f32=True, **kw)
    assert ops.last_conv_mx8_phase_in and ops.last_conv_phase and not ops.last_conv_mx8_phase
    assert y.dtype == torch.float32 and tuple(y.shape) == (n, h, h, rows)
    # bf16 out: the same accumulators through the same epilogue, rounded once on the store
    yb = ops.conv(xb, w, bias, ks=3, pool_out=True, emit_bits=True, emit_mx8=True, **kw)
    assert ops.last_conv_mx8_phase_in and yb.dtype == torch.bfloat16
    assert torch.equal(yb, y.bfloat16())
    if not ops.lib.xmc_conv2d_mx8_phase_in_workspace_bytes(C.byref(_desc(ops, n, 2 * h, k, rows))) or ops.no_split_k:
        assert torch.equal(yb.bits.to(torch.int32) & 0xFFFF, bits_of(yb))          # (y > 0) as bits: launches without split-K
    return y, wl, ref_kw


@pytest.mark.parametrize("h,n,k,rows,form,split_k,opts", CASES)
def test_conv_phase_in_mx8_exact_on_lossless_operands(h, n, k, rows, form, split_k, opts):
    """Activations and tap sums whose MX quantisation is exact: the launch must equal float64 avg_pool2(conv3x3(x)) with the
    epilogue applied in float64, up to float32 accumulation -- tap sets, per-parity patch origin and stride-2 gather, halo,
    both operands' block scales, split-K and every epilogue option of the two call sites."""
    ops = _ops()
    ops.no_split_k = not split_k
    gen = np.random.default_rng(h * 1000 + k + rows)
    tgen = torch.Generator().manual_seed(h + rows)
    x = torch.from_numpy(lossless_mx((n, 2 * h, 2 * h, k // 32), gen))
    xb = x.bfloat16()
    assert torch.equal(xb.float(), x)
    d = _desc(ops, n, 2 * h, k, rows)
    assert ops.lib.xmc_conv2d_mx8_phase_in_supported(C.byref(d)) == 1
    assert not split_k or ops.lib.xmc_conv2d_mx8_phase_in_workspace_bytes(C.byref(d)) > 0, "the case does not exercise what it names"
    y, wl, ref_kw = run_case(ops, xb.cuda(), h, n, k, rows, form, opts, gen, tgen)
    x64 = x.double().clamp_min(0) if form == "d" else x.double()               # relu_in of the forward site
    check_against_float64((h, n, k, rows, form, split_k, opts), y, x64, wl, opts.get("bands"), **ref_kw)


@pytest.mark.parametrize("scale", [1.0, 1e-4])
def test_conv_phase_in_mx8_generic_activations_exact_weights(scale):
    """Gaussian bf16 activations (and gradient-sized ones), quantised by the device; the reference runs on the DECODED packets,
    so only the kernel's handling of the per-block activation scales in its patch is under test.  Same gate."""
    ops = _ops()
    gen = np.random.default_rng(7)
    tgen = torch.Generator().manual_seed(7)
    tab = torch.from_numpy(e4m3_decode_table())
    for h, n, k, rows, form in ((16, 2, 192, 96, "d"), (8, 5, 1024, 96, "g")):
        hin = 2 * h
        xb = (torch.randn((n, hin, hin, k), generator=tgen) * scale).bfloat16().cuda()
        relu = form == "d"
        pk = ops.quantize_mx8(xb, relu=relu).cpu().view(n, hin, hin, k // 64, 80)
        el = tab[pk[..., :64].long()].view(n, hin, hin, k // 32, 32)
        sc = torch.exp2(pk[..., 64:66].double() - 127).reshape(n, hin, hin, k // 32, 1)
        xdec = (el * sc).reshape(n, hin, hin, k)
        xref = xb.double().cpu().clamp_min(0) if relu else xb.double().cpu()
        assert float((xdec - xref).norm() / xref.norm()) < 5e-2                      # they ARE the packets of xb
        y, wl, ref_kw = run_case(ops, xb, h, n, k, rows, form, {}, gen, tgen)
        check_against_float64(("decoded", scale, h, n, k, rows, form), y, xdec, wl, None, **ref_kw)


def test_conv_phase_in_mx8_accuracy_on_gaussian_data_vs_bf16_in_phase_kernel():
    """Generic data, 192 -> 96 channels at 32^2 -> 16^2 with relu_in (and the data-gradient form at gradient-sized values):
    norm-relative difference of the MX "in" launch to the bf16 "in" phase launch, the gate of
    test_conv_mx8_accuracy_on_gaussian_data_and_dgrad_adjoint (a CPU emulation of this computation gives 3.77e-2 forward,
    2.73e-2 with relu_in, 3.75e-2 at 1e-4)."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    n, h, cin, cout = 4, 16, 192, 96
    x = torch.randn((n, 2 * h, 2 * h, cin), generator=g).bfloat16().cuda()
    w = (torch.randn((cout, 9, cin), generator=g) * 0.03).cuda()
    wf, _ = ops.prep_conv_weight(w, None, True, phase="pool")
    dy = (torch.randn((n, 2 * h, 2 * h, cin), generator=g) * 1e-4).bfloat16().cuda()
    wp = (torch.randn((cin, 9, cout), generator=g) * 0.03).cuda()
    _, wd = ops.prep_conv_weight(wp, None, True, phase="ups")
    for name, t, wt, kw in (("fwd", x, wf, {}), ("fwd relu_in", x, wf, dict(relu_in=True)), ("dgrad", dy, wd, dict(alpha=4.0))):
        assert wt.phase[0] == "in" and wt.phase_mx8 is not None
        y8 = ops.conv(t, wt, None, ks=3, pool_out=True, out_f32=True, **kw)
        assert ops.last_conv_mx8_phase_in
        ops.fp8_phase_in_mx = False
        y16 = ops.conv(t, wt, None, ks=3, pool_out=True, out_f32=True, **kw)
        assert ops.last_conv_phase and not ops.last_conv_mx8_phase_in
        ops.fp8_phase_in_mx = True
        rel = float((y8 - y16).norm() / y16.norm())
        print(f"MX-fp8 in-phase vs bf16 in-phase {name}: norm-relative difference {rel:.3e}")
        assert rel < 6e-2, (name, rel)


def test_conv_phase_in_mx8_takes_producer_packets():
    """packets written by an MX convolution's epilogue (``emit_mx8``, ReLU-stored and not) serve the launch: same bytes as the
    launch that quantises a packet-less clone itself; its own ``emit_mx8`` packets equal the pass's."""
    ops = _ops()
    ops.no_split_k = True
    g = torch.Generator().manual_seed(3)
    n, h, c, rows = 3, 16, 192, 128
    w = (torch.randn((rows, 9, c), generator=g) * 0.03).cuda()
    wf, _ = ops.prep_conv_weight(w, None, True, phase="pool")
    bias = torch.randn(rows, generator=g).cuda()
    x = torch.randn((n, 2 * h, 2 * h, c), generator=g).bfloat16().cuda()
    w0 = (torch.randn((c, 9, c), generator=g) * 0.03).cuda()
    wf0, _ = ops.prep_conv_weight(w0, None, False)
    a_plain = ops.conv(x, wf0, None, ks=3, emit_mx8=True)                    # packets with the consumer's ReLU folded in
    assert a_plain.mx8 is not None and a_plain.mx8[1] is True
    a_relu = ops.conv(x, wf0, None, ks=3, relu_out=True, emit_mx8=True)      # stored after its ReLU: tag "relu"
    assert a_relu.mx8 is not None and a_relu.mx8[1] == "relu"
    for a in (a_plain, a_relu):
        y1 = ops.conv(a, wf, bias, ks=3, pool_out=True, relu_in=True, emit_mx8=True)
        assert ops.last_conv_mx8_phase_in
        y2 = ops.conv(a.clone(), wf, bias, ks=3, pool_out=True, relu_in=True)
        assert ops.last_conv_mx8_phase_in
        assert torch.equal(y1, y2)
        assert y1.mx8 is not None and y1.mx8[1] is True
        assert torch.equal(y1.mx8[0][:, :, :66], ops.quantize_mx8(y1, relu=True)[:, :, :66])


@pytest.mark.parametrize("split_k", [False, True])
def test_conv_phase_in_mx8_is_deterministic(split_k):
    """no float atomics: each split writes its own float32 slice and a finishing pass adds them in a fixed order"""
    ops = _ops()
    ops.no_split_k = not split_k
    g = torch.Generator().manual_seed(9)
    n, h, c, rows = 7, 8, 1536, 192
    x = torch.randn((n, 2 * h, 2 * h, c), generator=g).bfloat16().cuda()
    wf, _ = ops.prep_conv_weight((torch.randn((rows, 9, c), generator=g) * 0.02).cuda(), None, True, phase="pool")
    assert ops.lib.xmc_conv2d_mx8_phase_in_workspace_bytes(C.byref(_desc(ops, n, 2 * h, c, rows))) > 0      # (ops.no_split_k lends none)
    a = ops.conv(x, wf, None, ks=3, pool_out=True).clone()
    assert ops.last_conv_mx8_phase_in
    torch.cuda.synchronize()
    b = ops.conv(x, wf, None, ks=3, pool_out=True)
    assert ops.last_conv_mx8_phase_in
    assert torch.equal(a, b)


@pytest.mark.parametrize("phase_mx", [False, True])
def test_nothing_moves_while_the_in_switch_is_off(phase_mx):
    """ops.fp8 + fp8_phase with fp8_phase_in_mx off (and fp8_phase_mx on as well): a ``pool_out`` launch on an "in" site runs the
    bf16 "in" phase kernel, bit for bit the launch of the bf16 mode, sets neither indicator, and the weight gets no twin."""
    ops = _ops(phase_in_mx=False, phase_mx=phase_mx)
    g = torch.Generator().manual_seed(1)
    n, h, c, rows = 2, 16, 192, 128
    x = torch.randn((n, 2 * h, 2 * h, c), generator=g).bfloat16().cuda()
    res = torch.randn((n, h, h, rows), generator=g).bfloat16().cuda()
    wf, wd = ops.prep_conv_weight((torch.randn((rows, 9, c), generator=g) * 0.03).cuda(), None, True, phase="pool")
    assert wf.phase is not None and wf.phase[0] == "in" and wf.phase_mx8 is None
    assert (wd.phase_mx8 is not None) == phase_mx              # the "out" twin belongs to the other switch
    before = ops.mx8_phase_in_launches, ops.mx8_phase_launches
    y8 = ops.conv(x, wf, None, ks=3, pool_out=True, relu_in=True, res=res)
    assert ops.last_conv_phase and not ops.last_conv_mx8_phase and not ops.last_conv_mx8_phase_in
    ops.fp8 = False
    y16 = ops.conv(x, wf, None, ks=3, pool_out=True, relu_in=True, res=res)
    assert ops.last_conv_phase and not ops.last_conv_mx8_phase and not ops.last_conv_mx8_phase_in
    assert torch.equal(y8, y16)
    assert (ops.mx8_phase_in_launches, ops.mx8_phase_launches) == before
    # the domain is the C side's: the stride-2 forms and ups descriptors are outside
    ops.fp8 = True
    d = _desc(ops, n, 2 * h, c, rows)
    assert ops.lib.xmc_conv2d_mx8_phase_in_supported(C.byref(d)) == 1
    assert ops.lib.xmc_conv2d_mx8_phase_supported(C.byref(d)) == 0
    d.ups = 1
    assert ops.lib.xmc_conv2d_mx8_phase_in_supported(C.byref(d)) == 0
    for field in ("relu_in", "relu_out", "res_ups", "mask_after_res", "valid_h", "valid_w"):      # the rest of the stated domain
        d = _desc(ops, n, 2 * h, c, rows)
        setattr(d, field, 1)
        assert ops.lib.xmc_conv2d_mx8_phase_in_supported(C.byref(d)) == 0, field
    d = _desc(ops, n, 2 * h, c, rows)
    d.pool_out = 0
    assert ops.lib.xmc_conv2d_mx8_phase_in_supported(C.byref(d)) == 0
    d = _desc(ops, n, 2 * h, c, 80)
    assert ops.lib.xmc_conv2d_mx8_phase_in_supported(C.byref(d)) == 0          # cout % 32
    d = _desc(ops, n, 2 * h, 96, rows)
    assert ops.lib.xmc_conv2d_mx8_phase_in_supported(C.byref(d)) == 0          # a 96-channel reduction: not whole packets
    d = _desc(ops, n, 4, c, rows)
    assert ops.lib.xmc_conv2d_mx8_phase_in_supported(C.byref(d)) == 0          # 2 x 2 output grid


def _c1_b8_fp8_phase_in_cfg():
    from tests.test_gpu_step import _c1_b8_oracle
    o = _c1_b8_oracle()
    cfg = o["cfg"].copy()
    cfg.dtype = "bfloat16"
    cfg.conv_fp8 = cfg.conv_fp8_phase = cfg.conv_fp8_phase_in = True
    return o, cfg


def test_train_step_conv_fp8_phase_in_vs_fp32_oracle(monkeypatch):
    """config.conv_fp8 + conv_fp8_phase + conv_fp8_phase_in at the C1 network, per-device batch 8, against the float32 oracle with
    exactly the gates of test_train_step_conv_fp8_vs_fp32_oracle (1e-1 of the loss scale on the hinge losses, 1e-2 on the
    contrastive ones, second step finite); D's forward and G's backward both ran ``pool_out`` launches on
    conv_phase_in_mx8_kernel."""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.ops import HipOps
    o, cfg = _c1_b8_fp8_phase_in_cfg()
    seen = {"fwd": 0, "dgrad": 0}
    inner = HipOps.conv

    def counting(self, x, w, bias=None, **kw):
        y = inner(self, x, w, bias, **kw)
        if self.last_conv_mx8_phase_in:
            seen["fwd" if bias is not None else "dgrad"] += 1          # D's forward carries a bias, G's pullback none
            assert kw.get("pool_out") and not kw.get("ups")
        return y
    monkeypatch.setattr(HipOps, "conv", counting)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    ops = gen(train=True).ops
    assert ops.fp8 and ops.fp8_phase and ops.fp8_phase_mx and ops.fp8_phase_in_mx
    state = train_utils.load_flax_params(state, *o["init"])
    tb = {k: torch.as_tensor(v).cuda() for k, v in o["batch"].items()}
    state, m = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {})
    print("conv_phase_in_mx8 launches in one step:", seen, "counter:", ops.mx8_phase_in_launches, "out form:", ops.mx8_phase_launches)
    assert seen["fwd"] >= 1 and seen["dgrad"] >= 1 and ops.mx8_phase_in_launches == seen["fwd"] + seen["dgrad"]
    assert ops.mx8_phase_launches >= 1
    ref = o["ref_metrics"]
    scale = max(abs(float(ref[k])) for k in ("d_loss", "g_loss", "c_loss_d", "c_loss_g"))
    for k in ("d_loss", "g_loss", "c_loss_d", "c_loss_g"):
        r = abs(float(m[k]) - float(ref[k])) / scale
        print("conv_fp8_phase_in C1 b8", k, float(m[k]), float(ref[k]), r)
        assert np.isfinite(float(m[k])) and r < (1e-1 if k in ("d_loss", "g_loss") else 1e-2), (k, float(m[k]), float(ref[k]))
    state, m2 = train_utils.train_step(1, state, tb, xmc_gan, gen, disc, cfg, {})
    assert all(np.isfinite(float(v)) for v in m2.values())
    assert bool(torch.isfinite(state.g_optimizer.arena.params).all()) and bool(torch.isfinite(state.d_optimizer.arena.params).all())


def test_train_step_conv_fp8_phase_in_is_bit_reproducible_and_graph_replay_equals_eager():
    """the default (overlapped two-stream) schedule twice from the same state: bit-identical losses and parameters (the MX twins
    are made on the preparing stream); hipGraph replay of the step equals the eager step bit for bit."""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    o, cfg = _c1_b8_fp8_phase_in_cfg()
    tb = {k: torch.as_tensor(v).cuda() for k, v in o["batch"].items()}
    runs = []
    for mode in ("eager", "eager", "graph"):
        gen, disc, st = train_utils.create_train_state(cfg, 0)
        st = train_utils.load_flax_params(st, *o["init"])
        st, _ = train_utils.train_step(0, st, tb, xmc_gan, gen, disc, cfg, {})
        if mode == "graph":
            graphed = train_utils.GraphedTrainStep(st, tb, xmc_gan, gen, disc, cfg, {})
            st, m = graphed(graphed.state, tb)
        else:
            st, m = train_utils.train_step(1, st, tb, xmc_gan, gen, disc, cfg, {})
        torch.cuda.synchronize()
        assert gen(train=True).ops.mx8_phase_in_launches > 0
        runs.append(({k: float(v) for k, v in m.items()}, st.g_optimizer.arena.params.clone(), st.d_optimizer.arena.params.clone()))
        del st, gen, disc
        torch.cuda.empty_cache()
    for name, r in (("second eager run", runs[1]), ("graph replay", runs[2])):
        assert all(np.isfinite(v) for v in r[0].values())
        assert runs[0][0] == r[0], (name, runs[0][0], r[0])
        assert torch.equal(runs[0][1], r[1]) and torch.equal(runs[0][2], r[2]), name
