"""The "out" phase form of the MX-fp8 mode (``ops.fp8_phase_mx`` / ``config.conv_fp8_phase``) on the MI355X:
conv3x3(nearest_upsample2(x)) as four 2x2 convolutions on the low-resolution grid, multiplied by the block-scaled MFMA
(conv_phase_mx8_kernel) -- against float64 ``F.conv2d`` on operands whose quantisation is exact, against the bf16 phase
kernel on generic data, through producer packets, split-K, the training step, its overlapped schedule and hipGraph replay."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_mx8 import e4m3_decode_table, lossless_mx

pytestmark = pytest.mark.gpu

RND = {"next_binade": 0x1FFFFF, "ocp_floor": 0}          # mx_scale_byte's rounding constant (csrc/common.h)


def _ops(phase_mx=True):
    from xmcgan_image_generation_amd.ops import HipOps
    ops = HipOps(dtype=torch.bfloat16)
    ops.fp8 = True
    ops.fp8_phase_mx = phase_mx
    return ops


def exact_master(rows, k, gen, layout):
    """float32 3x3 master whose 16 "out"-form tap sums quantise EXACTLY: taps = integers in [-3, 3] times 2^e with one e in
    [-12, 3] per (row of the launch's weight, 32-wide block of its reduction axis).  ``layout`` "fwd": master (cout = rows, 9,
    cin = k), the launch reads the forward copy; "dgrad": master (cout = k, 9, cin = rows), the launch reads the data-gradient
    copy (rows = master cin, reduction = master cout)."""
    ints = gen.integers(-3, 4, size=(rows, 9, k)).astype(np.float64)
    e = gen.integers(-12, 4, size=(rows, 1, k // 32, 1))
    w = (ints.reshape(rows, 9, k // 32, 32) * 2.0 ** e).reshape(rows, 9, k)          # the weight AS THE LAUNCH SEES IT
    if layout == "dgrad":                                  # launch weight [ci][tap][co] = master [co][8 - tap][ci]
        return np.ascontiguousarray(w[:, ::-1, :].transpose(2, 1, 0)).astype(np.float32), w
    return w.astype(np.float32), w


def phase_taps(w):
    """(rows, 9, k) float64 launch weight -> (rows, 16, k) "out"-form tap sums, tap = (2a + b) * 4 + tu * 2 + tv"""
    sets = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}              # (phase bit, window position) -> 3x3 rows
    w9 = w.reshape(w.shape[0], 3, 3, w.shape[2])
    out = np.zeros((w.shape[0], 16, w.shape[2]))
    for a in range(2):
        for b in range(2):
            for tu in range(2):
                for tv in range(2):
                    t = (2 * a + b) * 4 + tu * 2 + tv
                    for dy in sets[(a, tu)]:
                        for dx in sets[(b, tv)]:
                            out[:, t] += w9[:, dy, dx]
    return out


def assert_fixture_is_lossless(wl):
    """CPU emulation of the weight path: the tap sums are exact in bf16, and exact in e4m3 under BOTH scale rules
    (mx_scale_byte + pack_fp8x4 of csrc/conv_stream_mx8.hip)."""
    e16 = phase_taps(wl)
    t = torch.from_numpy(e16).float()
    assert torch.equal(t.bfloat16().float().double(), torch.from_numpy(e16)), "tap sums not exact in bf16"
    rows, _, k = e16.shape
    blocks = e16.reshape(rows, 16, k // 32, 32)
    amax = np.abs(blocks).max(-1).astype(np.float32)
    codes = np.unique(np.abs(e4m3_decode_table()[:0x7F]))
    for rnd in RND.values():
        sb = ((((amax.view(np.uint32).astype(np.int64) + rnd) >> 23) & 0xFF) - 8).clip(0, None)
        q = np.abs(blocks) * 2.0 ** (127.0 - sb)[..., None]
        q = np.where(amax[..., None] > 0, q, 0.0)
        assert q.max() <= 448.0
        err = np.abs(q[..., None] - codes).min(-1).max()
        assert err == 0.0, ("weight fixture is not exact in e4m3", err)


def ref_rows(xup, w9, bands):
    """float64 conv3x3 (SAME) of ``xup`` (n, c, H, W) with ``w9`` (rows, 9, c) on the output row ranges ``bands`` (None: all
    rows) -> list of (r0, r1, (n, r1 - r0, W, rows))"""
    rows, _, c = w9.shape
    wt = torch.from_numpy(w9).reshape(rows, 3, 3, c).permute(0, 3, 1, 2).contiguous()
    H = xup.shape[2]
    xp = F.pad(xup, (1, 1, 1, 1))
    out = []
    for r0, r1 in (bands if bands is not None else [(0, H)]):
        out.append((r0, r1, F.conv2d(xp[:, :, r0:r1 + 2], wt).permute(0, 2, 3, 1)))
    return out


def check_against_float64(tag, y, x64, wl, bands, alpha=1.0, bias=None, mask=None):
    """the project's gate for this instruction and accumulator: max |got - ref| / (conv(|x|, |w|) + |ref|) < 2e-4"""
    xup = x64.permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
    got = y.double().cpu()
    worst = 0.0
    for (r0, r1, ref), (_, _, mag) in zip(ref_rows(xup, wl, bands), ref_rows(xup.abs(), np.abs(wl), bands)):
        ref = ref * alpha
        if bias is not None:
            ref = ref + bias.double().cpu()
        if mask is not None:
            ref = ref * (mask.double().cpu()[:, r0:r1] > 0)
        mag = mag * abs(alpha) + ref.abs()
        worst = max(worst, float(((got[:, r0:r1] - ref).abs() / mag.clamp_min(1e-30)).max()))
    print("conv_phase_mx8", tag, "max |error| / magnitude:", worst)
    assert worst < 2e-4, (tag, worst)


def bits_of(t):
    n, h, w, c = t.shape
    return ((t.float() > 0).view(n, h, w, c // 16, 16).to(torch.int32) << torch.arange(16, device=t.device, dtype=torch.int32)).sum(-1)


# low-resolution grid, n, reduction length K, rows, form, split-K, options.  Images per tile: 16 at 4^2, 4 at 8^2, 1 from 16^2 on.
# The float64 reference of the two largest grids covers bands of output rows (map edges, tile seams, the middle).
# Every case runs its launch with float32 output (gated against float64) AND with bf16 output (= that result rounded).
CASES = [
    (4, 17, 1536, 128, "g", True, {}),
    (4, 3, 1024, 96, "d", False, dict(mask="bf16")),
    (8, 3, 1024, 256, "g", False, {}),
    (8, 5, 1536, 96, "d", True, dict(mask="bf16")),
    (16, 2, 192, 96, "g", False, {}),
    (16, 3, 192, 256, "d", False, dict(mask="bits")),
    (16, 2, 384, 320, "d", False, dict(mask="bf16")),
    (32, 1, 384, 96, "g", False, {}),
    (32, 1, 192, 256, "d", False, dict(mask="bits")),
    (64, 1, 192, 96, "g", False, dict(bands=[(0, 6), (58, 70), (122, 128)])),
    (128, 1, 192, 96, "d", False, dict(mask="bits", bands=[(0, 10), (60, 68), (120, 136), (250, 256)])),
]


def run_case(ops, xb, h, n, k, rows, form, opts, gen, tgen):
    """one launch of the generator form (forward weight of a conv3x3(upsample2(.)) layer: bias, bf16 out) or of the
    discriminator-dgrad form (data-gradient weight of an avg_pool2(conv3x3(.)) layer: alpha = 0.25, device alpha, ReLU mask)"""
    master, wl = exact_master(rows, k, gen, "fwd" if form == "g" else "dgrad")
    assert_fixture_is_lossless(wl)
    wf, wd = ops.prep_conv_weight(torch.from_numpy(master).cuda(), None, True, phase="ups" if form == "g" else "pool")
    w = wf if form == "g" else wd
    assert w.phase is not None and w.phase[0] == "out" and w.phase_mx8 is not None
    kw, ref_kw = {}, {}
    if form == "g":
        bias = torch.randn(rows, generator=tgen).cuda()
        kw.update(bias=bias)
        ref_kw.update(bias=bias)
    else:
        alpha_dev = torch.full((1,), 0.75, device="cuda")
        m = torch.randn((n, 2 * h, 2 * h, rows), generator=tgen).clamp_min(0).bfloat16().cuda()
        if opts.get("mask") == "bits":
            m.bits = bits_of(m).to(torch.int16)
        kw.update(bias=None, alpha=0.25, alpha_dev=alpha_dev, mask=m)
        ref_kw.update(alpha=0.25 * 0.75, mask=m)
    bias = kw.pop("bias")
    y = ops.conv(xb, w, bias, ks=3, ups=True, out_f32=True, **kw)
    assert ops.last_conv_mx8_phase and ops.last_conv_phase
    assert y.dtype == torch.float32 and tuple(y.shape) == (n, 2 * h, 2 * h, rows)
    # bf16 out: the same accumulators through the same epilogue, rounded once on the store
    yb = ops.conv(xb, w, bias, ks=3, ups=True, emit_bits=True, **kw)
    assert ops.last_conv_mx8_phase and yb.dtype == torch.bfloat16
    assert torch.equal(yb, y.bfloat16())
    if not ops.lib.xmc_conv2d_mx8_workspace_bytes(C.byref(_desc(ops, n, h, k, rows))) or ops.no_split_k:
        assert torch.equal(yb.bits.to(torch.int32) & 0xFFFF, bits_of(yb))          # (y > 0) as bits: launches without split-K
    return y, wl, ref_kw


@pytest.mark.parametrize("h,n,k,rows,form,split_k,opts", CASES)
def test_conv_phase_mx8_exact_on_lossless_operands(h, n, k, rows, form, split_k, opts):
    """Activations and tap sums whose MX quantisation is exact: the phase launch must equal float64
    conv3x3(nearest_upsample2(x)) with the epilogue applied in float64, up to float32 accumulation -- tap sets, per-phase patch
    origin, halo, stride-2 store, both operands' block scales, split-K and every epilogue option of the two call sites."""
    ops = _ops()
    ops.no_split_k = not split_k
    gen = np.random.default_rng(h * 1000 + k + rows)
    tgen = torch.Generator().manual_seed(h + rows)
    x = torch.from_numpy(lossless_mx((n, h, h, k // 32), gen))
    xb = x.bfloat16()
    assert torch.equal(xb.float(), x)
    d = _desc(ops, n, h, k, rows)
    assert not split_k or ops.lib.xmc_conv2d_mx8_workspace_bytes(C.byref(d)) > 0, "the case does not exercise what it names"
    y, wl, ref_kw = run_case(ops, xb.cuda(), h, n, k, rows, form, opts, gen, tgen)
    check_against_float64((h, n, k, rows, form, split_k, opts), y, x.double(), wl, opts.get("bands"), **ref_kw)


def _desc(ops, n, h, k, rows, flags=None, pool_out=0):
    from xmcgan_image_generation_amd._lib import XMC_CONV_PACKED, XMC_CONV_PHASE, ConvDesc
    flags = XMC_CONV_PACKED | XMC_CONV_PHASE if flags is None else flags
    return ConvDesc(n, h, h, k, rows, 3, 1, 0, 0, 0, ops.code, 1.0, 1.0, flags, pool_out, 0, 0, 0, 0, None)


@pytest.mark.parametrize("scale", [1.0, 1e-4])
def test_conv_phase_mx8_generic_activations_exact_weights(scale):
    """Gaussian bf16 activations (and gradient-sized ones), quantised by the device; the reference runs on the DECODED packets,
    so only the kernel's handling of the per-block activation scales in its patch is under test.  Same gate."""
    ops = _ops()
    gen = np.random.default_rng(7)
    tgen = torch.Generator().manual_seed(7)
    tab = torch.from_numpy(e4m3_decode_table())
    for h, n, k, rows, form in ((16, 2, 192, 96, "g"), (8, 5, 1024, 96, "d")):
        xb = (torch.randn((n, h, h, k), generator=tgen) * scale).bfloat16().cuda()
        pk = ops.quantize_mx8(xb).cpu().view(n, h, h, k // 64, 80)
        el = tab[pk[..., :64].long()].view(n, h, h, k // 32, 32)
        sc = torch.exp2(pk[..., 64:66].double() - 127).reshape(n, h, h, k // 32, 1)
        xdec = (el * sc).reshape(n, h, h, k)
        assert float((xdec - xb.double().cpu()).norm() / xb.double().norm()) < 5e-2          # they ARE the packets of xb
        y, wl, ref_kw = run_case(ops, xb, h, n, k, rows, form, {}, gen, tgen)
        check_against_float64(("decoded", scale, h, n, k, rows, form), y, xdec, wl, None, **ref_kw)


def test_conv_phase_mx8_accuracy_on_gaussian_data_vs_bf16_phase_kernel():
    """Generic data, 192 -> 96 channels at 16^2 -> 32^2 (and the data-gradient form at gradient-sized values): norm-relative
    difference of the MX phase launch to the bf16 phase launch, the gate of
    test_conv_mx8_accuracy_on_gaussian_data_and_dgrad_adjoint (a CPU emulation of this computation gives 3.8e-2)."""
    ops = _ops()
    g = torch.Generator().manual_seed(5)
    n, h, cin, cout = 4, 16, 192, 96
    x = torch.randn((n, h, h, cin), generator=g).bfloat16().cuda()
    w = (torch.randn((cout, 9, cin), generator=g) * 0.03).cuda()
    wf, _ = ops.prep_conv_weight(w, None, True, phase="ups")
    dy = (torch.randn((n, h, h, cin), generator=g) * 1e-4).bfloat16().cuda()
    wp = (torch.randn((cin, 9, cout), generator=g) * 0.03).cuda()
    _, wd = ops.prep_conv_weight(wp, None, True, phase="pool")
    for name, t, wt in (("fwd", x, wf), ("dgrad", dy, wd)):
        y8 = ops.conv(t, wt, None, ks=3, ups=True, out_f32=True)
        assert ops.last_conv_mx8_phase
        ops.fp8_phase_mx = False
        y16 = ops.conv(t, wt, None, ks=3, ups=True, out_f32=True)
        assert ops.last_conv_phase and not ops.last_conv_mx8_phase
        ops.fp8_phase_mx = True
        rel = float((y8 - y16).norm() / y16.norm())
        print(f"MX-fp8 phase vs bf16 phase {name}: norm-relative difference {rel:.3e}")
        assert rel < 6e-2, (name, rel)


def test_conv_phase_mx8_takes_producer_packets():
    """packets written by the conditional-BatchNorm launch and by an MX convolution's epilogue (``emit_mx8``) serve the phase
    launch: same bytes as the launch that quantises a packet-less clone itself; its own ``emit_mx8`` packets equal the pass's."""
    ops = _ops()
    ops.no_split_k = True
    g = torch.Generator().manual_seed(3)
    n, h, c, rows = 3, 16, 192, 128
    w = (torch.randn((rows, 9, c), generator=g) * 0.03).cuda()
    wf, _ = ops.prep_conv_weight(w, None, True, phase="ups")
    bias = torch.randn(rows, generator=g).cuda()
    x = torch.randn((n, h, h, c), generator=g).bfloat16().cuda()
    mean, rstd = torch.randn(c, generator=g).cuda() * 0.1, (torch.rand(c, generator=g) + 0.5).cuda()
    gb = (torch.randn((n, 2 * c), generator=g) * 0.3).cuda()
    a0 = ops.cbn_act_fwd(x, mean, rstd, gb, 1, relu=True)
    assert a0.mx8 is not None and a0.mx8[1] is False
    w0 = (torch.randn((c, 9, c), generator=g) * 0.03).cuda()
    wf0, _ = ops.prep_conv_weight(w0, None, False)
    a1 = ops.conv(x, wf0, None, ks=3, emit_mx8=False)
    assert a1.mx8 is not None and a1.mx8[1] is False
    for a in (a0, a1):
        y1 = ops.conv(a, wf, bias, ks=3, ups=True, emit_mx8=True)
        assert ops.last_conv_mx8_phase
        y2 = ops.conv(a.clone(), wf, bias, ks=3, ups=True)
        assert ops.last_conv_mx8_phase
        assert torch.equal(y1, y2)
        assert y1.mx8 is not None and y1.mx8[1] is True
        assert torch.equal(y1.mx8[0][:, :, :66], ops.quantize_mx8(y1, relu=True)[:, :, :66])


@pytest.mark.parametrize("split_k", [False, True])
def test_conv_phase_mx8_is_deterministic(split_k):
    """no float atomics: each split writes its own float32 slice and a finishing pass adds them in a fixed order"""
    ops = _ops()
    ops.no_split_k = not split_k
    g = torch.Generator().manual_seed(9)
    n, h, c, rows = 7, 8, 1536, 192
    x = torch.randn((n, h, h, c), generator=g).bfloat16().cuda()
    wf, _ = ops.prep_conv_weight((torch.randn((rows, 9, c), generator=g) * 0.02).cuda(), None, True, phase="ups")
    assert ops.lib.xmc_conv2d_mx8_workspace_bytes(C.byref(_desc(ops, n, h, c, rows))) > 0      # (ops.no_split_k lends none)
    a = ops.conv(x, wf, None, ks=3, ups=True).clone()
    assert ops.last_conv_mx8_phase
    torch.cuda.synchronize()
    b = ops.conv(x, wf, None, ks=3, ups=True)
    assert torch.equal(a, b)


def test_nothing_moves_while_the_switch_is_off():
    """ops.fp8 with fp8_phase_mx off: an ``ups`` launch on a phase site runs the bf16 phase kernel, bit for bit the launch of
    the bf16 mode, and gets no MX twin.  The "in" form is not built: bit 4 + pool_out on the MX entry point is XMC_EINVAL."""
    ops = _ops(phase_mx=False)
    g = torch.Generator().manual_seed(1)
    n, h, c, rows = 2, 16, 192, 96
    x = torch.randn((n, h, h, c), generator=g).bfloat16().cuda()
    wf, _ = ops.prep_conv_weight((torch.randn((rows, 9, c), generator=g) * 0.03).cuda(), None, True, phase="ups")
    assert wf.phase is not None and wf.phase_mx8 is None
    y8 = ops.conv(x, wf, None, ks=3, ups=True)
    assert ops.last_conv_phase and not ops.last_conv_mx8_phase
    ops.fp8 = False
    y16 = ops.conv(x, wf, None, ks=3, ups=True)
    assert ops.last_conv_phase and not ops.last_conv_mx8_phase
    assert torch.equal(y8, y16)
    # the C entry point
    ops.fp8, ops.fp8_phase_mx = True, True
    wf2, _ = ops.prep_conv_weight((torch.randn((rows, 9, c), generator=g) * 0.03).cuda(), None, True, phase="ups")
    assert ops.lib.xmc_conv2d_mx8_phase_supported(C.byref(_desc(ops, n, h, c, rows))) == 1
    d = _desc(ops, n, 2 * h, c, rows, pool_out=1)
    d.ups = 0
    assert ops.lib.xmc_conv2d_mx8_phase_supported(C.byref(d)) == 0
    x8 = ops.quantize_mx8(torch.randn((n, 2 * h, 2 * h, c), generator=g).bfloat16().cuda())
    y = torch.zeros((n, h, h, rows), dtype=torch.bfloat16, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = ops.lib.xmc_conv2d_mx8(C.byref(d), p(x8), p(wf2.phase_mx8[0]), p(wf2.phase_mx8[1]), None, None, None, p(y), None, 0, None, None)
    assert rc == -22, rc                                   # XMC_EINVAL
    torch.cuda.synchronize()
    assert not bool(y.any())


def _c1_b8_fp8_phase_cfg():
    from tests.test_gpu_step import _c1_b8_oracle
    o = _c1_b8_oracle()
    cfg = o["cfg"].copy()
    cfg.dtype = "bfloat16"
    cfg.conv_fp8 = cfg.conv_fp8_phase = True
    return o, cfg


def test_train_step_conv_fp8_phase_vs_fp32_oracle(monkeypatch):
    """config.conv_fp8 + config.conv_fp8_phase at the C1 network, per-device batch 8, against the float32 oracle with exactly the
    gates of test_train_step_conv_fp8_vs_fp32_oracle (1e-1 of the loss scale on the hinge losses, 1e-2 on the contrastive
    ones, second step finite); G's forward and D's backward both ran ``ups`` launches on conv_phase_mx8_kernel."""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    from xmcgan_image_generation_amd.ops import HipOps
    o, cfg = _c1_b8_fp8_phase_cfg()
    seen = {"fwd": 0, "dgrad": 0}
    inner = HipOps.conv

    def counting(self, x, w, bias=None, **kw):
        y = inner(self, x, w, bias, **kw)
        if self.last_conv_mx8_phase:
            seen["dgrad" if kw.get("mask") is not None else "fwd"] += 1      # D's pullback carries the ReLU mask, G's forward a bias
            assert kw.get("ups")
        return y
    monkeypatch.setattr(HipOps, "conv", counting)
    gen, disc, state = train_utils.create_train_state(cfg, 0)
    ops = gen(train=True).ops
    assert ops.fp8 and ops.fp8_phase and ops.fp8_phase_mx
    state = train_utils.load_flax_params(state, *o["init"])
    tb = {k: torch.as_tensor(v).cuda() for k, v in o["batch"].items()}
    state, m = train_utils.train_step(0, state, tb, xmc_gan, gen, disc, cfg, {})
    print("conv_phase_mx8 launches in one step:", seen, "counter:", ops.mx8_phase_launches)
    assert seen["fwd"] >= 1 and seen["dgrad"] >= 1 and ops.mx8_phase_launches == seen["fwd"] + seen["dgrad"]
    ref = o["ref_metrics"]
    scale = max(abs(float(ref[k])) for k in ("d_loss", "g_loss", "c_loss_d", "c_loss_g"))
    for k in ("d_loss", "g_loss", "c_loss_d", "c_loss_g"):
        r = abs(float(m[k]) - float(ref[k])) / scale
        print("conv_fp8_phase C1 b8", k, float(m[k]), float(ref[k]), r)
        assert np.isfinite(float(m[k])) and r < (1e-1 if k in ("d_loss", "g_loss") else 1e-2), (k, float(m[k]), float(ref[k]))
    state, m2 = train_utils.train_step(1, state, tb, xmc_gan, gen, disc, cfg, {})
    assert all(np.isfinite(float(v)) for v in m2.values())
    assert bool(torch.isfinite(state.g_optimizer.arena.params).all()) and bool(torch.isfinite(state.d_optimizer.arena.params).all())


def test_train_step_conv_fp8_phase_is_bit_reproducible_and_graph_replay_equals_eager():
    """the default (overlapped two-stream) schedule twice from the same state: bit-identical losses and parameters (the MX twins
    are made on the preparing stream); hipGraph replay of the step equals the eager step bit for bit."""
    from xmcgan_image_generation_amd import train_utils, xmc_gan
    o, cfg = _c1_b8_fp8_phase_cfg()
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
        assert gen(train=True).ops.mx8_phase_launches > 0
        runs.append(({k: float(v) for k, v in m.items()}, st.g_optimizer.arena.params.clone(), st.d_optimizer.arena.params.clone()))
        del st, gen, disc
        torch.cuda.empty_cache()
    for name, r in (("second eager run", runs[1]), ("graph replay", runs[2])):
        assert all(np.isfinite(v) for v in r[0].values())
        assert runs[0][0] == r[0], (name, runs[0][0], r[0])
        assert torch.equal(runs[0][1], r[1]) and torch.equal(runs[0][2], r[2]), name
