"""Every launch family inside the guard-band allocator (tests/guard.py): the case-running bodies of the other GPU test modules are
called with torch's allocation functions routed through ``Guard.alloc``, at ``skew`` 0 (what torch hands out) and 16 (the weakest
pointer include/xmcgan_hip.h admits).  A body passes only if

1. its own float64 / bit-equality assertions still hold -- with NaN bytes around every operand and in every fresh output, a wrong
   ``*_bytes`` extent, a tail lane that is not multiplied away or an unwritten output element fails them;
2. no byte of any guard band changed (``Guard.check``): no tile overhang, no split-K slice or partial row past the workspace;
3. nothing was allocated behind the guard's back (``Guard.fallthrough`` is empty).

The cases are the SMALL rows of the existing tables -- ragged couts, N that is no multiple of the images per tile, split-K
workspaces at exactly their advertised size -- not the workload's layers.  No new references: the oracles are the ones the bodies
already carry.  The last test puts garbage into the canvas margin that the compact 3x3 launches of the ResNet leg leave unwritten."""
import functools
import math

import pytest
import torch

from tests import test_gpu_fused_opt as FO
from tests import test_gpu_inception as INC
from tests import test_gpu_kernels as K
from tests import test_gpu_mx8 as MX
from tests import test_gpu_mx8_phase as MXP
from tests import test_gpu_mx8_phase_in as MXI
from tests import test_gpu_resnet as RN
from tests import test_gpu_word_loss_fused as WL
from tests.guard import Guard, guarded

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
SKEWS = [0, 16]
skews = pytest.mark.parametrize("skew", SKEWS)            # the top decorator varies fastest: every case runs plain, then skewed


def _run(skew, body, *args, **kw):
    g = Guard("cuda", skew=skew)
    try:
        with guarded(g):
            out = body(*args, **kw)
    except Exception as e:                                  # a faulted device answers every later call with the same error:
        if "illegal memory access" in str(e) or "hipErrorLaunchFailure" in str(e):       # nothing more is started on it
            pytest.exit(f"GPU fault in {getattr(body, '__name__', body)}{args} at skew {skew}: {e}", returncode=3)
        raise
    assert g.served > 0, "the body allocated nothing through the guard"
    g.check()
    assert g.fallthrough == [], g.fallthrough
    return out


def _row(table, *head, **ex):
    """the row of a case table that starts with ``head`` and whose options include ``ex``"""
    rows = [r for r in table if tuple(r[:len(head)]) == head and all(r[-1].get(k) == v for k, v in ex.items())]
    assert len(rows) == 1, (head, ex, rows)
    return rows[0]


def _word(v):
    if isinstance(v, dict):
        return "+".join(sorted(k for k in v if v[k])) or "plain"
    if isinstance(v, bool):
        return "TF"[not v]
    return str(v).replace("torch.", "")


def _ids(rows):
    return ["-".join(_word(v) for v in (r if isinstance(r, tuple) else (r,))) for r in rows]


def _cases(rows):
    return pytest.mark.parametrize("case", rows, ids=_ids(rows))


@skews
def test_the_guard_sees_a_damaged_byte_on_the_device(skew):
    """positive control on the GPU (tests/test_guard_harness.py does the rest on the CPU): one byte written through the base
    buffer 40 bytes past a tensor is reported at that distance, and the tensor sits at the requested residue"""
    from tests.guard import GuardError
    g = Guard("cuda", skew=skew)
    with guarded(g):
        a = torch.zeros((5, 7), dtype=BF16, device="cuda")
        b = torch.ones(3).cuda()
    assert a.data_ptr() % 512 == skew and b.data_ptr() % 512 == skew and g.served == 2 and not a.any()
    base, off, n = g.recs[0][:3]
    assert base.data_ptr() + off == a.data_ptr() and n == 70
    base[off + n + 40] = 0
    with pytest.raises(GuardError) as ei:
        g.check()
    (d,) = ei.value.damage
    assert (d.shape, d.side, d.distance, d.count) == ((5, 7), "after", 40, 1)


# ------------------------------------------------------------------------------------------------ ops.conv, unpacked weights
# (implicit-GEMM and LDS-patch kernels).  (2, 8, 40, 24, valid=7) has cin = 40: outside the fragment-packed domain
# (cin % 32), so the ``valid=`` row runs here and the packed family takes the table's packed ``valid=`` row instead
CONV_ROWS = [_row(K.CONV_CASES, 2, 8, 16, 32, 3), _row(K.CONV_CASES, 2, 32, 3, 16, 3), _row(K.CONV_CASES, 2, 16, 24, 3, 3),
             _row(K.CONV_CASES, 2, 4, 40, 16, 1, True), _row(K.CONV_CASES, 2, 8, 16, 8, 3, res_ups=True, mask=True, bias=True),
             _row(K.CONV_CASES, 2, 64, 32, 40, 3), _row(K.CONV_CASES, 8, 8, 96, 136, 3), _row(K.CONV_CASES, 1, 8, 16, 16, 3, out_f32=True),
             _row(K.CONV_CASES, 2, 8, 40, 24, 3, valid=7)]


@skews
@pytest.mark.parametrize("dtype", K.DT, ids=["f32", "bf16"])
@_cases(CONV_ROWS)
def test_conv_unpacked(case, dtype, skew):
    _run(skew, K.test_conv_fwd, dtype, case)


# ------------------------------------------------------------------------------------- packed weight-streaming 3x3 + split-K
STREAM_ROWS = [_row(K.STREAM_CASES, 3, 64, 32, 72), _row(K.STREAM_CASES, 5, 8, 64, 3), _row(K.STREAM_CASES, 8, 4, 32, 32, 3, True),
               _row(K.STREAM_CASES, 8, 4, 256, 64), _row(K.STREAM_CASES, 4, 4, 384, 96, 3, True),
               _row(K.STREAM_CASES, 3, 16, 64, 64, 3, valid=14)]


@skews
@_cases(STREAM_ROWS)
def test_conv_stream_packed(case, skew):
    _run(skew, K.test_conv_stream_packed, case)


POOL_OUT_ROWS = [(2, 64, 32, 96, False, True), (1, 128, 64, 40, False, False)]


@skews
@_cases(POOL_OUT_ROWS)
def test_conv_stream_pool_out(case, skew):
    _run(skew, K.test_conv_stream_pool_out, case)


@skews
def test_conv_mask_bits(skew):
    _run(skew, K.test_conv_mask_bits, ("plain", 3, 16, 64, 96))          # y_bits / mask_bits are operands too


# --------------------------------------------------------------------------------------------------------- pointwise, packed
PW_ROWS = [_row(K.PW_CASES, 3, 16, 96, 40), _row(K.PW_CASES, 5, 8, 32, 3), _row(K.PW_CASES, 8, 8, 128, 64),
           _row(K.PW_CASES, 16, 8, 1024, 160), _row(K.PW_CASES, 2, 32, 160, 64)]


@skews
@_cases(PW_ROWS)
def test_conv_pointwise_packed(case, skew):
    _run(skew, K.test_conv_pointwise_packed, case)


@skews
@_cases([(9, 8, 7, 512, 128), (2, 16, 14, 256, 96)])
def test_conv_pointwise_compact(case, skew):
    _run(skew, K.test_conv_pointwise_compact, case)


@skews
@_cases(RN.DUAL_BLOCKS)
def test_pointwise_dual_source_forward(case, skew):
    _run(skew, RN.test_pointwise_dual_source_launch_vs_float64, case, 3)


@skews
@_cases(RN.DUAL_BLOCKS)
def test_pointwise_dual_source_data_gradient(case, skew):
    _run(skew, RN.test_pointwise_dual_source_data_gradient_vs_float64, case)


# ------------------------------------------------------------------------------------------------------------- phase kernels
PHASE_ROWS = [("ups", 3, 4, 64, 128), ("ups", 2, 32, 32, 96), ("pool", 3, 8, 64, 128), ("pool", 2, 64, 32, 96)]


@skews
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "gauss"])
@_cases(PHASE_ROWS)
def test_conv_phase(case, exact, skew):
    _run(skew, K.test_conv_phase, case, exact)


@skews
def test_conv_stride2_phase(skew):
    _run(skew, K.test_conv_stride2_phase, (3, 8, 64, 64))


# -------------------------------------------------------------------------------------------------------------------- MX-fp8
@skews
@pytest.mark.parametrize("rule", ["next_binade", "ocp_floor"])
def test_mx8_quantizer_scale_rules(rule, skew):
    _run(skew, MX.test_mx8_quantizer_scale_rules, rule)


MX_ROWS = sorted(MX.CASES, key=lambda c: c[0] * c[1] * c[1] * c[2] * c[3])[:2]


@skews
@_cases([c[:4] + (",".join(sorted(c[4])) or "plain",) for c in MX_ROWS])
def test_conv_mx8_exact_on_lossless_operands(case, skew):
    row = _row(MX.CASES, *case[:4])
    _run(skew, MX.test_conv_mx8_exact_on_lossless_operands, *row)


@skews
@pytest.mark.parametrize("relu,pool,mask", [(True, False, False), (False, False, True), (True, True, False)])
def test_conv_mx8_epilogue_emits_the_next_layers_packets(relu, pool, mask, skew):
    _run(skew, MX.test_conv_mx8_epilogue_emits_the_next_layers_packets, relu, pool, mask)


@skews
def test_conv_mx8_relu_on_store_and_bit_masks_split_k(skew):
    _run(skew, MX.test_conv_mx8_relu_on_store_and_bit_masks, True)


@skews
def test_cbn_act_emits_packets(skew):
    _run(skew, MX.test_cbn_act_emits_packets)


def _smallest(cases):
    """(h, n, k, rows, ...): least work first"""
    return min(cases, key=lambda c: c[0] * c[0] * c[1] * c[2] * c[3])


@skews
def test_conv_phase_mx8_exact(skew):
    _run(skew, MXP.test_conv_phase_mx8_exact_on_lossless_operands, *_smallest(MXP.CASES))


@skews
def test_conv_phase_in_mx8_exact(skew):
    _run(skew, MXI.test_conv_phase_in_mx8_exact_on_lossless_operands, *_smallest(MXI.CASES))


# ---------------------------------------------------------------------------------------------------------- weight gradients
WG_SETTINGS = [(F32, 0), (BF16, 0), (BF16, 1)]


@skews
@pytest.mark.parametrize("dtype,variant", WG_SETTINGS, ids=["f32-v0", "bf16-v0", "bf16-v1"])
@_cases(K.WG_CASES[:8])
def test_conv_wgrad(case, dtype, variant, skew):
    _run(skew, K.test_conv_wgrad, dtype, variant, case)


WG_PATCH_ROWS = [c for h in ((8, 8, 96, 64), (16, 4, 64, 64), (4, 16, 32, 96), (8, 16, 32, 136)) for c in K.WG_CASES if c[:4] == h]
assert len(WG_PATCH_ROWS) == 4


@skews
@_cases(WG_PATCH_ROWS)
def test_conv_wgrad_patch_kernels(case, skew):
    _run(skew, K.test_conv_wgrad, BF16, 1, case)


@skews
@_cases([("ups", 4, 4, 64, 64, False), ("ups", 2, 8, 96, 64, False), ("pool", 2, 16, 32, 96, False)])
def test_conv_wgrad_phase(case, skew):
    assert case in K.WGP_CASES
    _run(skew, K.test_conv_wgrad_phase, case)


@skews
@_cases([("ups", 2, 16, 32, 96), ("pool", 2, 16, 64, 64), ("pool", 8, 4, 64, 64), ("1x1", 2, 16, 1024, 96), ("generic", 2, 8, 16, 24)])
def test_conv_wgrad_first_write_every_kernel_path(case, skew):
    _run(skew, K.test_conv_wgrad_first_write_every_kernel_path, case)


# --------------------------------------------------------------------------------------------------------------------- GEMMs
GEMM_ROWS = [(70, 50, 33, False, False), (130, 140, 64, False, True), (17, 256, 768, True, False)]


@skews
@_cases(GEMM_ROWS)
def test_gemm(case, skew):
    _run(skew, K.test_gemm, case)


@skews
@_cases(GEMM_ROWS)
def test_gemm_bf16_mfma(case, skew):
    _run(skew, K.test_gemm_bf16_mfma, case)


@skews
def test_gemm_batched_strided(skew):
    _run(skew, K.test_gemm_batched_strided)


@skews
@pytest.mark.parametrize("out_dtype", [F32, BF16], ids=["f32", "bf16"])
def test_tn_gemm_two_segments(out_dtype, skew):
    _run(skew, WL.test_tn_gemm_two_segments, out_dtype)


# ---------------------------------------------------------------------------------------------------------------------- norm
@skews
@pytest.mark.parametrize("dtype", K.DT, ids=["f32", "bf16"])
def test_reduce_mid_and_bcast(dtype, skew):
    shapes = [(1, 1000, 3), (4, 16, 96), (2, 9, 4100), (1, 56, 24576)]
    assert set(shapes) <= set(K.REDUCE_SHAPES)
    _run(skew, K.test_reduce_mid_and_bcast, dtype, shapes)


CBN_GEOS = [(3, 8, 16, 1), (2, 16, 24, 4), (2, 16, 40, 16), (4, 4, 1536, 1), (2, 32, 64, 4)]


@skews
@pytest.mark.parametrize("dtype", K.DT, ids=["f32", "bf16"])
@_cases(CBN_GEOS)
def test_cbn(case, dtype, skew):
    _run(skew, K.test_cbn, dtype, case)


@skews
@_cases([(3, 8, 16, 1), (2, 16, 24, 4), (2, 16, 40, 16), (2, 16, 768, 16)])
def test_cbn_bf16_gamma_beta(case, skew):
    _run(skew, K.test_cbn_bf16_gamma_beta, case)           # gamma | beta are a column slice of a wider tensor: neighbouring bytes


# -------------------------------------------------------------------------------------------------------- pointwise / layout
@skews
@pytest.mark.parametrize("dtype", K.DT, ids=["f32", "bf16"])
def test_pointwise(dtype, skew):
    _run(skew, K.test_pointwise, dtype)


@skews
@pytest.mark.parametrize("dtype", K.DT, ids=["f32", "bf16"])
def test_expand_taps_and_rgb_paths(dtype, skew):
    _run(skew, K.test_expand_taps_and_rgb_paths, dtype)


@skews
def test_prep_conv_weight_layouts(skew):
    _run(skew, K.test_prep_conv_weight_layouts)


@skews
def test_prep_conv_weight_packed_matches_pack_of_plain(skew):
    _run(skew, K.test_prep_conv_weight_packed_matches_pack_of_plain)


# ------------------------------------------------------------------------------------------------------ attention and losses
@skews
@pytest.mark.parametrize("dtype", K.DT, ids=["f32", "bf16"])
def test_attention_for_g(dtype, skew):
    _run(skew, K.test_attention_for_g, dtype)


@skews
@_cases([(3, 256), (2, 128)])
def test_attention_for_g_on_mfma(case, skew):
    _run(skew, K.test_attention_for_g_on_mfma, case)


@skews
def test_l2norm_bwd(skew):
    _run(skew, K.test_l2norm_bwd)


@skews
def test_xent_hinge_proj(skew):
    _run(skew, K.test_xent_hinge_proj)


@skews
@_cases([(4, 96), (9, 2048)])
def test_contrastive_loss_fused(case, skew):
    _run(skew, K.test_contrastive_loss_fused_vs_float64_and_gemm_chain, *case)


@skews
@pytest.mark.parametrize("dtype", K.DT, ids=["f32", "bf16"])
def test_word_loss_kernels_vs_spec(dtype, skew):
    _run(skew, K.test_word_loss_kernels_vs_spec, dtype, dict(b=2, r=16, t=5, e=32, max_len=[5, 5]))


@skews
@_cases([(3, 128), (5, 768)])
def test_word_loss_prep_kernels(case, skew):
    _run(skew, WL.test_prep_kernels, *case)


@skews
def test_word_loss_cols_fwd_bwd(skew):
    _run(skew, WL.test_cols_fwd_bwd_vs_float64, 4, [1, 17, 1, 12])


@skews
def test_fused_word_loss(skew):
    _run(skew, WL.test_fused_word_loss_vs_spec_and_gemm_path, 4, [1, 17, 1, 12])


# ------------------------------------------------------------------------------------------- spectral norm and the optimiser
@skews
@pytest.mark.parametrize("u_axis", [0, 1])
def test_spectral(u_axis, skew):
    _run(skew, K.test_spectral, u_axis)


@skews
def test_adam_ema(skew):
    _run(skew, K.test_adam_ema)


@skews
def test_adam_ema_device_step_counter(skew):
    _run(skew, K.test_adam_ema_device_step_counter)


@skews
def test_spectral_bank_matches_per_weight_path(skew):
    _run(skew, K.test_spectral_bank_matches_per_weight_path)


@skews
@_cases([(64, 9, 32, "ups"), (64, 1, 96, None), (32, 1, 32, None)])
def test_wprep_copies(case, skew):
    _run(skew, FO.test_wprep_copies_equal_the_per_site_kernels_and_partials_equal_float64, case)


@skews
def test_fused_power_iteration(skew):
    _run(skew, FO.test_fused_power_iteration_equals_the_three_pass_one)


@skews
def test_adam_wprep_tiles(skew):
    _run(skew, FO.test_adam_wprep_tiles_equals_flat_adam_then_wprep)     # the arenas are single allocations: the band behind one
                                                                         # catches the optimiser kernel's padding guard


# ---------------------------------------------------------------------------------------------------------------- ResNet ops
@skews
@pytest.mark.parametrize("dtype", RN.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("hs", [16, 128])
def test_resize_to_canvas_and_adjoint(hs, dtype, skew):
    _run(skew, RN.test_resize_to_canvas_and_adjoint, dtype, hs)


@skews
@pytest.mark.parametrize("dtype", RN.DT, ids=["f32", "bf16"])
def test_stem_im2col_and_col2im(dtype, skew):
    _run(skew, RN.test_stem_im2col_and_col2im, dtype)


@skews
@pytest.mark.parametrize("dtype", RN.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [12, 3])
def test_maxpool_and_adjoint_first_maximum(c, dtype, skew):
    _run(skew, RN.test_maxpool_and_adjoint_first_maximum, dtype, c)


@skews
@pytest.mark.parametrize("dtype", RN.DT, ids=["f32", "bf16"])
@pytest.mark.parametrize("c", [36, 3])
def test_margin_subsample_relu_ops(c, dtype, skew):
    _run(skew, RN.test_margin_subsample_relu_ops, dtype, c)


@skews
def test_stem_as_one_implicit_gemm_launch(skew):
    _run(skew, RN.test_stem_as_one_implicit_gemm_launch_vs_float64_and_the_im2col_path, 2)


@skews
def test_stem_data_gradient_as_one_launch(skew):
    _run(skew, RN.test_stem_data_gradient_as_one_launch_vs_float64_and_the_col2im_path, 1)


# ----------------------------------------------------------------------------------------------------------------- Inception
@functools.lru_cache(maxsize=None)
def _inception_ops(name):
    """the operator table the Inception bodies take as a fixture: built once, outside the guard"""
    from xmcgan_image_generation_amd.ops import HipOps
    torch.cuda.set_device(0)
    return HipOps(dtype=INC.DT[name])


@skews
@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_inception_conv_every_geometry(name, skew):
    _run(skew, INC.test_conv_every_geometry, _inception_ops(name))


@skews
@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_inception_conv_slices_leave_other_channels_untouched(name, skew):
    _run(skew, INC.test_conv_slices_leave_other_channels_untouched, _inception_ops(name))


@skews
@pytest.mark.parametrize("name", ["f32", "bf16"])
def test_inception_pools(name, skew):
    _run(skew, INC.test_pools, _inception_ops(name))


# ------------------------------------------------------------------------------------- compact 3x3 launches: the canvas margin
def _ff(shape, dtype):
    """a tensor whose every byte is 0xFF (NaN in bf16), whatever the allocator handed out"""
    t = torch.empty(shape, dtype=dtype, device="cuda")
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _canvas(n, s, v, c, gen):
    """random valid corner, zero margin: (device bf16, float64 cpu)"""
    x = torch.zeros((n, s, s, c), dtype=BF16)
    x[:, :v, :v] = torch.randn((n, v, v, c), generator=gen).to(BF16)
    return x.cuda(), x.double()


def _compact3_chains(s, v):
    """the forward and backward launches of a stride-1 bottleneck block (pretrained_model_utils.ResNet50Features) around its 3x3
    layer, once compact (valid corner only, 3x3 output into 0xFF bytes) and once on whole canvases with zeroed margins"""
    n, c = 3, 64
    ops = K._ops(BF16)
    ops.stream_conv = True
    gen = torch.Generator().manual_seed(100 + s)
    w32 = {k: torch.randn((c, t, c), generator=gen) / math.sqrt(t * c) for k, t in (("c1", 1), ("c2", 9), ("c3", 1))}
    bias = {k: torch.randn(c, generator=gen).cuda() for k in w32}
    wf, wd, wr = {}, {}, {}
    for k, w in w32.items():
        wf[k], wd[k] = ops.prep_conv_weight(w.cuda(), None, True)
        wr[k] = w.to(BF16).double()
    x, xr = _canvas(n, s, v, c, gen)
    g, gr = _canvas(n, s, v, c, gen)
    got = {}
    for compact in (True, False):
        zero = (lambda: dict(compact=True, out=torch.zeros((n, s, s, c), dtype=BF16, device="cuda"))) if compact else dict
        poisoned = (lambda: dict(compact=True, out=_ff((n, s, s, c), BF16))) if compact else dict
        kept = (lambda: dict(compact=True, out=torch.full((n, s, s, c), 7.0, dtype=BF16, device="cuda"))) if compact else dict
        t = {}
        t["h1"] = ops.conv(x, wf["c1"], bias["c1"], ks=1, relu_out=True, valid=v, emit_bits=True, **zero())
        t["h2"] = ops.conv(t["h1"], wf["c2"], bias["c2"], ks=3, relu_out=True, valid=v, emit_bits=True, **poisoned())
        t["out"] = ops.conv(t["h2"], wf["c3"], bias["c3"], ks=1, res=x, relu_out=True, valid=v, emit_bits=True, **kept())
        t["dh2"] = ops.conv(g, wd["c3"], None, ks=1, mask=t["h2"], valid=v, **zero())
        assert getattr(t["h1"], "bits", None) is not None and getattr(t["h2"], "bits", None) is not None
        t["dh1"] = ops.conv(t["dh2"], wd["c2"], None, ks=3, mask=t["h1"], valid=v, **poisoned())
        t["gx"] = ops.conv(t["dh1"], wd["c1"], None, ks=1, valid=v, **kept())
        got[compact] = t
    torch.cuda.synchronize()
    return got, dict(x=xr, g=gr, w=wr, b={k: b.double().cpu() for k, b in bias.items()})


@skews
@_cases([(32, 28), (64, 56), (128, 112)])
def test_compact_3x3_launches_with_garbage_in_the_margin(case, skew):
    """3x3 launches with ``compact=True`` skip the tiles that lie in the canvas margin (y0 >= valid) and do not zero it: what the
    caller left there stays -- here 0xFF bytes.  Their neighbours in a bottleneck block are compact pointwise launches that read
    the valid corner only, so the valid corner of every tensor of the chain (and of the ReLU bits) equals the whole-canvas chain
    bit for bit, agrees with float64 and is finite; the margins of the final outputs keep the caller's values.
    conv_stream_kernel's tiles are 256 pixels (SBM), 256 / min(W, 64) rows: at 64 / 56 the row tiles at 56 and 60 are skipped, at
    128 / 112 the four at 112 .. 124 (two column tiles each); at 32 / 28 the last tile starts at row 24 and nothing is skipped --
    the chain holds there all the same, the margin is then whatever the convolution gives."""
    s, v = case
    got, ref = _run(skew, _compact3_chains, s, v)
    cp, full = got[True], got[False]
    corner = lambda t: t[:, :v, :v]
    for name in ("h1", "h2", "out", "dh2", "dh1", "gx"):
        a, b = corner(cp[name]), corner(full[name])
        assert bool(torch.isfinite(a.float()).all()), name
        assert torch.equal(a, b), name
    for name in ("h1", "h2"):
        assert torch.equal(corner(cp[name].bits), corner(full[name].bits)), name
    # the skipped tiles still hold the 0xFF bytes -- the garbage really is there
    rt = 256 // min(s, 64)
    y_skip = -(-v // rt) * rt
    assert (y_skip < s) == (s >= 64)
    for name in ("h2", "dh1"):
        assert y_skip == s or bool((cp[name][:, y_skip:].contiguous().view(torch.uint8) == 0xFF).all()), name
    margin = torch.ones((3, s, s), dtype=torch.bool, device="cuda")
    margin[:, :v, :v] = False
    for name in ("out", "gx"):
        assert bool((cp[name][margin] == 7.0).all()), name
        assert bool((full[name][margin] == 0).all()), name
    # float64 on the same bf16 operands, stage by stage (each stage from the kernel's own previous output)
    w, b = ref["w"], ref["b"]
    cpu = {k: corner(t).double().cpu() for k, t in cp.items()}
    conv = lambda t, k, ks: K._ref_conv(t, w[k], None, ks) + b[k]
    K._close(cpu["h1"], torch.relu(conv(corner(ref["x"]), "c1", 1)), BF16, "h1")
    K._close(cpu["h2"], torch.relu(conv(cpu["h1"], "c2", 3)), BF16, "h2")                  # (zero padding == the zero margin of h1)
    K._close(cpu["out"], torch.relu(conv(cpu["h2"], "c3", 1) + corner(ref["x"])), BF16, "out")
    K._close(cpu["dh2"], (corner(ref["g"]) @ w["c3"][:, 0]) * (cpu["h2"] > 0), BF16, "dh2")
    h1r = torch.zeros_like(cpu["h1"], requires_grad=True)
    (d,) = torch.autograd.grad(K._ref_conv(h1r, w["c2"], None, 3), h1r, cpu["dh2"])
    K._close(cpu["dh1"], d * (cpu["h1"] > 0), BF16, "dh1")
    K._close(cpu["gx"], cpu["dh1"] @ w["c1"][:, 0], BF16, "gx")
