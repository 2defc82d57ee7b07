"""Each of the seven optimiser entry points of the C ABI returns XMC_EINVAL for the arguments it rejects -- a NULL or misaligned
buffer, n <= 0, a missing step state, a table without its companions, a tile table that is too long, a guarded form without a
usable verdict -- BEFORE it launches anything: every buffer and the step state hold the same bits afterwards.  The entry points
share one validator per kernel (launch_adam_flat in csrc/pointwise.hip, launch_adam_tiles in csrc/spectral_batched.hip); this is
the place where a shim could silently lose a check.  (xmc_nonfinite_verdict's own arguments: test_verdict_rejects_bad_arguments.)"""
import numpy as np
import pytest
import torch

from tests import test_gpu_optimizer as TO

pytestmark = pytest.mark.gpu

EINVAL = -22
_FLAT = ["p", "g", "m", "v", "ema", "n", "lr", "beta1", "beta2", "eps"]
_DEV = _FLAT + ["step_state", "grad_scale", "ema_decay"]
_SN = _DEV + ["zero_grads", "map", "table", "n_entries", "kvec", "scal", "u", "vv"]
_TILES = ["table", "n_tab", "blocks", "p", "g", "m", "v", "ema", "lr", "beta1", "beta2", "eps", "step_state", "grad_scale", "ema_decay",
          "zero_grads", "kvec", "scal", "u", "vv", "wf", "wd", "pf", "pd", "part"]
ORDER = {"xmc_adam_ema": _FLAT + ["c1", "c2", "grad_scale", "ema_decay", "stream"],
         "xmc_adam_ema_dev": _DEV + ["stream"],
         "xmc_adam_ema_dev_sn": _SN + ["stream"],
         "xmc_adam_ema_dev_guarded": _DEV + ["verdict", "stream"],
         "xmc_adam_ema_dev_sn_guarded": _SN + ["verdict", "stream"],
         "xmc_adam_wprep_tiles": _TILES + ["stream"],
         "xmc_adam_wprep_tiles_guarded": _TILES + ["verdict", "stream"]}
HYPER = dict(lr=2e-4, beta1=0.5, beta2=0.999, eps=1e-8, grad_scale=0.5, ema_decay=0.999, c1=0.5, c2=1e-3, zero_grads=1)


def _ops():
    from xmcgan_image_generation_amd.ops import HipOps
    return HipOps(dtype=torch.bfloat16)


def _step_state():
    """t = 3 with (arbitrary) bias corrections in place, as the tile kernel reads them"""
    s = TO._state_bits(3)
    s[1], s[2] = 2.0, 1.5
    return s


def _flat_setup(ops):
    """a 64-element arena that is one spectral tensor (4 x 16), with everything the most general flat form takes"""
    rng = np.random.default_rng(41)
    t = {k: TO._dev(rng.standard_normal(64).astype(np.float32)) for k in ("p", "g", "m", "ema")}
    t["v"] = TO._dev(rng.uniform(1e-6, 1e-2, 64).astype(np.float32))
    bank = ops.sn_bank_create([dict(w_off=0, rows=4, cols=16, u_axis=0, taps=1, is_conv=False)])
    t.update(step_state=_step_state(), map=ops.sn_bank_map(bank, 64), table=bank["tab_fix"], kvec=torch.zeros(4).cuda(),
             scal=torch.ones(4).cuda(), u=torch.zeros(bank["nu"] + 4).cuda(), vv=torch.zeros(bank["nv"] + 4).cuda(),
             verdict=torch.zeros(4, dtype=torch.int32).cuda())
    return t, dict(HYPER, n=64, n_entries=bank["n"])


def _tile_setup(ops):
    """the spectral tile arena of tests/test_gpu_optimizer.py"""
    A = TO._wprep_arena(ops, True)
    t = {k: TO._dev(a) for k, a in A["state"].items()}
    bufs, part = ops.wprep_alloc(A["wp"])
    for b in bufs + [part]:
        b.zero_()
    t.update(g=TO._dev(A["grads"][0]), step_state=_step_state(), table=A["wp"]["tab"], kvec=torch.zeros(A["bank"]["n"]).cuda(),
             scal=TO._dev(A["scal"]), u=TO._dev(np.nan_to_num(A["u"])), vv=TO._dev(np.nan_to_num(A["v"])), part=part,
             verdict=torch.zeros(4, dtype=torch.int32).cuda(), **dict(zip(("wf", "wd", "pf", "pd"), bufs)))
    return t, dict(HYPER, n_tab=A["wp"]["n"], blocks=A["wp"]["blocks"])


def _bad_arguments(name):
    """{argument: the values the entry point must refuse}; "null": NULL, ("off", k): the good pointer moved by k bytes"""
    tiles, guarded = "tiles" in name, name.endswith("_guarded")
    bad = {k: ["null", ("off", 4)] for k in ("p", "g", "m", "v")}
    bad["ema"] = [("off", 4)]                        # (NULL is "no EMA")
    if tiles:
        bad.update(table=["null"], step_state=["null"], n_tab=[0, -1, 65], blocks=[0, -1], vv=["null", ("off", 4)],
                   **{k: ["null"] for k in ("scal", "u", "part")})          # kvec given: scal, u, vv and part must be
    else:
        bad["n"] = [0, -4]
    if name == "xmc_adam_ema":
        bad.update(c1=[0.0, -1.0], c2=[0.0])
    elif not tiles:
        bad["step_state"] = ["null"]
    if "_sn" in name:
        bad.update(n_entries=[0], **{k: ["null"] for k in ("map", "kvec", "scal", "u", "vv")})      # table given: all of them must be
    if guarded:
        bad["verdict"] = ["null", ("off", 2)]
    return bad


@pytest.mark.parametrize("name", list(ORDER))
def test_entry_point_rejects_bad_arguments_before_any_launch(name):
    ops = _ops()
    tensors, scalars = (_tile_setup if "tiles" in name else _flat_setup)(ops)
    fn = getattr(ops.lib, name)

    def call(**change):
        args = []
        for k in ORDER[name]:
            if k == "stream":
                args.append(ops._stream())
            elif k in scalars:
                args.append(change.get(k, scalars[k]))
            else:
                how = change.get(k)
                args.append(None if how == "null" else tensors[k].data_ptr() + (how[1] if how else 0))
        return fn(*args)

    before = {k: t.clone() for k, t in tensors.items()}
    refused = 0
    for k, values in _bad_arguments(name).items():
        assert k in ORDER[name], (name, k)
        for val in values:
            assert call(**{k: val}) == EINVAL, (name, k, val)
            refused += 1
    assert refused >= 11
    torch.cuda.synchronize()
    for k, t in tensors.items():                     # nothing was launched: parameters, moments, EMA, gradient, step state, copies
        assert torch.equal(t.view(torch.uint8), before[k].view(torch.uint8)), (name, k, "changed by a refused call")
    # ... and the unchanged argument list is one the entry point accepts (an unguarded form asks for no verdict: it has none)
    assert call() == 0
    torch.cuda.synchronize()
    assert not torch.equal(tensors["p"], before["p"]) and int(tensors["step_state"].view(torch.int32)[0]) == (3 if "tiles" in name or
                                                                                                            name == "xmc_adam_ema" else 4)
