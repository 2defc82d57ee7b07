"""The guard-band allocator of tests/guard.py on the CPU: it places tensors where it says, it sees one damaged byte on either
side of a tensor and names the allocation and the distance, it counts what it could not serve, and it leaves torch as it found it."""
import pytest
import torch

from tests.guard import MIN_BAND, Guard, GuardError, guarded

SKEWS = [0, 16]
DTYPES = [torch.float32, torch.bfloat16, torch.uint8, torch.int16, torch.float8_e4m3fn]


def _rec_of(g, t):
    """(base, off, nbytes) of the allocation that holds t"""
    for base, off, n, *_ in g.recs:
        if base.data_ptr() + off == t.data_ptr():
            return base, off, n
    raise AssertionError("tensor is not a guarded allocation")


@pytest.mark.parametrize("skew", SKEWS)
def test_allocations_are_contiguous_at_the_residue_and_poisoned(skew):
    g = Guard("cpu", skew=skew)
    for dtype in DTYPES:
        for shape in ((3, 5, 7), (1,), (40000,)):
            t = g.alloc(shape, dtype)
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
            assert t.data_ptr() % 512 == skew
            base, off, n = _rec_of(g, t)
            assert n == t.numel() * t.element_size() and off >= MIN_BAND and base.numel() - off - n >= MIN_BAND
            assert bool((base == 0xFF).all())                                      # the tensor itself too: "uninitialised" reads NaN
            if dtype in (torch.float32, torch.bfloat16, torch.float8_e4m3fn) and t.numel():
                assert bool(torch.isnan(t.float()).all())
            elif dtype == torch.int16 and t.numel():
                assert bool((t == -1).all())
    big = g.alloc((300000,), torch.float32)                                        # the band grows with the tensor
    base, off, n = _rec_of(g, big)
    assert off >= n and base.numel() - off - n >= n
    g.check()
    assert g.recs == []                                                            # checked: the references are dropped


@pytest.mark.parametrize("skew", SKEWS)
def test_a_clean_sequence_checks_clean_and_the_patched_functions_allocate_guarded(skew):
    g = Guard("cpu", skew=skew)
    with guarded(g):
        a = torch.empty((3, 5, 7), dtype=torch.bfloat16, device="cpu")
        b = torch.zeros(10, 3, dtype=torch.float32, device="cpu")
        c = torch.empty_like(a)
        d = torch.zeros_like(a, dtype=torch.float32)
        e = torch.full((4, 4), 2.5, device="cpu")
        f = torch.full((6,), -1, dtype=torch.int16, device="cpu")
        h = g.place(torch.arange(12.0).view(3, 4))
        cpu_only = torch.empty((2, 2))                                             # no device given: not the guard's business
        a.fill_(1.0), c.fill_(2.0), b.add_(1.0), h.mul_(2.0)                       # in-bounds writes
    for t in (a, b, c, d, e, f, h):
        assert t.data_ptr() % 512 == skew and t.is_contiguous()
        _rec_of(g, t)
    assert g.served == 7 and g.fallthrough == []
    assert d.dtype == torch.float32 and d.shape == a.shape and not d.any()
    assert bool((e == 2.5).all()) and e.dtype == torch.float32 and bool((f == -1).all())
    assert torch.equal(h, 2 * torch.arange(12.0).view(3, 4))
    with pytest.raises(AssertionError):
        _rec_of(g, cpu_only)
    g.check()


@pytest.mark.parametrize("skew", SKEWS)
def test_zeros_is_zero_inside_and_ff_outside(skew):
    g = Guard("cpu", skew=skew)
    with guarded(g):
        z = torch.zeros((5, 9), dtype=torch.bfloat16, device="cpu")
    base, off, n = _rec_of(g, z)
    assert n == 90 and not base[off:off + n].any()
    assert bool((base[:off] == 0xFF).all()) and bool((base[off + n:] == 0xFF).all())
    g.check()


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("k", [0, 1, 37, 4096, MIN_BAND - 1])
def test_one_byte_behind_a_tensor_is_reported_with_allocation_and_distance(skew, k):
    g = Guard("cpu", skew=skew)
    with guarded(g):
        first = torch.empty((8, 8), dtype=torch.float32, device="cpu")
        victim = torch.zeros((3, 5, 7), dtype=torch.bfloat16, device="cpu"); line = _line()      # noqa: E702
        last = torch.empty((16,), dtype=torch.uint8, device="cpu")
    base, off, n = _rec_of(g, victim)
    base[off + n + k] = 0x3C
    with pytest.raises(GuardError) as ei:
        g.check()
    (d,) = ei.value.damage
    assert (d.shape, d.dtype, d.side, d.distance, d.last, d.count, d.value) == ((3, 5, 7), torch.bfloat16, "after", k, k, 1, 0x3C)
    assert d.where == f"{__file__}:{line}"
    assert f"distance {k} " in str(ei.value) and "(3, 5, 7)" in str(ei.value) and d.where in str(ei.value)
    del first, last


@pytest.mark.parametrize("skew", SKEWS)
@pytest.mark.parametrize("k", [1, 2, 600, MIN_BAND])
def test_one_byte_in_front_of_a_tensor_is_reported_with_allocation_and_distance(skew, k):
    g = Guard("cpu", skew=skew)
    with guarded(g):
        other = torch.empty((8, 8), dtype=torch.float32, device="cpu")
        victim = torch.empty((11,), dtype=torch.int16, device="cpu"); line = _line()              # noqa: E702
    base, off, n = _rec_of(g, victim)
    base[off - k] = 0
    with pytest.raises(GuardError) as ei:
        g.check()
    (d,) = ei.value.damage
    assert (d.shape, d.dtype, d.side, d.distance, d.last, d.count, d.value) == ((11,), torch.int16, "before", -k, -k, 1, 0)
    assert d.where == f"{__file__}:{line}"
    del other


def _line():
    import sys
    return sys._getframe(1).f_lineno


def test_an_overhanging_run_reports_nearest_farthest_and_count_per_allocation():
    g = Guard("cpu", skew=16)
    a, b = g.alloc((100,), torch.float32), g.alloc((7, 3), torch.bfloat16)
    ba, oa, na = _rec_of(g, a)
    ba[oa + na + 8:oa + na + 24] = 0                                               # a 16-byte store 8 bytes past the end of a
    bb, ob, nb = _rec_of(g, b)
    bb[ob - 4:ob] = 1
    bb[ob + nb] = 2
    bad = g.damage()
    assert [(d.shape, d.side, d.distance, d.last, d.count) for d in bad] == [
        ((100,), "after", 8, 23, 16), ((7, 3), "before", -1, -4, 4), ((7, 3), "after", 0, 0, 1)]


@pytest.mark.parametrize("skew", SKEWS)
def test_a_fall_through_is_counted_and_served_by_the_original_function(skew):
    g = Guard("cpu", skew=skew)
    with guarded(g):
        wide = torch.zeros((6, 10), dtype=torch.float32, device="cpu")
        col = wide[:, 2:7]                                                          # must keep its strides: cannot be guarded
        like = torch.empty_like(col)
        pinned = torch.zeros((4,), device="cpu", requires_grad=True)
        ok = torch.empty_like(wide)
    assert g.served == 2 and len(g.fallthrough) == 2, g.fallthrough
    assert g.fallthrough[0].startswith("empty_like at " + __file__) and "strides" in g.fallthrough[0]
    assert g.fallthrough[1].startswith("zeros at " + __file__) and "requires_grad" in g.fallthrough[1]
    assert like.shape == col.shape and pinned.requires_grad and not pinned.any()
    _rec_of(g, ok)
    g.check()


@pytest.mark.parametrize("skew", SKEWS)
def test_patched_functions_are_restored_after_an_exception(skew):
    names = ("empty", "empty_like", "zeros", "zeros_like", "full")
    before = [getattr(torch, n) for n in names]
    methods = [torch.Tensor.cuda, torch.Tensor.to]
    had = ["cuda" in torch.Tensor.__dict__, "to" in torch.Tensor.__dict__]
    g = Guard("cpu", skew=skew)
    with pytest.raises(RuntimeError, match="boom"):
        with guarded(g):
            assert all(getattr(torch, n) is not f for n, f in zip(names, before))
            assert torch.Tensor.cuda is not methods[0] and torch.Tensor.to is not methods[1]
            torch.empty((2,), device="cpu")
            raise RuntimeError("boom")
    assert all(getattr(torch, n) is f for n, f in zip(names, before))
    assert [torch.Tensor.cuda, torch.Tensor.to] == methods
    assert ["cuda" in torch.Tensor.__dict__, "to" in torch.Tensor.__dict__] == had
    t = torch.empty((2,), device="cpu")
    assert g.served == 1 and t.data_ptr() != g.recs[0][0].data_ptr() + g.recs[0][1]
    assert torch.ones(3).to(torch.float64).dtype == torch.float64


def test_the_guard_keeps_a_dead_workspace_alive_until_it_is_checked():
    g = Guard("cpu")

    def launch():
        with guarded(g):
            ws = torch.empty((64,), dtype=torch.float32, device="cpu")            # a local that dies with the call
        base, off, n = _rec_of(g, ws)
        base[off + n + 3] = 7

    launch()
    with pytest.raises(GuardError) as ei:
        g.check()
    assert ei.value.damage[0].distance == 3 and ei.value.damage[0].shape == (64,)
    g.check()                                                                      # released: a second check has nothing to see
