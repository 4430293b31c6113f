"""The area-pool kernels (csrc/loss_pool.hip; ops.area_pool / ops.area_pool_bwd_add) against F.avg_pool2d in float64 and its autograd.

Bars, derived and not measured (eps = 2^-24, the unit round-off of fp32):
  forward   max|y - ref| <= f^2 * eps * max|x|: a sum of n = f^2 fp32 terms in ANY order is off by at most
            (n - 1) eps / (1 - (n - 1) eps) * sum|x_i| <= n eps sum|x_i| (n <= 256), and sum|x_i| / n <= max|x|; the scaling by the power of
            two 1/f^2 is exact.
  backward  max|out - ref| <= 2 eps * max(|gimg0| + |gs|/f^2): gs/f^2 is exact, the one fp32 add rounds by at most eps * |result| — the bar
            leaves that a factor of two.
  adjoint   |<pool(x), g> - <x, unpool(g)>| <= f^2 * eps * <|x|, |unpool(g)|>.  Both inner products are summed in float64 from the device
            results.  unpool(g) = g/f^2 is exact (asserted), so the right side is exact; on the left each y_p carries the forward's error,
            at most eps * sum_window|x| by the line above, and sum_p |g_p| sum_window|x| = f^2 <|x|, |unpool(g)|>."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oodgan import synth  # noqa: E402

EPS = 2.0 ** -24
# (f, (B,C,H,W), take the contiguous batch slice x[1:] of a batch one larger: a non-zero base offset)
CASES = [(2, (1, 3, 2, 2), False), (2, (3, 3, 6, 10), False),
         (4, (2, 3, 8, 12), True), (4, (1, 3, 256, 256), False), (4, (3, 3, 148, 76), False),
         (8, (1, 3, 8, 24), False), (8, (2, 3, 64, 64), False),
         (16, (1, 3, 16, 32), False), (16, (1, 3, 256, 256), False)]
IDS = [f'f{f}-{"x".join(map(str, s))}{"-slice" if sl else ""}' for f, s, sl in CASES]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _inputs(dev, f, shape, sliced):
    """(x, gimg0, gs) on the CPU and on the device; with ``sliced`` the device tensors are x[1:] of a batch one larger."""
    B, C, H, W = shape
    full = (B + 1, C, H, W) if sliced else shape
    small = (full[0], C, H // f, W // f)
    x = 3.0 * synth.normal('pool.x', full, 1)
    g0 = 3.0 * synth.normal('pool.g0', full, 2)
    gs = 3.0 * synth.normal('pool.gs', small, 3)
    cut = (lambda t: t[1:]) if sliced else (lambda t: t)
    xd, g0d, gsd = x.to(dev), g0.to(dev), gs.to(dev)
    return tuple(cut(t) for t in (x, g0, gs)), tuple(cut(t) for t in (xd, g0d, gsd))


@pytest.mark.parametrize('f,shape,sliced', CASES, ids=IDS)
def test_forward_backward_and_adjoint_vs_float64(dev, f, shape, sliced):
    from oodgan import _lib, ops
    (x, g0, gs), (xd, g0d, gsd) = _inputs(dev, f, shape, sliced)
    assert xd.is_contiguous() and (not sliced or xd.storage_offset() > 0)
    before = _lib.dispatch_count('area_pool')
    # forward, with and without the gradient buffer
    y = ops.area_pool(xd, f)
    y2, gz = ops.area_pool(xd, f, grad_buffer=True)
    ref = F.avg_pool2d(x.double(), f)
    assert y.shape == ref.shape and y.dtype == torch.float32 and gz.shape == y.shape
    e_f, bar_f = (y.double().cpu() - ref).abs().max().item(), f * f * EPS * x.abs().max().item()
    assert torch.equal(y, y2) and torch.equal(gz, torch.zeros_like(gz))
    # backward: gimg0 + the autograd of avg_pool2d, in float64
    xr = x.double().requires_grad_(True)
    (unpool,) = torch.autograd.grad(F.avg_pool2d(xr, f), xr, gs.double())
    want = g0.double() + unpool
    gimg = g0d.clone()
    out = ops.area_pool_bwd_add(gsd, gimg, f)
    assert out is gimg
    e_b = (gimg.double().cpu() - want).abs().max().item()
    bar_b = 2 * EPS * (g0.double().abs() + unpool.abs()).max().item()
    # the adjoint identity from the device results, summed in float64
    zero = torch.zeros_like(g0d)
    ops.area_pool_bwd_add(gsd, zero, f)
    lhs = (y.double().cpu() * gs.double()).sum().item()
    rhs = (x.double() * zero.double().cpu()).sum().item()
    bar_a = f * f * EPS * (x.double().abs() * unpool.abs()).sum().item()
    print(f'area_pool f={f} {shape}{" slice" if sliced else ""}: forward {e_f:.2e} (bar {bar_f:.2e}), backward {e_b:.2e} (bar {bar_b:.2e}), '
          f'adjoint |{lhs:.9g} - {rhs:.9g}| = {abs(lhs - rhs):.2e} (bar {bar_a:.2e})')
    assert e_f <= bar_f
    assert e_b <= bar_b
    assert abs(lhs - rhs) <= bar_a
    assert torch.equal(zero.double().cpu(), unpool)                  # g/f^2 is exact in fp32
    assert _lib.dispatch_count('area_pool') == before + 4            # one per accepted call


@pytest.mark.parametrize('f,shape,sliced', [CASES[0], CASES[4], CASES[8]], ids=[IDS[0], IDS[4], IDS[8]])
def test_gzero_is_written_and_leaves_y_alone(dev, f, shape, sliced):
    """A buffer pre-filled with NaN is exactly zero after the call (the library's own entry point, so that the buffer is ours)."""
    from oodgan import _lib, ops
    _, (xd, _, gsd) = _inputs(dev, f, shape, sliced)
    B, C, H, W = xd.shape
    y1, y2 = torch.full_like(gsd, float('nan')), torch.full_like(gsd, float('nan'))
    gz = torch.full_like(gsd, float('nan'))
    L = _lib.lib()
    _lib.check(L.oodgan_area_pool_fwd(ops._p(xd), ops._p(y1), None, B * C, H, W, f, ops._stream()), 'area_pool_fwd')
    _lib.check(L.oodgan_area_pool_fwd(ops._p(xd), ops._p(y2), ops._p(gz), B * C, H, W, f, ops._stream()), 'area_pool_fwd')
    assert torch.equal(gz, torch.zeros_like(gz)) and not torch.isnan(y1).any() and torch.equal(y1, y2)


@pytest.mark.parametrize('f,shape,sliced', CASES, ids=IDS)
def test_two_runs_give_identical_bits(dev, f, shape, sliced):
    from oodgan import ops
    _, (xd, g0d, gsd) = _inputs(dev, f, shape, sliced)
    ya, yb = ops.area_pool(xd, f), ops.area_pool(xd, f)
    ga, gb = ops.area_pool_bwd_add(gsd, g0d.clone(), f), ops.area_pool_bwd_add(gsd, g0d.clone(), f)
    assert torch.equal(ya, yb) and torch.equal(ga, gb)


def test_refusals_touch_nothing(dev):
    from oodgan import _lib, ops
    L = _lib.lib()
    x = synth.normal('pool.rx', (2, 3, 16, 32), 1).to(dev)
    gimg = synth.normal('pool.rg', (2, 3, 16, 32), 2).to(dev)
    gimg0 = gimg.clone()
    before = _lib.dispatch_count('area_pool')
    # the library: a status and a message, the pre-filled outputs untouched
    for f, H, W in ((1, 16, 32), (3, 16, 32), (5, 16, 32), (32, 16, 32), (4, 16, 30), (8, 12, 32), (2, 15, 32)):
        y, gz, gs = torch.full((2, 3, 16, 32), 7.0, device=dev), torch.full((2, 3, 16, 32), 9.0, device=dev), torch.ones(2, 3, 16, 32, device=dev)
        assert L.oodgan_area_pool_fwd(ops._p(x), ops._p(y), ops._p(gz), 6, H, W, f, ops._stream()) == -1, (f, H, W)
        assert L.oodgan_last_error()
        assert L.oodgan_area_pool_bwd_add(ops._p(gs), ops._p(gimg), 6, H, W, f, ops._stream()) == -1, (f, H, W)
        torch.cuda.synchronize()
        assert (y == 7.0).all() and (gz == 9.0).all() and torch.equal(gimg, gimg0)
    # the ops
    small = lambda f: torch.ones(2, 3, max(1, 16 // f), max(1, 32 // f), device=dev)
    for f in (1, 3, 5, 32):
        with pytest.raises((RuntimeError, ValueError)):
            ops.area_pool(x, f)
        with pytest.raises((RuntimeError, ValueError)):
            ops.area_pool_bwd_add(small(f), gimg, f)
    for f in (0, -2, 2.0, True, '2', None):
        with pytest.raises(ValueError, match='factor'):
            ops.area_pool(x, f)
    with pytest.raises(RuntimeError, match='multiple'):                     # H % f != 0
        ops.area_pool(x[:, :, :15].contiguous(), 2)
    with pytest.raises((RuntimeError, ValueError)):
        ops.area_pool_bwd_add(torch.ones(2, 3, 7, 16, device=dev), gimg[:, :, :15].contiguous(), 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.area_pool(x.cpu(), 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.area_pool_bwd_add(small(2).cpu(), gimg, 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.area_pool_bwd_add(small(2), gimg.cpu(), 2)
    with pytest.raises(ValueError, match='contiguous'):
        ops.area_pool(x[:, :, :, ::2], 2)
    with pytest.raises(ValueError, match='contiguous'):
        ops.area_pool(x.transpose(2, 3), 2)
    with pytest.raises(ValueError, match='contiguous'):
        ops.area_pool_bwd_add(small(2), gimg.transpose(2, 3), 2)
    with pytest.raises(ValueError, match='contiguous'):
        ops.area_pool_bwd_add(torch.ones(2, 3, 8, 32, device=dev)[:, :, :, ::2], gimg, 2)
    with pytest.raises(ValueError):
        ops.area_pool(x.double(), 2)
    with pytest.raises(ValueError, match='shape'):
        ops.area_pool_bwd_add(small(4), gimg, 2)
    torch.cuda.synchronize()
    assert torch.equal(gimg, gimg0)
    assert _lib.dispatch_count('area_pool') == before
    ops.area_pool(x, 2)
    assert _lib.dispatch_count('area_pool') == before + 1
    ops.area_pool_bwd_add(small(2), gimg, 2)
    assert _lib.dispatch_count('area_pool') == before + 2
