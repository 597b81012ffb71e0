"""GPU: the shared-parameter Gaussianization adjoint (zk_gauss_backward_shared behind ops.GAUSS_SHARED_ADJOINT; autograd.GaussSharedFn and
GaussSharedInverseFn) against the fixture gauss_f, tests/gauss_ref.py on the CPU in float32 and float64, and the per-row path it stands beside.
Bars: tests/parity.py (assert_parity at C = 2).  The sum over the rows is held to the bound of ANY order of float32 additions of the per-row
terms, (N - 1) 2^-24 sum_n |term_n| (each of the N - 1 additions rounds a partial sum that is at most sum |term| by at most 2^-24 of it)."""

import contextlib

import pytest
import torch

import gauss_ref as R
import parity
from conftest import T, golden
from parity import assert_parity

pytestmark = pytest.mark.gpu

_REF: dict = {}


@contextlib.contextmanager
def shared(on: bool):
    from zuko_amd import ops

    old = ops.GAUSS_SHARED_ADJOINT
    try:
        ops.GAUSS_SHARED_ADJOINT = on
        yield ops
    finally:
        ops.GAUSS_SHARED_ADJOINT = old


def _random(N, D, K, seed):
    """As _random of tests/test_gpu_gauss.py, with [D, K] parameters; and the weights of y and ladj."""
    gen = torch.Generator().manual_seed(seed)
    x = 1.5 * torch.randn(N, D, generator=gen)
    b, a = torch.randn(D, K, generator=gen), 0.5 * torch.randn(D, K, generator=gen)
    gy, gl = torch.randn(N, D, generator=gen), torch.randn(N, D, generator=gen)
    return x, b, a, gy, gl


def _grads(fwd, x, b, a, gy, gl, reduce=False):
    """(y, ladj, gx, gb, ga) of sum(y gy) + sum(ladj gl); gy / gl None: that output does not enter the loss; gl [N] with reduce."""
    xs, bs, as_ = x.clone().requires_grad_(), b.clone().requires_grad_(), a.clone().requires_grad_()
    y, ladj = fwd(xs, bs, as_)
    if reduce:
        ladj = ladj.sum(dim=-1)
    loss = 0.0
    if gy is not None:
        loss = loss + (y * gy).sum()
    if gl is not None:
        loss = loss + (ladj * gl).sum()
    return (y.detach(), ladj.detach(), *torch.autograd.grad(loss, (xs, bs, as_)))


def _n_star():
    """The smallest N whose partition has three row chunks at D = 6, K = 8, plus 1: the last chunk ends in a partial pass."""
    from zuko_amd import ops

    return next(n for n in range(1, 1 << 16) if ops.gauss_shared_chunks(n, 6, 8) >= 3) + 1


def _case(N, D, K, seed):
    """Inputs and the two CPU references (autograd through gauss_ref.forward), computed once and shared."""
    key = (N, D, K, seed)
    if key not in _REF:
        inp = _random(N, D, K, seed)
        r32 = _grads(R.forward, *inp)
        r64 = _grads(R.forward, *(t.double() for t in inp))
        for t in (*r32, *r64):
            assert bool(torch.isfinite(t).all()), f"{key}: the reference is not finite; pick another seed"
        _REF[key] = (inp, r32, r64)
    return _REF[key]


def _gpu(ops, inp, dev, **kw):
    x, b, a, gy, gl = (None if t is None else t.to(dev) for t in inp)
    return _grads(lambda *p: ops.gauss_forward(*p, reduce=kw.get("kernel_reduce", False)), x, b, a, gy, gl)


def _fixture(dev):
    g = golden("gauss_f.npz")
    assert tuple(int(v) for v in g["meta"]) == (131, 6, 8, 1)
    return g, tuple(T(g[k], dev) for k in ("x", "b", "a", "gy", "gl"))


def test_fixture(dev):
    g, (x, b, a, gy, gl) = _fixture(dev)
    with shared(True) as ops:
        xs, bs, as_ = x.clone().requires_grad_(), b.clone().requires_grad_(), a.clone().requires_grad_()
        y, ladj = ops.gauss_forward(xs, bs, as_)
        assert type(y.grad_fn).__name__.startswith("GaussSharedFn")
        gx, gb, ga = torch.autograd.grad((y * gy + ladj * gl).sum(), (xs, bs, as_))
        with torch.no_grad():
            y0, ladj0 = ops.gauss_forward(x, b, a)
    assert torch.equal(y, y0) and torch.equal(ladj, ladj0)
    assert gx.shape == x.shape and gb.shape == b.shape and ga.shape == a.shape
    for k, v in (("y", y), ("gx", gx), ("gb", gb), ("ga", ga)):
        assert_parity(v, g[k + "32"], g[k + "64"], f"gauss_f f32: {k} (GaussSharedFn)")


SHAPES = [(1, 1, 1, 71), (2, 3, 5, 72), (67, 5, 8, 73), (33, 64, 8, 74), (19, 70, 4, 75), (7, 130, 2, 76), (23, 2, 32, 77), ("N*", 6, 8, 78)]


@pytest.mark.parametrize("N,D,K,seed", SHAPES)
def test_shape_edges(N, D, K, seed, dev):
    from zuko_amd import ops

    if N == "N*":
        N = _n_star()
        assert ops.gauss_shared_chunks(N, D, K) >= 3 and ops.gauss_shared_chunks(N - 2, D, K) < 3
    inp, r32, r64 = _case(N, D, K, seed)
    with shared(True) as ops:
        got = _gpu(ops, inp, dev)
    for what, h, u, v in zip(("y", "ladj", "gx", "gb", "ga"), got, r32, r64):
        assert_parity(h, u, v, f"gauss shared ({N}, {D}, {K}) f32: {what}")


def test_summation_against_the_per_row_terms(dev):
    """The shared result against the float64 sum of the per-row path's own float32 terms, under the bound of this file's docstring."""
    N, D, K = _n_star(), 6, 8
    x, b, a, gy, gl = (t.to(dev) for t in _case(N, D, K, 78)[0])
    with shared(False) as ops:
        rows = _grads(ops.gauss_forward, x, b.expand(N, D, K).contiguous(), a.expand(N, D, K).contiguous(), gy, gl)
    with shared(True) as ops:
        got = _grads(ops.gauss_forward, x, b, a, gy, gl)
    assert rows[3].shape == (N, D, K) and got[3].shape == (D, K)
    for what, h, terms in (("gb", got[3], rows[3]), ("ga", got[4], rows[4])):
        t64 = terms.double()
        bound = (N - 1) * 2.0**-24 * t64.abs().sum(dim=0)
        d = (h.double() - t64.sum(dim=0)).abs()
        ratio = float((d / bound).max())
        parity.REPORT.append({"what": f"gauss shared ({N}, {D}, {K}) f32: {what} against the per-row terms", "n": int(d.numel()), "max_abs": float(d.max()),
                              "max_over_bound": ratio, "ok": bool((d <= bound).all())})
        assert bool((d <= bound).all()), f"{what}: max |d| / bound = {ratio:.3e}"
    same = bool(torch.equal(got[2], rows[2]))
    print(f"gx bit-identical between the shared and the per-row path: {same}")
    parity.REPORT.append({"what": f"gauss shared ({N}, {D}, {K}) f32: gx bit-identical to the per-row path (recorded, not asserted)", "n": int(got[2].numel()), "ok": True,
                          "bit_identical": same})


def test_optional_inputs(dev):
    N, D, K = 67, 5, 8
    inp, _, _ = _case(N, D, K, 73)
    x, b, a, gy, gl = inp
    w = torch.randn(N, generator=torch.Generator().manual_seed(79))
    runs = {"gy = None": (None, gl, False), "gl = None": (gy, None, False), "reduce, per-row weight": (gy, w, True)}
    for name, (wy, wl, red) in runs.items():
        r32 = _grads(R.forward, x, b, a, wy, wl, reduce=red)
        r64 = _grads(R.forward, *(None if t is None else t.double() for t in (x, b, a, wy, wl)), reduce=red)
        with shared(True) as ops:
            got = _gpu(ops, (x, b, a, wy, wl), dev, kernel_reduce=red)
        for what, h, u, v in zip(("y", "ladj", "gx", "gb", "ga"), got, r32, r64):
            assert_parity(h, u, v, f"gauss shared ({N}, {D}, {K}) f32, {name}: {what}")
        if red:
            with shared(True) as ops:
                wide = _gpu(ops, (x, b, a, gy, w[:, None].expand(N, D).contiguous()), dev)
            for what, h, u in zip(("gx", "gb", "ga"), got[2:], wide[2:]):
                assert torch.equal(h, u), f"{what}: the weight of the reduced ladj and the same weight per element differ"


def test_determinism_and_row_independence(dev):
    _, (x, b, a, gy, gl) = _fixture(dev)
    with shared(True) as ops:
        one = _grads(ops.gauss_forward, x, b, a, gy, gl)
        two = _grads(ops.gauss_forward, x, b, a, gy, gl)
        head = _grads(ops.gauss_forward, x[:64].contiguous(), b, a, gy[:64].contiguous(), gl[:64].contiguous())
    for what, u, v in zip(("gx", "gb", "ga"), one[2:], two[2:]):
        assert torch.equal(u, v), f"{what} differs between two calls"
    assert torch.equal(one[2][:64], head[2])


def test_feature_independence_and_nan(dev):
    N, D, K = 67, 5, 8
    x, b, a, gy, gl = (t.to(dev) for t in _case(N, D, K, 73)[0])
    xn = x.clone()
    xn[3, 2] = float("nan")
    with shared(True) as ops:
        clean = _grads(ops.gauss_forward, x, b, a, gy, gl)
        dirty = _grads(ops.gauss_forward, xn, b, a, gy, gl)
    mask = torch.zeros_like(x, dtype=torch.bool)
    mask[3, 2] = True
    assert torch.equal(torch.isnan(dirty[2]), mask) and torch.equal(dirty[2][~mask], clean[2][~mask])
    rows = torch.zeros(D, K, dtype=torch.bool, device=dev)
    rows[2] = True
    for what, u, v in zip(("gb", "ga"), dirty[3:], clean[3:]):
        assert torch.equal(torch.isnan(u), rows), f"{what}: NaN outside (or not all over) feature 2"
        assert torch.equal(u[~rows], v[~rows]), f"{what}: another feature's gradient changed"


def _inverse_reference(y, b, a, w):
    """(x, dL/dy, dL/db, dL/da) of L = sum(w x), x = f^-1(y), by the implicit function theorem on gauss_ref: the seed -w / f'(x) into the closed-form
    adjoint at x, summed over the rows."""
    N, D = y.shape
    x = R.inverse(y, b, a)
    _, ladj = R.forward(x, b, a)
    gy = w * torch.exp(-ladj)
    _, gb, ga = R.backward(x, b.expand(N, *b.shape), a.expand(N, *a.shape), -gy, torch.zeros_like(gy))
    return x, gy, gb.sum(dim=0), ga.sum(dim=0)


def test_inverse_direction(dev):
    g, (_, b, a, _, _) = _fixture(dev)
    y = T(g["y64"]).float()
    w = torch.randn(y.shape, generator=torch.Generator().manual_seed(80))
    r32 = _inverse_reference(y, b.cpu(), a.cpu(), w)
    r64 = _inverse_reference(y.double(), b.cpu().double(), a.cpu().double(), w.double())
    for t in (*r32, *r64):
        assert bool(torch.isfinite(t).all())
    with shared(True) as ops:
        ys, bs, as_ = y.to(dev).requires_grad_(), b.clone().requires_grad_(), a.clone().requires_grad_()
        x = ops.gauss_inverse(ys, bs, as_)
        assert type(x.grad_fn).__name__.startswith("GaussSharedInverseFn")
        grads = torch.autograd.grad((x * w.to(dev)).sum(), (ys, bs, as_))
        with torch.no_grad():
            x0 = ops.gauss_inverse(y.to(dev), b, a)
    assert torch.equal(x, x0)
    for what, h, u, v in zip(("x", "gy", "gb", "ga"), (x, *grads), r32, r64):
        assert_parity(h, u, v, f"gauss_f f32: {what} (GaussSharedInverseFn)")


def test_switch_and_fallbacks(dev):
    g, (x, b, a, gy, gl) = _fixture(dev)
    with shared(False) as ops:
        xs, bs = x.clone().requires_grad_(), b.clone().requires_grad_()
        assert type(ops.gauss_forward(xs, bs, a)[0].grad_fn).__name__.startswith("UnivariateFn")
        assert type(ops.gauss_inverse(xs, bs, a).grad_fn).__name__.startswith("UnivariateInverseFn")
        off = _grads(ops.gauss_forward, x, b, a, gy, gl)
    for k, v in (("gx", off[2]), ("gb", off[3]), ("ga", off[4])):
        assert_parity(v, g[k + "32"], g[k + "64"], f"gauss_f f32: {k} (switch off)")
    with shared(True) as ops:
        # K = 33: torch ops
        inp = _random(29, 3, 33, 81)
        r32, r64 = _grads(R.forward, *inp), _grads(R.forward, *(t.double() for t in inp))
        xs = inp[0].to(dev).requires_grad_()
        name = type(ops.gauss_forward(xs, inp[1].to(dev), inp[2].to(dev))[0].grad_fn).__name__
        assert "GaussShared" not in name and "Univariate" not in name
        for what, h, u, v in zip(("y", "ladj", "gx", "gb", "ga"), _gpu(ops, inp, dev), r32, r64):
            assert_parity(h, u, v, f"gauss shared switch on, K = 33 (torch ops): {what}")
        # [N, D, K] parameters: one row of parameters per element, the per-row kernel
        gg = golden("gauss_a.npz")
        xa, ba, aa, gya, gla = (T(gg[k], dev) for k in ("x", "b", "a", "gy", "gl"))
        assert ba.dim() == 3
        xs = xa.clone().requires_grad_()
        assert type(ops.gauss_forward(xs, ba, aa)[0].grad_fn).__name__.startswith("UnivariateFn")
        rows = _grads(ops.gauss_forward, xa, ba, aa, gya, gla)
        for k, v in (("gx", rows[2]), ("gb", rows[3]), ("ga", rows[4])):
            assert_parity(v, gg[k + "32"], gg[k + "64"], f"gauss_a f32: {k} (switch on, [N, D, K] parameters)")
        # float64: torch ops
        xs = x.double().requires_grad_()
        name = type(ops.gauss_forward(xs, b.double(), a.double())[0].grad_fn).__name__
        assert "GaussShared" not in name and "Univariate" not in name
        f64 = _grads(ops.gauss_forward, *(t.double() for t in (x, b, a, gy, gl)))
        for k, v in (("gx", f64[2]), ("gb", f64[3]), ("ga", f64[4])):
            assert_parity(v, g[k + "32"], g[k + "64"], f"gauss_f f64: {k} (switch on, torch ops)")
        # double backward through the new nodes raises
        xs = x.clone().requires_grad_()
        y, _ = ops.gauss_forward(xs, b, a)
        (g1,) = torch.autograd.grad(y.sum(), xs, create_graph=True)
        with pytest.raises(RuntimeError):
            g1.sum().backward()
        ys = T(g["y64"], dev).float().requires_grad_()
        (g1,) = torch.autograd.grad(ops.gauss_inverse(ys, b, a).sum(), ys, create_graph=True)
        with pytest.raises(RuntimeError):
            g1.sum().backward()


def test_whole_flow(dev):
    import test_gpu_gf as G
    import zuko_amd.flows as F
    from zuko_amd import _C

    name = "flow_gf_uncond"
    f = golden(name + ".npz")
    ref32, _, _ = G._reference(name)
    flow = G._flow(name).to(dev)
    x = T(f["x"], dev)
    with shared(True):
        _C.PROFILE = {}
        try:
            flow().log_prob(x).mean().backward()
            torch.cuda.synchronize()
            calls = set(_C.PROFILE)
        finally:
            _C.PROFILE = None
        assert "zk_gauss_backward_shared" in calls and "zk_gauss_backward" not in calls
        assert [k for k, _ in flow.named_parameters()] == list(f["param_names"])
        for k, p in flow.named_parameters():
            assert p.grad is not None, k
            assert_parity(p.grad, ref32[k], f["grad/" + k], f"{name} (shared adjoint): grad {k}")
        flow.zero_grad()
        flow().rsample((64,)).square().mean().backward()
        for k, p in flow.named_parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
        # twenty Adam steps, as test_training_lowers_the_loss of tests/test_gpu_gf.py
        torch.manual_seed(1)
        small = F.GF(2, transforms=2, components=4).to(dev)
        gen = torch.Generator().manual_seed(2)
        data = (torch.randn(256, 2, generator=gen) * 0.4 + torch.where(torch.rand(256, 1, generator=gen) < 0.5, -1.2, 1.2)).to(dev)
        opt = torch.optim.Adam(small.parameters(), lr=2e-2)
        losses = []
        for _ in range(20):
            loss = -small().log_prob(data).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        assert all(l == l for l in losses) and losses[-1] < losses[0], losses
        # a bfloat16 flow: one step on float32 copies
        half = G._flow(name).to(dev).to(torch.bfloat16)
        opt = torch.optim.Adam(half.parameters(), lr=1e-3)
        loss = -half().log_prob(x.to(torch.bfloat16)).mean()
        loss.backward()
        for k, p in half.named_parameters():
            assert p.grad is not None and p.grad.dtype == torch.bfloat16 and bool(torch.isfinite(p.grad).all()), k
        opt.step()
        assert all(bool(torch.isfinite(p).all()) for p in half.parameters())


def test_memory(dev):
    """One forward and backward at 2^14 x 64, K = 8, in units of 4 N D bytes (one [N, D] float32 tensor): at most 10 with the switch on (x's copy, y,
    ladj, the products and their weights, gx, the workspace; the expanded parameters alone would be 16), more than 32 with it off (the packed copy
    and its gradient are 16 each)."""
    N, D, K = 2**14, 64, 8
    x, b, a, gy, gl = (t.to(dev) for t in _random(N, D, K, 82))
    unit = 4 * N * D
    peak = {}
    for on in (True, False):
        with shared(on) as ops:
            xs, bs, as_ = x.clone().requires_grad_(), b.clone().requires_grad_(), a.clone().requires_grad_()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            y, ladj = ops.gauss_forward(xs, bs, as_)
            grads = torch.autograd.grad((y * gy + ladj * gl).sum(), (xs, bs, as_))
            torch.cuda.synchronize()
            peak[on] = (torch.cuda.max_memory_allocated() - before) / unit
            del y, ladj, grads
    print(f"peak memory over the level before the call, in [N, D] float32 tensors: shared {peak[True]:.2f}, per row {peak[False]:.2f}")
    parity.REPORT.append({"what": f"gauss shared ({N}, {D}, {K}): peak memory in units of 4 N D bytes", "shared": peak[True], "rows": peak[False], "n": 2,
                          "ok": peak[True] <= 10 and peak[False] > 32})
    assert peak[True] <= 10, peak
    assert peak[False] > 32, peak
