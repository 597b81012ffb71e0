"""GPU: the Gaussianization kernels (zk_gauss_forward / zk_gauss_inverse / zk_gauss_backward) against the fixtures recorded from the live reference
(tests/golden/gauss_{a..f}.npz) and against tests/gauss_ref.py, under the bars of tests/parity.py.

float32: assert_parity at C = 2.  float64: |d| <= 1e-12 max(1, exp((y^2 - 9) / 2)) element by element — 1e-12 scaled by the map's own conditioning
beyond |y| = 3 (erfinv amplifies a rounding error of its argument by sqrt(pi / 2) exp(y^2 / 2): the float64 REFERENCE carries that error, the
kernel's cancellation-free form does not), times 1 + |y| for ladj (ladj contains y^2 / 2)."""

import numpy as np
import pytest
import torch

import gauss_ref as R
import parity
from conftest import T, golden
from parity import assert_f64, assert_parity

pytestmark = pytest.mark.gpu

CASES = ["gauss_a", "gauss_b", "gauss_c", "gauss_d", "gauss_e", "gauss_f"]
DT = {"32": torch.float32, "64": torch.float64}


def _case(name, dev, dtype):
    g = golden(name + ".npz")
    x, b, a, gy, gl = (T(g[k], dev).to(dtype) for k in ("x", "b", "a", "gy", "gl"))
    return g, x, b, a, gy, gl


def _packed(b, a):
    """[b | a] as one buffer and the two views cut from it (what a conditioner emits)."""
    K = b.shape[-1]
    phi = torch.cat([b, a], dim=-1).contiguous()
    return phi, phi[..., :K], phi[..., K:]


def _cond(y64):
    return torch.clamp(torch.exp((y64.double() ** 2 - 9) / 2), min=1.0)


def assert_f64_scaled(hip, ref64, y64, what, ladj=False, reduced=False):
    """The float64 bar of this file's docstring.  `reduced`: hip / ref64 are sums over the last axis of y64's shape, the bound is the sum of the
    elements' bounds."""
    hip, ref64, y64 = hip.detach().cpu(), T(ref64) if isinstance(ref64, np.ndarray) else ref64.detach().cpu(), T(y64) if isinstance(y64, np.ndarray) else y64.detach().cpu()
    bound = 1e-12 * _cond(y64) * ((1 + y64.abs()) if ladj else 1.0)
    if reduced:
        bound = bound.sum(dim=-1)
    elif not ladj:
        inner = y64.abs() <= 3
        assert_f64(hip[inner], ref64[inner], what + " (|y| <= 3)")
    d = (hip - ref64).abs()
    assert torch.equal(torch.isnan(hip), torch.isnan(ref64)), f"{what}: NaN pattern"
    ratio = float((d / bound).nan_to_num().max())
    parity.REPORT.append({"what": what, "n": int(hip.numel()), "f64_max_abs": float(d.nan_to_num().max()), "f64_max_over_bound": ratio, "ok": ratio <= 1.0})
    assert ratio <= 1.0, f"{what}: max |d| / bound = {ratio:.3f} (max |d| {float(d.max()):.3e})"


@pytest.mark.parametrize("tag", ["32", "64"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_parity_forward_and_inverse(name, tag, dev):
    from zuko_amd import ops

    g, x, b, a, _, _ = _case(name, dev, DT[tag])
    shared = bool(g["meta"][3])
    runs = {"strided": (b, a)}
    if not shared:
        runs["packed"] = _packed(b, a)[1:]
    out = {}
    with torch.no_grad():
        for path, (bb, aa) in runs.items():
            y, ladj = ops.gauss_forward(x, bb, aa)
            y2, lsum = ops.gauss_forward(x, bb, aa, reduce=True)
            inv = ops.gauss_inverse(T(g["y64"], dev).float().to(DT[tag]), bb, aa)
            assert torch.equal(y, y2), f"{name} {path}: y differs between reduce=False and reduce=True"
            out[path] = (y, ladj, lsum, inv)
    if "packed" in out:  # the LDS-staged and the global-memory parameter paths run the same arithmetic
        for u, v, what in zip(out["packed"], out["strided"], ("y", "ladj", "ladj reduced", "inverse")):
            assert torch.equal(u, v), f"{name} f{tag}: {what} differs between the packed and the strided path"
    y, ladj, lsum, inv = out["strided"]
    assert lsum.shape == x.shape[:-1]
    if tag == "32":
        assert_parity(y, g["y32"], g["y64"], f"{name} f32: y")
        assert_parity(ladj, g["ladj32"], g["ladj64"], f"{name} f32: ladj")
        assert_parity(lsum, g["ladj32"].sum(-1), g["ladj64"].sum(-1), f"{name} f32: ladj reduced")
        assert_parity(inv, g["inv32"], g["inv64"], f"{name} f32: inverse")
    else:
        assert_f64_scaled(y, g["y64"], g["y64"], f"{name} f64: y")
        assert_f64_scaled(ladj, g["ladj64"], g["y64"], f"{name} f64: ladj", ladj=True)
        assert_f64_scaled(lsum, T(g["ladj64"]).sum(-1), g["y64"], f"{name} f64: ladj reduced", ladj=True, reduced=True)
        assert_f64_scaled(inv, g["inv64"], g["y64"], f"{name} f64: inverse")


@pytest.mark.parametrize("name", CASES)
def test_fixture_parity_gradients(name, dev):
    """gx, gb, ga of (y * gy + ladj * gl).sum() in float32: UnivariateFn from separate tensors, UnivariatePackedFn from the packed [b | a]."""
    from zuko_amd import ops

    g, x, b, a, gy, gl = _case(name, dev, torch.float32)
    K, shared = int(g["meta"][2]), bool(g["meta"][3])
    xs, bs, as_ = x.clone().requires_grad_(), b.clone().requires_grad_(), a.clone().requires_grad_()
    y, ladj = ops.gauss_forward(xs, bs, as_)
    assert type(y.grad_fn).__name__.startswith("UnivariateFn")
    gx, gb, ga = torch.autograd.grad((y * gy + ladj * gl).sum(), (xs, bs, as_))
    for k, v in (("gx", gx), ("gb", gb), ("ga", ga)):
        assert_parity(v, g[k + "32"], g[k + "64"], f"{name} f32: {k} (UnivariateFn)")
    assert_parity(y, g["y32"], g["y64"], f"{name} f32: y (UnivariateFn)")
    if shared:
        return
    phi = _packed(b, a)[0].requires_grad_()
    xs = x.clone().requires_grad_()
    y, ladj = ops.gauss_forward(xs, phi[..., :K], phi[..., K:], packed=phi)
    assert type(y.grad_fn).__name__.startswith("UnivariatePackedFn")
    gx2, gphi = torch.autograd.grad((y * gy + ladj * gl).sum(), (xs, phi))
    assert torch.equal(gx2, gx) and torch.equal(gphi[..., :K], gb) and torch.equal(gphi[..., K:], ga), f"{name}: the packed and the split autograd routes differ"
    # ladj reduced over features inside the kernel: its weight is per row
    glr = gl[:, 0].contiguous()
    y, lsum = ops.gauss_forward(xs, phi[..., :K], phi[..., K:], reduce=True, packed=phi)
    gx3, gphi3 = torch.autograd.grad((y * gy).sum() + (lsum * glr).sum(), (xs, phi))
    y, ladj = ops.gauss_forward(xs, phi[..., :K], phi[..., K:], packed=phi)
    gx4, gphi4 = torch.autograd.grad((y * gy + ladj * glr[:, None]).sum(), (xs, phi))
    assert torch.equal(gx3, gx4) and torch.equal(gphi3, gphi4), f"{name}: reduced and un-reduced ladj weights differ"


def test_unaligned_packed_parameters_are_bit_identical(dev):
    from zuko_amd import ops

    g, x, b, a, _, _ = _case("gauss_a", dev, torch.float32)
    N, D, K = (int(v) for v in g["meta"][:3])
    phi, pb, pa = _packed(b, a)
    buf = torch.empty(phi.numel() + 1, dtype=torch.float32, device=dev)
    off = buf[1:].view(N, D, 2 * K)
    off.copy_(phi)
    assert phi.data_ptr() % 16 == 0 and off.data_ptr() % 16 == 4
    yin = T(g["y64"], dev).float()
    with torch.no_grad():
        want = (*ops.gauss_forward(x, pb, pa), ops.gauss_forward(x, pb, pa, reduce=True)[1], ops.gauss_inverse(yin, pb, pa))
        got = (*ops.gauss_forward(x, off[..., :K], off[..., K:]), ops.gauss_forward(x, off[..., :K], off[..., K:], reduce=True)[1], ops.gauss_inverse(yin, off[..., :K], off[..., K:]))
    for u, v, what in zip(got, want, ("y", "ladj", "ladj reduced", "inverse")):
        assert torch.equal(u, v), what


def test_rows_are_independent_and_one_row_works(dev):
    from zuko_amd import ops

    g, x, b, a, _, _ = _case("gauss_a", dev, torch.float32)
    _, pb, pa = _packed(b, a)
    _, pb64, pa64 = _packed(b[:64], a[:64])
    _, pb1, pa1 = _packed(b[:1], a[:1])
    with torch.no_grad():
        y, ladj = ops.gauss_forward(x, pb, pa)
        y64, ladj64 = ops.gauss_forward(x[:64].contiguous(), pb64, pa64)
        y1, l1 = ops.gauss_forward(x[:1].contiguous(), pb1, pa1, reduce=True)
        x1 = ops.gauss_inverse(y[:1].contiguous(), pb1, pa1)
        xall = ops.gauss_inverse(y, pb, pa)
    assert torch.equal(y[:64], y64) and torch.equal(ladj[:64], ladj64)
    assert y1.shape == (1, x.shape[1]) and l1.shape == (1,) and torch.equal(y1, y[:1]) and torch.equal(x1, xall[:1])
    assert_parity(l1, g["ladj32"][:1].sum(-1), g["ladj64"][:1].sum(-1), "gauss N = 1: ladj reduced")


def _random(N, D, K, seed, dev):
    gen = torch.Generator().manual_seed(seed)
    x = 1.5 * torch.randn(N, D, generator=gen)
    b, a = torch.randn(N, D, K, generator=gen), 0.5 * torch.randn(N, D, K, generator=gen)
    return x, b, a


@pytest.mark.parametrize("tag", ["32", "64"])
def test_forty_components_read_from_global_memory(tag, dev):
    """K = 40: 80 floats per element are beyond the LDS image, so the packed buffer too takes the strided path."""
    from zuko_amd import ops

    x, b, a = _random(37, 5, 40, 51, dev)
    y32, l32 = R.forward(x, b, a)
    y64, l64 = R.forward(x.double(), b.double(), a.double())
    i32, i64 = R.inverse(y64.float(), b, a), R.inverse(y64.float().double(), b.double(), a.double())
    dt = DT[tag]
    _, pb, pa = _packed(b.to(dev, dt), a.to(dev, dt))
    with torch.no_grad():
        y, ladj = ops.gauss_forward(x.to(dev, dt), pb, pa)
        inv = ops.gauss_inverse(y64.float().to(dev, dt), pb, pa)
    if tag == "32":
        assert_parity(y, y32, y64, "gauss K = 40 f32: y")
        assert_parity(ladj, l32, l64, "gauss K = 40 f32: ladj")
        assert_parity(inv, i32, i64, "gauss K = 40 f32: inverse")
    else:
        assert_f64_scaled(y, y64, y64, "gauss K = 40 f64: y")
        assert_f64_scaled(ladj, l64, y64, "gauss K = 40 f64: ladj", ladj=True)
        assert_f64_scaled(inv, i64, y64, "gauss K = 40 f64: inverse")


def _grads(fwd, x, b, a, gy, gl):
    xs, bs, as_ = x.clone().requires_grad_(), b.clone().requires_grad_(), a.clone().requires_grad_()
    y, ladj = fwd(xs, bs, as_)
    return (y.detach(), ladj.detach(), *torch.autograd.grad((y * gy + ladj * gl).sum(), (xs, bs, as_)))


def test_thirty_three_components_train_on_torch_ops(dev):
    """K = 33 is beyond the adjoint kernel: a call that needs gradients runs the reference's expressions on the device."""
    from zuko_amd import ops

    x, b, a = _random(29, 3, 33, 52, dev)
    gen = torch.Generator().manual_seed(53)
    gy, gl = torch.randn(29, 3, generator=gen), torch.randn(29, 3, generator=gen)
    assert not ops.gauss_supported(33, torch.float32, True) and ops.gauss_supported(33, torch.float32, False)
    r32 = _grads(R.forward, x, b, a, gy, gl)
    r64 = _grads(R.forward, *(t.double() for t in (x, b, a, gy, gl)))
    got = _grads(ops.gauss_forward, *(t.to(dev) for t in (x, b, a, gy, gl)))
    for what, h, u, v in zip(("y", "ladj", "gx", "gb", "ga"), got, r32, r64):
        assert_parity(h, u, v, f"gauss K = 33 f32 (torch ops): {what}")


def test_torch_op_switch_matches_the_kernels(dev):
    from zuko_amd import ops

    g, x, b, a, gy, gl = _case("gauss_a", dev, torch.float32)
    old = ops.GAUSS_KERNEL
    try:
        ops.GAUSS_KERNEL = False
        with torch.no_grad():
            y, ladj = ops.gauss_forward(x, b, a)
            lsum = ops.gauss_forward(x, b, a, reduce=True)[1]
            inv = ops.gauss_inverse(T(g["y64"], dev).float(), b, a)
        got = _grads(ops.gauss_forward, x, b, a, gy, gl)
        assert "Univariate" not in type(ops.gauss_forward(x.clone().requires_grad_(), b, a)[0].grad_fn).__name__
    finally:
        ops.GAUSS_KERNEL = old
    assert_parity(y, g["y32"], g["y64"], "gauss torch ops f32: y")
    assert_parity(ladj, g["ladj32"], g["ladj64"], "gauss torch ops f32: ladj")
    assert_parity(lsum, g["ladj32"].sum(-1), g["ladj64"].sum(-1), "gauss torch ops f32: ladj reduced")
    assert_parity(inv, g["inv32"], g["inv64"], "gauss torch ops f32: inverse")
    for what, h in zip(("gx", "gb", "ga"), got[2:]):
        assert_parity(h, g[what + "32"], g[what + "64"], f"gauss torch ops f32: {what}")


def test_round_trip(dev):
    """inverse(forward(x)) on case a: the error against x is held to the reference's own float32 round trip."""
    from zuko_amd import ops

    g, x, b, a, _, _ = _case("gauss_a", dev, torch.float32)
    xc, bc, ac = x.cpu(), b.cpu(), a.cpu()
    ref = R.inverse(R.forward(xc, bc, ac)[0], bc, ac)
    _, pb, pa = _packed(b, a)
    with torch.no_grad():
        rt = ops.gauss_inverse(ops.gauss_forward(x, pb, pa)[0], pb, pa)
    assert_parity(rt, ref, xc.double(), "gauss f32: round trip")


@pytest.mark.parametrize("tag", ["32", "64"])
def test_far_tails_and_nan(tag, dev):
    from zuko_amd import ops

    g, x, b, a, _, _ = _case("gauss_a", dev, DT[tag])
    _, pb, pa = _packed(b, a)
    with torch.no_grad():
        for v in (50.0, -50.0):
            for bb, aa in ((pb, pa), (b, a)):
                y, ladj = ops.gauss_forward(torch.full_like(x, v), bb, aa)
                assert not torch.isnan(y).any() and not torch.isnan(ladj).any()
                assert float(y.abs().max()) <= 4.9 and bool((y * v > 0).all())
                assert bool((torch.isfinite(ladj) | (ladj == -float("inf"))).all())
                assert torch.isfinite(ops.gauss_inverse(y, bb, aa)).all()
        xn = x.clone()
        xn[3, 2] = float("nan")
        y, ladj = ops.gauss_forward(xn, pb, pa)
        y0, ladj0 = ops.gauss_forward(x, pb, pa)
        mask = torch.zeros_like(x, dtype=torch.bool)
        mask[3, 2] = True
        assert torch.equal(torch.isnan(y), mask) and torch.equal(torch.isnan(ladj), mask)
        assert torch.equal(y[~mask], y0[~mask]) and torch.equal(ladj[~mask], ladj0[~mask])
