"""GPU: the Gaussian mixture kernels (zk_gmm_log_prob / zk_gmm_backward) against tests/gmm_ref.py on the CPU — the fixtures of the live reference,
the shape and launch envelope, strides, the shared-row reduction, row independence, non-finite rows — and zuko_amd.mixtures.GMM on top of them.

Bars: tests/parity.py.  float32: assert_parity (allclose(1e-5, 1e-5) to the float32 reference, or an error against float64 within C = 2 of the float32
reference's own); float64: assert_f64 (1e-12).  References are computed once per shape (module-level cache) and never modified."""

import ctypes
import functools
import itertools

import pytest
import torch

import gmm_ref
from conftest import T, golden, sd_hash
from parity import assert_f64, assert_parity

pytestmark = pytest.mark.gpu

CASES = ["gmm_a", "gmm_b", "gmm_c", "gmm_d", "gmm_e", "gmm_f"]
COMBOS = list(itertools.product(gmm_ref.COVARIANCES, (False, True)))
SHAPES = [(1, 1), (2, 3), (5, 4), (16, 8), (33, 3), (64, 2), (4, 64)]
DTYPES = {torch.float32: 0, torch.float64: 1}


def rows_per_block(D, K, cov, tied, dtype=torch.float32):
    import zuko_amd._C as C
    from zuko_amd import ops

    r = ctypes.c_int(0)
    assert C.lib().zk_gmm_launch_geometry(DTYPES[dtype], D, K, ops.GMM_COVARIANCE[cov], int(tied), ctypes.byref(r)) == 0
    return r.value


@functools.lru_cache(maxsize=None)
def reference(D, K, cov, tied, N, seed=0):
    """x, phi, g (float32, CPU) and gmm_ref's log_prob / gphi / gx of sum(g * log_prob) in float32 and float64."""
    gen = torch.Generator().manual_seed(1000 * D + 10 * K + seed)
    phi = gmm_ref.random_phi(N, D, K, cov, tied, gen)
    x = 2.5 * torch.randn(N, D, generator=gen)
    g = torch.randn(N, generator=gen)
    out = {"x": x, "phi": phi, "g": g}
    for dtype in DTYPES:
        xt, pt = x.to(dtype).requires_grad_(), phi.to(dtype).requires_grad_()
        lp = gmm_ref.log_prob(xt, pt, D, K, cov, tied)
        gp, gx = torch.autograd.grad((lp * g.to(dtype)).sum(), (pt, xt))
        out[dtype] = (lp.detach(), gp, gx)
    return out


def check(got, ref, dtype, what, k):
    if dtype == torch.float64:
        assert_f64(got, ref[torch.float64][k][: got.shape[0]], what)
    else:
        n = got.shape[0]
        assert_parity(got, ref[torch.float32][k][:n], ref[torch.float64][k][:n], what)


def run_backward(x, phi, g, K, cov, tied):
    x, phi = x.detach().requires_grad_(), phi.detach().requires_grad_()
    from zuko_amd import ops

    lp = ops.gmm_log_prob(x, phi, K, cov, tied, 1e-6)
    gphi, gx = torch.autograd.grad((lp * g).sum(), (phi, x))
    return lp.detach(), gphi, gx


@pytest.mark.parametrize("name", CASES)
def test_fixture_parity(dev, name):
    """The recorded results of the live reference, through ops.gmm_log_prob and GmmLogProbFn, in both precisions."""
    from zuko_amd import autograd as AG

    f = golden(name + ".npz")
    N, D, K, cov, tied = (int(v) for v in f["meta"])
    cov, tied = gmm_ref.COVARIANCES[cov], bool(tied)
    for dtype in DTYPES:
        x, phi = T(f["x"], dev).to(dtype).requires_grad_(), T(f["phi"], dev).to(dtype).requires_grad_()
        lp = AG.GmmLogProbFn.apply(x, phi, K, cov, tied, 1e-6)
        gphi, gx = torch.autograd.grad((lp * T(f["g"], dev).to(dtype)).sum(), (phi, x))
        for got, key in ((lp.detach(), "log_prob"), (gphi, "gphi"), (gx, "gx")):
            if dtype == torch.float64:
                assert_f64(got, f[key + "64"], f"{name} f64: {key}")
            else:
                assert_parity(got, f[key + "32"], f[key + "64"], f"{name} f32: {key}")


@pytest.mark.parametrize("cov,tied", COMBOS)
@pytest.mark.parametrize("D,K", SHAPES)
def test_envelope(dev, D, K, cov, tied):
    """Forward at N in {1, R - 1, R + 1, 3 R + 1} (R = rows per block of the launch), backward at 3 R + 1, float32 and float64.  (33, 3): total = 1 785
    leaves rows misaligned for 16-byte loads; (64, 2) and (4, 64) are the edges of the envelope."""
    from zuko_amd import ops

    assert ops.gmm_supported(D, K, cov, tied)
    nmax = 3 * rows_per_block(D, K, cov, tied) + 1
    ref = reference(D, K, cov, tied, nmax)
    for dtype in DTYPES:
        R = rows_per_block(D, K, cov, tied, dtype)
        x, phi, g = (ref[k].to(dev, dtype) for k in ("x", "phi", "g"))
        tag = f"gmm envelope D={D} K={K} {cov}{' tied' if tied else ''} {'f64' if dtype == torch.float64 else 'f32'}"
        for N in sorted({1, max(R - 1, 1), R + 1, 3 * R + 1}):
            lp = ops.gmm_log_prob(x[:N], phi[:N], K, cov, tied, 1e-6)
            check(lp, ref, dtype, f"{tag}: log_prob N={N}", 0)
        N = 3 * R + 1
        lp, gphi, gx = run_backward(x[:N], phi[:N], g[:N], K, cov, tied)
        check(lp, ref, dtype, f"{tag}: log_prob under autograd", 0)
        check(gphi, ref, dtype, f"{tag}: gphi", 1)
        check(gx, ref, dtype, f"{tag}: gx", 2)


@pytest.mark.parametrize("cov,tied", [("full", False), ("full", True), ("spherical", False)])
def test_strides(dev, cov, tied):
    """phi as a column slice of a wider tensor (ld_phi = total + 3), x and gx as column slices: same bits as the packed call; nothing outside is written."""
    from zuko_amd import ops

    D, K = 5, 4
    N = 2 * rows_per_block(D, K, cov, tied) + 3
    ref = reference(D, K, cov, tied, N, seed=1)
    total = gmm_ref.total(D, K, cov, tied)
    x, phi, g = ref["x"].to(dev), ref["phi"].to(dev), ref["g"].to(dev)
    wide_phi = torch.full((N, total + 3), float("nan"), device=dev)
    wide_phi[:, 1 : 1 + total] = phi
    wide_x = torch.full((N, D + 2), float("nan"), device=dev)
    wide_x[:, 2:] = x
    lp = ops.gmm_log_prob(x, phi, K, cov, tied, 1e-6)
    lp_s = ops.gmm_log_prob(wide_x[:, 2:], wide_phi[:, 1 : 1 + total], K, cov, tied, 1e-6)
    assert torch.equal(lp, lp_s)
    check(lp_s, ref, torch.float32, f"gmm strides {cov}: log_prob", 0)
    gx, gphi = ops.gmm_backward(x, phi, g, K, cov, tied)
    wide_gx = torch.full((N, D + 3), 7.0, device=dev)
    wide_gphi = torch.full((N, total + 3), 7.0, device=dev)
    gx_s, gphi_s = ops.gmm_backward(wide_x[:, 2:], wide_phi[:, 1 : 1 + total], g, K, cov, tied, gx=wide_gx[:, 1 : 1 + D], gphi=wide_gphi[:, 3:])
    assert torch.equal(gx_s, gx) and torch.equal(gphi_s, gphi)
    assert bool((wide_gx[:, 0] == 7).all()) and bool((wide_gx[:, 1 + D :] == 7).all()) and bool((wide_gphi[:, :3] == 7).all())
    check(gphi_s, ref, torch.float32, f"gmm strides {cov}: gphi", 1)
    check(gx_s, ref, torch.float32, f"gmm strides {cov}: gx", 2)
    # one gradient only
    only_x, none = ops.gmm_backward(x, phi, g, K, cov, tied, need_phi=False)
    assert none is None and torch.equal(only_x, gx)
    none, only_phi = ops.gmm_backward(x, phi, g, K, cov, tied, need_x=False)
    assert none is None and torch.equal(only_phi, gphi)


@pytest.mark.parametrize("cov,tied", COMBOS)
def test_shared_row(dev, cov, tied):
    """ld_phi = 0 through the unconditional module at N = 3 R + 1: log_prob, and the parameter gradients (a sum over rows: per-block partial sums, then
    one sum over the blocks) against float64; two runs give the same bits."""
    from zuko_amd.mixtures import GMM

    D, K = 5, 4
    torch.manual_seed(3)
    m = GMM(D, components=K, covariance_type=cov, tied=tied)
    N = 3 * rows_per_block(D, K, cov, tied) + 1
    gen = torch.Generator().manual_seed(4)
    x, g = 2.0 * torch.randn(N, D, generator=gen), torch.randn(N, generator=gen)
    refs = {}
    for dtype in DTYPES:
        ps = [p.detach().to(dtype).requires_grad_() for p in m.phi]
        lp = gmm_ref.log_prob(x.to(dtype), torch.cat([p.flatten() for p in ps]), D, K, cov, tied)
        refs[dtype] = (lp.detach(), torch.autograd.grad((lp * g.to(dtype)).sum(), ps))
    m = m.to(dev)
    runs = []
    for _ in range(2):
        m.zero_grad()
        lp = m().log_prob(x.to(dev))
        (lp * g.to(dev)).sum().backward()
        runs.append([p.grad.clone() for p in m.phi])
    assert_parity(lp.detach(), refs[torch.float32][0], refs[torch.float64][0], f"gmm shared row {cov}: log_prob")
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), f"phi.{i}: two runs differ"
        assert_parity(a, refs[torch.float32][1][i], refs[torch.float64][1][i], f"gmm shared row {cov}{' tied' if tied else ''}: grad phi.{i}")
    m64 = m.double()
    m64.zero_grad()
    (m64().log_prob(x.to(dev).double()) * g.to(dev).double()).sum().backward()
    for i, p in enumerate(m64.phi):
        assert_f64(p.grad, refs[torch.float64][1][i], f"gmm shared row {cov} f64: grad phi.{i}", tol=1e-11)


@pytest.mark.parametrize("cov,tied", [("full", False), ("full", True), ("diagonal", False), ("spherical", True)])
def test_row_independence(dev, cov, tied):
    """Rows 0 .. R of an N = 3 R + 1 batch, evaluated alone, give the same bits: log_prob, gphi and gx."""
    D, K = 5, 4
    R = rows_per_block(D, K, cov, tied)
    ref = reference(D, K, cov, tied, 3 * R + 1, seed=2)
    x, phi, g = ref["x"].to(dev), ref["phi"].to(dev), ref["g"].to(dev)
    whole = run_backward(x, phi, g, K, cov, tied)
    part = run_backward(x[: R + 1], phi[: R + 1], g[: R + 1], K, cov, tied)
    for a, b, what in zip(whole, part, ("log_prob", "gphi", "gx")):
        assert torch.equal(a[: R + 1], b), what
    again = run_backward(x, phi, g, K, cov, tied)
    assert all(torch.equal(a, b) for a, b in zip(whole, again))


@pytest.mark.parametrize("cov", gmm_ref.COVARIANCES)
def test_non_finite_rows(dev, cov):
    """NaN and infinity patterns of the reference row by row (assert_parity demands identical patterns); clean rows keep their bits."""
    from zuko_amd import ops

    D, K = 5, 4
    ref = reference(D, K, cov, False, 8, seed=3)
    x, phi = ref["x"].clone(), ref["phi"].clone()
    x[0, 2] = float("nan")
    x[1] = 1e30
    x[2] = 1e3
    phi[3, 1] = float("-inf")
    phi[4, :K] = float("-inf")
    phi[5, K + D + 1] = float("nan")  # loc of component 1
    clean = [7]
    if cov != "full":
        x[6, 0] = float("inf")  # (full covariance: inf - inf in the substitution, order-dependent: the row stays finite there)
    else:
        clean.append(6)
    r32 = gmm_ref.log_prob(x, phi, D, K, cov, False)
    r64 = gmm_ref.log_prob(x.double(), phi.double(), D, K, cov, False)
    # the pattern the reference was seen to give: NaN, -inf, about -2e6 (here: a large finite negative), finite, NaN, NaN, (-inf), finite
    assert r32[[0, 4, 5]].isnan().all() and r32[1] == float("-inf") and torch.isfinite(r32[[2, 3, 7]]).all() and r32[2] < -1e4
    assert r32[6] == float("-inf") if cov != "full" else torch.isfinite(r32[6])
    lp = ops.gmm_log_prob(x.to(dev), phi.to(dev), K, cov, False, 1e-6)
    assert_parity(lp, r32, r64, f"gmm non-finite rows {cov}")
    lp_clean = ops.gmm_log_prob(ref["x"].to(dev), ref["phi"].to(dev), K, cov, False, 1e-6)
    assert torch.equal(lp[clean], lp_clean[clean])
    lp64 = ops.gmm_log_prob(x.to(dev).double(), phi.to(dev).double(), K, cov, False, 1e-6)
    assert_f64(lp64, r64, f"gmm non-finite rows {cov} f64")


@pytest.mark.parametrize("name,kw", [("flow_gmm_small", dict(features=5, context=3, components=4)), ("flow_gmm_uncond", dict(features=3, components=5))])
def test_module_against_the_reference(dev, name, kw):
    """The hash-checked seeded weights: log_prob at the parity bar, d log_prob.mean() / d parameter against the reference's float64 gradients within 2e-4 of
    max |grad| per tensor (the bar of tests/test_gpu_backward.py: the conditional model's MLP trains on the tile GEMMs)."""
    from zuko_amd.mixtures import GMM

    f = golden(name + ".npz")
    torch.manual_seed(11)
    m = GMM(**kw)
    assert sd_hash(m.state_dict()) == f["hash"].tobytes().decode()
    m = m.to(dev)
    x, c = T(f["x"], dev), (T(f["c"], dev) if "c" in f else None)
    lp = m(c).log_prob(x)
    assert_parity(lp.detach(), f["log_prob32"], f["log_prob64"], f"{name}: log_prob")
    lp.mean().backward()
    for k, p in m.named_parameters():
        ref = T(f["grad/" + k]).double()
        assert p.grad is not None, k
        d, scale = float((p.grad.double().cpu() - ref).abs().max()), float(ref.abs().max())
        assert d <= 2e-4 * scale, f"{k}: |d| {d:.3e} vs max |grad| {scale:.3e}"


def test_flow_with_a_gmm_base(dev):
    """Flow(transform, GMM): log_prob is base.log_prob(z) + ladj of the same objects; `expand` keeps log_prob; samples have the right shape."""
    import zuko_amd.flows as F
    from zuko_amd.lazy import Flow

    torch.manual_seed(2)
    flow = Flow(F.NSF(3, 2, transforms=2).transform, F.GMM(3, 2, components=3)).to(dev)
    gen = torch.Generator().manual_seed(5)
    x, c = torch.randn(70, 3, generator=gen).to(dev), torch.randn(70, 2, generator=gen).to(dev)
    with torch.no_grad():
        d = flow(c)
        z, ladj = d.transform.call_and_ladj(x)
        assert torch.equal(d.log_prob(x), flow.base(c).log_prob(z) + ladj)
        base = flow.base(c)
        assert base.batch_shape == (70,) and base.event_shape == (3,)
        assert torch.equal(base.expand((70,)).log_prob(z), base.log_prob(z))
        s = d.sample((7,))
        assert s.shape == (7, 70, 3) and bool(torch.isfinite(s).all())
        s = base.sample((7,))
        assert s.shape == (7, 70, 3) and bool(torch.isfinite(s).all())
        # the unconditional model: one shared row stays shared under expand
        u = F.GMM(3, components=5).to(dev)()
        e = u.expand((70,))
        assert u.batch_shape == () and e.batch_shape == (70,) and e.phi.dim() == 1
        assert torch.equal(e.log_prob(z), u.log_prob(z))
        assert u.sample((7,)).shape == (7, 3) and e.sample((2,)).shape == (2, 70, 3) and u.sample().shape == (3,)
        assert bool(torch.isfinite(e.sample((2,))).all())
    # training through the flow reaches the base's MLP
    flow(c).log_prob(x).mean().backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in flow.parameters())


def test_fallback(dev):
    """D = 65, and sample dimensions over a batch of mixtures, run the torch-op path: gmm_ref's values and gradients."""
    from zuko_amd import ops

    assert not ops.gmm_supported(65, 2, "diagonal", False) and not ops.gmm_supported(3, 65, "full", False)
    for D, K, cov, lead in ((65, 2, "diagonal", ()), (4, 3, "full", (3,))):
        N = 9
        gen = torch.Generator().manual_seed(D)
        phi = gmm_ref.random_phi(N, D, K, cov, False, gen)
        x = 2.5 * torch.randn(*lead, N, D, generator=gen)
        if lead:
            assert not ops._gmm_kernel_serves(x.to(dev), phi.to(dev), K, cov, False)
        outs = []
        for device, dtype in (("cpu", torch.float32), ("cpu", torch.float64), (dev, torch.float32)):
            xt, pt = x.to(device, dtype).clone().requires_grad_(), phi.to(device, dtype).clone().requires_grad_()
            lp = (gmm_ref.log_prob if device == "cpu" else lambda *a: ops.gmm_log_prob(a[0], a[1], a[3], a[4], a[5]))(xt, pt, D, K, cov, False)
            assert lp.shape == (*lead, N)
            outs.append((lp.detach(),) + torch.autograd.grad(lp.sum(), (pt, xt)))
        for r32, r64, got, what in zip(*outs, ("log_prob", "gphi", "gx")):
            assert_parity(got, r32, r64, f"gmm fallback D={D}: {what}")
    # double backward is the torch-op path's: the kernel path refuses it
    ops.GMM_KERNEL = False
    try:
        xt = x[0].detach().to(dev).requires_grad_()
        (gx,) = torch.autograd.grad(ops.gmm_log_prob(xt, phi.to(dev), K, cov, False).sum(), xt, create_graph=True)
        gx.square().sum().backward()
        assert xt.grad is not None and bool(torch.isfinite(xt.grad).all())
    finally:
        ops.GMM_KERNEL = True
