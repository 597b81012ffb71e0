"""CPU: the Gaussian mixture model without a kernel launch — tests/gmm_ref.py pinned to the fixtures of the live reference, the closed-form adjoint
of zk_gmm_backward against autograd, the module tree of zuko_amd.mixtures.GMM, `initialize`, and the host side of the C ABI."""

import ctypes
import itertools

import numpy as np
import pytest
import torch

import gmm_ref
from conftest import T, golden, sd_hash

CASES = ["gmm_a", "gmm_b", "gmm_c", "gmm_d", "gmm_e", "gmm_f"]
COMBOS = list(itertools.product(gmm_ref.COVARIANCES, (False, True)))
EINVAL = 1


def case(name):
    f = golden(name + ".npz")
    N, D, K, cov, tied = (int(v) for v in f["meta"])
    return f, N, D, K, gmm_ref.COVARIANCES[cov], bool(tied)


@pytest.mark.parametrize("name", CASES)
def test_ref_matches_the_live_reference(name):
    """float64 to 1e-12; float32 log_prob and gradients BITWISE (gmm_ref runs the same torch ops in the same order as the reference)."""
    f, N, D, K, cov, tied = case(name)
    assert f["phi"].shape == (N, gmm_ref.total(D, K, cov, tied)) and f["phi"].nbytes < 300e3
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        x, phi = T(f["x"]).to(dtype).requires_grad_(), T(f["phi"]).to(dtype).requires_grad_()
        lp = gmm_ref.log_prob(x, phi, D, K, cov, tied)
        gphi, gx = torch.autograd.grad((lp * T(f["g"]).to(dtype)).sum(), (phi, x))
        for got, want in ((lp.detach(), f["log_prob" + tag]), (gphi, f["gphi" + tag]), (gx, f["gx" + tag])):
            want = T(want)
            if dtype == torch.float64:
                assert torch.allclose(got, want, rtol=1e-12, atol=1e-12), f"{name}: max |d| {(got - want).abs().max():.3e}"
            else:
                assert torch.equal(got, want), f"{name}: float32 differs from the reference, max |d| {(got - want).abs().max():.3e}"


@pytest.mark.parametrize("cov,tied", COMBOS)
def test_closed_form_adjoint_matches_autograd(cov, tied):
    D, K, N = 6, 3, 23
    g = torch.Generator().manual_seed(7)
    phi = gmm_ref.random_phi(N, D, K, cov, tied, g, torch.float64).requires_grad_()
    x = (2.5 * torch.randn(N, D, generator=g, dtype=torch.float64)).requires_grad_()
    w = torch.randn(N, generator=g, dtype=torch.float64)
    want_phi, want_x = torch.autograd.grad((gmm_ref.log_prob(x, phi, D, K, cov, tied) * w).sum(), (phi, x))
    got_phi, got_x = gmm_ref.backward(x.detach(), phi.detach(), w, D, K, cov, tied)
    assert torch.allclose(got_phi, want_phi, rtol=1e-11, atol=1e-11), (got_phi - want_phi).abs().max()
    assert torch.allclose(got_x, want_x, rtol=1e-11, atol=1e-11), (got_x - want_x).abs().max()


def test_module_tree_and_seeded_weights():
    import zuko_amd
    from zuko_amd.mixtures import GMM

    assert zuko_amd.flows.GMM is zuko_amd.mixtures.GMM is GMM
    for name, kw in (("flow_gmm_small", dict(features=5, context=3, components=4)), ("flow_gmm_uncond", dict(features=3, components=5))):
        f = golden(name + ".npz")
        torch.manual_seed(11)
        m = GMM(**kw)
        assert sd_hash(m.state_dict()) == f["hash"].tobytes().decode(), name
        assert [k for k, _ in m.named_parameters()] == list(f["param_names"])
        for k, p in m.named_parameters():
            assert tuple(p.shape) == f["grad/" + k].shape
    m = GMM(5, 3, components=4)
    assert list(m.state_dict()) == ["hyper.0.weight", "hyper.0.bias", "hyper.2.weight", "hyper.2.bias", "hyper.4.weight", "hyper.4.bias"]
    assert m.hyper[-1].weight.shape == (m.total, 64) and not hasattr(m, "phi")
    m = GMM(3, components=5)
    assert list(m.state_dict()) == ["phi.0", "phi.1", "phi.2", "phi.3"] and not hasattr(m, "hyper")
    assert [tuple(p.shape) for p in m.phi] == [(5,), (5, 3), (5, 3), (5, 3)]
    with pytest.raises(NotImplementedError, match="Unknown covariance type"):
        GMM(3, components=2, covariance_type="banded")


@pytest.mark.parametrize("cov,tied", COMBOS)
def test_shapes_and_total(cov, tied):
    from zuko_amd.mixtures import GMM

    D, K = 5, 4
    m = GMM(D, components=K, covariance_type=cov, tied=tied)
    lead = 1 if tied else K
    want = [(K,), (K, D), (lead, 1 if cov == "spherical" else D)] + ([(lead, D * (D - 1) // 2)] if cov == "full" else [])
    assert [tuple(s) for s in m.shapes] == want
    assert m.total == sum(int(np.prod(s)) for s in want) == gmm_ref.total(D, K, cov, tied)
    assert (m.components, m.covariance_type, m.tied, m.epsilon) == (K, cov, tied, 1e-6)


@pytest.mark.parametrize("strategy", ["random", "kmeans", "kmeans++"])
def test_initialize(strategy):
    from zuko_amd.mixtures import GMM

    g = torch.Generator().manual_seed(3)
    centers = 4.0 * torch.randn(3, 4, generator=g)
    x = centers[torch.randint(0, 3, (400,), generator=g)] + 0.3 * torch.randn(400, 4, generator=g)
    for cov, tied in COMBOS:
        torch.manual_seed(5)
        m = GMM(4, components=3, covariance_type=cov, tied=tied)
        m.initialize(x, strategy)
        assert [tuple(p.shape) for p in m.phi] == [tuple(s) for s in m.shapes]
        assert all(torch.isfinite(p).all() for p in m.phi)
        assert torch.allclose(m.phi[0].exp().sum(), torch.tensor(1.0), atol=1e-5)
        # the data's own density under the fitted mixture beats a unit normal's by a wide margin
        phi = torch.cat([p.detach().flatten() for p in m.phi])
        assert gmm_ref.log_prob(x, phi, 4, 3, cov, tied).mean() > torch.distributions.Normal(0.0, 1.0).log_prob(x).sum(-1).mean() + 5
        torch.manual_seed(5)
        m = GMM(4, 2, components=3, covariance_type=cov, tied=tied)
        before = m.hyper[-1].weight.detach().clone()
        m.initialize(x, strategy)
        assert torch.equal(m.hyper[-1].weight, before * 1e-2)
        assert m.hyper[-1].bias.shape == (m.total,) and torch.isfinite(m.hyper[-1].bias).all()
    with pytest.raises(NotImplementedError, match="Unknown clustering strategy"):
        m.initialize(x, "spectral")
    with pytest.raises(AssertionError, match="larger than the number of components"):
        m.initialize(x[:3], strategy)


def test_total_and_geometry_queries():
    import zuko_amd._C as C
    from zuko_amd import ops
    from zuko_amd.mixtures import GMM

    lib = C.lib()
    for D, K, (cov, tied) in itertools.product((1, 2, 5, 33, 64), (1, 3, 64), COMBOS):
        code = ops.GMM_COVARIANCE[cov]
        assert lib.zk_gmm_total(D, K, code, int(tied)) == GMM(D, components=K, covariance_type=cov, tied=tied).total == gmm_ref.total(D, K, cov, tied)
        assert ops.gmm_supported(D, K, cov, tied, torch.float32)
        for dtype in (0, 1):
            rows = ctypes.c_int(0)
            assert lib.zk_gmm_launch_geometry(dtype, D, K, code, int(tied), ctypes.byref(rows)) == 0
            assert 1 <= rows.value <= 64 and rows.value & (rows.value - 1) == 0
            n = lib.zk_gmm_workspace_floats(dtype, 1000, D, K, code, int(tied))
            assert n >= lib.zk_gmm_total(D, K, code, int(tied)) and n % lib.zk_gmm_total(D, K, code, int(tied)) == 0
    assert lib.zk_gmm_total(65, 2, 0, 0) == -1 and lib.zk_gmm_total(2, 65, 0, 0) == -1 and lib.zk_gmm_total(0, 2, 0, 0) == -1
    assert lib.zk_gmm_total(2, 2, 3, 0) == -1 and lib.zk_gmm_workspace_floats(0, 0, 2, 2, 0, 0) == -1
    assert not ops.gmm_supported(65, 2, "full", False) and not ops.gmm_supported(2, 65, "full", False)
    assert not ops.gmm_supported(2, 2, "full", False, torch.float16)
    rows = ctypes.c_int(0)
    assert lib.zk_gmm_launch_geometry(0, 65, 2, 0, 0, ctypes.byref(rows)) == EINVAL
    assert lib.zk_gmm_launch_geometry(0, 8, 2, 0, 0, None) == EINVAL


def test_entry_points_reject_bad_blocks_without_a_device():
    """Every rejection happens on the host, before the device is touched: this runs without a GPU.  The pointers are never dereferenced."""
    import zuko_amd._C as C

    lib = C.lib()
    total = lib.zk_gmm_total(5, 4, 0, 0)
    fake = 4096  # a non-NULL address that nothing reads: every block below is refused first

    def block(**kw):
        base = dict(dtype=0, N=8, D=5, K=4, covariance=0, tied=0, epsilon=1e-6, x=fake, ldx=5, phi=fake, ld_phi=total, out=fake, g=fake, gphi=fake, ld_gphi=total,
                    gx=fake, ld_gx=5, work=fake)
        base.update(kw)
        return C.args("zk_gmm_args_v1", **base)

    def both(a, what):
        assert lib.zk_gmm_log_prob(a, None) == EINVAL, what
        assert lib.zk_gmm_backward(a, None) == EINVAL, what

    a = block()
    a.struct_size -= 8
    both(a, "struct_size")
    a = block()
    a.struct_size += 8
    both(a, "struct_size")
    a = block()
    a.version = 2
    both(a, "version")
    a = block()
    a.reserved = 1
    both(a, "reserved")
    for kw in (dict(D=0), dict(D=65), dict(K=0), dict(K=65), dict(N=0), dict(covariance=3), dict(tied=2), dict(dtype=2), dict(ld_phi=total - 1), dict(ld_phi=1),
               dict(ldx=4), dict(x=None), dict(phi=None)):
        both(block(**kw), str(kw))
    assert lib.zk_gmm_log_prob(block(out=None), None) == EINVAL
    for kw in (dict(g=None), dict(gphi=None, gx=None), dict(ld_gphi=total - 1), dict(ld_gx=4), dict(ld_phi=0, work=None)):
        assert lib.zk_gmm_backward(block(**kw), None) == EINVAL, str(kw)
    assert lib.zk_gmm_log_prob(None, None) == EINVAL and lib.zk_gmm_backward(None, None) == EINVAL


def test_cpu_tensors_raise():
    from zuko_amd import ops
    from zuko_amd.mixtures import GMM

    with pytest.raises(RuntimeError, match="HIP device"):
        ops.gmm_log_prob(torch.zeros(4, 3), torch.zeros(4, gmm_ref.total(3, 2, "full", False)), 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        GMM(3, components=5)().log_prob(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.gmm_backward(torch.zeros(4, 3), torch.zeros(4, 11), torch.zeros(4), 2)
