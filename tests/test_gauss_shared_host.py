"""CPU: the host side of the shared-parameter Gaussianization adjoint (zk_gauss_backward_shared, ops.GAUSS_SHARED_ADJOINT).  The two entry points are
declared, bound and exported and refuse what they do not serve before touching a device; the predicate and the route selection of
ops.gauss_forward / ops.gauss_inverse; and the yardstick of tests/test_gpu_gauss_shared.py — gauss_ref.backward summed over the rows — against
float64 autograd on [D, K] parameters.  No kernel is launched."""

import ctypes
import os

import pytest
import torch

import gauss_ref as R
from conftest import ROOT

EINVAL = 1
SYMBOLS = ("zk_gauss_backward_shared_floats", "zk_gauss_backward_shared")


def test_symbols_are_declared_bound_and_exported():
    import zuko_amd._C as C

    text = open(os.path.join(ROOT, "include", "zuko_amd.h")).read()
    lib = ctypes.CDLL(C.LIB_PATH)
    for sym in SYMBOLS:
        assert sym + "(" in text and sym in C.SIGNATURES and hasattr(lib, sym), sym
    assert C.RESTYPES["zk_gauss_backward_shared_floats"] is ctypes.c_int64  # a 64-bit count, not a hipError_t
    assert len(C.SIGNATURES["zk_gauss_backward_shared"]) == 12 and len(C.SIGNATURES["zk_gauss_backward_shared_floats"]) == 3


def test_entry_points_check_their_arguments_without_a_device():
    import zuko_amd._C as C

    lib = C.lib()
    for K in (0, 33, -1):
        assert lib.zk_gauss_backward_shared(4, 2, K, None, None, None, None, 0, None, None, None, None) == EINVAL, K
        assert lib.zk_gauss_backward_shared_floats(4, 2, K) <= 0, K
    # nothing to launch: 0 with every pointer NULL
    assert lib.zk_gauss_backward_shared(0, 2, 8, None, None, None, None, 0, None, None, None, None) == 0
    assert lib.zk_gauss_backward_shared(4, 0, 8, None, None, None, None, 0, None, None, None, None) == 0
    # phi / gphi off a 16-byte boundary (the check precedes every use of the pointers)
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    ok, off = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)
    assert lib.zk_gauss_backward_shared(4, 2, 8, None, off, None, None, 0, None, None, ok, None) == EINVAL
    assert lib.zk_gauss_backward_shared(4, 2, 8, None, ok, None, None, 0, None, None, off, None) == EINVAL
    for shape in ((1, 1, 1), (131, 6, 8), (2**16, 64, 8), (19, 130, 32)):
        assert lib.zk_gauss_backward_shared_floats(*shape) > 0, shape


@pytest.mark.parametrize("D,K", [(1, 1), (6, 8), (64, 8), (130, 32), (5, 3)])
def test_workspace_is_whole_partials_and_does_not_decrease_in_n(D, K):
    from zuko_amd import ops
    import zuko_amd._C as C

    lib = C.lib()
    last = 0
    ns = sorted(set(list(range(1, 700)) + [2**k + d for k in range(10, 24) for d in (-1, 0, 1)] + [8 * 1024 * 40 + d for d in range(-3, 4)]))
    for N in ns:
        floats = lib.zk_gauss_backward_shared_floats(N, D, K)
        assert floats >= last and floats > 0 and floats % (D * 2 * K) == 0, (N, floats, last)
        assert ops.gauss_shared_chunks(N, D, K) == floats // (D * 2 * K)
        last = floats
    # the documented partition: passes of 4 * (64 / min(64, D)) rows, eight to a chunk, at most max(1, 1024 / tiles) chunks
    tiles = (D + 63) // 64
    rows = 4 * (64 // min(64, D))
    for N in (1, 8 * rows, 8 * rows + 1, 16 * rows + 1, 2**22):
        passes = -(-N // rows)
        assert ops.gauss_shared_chunks(N, D, K) == min(-(-passes // 8), max(1, 1024 // tiles)), N
    assert ops.gauss_shared_chunks(100, 6, 33) == 0


def test_predicate():
    from zuko_amd import ops

    N, D, K = 7, 6, 8
    x = torch.zeros(N, D)
    shapes = ops._gauss_shared_shapes
    assert shapes(x, torch.zeros(D, K), torch.zeros(D, K))
    assert shapes(torch.zeros(D), torch.zeros(D, K), torch.zeros(D, K)) and shapes(torch.zeros(2, 3, D), torch.zeros(D, K), torch.zeros(D, K))
    assert shapes(x, torch.zeros(D, 1), torch.zeros(D, 1)) and shapes(x, torch.zeros(D, 32), torch.zeros(D, 32))
    assert shapes(x.bfloat16(), torch.zeros(D, K).bfloat16(), torch.zeros(D, K).bfloat16())
    assert not shapes(x, torch.zeros(1, D, K), torch.zeros(1, D, K))
    assert not shapes(x, torch.zeros(N, D, K), torch.zeros(N, D, K))
    assert not shapes(x, torch.zeros(D + 1, K), torch.zeros(D + 1, K)) and not shapes(x, torch.zeros(1, K), torch.zeros(1, K))
    assert not shapes(x, torch.zeros(D, K), torch.zeros(1, K)) and not shapes(x, torch.zeros(K), torch.zeros(K))
    assert not shapes(x, torch.zeros(D, 33), torch.zeros(D, 33))
    assert not shapes(x.double(), torch.zeros(D, K).double(), torch.zeros(D, K).double())
    assert not shapes(x, torch.zeros(D, K).double(), torch.zeros(D, K).double())
    assert not shapes(torch.zeros(()), torch.zeros(1, K), torch.zeros(1, K))
    # the public predicate also asks for device tensors
    assert not ops.gauss_shared_supported(x, torch.zeros(D, K), torch.zeros(D, K))


def test_route_selection(monkeypatch):
    """ops._gauss_route is what gauss_forward / gauss_inverse branch on; the device clause of the predicate is taken out so that CPU tensors reach
    the switch."""
    from zuko_amd import ops

    monkeypatch.setattr(ops, "gauss_shared_supported", ops._gauss_shared_shapes)
    N, D, K = 7, 6, 8
    x, b, a = torch.zeros(N, D), torch.zeros(D, K), torch.zeros(D, K)
    bn, an = torch.zeros(N, D, K), torch.zeros(N, D, K)
    phi = torch.zeros(N, D, 2 * K)
    assert ops.GAUSS_SHARED_ADJOINT is False  # off by default
    for on in (False, True):
        monkeypatch.setattr(ops, "GAUSS_SHARED_ADJOINT", on)
        assert ops._gauss_route(x, b, a, True) == ("shared" if on else "rows")
        assert ops._gauss_route(x, b, a, False) == "kernel"
        assert ops._gauss_route(x, bn, an, True) == "rows"
        assert ops._gauss_route(x, phi[..., :K], phi[..., K:], True, phi) == "packed"
        assert ops._gauss_route(x, torch.zeros(D, 33), torch.zeros(D, 33), True) == "torch"
        assert ops._gauss_route(x.double(), b.double(), a.double(), True) == "torch"
        assert ops._gauss_route(x.double(), b.double(), a.double(), False) == "kernel"
        monkeypatch.setattr(ops, "GAUSS_KERNEL", False)
        assert ops._gauss_route(x, b, a, True) == "torch" and ops._gauss_route(x, b, a, False) == "torch"
        monkeypatch.setattr(ops, "GAUSS_KERNEL", True)


def test_autograd_nodes_exist():
    from zuko_amd import autograd as AG

    for node in (AG.GaussSharedFn, AG.GaussSharedInverseFn):
        assert issubclass(node, torch.autograd.Function)


def test_summed_closed_form_adjoint_matches_autograd_on_shared_parameters():
    """The yardstick of the GPU tests: gauss_ref.backward on the parameters expanded to every row, summed over the rows, is the gradient of the [D, K]
    parameters."""
    N, D, K = 37, 3, 5
    g = torch.Generator().manual_seed(61)
    x = (1.5 * torch.randn(N, D, generator=g, dtype=torch.float64)).requires_grad_()
    b = torch.randn(D, K, generator=g, dtype=torch.float64).requires_grad_()
    a = (0.5 * torch.randn(D, K, generator=g, dtype=torch.float64)).requires_grad_()
    gy, gl = torch.randn(N, D, generator=g, dtype=torch.float64), torch.randn(N, D, generator=g, dtype=torch.float64)
    y, ladj = R.forward(x, b, a)
    want = torch.autograd.grad((y * gy + ladj * gl).sum(), (x, b, a))
    gx, gb, ga = R.backward(x.detach(), b.detach().expand(N, D, K), a.detach().expand(N, D, K), gy, gl)
    got = (gx, gb.sum(dim=0), ga.sum(dim=0))
    for t in (y, ladj, *want, *got):
        assert bool(torch.isfinite(t).all())
    for name, w, h in zip(("gx", "gb", "ga"), want, got):
        assert h.shape == w.shape and torch.allclose(h, w, rtol=1e-12, atol=1e-12), f"{name}: max |d| {(h - w).abs().max():.3e}"
