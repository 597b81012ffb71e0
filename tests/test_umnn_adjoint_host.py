"""Host side of the adjoint of the unconstrained monotone networks (zk_umnn_backward): the closed-form reverse sweep the kernel implements against
float64 autograd, the argument block and the entry points, the shape predicate against the library, the geometry / workspace queries and the
backward image of the signed weights.  No GPU."""

import ctypes

import numpy as np
import pytest
import torch

import umnn_adjoint_ref as ref
import umnn_ref
from conftest import T, golden
from mnn_nets import ENVELOPE, draw_inputs, draw_params

EINVAL = 1
SYMBOLS = ("zk_umnn_backward", "zk_umnn_backward_floats", "zk_umnn_backward_geometry", "zk_umnn_backward_workspace_floats")


def _w3(widths):
    return list(widths) + [0] * (3 - len(widths))


def _cases():
    g = golden("umnn_b.npz")
    W, B = umnn_ref.params_of(g)
    yield "umnn_b", W, B, T(g["x"]), T(g["signal"])
    W, B = draw_params(1, (16,), 3, seed=21)
    x, sig, _ = draw_inputs(67, 3, 1, seed=22)
    yield "S1-16", W, B, x, sig


@pytest.mark.parametrize("n_quad", [1, 7])
def test_closed_form_sweep_equals_float64_autograd(n_quad):
    for name, W, B, x, sig in _cases():
        N, D = x.shape
        F = W[0].shape[0]
        gen = torch.Generator().manual_seed(7 + n_quad)
        gy, gl = torch.randn(N, D, generator=gen, dtype=torch.float64), torch.randn(N, D, generator=gen, dtype=torch.float64)
        variants = [(gy, gl, None, slice(None)), (gy, None, None, slice(None)), (None, gl[:, 0].contiguous(), None, slice(None))]
        if F >= 3:
            cols = [2, 0]
            variants.append((gy[:, cols], gl[:, cols], cols, cols))
        for uy, ul, feat, cols in variants:
            xs, ss = x[:, cols], sig[:, cols]
            a = ref.autograd(W, B, xs, ss, uy, ul, feat=feat, n=n_quad, dtype=torch.float64)
            c = ref.closed_form(W, B, xs, ss, uy, ul, feat=feat, n=n_quad, dtype=torch.float64)
            assert ref.all_finite(a)
            for what, ta, tc in [("gx", a["gx"], c["gx"]), ("gsignal", a["gsignal"], c["gsignal"]), *[(f"gW{l}", u, v) for l, (u, v) in enumerate(zip(a["gW"], c["gW"]))],
                                 *[(f"gB{l}", u, v) for l, (u, v) in enumerate(zip(a["gB"], c["gB"]))]]:
                d, scale = float((ta - tc).abs().max()), max(1.0, float(ta.abs().max()))
                assert d <= 1e-12 * scale, f"{name}, n_quad {n_quad}, {what}: |d| {d:.3e} at scale {scale:.3e}"
            if feat is not None:
                for g in a["gW"] + a["gB"]:
                    assert not bool(g[1].any()), "the feature feat does not select"


def test_gx_is_the_integrand_at_the_upper_limit_not_the_derivative_of_the_quadrature_sum():
    W, B = draw_params(1, (16,), 2, seed=3)
    x, sig, _ = draw_inputs(9, 2, 1, seed=4)
    gy = torch.ones(9, 2, dtype=torch.float64)
    g = ref.autograd(W, B, x, sig, gy, None, n=3, dtype=torch.float64)
    Wd, Bd = [w.double() for w in W], [b.double() for b in B]
    assert torch.allclose(g["gx"], torch.exp(umnn_ref.integrand_log(Wd, Bd, x.double(), sig.double())), rtol=1e-13, atol=0)


def test_entry_points_and_block_agree_between_header_binding_and_library():
    import zuko_amd._C as C
    from zuko_amd import mnn_plan

    lib = C.lib()
    text = open(C._HEADER).read()
    for sym in SYMBOLS:
        assert sym in text and sym in C.SIGNATURES and hasattr(ctypes.CDLL(C.LIB_PATH), sym), sym
    assert "zk_umnn_bwd_args_v1" in C.STRUCTS and "zk_umnn_bwd_args_v1" in text and C._VERSION["zk_umnn_bwd_args_v1"] == 1
    fields = [f for f, _ in C.STRUCTS["zk_umnn_bwd_args_v1"]._fields_]
    base = [f for f, _ in C.STRUCTS["zk_mnn_bwd_args_v1"]._fields_ if f != "reserved"]
    for name in base + ["n_quad", "quad", "ld_col"]:
        assert name in fields, name
    # 12 x 4 bytes, 9 x 8 bytes of sizes and strides, 13 pointers
    assert ctypes.sizeof(C.STRUCTS["zk_umnn_bwd_args_v1"]) == 12 * 4 + 9 * 8 + 13 * 8
    Bl = mnn_plan.layout_backward(16, (64, 64))

    def block(**kw):
        base = dict(S=16, n_hidden=2, width0=64, width1=64, width2=0, n_features=5, image_floats=Bl.total, grad_floats=Bl.g_total, n_quad=32, N=0, Dsel=5, ldx=5,
                    ld_signal=84, ld_col=17, ld_gx=5, ld_gsignal=80, flat_total=100, flat_weights=60)
        base.update(kw)
        return C.args("zk_umnn_bwd_args_v1", **base)

    fn = lib.zk_umnn_backward
    assert fn(block(), None) == 0  # (the library's struct size is the header's; zero rows with every pointer null: accepted, nothing to launch)
    for delta in (-8, 8):
        bad = block()
        bad.struct_size += delta
        assert fn(bad, None) == EINVAL
    bad = block()
    bad.version = 2
    assert fn(bad, None) == EINVAL and fn(None, None) == EINVAL
    for kw in (dict(width0=30, width1=30), dict(width0=128), dict(width1=80), dict(width1=0), dict(n_hidden=4), dict(n_hidden=0), dict(S=0), dict(S=64), dict(image_floats=1),
               dict(image_floats=mnn_plan.layout(16, (64, 64)).total), dict(grad_floats=1), dict(ld_signal=83), dict(ld_col=15), dict(ldx=0), dict(Dsel=0),
               dict(Dsel=65536, ld_signal=1 << 22), dict(N=-1), dict(n_features=0), dict(n_quad=0), dict(n_quad=65)):
        assert fn(block(**kw), None) == EINVAL, kw
    assert fn(block(N=4), None) == EINVAL  # (rows but no pointers)
    one = ctypes.c_void_p(16)  # (never dereferenced: the block is refused first)
    assert fn(block(N=4, x=one, signal=one, image=one), None) == EINVAL  # (no quadrature table)
    assert fn(block(gx=one, ld_gx=4), None) == EINVAL and fn(block(gsignal=one, ld_gsignal=79), None) == EINVAL
    assert fn(block(N=4, x=one, signal=one, image=one, quad=one, gparams=one), None) == EINVAL  # (parameter gradients without table / workspace)
    assert fn(block(N=4, x=one, signal=one, image=one, quad=one, gparams=one, grad_table=one, work=one, flat_total=0), None) == EINVAL
    assert fn(block(N=4, x=one, signal=one, image=one, quad=one, gparams=one, grad_table=one, work=one, flat_weights=101), None) == EINVAL


def test_supported_predicate_agrees_with_the_library_over_the_envelope():
    import zuko_amd._C as C
    from zuko_amd import mnn_plan, ops

    lib = C.lib()
    wide64 = [(1, (64,)), (63, (64,)), (16, (64, 64)), (33, (64, 64)), (63, (64, 64, 64)), (16, (64, 48)), (7, (16, 48, 64))]
    outside = [(16, (30, 30)), (7, (16, 48, 128)), (64, (64,)), (0, (16,)), (16, (80,))]
    served = 0
    for S, widths in ENVELOPE + wide64 + outside:
        a, b = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = lib.zk_umnn_backward_floats(S, len(widths), *_w3(widths), ctypes.byref(a), ctypes.byref(b))
        assert (rc == 0) == ops.umnn_backward_supported(S, widths), (S, widths)
        if rc == 0:
            served += 1
            B = mnn_plan.layout_backward(S, widths)
            assert (a.value, b.value) == (B.total, B.g_total) and ops.umnn_supported(S, widths) and max(widths) <= 64
        else:
            assert rc == EINVAL
    assert served >= len(wide64) + 3  # (the 64-wide set, and the envelope's (1, (16,)), (62, (64,)), (4, (16, 16, 16)), (8, (64, 48)))
    for S, widths in wide64:
        assert ops.umnn_backward_supported(S, widths, 1) and ops.umnn_backward_supported(S, widths, 64)
        assert not ops.umnn_backward_supported(S, widths, 65) and not ops.umnn_backward_supported(S, widths, 0)
    assert lib.zk_umnn_backward_floats(16, 2, 64, 64, 0, None, None) == EINVAL
    assert isinstance(ops.UMNN_ADJOINT, bool) and issubclass(ops.UmnnForwardFn, torch.autograd.Function)


def test_geometry_and_workspace_queries_are_consistent():
    import zuko_amd._C as C
    from zuko_amd import mnn_plan

    lib = C.lib()
    for N, D in [(1, 1), (15, 3), (64, 3), (65, 3), (193, 3), (257, 5), (1 << 14, 64), (1 << 16, 64), (100037, 8), (37, 1030)]:
        r, c = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.zk_umnn_backward_geometry(N, D, ctypes.byref(r), ctypes.byref(c)) == 0
        r2, c2 = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.zk_umnn_backward_geometry(N, D, ctypes.byref(r2), ctypes.byref(c2)) == 0 and (r.value, c.value) == (r2.value, c2.value)
        assert r.value % 64 == 0 and r.value >= 64 and c.value == -(-N // r.value)
        for S, widths in [(16, (64, 64)), (63, (64, 64, 64)), (3, (32,))]:
            v = ctypes.c_int64(-1)
            assert lib.zk_umnn_backward_workspace_floats(N, D, S, len(widths), *_w3(widths), ctypes.byref(v)) == 0
            assert v.value == c.value * D * mnn_plan.layout_backward(S, widths).g_total
    v, r, c = ctypes.c_int64(-1), ctypes.c_int(), ctypes.c_int()
    assert lib.zk_umnn_backward_workspace_floats(0, 5, 16, 2, 64, 64, 0, ctypes.byref(v)) == 0 and v.value == 0
    for N, D in [(0, 3), (-1, 3), (5, 0), (5, 65536)]:
        assert lib.zk_umnn_backward_geometry(N, D, ctypes.byref(r), ctypes.byref(c)) == EINVAL
    assert lib.zk_umnn_backward_workspace_floats(5, 3, 16, 1, 128, 0, 0, ctypes.byref(v)) == EINVAL
    assert lib.zk_umnn_backward_workspace_floats(5, 3, 16, 2, 64, 64, 0, None) == EINVAL


@pytest.mark.parametrize("S,widths", [(1, (16,)), (7, (16, 48, 64)), (63, (64, 64, 64))])
def test_signed_backward_table_holds_the_forward_image_first_and_names_every_weight(S, widths):
    from zuko_amd import mnn_plan

    F = 3
    L, B = mnn_plan.layout(S, widths), mnn_plan.layout_backward(S, widths)
    idx = mnn_plan.index_table_backward(S, widths, F)
    assert idx.shape == (F, B.total) and np.array_equal(idx[:, : L.total], mnn_plan.index_table(S, widths, F))
    w_off, b_off, total = mnn_plan.flat_offsets(S, widths, F)
    named = np.unique(idx[idx >= 0])
    assert np.array_equal(named, np.arange(total)), "the image names every flat parameter"
    behind = np.unique(idx[:, L.total :][idx[:, L.total :] >= 0])
    hidden_weights = np.concatenate([np.arange(w_off[0], w_off[1]).reshape(F, widths[0], 1 + S)[:, :, 1:].reshape(-1), np.arange(w_off[1], w_off[len(widths)])])
    assert np.array_equal(behind, np.unique(hidden_weights)), "the transposed sections: the signal columns of W0 and every hidden-to-hidden weight"


def test_signed_backward_image_is_cached_per_network_kind_and_dropped_by_invalidate():
    import zuko_amd
    from zuko_amd import mnn_plan
    from zuko_amd.flows import MNN, UMNN

    u, m = UMNN(signal=3, stack=2, hidden_features=(16,)), MNN(signal=3, stack=2, hidden_features=(16,))
    assert mnn_plan.is_signed(u.integrand) and not mnn_plan.is_signed(m.network)
    # the kind is checked before anything is built: no device is touched
    assert mnn_plan.backward_image_of(u.integrand, "cpu") is None and mnn_plan.backward_image_of(m.network, "cpu", signed=True) is None
    wide = UMNN(signal=3, stack=2, hidden_features=(128,))
    assert mnn_plan.backward_image_of(wide.integrand, "cpu", signed=True) is None
    u.integrand.__dict__["_mnn_bwd_image_cache"] = ("key", object())
    zuko_amd.invalidate(u)
    assert "_mnn_bwd_image_cache" not in u.integrand.__dict__
