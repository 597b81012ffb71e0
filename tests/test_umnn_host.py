"""CPU: the unconstrained neural autoregressive flow's host side — module tree / state_dict / seeds against the reference's fixtures
(tests/golden/make_golden_unaf.py), the torch restatement the GPU tests use as reference (tests/umnn_ref.py) against the same fixtures, the
signed weight image walked by a numpy emulator of the kernel's tile order and pairing, and the argument-block checks of zk_umnn_forward /
zk_umnn_inverse.  No kernel is launched."""

import ctypes

import numpy as np
import pytest
import torch

import umnn_emulator
import umnn_ref
from conftest import T, golden, sd_hash

CASES = {"umnn_a": (16, (64, 64), 31), "umnn_b": (3, (32,), 32), "umnn_c": (7, (16, 48, 128), 33), "umnn_d": (16, (30, 30), 34), "umnn_e": (16, (64, 64), 35)}
UNAF_KW, UNAF_SEED = dict(features=5, context=3, transforms=2), 11


def test_unaf_module_tree_state_dict_and_seed_match_the_reference():
    import torch.nn as nn

    import zuko_amd.flows as F
    from zuko_amd.nn import MLP, Linear

    g = golden("flow_unaf_small.npz")
    torch.manual_seed(UNAF_SEED)
    flow = F.UNAF(**UNAF_KW)
    sd = flow.state_dict()
    assert sd_hash(sd) == bytes(g["hash"]).decode()
    assert [k for k, _ in flow.named_parameters()] == list(g["param_names"])
    assert {"transform.transforms.0.order", "transform.transforms.0.hyper.0.mask", "transform.transforms.0.univariate.integrand.0.weight",
            "transform.transforms.2.univariate.integrand.4.bias", "base.loc", "base.scale"} <= set(sd)
    assert tuple(sd["transform.transforms.0.univariate.integrand.0.weight"].shape) == (5, 64, 17)
    assert tuple(sd["transform.transforms.0.hyper.4.weight"].shape) == (5 * 17, 64)
    layer = flow.transform.transforms[0]
    assert [tuple(s) for s in layer.shapes] == [(16,), ()] and layer.univariate.per_feature
    net = layer.univariate.integrand
    assert type(net) is MLP and [type(m) for m in net] == [Linear, nn.ELU, Linear, nn.ELU, Linear]
    assert "stack=5" in repr(net[0])
    assert [type(t).__name__ for t in flow.transform.transforms] == ["MaskedAutoregressiveTransform", "UnconditionalTransform", "MaskedAutoregressiveTransform"]
    assert flow.transform.transforms[2].order.tolist() == [4, 3, 2, 1, 0]
    torch.manual_seed(UNAF_SEED + 100)
    other = F.UNAF(**UNAF_KW)
    assert sd_hash(other.state_dict()) != sd_hash(sd)
    other.load_state_dict(sd)
    assert sd_hash(other.state_dict()) == sd_hash(sd)
    assert isinstance(F.UNAF(1, 2, transforms=1).transform.transforms[0], F.ElementWiseTransform)


@pytest.mark.parametrize("name", list(CASES))
def test_umnn_parameters_and_integrand_equal_the_reference_under_the_same_seed(name):
    """The parameters are the fixture's; UMNN.g, the module tree's own torch-op forward (a STACKED plain MLP: its activations must be applied),
    is the reference's integrand: exp(ladj)."""
    from zuko_amd.flows import UMNN

    S, hidden, seed = CASES[name]
    g = golden(name + ".npz")
    torch.manual_seed(seed)
    m = UMNN(signal=S, stack=g["x"].shape[1], hidden_features=hidden)
    lins = [l for l in m.integrand if hasattr(l, "weight")]
    if name == "umnn_e":
        with torch.no_grad():
            lins[-1].weight.mul_(30.0)
            lins[-1].bias.mul_(30.0)
    for i, l in enumerate(lins):
        assert np.array_equal(l.weight.detach().numpy(), g[f"w{i}"]) and np.array_equal(l.bias.detach().numpy(), g[f"b{i}"])
    with torch.no_grad():
        gx = m.g(T(g["signal"]), T(g["x"]))
    assert torch.allclose(gx, T(g["ladj32"]).exp(), rtol=1e-5, atol=1e-5)
    m.train()  # with gradients on, the same modules one by one
    assert torch.allclose(m.g(T(g["signal"]), T(g["x"])).detach(), T(g["ladj32"]).exp(), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", list(CASES))
def test_umnn_ref_reproduces_the_fixtures(name):
    g = golden(name + ".npz")
    for dtype, tag, tol in ((torch.float64, "64", 1e-12), (torch.float32, "32", 1e-5)):
        W, B = umnn_ref.params_of(g, dtype=dtype)
        x, sig, cst = T(g["x"]).to(dtype), T(g["signal"]).to(dtype), T(g["constant"]).to(dtype)
        y, ladj = umnn_ref.forward(W, B, x, sig, cst)
        got = [(y, "y"), (ladj, "ladj")]
        if "targets" in g:
            got.append((umnn_ref.inverse(W, B, T(g["targets"]).to(dtype), sig, cst), "inv"))
        for val, key in got:
            ref = T(g[key + tag])
            d = float((val - ref).abs().max())
            print(f"{name} {key}{tag}: max |d| {d:.3e}")
            # (umnn_e: |y| reaches 1.8e3, the relative term of the bar is the one at work there)
            assert val.dtype == ref.dtype and torch.allclose(val, ref, rtol=tol, atol=tol), f"{name} {key}{tag}: {d:.3e}"
    # a column selection picks the networks of those features
    W, B = umnn_ref.params_of(g, dtype=torch.float64)
    x, sig, cst = T(g["x"]).double(), T(g["signal"]).double(), T(g["constant"]).double()
    y, ladj = umnn_ref.forward(W, B, x[:, [2, 1]], sig[:, [2, 1]], cst[:, [2, 1]], feat=[2, 1])
    assert torch.allclose(y, T(g["y64"])[:, [2, 1]], rtol=1e-12, atol=1e-12) and torch.allclose(ladj, T(g["ladj64"])[:, [2, 1]], rtol=1e-12, atol=1e-12)
    if "targets" in g:  # the targets of rows 0 and 1 lie outside f(+-bound) + constant: the bisection ends at the interval's ends
        assert np.all(g["inv32"][0] == 10.0) and np.all(g["inv32"][1] == -10.0)
    else:  # the stiff integrand: the squash is at work on both sides
        assert g["ladj64"].min() < -5 and g["ladj64"].max() > 5


@pytest.mark.parametrize("S,widths,n_quad", [(16, (64, 64), 32), (3, (32,), 5), (7, (16, 48, 128), 32)])
def test_signed_weight_image_walked_in_the_kernels_order_reproduces_umnn_ref(S, widths, n_quad):
    """Host index table applied to random SIGNED weights -> image; the emulator reads it exactly where the kernel does and pairs the quadrature's
    points as the kernel does (an even and an odd number of them).  Covers the K padding of the signal product (S = 3, 7), rectangular tiles, three
    layers, the place of the constant, and the inverse."""
    from zuko_amd import mnn_plan

    F, n = 3, 21
    rng = np.random.default_rng(S)
    dims = [1 + S, *widths, 1]
    W = [rng.uniform(-1, 1, (F, b, a)) / np.sqrt(a) for a, b in zip(dims[:-1], dims[1:])]
    B = [rng.uniform(-1, 1, (F, b)) / np.sqrt(a) for a, b in zip(dims[:-1], dims[1:])]
    L = mnn_plan.layout(S, widths)
    idx = mnn_plan.index_table(S, widths, F)
    flat = np.concatenate([w.reshape(-1) for w in W] + [b.reshape(-1) for b in B])
    assert any((w < 0).any() for w in W)
    images = np.where(idx < 0, 0.0, flat[np.maximum(idx, 0)])
    x = rng.uniform(-9.5, 9.5, (n, F))
    sig = 1.5 * rng.standard_normal((n, F, S))
    cst = rng.standard_normal((n, F))
    Wt, Bt = [T(w) for w in W], [T(b) for b in B]
    y_ref, ladj_ref = umnn_ref.forward(Wt, Bt, T(x), T(sig), T(cst), n=n_quad)
    nodes, weights = (v.numpy() for v in umnn_ref.rule(n_quad, T(x)))
    for f in range(F):
        y, ladj = umnn_emulator.evaluate(images[f], L, x[:, f], sig[:, f], cst[:, f], nodes, weights)
        assert np.allclose(y, y_ref[:, f].numpy(), rtol=1e-12, atol=1e-12), f"feature {f}: y"
        assert np.allclose(ladj, ladj_ref[:, f].numpy(), rtol=1e-12, atol=1e-12), f"feature {f}: ladj"
    inv_ref = umnn_ref.inverse(Wt, Bt, y_ref[:, :1], T(sig)[:, :1], T(cst)[:, :1], feat=[0], n=n_quad)
    inv = umnn_emulator.invert(images[0], L, y_ref[:, 0].numpy(), sig[:, 0], cst[:, 0], nodes, weights)
    assert np.allclose(inv, inv_ref[:, 0].numpy(), rtol=1e-12, atol=1e-12)
    assert np.abs(inv - x[:, 0]).max() < 1e-5


def test_flat_parameters_are_signed_for_a_umnn_and_absolute_for_an_mnn():
    from zuko_amd import mnn_plan
    from zuko_amd.flows import MNN, UMNN

    torch.manual_seed(0)
    u, m = UMNN(signal=4, stack=3, hidden_features=(16,)).integrand, MNN(signal=4, stack=3, hidden_features=(16,)).network
    assert mnn_plan.is_signed(u) and not mnn_plan.is_signed(m)
    assert mnn_plan.shape_of(u) == mnn_plan.shape_of(m) == (4, (16,), 3)
    fu, fm = mnn_plan.flat_parameters(u), mnn_plan.flat_parameters(m)
    assert fu.shape == fm.shape and bool((fu[: 3 * 16 * 5] < 0).any()) and bool((fm[: 3 * 16 * 5] >= 0).all())
    assert torch.equal(fu[: 3 * 16 * 5], u[0].weight.detach().reshape(-1))


def test_supported_predicate_agrees_with_the_library():
    import zuko_amd._C as C
    from zuko_amd import ops

    lib = C.lib()
    for S, widths in [(16, (64, 64)), (3, (32,)), (7, (16, 48, 128)), (63, (128, 128)), (1, (16,)), (16, (128, 128, 64)), (16, (128, 128, 128)), (16, (30, 30)),
                      (64, (64,)), (0, (64,)), (16, (144,)), (16, (64, 64, 64, 64)), (16, ())]:
        w = list(widths[:3]) + [0] * (3 - min(3, len(widths)))
        assert ops.umnn_supported(S, widths) == (lib.zk_mnn_image_floats(S, len(widths), *w) > 0), (S, widths)
    assert ops.umnn_supported(16, (64, 64)) and not ops.umnn_supported(16, (30, 30))


def test_umnn_entry_points_reject_foreign_blocks_and_unsupported_shapes_without_a_device():
    import zuko_amd._C as C

    lib, EINVAL = C.lib(), 1
    text = open(C._HEADER).read()
    for sym in ("zk_umnn_forward", "zk_umnn_inverse"):
        assert sym in text and sym in C.SIGNATURES and hasattr(ctypes.CDLL(C.LIB_PATH), sym)
    assert "zk_umnn_args_v1" in C.STRUCTS

    def block(**kw):
        base = dict(S=16, n_hidden=2, width0=64, width1=64, width2=0, n_features=5, image_floats=lib.zk_mnn_image_floats(16, 2, 64, 64, 0), N=0, Dsel=5, ldx=5,
                    ld_signal=85, ld_col=17, ldy=5, ld_constant=85, ld_constant_col=17, n_quad=32, n_bisect=25, bound=10.0)
        base.update(kw)
        return C.args("zk_umnn_args_v1", **base)

    for fn in (lib.zk_umnn_forward, lib.zk_umnn_inverse):
        assert fn(block(), None) == 0  # (a well-formed block over zero rows: accepted, nothing to launch — with every pointer null)
        assert fn(block(ld_col=16, ld_signal=80), None) == 0 and fn(block(n_quad=1), None) == 0 and fn(block(n_quad=64), None) == 0
        bad = block()
        bad.struct_size -= 8
        assert fn(bad, None) == EINVAL
        bad = block()
        bad.struct_size += 8
        assert fn(bad, None) == EINVAL
        bad = block()
        bad.version = 2
        assert fn(bad, None) == EINVAL
        assert fn(None, None) == EINVAL
        for kw in (dict(n_quad=0), dict(n_quad=65), dict(ld_col=15), dict(ld_signal=83), dict(width0=30, width1=30), dict(width0=144), dict(width1=0), dict(n_hidden=4),
                   dict(n_hidden=0), dict(S=0), dict(S=64), dict(image_floats=1), dict(n_hidden=3, width0=128, width1=128, width2=128), dict(ldy=4), dict(Dsel=0),
                   dict(N=-1), dict(n_features=0), dict(ld_constant=-1), dict(ld_constant_col=-1), dict(Dsel=(1 << 20) + 1, ldy=1 << 21, ld_signal=1 << 25)):
            assert fn(block(**kw), None) == EINVAL, kw
        assert fn(block(N=4), None) == EINVAL  # (rows but no pointers)
    assert lib.zk_umnn_forward(block(Dsel=1 << 20, ldy=1 << 21, ld_signal=1 << 25), None) == 0  # (the largest column count)
    # the bisection's parameters are the inverse's alone
    assert lib.zk_umnn_inverse(block(bound=0.0), None) == EINVAL and lib.zk_umnn_inverse(block(n_bisect=65), None) == EINVAL
    assert lib.zk_umnn_inverse(block(n_bisect=64), None) == 0 and lib.zk_umnn_forward(block(n_bisect=65, bound=0.0), None) == 0


def test_other_activations_are_not_served():
    import torch.nn as nn

    from zuko_amd import mnn_plan
    from zuko_amd.flows import UMNN

    assert mnn_plan.shape_of(UMNN(signal=4, stack=3, hidden_features=(16, 16)).integrand) == (4, (16, 16), 3)
    for act in (nn.Tanh, nn.ReLU, lambda: nn.ELU(alpha=0.5)):
        net = UMNN(signal=4, stack=3, hidden_features=(16, 16), activation=act).integrand
        assert mnn_plan.shape_of(net) is None and mnn_plan.image_of(net, "cpu") is None


def test_cpu_tensors_are_rejected():
    from zuko_amd import ops
    from zuko_amd.flows import UMNN, UNAF

    flow = UNAF(3, 2, transforms=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        flow(torch.randn(4, 2)).log_prob(torch.randn(4, 3))
    m = UMNN(signal=4, stack=3, hidden_features=(16,))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.randn(7, 3, 4), torch.randn(7, 3))(torch.randn(7, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.umnn_inverse(torch.randn(7, 3), torch.randn(7, 3, 4), None, m.integrand)


def test_invalidate_drops_the_weight_image():
    import zuko_amd
    from zuko_amd.flows import UNAF

    flow = UNAF(3, 0, transforms=1)
    net = flow.transform.transforms[0].univariate.integrand
    net.__dict__["_mnn_image_cache"] = ("key", object())
    net.__dict__["_mnn_feat_cache"] = {"k": None}
    zuko_amd.invalidate(flow)
    assert "_mnn_image_cache" not in net.__dict__ and "_mnn_feat_cache" not in net.__dict__


def test_fused_plan_probes_return_no_plan_for_the_new_univariate():
    from zuko_amd.flows import UNAF

    layer = UNAF(4, 1, transforms=1).transform.transforms[0]
    assert layer._fusable_layout() is None and layer._rqs_spec() is None
    assert layer.fused_state(torch.device("cpu")) is None and layer.incremental_state(torch.device("cpu")) is None


@pytest.mark.parametrize("randperm,C", [(False, 2), (True, 0)])
def test_wavefront_inverse_hands_the_sweeps_features_and_constants_to_a_per_feature_map(randperm, C):
    """The ordered inverse of a UNAF layer (zuko_amd/flows/autoregressive.py: wavefront_inverse with `with_features=True`) walked on the CPU with torch
    stand-ins, float64: every sweep inverts its own features with THEIR networks and constants (phi unpacked by the layer's shapes), and the result
    is the reference loop's (every feature, every sweep)."""
    import torch.nn.functional as Fn

    import zuko_amd.flows as F
    from zuko_amd.flows.autoregressive import MaskedAutoregressiveTransform, wavefront_inverse
    from zuko_amd.utils import unpack

    torch.manual_seed(6)
    flow = F.UNAF(5, C, transforms=2, randperm=randperm, signal=6, hidden_features=[24, 24], network=dict(hidden_features=(16, 32))).double()
    N, n_quad = 11, 8  # (fewer nodes than the product's 32: the schedule is what is checked)

    def linear(h, w, b, m, act):
        out = Fn.linear(h, w * m, b)
        return out if act is None else act(out)

    for lazy in (t for t in flow.transform.transforms if isinstance(t, MaskedAutoregressiveTransform)):
        assert lazy.univariate.per_feature and lazy.total == 7
        lins = [l for l in lazy.univariate.integrand if hasattr(l, "weight")]
        W, B = [l.weight.detach() for l in lins], [l.bias.detach() for l in lins]
        g = torch.Generator().manual_seed(9)
        y = torch.randn(N, 5, generator=g, dtype=torch.float64) * 0.5
        c = torch.randn(N, C, generator=g, dtype=torch.float64) if C else None
        mods = list(lazy.hyper)
        seen = []

        def inverse_of(phi, ys, idx):
            feat = list(range(*idx)) if isinstance(idx, tuple) else idx.tolist()
            seen.extend(feat)
            signal, constant = unpack(phi, lazy.shapes)
            return umnn_ref.inverse(W, B, ys, signal, constant, feat=feat, n=n_quad)

        with torch.no_grad():
            x_w = wavefront_inverse(lazy, y, c, lazy.passes, linear, inverse_of, with_features=True)
            x_r = torch.zeros_like(y)
            for _ in range(lazy.passes):
                h = x_r if c is None else torch.cat((x_r, c), dim=-1)
                for i in range(0, len(mods) - 1, 2):
                    h = linear(h, mods[i].weight, mods[i].bias, mods[i].mask, mods[i + 1])
                phi = linear(h, mods[-1].weight, mods[-1].bias, mods[-1].mask, None).unflatten(-1, (5, lazy.total))
                x_r = umnn_ref.inverse(W, B, y, phi[..., :6], phi[..., 6], n=n_quad)
            y_back = umnn_ref.forward(W, B, x_w, phi[..., :6], phi[..., 6], n=n_quad)[0]
        assert sorted(seen) == list(range(5)), "every feature inverted exactly once"
        assert (x_w - x_r).abs().max().item() <= 1e-12
        assert (y_back - y).abs().max().item() < 1e-5
