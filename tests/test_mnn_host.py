"""CPU: the neural autoregressive flow's host side — module tree / state_dict / seeds against the reference's fixtures, the torch restatement
the GPU tests use as reference (tests/mnn_ref.py) against the same fixtures, the weight image walked by a numpy emulator of the kernel's tile
order, and the argument-block checks of zk_mnn_forward / zk_mnn_inverse.  No kernel is launched."""

import ctypes

import numpy as np
import pytest
import torch

import mnn_emulator
import mnn_ref
from conftest import T, golden, sd_hash

CASES = {"mnn_a": (16, (64, 64), 21), "mnn_b": (3, (32,), 22), "mnn_c": (7, (16, 48, 128), 23), "mnn_d": (16, (30, 30), 24)}
NAF_KW, NAF_SEED = dict(features=5, context=3, transforms=2), 11


def test_naf_module_tree_state_dict_and_seed_match_the_reference():
    import zuko_amd.flows as F
    from zuko_amd.nn import MonotonicLinear, MonotonicMLP, TwoWayELU

    g = golden("flow_naf_small.npz")
    torch.manual_seed(NAF_SEED)
    flow = F.NAF(**NAF_KW)
    sd = flow.state_dict()
    assert sd_hash(sd) == bytes(g["hash"]).decode()
    assert [k for k, _ in flow.named_parameters()] == list(g["param_names"])
    assert {"transform.transforms.0.order", "transform.transforms.0.hyper.0.mask", "transform.transforms.0.univariate.network.0.weight",
            "transform.transforms.2.univariate.network.4.bias", "base.loc", "base.scale"} <= set(sd)
    assert tuple(sd["transform.transforms.0.univariate.network.0.weight"].shape) == (5, 64, 17)
    assert tuple(sd["transform.transforms.0.hyper.4.weight"].shape) == (5 * 16, 64)
    net = flow.transform.transforms[0].univariate.network
    assert isinstance(net, MonotonicMLP) and [type(m) for m in net] == [MonotonicLinear, TwoWayELU, MonotonicLinear, TwoWayELU, MonotonicLinear]
    assert "stack=5" in repr(net[0])
    torch.manual_seed(NAF_SEED + 100)
    other = F.NAF(**NAF_KW)
    assert sd_hash(other.state_dict()) != sd_hash(sd)
    other.load_state_dict(sd)
    assert sd_hash(other.state_dict()) == sd_hash(sd)
    assert isinstance(F.NAF(1, 2, transforms=1).transform.transforms[0], F.ElementWiseTransform)


@pytest.mark.parametrize("name", list(CASES))
def test_monotonic_mlp_parameters_equal_the_reference_under_the_same_seed(name):
    from zuko_amd.flows import MNN

    S, hidden, seed = CASES[name]
    g = golden(name + ".npz")
    torch.manual_seed(seed)
    m = MNN(signal=S, stack=g["x"].shape[1], hidden_features=hidden)
    lins = [l for l in m.network if hasattr(l, "weight")]
    for i, l in enumerate(lins):
        assert np.array_equal(l.weight.detach().numpy(), g[f"w{i}"]) and np.array_equal(l.bias.detach().numpy(), g[f"b{i}"])
    # the torch-op forward of the module tree (the autograd / fallback path) is the reference's
    with torch.no_grad():
        y = m.f(T(g["signal"]), T(g["x"]))
    assert torch.allclose(y, T(g["y32"]), rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("name", list(CASES))
def test_mnn_ref_reproduces_the_fixtures(name):
    g = golden(name + ".npz")
    for dtype, tag, tol in ((torch.float64, "64", 1e-12), (torch.float32, "32", 1e-5)):
        W, B = mnn_ref.params_of(g, dtype=dtype)
        x, sig, tg = T(g["x"]).to(dtype), T(g["signal"]).to(dtype), T(g["targets"]).to(dtype)
        y, ladj = mnn_ref.forward(W, B, x, sig)
        inv = mnn_ref.inverse(W, B, tg, sig)
        for got, key in ((y, "y"), (ladj, "ladj"), (inv, "inv")):
            ref = T(g[key + tag])
            d = float((got - ref).abs().max())
            print(f"{name} {key}{tag}: max |d| {d:.3e}")
            assert got.dtype == ref.dtype and torch.allclose(got, ref, rtol=tol, atol=tol), f"{name} {key}{tag}: {d:.3e}"
    # a column selection picks the networks of those features
    W, B = mnn_ref.params_of(g, dtype=torch.float64)
    x, sig = T(g["x"]).double(), T(g["signal"]).double()
    y, ladj = mnn_ref.forward(W, B, x[:, [2, 1]], sig[:, [2, 1]], feat=[2, 1])
    assert torch.allclose(y, T(g["y64"])[:, [2, 1]], rtol=1e-12, atol=1e-12) and torch.allclose(ladj, T(g["ladj64"])[:, [2, 1]], rtol=1e-12, atol=1e-12)
    # the targets of rows 0..3 lie outside f(+-bound): the bisection runs into an end of the interval
    assert np.all(g["inv32"][[0, 2]] > 9.99) and np.all(g["inv32"][[1, 3]] < -9.99)


@pytest.mark.parametrize("S,widths", [(16, (64, 64)), (3, (32,)), (7, (16, 48, 128))])
def test_weight_image_walked_in_the_kernels_tile_order_reproduces_mnn_ref(S, widths):
    """Host index table applied to random weights -> image; the emulator reads it exactly where the kernel does.  Covers the K padding of the
    signal product (S = 3, 7: not multiples of 4), rectangular tiles, and the ELU split inside a 16-row tile (16 -> 8 | 8, 48 -> 24 | 24)."""
    from zuko_amd import mnn_plan

    F, n = 3, 37
    rng = np.random.default_rng(S)
    dims = [1 + S, *widths, 1]
    W = [rng.uniform(-1, 1, (F, b, a)) / np.sqrt(a) for a, b in zip(dims[:-1], dims[1:])]
    B = [rng.uniform(-1, 1, (F, b)) / np.sqrt(a) for a, b in zip(dims[:-1], dims[1:])]
    L = mnn_plan.layout(S, widths)
    idx = mnn_plan.index_table(S, widths, F)
    assert idx.shape == (F, L.total) and idx.dtype == np.int32
    w_off, b_off, total = mnn_plan.flat_offsets(S, widths, F)
    flat = np.concatenate([np.abs(w).reshape(-1) for w in W] + [b.reshape(-1) for b in B])
    assert flat.size == total and idx.max() < total
    images = np.where(idx < 0, 0.0, flat[np.maximum(idx, 0)])
    used = np.unique(idx[idx >= 0])
    assert used.size == total, "every parameter appears in the image"
    x = rng.uniform(-9.5, 9.5, (n, F))
    sig = 1.5 * rng.standard_normal((n, F, S))
    y_ref, ladj_ref = mnn_ref.forward([T(w) for w in W], [T(b) for b in B], T(x), T(sig))
    for f in range(F):
        y, dy = mnn_emulator.evaluate(images[f], L, x[:, f], sig[:, f])
        assert np.allclose(y, y_ref[:, f].numpy(), rtol=1e-12, atol=1e-12), f"feature {f}: y"
        assert np.allclose(np.log(dy), ladj_ref[:, f].numpy(), rtol=1e-12, atol=1e-12), f"feature {f}: ladj"


def test_layout_matches_the_library_and_the_supported_predicate():
    import zuko_amd._C as C
    from zuko_amd import mnn_plan, ops

    lib = C.lib()
    for S, widths in [(16, (64, 64)), (3, (32,)), (7, (16, 48, 128)), (63, (128, 128)), (1, (16,)), (16, (128, 128, 64)), (16, (128, 128, 128)), (16, (30, 30)),
                      (64, (64,)), (0, (64,)), (16, (144,)), (16, (64, 64, 64, 64)), (16, ())]:
        w = list(widths[:3]) + [0] * (3 - min(3, len(widths)))
        got = lib.zk_mnn_image_floats(S, len(widths), *w)
        L = mnn_plan.layout(S, widths)
        assert got == (-1 if L is None else L.total), (S, widths, got)
        assert ops.mnn_supported(S, widths) == (L is not None)
    assert ops.mnn_supported(16, (64, 64)) and ops.mnn_supported(63, (128, 128)) and ops.mnn_supported(16, (128, 128, 64))
    assert not ops.mnn_supported(16, (30, 30)) and not ops.mnn_supported(16, (128, 128, 128)) and not ops.mnn_supported(64, (64,))
    assert 4 * mnn_plan.layout(16, (128, 128, 64)).total <= mnn_plan.LDS_MAX


def test_mnn_entry_points_reject_foreign_blocks_and_unsupported_shapes_without_a_device():
    import zuko_amd._C as C

    lib, EINVAL = C.lib(), 1
    text = open(C._HEADER).read()
    for sym in ("zk_mnn_forward", "zk_mnn_inverse", "zk_mnn_image_floats"):
        assert sym in text and sym in C.SIGNATURES and hasattr(ctypes.CDLL(C.LIB_PATH), sym)
    assert "zk_mnn_args_v1" in C.STRUCTS

    def block(**kw):
        base = dict(S=16, n_hidden=2, width0=64, width1=64, width2=0, n_features=5, image_floats=lib.zk_mnn_image_floats(16, 2, 64, 64, 0), N=0, Dsel=5, ldx=5,
                    ld_signal=80, ldy=5, n_bisect=25, bound=10.0)
        base.update(kw)
        return C.args("zk_mnn_args_v1", **base)

    for fn in (lib.zk_mnn_forward, lib.zk_mnn_inverse):
        assert fn(block(), None) == 0  # (a well-formed block over zero rows: accepted, nothing to launch — with every pointer null)
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
        for kw in (dict(width0=30, width1=30), dict(width0=144), dict(width1=0), dict(n_hidden=4), dict(n_hidden=0), dict(S=0), dict(S=64), dict(image_floats=1),
                   dict(n_hidden=3, width0=128, width1=128, width2=128), dict(ld_signal=79), dict(ldy=4), dict(Dsel=0), dict(N=-1), dict(n_features=0),
                   dict(Dsel=(1 << 20) + 1, ldy=1 << 21, ld_signal=1 << 25)):
            assert fn(block(**kw), None) == EINVAL, kw
        assert fn(block(N=4), None) == EINVAL  # (rows but no pointers)
    assert lib.zk_mnn_forward(block(Dsel=1 << 20, ldy=1 << 21, ld_signal=1 << 25), None) == 0  # (the largest column count)
    # the bisection's parameters are the inverse's alone
    assert lib.zk_mnn_inverse(block(bound=0.0), None) == EINVAL and lib.zk_mnn_inverse(block(n_bisect=65), None) == EINVAL
    assert lib.zk_mnn_inverse(block(n_bisect=64), None) == 0 and lib.zk_mnn_forward(block(n_bisect=65, bound=0.0), None) == 0


def test_cpu_tensors_are_rejected_and_stacked_linear_is_provided():
    from zuko_amd import nn as ZN
    from zuko_amd.flows import NAF

    lin = ZN.Linear(3, 4, stack=5)
    assert tuple(lin.weight.shape) == (5, 4, 3) and tuple(lin.bias.shape) == (5, 4)
    assert tuple(lin(torch.randn(7, 5, 3)).shape) == (7, 5, 4)
    flow = NAF(3, 2, transforms=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        flow(torch.randn(4, 2)).log_prob(torch.randn(4, 3))


def test_invalidate_drops_the_weight_image():
    import zuko_amd
    from zuko_amd.flows import NAF

    flow = NAF(3, 0, transforms=1)
    net = flow.transform.transforms[0].univariate.network
    net.__dict__["_mnn_image_cache"] = ("key", object())
    net.__dict__["_mnn_feat_cache"] = {"k": None}
    zuko_amd.invalidate(flow)
    assert "_mnn_image_cache" not in net.__dict__ and "_mnn_feat_cache" not in net.__dict__


@pytest.mark.parametrize("randperm,C", [(False, 2), (True, 0)])
def test_wavefront_inverse_hands_the_sweeps_features_to_a_per_feature_map(randperm, C):
    """The ordered inverse of a NAF layer (zuko_amd/flows/autoregressive.py: wavefront_inverse with `with_features=True`) walked on the CPU with torch
    stand-ins, float64: every sweep inverts its own features with THEIR networks, and the result is the reference loop's (every feature, every sweep)."""
    import torch.nn.functional as Fn

    import zuko_amd.flows as F
    from zuko_amd.flows.autoregressive import MaskedAutoregressiveTransform, wavefront_inverse

    torch.manual_seed(6)
    flow = F.NAF(5, C, transforms=2, randperm=randperm, hidden_features=[24, 24], network=dict(hidden_features=(16, 32))).double()
    N = 19

    def linear(h, w, b, m, act):
        out = Fn.linear(h, w * m, b)
        return out if act is None else act(out)

    for lazy in (t for t in flow.transform.transforms if isinstance(t, MaskedAutoregressiveTransform)):
        assert lazy.univariate.per_feature
        lins = [l for l in lazy.univariate.network if hasattr(l, "weight")]
        W, B = [l.weight.detach() for l in lins], [l.bias.detach() for l in lins]
        g = torch.Generator().manual_seed(9)
        y = torch.randn(N, 5, generator=g, dtype=torch.float64) * 0.5
        c = torch.randn(N, C, generator=g, dtype=torch.float64) if C else None
        mods = list(lazy.hyper)
        seen = []

        def inverse_of(phi, ys, idx):
            feat = list(range(*idx)) if isinstance(idx, tuple) else idx.tolist()
            seen.extend(feat)
            return mnn_ref.inverse(W, B, ys, phi, feat=feat)

        with torch.no_grad():
            x_w = wavefront_inverse(lazy, y, c, lazy.passes, linear, inverse_of, with_features=True)
            x_r = torch.zeros_like(y)
            for _ in range(lazy.passes):
                h = x_r if c is None else torch.cat((x_r, c), dim=-1)
                for i in range(0, len(mods) - 1, 2):
                    h = linear(h, mods[i].weight, mods[i].bias, mods[i].mask, mods[i + 1])
                phi = linear(h, mods[-1].weight, mods[-1].bias, mods[-1].mask, None).unflatten(-1, (5, lazy.total))
                x_r = mnn_ref.inverse(W, B, y, phi)
            y_back = mnn_ref.forward(W, B, x_w, phi, tangent=False)[0]
        assert sorted(seen) == list(range(5)), "every feature inverted exactly once"
        assert (x_w - x_r).abs().max().item() <= 1e-12
        assert (y_back - y).abs().max().item() < 1e-5


def test_feature_tables_are_checked_on_the_host_and_cached_by_tensor_identity():
    """ops._mnn_feat: a selection outside the stack raises (the kernel's clamp is only a memory guard); an index tensor's table is cached against
    the tensor OBJECT and its version, never against an address another tensor could be given later."""
    from zuko_amd import ops
    from zuko_amd.flows import MNN

    net = MNN(signal=4, stack=5, hidden_features=(16,)).network
    assert ops._mnn_feat(net, None, "cpu") is None
    assert ops._mnn_feat(net, (1, 4), "cpu").tolist() == [1, 2, 3] and ops._mnn_feat(net, (1, 4), "cpu").dtype == torch.int32
    for bad in ((3, 6), (-1, 2), (2, 2)):
        with pytest.raises(IndexError):
            ops._mnn_feat(net, bad, "cpu")
    with pytest.raises(IndexError):
        ops._mnn_feat(net, torch.tensor([0, 5]), "cpu")
    with pytest.raises(IndexError):
        ops._mnn_feat(net, torch.tensor([-1, 2]), "cpu")
    a = torch.tensor([3, 1])
    ta = ops._mnn_feat(net, a, "cpu")
    assert ta.tolist() == [3, 1] and ops._mnn_feat(net, a, "cpu") is ta
    b = torch.tensor([0, 4])
    b.set_(a.untyped_storage(), 0, (2,))  # another tensor on the SAME memory, as the caching allocator may arrange after a free
    b.copy_(torch.tensor([0, 4]))
    assert b.data_ptr() == a.data_ptr() and b.numel() == a.numel() and ops._mnn_feat(net, b, "cpu").tolist() == [0, 4]
    c = torch.tensor([2, 2])
    tc = ops._mnn_feat(net, c, "cpu")
    c[0] = 4  # an in-place write bumps the version: the table follows
    assert tc.tolist() == [2, 2] and ops._mnn_feat(net, c, "cpu").tolist() == [4, 2]
