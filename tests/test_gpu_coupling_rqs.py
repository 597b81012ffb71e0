"""GPU: coupling transforms whose univariate map is the rational-quadratic spline (the coupling form of neural spline flows) on the fused launch
(csrc/fused_coupling.hip: coupling_rqs_kernel; zk_coupling_forward_v2 / zk_coupling_inverse_v2), forward and inverse, against the oracle."""

import dataclasses
import functools
from functools import partial

import pytest
import torch

from oracle import zuko_oracle as O
from parity import assert_parity, d64, to_f64

# (D, ctx, K, hidden, N)
CASES = [
    (5, 3, 8, [32, 32], 1000),          # a partial group, context, D not a multiple of 4
    (12, 2, 16, [40, 70, 24], 77),      # widths off the tile grid, fewer rows than a block, second group partial
    (7, 0, 4, [48], 257),               # two linear layers only
    (64, 0, 8, [256], 4096 + 5),        # 8 groups, many ring chunks, ragged tail
    (32, 0, 8, [512, 512], 300),        # all 32 activation tiles live: the register corner
]
IDS = [f"D{D}-c{c}-K{K}-{'x'.join(map(str, h))}-N{N}" for D, c, K, h, N in CASES]


def _nice(D, ctx, K, hidden, univariate=None, transforms=3):
    import zuko_amd.flows as F
    from zuko_amd.transforms import MonotonicRQSTransform

    return F.NICE(D, ctx, transforms=transforms, hidden_features=hidden, univariate=univariate or MonotonicRQSTransform, shapes=[(K,), (K,), (K - 1,)])


def _spec(flow, uni, D):
    return O.spec_from_state_dict({k: v.detach().cpu().clone() for k, v in flow.state_dict().items() if v is not None}, "coupling", uni, D)


@functools.lru_cache(maxsize=None)
def _reference(D, ctx, K, hidden, N):
    """The flow on the CPU, its inputs and the oracle's answers in float32 and float64: computed once per case and only read by the tests."""
    torch.manual_seed(D + N + K)
    flow = _nice(D, ctx, K, list(hidden))
    spec = _spec(flow, O.uni_rqs(K), D)
    spec64 = to_f64(spec)
    g = torch.Generator().manual_seed(3)
    x = 2.5 * torch.randn(N, D, generator=g)
    c = torch.randn(N, ctx, generator=g) if ctx else None
    with torch.no_grad():
        fwd = O.flow_forward(spec, x, c) + O.flow_forward(spec64, d64(x), d64(c))
        lp = (O.flow_log_prob(spec, x, c), O.flow_log_prob(spec64, d64(x), d64(c)))
        inv = (O.flow_inverse(spec, fwd[0], c), O.flow_inverse(spec64, d64(fwd[0]), d64(c)))
    return flow, spec, spec64, x, c, fwd, lp, inv


def _on_device(case, dev):
    import copy

    D, ctx, K, hidden, N = case
    ref = _reference(D, ctx, K, tuple(hidden), N)
    flow = copy.deepcopy(ref[0]).to(dev)
    return (flow,) + ref[1:]


def _count_launches(flow, dev, monkeypatch):
    """Wraps every transform's FusedCoupling.run: the returned list receives (transform index, inverse) per fused launch."""
    launches = []
    for i, t in enumerate(flow.transform.transforms):
        st = t.fused_state(dev)
        assert st is not None, f"transform {i}: no fused state"

        def run(x_, c_, inv_=False, _run=st.run, _i=i):
            launches.append((_i, bool(inv_)))
            return _run(x_, c_, inv_)

        monkeypatch.setattr(st, "run", run)
    return launches


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_log_prob(dev, case, monkeypatch):
    D, ctx, K, hidden, N = case
    flow, spec, spec64, x, c, (zo, lo, z64, l64), (lpo, lp64), _ = _on_device(case, dev)
    xg, cg = x.to(dev), None if c is None else c.to(dev)
    T = len(flow.transform.transforms)
    tag = f"spline coupling D={D} ctx={ctx} K={K} hidden={hidden} N={N}"
    with torch.no_grad():
        launches = _count_launches(flow, dev, monkeypatch)
        assert all(t.fused_state(dev).uni_kind == 1 and t.fused_state(dev).bins == K and not t.fused_state(dev).split for t in flow.transform.transforms)
        z, ladj = flow(cg).transform.call_and_ladj(xg)
        assert launches == [(i, False) for i in range(T)], "one forward launch per transform"
        del launches[:]
        lp = flow(cg).log_prob(xg)
        assert launches == [(i, False) for i in range(T)], "log_prob: one forward launch per transform"
        del launches[:]
        monkeypatch.setenv("ZUKO_AMD_NO_FUSED_COUPLING", "1")
        z_l, ladj_l = flow(cg).transform.call_and_ladj(xg)
        lp_l = flow(cg).log_prob(xg)
        monkeypatch.delenv("ZUKO_AMD_NO_FUSED_COUPLING")
        assert launches == [], "ZUKO_AMD_NO_FUSED_COUPLING=1: the layer-wise path"
    outside = float((x.abs() > 5).float().mean())
    print(f"{tag}: share of |x| > 5: {outside:.4f}, mean |ladj| {float(lo.abs().mean()):.3f}")
    assert outside > 0.0
    assert_parity(z, zo, z64, f"{tag}: z fused")
    assert_parity(ladj, lo, l64, f"{tag}: ladj fused")
    assert_parity(lp, lpo, lp64, f"{tag}: log_prob fused")
    assert_parity(z_l, zo, z64, f"{tag}: z layer-wise")
    assert_parity(ladj_l, lo, l64, f"{tag}: ladj layer-wise")
    assert_parity(lp_l, lpo, lp64, f"{tag}: log_prob layer-wise")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_inverse_and_sampling(dev, case, monkeypatch):
    D, ctx, K, hidden, N = case
    flow, spec, spec64, x, c, (zo, lo, z64, l64), _, (xo, x64) = _on_device(case, dev)
    cg = None if c is None else c.to(dev)
    T = len(flow.transform.transforms)
    tag = f"spline coupling inverse D={D} ctx={ctx} K={K} hidden={hidden} N={N}"
    with torch.no_grad():
        launches = _count_launches(flow, dev, monkeypatch)
        xi = flow(cg).transform.inv(zo.to(dev))
        assert launches == [(i, True) for i in reversed(range(T))], "one inverse launch per transform"
        assert_parity(xi, xo, x64, f"{tag}: x = inv(z of the oracle)")
        z_back, _ = flow(cg).transform.call_and_ladj(xi)
        assert_parity(z_back, zo, z64, f"{tag}: round trip z -> x -> z", c=8.0)
        # one transform: x and the forward map's log-determinant from ONE inverse launch; inv.call_and_ladj hands out (x, -ladj) of that launch
        t0 = flow.transform.transforms[0](cg)
        del launches[:]
        x0, l0 = t0.inverse_and_ladj(zo.to(dev))
        x1 = t0.inv(zo.to(dev))
        x2, l2 = t0.inv.call_and_ladj(zo.to(dev))
        assert launches == [(0, True)] * 3
        assert torch.equal(x2, x0) and torch.equal(x2, x1) and torch.equal(l2, -l0)
        of, olf = O.layer_forward(spec.layers[0], x0.cpu(), c)
        _, olf64 = O.layer_forward(spec64.layers[0], d64(x0), d64(c))
        assert_parity(l0, olf, olf64, f"{tag}: ladj of the inverse launch vs the oracle's forward ladj at the solution")
        # sampling: x and log_prob from the inverse launches (a few context rows: the sample is [513, rows, D])
        cs = None if c is None else c[:4]
        del launches[:]
        torch.manual_seed(0)
        xs, lp = (flow(cs.to(dev)) if cs is not None else flow()).rsample_and_log_prob((513,))
        assert launches == [(i, True) for i in reversed(range(T))], "rsample_and_log_prob: one inverse launch per transform"
        lpo = O.flow_log_prob(spec, xs.cpu(), cs)
    rel = ((lp.cpu() - lpo).abs() / lpo.abs().clamp_min(1.0)).max()
    print(f"{tag}: rsample_and_log_prob vs oracle log_prob at the sample: max relative difference {float(rel):.3e}")
    assert rel < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_non_finite_inputs(dev, case, monkeypatch):
    """NaN / inf in a pass-through column (or the context): every moved column of the row goes the way the reference's all-NaN parameters send it and ladj is
    NaN, the pass-through columns leave unchanged.  NaN / +inf / -inf in a moved column: that column keeps the value, ladj NaN, the row's other columns are
    finite.  Other rows: the bits of a run without the bad rows."""
    D, ctx, K, hidden, N = case
    flow, spec, spec64, x, c, *_ = _on_device(case, dev)
    lazy = flow.transform.transforms[0]
    a_col, b_col = int(lazy.mask.nonzero()[0]), int((~lazy.mask).nonzero()[-1])
    n = 24
    xb, cb = x[:n].clone(), None if c is None else c[:n].clone()
    nan, inf = float("nan"), float("inf")
    xb[1, a_col], xb[3, a_col], xb[5, b_col], xb[7, b_col], xb[9, b_col] = nan, inf, nan, inf, -inf
    bad = [1, 3, 5, 7, 9]
    if cb is not None:
        cb[11, 0], cb[13, ctx - 1] = nan, -inf
        bad += [11, 13]
    good = [i for i in range(n) if i not in bad]
    launches = _count_launches(flow, dev, monkeypatch)
    with torch.no_grad():
        yb, lb = lazy(None if cb is None else cb.to(dev)).call_and_ladj(xb.to(dev))
        yc, lc = lazy(None if c is None else c[:n].to(dev)).call_and_ladj(x[:n].to(dev))
        assert launches == [(0, False)] * 2
        oy, ol = O.layer_forward(spec.layers[0], xb, cb)
        oy64, ol64 = O.layer_forward(spec64.layers[0], d64(xb), d64(cb))
    tag = f"spline coupling non-finite D={D} ctx={ctx} K={K} hidden={hidden}"
    assert_parity(yb, oy, oy64, f"{tag}: y")      # (identical NaN pattern, identical infinities, parity on the finite values)
    assert_parity(lb, ol, ol64, f"{tag}: ladj")
    yb, lb = yb.cpu(), lb.cpu()
    assert torch.equal(yb[good], yc.cpu()[good]) and torch.equal(lb[good], lc.cpu()[good]), "rows without a non-finite input changed"
    keep = lazy.mask.cpu()
    assert torch.equal(yb[:, keep].nan_to_num(7.0, 8.0, 9.0), xb[:, keep].nan_to_num(7.0, 8.0, 9.0)), "pass-through columns changed"
    assert torch.isnan(lb[bad]).all() and torch.isfinite(lb[good]).all()
    for r in [1, 3] + ([11, 13] if cb is not None else []):
        inside = xb[r, ~keep] > -5.0  # (all-NaN parameters: NaN right of -bound, the value itself at or left of it)
        assert torch.isnan(yb[r, ~keep][inside]).all() and torch.equal(yb[r, ~keep][~inside], xb[r, ~keep][~inside])
    others = [j for j in range(D) if j != b_col]
    assert torch.isnan(yb[5, b_col]) and yb[7, b_col] == inf and yb[9, b_col] == -inf and torch.isfinite(yb[[5, 7, 9]][:, others]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_graph_capture_replays_the_eager_bits(dev, case):
    import zuko_amd

    D, ctx, K, hidden, N = case
    flow, spec, spec64, x, c, *_ = _on_device(case, dev)
    xg, cg = x.to(dev), None if c is None else c.to(dev)
    with torch.no_grad():
        eager = flow(cg).log_prob(xg)
    captured = zuko_amd.capture(flow, xg, cg)
    assert torch.equal(captured(xg, cg), eager)
    x2 = xg.flip(0).contiguous()
    c2 = None if cg is None else cg.flip(0).contiguous()
    with torch.no_grad():
        eager2 = flow(c2).log_prob(x2)
    assert torch.equal(captured(x2, c2), eager2)


@pytest.mark.gpu
def test_keywords_are_served_and_other_univariates_decline(dev, monkeypatch):
    """bound / slope keywords reach the kernel and meet the parity bar; K without an instantiation, an unknown keyword, float64 inputs and parameters that
    need gradients run layer by layer with zero fused launches — and are right.  What a declined call returns is the layer-wise kernels' result, which
    this change does not touch (the five cases above hold that path to the parity bar at K = 4, 8, 16), so the check here is that the ROUTE is right: a
    call that lost its keyword, its bin count or its bound on the way would be wrong by 1e-2 and more.  The bar for it is allclose(1e-4, 1e-4) to the
    float32 oracle: tests/parity.py records that two correct float32 evaluations of a spline's log-derivative sit up to 5e-5 .. 9e-5 apart."""
    from zuko_amd.transforms import MonotonicRQSTransform

    D, ctx, N = 6, 2, 200
    g = torch.Generator().manual_seed(5)
    x, c = 2.5 * torch.randn(N, D, generator=g), torch.randn(N, ctx, generator=g)

    def check(flow_cpu, uni, tag, fused, dtype=torch.float32, grad=False):
        import copy

        spec = _spec(flow_cpu, uni, D)
        spec64 = to_f64(spec)
        flow = copy.deepcopy(flow_cpu).to(dev)
        launches = []
        for i, t in enumerate(flow.transform.transforms):
            st = t.fused_state(dev)
            assert (st is not None) == (fused or grad), f"{tag}: fused_state"  # (float64 weights have no fused state; with gradients the state exists and is not used)
            if st is not None:
                monkeypatch.setattr(st, "run", lambda x_, c_, inv_=False, _run=st.run, _i=i: launches.append((_i, bool(inv_))) or _run(x_, c_, inv_))
        for p in flow.parameters():
            p.requires_grad_(grad)
        with torch.set_grad_enabled(grad):
            z, ladj = flow(c.to(dev, dtype)).transform.call_and_ladj(x.to(dev, dtype))
            xi = flow(c.to(dev, dtype)).transform.inv(z.detach())
        assert launches == ([(i, False) for i in range(2)] + [(i, True) for i in (1, 0)] if fused else []), f"{tag}: fused launches {launches}"
        with torch.no_grad():
            z64, l64 = O.flow_forward(spec64, d64(x), d64(c))
            x64 = O.flow_inverse(spec64, d64(z.detach()), d64(c))
            if dtype == torch.float32:
                zo, lo = O.flow_forward(spec, x, c)
                xo = O.flow_inverse(spec, z.detach().cpu(), c)
        if dtype == torch.float64:
            # the float64 kernels are held to 1e-12 per call (parity.assert_f64); two transforms with a 3-layer conditioner each, and for the inverse the
            # spline's smallest slope (>= the 1e-3 of `slope`) amplifying by up to 1e3, stay within 1e-9 — six orders below what a float32 path could give
            assert torch.allclose(z.cpu(), z64, rtol=1e-9, atol=1e-9) and torch.allclose(ladj.cpu(), l64, rtol=1e-9, atol=1e-9) and torch.allclose(xi.cpu(), x64, rtol=1e-9, atol=1e-9)
            return
        if fused:
            assert_parity(z, zo, z64, f"{tag}: z")
            assert_parity(ladj, lo, l64, f"{tag}: ladj")
            assert_parity(xi, xo, x64, f"{tag}: inverse")
        else:
            for name, got, want in (("z", z, zo), ("ladj", ladj, lo), ("inverse", xi, xo)):
                d = float((got.detach().cpu() - want).abs().max())
                print(f"{tag}: {name}: max |layer-wise - oracle| = {d:.3e}")
                assert torch.allclose(got.detach().cpu(), want, rtol=1e-4, atol=1e-4), f"{tag}: {name}: max |d| {d:.3e}"

    torch.manual_seed(11)
    kw = _nice(D, ctx, 8, [32, 24], univariate=partial(MonotonicRQSTransform, bound=3.0, slope=1e-2), transforms=2)
    check(kw, dataclasses.replace(O.uni_rqs(8, 1e-2), bound=3.0), "bound=3, slope=1e-2", fused=True)
    for K in (3, 32):
        torch.manual_seed(K)
        check(_nice(D, ctx, K, [32, 24], transforms=2), O.uni_rqs(K), f"K={K}", fused=False)
    torch.manual_seed(12)
    check(_nice(D, ctx, 8, [32, 24], univariate=partial(MonotonicRQSTransform, cache_size=0), transforms=2), O.uni_rqs(8), "unknown keyword", fused=False)
    torch.manual_seed(13)
    plain = _nice(D, ctx, 8, [32, 24], transforms=2)
    check(plain, O.uni_rqs(8), "plain", fused=True)
    check(plain.double(), O.uni_rqs(8), "float64", fused=False, dtype=torch.float64)
    torch.manual_seed(13)
    check(_nice(D, ctx, 8, [32, 24], transforms=2), O.uni_rqs(8), "parameters require grad", fused=False, grad=True)
