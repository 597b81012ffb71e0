"""The base density folded into the last autoregressive launch of `NormalizingFlow.log_prob` (csrc/zk_ar_common.h: ArArgs::base_loc; arht_kernel,
arxt_kernel): a no-grad log_prob of a flow whose last transform runs on an operand-split static-shape kernel is T launches — the last one adds
log N(y; loc, scale) to the running log-determinant and writes no y.  ZUKO_AMD_NO_FUSED_BASE=1 keeps the two-launch path (transform, then
zk_diag_normal_log_prob), which is the comparison here next to the CPU oracle.

Shapes: the registry's cfg2 (NSF) and cfg3 (MAF) flows, whose conditioners are prebuilt (both kernels really run; their last transform has the
DESCENDING feature order, so a table indexed by slot instead of by feature id shows with a base whose loc differs per feature).  Rows 1, 16, 17, 127,
128, 129: the wavefront (16 rows) and workgroup (128 rows) tile edges; 128 * 256 + 17: the second round of the persistent grid of 256 workgroups,
whose last tile requests its own rows again.

Bound of the comparison with the two-launch path (nothing is bitwise: 64 + 64 terms are summed per lane, then over four lanes, instead of by a
wavefront reduction, and x / (2 s^2) is a product with the rounded reciprocal): every term of the base's log-density is negative, so the sum of the
magnitudes of what is added up is S = |log N(z)| + |ladj|; a reordered f32 sum of n = 2 D + 4 terms differs by at most n 2^-24 S from the exact sum on
either side, the reciprocal adds 3 roundings of relative 2^-24 per term: |terminal - two-launch| <= (4 D + 8 + 6) 2^-24 S, asserted per row."""

import pytest
import torch

from conftest import build_flow, oracle_spec
from oracle import zuko_oracle as O
from parity import assert_parity, d64, to_f64

pytestmark = pytest.mark.gpu

ROWS = [1, 16, 17, 127, 128, 129, 128 * 256 + 17]
NBIG = ROWS[-1]
HEAD = 384  # rows of the big batch the oracle evaluates: the first HEAD and the last HEAD (rows are independent; the GPU comparison covers all of them)
_CACHE: dict = {}


def _flow(name: str, base: str, dev):
    """(flow on the device, x [NBIG, D] on the host, fp32 / fp64 oracle log_prob of the first and last HEAD rows), built once per (flow, base)."""
    key = (name, base)
    if key not in _CACHE:
        flow, entry = build_flow(name)
        D = entry[1]["features"]
        if base == "shifted":  # loc different for every feature, scale in [0.5, 2]
            g = torch.Generator().manual_seed(3)
            with torch.no_grad():
                flow.base.loc.copy_(torch.linspace(-1.5, 1.5, D)[torch.randperm(D, generator=g)])
                flow.base.scale.copy_(0.5 + 1.5 * torch.rand(D, generator=g))
        assert int(flow.transform.transforms[-1].order[0]) == D - 1, "the last transform is expected to have the descending order"
        spec = oracle_spec(flow, entry)
        x = torch.randn(NBIG, D, generator=torch.Generator().manual_seed(17)) * 1.2
        sel = torch.cat([torch.arange(HEAD), torch.arange(NBIG - HEAD, NBIG)])
        with torch.no_grad():
            ref32 = O.flow_log_prob(spec, x[sel])
            ref64 = O.flow_log_prob(to_f64(spec), d64(x[sel]))
        _CACHE[key] = (flow.to(dev), x, sel, ref32, ref64)
    return _CACHE[key]


def _terminal_launches(fn):
    """Runs fn() with the entry-point profile on; returns (result, launches of zk_ar_forward_static with a base, calls of zk_diag_normal_log_prob)."""
    from zuko_amd import _C

    _C.PROFILE = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        prof = _C.PROFILE
    finally:
        _C.PROFILE = None
    term = sum(1 for _, _, args in prof.get("zk_ar_forward_static", []) if args[0].base_loc)
    return out, term, len(prof.get("zk_diag_normal_log_prob", []))


def _two_launch(flow, x, monkeypatch):
    """log_prob, ladj of the two-launch path."""
    monkeypatch.setenv("ZUKO_AMD_NO_FUSED_BASE", "1")
    with torch.no_grad():
        lp = flow().log_prob(x)
        ladj = flow().transform.call_and_ladj(x)[1]
    monkeypatch.delenv("ZUKO_AMD_NO_FUSED_BASE")
    return lp, ladj


@pytest.mark.parametrize("precision", ["f16x2", "bf16x3"])
@pytest.mark.parametrize("base", ["standard", "shifted"])
@pytest.mark.parametrize("name", ["nsf_cfg2", "maf_cfg3"])
def test_terminal_log_prob_matches_two_launch_path_and_oracle(dev, matmul, monkeypatch, name, base, precision):
    matmul(precision)
    flow, x, sel, ref32, ref64 = _flow(name, base, dev)
    D = x.shape[1]
    xg = x.to(dev)
    for N in ROWS:
        with torch.no_grad():
            lp, term, normal = _terminal_launches(lambda: flow().log_prob(xg[:N]))
        assert term == 1 and normal == 0, f"{name} N={N}: {term} terminal launches, {normal} zk_diag_normal_log_prob calls"
        old, ladj = _two_launch(flow, xg[:N], monkeypatch)
        assert lp.shape == old.shape == (N,)
        S = (old - ladj).abs() + ladj.abs()
        err = (lp - old).abs()
        tol = (4 * D + 14) * 2.0**-24 * S
        print(f"{name} {base} {precision} N={N}: max |terminal - two-launch| = {err.max().item():.3e} (bound {tol.min().item():.3e} .. {tol.max().item():.3e})")
        assert bool((err <= tol).all()), f"{name} {base} {precision} N={N}: max |terminal - two-launch| {err.max().item():.3e} above the summation-order bound {tol[err.argmax()].item():.3e}"
        if N == NBIG:
            assert_parity(lp[sel.to(dev)], ref32, ref64, f"fused base {name} {base} {precision} N={N}: log_prob")
        else:
            assert_parity(lp, ref32[:N], ref64[:N], f"fused base {name} {base} {precision} N={N}: log_prob")


@pytest.mark.parametrize("name", ["nsf_cfg2", "maf_cfg3"])
def test_terminal_non_finite_rows(dev, matmul, monkeypatch, name):
    """inf / NaN at the first and the last row of a workgroup tile: the NaN pattern is the two-launch path's, every other row keeps its bits."""
    matmul("f16x2")
    flow, x, _, _, _ = _flow(name, "shifted", dev)
    N = 300
    clean = x[:N].to(dev)
    bad = clean.clone()
    bad[0, 5], bad[127, 63], bad[128, 0], bad[255, 31] = float("inf"), float("nan"), float("nan"), float("-inf")
    rows = torch.tensor([0, 127, 128, 255], device=dev)
    with torch.no_grad():
        lp_clean = flow().log_prob(clean)
        lp, term, _ = _terminal_launches(lambda: flow().log_prob(bad))
    assert term == 1
    old, _ = _two_launch(flow, bad, monkeypatch)
    assert torch.equal(lp.isnan(), old.isnan()) and torch.equal(lp.isinf(), old.isinf())
    assert bool(lp[rows].isnan().all())
    others = torch.ones(N, dtype=torch.bool, device=dev)
    others[rows] = False
    assert torch.isfinite(lp[others]).all() and torch.equal(lp[others], lp_clean[others]), "rows next to a non-finite one must not change by a bit"


def test_terminal_path_is_taken_and_left(dev, matmul, monkeypatch):
    import zuko_amd.flows as F
    from zuko_amd.distributions import DiagNormal
    from zuko_amd.lazy import Flow, UnconditionalDistribution

    matmul("f16x2")
    flow, x, _, _, _ = _flow("nsf_cfg2", "standard", dev)
    xg = x[:257].to(dev)
    T = len(flow.transform.transforms)
    with torch.no_grad():
        lp, term, normal = _terminal_launches(lambda: flow().log_prob(xg))
    assert (term, normal) == (1, 0), "no-grad log_prob of cfg2: T launches, the last one terminal"
    old, _ = _two_launch(flow, xg, monkeypatch)

    # ZUKO_AMD_NO_FUSED_BASE=1: the two-launch path
    monkeypatch.setenv("ZUKO_AMD_NO_FUSED_BASE", "1")
    with torch.no_grad():
        lp_env, term, normal = _terminal_launches(lambda: flow().log_prob(xg))
    monkeypatch.delenv("ZUKO_AMD_NO_FUSED_BASE")
    assert (term, normal) == (0, 1) and torch.equal(lp_env, old)

    # a base that requires grad, under grad mode (the transforms' parameters frozen: they stay on the fused kernel): the base is torch's Normal.log_prob,
    # through which its gradient flows as in the reference — no terminal launch, the two-launch path's z and log-determinant
    D = xg.shape[1]
    trainable = Flow(flow.transform, UnconditionalDistribution(DiagNormal, torch.zeros(D), torch.ones(D), buffer=False)).to(dev)
    req = [p.requires_grad for p in flow.transform.parameters()]
    try:
        for p in flow.transform.parameters():
            p.requires_grad_(False)
        lp_g, term, _ = _terminal_launches(lambda: trainable().log_prob(xg))
        assert term == 0 and lp_g.requires_grad
        with torch.no_grad():
            z, ladj = flow().transform.call_and_ladj(xg)
            ref = trainable().base.log_prob(z) + ladj
        assert torch.equal(lp_g.detach(), ref)
        lp_g.sum().backward()
        assert trainable.base._0.grad is not None and torch.isfinite(trainable.base._0.grad).all()
        with torch.no_grad():  # the same flow without grad mode: terminal again
            _, term, normal = _terminal_launches(lambda: trainable().log_prob(xg))
        assert (term, normal) == (1, 0)
    finally:
        for p, r in zip(flow.transform.parameters(), req):
            p.requires_grad_(r)

    # a coupling transform as the last member
    torch.manual_seed(2)
    nvp = F.RealNVP(features=8, context=0, transforms=2, hidden_features=[32, 32]).to(dev)
    xs = torch.randn(129, 8, generator=torch.Generator().manual_seed(4)).to(dev)
    with torch.no_grad():
        lp_n, term, normal = _terminal_launches(lambda: nvp().log_prob(xs))
    old_n, _ = _two_launch(nvp, xs, monkeypatch)
    assert (term, normal) == (0, 1) and torch.equal(lp_n, old_n)


@pytest.mark.parametrize("name", ["nsf_cfg2", "maf_cfg3"])
def test_transform_call_and_ladj_is_unchanged(dev, matmul, monkeypatch, name):
    matmul("f16x2")
    flow, x, _, _, _ = _flow(name, "shifted", dev)
    xg = x[:129].to(dev)
    with torch.no_grad():
        z, ladj = flow().transform.call_and_ladj(xg)
        monkeypatch.setenv("ZUKO_AMD_NO_FUSED_BASE", "1")
        z0, ladj0 = flow().transform.call_and_ladj(xg)
    assert z is not None and torch.equal(z, z0) and torch.equal(ladj, ladj0)


def test_two_part_kernel_product_launch_equals_its_diagnostic_twin(dev, matmul):
    """The two-part kernel's y and log-determinant at N = 129, bit for bit against its diagnostic twin (whose bins and knots tests/test_gpu_bins.py checks):
    the comparison a change of the last layer's row order or of its descale has to keep."""
    from zuko_amd.nn import MaskedLinear

    matmul("f16x2")
    flow, x, _, _, _ = _flow("nsf_cfg2", "standard", dev)
    N, D, K = 129, x.shape[1], 8
    inp = x[:N].to(dev).contiguous()
    for lazy in (flow.transform.transforms[0], flow.transform.transforms[-1]):  # ascending and descending order
        st = lazy.fused_state(dev)
        assert st is not None and st.ready(N)
        st.refresh([m for m in lazy.hyper if isinstance(m, MaskedLinear)])
        assert st._half_serves(inp), "the two-part kernel must serve this launch"
        y, ladj = torch.empty(N, D, device=dev), torch.empty(N, device=dev)
        yd, ld = torch.empty_like(y), torch.empty_like(ladj)
        bins = torch.empty(N, D, dtype=torch.int32, device=dev)
        knots = torch.empty(N, D, K + 1, device=dev)
        st.run(inp, y, ladj, False)
        st.run_diag(inp, yd, ld, bins, knots)
        assert torch.equal(y.view(torch.int32), yd.view(torch.int32)) and torch.equal(ladj.view(torch.int32), ld.view(torch.int32))
        assert int(bins.min()) >= 0 and int(bins.max()) < K and bool(torch.isfinite(knots).all())
