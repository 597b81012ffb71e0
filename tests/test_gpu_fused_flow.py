"""The FLOW launch of the two-part fused autoregressive kernel on the GPU (csrc/fused_ar_half_impl.h: arhf_kernel; zuko_amd/fused.py: FusedFlow): all T
transforms of a composed autoregressive flow in one persistent launch.  Its schedule is checked on the CPU by tests/test_flow_schedule.py.

Shapes: the cfg2 conditioner (NSF, 64 features, 256 x 3, 50 chunks per pass) and MAF(16, [128, 128]), whose pass is three chunks — shorter than the
four-slot ring.  T = 2 and 3: both feature orders of the alternating composition, an even and an odd number of passes per tile (the bias double
buffer starts a tile in either half).  Rows: 129 (a partial second tile) and 256 * 128 + 129 (on the persistent grid of 256 workgroups the first
two run two tiles: the ring wraps across a tile and a transform boundary, and the last pass of the first tile requests the next tile's rows).
Row 100 is NaN.

Per case: log_prob and call_and_ladj equal the path with ZUKO_AMD_NO_FUSED_FLOW=1 (one launch per transform) BIT FOR BIT — every transform's
arithmetic and summation order is the per-transform kernel's, only where x is read from and when y leaves differ —, two runs are bitwise equal, the NaN
row is NaN in its own outputs only, and log_prob meets the oracle bars of tests/parity.py (the oracle evaluates the first and the last 129 rows)."""

import pytest
import torch

from oracle import zuko_oracle as O
from parity import assert_parity, d64, to_f64

pytestmark = pytest.mark.gpu

BIG = 256 * 128
ROWS = [129, BIG + 129]
NMAX = ROWS[-1]
BAD = 100
_CACHE: dict = {}


def _flow(name: str, T: int, dev):
    """(flow on the device, x [NMAX, D] on the device, rows the oracle evaluated, its fp32 / fp64 log_prob of them), built once per case."""
    key = (name, T)
    if key not in _CACHE:
        import zuko_amd.flows as F

        torch.manual_seed(7 + T)
        if name == "nsf_cfg2":
            D, uni = 64, O.uni_rqs(8)
            flow = F.NSF(features=D, context=0, transforms=T, bins=8, hidden_features=[256] * 3)
        else:
            D, uni = 16, O.UNI_AFFINE
            flow = F.MAF(D, 0, transforms=T, hidden_features=[128, 128])
        sd = {k: v.detach().cpu() for k, v in flow.state_dict().items() if v is not None}
        spec = O.spec_from_state_dict(sd, "ar", uni, D)
        x = torch.randn(NMAX, D, generator=torch.Generator().manual_seed(31)) * 1.2
        x[BAD, D // 2] = float("nan")
        sel = torch.cat([torch.arange(129), torch.arange(NMAX - 129, NMAX)])
        with torch.no_grad():
            ref32 = O.flow_log_prob(spec, x[sel])
            ref64 = O.flow_log_prob(to_f64(spec), d64(x[sel]))
        _CACHE[key] = (flow.to(dev), x.to(dev), sel, ref32, ref64)
    return _CACHE[key]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _launches(fn):
    """fn() with the entry-point profile on: (result, flow launches, per-transform launches of zk_ar_forward_static)."""
    from zuko_amd import _C

    _C.PROFILE = {}
    try:
        out = fn()
        torch.cuda.synchronize()
        prof = _C.PROFILE
    finally:
        _C.PROFILE = None
    calls = [args[0].flow_transforms for _, _, args in prof.get("zk_ar_forward_static", [])]
    return out, [c for c in calls if c > 0], sum(1 for c in calls if c == 0)


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("name", ["nsf_cfg2", "maf16"])
def test_flow_launch_is_bitwise_the_per_transform_path(dev, matmul, monkeypatch, name, T):
    matmul("f16x2")
    flow, x, sel, ref32, ref64 = _flow(name, T, dev)
    for N in ROWS:
        xn = x[:N]
        keep = torch.ones(N, dtype=torch.bool, device=dev)
        keep[BAD] = False
        with torch.no_grad():
            lp, fl, single = _launches(lambda: flow().log_prob(xn))
            assert fl == [T] and single == 0, f"{name} T={T} N={N}: log_prob made flow launches {fl} and {single} per-transform launches"
            (y, ladj), fl, single = _launches(lambda: flow().transform.call_and_ladj(xn))
            assert fl == [T] and single == 0, f"{name} T={T} N={N}: call_and_ladj made flow launches {fl} and {single} per-transform launches"
            lp2 = flow().log_prob(xn)
            y2, ladj2 = flow().transform.call_and_ladj(xn)
            monkeypatch.setenv("ZUKO_AMD_NO_FUSED_FLOW", "1")
            lp0, fl, single = _launches(lambda: flow().log_prob(xn))
            y0, ladj0 = flow().transform.call_and_ladj(xn)
            monkeypatch.delenv("ZUKO_AMD_NO_FUSED_FLOW")
        assert fl == [] and single == T, "ZUKO_AMD_NO_FUSED_FLOW=1 keeps one launch per transform"
        assert torch.equal(_bits(lp), _bits(lp2)) and torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(ladj), _bits(ladj2)), f"{name} T={T} N={N}: two runs differ"
        assert torch.equal(_bits(lp), _bits(lp0)), f"{name} T={T} N={N}: log_prob differs from the per-transform path in {int((_bits(lp) != _bits(lp0)).sum())} rows"
        assert torch.equal(_bits(y), _bits(y0)), f"{name} T={T} N={N}: y differs from the per-transform path in {int((_bits(y) != _bits(y0)).sum())} values"
        assert torch.equal(_bits(ladj), _bits(ladj0)), f"{name} T={T} N={N}: ladj differs from the per-transform path in {int((_bits(ladj) != _bits(ladj0)).sum())} rows"
        assert torch.equal(lp.isnan(), ~keep) and torch.equal(ladj.isnan(), ~keep), f"{name} T={T} N={N}: the NaN row and only it"
        assert bool(torch.isfinite(y[keep]).all()) and bool(y[BAD].isnan().any())
        rows = sel[sel < N] if N < NMAX else sel
        rows = rows[rows != BAD]
        pick = torch.isin(sel, rows)
        assert_parity(lp[rows.to(dev)], ref32[pick], ref64[pick], f"fused flow {name} T={T} N={N}: log_prob")


def test_flow_launch_declines(dev, matmul, monkeypatch):
    """Compositions the flow launch must leave to the per-transform launches, with their results: weights that require grad under grad mode, and a
    member whose weights keep the three-part kernel (one out unit 2^-20 below its layer: zuko_amd/fused.py, half_scales)."""
    matmul("f16x2")
    flow, x, _, _, _ = _flow("nsf_cfg2", 2, dev)
    xn = x[:129]
    with torch.no_grad():
        lp_ref = flow().log_prob(xn)
    lp, fl, single = _launches(lambda: flow().log_prob(xn))  # grad mode, trainable weights: the autograd path
    assert fl == [] and lp.requires_grad
    assert torch.allclose(lp.detach()[:BAD], lp_ref[:BAD], rtol=1e-4, atol=1e-4)

    import copy

    other = copy.deepcopy(flow)
    from zuko_amd.nn import MaskedLinear

    lin = [m for m in other.transform.transforms[1].hyper if isinstance(m, MaskedLinear)][1]
    with torch.no_grad():
        lin.weight[int((lin.weight * lin.mask).abs().amax(dim=1).argmax())] *= 2.0**-20
        lp, fl, single = _launches(lambda: other().log_prob(xn))
        assert fl == [] and single == 2, f"a member on the three-part kernel: flow launches {fl}, per-transform launches {single}"
        monkeypatch.setenv("ZUKO_AMD_NO_FUSED_FLOW", "1")
        lp0 = other().log_prob(xn)
        monkeypatch.delenv("ZUKO_AMD_NO_FUSED_FLOW")
    assert torch.equal(_bits(lp), _bits(lp0))
