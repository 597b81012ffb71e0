"""The weight ring of the two-part fused autoregressive kernel on the GPU (csrc/fused_ar_half_impl.h: ArhRing4; its static schedule is checked on the
CPU by tests/test_half_ring_schedule.py).

Shapes: the cfg2 (NSF, 50 chunks) and cfg3 (MAF, 17 chunks) conditioners and MAF(16, [128, 128]), whose stream is three chunks — shorter than the
four-slot ring, so a slot holds the same chunk of consecutive tiles.  Rows 1, 127, 129 (the workgroup tile's edge) and 32 768 + 129, 2 * 32 768 + 129:
on the persistent grid of 256 workgroups of 128 rows the first workgroups run two and three tiles — the ring wraps from one tile into the next in
more than one slot phase (50 and 17 chunks on four slots) and the last tile requests its own rows again.  Row 100 of every batch longer than
that is NaN: its sample's NaN crosses every chunk boundary of the pass.

Per shape and batch: two consecutive runs agree bit for bit (a visibility race shows as a difference); the product launch equals its diagnostic
twin bit for bit (the spline kernels: cfg2 — the affine map has no diagnostic twin); the terminal launch is within the summation-order bound
of tests/test_gpu_fused_base.py of the two-launch path; everything is within the oracle bars of tests/parity.py (the oracle evaluates the first
129 rows and the last 129 rows of both long batches, once per shape)."""

import pytest
import torch

from conftest import build_flow, oracle_spec
from oracle import zuko_oracle as O
from parity import assert_parity, d64, to_f64

pytestmark = pytest.mark.gpu

BIG = 32768  # rows of one round of the persistent grid: 256 workgroups x 128 rows
ROWS = [1, 127, 129, BIG + 129, 2 * BIG + 129]
NMAX = ROWS[-1]
BAD = 100
_CACHE: dict = {}


def _build(name: str):
    if name == "maf16":
        import zuko_amd.flows as F

        torch.manual_seed(11)
        flow = F.MAF(16, 0, transforms=2, hidden_features=[128, 128])
        sd = {k: v.detach().cpu() for k, v in flow.state_dict().items() if v is not None}
        return flow, O.spec_from_state_dict(sd, "ar", O.UNI_AFFINE, 16)
    flow, entry = build_flow(name)
    return flow, oracle_spec(flow, entry)


def _flow(name: str, dev):
    """(flow on the device, x [NMAX, D] on the device, rows the oracle evaluated, its fp32 / fp64 log_prob of them), built once per shape."""
    if name not in _CACHE:
        flow, spec = _build(name)
        D = int(flow.transform.transforms[0].order.numel())
        x = torch.randn(NMAX, D, generator=torch.Generator().manual_seed(29)) * 1.2
        x[BAD, D // 2] = float("nan")
        sel = torch.cat([torch.arange(129), torch.arange(BIG, BIG + 129), torch.arange(2 * BIG, 2 * BIG + 129)])
        with torch.no_grad():
            ref32 = O.flow_log_prob(spec, x[sel])
            ref64 = O.flow_log_prob(to_f64(spec), d64(x[sel]))
        _CACHE[name] = (flow.to(dev), x.to(dev), sel, ref32, ref64)
    return _CACHE[name]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("name", ["nsf_cfg2", "maf_cfg3", "maf16"])
def test_ring_over_tile_wraps(dev, matmul, monkeypatch, name):
    from zuko_amd import static_ar
    from zuko_amd.nn import MaskedLinear

    matmul("f16x2")
    flow, x, sel, ref32, ref64 = _flow(name, dev)
    D = x.shape[1]
    for lazy in flow.transform.transforms[:2]:  # ascending and descending order
        st = lazy.fused_state(dev)
        assert st is not None and st.ready(NMAX)
        st.refresh([m for m in lazy.hyper if isinstance(m, MaskedLinear)])
        assert st._half_serves(x), "the two-part kernel must serve these launches"
        th = static_ar.half_tables(st.plan, st.plan.layout.kind, st.act)[0]
        assert th["NR"] == 4, "these shapes run the four-slot ring"
    for N in ROWS:
        xn = x[:N]
        keep = torch.ones(N, dtype=torch.bool, device=dev)
        if N > BAD:
            keep[BAD] = False
        # the transform launches: twice, and (splines) against the diagnostic twin
        for lazy in (flow.transform.transforms[0], flow.transform.transforms[-1]):
            st = lazy.fused_state(dev)
            y, ladj = torch.empty(N, D, device=dev), torch.empty(N, device=dev)
            y2, ladj2 = torch.empty_like(y), torch.empty_like(ladj)
            st.run(xn, y, ladj, False)
            st.run(xn, y2, ladj2, False)
            assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(ladj), _bits(ladj2)), f"{name} N={N}: two runs of the product launch differ"
            if name == "nsf_cfg2":
                K = 8
                yd, ld = torch.empty_like(y), torch.empty_like(ladj)
                bins = torch.empty(N, D, dtype=torch.int32, device=dev)
                knots = torch.empty(N, D, K + 1, device=dev)
                st.run_diag(xn, yd, ld, bins, knots)
                assert torch.equal(_bits(y), _bits(yd)) and torch.equal(_bits(ladj), _bits(ld)), f"{name} N={N}: the product launch differs from its diagnostic twin"
            if N > BAD:
                assert bool(ladj[BAD].isnan()) and bool(torch.isfinite(ladj[keep]).all()), f"{name} N={N}: the NaN row and only it"
        # log_prob: terminal launch, twice, against the two-launch path and the oracle
        with torch.no_grad():
            lp = flow().log_prob(xn)
            lp2 = flow().log_prob(xn)
            monkeypatch.setenv("ZUKO_AMD_NO_FUSED_BASE", "1")
            old = flow().log_prob(xn)
            ladj = flow().transform.call_and_ladj(xn)[1]
            monkeypatch.delenv("ZUKO_AMD_NO_FUSED_BASE")
        assert torch.equal(_bits(lp), _bits(lp2)), f"{name} N={N}: two runs of log_prob differ"
        assert torch.equal(lp.isnan(), ~keep) and torch.equal(old.isnan(), ~keep), f"{name} N={N}: the NaN row and only it"
        S = (old - ladj).abs() + ladj.abs()
        err, tol = (lp - old).abs()[keep], ((4 * D + 14) * 2.0**-24 * S)[keep]
        print(f"{name} N={N}: max |terminal - two-launch| = {err.max().item():.3e} (bound {tol.min().item():.3e} .. {tol.max().item():.3e})")
        assert bool((err <= tol).all()), f"{name} N={N}: max |terminal - two-launch| {err.max().item():.3e} above the summation-order bound {tol[err.argmax()].item():.3e}"
        rows = sel[sel < N]
        rows = rows[rows != BAD]
        pick = torch.isin(sel, rows)
        assert_parity(lp[rows.to(dev)], ref32[pick], ref64[pick], f"half ring {name} N={N}: log_prob")
