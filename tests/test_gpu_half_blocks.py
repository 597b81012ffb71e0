"""The two-part fused autoregressive kernel with its blocks as single inline-assembly statements (csrc/fused_ar_half_impl.h: arh_wait_block — the counted
wait and the three matrix instructions of a block in one string, the wait states behind a tile's last block written by hand — and arh_relu_max: an out
tile's ReLU and its entry into the sample maximum behind the tile's descale).  A wait that is too short, or a vector instruction that reads an
accumulator early, shows here as an O(1) or a run-to-run difference; tests/test_codegen_half_padding.py counts the wait states in the ISA.

Flows: T = 2 and 3 of MAF(16, [128, 128]) — a pass of three chunks, and out tiles whose first block is also their last — and of the cfg2 conditioner
NSF(64, [256] * 3, 8 bins).  Rows: 129 (a second tile with one live row) and 32 897 (257 tiles: on the grid of 256 workgroups one owns two).  Row 100
is NaN.  Per case: two evaluations are bitwise equal; the flow launch, the per-transform launches (ZUKO_AMD_NO_FUSED_FLOW=1) and — the spline flows —
the chain of diagnostic twins give bitwise the same y and log-determinant; log_prob meets the bars of tests/parity.py against the oracle and against the
unchanged three-part kernel (set_matmul_precision("bf16x3")); only the NaN row is NaN."""

import pytest
import torch

from oracle import zuko_oracle as O
from parity import assert_parity, d64, to_f64

pytestmark = pytest.mark.gpu

ROWS = [129, 256 * 128 + 129]
NMAX = ROWS[-1]
BAD = 100
_CACHE: dict = {}


def _flow(name: str, T: int, dev):
    """(flow on the device, x [NMAX, D] on the device, rows the oracle evaluated, its fp32 / fp64 log_prob of them), built once per case."""
    key = (name, T)
    if key not in _CACHE:
        import zuko_amd.flows as F

        torch.manual_seed(17 + T)
        if name == "nsf_cfg2":
            D, uni = 64, O.uni_rqs(8)
            flow = F.NSF(features=D, context=0, transforms=T, bins=8, hidden_features=[256] * 3)
        else:
            D, uni = 16, O.UNI_AFFINE
            flow = F.MAF(D, 0, transforms=T, hidden_features=[128, 128])
        sd = {k: v.detach().cpu() for k, v in flow.state_dict().items() if v is not None}
        spec = O.spec_from_state_dict(sd, "ar", uni, D)
        x = torch.randn(NMAX, D, generator=torch.Generator().manual_seed(37)) * 1.2
        x[BAD, D // 2] = float("nan")
        sel = torch.cat([torch.arange(129), torch.arange(NMAX - 129, NMAX)])
        with torch.no_grad():
            ref32 = O.flow_log_prob(spec, x[sel])
            ref64 = O.flow_log_prob(to_f64(spec), d64(x[sel]))
        _CACHE[key] = (flow.to(dev), x.to(dev), sel, ref32, ref64)
    return _CACHE[key]


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def _twin_chain(flow, xn, dev):
    """y and the summed log-determinant of the transforms' diagnostic twins, launched one after the other (the sum in the flow kernel's order)."""
    N, D = xn.shape
    cur, total = xn, None
    for lazy in flow.transform.transforms:
        st = lazy.fused_state(dev)
        y, ld = torch.empty(N, D, device=dev), torch.empty(N, device=dev)
        st.run_diag(cur, y, ld, torch.empty(N, D, dtype=torch.int32, device=dev), torch.empty(N, D, 9, device=dev))
        cur, total = y, (ld if total is None else total + ld)
    return cur, total


@pytest.mark.parametrize("N", ROWS)
@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("name", ["maf16", "nsf_cfg2"])
def test_blocks_as_single_statements(dev, matmul, monkeypatch, name, T, N):
    matmul("f16x2")
    flow, x, sel, ref32, ref64 = _flow(name, T, dev)
    xn = x[:N]
    keep = torch.ones(N, dtype=torch.bool, device=dev)
    keep[BAD] = False
    with torch.no_grad():
        lp, (y, ladj) = flow().log_prob(xn), flow().transform.call_and_ladj(xn)
        lp2, (y2, ladj2) = flow().log_prob(xn), flow().transform.call_and_ladj(xn)
        monkeypatch.setenv("ZUKO_AMD_NO_FUSED_FLOW", "1")
        lp0, (y0, ladj0) = flow().log_prob(xn), flow().transform.call_and_ladj(xn)
        monkeypatch.delenv("ZUKO_AMD_NO_FUSED_FLOW")
        if name == "nsf_cfg2":
            yd, ld = _twin_chain(flow, xn, dev)
        matmul("bf16x3")
        lp3 = flow().log_prob(xn)
        matmul("f16x2")
    tag = f"{name} T={T} N={N}"
    assert torch.equal(_bits(lp), _bits(lp2)) and torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(ladj), _bits(ladj2)), f"{tag}: two evaluations differ"
    assert torch.equal(_bits(lp), _bits(lp0)), f"{tag}: log_prob differs from the per-transform launches in {int((_bits(lp) != _bits(lp0)).sum())} rows"
    assert torch.equal(_bits(y), _bits(y0)), f"{tag}: y differs from the per-transform launches in {int((_bits(y) != _bits(y0)).sum())} values"
    assert torch.equal(_bits(ladj), _bits(ladj0)), f"{tag}: ladj differs from the per-transform launches in {int((_bits(ladj) != _bits(ladj0)).sum())} rows"
    if name == "nsf_cfg2":
        assert torch.equal(_bits(y[keep]), _bits(yd[keep])), f"{tag}: y differs from the diagnostic twins in {int((_bits(y[keep]) != _bits(yd[keep])).sum())} values"
        assert torch.equal(_bits(ladj[keep]), _bits(ld[keep])), f"{tag}: ladj differs from the diagnostic twins in {int((_bits(ladj[keep]) != _bits(ld[keep])).sum())} rows"
        assert bool(ld[BAD].isnan())
    assert torch.equal(lp.isnan(), ~keep) and torch.equal(ladj.isnan(), ~keep) and torch.equal(lp3.isnan(), ~keep), f"{tag}: the NaN row and only it"
    assert bool(torch.isfinite(y[keep]).all()) and bool(y[BAD].isnan().any())
    rows = sel[sel < N] if N < NMAX else sel
    rows = rows[rows != BAD]
    pick = torch.isin(sel, rows)
    assert_parity(lp[rows.to(dev)], ref32[pick], ref64[pick], f"half blocks {tag}: log_prob")
    assert_parity(lp[rows.to(dev)], lp3[rows.to(dev)], ref64[pick], f"half blocks {tag}: log_prob against the three-part kernel")
