"""The two-part fused autoregressive kernel with the operand split of in pair p + 1 standing among the matrix instructions of the consuming layer's
blocks (csrc/fused_ar_half_impl.h: ARH_SPLIT_GAPS, arh_gap_plan).  The split instructions are the same, so every result is BITWISE the one of a build with
the switch off; a split that ends behind its first reader, or reads an out tile the layer has already overwritten, shows as an O(1) difference.

Cases, rows and the two poisoned rows: tests/half_gaps_cases.py.  Per case: two evaluations are bitwise equal; the flow launch, the per-transform launches
(ZUKO_AMD_NO_FUSED_FLOW=1) and — the spline flow — the chain of diagnostic twins give bitwise the same y and log-determinant; all are bitwise equal to the
build with the switch off, made and evaluated by a child process in a cache directory of its own (once per session); log_prob meets the bars of
tests/parity.py against the oracle; the two poisoned rows, and only they, are NaN."""

import os
import subprocess
import sys

import pytest
import torch

import half_gaps_cases as C
from oracle import zuko_oracle as O
from parity import assert_parity, d64, to_f64

pytestmark = pytest.mark.gpu

_CACHE: dict = {}


def _flow(name: str, T: int, dev):
    """(flow on the device, x [NMAX, D] on the device, rows the oracle evaluated, its fp32 / fp64 log_prob of them), built once per case."""
    key = (name, T)
    if key not in _CACHE:
        flow, D = C.build_flow(name, T)
        uni = O.uni_rqs(8) if name == "nsf_cfg2" else O.UNI_AFFINE
        sd = {k: v.detach().cpu() for k, v in flow.state_dict().items() if v is not None}
        spec = O.spec_from_state_dict(sd, "ar", uni, D)
        x = C.inputs(D)
        sel = torch.cat([torch.arange(129), torch.arange(C.NMAX - 129, C.NMAX)])
        sel = sel[(sel != C.BAD) & (sel != C.OVER)]
        with torch.no_grad():
            ref32 = O.flow_log_prob(spec, x[sel])
            ref64 = O.flow_log_prob(to_f64(spec), d64(x[sel]))
        _CACHE[key] = (flow.to(dev), x.to(dev), sel, ref32, ref64)
    return _CACHE[key]


@pytest.fixture(scope="module")
def switched_off(tmp_path_factory):
    """{(name, T, N): (log_prob, y, ladj)} of the build with -DARH_SPLIT_GAPS=0: compiled into its own cache directory and evaluated by a child process."""
    out = str(tmp_path_factory.mktemp("half_gaps_off"))
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "half_gaps_cases.py"), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    return torch.load(os.path.join(out, "outputs.pt"))


@pytest.fixture(scope="module")
def odd_tiles_kernels(tmp_path_factory):
    """The shipped-default kernels of MAF(16, [112, 112]), which is not a prebuilt shape: compiled into a cache directory that this module's lookups
    search first."""
    from zuko_amd import static_ar

    out = str(tmp_path_factory.mktemp("half_gaps_maf112"))
    static_ar.build_half_variant([C.MAF112], out)
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("ZUKO_AMD_CACHE_DIR", out)
        static_ar.rescan()
        yield out
    static_ar.rescan()


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


@pytest.mark.parametrize("N", C.ROWS)
@pytest.mark.parametrize("name,T", C.CASES)
def test_split_among_the_matrix_instructions(dev, matmul, monkeypatch, request, switched_off, name, T, N):
    matmul("f16x2")
    if name == "maf112":
        request.getfixturevalue("odd_tiles_kernels")
    flow, x, sel, ref32, ref64 = _flow(name, T, dev)
    xn = x[:N]
    keep = torch.ones(N, dtype=torch.bool, device=dev)
    keep[C.BAD] = keep[C.OVER] = False
    lp, y, ladj = C.evaluate(flow, xn)
    lp2, y2, ladj2 = C.evaluate(flow, xn)
    monkeypatch.setenv("ZUKO_AMD_NO_FUSED_FLOW", "1")
    lp0, y0, ladj0 = C.evaluate(flow, xn)
    monkeypatch.delenv("ZUKO_AMD_NO_FUSED_FLOW")
    assert C.served_by_two_part_kernels(flow, dev), "the two-part kernels must have served these launches"
    tag = f"{name} T={T} N={N}"
    assert torch.equal(_bits(lp), _bits(lp2)) and torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(ladj), _bits(ladj2)), f"{tag}: two evaluations differ"
    for what, a, b in (("log_prob", lp, lp0), ("y", y, y0), ("ladj", ladj, ladj0)):
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: {what} differs from the per-transform launches in {int((_bits(a) != _bits(b)).sum())} values"
    if name == "nsf_cfg2":
        with torch.no_grad():
            yd, ld = _twin_chain(flow, xn, dev)
        assert torch.equal(_bits(y[keep]), _bits(yd[keep])), f"{tag}: y differs from the diagnostic twins in {int((_bits(y[keep]) != _bits(yd[keep])).sum())} values"
        assert torch.equal(_bits(ladj[keep]), _bits(ld[keep])), f"{tag}: ladj differs from the diagnostic twins in {int((_bits(ladj[keep]) != _bits(ld[keep])).sum())} rows"
        assert bool(ld[C.BAD].isnan()) and bool(ld[C.OVER].isnan())
    for what, a, b in zip(("log_prob", "y", "ladj"), (lp, y, ladj), switched_off[(name, T, N)]):
        b = b.to(dev)
        assert torch.equal(_bits(a), _bits(b)), f"{tag}: {what} differs from the build with the switch off in {int((_bits(a) != _bits(b)).sum())} values"
    assert torch.equal(lp.isnan(), ~keep) and torch.equal(ladj.isnan(), ~keep), f"{tag}: the two poisoned rows and only they"
    assert bool(torch.isfinite(y[keep]).all()) and bool(y[C.BAD].isnan().any()) and bool(y[C.OVER].isnan().any())
    rows = sel[sel < N] if N < C.NMAX else sel
    pick = torch.isin(sel, rows)
    assert_parity(lp[rows.to(dev)], ref32[pick], ref64[pick], f"half gaps {tag}: log_prob")
