"""The two-part (f16 x 2) fused autoregressive kernel evaluates its ReLU as one max instruction, which would turn a NaN into 0: every
path by which a NaN could reach a hidden value is closed in front of it (csrc/fused_ar_half_impl.h).  This is the path through the
hidden layers: a row whose FIRST hidden layer overflows f32 (x itself stays far inside the range the kernel's input check covers) must
come out non-finite exactly as the reference's does, and no other row may notice."""

import pytest
import torch

from oracle import zuko_oracle as O


@pytest.mark.gpu
def test_two_part_kernel_hidden_overflow_poisons_its_row_only(dev, matmul):
    from zuko_amd.flows import NSF
    from zuko_amd.nn import MaskedLinear

    matmul("f16x2")
    D, ROW = 64, 41
    N = 2 * 256 * 128 + 77  # more than two tiles per workgroup and a ragged last one
    torch.manual_seed(5)
    flow = NSF(D, 0, transforms=2, bins=8, hidden_features=[256] * 3).to(dev)  # the benchmark's conditioner (cfg2), two transforms: the second one accumulates
    t0 = flow.transform.transforms[0]
    lins = [m for m in t0.hyper if isinstance(m, MaskedLinear)]
    with torch.no_grad():  # a first layer with a gain of 2e9, taken back by the layers behind it: ordinary rows stay ordinary, every scale stays eligible (fused.half_scales)
        lins[0].weight.mul_(2e9)
        lins[0].bias.mul_(2e9)
        lins[1].weight.mul_(1e-4)
        lins[2].weight.mul_(1e-4)
        lins[3].weight.mul_(1e-1)
    x = torch.randn(N, D, generator=torch.Generator().manual_seed(1))
    xs = x.clone()
    xs[ROW] = torch.where(x[ROW] < 0, -1e31, 1e31)  # |x| = 1e31 < 65520 x 2^90 (the input check's bound); |W x| ~ 1e39 overflows f32 in the first hidden layer
    with torch.no_grad():
        lp0 = flow().log_prob(x.to(dev))
        lp1 = flow().log_prob(xs.to(dev))
        torch.cuda.synchronize()
        for t in flow.transform.transforms:
            st = t.fused_state(dev)
            assert st.half is not None and st.half_ok, "the two-part kernel must have served these launches"
        spec = O.spec_from_state_dict({k: v.detach().cpu() for k, v in flow.state_dict().items() if v is not None}, "ar", O.uni_rqs(8), D)
        ref = O.flow_log_prob(spec, xs[:128])
    lp0, lp1 = lp0.cpu(), lp1.cpu()
    assert not torch.isfinite(ref[ROW]), "the row must overflow in the reference"
    assert torch.isfinite(ref[torch.arange(128) != ROW]).all()
    assert bool(torch.isnan(lp1[ROW])) == bool(torch.isnan(ref[ROW])) and bool(torch.isinf(lp1[ROW])) == bool(torch.isinf(ref[ROW]))
    others = torch.arange(N) != ROW
    assert torch.isfinite(lp0).all()
    assert torch.equal(lp1[others], lp0[others]), "rows next to the overflowing one must not change by a bit"
