"""CPU: the oracle's coupling layer with the spline univariate against the live reference's recorded results
(tests/golden/flow_nice_rqs_small.npz, written by tests/golden/make_golden_coupling_rqs.py) — bit for bit."""

import torch

from conftest import T, golden
from oracle import zuko_oracle as O


def test_oracle_reproduces_the_reference_spline_coupling_flow_bitwise():
    g = golden("flow_nice_rqs_small.npz")
    sd = {k[3:]: T(v) for k, v in g.items() if k.startswith("sd/")}
    spec = O.spec_from_state_dict(sd, "coupling", O.uni_rqs(8), 5)
    assert len(spec.layers) == 3 and all(tuple(l.weights[-1].shape) == (l.uni.total * int((~l.mask).sum()), 32) for l in spec.layers)
    x, c = T(g["x"]), T(g["c"])
    assert x.shape == (64, 5) and c.shape == (64, 3) and float((x.abs() > 5).float().mean()) > 0.0  # the identity tails are exercised
    with torch.no_grad():
        z, ladj = O.flow_forward(spec, x, c)
        lp = O.flow_log_prob(spec, x, c)
        inv = O.flow_inverse(spec, T(g["z"]), c)
    assert torch.equal(z, T(g["z"])) and torch.equal(ladj, T(g["ladj"]))
    assert torch.equal(lp, T(g["log_prob"]))
    assert torch.equal(inv, T(g["inv"]))
