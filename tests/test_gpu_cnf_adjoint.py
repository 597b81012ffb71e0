"""GPU: the adjoint of the continuous flow.  zk_cnf_adjoint_step through the C ABI against tests/cnf_adjoint_ref.py (one reverse step, the chunk
reduction, row independence, accumulation), and the flow-level training paths with ops.CNF_ADJOINT on: log_prob and rsample gradients, the
fallbacks, the default, double backward."""

import ctypes

import numpy as np
import pytest
import torch

import cnf_adjoint_ref as ref
import cnf_ref
import parity
from conftest import T, golden
from parity import C_NOISE, assert_parity

pytestmark = pytest.mark.gpu

# (F, C, hidden, Q, fixture | seed): the smallest shapes that reach one, two and three hidden layers, F = 1 and F = 16, a partial last k-step
# (F = 3, 5, 6) and both forms of `pre` (per row with a context, one shared row without)
SHAPES = {"a": (3, 2, (64, 64), 3, "cnf_a"), "b": (5, 0, (64, 64), 3, "cnf_b"), "d": (1, 0, (16,), 3, "cnf_d"), "s3": (16, 3, (16, 48, 64), 2, 101), "s1": (6, 1, (32,), 8, 102)}
ROWS = 67  # one full 64-row group and a partial one
FLOW_KW, FLOW_SEED = dict(features=3, context=2), 17
_CASES: dict = {}
_REFS: dict = {}


class _Case:
    """A field on the device with its backward image, and the operands of one reverse step at ROWS rows."""

    def __init__(self, key, dev):
        from zuko_amd import cnf_plan
        from zuko_amd.flows import CNF

        F, C, hidden, Q, src = SHAPES[key]
        g = golden(src + ".npz") if isinstance(src, str) else None
        torch.manual_seed(0 if g is not None else src)
        flow = CNF(F, C, hidden_features=hidden, freqs=Q)
        lins = [m for m in flow.transform.ode if hasattr(m, "weight")]
        if g is not None:  # the fixture's weights
            with torch.no_grad():
                for i, lin in enumerate(lins):
                    lin.weight.copy_(T(g[f"w{i}"]))
                    lin.bias.copy_(T(g[f"b{i}"]))
        self.F, self.C, self.Q, self.hidden = F, C, Q, hidden
        self.W = [l.weight.detach().clone() for l in lins]
        self.B = [l.bias.detach().clone() for l in lins]
        self.fr = flow.transform.freqs.detach().clone()
        self.module = flow.to(dev).eval().transform
        self.dev = dev
        self.img = cnf_plan.backward_image_of(self.module, dev)
        assert self.img is not None
        self.img.refresh(self.module)
        gen = torch.Generator().manual_seed(7 + F)
        self.x = T(g["x"][:ROWS]).float() if g is not None else torch.randn(ROWS, F, generator=gen)
        self.c = None if C == 0 else (T(g["c"][:ROWS]).float() if g is not None else torch.randn(ROWS, C, generator=gen))
        self.ax = torch.randn(ROWS, F, generator=gen)
        self.al = torch.randn(ROWS, generator=gen)
        if g is not None:  # an accepted step of the fixture: the checkpoint's time is the time AFTER it
            t, dt, _ = [r for r in g["fwd_att32"] if r[2]][2]
            self.t, self.dt = float(np.float32(t + dt)), float(np.float32(dt))
        else:
            self.t, self.dt = 0.625, 0.3125

    def pre(self, c):
        lin = self.module.ode[0]
        with torch.no_grad():
            return lin.bias.detach().clone() if c is None else torch.addmm(lin.bias, c.to(self.dev), lin.weight[:, 2 * self.Q + self.F :].t()).contiguous()

    def run(self, x, ax, al, c, t=None, dt=None, gpre=None, gparams=None, pre=None, ax_next=None):
        """One launch: (ax_next, gpre, gparams) on the device; gpre / gparams are added to when given."""
        from zuko_amd import ops

        N = x.shape[0]
        x, ax = x.to(self.dev), ax.to(self.dev)
        al = None if al is None else al.to(self.dev)
        pre = self.pre(c) if pre is None else pre
        ax_next = torch.full((N, self.F), float("nan"), device=self.dev) if ax_next is None else ax_next
        gpre = torch.zeros(N, self.hidden[0], device=self.dev) if gpre is None else gpre
        gparams = torch.zeros(self.img.flat_total, device=self.dev) if gparams is None else gparams
        work = torch.full((ops.cnf_adjoint_workspace(self.img, N),), float("nan"), device=self.dev)
        ops.cnf_adjoint_step(self.img, x, ax, al, pre, self.t if t is None else t, self.dt if dt is None else dt, cnf_ref.TRACE_SCALE, ax_next, gpre, gparams, work)
        torch.cuda.synchronize()
        return ax_next, gpre, gparams

    def split(self, gparams):
        """The flat gradient as ([g W_l], [g b_l]) on the CPU."""
        from zuko_amd import cnf_plan

        w_off, b_off, _, _ = cnf_plan.flat_offsets(self.F, self.Q, self.C, self.hidden)
        gp = gparams.cpu()
        return [gp[o : o + w.numel()].reshape(w.shape) for o, w in zip(w_off, self.W)], [gp[o : o + b.numel()] for o, b in zip(b_off, self.B)]

    def reference(self, x, ax, al, c, t=None, dt=None):
        """cnf_adjoint_ref.reverse_step on the CPU in both precisions: {tag: (ax_next, gW, gB, gpre)}."""
        out = {}
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            cast = lambda v: None if v is None else v.to(dtype)
            r = ref.reverse_step([cast(w) for w in self.W], [cast(b) for b in self.B], cast(self.fr), self.t if t is None else t, self.dt if dt is None else dt, cast(x), cast(ax),
                                 cast(al), cast(c))
            out[tag] = r[:4]
        return out

    def compare(self, got, want, what):
        """ax_next and gpre per element, gparams per parameter tensor (of W0 the columns the kernel owns; b0 belongs to gpre)."""
        ax_next, gpre, gparams = got
        assert_parity(ax_next, want["32"][0], want["64"][0], what + ": ax_next")
        assert_parity(gpre, want["32"][3], want["64"][3], what + ": gpre")
        gW, gB = self.split(gparams)
        own = 2 * self.Q + self.F
        for l in range(len(self.W)):
            cols = slice(0, own) if l == 0 else slice(None)
            assert_parity(gW[l][:, cols], want["32"][1][l][:, cols], want["64"][1][l][:, cols], what + f": g W{l}")
            if l == 0:
                assert not bool(gW[0][:, own:].any()) and not bool(gB[0].any()), what + ": the context's columns of W0 and b0 are the host's"
            else:
                assert_parity(gB[l], want["32"][2][l], want["64"][2][l], what + f": g b{l}")


def _case(key, dev) -> _Case:
    if key not in _CASES:
        _CASES[key] = _Case(key, dev)
    return _CASES[key]


def _ref(key, dev, with_l):
    if (key, with_l) not in _REFS:
        k = _case(key, dev)
        _REFS[key, with_l] = k.reference(k.x, k.ax, k.al if with_l else None, k.c)
    return _REFS[key, with_l]


@pytest.mark.parametrize("with_l", [True, False], ids=["al", "value"])
@pytest.mark.parametrize("key", list(SHAPES))
def test_reverse_step_against_the_restatement(dev, key, with_l):
    k = _case(key, dev)
    got = k.run(k.x, k.ax, k.al if with_l else None, k.c)
    k.compare(got, _ref(key, dev, with_l), f"cnf adjoint step {key} {'al' if with_l else 'value'}")


def test_chunk_reduction_over_three_chunks(dev):
    """The smallest N that spans three chunks; gparams against the sum of the three chunks' references, in chunk order."""
    import zuko_amd._C as C

    k = _case("a", dev)
    rows, chunks = ctypes.c_int(), ctypes.c_int()
    N = 129
    assert C.lib().zk_cnf_adjoint_geometry(N, ctypes.byref(rows), ctypes.byref(chunks)) == 0 and chunks.value == 3 and rows.value == 64
    assert C.lib().zk_cnf_adjoint_geometry(N - 1, ctypes.byref(rows), ctypes.byref(chunks)) == 0 and chunks.value == 2
    gen = torch.Generator().manual_seed(23)
    x, c, ax, al = torch.randn(N, k.F, generator=gen), torch.randn(N, k.C, generator=gen), torch.randn(N, k.F, generator=gen), torch.randn(N, generator=gen)
    got = k.run(x, ax, al, c)
    parts = [k.reference(x[s], ax[s], al[s], c[s]) for s in (slice(0, 64), slice(64, 128), slice(128, 129))]
    want = {}
    for tag in ("32", "64"):
        gW = [parts[0][tag][1][l] + parts[1][tag][1][l] + parts[2][tag][1][l] for l in range(len(k.W))]
        gB = [parts[0][tag][2][l] + parts[1][tag][2][l] + parts[2][tag][2][l] for l in range(len(k.B))]
        want[tag] = (torch.cat([p[tag][0] for p in parts]), gW, gB, torch.cat([p[tag][3] for p in parts]))
    k.compare(got, want, "cnf adjoint three chunks")


def test_rows_are_independent_and_runs_repeat(dev):
    """ax_next / gpre of a row: the same bits in a subset of the batch, with NaN-padded row strides, alone (N = 1) and in a second run; gparams
    repeats bit for bit."""
    k = _case("a", dev)
    for al in (k.al, None):
        ax_next, gpre, gparams = k.run(k.x, k.ax, al, k.c)
        again = k.run(k.x, k.ax, al, k.c)
        assert torch.equal(ax_next, again[0]) and torch.equal(gpre, again[1]) and torch.equal(gparams, again[2])
        assert bool(torch.isfinite(ax_next).all()) and bool(torch.isfinite(gpre).all()) and bool(torch.isfinite(gparams).all())
        sel = torch.tensor([66, 3, 64, 17, 0])
        sub = k.run(k.x[sel], k.ax[sel], None if al is None else al[sel], k.c[sel])
        assert torch.equal(sub[0], ax_next[sel.to(dev)]) and torch.equal(sub[1], gpre[sel.to(dev)])
        one = k.run(k.x[5:6], k.ax[5:6], None if al is None else al[5:6], k.c[5:6])
        assert torch.equal(one[0], ax_next[5:6]) and torch.equal(one[1], gpre[5:6])
        # row strides with NaN in the padding: x [N, F + 3], ax [N, F + 1], ax_next [N, F + 2], pre [N, H + 4], gpre [N, H + 8]
        N, F, H = ROWS, k.F, k.hidden[0]
        nan = lambda *s: torch.full(s, float("nan"), device=dev)
        xp, ap, yp, pp, gp = nan(N, F + 3), nan(N, F + 1), nan(N, F + 2), nan(N, H + 4), nan(N, H + 8)
        xp[:, :F], ap[:, :F], pp[:, :H], gp[:, :H] = k.x.to(dev), k.ax.to(dev), k.pre(k.c), 0.0
        pad = k.run(xp[:, :F], ap[:, :F], al, None, pre=pp[:, :H], gpre=gp[:, :H], ax_next=yp[:, :F])
        assert torch.equal(pad[0], ax_next) and torch.equal(pad[1], gpre) and torch.equal(pad[2], gparams)
        assert bool(torch.isnan(yp[:, F:]).all()) and bool(torch.isnan(gp[:, H:]).all())
    # the unconditional case reads ONE shared row of pre
    b = _case("b", dev)
    shared = b.pre(None)
    assert shared.dim() == 1
    u, v = b.run(b.x, b.ax, b.al, None, pre=shared), b.run(b.x, b.ax, b.al, None, pre=shared.expand(ROWS, -1).contiguous())
    assert all(torch.equal(p, q) for p, q in zip(u, v))


def test_two_launches_accumulate(dev):
    """Two launches into the same gpre / gparams equal the sum of two launches into zeroed buffers: gpre bit for bit (a launch adds its stages'
    sum once), gparams too (the reduction adds the chunks' sum once)."""
    k = _case("a", dev)
    t2, dt2 = k.t - k.dt, k.dt * 0.75
    first = k.run(k.x, k.ax, k.al, k.c)
    second = k.run(k.x * 0.5, first[0].cpu(), k.al, k.c, t=t2, dt=dt2)
    gpre, gparams = first[1].clone(), first[2].clone()
    both = k.run(k.x * 0.5, first[0].cpu(), k.al, k.c, t=t2, dt=dt2, gpre=gpre, gparams=gparams)
    assert torch.equal(both[0], second[0])
    assert torch.equal(both[1], first[1] + second[1]) and torch.equal(both[2], first[2] + second[2])
    assert bool(second[1].any()) and bool(second[2].any())


def _flow_and_fixture(dev, dtype=torch.float32):
    from zuko_amd.flows import CNF

    g = golden("flow_cnf_small.npz")
    torch.manual_seed(FLOW_SEED)
    return CNF(**FLOW_KW).to(dev).to(dtype).train(), g


def test_training_gradients_on_the_kernel_path(dev, monkeypatch):
    """train() mode with the switch on: log_prob integrates on zk_cnf_step, backward on zk_cnf_adjoint_step.  The bar of the torch-op path's test:
    every parameter's gradient lies within C_NOISE times the float32 reference's own largest relative distance to the float64 reference."""
    from zuko_amd import ops

    monkeypatch.setattr(ops, "CNF_ADJOINT", True)
    flow, g = _flow_and_fixture(dev)
    names = list(g["param_names"])
    rel = lambda got, k: float((got.cpu().double() - T(g["grad/" + k]).double()).abs().max()) / float(np.abs(g["grad/" + k]).max())
    lp = flow(T(g["c"], dev)).log_prob(T(g["x"], dev))
    stats = dict(ops.CNF_STATS)
    assert stats["path"] == "kernel" and lp.requires_grad and stats["t_end"] == 1.0
    lp.mean().backward()
    assert ops.CNF_STATS["adjoint_steps"] == stats["accepted"] >= 1
    got = dict(flow.named_parameters())
    assert list(got) == names
    ref32 = max(rel(T(g["grad32/" + k]), k) for k in names)
    for k in names:
        d = rel(got[k].grad, k)
        parity.REPORT.append({"what": f"cnf adjoint training gradient {k}", "relative_to_largest_entry": d, "reference": ref32, "c": C_NOISE, "ok": d <= C_NOISE * ref32})
        print(f"cnf adjoint training gradient {k}: {d:.3e} of the largest entry, the float32 reference {ref32:.3e}")
    for k in names:
        assert rel(got[k].grad, k) <= C_NOISE * ref32, f"{k}: {rel(got[k].grad, k):.3e} > {C_NOISE:g} x {ref32:.3e}"


def test_rsample_gradients_on_the_kernel_path(dev, monkeypatch):
    """rsample(...).square().mean().backward() with the switch on: the value alone goes through the node (no trace term).  The draw of the base
    differs between precisions, so the comparison with the float64 torch-op path runs on the same map with a fixed z — transform.inv(z), what
    rsample applies to its draw — at the bar of the log_prob test."""
    from zuko_amd import ops

    flow, g = _flow_and_fixture(dev)
    c = T(g["c"], dev)[:8]
    z = torch.randn(2, 8, 3, generator=torch.Generator().manual_seed(3)).to(dev)
    names = list(g["param_names"])
    flow64, _ = _flow_and_fixture(dev, torch.float64)
    c64 = c.double().requires_grad_()
    flow64(c64).transform.inv(z.double()).square().mean().backward()
    assert ops.CNF_STATS["path"] == "torch"
    want = {k: p.grad.cpu() for k, p in flow64.named_parameters()}
    monkeypatch.setattr(ops, "CNF_ADJOINT", True)
    torch.manual_seed(3)
    r = flow(c).rsample((2,))
    assert ops.CNF_STATS["path"] == "kernel" and r.shape == (2, 8, 3) and r.grad_fn is not None
    r.square().mean().backward()
    assert ops.CNF_STATS["adjoint_steps"] == ops.CNF_STATS["accepted"]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()) for p in flow.parameters())
    flow.zero_grad()
    c32 = c.clone().requires_grad_()
    flow(c32).transform.inv(z).square().mean().backward()
    assert ops.CNF_STATS["path"] == "kernel"
    rel = lambda a, b: float((a.cpu().double() - b).abs().max()) / float(b.abs().max())
    ref32 = max(float(np.abs(g["grad32/" + k] - g["grad/" + k]).max()) / float(np.abs(g["grad/" + k]).max()) for k in names)
    got = dict(flow.named_parameters())
    for k in names:
        d = rel(got[k].grad, want[k])
        print(f"cnf adjoint rsample gradient {k}: {d:.3e} of the largest entry (bar {C_NOISE * ref32:.3e})")
        assert d <= C_NOISE * ref32, f"{k}: {d:.3e} > {C_NOISE:g} x {ref32:.3e}"
    d = rel(c32.grad, c64.grad.cpu())
    assert d <= C_NOISE * ref32, f"context: {d:.3e} > {C_NOISE:g} x {ref32:.3e}"


def test_fallbacks_with_the_switch_on(dev, monkeypatch):
    from zuko_amd import ops
    from zuko_amd.flows import CNF

    monkeypatch.setattr(ops, "CNF_ADJOINT", True)
    x, c = torch.randn(16, 3, generator=torch.Generator().manual_seed(1)).to(dev), torch.randn(16, 2, generator=torch.Generator().manual_seed(2)).to(dev)
    for kw, dtype in ((dict(hidden_features=(16, 48, 128)), torch.float32), ({}, torch.float64), (dict(exact=False), torch.float32)):
        torch.manual_seed(5)
        flow = CNF(3, 2, **kw).to(dev).to(dtype).train()
        lp = flow(c.to(dtype)).log_prob(x.to(dtype))
        assert ops.CNF_STATS["path"] == "torch" and lp.requires_grad, kw
    # eval(): the parameters are not in phi; without a gradient to x or c nothing is recorded, with one the node serves x and c only
    torch.manual_seed(5)
    flow = CNF(3, 2).to(dev).eval()
    lp = flow(c).log_prob(x)
    assert ops.CNF_STATS["path"] == "kernel" and not lp.requires_grad
    xg = x.clone().requires_grad_()
    flow(c).log_prob(xg).sum().backward()
    assert ops.CNF_STATS["path"] == "kernel" and xg.grad is not None and all(p.grad is None for p in flow.parameters())


def test_the_switch_is_off_by_default(dev):
    import zuko_amd._C as C
    from zuko_amd import ops

    assert ops.CNF_ADJOINT is False
    flow, g = _flow_and_fixture(dev)
    keep = C.PROFILE
    C.PROFILE = {}
    try:
        flow(T(g["c"], dev)[:8]).log_prob(T(g["x"], dev)[:8]).mean().backward()
        calls = dict(C.PROFILE)
    finally:
        C.PROFILE = keep
    assert ops.CNF_STATS["path"] == "torch" and len(calls.get("zk_cnf_adjoint_step", [])) == 0 and "adjoint_steps" not in ops.CNF_STATS


def test_double_backward_raises(dev, monkeypatch):
    from zuko_amd import ops

    monkeypatch.setattr(ops, "CNF_ADJOINT", True)
    flow, g = _flow_and_fixture(dev)
    x = T(g["x"], dev)[:8].clone().requires_grad_()
    lp = flow(T(g["c"], dev)[:8]).log_prob(x).sum()
    assert ops.CNF_STATS["path"] == "kernel"
    (gx,) = torch.autograd.grad(lp, x, create_graph=True)
    with pytest.raises(RuntimeError):
        gx.sum().backward()
