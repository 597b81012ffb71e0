"""GPU: the continuous flow under Hutchinson's estimator on the kernels (ops.CNF_HUTCHINSON).  zk_cnf_step_v2 with a probe against tests/cnf_ref.py:
step(..., eps=) at the fixtures' pinned attempts, row independence, the v2 blocks' refusals; the flow level against the reference's fixture
(tests/golden/make_golden_cnf_hutch.py) and the float64 truth at the reference's own distance; the draw of the probe; zk_cnf_adjoint_step_v2 against
tests/cnf_hutch_adjoint_ref.py; training gradients with both switches on; every fallback and the default."""

import numpy as np
import pytest
import torch

import cnf_hutch_adjoint_ref as href
import cnf_ref
import parity
from conftest import T, golden
from parity import C_NOISE, assert_parity
from test_gpu_cnf import ATOL, KERNEL_CASES, RTOL, _distances, _flow, _restated, _Stepper
from test_gpu_cnf_adjoint import ROWS, SHAPES, _case

pytestmark = pytest.mark.gpu

FLOW_KW, FLOW_SEED = dict(features=3, context=2, exact=False), 17
_RESTATED: dict = {}


def _probe(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def _step(st, x, l, pre, t, dt, eps, y=None):
    """zk_cnf_step (eps None) / zk_cnf_step_v2 on a _Stepper's image: (y, l_next, rows, err)."""
    from zuko_amd import ops

    N = x.shape[0]
    y = torch.full((N, x.shape[1]), float("nan"), device=st.dev) if y is None else y
    ln = torch.full((N,), float("nan"), device=st.dev)
    err, rows = torch.zeros(1, device=st.dev), torch.full((N,), float("nan"), device=st.dev)
    ops.cnf_step(st.img, x, l, pre, float(t), float(dt), ATOL, RTOL, cnf_ref.TRACE_SCALE, y, ln, err, rows, eps=eps)
    torch.cuda.synchronize()
    return y, ln, rows, err


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_step_kernel_with_a_probe_at_the_pinned_attempts(dev, name):
    g = golden(name + ".npz")
    st = _Stepper(name, dev)
    c = T(g["c"]) if "c" in g else None
    pre = st.pre(None if c is None else c.to(dev))
    att = g["fwd_att32"]
    for k, i in enumerate(g["fwd_pin"]):
        x, l = T(g[f"fwd_pin{k}_x"]), T(g[f"fwd_pin{k}_l"])
        eps = _probe(x.shape, 50 + k)
        want = {}
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            W, B, fr = cnf_ref.params_of(g, dtype)
            want[tag] = cnf_ref.step(W, B, fr, att[i, 0], att[i, 1], x.to(dtype), l.to(dtype), None if c is None else c.to(dtype), eps=eps.to(dtype))
        y, ln, rows, err = _step(st, x.to(dev), l.to(dev), pre, att[i, 0], att[i, 1], eps.to(dev))
        what = f"cnf probe step {name} attempt {i}"
        assert_parity(y, want["32"][0], want["64"][0], what + ": y")
        assert_parity(ln, want["32"][1], want["64"][1], what + ": l")
        assert_parity(rows, want["32"][2], want["64"][2], what + ": ratio")
        assert torch.equal(err.view(torch.int32), rows.max().reshape(1).view(torch.int32)), f"{what}: err {err.item()!r} != max of the rows {rows.max().item()!r}"
        exact = _step(st, x.to(dev), l.to(dev), pre, att[i, 0], att[i, 1], None)
        assert torch.equal(y, exact[0]), f"{what}: y depends on the mode"
        assert not torch.equal(ln, exact[1]), f"{what}: the probe was not used"
        zero = _step(st, x.to(dev), l.to(dev), pre, att[i, 0], att[i, 1], torch.zeros_like(eps).to(dev))
        assert torch.equal(zero[0], y) and torch.equal(zero[1], l.to(dev)), f"{what}: a zero probe moves l"


def test_step_kernel_with_a_probe_rows_are_independent(dev):
    """A row's outputs: the same bits in a subset of the batch, alone (N = 1), with NaN-padded row strides of x and eps, and in a second run."""
    g = golden("cnf_a.npz")
    st = _Stepper("cnf_a", dev)
    pre = st.pre(T(g["c"], dev))
    x = T(g["x"], dev)  # 67 rows: one full block and a partial one
    N, F = x.shape
    l = torch.linspace(-0.01, 0.01, N, device=dev)
    eps = _probe(x.shape, 9).to(dev)
    y, ln, rows, err = _step(st, x, l, pre, 0.25, 0.125, eps)
    again = _step(st, x, l, pre, 0.25, 0.125, eps)
    assert all(torch.equal(u, v) for u, v in zip((y, ln, rows, err), again))
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(ln).all()) and float(err) == float(rows.max())
    sel = torch.tensor([66, 3, 64, 17, 0], device=dev)
    ys, ls, rs, es = _step(st, x[sel].contiguous(), l[sel].contiguous(), pre[sel].contiguous(), 0.25, 0.125, eps[sel].contiguous())
    assert torch.equal(ys, y[sel]) and torch.equal(ls, ln[sel]) and torch.equal(rs, rows[sel]) and float(es) == float(rows[sel].max())
    y1, l1, r1, e1 = _step(st, x[5:6].contiguous(), l[5:6].contiguous(), pre[5:6].contiguous(), 0.25, 0.125, eps[5:6].contiguous())
    assert torch.equal(y1, y[5:6]) and torch.equal(l1, ln[5:6]) and torch.equal(r1, rows[5:6]) and float(e1) == float(rows[5])
    xp, ep, yp = (torch.full((N, F + k), float("nan"), device=dev) for k in (3, 5, 2))
    xp[:, :F], ep[:, :F] = x, eps
    y2, l2, r2, e2 = _step(st, xp[:, :F], l, pre, 0.25, 0.125, ep[:, :F], y=yp[:, :F])
    assert torch.equal(y2, y) and torch.equal(l2, ln) and torch.equal(r2, rows) and torch.equal(e2, err) and bool(torch.isnan(yp[:, F:]).all())


def test_v2_block_refusals_and_the_v1_call_through_it(dev):
    import zuko_amd._C as C

    g = golden("cnf_a.npz")
    st = _Stepper("cnf_a", dev)
    pre = st.pre(T(g["c"], dev))
    x = T(g["x"], dev)
    N, F = x.shape
    l, eps = torch.zeros(N, device=dev), _probe(x.shape, 9).to(dev)
    lay = st.img.layout
    w = list(lay.widths) + [0, 0]
    EINVAL = 1

    def call(struct="zk_cnf_args_v2", fn="zk_cnf_step_v2", edit=None, **kw):
        y, ln, err = torch.full((N, F), float("nan"), device=dev), torch.full((N,), float("nan"), device=dev), torch.zeros(1, device=dev)
        base = dict(features=F, freqs=lay.Q, n_hidden=len(lay.widths), width0=w[0], width1=w[1], width2=w[2], image_floats=lay.total, n_tangents=F, N=N, ldx=F, ldy=F,
                    ld_pre=pre.stride(0), t=0.25, dt=0.125, atol=ATOL, rtol=RTOL, trace_scale=cnf_ref.TRACE_SCALE, x=x.data_ptr(), l=l.data_ptr(), pre=pre.data_ptr(),
                    image=st.img.data.data_ptr(), y=y.data_ptr(), l_next=ln.data_ptr(), err=err.data_ptr())
        base.update(kw)
        a = C.args(struct, **base)
        if edit:
            edit(a)
        rc = getattr(C.lib(), fn)(a, C.stream())
        torch.cuda.synchronize()
        return rc, y, ln, err

    def resize(a):
        a.struct_size -= 8

    def reversion(a):
        a.version = 1

    probe = dict(eps=eps.data_ptr(), ld_eps=F)
    for rc, y, ln, err in (call(**probe, n_tangents=0), call(**probe, n_tangents=0, l=None, l_next=None), call(eps=eps.data_ptr(), ld_eps=F - 1), call(edit=resize, **probe),
                           call(edit=reversion, **probe), call(edit=reversion)):
        assert rc == EINVAL and bool(torch.isnan(y).all()) and bool(torch.isnan(ln).all()) and float(err) == 0.0  # (refused before any launch)
    v1, v2, v2p = call("zk_cnf_args_v1", "zk_cnf_step"), call(), call(**probe)
    assert v1[0] == v2[0] == v2p[0] == 0 and all(torch.equal(u, v) for u, v in zip(v1[1:], v2[1:]))
    assert torch.equal(v2p[1], v1[1]) and not torch.equal(v2p[2], v1[2])


def _fixture_flow(dev, dtype=torch.float32, train=False):
    from zuko_amd.flows import CNF

    torch.manual_seed(FLOW_SEED)
    flow = CNF(**FLOW_KW).to(dev).to(dtype)
    return flow.train() if train else flow.eval()


def _log_prob(z, ladj):
    return -0.5 * (z**2).sum(-1) - 0.5 * z.shape[-1] * np.log(2 * np.pi) + ladj


def _cnf_a_restated(eps, key):
    """What _distances needs for cnf_a's weights with a probe, from cnf_ref on the CPU, computed once per probe."""
    if key not in _RESTATED:
        g = golden("cnf_a.npz")
        W, B, fr = cnf_ref.params_of(g, torch.float32)
        _RESTATED[key] = _restated(W, B, fr, T(g["x"]), T(g["c"]), eps=eps)
    return _RESTATED[key]


@pytest.mark.parametrize("name", ["flow_cnf_hutch", "cnf_a"])
def test_flow_level_on_the_kernel_with_the_switch_on(dev, monkeypatch, name):
    """call_and_ladj(x, eps=) of an exact=False transform without gradients: on the kernel, at the reference's own distance from the float64 truth.
    (Without the feature the call takes the torch-op path.)"""
    from zuko_amd import ops

    monkeypatch.setattr(ops, "CNF_HUTCHINSON", True)
    if name == "flow_cnf_hutch":
        g = golden("flow_cnf_hutch.npz")
        flow, eps, ref = _fixture_flow(dev), T(g["eps"]), g
        exact_lp = None
    else:
        g = golden("cnf_a.npz")
        flow, eps = _flow("cnf_a", dev, exact=False), _probe(g["x"].shape, 5)
        ref, exact_lp = _cnf_a_restated(eps, "seed 5"), T(g["lp_truth"])
    x, c = T(g["x"], dev), T(g["c"], dev)
    with torch.no_grad():
        z, ladj = flow.transform(c).call_and_ladj(x, eps=eps.to(dev))
    stats = dict(ops.CNF_STATS)
    assert stats["path"] == "kernel" and stats["trace"] == "hutchinson" and stats["t_end"] == 1.0 and stats["accepted"] >= 1, stats
    parity.REPORT.append({"what": f"cnf hutchinson {name}: attempts", "attempts": stats["attempts"], "accepted": stats["accepted"], "ok": True})
    lp = _log_prob(z, ladj)
    _distances(lp, z, ref, f"cnf hutchinson {name}")
    if exact_lp is None:
        with torch.no_grad():
            exact_lp = _flow("flow_cnf_small", dev)(c).log_prob(x).cpu().double()
        assert ops.CNF_STATS["trace"] == "exact"
    assert float((lp.cpu().double() - exact_lp).abs().max()) > 1e-3  # (the estimate is not the exact trace: the probe was used)


def test_the_draw_of_the_probe(dev, monkeypatch):
    """eps = None: ONE torch.randn_like(x) before the integration on both paths — the same probe and the same generator state under the same seed."""
    from zuko_amd import ops

    g = golden("cnf_a.npz")
    flow = _flow("cnf_a", dev, exact=False)
    x, c = T(g["x"], dev), T(g["c"], dev)
    torch.manual_seed(123)
    drawn = torch.randn_like(x)
    ref = _cnf_a_restated(drawn.cpu(), "drawn 123")
    out, states = {}, {}
    for on in (True, False):
        monkeypatch.setattr(ops, "CNF_HUTCHINSON", on)
        torch.manual_seed(123)
        with torch.no_grad():
            z, ladj = flow.transform(c).call_and_ladj(x)
        assert ops.CNF_STATS["path"] == ("kernel" if on else "torch")
        states[on] = torch.cuda.get_rng_state(dev)
        out[on] = (z, _log_prob(z, ladj))
        _distances(out[on][1], z, ref, f"cnf hutchinson drawn probe, switch {'on' if on else 'off'}")
    assert torch.equal(states[True], states[False])
    monkeypatch.setattr(ops, "CNF_HUTCHINSON", True)
    with torch.no_grad():
        a, b = flow.transform(c).call_and_ladj(x)[1], flow.transform(c).call_and_ladj(x)[1]
        assert ops.CNF_STATS["path"] == "kernel" and float((a - b).abs().max()) > 1e-3  # (two draws)
        # x [1, 3] against c [67, 2]: the probe is drawn like x, the kernel's rows are the broadcast ones — the call goes to the torch-op path, whose
        # vector-Jacobian product refuses a probe of another shape than the field's value, as the reference's does
        with pytest.raises(RuntimeError, match="shape"):
            flow.transform(c).call_and_ladj(x[:1])
        assert ops.CNF_STATS["path"] == "torch"


def _adjoint(k, x, ax, al, c, eps, t=None, dt=None, gpre=None, gparams=None, pre=None, v1=False):
    """One launch of zk_cnf_adjoint_step_v2 (zk_cnf_adjoint_step with v1) on a _Case of tests/test_gpu_cnf_adjoint.py: (ax_next, gpre, gparams)."""
    from zuko_amd import ops

    N, dev = x.shape[0], k.dev
    pre = k.pre(c) if pre is None else pre
    ax_next = torch.full((N, k.F), float("nan"), device=dev)
    gpre = torch.zeros(N, k.hidden[0], device=dev) if gpre is None else gpre
    gparams = torch.zeros(k.img.flat_total, device=dev) if gparams is None else gparams
    work = torch.full((ops.cnf_adjoint_workspace(k.img, N),), float("nan"), device=dev)
    ops.cnf_adjoint_step(k.img, x.to(dev), ax.to(dev), None if al is None else al.to(dev), pre, k.t if t is None else t, k.dt if dt is None else dt, cnf_ref.TRACE_SCALE, ax_next,
                         gpre, gparams, work, eps=None if v1 else eps.to(dev))
    torch.cuda.synchronize()
    return ax_next, gpre, gparams


@pytest.mark.parametrize("key", list(SHAPES))
def test_reverse_step_with_a_probe_against_the_restatement(dev, key):
    """Every shape (with a context: pre per row; without: one shared row) in both precisions; without al the v1 call's bits; a second run's bits."""
    k = _case(key, dev)
    eps = _probe(k.x.shape, 300 + k.F)
    want = {}
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        cast = lambda v: None if v is None else v.to(dtype)
        want[tag] = href.reverse_step([cast(w) for w in k.W], [cast(b) for b in k.B], cast(k.fr), k.t, k.dt, cast(k.x), cast(k.ax), cast(k.al), cast(eps), cast(k.c))[:4]
    got = _adjoint(k, k.x, k.ax, k.al, k.c, eps)
    k.compare(got, want, f"cnf probe adjoint step {key}")
    again = _adjoint(k, k.x, k.ax, k.al, k.c, eps)
    assert all(torch.equal(u, v) for u, v in zip(got, again))
    exact = _adjoint(k, k.x, k.ax, k.al, k.c, eps, v1=True)
    assert not torch.equal(got[0], exact[0]) and not torch.equal(got[2], exact[2])  # (the probe was used)
    value, value1 = _adjoint(k, k.x, k.ax, None, k.c, eps), _adjoint(k, k.x, k.ax, None, k.c, eps, v1=True)
    assert all(torch.equal(u, v) for u, v in zip(value, value1))
    if k.C == 0:  # ONE shared row of pre, or the same row for every x row
        rows = _adjoint(k, k.x, k.ax, k.al, None, eps, pre=k.pre(None).expand(ROWS, -1).contiguous())
        assert k.pre(None).dim() == 1 and all(torch.equal(u, v) for u, v in zip(got, rows))


def test_two_probe_launches_accumulate_and_rows_are_independent(dev):
    k = _case("a", dev)
    eps = _probe(k.x.shape, 303)
    t2, dt2 = k.t - k.dt, k.dt * 0.75
    first = _adjoint(k, k.x, k.ax, k.al, k.c, eps)
    second = _adjoint(k, k.x * 0.5, first[0].cpu(), k.al, k.c, eps, t=t2, dt=dt2)
    both = _adjoint(k, k.x * 0.5, first[0].cpu(), k.al, k.c, eps, t=t2, dt=dt2, gpre=first[1].clone(), gparams=first[2].clone())
    assert torch.equal(both[0], second[0]) and torch.equal(both[1], first[1] + second[1]) and torch.equal(both[2], first[2] + second[2])
    assert bool(second[1].any()) and bool(second[2].any())
    sel = torch.tensor([66, 3, 64, 17, 0])
    sub = _adjoint(k, k.x[sel], k.ax[sel], k.al[sel], k.c[sel], eps[sel])
    assert torch.equal(sub[0], first[0][sel.to(dev)]) and torch.equal(sub[1], first[1][sel.to(dev)])
    one = _adjoint(k, k.x[5:6], k.ax[5:6], k.al[5:6], k.c[5:6], eps[5:6])
    assert torch.equal(one[0], first[0][5:6]) and torch.equal(one[1], first[1][5:6])


def _loss(flow, x, c, eps):
    d = flow(c)
    z, ladj = d.transform.call_and_ladj(x, eps=eps)
    return -(d.base.log_prob(z) + ladj).mean()


def test_training_gradients_on_the_kernel_path_with_a_probe(dev, monkeypatch):
    """train() mode with both switches on: the bar of test_gpu_cnf_adjoint.py: test_training_gradients_on_the_kernel_path against the reference's
    gradients under the fixture's probe."""
    from zuko_amd import ops

    monkeypatch.setattr(ops, "CNF_ADJOINT", True)
    monkeypatch.setattr(ops, "CNF_HUTCHINSON", True)
    g = golden("flow_cnf_hutch.npz")
    flow = _fixture_flow(dev, train=True)
    names = list(g["param_names"])
    x, c, eps = T(g["x"], dev), T(g["c"], dev), T(g["eps"], dev)
    rel = lambda got, k: float((got.cpu().double() - T(g["grad/" + k]).double()).abs().max()) / float(np.abs(g["grad/" + k]).max())
    loss = _loss(flow, x, c, eps)
    stats = dict(ops.CNF_STATS)
    assert stats["path"] == "kernel" and stats["trace"] == "hutchinson" and loss.requires_grad and stats["t_end"] == 1.0, stats
    loss.backward()
    assert ops.CNF_STATS["adjoint_steps"] == stats["accepted"] >= 1
    got = dict(flow.named_parameters())
    assert list(got) == names
    ref32 = max(rel(T(g["grad32/" + k]), k) for k in names)
    for k in names:
        d = rel(got[k].grad, k)
        parity.REPORT.append({"what": f"cnf hutchinson training gradient {k}", "relative_to_largest_entry": d, "reference": ref32, "c": C_NOISE, "ok": d <= C_NOISE * ref32})
        print(f"cnf hutchinson training gradient {k}: {d:.3e} of the largest entry, the float32 reference {ref32:.3e}")
    for k in names:
        assert rel(got[k].grad, k) <= C_NOISE * ref32, f"{k}: {rel(got[k].grad, k):.3e} > {C_NOISE:g} x {ref32:.3e}"
    # eval(): the parameters are not in phi; the node serves x and the context
    flow.eval()
    flow.zero_grad()
    xg, cg = x[:8].clone().requires_grad_(), c[:8].clone().requires_grad_()
    loss = _loss(flow, xg, cg, eps[:8])
    assert ops.CNF_STATS["path"] == "kernel" and ops.CNF_STATS["trace"] == "hutchinson"
    (gx, gc) = torch.autograd.grad(loss, (xg, cg), create_graph=True)
    assert bool(gx.any()) and bool(gc.any()) and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gc).all()) and all(p.grad is None for p in flow.parameters())
    with pytest.raises(RuntimeError):
        gx.sum().backward()


def test_fallbacks_and_the_default(dev, monkeypatch):
    import zuko_amd._C as C
    from zuko_amd import ops
    from zuko_amd.flows import CNF

    assert ops.CNF_HUTCHINSON is False
    x, c = _probe((16, 3), 1).to(dev), _probe((16, 2), 2).to(dev)
    flow = _fixture_flow(dev, train=True)
    keep = C.PROFILE
    C.PROFILE = {}
    try:
        monkeypatch.setattr(ops, "CNF_ADJOINT", True)
        _loss(flow, x, c, None).backward()
        with torch.no_grad():
            flow.transform(c).call_and_ladj(x)
        calls = dict(C.PROFILE)
    finally:
        C.PROFILE = keep
    assert ops.CNF_STATS["path"] == "torch" and not calls.get("zk_cnf_step_v2") and not calls.get("zk_cnf_adjoint_step_v2") and not calls.get("zk_cnf_step")
    monkeypatch.setattr(ops, "CNF_HUTCHINSON", True)
    for kw, dtype in ((dict(hidden_features=(16, 48, 128)), torch.float32), ({}, torch.float64)):
        torch.manual_seed(5)
        flow = CNF(3, 2, exact=False, **kw).to(dev).to(dtype).train()
        loss = _loss(flow, x.to(dtype), c.to(dtype), None)
        assert ops.CNF_STATS["path"] == "torch" and loss.requires_grad, kw
    monkeypatch.setattr(ops, "CNF_KERNEL", False)
    with torch.no_grad():
        _fixture_flow(dev).transform(c).call_and_ladj(x)
    assert ops.CNF_STATS["path"] == "torch"
