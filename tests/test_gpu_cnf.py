"""GPU: the continuous normalizing flow.  zk_cnf_step through the C ABI against tests/cnf_ref.py at the fixtures' pinned attempts and over their
accepted sequences, the kernel's row independence and error word, the adaptive integration at flow level against the float64 truth at the
reference's own distance, every fallback to the torch-op path at the same bars, training gradients, sampling and the refusal to capture."""

import numpy as np
import pytest
import torch

import cnf_ref
import parity
from conftest import T, golden
from parity import C_NOISE, assert_f64, assert_parity

pytestmark = pytest.mark.gpu

CASES = {"cnf_a": (3, 2, (64, 64), 3, 41), "cnf_b": (5, 0, (64, 64), 3, 42), "cnf_c": (16, 3, (16, 48, 128), 2, 43), "cnf_d": (1, 0, (16,), 3, 44),
         "cnf_e": (4, 2, (30, 30), 3, 45)}
KERNEL_CASES = ["cnf_a", "cnf_b", "cnf_c", "cnf_d"]
FLOW_KW, FLOW_SEED = dict(features=3, context=2), 17
ATOL, RTOL = 1e-6, 1e-5
_FLOWS: dict = {}
_REFS: dict = {}


def _flow(name, dev, **kw):
    """The zuko_amd flow of a fixture on the device (the same seed gives the reference's weights: tests/test_cnf_host.py), cached."""
    from zuko_amd.flows import CNF

    key = (name, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _FLOWS:
        if name == "flow_cnf_small":
            torch.manual_seed(FLOW_SEED)
            flow = CNF(**FLOW_KW, **kw)
        else:
            F, C, hidden, Q, seed = CASES[name]
            torch.manual_seed(seed)
            flow = CNF(F, C, hidden_features=hidden, freqs=Q, **kw)
        _FLOWS[key] = flow.eval().to(dev)
    return _FLOWS[key]


class _Stepper:
    """zk_cnf_step on a flow's weight image, one call = one launch."""

    def __init__(self, name, dev):
        from zuko_amd import cnf_plan

        self.module = _flow(name, dev).transform
        self.img = cnf_plan.image_of(self.module, dev)
        assert self.img is not None
        self.img.refresh(self.module)
        self.dev = dev

    def pre(self, c):
        lin, Q2 = self.module.ode[0], 2 * self.img.Q
        with torch.no_grad():
            return lin.bias.detach().clone() if c is None else torch.addmm(lin.bias, c, lin.weight[:, Q2 + self.img.F :].t()).contiguous()

    def __call__(self, x, l, pre, t, dt, y=None, with_rows=True):
        from zuko_amd import ops

        N = x.shape[0]
        y = torch.full((N, x.shape[1]), float("nan"), device=self.dev) if y is None else y
        ln = None if l is None else torch.full((N,), float("nan"), device=self.dev)
        err = torch.zeros(1, device=self.dev)
        rows = torch.full((N,), float("nan"), device=self.dev) if with_rows else None
        ops.cnf_step(self.img, x, l, pre, float(t), float(dt), ATOL, RTOL, cnf_ref.TRACE_SCALE, y, ln, err, rows)
        torch.cuda.synchronize()
        return y, ln, rows, err


def _ref_steps(name):
    """cnf_ref on the CPU at the fixture's pinned attempts, both precisions, computed once: {(mode, k, tag): (y, l, ratio)}."""
    if name not in _REFS:
        g = golden(name + ".npz")
        out = {}
        for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
            W, B, fr = cnf_ref.params_of(g, dtype)
            c = T(g["c"]).to(dtype) if "c" in g else None
            for mode, with_l in (("fwd", True), ("inv", False)):
                att = g[f"{mode}_att32"]
                for k, i in enumerate(g[f"{mode}_pin"]):
                    l = T(g[f"{mode}_pin{k}_l"]).to(dtype) if with_l else None
                    out[mode, k, tag] = cnf_ref.step(W, B, fr, att[i, 0], att[i, 1], T(g[f"{mode}_pin{k}_x"]).to(dtype), l, c)
        _REFS[name] = out
    return _REFS[name]


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_step_kernel_at_the_pinned_attempts(dev, name):
    g = golden(name + ".npz")
    st = _Stepper(name, dev)
    pre = st.pre(T(g["c"], dev) if "c" in g else None)
    ref = _ref_steps(name)
    for mode, with_l in (("fwd", True), ("inv", False)):
        att = g[f"{mode}_att32"]
        for k, i in enumerate(g[f"{mode}_pin"]):
            x = T(g[f"{mode}_pin{k}_x"], dev)
            l = T(g[f"{mode}_pin{k}_l"], dev) if with_l else None
            y, ln, rows, err = st(x, l, pre, att[i, 0], att[i, 1])
            (y32, l32, r32), (y64, l64, r64) = ref[mode, k, "32"], ref[mode, k, "64"]
            what = f"cnf step {name} {mode} attempt {i}"
            assert_parity(y, y32, y64, what + ": y")
            assert_parity(rows, r32, r64, what + ": ratio")
            if with_l:
                assert_parity(ln, l32, l64, what + ": l")
            assert torch.equal(err.view(torch.int32), rows.max().reshape(1).view(torch.int32)), f"{what}: err {err.item()!r} != max of the rows {rows.max().item()!r}"
            assert (float(err) < 1.0) == bool(att[i, 2]), f"{what}: the kernel's decision differs from the reference's"


@pytest.mark.parametrize("name", KERNEL_CASES)
def test_step_kernel_over_the_pinned_accepted_sequence(dev, name):
    """The reference's accepted steps, forward with tangents and backward with n_tangents = 0, end to end on the kernel."""
    g = golden(name + ".npz")
    st = _Stepper(name, dev)
    pre = st.pre(T(g["c"], dev) if "c" in g else None)
    for mode, start, with_l in (("fwd", "x", True), ("inv", "zin", False)):
        x = T(g[start], dev)
        l = torch.zeros(x.shape[0], device=dev) if with_l else None
        for t, dt, ok in g[f"{mode}_att32"]:
            if ok:
                x, l, _, err = st(x, l, pre, t, dt, with_rows=False)
                assert float(err) < 1.0
        assert_parity(x, g[f"{mode}_y32"], g[f"{mode}_y64"], f"cnf sequence {name} {mode}: y")
        if with_l:
            assert_parity(l, g["fwd_l32"], g["fwd_l64"], f"cnf sequence {name}: l")


def test_step_kernel_rows_are_independent_and_the_error_word_propagates_nan(dev):
    """A row's outputs: the same bits in a subset of the batch, with NaN-padded row strides, alone (N = 1) and in a second run; a NaN planted in one
    row of the last partial block turns `err` into NaN and changes no other row."""
    name = "cnf_a"
    g = golden(name + ".npz")
    st = _Stepper(name, dev)
    c = T(g["c"], dev)
    pre = st.pre(c)
    x = T(g["x"], dev)  # 67 rows: one full block and a partial one
    l = torch.linspace(-0.01, 0.01, x.shape[0], device=dev)
    N, F = x.shape
    for with_l in (True, False):
        li = l if with_l else None
        y, ln, rows, err = st(x, li, pre, 0.25, 0.125)
        again = st(x, li, pre, 0.25, 0.125)
        assert torch.equal(y, again[0]) and torch.equal(rows, again[2]) and torch.equal(err, again[3]) and (not with_l or torch.equal(ln, again[1]))
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(rows).all()) and float(err) == float(rows.max())
        sel = torch.tensor([66, 3, 64, 17, 0], device=dev)
        ys, ls, rs, es = st(x[sel].contiguous(), None if li is None else li[sel].contiguous(), pre[sel].contiguous(), 0.25, 0.125)
        assert torch.equal(ys, y[sel]) and torch.equal(rs, rows[sel]) and float(es) == float(rows[sel].max()) and (not with_l or torch.equal(ls, ln[sel]))
        y1, l1, r1, e1 = st(x[5:6].contiguous(), None if li is None else li[5:6].contiguous(), pre[5:6].contiguous(), 0.25, 0.125)
        assert torch.equal(y1, y[5:6]) and torch.equal(r1, rows[5:6]) and float(e1) == float(rows[5])
        # row strides with NaN in the padding: x [N, F + 3], y [N, F + 2], pre [N, H + 4]
        xp = torch.full((N, F + 3), float("nan"), device=dev)
        xp[:, :F] = x
        pp = torch.full((N, pre.shape[1] + 4), float("nan"), device=dev)
        pp[:, : pre.shape[1]] = pre
        yp = torch.full((N, F + 2), float("nan"), device=dev)
        y2, l2, r2, e2 = st(xp[:, :F], li, pp[:, : pre.shape[1]], 0.25, 0.125, y=yp[:, :F])
        assert torch.equal(y2, y) and torch.equal(r2, rows) and torch.equal(e2, err) and bool(torch.isnan(yp[:, F:]).all()) and (not with_l or torch.equal(l2, ln))
        # a NaN in row 65 (the partial block)
        xn = x.clone()
        xn[65, 1] = float("nan")
        y3, l3, r3, e3 = st(xn, li, pre, 0.25, 0.125)
        keep = torch.arange(N, device=dev) != 65
        assert bool(torch.isnan(e3).all()) and bool(torch.isnan(r3[65])) and torch.equal(y3[keep], y[keep]) and torch.equal(r3[keep], rows[keep])
        assert not with_l or torch.equal(l3[keep], ln[keep])
    # the unconditional case reads ONE shared row of pre
    gb = golden("cnf_b.npz")
    sb = _Stepper("cnf_b", dev)
    xb = T(gb["x"], dev)
    lb = torch.zeros(xb.shape[0], device=dev)
    shared = sb.pre(None)
    assert shared.dim() == 1
    a, b = sb(xb, lb, shared, 0.0, 0.5), sb(xb, lb, shared.expand(xb.shape[0], -1).contiguous(), 0.0, 0.5)
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def _distances(got_lp, got_z, g, what):
    """The distance of log_prob and z to the float64 truth, against the largest of the float32 reference's three distances (default tolerances, both
    scaled by 0.98 and by 1.02: a step sequence that differs at a borderline decision moves the result that much)."""
    for key, got in (("lp", got_lp), ("z", got_z)):
        truth = T(g[key + "_truth"])
        ref = max(float((T(g[key + tag]).double() - truth).abs().max()) for tag in ("32", "32_098", "32_102"))
        d = float((got.detach().cpu().double() - truth).abs().max())
        parity.REPORT.append({"what": f"{what}: {key} vs float64 truth", "distance": d, "reference_distance": ref, "c": C_NOISE, "ok": d <= C_NOISE * ref})
        print(f"{what}: |{key} - truth| {d:.3e}, the reference's {ref:.3e}")
        assert d <= C_NOISE * ref, f"{what}: |{key} - truth| = {d:.3e} > {C_NOISE:g} x {ref:.3e}"


def _flow_level(flow, g, dev, what, path):
    from zuko_amd import ops

    x = T(g["x"], dev)
    c = T(g["c"], dev) if "c" in g else None
    with torch.no_grad():
        d = flow(c)
        lp = d.log_prob(x)
        stats = dict(ops.CNF_STATS)
        assert stats["path"] == path, f"{what}: log_prob took the {stats['path']} path"
        if path == "kernel":
            assert stats["t_end"] == 1.0 and stats["accepted"] >= 1
            parity.REPORT.append({"what": f"{what}: attempts of log_prob", "attempts": stats["attempts"], "accepted": stats["accepted"], "reference_attempts": int(len(g["fwd_att32"])) if "fwd_att32" in g else None, "ok": True})
        z = d.transform(x)
        assert ops.CNF_STATS["path"] == path
        back = d.transform.inv(z)
        if path == "kernel":
            assert ops.CNF_STATS["t_end"] == 0.0
    _distances(lp, z, g, what)
    rt, rt_ref = float((back - x).abs().max()), float(np.abs(g["inv32"] - g["x"]).max())
    print(f"{what}: round trip {rt:.3e}, the reference's {rt_ref:.3e}")
    assert rt <= C_NOISE * rt_ref, f"{what}: round trip {rt:.3e} > {C_NOISE:g} x {rt_ref:.3e}"


@pytest.mark.parametrize("name", KERNEL_CASES + ["flow_cnf_small"])
def test_adaptive_integration_on_the_kernel(dev, name):
    _flow_level(_flow(name, dev), golden(name + ".npz"), dev, f"cnf adaptive {name}", "kernel")


def test_fallback_outside_the_envelope(dev):
    from zuko_amd import ops

    assert not ops.cnf_supported(4, 2, (30, 30), 3)
    _flow_level(_flow("cnf_e", dev), golden("cnf_e.npz"), dev, "cnf fallback (30, 30)", "torch")


def test_fallback_with_the_switch_off(dev, monkeypatch):
    from zuko_amd import ops

    monkeypatch.setattr(ops, "CNF_KERNEL", False)
    _flow_level(_flow("cnf_a", dev), golden("cnf_a.npz"), dev, "cnf fallback CNF_KERNEL = False", "torch")


def _restated(W, B, fr, x, c, act="elu", eps=None):
    """What _distances needs, from cnf_ref on the CPU: float32 at default tolerances and scaled by 0.98 / 1.02, float64 at the truth's."""
    def run(dtype, scale=1.0, atol=ATOL, rtol=RTOL):
        cast = lambda v: None if v is None else v.to(dtype)
        z, l, _ = cnf_ref.integrate([cast(w) for w in W], [cast(b) for b in B], cast(fr), cast(x), cast(c), atol=atol * scale, rtol=rtol * scale, act=act, eps=cast(eps))
        return (-0.5 * (z**2).sum(-1) - 0.5 * z.shape[-1] * np.log(2 * np.pi) + l / cnf_ref.TRACE_SCALE).numpy(), z.numpy()

    g = {}
    g["lp32"], g["z32"] = run(torch.float32)
    g["lp32_098"], g["z32_098"] = run(torch.float32, 0.98)
    g["lp32_102"], g["z32_102"] = run(torch.float32, 1.02)
    g["lp_truth"], g["z_truth"] = run(torch.float64, atol=1e-10, rtol=1e-9)
    return g


def test_fallback_for_another_activation(dev):
    import torch.nn as nn

    from zuko_amd import ops

    flow = _flow("cnf_a", dev, activation=nn.Tanh)
    g = golden("cnf_a.npz")
    lins = [m for m in flow.transform.ode if hasattr(m, "weight")]
    W, B = [l.weight.detach().cpu() for l in lins], [l.bias.detach().cpu() for l in lins]
    x, c = T(g["x"]), T(g["c"])
    ref = _restated(W, B, flow.transform.freqs.cpu(), x, c, act="tanh")
    with torch.no_grad():
        d = flow(c.to(dev))
        lp = d.log_prob(x.to(dev))
        assert ops.CNF_STATS["path"] == "torch"
        z = d.transform(x.to(dev))
    _distances(lp, z, ref, "cnf fallback Tanh")


def test_fallback_for_hutchinsons_estimator(dev):
    from zuko_amd import ops

    flow = _flow("cnf_a", dev, exact=False)
    g = golden("cnf_a.npz")
    W, B, fr = cnf_ref.params_of(g, torch.float32)
    x, c = T(g["x"]), T(g["c"])
    eps = torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
    ref = _restated(W, B, fr, x, c, eps=eps)
    with torch.no_grad():
        z, ladj = flow.transform(c.to(dev)).call_and_ladj(x.to(dev), eps=eps.to(dev))
        assert ops.CNF_STATS["path"] == "torch"
    lp = -0.5 * (z**2).sum(-1) - 0.5 * z.shape[-1] * np.log(2 * np.pi) + ladj
    _distances(lp, z, ref, "cnf fallback exact=False")
    assert float((T(ref["lp_truth"]) - T(g["lp_truth"])).abs().max()) > 1e-3  # (the estimate is not the exact trace: the probe was used)


def test_fallback_in_float64_over_the_pinned_sequence(dev):
    """float64 goes to the torch-op path; its one-step function driven over the reference's accepted steps is the reference's to 1e-12, and the
    adaptive call is the float64 reference's."""
    from zuko_amd import ops
    from zuko_amd.utils import _Bundle, dopri45

    g = golden("cnf_a.npz")
    torch.manual_seed(CASES["cnf_a"][4])
    from zuko_amd.flows import CNF

    flow = CNF(3, 2, hidden_features=(64, 64)).double().eval().to(dev)
    x, c = T(g["x"], dev).double(), T(g["c"], dev).double()
    with torch.no_grad():
        tr = flow.transform(c)
        system = tr.augmented(x)
        state = _Bundle((x, torch.zeros_like(x[:, 0])))
        for t, dt, ok in g["fwd_att32"]:
            if ok:
                state = dopri45(lambda t, s: _Bundle(system(t, *s)), state, torch.tensor(t, dtype=torch.float64, device=dev), torch.tensor(dt, dtype=torch.float64, device=dev))
        assert_f64(state[0], g["fwd_y64"], "cnf float64 pinned sequence: y")
        assert_f64(state[1], g["fwd_l64"], "cnf float64 pinned sequence: l")
        lp = flow(c).log_prob(x)
        assert ops.CNF_STATS["path"] == "torch" and lp.dtype == torch.float64
        assert_f64(lp, g["lp64"], "cnf float64 adaptive: log_prob", tol=1e-9)


def test_training_gradients_on_the_torch_op_path(dev):
    """train() mode: log_prob runs in torch ops (grad of grad through the exact trace, the checkpoint adjoint backwards).  In float64 the gradients
    are the reference's float64 ones at the bar of the NAF training test, 2e-4 of the largest entry.  In float32 an adaptive integration's
    gradient is as far from the float64 one as its step sequence and rounding make it — the float32 reference's own distance is in the fixture
    (up to 2.8e-3 of the largest entry) — so the float32 bar is the suite's noise bar: C_NOISE times the reference's largest relative distance."""
    from zuko_amd import ops
    from zuko_amd.flows import CNF

    g = golden("flow_cnf_small.npz")
    names = list(g["param_names"])
    rel = lambda got, k: float((got.cpu().double() - T(g["grad/" + k]).double()).abs().max()) / float(np.abs(g["grad/" + k]).max())
    worst = {}
    for dtype in (torch.float64, torch.float32):
        torch.manual_seed(FLOW_SEED)
        flow = CNF(**FLOW_KW).to(dev).to(dtype).train()
        lp = flow(T(g["c"], dev).to(dtype)).log_prob(T(g["x"], dev).to(dtype))
        assert ops.CNF_STATS["path"] == "torch" and lp.requires_grad and lp.dtype == dtype
        lp.mean().backward()
        got = dict(flow.named_parameters())
        assert list(got) == names
        worst[dtype] = {k: rel(got[k].grad, k) for k in names}
        for k in names:
            parity.REPORT.append({"what": f"cnf training gradient {k} {dtype}", "relative_to_largest_entry": worst[dtype][k], "ok": True})
    for k in names:
        assert worst[torch.float64][k] <= 2e-4, f"float64 {k}: {worst[torch.float64][k]:.3e} of the largest entry"
    ref32 = max(rel(T(g["grad32/" + k]), k) for k in names)
    got32 = max(worst[torch.float32].values())
    print(f"float32 training gradients: {got32:.3e} of the largest entry from the float64 ones, the float32 reference {ref32:.3e}")
    assert got32 <= C_NOISE * ref32, f"float32: {got32:.3e} > {C_NOISE:g} x {ref32:.3e}"


def test_sampling_paths(dev):
    from zuko_amd import ops

    flow = _flow("flow_cnf_small", dev)
    c = T(golden("flow_cnf_small.npz")["c"], dev)[:8]
    torch.manual_seed(3)
    with torch.no_grad():
        s = flow(c).sample((4,))
    assert ops.CNF_STATS["path"] == "kernel" and ops.CNF_STATS["t_end"] == 0.0 and s.shape == (4, 8, 3) and bool(torch.isfinite(s).all())
    with torch.no_grad():
        back = flow(c).transform(s)
    assert ops.CNF_STATS["path"] == "kernel" and float(back.abs().max()) < 6.0  # (standard-normal draws came back)
    flow.train()
    try:
        r = flow(c).rsample((2,))
        assert ops.CNF_STATS["path"] == "torch" and r.shape == (2, 8, 3) and r.grad_fn is not None
    finally:
        flow.eval()


def test_graph_capture_is_refused(dev):
    import zuko_amd

    g = golden("flow_cnf_small.npz")
    flow = _flow("flow_cnf_small", dev)
    with pytest.raises(NotImplementedError, match="cannot be captured"):
        zuko_amd.capture(flow, T(g["x"], dev), T(g["c"], dev))
    with pytest.raises(NotImplementedError, match="cannot be captured"):
        zuko_amd.capture_step(flow, torch.optim.Adam(flow.parameters(), capturable=True), T(g["x"], dev), T(g["c"], dev))
