r"""Generate the fixtures of the continuous normalizing flow from the LIVE reference (CPU; not a test).

    ZUKO_REFERENCE=/path/to/a/checkout/of/zuko  python tests/golden/make_golden_cnf.py

cnf_{a..e}.npz: the weights of `zuko.flows.CNF(features, context, hidden_features=hidden, freqs=freqs)` under a fixed seed (w0, b0, w1, ..., freqs),
x, c ~ N(0, 1) and what the reference makes of them.  Two integrations are followed: "fwd" = call_and_ladj(x) (t 0 -> 1, value and log-determinant
state) and "inv" = transform.inv(z32) (t 1 -> 0, value only), each with

  * `<m>_att32` / `<m>_att64` [A, 3]: (t, dt, accepted) of every attempted step of the float32 / float64 reference at default tolerances (recorded by
    wrapping zuko.utils.dopri45), t and dt exactly as the reference carried them;
  * `<m>_y32` / `<m>_l32` / `<m>_y64` / `<m>_l64`: the state after driving the reference's OWN dopri45 over the accepted steps of `<m>_att32` (the
    same (t, dt) in both precisions) — the "pinned sequence" results; l is the log-determinant component (trace_scale included), fwd only;
  * `<m>_pin` [3]: indices into `<m>_att32` of three attempts — the first (dt = t1 - t0), the first rejected one after it, and an accepted step in
    the middle of the interval — and for each of them k = 0..2: `<m>_pin{k}_x` / `_l` (the float32 state the attempt starts from, taken from the
    float32 pinned drive), `<m>_pin{k}_y32` / `_l32` / `_r32` and `..64`: the step's result and the per-row ratio
    max_j err_j / (atol + rtol max(|state_j|, |next_j|)) in float32 and, from the same inputs, in float64.

The adaptive results: lp32 / z32 / inv32 and lp64 / z64 / inv64 (log_prob, z = transform(x), transform.inv(z)) at default tolerances, lp_truth /
z_truth / inv_truth in float64 at atol = 1e-10, rtol = 1e-9 (inv_truth inverts z32, as inv32 does), and lp32_098 / z32_098 / lp32_102 / z32_102: the
float32 reference with both tolerances scaled by 0.98 and 1.02 — stand-ins for a step sequence that differs at a borderline decision.

flow_cnf_small.npz: CNF(3, 2) under seed 17: the state_dict's hash and parameter names, x, c, the adaptive results as above, and the float64
gradient of log_prob.mean() for every parameter, taken in train() mode (`grad/<name>`, stored rounded to float32: the tests' bar is 2e-4 of the
largest entry), and the float32 reference's gradient (`grad32/<name>`): adaptive float32 training gradients sit 5e-5 .. 3e-3 of the largest entry
away from the float64 ones, which is the measure for a float32 implementation.
"""

from __future__ import annotations

import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.environ["ZUKO_REFERENCE"])

import zuko  # noqa: E402  (the real reference)
import zuko.transforms  # noqa: E402
import zuko.utils  # noqa: E402
from zuko.flows import CNF  # noqa: E402

CASES = {  # name: (features, context, hidden, freqs, N, seed)
    "cnf_a": (3, 2, (64, 64), 3, 67, 41),
    "cnf_b": (5, 0, (64, 64), 3, 130, 42),
    "cnf_c": (16, 3, (16, 48, 128), 2, 33, 43),
    "cnf_d": (1, 0, (16,), 3, 257, 44),
    "cnf_e": (4, 2, (30, 30), 3, 33, 45),
}
TRUTH = dict(atol=1e-10, rtol=1e-9)


def sd_hash(sd: dict) -> str:
    h = hashlib.sha256()
    for k in sorted(sd):
        v = sd[k]
        if v is None:
            continue
        h.update(k.encode())
        h.update(str(tuple(v.shape)).encode())
        h.update(v.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


class Recorder:
    """Wraps zuko.utils.dopri45 (every attempted step of an adaptive integration goes through it with error=True) and zuko.transforms.odeint (to get
    hold of the system a transformation integrates)."""

    def __init__(self):
        self.attempts, self.systems = [], []
        self._dopri, self._odeint = zuko.utils.dopri45, zuko.transforms.odeint

    def __enter__(self):
        def dopri(f, x, t, dt, error=False):
            if error:
                self.attempts.append((t.item(), dt.item()))
            return self._dopri(f, x, t, dt, error=error)

        def odeint(f, x, t0, t1, phi=(), atol=1e-6, rtol=1e-5):
            self.systems.append((f, x, t0, t1))
            return self._odeint(f, x, t0, t1, phi, atol, rtol)

        zuko.utils.dopri45, zuko.transforms.odeint = dopri, odeint
        return self

    def __exit__(self, *exc):
        zuko.utils.dopri45, zuko.transforms.odeint = self._dopri, self._odeint

    def table(self) -> np.ndarray:
        """[A, 3] float64: t, dt, accepted (an attempt was accepted when the next one starts elsewhere; the last one always was)."""
        a = np.array(self.attempts, dtype=np.float64).reshape(-1, 2)
        acc = np.ones(len(a))
        acc[:-1] = a[1:, 0] != a[:-1, 0]
        return np.concatenate([a, acc[:, None]], axis=1)


def system_of(transform, x, with_ladj: bool):
    """The packed system the reference integrates for call_and_ladj(x) / _call(x): g(t, flat) on flat = cat(x.flatten(), ladj.flatten())."""
    with Recorder() as rec, torch.no_grad():
        transform.call_and_ladj(x) if with_ladj else transform(x)
    f, state, _, _ = rec.systems[0]
    if torch.is_tensor(state):
        return (lambda t, v: f(t, v.reshape(x.shape)).flatten()), [x.shape]
    shapes = [v.shape for v in state]
    return (lambda t, v: torch.cat([p.flatten() for p in f(t, *zuko.utils.unpack(v, shapes))])), shapes


def one_step(g, shapes, parts, t, dt, atol, rtol):
    """The reference's dopri45 on the packed state: (next parts, per-row ratio)."""
    dtype = parts[0].dtype
    flat = torch.cat([p.flatten() for p in parts])
    with torch.no_grad():
        y, err = zuko.utils.dopri45(g, flat, torch.as_tensor(t, dtype=dtype), torch.as_tensor(dt, dtype=dtype), error=True)
    ratio = err / (atol + rtol * torch.max(abs(flat), abs(y)))
    ys, rs = zuko.utils.unpack(y, shapes), zuko.utils.unpack(ratio, shapes)
    rows = rs[0].max(dim=-1).values
    if len(rs) > 1:
        rows = torch.max(rows, rs[1])
    return [v.clone() for v in ys], rows


def follow(out, mode, transforms, start, with_ladj, att32):
    """Drive the reference's one-step function over the accepted attempts of `att32` in both precisions, and pin three attempts."""
    atol, rtol = transforms[0].atol, transforms[0].rtol
    idx_rej = next((i for i in range(1, len(att32)) if att32[i, 2] == 0), 0)
    acc = [i for i in range(len(att32)) if att32[i, 2] == 1]
    idx_mid = acc[len(acc) // 2]
    pins = [0, idx_rej, idx_mid]
    out[f"{mode}_pin"] = np.array(pins)
    states32 = {}
    for tag, tr, dtype in (("32", transforms[0], torch.float32), ("64", transforms[1], torch.float64)):
        x0 = start.to(dtype)
        g, shapes = system_of(tr, x0, with_ladj)
        parts = [x0] + ([torch.zeros_like(x0[..., 0])] if with_ladj else [])
        for i, (t, dt, ok) in enumerate(att32):
            if tag == "32":
                states32[i] = [p.clone() for p in parts]
            if ok:
                parts, _ = one_step(g, shapes, parts, t, dt, atol, rtol)
        out[f"{mode}_y{tag}"] = parts[0].numpy()
        if with_ladj:
            out[f"{mode}_l{tag}"] = parts[1].numpy()
        for k, i in enumerate(pins):
            inp = [p.to(dtype) for p in states32[i]]  # (the float32 drive ran first: the same inputs in both precisions)
            nxt, rows = one_step(g, shapes, inp, att32[i, 0], att32[i, 1], atol, rtol)
            if tag == "32":
                out[f"{mode}_pin{k}_x"] = inp[0].numpy()
                if with_ladj:
                    out[f"{mode}_pin{k}_l"] = inp[1].numpy()
            out[f"{mode}_pin{k}_y{tag}"], out[f"{mode}_pin{k}_r{tag}"] = nxt[0].numpy(), rows.numpy()
            if with_ladj:
                out[f"{mode}_pin{k}_l{tag}"] = nxt[1].numpy()


def flows_of(seed, kw):
    torch.manual_seed(seed)
    f32 = CNF(**kw).eval()
    torch.manual_seed(seed)
    f64 = CNF(**kw).double().eval()
    for p in (*f32.parameters(), *f64.parameters()):
        p.requires_grad_(False)
    return f32, f64


def adaptive(out, f32, f64, x, c):
    def run(flow, cast, scale=1.0, zin=None, **tol):
        tr = flow.transform
        keep = tr.atol, tr.rtol
        tr.atol, tr.rtol = (tol.get("atol", keep[0]) * scale, tol.get("rtol", keep[1]) * scale)
        try:
            with torch.no_grad():
                d = flow(None if c is None else cast(c))
                z = d.transform(cast(x))
                lp = d.log_prob(cast(x))
                inv = d.transform.inv(z if zin is None else cast(zin))
        finally:
            tr.atol, tr.rtol = keep
        return lp, z, inv

    lp32, z32, inv32 = run(f32, lambda t: t)
    lp64, z64, inv64 = run(f64, lambda t: t.double())
    lpt, zt, invt = run(f64, lambda t: t.double(), zin=z32, **TRUTH)
    out.update(lp32=lp32.numpy(), z32=z32.numpy(), inv32=inv32.numpy(), lp64=lp64.numpy(), z64=z64.numpy(), inv64=inv64.numpy(),
               lp_truth=lpt.numpy(), z_truth=zt.numpy(), inv_truth=invt.numpy())
    for tag, scale in (("098", 0.98), ("102", 1.02)):
        lp, z, _ = run(f32, lambda t: t, scale=scale)
        out["lp32_" + tag], out["z32_" + tag] = lp.numpy(), z.numpy()
    return z32


def cnf_case(name: str) -> None:
    F, C, hidden, Q, N, seed = CASES[name]
    kw = dict(features=F, context=C, hidden_features=hidden, freqs=Q)
    f32, f64 = flows_of(seed, kw)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(N, F, generator=g)
    c = torch.randn(N, C, generator=g) if C else None
    out = {"x": x.numpy(), "freqs": f32.transform.freqs.numpy(), "hash": np.frombuffer(sd_hash(f32.state_dict()).encode(), dtype=np.uint8)}
    if c is not None:
        out["c"] = c.numpy()
    for i, l in enumerate(m for m in f32.transform.ode if hasattr(m, "weight")):
        out[f"w{i}"], out[f"b{i}"] = l.weight.numpy(), l.bias.numpy()
    z32 = adaptive(out, f32, f64, x, c)
    out["zin"] = z32.numpy()
    for mode, start, with_ladj in (("fwd", x, True), ("inv", z32, False)):
        trs = []
        for tag, flow, cast in (("32", f32, lambda t: t), ("64", f64, lambda t: t.double())):
            tr = flow.transform(None if c is None else cast(c))
            tr = tr if mode == "fwd" else tr.inv
            trs.append(tr)
            with Recorder() as rec, torch.no_grad():
                tr.call_and_ladj(cast(start)) if with_ladj else tr(cast(start))
            out[f"{mode}_att{tag}"] = rec.table()
        follow(out, mode, trs, start, with_ladj, out[f"{mode}_att32"])
    np.savez(os.path.join(HERE, name + ".npz"), **out)
    d = lambda a, b: float(np.abs(out[a].astype(np.float64) - out[b]).max())
    print(name, f"attempts fwd {len(out['fwd_att32'])} / {len(out['fwd_att64'])}, inv {len(out['inv_att32'])} / {len(out['inv_att64'])}; pins {out['fwd_pin'].tolist()};",
          f"|lp32 - truth| {d('lp32', 'lp_truth'):.2e}, 0.98: {d('lp32_098', 'lp_truth'):.2e}, 1.02: {d('lp32_102', 'lp_truth'):.2e}; |z32 - truth| {d('z32', 'z_truth'):.2e};",
          f"round trip {float(np.abs(out['inv32'] - out['x']).max()):.2e}; pinned |y32 - y64| {d('fwd_y32', 'fwd_y64'):.2e}, |l32 - l64| {d('fwd_l32', 'fwd_l64'):.2e};",
          "ratios " + " ".join(f"{out[f'fwd_pin{k}_r32'].max():.3g}" for k in range(3)))


def flow_case() -> None:
    seed, kw = 17, dict(features=3, context=2)
    f32, f64 = flows_of(seed, kw)
    g = torch.Generator().manual_seed(seed + 1)
    x, c = torch.randn(64, 3, generator=g), torch.randn(64, 2, generator=g)
    out = {"hash": np.frombuffer(sd_hash(f32.state_dict()).encode(), dtype=np.uint8), "x": x.numpy(), "c": c.numpy()}
    adaptive(out, f32, f64, x, c)
    torch.manual_seed(seed)
    train = CNF(**kw).double().train()
    train(c.double()).log_prob(x.double()).mean().backward()
    names = []
    for k, p in train.named_parameters():
        names.append(k)
        out["grad/" + k] = p.grad.numpy().astype(np.float32)
    out["param_names"] = np.array(names)
    torch.manual_seed(seed)
    train32 = CNF(**kw).train()
    train32(c).log_prob(x).mean().backward()
    for k, p in train32.named_parameters():
        out["grad32/" + k] = p.grad.numpy()
    np.savez(os.path.join(HERE, "flow_cnf_small.npz"), **out)
    print("flow_cnf_small", len(names), "parameters,", f"|lp32 - truth| {np.abs(out['lp32'] - out['lp_truth']).max():.2e}")


if __name__ == "__main__":
    print("zuko", zuko.__version__)
    torch.set_num_threads(8)
    for name in CASES:
        cnf_case(name)
    flow_case()
