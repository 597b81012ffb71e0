"""numpy emulator of csrc/umnn.hip: walks ONE feature's weight image (zuko_amd/mnn_plan.py, of the signed weights) in the kernel's tile order,
lane by lane, with the matrix instruction's operand maps of tests/mnn_emulator.py, and runs the quadrature as the kernel does: the points
t_0 x, t_1 x, ..., x go through the network two at a time, the weighted sum is taken in the order of the nodes.  Arithmetic in float64: what
it checks is the image (index table, signs, K padding, tile and K order), the pairing and the place of the constant, not rounding."""

from __future__ import annotations

import numpy as np

from mnn_emulator import J, LANE, Q, mfma, sum_q


def elu(p: np.ndarray) -> np.ndarray:
    return np.where(p > 0, p, np.expm1(np.minimum(p, 0)))


def squash(h: np.ndarray) -> np.ndarray:
    return h / (1 + np.abs(h / 7))


def tail(image: np.ndarray, L, c0: list, us: list) -> list:
    """h at the points `us` ([64] each: one point per lane's element) behind the signal's share c0 of the first layer."""
    f4 = lambda off: image[off + 4 * Q[:, None] + np.arange(4)[None, :]]  # the 16-byte read at off + 4 q
    v = [[elu(f4(L.o_w0x + 16 * o) * u[:, None] + c0[o]) for o in range(L.T[0])] for u in us]
    for l in range(1, len(L.widths)):
        nv = [[] for _ in us]
        for o in range(L.T[l]):
            ov = [f4(L.o_b[l] + 16 * o) for _ in us]
            for i in range(L.T[l - 1]):
                a4 = image[L.o_w[l] + (o * L.T[l - 1] + i) * 256 + 4 * LANE[:, None] + np.arange(4)[None, :]]  # one read feeds every point
                for r in range(4):
                    for p in range(len(us)):
                        ov[p] = mfma(a4[:, r], v[p][i][:, r], ov[p])
            for p in range(len(us)):
                nv[p].append(elu(ov[p]))
        v = nv
    out = []
    for p in range(len(us)):
        py = np.zeros(64)
        for o in range(L.T[-1]):
            py = py + (f4(L.o_wl + 16 * o) * v[p][o]).sum(1)
        out.append(sum_q(py) + image[L.o_bl])
    return out


def integral(image, L, c0, xs, nodes, weights, ladj: bool):
    """(x sum_i w_i g(t_i x), h(x) | None) with the kernel's pairing of the n (+ 1 with ladj) points."""
    n = len(nodes)
    m = n + (1 if ladj else 0)
    point = lambda k: nodes[k] * xs if k < n else xs
    acc, hx, k = np.zeros(64), None, 0
    while k < m:
        ks = [k, k + 1] if k + 1 < m else [k]
        for kk, h in zip(ks, tail(image, L, c0, [point(kk) for kk in ks])):
            if kk < n:
                acc = acc + weights[kk] * np.exp(squash(h))
            else:
                hx = h
        k += 2
    return xs * acc, hx


def signal_share(image, L, row, signal):
    f4 = lambda off: image[off + 4 * Q[:, None] + np.arange(4)[None, :]]
    c0 = [f4(L.o_b0 + 16 * o) for o in range(L.T[0])]
    for s in range(L.ks):
        k = 4 * s + Q
        sig = np.where(k < L.S, signal[row, np.minimum(k, L.S - 1)], 0.0)
        for o in range(L.T[0]):
            c0[o] = mfma(image[L.o_w0s + (o * L.ks + s) * 64 + LANE], sig, c0[o])
    return c0


def evaluate(image: np.ndarray, L, x: np.ndarray, signal: np.ndarray, constant: np.ndarray, nodes: np.ndarray, weights: np.ndarray):
    """(y, ladj) [n] of one feature: image [L.total] float64, x [n], signal [n, S], constant [n], the rule on [0, 1]."""
    n = x.shape[0]
    y, ladj = np.zeros(n), np.zeros(n)
    for t0 in range(0, n, 16):
        row = np.minimum(t0 + J, n - 1)
        fx, hx = integral(image, L, signal_share(image, L, row, signal), x[row], nodes, weights, True)
        ok = (Q == 0) & (t0 + J < n)
        y[t0 + J[ok]], ladj[t0 + J[ok]] = (fx + constant[row])[ok], squash(hx)[ok]
    return y, ladj


def invert(image, L, y, signal, constant, nodes, weights, bound: float = 10.0, steps: int = 25):
    """The kernel's bisection for one feature: [n]."""
    n = y.shape[0]
    out = np.zeros(n)
    for t0 in range(0, n, 16):
        row = np.minimum(t0 + J, n - 1)
        c0 = signal_share(image, L, row, signal)
        target = y[row] - constant[row]
        lo, hi = np.full(64, -bound), np.full(64, bound)
        for _ in range(steps):
            c = (lo + hi) / 2
            below = integral(image, L, c0, c, nodes, weights, False)[0] < target
            lo, hi = np.where(below, c, lo), np.where(below, hi, c)
        ok = (Q == 0) & (t0 + J < n)
        out[t0 + J[ok]] = ((lo + hi) / 2)[ok]
    return out
