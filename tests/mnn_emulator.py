"""numpy emulator of csrc/mnn.hip: walks ONE feature's weight image (zuko_amd/mnn_plan.py) in the kernel's tile order, lane by lane, with the
matrix instruction's operand maps — v_mfma_f32_16x16x4_f32: lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15] and holds
D[4 (l >> 4) + r][l & 15] in register r.  Arithmetic in float64: what it checks is the image (index table, K padding, tile and K order,
the ELU split inside a 16-row tile), not rounding.  In the style of tests/plan_emulators.py."""

from __future__ import annotations

import numpy as np

LANE = np.arange(64)
J, Q = LANE & 15, LANE >> 4


def mfma(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """a, b [64] (one register per lane), c [64, 4] -> c + A B in the lane layout."""
    A = a.reshape(4, 16).T  # [i][k]
    B = b.reshape(4, 16)  # [k][col]
    D = A @ B  # [16, 16]
    return c + D.reshape(4, 4, 16).transpose(0, 2, 1).reshape(64, 4)  # lane 16 q + j, register r <- D[4 q + r][j]


def act(p: np.ndarray, tile: int, half: int):
    """two-way ELU on a [64, 4] fragment of tile `tile`: lane (j, q), register r holds unit 16 tile + 4 q + r."""
    unit = 16 * tile + 4 * Q[:, None] + np.arange(4)[None, :]
    first = unit < half
    s = np.where(first, p, -p)
    a = np.where(s > 0, s, np.expm1(np.minimum(s, 0)))
    d = np.where(s > 0, 1.0, np.exp(np.minimum(s, 0)))
    return np.where(first, a, -a), d


def sum_q(p: np.ndarray) -> np.ndarray:
    p = p + p[LANE ^ 16]
    return p + p[LANE ^ 32]


def evaluate(image: np.ndarray, L, x: np.ndarray, signal: np.ndarray):
    """(y, dy/dx) [n] of one feature: image [L.total] float64, x [n], signal [n, S]."""
    n = x.shape[0]
    y, dy = np.zeros(n), np.zeros(n)
    f4 = lambda off: image[off + 4 * Q[:, None] + np.arange(4)[None, :]]  # the 16-byte read at off + 4 q
    for t0 in range(0, n, 16):
        row = np.minimum(t0 + J, n - 1)
        xs = x[row]
        c0 = [f4(L.o_b0 + 16 * o) for o in range(L.T[0])]
        for s in range(L.ks):
            k = 4 * s + Q
            sig = np.where(k < L.S, signal[row, np.minimum(k, L.S - 1)], 0.0)
            for o in range(L.T[0]):
                c0[o] = mfma(image[L.o_w0s + (o * L.ks + s) * 64 + LANE], sig, c0[o])
        v, t = [], []
        for o in range(L.T[0]):
            w = f4(L.o_w0x + 16 * o)
            a, d = act(w * xs[:, None] + c0[o], o, (L.widths[0] + 1) // 2)
            v.append(a)
            t.append(d * w)
        for l in range(1, len(L.widths)):
            nv, nt = [], []
            for o in range(L.T[l]):
                ov, ot = f4(L.o_b[l] + 16 * o), np.zeros((64, 4))
                for i in range(L.T[l - 1]):
                    a4 = image[L.o_w[l] + (o * L.T[l - 1] + i) * 256 + 4 * LANE[:, None] + np.arange(4)[None, :]]
                    for r in range(4):
                        ov = mfma(a4[:, r], v[i][:, r], ov)
                        ot = mfma(a4[:, r], t[i][:, r], ot)
                a, d = act(ov, o, (L.widths[l] + 1) // 2)
                nv.append(a)
                nt.append(d * ot)
            v, t = nv, nt
        py, pd = np.zeros(64), np.zeros(64)
        for o in range(L.T[-1]):
            w = f4(L.o_wl + 16 * o)
            py, pd = py + (w * v[o]).sum(1), pd + (w * t[o]).sum(1)
        yy, dd = sum_q(py) + image[L.o_bl], sum_q(pd)
        ok = (Q == 0) & (t0 + J < n)
        y[t0 + J[ok]], dy[t0 + J[ok]] = yy[ok], dd[ok]
    return y, dy
