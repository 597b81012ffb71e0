"""CPU: the plan of the spline coupling kernel (zuko_amd/coupling_plan.py: build_coupling_plan(total = 3 K - 1); csrc/fused_coupling.hip:
coupling_rqs_kernel), walked in numpy the way the kernel walks it."""

import numpy as np
import pytest
import torch

from zuko_amd import coupling_plan as cp

TILE = cp.TILE
CASES = [(5, 3, 8, [32, 32]), (12, 2, 16, [40, 70, 24]), (7, 0, 4, [48]), (64, 0, 8, [256])]


def _net(features, context, K, hidden, seed=0):
    """Weights / biases (float64) of MLP(kept + context, moved * (3 K - 1), hidden) under the default checkered mask."""
    rng = np.random.default_rng(seed)
    mask = np.arange(features) % 2 == 1
    idx_a, idx_b = np.nonzero(mask)[0], np.nonzero(~mask)[0]
    total = 3 * K - 1
    sizes = [len(idx_a) + context] + list(hidden) + [len(idx_b) * total]
    W = [rng.standard_normal((o, i)) / np.sqrt(i) for i, o in zip(sizes[:-1], sizes[1:])]
    b = [0.3 * rng.standard_normal(o) for o in sizes[1:]]
    return idx_a, idx_b, total, W, b


def _tile_mat(blk):  # [64 lanes, 4] -> A[i][k = 4 q + r]: lane (i, q) holds A[i][4 q .. 4 q + 3]
    return blk.reshape(4, 16, 4).transpose(1, 0, 2).reshape(16, 16)


def simulate_coupling_rqs(plan, W, b, x, ctx):
    """The kernel's walk: first-layer gather through amap, hidden layers in (4 out-tiles, in-tile) steps with chunk padding between layers, the
    last layer group by group / in-tile by in-tile / nt out-tiles, then lane (j, q) of group g reads parameter p of slot 4 g + q from row
    4 q + (p & 3) of out-tile p >> 2.  Returns phi [n, moved, total] (rows of fmap's order)."""
    n = x.shape[0]
    wcat, bcat = np.concatenate([w.reshape(-1) for w in W]), np.concatenate(b)
    stream = np.where(plan.gather >= 0, wcat[np.maximum(plan.gather, 0)], 0.0).reshape(-1, 64, 4)
    bias = np.where(plan.bias_gather >= 0, bcat[np.maximum(plan.bias_gather, 0)], 0.0)
    cur = np.zeros((n, plan.nit * TILE))
    for i, src in enumerate(plan.amap):
        if src >= 0:
            cur[:, i] = x[:, src]
        elif src <= -2:
            cur[:, i] = ctx[:, -2 - src]
    pos, L = 0, plan.n_layers
    for l in range(L - 1):
        n_in = plan.nit if l == 0 else plan.tiles[l - 1]
        out = np.zeros((n, cp.MAX_T * TILE))
        for otg in range(-(-plan.tiles[l] // 4)):
            sl = slice(otg * 4 * TILE, (otg * 4 + 4) * TILE)
            out[:, sl] = bias[plan.bias_off[l] + sl.start : plan.bias_off[l] + sl.stop]
            for it in range(n_in):
                for t in range(4):
                    out[:, (otg * 4 + t) * TILE : (otg * 4 + t + 1) * TILE] += cur[:, it * TILE : (it + 1) * TILE] @ _tile_mat(stream[pos]).T
                    pos += 1
        pos = -(-pos // cp.CHUNK) * cp.CHUNK
        cur = np.maximum(out, 0.0)
        cur[:, plan.widths[l] :] = 0.0
    phi = np.full((n, plan.moved, plan.total), np.nan)
    for g in range(plan.n_groups):
        b0 = plan.bias_off[L - 1] + g * plan.nt * TILE
        acc = np.zeros((n, plan.nt, TILE)) + bias[b0 : b0 + plan.nt * TILE].reshape(plan.nt, TILE)
        for it in range(plan.tiles[-1]):
            for t in range(plan.nt):
                acc[:, t, :] += cur[:, it * TILE : (it + 1) * TILE] @ _tile_mat(stream[pos]).T
                pos += 1
        for q in range(4):
            slot = 4 * g + q
            if plan.fmap[slot] >= 0:
                for p in range(plan.total):
                    phi[:, slot, p] = acc[:, p >> 2, 4 * q + (p & 3)]
    assert -(-pos // cp.CHUNK) == plan.n_chunks and plan.n_blocks == plan.n_chunks * cp.CHUNK
    return phi


@pytest.mark.parametrize("features,context,K,hidden", CASES)
def test_spline_plan_reproduces_the_conditioner(features, context, K, hidden):
    idx_a, idx_b, total, W, b = _net(features, context, K, hidden)
    plan = cp.build_coupling_plan([w.shape for w in W], idx_a, idx_b, features, context, total=total)
    assert plan is not None and plan.total == total and plan.nt == -(-total // 4) and plan.n_groups == -(-len(idx_b) // 4)
    assert plan.split_gather is None and plan.split_chunks == 0
    rng = np.random.default_rng(1)
    x, ctx = 2.5 * rng.standard_normal((37, features)), rng.standard_normal((37, context))
    h = np.concatenate([x[:, idx_a], ctx], axis=1)
    for l, (w, bb) in enumerate(zip(W, b)):
        h = h @ w.T + bb
        if l < len(W) - 1:
            h = np.maximum(h, 0.0)
    ref = h.reshape(37, len(idx_b), total)  # MLP(cat(x_a, c)).unflatten(-1, (moved, 3 K - 1)), float64
    phi = simulate_coupling_rqs(plan, W, b, x, ctx)
    assert np.isfinite(phi).all()
    np.testing.assert_allclose(phi, ref, rtol=1e-12, atol=1e-12)
    # every weight and bias of the last layer appears exactly once in the stream / bias image
    w_off = sum(w.size for w in W[:-1])
    last = plan.gather[plan.gather >= w_off]
    assert np.array_equal(np.sort(last), np.arange(w_off, w_off + W[-1].size))
    b_off = sum(len(v) for v in b[:-1])
    lastb = plan.bias_gather[plan.bias_off[-1] :]
    assert len(lastb) == plan.n_groups * plan.nt * TILE
    assert np.array_equal(np.sort(lastb[lastb >= 0]), np.arange(b_off, b_off + len(b[-1])))
    # padding: parameters 3 K - 1 .. 4 nt - 1 of a slot and the slots beyond `moved` read as -1 (0 in the image)
    img = lastb.reshape(plan.n_groups, plan.nt, 4, 4)  # [g, t, q, r]
    for g in range(plan.n_groups):
        for t in range(plan.nt):
            for q in range(4):
                for r in range(4):
                    slot, p = 4 * g + q, 4 * t + r
                    want = b_off + slot * total + p if (slot < len(idx_b) and p < total) else -1
                    assert img[g, t, q, r] == want
    assert len(plan.fmap) == 4 * plan.n_groups
    assert np.array_equal(plan.fmap[: len(idx_b)], idx_b) and (plan.fmap[len(idx_b) :] == -1).all()


def test_default_total_leaves_the_affine_plan_as_it_is():
    idx_a, idx_b = np.arange(1, 12, 2), np.arange(0, 12, 2)
    shapes = [(40, 8), (24, 40), (12, 24)]
    p0 = cp.build_coupling_plan(shapes, idx_a, idx_b, 12, 2)
    p2 = cp.build_coupling_plan(shapes, idx_a, idx_b, 12, 2, total=2)
    assert p0 is not None and p0.total == 2 and p0.nt == 1 and p0.n_groups == 1 and len(p0.fmap) == 8
    for name in ("gather", "bias_gather", "amap", "fmap"):
        assert np.array_equal(getattr(p0, name), getattr(p2, name)), name
    assert (p0.n_blocks, p0.n_chunks, p0.bias_off, p0.tiles, p0.widths) == (p2.n_blocks, p2.n_chunks, p2.bias_off, p2.tiles, p2.widths)
    # a last layer that does not hold `total` rows per moved feature, or a bin count without a kernel, is no plan
    assert cp.build_coupling_plan(shapes, idx_a, idx_b, 12, 2, total=23) is None
    assert cp.build_coupling_plan([(40, 8), (6 * 8, 40)], idx_a, idx_b, 12, 2, total=8) is None


def test_spline_plan_that_exceeds_the_lds_is_refused():
    """K = 16 on 256 features with three hidden layers: the 72 KiB ring and four row images of 16 x 260 floats (65 KiB) leave 23 KiB; the last bias
    image alone is 32 groups x 12 tiles x 16 floats = 24 KiB."""
    features, K = 256, 16
    mask = np.arange(features) % 2 == 1
    idx_a, idx_b = np.nonzero(mask)[0], np.nonzero(~mask)[0]
    shapes = [(64, 128), (64, 64), (64, 64), (128 * (3 * K - 1), 64)]
    assert cp.lds_bytes(3 * 512 + 32 * 12 * 16, 32, features, 0) > cp.LDS_LIMIT
    assert cp.build_coupling_plan(shapes, idx_a, idx_b, features, 0, total=3 * K - 1) is None
    # the same network with 4 bins fits
    shapes[-1] = (128 * 11, 64)
    small = cp.build_coupling_plan(shapes, idx_a, idx_b, features, 0, total=11)
    assert small is not None and cp.lds_bytes(len(small.bias_gather), small.n_groups, features, 0) <= cp.LDS_LIMIT
