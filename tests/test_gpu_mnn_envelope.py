"""GPU: the monotone-network kernels (zk_mnn_* of csrc/mnn.hip, zk_umnn_* of csrc/umnn.hip) over the envelope ops.mnn_supported admits, through the
C ABI against the CPU references tests/mnn_ref.py / tests/umnn_ref.py in float32 and float64 (tests/test_mnn_host.py and tests/test_umnn_host.py pin
both to the reference project's fixtures):

  1. network shapes (tests/mnn_nets.py: ENVELOPE): LDS grants above 64 KiB, the 8-tile instantiation with full, odd and single tiles, every
     k-step count of the signal product's ends;
  2. every launch geometry the launchers can pick (GEOMETRY_SHAPES; tests/test_mnn_geometry_host.py shows the list is complete), each compared with
     the reference on a row sample and bit for bit with launches of slices that take the smallest geometry;
  3. quadrature sizes 1, 2, 7, 33, 64 (UMNN);
  4. non-finite x, signal and targets.

Weights: uniform(-1, 1) / sqrt(fan_in); x uniform in +-9.5, signal 1.5 randn, constant randn (tests/mnn_nets.py).  Bar: parity.assert_parity with its
default constant; the round trip of the inverse within C_NOISE of the float32 reference's own, as tests/test_gpu_mnn.py.

Row samples smaller than the 2048 rows of the forward comparisons, chosen by the cost of the CPU reference (the unconstrained network's inverse costs
25 x n_quad evaluations per element): every one is named where it is taken; the bit identity with the slices covers ALL rows and columns."""

import pytest
import torch

from mnn_nets import ENVELOPE, GEOMETRY_SHAPES, LARGE_LDS, SMALL_TM8, Case, draw_inputs, draw_params, geometry, sample_rows, shape_id
from parity import C_NOISE, _stats, assert_parity

pytestmark = pytest.mark.gpu

FAMILIES = ["mnn", "umnn"]
F32, F64 = torch.float32, torch.float64
UMNN_INVERSE_SHAPES = LARGE_LDS + [(1, (16,))]
DEFAULT = (16, (64, 64))


@pytest.fixture(scope="module")
def case_of(dev):
    """(family, (S, widths), F[, n_quad]) -> Case with seeded weights, made once per module."""
    made = {}

    def get(family, shape, F, n_quad=32):
        key = (family, shape, F, n_quad)
        if key not in made:
            S, widths = shape
            W, B = draw_params(S, widths, F, seed=1000 * S + sum(widths) + F)
            made[key] = Case(family, W, B, dev, n_quad)
        return made[key]

    return get


def _dev(dev, *ts):
    return tuple(t.to(dev) for t in ts)


def _padded(case, x, sig, cst):
    """The same call through NaN-padded row strides of x, of the signal and of the constant."""
    dev = x.device
    N, D, S = sig.shape
    xp, sp, cp = (torch.full(s, float("nan"), device=dev) for s in ((N, D + 3), (N, D * S + 5), (N, D + 2)))
    xp[:, :D], sp[:, : D * S], cp[:, :D] = x, sig.reshape(N, -1), cst
    if case.family == "mnn":
        return case.net.forward(xp[:, :D], sp[:, : D * S])
    return case.net.forward(xp[:, :D], sp[:, : D * S].unflatten(1, (D, S)), cp[:, :D])


def _small_before(case_of, family, dev):
    """A small image on the 8-tile kernel functions: launched before a large one (whose LDS grant then GROWS from this one) and again after it."""
    small = case_of(family, SMALL_TM8, 3)
    inputs = _dev(dev, *draw_inputs(67, 3, SMALL_TM8[0], seed=77))
    return small, inputs


@pytest.mark.parametrize("family,shape", [(f, s) for f in FAMILIES for s in ENVELOPE], ids=lambda v: v if isinstance(v, str) else shape_id(v))
def test_forward_over_the_shape_envelope(dev, case_of, family, shape):
    S, widths = shape
    N, F = 400, 3
    case = case_of(family, shape, F)
    small, small_in = _small_before(case_of, family, dev)
    y_s, ladj_s = small.forward(*small_in)
    x, sig, cst = draw_inputs(N, F, S, seed=S + 31 * len(widths))
    xd, sd, cd = _dev(dev, x, sig, cst)
    y, ladj = case.forward(xd, sd, cd)
    (y32, l32), (y64, l64) = case.ref_forward(x, sig, cst, F32), case.ref_forward(x, sig, cst, F64)
    assert bool(torch.isfinite(y64).all() and torch.isfinite(l64).all() and torch.isfinite(y32).all() and torch.isfinite(l32).all())
    what = f"{family} {shape_id(shape)}: forward"
    assert_parity(y, y32, y64, f"{what} y")
    assert_parity(ladj, l32, l64, f"{what} ladj")
    y_r, ladj_r = case.forward(xd, sd, cd, reduce=True)
    assert torch.equal(y_r, y)
    assert_parity(ladj_r, l32.sum(-1, dtype=F32), l64.sum(-1), f"{what} ladj reduced")
    # the row sum adds the columns left to right: exactly the fp32 sum of the per-element values in that order
    acc = torch.zeros_like(ladj_r)
    for d in range(F):
        acc = acc + ladj[:, d]
    assert torch.equal(ladj_r, acc)
    y_p, ladj_p = _padded(case, xd, sd, cd)
    assert torch.equal(y_p, y) and torch.equal(ladj_p, ladj)
    # the small image again, after whatever grant this shape took: the same bits
    y_s2, ladj_s2 = small.forward(*small_in)
    assert torch.equal(y_s2, y_s) and torch.equal(ladj_s2, ladj_s)


def _inverse_check(case, what, x, sig, cst, dev):
    """Targets = the float64 forward values rounded to float32; assert_parity on the solutions, and the round trip |f(x) - target| in float64 within
    C_NOISE of the float32 reference's own (tests/test_gpu_mnn.py: test_inverse_parity_and_round_trip)."""
    t = case.ref_forward(x, sig, cst, F64)[0].float().contiguous()
    got = case.inverse(*_dev(dev, t, sig, cst))
    inv32, inv64 = case.ref_inverse(t, sig, cst, F32), case.ref_inverse(t, sig, cst, F64)
    assert float(inv64.abs().max()) < 9.99, "a bisection of the reference ended at the bound"
    assert_parity(got, inv32, inv64, f"{what} x")
    res = lambda v: (case.ref_forward(v.cpu(), sig, cst, F64)[0] - t.double()).abs()
    r_hip, r_ref = _stats(res(got)), _stats(res(inv32))
    print(f"{what}: round trip |f(inv(y)) - y| max/p99.9/median  kernel {r_hip[0]:.3e}/{r_hip[1]:.3e}/{r_hip[2]:.3e}  float32 reference {r_ref[0]:.3e}/{r_ref[1]:.3e}/{r_ref[2]:.3e}")
    assert all(a <= C_NOISE * b for a, b in zip(r_hip, r_ref)), (r_hip, r_ref)


@pytest.mark.parametrize("family,shape", [("mnn", s) for s in ENVELOPE] + [("umnn", s) for s in ENVELOPE if s == SMALL_TM8 or s in UMNN_INVERSE_SHAPES],
                         ids=lambda v: v if isinstance(v, str) else shape_id(v))
def test_inverse_over_the_shape_envelope(dev, case_of, family, shape):
    """MNN: all shapes at 400 x 3.  UMNN: the two images above 64 KiB and the smallest network (and, before them, the small 8-tile image their grant
    grows from) at 67 x 2: its CPU reference costs 25 x 32 evaluations per element."""
    S, widths = shape
    N, F = (400, 3) if family == "mnn" else (67, 2)
    case = case_of(family, shape, F)
    small, small_in = _small_before(case_of, family, dev)
    x_s = small.inverse(*small_in)
    x, sig, cst = draw_inputs(N, F, S, seed=5 + S + 31 * len(widths))
    _inverse_check(case, f"{family} {shape_id(shape)}: inverse", x, sig, cst, dev)
    assert torch.equal(small.inverse(*small_in), x_s)


# ---- 2. launch geometries -----------------------------------------------------------------------------------------------------------------


def _tiles(N, D):
    """(row slice, column slice) pairs that cover an [N, D] batch: <= 1000 rows, and <= 400 columns where there are more than 64."""
    cstep = D if D <= 64 else 400
    return [(slice(a, min(N, a + 1000)), slice(c, min(D, c + cstep))) for a in range(0, N, 1000) for c in range(0, D, cstep)]


def _call(fn, a, sig, cst, rows, cols, D):
    """One contiguous launch of the rows `rows` and columns `cols` (with their features) of a batch."""
    feat = None if (cols.start, cols.stop) == (0, D) else list(range(cols.start, cols.stop))
    return fn(a[rows, cols].contiguous(), sig[rows, cols].contiguous(), cst[rows, cols].contiguous(), feat=feat)


@pytest.mark.parametrize("family,shape", [(f, s) for f in FAMILIES for s in GEOMETRY_SHAPES], ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_every_launch_geometry_equals_the_reference_and_the_smallest_geometry(dev, case_of, family, shape):
    """Reference parity on a row sample (the first and last 300 rows, rows around multiples of 64, 128 and 256: 2048 rows of the tall batches, every
    row of the short ones), then bit identity of ALL rows and columns with launches of <= 1000 rows (<= 400 columns) and with single-column
    launches, every one of which takes the (64, 1) geometry.  The sample is thinned where the CPU reference would take more than a few seconds: 8 of
    the 64 columns at the benchmark's proportions (a whole 4-column block and the last column among them) and about 40 of the 600 / 1030 (the first
    and last 8 and every 37th); every other sampled row for the inverse and for the quadrature at the wide network; the UMNN inverse (25 x 32
    evaluations per element) on every 4th sampled row, at the wide network on every 16th and 4 columns."""
    N, D = shape
    net = DEFAULT if shape == (16384, 64) else (2, (16,))
    S = net[0]
    assert geometry(N, D, family) == GEOMETRY_SHAPES[shape]
    case = case_of(family, net, D)
    x, sig, cst = draw_inputs(N, D, S, seed=N % 1000 + D)
    xd, sd, cd = _dev(dev, x, sig, cst)
    y, ladj = case.forward(xd, sd, cd)
    inv = case.inverse(y, sd, cd)  # (targets: the kernel's own forward values, all inside f(+-bound))
    y_c, inv_c = y.cpu(), inv.cpu()

    rows = sample_rows(N)
    wide = net == DEFAULT
    cols = [0, 1, 2, 3, 4, 31, 62, 63] if wide else list(range(D)) if D <= 64 else sorted(set(range(8)) | set(range(D - 8, D)) | set(range(0, D, 37)))
    what = f"{family} geometry {GEOMETRY_SHAPES[shape]} at {N}x{D}:"
    pick = lambda a, r, c: a[r][:, c]
    r_f = rows[::2] if wide and family == "umnn" else rows
    ref32, ref64 = (case.ref_forward(pick(x, r_f, cols), pick(sig, r_f, cols), pick(cst, r_f, cols), dt, feat=cols) for dt in (F32, F64))
    assert_parity(pick(y_c, r_f, cols), ref32[0], ref64[0], f"{what} forward y")
    assert_parity(pick(ladj.cpu(), r_f, cols), ref32[1], ref64[1], f"{what} forward ladj")
    if family == "umnn":
        r_i, c_i = (rows[::16], cols[:4]) if wide else (rows[::4], cols)
    else:
        r_i, c_i = (rows[::2], cols) if wide else (rows, cols)
    i32, i64 = (case.ref_inverse(pick(y_c, r_i, c_i), pick(sig, r_i, c_i), pick(cst, r_i, c_i), dt, feat=c_i) for dt in (F32, F64))
    assert_parity(pick(inv_c, r_i, c_i), i32, i64, f"{what} inverse x")

    w = min(N, 1000)
    singles = range(D) if D <= 64 else [0, 1, 5, D // 2, D - 2, D - 1]
    tiles = _tiles(N, D) + [(r, slice(c, c + 1)) for c in singles for r in (slice(0, w), slice(N - w, N))]
    bad = []
    for r, c in tiles:
        assert geometry(r.stop - r.start, c.stop - c.start, family) == (64, 1), (r, c)
        y_k, ladj_k = _call(case.forward, xd, sd, cd, r, c, D)
        if not (torch.equal(y_k, y[r, c]) and torch.equal(ladj_k, ladj[r, c]) and torch.equal(_call(case.inverse, y, sd, cd, r, c, D), inv[r, c])):
            bad.append((r.start, r.stop, c.start, c.stop))
    assert not bad, f"(rows, columns) {bad[:8]} differ from their own launch"


@pytest.mark.parametrize("family", FAMILIES)
def test_a_permuted_feature_table_under_four_features_per_block(dev, case_of, family):
    """Dsel = 6 of F = 9 features in a scrambled order at 16389 rows: geometry (64, 4), the second block of columns holds two features."""
    N, F, feat = 16389, 9, [7, 2, 8, 0, 5, 3]
    D, net = len(feat), (2, (16,))
    assert geometry(N, D, family) == (64, 4) and geometry(N, 1, family) == (64, 1)
    case = case_of(family, net, F)
    x, sig, cst = draw_inputs(N, D, net[0], seed=9)
    xd, sd, cd = _dev(dev, x, sig, cst)
    y, ladj = case.forward(xd, sd, cd, feat=feat)
    inv = case.inverse(y, sd, cd, feat=feat)
    for j, f in enumerate(feat):
        c = slice(j, j + 1)
        one = (xd[:, c].contiguous(), sd[:, c].contiguous(), cd[:, c].contiguous())
        y_j, ladj_j = case.forward(*one, feat=[f])
        assert torch.equal(y_j, y[:, c]) and torch.equal(ladj_j, ladj[:, c]), f"column {j} (feature {f})"
        assert torch.equal(case.inverse(y[:, c].contiguous(), one[1], one[2], feat=[f]), inv[:, c]), f"inverse, column {j} (feature {f})"
    rows = sample_rows(N)
    ref32, ref64 = (case.ref_forward(x[rows], sig[rows], cst[rows], dt, feat=feat) for dt in (F32, F64))
    what = f"{family} permuted features, geometry (64, 4):"
    assert_parity(y[rows.to(dev)], ref32[0], ref64[0], f"{what} forward y")
    assert_parity(ladj[rows.to(dev)], ref32[1], ref64[1], f"{what} forward ladj")
    y_r, ladj_r = case.forward(xd, sd, cd, feat=feat, reduce=True)
    acc = torch.zeros_like(ladj_r)
    for d in range(D):
        acc = acc + ladj[:, d]
    assert torch.equal(y_r, y) and torch.equal(ladj_r, acc)


# ---- 3. quadrature sizes ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("n_quad", [1, 2, 7, 33, 64])
def test_quadrature_sizes(dev, case_of, n_quad):
    """Odd sizes end the forward direction on a (node, x) pair and the inverse on a lone node; 1 and 64 are the limits of the ABI."""
    S, F = DEFAULT[0], 3
    case = case_of("umnn", DEFAULT, F, n_quad)
    assert case.net.n_quad == n_quad and case.net.quad.numel() == 2 * n_quad
    x, sig, cst = draw_inputs(130, F, S, seed=40 + n_quad)
    y, ladj = case.forward(*_dev(dev, x, sig, cst))
    (y32, l32), (y64, l64) = case.ref_forward(x, sig, cst, F32), case.ref_forward(x, sig, cst, F64)
    assert_parity(y, y32, y64, f"umnn n_quad {n_quad}: forward y")
    assert_parity(ladj, l32, l64, f"umnn n_quad {n_quad}: forward ladj")
    if n_quad in (1, 7):
        _inverse_check(case, f"umnn n_quad {n_quad}: inverse", x[:67], sig[:67], cst[:67], dev)


# ---- 4. non-finite inputs -----------------------------------------------------------------------------------------------------------------

X_CLASSES = [float("inf"), float("-inf"), float("nan"), 0.0, 10.0, -10.0, 1e30, -1e30]


@pytest.mark.parametrize("family", FAMILIES)
def test_non_finite_inputs_follow_the_reference(dev, case_of, family):
    """24 rows of every x in X_CLASSES (each class compared on its own, so that the scale of one does not hide another), then a row with a NaN and a
    row with an inf in one feature's signal; assert_parity requires the NaN pattern and the infinities of the float32 reference."""
    S, F, R = DEFAULT[0], 3, 24
    case = case_of(family, DEFAULT, F)
    N = R * len(X_CLASSES) + 2
    x, sig, cst = draw_inputs(N, F, S, seed=99)
    for k, v in enumerate(X_CLASSES):
        x[k * R : (k + 1) * R] = v
    sig[N - 2, 1, 5], sig[N - 1, 2, 0] = float("nan"), float("inf")
    y, ladj = (t.cpu() for t in case.forward(*_dev(dev, x, sig, cst)))
    (y32, l32), (y64, l64) = case.ref_forward(x, sig, cst, F32), case.ref_forward(x, sig, cst, F64)
    assert bool(torch.isnan(y32[2 * R : 3 * R]).all() and torch.isnan(y32[N - 2, 1])) and not bool(torch.isnan(y32[N - 2, [0, 2]]).any())
    for k, v in list(enumerate(X_CLASSES)) + [(len(X_CLASSES), "signal")]:
        r = slice(k * R, min(N, (k + 1) * R))
        assert_parity(y[r], y32[r], y64[r], f"{family} non-finite, x = {v}: forward y")
        assert_parity(ladj[r], l32[r], l64[r], f"{family} non-finite, x = {v}: forward ladj")


@pytest.mark.parametrize("family", FAMILIES)
def test_non_finite_targets_end_where_the_reference_ends(dev, case_of, family):
    """Targets NaN and +-inf: every comparison of the bisection goes one way, and the kernel returns the end of the interval the float32 reference
    returns, bit for bit."""
    S, F = DEFAULT[0], 3
    case = case_of(family, DEFAULT, F)
    _, sig, cst = draw_inputs(48, F, S, seed=98)
    t = torch.empty(48, F)
    t[:16], t[16:32], t[32:] = float("nan"), float("inf"), float("-inf")
    got = case.inverse(*_dev(dev, t, sig, cst)).cpu()
    ref = case.ref_inverse(t, sig, cst, F32)
    assert bool((ref[:16] < -9.99).all() and (ref[16:32] > 9.99).all() and (ref[32:] < -9.99).all())
    assert torch.equal(got, ref)
