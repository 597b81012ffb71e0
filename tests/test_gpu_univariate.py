"""GPU parity: univariate transform kernels (through the C-ABI) against the golden vectors of the
reference and against the CPU oracle on fresh seeded inputs.

Tolerances (north_star): fp32 allclose(rtol=1e-5, atol=1e-5) on y / ladj / inverse — or, where two correct fp32
evaluations cannot agree that closely (ill-conditioned bins, bisection inverses, the Beta-pdf form of the Bernstein
basis), within 4x the fp32 reference's own distance from the float64 oracle (tests/parity.py); bit-exact spline bin
index on shared knots; fp64 1e-12."""

import numpy as np
import pytest
import torch

from conftest import T, golden
from oracle import zuko_oracle as O
from parity import C_ADVERSARIAL, assert_f64, assert_parity, d64

pytestmark = pytest.mark.gpu

TOL = {"f32": 1e-5, "f64": 1e-12}


def close(a, b, what, tol):
    a = a.detach().cpu()
    b = T(b) if isinstance(b, np.ndarray) else b.detach().cpu()
    assert a.shape == b.shape, f"{what}: shape {tuple(a.shape)} vs {tuple(b.shape)}"
    ok = torch.allclose(a, b, rtol=tol, atol=tol, equal_nan=True)
    if not ok:
        d = (a - b).abs().nan_to_num()
        i = d.argmax()
        raise AssertionError(f"{what}: max|d|={d.max():.3e} at {np.unravel_index(int(i), a.shape)}: {a.flatten()[i]} vs {b.flatten()[i]}; nan mismatch={int((a.isnan() != b.isnan()).sum())}")


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_rqs_golden(dev, tag):
    from zuko_amd import ops
    import zuko_amd.transforms as ZT

    g = golden(f"rqs_{tag}.npz")
    tol = TOL[tag]
    w, h, d, x = (T(g[n], dev) for n in ("widths", "heights", "derivatives", "x"))
    with torch.no_grad():
        # 1) shared knots: bin index must be bit-exact, values to tolerance
        y, ladj, k = ops.rqs_from_knots(x, T(g["horizontal"], dev), T(g["vertical"], dev), T(g["slopes"], dev))
        assert torch.equal(k.cpu().long(), T(g["k"])), "bin index differs on shared knots"
        close(y, g["y"], "y (shared knots)", tol)
        close(ladj, g["ladj"], "ladj (shared knots)", tol)
        xi, _, ki = ops.rqs_from_knots(T(g["y_in"], dev), T(g["horizontal"], dev), T(g["vertical"], dev), T(g["slopes"], dev), inverse=True)
        assert torch.equal(ki.cpu().long(), T(g["k_inv"]))
        close(xi, g["x_inv"], "x_inv (shared knots)", tol)
        # 2) from unconstrained parameters (device expf vs Sleef: knots may move by an ulp)
        t = ZT.MonotonicRQSTransform(w, h, d)
        y2, l2 = t.call_and_ladj(x)
        k2 = t.bin_index(x)
        flips = int((k2.cpu().long() != T(g["k"])).sum())
        edge = np.isin(np.arange(x.shape[0]), np.arange(16))[:, None] & np.ones_like(g["k"], bool)
        assert int(((k2.cpu().long() != T(g["k"])) & ~T(edge)).sum()) == 0, "bin flips away from the adversarial rows"
        same = k2.cpu().long() == T(g["k"])
        if tag == "f32":
            w64, h64, dd64, x64 = (d64(g[n]) for n in ("widths", "heights", "derivatives", "x"))
            y64, l64 = O.rqs_forward(w64, h64, dd64, x64)
            assert_parity(y2, g["y"], y64, "rqs golden f32: y from parameters", where=same)
            assert_parity(l2, g["ladj"], l64, "rqs golden f32: ladj from parameters", where=same, c=C_ADVERSARIAL)
            # elements whose bin flipped (x within rounding of a knot the two evaluations place an ulp apart) are COMPARED, not skipped:
            # the spline is C1 at a knot, so y and log|dy/dx| of the neighbouring bin differ from the reference's by O(knot distance) — bars: y within
            # 1e-5 (1 + |y|) + the largest slope around the knot x 4 ulps of the knot; ladj within 1e-4 (the second derivative jumps at a knot and the
            # adversarial rows have bins 1e-3 wide; measured on this set: 6 flipped elements, max |dy| 2.7e-6, max |dladj| 1.1e-5)
            flip = ~same
            if flip.any():
                yv, yr, lv, lr = y2.cpu()[flip].double(), T(g["y"])[flip].double(), l2.cpu()[flip].double(), T(g["ladj"])[flip].double()
                slope = T(g["slopes"]).double().abs().amax(dim=-1)[flip]
                knot_ulp = 4 * 2.0 ** -23 * torch.maximum(x.cpu().abs().double()[flip], torch.tensor(1.0, dtype=torch.float64))
                ey, el = (yv - yr).abs(), (lv - lr).abs()
                print(f"rqs[f32] flipped elements: {int(flip.sum())}, max |dy| {ey.max():.2e}, max |dladj| {el.max():.2e}")
                assert bool((ey <= 1e-5 * (1 + yr.abs()) + slope * knot_ulp).all()), f"y on bin-flipped elements: max |d| {ey.max():.3e}"
                assert bool((el <= 1e-4).all()), f"ladj on bin-flipped elements: max |d| {el.max():.3e}"
        else:
            close(torch.where(same.to(dev), y2, T(g["y"], dev)), g["y"], "y", tol)
            close(torch.where(same.to(dev), l2, T(g["ladj"], dev)), g["ladj"], "ladj", tol)
        print(f"rqs[{tag}] end-to-end bin flips on adversarial set: {flips}")
        close(t.log_abs_det_jacobian(x, y2), l2, "ladj method", 0)
        xi2 = t.inv(T(g["y_in"], dev))
        same_i = (ops.rqs_inverse(T(g["y_in"], dev), w, h, d, want_bins=True)[1].cpu().long() == T(g["k_inv"]))
        if tag == "f32":  # (the inverse divides knot rounding noise by the local slope, as small as 1e-3 on this set)
            assert_parity(xi2, g["x_inv"], O.rqs_inverse(w64, h64, dd64, d64(g["y_in"])), "rqs golden f32: inverse from parameters", where=same_i)
        else:
            close(torch.where(same_i.to(dev), xi2, T(g["x_inv"], dev)), g["x_inv"], "inverse", tol)
        # 3) feature-reduced ladj
        yr, lr = t.call_and_ladj_reduced(x)
        close(yr, y2, "reduced y", 0)
        close(lr, l2.sum(-1), "reduced ladj (same values, another summation tree over 64 features)", 64 * 2.0**-23 * 4 if tag == "f32" else 1e-11)
        # 4) unbatched parameters broadcast against x (tests/test_transforms.py:12-32 of the reference)
        t1 = ZT.MonotonicRQSTransform(w[0, 0], h[0, 0], d[0, 0])
        yl, ll = t1.call_and_ladj(T(g["x_lin"], dev))
        close(yl, g["y_lin"], "y_lin", tol)
        close(ll, g["ladj_lin"], "ladj_lin", tol)
        if tag == "f32":
            w1, h1, d1 = d64(g["widths"])[0, 0], d64(g["heights"])[0, 0], d64(g["derivatives"])[0, 0]
            yl32 = T(g["y_lin"])
            assert_parity(t1.inv(T(g["y_lin"], dev)), O.rqs_inverse(T(g["widths"])[0, 0], T(g["heights"])[0, 0], T(g["derivatives"])[0, 0], yl32), O.rqs_inverse(w1, h1, d1, yl32.double()), "rqs golden f32: inverse of y_lin")
        else:
            close(t1.inv(yl), g["x_lin"], "roundtrip", 1e-9)


@pytest.mark.parametrize("shape,K", [((1000, 64), 8), ((257, 3), 8), ((33, 200), 8), ((5, 7, 11), 4), ((64, 16), 16), ((40, 6), 5), ((0, 8), 8), ((3, 1), 8), ((40, 6), 64)])
def test_rqs_vs_oracle_shapes(dev, shape, K):
    """Packed phi (LDS-staged path), ragged / non-power-of-two feature counts, D > 64, 3-d batches,
    generic bin counts (K = 5, and K = 64: the cap of the run-time path), empty input."""
    import zuko_amd.transforms as ZT
    from zuko_amd.utils import unpack

    gen = torch.Generator().manual_seed(hash((shape, K)) % 2**31)
    phi = torch.randn(*shape, 3 * K - 1, generator=gen) * 1.5
    x = torch.randn(*shape, generator=gen) * 2.2
    w, h, d = unpack(phi, [(K,), (K,), (K - 1,)])
    hor, ver, der = O.rqs_knots(w, h, d)
    phig = phi.to(dev)
    wg, hg, dg = unpack(phig, [(K,), (K,), (K - 1,)])  # views of ONE packed buffer
    t = ZT.MonotonicRQSTransform(wg, hg, dg)
    with torch.no_grad():
        y, ladj = t.call_and_ladj(x.to(dev))
        if x.numel() == 0:
            assert y.shape == x.shape
            return
        k = t.bin_index(x.to(dev)).cpu().long()
        oy, ol, ok = O.rqs_forward_from_knots(hor, ver, der, x)
        same = k == ok
        assert (~same).float().mean() < 1e-4
        # Parameters ~ 1.5*N(0,1) produce very narrow / steep bins, where an ulp of difference in a
        # knot (device expf vs Sleef) moves y and ladj by far more than 1e-5 — for the reference's
        # own fp32 evaluation too.  So the bar here is "no worse than the fp32 reference's rounding
        # noise", both measured against the float64 oracle: max and 99.9th percentile within 4x.
        y64, l64, k64 = O.rqs_forward_from_knots(*O.rqs_knots(w.double(), h.double(), d.double()), x.double())
        good = same & (ok == k64)
        for what, mine, ref32, ref64 in (("y", y.cpu(), oy, y64), ("ladj", ladj.cpu(), ol, l64)):
            e_hip = (mine.double() - ref64).abs()[good]
            e_ref = (ref32.double() - ref64).abs()[good]
            assert e_hip.max() <= 4 * e_ref.max() + 1e-6, f"{what}: hip max err {e_hip.max():.3e} vs fp32-reference max err {e_ref.max():.3e}"
            q = lambda e: torch.quantile(e, 0.999) if e.numel() > 1000 else e.max()
            assert q(e_hip) <= 4 * q(e_ref) + 1e-6, f"{what}: p99.9 {q(e_hip):.3e} vs {q(e_ref):.3e}"
            assert torch.median(e_hip) <= 4 * torch.median(e_ref) + 1e-7
        yr, lr = t.call_and_ladj_reduced(x.to(dev))
        close(lr, ladj.sum(-1), "reduced", 1e-3)
        xr = t.inv(y)
        close(xr, x, "roundtrip", 5e-3)
        # strided (non-packed) parameters take the other instantiation: same numbers
        t2 = ZT.MonotonicRQSTransform(wg.contiguous(), hg.contiguous(), dg.contiguous())
        y2, l2 = t2.call_and_ladj(x.to(dev))
        close(y2, y, "strided y", 0)
        close(l2, ladj, "strided ladj", 0)


@pytest.mark.parametrize("N,D,K", [(4096, 64, 8), (1000, 64, 8), (512, 16, 8), (96, 128, 8), (33, 192, 4), (256, 64, 16), (128, 64, 4), (64, 1, 8), (3, 64, 8)])
def test_rqs_stream_kernel_matches_general(dev, N, D, K, monkeypatch):
    """The fp32 stream kernel (packed, 16-byte aligned phi, N*D % 64 == 0) and the general kernel run the
    same arithmetic: bit-identical y / ladj / inverse for every ladj mode and every tile-dealing scheme,
    and both agree with the oracle to the north_star tolerance on a well-conditioned spline."""
    from zuko_amd import ops

    gen = torch.Generator().manual_seed(N * 131 + D * 7 + K)
    phi = (torch.randn(N, D, 3 * K - 1, generator=gen) * 0.7).to(dev)
    x = (torch.randn(N, D, generator=gen) * 2.5).to(dev)
    x[0, 0] = 7.0  # outside the spline's support: identity, ladj 0
    w, h, d = phi[..., :K], phi[..., K : 2 * K], phi[..., 2 * K :]
    with torch.no_grad():
        monkeypatch.setenv("ZUKO_AMD_NO_STREAM", "1")
        y0, l0 = ops.rqs_forward(x, w, h, d)
        _, r0 = ops.rqs_forward(x, w, h, d, reduce=True)
        i0 = ops.rqs_inverse(y0, w, h, d)
        monkeypatch.setenv("ZUKO_AMD_NO_STREAM", "0")
        for chunk in ("-1", "0", "2", "4", "6"):
            monkeypatch.setenv("ZUKO_AMD_K1_CHUNK", chunk)
            y1, l1 = ops.rqs_forward(x, w, h, d)
            y2, r1 = ops.rqs_forward(x, w, h, d, reduce=True)
            i1 = ops.rqs_inverse(y0, w, h, d)
            assert torch.equal(y1, y0) and torch.equal(l1, l0) and torch.equal(y2, y0) and torch.equal(i1, i0), chunk
            close(r1, r0, f"reduced ladj (chunk {chunk})", 2e-6 * D)  # different summation trees
        assert y0[0, 0] == 7.0 and l0[0, 0] == 0.0
    oy, ol, _ = O.rqs_forward_from_knots(*O.rqs_knots(w.cpu().double(), h.cpu().double(), d.cpu().double()), x.cpu().double())
    close(y0.double(), oy, "y vs float64 oracle", 2e-5)
    close(l0.double(), ol, "ladj vs float64 oracle", 1e-4)
    close(i0, x, "round trip", 1e-4)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_affine_golden(dev, tag):
    import zuko_amd.transforms as ZT

    g = golden(f"affine_{tag}.npz")
    tol = TOL[tag]
    t = ZT.MonotonicAffineTransform(T(g["shift"], dev), T(g["scale"], dev))
    with torch.no_grad():
        y, ladj = t.call_and_ladj(T(g["x"], dev))
        close(y, g["y"], "y", tol)
        close(ladj, g["ladj"], "ladj", tol)
        close(t.inv(T(g["x"], dev)), g["x_inv"], "inverse", tol)
        _, lr = t.call_and_ladj_reduced(T(g["x"], dev))
        close(lr, T(g["ladj"]).sum(-1), "reduced", 10 * tol)
        # packed [shift, scale] pairs as the MAF conditioner emits them
        phi = torch.stack((T(g["shift"]), T(g["scale"])), dim=-1).to(dev)
        tp = ZT.MonotonicAffineTransform(phi[..., 0], phi[..., 1])
        yp, lp = tp.call_and_ladj(T(g["x"], dev))
        close(yp, y, "packed y", 0)
        close(lp, ladj, "packed ladj", 0)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_sos_golden(dev, tag):
    import zuko_amd.transforms as ZT

    g = golden(f"sos_{tag}.npz")
    t = ZT.SOSPolynomialTransform(T(g["a"], dev))
    with torch.no_grad():
        y, ladj = t.call_and_ladj(T(g["x"], dev))
        xi = t.inv(T(g["y"], dev))
        if tag == "f32":
            y64, l64 = O.sos_forward(d64(g["a"]), d64(g["x"]))
            assert_parity(y, g["y"], y64, "sos golden f32: y")
            assert_parity(ladj, g["ladj"], l64, "sos golden f32: ladj")
            assert_parity(xi, g["x_inv"], O.sos_inverse(d64(g["a"]), d64(g["y"])), "sos golden f32: inverse (25-step bisection)")
        else:
            assert_f64(y, g["y"], "sos golden f64: y")
            assert_f64(ladj, g["ladj"], "sos golden f64: ladj")
            assert_f64(xi, g["x_inv"], "sos golden f64: inverse (25-step bisection: interval 20 / 2^25)", 20.0 / 2**25)
        tol = 1e-5 if tag == "f32" else 1e-12
        c = torch.randn(g["x"].shape, generator=torch.Generator().manual_seed(3), dtype=T(g["x"]).dtype).to(dev)
        ts = ZT.ShiftedSOSPolynomialTransform(T(g["a"], dev), c)
        ys, ls = ts.call_and_ladj(T(g["x"], dev))
        close(ys, y + c, "shifted y", tol)
        close(ts.inv(ys), g["x"], "shifted roundtrip", 1e-4)


@pytest.mark.parametrize("tag", ["f32", "f64"])
@pytest.mark.parametrize("name", ["bern", "bbern"])
def test_bernstein_golden(dev, tag, name):
    import zuko_amd.transforms as ZT

    g = golden(f"{name}_{tag}.npz")
    cls = ZT.BoundedBernsteinTransform if name == "bbern" else ZT.BernsteinTransform
    t = cls(T(g["theta"], dev))
    with torch.no_grad():
        y, ladj = t.call_and_ladj(T(g["x"], dev))
        xi = t.inv(T(g["y"], dev))
    if tag == "f32":
        # the reference evaluates the basis as Beta(i + 1, M - i + 1).log_prob(u).exp() (lgamma, log, exp in fp32) and takes
        # the derivative by autograd through it (zuko/transforms.py:729-740, 623-637); the kernel evaluates the same
        # polynomial by de Casteljau with the closed-form derivative.  Both against the float64 oracle:
        y64, l64 = O.bern_forward(d64(g["theta"]), d64(g["x"]), name == "bbern")
        assert_parity(y, g["y"], y64, f"{name} golden f32: y")
        # (round 6: the derivative is a de Casteljau sweep over the positive coefficient differences — 1.3e-6 from float64 on the adversarial `bern` set, where the
        #  float32 reference itself sits 1.6e-5 away; until then the comparison needed its own constant, ratio 2.93)
        assert_parity(ladj, g["ladj"], l64, f"{name} golden f32: ladj")
        assert_parity(xi, g["x_inv"], O.bern_inverse(d64(g["theta"]), d64(g["y"]), name == "bbern"), f"{name} golden f32: inverse (24-step bisection)")
    else:
        # float64: the closed form equals the reference's Beta-pdf form to 6e-14 on this set (measured in the build container
        # with an 80-bit evaluation: tests/test_oracle_c.py holds the C restatement to the same 1e-12)
        assert_f64(y, g["y"], f"{name} golden f64: y")
        assert_f64(ladj, g["ladj"], f"{name} golden f64: ladj")
        assert_f64(xi, g["x_inv"], f"{name} golden f64: inverse (24-step bisection: interval 10 / 2^24)", 10.0 / 2**24)


@pytest.mark.parametrize("bounded", [False, True])
@pytest.mark.parametrize("eps", [1e-3, 2e-2])
def test_bernstein_eps_is_a_run_time_argument(dev, bounded, eps):
    """`eps` (MonotonicTransform's kwarg, zuko/transforms.py:594: continuation margin + bisection depth) away from its default: forward,
    ladj and inverse in float64 against the oracle (whose eps argument is pinned to the live reference in tests/test_integration_option2.py),
    with inputs inside the widened margins and beyond the bound; float32 against the measured bar."""
    import zuko_amd.transforms as ZT

    g = torch.Generator().manual_seed(7)
    theta = torch.randn(64, 3, 17 if bounded else 16, generator=g, dtype=torch.float64)
    x = torch.randn(64, 3, generator=g, dtype=torch.float64) * 3.5
    x[0, 0], x[0, 1], x[1, 0], x[1, 1] = 4.99, -4.995, 5.2, -5.5
    cls = ZT.BoundedBernsteinTransform if bounded else ZT.BernsteinTransform
    oy, ol = O.bern_forward(theta, x, bounded, eps=eps)
    ox = O.bern_inverse(theta, oy, bounded, eps=eps)
    with torch.no_grad():
        t = cls(theta.to(dev), eps=eps)
        y, ladj = t.call_and_ladj(x.to(dev))
        assert_f64(y, oy, f"bernstein eps={eps} bounded={bounded} f64: y")
        assert_f64(ladj, ol, f"bernstein eps={eps} bounded={bounded} f64: ladj")
        assert_f64(t.inv(oy.to(dev)), ox, f"bernstein eps={eps} bounded={bounded} f64: inverse", 10.0 / 2 ** (np.ceil(np.log2(10.0 / eps)) - 1))
        t32 = cls(theta.float().to(dev), eps=eps)
        y32, l32 = t32.call_and_ladj(x.float().to(dev))
        ry, rl = O.bern_forward(theta.float(), x.float(), bounded, eps=eps)
        assert_parity(y32, ry, oy, f"bernstein eps={eps} bounded={bounded} f32: y")
        assert_parity(l32, rl, ol, f"bernstein eps={eps} bounded={bounded} f32: ladj")


def test_rqs_bin_count_above_the_cap_fails_cleanly(dev):
    """K = 65 is one more than the run-time path is built for (ZK_RQS_KMAX): an error from the entry point, no launch."""
    import zuko_amd.transforms as ZT

    K = 65
    gen = torch.Generator().manual_seed(65)
    phi = torch.randn(40, 6, 3 * K - 1, generator=gen).to(dev)
    x = torch.randn(40, 6, generator=gen).to(dev)
    t = ZT.MonotonicRQSTransform(phi[..., :K], phi[..., K : 2 * K], phi[..., 2 * K :])
    with torch.no_grad():
        with pytest.raises(RuntimeError, match="zk_rqs_forward"):
            t.call_and_ladj(x)
        with pytest.raises(RuntimeError, match="zk_rqs_inverse"):
            t.inv(x)


# Coefficient counts with no register-resident instantiation (csrc/elementwise.hip: launch_bern) take the run-time count: NC = 9 is the
# smallest such count both maps reach, NC = 42 a middle one, NC = 72 the cap.  D = 70 > 64 takes the segmented path of the driver.
# float64 bars: 1e-12 up to NC = 42; at NC = 72 the oracle's lgamma-based Beta density of degree 71 is itself 2.6e-12 from a float64
# emulation of the closed forms in ladj (5.3e-13 in y), so the bar there is 1e-10 — 40x that distance, far below any wrong coefficient.
BERN_RUNTIME_CASES = [(False, 7, (40, 6), 1e-12), (True, 4, (40, 6), 1e-12), (False, 40, (40, 6), 1e-12), (False, 70, (40, 6), 1e-10), (True, 67, (40, 6), 1e-10),
                      (False, 7, (3, 70), 1e-12)]


@pytest.mark.parametrize("bounded,M,shape,tol64", BERN_RUNTIME_CASES)
def test_bernstein_run_time_coefficient_counts(dev, bounded, M, shape, tol64):
    """Forward, ladj and inverse of the run-time-count path in float64 and float32 against the oracle, with inputs in both linear tails and
    beyond the bound; strided parameters take the other instantiation and give the same numbers."""
    import zuko_amd.transforms as ZT

    g = torch.Generator().manual_seed(1000 * M + shape[1] + int(bounded))
    theta = torch.randn(*shape, M, generator=g, dtype=torch.float64)
    x = torch.randn(*shape, generator=g, dtype=torch.float64) * 3.5
    x[0, 0], x[0, 1], x[1, 0], x[1, 1] = 4.999995, -4.999996, 5.2, -5.5  # both tails (|u - 1/2| >= 1/2 - eps), beyond the bound
    cls = ZT.BoundedBernsteinTransform if bounded else ZT.BernsteinTransform
    what = f"bernstein M={M} bounded={bounded} {shape}"
    oy, ol = O.bern_forward(theta, x, bounded)
    ox = O.bern_inverse(theta, oy, bounded)
    with torch.no_grad():
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            th = theta.to(dt).to(dev)
            wide = torch.zeros(*shape, M + 3, dtype=dt, device=dev)
            wide[..., :M] = th
            t, ts = cls(th), cls(wide[..., :M])  # one packed buffer / element stride M + 3
            xin, yin = x.to(dt).to(dev), oy.to(dt).to(dev)
            y, ladj = t.call_and_ladj(xin)
            xi = t.inv(yin)
            y2, l2 = ts.call_and_ladj(xin)
            close(y2, y, f"{what} {tag}: strided y", 0)
            close(l2, ladj, f"{what} {tag}: strided ladj", 0)
            close(ts.inv(yin), xi, f"{what} {tag}: strided inverse", 0)
            if tag == "f64":
                assert_f64(y, oy, f"{what} f64: y", tol64)
                assert_f64(ladj, ol, f"{what} f64: ladj", tol64)
                assert_f64(xi, ox, f"{what} f64: inverse (24-step bisection: interval 10 / 2^24)", 10.0 / 2**24)
            else:
                ry, rl = O.bern_forward(theta.float(), x.float(), bounded)
                assert_parity(y, ry, oy, f"{what} f32: y")
                assert_parity(ladj, rl, ol, f"{what} f32: ladj")
                assert_parity(xi, O.bern_inverse(theta.float(), oy.float(), bounded), O.bern_inverse(theta, oy.float().double(), bounded), f"{what} f32: inverse (24-step bisection)")


def test_bernstein_above_the_cap_is_refused():
    import zuko_amd.transforms as ZT

    with pytest.raises(NotImplementedError):
        ZT.BernsteinTransform(torch.zeros(4, 2, 71))  # NC = 73 > 72 constrained coefficients


@pytest.mark.parametrize("P,L1", [(2, 3), (4, 2)])
@pytest.mark.parametrize("shifted", [False, True])
def test_sos_run_time_shapes(dev, P, L1, shifted):
    """Any layout other than SOSPF's 3 x 5 takes the run-time counts of sos_f / sos_g / sos_inv: float64 and float32 against the oracle,
    with and without the shift constant."""
    import zuko_amd.transforms as ZT

    g = torch.Generator().manual_seed(100 * P + L1)
    a = torch.randn(40, 6, P, L1, generator=g, dtype=torch.float64)
    x = torch.randn(40, 6, generator=g, dtype=torch.float64) * 4.0
    c = torch.randn(40, 6, generator=g, dtype=torch.float64) if shifted else None
    shift = lambda v, cc: v if cc is None else v + cc
    what = f"sos {P}x{L1} shifted={shifted}"
    oy, ol = O.sos_forward(a, x)
    oy = shift(oy, c)
    ox = O.sos_inverse(a, oy if c is None else oy - c)
    with torch.no_grad():
        for dt, tag in ((torch.float64, "f64"), (torch.float32, "f32")):
            ad, cd = a.to(dt).to(dev), None if c is None else c.to(dt).to(dev)
            t = ZT.ShiftedSOSPolynomialTransform(ad, cd) if shifted else ZT.SOSPolynomialTransform(ad)
            y, ladj = t.call_and_ladj(x.to(dt).to(dev))
            xi = t.inv(oy.to(dt).to(dev))
            if tag == "f64":
                assert_f64(y, oy, f"{what} f64: y")
                assert_f64(ladj, ol, f"{what} f64: ladj")
                assert_f64(xi, ox, f"{what} f64: inverse (25-step bisection: interval 20 / 2^25)", 20.0 / 2**25)
            else:
                c32 = None if c is None else c.float()
                ry, rl = O.sos_forward(a.float(), x.float())
                assert_parity(y, shift(ry, c32), oy, f"{what} f32: y")
                assert_parity(ladj, rl, ol, f"{what} f32: ladj")
                y32 = oy.float()
                assert_parity(xi, O.sos_inverse(a.float(), y32 if c32 is None else y32 - c32), O.sos_inverse(a, y32.double() if c is None else y32.double() - c32.double()), f"{what} f32: inverse (25-step bisection)")


def test_normal_log_prob_and_sum(dev):
    from zuko_amd import ops

    gen = torch.Generator().manual_seed(5)
    z = torch.randn(1000, 64, generator=gen)
    loc = torch.randn(64, generator=gen)
    scale = torch.rand(64, generator=gen) + 0.5
    ladj = torch.randn(1000, generator=gen)
    ref = O.diag_normal_log_prob(z, loc, scale) + ladj
    out = ops.diag_normal_log_prob(z.to(dev), loc.to(dev), scale.to(dev), ladj.to(dev))
    close(out, ref, "normal log prob", 1e-5)
    s = ops.sum_f64(out, -1.0 / 1000)
    assert abs(s.item() - (-ref.double().mean().item())) < 1e-6
