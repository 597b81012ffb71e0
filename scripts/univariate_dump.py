"""Outputs of every stand-alone univariate entry point on fixed inputs, for comparing two builds bit by bit.

    python scripts/univariate_dump.py OUT.npz [--root DIR]      # DIR: the checkout whose zuko_amd is imported (default: this one)
    python scripts/univariate_dump.py --compare PARENT.npz BRANCH.npz

RQS forward / inverse (K = 8: static, K = 5: run-time count) and from_knots, affine, SOS (3 x 5: static, 2 x 3: run-time counts, with and without
the shift), Bernstein (M = 16 unbounded / 17 bounded: static, M = 7 / 4: run-time count), in float32 and float64 at (257, 3) and (33, 200), and the
float32 backward of the spline and the affine map.  Every input has values outside the map's support and one NaN.

--compare: bitwise equality of every array, except (a) `ladj` of the run-time-count spline, which must be `==` with the same NaN pattern (outside the
support the first / last bin replaces the wrapped one under 0 * log: the sign of zero may differ), and (b) the run-time-count Bernstein polynomial, whose
derivative changed on purpose: `y` must be bitwise equal outside the unbounded map's linear tails (whose slope is that derivative), and for `ladj` and the
inverse the distance of both builds from the float64 oracle is printed: the second build must not be further than the first in max or median."""

import os
import sys

import numpy as np


def dump(out: str, root: str) -> None:
    sys.path.insert(0, root)
    import torch

    from oracle import zuko_oracle as O
    from zuko_amd import ops
    from zuko_amd.utils import unpack

    dev = torch.device("cuda:0")
    res = {}

    def put(name, **arrays):
        for k, v in arrays.items():
            res[f"{name}/{k}"] = v.detach().cpu().numpy()

    for shape in ((257, 3), (33, 200)):
        for dt, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
            g = torch.Generator().manual_seed(20 + shape[0])
            sh = f"{shape[0]}x{shape[1]}/{tag}"

            def inputs(scale, far):
                x = (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(dt)
                x[0, 0], x[0, 1], x[1, 0], x[2, 1] = far, -far * 1.25, far * 0.999999, float("nan")
                return x.to(dev)

            with torch.no_grad():
                for K in (8, 5):
                    phi = (torch.randn(*shape, 3 * K - 1, generator=g, dtype=torch.float64) * 1.2).to(dt).to(dev)
                    w, h, d = unpack(phi, [(K,), (K,), (K - 1,)])
                    x = inputs(2.5, 7.0)
                    y, ladj = ops.rqs_forward(x, w, h, d)
                    _, red = ops.rqs_forward(x, w, h, d, reduce=True)
                    ys, ls = ops.rqs_forward(x, w.contiguous(), h.contiguous(), d.contiguous())
                    put(f"rqs/K{K}/{sh}", y=y, ladj=ladj, ladj_reduced=red, y_strided=ys, ladj_strided=ls, inv=ops.rqs_inverse(x, w, h, d))
                    if K == 8:
                        hor, ver, der = (t.to(dev) for t in O.rqs_knots(w.cpu(), h.cpu(), d.cpu()))
                        yk, lk, kk = ops.rqs_from_knots(x, hor, ver, der)
                        xk, _, ki = ops.rqs_from_knots(x, hor, ver, der, inverse=True)
                        put(f"rqs_knots/K{K}/{sh}", y=yk, ladj=lk, k=kk, inv=xk, k_inv=ki)
                shift, scale = (torch.randn(*shape, generator=g, dtype=torch.float64).to(dt).to(dev) for _ in range(2))
                x = inputs(2.0, float("inf"))
                y, ladj = ops.affine_forward(x, shift, scale)
                put(f"affine/{sh}", y=y, ladj=ladj, inv=ops.affine_inverse(x, shift, scale))
                for P, L1 in ((3, 5), (2, 3)):
                    a = torch.randn(*shape, P, L1, generator=g, dtype=torch.float64).to(dt).to(dev)
                    c = torch.randn(*shape, generator=g, dtype=torch.float64).to(dt).to(dev)
                    x = inputs(4.0, 12.0)
                    for cc, name in ((None, "plain"), (c, "shifted")):
                        y, ladj = ops.sos_forward(x, a, cc)
                        put(f"sos/{P}x{L1}/{name}/{sh}", y=y, ladj=ladj, inv=ops.sos_inverse(x, a, cc))
                for bounded, M in ((False, 16), (True, 17), (False, 7), (True, 4)):
                    theta = torch.randn(*shape, M, generator=g, dtype=torch.float64).to(dt).to(dev)
                    x = inputs(3.0, 5.5)
                    x[3, 0], x[3, 1] = 4.999995, -4.999996  # the linear tails inside the bound
                    y, ladj = ops.bernstein_forward(x, theta, bounded)
                    kind = "static" if M > 8 else "dyn"
                    put(f"bern/{kind}/M{M}b{int(bounded)}/{sh}", theta=theta, x=x, y=y, ladj=ladj, inv=ops.bernstein_inverse(x, theta, bounded))
            if tag == "f32":  # the backward kernels are float32
                for K in (8, 5):
                    phi = (torch.randn(*shape, 3 * K - 1, generator=g) * 1.2).to(dev).requires_grad_()
                    x = inputs(2.5, 7.0).requires_grad_()
                    gy, gl = (torch.randn(*shape, generator=g).to(dev) for _ in range(2))
                    w, h, d = unpack(phi, [(K,), (K,), (K - 1,)])
                    y, ladj = ops.rqs_forward(x, w, h, d, packed=phi)
                    ((y * gy).sum() + (ladj * gl).sum()).backward()
                    put(f"rqs_backward/K{K}/{sh}", gx=x.grad, gphi=phi.grad)
                phi = torch.randn(*shape, 2, generator=g).to(dev).requires_grad_()
                x = inputs(2.0, 30.0).requires_grad_()
                gy, gl = (torch.randn(*shape, generator=g).to(dev) for _ in range(2))
                y, ladj = ops.affine_forward(x, phi[..., 0], phi[..., 1], packed=phi)
                ((y * gy).sum() + (ladj * gl).sum()).backward()
                put(f"affine_backward/{sh}", gx=x.grad, gphi=phi.grad)
    torch.cuda.synchronize()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez_compressed(out, **res)
    print(f"wrote {len(res)} arrays to {out}")


def compare(pa: str, pb: str, root: str) -> int:
    sys.path.insert(0, root)
    import torch

    from oracle import zuko_oracle as O

    A, B = np.load(pa), np.load(pb)
    assert sorted(A.files) == sorted(B.files), "the two dumps hold different arrays"
    bad = 0
    bits = lambda v: v.view(np.uint32 if v.dtype.itemsize == 4 else np.uint64)
    n_bit = n_eq = 0
    for k in sorted(A.files):
        a, b = A[k], B[k]
        leaf = k.rsplit("/", 1)[1]
        if k.startswith("bern/dyn/") and leaf == "y":
            # bitwise outside the linear tails; inside them the unbounded map's y follows the tails' slopes (below), and a NaN may differ in its payload
            x = A[k[: -1] + "x"].astype(np.float64)
            u = (x + 5.0) / 10.0
            free = np.isnan(x) | (((u <= 1e-6) | (u >= 1 - 1e-6)) & ("b0/" in k))
            ok = np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(bits(a)[~free], bits(b)[~free])
            rel = float(np.nanmax(np.abs(a[free].astype(np.float64) - b[free]) / np.abs(a[free]), initial=0.0)) if free.any() else 0.0
            bad += not ok
            print(f"{'ok  ' if ok else 'FAIL'} {k}: bitwise equal outside the unbounded tails; {int((bits(a) != bits(b)).sum())} of {int(free.sum())} tail / NaN elements differ, max relative {rel:.2e}")
        elif k.startswith("bern/dyn/") and leaf in ("ladj", "inv"):
            base = k.rsplit("/", 1)[0]
            bounded = "b1/" in k
            theta, x = torch.from_numpy(A[base + "/theta"]).double(), torch.from_numpy(A[base + "/x"]).double()
            ref = O.bern_forward(theta, x, bounded)[1] if leaf == "ladj" else O.bern_inverse(theta, x, bounded)
            ref = ref.numpy()
            assert np.array_equal(np.isnan(a), np.isnan(b)), f"{k}: NaN pattern differs"
            fin = np.isfinite(ref) & np.isfinite(a) & np.isfinite(b)
            ea, eb = np.abs(a[fin].astype(np.float64) - ref[fin]), np.abs(b[fin].astype(np.float64) - ref[fin])
            ok = eb.max() <= ea.max() and np.median(eb) <= np.median(ea)
            bad += not ok
            print(f"{'ok  ' if ok else 'FAIL'} {k}: |first - f64 oracle| max {ea.max():.3e} median {np.median(ea):.3e}   |second - f64 oracle| max {eb.max():.3e} median {np.median(eb):.3e}")
        elif k.startswith("rqs/K5/") and "ladj" in leaf:
            with np.errstate(invalid="ignore"):
                ok = np.array_equal(np.isnan(a), np.isnan(b)) and bool(np.all((a == b) | np.isnan(a)))
            n_eq += ok
            bad += not ok
            if not ok:
                print(f"FAIL {k}: not == with the same NaN pattern")
        else:
            ok = a.shape == b.shape and np.array_equal(bits(a) if a.dtype.kind == "f" else a, bits(b) if b.dtype.kind == "f" else b)
            n_bit += ok
            bad += not ok
            if not ok:
                print(f"FAIL {k}: not bitwise equal ({int((bits(a) != bits(b)).sum())} of {a.size} elements)")
    print(f"{n_bit} arrays bitwise equal, {n_eq} run-time-count spline ladj arrays == with the same NaN pattern, {bad} failures")
    return 1 if bad else 0


if __name__ == "__main__":
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = sys.argv[1:]
    root = here
    if "--root" in args:
        i = args.index("--root")
        root = os.path.abspath(args[i + 1])
        del args[i : i + 2]
    if args and args[0] == "--compare":
        sys.exit(compare(args[1], args[2], root))
    dump(args[0], root)
