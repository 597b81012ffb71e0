"""Every output tensor of the small-network kernels (NAF csrc/mnn*.hip, UNAF csrc/umnn*.hip, CNF csrc/cnf*.hip) through the C ABI, for a comparison
bit by bit between two builds of the library (ZUKO_AMD_LIB chooses the one a run loads).

    ZUKO_AMD_LIB=<library A> python scripts/small_net_outputs.py --out DIR_A
    ZUKO_AMD_LIB=<library B> python scripts/small_net_outputs.py --out DIR_B
    python scripts/small_net_outputs.py --compare DIR_A DIR_B

One process per library.  The cases are the smallest that reach every instantiation of the nine kernel templates and both forms of every helper the
three families share (profiles/small_net_frame/README.md); networks, fixtures and calling conventions are the tests' own (tests/mnn_nets.py,
tests/golden, the BwdNet / _Case / _Stepper helpers of the GPU tests).  --compare applies torch.equal on the int32 views of the saved tensors and
fails on any difference, any missing tensor and any NaN."""

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

HIDDEN_TM4 = [(16,), (32, 48), (64, 64, 64)]
HIDDEN_TM8 = [(128,), (16, 80, 128)]


def forward_inverse(out, dev):
    """NAF and UNAF forward and inverse: both tile-count instantiations, one to three layers, S with one, five and sixteen k-steps, a partial row
    tile and four row tiles; one shape of the launch-geometry table that puts four features into a block."""
    from mnn_nets import GEOMETRY_SHAPES, Case, draw_inputs, draw_params

    def run(tag, case, x, sig, cst):
        y, ladj = case.forward(x, sig, cst)
        out[f"{tag}/y"], out[f"{tag}/ladj"] = y, ladj
        out[f"{tag}/ladj_rows"] = case.forward(x, sig, cst, reduce=True)[1]
        out[f"{tag}/inverse"] = case.inverse(x, sig, cst)

    for family in ("mnn", "umnn"):
        for widths in HIDDEN_TM4 + HIDDEN_TM8:
            for S in (1, 17, 63):
                case = Case(family, *draw_params(S, widths, 3, seed=5), dev, n_quad=7)
                for N in (13, 200):
                    x, sig, cst = (t.to(dev) for t in draw_inputs(N, 3, S, seed=6))
                    run(f"{family}/{'x'.join(map(str, widths))}/S{S}/N{N}", case, x, sig, cst)
        (N, D), (_, feats) = next((k, v) for k, v in GEOMETRY_SHAPES.items() if v[1] == 4)
        assert feats == 4
        case = Case(family, *draw_params(2, (16,), D, seed=7), dev, n_quad=3)
        x, sig, cst = (t.to(dev) for t in draw_inputs(N, D, 2, seed=8))
        run(f"{family}/geometry/N{N}xD{D}", case, x, sig, cst)


def monotone_adjoints(out, dev):
    """NAF and UNAF adjoint: one to three layers x one, two and four signal tiles, four chunks (the last with 8 rows), with and without parameter
    gradients, gl per column and reduced; UNAF with an even and an odd number of quadrature nodes."""
    import test_gpu_mnn_adjoint as naf
    import test_gpu_umnn_adjoint as unaf
    from mnn_nets import draw_inputs, draw_params

    N, F = 200, 3
    for widths in HIDDEN_TM4:
        for S in (5, 20, 40):
            x, sig, _ = draw_inputs(N, F, S, seed=31)
            gy, gl = naf.upstream(N, F, dev, seed=32)
            nets = [("mnn", naf.BwdNet(*draw_params(S, widths, F, seed=30), dev), sig.reshape(N, -1))]
            nets += [(f"umnn/q{nq}", unaf.BwdNet(*draw_params(S, widths, F, seed=30), dev, nq), sig) for nq in (2, 5)]
            for name, net, s in nets:
                tag = f"{name}_bwd/{'x'.join(map(str, widths))}/S{S}"
                for gl_name, g in (("gl_cols", gl), ("gl_rows", gl[:, 0].contiguous())):
                    for want in ((True, True, True), (True, True, False)):
                        gx, gs, gp = net.backward(x.to(dev), s.to(dev), gy, g, want=want)
                        k = f"{tag}/{gl_name}/{'params' if want[2] else 'inputs'}"
                        out[k + "/gx"], out[k + "/gsignal"] = gx, gs
                        if gp is not None:
                            out[k + "/gparams"] = gp


def cnf_steps(out, dev):
    """CNF step: the fixtures of both tile-count instantiations, with the trace (n_tangents = F) and without."""
    import test_gpu_cnf as t
    from conftest import T, golden

    for name in t.KERNEL_CASES:
        F, C = t.CASES[name][:2]
        g = golden(name + ".npz")
        step = t._Stepper(name, dev)
        x = T(g["x"]).float().to(dev)
        pre = step.pre(None if C == 0 else T(g["c"]).float().to(dev))
        t0, dt = float(g["fwd_att32"][0][0]), float(g["fwd_att32"][0][1])
        for traced in (True, False):
            l = torch.linspace(-1.0, 1.0, x.shape[0], device=dev) if traced else None
            y, ln, rows, err = step(x, l, pre, t0, dt)
            k = f"cnf/{name}/{'trace' if traced else 'value'}"
            out[k + "/y"], out[k + "/err"], out[k + "/err_rows"] = y, err, rows
            if traced:
                out[k + "/l_next"] = ln


def cnf_adjoints(out, dev):
    """CNF adjoint: every shape of the test's table at four chunks, with and without al, with and without parameter gradients, and a second launch
    into the first one's gpre and gparams."""
    import test_gpu_cnf_adjoint as t
    from zuko_amd import ops

    N = 200
    for key in t.SHAPES:
        k = t._Case(key, dev)
        gen = torch.Generator().manual_seed(40 + k.F)
        x, ax, al = torch.randn(N, k.F, generator=gen), torch.randn(N, k.F, generator=gen), torch.randn(N, generator=gen)
        c = None if k.C == 0 else torch.randn(N, k.C, generator=gen)
        for with_l in (True, False):
            tag = f"cnf_adj/{key}/{'al' if with_l else 'value'}"
            first = k.run(x, ax, al if with_l else None, c)
            out[tag + "/ax_next"], out[tag + "/gpre"], out[tag + "/gparams"] = (v.clone() for v in first)
            second = k.run(x * 0.5, first[0].cpu(), al if with_l else None, c, t=k.t - k.dt, dt=k.dt * 0.75, gpre=first[1], gparams=first[2])
            out[tag + "/twice/ax_next"], out[tag + "/twice/gpre"], out[tag + "/twice/gparams"] = second
            # no parameter gradients: the launch stops behind the row loop
            ax_next, gpre = torch.full((N, k.F), float("nan"), device=dev), torch.zeros(N, k.hidden[0], device=dev)
            work = torch.full((ops.cnf_adjoint_workspace(k.img, N),), float("nan"), device=dev)
            ops.cnf_adjoint_step(k.img, x.to(dev), ax.to(dev), al.to(dev) if with_l else None, k.pre(c), k.t, k.dt, t.cnf_ref.TRACE_SCALE, ax_next, gpre, None, work)
            torch.cuda.synchronize()
            out[tag + "/inputs/ax_next"], out[tag + "/inputs/gpre"] = ax_next, gpre


def save(path):
    dev = torch.device("cuda:0")
    out = {}
    for part in (forward_inverse, monotone_adjoints, cnf_steps, cnf_adjoints):
        part(out, dev)
        torch.cuda.synchronize()
    os.makedirs(path, exist_ok=True)
    torch.save({k: v.detach().cpu() for k, v in out.items()}, os.path.join(path, "outputs.pt"))
    print(f"{len(out)} tensors from {os.environ.get('ZUKO_AMD_LIB', 'the library of this tree')} -> {path}")


def compare(a, b):
    A, B = (torch.load(os.path.join(d, "outputs.pt")) for d in (a, b))
    bad = [k for k in sorted(set(A) | set(B)) if k not in A or k not in B or A[k].shape != B[k].shape or not torch.equal(A[k].view(torch.int32), B[k].view(torch.int32))]
    nan = [k for k in sorted(set(A) | set(B)) for s in (A, B) if k in s and bool(torch.isnan(s[k]).any())]
    for k in bad:
        print("DIFFERS", k)
    for k in nan:
        print("NaN", k)
    print(f"{len(A)} / {len(B)} tensors, {len(bad)} differ, {len(nan)} hold a NaN")
    return 1 if bad or nan or not A else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", metavar="DIR")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ns = ap.parse_args()
    if bool(ns.out) == bool(ns.compare):
        ap.error("one of --out and --compare")
    sys.exit(compare(*ns.compare) if ns.compare else save(ns.out))
