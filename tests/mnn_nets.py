"""Shared by the GPU tests of the monotone-network kernels (csrc/mnn.hip, csrc/umnn.hip): the networks on the device behind the C ABI, seeded
random parameters and inputs, the float32 / float64 CPU references, and the shape tables of the envelope and launch-geometry tests.

MnnNet / UmnnNet take a fixture (the dict of a tests/golden/*.npz written by make_golden_naf.py / make_golden_unaf.py) or a (weights, biases)
pair in the layout of tests/mnn_ref.py: weights[l] [F, out, in], biases[l] [F, out]."""

from __future__ import annotations

import ctypes

import numpy as np
import torch

import mnn_ref
import umnn_ref

# (S, widths) -> the path of the kernels it is there for (zk_mnn_image_floats * 4 = the LDS grant; TM = the tile-count instantiation, 8 when a layer
# is wider than 64).  Small images first: a grant above 64 KiB then grows from an earlier, smaller one of the same kernel function.
ENVELOPE = [
    (17, (80, 112)),       # TM 8: 5 and 7 tiles, the unpaired last tile of the paired loop
    (63, (128, 128)),      # 98 KiB, 16 signal k-steps (the last one padded), 8 x 8 tiles
    (16, (128, 128, 64)),  # 106 KiB, the largest three-layer image
    (1, (16,)),            # the smallest of everything: one k-step with three zero columns, no hidden-to-hidden layer
    (60, (128,)),          # S a multiple of 4 near the top; 8-tile first layer feeding the last layer directly
    (62, (64,)),           # TM 4: padded last k-step
    (5, (128, 16, 128)),   # 8 -> 1 -> 8 tiles
    (4, (16, 16, 16)),     # TM 4: 1 -> 1 -> 1 tiles
    (8, (64, 48)),         # TM 4: odd tile count
]
LARGE_LDS = [(63, (128, 128)), (16, (128, 128, 64))]  # images above 64 KiB: the per-function opt-in
SMALL_TM8 = (17, (80, 112))  # a small image on the kernel functions the large ones run on

# (N, Dsel) -> (rows_per_block, feats_per_block) of the launchers' heuristic (zk_mnn_launch_geometry / zk_umnn_launch_geometry)
GEOMETRY_SHAPES = {
    (1031, 5): (64, 1),
    (16389, 6): (64, 4),    # the last block holds two features: the feature loop leaves through its `break`
    (100037, 8): (128, 4),
    (131149, 8): (256, 4),  # the last row block is partial, its last tile has 13 rows
    (16384, 64): (256, 4),  # the benchmark's proportions
    # few rows, very many columns: fewer than 512 (64-row tile, 4-column group) pairs keep one feature per block, yet the column count alone gives
    # 1024 blocks, so the rows per block stay above 64 (a block then simply finds fewer rows than it could take)
    (129, 600): (128, 1),
    (37, 1030): (256, 1),
}


def shape_id(shape) -> str:
    S, widths = shape
    return f"S{S}-" + "x".join(str(w) for w in widths)


def geometry(N: int, Dsel: int, family: str = "mnn"):
    """(rows_per_block, feats_per_block) the launcher of `family` ("mnn" | "umnn") picks for an [N, Dsel] call: the library's host-only query."""
    import zuko_amd._C as C

    r, f = ctypes.c_int(-1), ctypes.c_int(-1)
    C.check(getattr(C.lib(), f"zk_{family}_launch_geometry")(N, Dsel, ctypes.byref(r), ctypes.byref(f)), f"zk_{family}_launch_geometry")
    return r.value, f.value


def draw_params(S: int, widths, F: int, seed: int):
    """(weights, biases) in float32 on the CPU: uniform(-1, 1) / sqrt(fan_in) from a seeded numpy generator (the draw of
    tests/test_mnn_host.py: test_weight_image_walked_in_the_kernels_tile_order_reproduces_mnn_ref).  Signed: MnnNet / mnn_ref take |W|."""
    rng = np.random.default_rng(seed)
    dims = [1 + S, *widths, 1]
    W = [torch.from_numpy((rng.uniform(-1, 1, (F, b, a)) / np.sqrt(a)).astype(np.float32)) for a, b in zip(dims[:-1], dims[1:])]
    B = [torch.from_numpy((rng.uniform(-1, 1, (F, b)) / np.sqrt(a)).astype(np.float32)) for a, b in zip(dims[:-1], dims[1:])]
    return W, B


def draw_inputs(N: int, D: int, S: int, seed: int):
    """x uniform in +-9.5 [N, D], signal = 1.5 randn [N, D, S], constant = randn [N, D]: float32 on the CPU."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-9.5, 9.5, (N, D)).astype(np.float32)
    sig = (1.5 * rng.standard_normal((N, D, S))).astype(np.float32)
    cst = rng.standard_normal((N, D)).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(sig), torch.from_numpy(cst)


def double(ts):
    return [t.double() for t in ts]


def sample_rows(N: int, edge: int = 300, per_multiple: int = 96) -> torch.Tensor:
    """About 2048 rows of an N-row batch: the first and last `edge`, and the five rows around `per_multiple` multiples of 64, of 128 and of 256
    spread over the batch (the seams of the row tiles, of the blocks and of a block's last wavefront pass)."""
    rows = set(range(min(edge, N))) | set(range(max(0, N - edge), N))
    for m in (64, 128, 256):
        for k in np.unique(np.linspace(1, max(1, (N - 1) // m), per_multiple).astype(np.int64)):
            rows |= {r for r in range(int(k) * m - 2, int(k) * m + 3) if 0 <= r < N}
    return torch.tensor(sorted(rows), dtype=torch.long)


class MnnNet:
    """Per-feature monotone networks on the device: the weight image built as the product builds it (host index table + zk_gather_f32)."""

    ref = mnn_ref
    signed = False

    def __init__(self, g, dev):
        import zuko_amd._C as C
        from zuko_amd import mnn_plan

        if isinstance(g, dict):
            self.W, self.B = self.ref.params_of(g, device=dev)
        else:
            self.W, self.B = [w.to(device=dev, dtype=torch.float32) for w in g[0]], [b.to(device=dev, dtype=torch.float32) for b in g[1]]
        self.S, self.widths, self.F = self.W[0].shape[2] - 1, tuple(w.shape[1] for w in self.W[:-1]), self.W[0].shape[0]
        self.L = mnn_plan.layout(self.S, self.widths)
        idx = torch.from_numpy(mnn_plan.index_table(self.S, self.widths, self.F).reshape(-1)).to(dev)
        flat = torch.cat([(w if self.signed else w.abs()).reshape(-1) for w in self.W] + [b.reshape(-1) for b in self.B])
        self.image = torch.empty(idx.numel(), dtype=torch.float32, device=dev)
        C.check(C.lib().zk_gather_f32(flat.data_ptr(), None, idx.data_ptr(), idx.numel(), self.image.data_ptr(), C.stream()), "zk_gather_f32")
        torch.cuda.synchronize()

    def _args(self, x, sig, out, feat, **extra):
        import zuko_amd._C as C

        N, D = x.shape
        w = list(self.widths) + [0, 0]
        assert x.stride(1) == 1 and sig.stride(1) == 1 and sig.shape == (N, D * self.S)
        return C.args("zk_mnn_args_v1", S=self.S, n_hidden=len(self.widths), width0=w[0], width1=w[1], width2=w[2], n_features=self.F, image_floats=self.L.total, N=N, Dsel=D,
                      ldx=x.stride(0), ld_signal=sig.stride(0), ldy=D, x=x.data_ptr(), signal=sig.data_ptr(), image=self.image.data_ptr(),
                      feat=None if feat is None else feat.data_ptr(), y=out.data_ptr(), **extra)

    def forward(self, x, sig, feat=None, reduce=False):
        """x [N, D] and sig [N, D * S] (last stride 1, any row stride) -> (y, ladj)."""
        import zuko_amd._C as C

        N, D = x.shape
        y = torch.empty((N, D), dtype=torch.float32, device=x.device)
        ladj = torch.empty((N,) if reduce else (N, D), dtype=torch.float32, device=x.device)
        work = torch.empty((N, D), dtype=torch.float32, device=x.device)
        a = self._args(x, sig, y, feat, ladj=ladj.data_ptr(), work=work.data_ptr(), ladj_reduced=int(reduce))
        C.check(C.lib().zk_mnn_forward(a, C.stream()), "zk_mnn_forward")
        return y, ladj

    def inverse(self, t, sig, feat=None):
        import zuko_amd._C as C

        x = torch.empty(t.shape, dtype=torch.float32, device=t.device)
        C.check(C.lib().zk_mnn_inverse(self._args(t, sig, x, feat, n_bisect=25, bound=10.0), C.stream()), "zk_mnn_inverse")
        return x


class UmnnNet:
    """Per-feature integrand networks on the device: the weight image built as the product builds it (host index table + zk_gather_f32) from the
    SIGNED weights, and the quadrature table."""

    ref = umnn_ref
    signed = True

    def __init__(self, g, dev, n_quad=32):
        MnnNet.__init__(self, g, dev)
        t, w = np.polynomial.legendre.leggauss(n_quad)
        self.n_quad = n_quad
        self.quad = torch.from_numpy(np.concatenate([(t + 1) / 2, w / 2]).astype(np.float32)).to(dev)
        torch.cuda.synchronize()

    def _args(self, x, sig, cst, out, feat, **extra):
        """x [N, D], sig [N, D, S] (last stride 1, any column and row stride), cst [N, D] (any strides) | None."""
        import zuko_amd._C as C

        N, D = x.shape
        w = list(self.widths) + [0, 0]
        assert x.stride(1) == 1 and sig.stride(2) == 1 and sig.shape == (N, D, self.S)
        kw = {} if cst is None else dict(constant=cst.data_ptr(), ld_constant=cst.stride(0), ld_constant_col=cst.stride(1))
        return C.args("zk_umnn_args_v1", S=self.S, n_hidden=len(self.widths), width0=w[0], width1=w[1], width2=w[2], n_features=self.F, image_floats=self.L.total, N=N,
                      Dsel=D, n_quad=self.n_quad, ldx=x.stride(0), ld_signal=sig.stride(0), ld_col=sig.stride(1), ldy=D, x=x.data_ptr(), signal=sig.data_ptr(),
                      image=self.image.data_ptr(), quad=self.quad.data_ptr(), feat=None if feat is None else feat.data_ptr(), y=out.data_ptr(), **kw, **extra)

    def forward(self, x, sig, cst, feat=None, reduce=False):
        import zuko_amd._C as C

        N, D = x.shape
        y = torch.empty((N, D), dtype=torch.float32, device=x.device)
        ladj = torch.empty((N,) if reduce else (N, D), dtype=torch.float32, device=x.device)
        work = torch.empty((N, D), dtype=torch.float32, device=x.device)
        a = self._args(x, sig, cst, y, feat, ladj=ladj.data_ptr(), work=work.data_ptr(), ladj_reduced=int(reduce))
        C.check(C.lib().zk_umnn_forward(a, C.stream()), "zk_umnn_forward")
        return y, ladj

    def inverse(self, t, sig, cst, feat=None):
        import zuko_amd._C as C

        x = torch.empty(t.shape, dtype=torch.float32, device=t.device)
        C.check(C.lib().zk_umnn_inverse(self._args(t, sig, cst, x, feat, n_bisect=25, bound=10.0), C.stream()), "zk_umnn_inverse")
        return x


class Case:
    """One family ("mnn" | "umnn") behind one calling convention, so that a test body serves both: device tensors in, device tensors out; the
    references on the CPU.  x [N, D], sig [N, D, S], cst [N, D] (UMNN only; ignored for MNN)."""

    def __init__(self, family: str, W, B, dev, n_quad: int = 32):
        self.family, self.dev, self.n_quad = family, dev, n_quad
        self.W32, self.B32 = [w.float().cpu() for w in W], [b.float().cpu() for b in B]
        self.W64, self.B64 = double(self.W32), double(self.B32)
        self.net = MnnNet((W, B), dev) if family == "mnn" else UmnnNet((W, B), dev, n_quad)

    def _feat(self, feat):
        return None if feat is None else torch.as_tensor(list(feat), dtype=torch.int32, device=self.dev)

    def forward(self, x, sig, cst, feat=None, reduce=False):
        if self.family == "mnn":
            return self.net.forward(x, sig.flatten(1) if sig.dim() == 3 else sig, self._feat(feat), reduce)
        return self.net.forward(x, sig, cst, self._feat(feat), reduce)

    def inverse(self, t, sig, cst, feat=None):
        if self.family == "mnn":
            return self.net.inverse(t, sig.flatten(1) if sig.dim() == 3 else sig, self._feat(feat))
        return self.net.inverse(t, sig, cst, self._feat(feat))

    def _p(self, dtype):
        return (self.W32, self.B32) if dtype == torch.float32 else (self.W64, self.B64)

    def ref_forward(self, x, sig, cst, dtype, feat=None):
        """(y, ladj) of the CPU reference in `dtype` on CPU inputs."""
        W, B = self._p(dtype)
        feat = None if feat is None else list(feat)
        if self.family == "mnn":
            return mnn_ref.forward(W, B, x.to(dtype), sig.to(dtype), feat)
        return umnn_ref.forward(W, B, x.to(dtype), sig.to(dtype), cst.to(dtype), feat, n=self.n_quad)

    def ref_inverse(self, t, sig, cst, dtype, feat=None):
        W, B = self._p(dtype)
        feat = None if feat is None else list(feat)
        if self.family == "mnn":
            return mnn_ref.inverse(W, B, t.to(dtype), sig.to(dtype), feat)
        return umnn_ref.inverse(W, B, t.to(dtype), sig.to(dtype), cst.to(dtype), feat, n=self.n_quad)
