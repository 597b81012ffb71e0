"""Host side of the monotone-network adjoint (zk_mnn_backward): the closed-form reverse sweep the kernel implements against float64 autograd,
the backward image and the gradient table walked as the kernel's matrix instructions walk them, the argument block, the refusals that need no
device, and the geometry / workspace queries.  No GPU."""

import ctypes

import numpy as np
import pytest
import torch

import mnn_adjoint_ref as ref
from mnn_nets import draw_inputs, draw_params

SHAPES = [(1, (16,)), (3, (32,)), (7, (16, 48, 64)), (16, (64, 64))]
TABLE_SHAPES = SHAPES + [(63, (64, 64, 64))]
EINVAL = 1


def _w3(widths):
    return list(widths) + [0] * (3 - len(widths))


@pytest.mark.parametrize("subset", [False, True], ids=["all", "feat-subset"])
@pytest.mark.parametrize("S,widths", SHAPES)
def test_closed_form_sweep_equals_float64_autograd(S, widths, subset):
    F, N = 4, 23
    W, B = draw_params(S, widths, F, seed=3 + S)
    feat = [2, 0, 3] if subset else None
    D = len(feat) if subset else F
    x, sig, _ = draw_inputs(N, D, S, seed=5 + S)
    gen = torch.Generator().manual_seed(7 + S)
    gy, gl = torch.randn(N, D, generator=gen, dtype=torch.float64), torch.randn(N, D, generator=gen, dtype=torch.float64)
    for upstream in ((gy, gl), (gy, None), (None, gl[:, 0].contiguous())):
        a = ref.autograd(W, B, x, sig, *upstream, feat=feat, dtype=torch.float64)
        c = ref.closed_form(W, B, x, sig, *upstream, feat=feat, dtype=torch.float64)
        assert ref.all_finite(a)
        for name, ta, tc in [("gx", a["gx"], c["gx"]), ("gsignal", a["gsignal"], c["gsignal"]), *[(f"gW{l}", u, v) for l, (u, v) in enumerate(zip(a["gW"], c["gW"]))],
                             *[(f"gB{l}", u, v) for l, (u, v) in enumerate(zip(a["gB"], c["gB"]))]]:
            d, scale = float((ta - tc).abs().max()), max(1.0, float(ta.abs().max()))
            assert d <= 1e-12 * scale, f"{name}: |d| {d:.3e} at scale {scale:.3e}"
        if subset:
            for g in a["gW"] + a["gB"]:
                assert not bool(g[1].any()), "the feature feat does not select"


@pytest.mark.parametrize("S,widths", TABLE_SHAPES)
def test_gradient_table_is_a_bijection_and_the_forward_tables_are_untouched(S, widths):
    from zuko_amd import mnn_plan

    F = 3
    L, B = mnn_plan.layout(S, widths), mnn_plan.layout_backward(S, widths)
    table = mnn_plan.grad_table(S, widths, F)
    total = mnn_plan.flat_offsets(S, widths, F)[2]
    assert table.shape == (F, B.g_total) and table.dtype == np.int32
    used = table[table >= 0]
    assert used.size == total and np.array_equal(np.sort(used), np.arange(total)), "every flat parameter is named exactly once"
    idx_b = mnn_plan.index_table_backward(S, widths, F)
    assert idx_b.shape == (F, B.total) and np.array_equal(idx_b[:, : L.total], mnn_plan.index_table(S, widths, F)), "the backward image begins with the forward image"
    # the feature a partial's float belongs to is the row of the table it stands in
    dims = [1 + S, *widths, 1]
    w_off, b_off, _ = mnn_plan.flat_offsets(S, widths, F)
    owner = np.empty(total, dtype=np.int64)
    for l, (a, b) in enumerate(zip(dims[:-1], dims[1:])):
        owner[w_off[l] : w_off[l] + F * a * b] = np.repeat(np.arange(F), a * b)
        owner[b_off[l] : b_off[l] + F * b] = np.repeat(np.arange(F), b)
    for f in range(F):
        assert np.all(owner[table[f][table[f] >= 0]] == f)


def _mfma(A, Bm):
    """v_mfma_f32_16x16x4_f32 on lane vectors: A[lane] = A(m = lane & 15, k = lane >> 4), B[lane] = B(k = lane >> 4, n = lane & 15); returns D[m, n]."""
    lane = np.arange(64)
    Am, Bk = np.zeros((16, 4)), np.zeros((4, 16))
    Am[lane & 15, lane >> 4] = A
    Bk[lane >> 4, lane & 15] = Bm
    return Am @ Bk


def _frag(M):
    """The accumulator layout of a [16 units, 16 elements] tile: lane (j, q) holds units 4 q + r of element j -> [64, 4]."""
    lane = np.arange(64)
    return np.stack([M[4 * (lane >> 4) + r, lane & 15] for r in range(4)], axis=1)


@pytest.mark.parametrize("S,widths", [(7, (16, 48, 64)), (3, (32,)), (16, (64, 64))])
def test_backward_image_and_partial_walked_as_the_kernel_walks_them(S, widths):
    """An emulation of the three kinds of product of csrc/mnn_backward.hip on the tables alone, in float64: A_l^T pb through the transposed tiles (the
    gradient in accumulator layout is the B operand as it stands), A_0[:, 1:]^T pb_0, and the outer products over the wave's 16 elements whose
    accumulators land in the partial where grad_table says."""
    from zuko_amd import mnn_plan

    F, f = 2, 1
    rng = np.random.default_rng(S)
    W, Bs = draw_params(S, widths, F, seed=11)
    flat = torch.cat([w.abs().reshape(-1) for w in W] + [b.reshape(-1) for b in Bs]).double().numpy()
    L, B = mnn_plan.layout(S, widths), mnn_plan.layout_backward(S, widths)
    idx = mnn_plan.index_table_backward(S, widths, F)[f]
    img = np.where(idx >= 0, flat[np.maximum(idx, 0)], 0.0)
    table = mnn_plan.grad_table(S, widths, F)[f]
    A = [w[f].abs().double().numpy() for w in W]
    lane = np.arange(64)
    j, q = lane & 15, lane >> 4
    for l in range(1, len(widths)):
        To, Ti = L.T[l], L.T[l - 1]
        pb = rng.standard_normal((widths[l], 16))  # [out units, elements]
        want = A[l].T @ pb
        for i in range(Ti):
            acc = np.zeros((16, 16))
            for o in range(To):
                tile = img[B.o_wT[l] + (i * To + o) * 256 :][:256].reshape(64, 4)
                fr = _frag(pb[16 * o : 16 * o + 16])
                for r in range(4):
                    acc += _mfma(tile[:, r], fr[:, r])
            assert np.allclose(acc, want[16 * i : 16 * i + 16], rtol=1e-12, atol=1e-12), (l, i)
        # outer product: operands are the fragments transposed through M[element][unit]; k-step s of either is M.flat[64 s + lane]
        v = rng.standard_normal((widths[l - 1], 16))
        G = np.zeros(B.g_total)
        for o in range(To):
            for i in range(Ti):
                Mp, Mv = pb[16 * o : 16 * o + 16].T.reshape(-1), v[16 * i : 16 * i + 16].T.reshape(-1)  # [element][unit]
                acc = np.zeros((16, 16))
                for s in range(4):
                    acc += _mfma(Mp[64 * s + lane], Mv[64 * s + lane])
                G[B.g_w[l] + (o * Ti + i) * 256 :][:256] = _frag(acc).reshape(-1)
        got = np.zeros(flat.size)
        sel = table >= 0
        got[table[sel]] = G[sel]
        w_off = mnn_plan.flat_offsets(S, widths, F)[0]
        n = widths[l] * widths[l - 1]
        assert np.allclose(got[w_off[l] + f * n :][:n].reshape(widths[l], widths[l - 1]), pb @ v.T, rtol=1e-12, atol=1e-12), l
    # the signal's share of the first layer
    pb0 = rng.standard_normal((widths[0], 16))
    want = A[0][:, 1:].T @ pb0
    sig = rng.standard_normal((16, S))  # [element, signal feature]
    G = np.zeros(B.g_total)
    for i in range(B.ts):
        acc = np.zeros((16, 16))
        for o in range(L.T[0]):
            tile = img[B.o_w0sT + (i * L.T[0] + o) * 256 :][:256].reshape(64, 4)
            fr = _frag(pb0[16 * o : 16 * o + 16])
            for r in range(4):
                acc += _mfma(tile[:, r], fr[:, r])
        rows = min(16, S - 16 * i)
        assert np.allclose(acc[:rows], want[16 * i : 16 * i + rows], rtol=1e-12, atol=1e-12) and not acc[rows:].any(), i
        for o in range(L.T[0]):
            Mp = pb0[16 * o : 16 * o + 16].T.reshape(-1)
            acc = np.zeros((16, 16))
            for s in range(4):
                b = np.where(16 * i + j < S, sig[4 * s + q, np.minimum(16 * i + j, S - 1)], 0.0)
                acc += _mfma(Mp[64 * s + lane], b)
            G[B.g_w0s + (o * B.ts + i) * 256 :][:256] = _frag(acc).reshape(-1)
    got = np.zeros(flat.size)
    sel = table >= 0
    got[table[sel]] = G[sel]
    n = widths[0] * (1 + S)
    assert np.allclose(got[f * n :][:n].reshape(widths[0], 1 + S)[:, 1:], pb0 @ sig, rtol=1e-12, atol=1e-12)


def test_layout_and_supported_predicate_agree_with_the_library():
    import zuko_amd._C as C
    from zuko_amd import mnn_plan, ops

    lib = C.lib()
    shapes = TABLE_SHAPES + [(63, (64,)), (16, (64, 48)), (4, (16, 16, 16)), (16, (128, 128)), (16, (80,)), (16, (64, 128, 64)), (16, (30, 30)), (64, (64,)), (0, (16,)),
                             (16, (128, 128, 128))]
    for S, widths in shapes:
        a, b = ctypes.c_int(-1), ctypes.c_int(-1)
        rc = lib.zk_mnn_backward_floats(S, len(widths), *_w3(widths), ctypes.byref(a), ctypes.byref(b))
        B = mnn_plan.layout_backward(S, widths)
        assert (rc == 0) == (B is not None) == ops.mnn_backward_supported(S, widths), (S, widths)
        if B is not None:
            assert (a.value, b.value) == (B.total, B.g_total) and ops.mnn_supported(S, widths)
            assert 4 * (max(B.total, B.g_total) + mnn_plan.BWD_SCRATCH) <= mnn_plan.LDS_MAX
        else:
            assert rc == EINVAL
    # every shape of the forward kernel whose widths are all <= 64 is served; nothing wider is
    for S in (1, 16, 63):
        for widths in [(16,), (64,), (64, 64), (16, 48, 64), (64, 64, 64)]:
            assert ops.mnn_backward_supported(S, widths)
        for widths in [(80,), (64, 128), (128, 64, 64)]:
            assert ops.mnn_supported(S, widths) and not ops.mnn_backward_supported(S, widths)
    assert lib.zk_mnn_backward_floats(16, 2, 64, 64, 0, None, None) == EINVAL


def test_geometry_and_workspace_queries_are_consistent_and_deterministic():
    import zuko_amd._C as C
    from zuko_amd import mnn_plan

    lib = C.lib()

    def geometry(N, D):
        r, c = ctypes.c_int(-1), ctypes.c_int(-1)
        assert lib.zk_mnn_backward_geometry(N, D, ctypes.byref(r), ctypes.byref(c)) == 0
        return r.value, c.value

    def workspace(N, D, S, widths):
        v = ctypes.c_int64(-1)
        assert lib.zk_mnn_backward_workspace_floats(N, D, S, len(widths), *_w3(widths), ctypes.byref(v)) == 0
        return v.value

    for N, D in [(1, 1), (15, 3), (64, 3), (65, 3), (193, 3), (257, 5), (1 << 14, 64), (1 << 16, 64), (1 << 16, 1), (100037, 8), (37, 1030)]:
        rows, chunks = geometry(N, D)
        assert (rows, chunks) == geometry(N, D), "a pure function of the two sizes"
        assert rows % 64 == 0 and rows >= 64 and chunks == -(-N // rows) and (chunks - 1) * rows < N
        assert chunks * D <= max(512, D), "the grid stays near 512 blocks"
        for S, widths in [(16, (64, 64)), (63, (64, 64, 64))]:
            assert workspace(N, D, S, widths) == chunks * D * mnn_plan.layout_backward(S, widths).g_total
    # modest at the benchmark's largest batch: 2^16 rows x 64 features
    assert workspace(1 << 16, 64, 16, (64, 64)) * 4 <= 16 << 20 and workspace(1 << 16, 64, 63, (64, 64, 64)) * 4 <= 32 << 20
    assert geometry(193, 3) == (64, 4)
    assert workspace(0, 5, 16, (64, 64)) == 0
    r, c, v = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
    for N, D in [(0, 3), (-1, 3), (5, 0), (5, 65536)]:
        assert lib.zk_mnn_backward_geometry(N, D, ctypes.byref(r), ctypes.byref(c)) == EINVAL
    assert lib.zk_mnn_backward_geometry(5, 3, None, ctypes.byref(c)) == EINVAL
    assert lib.zk_mnn_backward_workspace_floats(5, 3, 16, 1, 128, 0, 0, ctypes.byref(v)) == EINVAL
    assert lib.zk_mnn_backward_workspace_floats(5, 3, 16, 2, 64, 64, 0, None) == EINVAL


def test_entry_point_and_block_exist_and_bad_blocks_are_refused_without_a_device():
    import zuko_amd._C as C
    from zuko_amd import mnn_plan

    lib = C.lib()
    text = open(C._HEADER).read()
    for sym in ("zk_mnn_backward", "zk_mnn_backward_floats", "zk_mnn_backward_geometry", "zk_mnn_backward_workspace_floats"):
        assert sym in text and sym in C.SIGNATURES and hasattr(ctypes.CDLL(C.LIB_PATH), sym)
    assert "zk_mnn_bwd_args_v1" in C.STRUCTS and "zk_mnn_bwd_args_v1" in text
    fields = [f for f, _ in C.STRUCTS["zk_mnn_bwd_args_v1"]._fields_]
    for name in ("gy", "gl", "gl_reduced", "gx", "gsignal", "ld_gx", "ld_gsignal", "gparams", "work", "feat"):
        assert name in fields
    Bl = mnn_plan.layout_backward(16, (64, 64))

    def block(**kw):
        base = dict(S=16, n_hidden=2, width0=64, width1=64, width2=0, n_features=5, image_floats=Bl.total, grad_floats=Bl.g_total, N=0, Dsel=5, ldx=5, ld_signal=80,
                    ld_gx=5, ld_gsignal=80, flat_total=100, flat_weights=60)
        base.update(kw)
        return C.args("zk_mnn_bwd_args_v1", **base)

    fn = lib.zk_mnn_backward
    assert fn(block(), None) == 0  # (a well-formed block over zero rows with every pointer null: accepted, nothing to launch)
    for delta in (-8, 8):
        bad = block()
        bad.struct_size += delta
        assert fn(bad, None) == EINVAL
    bad = block()
    bad.version = 2
    assert fn(bad, None) == EINVAL and fn(None, None) == EINVAL
    for kw in (dict(width0=30, width1=30), dict(width0=128), dict(width1=80), dict(width1=0), dict(n_hidden=4), dict(n_hidden=0), dict(S=0), dict(S=64), dict(image_floats=1),
               dict(image_floats=mnn_plan.layout(16, (64, 64)).total), dict(grad_floats=1), dict(ld_signal=79), dict(ldx=0), dict(Dsel=0), dict(Dsel=65536, ld_signal=1 << 22),
               dict(N=-1), dict(n_features=0)):
        assert fn(block(**kw), None) == EINVAL, kw
    assert fn(block(N=4), None) == EINVAL  # (rows but no pointers)
    one = ctypes.c_void_p(16)  # (never dereferenced: the block is refused first)
    assert fn(block(gx=one, ld_gx=4), None) == EINVAL and fn(block(gsignal=one, ld_gsignal=79), None) == EINVAL
    assert fn(block(N=4, x=one, signal=one, image=one, gparams=one), None) == EINVAL  # (parameter gradients without params / table / workspace)
    assert fn(block(N=4, x=one, signal=one, image=one, gparams=one, params=one, grad_table=one, work=one, flat_total=0), None) == EINVAL
    assert fn(block(N=4, x=one, signal=one, image=one, gparams=one, params=one, grad_table=one, work=one, flat_weights=101), None) == EINVAL


def test_switch_and_feature_check_exist():
    from zuko_amd import ops

    assert isinstance(ops.MNN_ADJOINT, bool) and ops.MNN_KERNEL is True
    assert ops.mnn_backward_supported(16, (64, 64)) and not ops.mnn_backward_supported(16, (128, 128)) and not ops.mnn_backward_supported(16, (30, 30))
    assert issubclass(ops.MnnForwardFn, torch.autograd.Function)
