"""GPU: zk_ar_inverse_incremental (csrc/inc_inverse.hip) over the envelope its plan admits, driven through IncAR (zuko_amd/incremental.py) so that
the kernel under test is unambiguous; the cases are tests/inc_cases.py (tests/test_inc_envelope_host.py shows every one has the recorded plan).

  1. all 30 instantiations ({affine, RQS-8 / 4 / 16} x {1, 2, 3 hidden layers} x {f32, HALF pulls}, {SOS, Bernstein} x {1, 2, 3}) at three small
     shapes, contiguous and through NaN-padded row strides of y and of the context;
  2. the plan edges of the table, either order of the flow;
  3. row tails N = 1 .. 65, into a slice of a NaN-filled buffer;
  4. batches whose workgroups take two and four tiles (the weight ring restarts on its stream with look-ahead loads in flight), for plans of 1, 2,
     3, 5, 6 and 57 / 60 chunks: the reference, and every row bit for bit against launches that give each workgroup one tile;
  5. every activation code;
  6. non-finite y and context;
  7. refresh after an in-place weight update, after a switch of the matmul precision, after zuko_amd.invalidate.

Reference: the reference project's loop in plain torch on the CPU, in float32 and float64 — x = 0, `passes` sweeps of the masked conditioner
(O.mlp_forward) and O.univariate_inverse; log|dy/dx| from O.univariate_forward at the KERNEL's x, summed over the features.  Inputs: standard
normal y and context, weights at default initialisation (inc_cases.seed_of).  Bar: parity.assert_parity with its default constant on x and (kinds
0-3) on ladj.  The bisection maps (SOS, Bernstein) are compared on x only — no caller asks those kernels for ladj.  Two bisections can end one
bracket apart when a comparison sits within rounding of the target; a comparison that cannot meet assert_parity for that reason would be named in
ABS_BAR and held to 5e-5 absolute against the float64 reference instead (the bar of test_polynomial_flows_invert_in_one_incremental_launch).  None
needed it: ABS_BAR is empty, every SOS / Bernstein comparison of this file meets assert_parity."""

import pytest
import torch

import inc_cases as T
from oracle import zuko_oracle as O
from parity import REPORT, assert_parity, to_f64

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
N_SMALL, N_WIDE = 193, 130  # three full 64-row tiles and one row; 130 for D >= 64 (the cost of the CPU reference)
ACTIVATIONS = {2: ("ELU", torch.nn.functional.elu), 3: ("Tanh", torch.tanh), 4: ("SiLU", torch.nn.functional.silu), 5: ("GELU", torch.nn.functional.gelu),
               6: ("Sigmoid", torch.sigmoid), 7: ("LeakyReLU", torch.nn.functional.leaky_relu)}

# comparisons of the bisection maps held to 5e-5 absolute against the float64 reference (see the module docstring): substrings of their names
ABS_BAR: tuple = ()


@pytest.fixture(scope="module", autouse=True)
def _environment():
    """No run-time compile from any call of this module; the HALF stream allowed (it is used when the matmul precision is "f16x2")."""
    import zuko_amd

    mp = pytest.MonkeyPatch()
    mp.setenv("ZUKO_AMD_JIT", "0")
    mp.setenv("ZUKO_AMD_INVERSE_HALF", "1")
    keep = zuko_amd.matmul_precision()
    yield
    zuko_amd.set_matmul_precision(keep)
    mp.undo()


class Net:
    """A case's flow on the device with the oracle's description of either layer."""

    def __init__(self, case, dev, act_code=1):
        self.case, self.dev, self.act_code = case, dev, act_code
        ctor = None if act_code == 1 else getattr(torch.nn, ACTIVATIONS[act_code][0])
        self.act = torch.relu if act_code == 1 else ACTIVATIONS[act_code][1]
        flow, self.layers, self.ol = T.build(case, activation=ctor)
        self.flow = flow.to(dev)

    def state(self, li, half):
        """IncAR of layer li, refreshed, in f32 or HALF form."""
        import zuko_amd

        zuko_amd.set_matmul_precision("f16x2" if half else "bf16x3")
        st = T.state_of(self.case, self.layers[li], self.dev)
        assert st is not None and st.act == self.act_code and st.plan.layout.kind == T.UNI_KIND[self.case.kind]
        st.refresh(T.linears(self.layers[li]))
        if half:
            assert st.h_ok, "the weights at default initialisation admit the HALF stream"
        return st

    def run(self, li, y, c, half=False, out=None):
        """(x, ladj or None) of one launch; ladj is asked for exactly where the library asks for it (kinds 0-3)."""
        st = self.state(li, half)
        x, l = st.run(y, c, self.case.kind not in T.BISECTION, out=out)
        return x, l

    def phi(self, li, x, c, ol):
        inp = x if c is None else torch.cat((x, c), dim=-1)
        return O.mlp_forward(inp, ol.weights, ol.biases, ol.masks, act=self.act).unflatten(-1, (-1, ol.uni.total))

    def ref_inverse(self, li, y, c, dtype, ol=None):
        """The reference's loop (zuko/transforms.py:994-1000) in `dtype`; O.ar_inverse itself where the activation is the oracle's (ReLU)."""
        ol = self.ol[li] if ol is None else ol
        ol = to_f64(ol) if dtype == F64 else ol
        y, c = y.cpu().to(dtype), None if c is None else c.cpu().to(dtype)
        if self.act_code == 1:
            return O.ar_inverse(ol, y, c)
        x = torch.zeros_like(y)
        for _ in range(ol.passes):
            x = O.univariate_inverse(ol.uni, self.phi(li, x, c, ol), y)
        return x

    def ref_ladj(self, li, x, c, dtype, ol=None):
        """log|dy/dx| of the forward map at x (the kernel's), summed over the features."""
        ol = self.ol[li] if ol is None else ol
        ol = to_f64(ol) if dtype == F64 else ol
        x, c = x.cpu().to(dtype), None if c is None else c.cpu().to(dtype)
        if self.act_code == 1:
            return O.ar_forward(ol, x, c)[1]
        return O.univariate_forward(ol.uni, self.phi(li, x, c, ol), x)[1].sum(dim=-1)


@pytest.fixture(scope="module")
def net_of(dev):
    made = {}

    def get(case, act_code=1):
        key = (case.name, act_code)
        if key not in made:
            made[key] = Net(case, dev, act_code)
        return made[key]

    return get


def _check_x(case, got, r32, r64, what):
    if case.kind in T.BISECTION and any(s in what for s in ABS_BAR):
        got, r32, r64 = got.detach().cpu(), r32.cpu(), r64.cpu()
        assert torch.equal(torch.isnan(got), torch.isnan(r32)) and torch.equal(torch.isinf(got), torch.isinf(r32)), f"{what}: non-finite pattern differs"
        fin = torch.isfinite(r32)
        d = float((got[fin].double() - r64[fin]).abs().max())
        REPORT.append({"what": what, "n": int(fin.sum()), "abs_bar": 5e-5, "hip_vs_f64": {"max": d}, "ref32_vs_f64": {"max": float((r32[fin].double() - r64[fin]).abs().max())}, "ok": d < 5e-5})
        assert d < 5e-5, f"{what}: {d:.3e} from the float64 reference"
        return
    assert_parity(got, r32, r64, what)


def _compare(net, li, y, c, x, ladj, what, rows=None, refs=None, ol=None):
    """x (and ladj, kinds 0-3) of a launch against the float32 / float64 reference, on `rows` (a LongTensor on the CPU) or on all of them.
    Returns the references of x, for tests that compare several launches with them."""
    sel = (lambda t: t) if rows is None else (lambda t: None if t is None else t.cpu()[rows])
    ys, cs, xs = sel(y), sel(c), sel(x)
    r32, r64 = refs if refs is not None else (net.ref_inverse(li, ys, cs, F32, ol), net.ref_inverse(li, ys, cs, F64, ol))
    _check_x(net.case, xs, r32, r64, f"{what}: x")
    if ladj is not None:
        assert_parity(sel(ladj), net.ref_ladj(li, xs, cs, F32, ol), net.ref_ladj(li, xs, cs, F64, ol), f"{what}: ladj")
    return r32, r64


def _padded(y, c):
    """The same values through NaN-padded row strides (D + 3 and C + 5)."""
    N, D = y.shape
    yp = torch.full((N, D + 3), float("nan"), device=y.device)
    yp[:, :D] = y
    if c is None:
        return yp[:, :D], None
    cp = torch.full((N, c.shape[1] + 5), float("nan"), device=y.device)
    cp[:, : c.shape[1]] = c
    return yp[:, :D], cp[:, : c.shape[1]]


def _to(dev, *ts):
    return tuple(None if t is None else t.to(dev) for t in ts)


def _forms(case):
    return (False, True) if case.kind in T.HALF_KINDS else (False,)


def _tag(case, half, li):
    return f"{case.name} {'HALF' if half else 'f32'} layer {li}"


def _same(a, b):
    return (a is None and b is None) or torch.equal(a, b)


# ---- 1. every instantiation ------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case,half", [(c, h) for c in T.INSTANTIATIONS for h in _forms(c)], ids=lambda v: v.name if isinstance(v, T.Case) else ("HALF" if v else "f32"))
def test_every_instantiation(dev, net_of, case, half):
    net = net_of(case)
    y, c = T.draw(case, N_SMALL)
    yd, cd = _to(dev, y, c)
    for li in (0, 1):
        x, ladj = net.run(li, yd, cd, half)
        _compare(net, li, y, c, x, ladj, f"inc instantiation {_tag(case, half, li)} contiguous")
        yp, cp = _padded(yd, cd)
        assert yp.stride(0) == case.D + 3 and (cp is None or cp.stride(0) == case.C + 5)
        xp, lp = net.run(li, yp, cp, half)
        assert torch.equal(xp, x) and _same(lp, ladj), "row strides of y / context change the result"
        _compare(net, li, y, c, xp, lp, f"inc instantiation {_tag(case, half, li)} strided")


# ---- 2. every plan edge ----------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("case,half", [(c, h) for c in T.EDGES for h in _forms(c)], ids=lambda v: v.name if isinstance(v, T.Case) else ("HALF" if v else "f32"))
def test_every_plan_edge(dev, net_of, case, half):
    net = net_of(case)
    y, c = T.draw(case, N_WIDE if case.D >= 64 else N_SMALL)
    yd, cd = _to(dev, y, c)
    for li in (0, 1):
        x, ladj = net.run(li, yd, cd, half)
        _compare(net, li, y, c, x, ladj, f"inc edge {_tag(case, half, li)} ({case.note})")


# ---- 3. row tails ----------------------------------------------------------------------------------------------------------------------------

TAIL_CASES = [T.BY_NAME["maf-D6-C3-h24^1"], T.BY_NAME["nsf8-D13-C2-h52^2"]]  # one chunk; context, several chunks


@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: c.name)
def test_row_tails(dev, net_of, case):
    """N = 1 .. 65: the reference, the same rows of the N = 193 launch bit for bit, and nothing stored past row N - 1."""
    net = net_of(case)
    y, c = T.draw(case, N_SMALL)
    yd, cd = _to(dev, y, c)
    li = 1
    x_all, l_all = net.run(li, yd, cd)
    refs = _compare(net, li, y, c, x_all, l_all, f"inc tails {case.name} N = {N_SMALL}")
    for N in (1, 15, 16, 17, 63, 64, 65):
        big = torch.full((N + 70, case.D), float("nan"), device=dev)
        lbig = torch.full((N + 70,), float("nan"), device=dev)
        x, ladj = net.run(li, yd[:N], None if cd is None else cd[:N], out=(big[3 : 3 + N], lbig[3 : 3 + N]))
        assert x.data_ptr() == big[3].data_ptr()
        assert bool(torch.isnan(big[:3]).all() and torch.isnan(big[3 + N :]).all() and torch.isnan(lbig[:3]).all() and torch.isnan(lbig[3 + N :]).all()), f"N = {N}: a store outside the N rows"
        assert torch.equal(x, x_all[:N]) and torch.equal(ladj, l_all[:N]), f"N = {N}: differs from the same rows of the N = {N_SMALL} launch"
        _compare(net, li, y[:N], None if c is None else c[:N], x, ladj, f"inc tails {case.name} N = {N}", refs=(refs[0][:N], refs[1][:N]))


# ---- 4. several tiles per workgroup ----------------------------------------------------------------------------------------------------------

GRID_ROWS = 256 * 64  # the launch caps the grid at 256 workgroups of 64 rows
N_TWO, N_FOUR = GRID_ROWS + 65, 3 * GRID_ROWS + 1  # workgroups 0 and 1 take a second tile; workgroup 0 takes a fourth
# plans of 1, 2 (first group of three), 3 and 5 chunks in f32 form, 6 in HALF form, one SOS and one Bernstein case
MULTI = [("maf-D6-C3-h24^1", False, 1), ("maf-D10-C0-h40^2", False, 2), ("maf-D13-C2-h52^2", False, 3), ("nsf8-D13-C2-h52^2", False, 5), ("nsf8-D13-C2-h52^3", True, 6),
         ("sospf-D6-C3-h24^1", False, 2), ("bpf-D6-C3-h24^1", False, 2)]


def _boundary_rows(N):
    """The rows a second, third or fourth tile of a workgroup can get wrong, and their neighbours: the first 64, the 64 before and 128 after every
    multiple of the grid's 16 384 rows, the last 65."""
    r = set(range(64)) | set(range(N - 65, N))
    for k in range(GRID_ROWS, N, GRID_ROWS):
        r |= set(range(k - 64, min(N, k + 128)))
    return torch.tensor(sorted(r))


def _equals_its_slices(net, li, yd, cd, half, x, ladj, step):
    """Bit identity of ALL rows with launches of `step`-row slices of the same input, each one tile per workgroup (rows are independent)."""
    assert step <= GRID_ROWS
    for a in range(0, yd.shape[0], step):
        xs, ls = net.run(li, yd[a : a + step], None if cd is None else cd[a : a + step], half)
        assert torch.equal(xs, x[a : a + step]) and _same(ls, None if ladj is None else ladj[a : a + step]), f"rows {a} .. differ from their own one-tile-per-workgroup launch"


@pytest.mark.parametrize("name,half,n_chunks", MULTI, ids=lambda v: v if isinstance(v, str) else ("HALF" if v is True else "f32" if v is False else f"{v}chunks"))
def test_several_tiles_per_workgroup(dev, net_of, name, half, n_chunks):
    """Both batch sizes: ALL rows bit for bit against launches of 16 384-row slices (one tile per workgroup), and the reference — on every row for the
    affine cases; for the splines and the bisection maps, whose CPU reference over 49 153 rows costs 10 s (RQS) to 100 s (SOS, Bernstein: 25 quadratures
    per element and sweep), on _boundary_rows: about 700 rows that hold every tile workgroup 0 takes and the rows around each restart of the grid.
    One reference over the larger batch: rows are independent, the smaller batch is its first rows."""
    case = T.BY_NAME[name]
    net = net_of(case)
    li = 1
    st = net.state(li, half)
    assert (st.half.n_chunks if half else st.plan.n_chunks) == n_chunks
    y, c = T.draw(case, N_FOUR, salt=7)
    yd, cd = _to(dev, y, c)
    rows = None if case.kind == "maf" else _boundary_rows(N_FOUR)
    pick = (lambda t: t) if rows is None else (lambda t: None if t is None else t[rows])
    r32, r64 = net.ref_inverse(li, pick(y), pick(c), F32), net.ref_inverse(li, pick(y), pick(c), F64)
    for N in (N_TWO, N_FOUR):
        x, ladj = net.run(li, yd[:N], None if cd is None else cd[:N], half)
        _equals_its_slices(net, li, yd[:N], None if cd is None else cd[:N], half, x, ladj, GRID_ROWS)
        what = f"inc multi-tile {_tag(case, half, li)} ({n_chunks} chunks) N = {N}"
        if rows is None:
            _compare(net, li, y[:N], None if c is None else c[:N], x, ladj, what, refs=(r32[:N], r64[:N]))
        else:
            keep = rows < N
            _compare(net, li, y, c, x, ladj, f"{what}, {int(keep.sum())} rows", rows=rows[keep], refs=(r32[keep], r64[keep]))


@pytest.mark.parametrize("half", [False, True], ids=["f32", "HALF"])
def test_several_tiles_per_workgroup_at_the_long_stream(dev, net_of, half):
    """The D = 64 NSF with random orders (57 / 60 chunks, four static and four dynamic first-layer tiles) at 16 384 + 65 rows: the reference on 256
    rows — the first 64, the last 127 of the workgroups' first tiles and the 65 of their second — and bit identity of ALL rows with launches of
    4 096-row slices of the same input, each one tile per workgroup (rows are independent: this holds exactly)."""
    case = T.BY_NAME["nsf8-D64-C0-h256^3-randperm"]
    net = net_of(case)
    N = N_TWO
    y, _ = T.draw(case, N, salt=7)
    yd = y.to(dev)
    rows = torch.cat((torch.arange(0, 64), torch.arange(GRID_ROWS - 127, GRID_ROWS), torch.arange(GRID_ROWS, N)))
    assert rows.numel() == 256
    for li in (0, 1):
        st = net.state(li, half)
        assert (st.half.n_chunks if half else st.plan.n_chunks) == (60 if half else 57)
        x, ladj = net.run(li, yd, None, half)
        _compare(net, li, y, None, x, ladj, f"inc multi-tile {_tag(case, half, li)} N = {N}, 256 rows", rows=rows)
        _equals_its_slices(net, li, yd, None, half, x, ladj, 4096)


# ---- 5. activations --------------------------------------------------------------------------------------------------------------------------

ACT_CASES = [(k, code, False) for k in ("maf", "nsf8") for code in ACTIVATIONS] + [(k, code, True) for k in ("maf", "nsf8") for code in (3, 5)]


@pytest.mark.parametrize("kind,code,half", ACT_CASES, ids=lambda v: v if isinstance(v, str) else ("HALF" if v is True else "f32" if v is False else ACTIVATIONS[v][0]))
def test_activations(dev, net_of, kind, code, half):
    """Codes 2-7 of inc_act; in HALF form Tanh and GELU, whose activations are negative while a pair's scale is taken from absolute values."""
    case = T.BY_NAME[f"{kind}-D13-C2-h52^2"]
    net = net_of(case, code)
    y, c = T.draw(case, N_SMALL)
    yd, cd = _to(dev, y, c)
    for li in (0, 1):
        x, ladj = net.run(li, yd, cd, half)
        _compare(net, li, y, c, x, ladj, f"inc activation {ACTIVATIONS[code][0]} (code {code}) {_tag(case, half, li)}")


# ---- 6. non-finite inputs --------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("kind", ["maf", "nsf8", "sospf", "bpf"])
def test_non_finite_inputs_follow_the_reference(dev, net_of, kind):
    """NaN, +inf and -inf in one feature of y (rows 5, 21, 70) and in one context column (rows 40, 100, 150), the same values in the reference's
    input.  The closed-form maps hand a non-finite value on and the reference's next sweep makes every parameter of the row NaN; its bisection never
    returns a NaN (the bracket closes on an end), so for SOS / Bernstein the reference's rows hold no NaN (Bernstein: x = +-inf where y is, the lower
    end elsewhere) — assert_parity requires the reference's pattern and its values."""
    case = T.BY_NAME[f"{kind}-D13-C2-h52^2"]
    net = net_of(case)
    y, c = T.draw(case, N_SMALL, salt=3)
    nan, inf = float("nan"), float("inf")
    y[5, 4], y[21, 0], y[70, 12] = nan, inf, -inf
    c[40, 1], c[100, 0], c[150, 1] = nan, inf, -inf
    poisoned = [5, 21, 70, 40, 100, 150]
    yd, cd = _to(dev, y, c)
    for li in (0, 1):
        x, ladj = net.run(li, yd, cd)
        r32, _ = _compare(net, li, y, c, x, ladj, f"inc non-finite {_tag(case, False, li)}")
        clean = torch.ones(N_SMALL, dtype=torch.bool)
        clean[poisoned] = False
        assert bool(torch.isfinite(x.cpu()[clean]).all()) and bool(torch.isfinite(r32[clean]).all())
        if kind in ("maf", "nsf8"):
            # all NaN, except that the reference's spline under NaN parameters passes y = -inf through (-inf lies below its first knot, the constant -B)
            through = torch.zeros(len(poisoned), case.D, dtype=torch.bool)
            through[2, 12] = kind == "nsf8"
            assert torch.equal(torch.isnan(r32[poisoned]), ~through) and bool((r32[poisoned][through] == -inf).all())
            assert torch.equal(torch.isnan(x.cpu()[poisoned]), ~through) and bool(torch.isnan(ladj.cpu()[poisoned]).all())
        else:
            assert not bool(torch.isnan(r32[poisoned]).any()), "the reference's bisection returns no NaN"


# ---- 7. refresh ------------------------------------------------------------------------------------------------------------------------------


def test_refresh_follows_the_weights_and_the_precision(dev):
    import zuko_amd

    case = T.BY_NAME["nsf8-D13-C2-h52^2"]
    net = Net(case, dev)  # (its own flow: the weights change)
    li = 1
    layer = net.layers[li]
    y, c = T.draw(case, N_SMALL, salt=5)
    yd, cd = _to(dev, y, c)
    x0, l0 = net.run(li, yd, cd)
    _compare(net, li, y, c, x0, l0, f"inc refresh {case.name}: first call")
    # an in-place update of a hidden layer under no_grad bumps the version: the stream is rebuilt
    lin = T.linears(layer)[1]
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        lin.weight.add_((0.05 * torch.randn(lin.weight.shape, generator=g)).to(dev))
    new = T.oracle_layer(case, layer)
    assert not torch.equal(new.weights[1], net.ol[li].weights[1])
    x1, l1 = net.run(li, yd, cd)
    assert not torch.equal(x1, x0)
    _compare(net, li, y, c, x1, l1, f"inc refresh {case.name}: after weight.add_", ol=new)
    # the precision switched with the f32 stream already built: the next call builds the HALF stream and runs it
    st = layer.incremental_state(dev)
    assert not st.h_ok
    x2, l2 = net.run(li, yd, cd, half=True)
    assert st.h_ok and layer.incremental_state(dev) is st
    _compare(net, li, y, c, x2, l2, f"inc refresh {case.name}: HALF after the f32 stream", ol=new)
    # invalidate drops the state: a new one, the same bits
    zuko_amd.invalidate(net.flow)
    x3, l3 = net.run(li, yd, cd, half=True)
    assert layer.incremental_state(dev) is not st
    assert torch.equal(x3, x2) and torch.equal(l3, l2)


# ---- the product path ------------------------------------------------------------------------------------------------------------------------


def test_the_flow_reaches_the_kernel_for_a_small_conditioner(dev, net_of, monkeypatch):
    """flow(c).transform.inv of a small conditional NSF: one IncAR.run per autoregressive layer, and the result of chaining the layers by hand."""
    import zuko_amd
    from zuko_amd import incremental as inc

    case = T.BY_NAME["nsf8-D13-C2-h52^2"]
    net = net_of(case)
    zuko_amd.set_matmul_precision("bf16x3")
    calls = []
    run = inc.IncAR.run

    def counted(self, *a, **k):
        calls.append(self)
        return run(self, *a, **k)

    monkeypatch.setattr(inc.IncAR, "run", counted)
    y, c = T.draw(case, N_SMALL, salt=9)
    yd, cd = _to(dev, y, c)
    with torch.no_grad():
        x = net.flow(cd).transform.inv(yd)
    assert len(calls) == 2 and calls[0] is net.layers[1].incremental_state(dev) and calls[1] is net.layers[0].incremental_state(dev)
    monkeypatch.undo()
    x1, _ = net.run(1, yd, cd)
    x0, _ = net.run(0, x1, cd)
    assert torch.equal(x, x0)
    r32, r64 = (net.ref_inverse(0, net.ref_inverse(1, y, c, dt), c, dt) for dt in (F32, F64))
    assert_parity(x, r32, r64, f"inc product path {case.name}: transform.inv")
