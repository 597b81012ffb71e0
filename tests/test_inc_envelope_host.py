"""CPU: the case table of the incremental inverse kernel (tests/inc_cases.py).

  1. every entry is served by the incremental kernel — `incremental_state` is not None for either autoregressive layer of its flow — with exactly
     the plan the table records, so that tests/test_gpu_inc_envelope.py can never test a fall-back and a change of the planner is a diff of the table
     (inc_cases.direct names the entries whose plan exists but which the library declines for its forward kernel's sake: asserted as exactly that);
  2. the table covers what it is there for: all 30 (kind, hidden layers, HALF) instantiations and the plan edges named in COVERAGE below;
  3. the numpy walk of the kernel's stream and tables (tests/plan_emulators.py: simulate_inc) in float64 equals the oracle's `passes`-sweep inverse
     and the forward log-determinant at the solution on every edge entry, with the f32 stream and (kinds 0-3) with the HALF stream, at the bars of
     tests/test_fused_plan.py: test_incremental_inverse_plan_simulation_matches_oracle."""

import numpy as np
import pytest
import torch

import inc_cases as T
from oracle import zuko_oracle as O
from plan_emulators import simulate_inc

CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def built():
    made = {}

    def get(case):
        if case.name not in made:
            made[case.name] = T.build(case)
        return made[case.name]

    return get


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_every_entry_gets_the_recorded_plan(built, case):
    from zuko_amd import incremental as inc

    flow, layers, _ = built(case)
    got = []
    for layer in layers:
        if T.direct(case):  # declined by the library on behalf of the FORWARD kernel's layout, nothing else: the GPU file builds the state from the plan
            from zuko_amd import fused

            assert layer.incremental_state(CPU) is None and layer._rqs_spec() is not None and case.D % 4 != 0 and not fused.layout_supports(T.layout_of(case.kind), case.D)
        else:
            assert layer.incremental_state(CPU) is not None, f"{case.name}: incremental_state is None — the partial sweeps would serve this layer"
        st = T.state_of(case, layer, CPU)
        plan = T.plan_of(case, layer)
        assert plan is not None
        assert plan.layout.kind == st.plan.layout.kind == T.UNI_KIND[case.kind] and plan.n_hidden == case.nh and plan.features == case.D and plan.din == case.D + case.C
        assert np.array_equal(plan.gather, st.plan.gather) and np.array_equal(plan.prog, st.plan.prog) and np.array_equal(plan.featmap, st.plan.featmap)
        assert plan.n_blocks == plan.n_chunks * inc.CHUNK and st.half.n_images == st.half.n_chunks * inc.CHUNK
        got.append(T.summary(plan, st.half.n_chunks))
    assert case.name in T.EXPECT, f"{case.name}: no recorded plan; measured {tuple(got)}"
    assert tuple(got) == tuple(T.EXPECT[case.name]), f"{case.name}: the planner gives {tuple(got)}"


def test_the_table_covers_the_envelope():
    """COVERAGE, in code: what the GPU file relies on the table for."""
    assert set(T.EXPECT) == set(T.BY_NAME)
    inst = {(c.kind, c.nh, half) for c in T.CASES for half in ((False, True) if c.kind in T.HALF_KINDS else (False,))}
    assert inst == {(k, nh, h) for k in T.KINDS for nh in (1, 2, 3) for h in ((False, True) if k in T.HALF_KINDS else (False,))} and len(inst) == 30
    # every kind x depth appears at each of the three small shapes
    assert {(c.kind, c.nh, c.D, c.C) for c in T.INSTANTIATIONS} == {(k, nh, D, C) for k in T.KINDS for nh in (1, 2, 3) for (D, C, _) in T.SHAPES}
    plans = [p for name in T.BY_NAME for p in T.EXPECT[name]]
    G, first, nit, ns, nd, nch, hch = (set(v) for v in zip(*plans))
    assert {2, 3, 4} <= first
    assert {1, 17} <= G
    assert any(p[3] == 4 and p[4] == 4 for p in plans), "four static and four dynamic first-layer tiles in one plan"
    assert 0 in nd
    assert 5 in nit
    assert {1, 2, 3} <= nch and max(nch) > 3
    assert {1, 2, 3, 5} <= {p[5] for c in T.INSTANTIATIONS if c.kind in ("maf", "nsf8") for p in T.EXPECT[c.name]}, "the small f32 cases of the multi-tile test"
    # the product path serves every kind (direct(case) entries are the 4- / 16-bin splines at D % 4 != 0 only), in either form
    assert {c.kind for c in T.CASES if not T.direct(c)} == set(T.KINDS) and all(c.kind in ("nsf4", "nsf16") and c.D % 4 for c in T.CASES if T.direct(c))
    assert any(c.D % 4 for c in T.CASES)
    assert any(c.C and (c.D % 16) and c.D // 16 == (c.D + c.C - 1) // 16 for c in T.CASES), "context inside a feature tile"
    assert any(c.C >= 64 and c.D % 16 == 0 for c in T.CASES), "four whole context tiles"


def _walk(case, layer, ol, half):
    from zuko_amd import fused, incremental as inc

    lins = T.linears(layer)
    plan = T.plan_of(case, layer)
    W = [l.weight.detach().double().numpy() for l in lins]
    B = [l.bias.detach().double().numpy() for l in lins]
    Mk = [l.mask.numpy() for l in lins]
    g = torch.Generator().manual_seed(T.seed_of(case) + 3)
    y = torch.randn(30, case.D, generator=g, dtype=torch.float64)
    c = torch.randn(30, case.C, generator=g, dtype=torch.float64) if case.C else None
    uni = T.oracle_uni(case.kind)
    o64 = O.ARLayer(uni, [torch.from_numpy(w) for w in W], [torch.from_numpy(b) for b in B], [torch.from_numpy(m) for m in Mk], layer.passes, case.D)
    xo = O.ar_inverse(o64, y, c)
    _, lo = O.ar_forward(o64, xo, c)

    def inv_fn(phi, yv):
        ph, yy = torch.from_numpy(phi)[:, None, :], torch.from_numpy(yv)[:, None]
        x = O.univariate_inverse(uni, ph, yy)
        _, l = O.univariate_forward(uni, ph, x)
        return x[:, 0].numpy(), l[:, 0].numpy()

    relu = lambda v: np.maximum(v, 0)
    cn = None if c is None else c.numpy()
    if not half:
        xs, ls = simulate_inc(plan, W, B, Mk, y.numpy(), cn, relu, inv_fn)
        ex, el = np.abs(xs - xo.numpy()).max(), np.abs(ls - lo.numpy()).max()
        if case.kind in T.BISECTION:  # (both walks stop at the same 2^-24 bracket unless a comparison sits within rounding of the target)
            assert ex < 1e-5 and el < 1e-3, (ex, el)
        else:
            assert ex < 1e-12 and el < 1e-11, (ex, el)
        return
    hs = inc.half_stream(plan, [l.mask for l in lins])
    wexp = [0] + [e for _, e in fused.half_scales(lins)][1:]
    xh, lh = simulate_inc(plan, W, B, Mk, y.numpy(), cn, relu, inv_fn, half=hs, wexp=wexp)
    ex, el = np.abs(xh - xo.numpy()).max(), np.abs(lh - lo.numpy()).max()
    assert ex < 1e-6 * max(1.0, np.abs(xo.numpy()).max()) and el < 1e-5, (ex, el)


# entries whose walk is too slow for both layers of the flow: the plan assertions above hold for both
ONE_LAYER = {"bpf-D64-C0-h256^3": "64 features x 24 bisection steps of the degree-16 Bernstein map per layer (4.5 s); the descending layer of this shape is "
                                  "walked by test_fused_plan.py: test_incremental_inverse_plan_simulation_matches_oracle"}


@pytest.mark.parametrize("case,half", [(c, h) for c in T.EDGES for h in ((False, True) if c.kind in T.HALF_KINDS else (False,))],
                         ids=lambda v: v.name if isinstance(v, T.Case) else ("HALF" if v else "f32"))
def test_numpy_walk_of_every_edge_plan_matches_the_oracle(built, case, half):
    """Both layers of the flow (either order), 30 rows, float64; the HALF stream for kinds 0-3 (the polynomial maps have none)."""
    flow, layers, ols = built(case)
    todo = list(zip(layers, ols))
    if case.name in ONE_LAYER:
        todo = todo[:1]
    for layer, ol in todo:
        _walk(case, layer, ol, half)
