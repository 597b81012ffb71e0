"""Case table of the incremental inverse kernel (zk_ar_inverse_incremental, csrc/inc_inverse.hip; plan: zuko_amd/incremental.py), shared by
tests/test_inc_envelope_host.py (every entry gets the plan recorded here; the table covers what its docstring claims) and
tests/test_gpu_inc_envelope.py (the kernel against the reference's loop on every entry).

A case is a two-transform flow (ascending order, then descending — or two random orders with `randperm`) of one kind:

    maf (affine)  nsf8 / nsf4 / nsf16 (rational-quadratic splines)  sospf  bpf      — uni kinds 0, 1, 2, 3, 5, 6 of the kernel

EXPECT records, for either autoregressive layer of the flow, what `build_inc_plan` gives on the masks the library's constructors build:

    (n_groups, slots of the first group, nit = 16-wide input tiles, max n_static, max n_dynamic first-layer tiles of a group, n_chunks, HALF n_chunks)

A change of the planner (or of the mask construction) shows up as a difference from these tuples.  Weights: default initialisation under
`seed_of(case)`; the seed also fixes the orders of the `randperm` cases."""

from __future__ import annotations

import zlib
from dataclasses import dataclass, field

import numpy as np
import torch

KINDS = ("maf", "nsf8", "nsf4", "nsf16", "sospf", "bpf")
UNI_KIND = {"maf": 0, "nsf8": 1, "nsf4": 2, "nsf16": 3, "sospf": 5, "bpf": 6}
BINS = {"nsf8": 8, "nsf4": 4, "nsf16": 16}
HALF_KINDS = ("maf", "nsf8", "nsf4", "nsf16")  # the polynomial maps have no HALF instantiation
BISECTION = ("sospf", "bpf")


@dataclass(frozen=True)
class Case:
    kind: str
    D: int
    C: int
    hidden: tuple
    randperm: bool = False
    passes: int | None = None
    note: str = field(default="", compare=False)

    @property
    def name(self) -> str:
        h = "x".join(str(w) for w in self.hidden) if len(set(self.hidden)) > 1 else f"{self.hidden[0]}^{len(self.hidden)}"
        return f"{self.kind}-D{self.D}-C{self.C}-h{h}" + ("-randperm" if self.randperm else "") + (f"-passes{self.passes}" if self.passes else "")

    @property
    def nh(self) -> int:
        return len(self.hidden)


# every instantiation: six kinds x one, two, three hidden layers, at three shapes (D, C, width)
SHAPES = ((6, 3, 24), (13, 2, 52), (10, 0, 40))
INSTANTIATIONS = [Case(k, D, C, (w,) * nh) for k in KINDS for nh in (1, 2, 3) for (D, C, w) in SHAPES]

# plan edges
EDGES = [
    Case("maf", 2, 0, (16,), note="one group of two slots"),
    Case("maf", 2, 3, (16, 16), note="one group of two slots, context"),
    Case("nsf8", 3, 0, (16,), note="one group of three slots"),
    Case("maf", 5, 2, (24, 32), note="first group of two slots"),
    Case("maf", 7, 2, (32,), note="first group of three slots"),
    Case("maf", 17, 0, (68, 68), note="two input tiles, two dynamic tiles, first group of three"),
    Case("nsf8", 21, 0, (84,), note="two static and two dynamic tiles"),
    Case("maf", 33, 0, (132, 132), note="nine groups, three input tiles"),
    Case("maf", 67, 0, (256, 256), note="17 groups, five input tiles, four static tiles, padded last group"),
    Case("maf", 68, 0, (272,), note="MAX_FEATURES and the widest hidden layer (17 x 16)"),
    Case("maf", 65, 0, (256,) * 3, note="17 groups, three hidden layers"),
    Case("nsf8", 64, 0, (256,) * 3, randperm=True, note="four static AND four dynamic tiles in one group"),
    Case("nsf4", 20, 5, (80, 80), randperm=True, note="context shares an input tile with features"),
    Case("nsf4", 6, 2, (32, 32), passes=2, note="no dynamic tile"),
    Case("maf", 8, 4, (32, 32), passes=2, note="no dynamic tile, one chunk"),
    Case("maf", 16, 64, (64, 64), note="five input tiles: four whole context tiles"),
    Case("maf", 8, 60, (32,), note="five input tiles, one chunk"),
    Case("nsf8", 12, 40, (48, 48), note="context across three tiles"),
    Case("nsf16", 32, 0, (128,), note="12 last-layer tiles per group"),
    Case("bpf", 64, 0, (256,) * 3, note="5 last-layer tiles at 17 groups"),
]

CASES = INSTANTIATIONS + EDGES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# name -> per layer (n_groups, first, nit, max ns, max nd, n_chunks, HALF n_chunks)
EXPECT: dict = {
    "maf-D6-C3-h24^1": ((2, 4, 1, 0, 1, 1, 1), (2, 4, 1, 0, 1, 1, 1)),
    "maf-D13-C2-h52^1": ((4, 4, 1, 1, 1, 2, 2), (4, 4, 1, 1, 1, 2, 2)),
    "maf-D10-C0-h40^1": ((3, 4, 1, 0, 1, 2, 2), (3, 4, 1, 0, 1, 2, 2)),
    "maf-D6-C3-h24^2": ((2, 4, 1, 0, 1, 1, 1), (2, 4, 1, 0, 1, 1, 1)),
    "maf-D13-C2-h52^2": ((4, 4, 1, 1, 1, 3, 3), (4, 4, 1, 1, 1, 3, 3)),
    "maf-D10-C0-h40^2": ((3, 3, 1, 0, 1, 2, 2), (3, 3, 1, 0, 1, 2, 2)),
    "maf-D6-C3-h24^3": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "maf-D13-C2-h52^3": ((4, 4, 1, 1, 1, 3, 3), (4, 4, 1, 1, 1, 3, 3)),
    "maf-D10-C0-h40^3": ((3, 3, 1, 0, 1, 2, 2), (3, 3, 1, 0, 1, 2, 2)),
    "nsf8-D6-C3-h24^1": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "nsf8-D13-C2-h52^1": ((4, 4, 1, 1, 1, 4, 5), (4, 4, 1, 1, 1, 4, 5)),
    "nsf8-D10-C0-h40^1": ((3, 4, 1, 0, 1, 3, 3), (3, 4, 1, 0, 1, 3, 3)),
    "nsf8-D6-C3-h24^2": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "nsf8-D13-C2-h52^2": ((4, 4, 1, 1, 1, 5, 5), (4, 4, 1, 1, 1, 5, 5)),
    "nsf8-D10-C0-h40^2": ((3, 3, 1, 0, 1, 3, 4), (3, 3, 1, 0, 1, 3, 4)),
    "nsf8-D6-C3-h24^3": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "nsf8-D13-C2-h52^3": ((4, 4, 1, 1, 1, 5, 6), (4, 4, 1, 1, 1, 5, 6)),
    "nsf8-D10-C0-h40^3": ((3, 3, 1, 0, 1, 3, 4), (3, 3, 1, 0, 1, 3, 4)),
    "nsf4-D6-C3-h24^1": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "nsf4-D13-C2-h52^1": ((4, 4, 1, 1, 1, 3, 3), (4, 4, 1, 1, 1, 3, 3)),
    "nsf4-D10-C0-h40^1": ((3, 4, 1, 0, 1, 2, 2), (3, 4, 1, 0, 1, 2, 2)),
    "nsf4-D6-C3-h24^2": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "nsf4-D13-C2-h52^2": ((4, 4, 1, 1, 1, 3, 4), (4, 4, 1, 1, 1, 3, 4)),
    "nsf4-D10-C0-h40^2": ((3, 3, 1, 0, 1, 2, 3), (3, 3, 1, 0, 1, 2, 3)),
    "nsf4-D6-C3-h24^3": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "nsf4-D13-C2-h52^3": ((4, 4, 1, 1, 1, 4, 4), (4, 4, 1, 1, 1, 4, 4)),
    "nsf4-D10-C0-h40^3": ((3, 3, 1, 0, 1, 3, 3), (3, 3, 1, 0, 1, 3, 3)),
    "nsf16-D6-C3-h24^1": ((2, 4, 1, 0, 1, 3, 3), (2, 4, 1, 0, 1, 3, 3)),
    "nsf16-D13-C2-h52^1": ((4, 4, 1, 1, 1, 7, 8), (4, 4, 1, 1, 1, 7, 8)),
    "nsf16-D10-C0-h40^1": ((3, 4, 1, 0, 1, 4, 5), (3, 4, 1, 0, 1, 4, 5)),
    "nsf16-D6-C3-h24^2": ((2, 4, 1, 0, 1, 3, 3), (2, 4, 1, 0, 1, 3, 3)),
    "nsf16-D13-C2-h52^2": ((4, 4, 1, 1, 1, 7, 8), (4, 4, 1, 1, 1, 7, 8)),
    "nsf16-D10-C0-h40^2": ((3, 3, 1, 0, 1, 5, 5), (3, 3, 1, 0, 1, 5, 5)),
    "nsf16-D6-C3-h24^3": ((2, 4, 1, 0, 1, 3, 3), (2, 4, 1, 0, 1, 3, 3)),
    "nsf16-D13-C2-h52^3": ((4, 4, 1, 1, 1, 8, 9), (4, 4, 1, 1, 1, 8, 9)),
    "nsf16-D10-C0-h40^3": ((3, 3, 1, 0, 1, 5, 6), (3, 3, 1, 0, 1, 5, 6)),
    "sospf-D6-C3-h24^1": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "sospf-D13-C2-h52^1": ((4, 4, 1, 1, 1, 3, 4), (4, 4, 1, 1, 1, 3, 4)),
    "sospf-D10-C0-h40^1": ((3, 4, 1, 0, 1, 2, 3), (3, 4, 1, 0, 1, 2, 3)),
    "sospf-D6-C3-h24^2": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "sospf-D13-C2-h52^2": ((4, 4, 1, 1, 1, 4, 4), (4, 4, 1, 1, 1, 4, 4)),
    "sospf-D10-C0-h40^2": ((3, 3, 1, 0, 1, 3, 3), (3, 3, 1, 0, 1, 3, 3)),
    "sospf-D6-C3-h24^3": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "sospf-D13-C2-h52^3": ((4, 4, 1, 1, 1, 4, 5), (4, 4, 1, 1, 1, 4, 5)),
    "sospf-D10-C0-h40^3": ((3, 3, 1, 0, 1, 3, 3), (3, 3, 1, 0, 1, 3, 3)),
    "bpf-D6-C3-h24^1": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "bpf-D13-C2-h52^1": ((4, 4, 1, 1, 1, 4, 4), (4, 4, 1, 1, 1, 4, 4)),
    "bpf-D10-C0-h40^1": ((3, 4, 1, 0, 1, 3, 3), (3, 4, 1, 0, 1, 3, 3)),
    "bpf-D6-C3-h24^2": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "bpf-D13-C2-h52^2": ((4, 4, 1, 1, 1, 4, 5), (4, 4, 1, 1, 1, 4, 5)),
    "bpf-D10-C0-h40^2": ((3, 3, 1, 0, 1, 3, 3), (3, 3, 1, 0, 1, 3, 3)),
    "bpf-D6-C3-h24^3": ((2, 4, 1, 0, 1, 2, 2), (2, 4, 1, 0, 1, 2, 2)),
    "bpf-D13-C2-h52^3": ((4, 4, 1, 1, 1, 5, 5), (4, 4, 1, 1, 1, 5, 5)),
    "bpf-D10-C0-h40^3": ((3, 3, 1, 0, 1, 3, 4), (3, 3, 1, 0, 1, 3, 4)),
    "maf-D2-C0-h16^1": ((1, 2, 1, 0, 1, 1, 1), (1, 2, 1, 0, 1, 1, 1)),
    "maf-D2-C3-h16^2": ((1, 2, 1, 0, 1, 1, 1), (1, 2, 1, 0, 1, 1, 1)),
    "nsf8-D3-C0-h16^1": ((1, 3, 1, 0, 1, 1, 1), (1, 3, 1, 0, 1, 1, 1)),
    "maf-D5-C2-h24x32": ((2, 2, 1, 0, 1, 1, 1), (2, 2, 1, 0, 1, 1, 1)),
    "maf-D7-C2-h32^1": ((2, 3, 1, 0, 1, 1, 1), (2, 3, 1, 0, 1, 1, 1)),
    "maf-D17-C0-h68^2": ((5, 3, 2, 0, 1, 3, 4), (5, 3, 2, 1, 2, 3, 4)),
    "nsf8-D21-C0-h84^1": ((6, 4, 2, 2, 1, 8, 8), (6, 4, 2, 2, 2, 8, 8)),
    "maf-D33-C0-h132^2": ((9, 3, 3, 1, 2, 7, 8), (9, 3, 3, 2, 2, 7, 8)),
    "maf-D67-C0-h256^2": ((17, 4, 5, 4, 1, 19, 20), (17, 4, 5, 4, 2, 19, 20)),
    "maf-D68-C0-h272^1": ((17, 4, 5, 4, 1, 13, 13), (17, 4, 5, 4, 1, 13, 13)),
    "maf-D65-C0-h256^3": ((17, 4, 5, 3, 1, 25, 26), (17, 4, 5, 4, 2, 25, 26)),
    "nsf8-D64-C0-h256^3-randperm": ((17, 3, 4, 4, 4, 57, 60), (17, 3, 4, 4, 4, 57, 60)),
    "nsf4-D20-C5-h80^2-randperm": ((5, 4, 2, 1, 2, 5, 5), (5, 4, 2, 1, 2, 5, 5)),
    "nsf4-D6-C2-h32^2-passes2": ((2, 3, 1, 1, 0, 2, 2), (2, 3, 1, 1, 0, 2, 2)),
    "maf-D8-C4-h32^2-passes2": ((2, 4, 1, 1, 0, 1, 1), (2, 4, 1, 1, 0, 1, 1)),
    "maf-D16-C64-h64^2": ((4, 4, 5, 4, 1, 3, 3), (4, 4, 5, 4, 1, 3, 3)),
    "maf-D8-C60-h32^1": ((2, 4, 5, 4, 1, 1, 1), (2, 4, 5, 4, 1, 1, 1)),
    "nsf8-D12-C40-h48^2": ((3, 4, 4, 3, 1, 3, 4), (3, 4, 4, 3, 1, 3, 4)),
    "nsf16-D32-C0-h128^1": ((8, 4, 2, 1, 1, 21, 23), (8, 4, 2, 1, 1, 21, 23)),
    "bpf-D64-C0-h256^3": ((17, 3, 4, 4, 2, 51, 53), (17, 3, 4, 4, 2, 51, 53)),
}


def seed_of(case: Case) -> int:
    return zlib.crc32(case.name.encode()) & 0x7FFFFFFF


def layout_of(kind: str):
    """The kernel's one-feature-per-lane layout of a kind's univariate map (what MaskedAutoregressiveTransform.incremental_state derives)."""
    from zuko_amd import fused

    if kind == "maf":
        return fused.UniLayout(0, 2, 1, 1)
    if kind in BINS:
        b = BINS[kind]
        return fused.UniLayout(UNI_KIND[kind], 3 * b - 1, 1, (3 * b - 1 + 3) // 4, b)
    return fused.UniLayout(5, 16, 1, 4) if kind == "sospf" else fused.UniLayout(6, 17, 1, 5)


def oracle_uni(kind: str):
    from oracle import zuko_oracle as O

    if kind == "maf":
        return O.UNI_AFFINE
    if kind in BINS:
        return O.uni_rqs(BINS[kind])
    return O.uni_sos() if kind == "sospf" else O.uni_bpf()


def linears(layer) -> list:
    return [m for m in layer.hyper if hasattr(m, "mask")]


def build(case: Case, activation=None):
    """(flow, its MaskedAutoregressiveTransform layers, the oracle's ARLayer of each) on the CPU, weights at default initialisation under seed_of(case).
    The ARLayers hold CLONES of the parameters: they keep describing the initial weights after an in-place update of the flow."""
    import zuko_amd.flows as F
    from oracle import zuko_oracle as O
    from zuko_amd.flows.autoregressive import MaskedAutoregressiveTransform

    kw = dict(features=case.D, context=case.C, transforms=2, hidden_features=list(case.hidden), randperm=case.randperm)
    if case.passes is not None:
        kw["passes"] = case.passes
    if activation is not None:
        kw["activation"] = activation
    if case.kind in BINS:
        kw["bins"] = BINS[case.kind]
    ctor = {"maf": F.MAF, "sospf": F.SOSPF, "bpf": F.BPF}.get(case.kind, F.NSF)
    torch.manual_seed(seed_of(case))
    flow = ctor(**kw)
    layers = [t for t in flow.transform.transforms if isinstance(t, MaskedAutoregressiveTransform)]
    assert len(layers) == 2
    return flow, layers, [oracle_layer(case, t) for t in layers]


def oracle_layer(case: Case, layer):
    """The oracle's description of `layer` at its CURRENT parameters (cloned, on the CPU)."""
    from oracle import zuko_oracle as O

    lins = linears(layer)
    cp = lambda t: t.detach().cpu().clone()
    return O.ARLayer(oracle_uni(case.kind), [cp(l.weight) for l in lins], [cp(l.bias) for l in lins], [cp(l.mask) for l in lins], layer.passes, case.D)


def plan_of(case: Case, layer):
    from zuko_amd import incremental as inc

    return inc.build_inc_plan([l.mask for l in linears(layer)], case.D, layer.order.cpu().numpy(), layout_of(case.kind))


def summary(plan, half_chunks: int) -> tuple:
    """The tuple EXPECT records."""
    return (plan.n_groups, int((plan.featmap[:4] >= 0).sum()), plan.nit, int(plan.prog[:, 0].max()), int(plan.prog[:, 1].max()), plan.n_chunks, half_chunks)


def direct(case: Case) -> bool:
    """Entries the library's product path does not hand to this kernel although their plan exists: the 4- and 16-bin splines at a feature count that is
    no multiple of four, which `_fusable_layout` declines on behalf of the FORWARD kernel's epilogue (fused.layout_supports).  The incremental kernel
    has no such limit; the tests build its state from the plan with the arguments `incremental_state` would pass, so that the three shapes of
    INSTANTIATIONS serve every kind."""
    return case.kind in ("nsf4", "nsf16") and case.D % 4 != 0


def state_of(case: Case, layer, device):
    """IncAR of `layer` on `device`: the library's own (`incremental_state`) or, for direct(case), one built from the plan and kept on the layer."""
    from zuko_amd import incremental as inc
    from zuko_amd.nn import _act_code

    if not direct(case):
        return layer.incremental_state(device)
    held = layer.__dict__.setdefault("_test_inc_states", {})
    if str(device) not in held:
        assert layer.incremental_state(device) is None and layer._fusable_layout() is None
        K, bound, slope = layer._rqs_spec()
        assert K == BINS[case.kind]
        codes = {_act_code(m) for m in layer.hyper if not hasattr(m, "mask")}
        assert len(codes) == 1 and None not in codes
        held[str(device)] = inc.IncAR(plan_of(case, layer), linears(layer), device, codes.pop(), bound, slope)
    return held[str(device)]


def expects_incremental(layer) -> bool:
    """Whether `layer` (a MaskedAutoregressiveTransform) is served by the incremental kernel: the conditions of its `incremental_state`, evaluated on
    the host — what the tests of the product path state about the inverse they exercise."""
    return layer.incremental_state(torch.device("cpu")) is not None


def draw(case: Case, N: int, salt: int = 0):
    """y [N, D] and context [N, C] (or None), standard normal, seeded per case."""
    g = torch.Generator().manual_seed(seed_of(case) + 1 + salt)
    y = torch.randn(N, case.D, generator=g)
    c = torch.randn(N, case.C, generator=g) if case.C else None
    return y, c
