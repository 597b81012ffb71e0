"""The schedule of the FLOW launch of the two-part fused autoregressive kernel (csrc/fused_ar_half_impl.h: arhf_kernel), checked on the CPU.

A workgroup carries its row tile through the T transforms of a composed flow; the T streams lie back to back, so the four-slot ring of
tests/test_half_ring_schedule.py runs over T * NCHUNK chunks per tile and its look-ahead crosses a transform boundary like a chunk boundary.
static_ar.half_flow_schedule lists the T passes of a tile as events.  The walk runs them over several tiles and asserts

  (a), (b)  of tests/test_half_ring_schedule.py for every image: a slot is refilled only behind a barrier every wavefront reaches behind its last
            read of the slot, and an image is read only behind a barrier behind the vmcnt wait that covers its DMA;
  (c)       the bias image of the NEXT pass (of the next tile's first pass behind the last one) is requested once per pass, behind a barrier of the
            pass in progress — every wavefront has then left the pass before, the last reader of the buffer the request overwrites — and a vmcnt wait
            that covers it, followed by a barrier, stands in front of the next pass's first read;
  (d)       the next tile's rows are requested in a tile's LAST pass only, and the one wait that leaves vector-memory operations in flight leaves
            exactly those rows: in every other pass each wait is vmcnt(0).

Shapes: the cfg2 (50 chunks per pass) and cfg3 (17) conditioners and MAF(16, [128, 128]), whose pass is three chunks — shorter than the ring;
T = 2 and 3 (an odd T changes the bias buffer a tile starts in)."""

import pytest

SHAPES = {
    "cfg2": (("rqs", 64, 0, (256, 256, 256), 8), 50),
    "cfg3": (("affine", 64, 0, (256, 256, 256), 0), 17),
    "maf16": (("affine", 16, 0, (128, 128), 0), 3),
}
_TABLES: dict = {}


def _tables(name: str) -> list:
    if name not in _TABLES:
        from zuko_amd import static_ar

        _TABLES[name] = [static_ar.half_tables(plan, lay.kind, 1)[0] for plan, lay, _ in static_ar._plans_for(*SHAPES[name][0])]
    return _TABLES[name]


def walk(t: dict, T: int, tiles: int, passes=None) -> dict:
    """Runs the flow schedule of tables `t` over `tiles` tiles of one workgroup and asserts (a) - (d); returns counts."""
    from zuko_amd import static_ar

    pro, sched = static_ar.half_flow_schedule(t, T) if passes is None else passes
    assert len(sched) == T
    nr, ch, per, nch, images, nit = t["NR"], t["CH"], t["CH"] // t["WAVES"], t["NCHUNK"], t["IMAGES"], t["NIT"]
    size = lambda g: min(images, (g % nch + 1) * ch) - (g % nch) * ch
    st = dict(issued=0, vm=[], landed=set(), visible=set(), lds=[], requested={}, returned={}, at_barrier=None, last=None, barriers=0,
              bias_state=None, bias_requests=0, buf=0, barriers_in_pass=0)
    owner: dict = {}

    def step(e, p):  # p: passes completed before this one (counted on through the tiles); -1: prologue
        kind = e[0]
        if kind == "issue":
            g = st["issued"]
            slot = g % nr
            if slot in owner:  # (a)
                q = owner[slot]
                assert st["last"] == "barrier", f"chunk {g}: the DMA issue does not stand behind a barrier"
                req, ret = st["at_barrier"]
                assert req.get(q, 0) == size(q), f"chunk {g} -> slot {slot}: chunk {q} in it had {req.get(q, 0)} of {size(q)} images requested at the barrier"
                assert ret.get(q, 0) == size(q), f"chunk {g} -> slot {slot}: {size(q) - ret.get(q, 0)} reads of chunk {q} had not returned at the barrier"
            owner[slot] = g
            st["vm"] += [g] * per
            st["issued"] += 1
        elif kind == "x":
            assert p < 0 or p % T == T - 1, "(d) rows requested in a pass that is not the tile's last"
            st["vm"] += ["x"] * e[1]
        elif kind == "bias":
            assert st["barriers_in_pass"] >= 1, "(c) the bias request does not stand behind a barrier of its own pass"
            assert st["bias_state"] is None, "(c) two bias requests in one pass"
            st["vm"] += ["bias"] * 2  # (up to two pieces per wavefront)
            st["bias_state"] = "requested"
            st["bias_requests"] += 1
        elif kind == "wait":
            n = e[1]
            if n:
                assert st["vm"][len(st["vm"]) - n :] == ["x"] * n, f"(d) a wait leaves {st['vm'][len(st['vm']) - n:]} in flight, not the {n} row loads"
            done, st["vm"] = (st["vm"][: len(st["vm"]) - n], st["vm"][len(st["vm"]) - n :]) if n < len(st["vm"]) else ([], st["vm"])
            st["landed"] |= {g for g in done if isinstance(g, int) and g not in st["vm"]}
            if st["bias_state"] == "requested" and "bias" not in st["vm"]:
                st["bias_state"] = "landed"
            if e[2]:
                for g, _ in st["lds"]:
                    st["returned"][g] = st["returned"].get(g, 0) + 1
                st["lds"] = []
        elif kind == "barrier":
            st["visible"] |= st["landed"]
            if st["bias_state"] == "landed":
                st["bias_state"] = "visible"
            st["at_barrier"] = (dict(st["requested"]), dict(st["returned"]))
            st["barriers"] += 1
            st["barriers_in_pass"] += 1
        elif kind == "read":
            g = p * nch + e[1] // ch
            assert owner.get(g % nr) == g, f"pass {p} image {e[1]}: slot {g % nr} holds chunk {owner.get(g % nr)}, not {g}"
            assert g in st["visible"], f"pass {p} image {e[1]}: chunk {g} is read before a barrier behind the vmcnt wait that covers its DMA"  # (b)
            st["lds"].append((g, e[1]))
            st["requested"][g] = st["requested"].get(g, 0) + 1
        elif kind == "settle":
            n = e[1]
            done, st["lds"] = (st["lds"][: len(st["lds"]) - n], st["lds"][len(st["lds"]) - n :]) if n < len(st["lds"]) else ([], st["lds"])
            for g, _ in done:
                st["returned"][g] = st["returned"].get(g, 0) + 1
        else:
            raise AssertionError(e)
        st["last"] = kind

    for e in pro:
        step(e, -1)
    p = 0
    for tile in range(tiles):
        for k in range(T):
            ev = sched[k]
            assert [e[1] for e in ev if e[0] == "read"] == list(range(images)), "a pass reads every image of its transform's stream once, in stream order"
            assert sum(1 for e in ev if e[0] == "x") == int(k == T - 1), "(d) rows are requested once, in the last pass"
            if p > 0:
                assert st["bias_state"] == "visible", f"(c) pass {p} starts while its bias image is {st['bias_state']}"
            st["bias_state"], st["barriers_in_pass"] = None, 0
            for e in ev:
                step(e, p)
            assert not st["lds"], "a pass ends with every weight read returned"
            p += 1
            assert st["issued"] == p * nch + nr - 1, "a pass requests as many chunks as it reads"
    assert st["bias_requests"] == tiles * T
    return st


@pytest.mark.parametrize("T", [2, 3])
@pytest.mark.parametrize("name", list(SHAPES))
def test_flow_schedule_keeps_slots_visibility_and_bias(name, T):
    for t in _tables(name):
        assert (t["NCHUNK"], t["NR"]) == (SHAPES[name][1], 4)
        st = walk(t, T, tiles=5)  # (5 T NCHUNK chunks: every slot phase and both bias buffers at a tile's start)
        assert st["barriers"] == 1 + 5 * T * t["NCHUNK"], "one barrier per chunk"


def test_the_walk_catches_a_bias_request_behind_the_last_barrier(monkeypatch):
    """Requested behind the pass's LAST barrier the image would be published by a barrier of the next pass, behind its first bias reads: (c) fails."""
    from zuko_amd import static_ar

    t = _tables("cfg2")[0]
    monkeypatch.setattr(static_ar, "half_flow_bias_chunk", lambda _t: _t["NCHUNK"] - 1)
    with pytest.raises(AssertionError, match=r"\(c\) pass 1 starts while its bias image is requested"):
        walk(t, 2, tiles=2)


def test_the_walk_catches_rows_left_in_flight_by_a_pass_that_requested_none():
    """A pass that is not the tile's last but waits vmcnt(NIT) at the rows' barrier would leave DMA pieces in flight: (d) fails."""
    from zuko_amd import static_ar

    t = _tables("cfg2")[0]
    pro, sched = static_ar.half_flow_schedule(t, 2)
    last = sched[1]
    wrong = [e for e in last if e[0] != "x"]  # the last pass's waits without its row request
    with pytest.raises(AssertionError, match=r"\(d\)"):
        walk(t, 2, tiles=2, passes=(pro, [wrong, last]))
