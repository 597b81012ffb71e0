"""The weight ring of the TWO-PART fused autoregressive kernel (csrc/fused_ar_half_impl.h: ArhRing4 — four slots, a chunk visible one chunk before
it is read — and the three-slot ArhRing that shapes too large for four slots keep), checked on the CPU.

The kernel's pass over a tile is straight-line code generated from the tables of zuko_amd/static_ar.py, the same for every wavefront of the
workgroup; static_ar.half_schedule lists it as events (image reads with their look-ahead, counted LDS waits, vmcnt waits, barriers, DMA issues).
The walk below runs that list over several tiles — chunk g of the stream, counted on through the tiles, lives in slot g mod NR, so the slot phase
changes from tile to tile whenever NR does not divide the chunk count — and asserts for every image

  (a) a slot is refilled only behind a barrier that every wavefront reaches behind its last read of that slot: at the barrier in front of the
      DMA issue every image of the chunk the slot held has been requested AND has returned (a counted LDS wait has covered it);
  (b) an image is read only behind a barrier that itself stands behind the vmcnt wait covering the image's DMA in every wavefront.

(The model's vector-memory queue holds the DMA pieces and the next tile's row loads only.  Whatever else a wavefront has in flight — the running
log-derivative's load, a tile's stores — is younger than some piece and makes a counted wait cover MORE, never less.)

Chunk counts of the shapes (all prebuilt, zuko_amd/static_ar.py: PREBUILT):  cfg2 50 (2 mod 4), cfg3 17 (1 mod 4), cfg1 7 (3 mod 4),
MAF(16, [128, 128]) 3 (<= 3), NSF(16, context 2, [64, 64]) 4 (0 mod 4), MAF(12, [64, 64]) 2, MAF(7, context 2, [40]) 1 — the stream ends inside
the chunk in all but cfg2 and cfg3 —, NSF(128, [256] * 3) 88: four slots do not fit beside its row tiles, it keeps three.

The second half compiles the cfg2 kernel as tests/test_codegen_half.py does and looks at the ring in the ISA."""

import re

import pytest

from test_codegen_half import _check_raw_reads, _isa

SHAPES = {
    "cfg2": (("rqs", 64, 0, (256, 256, 256), 8), 50, 4),
    "cfg3": (("affine", 64, 0, (256, 256, 256), 0), 17, 4),
    "cfg1": (("rqs", 3, 5, (128, 128, 128), 8), 7, 4),
    "maf16": (("affine", 16, 0, (128, 128), 0), 3, 4),
    "nsf16c2": (("rqs", 16, 2, (64, 64), 8), 4, 4),
    "maf12": (("affine", 12, 0, (64, 64), 0), 2, 4),
    "maf7c2": (("affine", 7, 2, (40,), 0), 1, 4),
    "nsf128": (("rqs", 128, 0, (256, 256, 256), 8), 88, 3),
}
_TABLES: dict = {}


def _tables(name: str) -> list:
    """The two-part tables of both feature orders of a shape."""
    if name not in _TABLES:
        from zuko_amd import static_ar

        _TABLES[name] = [static_ar.half_tables(plan, lay.kind, 1)[0] for plan, lay, _ in static_ar._plans_for(*SHAPES[name][0])]
    return _TABLES[name]


def walk(t: dict, tiles: int) -> dict:
    """Runs static_ar.half_schedule(t) over `tiles` tiles of one workgroup and asserts (a) and (b); returns counts."""
    from zuko_amd import static_ar

    pro, ev = static_ar.half_schedule(t)
    nr, ch, per, nch, images = t["NR"], t["CH"], t["CH"] // t["WAVES"], t["NCHUNK"], t["IMAGES"]
    size = lambda g: min(images, (g % nch + 1) * ch) - (g % nch) * ch  # images of chunk g that are read
    st = dict(issued=0, vm=[], landed=set(), visible=set(), lds=[], requested={}, returned={}, at_barrier=None, barriers=0, waits=0, drains=0, reads=0, last=None)
    owner: dict = {}  # slot -> chunk it holds

    def step(e, tile):
        kind = e[0]
        if kind == "issue":
            g = st["issued"]
            slot = g % nr
            if slot in owner:  # (a)
                p = owner[slot]
                assert st["last"] == "barrier", f"chunk {g}: the DMA issue does not stand behind a barrier"
                req, ret = st["at_barrier"]
                assert req.get(p, 0) == size(p), f"chunk {g} -> slot {slot}: chunk {p} in it had {req.get(p, 0)} of {size(p)} images requested at the barrier"
                assert ret.get(p, 0) == size(p), f"chunk {g} -> slot {slot}: {size(p) - ret.get(p, 0)} reads of chunk {p} had not returned at the barrier"
            owner[slot] = g
            st["vm"] += [g] * per
            st["issued"] += 1
        elif kind == "x":
            st["vm"] += ["x"] * e[1]
        elif kind == "wait":
            n = e[1]
            done, st["vm"] = (st["vm"][: len(st["vm"]) - n], st["vm"][len(st["vm"]) - n :]) if n < len(st["vm"]) else ([], st["vm"])
            st["landed"] |= {g for g in done if g != "x" and g not in st["vm"]}
            st["waits"] += 1
            if e[2]:
                st["drains"] += 1
                for g, _ in st["lds"]:
                    st["returned"][g] = st["returned"].get(g, 0) + 1
                st["lds"] = []
        elif kind == "barrier":
            st["visible"] |= st["landed"]
            st["at_barrier"] = (dict(st["requested"]), dict(st["returned"]))
            st["barriers"] += 1
        elif kind == "read":
            g = tile * nch + e[1] // ch
            assert owner.get(g % nr) == g, f"tile {tile} image {e[1]}: slot {g % nr} holds chunk {owner.get(g % nr)}, not {g}"
            assert g in st["visible"], f"tile {tile} image {e[1]}: chunk {g} is read before a barrier behind the vmcnt wait that covers its DMA"  # (b)
            st["lds"].append((g, e[1]))
            st["requested"][g] = st["requested"].get(g, 0) + 1
            st["reads"] += 1
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
    for tile in range(tiles):
        pos = [e[1] for e in ev if e[0] == "read"]
        assert pos == list(range(images)), "a tile pass reads every image of the stream once, in stream order"
        for e in ev:
            step(e, tile)
        assert not st["lds"], "a tile ends with every weight read returned"
        assert st["issued"] == (tile + 1) * nch + nr - 1, "a tile pass requests as many chunks as it reads"
    return st


@pytest.mark.parametrize("name", list(SHAPES))
def test_ring_schedule_keeps_slots_and_visibility(name):
    _, n_chunks, nr = SHAPES[name]
    for t in _tables(name):
        assert (t["NCHUNK"], t["NR"]) == (n_chunks, nr), (t["NCHUNK"], t["NR"])
        st = walk(t, tiles=9)  # (more than two rounds of every slot phase: 9 NCHUNK chunks)
        per_tile = (st["barriers"] - 1) // 9
        assert per_tile == n_chunks and (st["barriers"] - 1) % 9 == 0, "one barrier per chunk"
        tail_inside = nr == 4 and t["IMAGES"] - (n_chunks - 1) * t["CH"] < t["BPOS"] + 2
        assert st["drains"] == 1 + 9 * (n_chunks if nr == 3 else int(tail_inside)), "four slots: no boundary drains the LDS queue but one whose chunk ends early"
        print(f"{name}: {n_chunks} chunks, NR {nr}, {st['reads'] // 9} reads, {per_tile} barriers and {st['drains'] // 9 if nr == 3 else int(tail_inside)} LDS drains per tile")


def test_slot_phase_changes_from_tile_to_tile():
    t = _tables("cfg2")[0]
    assert t["NCHUNK"] % t["NR"] == 2, "cfg2: 50 chunks on four slots — a tile starts in slot 0 or 2"
    chunks = sorted({_tables(n)[0]["NCHUNK"] % 4 for n in SHAPES if SHAPES[n][2] == 4})
    assert chunks == [0, 1, 2, 3], chunks


@pytest.mark.parametrize("name", ["cfg2", "cfg1"])
def test_the_walk_catches_a_barrier_too_close_to_the_chunk_boundary(name):
    """BPOS = 0 puts the barrier behind the chunk's first request, where the last block of the chunk before may still be outstanding: (a) fails."""
    t = dict(_tables(name)[0], BPOS=0)
    with pytest.raises(AssertionError, match="had not returned at the barrier"):
        walk(t, tiles=6)


def test_the_walk_catches_a_wait_that_leaves_the_chunk_in_flight(monkeypatch):
    """A vmcnt that lets two more chunks' pieces stay in flight makes a chunk visible only at the barrier INSIDE it: (b) fails."""
    from zuko_amd import static_ar

    t = _tables("cfg2")[0]
    per = t["CH"] // t["WAVES"]
    pro, ev = static_ar.half_schedule(t)
    loose = [("wait", e[1] + 2 * per, e[2]) if e[0] == "wait" else e for e in ev]
    monkeypatch.setattr(static_ar, "half_schedule", lambda _t: (pro, loose))
    with pytest.raises(AssertionError, match="is read before a barrier"):
        walk(t, tiles=3)


# ---- the compiled cfg2 kernel -----------------------------------------------------------------------------------------


def _product(s: str) -> list:
    names = re.findall(r"^(_ZN2zk10arh_kernel\S+):", s, flags=re.M)
    product = [n for n in names if n.endswith("ELb0EEEvNS_6ArArgsE")]
    assert len(names) == 2 and len(product) == 1, names
    i = s.index(product[0] + ":")
    lines = [x.strip() for x in s[i : s.index(".Lfunc_end", i)].split("\n")]
    return [l for l in lines if l and not l.startswith((";", "//", "."))]


def test_cfg2_ring_in_the_isa():
    s = _isa()
    ops = _product(s)
    t = _tables("cfg2")[0]
    assert t["NR"] == 4
    bars = [i for i, l in enumerate(ops) if l.startswith("s_barrier")]
    assert len(bars) == 1 + t["NCHUNK"], f"{len(bars)} barriers: the staging barrier and one per chunk"
    # the wait in front of every ring barrier counts vector-memory operations only: the boundary's lgkmcnt(0) drain is gone
    counts = []
    for b in bars[1:]:
        w = next(l for l in reversed(ops[:b]) if l.startswith("s_waitcnt"))
        m = re.fullmatch(r"s_waitcnt vmcnt\((\d+)\)", w)
        assert m, f"'{w}' in front of a ring barrier"
        counts.append(int(m.group(1)))
    assert sorted(counts) == [0] * (t["NCHUNK"] - 1) + [t["NIT"]], counts  # (NIT: the barrier that finds the next tile's row loads younger than its pieces)
    loop = ops[bars[1] : bars[-1]]
    assert not any("vmcnt" in l and "lgkmcnt(0)" in l for l in loop), "a wait of the tile loop drains the LDS queue together with the DMA"
    # moving the ring on costs no multiply, and a chunk's pieces leave from a scalar base with the lane's 32-bit offset
    assert not [l for l in loop if l.startswith("s_mul")], "scalar multiply in the tile loop"
    dma = [l for l in ops if l.startswith("global_load_lds_dwordx4")]
    assert len(dma) == 3 * (3 + t["NCHUNK"]), len(dma)
    assert all(re.fullmatch(r"global_load_lds_dwordx4 v\d+, s\[\d+:\d+\](?: offset:\d+)?", l) for l in dma), [l for l in dma if " off" in l][:3]
    stats = _check_raw_reads(s, "_ZN2zk10arh_kernel")
    assert len(stats) == 2 and all(m == 1800 and r >= 1200 for r, m in stats), stats
