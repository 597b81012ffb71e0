r"""Static-shape instantiations of the fused autoregressive kernel, generated per conditioner.

csrc/fused_ar_static_impl.h holds the kernel as a template over a `Shape` struct of constexpr tables: which 16 x 16 weight
tiles of every layer hold non-zero weights and where each of them sits in the weight stream (zuko_amd/fused.py:build_plan —
with the hidden units sorted by dependency count the masks of zuko/nn.py:270-295 are block triangular, so all of this is
fixed per (features, context, hidden widths, order, univariate map)).  This module turns a plan into that struct, compiles the
one-kernel translation unit with hipcc (gfx950, ~10-20 s) into zuko_amd/lib/ars/ars_<signature>.so and hands the launcher's
address to the library (zk_ar_forward_static).

* Ahead of time (`prebuild()`, run by zuko_amd/_build.py and __graft_entry__.build()): the conditioners of BASELINE.json's
  configurations and a few common shapes (PREBUILT below).  Their .so files travel with the tree.
* On first use (`lookup(..., rows)`): any other conditioner whose batch is large enough for the compile to pay
  (ZUKO_AMD_JIT_MIN_ROWS, default 2^15 rows in one call or 8 x that in total over the calls; ZUKO_AMD_JIT=0 disables it).  Without hipcc, or below the threshold, the generic
  tile-skipping kernel (widths <= 256) or the layer-wise kernels (wider) run instead — same results.

The generated families, each one record (`Family`: header, Shape fields, entry point, signature, index key, meta) served by one emitter
(`emit`), one compile function (`compile_unit`), one find-or-compile routine (`find_or_compile`) and one loader (`StaticKernel`):

* `ars`   the forward kernel on the f32 matrix instruction (csrc/fused_ar_static_impl.h), also the conditioner-only training forward;
* `arx`   its operand-split twin, three bf16 parts per operand (csrc/fused_ar_split_impl.h): inference and training forward;
* `arh`   the two-part twin of that, two f16 parts per operand (csrc/fused_ar_half_impl.h): inference launches only;
* `arsd`  the backward kernels, in three shapes: the dgrad chain on the f32 instruction, the operand-split chain over every layer, and the
          whole backward of the transform in one launch (tables with "chain" == 1, 2, 3).

The kernels are bit-identical to the generic kernel on the same plan (tests/test_gpu_flows.py), so none of this changes a
number; it removes the run-time tile tests, makes every LDS wait partial and lifts the generic kernel's width limit of 256
(one wavefront per SIMD, 32 + 32 activation tiles, for widths up to 512).
"""

from __future__ import annotations

import ctypes
import dataclasses
import fcntl
import hashlib
import json
import math
import os
import shutil
import subprocess
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
ARS_DIR = os.path.join(HERE, "lib", "ars")  # kernels built ahead of time (prebuild()); also the JIT's directory unless ZUKO_AMD_CACHE_DIR is set
ARS_ABI = 10  # == ARS_ABI of csrc/zk_ar_common.h
UNI_TYPES = {0: "zk::UniAffine", 1: "zk::UniRqs8", 2: "zk::UniRqs4", 3: "zk::UniRqs16", 4: "zk::UniCircRqs8", 5: "zk::UniSos3x5", 6: "zk::UniBern17"}
# 16 bins: the twelve accumulator tiles of a feature group do not fit the f32-instruction template's double-buffered last layer (it would
# spill), but the operand-split template holds them (255 VGPRs, no scratch): that kind exists as a split kernel only, forward only
SPLIT_ONLY_KINDS = {3, 5, 6}
_HEADERS = ("fused_ar_static_impl.h", "fused_ar_split_impl.h", "zk_ar_common.h", "zk_univariate.h", "zk_univariate_bwd.h", "zk_common.h", "zk_half.h")


def _hipcc() -> str | None:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    return None


def _arch() -> str:
    from . import _build

    return _build.ARCH


def _jit_dir() -> str:
    """Where kernels compiled on first use go: ZUKO_AMD_CACHE_DIR when set (a read-only install of the package), else lib/ars."""
    d = os.environ.get("ZUKO_AMD_CACHE_DIR")
    return os.path.join(d, "ars") if d else ARS_DIR


def _dirs() -> list[str]:
    d = _jit_dir()
    return [ARS_DIR] if d == ARS_DIR else [d, ARS_DIR]


def _find(name: str) -> str | None:
    for d in _dirs():
        path = os.path.join(d, name)
        if os.path.exists(path):
            return path
    return None


_WARNED: set = set()


def _warn_once(key: str, msg: str) -> None:
    if key not in _WARNED:
        _WARNED.add(key)
        sys.stderr.write(f"[zuko_amd static_ar] {msg}\n")


def hipcc_flags() -> list:
    """The flags every generated unit is compiled with, without those that say what to produce (_build_so: a shared object; the ISA guards of
    tests/test_codegen*.py: device assembly)."""
    return ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={_arch()}", "-Wno-unused-result", "-Wno-uninitialized", "-ffp-contract=off", f"-I{CSRC}"]


def _build_so(stem: str, source, meta: dict | None, verbose: bool, out_dir: str | None = None, only_dir: bool = False, cxxflags: list | None = None) -> str | None:
    """Compile the one-kernel translation unit `source()` into <dir>/<stem>.so (+ <stem>.json when `meta` is given); a no-op when it
    is there.  Returns the .so path, or None when there is no hipcc, the compile fails, or the directory cannot be written (read-only
    install, full disk): the caller then stays on the generic / layer-wise kernels — a failed JIT must never fail the user's call."""
    # (only_dir: a variant build — a kernel of the same name elsewhere, such as the prebuilt one, does not count; cxxflags: in place of ZUKO_AMD_STATIC_CXXFLAGS)
    have = (os.path.join(out_dir, stem + ".so") if os.path.exists(os.path.join(out_dir, stem + ".so")) else None) if only_dir else _find(stem + ".so")
    if have is not None and (meta is None or os.path.exists(have[: -len(".so")] + ".json")):
        return have
    hipcc = _hipcc()
    if hipcc is None:
        # (this used to be silent — the caller stays on the generic kernels: zk_ar_forward_split, correct but 1.1-1.6x slower)
        _warn_once("nohipcc", f"no hipcc on this machine: the static-shape kernel {stem} cannot be compiled; this conditioner runs on the generic operand-split kernel "
                              "(same results; 1.1-1.6x the generated kernel's time; conditioners wider than 256 run layer by layer).  Build it where a ROCm compiler is installed (zuko_amd.static_ar.prebuild, or one call at the "
                              "target batch size) and ship zuko_amd/lib/ars/ or ZUKO_AMD_CACHE_DIR with the package.")
        return None
    d = out_dir or _jit_dir()
    try:
        os.makedirs(d, exist_ok=True)
        so = os.path.join(d, stem + ".so")
        with open(os.path.join(d, f".lock_{stem}"), "w") as lock:
            fcntl.flock(lock, fcntl.LOCK_EX)  # (several ranks / test workers may want the same kernel at once)
            if os.path.exists(so) and (meta is None or os.path.exists(os.path.join(d, stem + ".json"))):
                return so
            src = os.path.join(d, stem + ".hip")
            with open(src, "w") as f:
                f.write(source())
            tmp = os.path.join(d, f".{stem}.so.{os.getpid()}")
            cmd = [hipcc, *hipcc_flags(), "-shared", "-no-hip-rt",
                   *(os.environ.get("ZUKO_AMD_STATIC_CXXFLAGS", "").split() if cxxflags is None else cxxflags),  # (probe / ablation builds into a ZUKO_AMD_CACHE_DIR of their own: NOT part of the kernel's signature)
                   src, f"-L{_torch_lib_dir()}", "-l:libamdhip64.so", "-o", tmp]
            if verbose:
                print("[zuko_amd static_ar]", " ".join(cmd), flush=True)
            elif out_dir is None:
                _warn_once("jit", f"compiling a static-shape kernel for this conditioner on first use ({stem}, 10-25 s; ZUKO_AMD_JIT=0 disables, ZUKO_AMD_CACHE_DIR redirects)")
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                sys.stderr.write(f"[zuko_amd static_ar] hipcc failed for {src}:\n{r.stdout[-2000:]}\n")
                try:
                    os.remove(tmp)
                except OSError:
                    pass
                return None
            os.replace(tmp, so)
            if meta is not None:
                with open(os.path.join(d, stem + ".json"), "w") as f:
                    json.dump(meta, f)
        return so
    except OSError as exc:
        _warn_once("oserror:" + d, f"cannot build kernels in {d} ({exc}); staying on the generic kernels (set ZUKO_AMD_CACHE_DIR to a writable directory)")
        return None


_HEADER_DIGEST: str | None = None


def _header_digest() -> str:
    """Digest of the kernel headers the generated units include (read once per process: it is consulted on every lookup of a kernel)."""
    global _HEADER_DIGEST
    if _HEADER_DIGEST is None:
        h = hashlib.sha256(str(ARS_ABI).encode())
        for name in _HEADERS:
            with open(os.path.join(CSRC, name), "rb") as f:
                h.update(f.read())
        _HEADER_DIGEST = h.hexdigest()[:12]
    return _HEADER_DIGEST


_HALF_DIGEST = None


def _half_digest() -> str:
    """_header_digest() extended by the two-part kernels' own header (an edit there rebuilds those kernels only)."""
    global _HALF_DIGEST
    if _HALF_DIGEST is None:
        h = hashlib.sha256(_header_digest().encode())
        with open(os.path.join(CSRC, "fused_ar_half_impl.h"), "rb") as f:
            h.update(f.read())
        _HALF_DIGEST = h.hexdigest()[:12]
    return _HALF_DIGEST


def _stamp_of(meta: dict) -> str:
    return _half_digest() if meta.get("half") else _header_digest()


# --------------------------------------------------------------------------------------------------------------------
# plan -> tables
# --------------------------------------------------------------------------------------------------------------------


def tables(plan, uni_kind: int, act: int = 1) -> dict | None:
    """The Shape tables of one plan (fused.ArPlan with its per-tile stream), or None when no static kernel can be built."""
    if plan.fine_gather is None or uni_kind not in UNI_TYPES or act not in range(8):
        return None
    L = plan.n_layers
    NH = L - 1
    if NH < 1 or NH > 6:
        return None
    tm = plan.fine_tilemask
    n_otg = tm.shape[1]
    widths = list(plan.widths)
    HT = [-(-w // 16) for w in widths]
    din4 = -(-plan.din // 4) * 4
    NIT = -(-plan.din // 16)
    TMAX = 4 * -(-max([NIT] + HT) // 4)
    if TMAX > 32:
        return None
    S_OTG, S_IT, S_MASK, NS = [], [], [], []
    for l in range(NH):
        n = 0
        for otg in range(n_otg):
            for it in range(tm.shape[2]):
                m = int(tm[l, otg, it])
                if m:
                    S_OTG.append(otg)
                    S_IT.append(it)
                    S_MASK.append(m)
                    n += 1
        NS.append(n)
    G_IT, GOFF = [], [0]
    for g in range(plan.n_groups):
        bits = int(plan.skip[NH * n_otg + g])
        G_IT += [it for it in range(32) if bits >> it & 1]
        GOFF.append(len(G_IT))
    waves = 8 if TMAX <= 16 else 4
    D = plan.features
    xs = ((D + 3) // 4) * 4 + 4
    bias_floats = plan.bias_off[-1] + len(plan.bias_gather[-1])
    base = (3 * 24 * 256 + bias_floats + 1024 + 256) * 4
    xlds = int(D % 4 == 0 and base + waves * 16 * xs * 4 <= 160 * 1024)
    if base + (waves * 16 * xs * 4 if xlds else 0) > 160 * 1024:
        return None
    if plan.n_groups * plan.layout.fpl * 4 > 1024:
        return None
    return {
        "uni": int(uni_kind), "ACT": int(act), "D": int(D), "DIN": int(din4), "NIT": int(NIT), "NH": int(NH), "HT": HT, "TMAX": int(TMAX), "NG": int(plan.n_groups),
        "NCHUNK": int(plan.fine_n_chunks), "BIAS_STRIDE": int(plan.max_width), "NS": NS, "S_OTG": S_OTG, "S_IT": S_IT, "S_MASK": S_MASK,
        "BASE": [int(b) for b in plan.fine_layer_block0[:NH]], "LAST_BASE": int(plan.fine_layer_block0[NH]), "GOFF": GOFF, "G_IT": G_IT,
        "WAVES": waves, "XLDS": xlds, "TRAIN_OK": int(act == 1 and NH <= 3 and waves == 8 and all(w % 16 == 0 for w in widths) and uni_kind != 3),  # (kinds 5, 6 — split kernels only: the conditioner-only training forward of SOSPF / BPF)
    }


def split_enabled() -> bool:
    """Whether the bf16x3 operand-split kernels may be used (ZUKO_AMD_EXACT_F32=1 keeps every product on the f32 matrix instruction)."""
    return os.environ.get("ZUKO_AMD_EXACT_F32", "0") != "1"


def split_geometry() -> tuple:
    """(wavefronts per workgroup, images per ring chunk) of the operand-split kernels: 8 x 24 = one workgroup of eight wavefronts per CU
    (two per SIMD) sharing one weight stream; ZUKO_AMD_SPLIT_GEOM=4x16 selects two independent workgroups per CU, one wavefront per
    SIMD each (twice the weight-stream traffic; measured 3-5 % slower on cfg2, profiles/r03/split_kernel.md)."""
    g = os.environ.get("ZUKO_AMD_SPLIT_GEOM", "8x24")
    try:
        w, c = (int(v) for v in g.split("x"))
    except ValueError:
        w, c = 8, 24
    return (w, c) if (w, c) in ((4, 16), (8, 24), (8, 48)) else (8, 24)


def split_tables(plan, uni_kind: int, act: int = 1):
    """Tables + gather indices of the OPERAND-SPLIT twin of a static-shape kernel (csrc/fused_ar_split_impl.h), or None.

    gfx950 has no xf32 / tf32 matrix instruction; its f32 one runs at 1/16 of the bf16 rate.  The split kernels write every f32
    operand as h + m + l with three bf16 numbers (8 + 8 + 8 significant bits: exact to 2^-25) and keep the six partial products down to
    2^-18 (hh, hm, mh, mm, hl, lh) on v_mfma_f32_16x16x32_bf16 with f32 accumulation: f32-grade results at 6/16 of the matrix time.
    A stream BLOCK is the 16 x 32 weight block (one out tile, one PAIR of in tiles) as three 1 KiB bf16 images (h, m, l); a lane's 8
    values of a k-group are [4 units of in tile 2 ip | the same 4 units of in tile 2 ip + 1], which is how the activations sit in the
    accumulator registers.  Returns (tables, gathers): gathers[l] int32 [blocks_l * 512] into W_l.flatten() (-1 = zero), every layer
    padded to whole 24-image chunks (8 blocks)."""
    t = tables(plan, uni_kind, act)
    if t is None:
        return None
    wide = t["WAVES"] != 8  # conditioners 257 - 512 wide: 32 activation tiles + their 16 operand pairs per wavefront = one wavefront per SIMD
    if wide and os.environ.get("ZUKO_AMD_SPLIT_WIDE", "1") == "0":
        return None
    cached = getattr(plan, "_split_cache", None)
    if cached is not None and cached[0] == (uni_kind, act, split_geometry()):
        return cached[1]
    NH, HT, NIT = t["NH"], t["HT"], t["NIT"]
    tm = plan.fine_tilemask
    n_otg, n_itile = tm.shape[1], tm.shape[2]
    waves, ch = (4, 24) if wide else split_geometry()
    B_OT, B_IP, NB, BASE, blocks_of = [], [], [], [], []
    cursor = 0  # in 1 KiB images; the layers follow each other without padding (a chunk boundary may fall anywhere, even inside a block)

    def pair_block(fg, t0, t1):
        idx = -np.ones((64, 8), dtype=np.int64)
        if t0 is not None:
            idx[:, :4] = fg[t0]
        if t1 is not None:
            idx[:, 4:] = fg[t1]
        return idx

    for l in range(NH):
        fg = plan.fine_gather[l].reshape(-1, 64, 4)
        pos, k = {}, 0
        for otg in range(n_otg):
            for it in range(n_itile):
                m = int(tm[l, otg, it])
                for b in range(4):
                    if m >> b & 1:
                        pos[(otg * 4 + b, it)] = k
                        k += 1
        n_in = NIT if l == 0 else HT[l - 1]
        blocks = []
        for ot in range(HT[l]):
            for ip in range(-(-n_in // 2)):
                t0, t1 = pos.get((ot, 2 * ip)), pos.get((ot, 2 * ip + 1))
                if t0 is None and t1 is None:
                    continue
                blocks.append(pair_block(fg, t0, t1))
                B_OT.append(ot), B_IP.append(ip)
        NB.append(len(blocks))
        BASE.append(cursor)
        cursor += 3 * len(blocks)
        blocks_of.append(blocks)
    # last layer: group g, kept in-tile it, tile t of the group  ->  group g, kept in-pair ip, tile t
    nt = plan.layout.nt
    fg = plan.fine_gather[NH].reshape(-1, 64, 4)
    G_IP, GOFFP, blocks, k = [], [0], [], 0
    for g in range(t["NG"]):
        its = t["G_IT"][t["GOFF"][g] : t["GOFF"][g + 1]]
        at = {it: k + i * nt for i, it in enumerate(its)}
        k += len(its) * nt
        for ip in sorted({it // 2 for it in its}):
            for b in range(nt):
                t0, t1 = at.get(2 * ip), at.get(2 * ip + 1)
                blocks.append(pair_block(fg, None if t0 is None else t0 + b, None if t1 is None else t1 + b))
            G_IP.append(ip)
        GOFFP.append(len(G_IP))
    last_base = cursor
    cursor += 3 * len(blocks)
    # The stream is ceil(images / ch) chunks long: every chunk's first image belongs to a real block (the kernel moves the ring on when
    # it reads that image, so a chunk of nothing but padding would never be consumed).  The gather kernel writes whole blocks: the
    # padding blocks may reach up to two images past the last chunk (STREAM_IMAGES is what the buffer must hold).
    n_chunks = -(-cursor // ch)
    pad_blocks = -(-(n_chunks * ch - cursor) // 3)
    blocks_of.append(blocks + [-np.ones((64, 8), dtype=np.int64)] * pad_blocks)
    stream_images = max(n_chunks * ch, cursor + 3 * pad_blocks)
    gathers = [np.stack(b).astype(np.int32).reshape(-1) if b else np.zeros(0, np.int32) for b in blocks_of]
    out = dict(t)
    for key in ("S_OTG", "S_IT", "S_MASK", "NS", "GOFF", "G_IT"):
        out.pop(key)
    nr = 2 if ch == 48 else 3  # (48-image chunks: two ring slots, half as many barriers)
    per_cu = 2 if (waves == 4 and not wide) else 1  # workgroups per CU
    xlds = int(t["D"] % 4 == 0 and (nr * ch * 256 + (t["BIAS_STRIDE"] * NH + t["NG"] * nt * 16) + 1024 + 256 + waves * 16 * (((t["D"] + 3) // 4) * 4 + 4)) * 4 * per_cu <= 160 * 1024)
    out.update({"split": 1, "TMAX": int(2 * -(-t["TMAX"] // 2)), "NB": NB, "B_OT": B_OT, "B_IP": B_IP, "BASE": BASE, "LAST_BASE": last_base, "GOFF": GOFFP, "G_IP": G_IP, "NCHUNK": n_chunks, "STREAM_IMAGES": stream_images,
                "WAVES": waves, "CH": ch, "NR": nr, "XLDS": xlds, "OCC": 1 if wide else 2})
    plan._split_cache = ((uni_kind, act, split_geometry()), (out, gathers))
    return out, gathers


def half_enabled() -> bool:
    """Whether the TWO-PART (2 x f16, three partial products) twins of the operand-split kernels may serve inference launches
    (zuko_amd.set_matmul_precision / ZUKO_AMD_MATMUL: "f16x2" default, "bf16x3" keeps every product on the three-part kernels)."""
    from . import fused

    return split_enabled() and fused.matmul_precision() == "f16x2"


def half_tables(plan, uni_kind: int, act: int = 1):
    """Tables + gather indices of the two-part twin of an operand-split kernel (csrc/fused_ar_half_impl.h), or None.

    Same blocks in the same order as split_tables — a block is the 16 x 32 weight block (one out tile, one pair of in tiles) — as TWO 1 KiB f16
    images (h, l) of the layer's weights times a power of two (zuko_amd/fused.py picks it: the layer's largest magnitude lands in [2^14, 2^15)),
    three partial products (lh, hl, hh) on v_mfma_f32_16x16x32_f16.  Eight wavefronts, conditioners up to 256 wide and three hidden layers (the
    kernel takes one descale factor per linear layer, four at most); the polynomial maps keep the three-part kernels."""
    ts = split_tables(plan, uni_kind, act)
    if ts is None:
        return None
    t, gathers = ts
    if t["WAVES"] != 8 or t["NH"] > 3 or uni_kind in SPLIT_ONLY_KINDS or t["CH"] != 24:
        return None
    cached = getattr(plan, "_half_cache", None)
    if cached is not None and cached[0] == (uni_kind, act):
        return cached[1]
    ch, NH, nt = t["CH"], t["NH"], plan.layout.nt
    n_last = t["GOFF"][-1] * nt
    cursor = 2 * (sum(t["NB"]) + n_last)
    n_chunks = -(-cursor // ch)
    pad_blocks = -(-(n_chunks * ch - cursor) // 2)
    last = gathers[NH][: n_last * 512]
    g = [np.asarray(x) for x in gathers[:NH]] + [np.concatenate([last, -np.ones(pad_blocks * 512, dtype=np.int32)]).astype(np.int32)]
    out = {k: v for k, v in t.items() if k not in ("split", "TRAIN_OK")}
    # Ring depth: FOUR slots (a chunk becomes visible one chunk before it is read: half_schedule) where they fit the 160 KiB next to the bias
    # image, the tables and the row tiles the three-slot geometry has chosen (XLDS stays what it was); else the three-slot protocol
    bias_floats = plan.bias_off[-1] + len(plan.bias_gather[-1])
    rows = t["WAVES"] * 16 * (((t["D"] + 3) // 4) * 4 + 4) if t["XLDS"] else 0
    nr = 4 if (4 * ch * 256 + bias_floats + 1024 + 256 + rows) * 4 <= 160 * 1024 else 3
    out.update({"half": 1, "BASE": [2 * sum(t["NB"][:l]) for l in range(NH)], "LAST_BASE": 2 * sum(t["NB"]), "NCHUNK": n_chunks, "STREAM_IMAGES": max(n_chunks * ch, cursor + 2 * pad_blocks),
                "NR": nr, "IMAGES": cursor, "BPOS": HALF_BPOS, "TRAIN_OK": 0})
    plan._half_cache = ((uni_kind, act), (out, g))
    return out, g


def flow_tables(tables: list):
    """Tables of the flow kernel that serves transforms with these two-part tables (half_tables, in the flow's order), and per transform whether its
    first layer follows the alternative pattern; or None.  The members may differ from the first one in the first layer's in pairs only, and all that
    differ must agree (a flow that alternates the ascending and the descending feature order: the orders mirror the input tiles).  The kernel wants
    the four-slot ring, rows staged in LDS, no context columns and two chunks or more per pass."""
    t0 = tables[0]
    if t0["NR"] != 4 or not t0["XLDS"] or t0["DIN"] != t0["D"] or t0["D"] % 4 or t0["NCHUNK"] < 2 or t0["STREAM_IMAGES"] != t0["NCHUNK"] * t0["CH"] or t0["BASE"][0] != 0:
        return None
    nb0 = t0["NB"][0]
    alt, flags = None, []
    for t in tables:
        if t == t0:
            flags.append(0)
            continue
        if {k: v for k, v in t.items() if k != "B_IP"} != {k: v for k, v in t0.items() if k != "B_IP"} or t["B_IP"][nb0:] != t0["B_IP"][nb0:] or (alt is not None and t["B_IP"][:nb0] != alt):
            return None
        alt = t["B_IP"][:nb0]
        flags.append(1)
    out = dict(t0, flow=1, FLOW_ALT=int(alt is not None), B_IP_ALT=alt if alt is not None else t0["B_IP"][:nb0])
    return out, flags


def lookup_flow(tf: dict, rows: int | None = None):
    """The flow kernel (StaticKernel) of flow_tables' tables, or None: found on disk, or compiled when `rows` reaches the JIT threshold."""
    if not _enabled() or not half_enabled():
        return None
    found = find_or_compile(ARHF, tf, _jit_allowed(rows), verbose=_jit_verbose())
    return None if found is None else found[0]


HALF_LOOK = 1  # == ARH_LOOK of csrc/fused_ar_half_impl.h: blocks of weight images requested ahead of the matrix instructions that consume them
HALF_BPOS = 8  # four-slot ring: the chunk's barrier stands behind the request of the block at images BPOS, BPOS + 1 (even, >= 2 (HALF_LOOK + 1))


def half_trigger(t: dict, c: int) -> int:
    """Four-slot ring: the stream position (image) of chunk c behind whose read the chunk's barrier stands — BPOS + 1, or the chunk's last real
    image when the stream ends before it (the last chunk; the wait there also drains the wavefront's LDS reads)."""
    ch = t["CH"]
    last = min(t["IMAGES"], (c + 1) * ch) - 1
    return min(c * ch + t["BPOS"] + 1, last)


def half_schedule(t: dict) -> tuple:
    """The static schedule of the two-part kernel's weight ring (csrc/fused_ar_half_impl.h: ArhRing / ArhRing4, arh_hidden, arh_body), the same for
    every wavefront: (prologue, one tile pass), each a list of events in program order

        ("issue",)            the wavefront's PER DMA pieces of the next stream chunk into the next slot (both counted round-robin from 0)
        ("x", n)              n vector-memory loads of the next tile's rows
        ("wait", n, drain)    s_waitcnt vmcnt(n); drain: also lgkmcnt(0)
        ("barrier",)
        ("read", pos)         LDS read of stream image pos of this pass
        ("settle", n)         s_waitcnt lgkmcnt(n): all but the youngest n image reads have returned

    (the bias reads that share the LDS queue stand in front of the request a settle leaves outstanding: they do not change which images return)."""
    return _half_prologue(t), _half_pass(t)


def _half_prologue(t: dict) -> list:
    return [("issue",)] * (t["NR"] - 1) + [("x", t["NIT"]), ("wait", 0, True), ("barrier",)]  # (ArLds::stage ends in __syncthreads())


def half_flow_bias_chunk(t: dict) -> int:
    """Flow kernel: the chunk of a pass behind whose barrier the NEXT pass's bias image is requested — the last but one, so that the last chunk's
    barrier publishes it (ArhRing4::bias_request)."""
    return t["NCHUNK"] - 2


def half_flow_schedule(t: dict, T: int) -> tuple:
    """half_schedule for the FLOW kernel (arhf_kernel: the passes of T transforms over one tile follow each other on one stream of T NCHUNK chunks):
    (prologue, [pass of transform 0, ..., pass of transform T - 1]).  The passes differ at the edges only: the next tile's rows are requested in
    the LAST pass — in the others the barrier at that place waits for vmcnt(0) like every other —, and every pass carries one more event,

        ("bias",)             the LDS-DMA request of the next pass's bias image into the buffer the pass in progress does not read

    behind the barrier of chunk half_flow_bias_chunk(t).  Four-slot ring only."""
    assert t["NR"] == 4 and t["NCHUNK"] >= 2
    return _half_prologue(t), [_half_pass(t, rows=(k == T - 1), bias_at=half_flow_bias_chunk(t)) for k in range(T)]


def _half_pass(t: dict, rows: bool = True, bias_at: int | None = None) -> list:
    """One tile pass of half_schedule.  rows: the pass requests the next tile's rows; bias_at: the chunk behind whose barrier ("bias",) stands."""
    ch, nr, per, look = t["CH"], t["NR"], t["CH"] // t["WAVES"], HALF_LOOK
    nit, last_base, images = t["NIT"], t["LAST_BASE"], t["IMAGES"]
    if nr == 4:
        trig = {half_trigger(t, c): c for c in range(t["NCHUNK"])}
        xpos = min((p for p in trig if p >= last_base), default=-1)  # (none: the rows are consumed, at the next tile's start, in front of the next barrier)
    else:
        xpos = -(-last_base // ch) * ch
    ev = []

    def read(pos):
        if nr != 4 and pos % ch == 0:
            ev.extend([("wait", (nr - 2) * per + (nit if pos == xpos and rows else 0), True), ("barrier",), ("issue",)])
        ev.append(("read", pos))
        if nr == 4 and pos in trig:
            ev.extend([("wait", nit if pos == xpos and rows else 0, pos % ch != t["BPOS"] + 1), ("barrier",), ("issue",)])
            if trig[pos] == bias_at:
                ev.append(("bias",))

    def layer(base, nb, last_of):
        lk = min(look, nb)
        for b in range(lk):
            read(base + 2 * b), read(base + 2 * b + 1)
        for s in range(nb):
            if s + lk < nb:
                read(base + 2 * (s + lk)), read(base + 2 * (s + lk) + 1)
            ahead = lk if s + lk < nb else nb - 1 - s
            ev.append(("settle", (2 if s + lk < nb else 0) if last_of(s) else 2 * ahead))

    off = 0
    for l in range(t["NH"]):
        nb = t["NB"][l]
        ots = t["B_OT"][off : off + nb]
        layer(t["BASE"][l], nb, lambda s: s + 1 == nb or ots[s + 1] != ots[s])
        off += nb
    if rows:
        ev.append(("x", nit))
    nbl = (images - last_base) // 2
    nt = nbl // max(t["GOFF"][-1], 1)
    ends = {g1 * nt - 1 for g1 in t["GOFF"][1:]}
    layer(last_base, nbl, lambda s: s in ends)
    return ev


# --------------------------------------------------------------------------------------------------------------------
# the generated families: what a translation unit looks like, how it is named, what its meta holds
# --------------------------------------------------------------------------------------------------------------------


def _split(t: dict):
    """(core, l0): everything but the first layer's input-tile list, and that list (a descending feature order changes only it)."""
    n0 = t["NS"][0]
    core = {k: v for k, v in t.items() if k != "S_IT"}
    core["S_IT_rest"] = t["S_IT"][n0:]
    return core, t["S_IT"][:n0]


def _digest(obj) -> str:
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()[:16]


def _arr(name: str, ctype: str, vals) -> str:
    vals = list(vals) or [0]
    return f"  static constexpr {ctype} {name}[{len(vals)}] = {{{', '.join(str(int(v)) for v in vals)}}};"


def _pick(t: dict, *names) -> dict:
    return {n: t[n] for n in names}


@dataclasses.dataclass(frozen=True)
class Family:
    """One family of generated kernels: everything emit / compile_unit / find_or_compile need to know about it."""

    prefix: str          # of the file stem: <prefix>_<signature digest>
    header: str          # the template the unit instantiates (csrc/)
    stamp: object        # () -> digest of the headers the unit depends on: part of the signature, checked by _scan
    shape: tuple         # the lines of `struct Shape`, in order: (C type, names) — "int" / "bool": one line of scalars, a name being a table field or
                         # "NAME=literal"; "int[]" / "unsigned char[]": one array per name
    prefix_sums: dict    # array -> the name of its prefix-sum companion, printed right after it
    entry: str           # the extern "C" symbol ...
    params: tuple        # ... and its parameters (C type, name), all forwarded to the launcher
    launcher: str        # the launcher expression ({uni}: the univariate map's type)
    sig: object          # (tables, alt) -> what the signature digest is taken of (next to the stamp)
    index: object        # tables -> the key the unit's meta is indexed under (_scan, _found); None: found by file name
    meta: object         # tables -> the family's own fields of the meta JSON


FLOW_ENTRY = "zk_arhf_launch"
_FORWARD = dict(entry="zk_ars_launch", params=(("const zk::ArArgs*", "a"), ("int", "abi"), ("int", "args_bytes"), ("int", "train"), ("void*", "stream")))
_BACKWARD = dict(entry="zk_ars_dgrad_launch", params=(("const zk::ArArgs*", "a"), ("int", "abi"), ("int", "args_bytes"), ("void*", "stream")))

# the f32-instruction forward kernel (csrc/fused_ar_static_impl.h).  Indexed by its core: one kernel serves both feature orders when they differ in
# the first layer's input tiles only (`alt`, rev 1)
ARS = Family(
    prefix="ars", header="fused_ar_static_impl.h", stamp=_header_digest, **_FORWARD, launcher="zk::ars_launch<Shape, {uni}>",
    shape=(("int", ("D", "DIN", "NIT", "NH", "TMAX", "NG", "NCHUNK")), ("int", ("BIAS_STRIDE", "LAST_BASE", "WAVES", "ACT")), ("bool", ("XLDS", "HAS_ALT", "TRAIN_OK")),
           ("int[]", ("HT", "NS", "BASE")), ("unsigned char[]", ("S_OTG", "S_IT", "S_ALT", "S_MASK")), ("int[]", ("GOFF",)), ("unsigned char[]", ("G_IT",))),
    prefix_sums={"NS": "SOFF"},
    sig=lambda t, alt: {"core": _split(t)[0], "l0": _split(t)[1], "alt": alt},
    index=lambda t: _digest(_split(t)[0]),
    meta=lambda t: _pick(t, "uni", "ACT", "D", "DIN", "HT", "WAVES", "TRAIN_OK", "XLDS"),
)
# its operand-split twin, three bf16 parts per operand (csrc/fused_ar_split_impl.h: arx_kernel)
ARX = Family(
    prefix="arx", header="fused_ar_split_impl.h", stamp=_header_digest, **_FORWARD, launcher="zk::arx_launch<Shape, {uni}>",
    shape=(("int", ("D", "DIN", "NIT", "NH", "TMAX", "NG", "NCHUNK")), ("int", ("BIAS_STRIDE", "LAST_BASE", "WAVES", "CH", "NR", "ACT", "OCC")),
           ("bool", ("XLDS", "HAS_ALT=false", "TRAIN_OK")), ("int[]", ("HT", "NB", "BASE")), ("unsigned char[]", ("B_OT", "B_IP")), ("int[]", ("GOFF",)), ("unsigned char[]", ("G_IP",))),
    prefix_sums={"NB": "BOFF"},
    sig=lambda t, alt: {"split": t},
    index=lambda t: "x" + _digest(t),
    meta=lambda t: dict(_pick(t, "uni", "ACT", "D", "DIN", "HT", "WAVES", "CH", "TRAIN_OK", "XLDS", "NCHUNK"), split=1),
)
# the two-part twin of that, two f16 parts per operand, inference only (csrc/fused_ar_half_impl.h: arh_kernel); stamped by its own header too
ARH = dataclasses.replace(
    ARX, prefix="arh", header="fused_ar_half_impl.h", stamp=_half_digest, launcher="zk::arh_launch<Shape, {uni}>",
    shape=ARX.shape[:2] + (("int", ("IMAGES", "BPOS")), ("bool", ("XLDS",))) + ARX.shape[3:],
    sig=lambda t, alt: {"half": t},
    index=lambda t: "h" + _digest(t),
    meta=lambda t: dict(_pick(t, "uni", "ACT", "D", "DIN", "HT", "WAVES", "CH", "TRAIN_OK", "XLDS", "NCHUNK"), half=1, split=2),
)
# the FLOW launch of the two-part kernel: all transforms of a composed flow in one persistent launch (arhf_kernel; zuko_amd/fused.py: FusedFlow).  A unit of
# its own, from flow_tables: the two-part tables of the flow's first transform plus the first layer's in pairs under the flow's other feature order
ARHF = dataclasses.replace(
    ARH, prefix="arhf", entry=FLOW_ENTRY, launcher="zk::arhf_launch<Shape, {uni}>",
    params=(("const zk::ArArgs*", "a"), ("const zk::ArhFlow*", "f"), ("int", "abi"), ("int", "args_bytes"), ("int", "flow_bytes"), ("void*", "stream")),
    shape=ARH.shape + (("bool", ("FLOW_ALT",)), ("unsigned char[]", ("B_IP_ALT",))),
    sig=lambda t, alt: {"flow": t},
    index=lambda t: "f" + _digest(t),
    meta=lambda t: dict(_pick(t, "uni", "ACT", "D", "DIN", "HT", "WAVES", "CH", "XLDS", "NCHUNK", "NR", "FLOW_ALT"), half=1, flow=1),
)
# the backward kernels, in three shapes told apart by the tables' "chain" field (chain_tables: 1, chain_split_tables: 2 and 3).  Their signature
# covers the whole tables, so they are found by file name
ARSD_F32 = Family(  # dgrad through the hidden layers on the f32 instruction (csrc/fused_ar_static_impl.h: ars_dgrad_kernel)
    prefix="arsd", header="fused_ar_static_impl.h", stamp=_header_digest, **_BACKWARD, launcher="zk::ars_dgrad_launch<Shape>",
    shape=(("int", ("DIN", "DOUT", "NIT", "NH", "TMAX", "NCHUNK", "WAVES=8", "ACT=1")), ("bool", ("HAS_ALT=false",)), ("int[]", ("HT", "NS", "BASE")),
           ("unsigned char[]", ("S_OTG", "S_IT", "S_ALT", "S_MASK"))),
    prefix_sums={"NS": "SOFF"},
    sig=lambda t, alt: {"t": t},
    index=None,
    meta=lambda t: _pick(t, "DIN", "DOUT", "HT"),
)
ARSD_SPLIT = dataclasses.replace(  # dgrad through every layer, operand-split (csrc/fused_ar_split_impl.h: arxd_kernel)
    ARSD_F32, header="fused_ar_split_impl.h", launcher="zk::arxd_launch<Shape>",
    shape=(("int", ("DIN0", "DOUT", "NH", "TMAX", "NCHUNK", "WAVES=8", "CH", "NP0", "ACT=1")), ("int[]", ("HT", "NB", "BASE")), ("unsigned char[]", ("P0", "B_OT", "B_IP"))),
    prefix_sums={"NB": "BOFF"},
    meta=lambda t: {"DIN": t["DIN0"], "DOUT": t["DOUT"], "HT": t["HT"]},
)
ARSD_FULL = dataclasses.replace(  # the whole backward of the transform in one launch (arxb_kernel)
    ARSD_SPLIT, launcher="zk::arxb_launch<Shape, {uni}>", shape=ARSD_SPLIT.shape + (("int", ("NG",)), ("int[]", ("PB",))))
FAMILIES = {"ars": ARS, "arx": ARX, "arh": ARH, "arhf": ARHF, "arsd": {1: ARSD_F32, 2: ARSD_SPLIT, 3: ARSD_FULL}}


def emit(fam: Family, t: dict, alt: list | None = None) -> str:
    """C++ source of the translation unit of family `fam` for tables `t`; `alt` (ARS): the first layer's input tiles under the alternative order."""
    v = dict(t, HAS_ALT=alt is not None)
    if "S_IT" in t:
        n0 = t["NS"][0]
        v["S_ALT"] = (alt if alt is not None else t["S_IT"][:n0]) + t["S_IT"][n0:]
    lines = ["// generated by zuko_amd/static_ar.py — do not edit", f'#include "{fam.header}"', "namespace {", "struct Shape {"]
    for ctype, names in fam.shape:
        if ctype.endswith("[]"):
            for name in names:
                lines.append(_arr(name, ctype[:-2], v[name]))
                if name in fam.prefix_sums:
                    lines.append(_arr(fam.prefix_sums[name], "int", [sum(v[name][:i]) for i in range(len(v[name]) + 1)]))
        else:
            show = (lambda x: "true" if x else "false") if ctype == "bool" else str
            lines.append(f"  static constexpr {ctype} " + ", ".join(n.replace("=", " = ") if "=" in n else f"{n} = {show(v[n])}" for n in names) + ";")
    launcher = fam.launcher.format(uni=UNI_TYPES.get(t.get("uni")))
    lines += [
        "};",
        "}  // namespace",
        f'extern "C" int {fam.entry}({", ".join(f"{c} {n}" for c, n in fam.params)}) {{ return {launcher}({", ".join(n for _, n in fam.params)}); }}',
        "",
    ]
    return "\n".join(lines)


def _identity(fam: Family, t: dict, alt: list | None = None):
    """(file stem, meta) of the unit `emit(fam, t, alt)`: the stem carries the digest of everything the unit is made from."""
    stamp = fam.stamp()
    ident = fam.sig(t, alt)
    stem = f"{fam.prefix}_{_digest(dict(ident, headers=stamp))}"
    meta = {"so": stem + ".so", "core": "chain" if fam.index is None else fam.index(t), "l0": ident.get("l0", []), "alt": alt, "headers": stamp, **fam.meta(t)}
    return stem, meta


# --------------------------------------------------------------------------------------------------------------------
# compile / find / load
# --------------------------------------------------------------------------------------------------------------------


class StaticKernel:
    """A loaded generated kernel: `launcher` is the address of its entry point, handed to the library in the argument block."""

    def __init__(self, so: str, meta: dict, entry: str) -> None:
        self.so, self.meta = so, meta
        self.cdll = ctypes.CDLL(so)
        self.launcher = ctypes.cast(getattr(self.cdll, entry), ctypes.c_void_p)


_LOCK = threading.Lock()
_LOADED: dict[str, StaticKernel] = {}
_INDEX: dict | None = None  # core digest -> list of meta dicts found on disk


def _scan() -> dict:
    global _INDEX
    idx: dict = {}
    for d in _dirs():
        try:
            names = sorted(os.listdir(d)) if os.path.isdir(d) else []
        except OSError:
            names = []
        for name in names:
            if name.endswith(".json"):
                try:
                    with open(os.path.join(d, name)) as f:
                        meta = json.load(f)
                except (OSError, ValueError):
                    continue
                if meta.get("headers") == _stamp_of(meta) and os.path.exists(os.path.join(d, meta["so"])):
                    meta["dir"] = d
                    idx.setdefault(meta["core"], []).append(meta)
    _INDEX = idx
    return idx


def _torch_lib_dir() -> str:
    import importlib.util

    spec = importlib.util.find_spec("torch")
    return os.path.join(os.path.dirname(spec.origin), "lib")


def compile_unit(fam: Family, t: dict, alt: list | None = None, verbose: bool = False, out_dir: str | None = None) -> dict | None:
    """Build <stem>.so, the kernel of family `fam` for tables `t` (no-op when it is there and current); returns its meta or None (no hipcc /
    failure / read-only directory)."""
    stem, meta = _identity(fam, t, alt)
    so = _build_so(stem, lambda: emit(fam, t, alt), meta, verbose, out_dir)
    if so is None:
        return None
    global _INDEX
    _INDEX = None
    return dict(meta, dir=os.path.dirname(so))


def _load(meta: dict, entry: str = _FORWARD["entry"]) -> StaticKernel | None:
    k = _LOADED.get(meta["so"])
    if k is None:
        so = os.path.join(meta.get("dir", ARS_DIR), meta["so"])
        try:
            k = StaticKernel(so, meta, entry)
        except OSError as exc:
            _warn_once("load:" + so, f"cannot load {so}: {exc}")
            return None
        _LOADED[meta["so"]] = k
    return k


def _found(fam: Family, t: dict, l0: list | None):
    """(meta, rev) of a kernel on disk that serves tables `t`, or None.  l0 (ARS): the first layer's input tiles the kernel must have as its primary
    (rev 0) or alternative (rev 1) pattern."""
    if fam.index is None:
        name = _identity(fam, t)[0] + ".so"
        so = _LOADED[name].so if name in _LOADED else _find(name)
        return None if so is None else ({"so": name, "dir": os.path.dirname(so)}, 0)
    idx = _INDEX if _INDEX is not None else _scan()
    for meta in idx.get(fam.index(t), []):
        if l0 is None or meta["l0"] == l0:
            return meta, 0
        if meta["alt"] is not None and meta["alt"] == l0:
            return meta, 1
    return None


def find_or_compile(fam: Family, t: dict, allow: bool, l0: list | None = None, verbose: bool = False, out_dir: str | None = None):
    """(StaticKernel, rev) of family `fam` for tables `t`: found on disk, else compiled when `allow`; None otherwise.  (A compile runs OUTSIDE the
    module lock — the per-kernel file lock serialises ranks / threads that want the same kernel — so that other threads' lookups do not wait
    10-25 s behind it.)"""
    with _LOCK:
        found = _found(fam, t, l0)
    if found is None and allow:
        meta = compile_unit(fam, t, None, verbose, out_dir)
        found = None if meta is None else (meta, 0)
    if found is None:
        return None
    with _LOCK:
        k = _load(found[0], fam.entry)
    return None if k is None else (k, found[1])


def build_half_variant(configs: list, out_dir: str, cxxflags: list | None = None, jobs: int = 4) -> list:
    """Compile the two-part kernels (both feature orders' units and the flow unit) of every (kind, features, context, hidden, bins) in `configs` into
    <out_dir>/ars with the extra compiler flags `cxxflags`, whether or not kernels of the same names exist elsewhere; returns the .so paths.  A process
    started with ZUKO_AMD_CACHE_DIR=<out_dir> finds them before the prebuilt ones (probe and ablation builds: scripts/build_half_variant.py)."""
    from concurrent.futures import ThreadPoolExecutor

    ars = os.path.join(os.path.abspath(out_dir), "ars")
    work = []
    for cfg in configs:
        tabs = [half_tables(plan, layout.kind, 1) for plan, layout, _ in _plans_for(*cfg)]
        if any(t is None for t in tabs):
            raise ValueError(f"no two-part kernel for {cfg}")
        for t, _ in tabs:
            if (ARH, t) not in work:
                work.append((ARH, t))
        tf = flow_tables([t for t, _ in tabs])
        if tf is not None:
            work.append((ARHF, tf[0]))

    def one(w):
        fam, t = w
        stem, meta = _identity(fam, t)
        return _build_so(stem, lambda: emit(fam, t), dict(meta, flags=list(cxxflags or [])), False, ars, only_dir=True, cxxflags=list(cxxflags or []))

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        sos = list(ex.map(one, work))
    if any(so is None for so in sos):
        raise RuntimeError("zuko_amd.static_ar: a variant kernel failed to compile")
    rescan()
    return sos


def rescan() -> None:
    """Forget which kernels were found on disk: the next lookup reads the directories (ZUKO_AMD_CACHE_DIR, lib/ars) again."""
    global _INDEX
    with _LOCK:
        _INDEX = None


def loaded_kernels() -> dict:
    """{file name: path} of the generated kernels this process has loaded."""
    with _LOCK:
        return {name: k.so for name, k in _LOADED.items()}


def _enabled() -> bool:
    return os.environ.get("ZUKO_AMD_NO_STATIC_AR", "0") != "1"


def jit_enabled() -> bool:
    return os.environ.get("ZUKO_AMD_JIT", "1") != "0" and _hipcc() is not None


def jit_min_rows() -> int:
    try:
        return int(os.environ.get("ZUKO_AMD_JIT_MIN_ROWS", str(1 << 15)))
    except ValueError:
        return 1 << 15


def _jit_allowed(rows: int | None) -> bool:
    return rows is not None and rows >= jit_min_rows() and jit_enabled()


def _jit_verbose() -> bool:
    return os.environ.get("ZUKO_AMD_JIT_VERBOSE", "0") == "1"


JIT_CUMULATIVE_FACTOR = 8


def effective_rows(holder, rows: int, count: bool = True) -> int:
    """The batch size the JIT threshold is compared with: `rows` itself, or the threshold once `holder` (a plan / state object living as long as
    the conditioner) has seen JIT_CUMULATIVE_FACTOR x the threshold in TOTAL — a training loop with small batches gets its kernel after a few
    dozen steps instead of never.  (ZUKO_AMD_JIT=0 still disables every compile.)"""
    thr = jit_min_rows()
    seen = getattr(holder, "_jit_rows_seen", 0) + (max(int(rows), 0) if count else 0)  # (count=False: a second consultation within the same step)
    try:
        holder._jit_rows_seen = seen
    except AttributeError:
        return rows
    return rows if rows >= thr or seen < JIT_CUMULATIVE_FACTOR * thr else thr


def lookup(plan, uni_kind: int, act: int, rows: int | None = None):
    """(StaticKernel, rev) for this plan, or None.  Kernels found on disk are used whatever the batch; a missing one is compiled
    when `rows` reaches the JIT threshold."""
    if not _enabled():
        return None
    t = tables(plan, uni_kind, act)
    if t is None:
        return None
    allow = _jit_allowed(rows)
    if split_enabled():  # the operand-split kernel (6/16 of the f32 matrix time) when there is one or one may be built
        ts = split_tables(plan, uni_kind, act)
        found = None if ts is None else find_or_compile(ARX, ts[0], allow, verbose=_jit_verbose())
        if found is not None:
            return found
    if uni_kind in SPLIT_ONLY_KINDS:
        return None
    return find_or_compile(ARS, t, allow, l0=_split(t)[1], verbose=_jit_verbose())


def lookup_half(plan, uni_kind: int, act: int, rows: int | None = None):
    """The two-part kernel (StaticKernel) for this plan, or None: found on disk, or compiled when `rows` reaches the JIT threshold."""
    if not _enabled() or not half_enabled():
        return None
    ts = half_tables(plan, uni_kind, act)
    found = None if ts is None else find_or_compile(ARH, ts[0], _jit_allowed(rows), verbose=_jit_verbose())
    return None if found is None else found[0]


# --------------------------------------------------------------------------------------------------------------------
# the backward twin: dgrad through the hidden layers (csrc/fused_ar_static_impl.h: ars_dgrad_kernel)
# --------------------------------------------------------------------------------------------------------------------


def chain_tables(masks_sorted: list, rows: list, cols: list):
    """Tables + gather indices of the dgrad chain of a masked conditioner.

    masks_sorted[l] (bool [out_l, in_l], l = 0 .. n-2: every linear layer but the last) are the masks in the SORTED unit order of
    zuko_amd/train.py:SortedPlan; rows[l] / cols[l] map a sorted row / column back to the module's (so that the weight stream can be
    gathered straight from the module's parameters).  Chain layer c multiplies by the TRANSPOSE of layer l = n-2-c.  Returns
    (tables, gathers) — gathers[c]: int32 index into W_l.flatten() per stream element (-1 = zero), whole 24-tile chunks per layer —
    or None when the widths do not fit (multiples of 16 up to 256 for the hidden layers, a multiple of 4 for the input)."""
    n1 = len(masks_sorted)
    if n1 < 1 or n1 > 4:
        return None
    widths_out = [m.shape[0] for m in masks_sorted]
    if any(w % 16 or w > 256 for w in widths_out) or masks_sorted[0].shape[1] % 4 or masks_sorted[0].shape[1] > 256:
        return None
    lane = np.arange(64)
    li, lq = lane % 16, lane // 16
    S_OTG, S_IT, S_MASK, NS, HT, BASE, gathers = [], [], [], [], [], [], []
    cursor = 0
    for c in range(n1):
        l = n1 - 1 - c
        M = np.asarray(masks_sorted[l], dtype=bool)  # [out_l, in_l]
        out_l, in_l = M.shape
        n_ot, n_it = -(-in_l // 16), -(-out_l // 16)  # chain outputs = the layer's inputs, chain inputs = the layer's outputs
        HT.append(n_ot)
        blocks, n = [], 0
        for otg in range(-(-n_ot // 4)):
            for it in range(n_it):
                m4 = 0
                for t in range(4):
                    ot = otg * 4 + t
                    if ot < n_ot and M[it * 16 : (it + 1) * 16, ot * 16 : (ot + 1) * 16].any():
                        m4 |= 1 << t
                if m4:
                    S_OTG.append(otg), S_IT.append(it), S_MASK.append(m4)
                    n += 1
                    for t in range(4):
                        if m4 >> t & 1:
                            a_ = (otg * 4 + t) * 16 + li[:, None]                        # chain row  = sorted INPUT unit of layer l
                            b_ = it * 16 + (4 * lq)[:, None] + np.arange(4)[None, :]      # chain col  = sorted OUTPUT unit of layer l
                            ok = (a_ < in_l) & (b_ < out_l)
                            idx = np.where(ok, np.asarray(rows[l])[np.minimum(b_, out_l - 1)] * in_l + np.asarray(cols[l])[np.minimum(a_, in_l - 1)], -1)
                            blocks.append(idx.reshape(-1))
        NS.append(n)
        pad = -(-len(blocks) // 24) * 24 - len(blocks)
        blocks += [-np.ones(256, dtype=np.int64)] * pad
        BASE.append(cursor)
        cursor += len(blocks)
        gathers.append(np.concatenate(blocks).astype(np.int32) if blocks else np.zeros(0, np.int32))
    NIT = -(-widths_out[-1] // 16)
    t = {"chain": 1, "DIN": int(widths_out[-1]), "DOUT": int(masks_sorted[0].shape[1]), "NIT": int(NIT), "NH": n1, "HT": HT, "TMAX": int(4 * -(-max([NIT] + HT) // 4)),
         "NCHUNK": cursor // 24, "NS": NS, "S_OTG": S_OTG, "S_IT": S_IT, "S_MASK": S_MASK, "BASE": BASE}
    if t["TMAX"] > 16 or cursor == 0:
        return None
    return t, gathers


def chain_split_tables(masks_sorted: list, rows: list, cols: list, packed: dict | None = None):
    """Tables + gather indices of the operand-split dgrad chain over ALL n linear layers (csrc/fused_ar_split_impl.h: arxd_kernel), from the
    gradient of the packed parameters down to the conditioner's input.  Arguments as chain_tables, but for every layer l = 0 .. n-1.
    Chain layer c multiplies by the transpose of layer l = n-1-c; a block is (out tile = 16 sorted INPUT units of layer l, in pair = 32
    sorted OUTPUT units of layer l) as three bf16 images (split_tables).  Layer 0 is walked in-pair major (its input g_phi is streamed
    from global memory), the others out-tile major.  Returns (tables, gathers) or None.

    packed = {"uni": kind, "featmap": int array [NG * 4 * FPL], "nt", "fpl", "total"} (the forward plan's grouping of the features,
    zuko_amd/fused.py: build_plan): the tables of arxb_kernel instead — the whole backward of the transform in one launch.  Its first layer
    runs over the FORWARD kernel's packed order of phi (unit 16 (g NT + t) + 4 q + r = parameter 4 t + r of the features of lane q in group
    g), in which a lane owns the parameters of its own features and computes their gradient itself; MODROW maps a packed unit to its row of
    the last linear layer (-1: padding slot)."""
    n = len(masks_sorted)
    if n < 2 or n > 4:
        return None
    hidden = [m.shape[0] for m in masks_sorted[:-1]]
    din, dphi = masks_sorted[0].shape[1], masks_sorted[-1].shape[0]
    if any(w % 16 or w > 256 for w in hidden) or din % 4 or din > 256 or (packed is None and dphi % 4):
        return None  # (module-order g_phi rows are read 16 bytes at a time; packed rows are whole tiles)
    masks_sorted, rows = list(masks_sorted), list(rows)
    if packed is not None:
        fm, nt, fpl, total = np.asarray(packed["featmap"]), int(packed["nt"]), int(packed["fpl"]), int(packed["total"])
        ng = len(fm) // (4 * fpl)
        if ng * 4 * fpl != len(fm) or (ng * nt) % 2 or (nt % 2 and ng % 2) or fpl * total > 4 * nt or dphi % total or dphi // total > din or rows[-1] is None:
            return None  # (dphi / total features, the other din - features inputs are context)
        u = np.arange(ng * nt * 16)
        g_, t_, q_, r_ = u // (16 * nt), (u // 16) % nt, (u % 16) // 4, u % 4
        fi_, k_ = np.divmod(4 * t_ + r_, total)
        f_ = np.where(fi_ < fpl, fm[(g_ * 4 + q_) * fpl + np.minimum(fi_, fpl - 1)], -1)
        mod_row = np.where(f_ >= 0, f_ * total + k_, -1)                                       # packed unit -> row of the last linear layer (module order)
        if sorted(mod_row[mod_row >= 0].tolist()) != list(range(dphi)) or not np.array_equal(np.asarray(rows[-1]), np.arange(dphi)):
            return None
        M_last = np.asarray(masks_sorted[-1], dtype=bool)
        masks_sorted[-1] = np.where((mod_row >= 0)[:, None], M_last[np.maximum(mod_row, 0)], False)
        rows[-1] = mod_row
    ch = 24
    lane = np.arange(64)
    li, lq = lane % 16, lane // 16
    HT, NB, BASE, B_OT, B_IP, blocks_of, P0 = [], [], [], [], [], [], []
    cursor = 0
    for c in range(n):
        l = n - 1 - c
        M = np.asarray(masks_sorted[l], dtype=bool)
        out_l, in_l = M.shape
        n_ot, n_ip = -(-in_l // 16), -(-(-(-out_l // 16)) // 2)
        HT.append(n_ot)

        def block(ot, ip):
            a_ = ot * 16 + li[:, None]                                                        # sorted input unit of layer l
            e = np.arange(8)[None, :]
            b_ = (2 * ip + e // 4) * 16 + (4 * lq)[:, None] + e % 4                            # sorted output unit of layer l
            row = np.asarray(rows[l])[np.minimum(b_, out_l - 1)]
            ok = (a_ < in_l) & (b_ < out_l) & (row >= 0)
            return np.where(ok, row * in_l + np.asarray(cols[l])[np.minimum(a_, in_l - 1)], -1)

        def live(ot, ip):
            return bool(M[ip * 32 : ip * 32 + 32, ot * 16 : ot * 16 + 16].any())

        order = [(ot, ip) for ip in range(n_ip) for ot in range(n_ot)] if c == 0 else [(ot, ip) for ot in range(n_ot) for ip in range(n_ip)]
        blocks = []
        for ot, ip in order:
            if live(ot, ip):
                blocks.append(block(ot, ip))
                B_OT.append(ot), B_IP.append(ip)
                if c == 0 and (not P0 or P0[-1] != ip):
                    P0.append(ip)
        if not blocks:
            return None
        NB.append(len(blocks))
        BASE.append(cursor)
        cursor += 3 * len(blocks)
        blocks_of.append(blocks)
    n_chunks = -(-cursor // ch)
    pad = -(-(n_chunks * ch - cursor) // 3)
    blocks_of[-1] = blocks_of[-1] + [-np.ones((64, 8), dtype=np.int64)] * pad
    t = {"chain": 2, "DIN0": int(masks_sorted[-1].shape[0]), "DOUT": int(din), "NH": n, "HT": HT, "TMAX": int(2 * -(-max(HT) // 2)), "NB": NB, "BASE": BASE, "B_OT": B_OT, "B_IP": B_IP,
         "NP0": len(P0), "P0": P0, "NCHUNK": n_chunks, "STREAM_IMAGES": max(n_chunks * ch, cursor + 3 * pad), "WAVES": 8, "CH": ch}
    if t["TMAX"] > 16:
        return None
    if packed is not None:  # first block of every packed pair (layer 0 is in-pair major: the blocks of a pair are consecutive)
        n_pairs = t["DIN0"] // 32
        ips = np.asarray(B_IP[: NB[0]])
        t.update({"chain": 3, "uni": int(packed["uni"]), "NG": ng, "NT": nt, "PB": [int((ips < pp).sum()) for pp in range(n_pairs + 1)], "MODROW": [int(r) for r in mod_row]})
    return t, [np.stack(b).astype(np.int32).reshape(-1) for b in blocks_of]


def chain_kernel(t: dict, allow_compile: bool):
    """The loaded backward kernel for tables `t` (chain_tables / chain_split_tables), built on demand when allowed; None otherwise."""
    found = find_or_compile(FAMILIES["arsd"][t["chain"]], t, allow_compile)
    return None if found is None else found[0]


# --------------------------------------------------------------------------------------------------------------------
# ahead-of-time list
# --------------------------------------------------------------------------------------------------------------------

# (univariate, features, context, hidden widths, bins): the conditioners of BASELINE.json's configurations first
PREBUILT = [
    ("rqs", 64, 0, (256, 256, 256), 8),     # cfg2: NSF(64, T=8, K=8, H=[256]^3)  — the headline
    ("affine", 64, 0, (256, 256, 256), 0),  # cfg3: MAF(64, T=8, H=[256]^3)
    ("rqs", 3, 5, (128, 128, 128), 8),      # cfg1: NSF(3, context 5, H=[128]^3)
    ("rqs", 32, 0, (512, 512), 8),          # widths beyond the generic kernel's 256 (one wavefront per SIMD)
    ("rqs", 32, 0, (256, 256), 8),
    ("affine", 16, 0, (128, 128), 0),
    # shapes the GPU tests exercise (widths that are not multiples of 16 / 64, a context that straddles a tile, one hidden layer, three
    # wide layers): built ahead so that `pytest -m gpu` on a fresh box compiles nothing
    ("rqs", 20, 3, (100, 72), 8),
    ("affine", 7, 2, (40,), 0),
    ("rqs", 24, 8, (384, 512, 320), 8),
    ("rqs", 16, 2, (64, 64), 8, "ELU"),
    ("affine", 12, 0, (48, 32), 0, "Tanh"),
    ("rqs", 64, 0, (256, 256, 256), 16),   # NSF(bins=16): operand-split kernel only (SPLIT_ONLY_KINDS)
    ("affine", 12, 0, (64, 64), 0),        # training: a last feature group that is not full (padding slots in the packed phi / g_phi rows)
    # three more shapes of the static-shape table (profiles/r04/static_shapes.jsonl, tests/test_gpu_flows.py::test_static_shape_table): 128 features, a context
    # behind 64 features, three 512-wide layers
    ("rqs", 128, 0, (256, 256, 256), 8), ("rqs", 64, 8, (256, 256), 8), ("rqs", 16, 0, (512, 512, 512), 8),
    # the polynomial flows (forward, operand-split kernels only): the shapes of the golden flows and a 64-feature one of each
    ("sos", 4, 2, (32, 32), 0), ("bern", 4, 2, (32, 32), 0), ("sos", 64, 0, (256, 256, 256), 0), ("bern", 64, 0, (256, 256, 256), 0),
]


def _plans_for(kind: str, features: int, context: int, hidden, bins: int, activation: str | None = None):
    """Plans of the ascending- and descending-order transform of such a flow (MAF / NSF alternate the two).  (The activation does not
    enter the plan: it is a field of the tables.)"""
    import torch

    from . import fused
    from .flows.autoregressive import MaskedAutoregressiveTransform
    from .nn import MaskedLinear
    from .transforms import BoundedBernsteinTransform, MonotonicAffineTransform, MonotonicRQSTransform, ShiftedSOSPolynomialTransform

    out = []
    for order in (torch.arange(features), torch.flipud(torch.arange(features))):
        if kind == "affine":
            t = MaskedAutoregressiveTransform(features, context, order=order, hidden_features=list(hidden), univariate=MonotonicAffineTransform, shapes=[(), ()])
            layout = fused.uni_layout("affine", 2)
        elif kind == "sos":  # SOSPF's defaults
            t = MaskedAutoregressiveTransform(features, context, order=order, hidden_features=list(hidden), univariate=ShiftedSOSPolynomialTransform, shapes=[(3, 5), ()])
            layout = fused.uni_layout("sos", 16)
        elif kind == "bern":  # BPF's default
            t = MaskedAutoregressiveTransform(features, context, order=order, hidden_features=list(hidden), univariate=BoundedBernsteinTransform, shapes=[(17,)])
            layout = fused.uni_layout("bern", 17)
        else:
            t = MaskedAutoregressiveTransform(features, context, order=order, hidden_features=list(hidden), univariate=MonotonicRQSTransform, shapes=[(bins,), (bins,), (bins - 1,)])
            layout = fused.uni_layout("rqs", 3 * bins - 1, bins)
        masks = [m.mask for m in t.hyper if isinstance(m, MaskedLinear)]
        wide = max(list(hidden) + [features + context]) > fused.MAX_WIDTH
        out.append((fused.build_plan(masks, features, layout, max_width=fused.MAX_WIDTH_WIDE if wide else fused.MAX_WIDTH), layout, [m for m in t.hyper if isinstance(m, MaskedLinear)]))
    return out


def chain_tables_for(lins, full: bool = False, packed: dict | None = None):
    """chain_tables (full: chain_split_tables, with `packed` the whole-backward tables) of a masked ReLU conditioner given its linear layers
    (through zuko_amd/train.py:SortedPlan), or None."""
    import torch

    from .train import SortedPlan

    sp = SortedPlan(lins, 1, torch.device("cpu"))
    n = len(lins)
    if n < 2 or n > 4 or any(m is None for m in sp.mask_s_cpu):
        return None
    if full:
        return chain_split_tables(sp.mask_s_cpu, sp.rows_cpu, sp.cols_cpu, packed=packed) if (packed is not None or sp.shapes[-1][0] % 4 == 0) else None
    return chain_tables(sp.mask_s_cpu[: n - 1], sp.rows_cpu[: n - 1], sp.cols_cpu[: n - 1])


def prebuild(verbose: bool = True, jobs: int = 4) -> list[str]:
    """Compile every PREBUILT kernel that is missing or stale; returns the .so names."""
    from concurrent.futures import ThreadPoolExecutor

    # kernels built against another version of the template / headers can never be selected again: drop them
    if os.path.isdir(ARS_DIR):
        for name in os.listdir(ARS_DIR):
            if name.endswith(".json"):
                try:
                    with open(os.path.join(ARS_DIR, name)) as f:
                        m_ = json.load(f)
                        stale = m_.get("headers") != _stamp_of(m_)
                except (OSError, ValueError):
                    stale = True
                if stale:
                    for ext in (".json", ".so", ".hip"):
                        try:
                            os.remove(os.path.join(ARS_DIR, name[: -len(".json")] + ext))
                        except OSError:
                            pass
            elif name.startswith(".lock_"):
                try:
                    os.remove(os.path.join(ARS_DIR, name))
                except OSError:
                    pass
    work = []  # (family, tables, alt), every unit once

    def want(fam, t, alt=None):
        if (fam, t, alt) not in work:
            work.append((fam, t, alt))

    for entry in PREBUILT:
        kind, features, context, hidden, bins = entry[:5]
        import torch

        from .nn import _act_code

        act = _act_code(getattr(torch.nn, entry[5])()) if len(entry) > 5 else 1
        (pa, layout, lins_a), (pd, _, lins_d) = _plans_for(kind, features, context, hidden, bins)
        if act == 1:  # the training backward of the same conditioners (one kernel per feature order; the polynomial flows — SPLIT_ONLY_KINDS — train on the two-node path: chains without the packed variant)
            for lins, pl in ((lins_a, pa), (lins_d, pd)):
                cands = [chain_tables_for(lins), chain_tables_for(lins, full=True)]
                if (features + context) % 4 == 0 and layout.kind in (0, 1) and layout.total in (2, 23) and pl is not None:  # what zuko_amd/train.py:autoregressive() covers
                    cands.append(chain_tables_for(lins, full=True, packed={"uni": layout.kind, "featmap": pl.featmap, "nt": layout.nt, "fpl": layout.fpl, "total": layout.total}))
                for tg in cands:
                    if tg is not None:
                        want(FAMILIES["arsd"][tg[0]["chain"]], tg[0])
        for pl in (pa, pd):
            ts = split_tables(pl, layout.kind, act)
            if ts is not None:
                want(ARX, ts[0])
            th = half_tables(pl, layout.kind, act)  # the two-part twin (inference launches)
            if th is not None:
                want(ARH, th[0])
        tha, thd = (half_tables(pl, layout.kind, act) if pl is not None else None for pl in (pa, pd))
        tf = flow_tables([tha[0], thd[0]]) if tha is not None and thd is not None else None  # the flow launch of a composition that starts in the ascending order
        if tf is not None:
            want(ARHF, tf[0])
        if layout.kind in SPLIT_ONLY_KINDS:
            continue  # (no f32-instruction kernel, no training chain for this kind)
        ta, td = tables(pa, layout.kind, act), tables(pd, layout.kind, act)
        if ta is None or td is None:
            raise RuntimeError(f"zuko_amd.static_ar: no static kernel for the prebuilt shape {entry}")
        (ca, la), (cdesc, ld) = _split(ta), _split(td)
        if ca == cdesc:
            want(ARS, ta, None if la == ld else ld)
        else:
            want(ARS, ta), want(ARS, td)
    # the alternative workgroup geometry of the split kernels, for the headline conditioner only (tests/test_gpu_flows.py exercises it)
    prev = os.environ.get("ZUKO_AMD_SPLIT_GEOM")
    if prev is None:
        os.environ["ZUKO_AMD_SPLIT_GEOM"] = "4x16"
        try:
            kind, features, context, hidden, bins = PREBUILT[0][:5]
            for pl, layout, _ in _plans_for(kind, features, context, hidden, bins):
                pl._split_cache = None
                ts = split_tables(pl, layout.kind, 1)
                if ts is not None:
                    want(ARX, ts[0])
        finally:
            del os.environ["ZUKO_AMD_SPLIT_GEOM"]
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        metas = list(ex.map(lambda w: compile_unit(*w, verbose, ARS_DIR), work))
    if any(m is None for m in metas):
        raise RuntimeError("zuko_amd.static_ar: a prebuilt static kernel failed to compile")
    return [m["so"] for m in metas]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    import zuko_amd.static_ar as me  # (as a package module: the relative imports above need it)

    print("\n".join(me.prebuild()))
