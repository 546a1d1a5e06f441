"""The training GEMM's entry points (csrc/pntf_gemm.hip) against recorded result bits.

tests/golden/gemm_bits.json holds, per case id, the sha256 of the output bytes that
pntf_tt_gemm, pntf_tt_linear_act and pntf_tt_linear_bwd gave at the last commit before the
file's build variants were removed and its host launch code was rewritten;
tests/golden/make_gemm_goldens.py wrote it on an MI355X through the functions below.  The same
calls must give the same bits whatever the host side looks like later: a difference means that
another kernel ran, that a grid or a split changed, or that a kernel's arithmetic did.  No
tolerance.  None of these paths uses atomics, and every case gave equal bits twice at recording.

Split-K factors and grid sizes follow the CU count, so the digests hold for the recorded count
alone: on a device with another count (and only then) the GPU tests skip, saying so.

Cases, each a few milliseconds:
  pntf_tt_gemm        gemm_oracle.all_cases with M·N <= 129·256 and K <= 2049 (the filter of
                      test_recorded_c32_covers_the_small_cases); panel shapes under panel modes
                      0, 1, 2, 3, 6, 7, 8, weight-gradient shapes under wgrad modes 0, 1, 2, the
                      rest once.  The cases tagged "ldb" and "pad" run with the padded strides
                      that test_gemm_engines.py gives them (NaN in every padding; the digest
                      covers C's padding too) and those tagged "mis" with A one float off a
                      16-byte boundary; every other case has natural strides.  Regime shapes from the CU count (REGIMES below): a second round
                      of tiles on grids rounded up to 8 per panel mode, more than 32 splits, the
                      XCD padding's empty splits (K = 2049, among the small cases), and a split-K
                      factor rounded down to whole waves of workgroups.
  pntf_tt_linear_act  schedules 0-3 at m = 33, layouts (0, 0), (3, 1), (12, 2), all four (k, n),
                      with and without res.  At the m that reaches AUTO's fused branch (three
                      full rounds of blocks per wave less 31 points, from the CU count; no test
                      before this one reached that branch, and there the workgroup caps of both
                      fused kernels' grids bind): layout (0, 0) under schedules 0-3 with and
                      without res, layout (3, 1) under schedules 0 and 3 with res, all four
                      (k, n); schedule 0 runs under panel mode 2 there (AUTO never fuses under
                      the default mode).  Left out at that m: layout (12, 2), 15 planes or
                      0.75 GB per tensor and several seconds of operand generation and hashing
                      per case, and the other six schedule / res combinations of (3, 1).
  pntf_tt_linear_bwd  both bwd modes at m = 33 and 65, the same layouts, all four (kc, nc), with
                      and without res; the digest covers out and gbias.
"""
import ctypes
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import gemm_oracle as G
from pntf import _lib

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_bits.json")
PANEL_MODES = (0, 1, 2, 3, 6, 7, 8)
WGRAD_MODES = (0, 1, 2)
LAYOUTS = ((0, 0), (3, 1), (12, 2))
NAN = float("nan")


def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


def cus_of_device():
    return torch.cuda.get_device_properties(0).multi_processor_count


def dev():
    return torch.device("cuda:0")


def vp(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------ cases (no GPU needed)


def whole_waves_case(cus):
    """cus/2 + 1 row tiles and four 512-row lengths of K: 4 splits overfill the CUs and the
    dispatcher rounds them down to 3"""
    c = G.make_case(0, 0, 128 * (cus // 2) + 1, 128, 3 * 512 + 1, 0.0, "randn", "waves")
    tiles = G.ceil_div(c.M, G.BM)
    unrounded = min(G.ceil_div(2 * cus, tiles), G.ceil_div(c.K, 512))
    assert 1 < G.splits_for(c.M, c.N, c.K, cus) < unrounded and tiles * unrounded > cus, c
    return c


def gemm_modes(c):
    """(kind, modes) under which a case of natural layout reaches an engine of its own"""
    if not c.ta and c.beta in (0.0, 1.0) and G.panel_shape(c.N, c.K):
        return "p", PANEL_MODES
    if c.ta and not c.tb and c.beta == 0.0 and G.wgrad_shape(c.M, c.N):
        return "w", WGRAD_MODES
    return "d", (None,)


def gemm_cases(cus):
    """[(id, case, panel mode or None, wgrad mode or None)]"""
    small = [c for c in G.all_cases(cus) if c.M * c.N <= 129 * 256 and c.K <= 2049]
    out = []
    for c in small:
        kind, ms = gemm_modes(c)
        out += [(c, kind, m) for m in ms]
    # REGIMES: a second round of tiles per panel engine, > 32 splits, whole waves of workgroups
    for K, N in G.KN:
        out += [(G.panel_loop_case(m, K, N, cus), "p", m) for m in G.PANEL_MODES]
    groups = G.make_case(1, 0, 128, 128, G.wgrad_k_groups())
    assert G.wgrad_plan(128, 128, groups.K, cus).real > G.RG
    out += [(groups, "w", m) for m in WGRAD_MODES]
    out += [(G.make_case(ta, tb, 130, 128, G.RG * 512 + 1, 0.0, "randn", "groups"), "d", None)
            for ta in (0, 1) for tb in (0, 1)]
    out.append((whole_waves_case(cus), "d", None))
    named = []
    for c, kind, m in out:
        cid = "gemm/%s%s/%d%d-%dx%dx%d-b%g-%s-%s" % (kind, "" if m is None else m, c.ta, c.tb,
                                                      c.M, c.N, c.K, c.beta, c.data, c.tag)
        named.append((cid, c, m if kind == "p" else None, m if kind == "w" else None))
    assert len({n[0] for n in named}) == len(named)
    return named


def auto_fused_m(n, cus):
    """three full rounds of 32-point blocks for every wave of pntf_tt_linear_act's grid, less 31
    points: AUTO (schedule 0) fuses under panel modes below 3 (rounds >= 3, >= 90 % full)"""
    ng = n // 128
    nwg = cus // ng
    if ng == 2:
        nwg = G.ceil_div(nwg, 8) * 8
    return 32 * 3 * 4 * nwg - 31


def act_cases(cus):
    """[(id, ndir, nl, k, n, m, res, schedule, panel mode or None)]"""
    out = []
    for k, n in G.KN:
        for ndir, nl in LAYOUTS:
            for res in (0, 1):
                out += [("act/s%d/%d.%d-%dx%d-m33-r%d" % (s, ndir, nl, k, n, res),
                         ndir, nl, k, n, 33, res, s, None) for s in (0, 1, 2, 3)]
        # AUTO's fused m: schedule 0 under panel mode 2 (it fuses below mode 3 only)
        m = auto_fused_m(n, cus)
        big = [(0, 0, res, s) for res in (0, 1) for s in (0, 1, 2, 3)] + \
              [(3, 1, 1, s) for s in (0, 3)]
        out += [("act/s%d%s/%d.%d-%dx%d-m%d-r%d" % (s, "" if s else "p2", ndir, nl, k, n, m, res),
                 ndir, nl, k, n, m, res, s, None if s else 2) for ndir, nl, res, s in big]
    return out


def bwd_cases():
    """[(id, ndir, nl, kc, nc, m, res, bwd mode)]"""
    return [("bwd/m%d/%d.%d-%dx%d-m%d-r%d" % (mode, ndir, nl, kc, nc, m, res),
             ndir, nl, kc, nc, m, res, mode)
            for kc, nc in G.KN for ndir, nl in LAYOUTS for m in (33, 65) for res in (0, 1)
            for mode in (0, 1)]


def all_ids(cus):
    return [c[0] for c in gemm_cases(cus)] + [c[0] for c in act_cases(cus)] + \
        [c[0] for c in bwd_cases()]


# ------------------------------------------------------------------ the calls


class modes:
    """set the panel / weight-gradient / bwd modes for a block and restore them"""

    def __init__(self, lib, panel=None, wgrad=None, bwd=None):
        self.lib, self.want = lib, (panel, wgrad, bwd)

    def setters(self):
        return (self.lib.pntf_tt_set_panel_mode, self.lib.pntf_tt_set_wgrad_mode,
                self.lib.pntf_tt_set_bwd_mode)

    def __enter__(self):
        self.prev = [fn(-1 if v is None else v) for fn, v in zip(self.setters(), self.want)]

    def __exit__(self, *exc):
        for fn, v in zip(self.setters(), self.prev):
            fn(v)


PAD_STRIDES = {(77, 77): (4, 8, 12), (130, 9): (1, 3, 5), (130, 1100): (8, 4, 1)}   # by (M, K)


def layout_of(c):
    """((floats added to the natural lda, ldb, ldc), floats A lies off a 16-byte boundary): what
    test_gemm_engines.py gives the cases tagged "ldb", "pad" and "mis"; natural otherwise"""
    if c.tag == "ldb":
        return (0, 4 + 8 * c.tb, 0), 0
    if c.tag == "pad":
        return PAD_STRIDES[(c.M, c.K)], 0
    return (0, 0, 0), int(c.tag == "mis")


def padded(x, pad, mis=0):
    """host (rows, cols) fp32 -> device rows of stride cols + pad, NaN in the padding, starting
    `mis` floats into its (16-byte aligned) buffer; returns (buffer, view of the rows)"""
    rows, cols = x.shape
    buf = torch.full((mis + rows * (cols + pad),), NAN, device=dev())
    view = buf[mis:].view(rows, cols + pad)
    view[:, :cols] = gpu(x)
    return buf, view


def run_gemm(lib, c, panel, wgrad):
    """one pntf_tt_gemm call as test_gemm_engines.py makes it: C NaN-filled at beta = 0, work
    NaN-filled and exactly pntf_tt_gemm_work_floats long, strides and alignment by layout_of;
    the digest of C with its padding"""
    opA, opB, C0 = G.operands(c)
    (pa, pb, pc), mis = layout_of(c)
    _, dA = padded(np.ascontiguousarray(opA.T) if c.ta else opA, pa, mis)
    _, dB = padded(np.ascontiguousarray(opB.T) if c.tb else opB, pb)
    _, C = padded(np.full((c.M, c.N), np.nan, np.float32) if C0 is None else C0, pc)
    nw = int(lib.pntf_tt_gemm_work_floats(c.M, c.N, c.K))
    work = torch.full((nw,), NAN, device=dev()) if nw else None
    with modes(lib, panel=panel, wgrad=wgrad):
        st = lib.pntf_tt_gemm(c.ta, c.tb, c.M, c.N, c.K, vp(dA), dA.shape[1], vp(dB), dB.shape[1],
                              vp(C), C.shape[1], c.beta, vp(work), nw, stream())
    assert st == 0, (c, lib.pntf_tt_gemm_last_error())
    return digest(C)


@functools.lru_cache(maxsize=2)
def planes(tag, R, m, width):
    """(R, m, width) seeded normal fp32 planes; not modified by a caller"""
    rng = G.rng_of("bits", tag, R, m, width)
    return rng.standard_normal((R, m, width), dtype=np.float32)


@functools.lru_cache(maxsize=2)
def act_operands(rows, k, n):
    """(x (rows, k), W (n, k), bias (n)) of a pntf_tt_linear_act case; not modified by a caller"""
    rng = G.rng_of("bits-act", rows, k, n)
    x = rng.standard_normal((rows, k), dtype=np.float32)
    W = rng.standard_normal((n, k), dtype=np.float32) / np.float32(np.sqrt(k))
    return x, W, rng.standard_normal(n, dtype=np.float32)


def run_act(lib, cid, ndir, nl, k, n, m, res, sched, panel):
    """one pntf_tt_linear_act call (act = 1); the digest of y and h"""
    R = 1 + ndir + nl
    dx, dW, db = (gpu(a) for a in act_operands(R * m, k, n))
    dr = gpu(planes("res", R, m, n)) if res else None
    y, h = (torch.full((R, m, n), NAN, device=dev()) for _ in range(2))
    nw = max(int(lib.pntf_tt_gemm_work_floats(R * m, n, k)), 2 * k * n)
    work = torch.full((nw,), NAN, device=dev())
    with modes(lib, panel=panel):
        st = lib.pntf_tt_linear_act(ndir, nl, vp(dx), m, k, vp(dW), n, vp(db), vp(dr), vp(y), vp(h),
                                    1, sched, vp(work), nw, stream())
    assert st == 0, (cid, lib.pntf_tt_gemm_last_error(), lib.pntf_tt_last_error())
    return digest(y, h)


def run_bwd(lib, cid, ndir, nl, kc, nc, m, res, mode):
    """one pntf_tt_linear_bwd call; the digest of out and gbias"""
    R = 1 + ndir + nl
    gy, W = G.randn_pair(R * m, kc, nc, "bits-bwd")
    dgy, dW = gpu(gy), gpu(W / np.float32(np.sqrt(kc)))
    dyp = gpu(planes("yprev", R, m, nc))
    dr = gpu(planes("res", R, m, nc)) if res else None
    out = torch.full((R, m, nc), NAN, device=dev())
    gb = torch.full((nc,), NAN, device=dev())
    nw = int(lib.pntf_tt_linear_bwd_work_floats(kc, nc))
    work = torch.full((nw,), NAN, device=dev())
    with modes(lib, bwd=mode):
        st = lib.pntf_tt_linear_bwd(ndir, nl, vp(dgy), m, kc, vp(dW), nc, vp(dyp), vp(dr), vp(out),
                                    vp(gb), vp(work), nw, stream())
    assert st == 0, (cid, lib.pntf_tt_gemm_last_error())
    return digest(out, gb)


def run_family(lib, family, cus):
    """{id: digest} of one family: "gemm", "act" or "bwd" """
    if family == "gemm":
        return {cid: run_gemm(lib, c, p, w) for cid, c, p, w in gemm_cases(cus)}
    if family == "act":
        return {c[0]: run_act(lib, *c) for c in act_cases(cus)}
    return {c[0]: run_bwd(lib, *c) for c in bwd_cases()}


FAMILIES = ("gemm", "act", "bwd")


# ------------------------------------------------------------------ tests


def test_the_fixture_holds_exactly_the_cases_of_this_file():
    """every case listed here has a recorded digest and the other way round (at the recorded CU
    count), so the GPU tests below, which compare every case of their family, leave none out"""
    f = recorded()
    assert sorted(all_ids(f["cus"])) == sorted(f["digests"])
    assert len(f["digests"]) > 2000


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_bits_equal_the_recorded_ones(family):
    f, cus = recorded(), cus_of_device()
    if cus != f["cus"]:
        pytest.skip("digests were recorded on %d CUs (%s); this device has %d, and split-K "
                    "factors and grids follow the count" % (f["cus"], f["device"], cus))
    want = {k: v for k, v in f["digests"].items() if k.startswith(family + "/")}
    got = run_family(_lib.load(), family, cus)
    assert len(got) == len(want) and sorted(got) == sorted(want)
    bad = [k for k in got if got[k] != want[k]]
    assert not bad, (len(bad), bad[:20])
