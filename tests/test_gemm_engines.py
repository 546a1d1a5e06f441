"""Every engine of pntf_tt_gemm (csrc/pntf_gemm.hip) against fp64 at its launch edges, called
through ctypes: the LDS-tiled gemm_kernel with gemm_reduce1/2, panel_gemm_kernel,
panel_lds_kernel, panel_x6_kernel (V = 3, 0, 1), panel_x6s_kernel, wgrad_kernel,
wgrad_x6_kernel and the three pack kernels, plus the fused pntf_tt_linear_act.

Every call: C NaN-filled at beta = 0 (random C0 otherwise), `work` NaN-filled and exactly
pntf_tt_gemm_work_floats(M, N, K) floats long, 1024 sentinel floats behind C and behind work
that must keep their bits, operands that must keep their bits, every padding of a non-natural
lda / ldb / ldc NaN (C's still NaN afterwards), and the result NaN-free and within

    |got - ref64| <= c·EPS32·(|op(A)|·|op(B)| + |beta·C0|) + tiny          elementwise,

no element left out (tests/gemm_oracle.py: reference, bound, planted operands and the CPU proof
that they tell a dropped split product from rounding).  Shapes that exist to reach a launch regime
are derived from the device's CU count through gemm_oracle's restatement of the host arithmetic,
and each asserts that the restatement says it reaches it.

c32 (CPU torch.float32 over every case, `python tests/gemm_oracle.py`) = 4.43 (a wide-dynamic-range case; 3.5 on randn, 3.1 on planted operands), so c = 17.7.
Worst err / (EPS32·bound) measured on the MI355X, per engine:

    engine                                c32     c      worst ratio on MI355X
    gemm_kernel (+ reduce1/2)             4.43    17.7   4.42  (LDS shapes 2.41, panel mode 0 3.93,
                                                               wgrad mode 0 4.42)
    panel_gemm_kernel  (panel mode 1)     4.43    17.7   3.93
    panel_lds_kernel   (panel mode 2)     4.43    17.7   3.93
    panel_x6_kernel    (modes 3 / 6 / 7)  4.43    17.7   3.69 / 6.39 / 3.69
    panel_x6s_kernel   (panel mode 8)     4.43    17.7   3.69
    wgrad_kernel       (wgrad mode 1)     4.43    17.7   2.52
    wgrad_x6_kernel    (wgrad mode 2)     4.43    17.7   3.13
    linear_act         (schedules 1-3)    4.43    17.7   2.63 / 0.20 / 2.63

Two mutants of the kernels, run once each on a scratch copy, fail this file: the product
w[1]·x[1] removed from x6_mma (wgrad_x6_kernel 110-117 at K = 1, panel mode 6 32.5-32.8 on the
a2b2 pair) and the third split term zeroed in x6_pack_kernel (panel modes 3 / 6 / 7 and
linear_act schedule 2, 32.1-32.2 on the a1b3 pair).

Not covered: PNTF_WGRAD_RING (read once at process start), panel modes
4 / 5 (compositions of 2 and 3), and pntf_tt_linear_bwd, whose epilogue is always the act adjoint
(no identity activation; tests/test_tape_kernels.py holds it against the adjoint's reference).
"""
import ctypes
import re

import numpy as np
import pytest
import torch

import gemm_oracle as G
from pntf import _lib

SENT = -1.2345e33
SLACK = 1024
NAN = float("nan")
RATIO = {}
ERR_WORKSPACE = 2


# ------------------------------------------------------------------ CPU: the oracle itself


PLANTED_CPU = [G.make_case(0, 0, 33, 128, K, 0.0, t, "cpu") for K in (128, 256) for t in G.TARGETS]


def test_c_follows_from_c32():
    assert G.C == min(64.0, max(8.0, 4.0 * G.C32))


def test_bf16_split_is_rne_and_exact():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415927,
                  1e-12, 6.5e11, 0.0], np.float32)
    want = np.array([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.140625, 0, 0, 0.0], np.float32)
    got = G.bf16_rne(x)
    assert (got[:5] == want[:5]).all() and got[7] == 0.0
    assert (got.view(np.uint32) & 0xFFFF == 0).all()
    x = G.randn_pair(64, 64, 1)[0]
    x1, x2, x3 = G.split3(x)
    rem = x.astype(np.float64) - x1 - x2 - x3
    assert (np.abs(rem) <= 2.0 ** -24 * np.abs(x)).all()
    assert (np.abs(x2) <= 2.0 ** -8 * np.abs(x)).all() and (np.abs(x3) <= 2.0 ** -16 * np.abs(x)).all()


@pytest.mark.parametrize("case", PLANTED_CPU, ids=lambda c: "%s-K%d" % (c.data, c.K))
def test_planted_cases_hold_for_the_emulation_and_the_yardstick(case):
    opA, opB, C0 = G.operands(case)
    ref, Ab, tiny = G.reference(case, opA, opB, C0)
    full = G.worst_ratio(torch.from_numpy(G.emulate(opA, opB)), ref, Ab, tiny)
    f32 = G.worst_ratio(G.fp32_product(case, opA, opB, C0), ref, Ab, tiny)
    assert full <= G.C and f32 <= G.C32, (full, f32)


@pytest.mark.parametrize("drop", G.PRODUCTS)
def test_every_dropped_product_exceeds_the_bound_on_a_planted_case(drop):
    """each single-product mutant of the emulation fails the GPU tests' bound on its planted pair
    (all of its elements, not one), at both reduction lengths"""
    for case in PLANTED_CPU:
        if drop != "a1b1" and case.data != drop:
            continue
        opA, opB, C0 = G.operands(case)
        ref, Ab, tiny = G.reference(case, opA, opB, C0)
        err = (torch.from_numpy(G.emulate(opA, opB, drop=drop)).double() - ref).abs() - tiny
        bad = err > G.C * G.EPS32 * Ab
        assert bool(bad.any()), (drop, case)
        if drop != "a1b1":
            assert bool(bad.all()), (drop, case, float(bad.double().mean()))


def test_randn_does_not_separate_a_dropped_low_product():
    """why the planted operands exist: on randn data the order-2^-16 mutants stay inside c"""
    case = G.make_case(0, 0, 33, 128, 256, 0.0, "randn", "cpu")
    opA, opB, C0 = G.operands(case)
    ref, Ab, tiny = G.reference(case, opA, opB, C0)
    for drop in ("a2b2", "a1b3", "a3b1"):
        assert G.worst_ratio(torch.from_numpy(G.emulate(opA, opB, drop=drop)), ref, Ab, tiny) <= G.C


def test_recorded_c32_covers_the_small_cases():
    """the fp32 yardstick re-measured on the planted, logmag and edge cases (the full measurement
    is `python tests/gemm_oracle.py`)"""
    cases = [c for c in G.all_cases() if c.M * c.N <= 129 * 256 and c.K <= 2049]
    assert len(cases) > 300
    assert max(G.c32_of(c) for c in cases) <= G.C32


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() \
        else 256          # num_cus() without a device


def test_work_floats_covers_every_mode():
    """pntf_tt_gemm_work_floats (a host function) equals its restatement and is at least what any
    panel / weight-gradient mode or the split-K path uses, for every case of this file"""
    lib, cus = _lib.load(), _cus()
    for c in G.all_cases(cus):
        got = int(lib.pntf_tt_gemm_work_floats(c.M, c.N, c.K))
        assert got == G.work_floats(c.M, c.N, c.K, cus), c
        assert got >= G.work_needed(c, cus), c
    assert lib.pntf_tt_gemm_work_floats(0, 128, 5) == 0


def test_mode_setters_ignore_out_of_range_values():
    lib = _lib.load()
    for fn, hi in ((lib.pntf_tt_set_panel_mode, 8), (lib.pntf_tt_set_wgrad_mode, 2),
                   (lib.pntf_tt_set_bwd_mode, 1)):
        prev = fn(-1)
        try:
            for bad in (-1, hi + 1, 1 << 20, -(1 << 31)):
                assert fn(bad) == prev
            assert fn(hi) == prev and fn(hi + 1) == hi and fn(0) == hi and fn(-7) == 0
        finally:
            fn(prev)
        assert fn(-1) == prev


# ------------------------------------------------------------------ GPU harness


def dev():
    return torch.device("cuda:0")


def vp(t, off=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + 4 * off)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


class Guarded:
    """`n` device floats filled with `fill` (at a float offset `mis` from an aligned address),
    1024 sentinel floats behind them"""

    def __init__(self, n, fill=NAN, mis=0):
        self.buf = torch.full((mis + n + SLACK,), SENT, device=dev())
        self.t = self.buf[mis:mis + n]
        self.t.fill_(fill)
        self.n, self.mis = n, mis

    def ptr(self):
        return vp(self.buf, self.mis)

    def slack_ok(self):
        return bool((self.buf[self.mis + self.n:] == SENT).all()) and \
            bool((self.buf[:self.mis] == SENT).all())


def matrix(x, ld, mis=0):
    """host (rows, cols) fp32 -> device rows of stride ld >= cols with NaN in the padding; returns
    (flat device buffer, pointer, bit copy)"""
    rows, cols = x.shape
    host = torch.full((rows, ld), NAN)
    host[:, :cols] = torch.from_numpy(x)
    buf = torch.full((mis + rows * ld,), NAN, device=dev())
    buf[mis:] = host.reshape(-1).to(dev())
    return buf, vp(buf, mis), buf.clone()


def run_case(lib, c, key, pads=(0, 0, 0), mis_a=0, mis_b=0, mis_work=0, short=0, repeat=1,
             expect=0):
    """one guarded pntf_tt_gemm call (`repeat` of them, bitwise equal) held to the bound; returns
    the worst ratio.  pads: floats added to the natural lda, ldb, ldc; short: floats taken off the
    work buffer; expect: the status the call must return (a failing call must leave C alone)"""
    opA, opB, C0 = G.operands(c)
    ref, Ab, tiny = G.reference(c, opA, opB, C0)
    sA = np.ascontiguousarray(opA.T) if c.ta else opA
    sB = np.ascontiguousarray(opB.T) if c.tb else opB
    lda, ldb, ldc = sA.shape[1] + pads[0], sB.shape[1] + pads[1], c.N + pads[2]
    dA, pA, kA = matrix(sA, lda, mis_a)
    dB, pB, kB = matrix(sB, ldb, mis_b)
    nw = int(lib.pntf_tt_gemm_work_floats(c.M, c.N, c.K)) - short
    first = None
    for _ in range(repeat):
        Cb = Guarded(c.M * ldc)
        Cv = Cb.t.view(c.M, ldc)
        if C0 is not None:
            Cv[:, :c.N] = torch.from_numpy(C0).to(dev())
        work = Guarded(nw, mis=mis_work) if nw > 0 else None
        st = lib.pntf_tt_gemm(c.ta, c.tb, c.M, c.N, c.K, pA, lda, pB, ldb, Cb.ptr(), ldc, c.beta,
                              work.ptr() if work else None, max(nw, 0), stream())
        torch.cuda.synchronize()
        assert st == expect, (c, st, lib.pntf_tt_gemm_last_error())
        assert Cb.slack_ok(), ("wrote past C", c)
        assert work is None or work.slack_ok(), ("wrote past work", c)
        assert same_bits(dA, kA) and same_bits(dB, kB), ("an operand changed", c)
        assert bool(torch.isnan(Cv[:, c.N:]).all()), ("C's padding written", c)
        got = Cv[:, :c.N]
        if expect != 0:
            assert bool(torch.isnan(got).all()) if C0 is None else \
                same_bits(got.contiguous(), torch.from_numpy(C0).to(dev())), ("C touched", c)
            return 0.0
        assert not bool(torch.isnan(got).any()), ("NaN in the result", c)
        if first is None:
            first = got.contiguous()
        else:
            assert same_bits(first, got.contiguous()), ("two runs differ", c)
    r = G.worst_ratio(first, ref.to(dev()), Ab.to(dev()), tiny)
    RATIO[key] = max(RATIO.get(key, 0.0), r)
    print("ratio %-18s %8.3f  %s" % (key, r, tuple(c)))
    assert r <= G.C, (key, c, r)
    return r


class modes:
    """set the panel / weight-gradient modes for a block and restore them"""

    def __init__(self, lib, panel=None, wgrad=None):
        self.lib, self.panel, self.wgrad = lib, panel, wgrad

    def __enter__(self):
        self.p0 = self.lib.pntf_tt_set_panel_mode(-1 if self.panel is None else self.panel)
        self.w0 = self.lib.pntf_tt_set_wgrad_mode(-1 if self.wgrad is None else self.wgrad)

    def __exit__(self, *exc):
        self.lib.pntf_tt_set_panel_mode(self.p0)
        self.lib.pntf_tt_set_wgrad_mode(self.w0)


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for k in sorted(RATIO):
        print("worst ratio %-18s %.3f  (c = %.1f)" % (k, RATIO[k], G.C))


def pkey(mode):
    return "%s/m%d" % (G.PANEL_ENGINE[mode], mode)


def wkey(mode):
    return "%s/w%d" % (G.WGRAD_ENGINE[mode], mode)


# ------------------------------------------------------------------ panel path


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", G.KN)
@pytest.mark.parametrize("mode", (0,) + G.PANEL_MODES)
def test_panel_rows(mode, K, N):
    """ta = 0, K, N in {128, 256}: a single row, the 32-row tile edge, the 4-tile workgroup edge
    and grids rounded up to 8 with idle workgroups, beta 0 and 1, both tb; planted operands at
    M = 33; the wide dynamic range; mode 0 sends the shape to gemm_kernel"""
    lib = _lib.load()
    with modes(lib, panel=mode):
        for c in G.panel_cases(K, N):
            run_case(lib, c, pkey(mode))


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", G.KN)
@pytest.mark.parametrize("mode", G.PANEL_MODES)
def test_panel_second_round_of_tiles(mode, K, N):
    lib, cus = _lib.load(), _cus()
    c = G.panel_loop_case(mode, K, N, cus)
    grid = G.panel_grid(mode, c.M, N, K, c.beta, cus)
    assert grid.rounds == 2 and G.ceil_div(c.M, 128) == grid.per_group + 1, (c, grid)
    with modes(lib, panel=mode):
        run_case(lib, c, pkey(mode))


@pytest.mark.gpu
@pytest.mark.parametrize("K,N", G.KN)
@pytest.mark.parametrize("mode", (0,) + G.PANEL_MODES)
def test_panel_padded_ldb(mode, K, N):
    """ldb above natural with NaN in B's padding, both tb (the pack kernels read B by ldb)"""
    lib = _lib.load()
    with modes(lib, panel=mode):
        for c in G.panel_ldb_cases(K, N):
            run_case(lib, c, pkey(mode), pads=(0, 4 + 8 * c.tb, 0))


# ------------------------------------------------------------------ weight-gradient path


@pytest.mark.gpu
@pytest.mark.parametrize("M,N", G.KN)
@pytest.mark.parametrize("mode", (0, 1, 2))
def test_wgrad_reduction_lengths(mode, M, N):
    """ta = 1, tb = 0, beta = 0, M, N in {128, 256}: K from 1 across the 16-row chunk and the
    128- / 256-row split edges; T >= 2: a K whose XCD padding launches empty splits; T = 1: more
    than 32 splits (a second gemm_reduce1 group); planted operands at K = 256 and at the
    empty-split K; each call twice with equal bits"""
    lib, cus = _lib.load(), _cus()
    T = (M // 128) * (N // 128)
    ke, kg = G.wgrad_k_empty(T, cus), G.wgrad_k_groups()
    if T >= 2:
        plan = G.wgrad_plan(M, N, ke, cus)
        assert plan.xcd and plan.empty > 0 and plan.real >= 8 and plan.last_rows == 1, plan
    else:
        assert G.wgrad_plan(M, N, kg, cus).real > G.RG
        assert G.splits_for(M, N, kg, cus) > G.RG
    assert G.wgrad_plan(M, N, 257, cus).last_rows == 1        # a last split ragged by one row
    with modes(lib, wgrad=mode):
        for c in G.wgrad_cases(M, N, cus):
            run_case(lib, c, wkey(mode), repeat=2)


# ------------------------------------------------------------------ LDS-tiled kernel


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_lds_tiled_forms(ta, tb):
    """all four (ta, tb) forms at K = 1, BK - 1, BK, BK + 1, 64, 77, a split-K length and one with
    more than 32 splits; M = 1, a full tile, one row past it and a ragged second tile; N of one
    and three tiles; beta 0, 0.5, 1"""
    lib, cus = _lib.load(), _cus()
    ks = G.lds_k_split(cus)
    assert G.splits_for(200, 384, ks, cus) > 1 and G.splits_for(1, 128, ks, cus) > 1
    assert G.splits_for(130, 128, G.RG * 512 + 1, cus) > G.RG
    for c in G.lds_cases(ta, tb, cus):
        assert not (G.panel_shape(c.N, c.K) and not ta) and not (ta and G.wgrad_shape(c.M, c.N))
        run_case(lib, c, "gemm_kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("ta,tb", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_lds_tiled_padded_strides(ta, tb):
    """lda, ldb and ldc above natural (odd float counts as well), NaN in every padding; C's
    padding must still be NaN"""
    lib = _lib.load()
    for i, c in enumerate(G.lds_pad_cases(ta, tb)):
        run_case(lib, c, "gemm_kernel", pads=((4, 8, 12), (1, 3, 5), (8, 4, 1))[i])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["A", "work", "B"])
def test_misaligned_operands_fall_back(what):
    """the panel and weight-gradient paths need 16-byte aligned A (B) and work; 4 bytes off, the
    LDS-tiled kernel serves the shape, under every mode"""
    lib = _lib.load()
    for c in G.lds_fallback_cases():
        if what == "B" and not c.ta:
            continue
        for pm, wm in ((3, 2), (2, 1), (8, 2)):
            with modes(lib, panel=pm, wgrad=wm):
                run_case(lib, c, "gemm_kernel", mis_a=what == "A", mis_b=what == "B",
                         mis_work=what == "work")


# ------------------------------------------------------------------ workspace contract


@pytest.mark.gpu
def test_work_one_float_short():
    """one float short of pntf_tt_gemm_work_floats: the split-K path refuses with
    PNTF_ERR_WORKSPACE and leaves C alone; a panel shape runs the LDS-tiled kernel instead (K <=
    256 never splits) and stays correct (include/pntf.h)"""
    lib, cus = _lib.load(), _cus()
    c = G.make_case(0, 1, 77, 128, G.lds_k_split(cus), 0.0, "randn", "short")
    assert G.work_floats(c.M, c.N, c.K, cus) == G.splits_for(c.M, c.N, c.K, cus) * c.M * c.N
    run_case(lib, c, "gemm_kernel", short=1, expect=ERR_WORKSPACE)
    run_case(lib, c._replace(beta=1.0), "gemm_kernel", short=1, expect=ERR_WORKSPACE)
    for K, N in G.KN:
        assert G.work_floats(77, N, K, cus) == G.panel_pack_floats(3, N, K)
        with modes(lib, panel=3):
            run_case(lib, G.make_case(0, 1, 77, N, K, 0.0, "randn", "short"), "gemm_kernel", short=1)
    # the weight-gradient path needs its launched splits only, fewer than the size's 7 spare
    # ones: one float short it still runs
    c = G.make_case(1, 0, 128, 128, 4096, 0.0, "randn", "short")
    with modes(lib, wgrad=2):
        run_case(lib, c, wkey(2), short=1)


# ------------------------------------------------------------------ dispatch


def _engines_run(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    found = set()
    for n in names:
        m = re.search(r"(?<![A-Za-z0-9_])(gemm_kernel|panel_gemm_kernel|panel_lds_kernel|"
                      r"panel_x6_kernel|panel_x6s_kernel|wgrad_kernel|wgrad_x6_kernel)(?![A-Za-z0-9_])", n)
        if m:
            found.add(m.group(1))
    return found, names


DISPATCH = [("panel", m, G.PANEL_ENGINE[m]) for m in (0,) + G.PANEL_MODES] + \
           [("wgrad", m, G.WGRAD_ENGINE[m]) for m in (0, 1, 2)] + [("lds", 0, "gemm_kernel")]


@pytest.mark.gpu
@pytest.mark.parametrize("path,mode,engine", DISPATCH)
def test_dispatch_runs_the_named_engine(path, mode, engine):
    """the accuracy cases above reach the engine they name, not the fallback: a profiled
    representative call (the harness of every other test) launches that kernel and no other
    GEMM engine"""
    lib, cus = _lib.load(), _cus()
    if path == "panel":
        c, ctx = G.panel_cases(256, 256)[3], modes(lib, panel=mode)
    elif path == "wgrad":
        c, ctx = G.wgrad_cases(256, 128, cus)[-1], modes(lib, wgrad=mode)
    else:
        c, ctx = G.lds_cases(1, 1, cus)[5], modes(lib)
    with ctx:
        found, names = _engines_run(lambda: run_case(lib, c, "dispatch"))
    assert found == {engine}, (found, names)
    assert not any("Cijk" in n for n in names), names


# ------------------------------------------------------------------ fused Linear + act


@pytest.mark.gpu
@pytest.mark.parametrize("k,n", G.KN)
def test_linear_act_identity_planted(k, n):
    """the planted operands through pntf_tt_linear_act with act = 0, no residual, a zero bias and
    one plane (y = x·Wᵀ): schedules 1 and 3 (the fused fp32-MFMA kernels) and 2 (the GEMM + act
    pair under the default panel mode); h is not written"""
    lib = _lib.load()
    for c in G.fused_cases():
        if (c.K, c.N) != (k, n):
            continue
        opA, opB, _ = G.operands(c)
        ref, Ab, tiny = G.reference(c, opA, opB, None)
        dx, px, kx = matrix(opA, k)
        dW, pW, kW = matrix(np.ascontiguousarray(opB.T), k)
        bias = torch.zeros(n, device=dev())
        nw = int(lib.pntf_tt_gemm_work_floats(c.M, n, k))
        for sched in (1, 2, 3):
            y, h, work = Guarded(c.M * n), Guarded(c.M * n), Guarded(nw)
            st = lib.pntf_tt_linear_act(0, 0, px, c.M, k, pW, n, vp(bias), None, y.ptr(), h.ptr(), 0,
                                        sched, work.ptr(), nw, stream())
            torch.cuda.synchronize()
            assert st == 0, (lib.pntf_tt_gemm_last_error(), lib.pntf_tt_last_error())
            assert y.slack_ok() and h.slack_ok() and work.slack_ok()
            assert same_bits(dx, kx) and same_bits(dW, kW) and bool((bias == 0).all())
            assert bool(torch.isnan(h.t).all()), "h written at act = 0"
            got = y.t.view(c.M, n)
            assert not bool(torch.isnan(got).any())
            r = G.worst_ratio(got, ref.to(dev()), Ab.to(dev()), tiny)
            key = "linear_act/s%d" % sched
            RATIO[key] = max(RATIO.get(key, 0.0), r)
            print("ratio %-18s %8.3f  %s" % (key, r, tuple(c)))
            assert r <= G.C, (key, c, r)
