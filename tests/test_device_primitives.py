"""The fused kernels' __device__ primitives, one by one, against fp64 ("Device
primitives, one by one").

field_kernel, field_split_kernel, field_quad_kernel, wide_field_kernel (the headline), the plan
kernels and the Taylor residual_kernel reach these functions only through whole 13-layer
networks, where the suite holds them to 1e-4 per pair.  tests/prim_probe.hip calls them from
tiny test-only kernels with no network around them; it includes the project headers as
csrc/pntf_kernels.hip does and is compiled here, once per session, with the shipped wide unit's
flags and defines (build.UNITS "wide_d3_k1": -DPNTF_RING_NL=6, which pntf_wide.h needs; the
residual unit's primitives nx6_split / nx6_mma depend on no define), so the functions under test
are the ones the kernels inline.  tests/prim_oracle.py holds the references, bound forms and
inputs.

What is asserted:
  * activations (sp_sig, sig10, wsp_sig, smooth_merge, head_sig): |got - ref64| <= c·eps32·A +
    tiny, c = 4·c32 clamped to [8, 64]; sp == y bit for bit wherever 10y > 20; σ in [0, 1];
    σ(y) + σ(-y) within 2 eps32 of 1; nothing but finite numbers from finite inputs — at ±0, the
    torch threshold, the exp2 underflow points, the smallest normal, a denormal, 1e-6..1e4;
  * sincos_fast: the bound with A = 1 + |q| and s² + c² = 1 to the matching bound inside
    |q| <= Q, Q found on the CPU from the reduction in exact arithmetic (and pinned: 2^24);
    beyond Q only finite values in [-1, 1];
  * wx6_split / nx6_split: every term equals gemm_oracle.split3 bit for bit;
  * wx6_mma / nx6_mma: C + W·X to c·eps32·(|W|·|X| + |C|) + tiny on operands planted so that each
    of the six products, if dropped, is a gross error in every element — which
    test_planted_cases_expose_every_dropped_product proves on the CPU with the emulation.

The probe tests the primitives, not each layer's use of them: a layer that skipped a split term
in xlayer or taylor_layer_x6 still needs the whole-network goldens.

Measured (MI355X; `python tests/prim_oracle.py` re-measures c32; DESIGN.md §4 has the table with
the code mutants):

    primitive                      c32 (CPU fp32)   c     worst ratio on MI355X
    σ(10y): sp_sig, sig10, wsp_sig   0.979          8     1.21
    softplus10: sp_sig, wsp_sig      0.620          8     0.82 (450140 before the log1p fix)
    merge s0 / M, m                  0.979 / 0.744  8     1.21 / 0.99 (450140 before the fix)
    head_sig                         0.978          8     1.10
    sincos_fast sin / cos            0.176 / 0.297  8     0.70 / 0.89
    wx6_mma                          2.38           9.6   3.39
    nx6_mma                          1.71           8     5.92
"""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import gemm_oracle as G
import prim_oracle as P

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE_SRC = os.path.join(HERE, "prim_probe.hip")
EPS, TINY = P.EPS32, P.TINY32
RATIO = {}          # what -> worst ratio seen (printed for DESIGN.md's table)

gpu = pytest.mark.gpu


# ------------------------------------------------------------------ building the probe


def probe_command(out):
    """hipcc line of the probe: the library's flags (without the listing / remark options, as the
    variant builds of test_capi_host.py) and the defines of the shipped wide τ+∇τ unit"""
    from pntf import build
    defs, = [d for name, _, d in build.UNITS if name == "wide_d3_k1"]
    flags = [f for f in build.CXXFLAGS if not f.startswith(("-save-temps", "-Rpass"))]
    return [build.hipcc()] + flags + defs + ["-shared", PROBE_SRC, "-o", out]


@pytest.fixture(scope="session")
def probe_path(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("prim_probe") / "libprim_probe.so")
    r = subprocess.run(probe_command(out), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def test_probe_compiles_for_gfx950(probe_path):
    """Not a GPU test: the probe includes pntf_field.h / pntf_wide.h / pntf_taylor.h and calls
    their primitives by name, so a header change that breaks the coupling fails here, where the
    code is written, and not first on the GPU."""
    from pntf import build
    assert "--offload-arch=gfx950" in probe_command("x") and "-DPNTF_RING_NL=6" in probe_command("x")
    assert os.path.getsize(probe_path) > 0
    with open(probe_path, "rb") as fh:
        blob = fh.read()
    assert build.ARCH.encode() in blob                       # a gfx950 code object is inside
    for sym in (b"probe_sp_sig", b"probe_sig10", b"probe_wsp_sig", b"probe_merge", b"probe_head",
                b"probe_sincos", b"probe_wx6", b"probe_nx6"):
        assert sym in blob, sym


class Probe:
    """the loaded probe; every call takes fp32 numpy arrays and returns fp32 numpy arrays"""

    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.dev = torch.device("cuda:0")
        kinv = self.lib.probe_wide_kappa_inv
        kap = self.lib.probe_wide_kappa
        kinv.restype = kap.restype = ctypes.c_float
        # the constants the oracle assumes are the kernels'
        assert kap() == np.float32(P.KAPPA32) and kinv() == np.float32(P.KAPPA_INV32)

    def _up(self, a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)

    def _call(self, name, ins, n_out, out_shape, *scalars):
        ins = [self._up(a) for a in ins]
        outs = [torch.full(out_shape, float("nan"), dtype=torch.float32, device=self.dev)
                for _ in range(n_out)]
        torch.cuda.synchronize()
        args = [ctypes.c_void_p(t.data_ptr()) for t in ins + outs] + [ctypes.c_int(s) for s in scalars]
        err = getattr(self.lib, name)(*args)
        assert err == 0, (name, "hip error", err)
        return [t.cpu().numpy() for t in outs]

    def ew(self, name, n_out, *ins):
        n = len(ins[0])
        assert n <= 65536 and all(len(a) == n and a.dtype == np.float32 for a in ins)
        return self._call(name, ins, n_out, (n,), n)

    def x6(self, kind, W, X, C, S):
        M, kb = P.GEOM[kind]
        assert W.shape == (M, kb * S) and X.shape == (kb * S, M) and C.shape == (M, M)
        terms, out = self._call("probe_" + kind, P.a_operand(kind, W, S) + [X, C], 2,
                                (3 * kb * S * M,), S)
        return terms.reshape(3, kb * S, M), out[:M * M].reshape(M, M)


@pytest.fixture(scope="session")
def probe(probe_path):
    return Probe(probe_path)


# ------------------------------------------------------------------ holding a result


def hold(what, got, ref, A, c):
    r = P.ratio(got, ref, A)
    worst = float(r.max())
    at = int(r.argmax())
    RATIO[what] = max(RATIO.get(what, 0.0), worst)
    print("RATIO %s %.3f (c = %.1f) at element %d" % (what, worst, c, at))
    assert worst <= c, (what, worst, c, at, float(torch.as_tensor(got).reshape(-1)[at]),
                        float(ref.reshape(-1)[at]))


def finite(what, *arrs):
    for a in arrs:
        assert np.isfinite(a).all(), (what, "NaN or inf from a finite input")


def sigma_properties(what, sg, nb):
    """σ in [0, 1], and σ(y) + σ(-y) within 2 eps32 of 1 (elements i, i + nb are y, -y)"""
    assert (sg >= 0.0).all() and (sg <= 1.0).all(), what
    s = sg[:nb].astype(np.float64) + sg[nb:2 * nb].astype(np.float64)
    w = float(np.abs(s - 1.0).max())
    print("SYMM %s %.3f eps32" % (what, w / EPS))
    assert w <= 2.0 * EPS, (what, w / EPS)


def c_of(fn, *xs):
    """name -> c = 4·c32 within [8, 64], c32 from the float32 evaluation on the CPU"""
    c32 = P.c32_of(fn, *xs)
    print("C32 %s %s" % (fn.__name__, {k: round(v, 3) for k, v in c32.items()}))
    return {k: P.clamp_c(v) for k, v in c32.items()}


# ------------------------------------------------------------------ activations


@pytest.fixture(scope="module")
def act():
    y, nb = P.act_inputs()
    return y, nb, P.evaluate(P.ref_sp_sig, "bd", y), c_of(P.ref_sp_sig, y)


def test_inputs_cover_the_edges():
    """the inputs hold what the tests claim: ±0, the threshold and its neighbours, both exp2
    underflow points, the smallest normal, a denormal, 1e-6..1e4 in both signs, and a ragged
    final wave whose last lane is planted"""
    y, nb = P.act_inputs()
    assert len(y) <= 65536 and len(y) % 64 == 37 and y[-1] == np.nextafter(np.float32(2), np.float32(3))
    assert (y[nb:2 * nb] == -y[:nb]).all()
    a = np.abs(y)
    for v in (0.0, 2.0, P.TINY32, 1e-40) + tuple(P.Y_UNDERFLOW) + (P.Y_ONE,):
        assert (a == np.float32(v)).any(), v
    assert np.signbit(y[y == 0]).any() and not np.signbit(y[y == 0]).all()
    assert ((a > 0) & (a < TINY)).any() and a.max() > 9e3 and a[a > TINY].min() < 2e-6
    assert ((y > np.float32(2)) & (y < np.float32(2.00001))).sum() >= 8
    x = 10.0 * a.astype(np.float64) / P.LN2
    assert ((x > 125.9) & (x < 126)).any() and ((x > 126) & (x < 126.1)).any()
    assert ((x > 148.9) & (x < 149)).any() and ((x > 149) & (x < 149.1)).any()
    zs, zg = P.merge_inputs()
    assert len(zs) <= 65536 and len(zs) % 64 == 37 and (zs == zg).sum() > 100
    assert max(np.abs(zs).max(), np.abs(zg).max()) >= 100.0


@gpu
def test_sp_sig(probe, act):
    """σ to its bound, the threshold, finiteness (the softplus value: test_sp_sig_softplus_bound)"""
    y, nb, bd, c = act
    sp, sg = probe.ew("probe_sp_sig", 2, y)
    finite("sp_sig", sp, sg)
    hold("sp_sig.sg", sg, *bd["sg"], c["sg"])
    over = 10.0 * y.astype(np.float64) > 20.0
    assert over.sum() > 1000
    assert (sp[over].view(np.uint32) == y[over].view(np.uint32)).all(), "sp != y above the threshold"
    sigma_properties("sp_sig.sg", sg, nb)
    assert (sp >= 0.0).all()


@gpu
def test_sp_sig_softplus_bound(probe, act):
    """Regression case of the bug this file found.  softplus10(y) = max(y, 0) + log(1 + t)/10,
    t = e^{-10|y|}, was evaluated as v_log of fl(1 + t) alone (sp_sig, wsp_sig, log1p_small in
    the merge): the rounding of 1 + t is an absolute 2^-24 in the log, 5.96e-9 in softplus10,
    and for y < 0, where the value is the log term alone, a relative error.  Measured before the
    fix: worst ratio 450140.5 (c = 8) at y = -1.6635532 (t = 2^-24, where 1 + t first rounds to
    1): 0 for 5.96e-9; every y < -1.6636 gave exactly 0, and 1847 of the 32165 inputs,
    -8.49 <= y <= -0.479, were outside the bound.  The fix adds the rounding error of 1 + t back
    (pntf_field.h one_plus_err)."""
    y, nb, bd, c = act
    sp, _ = probe.ew("probe_sp_sig", 2, y)
    bad = y[(P.ratio(sp, *bd["sp"]) > c["sp"]).numpy()]
    if len(bad):
        print("OUTSIDE sp_sig.sp: %d of %d inputs, y from %.7g to %.7g" % (
            len(bad), len(y), bad.min(), bad.max()))
    hold("sp_sig.sp", sp, *bd["sp"], c["sp"])


@gpu
def test_sig10(probe, act):
    y, nb, bd, c = act
    sg, = probe.ew("probe_sig10", 1, y)
    finite("sig10", sg)
    hold("sig10", sg, *bd["sg"], c["sg"])
    sigma_properties("sig10", sg, nb)
    sg2 = probe.ew("probe_sp_sig", 2, y)[1]
    assert (sg.view(np.uint32) == sg2.view(np.uint32)).all()      # one formula, two spellings


def _wsp(probe, y):
    yk = (y * np.float32(P.KAPPA32)).astype(np.float32)
    assert np.isfinite(yk).all()
    spk, sg = probe.ew("probe_wsp_sig", 2, yk)
    return yk, spk, sg


@gpu
def test_wsp_sig(probe, act):
    """the wide kernels' activation takes y' = fl(κ·y) and returns κ·softplus10(y) and σ(10y);
    the rounding of κ·y is the 10|y| term of A.  (The softplus value:
    test_wsp_sig_softplus_bound.)"""
    y, nb, bd, c = act
    yk, spk, sg = _wsp(probe, y)
    finite("wsp_sig", spk, sg)
    hold("wsp_sig.sg", sg, *bd["sg"], c["sg"])
    one = yk.astype(np.float64) >= 24.0          # 1 + 2^-y' rounds to 1: sp' is y' itself
    assert one.sum() > 1000 and (spk[one].view(np.uint32) == yk[one].view(np.uint32)).all()
    sigma_properties("wsp_sig.sg", sg, nb)
    assert (spk >= 0.0).all()


@gpu
def test_wsp_sig_softplus_bound(probe, act):
    """the same regression case for the wide kernels' activation (log2 of fl(1 + 2^-|y'|)): before
    the fix, worst ratio 450140.5 (c = 8) at y = -1.6635532, 0 for 5.96e-9"""
    y, nb, bd, c = act
    yk, spk, _ = _wsp(probe, y)
    hold("wsp_sig.sp", spk.astype(np.float64) * P.KAPPA_INV32, *bd["sp"], c["sp"])


@pytest.fixture(scope="module")
def mrg():
    zs, zg = P.merge_inputs()
    return zs, zg, P.evaluate(P.ref_merge, "bd", zs, zg), c_of(P.ref_merge, zs, zg)


@gpu
def test_merge(probe, mrg):
    """the switch to its bound and the symmetries (max / min: test_merge_max_min_bound)"""
    zs, zg, bd, c = mrg
    M, m, s0 = probe.ew("probe_merge", 3, zs, zg)
    finite("merge", M, m, s0)
    hold("merge.s0", s0, *bd["s0"], c["s0"])
    assert (s0 >= 0.0).all() and (s0 <= 1.0).all()
    eq = zs == zg
    assert (s0[eq] == 0.5).all()
    # the arguments swapped: the same max and min, the complementary switch
    M2, m2, s02 = probe.ew("probe_merge", 3, zg, zs)
    assert (M2.view(np.uint32) == M.view(np.uint32)).all() and (m2.view(np.uint32) == m.view(np.uint32)).all()
    assert float(np.abs(s0.astype(np.float64) + s02 - 1.0).max()) <= 2.0 * EPS


@gpu
def test_merge_max_min_bound(probe, mrg):
    """the same regression case in the merge: where max(zs, zg) (or min) is 0 or tiny,
    M = max + log1p(e^{-10|d|})/10 is the log term alone.  Before the fix: worst ratio 450140.5
    (c = 8) at zs = -1.6635532, zg = 0, M = 0 for 5.96e-9."""
    zs, zg, bd, c = mrg
    M, m, _ = probe.ew("probe_merge", 3, zs, zg)
    hold("merge.M", M, *bd["M"], c["M"])
    hold("merge.m", m, *bd["m"], c["m"])


@gpu
def test_head_sigmoid(probe):
    """σ(0.1·y4): the same arguments times 100, so 0.1|y| crosses the exp2 underflow (and, for
    y < 0, overflow) points"""
    y, nb = P.act_inputs(100.0)
    bd, c = P.evaluate(P.ref_head, "bd", y), c_of(P.ref_head, y)
    tau, = probe.ew("probe_head", 1, y)
    finite("head", tau)
    hold("head_sig", tau, *bd["tau"], c["tau"])
    sigma_properties("head_sig", tau, nb)


# ------------------------------------------------------------------ sincos_fast

Q_PINNED = 2.0 ** 24       # DESIGN.md §4 and the comment of sincos_fast (pntf_field.h)


@pytest.fixture(scope="module")
def domain():
    return P.sincos_domain()


def test_sincos_domain(domain):
    """The two-term Cody-Waite reduction evaluated in exact arithmetic, octave by octave: up to
    Q the reduced argument is within eps32·|q| of q - 2πk, |r| <= π + eps32·|q| (NOT π: q =
    fl(π) gives r = q > π) and |r| <= 3π/2; Q is what the documents say."""
    Q, rows = domain
    for j, over, rel, err in rows:
        print("octave 2^%-2d  (|r|-pi)/(eps32|q|) %9.3f  |r|/pi %.4f  err/(eps32|q|) %.3f"
              % (j, over, rel, err))
    assert Q == Q_PINNED
    assert P.workload_qmax() < 64.0 < Q                       # the workload is deep inside
    # the old claim |r| <= π fails at once, by ulps
    over, rel, err = P.reduction_figures(np.float32(math.pi))
    assert 0.0 < over <= 1.0 and err == 0.0
    # beyond Q the figure that breaks is |r| <= 3π/2 (k drifts off the nearest revolution)
    assert any(rel > 1.5 for j, _, rel, _ in rows if 2.0 ** j > Q)
    assert all(err <= 1.0 and over <= 1.0 for _, over, _, err in rows)


def test_sincos_inputs_cover_the_edges(domain):
    q, inside = P.sincos_inputs(domain[0])
    a = np.abs(q.astype(np.float64))
    assert len(q) <= 65536 and len(q) % 64 == 37 and q[-1] == np.float32(math.pi)
    assert ((a <= math.pi).sum() > 8000 and a.max() > 1e38 and (a == 1e5).any()
            and (~inside).sum() >= 400)
    qm = P.workload_qmax()
    assert 10.0 < qm < 64.0 and ((a > 0.9 * qm) & (a <= qm)).any()
    for m in (1, 2, 3, 4, 63, 64):
        assert (q == np.float32(m * math.pi / 2)).any()


@gpu
def test_sincos_fast(probe, domain):
    Q = domain[0]
    q, inside = P.sincos_inputs(Q)
    s, c = probe.ew("probe_sincos", 2, q)
    finite("sincos", s, c)
    assert (np.abs(s) <= 1.0).all() and (np.abs(c) <= 1.0).all()      # everywhere, beyond Q too
    qi = q[inside]
    bd, cc = P.evaluate(P.ref_sincos, "bd", qi), c_of(P.ref_sincos, qi)
    hold("sincos.s", s[inside], *bd["s"], cc["s"])
    hold("sincos.c", c[inside], *bd["c"], cc["c"])
    # s = s0 + es, c = c0 + ec with |es|, |ec| <= E = c·eps32·A:  |s² + c² - 1| = |2 (s0 es + c0 ec)
    # + es² + ec²| <= 2·sqrt(2)·E + 2 E²
    E = max(cc.values()) * EPS * (1.0 + np.abs(qi.astype(np.float64)))
    unit = np.abs(s[inside].astype(np.float64) ** 2 + c[inside].astype(np.float64) ** 2 - 1.0)
    print("UNIT sincos %.3f of its bound" % float((unit / (2 * math.sqrt(2) * E + 2 * E * E)).max()))
    assert (unit <= 2 * math.sqrt(2) * E + 2 * E * E).all()
    # in the workload's range the error, in absolute terms
    w = np.abs(qi.astype(np.float64)) <= P.workload_qmax()
    print("ABS sincos |q| <= %.2f: %.3e" % (P.workload_qmax(), max(
        float((torch.from_numpy(s[inside][w]).double() - bd["s"][0][w]).abs().max()),
        float((torch.from_numpy(c[inside][w]).double() - bd["c"][0][w]).abs().max()))))


# ------------------------------------------------------------------ split-bf16: the condition


@pytest.fixture(scope="module")
def c_x6():
    out = {}
    for kind in P.GEOM:
        c32 = P.product_c32(kind)
        out[kind] = P.clamp_c(c32)
        print("C32 %s %.3f -> c = %.1f" % (kind, c32, out[kind]))
    return out


@pytest.mark.parametrize("kind", list(P.GEOM))
def test_planted_cases_expose_every_dropped_product(kind, c_x6):
    """The condition the GPU product tests rest on, on the CPU with gemm_oracle.emulate: on every
    planted case the six-product scheme stays inside c in every element, and with any one product
    left out every element of that product's case is outside c."""
    c = c_x6[kind]
    for S in P.S_BLOCKS:
        for target in P.TARGETS6:
            for with_c in (False, True):
                W, X, C = P.product_operands(kind, target, S, with_c)
                ref, Ab, tiny = P.product_reference(W, X, C)
                full = torch.from_numpy(C + G.emulate(W, X))
                assert G.worst_ratio(full, ref, Ab, tiny) <= c, (S, target, with_c)
                mut = torch.from_numpy(C + G.emulate(W, X, drop=target))
                err = ((mut.double() - ref).abs() - tiny) / (EPS * Ab)
                assert float(err.min()) > c, (S, target, with_c, float(err.min()), c)


def test_a_operand_layout_is_the_packed_one():
    """the k order the tests feed the probe is the one tests/test_x6_pack.py pins for the packed
    weights: wide, element i of lane l in block b of a 32-feature tile is feature (i & 3) + 16 b +
    8 (i >> 2) + 4 (l >> 5); narrow, 16 (2 b + (i >> 2)) + 4 (l >> 4) + (i & 3); every column of
    a block appears once per row"""
    for kind, (M, kb) in P.GEOM.items():
        cols, rows = P.a_operand_cols(kind, 2)
        for B in range(2):
            for r in range(M):
                got = np.sort(cols[B][rows == r].reshape(-1))
                assert (got == np.arange(kb * B, kb * (B + 1))).all(), (kind, B, r)
    cols, _ = P.a_operand_cols("wx6", 2)
    assert cols[1, 37, 5] == (5 & 3) + 16 + 8 * (5 >> 2) + 4 * (37 >> 5)
    cols, _ = P.a_operand_cols("nx6", 2)
    assert cols[1, 37, 5] == 16 * (2 + (5 >> 2)) + 4 * (37 >> 4) + (5 & 3)


# ------------------------------------------------------------------ split-bf16: on the device


def check_terms(what, terms, X):
    want = G.split3(X)
    for p in range(3):
        assert (terms[p].view(np.uint32) == want[p].view(np.uint32)).all(), (what, "term", p)
    exact = (want[0].astype(np.float64) + want[1] + want[2]) == X.astype(np.float64)
    got = terms[0].astype(np.float64) + terms[1] + terms[2]
    assert (got[exact] == X.astype(np.float64)[exact]).all(), what
    assert (terms[:, X == 0] == 0).all(), (what, "zeros")
    return exact


@gpu
@pytest.mark.parametrize("kind", list(P.GEOM))
def test_split_terms(probe, kind):
    M, kb = P.GEOM[kind]
    for S in (1, 16):
        W0, C0 = np.zeros((M, kb * S), np.float32), np.zeros((M, M), np.float32)
        for name, X in P.split_inputs(kind, S).items():
            terms, out = probe.x6(kind, W0, X, C0, S)
            exact = check_terms((kind, S, name), terms, X)
            assert (out == 0).all()
            if name in ("randn", "planted", "bf16"):
                assert exact.all(), (kind, S, name)
            if name == "bf16":
                assert (terms[1] == 0).all() and (terms[2] == 0).all()
            if name == "logmag":
                assert (X == 0).sum() > 0


@gpu
@pytest.mark.parametrize("kind", list(P.GEOM))
def test_split_products(probe, kind, c_x6):
    c = c_x6[kind]
    for data, S, with_c in P.product_cases():
        W, X, C = P.product_operands(kind, data, S, with_c)
        terms, out = probe.x6(kind, W, X, C, S)
        check_terms((kind, data, S), terms, X)
        ref, Ab, tiny = P.product_reference(W, X, C)
        r = G.worst_ratio(torch.from_numpy(out), ref, Ab, tiny)
        what = "%s.%s" % (kind, data if data in ("randn", "logmag") else "planted")
        RATIO[what] = max(RATIO.get(what, 0.0), r)
        print("RATIO %s_mma %s S=%d C=%d %.3f (c = %.1f)" % (kind, data, S, with_c, r, c))
        assert r <= c, (kind, data, S, with_c, r, c)
