"""CPU-side oracle of tests/test_device_primitives.py — TEST ONLY.  Nothing here touches a GPU.

The device primitives of the fused kernels (csrc/pntf_field.h sp_sig, sig10, smooth_merge,
head_sig, sincos_fast; pntf_wide.h wsp_sig, wx6_split, wx6_mma; pntf_taylor.h nx6_split,
nx6_mma) restated as plain functions, generic as tests/tape_oracle.py is: on torch.float64
they are the reference, on torch.float32 the yardstick c32 is measured with, and on `Bd` values
they give the first-order absolute-value bound form A.  A result holds when, elementwise,

    |got - ref64| <= c·EPS32·A + tiny,      tiny = TINY32·max(1, A)  (per element),

with c = 4·c32 clamped to [8, 64] (the rule and its reasons: tests/test_tape_kernels.py), c32 =
the worst err / (EPS32·A) of the float32 evaluation over every input of the test.

Elementwise references.  softplus10 has torch's threshold branch (y itself where 10y > 20);
σ(10y), σ(0.1y), the merge max + log1p(e^{-10|d|})/10 with its switch σ(10d), and sin / cos of
the fp32 q have no threshold tricks.  An input is exact (A = |x|); for sincos A = 1 + |q|: the
result is at most 1 and the reduction of q costs ulps of q.  wsp_sig takes y' = fl(κ·y): its
references are those of y, and the rounding of κ·y is the 10|y| term that σ(10y) and
softplus10(y) already carry in A.

The sincos reduction.  `reduce_exact` evaluates sincos_fast's three fp32 steps (k =
rint(fl(q·fl(1/2π))), r = fma(-k, fp32(2π), q), r = fma(-k, lo, r)) in exact rational arithmetic,
each rounded to fp32 once as the hardware does; `sincos_domain` scans octaves for the largest
Q = 2^j such that for every sample |q| <= Q
    |r| <= π + EPS32·|q|  and  |r| <= 3π/2      (k is the nearest revolution up to the
                                                  rounding of q/2π; never more than a quarter
                                                  turn off),
    |r - (q - 2πk)| <= EPS32·|q|                  (the reduction error).
The header's earlier claim |r| <= π is false from q = fl(π) on (k = 0, r = q > π); what holds
is the first line, which v_sin / v_cos (valid to ±256 revolutions) absorb.

Split-bf16.  The splits and the six products come from tests/gemm_oracle.py (split3, bf16_rne,
emulate, planted, worst_ratio); here are only the operand layouts of the two MFMAs and the
cases.  In gemm_oracle's naming a = the weights W (the MFMA's A operand), b = the activations X.
"""
import math
import zlib
from fractions import Fraction

import numpy as np
import torch

import gemm_oracle as G
import tape_oracle as T

EPS32 = 2.0 ** -23
TINY32 = 2.0 ** -126
F64, F32 = torch.float64, torch.float32
LN2 = math.log(2.0)
KAPPA32 = float(np.float32(10.0 / LN2))              # WIDE_KAPPA as the kernels hold it
KAPPA_INV32 = float(np.float32(LN2 / 10.0))          # WKAPPA_INV


def rng_of(*seed):
    return np.random.default_rng(zlib.crc32(repr(seed).encode()))


def clamp_c(c32):
    return min(64.0, max(8.0, 4.0 * c32))


# ------------------------------------------------------------------ elementwise references
# each returns a dict name -> value; x: torch tensors of a float dtype, or Bd


def ref_sp_sig(y):
    return {"sp": T.softplus10(y), "sg": T.sig10(y)}


def ref_sig10(y):
    return {"sg": T.sig10(y)}


def ref_merge(zs, zg):
    d = zs - zg
    lse = T._log1p(T._exp(-(T._abs(d) * T.SCALE))) / T.SCALE
    return {"M": T._max(zs, zg) + lse, "m": T._min(zs, zg) - lse, "s0": T.sig10(d)}


def ref_head(y):
    return {"tau": T._sigmoid(y * 0.1)}


def ref_sincos(q):
    if isinstance(q, T.Bd):
        A = 1.0 + q.v.abs()
        return {"s": T.Bd(torch.sin(q.v), A), "c": T.Bd(torch.cos(q.v), A)}
    return {"s": torch.sin(q), "c": torch.cos(q)}


def evaluate(fn, mode, *xs):
    """fn on fp32 numpy inputs: mode F64 / F32 -> dict of tensors; "bd" -> dict of (ref64, A)"""
    ts = [torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)) for x in xs]
    if mode == "bd":
        return {k: (v.v, v.A) for k, v in fn(*[T.Bd(t.double()) for t in ts]).items()}
    return fn(*[t.to(mode) for t in ts])


def ratio(got, ref, A):
    """elementwise (|got - ref| - tiny) / (EPS32·A), tiny = TINY32·max(1, A); inf where got is
    not finite"""
    got = torch.as_tensor(got).double().reshape(ref.shape)
    over = ((got - ref).abs() - TINY32 * A.clamp(min=1.0)).clamp(min=0.0)
    r = over / (EPS32 * A).clamp(min=1e-300)
    return torch.where(torch.isfinite(got), r, torch.full_like(r, float("inf")))


def c32_of(fn, *xs):
    """dict name -> worst ratio of the float32 evaluation on the CPU"""
    bd, r32 = evaluate(fn, "bd", *xs), evaluate(fn, F32, *xs)
    return {k: float(ratio(r32[k], *bd[k]).max()) for k in bd}


# ------------------------------------------------------------------ elementwise inputs


def neighbours(x, n):
    """x and its n fp32 neighbours on each side"""
    x = np.float32(x)
    out, lo, hi = [x], x, x
    for _ in range(n):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        out += [lo, hi]
    return np.array(out, dtype=np.float32)


def _ragged(x, plant):
    """at most 65536 values, a ragged final wave (length = 37 mod 64) with `plant` in its last
    lane"""
    x = np.asarray(x, dtype=np.float32)
    n = min(len(x), 65536 - 64)
    n -= (n - 36) % 64
    assert n % 64 == 36 and 0 < n <= len(x), (n, len(x))
    return np.concatenate([x[:n], np.array([plant], np.float32)])


# |y| at which exp2(-10|y|/ln 2) reaches 2^-126 (the smallest normal) and 2^-149 (the smallest
# denormal), and at which 1 + e^{-10|y|} starts to round to 1 (2^-24)
Y_UNDERFLOW = (126 * LN2 / 10, 149 * LN2 / 10)
Y_ONE = 24 * LN2 / 10


def act_base(scale=1.0):
    """planted magnitudes of an activation argument (times `scale`: the head's argument is 0.1 y
    where the activations' is 10 y), without signs"""
    rng = rng_of("act", scale)
    parts = [np.zeros(1, np.float32), neighbours(2.0 * scale, 8), neighbours(Y_ONE * scale, 8),
             np.array([TINY32, 1e-40, 2.0 ** -149], np.float32)]
    for y in Y_UNDERFLOW + (128 * LN2 / 10,):        # 128: exp2 of the opposite sign overflows
        parts.append(neighbours(y * scale, 8))
    parts.append(np.power(10.0, rng.uniform(-6.0, 4.0, 16000)).astype(np.float32) * np.float32(scale))
    return np.concatenate(parts)


def act_inputs(scale=1.0):
    """[base | -base | planted tail]: element i and i + len(base) are y and -y"""
    b = act_base(scale)
    b = b[:len(b) - (len(b) - 18) % 32]              # 2 len(b) = 36 mod 64: _ragged cuts nothing
    return _ragged(np.concatenate([b, -b]), np.nextafter(np.float32(2.0 * scale), np.float32(np.inf))), len(b)


def merge_inputs():
    """(zs, zg): zs == zg; zs - zg at the planted activation arguments around several zg; and
    magnitudes up to 1e2 at random"""
    rng = rng_of("merge")
    b = act_base()
    b = b[b <= 200.0]
    d = np.concatenate([b, -b])
    zs, zg = [], []
    eq = np.concatenate([np.array([0.0, -0.0, 1.0, -1.0, 100.0, -100.0, TINY32, 1e-40], np.float32),
                         np.power(10.0, rng.uniform(-6, 2, 500)).astype(np.float32)])
    zs.append(eq)
    zg.append(eq.copy())
    for g in (0.0, 0.37, -1.0, 3.0, -100.0, 64.0):
        g32 = np.full(d.shape, g, np.float32)
        zs.append((g32 + d).astype(np.float32))      # fl(zg + d): zs - zg is d up to its rounding
        zg.append(g32)
    mag = np.power(10.0, rng.uniform(-6, 2, (2, 8000))) * rng.choice([-1.0, 1.0], (2, 8000))
    zs.append(mag[0].astype(np.float32))
    zg.append(mag[1].astype(np.float32))
    near = np.power(10.0, rng.uniform(-3, 2, 4000)) * rng.choice([-1.0, 1.0], 4000)
    zs.append((near + rng.standard_normal(4000) * 0.3).astype(np.float32))
    zg.append(near.astype(np.float32))
    zs, zg = np.concatenate(zs), np.concatenate(zg)
    return _ragged(zs, 2.0), _ragged(zg, 0.0)


# ------------------------------------------------------------------ sincos_fast

PI = Fraction("3.14159265358979323846264338327950288419716939937510582097494459230781640628620899")
INV2PI32 = Fraction(float(np.float32(0.159154943091895336)))
C1_32 = Fraction(float(np.float32(6.28318548202514648)))
C2_32 = Fraction(float(np.float32(-1.74845553146951720e-7)))


def _rnd32(x):
    """a rational -> the nearest fp32 (ties to even, gradual underflow), as a rational"""
    if x == 0:
        return Fraction(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    u = Fraction(2) ** (max(e, -126) - 23)
    n = a / u
    fl = n.numerator // n.denominator
    rem = n - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2 == 1):
        fl += 1
    return fl * u if x > 0 else -fl * u


def reduce_exact(q):
    """sincos_fast's reduction of the fp32 q, each step rounded to fp32 once: (q, k, r) as
    rationals"""
    q = Fraction(float(np.float32(q)))
    k = Fraction(round(_rnd32(q * INV2PI32)))         # rintf: ties to even, as Python's round
    r = _rnd32(q - k * C1_32)                         # fmaf(-k, fp32(2π), q)
    r = _rnd32(r - k * C2_32)                         # fmaf(-k, lo, r)
    return q, k, r


def reduction_figures(q):
    """(|r| - π) / (EPS32·|q|), |r| / π, |r - (q - 2πk)| / (EPS32·|q|) of one fp32 q != 0"""
    q, k, r = reduce_exact(q)
    s = Fraction(EPS32) * abs(q)
    return float((abs(r) - PI) / s), float(abs(r) / PI), float(abs(r - (q - 2 * k * PI)) / s)


def _octave_samples(j, n, rng):
    """fp32 samples of [2^(j-1), 2^j]: uniform, and the half revolutions (where k switches) with
    their neighbours"""
    lo, hi = 2.0 ** (j - 1), 2.0 ** j
    qs = list(rng.uniform(lo, hi, n).astype(np.float32)) + [np.float32(hi)]
    m0, m1 = math.ceil(lo / (2 * math.pi) - 0.5), math.floor(hi / (2 * math.pi) - 0.5)
    if m1 >= m0 and m1 >= 0:
        for m in np.unique(rng.integers(max(m0, 0), m1 + 1, n // 4)):
            qs += list(neighbours((m + 0.5) * 2 * math.pi, 1))
    return [q for q in qs if lo <= q <= hi]


def sincos_domain(jmax=30, n=96):
    """(Q, rows): the largest Q = 2^j below which every sample meets the three conditions of the
    module header, and per octave j the worst of the three figures"""
    rng = rng_of("sincos-domain")
    rows, Q = [], None
    for j in range(2, jmax + 1):
        fig = np.array([reduction_figures(q) for q in _octave_samples(j, n, rng)])
        w = fig.max(axis=0)
        rows.append((j, float(w[0]), float(w[1]), float(w[2])))
        ok = w[0] <= 1.0 and w[1] <= 1.5 and w[2] <= 1.0
        if Q is None and not ok:
            Q = 2.0 ** (j - 1)
    return (2.0 ** jmax if Q is None else Q), rows


def workload_qmax():
    """the largest |2π·B·x| of the synthetic workload: x in the box [-0.5, 0.5]^dim, B from
    synth.make_B_table (dim 3 and 6)"""
    from pntf import synth
    return max(float(2 * math.pi * 0.5 * np.abs(synth.make_B_table(dim=dim).astype(np.float64))
                     .sum(axis=1).max()) for dim in (3, 6))


def sincos_inputs(Q):
    """(q, inside): fp32 arguments and the mask |q| <= Q"""
    rng = rng_of("sincos")
    qmax = workload_qmax()
    parts = [np.linspace(0.0, math.pi, 8192), np.array([0.0, -0.0, TINY32, 1e-40]),
             rng.uniform(-qmax, qmax, 8192),
             np.power(10.0, rng.uniform(-6, 5, 6000)) * rng.choice([-1.0, 1.0], 6000),
             np.array([1e5, -1e5, Q, -Q]),
             np.power(10.0, rng.uniform(math.log10(Q), 38.0, 500)) * rng.choice([-1.0, 1.0], 500),
             np.array([3.0e38, -3.0e38])]
    ms = np.concatenate([np.arange(1, 65), rng.integers(65, int(1e5 / (math.pi / 2)), 400)])
    for m in ms:                                            # multiples of π/2 (2π among them)
        nb = neighbours(m * (math.pi / 2), 2)
        parts += [nb, -nb]
    parts.append(np.concatenate([neighbours(m * 2 * math.pi, 2) for m in (1, 2, 3, 100, 1000, 15915)]))
    q = _ragged(np.concatenate(parts).astype(np.float32), np.float32(math.pi))
    return q, np.abs(q.astype(np.float64)) <= Q


# ------------------------------------------------------------------ split-bf16 layouts and cases
# W (M, K) weights, X (K, N) activations, C (M, N).  kind "wx6": v_mfma_f32_32x32x16_bf16, M = N =
# 32, k blocks of 16; "nx6": v_mfma_f32_16x16x32_bf16, M = N = 16, k blocks of 32.

GEOM = {"wx6": (32, 16), "nx6": (16, 32)}           # kind -> (M = N, features per k block)
S_BLOCKS = (1, 2, 8, 16)
TARGETS6 = G.PRODUCTS                               # a1b1 too: planted() builds it like the rest


def a_operand_cols(kind, S):
    """(S, 64, 8) column of W that element i of lane l holds in k block B, and (64,) its row"""
    l, i = np.arange(64)[:, None], np.arange(8)[None, :]
    B = np.arange(S)[:, None, None]
    if kind == "wx6":       # pntf_wide.h: the feature of register 8 b + i of lane half l >> 5
        return 16 * B + (i & 3) + 8 * (i >> 2) + 4 * (l >> 5), np.arange(64) & 31
    return 16 * (2 * B + (i >> 2)) + 4 * (l >> 4) + (i & 3), np.arange(64) & 15


def a_operand(kind, W, S):
    """the three bf16 terms of W as the MFMA's A operand in k-block order: 3 x (S, 64, 8) uint16"""
    cols, rows = a_operand_cols(kind, S)
    vals = W[rows[None, :, None], cols]
    return [np.ascontiguousarray((t.view(np.uint32) >> 16).astype(np.uint16))
            for t in G.split3(np.ascontiguousarray(vals))]


def product_operands(kind, data, S, with_c, *seed):
    """(W, X, C) fp32; data = "randn", "logmag" or a planted target of TARGETS6"""
    M, kb = GEOM[kind]
    K = kb * S
    if data == "randn":
        W, X = G.randn_pair(M, K, M, kind, *seed)
    elif data == "logmag":
        W, X = G.logmag_pair(M, K, M, kind, *seed)
    else:
        W, X = G.planted(data, M, K, M, kind, *seed)
    C = np.zeros((M, M), np.float32)
    if with_c:
        s = float(np.abs(W).max() * np.abs(X).max()) if data == "logmag" else math.sqrt(K)
        C = (rng_of("c0", kind, data, S, *seed).standard_normal((M, M)) * s).astype(np.float32)
    return W, X, C


def product_cases():
    return [(data, S, with_c) for data in TARGETS6[1:] + ("randn", "logmag") for S in S_BLOCKS
            for with_c in (False, True)]


def product_reference(W, X, C):
    """(ref64, Abound, tiny) of C + W·X"""
    w, x, c = (torch.from_numpy(a).double() for a in (W, X, C))
    tiny = TINY32 * max(1.0, float(np.abs(W).max())) * max(1.0, float(np.abs(X).max()))
    return c + w @ x, c.abs() + w.abs() @ x.abs(), tiny


def product_c32(kind):
    """the worst ratio of the same products in torch.float32 on the CPU over every case"""
    worst = 0.0
    for data, S, with_c in product_cases():
        W, X, C = product_operands(kind, data, S, with_c)
        got = torch.from_numpy(C) + torch.from_numpy(W) @ torch.from_numpy(X)
        worst = max(worst, G.worst_ratio(got, *product_reference(W, X, C)))
    return worst


def split_inputs(kind, S):
    """dict name -> X (K, N) for the split tests: randn, log-magnitude 1e-12..1e12 (with exact
    zeros), planted three-term values, and exact bf16 values"""
    M, kb = GEOM[kind]
    K = kb * S
    out = {"randn": G.randn_pair(M, K, M, kind, "split")[1],
           "logmag": G.logmag_pair(M, K, M, kind, "split")[1],
           "planted": G.planted("a1b3", M, K, M, kind, "split")[1]}
    out["bf16"] = G.bf16_rne(out["randn"])
    out["bf16"][::7, ::3] = 0.0
    return out


if __name__ == "__main__":
    Q, rows = sincos_domain()
    for r in rows:
        print("octave 2^%-2d  (|r|-pi)/(eps|q|) %.3f  |r|/pi %.4f  err/(eps|q|) %.3f" % r)
    print("Q = 2^%d" % round(math.log2(Q)))
    y, _ = act_inputs()
    print("c32 sp_sig", c32_of(ref_sp_sig, y))
    print("c32 head", c32_of(ref_head, act_inputs(100.0)[0]))
    print("c32 merge", c32_of(ref_merge, *merge_inputs()))
    q, inside = sincos_inputs(Q)
    print("c32 sincos", c32_of(ref_sincos, q[inside]))
    for kind in GEOM:
        c32 = product_c32(kind)
        print("c32 %s %.3f -> c = %.1f" % (kind, c32, clamp_c(c32)))
