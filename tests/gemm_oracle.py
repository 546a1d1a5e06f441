"""CPU-side oracle of tests/test_gemm_engines.py: the fp64 reference and bound form of
pntf_tt_gemm, operands built to expose a wrong split-bf16 product, a numpy emulation of that
product ("the GEMMs on the bf16 matrix cores") that proves on the CPU that they
do, and a restatement of the dispatcher's launch arithmetic (csrc/pntf_gemm.hip, host side) from
which the tests derive the shapes that reach each launch regime.  Nothing here touches a GPU.

Reference and bound:  ref64 = op(A)·op(B) + beta·C0 in fp64 from the fp32 operands,
Abound = |op(A)|·|op(B)| + |beta·C0|, and a result holds when, elementwise,

    |got - ref64| <= c·EPS32·Abound + tiny,       tiny = TINY32 x the largest magnitudes in play.

c is not chosen: c32 is the worst err / (EPS32·Abound) of the same product evaluated in
torch.float32 on the CPU over every case of the test file (`python tests/gemm_oracle.py`
re-measures it; never the kernel under test), and c = 4·c32 clamped to [8, 64] (the factor 4 for
the MFMA's other summation order).

Planted operands.  With terms numbered from 1 as x = x1 + x2 + x3, every element is
    a = s1·h + s2·h·2^-9 + s3·h·2^-18,   h = (q / 32)·2^e, q in 40..56, e in -1..1, s = ±1
(and likewise b from g).  h has 6 significant bits and lies in [1.25, 1.75]·2^e, so the
round-to-nearest-even bf16 split of a is exactly (s1·h, s2·h·2^-9, s3·h·2^-18): each lower term is
below half a bf16 ulp of the one above it and a is an fp32 number (24 bits from 2^e to 2^(e-23)).
For the target product a_i·b_j the signs of term i of A and term j of B are both eps[k], a
function of the reduction index alone, so every one of the K target products is positive; all
other signs are independent coin flips, so every other product, the leading a1·b1 included,
random-walks.  A has terms 1..i, B terms 1..j.  Dropping the target then moves every element by
2^-9 (a1b2, a2b1) or 2^-18 (a2b2, a1b3, a3b1) of Abound = 2^14 or 32 units of EPS32·Abound,
whatever K is.  (A wider exponent spread changes none of this but raises the fp32 yardstick's own
error on these operands, 5.2 at e in -3..3 against 3.1, and with it c for every case.)  On randn data the same drop is a random walk of 2^-17/sqrt(K) of Abound, below
rounding noise.
"""
import functools
import math
import zlib
from collections import namedtuple

import numpy as np
import torch

EPS32 = 2.0 ** -23
TINY32 = float(np.finfo(np.float32).tiny)

# c32 as measured by `python tests/gemm_oracle.py` over every case of test_gemm_engines.py (at
# 256 CUs); C is what the tests hold the kernels to
C32 = 4.43
C = min(64.0, max(8.0, 4.0 * C32))

PRODUCTS = ("a1b1", "a1b2", "a2b1", "a2b2", "a1b3", "a3b1")     # the six of order >= 2^-16
TARGETS = PRODUCTS[1:]                                          # one planted pair each


def rng_of(*seed):
    return np.random.default_rng(zlib.crc32(repr(seed).encode()))


# ------------------------------------------------------------------ split-bf16 emulation


def bf16_rne(x):
    """fp32 -> the nearest bf16 (ties to even), returned as fp32; finite inputs"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x):
    """x = x1 + x2 + x3 (+ a remainder below 2^-24 |x|): x1 = bf16(x), x2 = bf16(x - x1),
    x3 = bf16(x - x1 - x2); the fp32 subtractions are exact"""
    x = np.asarray(x, dtype=np.float32)
    x1 = bf16_rne(x)
    r1 = x - x1
    x2 = bf16_rne(r1)
    x3 = bf16_rne(r1 - x2)
    return x1, x2, x3


def emulate(opA, opB, drop=None):
    """op(A)·op(B) as the six bf16 products of order >= 2^-16, each accumulated in fp32 (a bf16
    product is exact in fp32), summed smallest order first; `drop` names one product to leave out"""
    a, b = split3(opA), split3(opB)

    def prod(name):
        if name == drop:
            return np.zeros((opA.shape[0], opB.shape[1]), np.float32)
        return a[int(name[1]) - 1] @ b[int(name[3]) - 1]

    low = (prod("a3b1") + prod("a2b2")) + prod("a1b3")
    mid = prod("a2b1") + prod("a1b2")
    return ((low + mid) + prod("a1b1")).astype(np.float32)


# ------------------------------------------------------------------ operands


def _mags(rng, *shape):
    q = rng.integers(40, 57, size=shape).astype(np.float64) / 32.0
    return q * np.exp2(rng.integers(-1, 2, size=shape).astype(np.float64))


def _signs(rng, *shape):
    return rng.integers(0, 2, size=shape).astype(np.float64) * 2.0 - 1.0


SCALE = (1.0, 2.0 ** -9, 2.0 ** -18)


def planted(target, M, K, N, *seed):
    """(op(A) (M, K), op(B) (K, N)) fp32 whose target product adds coherently (module header)"""
    i, j = int(target[1]), int(target[3])
    rng = rng_of("plant", target, M, K, N, *seed)
    eps = _signs(rng, K)
    h, g = _mags(rng, M, K), _mags(rng, K, N)
    A, B = np.zeros((M, K)), np.zeros((K, N))
    for t in range(i):
        A += (eps[None, :] if t == i - 1 else _signs(rng, M, K)) * h * SCALE[t]
    for t in range(j):
        B += (eps[:, None] if t == j - 1 else _signs(rng, K, N)) * g * SCALE[t]
    A32, B32 = A.astype(np.float32), B.astype(np.float32)
    assert (A32 == A).all() and (B32 == B).all()            # fp32 numbers
    # the split is the planted one (on a sample of a large operand)
    for X, Y, n in ((A32[:512], (np.abs(h[:512]) * SCALE[i - 1]), i),
                    (B32[:, :512], (np.abs(g[:, :512]) * SCALE[j - 1]), j)):
        assert (np.abs(split3(X)[n - 1]) == Y).all()
    return A32, B32


def randn_pair(M, K, N, *seed):
    rng = rng_of("randn", M, K, N, *seed)
    return (rng.standard_normal((M, K)).astype(np.float32),
            rng.standard_normal((K, N)).astype(np.float32))


def logmag_pair(M, K, N, *seed):
    """magnitudes log-uniform over 1e-12..1e12, random signs, 5 % exact zeros in A and 2 % in B"""
    rng = rng_of("logmag", M, K, N, *seed)

    def one(z, *shape):
        x = np.power(10.0, rng.random(shape) * 24.0 - 12.0) * _signs(rng, *shape)
        x[rng.random(shape) < z] = 0.0
        return x.astype(np.float32)

    return one(0.05, M, K), one(0.02, K, N)


# A GEMM case: C (M, N) = beta·C0 + op(A) (M, K)·op(B) (K, N); data = "randn", "logmag" or a
# planted target; tag separates cases of equal shape
Case = namedtuple("Case", "ta tb M N K beta data tag")


def make_case(ta, tb, M, N, K, beta=0.0, data="randn", tag=""):
    return Case(int(ta), int(tb), int(M), int(N), int(K), float(beta), data, tag)


def _operands(c):
    if c.data == "randn":
        opA, opB = randn_pair(c.M, c.K, c.N, c.tag)
    elif c.data == "logmag":
        opA, opB = logmag_pair(c.M, c.K, c.N, c.tag)
    else:
        opA, opB = planted(c.data, c.M, c.K, c.N, c.tag)
    C0 = None
    if c.beta != 0.0:
        s = float(np.abs(opA).max() * np.abs(opB).max()) if c.data == "logmag" else math.sqrt(c.K)
        C0 = (rng_of("c0", c).standard_normal((c.M, c.N)) * s).astype(np.float32)
    return opA, opB, C0


@functools.lru_cache(maxsize=64)
def _operands_small(c):
    return _operands(c)


def operands(c):
    """(op(A), op(B), C0 or None) of a case, fp32 numpy; never modified by a caller (small cases
    are shared between tests)"""
    return _operands_small(c) if c.M * c.K + c.K * c.N <= (1 << 20) else _operands(c)


def reference(c, opA, opB, C0):
    """(ref64, Abound, tiny): torch fp64 (M, N) tensors and the absolute slack"""
    a, b = torch.from_numpy(opA).double(), torch.from_numpy(opB).double()
    ref, Ab = a @ b, a.abs() @ b.abs()
    if C0 is not None:
        c0 = torch.from_numpy(C0).double() * c.beta
        ref, Ab = ref + c0, Ab + c0.abs()
    tiny = TINY32 * max(1.0, float(np.abs(opA).max())) * max(1.0, float(np.abs(opB).max()))
    return ref, Ab, tiny


def worst_ratio(got, ref, Ab, tiny):
    """max over elements of (|got - ref| - tiny) / (EPS32·Abound); inf where Abound is 0 and the
    error exceeds tiny, or where got is not finite"""
    err = (got.double() - ref).abs() - tiny
    r = torch.where(err <= 0, torch.zeros_like(err), err / (EPS32 * Ab))
    r = torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))
    return float(r.max()) if r.numel() else 0.0


def fp32_product(c, opA, opB, C0):
    """the yardstick: the same product in torch.float32 on the CPU"""
    got = torch.from_numpy(opA) @ torch.from_numpy(opB)
    if C0 is not None:
        got = got + np.float32(c.beta) * torch.from_numpy(C0)
    return got


# ------------------------------------------------------------------ launch arithmetic
# The host side of csrc/pntf_gemm.hip restated (tt_gemm, splits_for, wgrad_splits,
# pntf_tt_gemm_work_floats); cus = the device's compute units (num_cus()).

BM, BN, BK, RG = 128, 128, 8, 32
PANEL_MODES = (1, 2, 3, 6, 7, 8)
PANEL_ENGINE = {0: "gemm_kernel", 1: "panel_gemm_kernel", 2: "panel_lds_kernel",
                3: "panel_x6_kernel", 6: "panel_x6_kernel", 7: "panel_x6_kernel",
                8: "panel_x6s_kernel"}
WGRAD_ENGINE = {0: "gemm_kernel", 1: "wgrad_kernel", 2: "wgrad_x6_kernel"}


def ceil_div(a, b):
    return -(-a // b)


def splits_for(M, N, K, cus):
    """split-K factor of the LDS-tiled kernel: two workgroups per CU, >= 512 of K per split,
    a grid above one wave of workgroups rounded down to whole waves"""
    tiles = ceil_div(M, BM) * (N // BN)
    s = min(ceil_div(2 * cus, tiles), ceil_div(K, 512), 512)
    if tiles * s > cus:
        s = (tiles * s // cus) * cus // tiles
    return max(s, 1)


def panel_shape(N, K):
    return K in (128, 256) and N in (128, 256)


def wgrad_shape(M, N):
    return M in (128, 256) and N in (128, 256)


WgradPlan = namedtuple("WgradPlan", "T rps real launched xcd empty last_rows")


def wgrad_plan(M, N, K, cus):
    """the weight-gradient launch: T tiles, rows per split (a multiple of 128), splits that hold
    rows, splits launched (padded to a multiple of 8 on the XCD map), the padded empty ones, and
    the rows of the last split that holds any"""
    T = (M // 128) * (N // 128)
    s0 = max(1, min(cus // T, ceil_div(K, 256)))
    rps = ceil_div(ceil_div(K, s0), 128) * 128
    real = ceil_div(K, rps)
    xcd = T > 1 and real >= 8
    launched = ceil_div(real, 8) * 8 if xcd else real
    return WgradPlan(T, rps, real, launched, xcd, launched - real, K - (real - 1) * rps)


PanelGrid = namedtuple("PanelGrid", "groups per_group cap rounds")


def panel_grid(mode, M, N, K, beta, cus):
    """the panel launch under a panel mode: column groups, workgroups per group, the cap on
    them, and the rounds of 128 rows the busiest workgroup runs"""
    wgs = ceil_div(M, 128)
    if mode == 1:
        groups, cap, pad8 = 1, cus, False
    elif mode == 2:
        groups = N // 128
        cap, pad8 = (2 if K == 128 and beta == 0.0 else 1) * cus // groups, groups == 2
    elif mode in (3, 6, 7):
        groups = max(1, N // (64 if K == 256 else 128))
        cap, pad8 = cus // groups, groups > 1
    elif mode == 8:
        groups = N // 64
        cap, pad8 = cus // groups, True
    else:
        raise ValueError(mode)
    nwg = min(wgs, cap)
    if pad8:
        nwg = ceil_div(nwg, 8) * 8
    return PanelGrid(groups, nwg, cap, ceil_div(wgs, nwg))


def panel_pack_floats(mode, N, K):
    return K * N * 3 // 2 if mode >= 3 else K * N


def work_floats(M, N, K, cus):
    """pntf_tt_gemm_work_floats"""
    if M <= 0 or N <= 0 or K <= 0:
        return 0
    s = splits_for(M, N, K, cus)
    split = s * M * N if s > 1 else 0
    packed = K * N * 3 // 2 if panel_shape(N, K) else 0
    T = (M // 128) * (N // 128) if wgrad_shape(M, N) else 0
    wgrad = (max(1, min(cus // T, ceil_div(K, 256))) + 7) * M * N if T else 0
    return max(split, packed, wgrad)


def work_needed(c, cus):
    """the most work floats any mode of the dispatcher uses for a case of natural layout"""
    need = 0
    if not c.ta and c.beta in (0.0, 1.0) and panel_shape(c.N, c.K):
        need = max(need, panel_pack_floats(3, c.N, c.K))
    if c.ta and not c.tb and c.beta == 0.0 and wgrad_shape(c.M, c.N):
        need = max(need, wgrad_plan(c.M, c.N, c.K, cus).launched * c.M * c.N)
    s = splits_for(c.M, c.N, c.K, cus)
    return max(need, s * c.M * c.N if s > 1 else 0)


# ------------------------------------------------------------------ the cases of the test file

KN = [(128, 128), (128, 256), (256, 128), (256, 256)]
PANEL_M = [1, 31, 32, 33, 127, 128, 129]
PANEL_PLANT_M = 33                                   # planted operands at this small M
WGRAD_K = [1, 3, 15, 16, 17, 127, 128, 129, 255, 256, 257]
WGRAD_PLANT_K = 256
LDS_K = [1, BK - 1, BK, BK + 1, 64, 77]
LDS_M = [1, 128, 129, 200]
LDS_BETA = [0.0, 0.5, 1.0]
FUSED_M = [33, 300]


def _target(*key):
    return TARGETS[zlib.crc32(repr(key).encode()) % len(TARGETS)]


def panel_cases(K, N):
    """the small panel cases of one (K, N): every M x beta x tb; planted operands (every target)
    at PANEL_PLANT_M, randn elsewhere"""
    out = []
    for beta in (0.0, 1.0):
        for tb in (0, 1):
            for M in PANEL_M:
                out.append(make_case(0, tb, M, N, K, beta))
            for t in TARGETS:
                out.append(make_case(0, tb, PANEL_PLANT_M, N, K, beta, t))
    out.append(make_case(0, 1, 129, N, K, 0.0, "logmag"))
    return out


# (K, N) -> (beta, tb, planted?) of the looping case: both betas, both tb and both kinds of data
LOOP_FORM = {(128, 128): (0.0, 1, True), (128, 256): (1.0, 0, False),
             (256, 128): (1.0, 1, True), (256, 256): (0.0, 0, False)}


def panel_loop_case(mode, K, N, cus):
    """128·(workgroup cap) + 33 rows: some workgroup of the engine runs a second round of tiles"""
    beta, tb, plant = LOOP_FORM[(K, N)]
    M = 128 * panel_grid(mode, 1 << 30, N, K, beta, cus).per_group + 33
    return make_case(0, tb, M, N, K, beta, _target(mode, K, N) if plant else "randn", "loop")


def panel_ldb_cases(K, N):
    return [make_case(0, tb, 77, N, K, beta, "randn", "ldb") for tb in (0, 1) for beta in (0.0, 1.0)]


def wgrad_k_empty(T, cus):
    """a reduction length whose XCD padding launches empty splits (9 splits padded to 16) and whose
    last real split holds one row; K = 2049 wherever a tile gets at least 9 workgroups"""
    return 8 * 256 + 1


def wgrad_k_groups():
    """M = N = 128: more than RG splits under every weight-gradient mode (the LDS-tiled kernel
    splits at 512 rows, the wgrad kernels at 256)"""
    return RG * 512 + 1


def wgrad_cases(M, N, cus):
    T = (M // 128) * (N // 128)
    out = [make_case(1, 0, M, N, K) for K in WGRAD_K]
    out += [make_case(1, 0, M, N, WGRAD_PLANT_K, 0.0, t) for t in TARGETS]
    out.append(make_case(1, 0, M, N, 257, 0.0, "logmag"))
    if T >= 2:
        out += [make_case(1, 0, M, N, wgrad_k_empty(T, cus), 0.0, t) for t in TARGETS[2:4]]
        out.append(make_case(1, 0, M, N, wgrad_k_empty(T, cus)))
    else:
        out.append(make_case(1, 0, M, N, wgrad_k_groups()))
    return out


def lds_k_split(cus):
    """a split-K length of the LDS-tiled kernel for a single tile: 3 splits"""
    return 2 * 512 + 76


def lds_cases(ta, tb, cus):
    """shapes neither the panel nor the weight-gradient path takes (M outside {128, 256} with ta,
    K outside {128, 256} without), N = 128 and 384"""
    out = []
    for K in LDS_K + [lds_k_split(cus)]:
        for i, M in enumerate(LDS_M):
            if ta and wgrad_shape(M, 128):
                M += 2
            beta = LDS_BETA[(i + K) % 3]
            out.append(make_case(ta, tb, M, 384 if (i + K) % 2 else 128, K, beta))
    out.append(make_case(ta, tb, 77, 128, 64, 0.5, "logmag"))
    out.append(make_case(ta, tb, 130, 128, RG * 512 + 1, 0.0, "randn", "groups"))
    return out


def lds_pad_cases(ta, tb):
    return [make_case(ta, tb, M, 256, K, beta, "randn", "pad")
            for M, K, beta in ((77, 77, 0.0), (130, 9, 0.5), (130, 1100, 1.0))]


def lds_fallback_cases():
    """panel shapes that fall back on a misaligned A or work, weight-gradient shapes on a
    misaligned A, B or work"""
    return [make_case(0, 1, 77, 128, 128, 0.0, "randn", "mis"),
            make_case(0, 0, 129, 256, 256, 1.0, "randn", "mis"),
            make_case(1, 0, 128, 256, 1100, 0.0, "randn", "mis")]


def fused_cases():
    return [make_case(0, 1, m, n, k, 0.0, t, "fused") for k, n in KN for m in FUSED_M
            for t in TARGETS]


def all_cases(cus=256):
    out = []
    for K, N in KN:
        out += panel_cases(K, N) + panel_ldb_cases(K, N)
        out += [panel_loop_case(mode, K, N, cus) for mode in PANEL_MODES]
    for M, N in KN:
        out += wgrad_cases(M, N, cus)
    for ta in (0, 1):
        for tb in (0, 1):
            out += lds_cases(ta, tb, cus) + lds_pad_cases(ta, tb)
    out += lds_fallback_cases() + fused_cases()
    return list(dict.fromkeys(out))


def c32_of(c):
    opA, opB, C0 = operands(c)
    ref, Ab, tiny = reference(c, opA, opB, C0)
    return worst_ratio(fp32_product(c, opA, opB, C0), ref, Ab, tiny)


if __name__ == "__main__":
    worst, at = 0.0, None
    for case in all_cases():
        r = c32_of(case)
        if r > worst:
            worst, at = r, case
    print("cases %d  c32 %.3f at %s  -> c = %.1f" % (
        len(all_cases()), worst, at, min(64.0, max(8.0, 4.0 * worst))))
