"""The wide kernels' fused epilogues (pntf_wide.h: a layer's softplus/σ or ⊙σ epilogue runs
inside the next layer's split of the same tile) against the fp64 oracle, at the smallest
shapes that reach every fused boundary:

  * n = 1, 32, 33, 95: a partial tile, an exact tile, a second tile with one live column, three
    tiles with a ragged last one;
  * one batch whose waves run 3 tiles each (one workgroup's workspace through the C ABI, the
    route of tests/test_workspace.py): the σ prefetch slots, the weight ring and the banks are
    handed from tile to tile;
  * dim 3 and dim 6; exact and compat mode (encoder[0]'s quirk runs inside a0's fused split);
  * τ only (no σ store path);
  * a 10-environment table (staged in LDS, split-bf16 fold fused with a0ᵀ's epilogue) and
    tables too large for LDS (14 environments at dim 3, 10 at dim 6: global table, fp32 fold).

Bounds: golden_util.close(pairs=True), what tests/test_gpu_parity.py holds the wide kernel to
per pair.  The oracle values are computed once per input set and shared.
"""
import ctypes

import numpy as np
import pytest
import torch

from golden_util import close, weights
from oracle import pntf_oracle as O
from pntf import _lib, ops, synth

pytestmark = pytest.mark.gpu

NS = (1, 32, 33, 95)
N_MAX = max(NS)
# (dim, environments): tables that fit the LDS staging area and tables that do not
LDS_TABLES = ((3, 10), (6, 5))
GLOBAL_TABLES = ((3, 14), (6, 10))
WIDE_G = 4 * (96 * 1024) * 4          # one workgroup's σ scratch (tests/test_workspace.py)
N_MULTI = 32 * 12 - 7                  # 12 tiles: at grid 1 each of the 4 waves runs 3
K_TAU_GRAD, SCHED_WIDE = 1, 3


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def W():
    return weights()


@pytest.fixture(scope="module")
def packed(W, dev):
    return ops.pack_weights([torch.from_numpy(v).to(dev) for v in W.values()])


def T(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


_inputs = {}
_oracle = {}


def inputs(dim, n_env, n=N_MAX):
    """n pairs with non-contiguous env ids over an n_env table; a batch of n' < n pairs is its
    first n' rows."""
    key = (dim, n_env, n)
    if key not in _inputs:
        xp = synth.make_pairs(n, dim, seed=1300 + 10 * dim + n_env)
        Bt = synth.make_B_table(n_env, dim, first_seed=80)
        env = synth.make_env_ids(n, n_env, contiguous=False, seed=n_env + dim)
        _inputs[key] = (xp, Bt, env)
    return _inputs[key]


def oracle(W, dim, n_env, compat, n=N_MAX):
    key = (dim, n_env, compat, n)
    if key not in _oracle:
        xp, Bt, env = inputs(dim, n_env, n)
        _oracle[key] = O.tau_grad(W, xp, Bt, env, dim=dim, compat=compat)
    return _oracle[key]


def run(packed, dev, dim, n_env, n, compat, total=N_MAX):
    xp, Bt, env = inputs(dim, n_env, total)
    mode = ops.GRAD_BACKGRAD_COMPAT if compat else ops.GRAD_EXACT
    return ops.tau_grad(packed, T(xp[:n], dev), T(Bt, dev), T(env[:n], dev, torch.int32), dim=dim,
                        mode=mode, schedule="wide_tile")


def check(t, d, to, do, n):
    t, d = t.cpu().numpy(), d.cpu().numpy()
    assert t.shape == (n,) and d.shape == do[:n].shape
    assert np.isfinite(t).all() and np.isfinite(d).all()
    close(t, to[:n, 0], pairs=True)
    close(d, do[:n], pairs=True)


@pytest.mark.parametrize("compat", [False, True], ids=["exact", "compat"])
@pytest.mark.parametrize("dim,n_env", LDS_TABLES, ids=["d3", "d6"])
@pytest.mark.parametrize("n", NS)
def test_tau_grad_lds_table_vs_oracle(packed, dev, W, n, dim, n_env, compat):
    to, do = oracle(W, dim, n_env, compat)
    t, d = run(packed, dev, dim, n_env, n, compat)
    check(t, d, to, do, n)


@pytest.mark.parametrize("compat", [False, True], ids=["exact", "compat"])
@pytest.mark.parametrize("dim,n_env", GLOBAL_TABLES, ids=["d3", "d6"])
@pytest.mark.parametrize("n", [33, 95])
def test_tau_grad_global_table_vs_oracle(packed, dev, W, n, dim, n_env, compat):
    to, do = oracle(W, dim, n_env, compat)
    t, d = run(packed, dev, dim, n_env, n, compat)
    check(t, d, to, do, n)


@pytest.mark.parametrize("dim,n_env", LDS_TABLES + GLOBAL_TABLES,
                         ids=["d3_lds", "d6_lds", "d3_global", "d6_global"])
@pytest.mark.parametrize("n", NS)
def test_tau_only_vs_oracle(packed, dev, W, n, dim, n_env):
    xp, Bt, env = inputs(dim, n_env)
    to, _ = oracle(W, dim, n_env, False)
    t = ops.tau(packed, T(xp[:n], dev), T(Bt, dev), T(env[:n], dev, torch.int32), dim=dim,
                schedule="wide_tile")
    t = t.cpu().numpy()
    assert t.shape == (n,) and np.isfinite(t).all()
    close(t, to[:n, 0], pairs=True)


@pytest.mark.parametrize("compat", [False, True], ids=["exact", "compat"])
@pytest.mark.parametrize("dim,n_env", LDS_TABLES + GLOBAL_TABLES[:1],
                         ids=["d3_lds", "d6_lds", "d3_global"])
def test_three_tiles_per_wave_vs_oracle(packed, dev, W, dim, n_env, compat):
    """One workgroup's workspace: grid 1, so each wave runs tiles w, w + 4, w + 8 and hands its
    ring, banks and σ slots over twice.  Against the oracle, and bit for bit the full-workspace
    run (one tile per wave)."""
    lib = _lib.load()
    n = N_MULTI
    xp, Bt, env = inputs(dim, n_env, n)
    to, do = oracle(W, dim, n_env, compat, n)
    d_xp, d_Bt, d_env = T(xp, dev), T(Bt, dev), T(env, dev, torch.int32)
    full = int(lib.pntf_workspace_bytes(n))
    assert full >= 3 * WIDE_G
    ws = torch.empty(full // 4, dtype=torch.int32, device=dev)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())                       # noqa: E731
    outs = []
    for wsb in (WIDE_G, full):
        ws.fill_(0x7fc00000)            # a σ read before its write gives a NaN
        t = torch.full((n,), float("inf"), device=dev)
        d = torch.full((n, 2 * dim), float("inf"), device=dev)
        st = lib.pntf_field_ex(K_TAU_GRAD, vp(packed), dim, vp(d_xp), n, vp(d_Bt), vp(d_env),
                               Bt.shape[0], int(compat), vp(t), vp(d), vp(ws), wsb, SCHED_WIDE,
                               ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        assert st == 0, lib.pntf_last_error()
        outs.append((t, d))
    (t1, d1), (tf, df) = outs
    check(t1, d1, to, do, n)
    assert torch.equal(t1.view(torch.int32), tf.view(torch.int32))
    assert torch.equal(d1.view(torch.int32), df.view(torch.int32))


@pytest.mark.parametrize("dim,fit", [(3, 13), (6, 6)])
def test_lds_and_global_table_kernels_agree(packed, dev, dim, fit):
    """Same pairs and env ids with the table at the LDS limit and padded by one environment
    (global table): τ bitwise equal; ∇τ per pair within 1e-5 (split-bf16 fold against fp32
    fold), the bound of test_wide_env_table_in_lds_matches_global."""
    n = N_MAX
    xp = T(synth.make_pairs(n, dim, seed=43), dev)
    Bt = synth.make_B_table(fit + 1, dim, first_seed=60)
    env = T(synth.make_env_ids(n, fit, contiguous=False, seed=fit), dev, torch.int32)
    t_l, d_l = ops.tau_grad(packed, xp, T(Bt[:fit], dev), env, dim=dim, schedule="wide_tile")
    t_g, d_g = ops.tau_grad(packed, xp, T(Bt, dev), env, dim=dim, schedule="wide_tile")
    assert torch.equal(t_l, t_g)
    dl, dg = d_l.double(), d_g.double()
    r = (dl - dg).norm(dim=1) / dg.norm(dim=1).clamp_min(1e-30)
    assert float(r.max()) < 1e-5, float(r.max())
    assert torch.isfinite(t_l).all() and torch.isfinite(d_l).all()
