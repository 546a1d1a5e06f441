"""The workspace contract of the C ABI (include/pntf.h): "a smaller ws lowers the grid, never
fails unless it holds less than one workgroup's slots".

Every GPU test here calls the C ABI through ctypes with a `ws_bytes` of its own choosing:
exactly one workgroup's scratch (grid 1: every wave runs several tiles of the batch, the
persistent loops past their first iteration), three workgroups' less one byte (must floor to
grid 2) and the full pntf_workspace_bytes(n).  The buffer behind `ws` is always allocated at the
full size plus a tail and filled with the fp32 NaN pattern before each call, so

  * a scratch read before its write shows up as a non-finite output,
  * a wave that stores outside [0, ws_bytes) — a wrong slot index, a grid the clamp let
    through — breaks the pattern there (it cannot fault: the memory is the test's),
  * the outputs at every reduced level must be the full-workspace run's bit for bit (a tile's
    instruction sequence does not depend on which wave runs it), and the full-workspace run is
    held to the fp64 oracle at the bounds of tests/test_gpu_parity.py.

The host-only tests at the end make only calls that fail before any launch.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from golden_util import close, weights
from oracle import pntf_oracle as O
from pntf import _lib, ops, synth

# One workgroup's scratch per kernel family, from p-ntfields_amd/csrc/pntf_common.h:
WAVE_G = 4 * (192 * 256) * 4     # WAVES · SCRATCH_FLOATS_PER_WAVE · sizeof(float): wave-tile
                                 # field kernels, plan_kernel, residual_kernel
SPLIT_G = 8 * (192 * 256) * 4    # SPLIT_WAVES · SCRATCH_FLOATS_PER_WAVE · 4: split kernels
WIDE_G = 4 * (96 * 1024) * 4     # WAVES · WSCRATCH_FLOATS_PER_WAVE · 4: wide kernels
assert (WAVE_G, SPLIT_G, WIDE_G) == (786432, 1572864, 1572864)

AUTO, WAVE, SPLIT, WIDE, QUAD = range(5)               # PNTF_SCHED_*
K_TAU, K_TAU_GRAD, K_VELOCITY, K_SPEED, K_TRAVEL = range(5)   # PNTF_FIELD_*
EXACT, COMPAT = 0, 1                                   # PNTF_GRAD_*
ERR_WORKSPACE = 2
G_OF = {WAVE: WAVE_G, SPLIT: SPLIT_G, WIDE: WIDE_G}
SCHED_NAME = {WAVE: "wave", SPLIT: "split", WIDE: "wide"}

NAN_PATTERN = 0x7fc00000
TAIL = 4096
V = ctypes.c_void_p

gpu = pytest.mark.gpu


def vp(t):
    return V(t.data_ptr() if t is not None else 0)


def T(a, dev, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dtype)


def levels(G, full):
    """ws_bytes levels of a family: grid 1, grid 2 (3G - 1 floors to two workgroups), full."""
    assert full >= 3 * G
    return [G, 3 * G - 1, full]


def bits(t):
    return t.view(torch.int32)


class Canary:
    """pntf_workspace_bytes(n) + TAIL bytes of NaN pattern behind `ws`."""

    def __init__(self, lib, dev, n):
        self.full = int(lib.pntf_workspace_bytes(n))
        words = (self.full + TAIL) // 4
        self.buf = torch.empty(words, dtype=torch.int32, device=dev)
        self.ref = torch.full((words,), NAN_PATTERN, dtype=torch.int32, device=dev).view(torch.uint8)

    def fill(self):
        self.buf.fill_(NAN_PATTERN)
        return vp(self.buf)

    def assert_intact_from(self, offset, what):
        got = self.buf.view(torch.uint8)[offset:]
        if not torch.equal(got, self.ref[offset:]):
            bad = torch.nonzero(got != self.ref[offset:])
            raise AssertionError("%s: %d bytes past ws_bytes = %d overwritten, first at offset %d"
                                 % (what, bad.numel(), offset, offset + int(bad[0])))

    def head_words(self, k):
        return self.buf[:k].cpu().numpy()


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        from pntf import build
        build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def W():
    return weights()


@pytest.fixture(scope="module")
def packed(W, dev):
    return ops.pack_weights([torch.from_numpy(v).to(dev) for v in W.values()])


@pytest.fixture(scope="module")
def canaries(lib, dev):
    made = {}

    def get(n):
        if n not in made:
            made[n] = Canary(lib, dev, n)
        return made[n]
    return get


def stream(dev):
    return V(torch.cuda.current_stream(dev).cuda_stream)


# ---------------------------------------------------------------- 1. field kernels
N_FIELD = 293        # 19 ragged 16-pair tiles / 10 ragged 32-pair tiles (5 pairs in the last)
BAD_ROW = 150        # 16-pair tile 9, 32-pair tile 4: a middle tile of every family
_field_inputs = {}
_field_oracle = {}


def field_inputs(dim, n_env=3):
    """Pairs, B table, non-contiguous env ids with one id outside the table at BAD_ROW."""
    key = (dim, n_env)
    if key not in _field_inputs:
        xp = synth.make_pairs(N_FIELD, dim, seed=700 + dim)
        Bt = synth.make_B_table(n_env, dim, first_seed=40)
        env = synth.make_env_ids(N_FIELD, n_env, contiguous=False, seed=dim)
        assert len(set(env.tolist())) == n_env
        env[BAD_ROW] = n_env + 2
        _field_inputs[key] = (xp, Bt, env)
    return _field_inputs[key]


def field_oracle(W, dim, n_env, compat):
    """fp64 τ (n, 1) and ∇τ on the valid rows (computed once per input set)."""
    key = (dim, n_env, compat)
    if key not in _field_oracle:
        xp, Bt, env = field_inputs(dim, n_env)
        e = env.copy()
        e[BAD_ROW] = 0
        _field_oracle[key] = O.tau_grad(W, xp, Bt, e, dim=dim, compat=compat)
    return _field_oracle[key]


def field_outputs(kind, n, dim, dev):
    """(out0, out1) filled with +inf: an unwritten valid row is not finite, an unwritten
    invalid row is not NaN."""
    inf = float("inf")
    vec = lambda: torch.full((n,), inf, device=dev)              # noqa: E731
    mat = lambda: torch.full((n, 2 * dim), inf, device=dev)      # noqa: E731
    if kind == K_TAU_GRAD:
        return vec(), mat()
    if kind == K_VELOCITY:
        return mat(), vec()
    return vec(), None


def run_field(lib, dev, packed, kind, sched, dim, mode, inputs, ws, ws_bytes, tau_out=True):
    xp, Bt, env = inputs
    n = xp.shape[0]
    out0, out1 = field_outputs(kind, n, dim, dev)
    if kind == K_VELOCITY and not tau_out:
        out1 = None
    st = lib.pntf_field_ex(kind, vp(packed), dim, vp(xp), n, vp(Bt), vp(env), Bt.shape[0], mode,
                           vp(out0), vp(out1), ws, ws_bytes, sched, stream(dev))
    assert st == 0, lib.pntf_last_error()
    return out0, out1


def field_levels(lib, dev, packed, canaries, kind, sched, dim, mode, inputs):
    """The call at the three ws_bytes levels: canary intact, reduced levels bitwise the full
    one.  Returns the full-workspace outputs."""
    can = canaries(N_FIELD)
    G = G_OF[sched]
    runs = []
    for wsb in levels(G, can.full):
        what = "%s dim %d kind %d ws_bytes %d" % (SCHED_NAME[sched], dim, kind, wsb)
        o = run_field(lib, dev, packed, kind, sched, dim, mode, inputs, can.fill(), wsb)
        can.assert_intact_from(wsb, what)
        runs.append((what, o))
    full = runs[-1][1]
    for what, o in runs[:-1]:
        for a, b in zip(o, full):
            if a is not None:
                assert torch.equal(bits(a), bits(b)), what + ": differs from the full-workspace run"
    return full


def check_bad_row(outs):
    """The row with the env id outside the table is NaN, every other row finite."""
    ok = np.ones(N_FIELD, bool)
    ok[BAD_ROW] = False
    for o in outs:
        if o is None:
            continue
        a = o.cpu().numpy()
        assert np.isnan(a[BAD_ROW]).all()
        assert np.isfinite(a[ok]).all()
    return ok


FIELD_CASES = [("tau_grad_exact", K_TAU_GRAD, EXACT, (3, 6)),
               ("tau_grad_compat", K_TAU_GRAD, COMPAT, (3,)),
               ("velocity", K_VELOCITY, EXACT, (3, 6)),
               ("speed", K_SPEED, EXACT, (3, 6))]


@gpu
@pytest.mark.parametrize("sched", [WAVE, SPLIT, WIDE], ids=lambda s: SCHED_NAME[s])
@pytest.mark.parametrize("case,dim", [(c, d) for c in FIELD_CASES for d in c[3]],
                         ids=lambda v: v[0] if isinstance(v, tuple) else "d%d" % v)
def test_field_small_workspace(lib, dev, packed, W, canaries, sched, case, dim):
    """pntf_field_ex, n = 293, 3 envs: at one workgroup's ws every wave (split: the workgroup)
    runs 2 or more ragged tiles, one of them holding the invalid env id."""
    _, kind, mode, _ = case
    xp, Bt, env = field_inputs(dim)
    inputs = (T(xp, dev), T(Bt, dev), T(env, dev, torch.int32))
    out0, out1 = field_levels(lib, dev, packed, canaries, kind, sched, dim, mode, inputs)
    ok = check_bad_row((out0, out1))
    to, do = field_oracle(W, dim, 3, mode == COMPAT)
    to, do = to[ok], do[ok]
    a0 = out0.cpu().numpy()[ok]
    if kind == K_TAU_GRAD:
        close(a0, to[:, 0], pairs=True)
        close(out1.cpu().numpy()[ok], do, pairs=True)
    elif kind == K_VELOCITY:
        close(a0, O.path_velocity(xp[ok], to, do, dim), pairs=True)
        close(out1.cpu().numpy()[ok], to[:, 0], pairs=True)
        # the τ output is optional: without it, the same velocities
        can = canaries(N_FIELD)
        v, _ = run_field(lib, dev, packed, kind, sched, dim, mode, inputs, can.fill(), can.full,
                         tau_out=False)
        assert torch.equal(bits(v), bits(out0))
    else:
        close(a0, O.speed(xp[ok], to, do, dim), pairs=True)


@gpu
@pytest.mark.parametrize("sched", [WAVE, SPLIT, WIDE], ids=lambda s: SCHED_NAME[s])
@pytest.mark.parametrize("dim", [3, 6])
def test_field_tau_and_travel_need_no_workspace(lib, dev, packed, W, sched, dim):
    """TAU and TRAVEL save nothing for a reverse sweep: ws = NULL, ws_bytes = 0 is accepted by
    every schedule, and the values are the oracle's."""
    xp, Bt, env = field_inputs(dim)
    inputs = (T(xp, dev), T(Bt, dev), T(env, dev, torch.int32))
    to, _ = field_oracle(W, dim, 3, False)
    for kind in (K_TAU, K_TRAVEL):
        out, _ = run_field(lib, dev, packed, kind, sched, dim, EXACT, inputs, None, 0)
        ok = check_bad_row((out,))
        ref = to[ok][:, 0] if kind == K_TAU else O.travel_time(xp[ok], to[ok], dim)
        close(out.cpu().numpy()[ok], ref, pairs=True)


@gpu
def test_wide_global_env_table_small_workspace(lib, dev, packed, W, canaries):
    """14 envs at dim 3 do not fit WBL_FLOATS (pntf_common.h): the wide kernel's global-table
    instantiation, several tiles per wave."""
    xp, Bt, env = field_inputs(3, 14)
    assert Bt.size > 5120
    inputs = (T(xp, dev), T(Bt, dev), T(env, dev, torch.int32))
    t, d = field_levels(lib, dev, packed, canaries, K_TAU_GRAD, WIDE, 3, EXACT, inputs)
    ok = check_bad_row((t, d))
    to, do = field_oracle(W, 3, 14, False)
    close(t.cpu().numpy()[ok], to[ok][:, 0], pairs=True)
    close(d.cpu().numpy()[ok], do[ok], pairs=True)


# ---------------------------------------------------------------- 2. residual kernel
N_RES = 149          # 10 ragged tiles: at grid 1 the four waves run 3, 3, 2, 2 of them


@gpu
@pytest.mark.parametrize("dim", [3, 6])
def test_residual_small_workspace(lib, dev, packed, W, canaries, dim):
    n, E, gamma = N_RES, 4, 1e-3
    xp = synth.make_pairs(n, dim, seed=800 + dim)
    Bt = synth.make_B_table(E, dim, first_seed=50)
    env = synth.make_env_ids(n, E, contiguous=False, seed=10 + dim)
    yobs = synth.make_speeds(n, seed=dim)
    d_xp, d_Bt, d_env, d_y = T(xp, dev), T(Bt, dev), T(env, dev, torch.int32), T(yobs, dev)
    can = canaries(n)
    inf = float("inf")
    runs = []
    for wsb in levels(WAVE_G, can.full):
        out = [torch.full((n,), inf, device=dev), torch.full((n, 2 * dim), inf, device=dev),
               torch.full((n, 2 * dim), inf, device=dev), torch.full((n,), inf, device=dev)]
        st = lib.pntf_eikonal_residual(vp(packed), dim, vp(d_xp), vp(d_y), n, vp(d_Bt), vp(d_env),
                                       E, gamma, vp(out[0]), vp(out[1]), vp(out[2]), vp(out[3]),
                                       can.fill(), wsb, stream(dev))
        assert st == 0, lib.pntf_last_error()
        can.assert_intact_from(wsb, "residual dim %d ws_bytes %d" % (dim, wsb))
        runs.append(out)
    full = runs[-1]
    for wsb, out in zip(levels(WAVE_G, can.full), runs[:-1]):
        for a, b in zip(out, full):
            assert torch.equal(bits(a), bits(b)), "ws_bytes %d differs from the full run" % wsb
    for o in full:
        assert torch.isfinite(o).all()
    to, do, lo, dfo = O.eikonal_residual(W, xp, yobs, Bt, env, dim=dim, gamma=gamma)
    tau, dtau, ltau, diff = [o.cpu().numpy() for o in full]
    close(tau, to[:, 0], pairs=True)
    close(dtau, do, pairs=True)
    close(ltau, lo, pairs=True)
    close(diff, dfo, pairs=True, diff=True)


# ---------------------------------------------------------------- 3. planners
def run_plan(lib, dev, packed, sched, dim, mode, step, tol, max_iter, inputs, ws, ws_bytes):
    xp0, Bt, env = inputs
    q = xp0.shape[0]
    path = torch.full((q, max_iter + 2, 2 * dim), float("inf"), device=dev)
    steps = torch.full((q,), -7, dtype=torch.int32, device=dev)
    st = lib.pntf_plan_ex(vp(packed), dim, vp(xp0), q, vp(Bt), vp(env), Bt.shape[0], mode,
                          step, tol, max_iter, vp(path), vp(steps), ws, ws_bytes, sched,
                          stream(dev))
    assert st == 0, lib.pntf_last_error()
    return path, steps


# (q, tile whose 16 queries start within tol).  With one workgroup's ws the wave-tile planner's
# wave w runs tiles w, w + 4, ...; the split planner's single workgroup runs every tile in order.
#   q = 149, 10 tiles: wave 1 runs 1 (active), 5 (zero iterations), 9 (the ragged last tile,
#                      active: no wave of this batch has a fourth tile);
#   q = 197, 13 tiles: wave 0 runs 0 (active), 4 (zero iterations), 8 (active), 12 (ragged last).
PLAN_BATCHES = [(149, 5), (197, 4)]


@gpu
@pytest.mark.parametrize("sched", [WAVE, SPLIT], ids=lambda s: SCHED_NAME[s])
@pytest.mark.parametrize("dim", [3, 6])
@pytest.mark.parametrize("q,pre", PLAN_BATCHES)
def test_planner_small_workspace(lib, dev, packed, W, canaries, sched, dim, q, pre):
    """pntf_plan_ex on one workgroup's ws: a wave's (split: the workgroup's) tile sequence holds
    an active tile, a tile that runs zero iterations — the weight ring prefetched by the tile
    before must reach the tile after untouched — another active tile and the ragged last one."""
    max_iter = 12
    if dim == 3:
        mode, step, tol, compat = COMPAT, 0.03, 0.06, True
        xp0 = synth.make_pairs(q, 3, seed=900 + q)
        Bt = synth.make_B_table(2, 3, first_seed=70)
    else:
        mode, step, tol, compat = EXACT, 0.015, 0.03, False
        xp0 = synth.make_box_pairs(q, 6, seed=900 + q)
        Bt = np.stack([synth.make_B(6, seed=12 + e, arm=True).T.copy() for e in range(2)])
    ntiles = (q + 15) // 16
    last = ntiles - 1
    first = pre % 4
    seq = list(range(first, ntiles, 4))                 # the wave-tile wave at grid 1
    assert seq[0] != pre and pre in seq and seq[-1] == last and q % 16 != 0
    lo, hi = 16 * pre, 16 * pre + 16
    xp0[lo:hi, dim:] = xp0[lo:hi, :dim]
    xp0[lo:hi, dim] += 0.001                            # |x_goal - x_start| = 0.001 < tol
    env = synth.make_env_ids(q, 2, contiguous=False, seed=q)
    bad = 16 * first + 7                                # an invalid env id in an active tile
    env[bad] = 2
    # one query of each tile of the sequence (and of the tile the split workgroup runs next)
    probe = sorted({16 * t + 3 for t in seq + [pre + 1]})
    start_dist = np.linalg.norm(xp0[:, dim:] - xp0[:, :dim], axis=1)
    active_tiles = [t for t in range(ntiles) if t != pre]
    assert all((start_dist[16 * t:16 * t + 16] > tol).any() for t in active_tiles)

    inputs = (T(xp0, dev), T(Bt, dev), T(env, dev, torch.int32))
    can = canaries(q)
    runs = []
    for wsb in levels(G_OF[sched], can.full):
        what = "plan %s dim %d q %d ws_bytes %d" % (SCHED_NAME[sched], dim, q, wsb)
        p, s = run_plan(lib, dev, packed, sched, dim, mode, step, tol, max_iter, inputs,
                        can.fill(), wsb)
        can.assert_intact_from(wsb, what)
        runs.append((what, p, s))
    _, path, steps = runs[-1]
    for what, p, s in runs[:-1]:
        assert torch.equal(s, steps), what + ": steps differ from the full-workspace run"
        assert torch.equal(bits(p), bits(path)), what + ": path differs from the full-workspace run"
    assert torch.isfinite(path).all()
    path, steps = path.cpu().numpy(), steps.cpu().numpy()
    assert steps[bad] == -1
    assert (np.delete(steps, bad) >= 0).all()
    assert (steps[lo:hi] == 0).all()
    assert (path[lo:hi] == xp0[lo:hi, None, :]).all()
    po, so = O.plan(W, xp0[probe], Bt, env[probe], dim=dim, step=step, tol=tol,
                    max_iter=max_iter, compat=compat)
    print("probe queries %s: steps %s, oracle %s, max |path - oracle| %.3g"
          % (probe, steps[probe].tolist(), so.tolist(), np.abs(path[probe] - po).max()))
    np.testing.assert_array_equal(steps[probe], so)
    assert np.abs(path[probe] - po).max() < 1e-3


# ---------------------------------------------------------------- 4. hand-off threshold
@gpu
def test_handoff_threshold(lib, dev, packed, canaries):
    """AUTO's quad planner hands its tail off to a SOLO launch only when ws holds the 8 + 8q
    bytes of the hand-off lists (include/pntf.h): at exactly that size it does, inside those
    bytes; one byte less, or ws = NULL, and nothing is touched.  Same bits as QUAD_TILE every
    time."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    q, dim, max_iter = cus + 44, 6, 20
    assert (q + 3) // 4 <= cus < q           # quad tiles, more than one query per CU
    xp0 = synth.make_box_pairs(q, dim, seed=33)
    # 50 queries start within tol, so at most `cus` are left and the tiles do hand off
    xp0[8:58, dim:] = xp0[8:58, :dim]
    xp0[8:58, dim] += 0.001
    B = synth.make_B(6, seed=12, arm=True).T.copy()[None]
    inputs = (T(xp0, dev), T(B, dev), None)
    kw = dict(dim=dim, mode=EXACT, step=0.015, tol=0.03, max_iter=max_iter, inputs=inputs)
    need = 8 + 8 * q
    can = canaries(q)
    assert can.full >= need

    pq, sq = run_plan(lib, dev, packed, QUAD, ws=None, ws_bytes=0, **kw)
    assert torch.isfinite(pq).all() and (sq >= 0).all()

    def same(p, s, what):
        assert torch.equal(s, sq), what + ": steps differ from QUAD_TILE"
        assert torch.equal(bits(p), bits(pq)), what + ": path differs from QUAD_TILE"

    p, s = run_plan(lib, dev, packed, AUTO, ws=can.fill(), ws_bytes=need, **kw)
    can.assert_intact_from(need, "hand-off with ws_bytes = 8 + 8q")
    done, handed = can.head_words(2).tolist()
    same(p, s, "ws_bytes = 8 + 8q")
    assert 0 < handed <= cus and done >= q - cus, (done, handed)

    p, s = run_plan(lib, dev, packed, AUTO, ws=can.fill(), ws_bytes=need - 1, **kw)
    can.assert_intact_from(0, "ws_bytes = 8 + 8q - 1")      # no hand-off attempted
    same(p, s, "ws_bytes = 8 + 8q - 1")

    can.fill()
    p, s = run_plan(lib, dev, packed, AUTO, ws=None, ws_bytes=need, **kw)
    can.assert_intact_from(0, "ws = NULL")
    same(p, s, "ws = NULL")


# ---------------------------------------------------------------- 5. host only
def test_workspace_minimum_is_one_workgroup(lib):
    assert lib.pntf_workspace_bytes(1) == max(WAVE_G, SPLIT_G, WIDE_G)


def test_workspace_below_one_workgroup_is_rejected(lib):
    """One byte less than a family's workgroup scratch: PNTF_ERR_WORKSPACE before any launch
    (the pointers are fake), with the family's requirement in the message."""
    fake = V(64)
    n = 293
    for sched, G, name in ((WAVE, WAVE_G, b"wave-tile"), (SPLIT, SPLIT_G, b"split-tile"),
                           (WIDE, WIDE_G, b"wide-tile")):
        st = lib.pntf_field_ex(K_TAU_GRAD, fake, 3, fake, n, fake, None, 1, 0, fake, fake, fake,
                               G - 1, sched, None)
        err = lib.pntf_last_error()
        assert st == ERR_WORKSPACE, (sched, st, err)
        assert name in err and b">= %d" % G in err and b"%d bytes" % (G - 1) in err, err
    for sched, G, name in ((WAVE, WAVE_G, b"wave-tile"), (SPLIT, SPLIT_G, b"split-tile")):
        st = lib.pntf_plan_ex(fake, 6, fake, n, fake, None, 1, 0, 0.015, 0.03, 5, fake, fake,
                              fake, G - 1, sched, None)
        err = lib.pntf_last_error()
        assert st == ERR_WORKSPACE, (sched, st, err)
        assert name in err and b">= %d" % G in err, err
    st = lib.pntf_eikonal_residual(fake, 3, fake, fake, n, fake, None, 1, 1e-3, fake, fake, fake,
                                   fake, fake, WAVE_G - 1, None)
    err = lib.pntf_last_error()
    assert st == ERR_WORKSPACE and b"wave-tile" in err and b">= %d" % WAVE_G in err, (st, err)


def test_null_workspace_is_rejected_for_grad_kinds(lib):
    fake = V(64)
    n = 293
    for kind in (K_TAU_GRAD, K_VELOCITY, K_SPEED):
        for sched in (WAVE, SPLIT, WIDE):
            st = lib.pntf_field_ex(kind, fake, 3, fake, n, fake, None, 1, 0, fake, fake, None,
                                   1 << 30, sched, None)
            assert st == ERR_WORKSPACE and b"null workspace" in lib.pntf_last_error(), (kind, sched)
    for sched in (WAVE, SPLIT):
        assert lib.pntf_plan_ex(fake, 6, fake, n, fake, None, 1, 0, 0.015, 0.03, 5, fake, fake,
                                None, 1 << 30, sched, None) == ERR_WORKSPACE
    assert lib.pntf_eikonal_residual(fake, 3, fake, fake, n, fake, None, 1, 1e-3, fake, fake,
                                     fake, fake, None, 1 << 30, None) == ERR_WORKSPACE
