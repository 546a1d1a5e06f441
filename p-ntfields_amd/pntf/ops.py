"""Torch-facing wrappers of the libpntf C ABI (device tensors in, device tensors out).

Every call is stream-ordered on torch's current HIP stream of the input's device; torch's
caching allocator owns all buffers (outputs and the scratch workspace).  Inputs must be
HIP (``cuda``) tensors: there is deliberately no CPU path.

The scratch workspace is cached per (device, stream): two streams of one device never share
a slot set, so concurrent calls on different streams cannot overwrite each other's saved σ
tiles.  The kernel schedule is an argument of every call (pntf_field_ex); nothing here
mutates process-wide library state.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import GRAD_BACKGRAD_COMPAT, GRAD_EXACT, PntfError, check

__all__ = ["GRAD_EXACT", "GRAD_BACKGRAD_COMPAT", "PntfError", "pack_weights", "tau",
           "tau_grad", "path_velocity", "speed", "travel_time", "plan", "eikonal_residual",
           "device_sum", "packed_floats", "workspace_bytes", "point_mesh_distance",
           "arm_mesh_distance", "polyline_mesh_distance", "plan_polylines", "grid_travel_time",
           "grid_travel_time_init", "grid_travel_time_pass", "grid_nodes", "speed_grid",
           "grid_descent", "grid_polyline_time"]

class StreamScratch:
    """Grow-only device scratch per (device, stream), least-recently-used first out.

    A buffer is recorded on the stream it serves, so the caching allocator keeps its memory
    alive until that stream's queued work is done even after the entry is dropped or
    replaced.  At most `cap` streams keep a buffer: a caller that cycles through short-lived
    streams does not pin one buffer per dead stream, and a recycled stream handle at worst
    reuses a live buffer of the right size."""

    def __init__(self, dtype, cap=8):
        self.dtype, self.cap = dtype, cap
        self.entries = collections.OrderedDict()

    def get(self, device, numel):
        stream = torch.cuda.current_stream(device)
        key = (device.index, stream.cuda_stream)
        buf = self.entries.pop(key, None)
        if buf is None or buf.numel() < numel:
            buf = torch.empty(max(int(numel), 1), dtype=self.dtype, device=device)
            if not torch.cuda.is_current_stream_capturing():
                buf.record_stream(stream)     # (a graph's pool keeps its buffers alive)
        self.entries[key] = buf
        while len(self.entries) > self.cap:
            self.entries.popitem(last=False)
        return buf


_ws_cache = StreamScratch(torch.uint8)


def _vp(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)


def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_device(t, name):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise PntfError("%s must be a HIP device tensor (got %s); the P-NTFields MI355X path "
                        "has no CPU fallback" % (name, getattr(t, "device", type(t))))


def packed_floats():
    return int(_lib.load().pntf_packed_floats())


def workspace_bytes(n):
    return int(_lib.load().pntf_workspace_bytes(int(n)))


def _workspace(device, n):
    """Scratch buffer per (device, stream) for the saved σ10 tiles of the reverse sweep
    (StreamScratch: grow-only, LRU over streams)."""
    return _ws_cache.get(device, workspace_bytes(n))


def pack_weights(params, out=None):
    """Pack the 30 state-dict tensors (reference order, see synth.state_dict_keys) into the
    MFMA fragment blob consumed by every kernel (pntf_pack_weights)."""
    lib = _lib.load()
    params = list(params)
    if len(params) != 30:
        raise PntfError("expected the 30 state-dict tensors of NN, got %d" % len(params))
    dev = params[0].device
    ts = []
    for i, p in enumerate(params):
        _require_device(p, "param[%d]" % i)
        ts.append(p.detach().to(torch.float32).contiguous())
    if out is None:
        out = torch.empty(packed_floats(), dtype=torch.float32, device=dev)
    arr = (ctypes.c_void_p * 30)(*[t.data_ptr() for t in ts])
    check(lib.pntf_pack_weights(arr, 30, _vp(out), _stream(dev)), "pntf_pack_weights")
    return out


def _prep(xp, Btab, env, dim):
    _require_device(xp, "xp")
    if dim not in (3, 6):
        raise PntfError("dim must be 3 or 6")
    if xp.dim() != 2 or xp.shape[1] != 2 * dim:
        raise PntfError("xp must be (n, %d), got %s" % (2 * dim, tuple(xp.shape)))
    xp = xp.detach().to(torch.float32).contiguous()
    _require_device(Btab, "B")
    Bt = Btab.detach().to(device=xp.device, dtype=torch.float32)
    if Bt.dim() == 2:
        Bt = Bt.unsqueeze(0)
    if Bt.dim() != 3 or Bt.shape[1] != dim or Bt.shape[2] != 128:
        raise PntfError("B must be (dim, 128) or (n_env, dim, 128), got %s" % (tuple(Btab.shape),))
    Bt = Bt.contiguous()
    if env is not None:
        _require_device(env, "env")
        if env.numel() != xp.shape[0]:
            raise PntfError("env must hold one id per pair")
        env = env.detach().to(torch.int32).contiguous()
    return xp, Bt, env


SCHEDULES = {"auto": 0, "wave_tile": 1, "split_tile": 2, "wide_tile": 3, "quad_tile": 4}
FIELD_TAU, FIELD_TAU_GRAD, FIELD_VELOCITY, FIELD_SPEED, FIELD_TRAVEL = range(5)


def resolved_schedule(n, schedule="auto"):
    """Name of the kernel family a field call of n pairs runs (pntf_field_schedule_for)."""
    r = int(_lib.load().pntf_field_schedule_for(int(n), _sched(schedule)))
    if r < 0:
        raise PntfError("bad batch size or schedule")
    return {v: k for k, v in SCHEDULES.items()}[r]


def _sched(schedule):
    if schedule not in SCHEDULES:
        raise PntfError("unknown schedule %r (one of %s)" % (schedule, sorted(SCHEDULES)))
    return SCHEDULES[schedule]


def _field(kind, packed, xp, Bt, env, dim, mode, out0, out1, ws, schedule, what):
    n = xp.shape[0]
    check(_lib.load().pntf_field_ex(kind, _vp(packed), dim, _vp(xp), n, _vp(Bt), _vp(env),
                                    Bt.shape[0], mode, _vp(out0), _vp(out1), _vp(ws),
                                    ws.numel() if ws is not None else 0, _sched(schedule),
                                    _stream(xp.device)), what)


def tau(packed, xp, Btab, env=None, dim=3, schedule="auto"):
    """τ (n,) — NN.out (model_res_sigmoid_multi.py:215-259)."""
    xp, Bt, env = _prep(xp, Btab, env, dim)
    out = torch.empty(xp.shape[0], dtype=torch.float32, device=xp.device)
    _field(FIELD_TAU, packed, xp, Bt, env, dim, 0, out, None, None, schedule, "pntf_tau")
    return out


def tau_grad(packed, xp, Btab, env=None, dim=3, mode=GRAD_EXACT, schedule="auto"):
    """τ (n,) and ∇τ (n, 2dim): Model.gradient(NN.out) (EXACT) or NN.out_backgrad (COMPAT)."""
    xp, Bt, env = _prep(xp, Btab, env, dim)
    n = xp.shape[0]
    t = torch.empty(n, dtype=torch.float32, device=xp.device)
    d = torch.empty((n, 2 * dim), dtype=torch.float32, device=xp.device)
    _field(FIELD_TAU_GRAD, packed, xp, Bt, env, dim, mode, t, d, _workspace(xp.device, n),
           schedule, "pntf_tau_grad")
    return t, d


def path_velocity(packed, xp, Btab, env=None, dim=3, mode=GRAD_BACKGRAD_COMPAT,
                  schedule="auto"):
    """[v_start | v_goal] (n, 2dim) and τ (n,) — Model.Gradient (:1218-1248)."""
    xp, Bt, env = _prep(xp, Btab, env, dim)
    n = xp.shape[0]
    v = torch.empty((n, 2 * dim), dtype=torch.float32, device=xp.device)
    t = torch.empty(n, dtype=torch.float32, device=xp.device)
    _field(FIELD_VELOCITY, packed, xp, Bt, env, dim, mode, v, t, _workspace(xp.device, n),
           schedule, "pntf_path_velocity")
    return v, t


def speed(packed, xp, Btab, env=None, dim=3, schedule="auto"):
    """Speed at the goal (n,) — Model.Speed (:1195-1216)."""
    xp, Bt, env = _prep(xp, Btab, env, dim)
    n = xp.shape[0]
    s = torch.empty(n, dtype=torch.float32, device=xp.device)
    _field(FIELD_SPEED, packed, xp, Bt, env, dim, GRAD_EXACT, s, None,
           _workspace(xp.device, n), schedule, "pntf_speed")
    return s


def travel_time(packed, xp, Btab, env=None, dim=3, schedule="auto"):
    """|x_g - x_s| / τ (n,) — Model.TravelTimes (:1173-1186)."""
    xp, Bt, env = _prep(xp, Btab, env, dim)
    tt = torch.empty(xp.shape[0], dtype=torch.float32, device=xp.device)
    _field(FIELD_TRAVEL, packed, xp, Bt, env, dim, 0, tt, None, None, schedule,
           "pntf_travel_time")
    return tt


def plan(packed, xp0, Btab, env=None, dim=3, step=0.03, tol=0.06, max_iter=500,
         mode=GRAD_BACKGRAD_COMPAT, schedule="auto"):
    """Batched bidirectional planner (test/gib_plan.py:74-86; arm: test/arm_plan.py:140-152).

    Returns path (q, max_iter + 2, 2dim) — row 0 the start, frozen rows repeating the final
    state — and steps (q,) int32 (updates taken per query).  `schedule` picks the kernel
    (include/pntf.h pntf_plan_ex): "wave_tile" (one wave per 16 queries), "split_tile" (four
    waves share 16 queries: lower latency per step) or "auto"."""
    sched = _sched(schedule)
    lib = _lib.load()
    xp0, Bt, env = _prep(xp0, Btab, env, dim)
    q = xp0.shape[0]
    path = torch.empty((q, max_iter + 2, 2 * dim), dtype=torch.float32, device=xp0.device)
    steps = torch.empty(q, dtype=torch.int32, device=xp0.device)
    ws = _workspace(xp0.device, q)
    check(lib.pntf_plan_ex(_vp(packed), dim, _vp(xp0), q, _vp(Bt), _vp(env), Bt.shape[0],
                           mode, float(step), float(tol), int(max_iter), _vp(path), _vp(steps),
                           _vp(ws), ws.numel(), sched, _stream(xp0.device)),
          "pntf_plan_ex")
    return path, steps


def plan_handoff_counts(device):
    """(queries the 4-query tiles counted done, queries handed to the SOLO launch) of the last
    AUTO quad-tile plan on the current stream (pntf_plan_ex's tail counters at the start of
    the workspace, pntf_quad.h "Tail hand-off").  A query that runs to max_iter without
    converging is never counted done, so when more than CUs queries of a batch never converge
    the hand-off does not fire (results are unaffected; the plan just keeps its MFMA tiles):
    a zero second count shows that."""
    ws = _ws_cache.get(device, 8)
    c = ws[:8].view(torch.int32).cpu()
    return int(c[0]), int(c[1])


def eikonal_residual(packed, xp, Btab, env=None, dim=3, yobs=None, gamma=1e-3, want=("tau",
                     "dtau", "ltau", "diff")):
    """Taylor-mode τ, ∇τ, diagonal ∇²τ and the per-pair Eikonal residual of Model.Loss
    (NN.out_laplace :710-848, Loss :914-946).  Returns a dict of the requested outputs."""
    lib = _lib.load()
    xp, Bt, env = _prep(xp, Btab, env, dim)
    n = xp.shape[0]
    dv = xp.device
    out = {}
    if "tau" in want:
        out["tau"] = torch.empty(n, dtype=torch.float32, device=dv)
    if "dtau" in want:
        out["dtau"] = torch.empty((n, 2 * dim), dtype=torch.float32, device=dv)
    if "ltau" in want:
        out["ltau"] = torch.empty((n, 2 * dim), dtype=torch.float32, device=dv)
    yo = None
    if "diff" in want:
        if yobs is None:
            raise PntfError("the residual needs yobs (n, 2)")
        _require_device(yobs, "yobs")
        yo = yobs.detach().to(torch.float32).reshape(n, 2).contiguous()
        out["diff"] = torch.empty(n, dtype=torch.float32, device=dv)
    ws = _workspace(dv, n)
    check(lib.pntf_eikonal_residual(_vp(packed), dim, _vp(xp), _vp(yo), n, _vp(Bt), _vp(env),
                                    Bt.shape[0], float(gamma), _vp(out.get("tau")),
                                    _vp(out.get("dtau")), _vp(out.get("ltau")),
                                    _vp(out.get("diff")), _vp(ws), ws.numel(), _stream(dv)),
          "pntf_eikonal_residual")
    return out


def device_sum(x):
    """Deterministic fp64 sum of a float32 device tensor (pntf_sum); returns a 0-d float64
    device tensor."""
    lib = _lib.load()
    _require_device(x, "x")
    x = x.detach().to(torch.float32).contiguous().reshape(-1)
    out = torch.empty((), dtype=torch.float64, device=x.device)
    check(lib.pntf_sum(_vp(x), x.numel(), _vp(out), _stream(x.device)), "pntf_sum")
    return out


def _spread10(x):
    x = (x | (x << 16)) & 0x030000FF
    x = (x | (x << 8)) & 0x0300F00F
    x = (x | (x << 4)) & 0x030C30C3
    return (x | (x << 2)) & 0x09249249


def morton_order(pts):
    """Permutation putting pts (n, 3) in 30-bit Morton (Z-curve) order, on the device."""
    lo = pts.min(0).values
    span = (pts.max(0).values - lo).clamp_min(1e-30)
    q = ((pts - lo) / span * 1023.0).long().clamp_(0, 1023)
    code = _spread10(q[:, 0]) | (_spread10(q[:, 1]) << 1) | (_spread10(q[:, 2]) << 2)
    return torch.argsort(code)


def point_mesh_distance(pts, tris, chunks=0, order=None):
    """Unsigned distance (n,) from pts (n, 3) to the triangle mesh tris (t, 3, 3) on the HIP
    kernel (pntf_point_mesh_distance) — what point_obstacle_distance returns
    (dataprocessing/speed_sampling_gpu.py:325-336: bvh_distance_queries, then sqrt).
    `chunks` = 0 picks the triangle split automatically; every value gives the same bits.
    `order` (default: n >= 4096) queries the points in Morton order, so each workgroup's
    points are compact and the kernel's exact tile culling skips far triangles; results are
    scattered back, bit-identical to the unordered query."""
    _require_device(pts, "pts")
    _require_device(tris, "tris")
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise PntfError("pts must be (n, 3), got %s" % (tuple(pts.shape),))
    tris = tris.reshape(-1, 3, 3) if tris.dim() == 4 and tris.shape[0] == 1 else tris
    if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3):
        raise PntfError("tris must be (t, 3, 3) or (1, t, 3, 3), got %s" % (tuple(tris.shape),))
    if pts.device != tris.device:
        raise PntfError("pts and tris must be on the same device")
    pts = pts.detach().to(torch.float32).contiguous()
    tris = tris.detach().to(torch.float32).contiguous()
    out = torch.empty(pts.shape[0], dtype=torch.float32, device=pts.device)
    if pts.shape[0] == 0:
        return out
    if order is None:
        order = pts.shape[0] >= 4096
    perm = morton_order(pts) if order else None
    q = pts[perm].contiguous() if order else pts
    res = torch.empty_like(out) if order else out
    check(_lib.load().pntf_point_mesh_distance(_vp(q), q.shape[0], _vp(tris), tris.shape[0],
                                                _vp(res), int(chunks), _stream(pts.device)),
          "pntf_point_mesh_distance")
    if order:
        out[perm] = res
    return out


def _link_vertices(chain, link_verts, device):
    """verts (V, 3) on the device and the frames' CSR offsets (F + 1,) int32 on the host."""
    F = len(chain.link_names)
    if isinstance(link_verts, dict):
        unknown = sorted(set(link_verts) - set(chain.link_names))
        if unknown:
            raise PntfError("link_verts names links that are not in the chain: %s" % unknown)
        link_verts = [link_verts.get(name) for name in chain.link_names]
    link_verts = list(link_verts)
    if len(link_verts) != F:
        raise PntfError("link_verts must be a dict by link name or a list of %d entries (one "
                        "per frame), got %d" % (F, len(link_verts)))
    parts, voff = [], np.zeros(F + 1, dtype=np.int64)
    for f, v in enumerate(link_verts):
        if v is None:
            v = torch.zeros((0, 3), dtype=torch.float32, device=device)
        _require_device(v, "link_verts[%d]" % f)
        if v.dim() != 2 or v.shape[1] != 3:
            raise PntfError("link_verts[%d] must be (v, 3), got %s" % (f, tuple(v.shape)))
        if v.device != device:
            raise PntfError("link_verts and theta must be on the same device")
        parts.append(v.detach().to(torch.float32))
        voff[f + 1] = voff[f] + v.shape[0]
    if voff[-1] > 0x7fffffff:
        raise PntfError("too many link vertices")
    return torch.cat(parts).contiguous(), voff.astype(np.int32)


def arm_mesh_distance(theta, chain, link_verts, tris, cap=None):
    """Minimum distance (n,) from the collision vertices of an arm posed at each joint vector
    theta (n, chain.dof) to the triangle mesh tris (t, 3, 3) or (1, t, 3, 3), on the HIP
    kernel (pntf_arm_mesh_distance) — what arm_obstacle_distance returns
    (dataprocessing/speed_sampling_gpu.py:153-218).  `chain` is a kin.SerialChain;
    `link_verts` its links' vertices in link-local coordinates, a dict link name -> (v, 3)
    tensor (links without an entry own none) or a list aligned with the frames.  `cap` bounds
    the result (min(cap, distance), the same bits) and lets the kernel skip triangles farther
    than that; None = exact."""
    _require_device(theta, "theta")
    _require_device(tris, "tris")
    if theta.dim() != 2 or theta.shape[1] != chain.dof:
        raise PntfError("theta must be (n, %d), got %s" % (chain.dof, tuple(theta.shape)))
    tris = tris.reshape(-1, 3, 3) if tris.dim() == 4 and tris.shape[0] == 1 else tris
    if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3):
        raise PntfError("tris must be (t, 3, 3) or (1, t, 3, 3), got %s" % (tuple(tris.shape),))
    if theta.device != tris.device:
        raise PntfError("theta and tris must be on the same device")
    verts, voff = _link_vertices(chain, link_verts, theta.device)
    theta = theta.detach().to(torch.float32).contiguous()
    tris = tris.detach().to(torch.float32).contiguous()
    out = torch.empty(theta.shape[0], dtype=torch.float32, device=theta.device)
    if theta.shape[0] == 0:
        return out
    host = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    check(_lib.load().pntf_arm_mesh_distance(
        _vp(theta), theta.shape[0], chain.dof, len(chain.link_names), host(chain.origins),
        host(chain.types), host(chain.axes), host(chain.cols), _vp(verts), host(voff),
        _vp(tris), tris.shape[0], float("inf") if cap is None else float(cap), _vp(out),
        _stream(theta.device)), "pntf_arm_mesh_distance")
    return out


def polyline_mesh_distance(pts, cnt, tris, cap=None):
    """Clearance of q polylines from the triangle mesh tris (t, 3, 3) or (1, t, 3, 3) on the HIP
    kernel (pntf_polyline_mesh_distance): pts (q, L, 3), polyline c = its first cnt[c] points
    (cnt (q,) integer, 0..L), joined in order.  Returns (dist (q,) float32, where (q,) int32):
    the exact minimum over the polyline's SEGMENTS of the segment -> mesh distance — 0.0 where a
    segment passes through a triangle even if both its ends are clear — and the lowest segment
    index that attains it.  One point (cnt 1) gives the point distance with where 0; an empty
    polyline (cnt 0) gives inf (or cap) and where -1.  `cap` bounds the result (min(cap,
    distance), the same bits, where -1 if the cap decided) and lets the kernel skip triangles
    farther than that; None = exact."""
    _require_device(pts, "pts")
    _require_device(cnt, "cnt")
    _require_device(tris, "tris")
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise PntfError("pts must be (q, L, 3), got %s" % (tuple(pts.shape),))
    if cnt.dim() != 1 or cnt.shape[0] != pts.shape[0] or cnt.is_floating_point():
        raise PntfError("cnt must be (q,) integers, one per polyline, got %s %s"
                        % (tuple(cnt.shape), cnt.dtype))
    tris = tris.reshape(-1, 3, 3) if tris.dim() == 4 and tris.shape[0] == 1 else tris
    if tris.dim() != 3 or tuple(tris.shape[1:]) != (3, 3):
        raise PntfError("tris must be (t, 3, 3) or (1, t, 3, 3), got %s" % (tuple(tris.shape),))
    if not (pts.device == cnt.device == tris.device):
        raise PntfError("pts, cnt and tris must be on the same device")
    lib = _lib.load()
    pts = pts.detach().to(torch.float32).contiguous()
    cnt = cnt.detach().to(torch.int32).contiguous()
    tris = tris.detach().to(torch.float32).contiguous()
    q, L = pts.shape[0], pts.shape[1]
    dist = torch.empty(q, dtype=torch.float32, device=pts.device)
    where = torch.empty(q, dtype=torch.int32, device=pts.device)
    if q == 0:
        return dist, where
    ws = _ws_cache.get(pts.device, int(lib.pntf_polyline_workspace_bytes(q)))
    check(lib.pntf_polyline_mesh_distance(
        _vp(pts), q, L, _vp(cnt), _vp(tris), tris.shape[0],
        float("inf") if cap is None else float(cap), _vp(dist), _vp(where), _vp(ws), ws.numel(),
        _stream(pts.device)), "pntf_polyline_mesh_distance")
    return dist, where


def plan_polylines(path, steps):
    """The planner's output as polylines: path (q, max_iter + 2, 2·dim) and steps (q,) of
    `plan` -> (pts (q, 2·(max_iter + 2), dim), cnt (q,) int32).  Query c's polyline is its start
    side path[c, 0..steps[c], :dim] followed by its goal side path[c, steps[c]..0, dim:] — the
    reference's point0 + reversed(point1) (test/gib_plan.py:92-93) — 2·steps[c] + 2 points;
    the junction between the two sides is a segment like any other.  steps -1 (invalid env)
    gives cnt 0; rows past cnt are zero.  Pure indexing: runs on CPU tensors too."""
    if path.dim() != 3 or path.shape[2] % 2 or steps.dim() != 1 or \
            steps.shape[0] != path.shape[0]:
        raise PntfError("path must be (q, rows, 2·dim) and steps (q,), got %s and %s"
                        % (tuple(path.shape), tuple(steps.shape)))
    q, rows, dim = path.shape[0], path.shape[1], path.shape[2] // 2
    s = steps.to(device=path.device, dtype=torch.int64)
    if q and int(s.max()) >= rows:
        raise PntfError("steps exceeds the path's rows")
    cnt = torch.where(s >= 0, 2 * s + 2, torch.zeros_like(s))
    s = s.clamp(min=0)[:, None]
    j = torch.arange(2 * rows, device=path.device)[None, :]
    first = j <= s
    row = torch.where(first, j, 2 * s + 1 - j).clamp(0, rows - 1)
    src = path.gather(1, row[:, :, None].expand(q, 2 * rows, 2 * dim))
    pts = torch.where(first[:, :, None], src[:, :, :dim], src[:, :, dim:])
    pts = pts * (j < cnt[:, None])[:, :, None]
    return pts.contiguous(), cnt.to(torch.int32)


def _grid_args(speed, what):
    _require_device(speed, "speed")
    if speed.dim() != 3 or not (speed.shape[0] == speed.shape[1] == speed.shape[2]) or \
            speed.shape[0] < 2:
        raise PntfError("%s: speed must be (n, n, n) with n >= 2, got %s"
                        % (what, tuple(speed.shape)))
    return speed.detach().to(torch.float32).contiguous()


def _grid_sources(src, speed, what):
    _require_device(src, "src")
    if src.dim() == 1:
        src = src[None]
    if src.dim() != 2 or src.shape[1] != 3 or src.shape[0] < 1:
        raise PntfError("%s: src must be (q, 3) with q >= 1, got %s" % (what, tuple(src.shape)))
    if src.device != speed.device:
        raise PntfError("%s: speed and src must be on the same device" % what)
    return src.detach().to(torch.float32).contiguous()


def grid_travel_time_init(speed, src, radius=4.0):
    """Initial state T (q, n, n, n) of the grid solver (pntf_grid_travel_time_init): +inf, except
    |x - x_s| / S_near at the node nearest each source and within radius·h of it."""
    speed = _grid_args(speed, "grid_travel_time_init")
    src = _grid_sources(src, speed, "grid_travel_time_init")
    n, q = speed.shape[0], src.shape[0]
    T = torch.empty((q, n, n, n), dtype=torch.float32, device=speed.device)
    check(_lib.load().pntf_grid_travel_time_init(_vp(speed), n, _vp(src), q, float(radius),
                                                  _vp(T), _stream(speed.device)),
          "pntf_grid_travel_time_init")
    return T


def grid_travel_time_pass(speed, T, inner=8, changed=None):
    """One pass of the grid solver on T (q, n, n, n) (pntf_grid_travel_time_pass): returns (a
    new tensor with every 8x8x8 tile advanced by `inner` sweeps, changed (q,) int32).  `changed`
    is accumulated into when given, else starts from zero."""
    speed = _grid_args(speed, "grid_travel_time_pass")
    _require_device(T, "T")
    n = speed.shape[0]
    if T.dim() != 4 or tuple(T.shape[1:]) != (n, n, n) or T.dtype != torch.float32 or \
            not T.is_contiguous() or T.device != speed.device or T.shape[0] < 1:
        raise PntfError("grid_travel_time_pass: T must be a contiguous float32 (q, %d, %d, %d) "
                        "tensor on the speed's device" % (n, n, n))
    q = T.shape[0]
    if changed is None:
        changed = torch.zeros(q, dtype=torch.int32, device=T.device)
    elif changed.shape != (q,) or changed.dtype != torch.int32 or changed.device != T.device \
            or not changed.is_contiguous():
        raise PntfError("grid_travel_time_pass: changed must be (q,) int32 on T's device")
    out = torch.empty_like(T)
    check(_lib.load().pntf_grid_travel_time_pass(_vp(speed), n, q, _vp(T), _vp(out), int(inner),
                                                  _vp(changed), _stream(T.device)),
          "pntf_grid_travel_time_pass")
    return out, changed


def grid_travel_time(speed, src, radius=4.0, inner=8, check_every=4, max_passes=None):
    """Travel time from each source src (q, 3) to every node of the n^3 grid of the unit box
    under the speed field speed (n, n, n) (node (i, j, k) at -0.5 + (i, j, k) / (n - 1); a node
    with speed <= 0 is a wall): the fixed point of the first-order upwind Eikonal scheme of
    include/pntf.h, i.e. the fast-marching solution, on the HIP kernels.

    Returns (T (q, n, n, n) float32 — +inf at walls and where no path leads —, passes (q,)
    int32, converged (q,) bool).  The host launches `check_every` passes (each: `inner` sweeps
    per 8x8x8 tile), reads the per-source change counters — the only synchronisation —, and
    repeats until a whole interval changed nothing for every source or `max_passes` (default
    8·n) passes have run; running out gives converged False, never an exception.  passes[c] is
    the number of passes launched when source c's counter first read 0 (max_passes otherwise).
    A converged T is the fixed point: its bits depend neither on check_every nor on the other
    sources of the batch.  A non-finite speed raises PntfError."""
    speed = _grid_args(speed, "grid_travel_time")
    src = _grid_sources(src, speed, "grid_travel_time")
    n, q = speed.shape[0], src.shape[0]
    if int(check_every) < 1 or int(inner) < 1:
        raise PntfError("grid_travel_time: inner and check_every must be >= 1")
    max_passes = 8 * n if max_passes is None else int(max_passes)
    if max_passes < 1:
        raise PntfError("grid_travel_time: max_passes must be >= 1")
    if not bool(torch.isfinite(speed).all()) or not bool(torch.isfinite(src).all()):
        raise PntfError("grid_travel_time: speed and src must be finite")
    lib, dev = _lib.load(), speed.device
    cur = grid_travel_time_init(speed, src, radius)
    nxt = torch.empty_like(cur)
    changed = torch.zeros(q, dtype=torch.int32, device=dev)
    passes = torch.full((q,), max_passes, dtype=torch.int32)
    converged = torch.zeros(q, dtype=torch.bool)
    done = 0
    while done < max_passes:
        for _ in range(min(int(check_every), max_passes - done)):
            check(lib.pntf_grid_travel_time_pass(_vp(speed), n, q, _vp(cur), _vp(nxt),
                                                 int(inner), _vp(changed), _stream(dev)),
                  "pntf_grid_travel_time_pass")
            cur, nxt = nxt, cur
            done += 1
        still = changed.cpu() == 0
        changed.zero_()
        passes[still & ~converged] = done
        converged |= still
        if bool(converged.all()):
            break
    return cur, passes.to(dev), converged.to(dev)


def grid_nodes(n, device):
    """Node coordinates (n^3, 3) float32 of the solver's grid, k fastest: -0.5 + (i, j, k) /
    (n - 1), evaluated in fp64 and rounded once."""
    ax = torch.arange(n, dtype=torch.float64, device=device) * (1.0 / (n - 1)) - 0.5
    return torch.stack(torch.meshgrid(ax, ax, ax, indexing="ij"), dim=-1).reshape(-1, 3).to(
        torch.float32)


def speed_grid(tris, n, offset, margin):
    """Ground-truth speed (n, n, n) at the solver's nodes for the obstacle mesh tris (t, 3, 3):
    clip(d, offset, margin) / margin with d = point_mesh_distance(nodes, tris) — the speed the
    samplers label their points with (dataprocessing/speed_sampling_gpu.py:415-419)."""
    _require_device(tris, "tris")
    if int(n) < 2 or not (0 <= offset <= margin and margin > 0):
        raise PntfError("speed_grid: need n >= 2 and 0 <= offset <= margin, margin > 0")
    d = point_mesh_distance(grid_nodes(int(n), tris.device), tris)
    return (d.clamp(float(offset), float(margin)) / float(margin)).reshape(n, n, n)


def _grid_points(p, q, what, name):
    _require_device(p, name)
    if p.dim() == 1:
        p = p[None]
    if p.dim() != 2 or p.shape[1] != 3 or (q is not None and p.shape[0] != q):
        raise PntfError("%s: %s must be (q, 3)%s, got %s"
                        % (what, name, "" if q is None else " with q = %d" % q, tuple(p.shape)))
    return p.detach().to(torch.float32).contiguous()


def grid_descent(T, src, goal, radius=4.0, step=0.5, max_points=None):
    """The minimum-time paths out of solved grid travel times (pntf_grid_descent): T (q, n, n, n)
    as `grid_travel_time` returned it for src (q, 3) with init radius `radius`, goal (q, 3) the
    points to descend from.  From the goal, steps of step·h (0 < step <= 1, h = 1 / (n - 1))
    against the gradient of the trilinear interpolant of T, until within max(radius, 2)·h of the
    source, where the path closes with a straight segment (include/pntf.h).

    Returns (pts (q, L, 3) float32 — row 0 the goal, rows past cnt zero —, cnt (q,) int32 >= 1,
    status (q,) int32: 0 ARRIVED, 1 TRUNCATED (needed more than L rows), 2 STALLED (no descent:
    a flat or non-finite gradient, or a step that did not lower T), 3 BLOCKED (stepped into a
    cell with a +inf corner), 4 UNREACHABLE (the goal's own cell has one) —, tgoal (q,) float32:
    the interpolated T at the goal, the optimal travel time, +inf when unreachable).
    L = max_points defaults to ceil(4·(n - 1) / step) + 2.  A query's bits depend neither on the
    batch nor on L beyond truncation.  Non-finite points raise PntfError before any launch."""
    what = "grid_descent"
    _require_device(T, "T")
    if T.dim() != 4 or not (T.shape[1] == T.shape[2] == T.shape[3]) or T.shape[1] < 2:
        raise PntfError("%s: T must be (q, n, n, n) with n >= 2, got %s" % (what, tuple(T.shape)))
    q, n = T.shape[0], T.shape[1]
    src = _grid_points(src, q, what, "src")
    goal = _grid_points(goal, q, what, "goal")
    if not (src.device == goal.device == T.device):
        raise PntfError("%s: T, src and goal must be on the same device" % what)
    step, radius = float(step), float(radius)
    if not (0.0 < step <= 1.0):
        raise PntfError("%s: step must be in (0, 1], got %r" % (what, step))
    if not radius >= 0.0:
        raise PntfError("%s: radius must be >= 0, got %r" % (what, radius))
    L = int(np.ceil(4.0 * (n - 1) / step)) + 2 if max_points is None else int(max_points)
    if L < 2:
        raise PntfError("%s: max_points must be >= 2, got %d" % (what, L))
    T = T.detach().to(torch.float32).contiguous()
    dev = T.device
    pts = torch.empty((q, L, 3), dtype=torch.float32, device=dev)
    cnt = torch.empty(q, dtype=torch.int32, device=dev)
    status = torch.empty(q, dtype=torch.int32, device=dev)
    tgoal = torch.empty(q, dtype=torch.float32, device=dev)
    if q == 0:
        return pts, cnt, status, tgoal
    if not bool(torch.isfinite(src).all()) or not bool(torch.isfinite(goal).all()):
        raise PntfError("%s: src and goal must be finite" % what)
    check(_lib.load().pntf_grid_descent(_vp(T), n, q, _vp(src), _vp(goal), radius, step, L,
                                        _vp(pts), _vp(cnt), _vp(status), _vp(tgoal),
                                        _stream(dev)), "pntf_grid_descent")
    return pts, cnt, status, tgoal


def grid_polyline_time(speed, pts, cnt, sub=0.5):
    """Travel time (q,) float32 of the polylines pts (q, L, 3), cnt (q,) integers (the first
    cnt[c] points, joined in order) under the node speed grid speed (n, n, n), on the HIP kernel
    (pntf_grid_polyline_time): every segment is cut into pieces of at most sub·h (sub > 0) and
    each piece adds its length over the trilinear speed at its midpoint.  +inf when a midpoint
    falls in a cell with a wall (speed <= 0) corner; 0 for cnt <= 1.  Points outside the box
    count with their full length at the speed of the nearest point of the box.  The bits depend
    neither on L nor on the other rows.  Non-finite points raise PntfError before any launch."""
    what = "grid_polyline_time"
    speed = _grid_args(speed, what)
    _require_device(pts, "pts")
    _require_device(cnt, "cnt")
    if pts.dim() != 3 or pts.shape[2] != 3:
        raise PntfError("%s: pts must be (q, L, 3), got %s" % (what, tuple(pts.shape)))
    if cnt.dim() != 1 or cnt.shape[0] != pts.shape[0] or cnt.is_floating_point():
        raise PntfError("%s: cnt must be (q,) integers, one per polyline, got %s %s"
                        % (what, tuple(cnt.shape), cnt.dtype))
    if not (pts.device == cnt.device == speed.device):
        raise PntfError("%s: speed, pts and cnt must be on the same device" % what)
    sub = float(sub)
    if not (0.0 < sub < float("inf")):
        raise PntfError("%s: sub must be > 0, got %r" % (what, sub))
    q, L = pts.shape[0], pts.shape[1]
    time = torch.zeros(q, dtype=torch.float32, device=pts.device)
    if q == 0 or L == 0:
        return time
    pts = pts.detach().to(torch.float32).contiguous()
    cnt = cnt.detach().to(torch.int32).contiguous()
    if not bool(torch.isfinite(pts).all()):
        raise PntfError("%s: pts must be finite" % what)
    check(_lib.load().pntf_grid_polyline_time(_vp(speed), speed.shape[0], _vp(pts), q, L,
                                              _vp(cnt), sub, _vp(time), _stream(pts.device)),
          "pntf_grid_polyline_time")
    return time
