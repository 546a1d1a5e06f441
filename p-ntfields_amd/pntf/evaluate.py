"""Evaluation of planned paths: did the planner converge, how long is the path, and does it
stay clear of the obstacle mesh — the success rate NTFields results are judged by, which the
reference's own scripts leave to an open3d viewer (test/gib_plan.py:92-109, test/arm_plan.py).

`path_report` works on the output of `ops.plan` / `Model.Plan`.  In workspace planning (dim 3)
the clearance is exact: the minimum segment -> triangle distance of the path's polyline on the
HIP kernel (ops.polyline_mesh_distance), so a step through a thin wall counts as a collision
even when both its ends are clear.  For the arm (joint space) the clearance is SAMPLED:
`arm_path_samples` subdivides every segment linearly in joint space and
`arm_path_clearance` takes the minimum of ops.arm_mesh_distance over the samples.

`field_report` judges the FIELD instead of a path: the model's TravelTimes and Speed at the
nodes of a grid over the box against the scene's ground truth — the speed from the exact
point -> mesh distance, and the travel time from a grid Eikonal solve of that speed
(ops.grid_travel_time) — together with the solver's own discretisation error at that grid.

`path_optimality` says how good a successful path is: its travel time and length against the
grid optimum — the minimum-time path out of that same grid solve (ops.grid_descent), both
priced under the same speed grid (ops.grid_polyline_time) — with the grid's own resolution
(`floor_rel`) beside the ratios.
"""
import dataclasses
import math

import torch

from . import ops
from ._lib import DESCENT_ARRIVED, PntfError

ARM_SCALE = math.pi / 0.5     # normalised joint coordinates -> radians (test/arm_plan.py)


@dataclasses.dataclass
class PathReport:
    """Per-query tensors (q,) and the batch's success rate."""
    converged: torch.Tensor     # bool: final |x_g - x_s| <= tol
    length: torch.Tensor        # float64: summed segment lengths of the polyline
    clearance: torch.Tensor     # float32: minimum distance to the mesh (inf for an empty path)
    where: torch.Tensor         # int32: segment of the minimum (-1: none)
    success: torch.Tensor       # bool: converged & (clearance > safety)
    success_rate: float         # mean of success (nan for an empty batch)


def polyline_length(pts, cnt):
    """Summed segment lengths (q,) float64 of the polylines pts (q, L, dim), cnt (q,)."""
    p = pts.to(torch.float64)
    seg = (p[:, 1:] - p[:, :-1]).norm(dim=2)
    j = torch.arange(seg.shape[1], device=pts.device)[None, :]
    return (seg * (j < cnt.to(torch.int64)[:, None] - 1)).sum(dim=1)


def path_report(path, steps, tol, *, tris=None, safety=0.0, cap=None, clearance=None,
                where=None):
    """Report on planned paths: path (q, max_iter + 2, 2·dim), steps (q,) as `ops.plan` returns
    them, `tol` the planner's tolerance.

      converged   final |x_g - x_s| <= tol, read from the last valid row path[c, steps[c]] (not
                  from steps: a query that used all its iterations may or may not have arrived);
                  False for steps -1 (invalid env)
      length      length of the polyline ops.plan_polylines builds (start side, junction, goal
                  side), accumulated in fp64
      clearance   minimum distance from the polyline's segments to the mesh `tris` (dim 3 only:
                  ops.polyline_mesh_distance, exact), or the `clearance` (and `where`) given by
                  the caller, e.g. the arm's sampled one (arm_path_clearance)
      where       segment index of that minimum, -1 if there is none
      success     converged & (clearance > safety)

    `cap` is passed to the kernel (distances above it are reported as cap); it must exceed
    `safety` to leave `success` unchanged."""
    if path.dim() != 3 or path.shape[2] % 2:
        raise PntfError("path must be (q, rows, 2·dim), got %s" % (tuple(path.shape),))
    q, dim = path.shape[0], path.shape[2] // 2
    pts, cnt = ops.plan_polylines(path, steps)
    s = steps.to(device=path.device, dtype=torch.int64)
    final = path.gather(1, s.clamp(min=0)[:, None, None].expand(q, 1, 2 * dim))[:, 0]
    converged = ((final[:, dim:] - final[:, :dim]).norm(dim=1) <= tol) & (s >= 0)
    if clearance is None:
        if tris is None:
            raise PntfError("path_report needs the mesh `tris` or a `clearance`")
        if dim != 3:
            raise PntfError("the mesh clearance of a path is defined for dim 3 (workspace "
                            "planning); pass the arm's sampled clearance (arm_path_clearance)")
        if cap is not None and not cap > safety:
            raise PntfError("cap must exceed safety")
        clearance, where = ops.polyline_mesh_distance(pts, cnt, tris, cap=cap)
    else:
        clearance = clearance.to(path.device)
        if clearance.shape != (q,):
            raise PntfError("clearance must be (q,), got %s" % (tuple(clearance.shape),))
        if where is None:
            where = torch.full((q,), -1, dtype=torch.int32, device=path.device)
    success = converged & (clearance > safety)
    rate = float(success.to(torch.float64).mean()) if q else float("nan")
    return PathReport(converged, polyline_length(pts, cnt), clearance, where, success, rate)


GIBSON_MARGIN = 0.5 / 12.0    # dataprocessing/speed_sampling_gpu.py:470-472; offset = margin / 10


@dataclasses.dataclass
class FieldReport:
    """Per-source tensors (q,) on the device, and the two grids they were taken on."""
    converged: torch.Tensor       # bool: the grid solve reached its fixed point
    passes: torch.Tensor          # int32: passes of the grid solve
    tt_mean_rel: torch.Tensor     # float64: mean |T_model - T_grid| / T_grid
    tt_max_rel: torch.Tensor      # float64: max of the same
    speed_mean_abs: torch.Tensor  # float64: mean |Speed - speed grid| over all nodes
    speed_max_abs: torch.Tensor   # float64: max of the same
    floor_mean_rel: torch.Tensor  # float64: the solver's own mean relative error at this n
    floor_max_rel: torch.Tensor   # float64: max of the same
    T_grid: torch.Tensor          # float32 (q, n, n, n): the grid travel times
    speed: torch.Tensor           # float32 (n, n, n): the ground-truth speed at the nodes


def field_report(travel_times, speed, tris, sources, n=65, offset=None, margin=None, radius=4.0):
    """How far a model's field is from the true travel time of a scene.  `travel_times` and
    `speed` are the model's epilogues (callables on (N, 6) pairs [x_start | x_goal] returning
    (N,) or (N, 1): Model.TravelTimes and Model.Speed), `tris` (t, 3, 3) the obstacle mesh,
    `sources` (q, 3) start points in the box [-0.5, 0.5]^3.  dim 3 only.

    Ground truth: the speed the samplers label points with, clip(d, offset, margin) / margin
    (ops.speed_grid; defaults: the reference's Gibson values margin = 0.5/12, offset =
    margin/10), at the n^3 nodes of the box, and T_grid = ops.grid_travel_time of that speed
    from each source: the first-order upwind Eikonal solution, initialised exactly within
    `radius` nodes of the source.  Per source:

      converged, passes          of the grid solve
      tt_mean_rel, tt_max_rel    |T_model - T_grid| / T_grid, T_model = travel_times from the
                                 source to every node, over the nodes outside the initial ball
                                 whose T_grid is finite
      speed_mean_abs, _max_abs   |speed(source -> node) - speed grid| over all nodes; the speed
                                 grid is exact, so this row has no resolution limit
      floor_mean_rel, _max_rel   the solver's own discretisation error at this n: a second solve
                                 with speed 1 everywhere, same source and radius, against
                                 |x - x_s|, relative, over the same nodes as the tt rows

    T_grid is itself a first-order approximation, a few percent off at n = 33..65 (the floor_*
    rows measure it in free space): a travel-time error BELOW THE FLOOR IS NOT RESOLVED at this
    n — raise n, do not read it as model error.  Rows over an empty node set are nan."""
    _require = ops._require_device
    _require(tris, "tris")
    _require(sources, "sources")
    if sources.dim() != 2 or sources.shape[1] != 3 or sources.shape[0] < 1:
        raise PntfError("sources must be (q, 3) with q >= 1 (the field report is defined for "
                        "dim 3), got %s" % (tuple(sources.shape),))
    margin = GIBSON_MARGIN if margin is None else float(margin)
    offset = margin / 10.0 if offset is None else float(offset)
    dev, n = tris.device, int(n)
    src = sources.detach().to(device=dev, dtype=torch.float32).contiguous()
    q = src.shape[0]
    S = ops.speed_grid(tris, n, offset, margin)
    T, passes, converged = ops.grid_travel_time(S, src, radius=radius)
    ones = torch.ones_like(S)
    U, _, _ = ops.grid_travel_time(ones, src, radius=radius)
    outside = ~torch.isfinite(ops.grid_travel_time_init(ones, src, radius)).reshape(q, -1)
    nodes = ops.grid_nodes(n, dev)
    rows = {k: torch.full((q,), float("nan"), dtype=torch.float64, device=dev)
            for k in ("tt_mean_rel", "tt_max_rel", "speed_mean_abs", "speed_max_abs",
                      "floor_mean_rel", "floor_max_rel")}
    for c in range(q):
        xp = torch.cat([src[c].expand(n ** 3, 3), nodes], dim=1).contiguous()
        with torch.no_grad():
            tm = travel_times(xp).reshape(-1).to(torch.float64)
            sm = speed(xp).reshape(-1).to(torch.float64)
        tg = T[c].reshape(-1).to(torch.float64)
        m = outside[c] & torch.isfinite(tg)
        es = (sm - S.reshape(-1).to(torch.float64)).abs()
        rows["speed_mean_abs"][c], rows["speed_max_abs"][c] = es.mean(), es.max()
        if bool(m.any()):
            et = ((tm - tg).abs() / tg)[m]
            dist = (nodes.to(torch.float64) - src[c].to(torch.float64)).norm(dim=1)
            ef = ((U[c].reshape(-1).to(torch.float64) - dist).abs() / dist)[m]
            rows["tt_mean_rel"][c], rows["tt_max_rel"][c] = et.mean(), et.max()
            rows["floor_mean_rel"][c], rows["floor_max_rel"][c] = ef.mean(), ef.max()
    return FieldReport(converged=converged, passes=passes, T_grid=T, speed=S, **rows)


@dataclasses.dataclass
class PathOptimality:
    """Per-query tensors (q,) on the device.  float64 rows are nan where undefined."""
    time: torch.Tensor               # float64: travel time of the planned polyline
    length: torch.Tensor             # float64: its length
    optimal_time: torch.Tensor       # float64: the grid's T at the goal (tgoal)
    optimal_path_time: torch.Tensor  # float64: travel time of the grid's own path
    optimal_length: torch.Tensor     # float64: its length
    time_ratio: torch.Tensor         # float64: time / optimal_time
    length_ratio: torch.Tensor       # float64: length / optimal_length
    status: torch.Tensor             # int32: the descent's status (0 = ARRIVED)
    solve_converged: torch.Tensor    # bool: the grid solve reached its fixed point
    floor_rel: torch.Tensor          # float64: |optimal_path_time - optimal_time| / optimal_time


def path_optimality(path, steps, tris, n=65, offset=None, margin=None, radius=4.0, step=0.5,
                    chunk=64):
    """How good a planned path is against the grid optimum.  path (q, max_iter + 2, 6) and
    steps (q,) as `ops.plan` returns them, `tris` (t, 3, 3) the obstacle mesh.  dim 3 only.

    The baseline is fast marching on a grid, the one NTFields planners are judged against: the
    scene's true speed at the n^3 nodes (ops.speed_grid, with field_report's defaults), the
    grid travel time T from each query's start path[c, 0, :3] (ops.grid_travel_time, init radius
    `radius`) and the minimum-time path from its goal path[c, 0, 3:] back down T
    (ops.grid_descent, steps of step·h).  Both the planned polyline (ops.plan_polylines) and
    the grid's path are priced under that same speed grid (ops.grid_polyline_time).  Queries
    are solved `chunk` at a time, which bounds the solver's state at 2·chunk·n^3·4 bytes; the
    result does not depend on chunk.  Per query:

      time, length                 of the planned polyline (length: polyline_length)
      optimal_time                 T interpolated at the goal
      optimal_path_time, _length   of the grid's own path
      time_ratio, length_ratio     time / optimal_time, length / optimal_length
      status, solve_converged      of the descent (0 = ARRIVED) and of the grid solve
      floor_rel                    |optimal_path_time - optimal_time| / optimal_time

    floor_rel is the disagreement of the grid's own path with the grid's own T: two first-order
    answers to the same question at this n, a few percent apart at n = 17..65.  It is the
    resolution of the comparison: a time_ratio WITHIN floor_rel OF 1 IS NOT RESOLVED at this
    n — raise n, do not read it as the planner beating or missing the optimum.  The float rows
    are nan where undefined: the planned path's rows (time, length, both ratios) for steps -1
    (invalid env), the optimum's rows (optimal_*, floor_rel, both ratios) for a descent that
    did not ARRIVE or a non-finite optimum (a goal in a cell with a wall corner)."""
    _require = ops._require_device
    _require(path, "path")
    _require(steps, "steps")
    _require(tris, "tris")
    if path.dim() != 3 or path.shape[2] != 6 or path.shape[1] < 1:
        raise PntfError("path must be (q, rows, 6): the optimality report is defined for dim "
                        "3, got %s" % (tuple(path.shape),))
    if int(chunk) < 1:
        raise PntfError("chunk must be >= 1")
    margin = GIBSON_MARGIN if margin is None else float(margin)
    offset = margin / 10.0 if offset is None else float(offset)
    dev, n, q = path.device, int(n), path.shape[0]
    path = path.detach().to(torch.float32)
    ppts, pcnt = ops.plan_polylines(path, steps)
    S = ops.speed_grid(tris.to(dev), n, offset, margin)
    f64 = dict(dtype=torch.float64, device=dev)
    opt_time, opt_path_time = torch.empty(q, **f64), torch.empty(q, **f64)
    opt_length = torch.empty(q, **f64)
    status = torch.empty(q, dtype=torch.int32, device=dev)
    converged = torch.empty(q, dtype=torch.bool, device=dev)
    for lo in range(0, q, int(chunk)):
        sl = slice(lo, min(lo + int(chunk), q))
        src, goal = path[sl, 0, :3].contiguous(), path[sl, 0, 3:].contiguous()
        T, _, conv = ops.grid_travel_time(S, src, radius=radius)
        dpts, dcnt, st, tgoal = ops.grid_descent(T, src, goal, radius=radius, step=step)
        opt_time[sl], status[sl], converged[sl] = tgoal.to(torch.float64), st, conv
        opt_path_time[sl] = ops.grid_polyline_time(S, dpts, dcnt).to(torch.float64)
        opt_length[sl] = polyline_length(dpts, dcnt)
    time = ops.grid_polyline_time(S, ppts, pcnt).to(torch.float64) if q else torch.empty(q, **f64)
    length = polyline_length(ppts, pcnt)
    opt = (status == DESCENT_ARRIVED) & torch.isfinite(opt_time) & torch.isfinite(opt_path_time)
    planned = steps.to(dev) >= 0
    nan = torch.full((q,), float("nan"), **f64)
    rows = dict(optimal_time=(opt_time, opt), optimal_path_time=(opt_path_time, opt),
                optimal_length=(opt_length, opt),
                floor_rel=((opt_path_time - opt_time).abs() / opt_time, opt),
                time=(time, planned), length=(length, planned),
                time_ratio=(time / opt_time, planned & opt),
                length_ratio=(length / opt_length, planned & opt))
    rows = {k: torch.where(ok, v, nan) for k, (v, ok) in rows.items()}
    return PathOptimality(status=status, solve_converged=converged, **rows)


def arm_path_samples(pts, cnt, resolution, scale=ARM_SCALE):
    """Joint-space samples of the polylines pts (q, L, dof) (normalised coordinates), cnt (q,):
    every segment is subdivided linearly into ceil(max_j |Δθ_j| / resolution) pieces (at least
    one), Δθ in radians (= scale · Δ), so no joint moves more than `resolution` between
    consecutive samples; each piece contributes its first point and every polyline its last
    point.  Returns (theta (n, dof) radians, query (n,) int64, segment (n,) int64), ordered by
    query, then along the path; the last point belongs to the last segment."""
    if not resolution > 0:
        raise PntfError("resolution must be > 0 radians")
    q, L, dof = pts.shape
    dev = pts.device
    cnt = cnt.to(device=dev, dtype=torch.int64)
    delta = pts[:, 1:] - pts[:, :-1]                                    # (q, L-1, dof)
    move = delta.abs().amax(dim=2).to(torch.float64) * scale
    pieces = torch.ceil(move / resolution).clamp(min=1).to(torch.int64)
    live = torch.arange(max(L - 1, 0), device=dev)[None, :] < cnt[:, None] - 1
    pieces = pieces * live
    flat = pieces.reshape(-1)
    seg_id = torch.repeat_interleave(torch.arange(flat.numel(), device=dev), flat)
    first = torch.cumsum(flat, 0) - flat
    k = torch.arange(seg_id.numel(), device=dev) - first[seg_id]
    frac = (k.to(torch.float64) / flat[seg_id].to(torch.float64)).to(pts.dtype)
    qi, si = seg_id // max(L - 1, 1), seg_id % max(L - 1, 1)
    theta = pts[qi, si] + frac[:, None] * delta.reshape(-1, dof)[seg_id]
    # the last point of every non-empty polyline
    has = torch.nonzero(cnt > 0)[:, 0]
    theta = torch.cat([theta, pts[has, cnt[has] - 1]])
    qi = torch.cat([qi, has])
    si = torch.cat([si, (cnt[has] - 2).clamp(min=0)])
    order = torch.argsort(qi, stable=True)
    return theta[order] * scale, qi[order], si[order]


def arm_path_clearance(pts, cnt, chain, link_verts, tris, resolution=0.05, scale=ARM_SCALE):
    """SAMPLED clearance of joint-space polylines (not exact: the arm may come closer between
    two samples): the minimum of ops.arm_mesh_distance over arm_path_samples(pts, cnt,
    resolution), and the segment of the (first) minimising sample.  Returns (clearance (q,)
    float32 — inf for an empty polyline — and where (q,) int32, -1 for an empty polyline)."""
    q = pts.shape[0]
    theta, qi, si = arm_path_samples(pts, cnt, resolution, scale)
    d = ops.arm_mesh_distance(theta, chain, link_verts, tris)
    clearance = torch.full((q,), float("inf"), dtype=torch.float32, device=pts.device)
    clearance.scatter_reduce_(0, qi, d, "amin")
    n = theta.shape[0]
    idx = torch.where(d == clearance[qi], torch.arange(n, device=pts.device),
                      torch.full((n,), n, device=pts.device))
    firstmin = torch.full((q,), n, dtype=torch.int64, device=pts.device)
    firstmin.scatter_reduce_(0, qi, idx, "amin")
    where = torch.where(firstmin < n, si[firstmin.clamp(max=max(n - 1, 0))] if n else firstmin,
                        torch.full_like(firstmin, -1))
    return clearance, where.to(torch.int32)
