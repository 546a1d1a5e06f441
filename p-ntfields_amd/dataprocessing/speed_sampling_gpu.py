"""Drop-in for the point (Gibson / 3-D) speed-sample generator of yhsong0804/P-NTFields,
`dataprocessing/speed_sampling_gpu.py`.

Same function names, arguments and return values as the reference's
  point_obstacle_distance(query_points, triangles_obs)            (:325-336)
  point_append_list(X_list, Y_list, triangles_obs, numsamples, dim, offset, margin)
                                                                     (:338-391)
  point_rand_sample_bound_points(numsamples, dim, v_obs, f_obs, offset, margin)
                                                                     (:393-421)
with the distance query on the HIP kernel pntf_point_mesh_distance instead of the CUDA
extension bvh_distance_queries.  Sampling follows the reference step for step: 8·numsamples
start points P ~ U[-0.5,0.5]^dim, goals nP = P + normalize(dP)·U[0,√dim), keep pairs whose
goal is inside the box, keep starts with offset < d(P) < margin, then query d(nP); repeat
until more than numsamples pairs; speed = clip(d, offset, margin)/margin.  Randomness is
torch's generator on the device, as in the reference, so outputs are reproducible under a
seed but not bit-equal to the reference's own draws.

The arm (6-dof) generator, with the reference's names and arguments as well:
  arm_obstacle_distance(th_batch, chain, out_path_, triangles_obs)   (:153-218)
      minimum distance of the posed arm's collision vertices to the mesh, per configuration,
      on the fused HIP kernel pntf_arm_mesh_distance (FK + distance + minimum);
  arm_append_list(X_list, Y_list, chain, out_path_, triangles_obs, numsamples, dim, offset,
                  margin)                                            (:220-285)
      5·numsamples draws, rL ~ U[0, √3) whatever dim is, theta = 2π·x, keep
      offset <= d0 <= margin (inclusive), same loop exits; `arm_obstacle_obb` (:77-151) is
      not restated (see the function);
  arm_rand_sample_bound_points(numsamples, dim, v_obs, f_obs, offset, margin, out_path_,
                               path_name_, end_effect_)             (:287-323)
      reads <out_path_>/<path_name_>.urdf, builds the chain to end_effect_ (pntf.kin, in
      place of pytorch_kinematics), returns (points (n, 2·dim) f32, speed (n, 2) f64).
The chain is a pntf.kin.SerialChain; link meshes are read from
<out_path_>/meshes/collision/<link>.obj (vertices only, in place of igl).

Out of scope: `arm_obstacle_obb` as a function of its own, mesh loading /
rescaling (igl, open3d) and the `sample_speed` driver that writes the .npy files (the on-disk
format is read by models/data_multi.py and models/data_mlp.py).
"""
import math
import os

import numpy as np
import torch

from pntf import kin, ops


def point_obstacle_distance(query_points, triangles_obs):
    """Unsigned distance (N,) from query_points (N, 3) to triangles_obs (1, M, 3, 3)
    (:325-336); the reference squeezes the result, so N = 1 gives a 0-d tensor."""
    return ops.point_mesh_distance(query_points, triangles_obs).squeeze()


def point_append_list(X_list, Y_list, triangles_obs, numsamples, dim, offset, margin):
    """Rejection-sample (x0, x1) pairs near obstacles (:338-391)."""
    device = triangles_obs.device
    OutsideSize = numsamples + 2
    WholeSize = 0
    while OutsideSize > 0:
        P = torch.rand((8 * numsamples, dim), dtype=torch.float32, device=device) - 0.5
        dP = torch.rand((8 * numsamples, dim), dtype=torch.float32, device=device) - 0.5
        rL = torch.rand((8 * numsamples, 1), dtype=torch.float32, device=device) * np.sqrt(dim)
        nP = P + torch.nn.functional.normalize(dP, dim=1) * rL
        inside = torch.all(nP <= 0.5, dim=1) & torch.all(nP >= -0.5, dim=1)
        x0 = P[inside, :]
        x1 = nP[inside, :]
        if x0.shape[0] <= 1:
            continue
        d0 = ops.point_mesh_distance(x0, triangles_obs)
        where_d = (d0 > offset) & (d0 < margin)
        x0 = x0[where_d]
        x1 = x1[where_d]
        y0 = d0[where_d]
        y1 = ops.point_mesh_distance(x1, triangles_obs)
        x = torch.cat((x0, x1), 1)
        y = torch.cat((y0.unsqueeze(1), y1.unsqueeze(1)), 1)
        X_list.append(x)
        Y_list.append(y)
        OutsideSize = OutsideSize - x.shape[0]
        WholeSize = WholeSize + x.shape[0]
        if WholeSize > numsamples:
            break
    return X_list, Y_list


def point_rand_sample_bound_points(numsamples, dim, v_obs, f_obs, offset, margin,
                                   device="cuda"):
    """(sampled_points (numsamples, 2·dim) f32, speed (numsamples, 2) f64) (:393-421)."""
    numsamples = int(numsamples)
    v_obs = torch.tensor(np.asarray(v_obs), dtype=torch.float32, device=device)
    f_obs = torch.tensor(np.asarray(f_obs), dtype=torch.long, device=device)
    t_obs = v_obs[f_obs].unsqueeze(dim=0)
    X_list, Y_list = point_append_list([], [], t_obs, numsamples, dim, offset, margin)
    X = torch.cat(X_list, 0)[:numsamples]
    Y = torch.cat(Y_list, 0)[:numsamples]
    sampled_points = X.detach().cpu().numpy()
    distance = Y.detach().cpu().numpy()
    speed = np.zeros((distance.shape[0], 2))
    speed[:, 0] = np.clip(distance[:, 0], a_min=offset, a_max=margin) / margin
    speed[:, 1] = np.clip(distance[:, 1], a_min=offset, a_max=margin) / margin
    return sampled_points, speed


# ------------------------------------------------------------------ arm generator

_obj_cache = {}


def _obj_vertices(path):
    """The `v x y z` lines of a Wavefront .obj as a (v, 3) float32 array, cached per path
    (the reference reads the file with igl for every batch, :174, and uses the vertices only)."""
    if path not in _obj_cache:
        rows = []
        with open(path) as fh:
            for line in fh:
                p = line.split()
                if len(p) >= 4 and p[0] == "v":
                    rows.append([float(p[1]), float(p[2]), float(p[3])])
        _obj_cache[path] = np.asarray(rows, dtype=np.float32).reshape(-1, 3)
    return _obj_cache[path]


def _arm_link_vertices(chain, out_path_, device):
    """Collision vertices of every frame of index > 1 (`if iter>1`, :172), on the device."""
    return [None if f <= 1 else torch.from_numpy(_obj_vertices(
        os.path.join(out_path_, "meshes", "collision", name + ".obj"))).to(device)
        for f, name in enumerate(chain.link_names)]


def arm_obstacle_distance(th_batch, chain, out_path_, triangles_obs, cap=None):
    """Per configuration of th_batch (n, dof), the minimum distance (n,) from the collision
    vertices of the posed arm to triangles_obs (1, M, 3, 3) (:153-218).  One fused kernel
    (FK, distance, minimum): the posed cloud is never stored, so the reference's batches of
    50 000 configurations are not needed.  `cap` (not in the reference) bounds the result."""
    verts = _arm_link_vertices(chain, out_path_, th_batch.device)
    return ops.arm_mesh_distance(th_batch, chain, verts, triangles_obs, cap=cap)


def arm_append_list(X_list, Y_list, chain, out_path_, triangles_obs, numsamples, dim, offset,
                    margin, cap=None):
    """Rejection-sample (x0, x1) configuration pairs near obstacles (:220-285).

    The reference first drops configurations by `arm_obstacle_obb` (:77-151, :249-251), a
    separating-axis test of hard-coded link boxes of one dataset against one hard-coded
    obstacle box, which moreover returns only the last link's test.  Done correctly it is a
    conservative prefilter for d0 <= margin, so leaving it out changes no accepted sample;
    it is not restated, and the kernel's exact culling (and `cap`) does that job."""
    device = triangles_obs.device
    OutsideSize = numsamples + 2
    WholeSize = 0
    scale = math.pi / 0.5
    while OutsideSize > 0:
        P = torch.rand((5 * numsamples, dim), dtype=torch.float32, device=device) - 0.5
        dP = torch.rand((5 * numsamples, dim), dtype=torch.float32, device=device) - 0.5
        rL = torch.rand((5 * numsamples, 1), dtype=torch.float32, device=device) * np.sqrt(3)
        nP = P + torch.nn.functional.normalize(dP, dim=1) * rL
        inside = torch.all(nP <= 0.5, dim=1) & torch.all(nP >= -0.5, dim=1)
        x0 = P[inside, :]
        x1 = nP[inside, :]
        if x0.shape[0] <= 1:
            continue
        d0 = arm_obstacle_distance(scale * x0, chain, out_path_, triangles_obs, cap=cap)
        where_d = (d0 >= offset) & (d0 <= margin)
        x0 = x0[where_d]
        x1 = x1[where_d]
        y0 = d0[where_d]
        y1 = arm_obstacle_distance(scale * x1, chain, out_path_, triangles_obs, cap=cap)
        x = torch.cat((x0, x1), 1)
        y = torch.cat((y0.unsqueeze(1), y1.unsqueeze(1)), 1)
        X_list.append(x)
        Y_list.append(y)
        OutsideSize = OutsideSize - x.shape[0]
        WholeSize = WholeSize + x.shape[0]
        if WholeSize > numsamples:
            break
    return X_list, Y_list


def arm_rand_sample_bound_points(numsamples, dim, v_obs, f_obs, offset, margin, out_path_,
                                 path_name_, end_effect_, device="cuda"):
    """(sampled_points (numsamples, 2·dim) f32, speed (numsamples, 2) f64) for the arm
    <out_path_>/<path_name_>.urdf up to the link end_effect_ (:287-323).  Only speeds clipped
    to [offset, margin] leave this function, so the kernel runs with cap = 2·margin."""
    numsamples = int(numsamples)
    with open(os.path.join(out_path_, path_name_ + ".urdf")) as fh:
        chain = kin.SerialChain.from_urdf(fh.read(), end_effect_)
    v_obs = torch.tensor(np.asarray(v_obs), dtype=torch.float32, device=device)
    f_obs = torch.tensor(np.asarray(f_obs), dtype=torch.long, device=device)
    t_obs = v_obs[f_obs].unsqueeze(dim=0)
    X_list, Y_list = arm_append_list([], [], chain, out_path_, t_obs, numsamples, dim, offset,
                                     margin, cap=2 * margin)
    X = torch.cat(X_list, 0)[:numsamples]
    Y = torch.cat(Y_list, 0)[:numsamples]
    sampled_points = X.detach().cpu().numpy()
    distance = Y.detach().cpu().numpy()
    speed = np.zeros((distance.shape[0], 2))
    speed[:, 0] = np.clip(distance[:, 0], a_min=offset, a_max=margin) / margin
    speed[:, 1] = np.clip(distance[:, 1], a_min=offset, a_max=margin) / margin
    return sampled_points, speed
