"""fp64 oracle and scenes for the arm sampler tests — TEST INFRASTRUCTURE ONLY.

Forward kinematics in a formulation independent of pntf.kin and of the kernel (which compose
3x4 matrices from the root): a chain is a list of joints (xyz, rpy, type, axis), a POINT of
frame f is carried from the tip frame back to the root, joint by joint — Rodrigues' rotation
formula (or the slide) on the point, then the joint origin as three elementary rotations of
the point (about x by roll, then y by pitch, then z by yaw: URDF's fixed-axis rpy) and the
shift.  No matrix is ever formed.  Pinned by closed forms in tests/test_arm_sampler.py.
Distances come from oracle.mesh_oracle.
"""
import numpy as np

from oracle import mesh_oracle as M

FIXED, REVOLUTE, PRISMATIC = "fixed", "revolute", "prismatic"
ROOT = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), FIXED, (1.0, 0.0, 0.0))   # frame 0 of every chain


def _rot_axis(p, k, ang):
    """Rotate points p (..., 3) about coordinate axis k by ang (broadcasting), on the point."""
    i, j = (k + 1) % 3, (k + 2) % 3
    c, s = np.cos(ang), np.sin(ang)
    out = np.empty(np.broadcast(p[..., 0], c).shape + (3,))
    out[..., k] = p[..., k]
    out[..., i] = c * p[..., i] - s * p[..., j]
    out[..., j] = s * p[..., i] + c * p[..., j]
    return out


def columns(spec):
    """Column of theta each joint reads (None for fixed joints): moving joints in order."""
    cols, k = [], 0
    for _, _, kind, _ in spec:
        cols.append(None if kind == FIXED else k)
        k += kind != FIXED
    return cols


def pose_points(spec, theta, f, v):
    """World positions (n, m, 3) of points v (m, 3) given in frame f, for theta (n, dof)."""
    theta = np.asarray(theta, np.float64)
    p = np.broadcast_to(np.asarray(v, np.float64)[None], (theta.shape[0], len(v), 3)).copy()
    cols = columns(spec)
    for g in range(f, -1, -1):
        xyz, rpy, kind, axis = spec[g]
        a = np.asarray(axis, np.float64)
        a = a / np.linalg.norm(a)
        if kind == REVOLUTE:
            q = theta[:, cols[g]][:, None, None]
            p = p * np.cos(q) + np.cross(a, p) * np.sin(q) + a * (p @ a)[..., None] * (1 - np.cos(q))
        elif kind == PRISMATIC:
            p = p + theta[:, cols[g]][:, None, None] * a
        for k in range(3):                       # roll about x, pitch about y, yaw about z
            p = _rot_axis(p, k, rpy[k])
        p = p + np.asarray(xyz, np.float64)
    return p


def frame_matrices(spec, theta):
    """(n, F, 3, 4) poses, read off the posed origin and unit points of each frame."""
    probe = np.concatenate([np.zeros((1, 3)), np.eye(3)])
    out = np.empty((len(theta), len(spec), 3, 4))
    for f in range(len(spec)):
        w = pose_points(spec, theta, f, probe)
        out[:, f, :, 3] = w[:, 0]
        out[:, f, :, :3] = np.swapaxes(w[:, 1:] - w[:, :1], 1, 2)
    return out


def posed_cloud(spec, theta, link_verts):
    """(n, V, 3): every frame's vertices posed, frames in order."""
    return np.concatenate([pose_points(spec, theta, f, v) for f, v in enumerate(link_verts)
                           if len(v)], axis=1)


def arm_mesh_distance(spec, theta, link_verts, tris):
    """Minimum over the posed vertices of the distance to the mesh, (n,) float64."""
    cloud = posed_cloud(spec, theta, link_verts)
    n, V, _ = cloud.shape
    return M.point_mesh_distance(cloud.reshape(-1, 3), tris).reshape(n, V).min(axis=1)


def origin_matrices(spec):
    """(F, 3, 4) joint origins as the explicit product Rz(yaw)·Ry(pitch)·Rx(roll) | xyz."""
    out = []
    for xyz, (r, p, y), _, _ in spec:
        Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]])
        Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
        Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
        out.append(np.concatenate([Rz @ Ry @ Rx, np.asarray(xyz, float)[:, None]], axis=1))
    return np.stack(out)


# ------------------------------------------------------------------ scenes
# Every scene keeps posed vertices and triangles inside [-0.5, 0.5]^3: the translation lengths
# along a chain (prismatic travel included) sum to <= 0.4 and link vertices lie within 0.05 of
# their frame — the coordinate range the project's distance tolerance was set for.

def link_blob(rng, v):
    """v vertices within 0.05 of the frame origin (a cube of half-width 0.028)."""
    return rng.uniform(-0.028, 0.028, (v, 3))


def boxed_mesh(rng, t, scale=0.2):
    """tests/test_mesh.py's random_mesh, shrunk into the box."""
    c = rng.uniform(-0.4, 0.4, (t, 1, 3))
    tris = c + rng.normal(0, scale, (t, 3, 3)) * rng.uniform(0.05, 1.0, (t, 1, 1))
    return tris * min(1.0, 0.5 / np.abs(tris).max())


def random_chain(rng, joints, reach=0.4):
    """Root + `joints` revolute joints with random axes, rpy and offsets summing to `reach`."""
    spec = [ROOT]
    for _ in range(joints):
        d = rng.normal(size=3)
        spec.append((tuple(d / np.linalg.norm(d) * reach / joints),
                     tuple(rng.uniform(-np.pi, np.pi, 3)), REVOLUTE, tuple(rng.normal(size=3))))
    return spec


PRISMATIC_TRAVEL = 0.05


def random_theta(rng, spec, n):
    """theta ~ U[-pi, pi] for rotations; a prismatic joint's value is a length, drawn from
    U[-PRISMATIC_TRAVEL, PRISMATIC_TRAVEL] so that the scene stays inside the box."""
    th = rng.uniform(-np.pi, np.pi, (n, sum(c is not None for c in columns(spec))))
    for (_, _, kind, _), c in zip(spec, columns(spec)):
        if kind == PRISMATIC:
            th[:, c] *= PRISMATIC_TRAVEL / np.pi
    return th


# The 7-link test arm: revolute, continuous, prismatic and fixed joints, non-zero rpy, a
# non-unit axis, a joint without an <axis> (default 1 0 0), and a side branch (l2 -> camera)
# that is not on the way to `tool`.  Offsets 0.05 + 0.05 + 0.08 + 0.07 + 0.06 + 0.04 = 0.35,
# plus 0.05 of prismatic travel.
URDF7_SPEC = [
    ROOT,
    ((0.0, 0.0, 0.05), (0.0, 0.0, 0.0), REVOLUTE, (0.0, 0.0, 1.0)),
    ((0.0, 0.03, 0.04), (0.3, 0.0, 0.0), REVOLUTE, (0.0, 2.0, 0.0)),
    ((0.08, 0.0, 0.0), (0.0, 0.5, 0.0), FIXED, (1.0, 0.0, 0.0)),
    ((0.07, 0.0, 0.0), (0.0, 0.0, -0.4), PRISMATIC, (1.0, 0.0, 1.0)),
    ((0.0, 0.0, 0.06), (0.1, -0.2, 0.3), REVOLUTE, (1.0, 0.0, 0.0)),
    ((0.04, 0.0, 0.0), (0.0, 0.0, 0.0), FIXED, (1.0, 0.0, 0.0)),
]
URDF7_LINKS = ["base", "l1", "l2", "l3", "l4", "l5", "tool"]
URDF7 = """<?xml version="1.0"?>
<robot name="arm7">
  <link name="base"/> <link name="l1"/> <link name="l2"/> <link name="camera"/>
  <link name="l3"/> <link name="l4"/> <link name="l5"/> <link name="tool"/>
  <joint name="j1" type="revolute">
    <parent link="base"/> <child link="l1"/>
    <origin xyz="0 0 0.05" rpy="0 0 0"/> <axis xyz="0 0 1"/>
    <limit lower="-3.14" upper="3.14" effort="1" velocity="1"/>
  </joint>
  <joint name="j_cam" type="revolute">
    <parent link="l2"/> <child link="camera"/>
    <origin xyz="0.2 0.2 0.2" rpy="1 1 1"/> <axis xyz="0 1 0"/>
  </joint>
  <joint name="j3" type="fixed">
    <parent link="l2"/> <child link="l3"/> <origin xyz="0.08 0 0" rpy="0 0.5 0"/>
  </joint>
  <joint name="j2" type="continuous">
    <parent link="l1"/> <child link="l2"/>
    <origin xyz="0 0.03 0.04" rpy="0.3 0 0"/> <axis xyz="0 2 0"/>
  </joint>
  <joint name="j4" type="prismatic">
    <parent link="l3"/> <child link="l4"/>
    <origin xyz="0.07 0 0" rpy="0 0 -0.4"/> <axis xyz="1 0 1"/>
  </joint>
  <joint name="j5" type="revolute">
    <parent link="l4"/> <child link="l5"/> <origin xyz="0 0 0.06" rpy="0.1 -0.2 0.3"/>
  </joint>
  <joint name="j6" type="fixed">
    <parent link="l5"/> <child link="tool"/> <origin xyz="0.04 0 0"/>
  </joint>
</robot>
"""


def revolute_arm_urdf(joints, reach=0.4):
    """URDF text, spec and link names of base -(fixed)- mount -(R)- link1 ... -(R)- link<joints>:
    joint k sits reach/joints along x from the one before it (the first on the mount) and
    turns about z, y, x, z, ... in turn, so the last link's frame is reach·(joints-1)/joints
    from the base and its vertices within `reach` of it."""
    step = reach / joints
    axes = [(0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)]
    names = ["base", "mount"] + ["link%d" % (k + 1) for k in range(joints)]
    spec = [ROOT, ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), FIXED, (1.0, 0.0, 0.0))]
    xml = ['<robot name="arm">'] + ['<link name="%s"/>' % n for n in names]
    xml.append('<joint name="j0" type="fixed"><parent link="base"/><child link="mount"/>'
               '</joint>')
    for k in range(joints):
        xyz = (0.0 if k == 0 else step, 0.0, 0.0)
        rpy = (0.0, 0.0, 0.0) if k == 0 else (0.2, -0.3, 0.1 * k)
        spec.append((xyz, rpy, REVOLUTE, axes[k % 3]))
        xml.append('<joint name="j%d" type="revolute"><parent link="%s"/><child link="%s"/>'
                   '<origin xyz="%r %r %r" rpy="%r %r %r"/><axis xyz="%r %r %r"/></joint>'
                   % ((k + 1, names[k + 1], names[k + 2]) + xyz + rpy + axes[k % 3]))
    xml.append("</robot>")
    return "\n".join(xml), spec, names


def write_arm(path, joints, rng, verts_per_link=20):
    """Write <path>/arm.urdf and <path>/meshes/collision/link<k>.obj (vertices only); returns
    (spec, link vertex list aligned with the frames — only frames of index > 1 own vertices,
    as in the reference's arm_obstacle_distance)."""
    import os
    text, spec, names = revolute_arm_urdf(joints)
    os.makedirs(os.path.join(path, "meshes", "collision"), exist_ok=True)
    with open(os.path.join(path, "arm.urdf"), "w") as fh:
        fh.write(text)
    link_verts = []
    for f, name in enumerate(names):
        if f <= 1:
            link_verts.append(np.zeros((0, 3)))
            continue
        v = link_blob(rng, verts_per_link).astype(np.float32)
        with open(os.path.join(path, "meshes", "collision", name + ".obj"), "w") as fh:
            fh.write("# collision vertices of %s\n" % name)
            for x, y, z in v:
                fh.write("v %.9g %.9g %.9g\n" % (x, y, z))
            fh.write("f 1 2 3\n")
        link_verts.append(v.astype(np.float64))
    return spec, link_verts
