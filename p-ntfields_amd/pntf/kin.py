"""Serial kinematic chains for the arm sampler (ops.arm_mesh_distance, pntf_arm.hip).

`SerialChain` is what the reference gets from pytorch_kinematics'
`build_serial_chain_from_urdf(text, end_link)` (dataprocessing/speed_sampling_gpu.py:295-297)
as far as the sampler uses it: the frames that `forward_kinematics(th, end_only=False)`
enumerates — the root link first (an identity fixed joint), then the child link of every
joint on the way to `end_link` — posed by the URDF convention

    M_f = M_{f-1} · O_f · J_f(theta),

O_f the joint's `origin` (xyz, rpy with R = Rz(yaw)·Ry(pitch)·Rx(roll)), J_f the rotation by
theta about the joint's axis (revolute / continuous), the translation by theta along it
(prismatic) or the identity (fixed).  Fixed joints read no joint value; the k-th moving joint
from the root reads column k of theta.  Parsing needs xml.etree only.
"""
import xml.etree.ElementTree as ET

import numpy as np
import torch

from ._lib import PntfError

FIXED, REVOLUTE, PRISMATIC = 0, 1, 2          # include/pntf.h PNTF_JOINT_*
_TYPES = {"fixed": FIXED, "revolute": REVOLUTE, "continuous": REVOLUTE, "prismatic": PRISMATIC}


def rpy_matrix(rpy):
    """URDF fixed-axis roll / pitch / yaw -> R = Rz(yaw)·Ry(pitch)·Rx(roll), float64 (3, 3)."""
    r, p, y = (float(v) for v in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def _floats(text, what):
    try:
        v = [float(s) for s in text.split()]
    except ValueError:
        v = []
    if len(v) != 3:
        raise PntfError("URDF: %s needs three numbers, got %r" % (what, text))
    return v


class SerialChain:
    """Frames of a serial chain, root first.

    Packed host tables (what pntf_arm_mesh_distance takes): `origins` (F, 3, 4) float32,
    `types` (F,) int32 (FIXED / REVOLUTE / PRISMATIC), `axes` (F, 3) float32 unit vectors,
    `cols` (F,) int32 — the column of theta a moving joint reads (0 for fixed joints, which
    read none).  `tables(device)` gives the same four as tensors on a device."""

    def __init__(self, origins, types, axes, link_names):
        self.origins = np.ascontiguousarray(origins, dtype=np.float32)
        self.types = np.ascontiguousarray(types, dtype=np.int32)
        self.axes = np.ascontiguousarray(axes, dtype=np.float32)
        moving = self.types != FIXED
        self.cols = np.where(moving, np.cumsum(moving) - 1, 0).astype(np.int32)
        self.dof = int(moving.sum())
        self.link_names = list(link_names)
        self._dev = {}

    @classmethod
    def from_arrays(cls, origins, types, axes, link_names=None):
        """origins (F, 3, 4) or (F, 4, 4); types (F,) of FIXED / REVOLUTE / PRISMATIC or their
        URDF names; axes (F, 3), normalised here (a fixed joint's axis is not used)."""
        origins = np.asarray(origins, dtype=np.float64)
        if origins.ndim != 3 or origins.shape[1] not in (3, 4) or origins.shape[2] != 4:
            raise PntfError("origins must be (F, 3, 4) or (F, 4, 4), got %s" % (origins.shape,))
        F = origins.shape[0]
        try:
            types = [_TYPES[t] if isinstance(t, str) else int(t) for t in types]
        except KeyError as e:
            raise PntfError("unsupported joint type %s" % e)
        if any(t not in (FIXED, REVOLUTE, PRISMATIC) for t in types):
            raise PntfError("joint types must be FIXED, REVOLUTE or PRISMATIC")
        axes = np.asarray(axes, dtype=np.float64).reshape(-1, 3)
        if F < 1 or len(types) != F or axes.shape[0] != F:
            raise PntfError("origins, types and axes must describe the same F >= 1 frames")
        norm = np.linalg.norm(axes, axis=1)
        if np.any((norm == 0) & (np.asarray(types) != FIXED)):
            raise PntfError("a moving joint needs a non-zero axis")
        axes = axes / np.where(norm > 0, norm, 1.0)[:, None]
        if link_names is None:
            link_names = ["frame%d" % f for f in range(F)]
        if len(link_names) != F:
            raise PntfError("link_names must name every frame")
        return cls(origins[:, :3, :], types, axes, link_names)

    @classmethod
    def from_urdf(cls, text, end_link):
        """The chain from the URDF's root link to `end_link` (frame 0 = the root link)."""
        try:
            robot = ET.fromstring(text)
        except ET.ParseError as e:
            raise PntfError("URDF: %s" % e)
        links = [l.get("name") for l in robot.findall("link")]
        up = {}                                   # child link -> its joint
        for j in robot.findall("joint"):
            parent, child = j.find("parent"), j.find("child")
            if parent is None or child is None:
                raise PntfError("URDF: joint %r lacks a parent or child" % j.get("name"))
            up[child.get("link")] = (j, parent.get("link"))
        roots = [l for l in links if l not in up]
        if not roots:
            raise PntfError("URDF: no root link (every link is some joint's child)")
        if end_link not in links:
            raise PntfError("URDF: no link %r" % (end_link,))
        path, link = [], end_link
        while link in up:
            j, parent = up[link]
            path.append((j, link))
            link = parent
            if len(path) > len(up) or link not in links:
                raise PntfError("URDF: %r is not reachable from the root link" % (end_link,))
        if link != roots[0]:
            raise PntfError("URDF: %r is not reachable from the root link %r"
                            % (end_link, roots[0]))
        origins, types, axes, names = [np.eye(4)[:3]], [FIXED], [[1.0, 0.0, 0.0]], [roots[0]]
        for j, child in reversed(path):
            kind = j.get("type")
            if kind not in _TYPES:
                raise PntfError("URDF: joint %r of type %r is not supported (fixed, revolute, "
                                "continuous, prismatic)" % (j.get("name"), kind))
            o = j.find("origin")
            xyz = _floats(o.get("xyz", "0 0 0"), "origin xyz") if o is not None else [0, 0, 0]
            rpy = _floats(o.get("rpy", "0 0 0"), "origin rpy") if o is not None else [0, 0, 0]
            a = j.find("axis")
            origins.append(np.concatenate([rpy_matrix(rpy), np.array(xyz)[:, None]], axis=1))
            types.append(_TYPES[kind])
            axes.append(_floats(a.get("xyz", "1 0 0"), "axis xyz") if a is not None
                        else [1.0, 0.0, 0.0])
            names.append(child)
        return cls.from_arrays(np.stack(origins), types, axes, names)

    def tables(self, device):
        """(origins, types, axes, cols) as tensors on `device` (cached per device)."""
        device = torch.device(device)
        if device not in self._dev:
            self._dev[device] = tuple(torch.from_numpy(a).to(device)
                                      for a in (self.origins, self.types, self.axes, self.cols))
        return self._dev[device]

    def forward_kinematics(self, theta):
        """Pose of every frame, (n, F, 3, 4) float32 on theta's device, for theta (n, dof):
        plain torch, for users and tests — the sampler's kernel composes the same products
        itself."""
        if theta.dim() != 2 or theta.shape[1] != self.dof:
            raise PntfError("theta must be (n, %d), got %s" % (self.dof, tuple(theta.shape)))
        theta = theta.detach().to(torch.float32)
        n, dev = theta.shape[0], theta.device
        origins, _, axes, _ = self.tables(dev)
        bottom = torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=dev)
        eye = torch.eye(4, device=dev)
        M = eye.expand(n, 4, 4)
        out = []
        for f in range(len(self.types)):
            J = eye.expand(n, 4, 4).clone()
            if self.types[f] != FIXED:
                q = theta[:, int(self.cols[f])]
                a = axes[f]
                if self.types[f] == REVOLUTE:
                    K = torch.zeros(3, 3, device=dev)
                    K[0, 1], K[0, 2], K[1, 0] = -a[2], a[1], a[2]
                    K[1, 2], K[2, 0], K[2, 1] = -a[0], -a[1], a[0]
                    s, c = torch.sin(q)[:, None, None], torch.cos(q)[:, None, None]
                    J[:, :3, :3] = c * eye[:3, :3] + s * K + (1 - c) * torch.outer(a, a)
                else:
                    J[:, :3, 3] = q[:, None] * a
            M = M @ (torch.cat([origins[f], bottom]) @ J)
            out.append(M[:, :3, :])
        return torch.stack(out, dim=1)
