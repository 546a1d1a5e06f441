"""pntf — MI355X-native hot path of P-NTFields (τ / ∇τ fields, path velocity, planner).

Host runtime for libpntf.so (HIP, gfx950).  `pntf.ops` holds the torch-facing entry
points, `pntf.net` the pieces shared by the drop-in `models` modules, `pntf.synth` the
seeded synthetic inputs, `pntf.dist` the multi-GPU sharding, `pntf.kin` the serial chains
(URDF) of the arm sampler, `pntf.evaluate` the report on planned paths (convergence, length,
clearance from the obstacle mesh, success rate) and on the field itself (travel time against
a grid Eikonal solve of the mesh's speed field).
"""
__version__ = "0.1.0"
