"""Drop-in for the last stage of the reference's main.py:83, mesh_reconstruction.py:22-37 (MeshReconstruction.reconstruct_mesh):
create_from_point_cloud_poisson(depth=6), then Laplacian smoothing x5 and the clean-ups; visualizer.py:107-110 runs the same step
once per frame.  ASSUMED (the reference source is not in this repository): the class takes no constructor argument but an optional
device, reconstruct_mesh takes the fused cloud (with normals, optionally colours) and returns the mesh; depth 6 and 5 smoothing
iterations are the reference's values as SURVEY.md section 2 records them.  Everything runs on the device
(pipeline.reconstruct_mesh)."""
from . import _lib, pipeline


class MeshReconstruction:
    def __init__(self, device="CUDA:0", depth=6, smooth_iterations=5):
        self.device = _lib.parse_device(device)
        self.depth = depth
        self.smooth_iterations = smooth_iterations

    def reconstruct_mesh(self, pcd):
        """-> TriangleMesh with vertex normals (and vertex colours when the cloud has colours)"""
        return pipeline.reconstruct_mesh(pcd, self.depth, self.smooth_iterations, ctx=_lib.default_context(self.device))
