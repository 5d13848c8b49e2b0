"""MI355X-native hot path of the stereo-depth + point-cloud fusion pipeline.

The directory name starts with a digit (it mirrors the upstream project name), so import it with
    import importlib; r3d = importlib.import_module("3d_reconstruction_project_amd")
or through the `r3d` alias module at the repository root (`import r3d`).
"""
from . import (_lib, cloud_ops, distributed, io_formats, mesh_ops, pipeline, normal_estimation, orientation, pointcloud, pointcloud_alignment,  # noqa: F401
               pointcloud_processing, poisson, posegraph, stereo_prepost, stereo_sgbm, synth, tsdf)
from ._lib import Context, R3DError, default_context  # noqa: F401
from .cloud_ops import (compute_fpfh_feature, compute_rgbd_odometry, correspondences_from_features, registration_fgr_based_on_correspondence,  # noqa: F401
                        registration_fgr_based_on_feature_matching, registration_ransac_based_on_correspondence,
                        registration_ransac_based_on_feature_matching)
from .stereo_sgbm import (STEREO_SGBM_MODE_HH, STEREO_SGBM_MODE_SGBM_3WAY, StereoSGBM, StereoSGBM_create, createRightMatcher, depth,  # noqa: F401
                          filterSpeckles, reference_matcher)
from .normal_estimation import NormalEstimation, estimate  # noqa: F401,E402
from .pointcloud import PointCloud, TriangleMesh  # noqa: F401,E402
from .pointcloud_alignment import GeneralizedICPAlignment, PointCloudAlignment, align, multi_scale_icp  # noqa: F401,E402
from .pointcloud_processing import PointCloudProcessingWithCUDA  # noqa: F401,E402
from .tsdf import ScalableTSDFVolume, TSDFVolumeColorType  # noqa: F401,E402
from .mesh_ops import FilterScope  # noqa: F401,E402
from .poisson import create_from_point_cloud_poisson  # noqa: F401,E402
from .mesh_reconstruction import MeshReconstruction  # noqa: F401,E402
from .posegraph import (GlobalOptimizationConvergenceCriteria, GlobalOptimizationLevenbergMarquardt, GlobalOptimizationOption, PoseGraph,  # noqa: F401,E402
                        PoseGraphEdge, PoseGraphNode, global_optimization)
from .io_formats import read_pose_graph, write_pose_graph  # noqa: F401,E402
from .stereo_prepost import (COLOR_BGR2GRAY, CV_16SC2, INTER_LINEAR, NORM_MINMAX, DisparityWLSFilter, createDisparityWLSFilter,  # noqa: F401,E402
                             cvtColor, initUndistortRectifyMap, normalize, remap)
