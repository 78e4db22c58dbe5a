"""selfocc_amd — MI355X-native implementation of SelfOcc's data-parallel hot path
(TPV/BEV lifter MSDA + SDF volume-rendering head + reprojection loss) behind the
reference's registry / config surface.  The arithmetic lives in csrc/*.hip behind the C ABI
of include/selfocc_hip.h; there is no CPU fallback."""
__version__ = "0.1.0"

_LAZY = {'DepthMetric': 'depth_metric', 'depth_errors': 'depth_metric', 'MeanIoU': 'occ', 'IoU': 'ssc_metric',
         'SSCMetrics': 'ssc_metric', 'kitti_occ_metrics': 'ssc_metric', 'cityscapes2semantickitti': 'ssc_metric',
         'openseed2nuscenes': 'ssc_metric', 'render_median_depth': 'render', 'median_depth_reference': 'render',
         'upsample_edges': 'render', 'neus_upsample_reference': 'render', 'render_normal_vis': 'render',
         'normal_vis_reference': 'render', 'field_grad': 'occ', 'field_grad_autograd': 'occ'}


def __getattr__(name):
    """``from selfocc_amd import DepthMetric`` (the depth-evaluation metric, depth_metric.py) or ``IoU, MeanIoU,
    SSCMetrics`` (the occupancy metrics, ssc_metric.py / occ.py) or ``render_median_depth, median_depth_reference, upsample_edges,
    neus_upsample_reference, render_normal_vis, normal_vis_reference`` (render.py) or ``field_grad, field_grad_autograd`` (the SDF
    gradient at arbitrary points, occ.py)
    without importing torch at package import."""
    if name in _LAZY:
        import importlib
        return getattr(importlib.import_module(f".{_LAZY[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
