"""MI355X-native U-Net lane-segmentation path (HIP kernels behind a C ABI).

Public surface:
  UNetHIP                      forward(image) -> logits, run_u8(frames)
  RKNN_model_container         drop-in for the reference's model container
  SegMetrics                   loss / Dice / IoU / precision / recall of a validation pass (metrics.py)
  ThresholdSweep               confusion counts and metrics at many thresholds from one pass (metrics.py)
  Ensemble                     the reference's ensemble_predict: several models' probabilities averaged on the device
                               (ensemble.py)
  LossSpec                     the general BCE + focal + Dice loss as UNetTrainer.set_loss keeps it (metrics.py)
  positive_counts, pos_weight_from_masks, sample_weights
                               mask statistics for sparse lanes (imbalance.py)
  FramePipeline, predict_video, jet_table
                               the reference's video mode: batched resize, mask overlay, streamed chunks (video.py)
  FitConfig, LaneFits, LaneTracker
                               the bird's-eye lane fit on the device: sliding windows, quadratic fit, curvature
                               (lanefit.py; follow.py and diagnose.py are imported as submodules the same way)
  CleanConfig, Components, LaneInstance
                               lane instances on the device: connected components, statistics, clean-up
                               (instances.py: label, clean, lane_instances)
  ViewConfig, lane_view, curve_table
                               the lane view on the device: lane area, markings and curves drawn in the camera frame
                               (laneview.py)
  seeded_state_dict, ...       reproducible weights / synthetic inputs
"""
from .state import (DEFAULT_FEATURES, INPUT_MEAN, INPUT_STD, num_parameters, seeded_state_dict,  # noqa: F401
                    state_dict_spec, synthetic_frames, synthetic_targets)


def __getattr__(name):  # lazy: importing the package must not need torch.cuda or the .so
    if name == "UNetHIP":
        from .model import UNetHIP
        return UNetHIP
    if name == "RKNN_model_container":
        from .py_utils.rknn_executor import RKNN_model_container
        return RKNN_model_container
    if name == "SegMetrics":
        from .metrics import SegMetrics
        return SegMetrics
    if name == "LossSpec":
        from .metrics import LossSpec
        return LossSpec
    if name in ("positive_counts", "pos_weight_from_masks", "sample_weights"):
        from . import imbalance
        return getattr(imbalance, name)
    if name in ("FramePipeline", "predict_video", "jet_table"):
        from . import video
        return getattr(video, name)
    if name in ("ThresholdSweep", "DEFAULT_THRESHOLDS"):
        from . import metrics
        return getattr(metrics, name)
    if name in ("FitConfig", "LaneFits", "LaneTracker"):
        from . import lanefit
        return getattr(lanefit, name)
    if name in ("CleanConfig", "Components", "LaneInstance"):
        from . import instances
        return getattr(instances, name)
    if name in ("ViewConfig", "lane_view", "curve_table"):
        from . import laneview
        return getattr(laneview, name)
    if name == "Ensemble":
        from .ensemble import Ensemble
        return Ensemble
    raise AttributeError(name)
