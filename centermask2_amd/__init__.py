"""centermask2_amd — MI355X-native CenterMask2 inference hot path (VoVNetV2-FPN, FCOS, CenterROIHeads)."""
__version__ = "0.1.0"

__all__ = ["Predictor", "load_weights", "GeneralizedRCNNWithTTA", "SlicedInference", "Visualizer", "draw_instance_predictions", "InstanceTracker",
           "VideoVisualizer", "CityscapesInstanceEvaluator", "__version__"]


def __getattr__(name):
    """`from centermask2_amd import Predictor, load_weights` without importing torch for users of the light submodules."""
    if name in ("Predictor", "load_weights"):
        from . import predictor
        return getattr(predictor, name)
    if name == "GeneralizedRCNNWithTTA":
        from .modeling import test_time_augmentation
        return test_time_augmentation.GeneralizedRCNNWithTTA
    if name == "SlicedInference":
        from .modeling import sliced_inference
        return sliced_inference.SlicedInference
    if name in ("Visualizer", "draw_instance_predictions"):
        from . import visualize
        return getattr(visualize, name)
    if name in ("InstanceTracker", "VideoVisualizer"):
        from . import video
        return getattr(video, name)
    if name == "CityscapesInstanceEvaluator":
        from . import evaluation
        return evaluation.CityscapesInstanceEvaluator
    raise AttributeError("module {!r} has no attribute {!r}".format(__name__, name))
