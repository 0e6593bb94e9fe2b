"""ai-camera_amd -- MI355X-native detect+track hot path behind the AI-Camera plugin API.

The directory name carries a hyphen (it mirrors the upstream repo name), so it is
imported with ``importlib.import_module("ai-camera_amd")``; ``src/`` at the repo root
re-exports the reference's module layout (``src.aicamera_tracker``,
``src.detector.yolo_detector`` ...) on top of it for drop-in use.

Submodules are imported lazily: importing the package never touches the GPU; the
first call that needs ``libaicam.so`` loads it and raises if it is missing.
"""
import importlib as _importlib

__version__ = "0.1.0"
PKG = __name__

_LAZY = ("config", "synthetic", "engine_file", "_lib", "hip_engine", "image_processing",
         "detector", "reid_model", "deepsort_tracker", "bytetrack", "ocsort", "botsort", "deepsort_bank", "xcam", "archive", "zones", "bestshot", "scene", "leftobj", "colours", "heatmap", "proximity", "render", "jpeg", "jpegdec", "gmc", "frames", "core", "pipeline", "distributed", "cli")


def __getattr__(name):
    if name in _LAZY:
        return _importlib.import_module(f"{__name__}.{name}")
    if name == "BYTETracker":
        return _importlib.import_module(f"{__name__}.bytetrack").BYTETracker
    if name == "OCSort":
        return _importlib.import_module(f"{__name__}.ocsort").OCSort
    if name == "BYTETrackerBank":
        return _importlib.import_module(f"{__name__}.bytetrack").BYTETrackerBank
    if name == "OCSortBank":
        return _importlib.import_module(f"{__name__}.ocsort").OCSortBank
    if name == "BoTSORT":
        return _importlib.import_module(f"{__name__}.botsort").BoTSORT
    if name == "BoTSORTBank":
        return _importlib.import_module(f"{__name__}.botsort").BoTSORTBank
    if name == "DeepSORTBank":
        return _importlib.import_module(f"{__name__}.deepsort_bank").DeepSORTBank
    if name == "CrossCamera":
        return _importlib.import_module(f"{__name__}.xcam").CrossCamera
    if name == "IdentityArchive":
        return _importlib.import_module(f"{__name__}.archive").IdentityArchive
    if name == "ZoneCounter":
        return _importlib.import_module(f"{__name__}.zones").ZoneCounter
    if name == "BestShots":
        return _importlib.import_module(f"{__name__}.bestshot").BestShots
    if name == "SceneWatch":
        return _importlib.import_module(f"{__name__}.scene").SceneWatch
    if name == "LeftObjects":
        return _importlib.import_module(f"{__name__}.leftobj").LeftObjects
    if name == "TrackColours":
        return _importlib.import_module(f"{__name__}.colours").TrackColours
    if name == "HeatMaps":
        return _importlib.import_module(f"{__name__}.heatmap").HeatMaps
    if name == "Proximity":
        return _importlib.import_module(f"{__name__}.proximity").Proximity
    if name == "Renderer":
        return _importlib.import_module(f"{__name__}.render").Renderer
    if name == "JpegEncoder":
        return _importlib.import_module(f"{__name__}.jpeg").JpegEncoder
    if name == "JpegDecoder":
        return _importlib.import_module(f"{__name__}.jpegdec").JpegDecoder
    if name == "CameraMotionBank":
        return _importlib.import_module(f"{__name__}.gmc").CameraMotionBank
    if name == "CameraMotion":
        return _importlib.import_module(f"{__name__}.gmc").CameraMotion
    raise AttributeError(name)
