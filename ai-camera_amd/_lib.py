"""ctypes binding of libaicam.so (the C ABI declared in include/aicam.h).

There is no CPU fallback: if the shared library is missing or a call fails, an exception is
raised -- the product path never routes around the HIP code.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libaicam.so")

OK, ERR_INVALID, ERR_NOT_FOUND, ERR_RUNTIME, ERR_NO_DEVICE, ERR_CAPACITY, ERR_FORMAT = 0, -1, -2, -3, -4, -5, -6
HOST, DEVICE = 0, 1
F32, F16 = 0, 1
MODEL_YOLO, MODEL_REID = 1, 2
PIX_BGR24, PIX_NV12, PIX_I420 = 0, 1, 2
YUV_BT601, YUV_BT709 = 0, 1
YUV_LIMITED, YUV_FULL = 0, 1
PROF_CLASSES = ("conv_igemm", "conv_direct", "misc", "letterbox", "crop_resize", "decode_nms", "tracker")


class AicError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libaicam error {code}: {msg}")
        self.code = code


class NoDeviceError(AicError):
    pass


class TrackerParams(C.Structure):
    _fields_ = [("max_cosine_distance", C.c_double), ("max_iou_distance", C.c_double), ("nn_budget", C.c_int32),
                ("max_age", C.c_int32), ("n_init", C.c_int32), ("max_tracks", C.c_int32),
                ("feature_dim", C.c_int32), ("first_track_id", C.c_int32)]


class ByteTrackParams(C.Structure):
    _fields_ = [("track_thresh", C.c_double), ("low_thresh", C.c_double), ("new_track_thresh", C.c_double),
                ("match_thresh", C.c_double), ("track_buffer", C.c_int32), ("frame_rate", C.c_int32),
                ("fuse_score", C.c_int32), ("max_tracks", C.c_int32), ("first_track_id", C.c_int32)]


class OCSortParams(C.Structure):
    _fields_ = [("det_thresh", C.c_double), ("iou_threshold", C.c_double), ("inertia", C.c_double), ("max_age", C.c_int32),
                ("min_hits", C.c_int32), ("delta_t", C.c_int32), ("use_byte", C.c_int32), ("max_tracks", C.c_int32),
                ("first_track_id", C.c_int32)]


class BoTSORTParams(C.Structure):
    _fields_ = [("track_high_thresh", C.c_double), ("track_low_thresh", C.c_double), ("new_track_thresh", C.c_double),
                ("match_thresh", C.c_double), ("proximity_thresh", C.c_double), ("appearance_thresh", C.c_double),
                ("feat_alpha", C.c_double), ("track_buffer", C.c_int32), ("frame_rate", C.c_int32), ("fuse_score", C.c_int32),
                ("with_reid", C.c_int32), ("feature_dim", C.c_int32), ("max_tracks", C.c_int32), ("first_track_id", C.c_int32)]


class GmcParams(C.Structure):
    _fields_ = [("downscale", C.c_int32), ("min_inliers", C.c_int32)]


class BestShotConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("streams", "frame_h", "frame_w", "thumb_w", "thumb_h", "max_tracks", "forget_after", "region",
                                         "head_q8", "pad", "min_w", "min_h")]


class SceneConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("streams", "frame_h", "frame_w", "cell")]


class LeftConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("streams", "frame_h", "frame_w", "cell", "max_objects")]


class ColoursConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("streams", "frame_h", "frame_w", "max_tracks", "forget_after", "torso0", "torso1", "legs0", "legs1",
                                         "inset_q8", "min_w", "min_h", "max_cover_q8")]


class HeatConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("streams", "frame_h", "frame_w", "cell", "max_tracks", "forget_after", "anchor", "min_move")]


class ProxConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("streams", "frame_h", "frame_w", "max_tracks", "forget_after", "metric", "near", "height_ratio_q8",
                                         "link_ticks", "unlink_ticks", "speed_shift", "still_speed", "run_speed")]


class JpegConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("max_images", "height", "width", "quality", "restart", "subsampling")] + [("max_bytes", C.c_int64)]


class JpegdecConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("max_images", "height", "width")]


class JpegdecInfo(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("status", "reason", "width", "height", "components", "sampling", "restart", "intervals")] + [
        ("entropy_offset", C.c_int64), ("entropy_bytes", C.c_int64)]


class PipelineParams(C.Structure):
    _fields_ = [("frame_h", C.c_int32), ("frame_w", C.c_int32), ("batch", C.c_int32), ("ring_frames", C.c_int32),
                ("max_persons", C.c_int32), ("conf_thresh", C.c_float), ("iou_thresh", C.c_float),
                ("max_det", C.c_int32), ("min_confidence", C.c_float), ("inject", C.c_int32),
                ("track_class_mask", C.c_uint64 * 2), ("tracker", TrackerParams)]


_P = C.c_void_p
_I = C.c_int
_F = C.c_float
_D = C.c_double
_SIGS = {
    "aic_last_error": (C.c_char_p, []),
    "aic_abi_version": (_I, []),
    "aic_device_count": (_I, [_P]),
    "aic_device_sync": (_I, [_I]),
    "aic_model_load": (_I, [C.c_char_p, _I, _I, _I, _P]),
    "aic_model_load_mem": (_I, [_P, C.c_size_t, _I, _I, _I, _P]),
    "aic_model_read_buffer": (_I, [_P, _I, _P, C.c_size_t]),
    "aic_model_conv_plan": (_I, [_P, _I, _I, _P]),
    "aic_model_conv_plan_live": (_I, [_P, _I, _I, _P]),
    "aic_model_row_band": (_I, [_P, _I, _I, _I, _P]),
    "aic_model_sparse_box": (_I, [_P, _I, _P]),
    "aic_debug_alloc_probe": (_I, [_I, _P, _P, _P, _P]),
    "aic_model_read_det": (_I, [_P, _I, _P, _P, _P]),
    "aic_detect_decode": (_I, [_P, _I, _I, _I, _F, _F, _I, _P, _P, _P, _P]),
    "aic_detect_live": (_I, [_P, _P, _I, _I, _I, _I, _I, _F, _F, _I, _P, _P, _P, _P]),
    "aic_model_destroy": (_I, [_P]),
    "aic_model_info": (_I, [_P, _P, _P, _P, _P, _P, _P, _P]),
    "aic_yolo_infer": (_I, [_P, _P, _I, _I, _F, _F, _I, _P, _P, _P, _P]),
    "aic_yolo_head": (_I, [_P, _P, _I, _I, _P, _P]),
    "aic_yolo_decode": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "aic_yolo_postprocess": (_I, [_P, _P, _P, _I, _F, _F, _I, _I, _F, _F, _F, _I, _I] + [_P] * 9),
    "aic_det_filter": (_I, [_I, _P, _P, _P, _P, _I, _I, _F, _P, _I] + [_P] * 9),
    "aic_reid_infer": (_I, [_P, _P, _I, _I, _P, _I]),
    "aic_reid_infer_live": (_I, [_P, _P, _I, _I, _I, _P, _I]),
    "aic_letterbox": (_I, [_I, _P, _I, _I, _I, _I, _P, _P, _P, _P]),
    "aic_letterbox_image": (_I, [_I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "aic_crop_resize": (_I, [_I, _P, _I, _I, _P, _I, _I, _I, _P, _P]),
    "aic_detect": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _I, _P, _P, _P, _P]),
    "aic_reid_embed": (_I, [_P, _P, _I, _I, _I, _P, _I, _P, _P]),
    "aic_crop_resize_ex": (_I, [_I, _P, _I, _I, _I, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "aic_reid_embed_bank": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _P, _P]),
    "aic_kf_initiate": (_I, [_I, _P, _I, _P, _P]),
    "aic_kf_predict": (_I, [_I, _P, _P, _I]),
    "aic_kf_predict_dt": (_I, [_I, _P, _P, _I, _F]),
    "aic_kf_project": (_I, [_I, _P, _P, _I, _P, _P]),
    "aic_kf_update": (_I, [_I, _P, _P, _P, _I]),
    "aic_kf_gating": (_I, [_I, _P, _P, _I, _P, _I, _I, _I, _P]),
    "aic_iou_cost": (_I, [_I, _P, _I, _P, _I, _P]),
    "aic_appearance_cost": (_I, [_I, _P, _P, _I, _I, _I, _P, _P, _I, _P]),
    "aic_lsap": (_I, [_P, _I, _I, _P, _P]),
    "aic_min_cost_matching": (_I, [_P, _I, _I, _D, _P, _P, _P]),
    "aic_match_cascade": (_I, [_P, _P, _P, _I, _I, _P, _P, _D, _D, _I, _P, _P, _P, _P, _P, _P, _P]),
    "aic_match_cascade_device": (_I, [_I, _P, _P, _P, _I, _I, _P, _P, _D, _D, _I, _I, _P, _P]),
    "aic_trk_prep_test": (_I, [_I, _I, _I, _P, _P, _P, _I, _I, _P, _I, _P, _P, _P, _I, _I, _P, _P]),
    "aic_tracker_option": (_I, [_P, C.c_char_p, _I]),
    "aic_tracker_create": (_I, [_I, _P, _P]),
    "aic_tracker_destroy": (_I, [_P]),
    "aic_tracker_predict": (_I, [_P]),
    "aic_tracker_update": (_I, [_P, _P, _P, _P, _P, _I, _P, _I, _I]),
    "aic_tracker_update_batch": (_I, [_P, _I, _P, _P, _P, _P, _P, _I, _P, _I, _I, _P, _P, _P, _P, _P, _P]),
    "aic_tracker_import_state": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I]),
    "aic_tracker_next_track_id": (_I, [_P, _P]),
    "aic_tracker_assoc_counters": (_I, [_P, _P, _P]),
    "aic_tracker_outputs": (_I, [_P, _P, _P, _I, _P]),
    "aic_tracker_num_tracks": (_I, [_P, _P]),
    "aic_tracker_export": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "aic_tracker_export_gallery": (_I, [_P, _I, _P, _I]),
    "aic_tracker_last_matches": (_I, [_P, _P, _P, _I, _P]),
    "aic_tracker_last_costs": (_I, [_P, _P, _P, _P, _I, _P, _P]),
    "aic_pipeline_create": (_I, [_P, _P, _P, _P]),
    "aic_pipeline_destroy": (_I, [_P]),
    "aic_pipeline_upload": (_I, [_P, _I, _P, _I]),
    "aic_pipeline_inject": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "aic_pipeline_run": (_I, [_P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "aic_pipeline_run_passes": (_I, [_P, _I, _I, _I, _P, _P, _P, _P]),
    "aic_pipeline_run_from_host": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "aic_pipeline_run_from_host_passes": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "aic_pipeline_group_times": (_I, [_P, _P, _P, _P, _I, _P]),
    "aic_pipeline_exchange_enable": (_I, [_P, _P, _P, _I, _I]),
    "aic_pipeline_exchange_stream": (_I, [_P, _P]),
    "aic_pipeline_exchange_wait": (_I, [_P, C.c_int64, _I, _P, _P]),
    "aic_pipeline_exchange_done": (_I, [_P, C.c_int64]),
    "aic_gallery_annotate": (_I, [_I, _P, _P, _I, _I, _I, _I, _D, _P, _P, _P, _P]),
    "aic_gid_create": (_I, [_I, _P]),
    "aic_gid_destroy": (_I, [_P]),
    "aic_gid_update": (_I, [_P, _I, _I, _P, _P, _P, _D, _P]),
    "aic_gid_lookup": (_I, [_P, _I, _I, _P]),
    "aic_gid_size": (_I, [_P, _P, _P, _P]),
    "aic_host_register": (_I, [_P, C.c_size_t]),
    "aic_host_unregister": (_I, [_P]),
    "aic_pipeline_tracker": (_I, [_P, _P]),
    "aic_pipeline_stats": (_I, [_P, _P, _P, _P, _P, _I]),
    "aic_pipeline_last_embeddings": (_I, [_P, _P, _I, _P, _P]),
    "aic_pipeline_option": (_I, [_P, C.c_char_p, _I]),
    "aic_pipeline_counters": (_I, [_P, _P, _P]),
    "aic_pipeline_assoc_frames": (_I, [_P, _P, _P]),
    "aic_pipeline_filter_counters": (_I, [_P, _P, _P, _P]),
    "aic_pipeline_lane_groups": (_I, [_P, _P]),
    "aic_pipeline_group_embeddings": (_I, [_P, _P, _I, _P, _I, _P, _P, _P]),
    "aic_overlay": (_I, [_I, _P, _I, _I, _I, _P, _I, _P, _I]),
    "aic_prof_enable": (_I, [_I, _I]),
    "aic_prof_reset": (_I, [_I]),
    "aic_prof_read": (_I, [_I, _I, _P, _P, _P, _P]),
    "aic_prof_read_union": (_I, [_I, _I, _P]),
    "aic_bytetrack_create": (_I, [_I, _P, _P]),
    "aic_bytetrack_destroy": (_I, [_P]),
    "aic_bytetrack_option": (_I, [_P, C.c_char_p, _I]),
    "aic_bytetrack_update_batch": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "aic_bytetrack_export": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "aic_bytetrack_counters": (_I, [_P, _P, _P, _P]),
    "aic_pipeline_create_bytetrack": (_I, [_P, _P, _P, _P]),
    "aic_ocsort_create": (_I, [_I, _P, _P]),
    "aic_ocsort_destroy": (_I, [_P]),
    "aic_ocsort_option": (_I, [_P, C.c_char_p, _I]),
    "aic_ocsort_update_batch": (_I, [_P, _I, _P, _P, _P, _P, _I, _P, _P, _P]),
    "aic_ocsort_export": (_I, [_P, _I] + [_P] * 14),
    "aic_ocsort_counters": (_I, [_P] * 8),
    "aic_pipeline_create_ocsort": (_I, [_P, _P, _P, _P]),
    "aic_botsort_create": (_I, [_I, _P, _P]),
    "aic_botsort_destroy": (_I, [_P]),
    "aic_botsort_option": (_I, [_P, C.c_char_p, _I]),
    "aic_botsort_update_batch": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P]),
    "aic_botsort_export": (_I, [_P, _I] + [_P] * 13),
    "aic_botsort_counters": (_I, [_P] * 7),
    "aic_pipeline_create_botsort": (_I, [_P, _P, _P, _P, _P]),
    "aic_bytetrack_bank_create": (_I, [_I, _P, _I, _P]),
    "aic_bytetrack_bank_destroy": (_I, [_P]),
    "aic_bytetrack_bank_option": (_I, [_P, C.c_char_p, _I]),
    "aic_bytetrack_bank_update": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "aic_bytetrack_bank_reset": (_I, [_P, _I]),
    "aic_bytetrack_bank_export": (_I, [_P, _I, _I] + [_P] * 11),
    "aic_bytetrack_bank_counters": (_I, [_P, _I, _P, _P, _P]),
    "aic_ocsort_bank_create": (_I, [_I, _P, _I, _P]),
    "aic_ocsort_bank_destroy": (_I, [_P]),
    "aic_ocsort_bank_option": (_I, [_P, C.c_char_p, _I]),
    "aic_ocsort_bank_update": (_I, [_P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "aic_ocsort_bank_reset": (_I, [_P, _I]),
    "aic_ocsort_bank_export": (_I, [_P, _I, _I] + [_P] * 14),
    "aic_ocsort_bank_counters": (_I, [_P, _I] + [_P] * 7),
    "aic_pipeline_reset_stream": (_I, [_P, _I]),
    "aic_gmc_create": (_I, [_I, _I, _I, _P, _P]),
    "aic_gmc_destroy": (_I, [_P]),
    "aic_gmc_reset": (_I, [_P]),
    "aic_gmc_estimate_batch": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "aic_pipeline_group_warps": (_I, [_P, _P, _I, _P]),
    "aic_botsort_bank_create": (_I, [_I, _P, _I, _P]),
    "aic_botsort_bank_destroy": (_I, [_P]),
    "aic_botsort_bank_option": (_I, [_P, C.c_char_p, _I]),
    "aic_botsort_bank_update": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "aic_botsort_bank_reset": (_I, [_P, _I]),
    "aic_botsort_bank_export": (_I, [_P, _I, _I] + [_P] * 13),
    "aic_botsort_bank_counters": (_I, [_P, _I] + [_P] * 6),
    "aic_gmc_bank_create": (_I, [_I, _I, _I, _P, _I, _P]),
    "aic_gmc_bank_destroy": (_I, [_P]),
    "aic_gmc_bank_reset": (_I, [_P, _I]),
    "aic_gmc_bank_estimate": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "aic_pipeline_create_botsort_bank": (_I, [_P, _P, _P, _P, _I, _P]),
    "aic_deepsort_bank_create": (_I, [_I, _P, _I, _P]),
    "aic_deepsort_bank_destroy": (_I, [_P]),
    "aic_deepsort_bank_option": (_I, [_P, C.c_char_p, _I]),
    "aic_deepsort_bank_update": (_I, [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "aic_deepsort_bank_reset": (_I, [_P, _I]),
    "aic_deepsort_bank_export": (_I, [_P, _I, _I] + [_P] * 11),
    "aic_deepsort_bank_export_gallery": (_I, [_P, _I, _I, _P, _I]),
    "aic_deepsort_bank_counters": (_I, [_P, _I, _P, _P]),
    "aic_gid_forget_rank": (_I, [_P, _I]),
    "aic_xcam_create": (_I, [_I, _I, _I, _I, _D, _P]),
    "aic_xcam_destroy": (_I, [_P]),
    "aic_xcam_option": (_I, [_P, C.c_char_p, _I]),
    "aic_xcam_link_deepsort_bank": (_I, [_P, _P, _P]),
    "aic_xcam_link_botsort_bank": (_I, [_P, _P, _P]),
    "aic_xcam_link_shards": (_I, [_P, _P, _P, _I, _P]),
    "aic_xcam_tables": (_I, [_P, _P, _P, _P]),
    "aic_xcam_shards": (_I, [_P, _P]),
    "aic_xcam_global_ids": (_I, [_P, _I, _P, _I, _P]),
    "aic_xcam_size": (_I, [_P, _P, _P, _P]),
    "aic_xcam_forget_stream": (_I, [_P, _I]),
    "aic_pipeline_link_cameras": (_I, [_P, _P, _P]),
    "aic_pipeline_create_deepsort_bank": (_I, [_P, _P, _P, _I, _P]),
    "aic_pipeline_deepsort_bank": (_I, [_P, _P]),
    "aic_zones_create": (_I, [_I, _I, _I, _I, _I, _P]),
    "aic_zones_destroy": (_I, [_P]),
    "aic_zones_set": (_I, [_P, _I, _I, _P, _P, _I, _P]),
    "aic_zones_update": (_I, [_P, _P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "aic_zones_counters": (_I, [_P, _I, _P, _P, _P, _P]),
    "aic_zones_reset": (_I, [_P, _I]),
    "aic_zones_option": (_I, [_P, C.c_char_p, _I]),
    "aic_render_create": (_I, [_I, _I, _P]),
    "aic_render_destroy": (_I, [_P]),
    "aic_render_option": (_I, [_P, C.c_char_p, C.c_int64]),
    "aic_render_set_masks": (_I, [_P, _I, _I, _P, _P]),
    "aic_render_rects": (_I, [_P, _P, _I, _P, _P]),
    "aic_render_frames": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P, _P, _P, _I, _P]),
    "aic_bestshot_params": (_I, [_I, _I, _I, _P]),
    "aic_bestshot_create": (_I, [_I, _P, _P]),
    "aic_bestshot_destroy": (_I, [_P]),
    "aic_bestshot_option": (_I, [_P, C.c_char_p, _I]),
    "aic_bestshot_reset": (_I, [_P, _I]),
    "aic_bestshot_update": (_I, [_P, _P, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "aic_bestshot_flush": (_I, [_P, _I, _I, _P, _P, _P, _P, _P]),
    "aic_bestshot_export": (_I, [_P, _I, _P, _P, _P]),
    "aic_bestshot_counters": (_I, [_P, _P, _P, _P]),
    "aic_scene_config_default": (_I, [_I, _I, _I, _P]),
    "aic_scene_create": (_I, [_I, _P, _P]),
    "aic_scene_destroy": (_I, [_P]),
    "aic_scene_option": (_I, [_P, C.c_char_p, _I]),
    "aic_scene_reset": (_I, [_P, _I]),
    "aic_scene_update": (_I, [_P, _P, _I, _I, _P, _P, _I, _P, _P, _P]),
    "aic_scene_export": (_I, [_P, _I, _P, _P, _P, _P]),
    "aic_left_config_default": (_I, [_I, _I, _I, _P]),
    "aic_left_create": (_I, [_I, _P, _P]),
    "aic_left_destroy": (_I, [_P]),
    "aic_left_option": (_I, [_P, C.c_char_p, _I]),
    "aic_left_reset": (_I, [_P, _I]),
    "aic_left_update": (_I, [_P, _P, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P]),
    "aic_left_export": (_I, [_P, _I, _P, _P, _P, _P, _P, _P, _P]),
    "aic_colours_config_default": (_I, [_I, _I, _I, _P]),
    "aic_colours_create": (_I, [_I, _P, _P]),
    "aic_colours_destroy": (_I, [_P]),
    "aic_colours_option": (_I, [_P, C.c_char_p, _I]),
    "aic_colours_reset": (_I, [_P, _I]),
    "aic_colours_update": (_I, [_P, _P, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "aic_colours_flush": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "aic_colours_export": (_I, [_P, _I, _P, _P]),
    "aic_colours_classify": (_I, [_P, _I, _P]),
    "aic_heat_config_default": (_I, [_I, _I, _I, _P]),
    "aic_heat_create": (_I, [_I, _P, _P]),
    "aic_heat_destroy": (_I, [_P]),
    "aic_heat_option": (_I, [_P, C.c_char_p, _I]),
    "aic_heat_reset": (_I, [_P, _I]),
    "aic_heat_update": (_I, [_P, _I, _P, _P, _I, _I, _P, _P, _P, _P, _P]),
    "aic_heat_flush": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "aic_heat_export": (_I, [_P, _I, _P, _P]),
    "aic_heat_decay": (_I, [_P, _I, _I, _I]),
    "aic_heat_export_layers": (_I, [_P, _I, _I, _P]),
    "aic_heat_import_layers": (_I, [_P, _I, _I, _P]),
    "aic_heat_set_lut": (_I, [_P, _P]),
    "aic_heat_lut": (_I, [_P]),
    "aic_heat_render": (_I, [_P, _P, _I, _I, _P, _I]),
    "aic_prox_config_default": (_I, [_I, _I, _I, _P]),
    "aic_prox_create": (_I, [_I, _P, _P]),
    "aic_prox_destroy": (_I, [_P]),
    "aic_prox_option": (_I, [_P, C.c_char_p, _I]),
    "aic_prox_reset": (_I, [_P, _I]),
    "aic_prox_set_ground": (_I, [_P, _I, _P, _I]),
    "aic_prox_update": (_I, [_P, _I, _P, _P, _I, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P]),
    "aic_prox_flush": (_I, [_P, _I, _I, _P, _P, _P, _P]),
    "aic_prox_export": (_I, [_P, _I, _P, _P]),
    "aic_prox_export_pairs": (_I, [_P, _I, _P, _P]),
    "aic_jpeg_tables": (_I, [_I, _P, _P]),
    "aic_jpeg_header": (_I, [_I, _I, _I, _I, _I, _P, _I, _P]),
    "aic_jpeg_config_default": (_I, [_I, _I, _P]),
    "aic_jpeg_create": (_I, [_I, _P, _P]),
    "aic_jpeg_destroy": (_I, [_P]),
    "aic_jpeg_option": (_I, [_P, C.c_char_p, _I]),
    "aic_jpeg_worst_case_bytes": (_I, [_P, _P]),
    "aic_jpeg_encode": (_I, [_P, _P, _I, _I, _P, _I, C.c_int64, _P, _P]),
    "aic_jpeg_coefficients": (_I, [_P, _P, _I, _I, _P]),
    "aic_jpeg_counters": (_I, [_P, _P, _P, _P]),
    "aic_jpegdec_probe": (_I, [_P, C.c_int64, _P]),
    "aic_jpegdec_create": (_I, [_I, _P, _P]),
    "aic_jpegdec_destroy": (_I, [_P]),
    "aic_jpegdec_option": (_I, [_P, C.c_char_p, _I]),
    "aic_jpegdec_decode": (_I, [_P, _P, _I, _P, _I, _P, _I, _P, _P]),
    "aic_jpegdec_coefficients": (_I, [_P, _P, _I, _P, _I, _I, _P]),
    "aic_jpegdec_counters": (_I, [_P, _P, _P, _P, _P]),
    "aic_pipeline_upload_jpeg": (_I, [_P, _I, _P, _I, _P, _I, _P, _P]),
    "aic_yuv_coeffs": (_I, [_I, _I, _P, _P, _P]),
    "aic_frames_to_bgr": (_I, [_I, _P, _I, _I, _I, _I, C.c_int64, C.c_int64, _I, _I, _I, _P]),
    "aic_frames_from_bgr": (_I, [_I, _P, _I, _I, _I, _I, C.c_int64, C.c_int64, _I, _I, _I, _P]),
    "aic_pipeline_read_frames": (_I, [_P, _I, _I, _P]),
    "aic_archive_index_create": (_I, [C.c_int64, _P]),
    "aic_archive_index_destroy": (_I, [_P]),
    "aic_archive_index_assign": (_I, [_P, _P, _P, C.c_int64, _I, _P, _P]),
    "aic_archive_index_find": (_I, [_P, C.c_int64, _P]),
    "aic_archive_index_remove": (_I, [_P, C.c_int64, _P]),
    "aic_archive_index_size": (_I, [_P, _P, _P]),
    "aic_archive_create": (_I, [_I, C.c_int64, _I, _P]),
    "aic_archive_destroy": (_I, [_P]),
    "aic_archive_put": (_I, [_P, _P, _P, C.c_int64, _P, _I, _I]),
    "aic_archive_remove": (_I, [_P, C.c_int64]),
    "aic_archive_search": (_I, [_P, _P, _I, _I, _I, _P, _P, _P, _P]),
    "aic_archive_size": (_I, [_P, _P, _P]),
    "aic_archive_export": (_I, [_P] * 8),
    "aic_archive_import": (_I, [_P] * 7 + [C.c_int64]),
    "aic_archive_clear": (_I, [_P]),
    "aic_archive_block_rows": (_I, [_P, _I, _P]),
    "aic_gid_find_key": (_I, [_P, C.c_int64, _P]),
    "aic_gid_link_keys": (_I, [_P, C.c_int64, C.c_int64, _P]),
    "aic_xcam_attach_archive": (_I, [_P, _P]),
    "aic_xcam_returning": (_I, [_P, _P, _P, _P, _P, _I, _P]),
}
EXPORTS = tuple(_SIGS)

_lib = None


def load():
    """Load libaicam.so (building nothing: see build.py / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: run `python ai-camera_amd/build.py` (hipcc, gfx950). "
                              "There is no CPU fallback for the hot path.")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)          # AttributeError if the ABI is incomplete
            fn.restype, fn.argtypes = res, args
        _lib = lib
    return _lib


def check(rc):
    if rc != OK:
        msg = load().aic_last_error().decode("utf-8", "replace")
        raise (NoDeviceError if rc == ERR_NO_DEVICE else AicError)(rc, msg)


def call(name, *args):
    check(getattr(load(), name)(*args))


def ptr(a):
    """void* of a C-contiguous NumPy array (or None), or the raw address of a device buffer."""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    assert a.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return a.ctypes.data_as(C.c_void_p)


def as_f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def device_count() -> int:
    n = C.c_int(0)
    call("aic_device_count", C.byref(n))
    return n.value


def debug_alloc_probe(device=0):
    """Tests: the first four elements of fresh, unwritten float / int32 / uint8 device buffers and of a page-locked uint8 buffer
    (aic_debug_alloc_probe, include/aicam.h): what AICAM_POISON_ALLOC filled them with in this process."""
    out = {"f32": np.zeros(4, np.float32), "i32": np.zeros(4, np.int32), "u8": np.zeros(4, np.uint8), "pinned_u8": np.zeros(4, np.uint8)}
    call("aic_debug_alloc_probe", int(device), *(ptr(out[k]) for k in ("f32", "i32", "u8", "pinned_u8")))
    return out


def prof_read(device=0):
    out = {}
    for i, name in enumerate(PROF_CLASSES):
        ms, n, fl, by = C.c_double(), C.c_int64(), C.c_double(), C.c_double()
        call("aic_prof_read", device, i, C.byref(ms), C.byref(n), C.byref(fl), C.byref(by))
        mu = C.c_double()
        call("aic_prof_read_union", device, i, C.byref(mu))
        out[name] = dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value, ms_union=mu.value)
    return out
