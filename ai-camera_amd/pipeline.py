"""TrackingPipeline: the batched end-to-end path (aic_pipeline_*) -- the loop body of
src/aicamera_tracker.py:169-207 over frames resident in HBM -- plus helpers shared by bench.py,
the CLI and the tests."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L
from . import config
from . import frames
from .core.tracker_core import TrackerCore
from .hip_engine import HipEngine


class TrackingPipeline:
    def __init__(self, yolo_engine, reid_engine, frame_hw, batch=8, ring_frames=None, max_persons=32, device=0,
                 dtype="fp16", conf_thresh=None, iou_thresh=config.YOLO_NMS_THRESHOLD,
                 max_det=config.YOLO_MAX_DET, min_confidence=config.DEEPSORT_MIN_CONFIDENCE, inject=False,
                 max_cosine_distance=config.DEEPSORT_MAX_DIST, nn_budget=config.DEEPSORT_NN_BUDGET,
                 max_iou_distance=config.DEEPSORT_MAX_IOU_DISTANCE, max_age=config.DEEPSORT_MAX_AGE,
                 n_init=config.DEEPSORT_N_INIT, max_tracks=512, tracker="deepsort", gmc=0, streams=1, _cameras=0,
                 pixel_format="bgr24", yuv_matrix="bt601", yuv_range="limited", **bytetrack_params):
        """tracker="bytetrack": a detector-only pipeline with ByteTrack (aic_pipeline_create_bytetrack); reid_engine may be None and is
        not used, bytetrack_params are BYTETracker's (track_thresh, track_buffer, match_thresh, mot20, frame_rate, low_thresh), and
        conf_thresh defaults to low_thresh so that the detector hands over ByteTrack's low band.
        tracker="ocsort": the same pipeline with OC-SORT (aic_pipeline_create_ocsort); the extra arguments are OCSort's (det_thresh,
        min_hits, iou_threshold, delta_t, inertia, use_byte; max_age is the named argument), and conf_thresh defaults to det_thresh,
        or to 0.1 with use_byte.
        tracker="botsort": BoT-SORT WITH the ReID engine (aic_pipeline_create_botsort): crop + ReID as for DeepSORT, the embeddings stay
        in HBM and feed the epoch kernel; the extra arguments are BoTSORT's (track_high_thresh, track_low_thresh, new_track_thresh,
        match_thresh, proximity_thresh, appearance_thresh, track_buffer, frame_rate, fuse_score, with_reid, feat_alpha), and conf_thresh
        defaults to track_low_thresh.  gmc=2 or 4 (BoT-SORT only): the camera motion of every frame is estimated on the device at that
        downscale (aic_pipeline_option "gmc", gmc.py) and warps the predicted tracks; group_warps() reads the last group's.
        streams=S (ByteTrack / OC-SORT only): one pipeline for S cameras.  The ring and every run range are tick-major, slot t * S + s
        being tick t of stream s; batch, slot and count are multiples of S, and the tracker is a bank of S streams.
        BoT-SORT or DeepSORT for S cameras: TrackingPipeline.botsort_bank(...) / TrackingPipeline.deepsort_bank(...), which pass the
        camera count as _cameras.
        pixel_format="nv12" or "i420" (any tracker, the bank constructors included; yuv_matrix "bt601" / "bt709", yuv_range "limited" /
        "full"): upload, run_raw_from_host*, run_from_host and stream take uint8 [n, H*3/2, W] frames instead of [n, H, W, 3]; they are
        unpacked into the BGR ring on the copy stream (frames.py, set_pixel_format), read_frames returns ring slots as BGR."""
        self._pix = (frames.format_code(pixel_format), frames.matrix_code(yuv_matrix), frames.range_code(yuv_range))
        self.streams = int(_cameras) or int(streams)
        self.cameras, self._device, self.xcam, self.link_after_run, self._bank = int(_cameras), device, None, False, None
        if _cameras and tracker not in ("botsort", "deepsort"):
            raise ValueError("a camera count needs TrackingPipeline.botsort_bank or TrackingPipeline.deepsort_bank")
        if int(streams) != 1 and tracker not in ("bytetrack", "ocsort"):
            raise ValueError("streams needs tracker='bytetrack' or 'ocsort'")
        if gmc and tracker != "botsort":
            raise ValueError("gmc needs tracker='botsort'")
        if tracker not in ("deepsort", "bytetrack", "ocsort", "botsort"):
            raise ValueError(f"tracker must be 'deepsort', 'bytetrack', 'ocsort' or 'botsort', not {tracker!r}")
        if tracker == "deepsort" and bytetrack_params:
            raise TypeError(f"unexpected arguments for a DeepSORT pipeline: {sorted(bytetrack_params)}")
        self.tracker_kind = tracker
        self.frame_h, self.frame_w = int(frame_hw[0]), int(frame_hw[1])
        self.batch = int(batch)
        self.ring_frames = int(ring_frames or 4 * batch)
        self.max_persons, self.max_det = int(max_persons), int(max_det)
        self.yolo = yolo_engine if isinstance(yolo_engine, HipEngine) else HipEngine(
            yolo_engine, device=device, dtype=dtype, max_items=self.batch, warm_up=False)
        lo, hi = config.track_class_mask()
        if tracker == "bytetrack":
            from .bytetrack import bytetrack_params as _btp
            self.reid = None
            self.bytetrack_params = _btp(max_tracks=max_tracks, **bytetrack_params)
            if conf_thresh is None:
                conf_thresh = self.bytetrack_params.low_thresh
            tp = L.TrackerParams(0.2, 0.7, 1, 1, 1, 1, 0, 1)          # ignored by aic_pipeline_create_bytetrack
            self.params = L.PipelineParams(self.frame_h, self.frame_w, self.batch, self.ring_frames, self.max_persons,
                                           float(conf_thresh), float(iou_thresh), self.max_det, 0.0,
                                           int(bool(inject)), (C.c_uint64 * 2)(lo, hi), tp)
            self._h = C.c_void_p()
            L.call("aic_pipeline_create_bytetrack", self.yolo._h, C.byref(self.params), C.byref(self.bytetrack_params),
                   C.byref(self._h))
            self.tracker_core = None
            if self.streams != 1:
                self.option("streams", self.streams)
            self._apply_pixel_format()
            return
        if tracker == "ocsort":
            from .ocsort import ocsort_params as _ocp
            self.reid = None
            # max_age is a named argument here: left at the DeepSORT default it means OC-SORT's own default (30)
            oc_age = 30 if max_age == config.DEEPSORT_MAX_AGE else max_age
            self.ocsort_params = _ocp(max_tracks=max_tracks, max_age=oc_age, **bytetrack_params)
            if conf_thresh is None:
                conf_thresh = 0.1 if self.ocsort_params.use_byte else self.ocsort_params.det_thresh
            tp = L.TrackerParams(0.2, 0.7, 1, 1, 1, 1, 0, 1)          # ignored by aic_pipeline_create_ocsort
            self.params = L.PipelineParams(self.frame_h, self.frame_w, self.batch, self.ring_frames, self.max_persons,
                                           float(conf_thresh), float(iou_thresh), self.max_det, 0.0,
                                           int(bool(inject)), (C.c_uint64 * 2)(lo, hi), tp)
            self._h = C.c_void_p()
            L.call("aic_pipeline_create_ocsort", self.yolo._h, C.byref(self.params), C.byref(self.ocsort_params), C.byref(self._h))
            self.tracker_core = None
            if self.streams != 1:
                self.option("streams", self.streams)
            self._apply_pixel_format()
            return
        if tracker == "botsort":
            from .botsort import botsort_params as _bsp
            self.reid = reid_engine if isinstance(reid_engine, HipEngine) else HipEngine(
                reid_engine, device=device, dtype=dtype, max_items=self.batch * self.max_persons, warm_up=False)
            self.botsort_params = _bsp(max_tracks=max_tracks, feature_dim=int(self.reid.out_dim), **bytetrack_params)
            if conf_thresh is None:
                conf_thresh = self.botsort_params.track_low_thresh
            tp = L.TrackerParams(0.2, 0.7, 1, 1, 1, 1, 0, 1)          # ignored by aic_pipeline_create_botsort
            self.params = L.PipelineParams(self.frame_h, self.frame_w, self.batch, self.ring_frames, self.max_persons,
                                           float(conf_thresh), float(iou_thresh), self.max_det, 0.0,
                                           int(bool(inject)), (C.c_uint64 * 2)(lo, hi), tp)
            self._h = C.c_void_p()
            if _cameras:
                L.call("aic_pipeline_create_botsort_bank", self.yolo._h, self.reid._h, C.byref(self.params), C.byref(self.botsort_params),
                       int(_cameras), C.byref(self._h))
            else:
                L.call("aic_pipeline_create_botsort", self.yolo._h, self.reid._h, C.byref(self.params), C.byref(self.botsort_params),
                       C.byref(self._h))
            self.tracker_core = None
            if gmc:
                self.option("gmc", int(gmc))
            self._apply_pixel_format()
            return
        if conf_thresh is None:
            conf_thresh = config.YOLO_CONF_THRESHOLD
        self.reid = reid_engine if isinstance(reid_engine, HipEngine) else HipEngine(
            reid_engine, device=device, dtype=dtype, max_items=self.batch * self.max_persons, warm_up=False)
        tp = L.TrackerParams(float(max_cosine_distance), float(max_iou_distance), int(nn_budget or 0), int(max_age),
                             int(n_init), int(max_tracks), int(self.reid.out_dim), 1)
        self.params = L.PipelineParams(self.frame_h, self.frame_w, self.batch, self.ring_frames, self.max_persons,
                                       float(conf_thresh), float(iou_thresh), self.max_det, float(min_confidence),
                                       int(bool(inject)), (C.c_uint64 * 2)(lo, hi), tp)
        self._h = C.c_void_p()
        if _cameras:                                             # a DeepSORT bank: the cameras' state is .bank's, there is no single tracker
            L.call("aic_pipeline_create_deepsort_bank", self.yolo._h, self.reid._h, C.byref(self.params), int(_cameras), C.byref(self._h))
            self.tracker_params, self.tracker_core = tp, None
            self._apply_pixel_format()
            return
        L.call("aic_pipeline_create", self.yolo._h, self.reid._h, C.byref(self.params), C.byref(self._h))
        th = C.c_void_p()
        L.call("aic_pipeline_tracker", self._h, C.byref(th))
        self.tracker_core = TrackerCore._from_handle(th, tp)
        self.tracker_core._dim = self.reid.out_dim
        self._apply_pixel_format()

    def _apply_pixel_format(self):
        if self._pix != (L.PIX_BGR24, L.YUV_BT601, L.YUV_LIMITED):
            self.set_pixel_format(*self._pix)

    def set_pixel_format(self, pixel_format="bgr24", yuv_matrix="bt601", yuv_range="limited"):
        """Between calls: the format of the host frames that upload / run*_from_host / stream take from now on."""
        pix = (frames.format_code(pixel_format), frames.matrix_code(yuv_matrix), frames.range_code(yuv_range))
        for key, v in zip(("pixel_format", "yuv_matrix", "yuv_range"), pix):
            self.option(key, v)
        self._pix = pix
        if hasattr(self, "_staging"):                            # stream()'s pinned buffers have the old format's shape
            for b in self._staging:
                self.unpin(b)
            del self._staging

    @property
    def host_frame_shape(self):
        """Shape of one host frame in the pipeline's pixel format: (H, W, 3) BGR24, (H*3/2, W) NV12 / I420."""
        return (self.frame_h, self.frame_w, 3) if self._pix[0] == L.PIX_BGR24 else (self.frame_h * 3 // 2, self.frame_w)

    def read_frames(self, slot, count):
        """Ring slots [slot, slot + count) as BGR uint8 [count, H, W, 3], between calls (what the frames that arrived as YUV were
        unpacked to)."""
        out = np.empty((int(count), self.frame_h, self.frame_w, 3), np.uint8)
        L.call("aic_pipeline_read_frames", self._h, int(slot), int(count), L.ptr(out))
        return out

    @classmethod
    def botsort_bank(cls, yolo_engine, reid_engine, frame_hw, cameras, gmc=0, **kw):
        """A BoT-SORT pipeline for `cameras` cameras (aic_pipeline_create_botsort_bank): the tracker is a bank of that many streams, fixed
        here because the smoothed features and the camera-motion estimator (gmc=2 or 4: a bank as well) are sized by it.  The other
        arguments are those of tracker="botsort"; the ring and every run range are tick-major as with streams=S, batch and
        ring_frames are multiples of `cameras`, reset_stream(s) works and `.streams` is the camera count."""
        cameras = int(cameras)
        if not 1 <= cameras <= 256:
            raise ValueError("cameras must be in 1..256")
        if "tracker" in kw or "streams" in kw:
            raise TypeError("botsort_bank fixes tracker and streams itself")
        batch = int(kw.get("batch", 8))
        if batch % cameras or int(kw.get("ring_frames") or 4 * batch) % cameras:
            raise ValueError("batch and ring_frames must be multiples of cameras")
        return cls(yolo_engine, reid_engine, frame_hw, tracker="botsort", gmc=gmc, _cameras=cameras, **kw)

    @classmethod
    def deepsort_bank(cls, yolo_engine, reid_engine, frame_hw, cameras, **kw):
        """A DeepSORT pipeline for `cameras` cameras (aic_pipeline_create_deepsort_bank): the tracker is a DeepSORT bank of that many
        streams (deepsort_bank.py: device association only, nn_budget > 0, max_tracks <= 512), fed from HBM -- boxes and embeddings are
        never copied for it.  The other arguments are those of a DeepSORT pipeline; the ring and every run range are tick-major as with
        streams=S, batch and ring_frames are multiples of `cameras`, reset_stream(s), link_cameras() and global_ids() work, `.bank`
        exports the cameras' tracks and galleries and `.streams` is the camera count.  A camera that exhausts max_tracks fails the run
        call (AicError, ERR_CAPACITY) and every later one until reset_stream(camera)."""
        cameras = int(cameras)
        if not 1 <= cameras <= 256:
            raise ValueError("cameras must be in 1..256")
        if "tracker" in kw or "streams" in kw:
            raise TypeError("deepsort_bank fixes tracker and streams itself")
        batch = int(kw.get("batch", 8))
        if batch % cameras or int(kw.get("ring_frames") or 4 * batch) % cameras:
            raise ValueError("batch and ring_frames must be multiples of cameras")
        return cls(yolo_engine, reid_engine, frame_hw, tracker="deepsort", _cameras=cameras, **kw)

    @property
    def bank(self):
        """deepsort_bank pipelines: the pipeline's DeepSORTBank (borrowed: export, export_gallery, counters, option), between run calls."""
        if self.tracker_kind != "deepsort" or not self.cameras:
            raise ValueError("bank needs a TrackingPipeline.deepsort_bank pipeline")
        if self._bank is None:
            from .deepsort_bank import DeepSORTBank
            h = C.c_void_p()
            L.call("aic_pipeline_deepsort_bank", self._h, C.byref(h))
            self._bank = DeepSORTBank._borrow(h, self.tracker_params, self.streams, self._device, int(self.reid.out_dim))
        return self._bank

    def reset_stream(self, s):
        """streams=S, botsort_bank and deepsort_bank pipelines, between run calls: stream s as after creation (a camera reconnecting).  An attached
        CrossCamera forgets the stream's identities with it."""
        L.call("aic_pipeline_reset_stream", self._h, int(s))
        if self.xcam is not None:
            self.xcam.forget_stream(s)

    archive = None

    def link_cameras(self, xcam=None, archive=None):
        """botsort_bank and deepsort_bank pipelines, between run calls: one cross-camera pass over the bank's activated / confirmed tracks
        (xcam.py).  The first call creates and keeps a CrossCamera unless one is handed over (a DeepSORT bank links within its
        max_cosine_distance); returns the identities merged by this call.  archive: an IdentityArchive (archive.py) the pass searches
        for returning people and deposits its rows in; it stays attached."""
        if self.tracker_kind not in ("botsort", "deepsort") or not self.cameras:
            raise ValueError("link_cameras needs a TrackingPipeline.botsort_bank or deepsort_bank pipeline")
        from .xcam import CrossCamera
        if xcam is not None:
            self.xcam = xcam
        if self.xcam is None and self.tracker_kind == "deepsort":
            p = self.tracker_params
            self.xcam = CrossCamera(self.streams, p.max_tracks or 512, int(self.reid.out_dim), p.max_cosine_distance, device=self._device)
        if self.xcam is None:
            p = self.botsort_params
            self.xcam = CrossCamera(self.streams, p.max_tracks or 512, p.feature_dim or 512, device=self._device)
        if archive is not None:
            self.archive = archive
        if self.archive is not None and self.xcam.archive is not self.archive:
            self.xcam.attach_archive(self.archive)
        return self.xcam.link_pipeline(self)

    def global_ids(self, stream, track_ids):
        """int64 global ids of the stream's local track ids after link_cameras(); -1 = not seen in a pass yet."""
        if self.xcam is None:
            raise RuntimeError("link_cameras() has not run yet")
        return self.xcam.global_ids(stream, track_ids)

    _zones = zone_result = zone_events = zone_occupancy = None

    def attach_zones(self, counter):
        """A ZoneCounter (zones.py) of `.streams` streams: after every run* call the call's tracks -- all frames, all streams, ONE
        counter.update -- go through it, and zone_events ([stream][frame] -> event rows), zone_occupancy ([stream] -> [frames, 32]),
        zone_result (the flat ZoneResult) and zone_counters() describe that call.  The rows are the run call's host outputs (the
        kernels read them from a staging upload, not from the tracker's HBM); the tracks returned are untouched.  None detaches."""
        if counter is not None and counter.streams != self.streams:
            raise ValueError(f"a counter of {counter.streams} streams for a pipeline of {self.streams}")
        self._zones = counter
        self.zone_result = self.zone_events = self.zone_occupancy = None

    def zone_counters(self):
        """[stream] -> dict(zone_in, zone_out, line_pos, line_neg) of the attached counter."""
        if self._zones is None:
            raise RuntimeError("attach_zones() has not run yet")
        return [self._zones.counters(s) for s in range(self.streams)]

    def _feed_stages(self, nt, rows, slot=0, host_frames=None):
        """What every run hands the attached analytics stages, in this order."""
        self._feed_zones(nt, rows)
        self._feed_best_shots(nt, rows, slot, host_frames)
        self._feed_scene(nt, rows, slot, host_frames)
        self._feed_left(nt, rows, slot, host_frames)
        self._feed_colours(nt, rows, slot, host_frames)
        self._feed_heat(nt, rows)
        self._feed_proximity(nt, rows)

    def _feed_zones(self, nt, rows, cap_events=256):
        """nt [count], rows [count, max_persons, 6] of a run call, tick-major (frame i is tick i // streams of stream i % streams)."""
        z = self._zones
        if z is None:
            return
        S, mp = self.streams, rows.shape[1]
        res = z.update([[rows[i, :min(int(nt[i]), mp)] for i in range(s, len(nt), S)] for s in range(S)], cap_events=cap_events)
        self.zone_result, self.zone_events = res, z.event_lists(res)
        off = np.concatenate([[0], np.cumsum(res.frames_per_stream)])
        self.zone_occupancy = [res.occupancy[off[s]:off[s + 1]] for s in range(S)]

    _best_shots = best_shot_result = None
    best_shot_cap = 16

    def attach_best_shots(self, best_shots, cap=16):
        """A BestShots (bestshot.py) of `.streams` streams for this frame size: after every run* call the call's frames and tracks -- all
        ticks, all streams, ONE best_shots.update -- go through it and best_shot_result is that call's BestShotResult (at most `cap`
        finals per stream per call; the rest wait, see .pending and best_shots.drain()).  Frames and rows reach the stage from the
        host side: the host array of run*_from_host (a YUV format converted with frames.to_bgr, the arithmetic of the pipeline's own
        unpack), read_frames(slot, count) for run / run_raw; with *_passes it sees the last pass only.  The tracks returned are
        untouched.  None detaches."""
        if best_shots is not None and (best_shots.streams != self.streams or (best_shots.frame_h, best_shots.frame_w) != (self.frame_h, self.frame_w)):
            raise ValueError(f"best shots of {best_shots.streams} streams of {best_shots.frame_h}x{best_shots.frame_w} for a pipeline of "
                             f"{self.streams} of {self.frame_h}x{self.frame_w}")
        self._best_shots, self.best_shot_cap, self.best_shot_result = best_shots, int(cap), None

    def _feed_best_shots(self, nt, rows, slot=0, host_frames=None):
        """nt [count], rows [count, max_persons, 6] of a run call, tick-major; host_frames: what a *_from_host call was handed."""
        b = self._best_shots
        if b is None:
            return
        S, mp, count = self.streams, rows.shape[1], len(nt)
        self.best_shot_result = b.update(self._host_bgr(slot, count, host_frames),
                                         [[rows[t * S + s, :min(int(nt[t * S + s]), mp)] for s in range(S)] for t in range(count // S)],
                                         cap=self.best_shot_cap)

    def _host_bgr(self, slot, count, host_frames):
        """The BGR frames of a run call on the host, [ticks, streams, H, W, 3]: the array a *_from_host call was handed (a YUV format
        converted with frames.to_bgr), else the ring read back."""
        if host_frames is None:
            bgr = self.read_frames(slot, count)
        elif self._pix[0] != L.PIX_BGR24:
            bgr = frames.to_bgr(host_frames, self._pix[0], matrix=self._pix[1], range=self._pix[2], device=config.resolve_device(self._device))
        else:
            bgr = host_frames
        return bgr.reshape(count // self.streams, self.streams, self.frame_h, self.frame_w, 3)

    _scene_watch = scene_result = None

    def attach_scene_watch(self, scene_watch):
        """A SceneWatch (scene.py) of `.streams` streams for this frame size: after every run* call the call's frames and tracks -- all
        ticks, all streams, ONE scene_watch.update -- go through it and scene_result is that call's SceneResult (records, row_motion
        per track row; no masks).  Frames and rows reach the stage from the host side, exactly as for attach_best_shots; with *_passes
        it sees the last pass only.  The tracks returned are untouched, and the detector still runs on idle cameras: `.active` is what
        a later change will read.  None detaches."""
        w = scene_watch
        if w is not None and (w.streams != self.streams or (w.frame_h, w.frame_w) != (self.frame_h, self.frame_w)):
            raise ValueError(f"a scene watch of {w.streams} streams of {w.frame_h}x{w.frame_w} for a pipeline of "
                             f"{self.streams} of {self.frame_h}x{self.frame_w}")
        self._scene_watch, self.scene_result = w, None

    def _feed_scene(self, nt, rows, slot=0, host_frames=None):
        """nt [count], rows [count, max_persons, 6] of a run call, tick-major; host_frames: what a *_from_host call was handed."""
        w = self._scene_watch
        if w is None:
            return
        S, mp, count = self.streams, rows.shape[1], len(nt)
        self.scene_result = w.update(self._host_bgr(slot, count, host_frames),
                                     [[rows[t * S + s, :min(int(nt[t * S + s]), mp)] for s in range(S)] for t in range(count // S)])

    _left_objects = left_result = None
    left_cap_events = 256

    def attach_left_objects(self, left_objects, cap_events=256):
        """A LeftObjects (leftobj.py) of `.streams` streams for this frame size: after every run* call the call's frames and tracks --
        all ticks, all streams, ONE left_objects.update -- go through it and left_result is that call's LeftResult (records, objects,
        at most `cap_events` events; no masks).  Frames and rows reach the stage from the host side, exactly as for attach_scene_watch;
        with *_passes it sees the last pass only.  The tracks returned are untouched.  None detaches."""
        w = left_objects
        if w is not None and (w.streams != self.streams or (w.frame_h, w.frame_w) != (self.frame_h, self.frame_w)):
            raise ValueError(f"left objects of {w.streams} streams of {w.frame_h}x{w.frame_w} for a pipeline of "
                             f"{self.streams} of {self.frame_h}x{self.frame_w}")
        self._left_objects, self.left_cap_events, self.left_result = w, int(cap_events), None

    def _feed_left(self, nt, rows, slot=0, host_frames=None):
        """nt [count], rows [count, max_persons, 6] of a run call, tick-major; host_frames: what a *_from_host call was handed."""
        w = self._left_objects
        if w is None:
            return
        S, mp, count = self.streams, rows.shape[1], len(nt)
        self.left_result = w.update(self._host_bgr(slot, count, host_frames),
                                    [[rows[t * S + s, :min(int(nt[t * S + s]), mp)] for s in range(S)] for t in range(count // S)],
                                    cap_events=self.left_cap_events)

    _colours = colour_result = None
    colour_cap = 16

    def attach_colours(self, stage, cap=16):
        """A TrackColours (colours.py) of `.streams` streams for this frame size: after every run* call the call's frames and tracks --
        all ticks, all streams, ONE stage.update -- go through it and colour_result is that call's ColourResult (row_tags per track
        row, at most `cap` ended tracks per stream per call; the rest wait, see .pending and stage.drain()).  Frames and rows reach the
        stage from the host side, exactly as for attach_best_shots; with *_passes it sees the last pass only.  The tracks returned are
        untouched.  None detaches."""
        w = stage
        if w is not None and (w.streams != self.streams or (w.frame_h, w.frame_w) != (self.frame_h, self.frame_w)):
            raise ValueError(f"track colours of {w.streams} streams of {w.frame_h}x{w.frame_w} for a pipeline of "
                             f"{self.streams} of {self.frame_h}x{self.frame_w}")
        self._colours, self.colour_cap, self.colour_result = w, int(cap), None

    def _feed_colours(self, nt, rows, slot=0, host_frames=None):
        """nt [count], rows [count, max_persons, 6] of a run call, tick-major; host_frames: what a *_from_host call was handed."""
        w = self._colours
        if w is None:
            return
        S, mp, count = self.streams, rows.shape[1], len(nt)
        self.colour_result = w.update(self._host_bgr(slot, count, host_frames),
                                      [[rows[t * S + s, :min(int(nt[t * S + s]), mp)] for s in range(S)] for t in range(count // S)],
                                      cap=self.colour_cap)

    _heat = heat_result = None
    heat_cap = 16

    def attach_heat_maps(self, stage, cap=16):
        """A HeatMaps (heatmap.py) of `.streams` streams for this frame size: after every run* call the call's tracks -- all ticks, all
        streams, ONE stage.update -- go through it and heat_result is that call's HeatResult (row_tags per track row, at most `cap`
        ended tracks per stream per call; the rest wait, see .pending and stage.drain()); stage.layers() / stage.render() show what
        has accumulated.  The stage reads rows only: they reach it from the host side, as for attach_colours; with *_passes it sees the
        last pass only.  The tracks returned are untouched.  None detaches."""
        w = stage
        if w is not None and (w.streams != self.streams or (w.frame_h, w.frame_w) != (self.frame_h, self.frame_w)):
            raise ValueError(f"heat maps of {w.streams} streams of {w.frame_h}x{w.frame_w} for a pipeline of "
                             f"{self.streams} of {self.frame_h}x{self.frame_w}")
        self._heat, self.heat_cap, self.heat_result = w, int(cap), None

    def _feed_heat(self, nt, rows):
        """nt [count], rows [count, max_persons, 6] of a run call, tick-major."""
        w = self._heat
        if w is None:
            return
        S, mp, count = self.streams, rows.shape[1], len(nt)
        self.heat_result = w.update([[rows[t * S + s, :min(int(nt[t * S + s]), mp)] for s in range(S)] for t in range(count // S)], cap=self.heat_cap)

    _prox = proximity_result = None
    proximity_cap, proximity_cap_pairs = 16, 64

    def attach_proximity(self, stage, cap=16, cap_pairs=64):
        """A Proximity (proximity.py) of `.streams` streams for this frame size: after every run* call the call's tracks -- all ticks, all
        streams, ONE stage.update -- go through it and proximity_result is that call's ProximityResult (records, row tags per track row,
        at most `cap_pairs` pair events per frame and `cap` ended tracks per stream per call; the rest wait, see .pending and
        stage.drain()).  The stage reads rows only: they reach it from the host side, as for attach_heat_maps; with *_passes it sees the
        last pass only.  The tracks returned are untouched.  None detaches."""
        w = stage
        if w is not None and (w.streams != self.streams or (w.frame_h, w.frame_w) != (self.frame_h, self.frame_w)):
            raise ValueError(f"proximity of {w.streams} streams of {w.frame_h}x{w.frame_w} for a pipeline of "
                             f"{self.streams} of {self.frame_h}x{self.frame_w}")
        self._prox, self.proximity_cap, self.proximity_cap_pairs, self.proximity_result = w, int(cap), int(cap_pairs), None

    def _feed_proximity(self, nt, rows):
        """nt [count], rows [count, max_persons, 6] of a run call, tick-major."""
        w = self._prox
        if w is None:
            return
        S, mp, count = self.streams, rows.shape[1], len(nt)
        self.proximity_result = w.update([[rows[t * S + s, :min(int(nt[t * S + s]), mp)] for s in range(S)] for t in range(count // S)],
                                         cap=self.proximity_cap, cap_pairs=self.proximity_cap_pairs)

    def close(self):
        for b in getattr(self, "_staging", []):
            try:
                self.unpin(b)
            except Exception:
                pass
        self._staging = []
        if getattr(self, "_bank", None) is not None:
            self._bank.close()                                   # borrowed: forgets the handle, destroys nothing
            self._bank = None
        if getattr(self, "_h", None):
            L.call("aic_pipeline_destroy", self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def group_warps(self):
        """float32 [frames, 2, 3]: the camera-motion warps of the most recently finished launch group (gmc pipelines)."""
        n = C.c_int32()
        L.call("aic_pipeline_group_warps", self._h, None, 0, C.byref(n))
        w = np.zeros((n.value, 2, 3), np.float32)
        L.call("aic_pipeline_group_warps", self._h, L.ptr(w), n.value, C.byref(n))
        return w

    def upload(self, slot, frames_bgr):
        f = np.ascontiguousarray(frames_bgr, dtype=np.uint8)
        if f.ndim == len(self.host_frame_shape):
            f = f[None]
        assert f.shape[1:] == self.host_frame_shape, f.shape
        L.call("aic_pipeline_upload", self._h, int(slot), L.ptr(f), len(f))

    def upload_jpeg(self, slot, files):
        """Decode JPEG files (a list of bytes, or a (buffer, offsets) pair as jpegdec.pack makes it; the buffer in host or device memory)
        straight into ring slots [slot, slot + n): the counterpart of upload for frames that arrive compressed (BGR24 pipelines only;
        every picture must have the pipeline's frame size).  Returns (status [n], reason [n]): a refused file leaves its slot as it
        was, its neighbours are unaffected."""
        from . import jpegdec as J
        buf, off = files if isinstance(files, tuple) else J.pack(files)
        off = np.ascontiguousarray(off, dtype=np.int64)
        n = off.size - 1
        if isinstance(buf, np.ndarray):
            buf = np.ascontiguousarray(buf, dtype=np.uint8)
            ptr, mem = (L.ptr(buf) if buf.size else None), L.HOST
        else:
            if buf.is_cuda:
                import torch
                torch.cuda.current_stream(buf.device).synchronize()           # the library reads it on its own stream
            ptr, mem = C.c_void_p(buf.data_ptr()), L.DEVICE if buf.is_cuda else L.HOST
        status, reason = np.zeros(n, np.int32), np.zeros(n, np.int32)
        L.call("aic_pipeline_upload_jpeg", self._h, int(slot), ptr, mem, L.ptr(off), n, L.ptr(status), L.ptr(reason))
        return status, reason

    def run_from_jpeg(self, files, slot=0, want_dets=False):
        """upload_jpeg, then run over the same slots: (tracks, dets, status, reason)."""
        status, reason = self.upload_jpeg(slot, files)
        tracks, dets = self.run(slot, len(status), want_dets)
        return tracks, dets, status, reason

    def inject(self, slot, detections):
        """detections: list (one per frame) of (boxes_xyxy [n,4], conf [n], class_ids [n])."""
        k, mp = len(detections), self.max_persons
        counts = np.zeros(k, np.int32)
        boxes, conf, cls = np.zeros((k, mp, 4), np.float32), np.zeros((k, mp), np.float32), np.zeros((k, mp), np.int32)
        for f, (b, c, ids) in enumerate(detections):
            n = len(b)
            counts[f] = n
            boxes[f, :n], conf[f, :n], cls[f, :n] = b, c, ids
        L.call("aic_pipeline_inject", self._h, int(slot), k, L.ptr(counts), L.ptr(boxes), L.ptr(conf), L.ptr(cls))

    def run(self, slot, count, want_dets=False):
        """Process ring slots [slot, slot+count): returns (tracks, dets); tracks[f] is the list of
        (x1, y1, x2, y2, track_id, class_name, conf) tuples of deepsort_tracker.py:126-141."""
        mp, md = self.max_persons, self.max_det
        nt = np.zeros(count, np.int32)
        rows, tconf = np.zeros((count, mp, 6), np.int32), np.zeros((count, mp), np.float32)
        nd = np.zeros(count, np.int32)
        db = np.zeros((count, md, 4), np.float32) if want_dets else None
        ds = np.zeros((count, md), np.float32) if want_dets else None
        dl = np.zeros((count, md), np.int32) if want_dets else None
        L.call("aic_pipeline_run", self._h, int(slot), int(count), L.ptr(nt), L.ptr(rows), L.ptr(tconf), L.ptr(nd),
               L.ptr(db), L.ptr(ds), L.ptr(dl))
        self._feed_stages(nt, rows, slot)
        tracks = [[(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), config.class_name(int(r[5])), float(c))
                   for r, c in zip(rows[f, :nt[f]], tconf[f, :nt[f]])] for f in range(count)]
        dets = None
        if want_dets:
            dets = [(db[f, :nd[f]], ds[f, :nd[f]], dl[f, :nd[f]]) for f in range(count)]
        return tracks, (dets if want_dets else nd)

    def _raw_bufs(self):
        if not hasattr(self, "_raw"):
            mp = self.max_persons
            self._raw = (np.zeros(self.ring_frames, np.int32), np.zeros((self.ring_frames, mp, 6), np.int32),
                         np.zeros((self.ring_frames, mp), np.float32), np.zeros(self.ring_frames, np.int32))
        return self._raw

    def run_raw(self, slot, count):
        """Timed path of bench.py: no Python-side unpacking, outputs stay in preallocated arrays."""
        nt, rows, tconf, nd = self._raw_bufs()
        L.call("aic_pipeline_run", self._h, int(slot), int(count), L.ptr(nt), L.ptr(rows), L.ptr(tconf), L.ptr(nd),
               None, None, None)
        self._feed_stages(nt[:count], rows[:count], slot)
        return nt[:count], rows[:count], nd[:count]

    def run_raw_passes(self, slot, count, passes):
        """`passes` consecutive walks over the same ring range as ONE call (a looped clip streamed continuously)."""
        nt, rows, tconf, nd = self._raw_bufs()
        L.call("aic_pipeline_run_passes", self._h, int(slot), int(count), int(passes), L.ptr(nt), L.ptr(rows), L.ptr(tconf), L.ptr(nd))
        self._feed_stages(nt[:count], rows[:count], slot)
        return nt[:count], rows[:count], nd[:count]

    def stats(self, reset=False):
        """Host wall-clock split (seconds) since the last reset: launch-group issue, waiting for the GPU, tracker."""
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        L.call("aic_pipeline_stats", self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n), int(reset))
        return dict(issue_s=a.value, wait_s=b.value, track_s=c.value, frames=n.value)

    def run_raw_from_host(self, frames_bgr, slot=0):
        """PCIe-inclusive timed path: frames (uint8 [n,H,W,3], or [n,H*3/2,W] with a YUV pixel_format; ideally pinned via pin()) stream
        host -> HBM per launch group on a copy stream, overlapped with compute."""
        f = frames_bgr
        assert f.dtype == np.uint8 and f.flags["C_CONTIGUOUS"] and f.shape[1:] == self.host_frame_shape
        count = len(f)
        nt, rows, tconf, nd = self._raw_bufs()
        L.call("aic_pipeline_run_from_host", self._h, L.ptr(f), int(slot), count, L.ptr(nt), L.ptr(rows), L.ptr(tconf), L.ptr(nd))
        self._feed_stages(nt[:count], rows[:count], slot, f)
        return nt[:count], rows[:count], nd[:count]

    def run_raw_from_host_passes(self, frames_bgr, passes, slot=0):
        """The host clip looped `passes` times as ONE continuous stream (bench.py's timed region)."""
        f = frames_bgr
        assert f.dtype == np.uint8 and f.flags["C_CONTIGUOUS"] and f.shape[1:] == self.host_frame_shape
        count = len(f)
        nt, rows, tconf, nd = self._raw_bufs()
        L.call("aic_pipeline_run_from_host_passes", self._h, L.ptr(f), int(slot), count, int(passes), L.ptr(nt), L.ptr(rows), L.ptr(tconf), L.ptr(nd))
        self._feed_stages(nt[:count], rows[:count], slot, f)
        return nt[:count], rows[:count], nd[:count]

    def run_from_host(self, frames_bgr, slot=0):
        """Frames in host memory -> per-frame track tuples (deepsort_tracker.py:126-141), as run() returns them."""
        nt, rows, nd = self.run_raw_from_host(frames_bgr, slot)
        tconf = self._raw_bufs()[2]
        return [[(int(r[0]), int(r[1]), int(r[2]), int(r[3]), int(r[4]), config.class_name(int(r[5])), float(c))
                 for r, c in zip(rows[f, :min(nt[f], self.max_persons)], tconf[f, :min(nt[f], self.max_persons)])] for f in range(len(frames_bgr))]

    def stream(self, frames_iter, read_back=False):
        """Frame source -> (frame, tracks) per frame, in order, through DOUBLE-BUFFERED PAGE-LOCKED STAGING: two buffers of `batch`
        frames are pinned once (never per call); a reader thread fills one from the source (cap.read() of
        src/aicamera_tracker.py:170) while the GPU works on the other, whose frames cross PCIe on the copy stream under compute.
        The yielded frame is a view of the staging buffer: use it before asking for the frame `batch` positions later.
        With a YUV pixel_format the staging buffers and the source's frames are [H*3/2, W]; read_back=True then yields, instead of the
        staged YUV frame, the BGR frame the ring holds for it (read_frames: one device-to-host copy per run call) -- what a consumer that
        draws on the frames needs.  A BGR pipeline ignores read_back."""
        import queue
        import threading
        if not hasattr(self, "_staging"):
            self._staging = [np.empty((self.batch,) + self.host_frame_shape, np.uint8) for _ in range(2)]
            for b in self._staging:
                self.pin(b)
        free, full = queue.Queue(), queue.Queue(maxsize=2)
        free.put(0), free.put(1)
        err = []

        def reader():
            try:
                it = iter(frames_iter)
                done = False
                while not done:
                    b = free.get()
                    n = 0
                    while n < self.batch:
                        try:
                            f = next(it)
                        except StopIteration:
                            done = True
                            break
                        if f.shape != self.host_frame_shape:
                            raise ValueError(f"frame of shape {f.shape}, the pipeline was built for {self.host_frame_shape}")
                        self._staging[b][n] = f
                        n += 1
                    full.put((b, n))
            except Exception as e:      # noqa: BLE001 -- handed to the consumer
                err.append(e)
            full.put((-1, 0))

        th = threading.Thread(target=reader, daemon=True)
        th.start()
        while True:
            b, n = full.get()
            if b < 0:
                break
            if n:
                tracks = self.run_from_host(self._staging[b][:n])
                if self.link_after_run:                  # the CLI's --link_cameras: identities follow every run call
                    self.link_cameras()
                shown = self.read_frames(0, n) if read_back and self._pix[0] != L.PIX_BGR24 else self._staging[b]
                for i in range(n):
                    yield shown[i], tracks[i]
            free.put(b)
        th.join()
        if err:
            raise err[0]

    def group_times(self):
        """Launch groups of the last call: (frames [G], latency seconds [G]) -- handed to the pipeline -> tuples on the host."""
        n = C.c_int32()
        L.call("aic_pipeline_group_times", self._h, None, None, None, 0, C.byref(n))
        fr, a, b = np.zeros(n.value, np.int32), np.zeros(n.value, np.float64), np.zeros(n.value, np.float64)
        L.call("aic_pipeline_group_times", self._h, L.ptr(fr), L.ptr(a), L.ptr(b), max(n.value, 1), C.byref(n))
        return fr, b - a

    @staticmethod
    def pin(array):
        """Page-lock a NumPy buffer (hipHostRegister) so H2D runs at PCIe rate and truly asynchronously."""
        L.call("aic_host_register", L.ptr(array), array.nbytes)
        return array

    @staticmethod
    def unpin(array):
        L.call("aic_host_unregister", L.ptr(array))

    def option(self, key, value):
        """Runtime option of the C pipeline (aic_pipeline_option): e.g. option("taper", 0) = full launch groups only."""
        L.call("aic_pipeline_option", self._h, str(key).encode(), int(value))

    def counters(self):
        a, b = C.c_int64(), C.c_int64()
        L.call("aic_pipeline_counters", self._h, C.byref(a), C.byref(b))
        d, h = C.c_int64(), C.c_int64()
        L.call("aic_pipeline_assoc_frames", self._h, C.byref(d), C.byref(h))
        fd, fh, fo = C.c_int64(), C.c_int64(), C.c_int64()
        L.call("aic_pipeline_filter_counters", self._h, C.byref(fd), C.byref(fh), C.byref(fo))
        l1 = C.c_int64()
        L.call("aic_pipeline_lane_groups", self._h, C.byref(l1))
        return dict(grown_groups=a.value, clipped_frames=b.value, assoc_device_frames=d.value, assoc_host_frames=h.value,
                    filter_device_groups=fd.value, filter_host_groups=fh.value, reid_overflow_rounds=fo.value, lane1_groups=l1.value)

    def group_embeddings(self):
        """Embeddings of every crop of the most recently finished launch group: (emb [rows, dim], crops_per_frame [frames])."""
        n, f, d = C.c_int32(), C.c_int32(), C.c_int32()
        L.call("aic_pipeline_group_embeddings", self._h, None, 0, None, 0, C.byref(n), C.byref(f), C.byref(d))
        emb, per = np.zeros((n.value, d.value), np.float32), np.zeros(f.value, np.int32)
        L.call("aic_pipeline_group_embeddings", self._h, L.ptr(emb), max(n.value, 1), L.ptr(per), max(f.value, 1),
               C.byref(n), C.byref(f), C.byref(d))
        return emb, per

    def last_embeddings(self):
        n, d = C.c_int32(), C.c_int32()
        L.call("aic_pipeline_last_embeddings", self._h, None, 1 << 30, C.byref(n), C.byref(d))
        out = np.zeros((n.value, d.value), np.float32)
        L.call("aic_pipeline_last_embeddings", self._h, L.ptr(out), max(n.value, 1), C.byref(n), C.byref(d))
        return out
