"""Command line with the flags of the reference's src/aicamera_tracker.py:20-67.

Frame sources (`--input`; the step BEFORE the path):
    a video file / no --input = webcam `--webcam_id`   cv2.VideoCapture, exactly as the reference (aicamera_tracker.py:113-135),
                                                        WHEN cv2 is importable (probed at start; it is not in this image)
    synthetic:WxH:persons:frames[:seed]                 the seeded scene of ai-camera_amd/synthetic.py
    path/to/frames.npy                                  uint8 [T,H,W,3] BGR (memory-mapped)
    raw:WxH:path                                        headerless BGR24 frames (memory-mapped), e.g. `ffmpeg -pix_fmt bgr24 -f rawvideo`;
                                                        with `--pixel_format nv12|i420` (`--yuv_matrix`, `--yuv_range`) tightly packed 4:2:0
                                                        frames, memory-mapped as [T, H*3/2, W] (`ffmpeg -pix_fmt nv12 -f rawvideo`)
    path/to/clip.mjpeg                                  JFIF files back to back (what `--output_codec mjpeg` writes, what cameras send),
                                                        decoded on the device, 16 files per call; a file the
                                                        decoder refuses prints a line and the previous frame takes its place
The loop body is the reference's (detect -> tracker update, timed the same way, aicamera_tracker.py:175,201-207).  `--batch N`
(N > 1, not a reference flag) runs the same loop through the batched pipeline with double-buffered page-locked staging
(TrackingPipeline.stream) instead of one synchronous call pair per frame.

Outputs (the step AFTER the path, §8(f)-3): tracks + info panel are drawn on every frame by the overlay kernel
(ai-camera_amd/visualization.py).  Unless `--no_save`: an annotated video through cv2.VideoWriter when cv2 is there
(aicamera_tracker.py:140-161), else annotated BGR24 frames appended to `<name>_tracked_<time>.bgr24` (+ `.json` with size / fps);
the tracks always go to a `.jsonl` next to it.  `--show_display` needs cv2 (imshow); without it the flag is accepted and ignored.
With `--inputs` the S frames of a tick and their tracks go through ONE `render.Renderer` call; `--redact
{off,box,head}`, `--redact_style mosaic:16|...|fill`, `--masks FILE.json` and `--draw_zones` (with `--zones`) pixelate or fill the tracked
objects, black out fixed regions and draw the zones, with `--input` as well; with none of them the written pixels are the overlay's.
`--best_shots DIR [--best_shot_size WxH] [--best_shot_region box|head]`: the best crop of every track, kept on the
device from the frames as ingested (before any `--redact`), written as `DIR/cam<S>_id<ID>_f<best_frame>.ppm` with a line in
`DIR/index.jsonl` when the track ends and, for the tracks still alive, at the end of the run.
`--left_objects [--left_cell {4,8,16}] [--left_after TICKS]`: abandoned and removed objects per camera.  Every
JSON line gains `"left_objects": [{uid, kind, box, owner, age}]` for the alarmed objects, every event (appeared, raised, ended) is
printed as a line of its own, and the output stage of --redact / --masks / --draw_zones draws them.
`--colours [--colours_file FILE.jsonl]`: what each track wears.  Every JSON line gains `"colours"`, one
`[upper, lower]` pair of colour names (or null) per track of the line; every ended track is appended to FILE as one JSON object with
its histograms, and the tracks still alive at the end of the run are flushed into it.
`--heat_maps DIR [--heat_cell {4,8,16,32}] [--heat_layer NAME] [--heat_paths FILE.jsonl] [--heat_overlay]`: where
people go.  At the end of the run each camera's twelve layers are written as `DIR/cam<S>_layers.npy` ([12, GH, GW] int32, the order of
heatmap.LAYERS) and the chosen layer (default dwell) over the camera's last frame as `DIR/cam<S>_<layer>.jpg`; `--heat_paths` appends
one JSON line per ended track (start, end, path length, cells, ...); `--heat_overlay` blends the layer into every saved frame before
boxes and labels are drawn.
`--proximity [--ground FILE.json] [--near N] [--proximity_file FILE.jsonl]`: who is with whom and how fast.  Every
JSON line gains `"parties"` (lists of track ids, parties of two or more first), `"units"` (parties + singles) and `"speed"`, one q8 value
per track of the line (-1 before the first measurement); every LINK / UNLINK of a pair is printed as a line of its own.  `--ground` holds
per camera `{"H": [9 ints], "shift": s}` or `{"pixels": [...], "ground": [...]}` (through proximity.homography) and selects the
ground-plane metric, `--near` is then in ground units; `--proximity_file` appends one JSON line per ended track.
`--scene_watch [--scene_cell {4,8,16}]`: a background model per camera on a coarse gray grid.  Every JSON line
gains `"scene": {active, moving_cells, motion_box, alarms}` and `"moving"`, one value per track of the line (256 = every cell under its
box moves, -1 = the box is off the frame); every alarm edge (dark, bright, defocus, scene, frozen) is printed as a line of its own.

Pixel formats: with `--batch N` (and `--inputs`) YUV frames cross PCIe as they are and the pipeline unpacks them
into its BGR ring on the device; frames that are saved or shown come back through TrackingPipeline.read_frames.  With `--batch 1` each
frame goes through frames.to_bgr before the plugin classes, whose signatures stay BGR.  `--output_pixel_format nv12` makes the headerless
writer append NV12 frames (`.nv12`, converted by frames.from_bgr after rendering) -- what an encoder takes.
`--output_codec mjpeg [--jpeg_quality N] [--jpeg_restart N]` encodes the annotated frames on the device instead and
appends them as JFIF files to `<name>.mjpeg` (+ `.json` with every frame's byte offset); `--best_shot_format jpg` writes the best shots
as `.jpg` (4:4:4 at `--jpeg_quality`).
"""
from __future__ import annotations

import argparse
import json
import time
from pathlib import Path

import numpy as np

from . import config, synthetic, visualization
from . import frames as pixfmt
from .detector import YOLODetector
from .deepsort_tracker import DeepSORT


HEAT_LAYERS = ("visits", "dwell", "starts", "ends", "dir0", "dir1", "dir2", "dir3", "dir4", "dir5", "dir6", "dir7")      # heatmap.LAYERS


def probe_cv2():
    try:
        import cv2   # noqa: PLC0415
        return cv2
    except Exception:   # noqa: BLE001 -- absent or broken: the codec-free sources still work
        return None


def parse_arguments(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description="AICamera: Real-time Object Detection & Tracking (MI355X engine)")
    p.add_argument("--input", type=str, default=None, help="video file (cv2), synthetic:WxH:persons:frames[:seed], frames.npy, raw:WxH:path or clip.mjpeg (decoded on the device)")
    p.add_argument("--inputs", type=str, default=None,
                   help="comma-separated sources of one frame size (as --input), --tracker bytetrack|ocsort|botsort|deepsort_bank only: one pipeline with one tracker "
                        "stream per source; the shortest source ends the run, one output per stream (suffix _s<k>)")
    p.add_argument("--webcam_id", type=int, default=0, help="webcam used when no --input is given (cv2)")
    p.add_argument("--output_dir", type=str, default="outputs")
    p.add_argument("--output_filename", type=str, default=None)
    p.add_argument("--show_display", action="store_true", help="cv2.imshow when cv2 is importable")
    p.add_argument("--no_save", action="store_true")
    p.add_argument("--yolo_engine", type=str, default=str(config.YOLO_ENGINE_PATH))
    p.add_argument("--reid_engine", type=str, default=str(config.REID_ENGINE_PATH))
    p.add_argument("--conf_thresh", type=float, default=None,
                   help=f"detector score floor (default {config.YOLO_CONF_THRESHOLD}; with --tracker bytetrack its low_thresh 0.1, with ocsort its det_thresh 0.6, with botsort its track_low_thresh 0.1)")
    p.add_argument("--tracker", type=str, default="deepsort", choices=("deepsort", "bytetrack", "ocsort", "botsort", "deepsort_bank"),
                   help="bytetrack / ocsort: no ReID model, the tracker's association on the device; botsort: IoU + ReID fusion on the device; "
                        "deepsort_bank (with --inputs): DeepSORT for every source, one bank on the device")
    p.add_argument("--gmc", type=int, default=0, choices=(0, 2, 4),
                   help="botsort only: estimate the camera motion on the device at this downscale and warp the predicted tracks (0 = off)")
    p.add_argument("--link_cameras", action="store_true",
                   help="--inputs with --tracker botsort or deepsort_bank only: link the cameras' identities on the device after every run call; every JSON line "
                        "gains \"global_ids\" parallel to \"tracks\" (-1 = not linked yet) and the overlay label shows the global id")
    p.add_argument("--archive", type=int, default=0, metavar="CAPACITY",
                   help="with --link_cameras: keep up to CAPACITY appearance rows of past tracks on the device; a person who comes back, on any "
                        "camera, gets the identity they had, and every JSON line gains \"returning\": [[track id, archived key, distance], ...]")
    p.add_argument("--archive_file", type=str, default=None, help="with --archive: load the archive from this .npz at the start if it exists, save it at the end")
    p.add_argument("--archive_min_gap", type=int, default=1, help="with --archive: link passes a row must have been gone for before it counts as returning")
    p.add_argument("--zones", type=str, default=None,
                   help="JSON file {\"cameras\": [{\"zones\": [[[x, y], ...], ...], \"lines\": [[[x, y], [x, y]], ...]}, ...]} in integer pixels, one entry per "
                        "source (a single entry serves every source): zone entries, dwell and line crossings are counted on the device and every "
                        "JSON line gains \"zones\": {occupancy, zone_in, zone_out, line_pos, line_neg, events}")
    p.add_argument("--best_shots", type=str, default=None, metavar="DIR",
                   help="keep the best crop of every track on the device (the sharpest, largest, least occluded one seen while it lived) and "
                        "write it when the track ends, and at the end of the run, as DIR/cam<S>_id<ID>_f<best_frame>.ppm with one line per "
                        "file in DIR/index.jsonl; the crops come from the frames as ingested, before any --redact")
    p.add_argument("--best_shot_size", type=str, default="64x128", metavar="WxH", help="with --best_shots: thumbnail size, multiples of 8 in 16..128 x 16..256")
    p.add_argument("--best_shot_region", type=str, default="box", choices=("box", "head"), help="with --best_shots: the whole box or its head (the top quarter)")
    p.add_argument("--best_shot_format", type=str, default="ppm", choices=("ppm", "jpg"),
                   help="with --best_shots: ppm (raw P6) or jpg (JFIF, 4:4:4 at --jpeg_quality, encoded on the device)")
    p.add_argument("--scene_watch", action="store_true",
                   help="watch every camera's scene on the device: every JSON line gains \"scene\": {active, moving_cells, motion_box, alarms} "
                        "and \"moving\" (per track, 0..256), and every alarm edge (dark, bright, defocus, scene, frozen) is printed as its own line")
    p.add_argument("--scene_cell", type=int, default=None, choices=(4, 8, 16), help="with --scene_watch: the grid's cell size in pixels (default 8)")
    p.add_argument("--left_objects", action="store_true",
                   help="report abandoned and removed objects on the device: every JSON line gains \"left_objects\": [{uid, kind, box, owner, age}] "
                        "for the alarmed ones, and every event (appeared, raised, ended) is printed as its own line")
    p.add_argument("--left_cell", type=int, default=None, choices=(4, 8, 16), help="with --left_objects: the grid's cell size in pixels (default 8)")
    p.add_argument("--left_after", type=int, default=None, metavar="TICKS",
                   help="with --left_objects: frames a change must rest before it is a candidate (min_ticks, default 50)")
    p.add_argument("--colours", action="store_true",
                   help="name what every track wears on the device: every JSON line gains \"colours\": one [upper, lower] pair of colour names "
                        "(or null) per track")
    p.add_argument("--colours_file", type=str, default=None, metavar="FILE.jsonl",
                   help="with --colours: append every ended track's descriptor (names, histograms) to FILE as one JSON object")
    p.add_argument("--heat_maps", type=str, default=None, metavar="DIR",
                   help="accumulate footfall, dwell, flow and start / end maps per camera on the device; at the end of the run write every "
                        "camera's layers as DIR/cam<S>_layers.npy and one layer over its last frame as DIR/cam<S>_<layer>.jpg")
    p.add_argument("--heat_cell", type=int, default=None, choices=(4, 8, 16, 32), help="with --heat_maps: the grid's cell size in pixels (default 16)")
    p.add_argument("--heat_layer", type=str, default=None, metavar="NAME",
                   help="with --heat_maps: the layer that is drawn (visits, dwell, starts, ends, dir0..dir7; default dwell)")
    p.add_argument("--heat_paths", type=str, default=None, metavar="FILE.jsonl", help="with --heat_maps: append one JSON line per ended track to FILE")
    p.add_argument("--heat_overlay", action="store_true", help="with --heat_maps: blend the layer into every saved frame, under boxes and labels")
    p.add_argument("--proximity", action="store_true",
                   help="who is with whom and how fast (DESIGN.md section 55): every JSON line gains \"parties\" (lists of track ids, parties of two "
                        "or more first), \"units\" and \"speed\" (one q8 value per track, -1 before the first measurement); every LINK / UNLINK of "
                        "a pair is printed as its own line")
    p.add_argument("--ground", type=str, default=None, metavar="FILE.json",
                   help="with --proximity: per camera {\"H\": [9 ints], \"shift\": s} or {\"pixels\": [[x, y], ..], \"ground\": [[X, Y], ..]} "
                        "(one object, or a list with one per camera); selects the ground-plane metric, --near is then in ground units")
    p.add_argument("--near", type=int, default=None, metavar="N",
                   help="with --proximity: how near is near -- per mille of the mean body height (default 700), or ground units with --ground")
    p.add_argument("--proximity_file", type=str, default=None, metavar="FILE.jsonl", help="with --proximity: append one JSON line per ended track to FILE")
    p.add_argument("--redact", type=str, default="off", choices=("off", "box", "head"),
                   help="privacy redaction of every tracked object on the saved frames: its whole box, or its head (the top quarter)")
    p.add_argument("--redact_style", type=str, default="mosaic:16",
                   help="mosaic:4 | mosaic:8 | mosaic:16 | mosaic:32 (cells of that many pixels, anchored at the frame's origin) or fill (black)")
    p.add_argument("--masks", type=str, default=None,
                   help="JSON file {\"cameras\": [{\"masks\": [[[x, y], ...], ...]}, ...]} in integer pixels, one entry per source (a single "
                        "entry serves every source): the polygons are blacked out on every saved frame")
    p.add_argument("--draw_zones", action="store_true", help="draw the zones and lines of --zones on the saved frames")
    p.add_argument("--device", type=str, default="cuda:0")
    p.add_argument("--dtype", type=str, default="fp16", choices=("fp16", "fp32"))
    p.add_argument("--batch", type=int, default=1, help="> 1: batched pipeline with double-buffered pinned staging")
    p.add_argument("--pixel_format", type=str, default="bgr24", choices=("bgr24", "nv12", "i420"),
                   help="pixel format of raw:WxH:path sources; nv12 / i420: tightly packed 4:2:0 frames of W*H*3/2 bytes, unpacked on the device")
    p.add_argument("--yuv_matrix", type=str, default="bt601", choices=("bt601", "bt709"), help="YUV matrix of --pixel_format / --output_pixel_format")
    p.add_argument("--yuv_range", type=str, default="limited", choices=("limited", "full"), help="YUV range of --pixel_format / --output_pixel_format")
    p.add_argument("--output_pixel_format", type=str, default="bgr24", choices=("bgr24", "nv12"),
                   help="nv12: the annotated frames are appended as NV12 to a headerless <name>.nv12 file (+ .json) instead of BGR24")
    p.add_argument("--output_codec", type=str, default="auto", choices=("auto", "mjpeg"),
                   help="mjpeg: the annotated frames are encoded on the device and appended as JFIF files to <name>.mjpeg (+ .json with the "
                        "byte offset of every frame); auto: a video file when OpenCV is importable, else headerless frames")
    p.add_argument("--jpeg_quality", type=int, default=None, metavar="N", help="with --output_codec mjpeg or --best_shot_format jpg: 1..100 (default 85)")
    p.add_argument("--jpeg_restart", type=int, default=None, metavar="N",
                   help="with --output_codec mjpeg: MCUs per restart interval, 1..65535, or 0 = one MCU row (default)")
    args = p.parse_args(argv)
    if args.best_shot_format != "ppm" and not args.best_shots:
        p.error("--best_shot_format needs --best_shots DIR")
    if args.jpeg_quality is not None and args.output_codec != "mjpeg" and args.best_shot_format != "jpg":
        p.error("--jpeg_quality needs --output_codec mjpeg or --best_shot_format jpg")
    if args.jpeg_restart is not None and args.output_codec != "mjpeg":
        p.error("--jpeg_restart needs --output_codec mjpeg")
    if args.output_codec == "mjpeg" and args.output_pixel_format != "bgr24":
        p.error("--output_codec mjpeg and --output_pixel_format nv12 are mutually exclusive")
    args.jpeg_quality = 85 if args.jpeg_quality is None else args.jpeg_quality
    args.jpeg_restart = 0 if args.jpeg_restart is None else args.jpeg_restart
    if not 1 <= args.jpeg_quality <= 100 or not 0 <= args.jpeg_restart <= 65535:
        p.error("--jpeg_quality is in 1..100, --jpeg_restart in 0..65535")
    if args.pixel_format != "bgr24":
        specs = args.inputs.split(",") if args.inputs is not None else [args.input]
        if not all(spec and spec.startswith("raw:") for spec in specs):
            p.error("--pixel_format nv12 / i420 applies to raw:WxH:path sources only")
    if args.gmc and args.tracker != "botsort":
        p.error("--gmc needs --tracker botsort")
    if args.link_cameras and (args.inputs is None or args.tracker not in ("botsort", "deepsort_bank")):
        p.error("--link_cameras needs --inputs a,b,c --tracker botsort or deepsort_bank")
    if args.archive < 0 or args.archive > (1 << 24) or args.archive_min_gap < 0:
        p.error("--archive CAPACITY is in 1..2^24, --archive_min_gap is >= 0")
    if args.archive and not args.link_cameras:
        p.error("--archive needs --link_cameras")
    if (args.archive_file is not None or args.archive_min_gap != 1) and not args.archive:
        p.error("--archive_file and --archive_min_gap need --archive CAPACITY")
    if args.tracker == "deepsort_bank" and args.inputs is None:
        p.error("--tracker deepsort_bank needs --inputs a,b,c (one source: --tracker deepsort)")
    if args.draw_zones and not args.zones:
        p.error("--draw_zones needs --zones FILE.json")
    if (args.best_shot_size != "64x128" or args.best_shot_region != "box") and not args.best_shots:
        p.error("--best_shot_size and --best_shot_region need --best_shots DIR")
    if args.scene_cell is not None and not args.scene_watch:
        p.error("--scene_cell needs --scene_watch")
    if args.colours_file is not None and not args.colours:
        p.error("--colours_file needs --colours")
    if (args.heat_cell is not None or args.heat_layer is not None or args.heat_paths is not None or args.heat_overlay) and not args.heat_maps:
        p.error("--heat_cell, --heat_layer, --heat_paths and --heat_overlay need --heat_maps DIR")
    if (args.ground is not None or args.near is not None or args.proximity_file is not None) and not args.proximity:
        p.error("--ground, --near and --proximity_file need --proximity")
    if args.near is not None and not 1 <= args.near <= (1 << 24 if args.ground else 4096):
        p.error("--near is 1..4096 per mille of body height, or 1..2^24 ground units with --ground")
    if args.ground is not None and args.near is None:
        p.error("--ground needs --near N, in ground units")
    if args.heat_layer is not None and args.heat_layer not in HEAT_LAYERS:
        p.error("--heat_layer is one of " + ", ".join(HEAT_LAYERS))
    if (args.left_cell is not None or args.left_after is not None) and not args.left_objects:
        p.error("--left_cell and --left_after need --left_objects")
    if args.left_after is not None and not 1 <= args.left_after <= 65534:
        p.error("--left_after must be in 1..65534")
    try:
        args.best_shot_wh = tuple(int(v) for v in args.best_shot_size.lower().split("x"))
        if len(args.best_shot_wh) != 2:
            raise ValueError
    except ValueError:
        p.error("--best_shot_size is WxH, e.g. 64x128")
    if args.inputs is not None:
        if args.input is not None:
            p.error("--inputs and --input are mutually exclusive")
        if args.tracker not in ("bytetrack", "ocsort", "botsort", "deepsort_bank"):
            p.error("--inputs needs --tracker bytetrack, ocsort, botsort or deepsort_bank")
    return args


def raw_frames(path, w, h, pixel_format="bgr24"):
    """The headerless file memory-mapped as uint8 [T, H, W, 3] (bgr24; a trailing partial frame is ignored) or [T, H*3/2, W] (nv12 / i420:
    W and H even, and the file must hold a whole number of frames)."""
    if pixel_format == "bgr24":
        arr = np.memmap(path, np.uint8, "r")
        n = arr.size // (h * w * 3)
        return arr[:n * h * w * 3].reshape(n, h, w, 3)
    if w <= 0 or h <= 0 or w % 2 or h % 2:
        raise SystemExit(f"Error: {pixel_format} frames need an even width and height, not {w}x{h}")
    fb, size = pixfmt.frame_bytes(pixel_format, h, w), Path(path).stat().st_size
    if size == 0 or size % fb:
        raise SystemExit(f"Error: {path} holds {size} bytes, not a whole number of {w}x{h} {pixel_format} frames of {fb} bytes")
    return np.memmap(path, np.uint8, "r").reshape(size // fb, h * 3 // 2, w)


MJPEG_CHUNK = 16          # files per decode call of a .mjpeg source


def mjpeg_source(path, device=0):
    """A Motion-JPEG file (JFIF files back to back, as --output_codec mjpeg writes them) decoded on the device (jpegdec.JpegDecoder,
    DESIGN.md section 43), MJPEG_CHUNK files per call.  A file the decoder refuses prints one line with the reason and the previous
    frame takes its place (black before the first), so the frame count stays the file's."""
    import json
    from . import jpegdec
    if not Path(path).exists():
        raise SystemExit(f"Error: Input video file not found: {path}")
    buf, off = jpegdec.split_mjpeg(path)
    n = off.size - 1
    heads = (jpegdec.probe(buf[off[k]:off[k + 1]]) for k in range(n))
    head = next((h for h in heads if h["status"] == 0), None)
    if head is None:
        raise SystemExit(f"Error: {path} holds no JPEG file this decoder accepts (baseline, 8 bit, gray or YCbCr 4:4:4 / 4:2:2 / 4:2:0)")
    w, h, fps = head["width"], head["height"], float(config.DEFAULT_OUTPUT_FPS)
    side = Path(str(path) + ".json")
    if side.exists():
        fps = float(json.loads(side.read_text()).get("fps", fps))
    name = Path(path).stem

    def frames():
        dec = jpegdec.JpegDecoder(h, w, max_images=MJPEG_CHUNK, device=device)
        prev = np.zeros((h, w, 3), np.uint8)
        for lo in range(0, n, MJPEG_CHUNK):
            hi = min(n, lo + MJPEG_CHUNK)
            bgr, status, reason = dec.decode_packed(buf[off[lo]:off[hi]], off[lo:hi + 1] - off[lo])
            for k in range(hi - lo):
                if status[k]:
                    print(f"{name}: frame {lo + k} refused ({jpegdec.REASONS[reason[k]]}); the previous frame takes its place")
                else:
                    prev = bgr[k]
                yield prev
        dec.close()
    return name, frames(), (w, h, fps)


def frame_source(spec, webcam_id=0, cv2=None, pixel_format="bgr24", device=0):
    """-> (name, frame iterator, (width, height, fps) or None when unknown before the first frame).  pixel_format: of raw: sources, whose
    frames are then [H*3/2, W].  device: where a .mjpeg source is decoded."""
    if spec is not None and spec.endswith(".mjpeg"):
        return mjpeg_source(spec, device)
    if spec is not None and spec.startswith("synthetic:"):
        parts = spec.split(":")
        w, h = (int(v) for v in parts[1].lower().split("x"))
        persons, frames = int(parts[2]), int(parts[3])
        seed = int(parts[4]) if len(parts) > 4 else 0
        sc = synthetic.Scene(seed=seed, n_targets=persons, width=w, height=h)
        return f"synthetic_{w}x{h}_{persons}", (sc.render(f) for f in range(frames)), (w, h, float(config.DEFAULT_OUTPUT_FPS))
    if spec is not None and spec.startswith("raw:"):
        _, size, path = spec.split(":", 2)
        w, h = (int(v) for v in size.lower().split("x"))
        if not Path(path).exists():
            raise SystemExit(f"Error: Input video file not found: {path}")
        arr = raw_frames(path, w, h, pixel_format)
        return Path(path).stem, (np.ascontiguousarray(arr[i]) for i in range(len(arr))), (w, h, float(config.DEFAULT_OUTPUT_FPS))
    if spec is not None and spec.endswith(".npy"):
        path = Path(spec)
        if not path.exists():
            raise SystemExit(f"Error: Input video file not found: {spec}")
        arr = np.load(path, mmap_mode="r")
        return path.stem, (np.ascontiguousarray(arr[i]) for i in range(len(arr))), (arr.shape[2], arr.shape[1], float(config.DEFAULT_OUTPUT_FPS))
    # a video file or a webcam: cv2.VideoCapture as in the reference (aicamera_tracker.py:113-135)
    if cv2 is None:
        what = f"video file {spec}" if spec else f"webcam {webcam_id}"
        raise SystemExit(f"Error: Could not open video source ({what}): OpenCV (cv2) is not importable here. "
                         "Use synthetic:WxH:persons:frames, a .npy frame dump or raw:WxH:path.")
    if spec is not None and not Path(spec).exists():
        raise SystemExit(f"Error: Input video file not found: {spec}")
    cap = cv2.VideoCapture(spec if spec is not None else webcam_id)
    name = Path(spec).stem if spec is not None else f"webcam_{webcam_id}"
    if not cap.isOpened():
        raise SystemExit(f"Error: Could not open video source ({name}).")
    w, h = int(cap.get(cv2.CAP_PROP_FRAME_WIDTH)), int(cap.get(cv2.CAP_PROP_FRAME_HEIGHT))
    fps = cap.get(cv2.CAP_PROP_FPS) or float(config.DEFAULT_OUTPUT_FPS)

    def frames():
        try:
            while cap.isOpened():
                ret, frame = cap.read()
                if not ret:
                    print("End of video stream or error reading frame.")
                    break
                yield frame
        finally:
            cap.release()
    return name, frames(), (w, h, float(fps))


class FrameWriter:
    """Annotated frames: cv2.VideoWriter when cv2 is there (mp4v / XVID as aicamera_tracker.py:155-156), else headerless BGR24.
    pixel_format="nv12": always headerless, NV12 (frames.from_bgr with the given matrix / range), suffix .nv12.
    mjpeg=dict(quality, restart, device): always Motion-JPEG -- the frames' JFIF files back to back, suffix .mjpeg, the side
    file lists every frame's byte offset; write() encodes a frame with the writer's own JpegEncoder, write_encoded() appends a file
    that a shared encoder made (the S frames of a tick in one call)."""

    def __init__(self, path_stem: Path, size, cv2=None, filename=None, pixel_format="bgr24", yuv_matrix="bt601", yuv_range="limited", mjpeg=None):
        self.cv2, self.raw, self.vw, self.frames = cv2, None, None, 0
        self.yuv = None if pixel_format == "bgr24" else (pixel_format, yuv_matrix, yuv_range)
        self.mjpeg, self.encoder, self.offsets = mjpeg, None, [0]
        w, h, fps = size
        if mjpeg is not None:
            self.path = path_stem.parent / ((filename or path_stem.name) + ".mjpeg")
            self.raw = open(self.path, "wb")
            self.meta = dict(width=w, height=h, fps=fps, codec="mjpeg", quality=mjpeg["quality"], restart=mjpeg["restart"], subsampling="420")
        elif cv2 is not None and self.yuv is None:
            name = filename or path_stem.name + ".mp4"
            if not name.lower().endswith((".mp4", ".avi")):
                name += ".mp4"
            self.path = path_stem.parent / name
            fourcc = cv2.VideoWriter_fourcc(*("mp4v" if name.lower().endswith(".mp4") else "XVID"))
            self.vw = cv2.VideoWriter(str(self.path), fourcc, fps, (w, h))
            if not self.vw.isOpened():
                print(f"Error: Could not open video writer for {self.path}. Video will not be saved.")
                self.vw = None
        else:
            self.path = path_stem.parent / ((filename or path_stem.name) + "." + pixel_format)
            self.raw = open(self.path, "wb")
            self.meta = dict(width=w, height=h, fps=fps, pixel_format=pixel_format)
            if self.yuv is not None:
                self.meta.update(yuv_matrix=yuv_matrix, yuv_range=yuv_range)
        print(f"Output video will be saved to: {self.path}")

    def write_encoded(self, data):
        self.raw.write(data)
        self.offsets.append(self.offsets[-1] + len(data))
        self.frames += 1

    def write(self, frame):
        if self.mjpeg is not None:
            if self.encoder is None:
                self.encoder = mjpeg_encoder(frame.shape[:2], 1, self.mjpeg)
            return self.write_encoded(self.encoder.encode(np.ascontiguousarray(frame)[None])[0])
        if self.vw is not None:
            self.vw.write(frame)
        elif self.raw is not None and self.yuv is not None:
            self.raw.write(pixfmt.from_bgr(frame, self.yuv[0], matrix=self.yuv[1], range=self.yuv[2]).tobytes())
        elif self.raw is not None:
            self.raw.write(np.ascontiguousarray(frame).tobytes())
        self.frames += 1

    def close(self):
        if self.vw is not None:
            self.vw.release()
        if self.encoder is not None:
            self.encoder.close()
        if self.raw is not None:
            self.raw.close()
            if self.mjpeg is not None:
                self.meta["offsets"] = self.offsets
            json.dump(dict(self.meta, frames=self.frames), open(str(self.path) + ".json", "w"))


def mjpeg_encoder(hw, max_images, opts):
    """The JpegEncoder of --output_codec mjpeg: 4:2:0, and no frame is ever dropped for its size."""
    from .jpeg import JpegEncoder
    return JpegEncoder(hw, max_images=max_images, quality=opts["quality"], restart=opts["restart"], subsampling="420", max_bytes="worst",
                       device=opts["device"])


def mjpeg_options(args):
    return dict(quality=args.jpeg_quality, restart=args.jpeg_restart, device=config.resolve_device(args.device)) if args.output_codec == "mjpeg" else None


class _FrameFree:
    """The loop's tracker call with ByteTrack / OC-SORT: update(boxes, scores, class_ids, frame) -- the frame is not needed (no ReID)."""

    def __init__(self, tracker):
        self.tracker = tracker

    def update(self, boxes, scores, class_ids, frame):
        return self.tracker.update(boxes, scores, class_ids)


class _BotSortFrame:
    """The loop's tracker call with BoT-SORT: the boxes of tracked classes above the low band are embedded from the frame (ReIDModel, as
    DeepSORT.update does) and handed to BoTSORT with their validity."""

    def __init__(self, reid_engine, device, dtype, gmc=0, frame_hw=None):
        from .botsort import BoTSORT
        from .reid_model import ReIDModel
        self.reid_model = ReIDModel(engine_path=reid_engine, input_shape=config.REID_INPUT_SHAPE, device=device, dtype=dtype)
        self.tracker = BoTSORT(device=device, feature_dim=self.reid_model.feature_dim)
        self.low = np.float32(self.tracker.params.track_low_thresh)
        self.gmc = None
        if gmc:
            from .gmc import CameraMotion
            self.gmc = CameraMotion(frame_hw[0], frame_hw[1], downscale=gmc, device=device)

    def update(self, boxes, scores, class_ids, frame):
        b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
        s = np.asarray(scores, dtype=np.float32).reshape(-1)
        k = np.asarray(class_ids).reshape(-1).astype(np.int64)
        names = np.array([config.class_name(int(c)) in config.CLASSES_TO_TRACK for c in k], dtype=bool)
        keep = np.nonzero((s > self.low) & names)[0]
        warp = None
        if self.gmc is not None:                 # the boxes as the tracker holds them (tlwh): x2 = x + w in fp32, as the pipeline's masks
            m = b[keep]
            warp = self.gmc.apply(frame, np.stack([m[:, 0], m[:, 1], m[:, 0] + (m[:, 2] - m[:, 0]), m[:, 1] + (m[:, 3] - m[:, 1])], 1))
        if not len(keep):
            return self.tracker.update(np.zeros((0, 4), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int32), warp=warp)
        feats, valid = self.reid_model.embed_boxes(frame, b[keep])
        rows, conf = self.tracker.update_batch_arrays([(b[keep], s[keep], k[keep].astype(np.int32), feats, warp,
                                                        np.asarray(valid).astype(np.int32))])[0]
        return self.tracker._tuples(rows, conf)


class _ZoneLines:
    """--zones: a ZoneCounter (zones.py) over the run's tracks and the "zones" object of every JSON line.  With a pipeline the counter is
    attached to it (one update per run call) and the cumulative counts of a line are those after the frame's run call; frame by frame
    (no pipeline) the tracker's tuples are handed over per frame."""

    def __init__(self, path, streams, device, pipe=None):
        from .zones import KINDS, ZoneCounter, load_zones_file
        geometry = load_zones_file(path, streams)
        self.kinds, self.streams, self.pipe = KINDS, streams, pipe
        self.counter = ZoneCounter(streams=streams, device=device)
        for s, (zs, ls) in enumerate(geometry):
            self.counter.set_zones(s, zs, ls)
        self._res, self._pos, self._counts = None, 0, None
        if pipe is not None:
            pipe.attach_zones(self.counter)

    def line(self, tracks):
        """The next frame's object, in the order the frames are yielded (tick-major over the streams)."""
        if self.pipe is None:
            res, s, f = self.counter.update_tuples([[tracks]]), 0, 0
            self._counts = None
        else:
            res = self.pipe.zone_result
            if res is not self._res:
                self._res, self._pos, self._counts = res, 0, None
            s, t = self._pos % self.streams, self._pos // self.streams
            self._pos += 1
            f = int(res.frames_per_stream[:s].sum()) + t
        if self._counts is None:
            self._counts = [self.counter.counters(k) for k in range(self.streams)]
        out = {"occupancy": res.occupancy[f, :self.counter.n_zones[s]].tolist()}
        out.update({k: v.tolist() for k, v in self._counts[s].items()})
        out["events"] = [{"kind": self.kinds[int(e[0])], "index": int(e[1]), "id": int(e[2]), "cls": int(e[3]), "frame": int(e[4]), "value": int(e[5]),
                          "anchor": [e[6] / 2, e[7] / 2]} for e in res.events[f, :min(int(res.n_events[f]), res.events.shape[1])]]
        return out

    def close(self):
        self.counter.close()


class _BestShotFiles:
    """--best_shots DIR: a BestShots (bestshot.py) over the run's frames and tracks; every final becomes DIR/cam<S>_id<ID>_f<best_frame>.ppm
    (binary P6, RGB) and a line of DIR/index.jsonl.  With a pipeline the stage is attached to it (one update per run call); frame by
    frame (no pipeline) the frame and the tracker's tuples are handed over per frame.  close() flushes what still lives."""

    def __init__(self, args, streams, size, device, pipe=None):
        from . import bestshot
        self.mod, self.pipe, self._res = bestshot, pipe, None
        self.shots = bestshot.BestShots(streams, (size[1], size[0]), thumb=args.best_shot_wh, region=args.best_shot_region, device=device)
        self.dir = Path(args.best_shots)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.index = open(self.dir / "index.jsonl", "a")
        self.link = bool(args.link_cameras)
        self.encoder = None
        if args.best_shot_format == "jpg":                       # thumbnails are small: 4:4:4, and none is dropped for its size
            from .jpeg import JpegEncoder
            self.encoder = JpegEncoder((args.best_shot_wh[1], args.best_shot_wh[0]), max_images=256, quality=args.jpeg_quality, subsampling="444",
                                       max_bytes="worst", device=device)
        if pipe is not None:
            pipe.attach_best_shots(self.shots)

    def _write(self, result):
        finals = self.mod.finals(result)
        files = self.mod.encode_finals(result, self.encoder) if self.encoder is not None and finals else None   # all of them in one call
        ext = "ppm" if self.encoder is None else "jpg"
        for i, (ev, thumb) in enumerate(finals):
            name = f"cam{ev['stream']}_id{ev['id']}_f{ev['best_frame']}.{ext}" if ev["has_shot"] else None   # None: never large enough to show
            if name and files is not None:
                self.mod.write_jpeg(self.dir / name, files[i])
            elif name:
                self.mod.write_ppm(self.dir / name, thumb)
            line = dict(ev, file=name, reason=self.mod.REASONS[ev["reason"]])
            if self.link and self.pipe is not None and self.pipe.xcam is not None:
                line["global_id"] = int(self.pipe.global_ids(ev["stream"], [ev["id"]])[0])
            self.index.write(json.dumps(line) + "\n")

    def after(self, frame, tracks):
        """After every yielded frame: the finals of the run call it came from (once), or of this frame."""
        if self.pipe is None:
            self._write(self.shots.update_tuples(np.ascontiguousarray(frame)[None, None], [[tracks]]))
        elif self.pipe.best_shot_result is not self._res:
            self._res = self.pipe.best_shot_result
            self._write(self._res)

    def close(self):
        try:
            res = self.shots.flush()
            self._write(res)
            while int(res.pending.sum()):
                res = self.shots.drain(cap=self.shots.max_tracks)
                self._write(res)
        finally:
            self.index.close()
            self.shots.close()
            if self.encoder is not None:
                self.encoder.close()


class _SceneLines:
    """--scene_watch: a SceneWatch (scene.py) over the run's frames and tracks.  With a pipeline the stage is attached to it (one update
    per run call, whose frames are then yielded in order); frame by frame (no pipeline) every frame is an update of its own."""

    def __init__(self, args, streams, size, device, pipe=None):
        from . import scene
        self.mod, self.pipe, self._res, self._i, self.streams = scene, pipe, None, 0, streams
        self.watch = scene.SceneWatch(streams, (size[1], size[0]), cell=args.scene_cell or 8, device=device)
        self.ids = {n: i for i, n in enumerate(config.CLASSES)}
        if pipe is not None:
            pipe.attach_scene_watch(self.watch)

    def after(self, frame, tracks):
        """After every yielded frame: ({"active", "moving_cells", "motion_box", "alarms"}, the moving share per track); prints the
        frame's alarm edges."""
        if self.pipe is None:
            rows = np.array([[t[0], t[1], t[2], t[3], t[4], self.ids.get(t[5], -1)] for t in tracks], np.int64).reshape(-1, 6).astype(np.int32)
            self._res, self._i = self.watch.update(np.ascontiguousarray(frame)[None, None], [[rows]]), 0
        elif self.pipe.scene_result is not self._res:
            self._res, self._i = self.pipe.scene_result, 0
        t, s = divmod(self._i, self.streams)
        self._i += 1
        res = self._res
        rec = res.records[t, s]
        for i, kind in enumerate(self.mod.KINDS):
            for raised, bit in ((True, i), (False, 8 + i)):
                if int(res.edges[t, s]) >> bit & 1:
                    print(json.dumps({"alarm": kind, "raised": raised, "stream": s, "frame": int(res.frame[t, s])}))
        scene = {"active": bool(res.active[t, s]), "moving_cells": int(res.n_moving[t, s]), "motion_box": [int(v) for v in res.motion_box[t, s]],
                 "alarms": self.mod.alarm_names(res.alarms[t, s])}
        return scene, [int(v) for v in res.rows_of(t, s)]

    def close(self):
        self.watch.close()


class _LeftLines:
    """--left_objects: a LeftObjects (leftobj.py) over the run's frames and tracks, attached to the pipeline or fed frame by frame as
    _SceneLines is."""

    def __init__(self, args, streams, size, device, pipe=None):
        from . import leftobj
        self.mod, self.pipe, self._res, self._i, self.streams = leftobj, pipe, None, 0, streams
        options = {} if args.left_after is None else dict(min_ticks=args.left_after)
        self.stage = leftobj.LeftObjects(streams, (size[1], size[0]), cell=args.left_cell or 8, device=device, **options)
        self.ids = {n: i for i, n in enumerate(config.CLASSES)}
        if pipe is not None:
            pipe.attach_left_objects(self.stage)

    def after(self, frame, tracks):
        """After every yielded frame: ([{uid, kind, box, owner, age}] of the alarmed objects, (result, stream, tick) for the output
        stage); prints the frame's events."""
        if self.pipe is None:
            rows = np.array([[t[0], t[1], t[2], t[3], t[4], self.ids.get(t[5], -1)] for t in tracks], np.int64).reshape(-1, 6).astype(np.int32)
            self._res, self._i = self.stage.update(np.ascontiguousarray(frame)[None, None], [[rows]]), 0
        elif self.pipe.left_result is not self._res:
            self._res, self._i = self.pipe.left_result, 0
        t, s = divmod(self._i, self.streams)
        self._i += 1
        res = self._res
        for e in res.events_of(s, t):
            print(json.dumps({"left_object": self.mod.EVENT_NAMES[int(e[2])], "stream": s, "frame": int(e[11]), "uid": int(e[3]),
                              "kind": self.mod.KIND_NAMES[int(e[4])], "box": [int(v) for v in e[5:9]], "owner": int(e[9]), "area": int(e[10])}))
        return res.alarmed(s, t), (res, s, t)

    def close(self):
        self.stage.close()


class _ColourLines:
    """--colours [--colours_file FILE]: a TrackColours (colours.py) over the run's frames and tracks, attached to the pipeline or fed
    frame by frame as _SceneLines is.  Every ended track goes to FILE as one JSON object; close() flushes what still lives."""

    def __init__(self, args, streams, size, device, pipe=None):
        from . import colours
        self.mod, self.pipe, self._res, self._i, self._at, self.streams = colours, pipe, None, 0, 0, streams
        self.stage = colours.TrackColours(streams, (size[1], size[0]), device=device)
        self.file = open(args.colours_file, "a") if args.colours_file else None
        if pipe is not None:
            pipe.attach_colours(self.stage)

    def _write(self, result):
        if self.file is not None:
            for ev in self.mod.finals(result):
                self.file.write(json.dumps(dict(ev, reason=self.mod.REASONS[ev["reason"]])) + "\n")

    def after(self, frame, tracks):
        """After every yielded frame: one [upper, lower] pair of names (or None) per track, in the order of the tracks."""
        if self.pipe is None:
            self._res, self._i, self._at = self.stage.update_tuples(np.ascontiguousarray(frame)[None, None], [[tracks]]), 0, 0
            self._write(self._res)
        elif self.pipe.colour_result is not self._res:
            self._res, self._i, self._at = self.pipe.colour_result, 0, 0
            self._write(self._res)
        self._i += 1
        tags = self._res.row_tags[self._at:self._at + len(tracks)]           # the call's rows lie frame after frame, as they were yielded
        self._at += len(tracks)
        return [[self.mod.name_of(int(t[0])), self.mod.name_of(int(t[1]))] for t in tags]

    def close(self):
        try:
            res = self.stage.flush()
            self._write(res)
            while int(res.pending.sum()):
                res = self.stage.drain(cap=self.stage.max_tracks)
                self._write(res)
        finally:
            if self.file is not None:
                self.file.close()
            self.stage.close()


class _ProxLines:
    """--proximity [--ground FILE.json] [--near N] [--proximity_file FILE.jsonl]: a Proximity (proximity.py) over the run's tracks,
    attached to the pipeline or fed frame by frame as _ColourLines is.  Every LINK / UNLINK is printed as a line of its own; every ended
    track goes to FILE as one JSON object; close() flushes what still lives."""

    def __init__(self, args, streams, size, device, pipe=None):
        from . import proximity
        self.mod, self.pipe, self._res, self._i, self._at, self.streams = proximity, pipe, None, 0, 0, streams
        maps = None
        if args.ground:
            with open(args.ground) as f:
                maps = json.load(f)
            maps = [maps] * streams if isinstance(maps, dict) else list(maps)
            if len(maps) != streams:
                raise ValueError(f"{args.ground} holds {len(maps)} ground maps for {streams} cameras")
        self.stage = proximity.Proximity(streams, (size[1], size[0]), metric="ground" if maps else "body", near=args.near, device=device)
        for s, m in enumerate(maps or []):
            H, shift = (m["H"], int(m.get("shift", 0))) if "H" in m else proximity.homography(m["pixels"], m["ground"])
            self.stage.set_ground(H, shift, stream=s)
        self.file = open(args.proximity_file, "a") if args.proximity_file else None
        if pipe is not None:
            pipe.attach_proximity(self.stage)

    def _write(self, result):
        if self.file is not None:
            for ev in result.ended():
                self.file.write(json.dumps(ev) + "\n")

    def after(self, frame, tracks):
        """After every yielded frame: (parties, units, the q8 speed per track, in the order of the tracks); prints the frame's pair events."""
        if self.pipe is None:
            self._res, self._i, self._at = self.stage.update_tuples([[tracks]]), 0, 0
            self._write(self._res)
        elif self.pipe.proximity_result is not self._res:
            self._res, self._i, self._at = self.pipe.proximity_result, 0, 0
            self._write(self._res)
        t, s = divmod(self._i, self.streams)
        self._i += 1
        res = self._res
        for e in res.pairs(t, s):
            print(json.dumps({"pair": e["kind"], "stream": s, "frame": e["frame"], "ids": list(e["ids"]), "duration": e["duration"],
                              "distance": e["distance"], "ticks": e["ticks"]}))
        tags = res.row_tags[self._at:self._at + len(tracks)]                 # the call's rows lie frame after frame, as they were yielded
        self._at += len(tracks)
        return res.parties(t, s), int(res.records[t, s, 9]), [int(v) for v in tags[:, 2]]

    def close(self):
        try:
            res = self.stage.flush()
            self._write(res)
            while int(res.pending.sum()):
                res = self.stage.drain(cap=self.stage.max_tracks)
                self._write(res)
        finally:
            if self.file is not None:
                self.file.close()
            self.stage.close()


class _HeatFiles:
    """--heat_maps DIR [--heat_cell N] [--heat_layer NAME] [--heat_paths FILE] [--heat_overlay]: a HeatMaps (heatmap.py) over the run's
    tracks, attached to the pipeline or fed frame by frame.  Every ended track goes to FILE as one JSON line; close() flushes what still
    lives, then writes every camera's layers and the chosen layer over its last frame."""

    def __init__(self, args, streams, size, device, pipe=None):
        from . import heatmap
        self.mod, self.pipe, self._res, self.streams, self.device = heatmap, pipe, None, streams, device
        self.layer, self.overlay_on = args.heat_layer or "dwell", args.heat_overlay
        self.dir = Path(args.heat_maps)
        self.dir.mkdir(parents=True, exist_ok=True)
        self.stage = heatmap.HeatMaps(streams, (size[1], size[0]), cell=args.heat_cell or 16, device=device)
        self.file = open(args.heat_paths, "a") if args.heat_paths else None
        self.last = np.zeros((streams, size[1], size[0], 3), np.uint8)      # every camera's last frame
        self.quality = args.jpeg_quality
        if pipe is not None:
            pipe.attach_heat_maps(self.stage)

    def _write(self, result):
        if self.file is not None:
            for ev in self.mod.paths(result):
                self.file.write(json.dumps(ev) + "\n")

    def after(self, frame, tracks, camera=0):
        """After every yielded frame."""
        if self.pipe is None:
            self._res = self.stage.update_tuples([[tracks]])
            self._write(self._res)
        elif self.pipe.heat_result is not self._res:
            self._res = self.pipe.heat_result
            self._write(self._res)
        self.last[camera] = frame

    def overlay(self, frames, cameras=None):
        """uint8 [n, H, W, 3] frames with the layer blended in (--heat_overlay), or as they came."""
        if not self.overlay_on:
            return frames
        return self.stage.render(np.ascontiguousarray(frames, dtype=np.uint8), cameras=cameras, layer=self.layer)

    def close(self):
        from .jpeg import JpegEncoder
        try:
            res = self.stage.flush()
            self._write(res)
            while int(res.pending.sum()):
                res = self.stage.drain(cap=self.stage.max_tracks)
                self._write(res)
            for c in range(self.streams):
                lay = self.stage.layers(c)
                np.save(self.dir / f"cam{c}_layers.npy", np.stack([lay[n] for n in self.mod.LAYERS]))
            drawn = self.stage.render(self.last, cameras=list(range(self.streams)), layer=self.layer)
            enc = JpegEncoder(drawn.shape[1:3], max_images=self.streams, quality=self.quality, subsampling="420", max_bytes="worst", device=self.device)
            try:
                for c, data in enumerate(enc.encode(drawn)):
                    (self.dir / f"cam{c}_{self.layer}.jpg").write_bytes(bytes(data))
            finally:
                enc.close()
        finally:
            if self.file is not None:
                self.file.close()
            self.stage.close()


class _Output:
    """The saved frames' last stage.  With --redact / --masks / --draw_zones, or for the S frames of a tick of --inputs, ONE
    render.Renderer call: redaction, static masks, the zones' outlines, labels and the info panel.  Classes travel as config.CLASSES ids,
    -1 (unknown) is always redacted."""

    def __init__(self, args, cameras, device):
        from .render import Renderer, load_masks_file, parse_style
        self.asked = args.redact != "off" or bool(args.masks) or args.draw_zones
        style, cell = parse_style(args.redact_style)
        masks = load_masks_file(args.masks, cameras) if args.masks else None
        geometry = None
        if args.draw_zones:
            from .zones import load_zones_file
            geometry = load_zones_file(args.zones, cameras)
        self.geometry, self.cameras, self.ids = geometry, cameras, {n: i for i, n in enumerate(config.CLASSES)}
        self.renderer = Renderer(cameras=cameras, redact=args.redact, style=style, cell=cell, device=device)
        try:
            for c, polys in enumerate(masks or []):
                self.renderer.set_masks(c, polys)
        except Exception:
            self.renderer.close()
            raise

    def draw(self, frames, tracks, shown, infos, left=None):
        """frames: S arrays [H, W, 3] of cameras 0..S-1, or one uint8 array [S, H, W, 3] (drawn in place) -> uint8 [S, H, W, 3] annotated.  tracks: the trackers' tuples (redaction), shown: the
        tuples as labelled, infos: the info panel's lines per frame."""
        batch = frames if isinstance(frames, np.ndarray) else np.ascontiguousarray(np.stack(frames), dtype=np.uint8)
        rows = [np.array([[t[0], t[1], t[2], t[3], 0, self.ids.get(t[5], -1)] for t in tr], np.int64).reshape(-1, 6) for tr in tracks]
        prims = []
        for c, (sh, info) in enumerate(zip(shown, infos)):
            pl = visualization.PrimList()
            if self.geometry is not None:
                visualization.zone_prims(pl, *self.geometry[c])
            if left is not None and left[c] is not None:                      # (LeftResult, stream, tick): the objects under the labels
                left[c][0].prims(left[c][1], left[c][2], pl)
            prims.append(visualization.info_prims(visualization.track_prims(pl, sh), list(info)))
        return self.renderer.render(batch, np.concatenate(rows).astype(np.int32), [len(r) for r in rows], prims)

    def close(self):
        self.renderer.close()


def main_streams(args, cv2):
    """--inputs: the sources as the streams of ONE pipeline (TrackingPipeline(streams=S), or TrackingPipeline.botsort_bank /
    deepsort_bank for --tracker botsort / deepsort_bank), their frames interleaved tick by tick."""
    from .pipeline import TrackingPipeline
    sources = [frame_source(spec, args.webcam_id, cv2, args.pixel_format, config.resolve_device(args.device)) for spec in args.inputs.split(",") if spec]
    yuv_in = dict(pixel_format=args.pixel_format, yuv_matrix=args.yuv_matrix, yuv_range=args.yuv_range)
    yuv_out = dict(pixel_format=args.output_pixel_format, yuv_matrix=args.yuv_matrix, yuv_range=args.yuv_range)
    S = len(sources)
    size = sources[0][2]
    if any(src[2][:2] != size[:2] for src in sources):
        print("Error: --inputs sources must have one frame size: " + ", ".join(f"{src[2][0]}x{src[2][1]}" for src in sources))
        return 1
    if args.conf_thresh is None:
        args.conf_thresh = (0.1 if args.tracker in ("bytetrack", "botsort") else
                            config.YOLO_CONF_THRESHOLD if args.tracker == "deepsort_bank" else 0.6)
    batch = max(1, args.batch // S) * S          # whole ticks per launch group
    dev = config.resolve_device(args.device)
    try:
        if args.tracker == "botsort":
            from .hip_engine import HipEngine
            reid = HipEngine(args.reid_engine, device=dev, dtype=args.dtype, max_items=batch * 64, warm_up=False)   # as the single-source path
            pipe = TrackingPipeline.botsort_bank(args.yolo_engine, reid, (size[1], size[0]), cameras=S, gmc=args.gmc, batch=batch,
                                                 ring_frames=batch, max_persons=512, max_tracks=512, device=dev, dtype=args.dtype,
                                                 conf_thresh=args.conf_thresh, **yuv_in)
        elif args.tracker == "deepsort_bank":
            from .hip_engine import HipEngine
            reid = HipEngine(args.reid_engine, device=dev, dtype=args.dtype, max_items=batch * 64, warm_up=False)   # as the single-source path
            pipe = TrackingPipeline.deepsort_bank(args.yolo_engine, reid, (size[1], size[0]), cameras=S, batch=batch, ring_frames=batch,
                                                  max_persons=512, max_tracks=512, device=dev, dtype=args.dtype,
                                                  conf_thresh=args.conf_thresh, **yuv_in)
        else:
            pipe = TrackingPipeline(args.yolo_engine, None, (size[1], size[0]), batch=batch, ring_frames=batch, max_persons=512,
                                    max_tracks=512, device=dev, dtype=args.dtype, conf_thresh=args.conf_thresh,
                                    tracker=args.tracker, streams=S, **yuv_in)
    except Exception as e:
        print(f"Error initializing YOLO Detector: {e}")
        return 1
    label = "AICamera: YOLOv8 + " + {"bytetrack": "ByteTrack", "ocsort": "OC-SORT", "botsort": "BoT-SORT", "deepsort_bank": "DeepSORT"}[args.tracker]
    outs, writers = [None] * S, [None] * S
    if not args.no_save:
        out_dir = Path(args.output_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
        stamp = time.strftime('%Y%m%d-%H%M%S')
        for k, (name, _, _) in enumerate(sources):
            stem = out_dir / f"{name}_tracked_{stamp}_s{k}"
            outs[k] = open(str(stem) + ".jsonl", "w")
            writers[k] = FrameWriter(stem, size, cv2, f"{args.output_filename}_s{k}" if args.output_filename else None, **yuv_out,
                                     mjpeg=mjpeg_options(args))
    pipe.link_after_run = bool(args.link_cameras)
    archive = None
    if args.archive:
        try:
            archive = _attach_archive(args, pipe, dev)
        except Exception as e:
            print(f"Error setting up --archive: {e}")
            pipe.close()
            return 1
    zones = None
    if args.zones:
        try:
            zones = _ZoneLines(args.zones, S, dev, pipe)
        except Exception as e:
            print(f"Error reading --zones {args.zones}: {e}")
            pipe.close()
            return 1
    shots = None
    if args.best_shots:
        try:
            shots = _BestShotFiles(args, S, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --best_shots: {e}")
            if zones is not None:
                zones.close()
            pipe.close()
            return 1
    watch = None
    if args.scene_watch:
        try:
            watch = _SceneLines(args, S, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --scene_watch: {e}")
            for f in (zones, shots):
                if f is not None:
                    f.close()
            pipe.close()
            return 1
    left = None
    if args.left_objects:
        try:
            left = _LeftLines(args, S, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --left_objects: {e}")
            for f in (zones, shots, watch):
                if f is not None:
                    f.close()
            pipe.close()
            return 1
    worn = None
    if args.colours:
        try:
            worn = _ColourLines(args, S, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --colours: {e}")
            for f in (zones, shots, watch, left):
                if f is not None:
                    f.close()
            pipe.close()
            return 1
    heat = None
    if args.heat_maps:
        try:
            heat = _HeatFiles(args, S, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --heat_maps: {e}")
            for f in (zones, shots, watch, left, worn):
                if f is not None:
                    f.close()
            pipe.close()
            return 1
    prox = None
    if args.proximity:
        try:
            prox = _ProxLines(args, S, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --proximity: {e}")
            for f in (zones, shots, watch, left, worn, heat):
                if f is not None:
                    f.close()
            pipe.close()
            return 1
    output = None
    if not args.no_save:
        try:
            output = _Output(args, S, dev)
        except Exception as e:
            print(f"Error setting up the output stage (--redact_style / --masks / --draw_zones): {e}")
            for f in outs + writers + [zones]:
                if f is not None:
                    f.close()
            pipe.close()
            return 1
    ticks = (f for tick in zip(*(src[1] for src in sources)) for f in tick)       # the shortest source ends the run
    n, t0 = 0, time.time()
    tick = []                                                                     # the tick's (tracks, labelled tracks) so far
    batch = np.empty((S, size[1], size[0], 3), np.uint8) if output is not None else None      # its frames: copied as they arrive
    encoder = mjpeg_encoder((size[1], size[0]), S, mjpeg_options(args)) if output is not None and args.output_codec == "mjpeg" else None
    try:
        for frame, tracks in pipe.stream(ticks, read_back=output is not None):   # (YUV sources: the frames drawn on come back from the ring)
            k, idx = n % S, n // S
            n += 1
            if shots is not None:
                shots.after(frame, tracks)
            scene = watch.after(frame, tracks) if watch is not None else None
            lost = left.after(frame, tracks) if left is not None else None
            wears = worn.after(frame, tracks) if worn is not None else None
            if heat is not None:
                heat.after(frame, tracks, k)
            together = prox.after(frame, tracks) if prox is not None else None
            gids = pipe.global_ids(k, [t[4] for t in tracks]).tolist() if args.link_cameras else None
            if output is not None:
                shown = tracks if gids is None else [t[:4] + (f"{t[4]} G{(g >> 32) & 0xfff}.{g & 0xffffffff}" if g >= 0 else t[4],) + t[5:] for t, g in zip(tracks, gids)]
                batch[k] = frame
                tick.append((tracks, shown, lost[1] if lost is not None else None))
                if len(tick) == S:                                                # the tick's S frames in ONE render call
                    if heat is not None:
                        batch[:] = heat.overlay(batch)
                    drawn = output.draw(batch, [t[0] for t in tick], [t[1] for t in tick],
                                        [[label, f"Input: {sources[c][0]} (stream {c})"] for c in range(S)], [t[2] for t in tick])
                    if encoder is not None:                                       # ... and in ONE encode call
                        for c, data in enumerate(encoder.encode(np.ascontiguousarray(drawn))):
                            writers[c].write_encoded(data)
                    else:
                        for c in range(S):
                            writers[c].write(drawn[c])
                    tick = []
            if outs[k]:
                line = {"frame": idx, "tracks": tracks}
                if gids is not None:
                    line["global_ids"] = gids
                if archive is not None:
                    line["returning"] = [[t, key, d] for c, t, key, d in pipe.xcam.returning() if c == k]
                if zones is not None:
                    line["zones"] = zones.line(tracks)
                if scene is not None:
                    line["scene"], line["moving"] = scene
                if lost is not None:
                    line["left_objects"] = lost[0]
                if wears is not None:
                    line["colours"] = wears
                if together is not None:
                    line["parties"], line["units"], line["speed"] = together
                outs[k].write(json.dumps(line) + "\n")
    except KeyboardInterrupt:
        print("Processing interrupted by user.")
    finally:
        for f in outs + writers:
            if f is not None:
                f.close()
        if zones is not None:
            zones.close()
        if shots is not None:
            shots.close()
        if watch is not None:
            watch.close()
        if left is not None:
            left.close()
        if worn is not None:
            worn.close()
        if heat is not None:
            heat.close()
        if prox is not None:
            prox.close()
        if output is not None:
            output.close()
        if encoder is not None:
            encoder.close()
        if archive is not None:
            if args.archive_file:
                archive.save(args.archive_file)
            pipe.xcam.attach_archive(None)
            archive.close()
        pipe.close()
    total = time.time() - t0
    print("\n--- Processing Summary ---")
    print(f"Streams: {S}; ticks processed: {n // S}; frames: {n}")
    print(f"Total time: {total:.2f} seconds; average FPS over all streams: {n / total if total > 0 else 0:.2f}")
    print("AICamera finished.")
    return 0


def _attach_archive(args, pipe, dev):
    """--archive: the pipeline's cross-camera object, made now so that the archive can be attached before the first pass."""
    from .archive import IdentityArchive
    from .xcam import CrossCamera
    if pipe.tracker_kind == "deepsort":
        p, dim, thr = pipe.tracker_params, int(pipe.reid.out_dim), pipe.tracker_params.max_cosine_distance
    else:
        p, dim, thr = pipe.botsort_params, pipe.botsort_params.feature_dim or 512, config.DEEPSORT_MAX_DIST
    archive = IdentityArchive(args.archive, dim, device=dev)
    if args.archive_file and Path(args.archive_file).exists():
        archive.load(args.archive_file)
    pipe.xcam = CrossCamera(pipe.streams, p.max_tracks or 512, dim, thr, device=dev)
    pipe.xcam.option("min_gap", args.archive_min_gap)
    pipe.archive = archive
    pipe.xcam.attach_archive(archive)
    return archive


def main(argv=None):
    args = parse_arguments(argv)
    cv2 = probe_cv2()
    if cv2 is None:
        print("OpenCV (cv2) is not importable: video files / webcams / --show_display are unavailable; codec-free sources and raw outputs are used.")
    if args.inputs is not None:
        return main_streams(args, cv2)
    print("Initializing YOLOv8 Detector...")
    name, frames, size = frame_source(args.input, args.webcam_id, cv2, args.pixel_format, config.resolve_device(args.device))
    yuv_in = dict(pixel_format=args.pixel_format, yuv_matrix=args.yuv_matrix, yuv_range=args.yuv_range)
    if args.pixel_format != "bgr24" and args.batch <= 1:       # the plugin classes' signatures stay BGR: convert frame by frame
        frames = (pixfmt.to_bgr(f, args.pixel_format, matrix=args.yuv_matrix, range=args.yuv_range)[0] for f in frames)
    bytetrack = args.tracker == "bytetrack"
    ocsort = args.tracker == "ocsort"
    botsort = args.tracker == "botsort"
    if args.conf_thresh is None:             # ByteTrack's bands need the detector's low band (low_thresh = 0.1); OC-SORT takes s > det_thresh
        args.conf_thresh = 0.1 if bytetrack or botsort else 0.6 if ocsort else config.YOLO_CONF_THRESHOLD
    pipe = detector = tracker = None
    try:
        if args.batch > 1:
            from .pipeline import TrackingPipeline
            # rows per frame = the tracker's slot capacity: a frame cannot emit more confirmed tracks than that, so nothing is ever
            # clipped (the per-frame path and the reference, deepsort_tracker.py:126-141, emit every confirmed track)
            from .hip_engine import HipEngine
            dev_id = config.resolve_device(args.device)
            reid = None if bytetrack or ocsort else HipEngine(args.reid_engine, device=dev_id, dtype=args.dtype, max_items=args.batch * 64, warm_up=False)   # arena for 64 crops per frame; busier groups take more ReID rounds
            pipe = TrackingPipeline(args.yolo_engine, reid, (size[1], size[0]), batch=args.batch, ring_frames=args.batch,
                                    max_persons=512, max_tracks=512, device=dev_id, dtype=args.dtype, conf_thresh=args.conf_thresh,
                                    tracker=args.tracker, gmc=args.gmc, **yuv_in)
        else:
            detector = YOLODetector(engine_path=args.yolo_engine, conf_threshold=args.conf_thresh, device=args.device, dtype=args.dtype)
    except Exception as e:   # aicamera_tracker.py:94-97
        print(f"Error initializing YOLO Detector: {e}")
        return 1
    if pipe is None and bytetrack:
        print("Initializing ByteTrack Tracker...")
        try:
            from .bytetrack import BYTETracker
            tracker = _FrameFree(BYTETracker(device=args.device))
        except Exception as e:
            print(f"Error initializing ByteTrack Tracker: {e}")
            return 1
    elif pipe is None and botsort:
        print("Initializing BoT-SORT Tracker...")
        try:
            tracker = _BotSortFrame(args.reid_engine, args.device, args.dtype, gmc=args.gmc, frame_hw=(size[1], size[0]))
        except Exception as e:
            print(f"Error initializing BoT-SORT Tracker: {e}")
            return 1
    elif pipe is None and ocsort:
        print("Initializing OC-SORT Tracker...")
        try:
            from .ocsort import OCSort
            tracker = _FrameFree(OCSort(device=args.device))
        except Exception as e:
            print(f"Error initializing OC-SORT Tracker: {e}")
            return 1
    elif pipe is None:
        print("Initializing DeepSORT Tracker...")
        try:
            tracker = DeepSORT(reid_model_path=args.reid_engine, device=args.device, dtype=args.dtype)
        except Exception as e:   # aicamera_tracker.py:107-110
            print(f"Error initializing DeepSORT Tracker: {e}")
            return 1
    print(f"Opened source: {name} ({size[0]}x{size[1]} @ {size[2]:.2f} FPS)")
    out_f, writer = None, None
    if not args.no_save:
        out_dir = Path(args.output_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
        stem = out_dir / f"{name}_tracked_{time.strftime('%Y%m%d-%H%M%S')}"
        out_f = open(str(stem) + ".jsonl", "w")
        writer = FrameWriter(stem, size, cv2, args.output_filename, args.output_pixel_format, args.yuv_matrix, args.yuv_range, mjpeg_options(args))
    if args.show_display and cv2 is None:
        print("--show_display ignored: no display backend (cv2) here.")
    frame_idx, total, display_fps = 0, 0.0, 0.0
    dev = config.resolve_device(args.device)
    zones = None
    if args.zones:
        try:
            zones = _ZoneLines(args.zones, 1, dev, pipe)
        except Exception as e:
            print(f"Error reading --zones {args.zones}: {e}")
            for f in (out_f, writer, pipe):
                if f is not None:
                    f.close()
            return 1
    shots = None
    if args.best_shots:
        try:
            shots = _BestShotFiles(args, 1, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --best_shots: {e}")
            for f in (out_f, writer, zones, pipe):
                if f is not None:
                    f.close()
            return 1
    watch = None
    if args.scene_watch:
        try:
            watch = _SceneLines(args, 1, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --scene_watch: {e}")
            for f in (out_f, writer, zones, shots, pipe):
                if f is not None:
                    f.close()
            return 1
    left = None
    if args.left_objects:
        try:
            left = _LeftLines(args, 1, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --left_objects: {e}")
            for f in (out_f, writer, zones, shots, watch, pipe):
                if f is not None:
                    f.close()
            return 1
    worn = None
    if args.colours:
        try:
            worn = _ColourLines(args, 1, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --colours: {e}")
            for f in (out_f, writer, zones, shots, watch, left, pipe):
                if f is not None:
                    f.close()
            return 1
    heat = None
    if args.heat_maps:
        try:
            heat = _HeatFiles(args, 1, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --heat_maps: {e}")
            for f in (out_f, writer, zones, shots, watch, left, worn, pipe):
                if f is not None:
                    f.close()
            return 1
    prox = None
    if args.proximity:
        try:
            prox = _ProxLines(args, 1, size, dev, pipe)
        except Exception as e:
            print(f"Error setting up --proximity: {e}")
            for f in (out_f, writer, zones, shots, watch, left, worn, heat, pipe):
                if f is not None:
                    f.close()
            return 1

    output = None
    if args.redact != "off" or args.masks or args.draw_zones or args.redact_style != "mosaic:16":
        try:
            output = _Output(args, 1, dev)
        except Exception as e:
            print(f"Error setting up the output stage (--redact_style / --masks / --draw_zones): {e}")
            for f in (out_f, writer, zones, pipe):
                if f is not None:
                    f.close()
            return 1

    def per_frame():
        nonlocal total
        for frame in frames:
            t0 = time.time()
            try:
                boxes, scores, cids, _ = detector.detect(frame)
            except Exception as e:
                print(f"Error during detection on frame {frame_idx}: {e}")
                continue
            try:
                tracks = tracker.update(boxes, scores, cids, frame)
            except Exception as e:
                print(f"Error during tracking on frame {frame_idx}: {e}")
                tracks = []
            total += time.time() - t0
            yield frame, tracks

    def batched():
        nonlocal total
        t_prev = time.time()
        for frame, tracks in pipe.stream(frames, read_back=writer is not None or (args.show_display and cv2 is not None)):
            now = time.time()
            total += now - t_prev      # the staging thread reads ahead; per-frame time = the stream's pace
            yield frame, tracks
            t_prev = time.time()

    try:
        for frame, tracks in (batched() if pipe is not None else per_frame()):
            frame_idx += 1
            display_fps = frame_idx / total if total > 0 else 0.0
            if shots is not None:
                shots.after(frame, tracks)
            scene = watch.after(frame, tracks) if watch is not None else None
            lost = left.after(frame, tracks) if left is not None else None
            wears = worn.after(frame, tracks) if worn is not None else None
            if heat is not None:
                heat.after(frame, tracks)
            together = prox.after(frame, tracks) if prox is not None else None
            if writer is not None or (args.show_display and cv2 is not None):      # aicamera_tracker.py:211-236
                if heat is not None and heat.overlay_on:
                    frame = heat.overlay(np.ascontiguousarray(frame)[None])[0]
                info = ["AICamera: YOLOv8 + " + ("ByteTrack" if bytetrack else "OC-SORT" if ocsort else "BoT-SORT" if botsort else "DeepSORT"), f"Input: {name}", f"FPS: {display_fps:.2f}"]
                vis = visualization.draw_frame(frame.copy(), tracks, info, dev) if output is None else output.draw([frame], [tracks], [tracks], [info], [lost[1] if lost is not None else None])[0]
                if args.show_display and cv2 is not None:
                    cv2.imshow("AICamera Tracking", vis)
                    if cv2.waitKey(1) & 0xFF == ord("q"):
                        print("Exiting...")
                        break
                if writer is not None:
                    writer.write(vis)
            if out_f:
                line = {"frame": frame_idx - 1, "tracks": tracks}
                if zones is not None:
                    line["zones"] = zones.line(tracks)
                if scene is not None:
                    line["scene"], line["moving"] = scene
                if lost is not None:
                    line["left_objects"] = lost[0]
                if wears is not None:
                    line["colours"] = wears
                if together is not None:
                    line["parties"], line["units"], line["speed"] = together
                out_f.write(json.dumps(line) + "\n")
            if frame_idx % 100 == 0:
                print(f"Processed {frame_idx} frames. Current FPS: {display_fps:.2f}")
    except KeyboardInterrupt:
        print("Processing interrupted by user.")
    finally:
        if out_f:
            out_f.close()
        if writer is not None:
            writer.close()
        if zones is not None:
            zones.close()
        if shots is not None:
            shots.close()
        if watch is not None:
            watch.close()
        if left is not None:
            left.close()
        if worn is not None:
            worn.close()
        if heat is not None:
            heat.close()
        if prox is not None:
            prox.close()
        if output is not None:
            output.close()
        if pipe is not None:
            clipped = pipe.counters()["clipped_frames"]
            if clipped:
                print(f"Warning: {clipped} frames had more confirmed tracks than the {pipe.max_persons} rows stored per frame.")
            pipe.close()
        if cv2 is not None and args.show_display:
            cv2.destroyAllWindows()
    print("\n--- Processing Summary ---")
    print(f"Total frames processed: {frame_idx}")
    print(f"Total time: {total:.2f} seconds")
    print(f"Average FPS: {frame_idx / total if total > 0 else 0:.2f}")
    print("AICamera finished.")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
