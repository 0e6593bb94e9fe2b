/*
 * aicam.h -- C ABI of libaicam.so, the MI355X (gfx950) detect+track hot path.
 *
 * The reference (abdur75648/AI-Camera) is pure Python and has no FFI; its hot path sits
 * behind Python plugin classes.  Each entry point below replaces the
 * arithmetic of the reference call site named in its comment (paths relative to the
 * reference repo) and is what the reference-side ctypes stub in INTEGRATION.md binds.
 *
 * Conventions
 *   - every function returns 0 (AIC_OK) or a negative AIC_ERR_* code; aic_last_error()
 *     returns the message of the last failure on the calling thread;
 *   - plain pointers and sizes only; `mem` arguments say where a buffer lives
 *     (AIC_HOST = host memory, AIC_DEVICE = HBM of the handle's device);
 *   - outputs are caller-owned buffers with explicit capacities;
 *   - one handle = one HIP stream; a handle is not thread-safe, distinct handles are
 *     independent (one process per GPU, one pipeline per video stream);
 *   - there is NO CPU fallback: without a gfx950 device every compute entry point
 *     fails with AIC_ERR_NO_DEVICE.  Host-side integer logic (aic_lsap,
 *     aic_min_cost_matching) is the only code that runs without a GPU, exactly as
 *     the reference keeps it on the host.
 */
#ifndef AICAM_H
#define AICAM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIC_ABI_VERSION 2

#define AIC_OK 0
#define AIC_ERR_INVALID (-1)   /* bad argument            (reference: ValueError / TypeError)  */
#define AIC_ERR_NOT_FOUND (-2) /* engine file missing     (reference: FileNotFoundError)        */
#define AIC_ERR_RUNTIME (-3)   /* HIP call / kernel failed (reference: RuntimeError)            */
#define AIC_ERR_NO_DEVICE (-4) /* no gfx950 device visible                                      */
#define AIC_ERR_CAPACITY (-5)  /* output buffer / static capacity too small                     */
#define AIC_ERR_FORMAT (-6)    /* malformed engine file                                         */

#define AIC_HOST 0
#define AIC_DEVICE 1

#define AIC_F32 0 /* fp32 activations, v_mfma_f32_16x16x4_f32: the parity mode           */
#define AIC_F16 1 /* fp16 activations / fp32 accumulate, v_mfma_f32_16x16x32_f16          */

#define AIC_MODEL_YOLO 1
#define AIC_MODEL_REID 2

typedef struct aic_model aic_model;       /* one engine file resident on one GPU          */
typedef struct aic_tracker aic_tracker;   /* DeepSORT core state of one video stream      */
typedef struct aic_pipeline aic_pipeline; /* detector + ReID + tracker over resident frames */
typedef struct aic_bytetrack aic_bytetrack; /* ByteTrack state of one video stream          */
typedef struct aic_botsort aic_botsort;     /* BoT-SORT state of one video stream           */
typedef struct aic_gmc aic_gmc;             /* camera-motion estimator of one video stream  */
typedef struct aic_ocsort aic_ocsort;     /* OC-SORT state of one video stream            */
typedef struct aic_bytetrack_bank aic_bytetrack_bank; /* ByteTrack state of 1..256 streams    */
typedef struct aic_ocsort_bank aic_ocsort_bank;       /* OC-SORT state of 1..256 streams      */
typedef struct aic_botsort_bank aic_botsort_bank;     /* BoT-SORT state of 1..256 streams     */
typedef struct aic_deepsort_bank aic_deepsort_bank;   /* DeepSORT state of 1..256 streams     */
typedef struct aic_gmc_bank aic_gmc_bank;             /* camera-motion estimator of 1..256 streams */

/* ------------------------------------------------------------------ library / device */
const char* aic_last_error(void);
int aic_abi_version(void);
int aic_device_count(int* count);
int aic_device_sync(int device);
/* Tests only: allocates one fresh device buffer of float, of int32 and of uint8 and one page-locked uint8 buffer through the library's
 * allocators, writes nothing into them and copies their first four elements out (host outputs of 4 elements each).  With
 * AICAM_POISON_ALLOC=zero|big|nan in the environment of the process (read once; csrc/poison_pattern.hpp) every fresh allocation of
 * the library is filled before use, and this call shows the fill; unset, it returns whatever the memory held. */
int aic_debug_alloc_probe(int device, float* f32_out, int32_t* i32_out, uint8_t* u8_out, uint8_t* pinned_u8_out);

/* ------------------------------------------------------------------ engines
 * Replaces TRTEngine (src/trt_utils/trt_engine.py:15-216): deserialise an engine file
 * (here: graph IR + fp32 weights written by ai-camera_amd/engine_file.py), keep it
 * resident, run it on a stream.  max_items = largest batch (frames for YOLO, crops for
 * ReID) the activation arena is sized for. */
int aic_model_load(const char* path, int device, int dtype, int max_items, aic_model** out);
int aic_model_load_mem(const void* blob, size_t nbytes, int device, int dtype, int max_items,
                       aic_model** out);
/* debugging / tests: the first `bytes` bytes of activation buffer `buf` (engine-file buffer index; NHWC, the engine's activation dtype,
 * items of the last run first) -- what a TensorRT user gets by marking a layer as an output (src/trt_utils/trt_engine.py:62-120 lists
 * only the marked I/O tensors).  A buffer, or the items of one, that no op of the last run wrote holds stale data. */
int aic_model_read_buffer(aic_model* m, int buf, void* out, size_t bytes);
/* Read-only: what a launch of n items runs at op `op` of the engine's op list, decided by the code the launch itself goes through.
 * out[24]: [0] -1 = no conv launch of its own (not a conv, or absorbed at load time), -2 = runs inside the launch that starts at op
 * out[1], 0 = one conv, 1 = conv with the next 1x1 in its epilogue, 2 = 64-channel BasicBlock pair in one kernel, 3 = C2f block in one
 * kernel; [1] first op of the launch, [2] ops it covers, [3] images per block (kind 2); kinds 0 / 1: [4] K order, [5..20] the planner's
 * form, mt, nt, wm, wn, nstage, th, tw, cpp, pitch, kord, g, tail, x2, run, blocks; [21] split source, [22] / [23] destination /
 * source channel offset. */
int aic_model_conv_plan(aic_model* m, int op, int n, int32_t* out);
/* Tests: the same answer with a device-side item count in force (the pipeline's device-filtered ReID rounds, aic_reid_infer_live):
 * the planner refuses some forms then, so the layer may run another kernel than aic_model_conv_plan names.  Launches nothing. */
int aic_model_conv_plan_live(aic_model* m, int op, int n, int32_t* out);
/* Read-only: the row band of op `op` of the engine's op list for frames of src_h x src_w -- the rows of its output map that can depend
 * on the frame when the letterboxed picture has flat borders above and below it (csrc/row_band.hpp) -- and what the last run of the
 * engine on frames (aic_detect, the pipeline) did with it.  out[8]: [0] 1 = every row (the op is not modelled, follows one that is
 * not, or the geometry has borders left / right), [1] / [2] first / last row of the band, [3] rows of the map, [4] 1 = the last run on
 * frames ran the launch that covers this op on a row window, [5] / [6] that window's first row and row count, [7] item slots whose
 * constant rows are in place (0: the next run on frames computes the full maps). */
int aic_model_row_band(aic_model* m, int op, int src_h, int src_w, int32_t* out);
/* Sparse box branches (csrc/engine.hpp): a detect run (aic_detect, the pipeline) may run the detector's box branches only at the anchors
 * its NMS will read, from lists made on the device -- the same bits at those anchors, which path a run took changes time only.
 * force: 1 = every eligible run takes the lists, at any launch size and any count (tests), 0 = the library chooses, < 0 = leave as it is.
 * out (may be NULL) [8], about the last run of the engine: [0] 1 = its box branches ran on the lists, [1..3] candidates of levels
 * 0 .. 2 and [4] listed neighbourhood pixels of level 0, as the device counted them (0 when no candidate pass ran), [5] 1 = a
 * candidate pass ran, [6] 1 = the engine's head has the shape the lists need, [7] 1 = level 0's first box conv is listed as well. */
int aic_model_sparse_box(aic_model* m, int force, int32_t* out);
/* Tests: the detector workspace as the last run and its decode left it, frames 0 .. n-1 (host outputs, each may be NULL):
 * boxes[n,A,4], max class logit[n,A], label[n,A].  After a run that took the lists only candidate anchors hold that run's boxes. */
int aic_model_read_det(aic_model* m, int n, float* boxes, float* max_logit, int32_t* labels);
int aic_model_destroy(aic_model* m);
/* kind, input H/W, classes (YOLO) or feature dim (ReID), anchors per image, conv FLOPs per item */
int aic_model_info(const aic_model* m, int* kind, int* in_h, int* in_w, int* out_dim,
                   int* n_anchors, double* flops_per_item, int* n_convs);

/* TRTEngine.infer for the YOLO engine (trt_engine.py:151-203 called at
 * src/detector/yolo_detector.py:97): images fp32 NCHW RGB in [0,1] -> the four NMS-plugin
 * tensors the detector reads (yolo_detector.py:44-54,108-112): num_dets[B],
 * bboxes[B,max_det,4] (xyxy, letterbox space), scores[B,max_det], labels[B,max_det]. */
int aic_yolo_infer(aic_model* m, const float* images_nchw, int batch, int mem, float conf_thresh,
                   float iou_thresh, int max_det, int32_t* num_dets, float* bboxes, float* scores,
                   int32_t* labels);
/* Raw head of the same engine for parity tests: per anchor 4*reg_max DFL logits and nc class
 * logits, anchors ordered level-major then row-major (8400 at 640x640). Host outputs. */
int aic_yolo_head(aic_model* m, const float* images_nchw, int batch, int mem, float* dfl_logits,
                  float* cls_logits);
/* Decode of the same head (DFL expectation, ltrb->xyxy*stride, arg-max class): boxes[B,A,4],
 * max class logit[B,A], label[B,A]. Host outputs. */
int aic_yolo_decode(aic_model* m, const float* images_nchw, int batch, int mem, float* boxes,
                    float* max_logit, int32_t* labels);

/* Tests / diagnostics: the post-processing of aic_yolo_infer / aic_detect alone, on head logits the caller supplies (the layout
 * aic_yolo_head returns: dfl_logits[B,A,4*reg_max], cls_logits[B,A,nc], host).  No conv runs: the logits are copied into the engine's
 * own head buffers and the production decode and select + sort + NMS launches run on them with the production arguments; the decode
 * kernel does the whole decode (no detect-branch tail has seen these logits).  use_geom != 0: the kept boxes are also un-letterboxed
 * (image_processing.py:141-183) with pad_w, pad_h, ratio into an orig_w x orig_h frame.  Every output is IN/OUT host memory: its
 * contents are uploaded before the kernels run, so a caller that prefills a sentinel sees which elements the kernels wrote.
 * boxes[B,A,4], max_logit[B,A], labels[B,A], n_cand[B], num_dets[B], out_boxes[B,max_det,4], out_boxes_orig[B,max_det,4] (may be
 * NULL when use_geom == 0, and is left alone then), out_scores[B,max_det], out_labels[B,max_det]. */
int aic_yolo_postprocess(aic_model* m, const float* dfl_logits, const float* cls_logits, int batch, float conf_thresh,
                         float iou_thresh, int max_det, int use_geom, float pad_w, float pad_h, float ratio, int orig_w,
                         int orig_h, float* boxes, float* max_logit, int32_t* labels, int32_t* n_cand, int32_t* num_dets,
                         float* out_boxes, float* out_boxes_orig, float* out_scores, int32_t* out_labels);
/* Tests / diagnostics: the pipeline's on-device detection filter (deepsort_tracker.py:88-101: conf >= min_conf and a tracked class,
 * in order) on host arrays.  Inputs num_dets[B], boxes[B,max_det,4], scores[B,max_det], labels[B,max_det]; mask[2]: bit c = class c
 * is tracked.  IN/OUT (uploaded first, as above): rank[B,max_det], frame_n[B], frame_d0[B], total[2] (rows present <= cap, rows the
 * filter passed), and the compact xyxy[cap,4], tlwh[cap,4], conf[cap], cls[cap], frame_of[cap]. */
int aic_det_filter(int device, const int32_t* num_dets, const float* boxes, const float* scores, const int32_t* labels,
                   int batch, int max_det, float min_conf, const uint64_t* mask, int cap, int32_t* rank, int32_t* frame_n,
                   int32_t* frame_d0, int32_t* total, float* xyxy, float* tlwh, float* conf, int32_t* cls,
                   int32_t* frame_of);

/* TRTEngine.infer for the ReID engine (src/tracker/reid_model.py:111-126): crops fp32 NCHW,
 * ImageNet-normalised -> embeddings[N, feature_dim] fp32. */
int aic_reid_infer(aic_model* m, const float* crops_nchw, int n, int mem, float* embeddings,
                   int out_mem);

/* ------------------------------------------------------------------ pre / post processing
 * letterbox + preprocess_yolo_input (src/utils/image_processing.py:7-70,73-102): u8 BGR HWC
 * frame -> fp32 NCHW RGB /255, padded with 114; also returns r and (pad_w, pad_h). */
int aic_letterbox(int device, const uint8_t* frame_bgr, int h, int w, int out_h, int out_w,
                  float* out_nchw, float* ratio, float* pad_w, float* pad_h);
/* letterbox() itself, any mode (image_processing.py:7-70: auto / scaleFill / scaleup / color): the caller works out the
 * geometry the mode produces (:33-67, host integer logic) and this resamples the frame to unpad_h x unpad_w (cv2.resize
 * INTER_LINEAR, :64) and surrounds it with the constant border (cv2.copyMakeBorder, :68).
 * out: u8 BGR HWC [(unpad_h + top + bottom), (unpad_w + left + right), 3], caller-owned. */
int aic_letterbox_image(int device, const uint8_t* frame_bgr, int h, int w, int unpad_h, int unpad_w, int top, int bottom,
                        int left, int right, int color_b, int color_g, int color_r, uint8_t* out_bgr);
/* _extract_image_crops + preprocess_reid_input (src/tracker/deepsort_tracker.py:143-159,
 * image_processing.py:105-138): int-truncate + clamp boxes, bilinear resize to out_h x out_w,
 * BGR->RGB, (x/255-mean)/std, NCHW. valid[i]=0 for empty crops (their tensor is zero). */
int aic_crop_resize(int device, const uint8_t* frame_bgr, int h, int w, const float* boxes_xyxy,
                    int n, int out_h, int out_w, float* out_nchw, int32_t* valid);

/* YOLODetector.detect (src/detector/yolo_detector.py:68-149) for a batch of same-size frames:
 * letterbox -> engine -> decode+NMS -> score filter -> scale_bboxes
 * (image_processing.py:141-183). boxes are xyxy in original-frame pixels, clipped.
 * Outputs are host arrays num_dets[B], boxes_xyxy[B,max_det,4], scores[B,max_det], labels[B,max_det].  At every batch size the call
 * writes num_dets[b] and the first min(num_dets[b], max_det) rows of frame b; rows past a frame's count are left as the caller
 * passed them.  aic_detect_decode, aic_detect_live and aic_yolo_infer with host outputs follow the same contract.
 * The result depends on the arguments only: every call uploads the frames it is handed, and no frame that this or another handle
 * was handed earlier is ever used in their place, however alike the two are. */
int aic_detect(aic_model* yolo, const uint8_t* frames_bgr, int batch, int h, int w, int mem,
               float conf_thresh, float iou_thresh, int max_det, int32_t* num_dets, float* boxes_xyxy,
               float* scores, int32_t* labels);
/* Decode + NMS of the last aic_detect run again, at another threshold, on what that run left on the device (no conv runs): the outputs
 * aic_detect would have given at these thresholds for frames 0 .. batch-1 of that run (frames of h x w). */
int aic_detect_decode(aic_model* yolo, int batch, int h, int w, float conf_thresh, float iou_thresh, int max_det,
                      int32_t* num_dets, float* boxes_xyxy, float* scores, int32_t* labels);
/* Tests: aic_detect with a device-side frame count holding n_live in force, as launches sized for a bound run (ConvArgs::n_dev):
 * frames at and past n_live are not computed and their outputs are left as the caller passed them. */
int aic_detect_live(aic_model* yolo, const uint8_t* frames_bgr, int batch, int n_live, int h, int w, int mem,
                    float conf_thresh, float iou_thresh, int max_det, int32_t* num_dets, float* boxes_xyxy,
                    float* scores, int32_t* labels);

/* crop -> ReID engine (deepsort_tracker.py:104-113 + reid_model.py:67-126) for one frame.  The result depends on the arguments only:
 * the crops come from frame_bgr as handed to this call, never from a frame an earlier call (aic_detect on the same frame a moment
 * before, say) left on the device. */
int aic_reid_embed(aic_model* reid, const uint8_t* frame_bgr, int h, int w, int mem,
                   const float* boxes_xyxy, int n, float* embeddings, int32_t* valid);

/* Parity-test entry points of the crop resamplers (tests/test_gpu_crop_paths.py); no production path goes through them.
 * Both stage a bank of frames [n_frames, h, w, 3] (host) byte_offset (0..3) bytes into a device buffer filled with a non-zero byte,
 * frame_of[n] (may be NULL: frame 0; checked against the bank on the host) and, when n_live >= 0, a device-side crop count holding
 * n_live (n_live < 0: none).
 * aic_crop_resize_ex: the crop kernel in any of its layouts -- mode 0: fp32 [n, 3, out_h, out_w]; mode 1: [n, out_h, out_w, 8] of
 * dtype; mode 2: fp16 [n, out_h, out_w, 4] (fp32 is refused with AIC_ERR_INVALID).  slack != 0: 16 readable bytes follow the bank and
 * the kernel takes its aligned 12-byte loads.  out is prefilled with 0xFF bytes and valid with -1: what the kernel does not store shows. */
int aic_crop_resize_ex(int device, const uint8_t* frames_bgr, int n_frames, int h, int w, int byte_offset, const float* boxes_xyxy,
                       const int32_t* frame_of, int n, int n_live, int out_h, int out_w, int mode, int dtype, int slack, void* out,
                       int32_t* valid);
/* aic_reid_embed_bank: one run of an fp16 ReID engine whose fused stem resamples the crops itself, set up as the pipeline's
 * device-filtered round sets it up (frames, boxes, frame_of, crop validity, device-side count).  AIC_ERR_INVALID for an engine that
 * would not take the fused crop or n > max_items.  The stem's pooled tensor stays in the engine (aic_model_read_buffer); rows at and
 * beyond n_live are not computed.  valid is prefilled with -1. */
int aic_reid_embed_bank(aic_model* reid, const uint8_t* frames_bgr, int n_frames, int h, int w, int byte_offset,
                        const float* boxes_xyxy, const int32_t* frame_of, int n, int n_live, float* embeddings, int32_t* valid);
/* Tests: aic_reid_infer for one group of n <= max_items crops with a device-side count holding n_live in force for the run, as the
 * pipeline's device-filtered round sets it: every launch is sized for n, the kernels that read the count leave items at and past
 * min(n_live, n) alone (n_live > n is allowed: the pipeline's count exceeds the bound in an overflow round).  Only the first
 * min(n_live, n) embeddings are copied out; the rest of `embeddings` is left as the caller filled it.  AIC_ERR_INVALID for
 * n > max_items or n_live < 0.  The activations stay in the engine (aic_model_read_buffer). */
int aic_reid_infer_live(aic_model* m, const float* crops_nchw, int n, int n_live, int mem, float* embeddings, int out_mem);

/* ------------------------------------------------------------------ Kalman filter (batched)
 * KalmanFilter.initiate/predict/project/update/gating_distance
 * (src/tracker/core/kalman_filter.py:55-83,85-120,122-151,153-204,206-249), n independent
 * filters per launch. mean[n,8], cov[n,8,8], z[n,4] fp32 host arrays. */
int aic_kf_initiate(int device, const float* z, int n, float* mean, float* cov);
int aic_kf_predict(int device, float* mean, float* cov, int n);
/* the same with the time step of KalmanFilter(dt) (kalman_filter.py:34-44: fp32(dt) on the position/velocity diagonal of the
 * motion matrix); aic_kf_predict is dt = 1, the only value the reference's tracker uses (tracker_core.py:30). */
int aic_kf_predict_dt(int device, float* mean, float* cov, int n, float dt);
int aic_kf_project(int device, const float* mean, const float* cov, int n, float* pmean, float* pcov);
int aic_kf_update(int device, float* mean, float* cov, const float* z, int n);
/* d2[n,m]: squared Mahalanobis distance of filter i to measurement zs[i*m+j] (shared_z=0) or
 * zs[j] (shared_z=1); +inf where S is not positive definite (kalman_filter.py:241-247). */
int aic_kf_gating(int device, const float* mean, const float* cov, int n, const float* zs, int m,
                  int shared_z, int only_position, float* d2);

/* ------------------------------------------------------------------ association costs
 * iou_cost (src/tracker/core/matching.py:13-106): 1-IoU[T,N] of tlwh boxes. */
int aic_iou_cost(int device, const float* track_tlwh, int t, const float* det_tlwh, int n, float* cost);
/* appearance_cost_metric + cosine_distance (matching.py:109-217): galleries[T,gmax,dim] with
 * gallery_len[T] valid rows each, det_feat[N,dim], has_feat[N]; cost[T,N] = min over gallery of
 * max(0, 1 - cos), INFTY_COST (1e5) where the gallery is empty or the detection has no feature. */
int aic_appearance_cost(int device, const float* galleries, const int32_t* gallery_len, int t,
                        int gmax, int dim, const float* det_feat, const uint8_t* has_feat, int n,
                        float* cost);

/* scipy.optimize.linear_sum_assignment as called at
 * src/tracker/core/linear_assignment.py:62 (SciPy 1.15.3, rectangular shortest augmenting
 * path, same tie-breaking). HOST code. row_ind/col_ind hold min(nr,nc) entries. */
int aic_lsap(const double* cost, int nr, int nc, int64_t* row_ind, int64_t* col_ind);
/* min_cost_matching on a precomputed fp32 cost block (linear_assignment.py:55-88): clamp
 * cost>max to max+1e-5, LSAP, accept iff cost<=max. HOST code. Outputs index into rows/cols. */
int aic_min_cost_matching(const float* cost, int nr, int nc, double max_distance, int32_t* match_row,
                          int32_t* match_col, int32_t* n_match);

/* matching_cascade + the IoU stage of TrackerCore._match (linear_assignment.py:91-157, tracker_core.py:83-177) on the
 * full cost matrices of one frame: app/maha/iou[T,N] (appearance cost, squared Mahalanobis distance, 1-IoU), state[T]
 * (1 tentative, 2 confirmed) and time_since_update[T] after predict().  HOST code.  Outputs: matches as (track index,
 * detection index) in the reference's order, unmatched tracks, unmatched detections; capacities min(T,N), T, N. */
int aic_match_cascade(const float* app, const float* maha, const float* iou, int t, int n, const int32_t* state,
                      const int32_t* time_since_update, double max_cosine_distance, double max_iou_distance,
                      int max_age, int32_t* match_track, int32_t* match_det, int32_t* n_match,
                      int32_t* unmatched_tracks, int32_t* n_unmatched_tracks, int32_t* unmatched_dets,
                      int32_t* n_unmatched_dets);

/* The same cascade run by the DEVICE association kernels (csrc/kernels_trk_dev.hip: wave-parallel restatement of the same
 * SciPy LSAP, preceded by a unique-optimum check that reads the answer off the matrix when it is the only optimum) on one
 * frame's matrices; at most 512 x 512.  flags: bit 0 = appearance stage alone, bit 1 = every problem through the LSAP (no
 * unique-optimum check).  match_det_of_track[T]: the detection each track got, or -1.  n_fast_lsap (may be NULL): [0] =
 * assignment problems settled by the check, [1] = by the LSAP.  Parity-test entry point of SURVEY.md §8(f)-4. */
int aic_match_cascade_device(int device, const float* app, const float* maha, const float* iou, int t, int n,
                             const int32_t* state, const int32_t* time_since_update, double max_cosine_distance,
                             double max_iou_distance, int max_age, int flags, int32_t* match_det_of_track,
                             int32_t* n_fast_lsap);

/* The epoch prep kernel of the device association alone (csrc/kernels_trk_dev.hip), on caller-provided tables: test entry point.
 * streams = 0: the single tracker's launch on rows [0, stream_dn[0]) of feat_n[rows, dim]; streams = S >= 1: the bank launch, stream s
 * reading rows row_map[...] (the streams' maps one behind the other, stream_dn[s] entries each) and skipped when has_sm[s] = 0.  Per
 * stream: n_tracks[s] tracks, track i = slot_glen_ghead[s][i][3] (gallery slot, length, ring head) into gal_n[s][cap][gmax][dim] (unit
 * rows).  dn_pad: pitch the tables are sized for (a multiple of 32, >= every stream's padded row count; streams = 0: equal to it).
 * Outputs, filled with -1 where the kernel writes nothing: sm[s][cap][17][dn_pad] and gram[s][dn_pad][dn_pad] floats, a stream's own
 * tables at its own padded pitch from the start of its slice. */
int aic_trk_prep_test(int device, int streams, int cap, const int32_t* n_tracks, const int32_t* slot_glen_ghead,
                      const float* gal_n, int gmax, int dim, const float* feat_n, int rows, const int32_t* stream_dn,
                      const int32_t* row_map, const int32_t* has_sm, int k, int dn_pad, float* sm, float* gram);

/* ------------------------------------------------------------------ tracker
 * TrackerCore (src/tracker/core/tracker_core.py:11-198) + Track lifecycle
 * (src/tracker/core/track.py:16-171).  Kalman state and feature galleries live in HBM;
 * lifecycle counters and the matching cascade run on the host. */
typedef struct aic_tracker_params {
    double max_cosine_distance; /* 0.2  src/config.py:23 (a Python float: kept in fp64)  */
    double max_iou_distance;    /* 0.7  src/config.py:26 */
    int32_t nn_budget;         /* 100  src/config.py:29; <=0 means unlimited up to capacity */
    int32_t max_age;           /* 70   src/config.py:27 */
    int32_t n_init;            /* 3    src/config.py:28 */
    int32_t max_tracks;        /* slot capacity (0 -> 512) */
    int32_t feature_dim;       /* 0 -> fixed by the first update */
    int32_t first_track_id;    /* 1    src/tracker/core/track.py:21 (per tracker) */
} aic_tracker_params;

int aic_tracker_create(int device, const aic_tracker_params* p, aic_tracker** out);
int aic_tracker_destroy(aic_tracker* t);
/* "device_assoc" = 1: predict/update run the whole frame (gating, cascade, LSAP, lifecycle, Kalman update) on the device,
 * the track table stays in HBM between calls (what the pipeline does k frames per launch); 0 (default for this entry
 * point): cost matrices on the device, cascade/LSAP/lifecycle in host C++.  Same results either way.
 * "lsap_fast" = 0: every assignment problem of the device path goes through the wave LSAP (default 1: unique optima are read
 * off the matrix).  "epoch_frames" = 1..16: frames per epoch launch of the device path (0 = default 16). */
int aic_tracker_option(aic_tracker* t, const char* key, int value);
/* TrackerCore.predict (tracker_core.py:44-49). */
int aic_tracker_predict(aic_tracker* t);
/* TrackerCore.update (tracker_core.py:51-81) on N detections: tlwh[N,4], conf[N], class id[N],
 * feat[N,dim] (host or device), has_feat[N] (NULL = all). */
int aic_tracker_update(aic_tracker* t, const float* det_tlwh, const float* conf, const int32_t* cls,
                       const float* feat, int feat_mem, const uint8_t* has_feat, int n, int dim);
/* k consecutive frames in ONE call, each a TrackerCore.predict() + TrackerCore.update() (tracker_core.py:44-49, 51-81), run
 * as epochs of the device association (csrc/kernels_trk_dev.hip; frames per epoch: aic_tracker_option "epoch_frames", default
 * 16) -- the pipeline's per-launch-group association with the embeddings supplied by the caller.  counts[k]; the rows of all
 * frames concatenated: det_tlwh[sum,4], conf[sum], class id[sum], feat[sum,dim] (host or device), has_feat[sum] (NULL = all).
 * Per frame (any may be NULL): n_out[k] confirmed tracks updated in the frame (true count), out6[k,cap_rows,6] + out_conf[k,
 * cap_rows] as aic_tracker_outputs; n_match[k], match_track_id / match_det [k,cap_rows] as aic_tracker_last_matches.  n_out and
 * n_match are the TRUE counts: only the first cap_rows rows / matches of a frame are stored, a caller compares the counts with
 * cap_rows to see a clipped frame.  Device
 * path only (nn_budget > 0, max_tracks <= 512, dim % 4 == 0): AIC_ERR_INVALID otherwise.  Same results as k predict/update calls. */
int aic_tracker_update_batch(aic_tracker* t, int k, const int32_t* counts, const float* det_tlwh, const float* conf,
                             const int32_t* cls, const float* feat, int feat_mem, const uint8_t* has_feat, int dim,
                             int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf, int32_t* n_match,
                             int32_t* match_track_id, int32_t* match_det);
/* Confirmed tracks updated this frame, formatted as deepsort_tracker.py:126-141:
 * out[k] = {x1,y1,x2,y2 (round-half-even ints), track_id, class_id}, conf[k]. */
int aic_tracker_outputs(aic_tracker* t, int32_t* out6, float* conf, int cap, int32_t* n_out);
int aic_tracker_num_tracks(const aic_tracker* t, int32_t* n);
/* Attribute surface of Track for callers/tests (track.py): per live track, in list order.
 * Any pointer may be NULL. mean[T,8], cov[T,8,8] are fetched from HBM. */
int aic_tracker_export(aic_tracker* t, int cap, int32_t* track_id, int32_t* state, int32_t* hits,
                       int32_t* age, int32_t* time_since_update, int32_t* cls, float* conf,
                       int32_t* gallery_len, float* mean, float* cov);
/* Gallery of live track `index` in FIFO order (track.py:70-74): out[gallery_len, dim]. */
int aic_tracker_export_gallery(aic_tracker* t, int index, float* out, int cap_rows);
/* The id the next new track will get (Track._next_id, track.py:21; per tracker here). */
int aic_tracker_next_track_id(aic_tracker* t, int32_t* next_id);
/* Inverse of aic_tracker_export + aic_tracker_export_gallery ("export / import of tracker state"): replaces the
 * whole state of TrackerCore.tracks (tracker_core.py:28) by n tracks in list order -- the arrays of aic_tracker_export, the
 * galleries of all tracks concatenated in FIFO order [sum(gallery_len), dim], and the next track id.  A tracker that
 * imports another's export continues exactly as the exporter would have (checkpoint / resume, moving a stream between GPUs).
 * Every argument is checked before the old state is touched. */
int aic_tracker_import_state(aic_tracker* t, int n, const int32_t* track_id, const int32_t* state, const int32_t* hits,
                             const int32_t* age, const int32_t* time_since_update, const int32_t* cls, const float* conf,
                             const int32_t* gallery_len, const float* mean, const float* cov, const float* galleries,
                             int dim, int next_track_id);
/* Device association: assignment problems (one per cascade level + the IoU stage) settled by the unique-optimum check /
 * solved by the wave LSAP since the tracker was created.  Either pointer may be NULL. */
int aic_tracker_assoc_counters(aic_tracker* t, int64_t* n_unique, int64_t* n_lsap);
/* (track_id, detection index) pairs of the last update, and its full cost matrices [T,N]
 * (appearance, squared Mahalanobis, 1-IoU), T = tracks alive before the update. */
int aic_tracker_last_matches(aic_tracker* t, int32_t* track_id, int32_t* det, int cap, int32_t* n);
int aic_tracker_last_costs(aic_tracker* t, float* app, float* maha, float* iou, int cap, int32_t* t_n,
                           int32_t* d_n);

/* A bank of `streams` (1..256) DeepSORT streams on one device: every epoch launch of the device association runs one kernel block per
 * stream (csrc/deepsort_bank.hpp, csrc/kernels_trk_dev.hip).  Each stream has its own track table, Kalman state, galleries and ids
 * (from first_track_id) and computes exactly what an aic_tracker with "device_assoc" fed the same frames computes.  Device association
 * only: AIC_ERR_INVALID (checked before the device) for streams outside 1..256, nn_budget <= 0, max_tracks > 512 (0 = 512) or a
 * feature_dim that is no multiple of 4 in 0..1024 (0 = 512).  Resident memory per stream: 2 * max_tracks * nn_budget * feature_dim * 4
 * bytes of galleries (210 MB at 512 x 100 x 512) + 340 * max_tracks bytes; an allocation that does not fit fails the create. */
int aic_deepsort_bank_create(int device, const aic_tracker_params* p, int streams, aic_deepsort_bank** out);
int aic_deepsort_bank_destroy(aic_deepsort_bank* b);
/* "epoch_frames" (0..16, 0 = 16), "lsap_fast" (0/1), "wave_cascade" (0/1), for the whole bank: same results either way. */
int aic_deepsort_bank_option(aic_deepsort_bank* b, const char* key, int value);
/* frames_per_stream[streams] consecutive frames of every stream (0 = none this call), F frames in all, stream-major: counts[F] and the
 * rows of all frames concatenated as aic_tracker_update_batch takes them (det_tlwh[sum,4], conf[sum], class id[sum], feat[sum,
 * feature_dim] raw host embeddings for all rows of the call or NULL, valid[sum]: 0 = the row has no feature, NULL = all have one).  One
 * staging upload, ceil(max frames / k) launches of `streams` blocks, one read-back, one sync.  n_out[F] (true counts), out6[F,cap_rows,6],
 * out_conf[F,cap_rows] as aic_tracker_update_batch.  A frame with more than 512 detections rejects the whole call before anything is
 * staged (AIC_ERR_CAPACITY).  A stream that exhausts max_tracks stops alone: status[streams] (may be NULL) gets 0 or the code that
 * stopped the stream, the frames before the failing one are delivered, the other streams complete, and later calls deliver nothing
 * for it until aic_deepsort_bank_reset.  With status NULL the call returns the first stopped stream's code after delivering the rest. */
int aic_deepsort_bank_update(aic_deepsort_bank* b, const int32_t* frames_per_stream, const int32_t* counts, const float* det_tlwh,
                             const float* conf, const int32_t* cls, const float* feat, const int32_t* valid, int cap_rows,
                             int32_t* n_out, int32_t* out6, float* out_conf, int32_t* status);
/* The stream as after create: no tracks, empty galleries, ids from first_track_id again, a stop cleared. */
int aic_deepsort_bank_reset(aic_deepsort_bank* b, int stream);
/* The arrays of aic_tracker_export for one stream (the first `cap` tracks; *n_tracks = the true count) and of
 * aic_tracker_export_gallery; AIC_ERR_INVALID for a stopped stream. */
int aic_deepsort_bank_export(aic_deepsort_bank* b, int stream, int cap, int32_t* track_id, int32_t* state, int32_t* hits,
                             int32_t* age, int32_t* time_since_update, int32_t* cls, float* conf, int32_t* gallery_len,
                             float* mean, float* cov, int32_t* n_tracks);
int aic_deepsort_bank_export_gallery(aic_deepsort_bank* b, int stream, int index, float* out, int cap_rows);
/* As aic_tracker_assoc_counters for one stream, since create or the stream's last reset. */
int aic_deepsort_bank_counters(aic_deepsort_bank* b, int stream, int64_t* n_unique, int64_t* n_lsap);

/* ------------------------------------------------------------------ ByteTrack
 * BYTETracker.update() of the ByteTrack authors (yolox/tracker/byte_tracker.py, matching.py) on the device, k frames per launch
 * (csrc/kernels_bytetrack.hip; specification: tests/bytetrack_oracle.py, deviations: DESIGN.md "ByteTrack").  No appearance model.
 * Defaults are ByteTrack's MOT17 settings; every threshold is rounded to fp32 once. */
typedef struct aic_bytetrack_params {
    double track_thresh;     /* 0.5: high band s > track_thresh                                          */
    double low_thresh;       /* 0.1: second band low_thresh < s < track_thresh                            */
    double new_track_thresh; /* a new track needs s >= this; 0 -> track_thresh + 0.1                      */
    double match_thresh;     /* 0.8: first association                                                    */
    int32_t track_buffer;    /* 30                                                                        */
    int32_t frame_rate;      /* 30: max_time_lost = int(frame_rate / 30 * track_buffer)                   */
    int32_t fuse_score;      /* 1 (= not mot20): IoU distance fused with the detection score               */
    int32_t max_tracks;      /* live tracks (0 -> 512, at most 512)                                       */
    int32_t first_track_id;  /* 1: ids are counted per tracker                                            */
} aic_bytetrack_params;

/* AIC_ERR_INVALID for a threshold outside (0, 1], low_thresh >= track_thresh, max_tracks over 512, ... (checked before the device). */
int aic_bytetrack_create(int device, const aic_bytetrack_params* p, aic_bytetrack** out);
int aic_bytetrack_destroy(aic_bytetrack* t);
/* "lsap_fast" = 0: every assignment problem goes through the wave LSAP (default 1: a unique optimum is read off the costs);
 * "epoch_frames" = 1..16: frames per epoch launch (0 = default 16).  Same results either way. */
int aic_bytetrack_option(aic_bytetrack* t, const char* key, int value);
/* k consecutive frames, each one BYTETracker.update(): counts[k]; the rows of all frames concatenated: boxes_xyxy[sum,4], conf[sum],
 * class id[sum].  Per frame (any may be NULL): n_out[k] output tracks (the TRUE count), out6[k,cap_rows,6] = {x1,y1,x2,y2
 * (round-half-even ints), track_id, class_id} + out_conf[k,cap_rows] (the track's score), as aic_tracker_update_batch.
 * AIC_ERR_CAPACITY when a frame has more than 512 detections, the live tracks outgrow max_tracks, or an assignment problem's extended
 * side (tracks + detections) exceeds 512; nothing is dropped, and the tracker refuses further updates after such an error. */
int aic_bytetrack_update_batch(aic_bytetrack* t, int k, const int32_t* counts, const float* boxes_xyxy, const float* conf,
                               const int32_t* cls, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf);
/* Live tracks in list order (the tracked list, then the lost list): state 1 Tracked / 2 Lost, start / end frame (end = the last
 * frame the track was updated), mean[n,8], cov[n,8,8].  n_tracks = all live tracks, n_tracked = the length of the tracked list; only the
 * first `cap` are stored.  Any pointer may be NULL. */
/* Assignment problems since creation settled by the unique-optimum check / by the wave LSAP, and the largest extended side met. */
int aic_bytetrack_counters(aic_bytetrack* t, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side);
/* After an update failed (AIC_ERR_CAPACITY) the tracker has no consistent state: export fails with AIC_ERR_INVALID. */
int aic_bytetrack_export(aic_bytetrack* t, int cap, int32_t* track_id, int32_t* state, int32_t* is_activated, int32_t* start_frame,
                         int32_t* end_frame, int32_t* cls, float* score, float* mean, float* cov, int32_t* n_tracks,
                         int32_t* n_tracked);

/* A bank: `streams` (1..256) independent ByteTrack streams on one device, e.g. the cameras of one installation.  Every epoch launch runs
 * one kernel block per stream, so a tick of all cameras costs one staging upload, one launch and one sync instead of `streams` of each.
 * Parameters and first_track_id apply to every stream (ids are counted per stream); each stream computes exactly what an aic_bytetrack
 * fed the same frames computes.  AIC_ERR_INVALID for streams outside 1..256 and as aic_bytetrack_create (checked before the device). */
int aic_bytetrack_bank_create(int device, const aic_bytetrack_params* p, int streams, aic_bytetrack_bank** out);
int aic_bytetrack_bank_destroy(aic_bytetrack_bank* b);
/* "lsap_fast", "epoch_frames" as aic_bytetrack_option, for the whole bank. */
int aic_bytetrack_bank_option(aic_bytetrack_bank* b, const char* key, int value);
/* frames_per_stream[streams] consecutive frames of every stream (0 and more than 16 are fine), F in all, stream-major: stream 0's frames,
 * then stream 1's, ...  counts[F], the detection arrays and the per-frame outputs n_out[F], out6[F,cap_rows,6], out_conf[F,cap_rows] are as
 * aic_bytetrack_update_batch.  A negative count or more than 512 detections in a frame rejects the whole call before anything is launched.
 * A stream that meets a capacity error is stopped alone: its frames from the failing one on (and every frame handed to it later) get
 * n_out = 0, the other streams' frames are processed.  status[streams] non-NULL: the call returns AIC_OK and status holds 0 or the error
 * code per stream; status NULL: the call returns the code of the lowest failing stream that was handed frames (the message names it). */
int aic_bytetrack_bank_update(aic_bytetrack_bank* b, const int32_t* frames_per_stream, const int32_t* counts, const float* boxes_xyxy,
                              const float* conf, const int32_t* cls, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf,
                              int32_t* status);
/* The stream as after create (no tracks, ids from first_track_id again), a stop cleared: a camera reconnecting. */
int aic_bytetrack_bank_reset(aic_bytetrack_bank* b, int stream);
/* As aic_bytetrack_export / aic_bytetrack_counters for one stream; export fails with AIC_ERR_INVALID for a stopped stream only. */
int aic_bytetrack_bank_export(aic_bytetrack_bank* b, int stream, int cap, int32_t* track_id, int32_t* state, int32_t* is_activated,
                              int32_t* start_frame, int32_t* end_frame, int32_t* cls, float* score, float* mean, float* cov,
                              int32_t* n_tracks, int32_t* n_tracked);
int aic_bytetrack_bank_counters(aic_bytetrack_bank* b, int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side);

/* ------------------------------------------------------------------ OC-SORT
 * OCSort.update() of the OC-SORT authors (ocsort.py, association.py, kalmanfilter.py) on the device, k frames per launch
 * (csrc/kernels_ocsort.hip; specification: tests/ocsort_oracle.py, deviations: DESIGN.md "OC-SORT").  No appearance model: SORT's 7-state
 * filter on [x, y, s, r], the velocity-direction term (OCM), the last-observation stage (OCR) and the virtual-trajectory replay (ORU).
 * Defaults are upstream's; every threshold is rounded to fp32 once. */
typedef struct aic_ocsort_params {
    double det_thresh;      /* 0.6: a detection takes part with s > det_thresh                            */
    double iou_threshold;   /* 0.3: a pair needs IoU >= this                                               */
    double inertia;         /* 0.2: weight of the velocity-direction term (OCM); 0 switches it off          */
    int32_t max_age;        /* 30: a track is removed at time_since_update > max_age                       */
    int32_t min_hits;       /* 3: output needs hit_streak >= min_hits (or frame <= min_hits)               */
    int32_t delta_t;        /* 3 (1..8): the observation the velocity direction is taken from               */
    int32_t use_byte;       /* 0; 1: a BYTE stage on the band 0.1 < s < det_thresh                          */
    int32_t max_tracks;     /* live tracks (0 -> 512, at most 512)                                         */
    int32_t first_track_id; /* 1: ids are counted per tracker                                              */
} aic_ocsort_params;

/* AIC_ERR_INVALID for a threshold outside (0, 1], inertia outside [0, 1], delta_t outside 1..8, max_tracks over 512, use_byte with
 * det_thresh <= 0.1, ... (checked before the device). */
int aic_ocsort_create(int device, const aic_ocsort_params* p, aic_ocsort** out);
int aic_ocsort_destroy(aic_ocsort* t);
/* "lsap_fast" = 0: stage 1 never takes upstream's read-off, every problem goes through the wave LSAP (default 1; the two are specified
 * separately, tests/ocsort_oracle.py change 10); "epoch_frames" = 1..16: frames per epoch launch (0 = default 16), same results. */
int aic_ocsort_option(aic_ocsort* t, const char* key, int value);
/* k consecutive frames, each one OCSort.update(): arrays and outputs as aic_bytetrack_update_batch; the rows are the tracks' last
 * observations, in upstream's order (the track list reversed).  AIC_ERR_CAPACITY when a frame has more than 512 detections or the live
 * tracks outgrow max_tracks; nothing is dropped, and the tracker refuses further updates after such an error. */
int aic_ocsort_update_batch(aic_ocsort* t, int k, const int32_t* counts, const float* boxes_xyxy, const float* conf,
                            const int32_t* cls, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf);
/* Live tracks in list order: counters of KalmanBoxTracker, frozen = the filter is frozen (the next observation replays the virtual
 * trajectory), has_obs, score, last_observation[n,4] (xyxy, -1 before the first), velocity[n,2] (dy, dx), mean[n,7], cov[n,7,7].  Only the
 * first `cap` are stored; any pointer may be NULL.  After an update failed the tracker has no consistent state: AIC_ERR_INVALID. */
int aic_ocsort_export(aic_ocsort* t, int cap, int32_t* track_id, int32_t* age, int32_t* hits, int32_t* hit_streak,
                      int32_t* time_since_update, int32_t* cls, int32_t* frozen, int32_t* has_obs, float* score,
                      float* last_observation, float* velocity, float* mean, float* cov, int32_t* n_tracks);
/* Since creation: stage-1 problems settled by the read-off / problems solved by the wave LSAP, the largest side the LSAP met, ORU replays
 * and their longest gap, pairs made by the OCR stage and by the BYTE stage. */
int aic_ocsort_counters(aic_ocsort* t, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_oru, int32_t* max_gap,
                        int64_t* n_ocr, int64_t* n_byte);

/* A bank of `streams` (1..256) OC-SORT streams: every call as its aic_bytetrack_bank_* counterpart, per-stream arrays as aic_ocsort_*. */
int aic_ocsort_bank_create(int device, const aic_ocsort_params* p, int streams, aic_ocsort_bank** out);
int aic_ocsort_bank_destroy(aic_ocsort_bank* b);
int aic_ocsort_bank_option(aic_ocsort_bank* b, const char* key, int value);
int aic_ocsort_bank_update(aic_ocsort_bank* b, const int32_t* frames_per_stream, const int32_t* counts, const float* boxes_xyxy,
                           const float* conf, const int32_t* cls, int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf,
                           int32_t* status);
int aic_ocsort_bank_reset(aic_ocsort_bank* b, int stream);
int aic_ocsort_bank_export(aic_ocsort_bank* b, int stream, int cap, int32_t* track_id, int32_t* age, int32_t* hits, int32_t* hit_streak,
                           int32_t* time_since_update, int32_t* cls, int32_t* frozen, int32_t* has_obs, float* score,
                           float* last_observation, float* velocity, float* mean, float* cov, int32_t* n_tracks);
int aic_ocsort_bank_counters(aic_ocsort_bank* b, int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_oru,
                             int32_t* max_gap, int64_t* n_ocr, int64_t* n_byte);

/* ------------------------------------------------------------------ BoT-SORT
 * BoTSORT.update() with ReID of the BoT-SORT authors (tracker/bot_sort.py, matching.py, kalman_filter.py) on the device, k frames per
 * launch (csrc/kernels_botsort.hip; specification: tests/botsort_oracle.py, deviations: DESIGN.md section 18): ByteTrack's bands and life
 * cycle, a Kalman filter on [cx, cy, w, h], one exponentially smoothed appearance vector per track, and a first association on
 * min(IoU distance, gated cosine distance / 2).  Camera motion is an input (a 2x3 affine per frame): aic_gmc_estimate_batch below
 * estimates it on the device, and a BoT-SORT pipeline does so itself with the option "gmc".
 * Defaults are upstream's; every threshold is rounded to fp32 once. */
typedef struct aic_botsort_params {
    double track_high_thresh; /* 0.6: high band s > track_high_thresh (only these detections carry a feature)     */
    double track_low_thresh;  /* 0.1: low band track_low_thresh < s < track_high_thresh                             */
    double new_track_thresh;  /* 0.7: a new track needs s >= this                                                   */
    double match_thresh;      /* 0.8: first association                                                             */
    double proximity_thresh;  /* 0.5: appearance is ignored for a pair with IoU distance above this (before fusion) */
    double appearance_thresh; /* 0.25: appearance is ignored for a pair with cosine distance / 2 above this          */
    double feat_alpha;        /* 0.9: smooth <- alpha smooth + (1 - alpha) feature, renormalised                     */
    int32_t track_buffer;     /* 30                                                                                 */
    int32_t frame_rate;       /* 30: max_time_lost = int(frame_rate / 30 * track_buffer)                            */
    int32_t fuse_score;       /* 1: IoU distance fused with the detection score                                      */
    int32_t with_reid;        /* 1; 0: features are ignored, the cost is the IoU distance                            */
    int32_t feature_dim;      /* 0 -> 512; a multiple of 4, at most 4096                                            */
    int32_t max_tracks;       /* live tracks (0 -> 512, at most 512)                                                */
    int32_t first_track_id;   /* 1: ids are counted per tracker                                                     */
} aic_botsort_params;

/* AIC_ERR_INVALID for a threshold outside (0, 1], track_low_thresh >= track_high_thresh, feat_alpha outside [0, 1), feature_dim not a
 * multiple of 4, max_tracks over 512, ... (checked before the device). */
int aic_botsort_create(int device, const aic_botsort_params* p, aic_botsort** out);
int aic_botsort_destroy(aic_botsort* t);
/* "lsap_fast" and "epoch_frames" as aic_bytetrack_option.  Same results either way. */
int aic_botsort_option(aic_botsort* t, const char* key, int value);
/* k consecutive frames, each one BoTSORT.update(): arrays and outputs as aic_bytetrack_update_batch, plus feat[sum, feature_dim] raw
 * embeddings (normalised on the device; NULL = no features, the call then runs as with_reid = 0), valid[sum] (0 = the row has no
 * feature; NULL = all have one) and warps[k, 6] (per frame r00 r01 t0 r10 r11 t1; NULL = no camera motion).  A feat row that does not
 * normalise to finite values in every element (a zero row, an inf or a NaN in it) is a row without a feature, as if valid were 0: it is
 * never compared, never enters a track's smoothed feature and does not set has_feat, and its detection still matches by IoU.  The
 * output rows are ALL tracks of the tracked list, as upstream.  Errors as aic_bytetrack_update_batch. */
int aic_botsort_update_batch(aic_botsort* t, int k, const int32_t* counts, const float* boxes_xyxy, const float* conf,
                             const int32_t* cls, const float* feat, const int32_t* valid, const float* warps, int cap_rows,
                             int32_t* n_out, int32_t* out6, float* out_conf);
/* Live tracks as aic_bytetrack_export (mean = [cx, cy, w, h, v...]) plus has_feat[n] and smooth_feat[n, feature_dim] (zeros without). */
int aic_botsort_export(aic_botsort* t, int cap, int32_t* track_id, int32_t* state, int32_t* is_activated, int32_t* start_frame,
                       int32_t* end_frame, int32_t* cls, float* score, float* mean, float* cov, int32_t* has_feat, float* smooth_feat,
                       int32_t* n_tracks, int32_t* n_tracked);
/* As aic_bytetrack_counters, plus the matched pairs (first association and unconfirmed tracks) whose winning term was the appearance
 * distance (d_emb < d_iou), and two shader-clock totals since creation: the appearance pass of the fused cost (the dot products) and
 * the whole epoch kernel.  The counts are 64-bit on the device as well. */
int aic_botsort_counters(aic_botsort* t, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side, int64_t* n_appearance,
                         int64_t* cost_cycles, int64_t* kernel_cycles);

/* A bank of `streams` (1..256) BoT-SORT streams: every call as its aic_bytetrack_bank_* counterpart.  Each stream has its own table,
 * smoothed features (max_tracks * feature_dim floats, allocated for `streams`) and ids, and computes exactly what an aic_botsort fed the
 * same frames computes.  AIC_ERR_INVALID for streams outside 1..256 and as aic_botsort_create (checked before the device). */
int aic_botsort_bank_create(int device, const aic_botsort_params* p, int streams, aic_botsort_bank** out);
int aic_botsort_bank_destroy(aic_botsort_bank* b);
int aic_botsort_bank_option(aic_botsort_bank* b, const char* key, int value);
/* As aic_bytetrack_bank_update (frames_per_stream[streams], F frames in all, stream-major; status[streams] and the per-stream failure
 * contract), plus, as aic_botsort_update_batch: feat[sum, feature_dim] for all rows of the call or NULL, valid[sum] or NULL, and
 * warps[F, 6] (one row per frame of the call, in the frames' order) or NULL.  The features are normalised once over all rows. */
int aic_botsort_bank_update(aic_botsort_bank* b, const int32_t* frames_per_stream, const int32_t* counts, const float* boxes_xyxy,
                            const float* conf, const int32_t* cls, const float* feat, const int32_t* valid, const float* warps,
                            int cap_rows, int32_t* n_out, int32_t* out6, float* out_conf, int32_t* status);
/* The stream as after create: no tracks, no smoothed features, ids from first_track_id again, a stop cleared. */
int aic_botsort_bank_reset(aic_botsort_bank* b, int stream);
/* As aic_botsort_export / aic_botsort_counters for one stream; export fails with AIC_ERR_INVALID for a stopped stream only. */
int aic_botsort_bank_export(aic_botsort_bank* b, int stream, int cap, int32_t* track_id, int32_t* state, int32_t* is_activated,
                            int32_t* start_frame, int32_t* end_frame, int32_t* cls, float* score, float* mean, float* cov,
                            int32_t* has_feat, float* smooth_feat, int32_t* n_tracks, int32_t* n_tracked);
int aic_botsort_bank_counters(aic_botsort_bank* b, int stream, int64_t* n_fast, int64_t* n_lsap, int32_t* max_side,
                              int64_t* n_appearance, int64_t* cost_cycles, int64_t* kernel_cycles);

/* ------------------------------------------------------------------ camera motion
 * The 2x3 affine of the camera motion between consecutive frames (previous-frame pixel coordinates -> current-frame ones, the `warps` of
 * aic_botsort_update_batch), estimated on the device (csrc/kernels_gmc.hip; specification: tests/gmc_oracle.py):
 * a gray pyramid level, integer block matching (16 x 16 blocks, +-8 gray pixels, SAD) with an integer sub-pixel step, and a robust
 * least-squares similarity from exact integer sums.  Deterministic: equal inputs give equal bits.  Working range per frame: a
 * translation below 8 * downscale pixels, about 1.4 degrees of rotation or 2.5 % of zoom; beyond it the identity is returned. */
typedef struct aic_gmc_params {
    int32_t downscale;   /* 2 or 4 (0 -> 4): frame pixels per gray pixel and side */
    int32_t min_inliers; /* 0 -> 8: fewer agreeing blocks give the identity       */
} aic_gmc_params;

/* AIC_ERR_INVALID for a downscale other than 0, 2, 4, a negative min_inliers, a frame smaller than one block plus its search margin
 * (32 * downscale pixels a side) or one with more than 2048 blocks (checked before the device). */
int aic_gmc_create(int device, int height, int width, const aic_gmc_params* p, aic_gmc** out);
int aic_gmc_destroy(aic_gmc* g);
/* Forget the previous frame: the next frame is a stream's first. */
int aic_gmc_reset(aic_gmc* g);
/* k consecutive u8 BGR frames [k, height, width, 3] in host or device memory (mem: AIC_HOST / AIC_DEVICE).  Frame f takes frame f - 1
 * of the call as its predecessor, frame 0 the last frame of the call before.  counts[k] and boxes_xyxy[sum, 4] (host memory; both may be
 * NULL) are the detection boxes of each frame: blocks under them are left out.  warps_out[k, 6] (r00 r01 t0 r10 r11 t1) and
 * stats_out[k, 4] (ok, blocks, blocks that entered the fit, inliers of the last fit) are host memory; either may be NULL.  A stream's
 * first frame, and a frame whose motion could not be estimated, get the identity and ok = 0. */
int aic_gmc_estimate_batch(aic_gmc* g, const uint8_t* frames_bgr, int k, int mem, const int32_t* counts, const float* boxes_xyxy,
                           float* warps_out, int32_t* stats_out);

/* A bank: the estimator of `streams` (1..256) cameras of one frame size whose frames come tick-major (frame t * streams + s = tick t of
 * camera s); aic_gmc is the bank of one.  AIC_ERR_INVALID as aic_gmc_create and for streams outside 1..256 (checked before the device). */
int aic_gmc_bank_create(int device, int height, int width, const aic_gmc_params* p, int streams, aic_gmc_bank** out);
int aic_gmc_bank_destroy(aic_gmc_bank* b);
/* Forget camera `stream`'s previous frame: its next frame is its first (identity, every block skipped). */
int aic_gmc_bank_reset(aic_gmc_bank* b, int stream);
/* `ticks` ticks of every camera: ticks * streams frames, counts, warps_out and stats_out rows, tick-major, otherwise as
 * aic_gmc_estimate_batch.  A frame's predecessor is the same camera's frame of the tick before (of the call before for tick 0). */
int aic_gmc_bank_estimate(aic_gmc_bank* b, const uint8_t* frames_bgr, int ticks, int mem, const int32_t* counts, const float* boxes_xyxy,
                          float* warps_out, int32_t* stats_out);

/* ------------------------------------------------------------------ end-to-end pipeline
 * The loop body of src/aicamera_tracker.py:169-207 (detect + track, the reference's own FPS
 * span) over frames that are already resident in HBM, batched: detection and ReID of
 * `batch` frames per launch group, association strictly frame by frame. */
typedef struct aic_pipeline_params {
    int32_t frame_h, frame_w;
    int32_t batch;          /* frames per detection/ReID launch group                    */
    int32_t ring_frames;    /* frames kept resident in HBM                                */
    int32_t max_persons;    /* rows per frame in the caller's track arrays; also sizes the crop buffers a launch
                             * group starts with (they grow: EVERY detection that passes the filter of
                             * deepsort_tracker.py:88-101 is embedded and tracked, none is dropped)      */
    float conf_thresh;      /* 0.3 src/config.py:17 */
    float iou_thresh;       /* 0.5 src/config.py:18 (unused by the reference, F4)        */
    int32_t max_det;        /* 300 (build decision D4)                                    */
    float min_confidence;   /* 0.3 src/config.py:24 */
    int32_t inject;         /* 1: association consumes injected boxes         */
    uint64_t track_class_mask[2]; /* bit c set = class id c is tracked (config.py:53)    */
    aic_tracker_params tracker;
} aic_pipeline_params;

int aic_pipeline_create(aic_model* yolo, aic_model* reid, const aic_pipeline_params* p,
                        aic_pipeline** out);
/* A detector-only pipeline with ByteTrack as its tracker (no ReID engine): launch groups run upload -> letterbox -> detector -> NMS ->
 * class-mask filter -> ByteTrack epochs on the tracker stream; crop, ReID and embedding copies are not issued.  inject = 1 feeds the
 * planted boxes, inject = 0 the detector's detections filtered by track_class_mask only (min_confidence and p->tracker are ignored: the
 * ByteTrack bands filter the scores, so conf_thresh should be at most low_thresh).  run / run_passes / run_from_host(_passes) and the
 * per-frame outputs behave as for DeepSORT.  aic_pipeline_tracker, the embedding read-backs, the gallery exchange and the options
 * "device_assoc", "device_assoc_limit", "device_filter" fail with AIC_ERR_INVALID on such a pipeline. */
int aic_pipeline_create_bytetrack(aic_model* yolo, const aic_pipeline_params* p, const aic_bytetrack_params* bp,
                                  aic_pipeline** out);
/* The same detector-only pipeline with OC-SORT as its tracker.  Rejections as on a ByteTrack pipeline; conf_thresh should be at most
 * det_thresh (0.1 with use_byte). */
int aic_pipeline_create_ocsort(aic_model* yolo, const aic_pipeline_params* p, const aic_ocsort_params* op,
                               aic_pipeline** out);
/* BoT-SORT as the pipeline's tracker, WITH the ReID engine: stage A as for DeepSORT with the host detection filter (crop + ReID for every
 * detection handed to the tracker; the embeddings stay in HBM and reach the epoch kernel directly), stage B as on a ByteTrack pipeline.
 * inject = 0 hands over the detections of a tracked class with score > track_low_thresh (min_confidence and p->tracker are ignored, so
 * conf_thresh should be at most track_low_thresh).  No camera-motion warp unless the option "gmc" is set (below).  bp->feature_dim must
 * be the ReID engine's output size.
 * aic_pipeline_last_embeddings / _group_embeddings work; aic_pipeline_tracker, the gallery exchange and the options "device_assoc",
 * "device_assoc_limit", "device_filter" fail with AIC_ERR_INVALID. */
int aic_pipeline_create_botsort(aic_model* yolo, aic_model* reid, const aic_pipeline_params* p, const aic_botsort_params* bp,
                                aic_pipeline** out);
/* A BoT-SORT pipeline for `streams` (1..256) cameras, fixed at creation (the smoothed features and the camera-motion estimator are sized
 * by it): the tracker is a BoT-SORT bank as above, ids per camera from bp->first_track_id, the ring and every run range are tick-major as with
 * the option "streams", and `batch` and `ring_frames` must be multiples of `streams`.  With the option "gmc" the estimator is a bank of
 * `streams` and aic_pipeline_group_warps returns the group's rows in slot order.  aic_pipeline_reset_stream works; the option "streams"
 * does not (AIC_ERR_INVALID, as on aic_pipeline_create_botsort). */
int aic_pipeline_create_botsort_bank(aic_model* yolo, aic_model* reid, const aic_pipeline_params* p, const aic_botsort_params* bp,
                                     int streams, aic_pipeline** out);
/* A DeepSORT pipeline for `streams` (1..256) cameras, fixed at creation: the tracker is a DeepSORT bank (aic_deepsort_bank_create) with
 * p->tracker as its parameters -- its create-time rejections apply: nn_budget > 0, max_tracks <= 512 -- feature_dim being the ReID
 * engine's output width (0, or that width), and every camera's ids starting at first_track_id.  The ring and every run range are
 * tick-major as with the option "streams"; `batch` and `ring_frames` must be multiples of `streams`.  Stage A is the DeepSORT pipeline's
 * (with inject = 0 the detection filter on the device and the device-sized ReID round, option "device_filter"); boxes and embeddings
 * stay in HBM and the group's association runs in one epoch-kernel block per camera.  There is no host association chain: a frame with
 * more than 512 detections fails the run call with AIC_ERR_CAPACITY before the group's association is launched.
 * A camera that exhausts max_tracks stops alone: the run call delivers the group's rows -- none for that camera from its failing frame
 * on, all of the other cameras', whose state is that after the group -- and returns AIC_ERR_CAPACITY at that launch group, naming the
 * camera; frames of later groups of the call are not processed.  Further run calls fail with AIC_ERR_INVALID until
 * aic_pipeline_reset_stream(p, camera).
 * aic_pipeline_reset_stream, aic_pipeline_link_cameras, aic_pipeline_group_embeddings / _last_embeddings and the option "epoch_frames"
 * work.  aic_pipeline_tracker, the gallery exchange and the options "device_assoc", "device_assoc_limit", "streams" and "gmc" fail with
 * AIC_ERR_INVALID. */
int aic_pipeline_create_deepsort_bank(aic_model* yolo, aic_model* reid, const aic_pipeline_params* p, int streams, aic_pipeline** out);
/* The bank of a pipeline from aic_pipeline_create_deepsort_bank, owned by the pipeline (do not destroy): aic_deepsort_bank_export,
 * _export_gallery, _counters and _option work on it between run calls -- the bank counterpart of aic_pipeline_tracker.
 * AIC_ERR_INVALID on any other pipeline. */
int aic_pipeline_deepsort_bank(aic_pipeline* p, aic_deepsort_bank** out);
int aic_pipeline_destroy(aic_pipeline* p);
/* Copy `count` u8 BGR frames into ring slots [slot, slot+count). */
int aic_pipeline_upload(aic_pipeline* p, int slot, const uint8_t* frames_bgr, int count);
/* Planted detections for ring slots (inject=1): counts[count], boxes[count,max_persons,4] ... */
int aic_pipeline_inject(aic_pipeline* p, int slot, int count, const int32_t* counts,
                        const float* boxes_xyxy, const float* conf, const int32_t* cls);
/* Process ring slots [slot, slot+count) in order. Per frame outputs (any may be NULL):
 * n_tracks[count] (the true number of confirmed tracks of the frame; when it exceeds max_persons only the first
 * max_persons rows are stored), tracks[count,max_persons,6] + track_conf as aic_tracker_outputs;
 * n_dets[count], det_boxes[count,max_det,4], det_scores, det_labels from the detector: the first min(n_dets, max_det) rows of a
 * frame, rows past a frame's count are left as the caller passed them (as aic_detect). */
int aic_pipeline_run(aic_pipeline* p, int slot, int count, int32_t* n_tracks, int32_t* tracks6,
                     float* track_conf, int32_t* n_dets, float* det_boxes, float* det_scores,
                     int32_t* det_labels);
/* The range [slot, slot+count) walked `passes` times back to back as one continuous stream (a looped clip): one call,
 * one pipeline fill and one un-overlapped tracker tail for passes*count frames; rows of a later pass overwrite the
 * earlier ones. bench.py's timed region is one such call with passes = K steps. */
int aic_pipeline_run_passes(aic_pipeline* p, int slot, int count, int passes, int32_t* n_tracks, int32_t* tracks6,
                            float* track_conf, int32_t* n_dets);
/* Same, but the frames of this call come from HOST memory (the reference's cap.read() buffers,
 * src/aicamera_tracker.py:170): each launch group's frames are copied into ring slots [slot, slot+count) on a copy
 * stream while the previous group computes. Pin the buffer once with aic_host_register for full PCIe rate. */
int aic_pipeline_run_from_host(aic_pipeline* p, const uint8_t* frames_bgr, int slot, int count, int32_t* n_tracks,
                               int32_t* tracks6, float* track_conf, int32_t* n_dets);
/* The host clip walked `passes` times as one continuous stream (bench.py's timed region: the reference's own span --
 * frame bytes in host memory -> track tuples on the host, src/aicamera_tracker.py:170-207 with yolo_detector.py:91's
 * .to(device) inside). */
int aic_pipeline_run_from_host_passes(aic_pipeline* p, const uint8_t* frames_bgr, int slot, int count, int passes,
                                      int32_t* n_tracks, int32_t* tracks6, float* track_conf, int32_t* n_dets);
/* Launch groups of the last call: frames, wall-clock second at which the group was handed to the pipeline (its H2D /
 * first launch enqueued) and at which its track tuples were on the host. done - submit = latency of every frame of the group. */
int aic_pipeline_group_times(aic_pipeline* p, int32_t* frames, double* submit_s, double* done_s, int cap, int32_t* n);
/* configs[4] of BASELINE.json -- optional cross-camera ReID gallery exchange (not in the reference: README.md:210 lists it
 * as future work; SURVEY.md §8e fixes its form).  enable: every `every_groups` launch groups the pipeline packs, on its tracker
 * stream, a shard fp32 [t_max, 2 + dim] (valid, track id, unit embedding of the newest gallery row) of the stream's first t_max
 * confirmed tracks into the caller's device buffers (two, alternating).  A consumer thread then calls wait(seq) -- blocks
 * until shard `seq` is packed, returns its buffer index and makes the exchange stream (exchange_stream: a hipStream_t the
 * caller runs its RCCL all-gather on, e.g. through torch.cuda.ExternalStream) wait for the pack kernel -- and done(seq) once
 * the collective has consumed the buffer.  shard0_dev = NULL disables.  Two buffers alternate: the stream's association waits
 * only when the consumer is two exchanges behind, and then for at most 60 s (AICAM_XCHG_WAIT_S) before the call fails with
 * AIC_ERR_RUNTIME -- a stuck peer ends the run loudly, it does not hang it. */
int aic_pipeline_exchange_enable(aic_pipeline* p, float* shard0_dev, float* shard1_dev, int t_max, int every_groups);
int aic_pipeline_exchange_stream(aic_pipeline* p, void** stream);
int aic_pipeline_exchange_wait(aic_pipeline* p, int64_t seq, int timeout_ms, int32_t* buffer, int32_t* ready);
int aic_pipeline_exchange_done(aic_pipeline* p, int64_t seq);
/* The annotation pass on an all-gathered set of shards ("consumed read-only by an extra cosine_min_gallery pass"):
 * gathered_dev = fp32 [world, t_max, 2 + dim] in HBM, `stream` = the hipStream_t to run on (the exchange stream; NULL = the
 * device's tracker stream), synchronised before returning.  Host outputs over ALL world * t_max rows (any may be NULL):
 * track_id[i] (-1 = slot empty), near_row[i] = the valid row of ANOTHER rank closest in cosine distance (ties: lowest row; -1 =
 * none), near_dist[i]; annotation[t_max, 3] = (rank, track id, distance) for this rank's rows where that distance is within
 * max_cosine_distance, else -1.  d(i, j) == d(j, i) bit for bit, so every rank derives the same table from the same bytes. */
int aic_gallery_annotate(int device, void* stream, const float* gathered_dev, int world, int rank, int t_max, int dim,
                         double max_cosine_distance, int32_t* track_id, int32_t* near_row, float* near_dist,
                         float* annotation);
/* Cross-camera global-ID policy on top of it (README.md:209 "smarter gallery management in ReID"; BASELINE.json configs[4]).
 * HOST code (csrc/global_id.cpp).  A track's global id is the (rank << 32 | track id) of the first sighting of its identity:
 * new tracks get their own, and two tracks of different cameras that are each other's nearest neighbour within the threshold
 * adopt the smaller of their global ids (transitively).  update() takes the arrays of aic_gallery_annotate; every rank feeds
 * it the same gathered data and therefore holds the same table -- no further communication.  lookup(): -1 = never seen. */
typedef struct aic_gid aic_gid;
int aic_gid_create(int world, aic_gid** out);
int aic_gid_destroy(aic_gid* g);
int aic_gid_update(aic_gid* g, int world, int t_max, const int32_t* track_id, const int32_t* near_row, const float* near_dist,
                   double max_cosine_distance, int32_t* n_links);
int aic_gid_lookup(aic_gid* g, int rank, int track_id, int64_t* global_id);
int aic_gid_size(aic_gid* g, int64_t* n_tracks, int64_t* n_identities, int64_t* n_links);
/* The rank's local track ids start over (a camera reset): its (rank, track id) keys of now must not be met again.  Every rank carries a
 * generation in the key's free upper bits (generation << 44 | rank << 32 | track id; rank takes 12 bits, generation 0 keys are the keys
 * above): sightings from here on are filed under the next generation and lookup() resolves the current generation only (-1 until the
 * recycled id is seen again).  Identities that other ranks adopted from the forgotten one keep their number.  The keys of earlier
 * generations stay in the table (ids merged into them must still resolve), so aic_gid_size / aic_xcam_size count forgotten tracks too
 * and the table grows by a camera's tracks with every reconnect, as it grows with every new track id on the rank path. */
int aic_gid_forget_rank(aic_gid* g, int rank);

/* ------------------------------------------------------------------ cross-camera identities inside one bank
 * The same answer for the cameras of ONE process: is this track of stream 3 the one stream 11 sees?  An aic_xcam holds the global-id
 * table above with world = streams and runs, per link call, one device pass on the tracker stream between the bank's update calls:
 * every stream's shard (valid, track id, unit embedding; fp32 [streams, t_max, 2 + dim]; the valid rows of a stream are a prefix of its
 * slice) is packed on the device, every live row's nearest row of another stream is found by a tiled all-pairs kernel whose cost follows
 * the live rows (same arithmetic, same bits as aic_gallery_annotate), the tables are read back once and the policy is applied on the
 * host.  The bank's own association never reads the result.
 * create: streams 1..256, t_max 1..512 (rows per stream: the first t_max eligible tracks in list order), dim a multiple of 4 in 4..1024.
 * link_deepsort_bank: rows = confirmed tracks with a gallery, the newest gallery entry's unit row.  link_botsort_bank: activated tracks
 * of the tracked list that have a feature, the smoothed unit feature.  AIC_ERR_INVALID before the device is touched when the bank's
 * stream count or feature dimension differs from the object's or when a stream is stopped by an error (reset it first);
 * AIC_ERR_CAPACITY when a packed track id is >= 2^24 (ids travel as fp32).  *n_links = identities merged by this call.
 * link_shards: the same pass on caller-made shards in host or device memory (mem: AIC_HOST / AIC_DEVICE; device memory 8-byte aligned).
 * The valid prefix of every stream is counted from the valid column on the device, and shards whose valid rows are not a prefix are
 * rejected with AIC_ERR_INVALID.  n_valid[streams] (host; may be NULL) is the caller's statement of those counts: a value outside
 * 0..t_max, or one that differs from the valid column, is AIC_ERR_INVALID and nothing is linked (host memory: before the device is
 * touched; device memory: after the pass's read-back, before the policy).
 * tables: the last pass's arrays over all streams * t_max rows, as aic_gallery_annotate's (any may be NULL).  shards: its shard array;
 * a row past a stream's valid prefix holds (0, 0) and the embedding an earlier pass of this object packed there, zeros before any did.
 * global_ids: -1 = never seen.  size: as aic_gid_size.  forget_stream: aic_gid_forget_rank for a camera that was reset.
 * option "tile": 32 / 64 = rows per tile of the nearest kernel, 0 (default) = by size; same results either way. */
typedef struct aic_xcam aic_xcam;
int aic_xcam_create(int device, int streams, int t_max, int dim, double max_cosine_distance, aic_xcam** out);
int aic_xcam_destroy(aic_xcam* x);
int aic_xcam_option(aic_xcam* x, const char* key, int value);
int aic_xcam_link_deepsort_bank(aic_xcam* x, aic_deepsort_bank* bank, int32_t* n_links);
int aic_xcam_link_botsort_bank(aic_xcam* x, aic_botsort_bank* bank, int32_t* n_links);
int aic_xcam_link_shards(aic_xcam* x, const float* shards, const int32_t* n_valid, int mem, int32_t* n_links);
int aic_xcam_tables(aic_xcam* x, int32_t* track_id, int32_t* near_row, float* near_dist);
int aic_xcam_shards(aic_xcam* x, float* out);
int aic_xcam_global_ids(aic_xcam* x, int stream, const int32_t* track_ids, int n, int64_t* global_ids);
int aic_xcam_size(aic_xcam* x, int64_t* n_tracks, int64_t* n_identities, int64_t* n_links);
int aic_xcam_forget_stream(aic_xcam* x, int stream);
/* The link pass for the bank of a pipeline from aic_pipeline_create_botsort_bank or aic_pipeline_create_deepsort_bank, between run
 * calls; AIC_ERR_INVALID on any other pipeline. */
int aic_pipeline_link_cameras(aic_pipeline* p, aic_xcam* x, int32_t* n_links);

/* ------------------------------------------------------------------ identity archive
 * The memory the link pass lacks: appearance rows of tracks that have ended, searched with int8 MFMA.  A row is known by an int64
 * key >= 0 (for bank rows the global-id key generation << 44 | stream << 32 | track id) and carries a camera and the ticks of its first
 * and last deposit.  Stored: int8 codes q_i = rint(v_i * (127 / m)), m = max |v_i|, half to even, and scale = m / 127; a distance is
 * max(+0, 1 - (float(dot) * scale_row) * scale_query) with the exact int32 dot of the codes; results are ranked by
 * (distance bits << 32 | slot).  The query is quantised the same way.
 *
 * aic_archive_index_*: the slot bookkeeping alone, HOST code, no device.  assign is an upsert of n keys at `tick`: a known key keeps its
 * slot and t_first; a new key takes the lowest free slot, or, when all `capacity` slots are taken, the slot of the smallest
 * (t_last, slot), whose key goes to evicted[i] (else -1).  Where one call names a slot twice the last row keeps it: the earlier rows get
 * slots[i] = -1.  find: -1 = unknown.  remove: *slot = the freed slot or -1.
 * aic_archive_*: create: capacity 1..2^24, dim a multiple of 4 in 4..1024 (checked before the device).  put: n fp32 rows [n, dim] in host
 * or device memory; a row that is all zero, holds a non-finite element or has no finite 127 / m fails the call with AIC_ERR_INVALID
 * and nothing of the call is stored.  search: n queries [n, dim], k in 1..32, filters[n] (NULL = none); outputs [n, k] on the host (any
 * may be NULL), missing places -1 / -1 / 1e5; one read-back, one synchronisation.  A slot is eligible when it is occupied,
 * camera != exclude_camera (-1 = none), t_lo <= t_last <= t_hi, key != exclude_key (-1 = none) and dist <= max_distance (fp32).
 * export: *n = the high-water mark; arrays [n] (rows [n, pitch], pitch = dim rounded up to 64), free slots have key -1; every array may
 * be NULL.  import replaces the contents with such arrays.  block_rows: the slots one block of a search of n_queries owns now. */
typedef struct aic_archive_filter {
    int32_t exclude_camera;
    float max_distance;
    int64_t t_lo, t_hi, exclude_key;
} aic_archive_filter;
typedef struct aic_archive_index aic_archive_index;
int aic_archive_index_create(int64_t capacity, aic_archive_index** out);
int aic_archive_index_destroy(aic_archive_index* ix);
int aic_archive_index_assign(aic_archive_index* ix, const int64_t* keys, const int32_t* cameras, int64_t tick, int n, int32_t* slots,
                             int64_t* evicted);
int aic_archive_index_find(aic_archive_index* ix, int64_t key, int32_t* slot);
int aic_archive_index_remove(aic_archive_index* ix, int64_t key, int32_t* slot);
int aic_archive_index_size(aic_archive_index* ix, int64_t* n_rows, int64_t* high_water);
typedef struct aic_archive aic_archive;
int aic_archive_create(int device, int64_t capacity, int dim, aic_archive** out);
int aic_archive_destroy(aic_archive* a);
int aic_archive_put(aic_archive* a, const int64_t* keys, const int32_t* cameras, int64_t tick, const float* rows, int n, int mem);
int aic_archive_remove(aic_archive* a, int64_t key);
int aic_archive_search(aic_archive* a, const float* queries, int n, int mem, int k, const aic_archive_filter* filters, int64_t* out_keys,
                       int32_t* out_slots, float* out_dist);
int aic_archive_size(aic_archive* a, int64_t* n_rows, int64_t* high_water);
int aic_archive_export(aic_archive* a, int64_t* keys, int32_t* cameras, int64_t* t_first, int64_t* t_last, float* scales, int8_t* rows,
                       int64_t* n);
int aic_archive_import(aic_archive* a, const int64_t* keys, const int32_t* cameras, const int64_t* t_first, const int64_t* t_last,
                       const float* scales, const int8_t* rows, int64_t n);
int aic_archive_clear(aic_archive* a);
int aic_archive_block_rows(aic_archive* a, int n_queries, int32_t* rows);
/* find_key: the global id of any filed key, whatever its rank's current generation (-1 = never filed).  link_keys: two filed keys become
 * one identity under the smaller root; *linked = 1 when that merged two identities.  AIC_ERR_INVALID for a key that was never filed. */
int aic_gid_find_key(aic_gid* g, int64_t key, int64_t* global_id);
int aic_gid_link_keys(aic_gid* g, int64_t key_a, int64_t key_b, int32_t* linked);
/* With an archive attached (same device, same dim), every link pass ends with three more steps at tick = passes so far: the pass's valid
 * rows whose key the archive does not hold are searched (k = 1, t_hi = tick - 1 - min_gap, max_distance = the object's threshold; the
 * queries stay on the device); where several name one archived row the smallest (distance bits, shard row) keeps it, and the winners'
 * keys are linked to the archived keys; then every valid row of the pass is deposited.  option "min_gap" (default 1, >= 0).  returning:
 * the last pass's winners, ascending shard row (*n = their number, at most cap are stored).  a == NULL detaches.  Attaching an archive that
 * holds rows of an earlier run (aic_archive_import) moves the tick behind their last deposit and starts every camera whose archived keys
 * the object never filed in a generation above them. */
int aic_xcam_attach_archive(aic_xcam* x, aic_archive* a);
int aic_xcam_returning(aic_xcam* x, int32_t* stream, int32_t* track_id, int64_t* archived_key, float* dist, int cap, int32_t* n);

/* ---- zone entries, dwell and line crossings per camera (csrc/zones.hpp) -------------------------------------
 * A tracker-agnostic stage over the rows every tracker delivers (x1 y1 x2 y2 id cls, int32).  `streams` (1..256) cameras, each with
 * up to 32 zones (simple polygons of 3..32 integer-pixel vertices, either winding) and 32 directed lines A->B, and a table of
 * max_tracks (1..512) slots; a track not seen for more than forget_after frames is forgotten.  anchor: 0 = the bottom centre of the
 * box, 1 = its centre.  All arithmetic is exact (doubled coordinates in int64); tests/zones_oracle.py is the specification.
 * Every argument error is AIC_ERR_INVALID before the device is touched: create, set, reset and option never touch it (the first
 * update does).  Coordinates of zones and lines outside +-2^20 are rejected; a row with a box coordinate outside it is ignored.
 * set: zone_nvert[n_zones], zone_xy = the zones' vertices one after another (x, y), line_xy[n_lines][4] = ax ay bx by; between
 * updates; the stream's state and counters start over; AIC_ERR_INVALID for a stopped stream (reset it first).
 * update: stream-major as the bank updates: frames_per_stream[streams], counts[F] rows per frame (F = the sum), rows6 [sum of
 * counts, 6] in host or device memory (mem: AIC_HOST / AIC_DEVICE).  A frame of more than 512 rows rejects the call with
 * AIC_ERR_CAPACITY before anything is staged.  Outputs (host): n_events[F] true counts, events[F, cap_events, 8] = kind (1 ENTER,
 * 2 EXIT, 3 LOST, 4 CROSS), zone / line index, track id, cls, frame, value (dwell in frames, or +-1 = the side of A->B the track ends
 * on), doubled anchor x, y; truncated at cap_events (0..65536), zero-filled; occupancy[F, 32].  A stream that needs more than
 * max_tracks slots stops alone: that frame and its later ones deliver nothing, status[streams] (may be NULL) gets 0 or
 * AIC_ERR_CAPACITY, the other streams finish, and later calls deliver nothing for it until aic_zones_reset.
 * counters: cumulative int64 [32] each (any may be NULL); they never depend on cap_events.
 * option "frames_per_launch": 0 (default) = a call's frames in one launch, k = at most k frames of a stream per launch; same results. */
typedef struct aic_zones aic_zones;
int aic_zones_create(int device, int streams, int max_tracks, int forget_after, int anchor, aic_zones** out);
int aic_zones_destroy(aic_zones* z);
int aic_zones_set(aic_zones* z, int stream, int n_zones, const int32_t* zone_nvert, const int32_t* zone_xy, int n_lines, const int32_t* line_xy);
int aic_zones_update(aic_zones* z, const int32_t* frames_per_stream, const int32_t* counts, const int32_t* rows6, int mem, int cap_events,
                     int32_t* n_events, int32_t* events, int32_t* occupancy, int32_t* status);
int aic_zones_counters(aic_zones* z, int stream, int64_t* zone_in, int64_t* zone_out, int64_t* line_pos, int64_t* line_neg);
int aic_zones_reset(aic_zones* z, int stream);
int aic_zones_option(aic_zones* z, const char* key, int value);

/* ---- privacy redaction, static masks and annotation of a bank of frames in one launch (csrc/render.hpp) -------
 * The output stage after the path: u8 BGR frames [n_frames, h, w, 3] of one size (h, w in 1..16384), the rows every tracker delivers
 * (x1 y1 x2 y2 id cls), per-frame primitive lists and per-camera mask polygons.  tests/render_oracle.py is the specification; the
 * device matches it bit for bit.  Per pixel, the first rule that applies, everything "original" read from the frame as handed in:
 *   (a) the colour of the LAST primitive of the frame's list that covers it.  prims [n, 8] as aic_overlay (kinds 0, 1, 2), and kind 3 =
 *       (3, ax, ay, bx, by, color, t, 0): a segment A->B of thickness t in 1..8.  dx = bx - ax, dy = by - ay; |dx| >= |dy| and dx != 0:
 *       hit iff min(ax, bx) <= x <= max(ax, bx) and 2 |dx (y - ay) - dy (x - ax)| <= t |dx|; |dy| > |dx|: the same with the axes
 *       exchanged; A == B draws nothing.  Text offsets index the call's one text buffer.  |coordinate| <= 2^20.
 *   (b) mask_color inside a mask polygon of the frame's camera (even-odd rule with half-open edges on the integer pixel (x, y)).
 *   (c) inside the union of the frame's redaction rectangles: fill_color (style 0), or (style 1, mosaic) the mean per channel of the
 *       original pixels of cell (x / cell, y / cell), grid anchored at the frame's origin, (sum + n / 2) / n over the n pixels the cell
 *       has inside the frame.
 *   (d) unchanged.
 * A row gives a rectangle: coordinates saturated to +-2^20, rows with x2 < x1 or y2 < y1 dropped; mode 1 (box) = (x1 - pad, y1 - pad,
 * x2 + pad, y2 + pad) inclusive, mode 2 (head) = the same x range, y from y1 - pad to y1 + (((y2 - y1) * head_q8) >> 8); mode 0 = none.
 * class_all 1 (default) redacts every row; after option "class_mask" (bit c = class c) only rows of those classes and rows whose cls
 * is outside 0..63 (an unknown class fails safe).
 * create, option, set_masks, rects and every argument error of frames never touch the device.
 * option keys: "mode" 0..2, "style" 0 / 1, "cell" 4 / 8 / 16 / 32, "fill_color", "mask_color" (B | G << 8 | R << 16), "pad" 0..4096,
 * "head_q8" 1..256, "class_mask", "class_all" 0 / 1, "chunk_frames" (0 = a call's frames in one device buffer, k = at most k frames per
 * upload, launch and download; same results).
 * set_masks: n_verts[n_polys] (n_polys in 0..32, 3..32 vertices each), xy = the vertices one after another (x, y).
 * rects: host only; rects4 [<= n_rows, 4] = x0 y0 x1 y1 the rows give under the current options, *n_rects their number.
 * frames: rows6 [sum of row_counts, 6] with row_counts[n_frames] (both may be NULL: no rows; at most 512 per frame, else
 * AIC_ERR_CAPACITY), prims [sum of prim_counts, 8] with prim_counts[n_frames] (may be NULL; at most 1500 per frame), cameras[n_frames]
 * (NULL: frame f is camera f % cameras).  Host frames (AIC_HOST) are uploaded, rendered and downloaded; device frames (AIC_DEVICE) are
 * rendered in place.  One stream synchronise ends the call. */
typedef struct aic_render aic_render;
int aic_render_create(int device, int cameras, aic_render** out);
int aic_render_destroy(aic_render* r);
int aic_render_option(aic_render* r, const char* key, int64_t value);
int aic_render_set_masks(aic_render* r, int camera, int n_polys, const int32_t* n_verts, const int32_t* xy);
int aic_render_rects(aic_render* r, const int32_t* rows6, int n_rows, int32_t* rects4, int* n_rects);
int aic_render_frames(aic_render* r, uint8_t* frames_bgr, int n_frames, int h, int w, int mem, const int32_t* rows6, const int32_t* row_counts,
                      const int32_t* prims, const int32_t* prim_counts, const uint8_t* text, int text_bytes, const int32_t* cameras);

/* ---- best shots: the best crop of every track, kept on the device, per camera (csrc/bestshot.hpp) -------------
 * A tracker-agnostic stage over u8 BGR frames of one size and the rows every tracker delivers (x1 y1 x2 y2 id cls, int32), for
 * `streams` (1..256) cameras per call.  Every counted row's region (box or head, the arithmetic of aic_render_rects, clipped to the
 * frame) is resampled to a thumb_h x thumb_w x 3 thumbnail by an integer area average and scored; a table of max_tracks slots per
 * stream keeps the best thumbnail per track id; a track unseen for more than forget_after ticks ENDS and is handed over with its shot.
 * tests/bestshot_oracle.py is the specification -- counted rows, candidates, the thumbnail, the score, the order of a tick, the
 * capacity rule -- and the device equals it bit for bit.
 * aic_bestshot_config: frame_h, frame_w in 1..16384; thumb_w in 16..128, thumb_h in 16..256, both multiples of 8; max_tracks 1..512; forget_after
 * 0..2^24; region 0 = box, 1 = head (head_q8 in 1..256); pad 0..64; min_w, min_h in 1..16384.  aic_bestshot_params fills the
 * documented defaults (64 x 128 thumbnails, 128 tracks, forget_after 70, box, head_q8 64, pad 0, min 8 x 16) around streams / frame size.
 * Every argument error is AIC_ERR_INVALID before the device is touched; create, option and reset never touch it.  The resident slot
 * thumbnails (streams * max_tracks * thumb_h * thumb_w * 3 bytes) are allocated by the first call that reaches the device; an
 * allocation that does not fit fails that call with AIC_ERR_CAPACITY.
 * update: `ticks` (0..65536) ticks; frames [ticks, streams, h, w, 3] tick-major in host or device memory (frames_mem); counts[ticks *
 * streams] and rows6 [sum of counts, 6] in the same order, both in host or both in device memory (rows_mem).  A frame of more than
 * 512 rows rejects the call with AIC_ERR_CAPACITY before anything is staged.  ticks = 0 only drains.  Outputs (host): n_final[streams],
 * events[streams, cap, 16] = reason (0 LIVE, 1 EXPIRED, 2 FLUSHED), stream, id, cls, first_frame, last_seen, sightings, has_shot,
 * best_frame, score, C.x0, C.y0, C.x1, C.y1, slot, 0; thumbs[streams, cap, thumb_h, thumb_w, 3] (only the n_final[s] first of a stream
 * are written); pending[streams] = ENDED slots still waiting for room; status[streams] (may be NULL) = 0 or the code the stream
 * stopped with.  cap in 0..4096 per stream per call; nothing is ever dropped.  A stream that needs more than max_tracks slots stops
 * alone with AIC_ERR_CAPACITY: that tick is not committed and later ticks deliver nothing until aic_bestshot_reset; export, flush and
 * a ticks = 0 drain still work.
 * flush: stream (or -1 = all) -- every live slot ENDS with reason FLUSHED, then the ENDED slots are emitted as by update.
 * export: every non-free slot of a stream in slot order (live ones with reason LIVE) into events[max_tracks, 16], thumbs[max_tracks,
 * ...]; changes nothing.  reset: the stream forgets everything, pending slots included; a stop is cleared.
 * option "ticks_per_launch": 0 (default) = as many ticks per launch as the budget allows, k = at most k; "launch_budget_mb" (1..65536,
 * default 1024): the candidate thumbnails and the staged frames of one launch each stay below it, one tick at the least; "stats" 0 / 1
 * (aic_bestshot_counters).  Same results. */
typedef struct aic_bestshot aic_bestshot;
typedef struct {
    int32_t streams, frame_h, frame_w, thumb_w, thumb_h, max_tracks, forget_after, region, head_q8, pad, min_w, min_h;
} aic_bestshot_config;
int aic_bestshot_params(int streams, int frame_h, int frame_w, aic_bestshot_config* out);
int aic_bestshot_create(int device, const aic_bestshot_config* params, aic_bestshot** out);
int aic_bestshot_destroy(aic_bestshot* b);
int aic_bestshot_option(aic_bestshot* b, const char* key, int value);
int aic_bestshot_reset(aic_bestshot* b, int stream);
int aic_bestshot_update(aic_bestshot* b, const uint8_t* frames_bgr, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6,
                        int rows_mem, int cap, int32_t* n_final, int32_t* events, uint8_t* thumbs, int32_t* pending, int32_t* status);
int aic_bestshot_flush(aic_bestshot* b, int stream, int cap, int32_t* n_final, int32_t* events, uint8_t* thumbs, int32_t* pending,
                       int32_t* status);
int aic_bestshot_export(aic_bestshot* b, int stream, int32_t* n, int32_t* events, uint8_t* thumbs);
/* After option "stats" 1 (0 = default): since creation, the rows handed to update, the candidates among them that were scored, and the
 * candidate thumbnails the could-still-win filter let through to the per-row buffer.  Any pointer may be NULL.  Host only. */
int aic_bestshot_counters(aic_bestshot* b, int64_t* rows, int64_t* candidates, int64_t* stored);
/* ---- scene watch: motion masks, an activity gate and tamper alarms per camera (csrc/scene.hpp) ----------------
 * A tracker-agnostic stage that looks at frames as scenes, for `streams` (1..256) cameras of one frame size per call.  Every u8 BGR
 * frame is reduced to a gray grid of cells of `cell` x `cell` pixels (cell 4, 8 or 16; the grid is frame_h / cell x frame_w / cell,
 * both >= 1, remainder rows and columns are not read); a per-cell background model (bg, dev in Q8, prev) marks the raw cells, a 3 x 3
 * vote cleans them, and per-stream counters turn the tick's statistics into the activity gate and five alarms.
 * tests/scene_oracle.py is the specification -- the order of a tick, every shift and threshold -- and the device equals it bit for bit.
 * Every argument error is AIC_ERR_INVALID before the device is touched; create, option and reset never touch it.  Device buffers are
 * allocated by the first call that reaches the device; an allocation that does not fit fails that call with AIC_ERR_CAPACITY.
 * update: `ticks` (0..65536) ticks; frames [ticks, streams, h, w, 3] tick-major in host or device memory (frames_mem), a device pointer
 * of any alignment.  counts (may be NULL: no rows) [ticks * streams] and rows6 [sum of counts, 6] = x1 y1 x2 y2 id cls in the same order,
 * both in host or both in device memory (rows_mem); a frame of more than 512 rows rejects the call with AIC_ERR_CAPACITY before anything
 * is staged.  Outputs (host): records [ticks, streams, 16] = frame, ready, active, n_moving, n_raw, x0, y0, x1, y1 (the clean cells' box
 * in pixels, x1 y1 exclusive, all -1 = none), mean_luma, sharp, ref_q8, n_changed, cond, alarms, edges (raised bits | cleared bits << 8;
 * bit 0 DARK, 1 BRIGHT, 2 DEFOCUS, 3 SCENE, 4 FROZEN); masks (may be NULL) [ticks, streams, grid_h, grid_w] u8, bit 0 clean, bit 1 raw;
 * row_motion (may be NULL) [sum of counts] = 256 * moving / covered cells of the row's box, -1 for an invalid or empty box.
 * reset: stream, or -1 = every stream, starts again at age 0.  export: bg, dev, prev as int32 [grid_h, grid_w] and scalars[16] = age,
 * quiet, ref_q8, alarms, on[5], off[5], 0, 0; changes nothing; all zeros for a stream that has seen no tick since create / reset.
 * option: thresh 0..255, noise_k_q4 0..4096, warmup 1..2^20, big_thresh 0..255, learn_shift 1..12, slow_extra 0..8 (their sum <= 14),
 * dev_init_q8 0..65280, min_neighbours 1..9, dark_luma 0..256, bright_luma 0..255, min_ref_q8 0..2^20, defocus_q8 0..256, scene_q16
 * 0..65536, ref_shift 1..12, hold 1..2^20, gate_cells 1..2^24, gate_hold 0..2^20 (defaults: DESIGN.md section 39); none of them sizes a
 * buffer, so they may change between calls.  "ticks_per_launch": 0 (default) = as many ticks per launch as the budget allows, k = at
 * most k; "launch_budget_mb" (1..65536, default 1024): the gray grids and the staged frames of one launch each stay below it, one tick
 * at the least.  Same results. */
typedef struct aic_scene aic_scene;
typedef struct {
    int32_t streams, frame_h, frame_w, cell;
} aic_scene_config;
int aic_scene_config_default(int streams, int frame_h, int frame_w, aic_scene_config* out);
int aic_scene_create(int device, const aic_scene_config* config, aic_scene** out);
int aic_scene_destroy(aic_scene* s);
int aic_scene_option(aic_scene* s, const char* key, int value);
int aic_scene_reset(aic_scene* s, int stream);
int aic_scene_update(aic_scene* s, const uint8_t* frames_bgr, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6,
                     int rows_mem, int32_t* records, uint8_t* masks, int32_t* row_motion);
int aic_scene_export(aic_scene* s, int stream, int32_t* bg, int32_t* dev, int32_t* prev, int32_t* scalars);
/* ---- left objects: abandoned and removed items per camera (csrc/left.hpp) ------------------------------------
 * A tracker-agnostic stage for `streams` (1..256) cameras of one frame size per call, on the gray grid of the scene watch (cell 4, 8 or
 * 16; a grid of more than 32768 cells is refused at create with AIC_ERR_CAPACITY).  Per cell a fast and a slow background (Q8), a
 * `still` counter and the last tracker id that covered it; the cells that stayed changed while nobody stood on them are candidates,
 * their 8-connected blobs (labelled by their smallest cell index y * grid_w + x) are matched from tick to tick against `max_objects`
 * (1..64) slots per stream, alarmed as LEFT or REMOVED after alarm_hold sightings and ended after gone_ticks misses.
 * tests/left_oracle.py is the specification -- the order of a tick, every shift and threshold -- and the device equals it bit for bit.
 * Every argument error is AIC_ERR_INVALID before the device is touched; create, option and reset never touch it.  Device buffers are
 * allocated by the first call that reaches the device; an allocation that does not fit fails that call with AIC_ERR_CAPACITY.
 * update: frames, counts, rows6 and their memory kinds as for aic_scene_update (counts NULL: no rows; a frame of more than 512 rows is
 * AIC_ERR_CAPACITY before anything is staged).  Outputs (host): records [ticks, streams, 8] = frame, ready, n_cand, n_blobs (kept, at
 * most 64), n_objects, n_alarmed, flags (bit 0: more than 64 blobs of a kept size, bit 1: blobs dropped for want of a slot), dropped;
 * objects [ticks, streams, max_objects, 12] = uid (0 = free slot, all zeros), kind (0, 1 LEFT, 2 REMOVED), alarmed, x0 y0 x1 y1 in
 * pixels (x1 y1 exclusive), owner (a tracker id or -1), born, area (cells), seen, missing; events [cap_events, 12] = tick of the call,
 * stream, type (1 APPEARED, 2 RAISED, 3 ENDED), uid, kind, x0 y0 x1 y1, owner, area, age, ordered by tick, stream, slot; *n_events = the
 * true count.  When it exceeds cap_events the first cap_events are delivered and the state has advanced all the same: *status (may be
 * NULL) = AIC_ERR_CAPACITY and the call returns AIC_OK, with status NULL the call returns AIC_ERR_CAPACITY.  cand (may be NULL) [ticks,
 * streams, grid_h, grid_w] u8; labels (may be NULL) the same shape in int32, -1 = no candidate (a blob of a size not kept has its label).
 * reset: stream, or -1 = every stream, starts again at age 0 with uids from 1.  export: fast, slow, still, last_id, last_tick as int32
 * [grid_h, grid_w], slots [max_objects, 12] as in objects, scalars[4] = age, uids issued, 0, 0; changes nothing; all zeros for a stream
 * that has seen no tick since create / reset.
 * option: fast_shift 1..8, slow_shift 1..12, thresh 1..255, warmup 1..2^20, decay 0..64, min_ticks 1..65534, absorb_ticks min_ticks + 1
 * ..65535, pad_cells 0..8, owner_window 0..2^20, min_cells 1..32768, max_cells min_cells..32768, alarm_hold 1..2^20, gone_ticks 0..2^20
 * (defaults: DESIGN.md section 44); none sizes a buffer.  "ticks_per_launch" and "launch_budget_mb" as for aic_scene_option. */
typedef struct aic_left aic_left;
typedef struct {
    int32_t streams, frame_h, frame_w, cell, max_objects;
} aic_left_config;
int aic_left_config_default(int streams, int frame_h, int frame_w, aic_left_config* out);
int aic_left_create(int device, const aic_left_config* config, aic_left** out);
int aic_left_destroy(aic_left* s);
int aic_left_option(aic_left* s, const char* key, int value);
int aic_left_reset(aic_left* s, int stream);
int aic_left_update(aic_left* s, const uint8_t* frames_bgr, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem,
                    int cap_events, int32_t* records, int32_t* objects, int32_t* events, int32_t* n_events, int32_t* status, uint8_t* cand,
                    int32_t* labels);
int aic_left_export(aic_left* s, int stream, int32_t* fast, int32_t* slow, int32_t* still, int32_t* last_id, int32_t* last_tick, int32_t* slots,
                    int32_t* scalars);
/* ---- clothing colours: what each track wears, per camera (csrc/colours.hpp) -----------------------------------
 * A tracker-agnostic stage over u8 BGR frames of one size and the rows every tracker delivers (x1 y1 x2 y2 id cls, int32), for
 * `streams` (1..256) cameras per call.  The pixels of a torso part and a legs part of every counted row's box (fractions torso0..torso1
 * and legs0..legs1 of its height in q8, inset by inset_q8 of its width on either side, clipped to the frame) are named with one of 12
 * colours (0 BLACK, GRAY, WHITE, RED, ORANGE, YELLOW, GREEN, CYAN, BLUE, PURPLE, PINK, 11 BROWN) and histogrammed; a part smaller than
 * min_w x min_h or covered by more than max_cover_q8 by one nearer box is not sampled.  A table of max_tracks slots per stream
 * accumulates every sample's shares (q8) per track id; a track unseen for more than forget_after ticks ENDS and is handed over as a
 * 48-int descriptor.  tests/colours_oracle.py is the specification -- valid and counted rows, the parts, the pixel rule, the order of a
 * tick, the capacity rule -- and the device equals it bit for bit.
 * aic_colours_config: frame_h, frame_w in 1..16384; max_tracks 1..512; forget_after 0..2^24; 0 <= torso0 < torso1 <= 256 and legs alike;
 * inset_q8 0..127; min_w, min_h in 1..16384; max_cover_q8 0..256.  aic_colours_config_default fills the documented defaults (128 tracks,
 * forget_after 70, torso 51..128, legs 141..230, inset 64, min 4 x 4, max_cover 64) around streams / frame size.
 * Every argument error is AIC_ERR_INVALID before the device is touched; create, option and reset never touch it.  Device buffers are
 * allocated by the first call that reaches the device; an allocation that does not fit fails that call with AIC_ERR_CAPACITY.
 * update: frames, counts, rows6, their memory kinds, ticks and cap as for aic_bestshot_update (a frame of more than 512 rows is
 * AIC_ERR_CAPACITY before anything is staged; ticks = 0 only drains).  Outputs (host): n_final[streams]; events[streams, cap, 48] =
 * reason (0 LIVE, 1 EXPIRED, 2 FLUSHED), stream, id, cls, first_frame, last_seen, sightings, samples_upper, samples_lower, top_upper,
 * second_upper, top_lower, second_lower, slot, 0, 0, hist_upper[12], hist_lower[12] (q8 shares, 0..256), 8 zeros -- top = the largest
 * bin (-1 without samples), second = the largest other bin with at least a quarter of it (else -1); only the n_final[s] first of a
 * stream are written; row_tags (may be NULL) [sum of counts, 4] = top_upper, top_lower and their shares from the row's slot after its
 * tick (-1 / 0 for a part without samples, four times -1 for a row not counted or of a stopped stream); pending[streams]; status[streams]
 * (may be NULL).  A stream that needs more than max_tracks slots stops alone with AIC_ERR_CAPACITY as a best-shot stream does.
 * flush, export (events[max_tracks, 48]), reset: as for aic_bestshot_*.  option "ticks_per_launch" and "launch_budget_mb" (the sampled
 * rows, 128 bytes each, and the staged frames of one launch each stay below it): same results.
 * aic_colours_classify (host only, no device): bins[i] = the colour of pixel bgr[3 i .. 3 i + 2], the rule the kernel applies. */
typedef struct aic_colours aic_colours;
typedef struct {
    int32_t streams, frame_h, frame_w, max_tracks, forget_after, torso0, torso1, legs0, legs1, inset_q8, min_w, min_h, max_cover_q8;
} aic_colours_config;
int aic_colours_config_default(int streams, int frame_h, int frame_w, aic_colours_config* out);
int aic_colours_create(int device, const aic_colours_config* config, aic_colours** out);
int aic_colours_destroy(aic_colours* c);
int aic_colours_option(aic_colours* c, const char* key, int value);
int aic_colours_reset(aic_colours* c, int stream);
int aic_colours_update(aic_colours* c, const uint8_t* frames_bgr, int frames_mem, int ticks, const int32_t* counts, const int32_t* rows6,
                       int rows_mem, int cap, int32_t* n_final, int32_t* events, int32_t* row_tags, int32_t* pending, int32_t* status);
int aic_colours_flush(aic_colours* c, int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status);
int aic_colours_export(aic_colours* c, int stream, int32_t* n, int32_t* events);
int aic_colours_classify(const uint8_t* bgr, int n, uint8_t* bins);
/* ---- heat maps: footfall, dwell, flow and paths per camera (csrc/heat.hpp) ---------------------------------------
 * A tracker-agnostic stage over the rows every tracker delivers (x1 y1 x2 y2 id cls, int32), for `streams` (1..256) cameras per call;
 * only render touches frames.  Every camera holds twelve int32 layers [GH, GW] over cells of cell x cell pixels (GW = ceil(frame_w /
 * cell), GH alike): 0 VISITS (a track entered the cell), 1 DWELL (a track stood in it, per tick), 2 STARTS, 3 ENDS (tracks first / last
 * seen there), 4..11 DIR0..DIR7 (steps of at least min_move doubled pixels by octant, clockwise from east, y down).  A counted row's
 * anchor is the middle of its bottom edge (anchor 0, foot) or of its box (1, centre) in doubled pixels, clamped into the frame.  A table
 * of max_tracks slots per stream remembers where each track stood last; a track unseen for more than forget_after ticks ENDS and is
 * handed over as a 16-int path summary.  ENDS is counted when the event leaves the table (so a track still `pending` is not in it yet).
 * Every layer cell and slot counter stops at 2^30.  tests/heat_oracle.py is the specification and the device equals it bit for bit.
 * aic_heat_config: frame_h, frame_w in 1..16384; cell 4, 8, 16 or 32; max_tracks 1..512; forget_after 0..2^24; anchor 0 / 1; min_move
 * 1..2^20; aic_heat_config_default fills cell 16, 128 tracks, forget_after 70, foot, min_move 4.  More than 32768 cells is
 * AIC_ERR_CAPACITY at create.  Resident memory: 48 bytes per cell and camera plus 32.8 KB of slot table per camera.
 * Every argument error is AIC_ERR_INVALID before the device is touched; create, option, reset, set_lut, lut and the range check of
 * import_layers never touch it.  Device buffers are allocated by the first call that reaches the device; an allocation that does not
 * fit fails that call with AIC_ERR_CAPACITY.
 * update: counts[ticks * streams] and rows6 (tick-major; both host or both device, rows_mem), ticks 0..65536 (0 only drains), cap
 * 0..4096; a frame of more than 512 rows is AIC_ERR_CAPACITY before anything is staged.  Outputs (host): n_final[streams];
 * events[streams, cap, 16] = reason (0 LIVE, 1 EXPIRED, 2 FLUSHED), stream, id, cls, first_frame, last_seen, sightings, cells, start_fx,
 * start_fy, end_fx, end_fy, path, max_step, moving, last cell (cy * GW + cx) -- only the n_final[s] first of a stream are written;
 * row_tags (may be NULL) [sum of counts, 4] = cell, ticks in that cell, step, octant or -1 for a counted row (-1, 0, 0, -1 for every
 * other row and for a stopped stream); pending[streams]; status[streams] (may be NULL).  A stream that needs more than max_tracks slots
 * stops alone with AIC_ERR_CAPACITY as a colour stream does, and that tick adds nothing to its layers.
 * flush, export (events[max_tracks, 16]), reset (the stream's table and layers): as for aic_colours_*.
 * decay: v >>= shift (1..31) on the layers of layer_mask (bit l = layer l) of one stream or of all (-1).  export_layers /
 * import_layers: int32 [popcount(layer_mask), GH, GW] of one stream, in layer order; import refuses a value outside 0..2^30 and takes
 * effect in call order, as a reset does.
 * render: n_frames (0..65536) BGR24 frames of frame_h x frame_w, packed, in host or device memory (mem; any alignment), changed in
 * place; frame f shows camera cameras[f] (NULL: f % streams).  The layer's cells become levels relative to the camera's maximum M
 * (M = 0: the camera's frames are untouched), are interpolated bilinearly between cell centres to L in 0..255, and a pixel with L >=
 * floor becomes (in * (256 - alpha_q8) + LUT[L] * alpha_q8 + 128) >> 8.  set_lut: 256 x 3 bytes BGR; aic_heat_lut (host only): the default.
 * option: "scale" (0 linear, 1 log, the default), "alpha_q8" (0..256, default 160), "floor" (0..255, default 8), "chunk_frames" (0 = a
 * call's frames at once, or at most k per upload / launch / download), "ticks_per_launch", "launch_budget_mb": same results. */
typedef struct aic_heat aic_heat;
typedef struct {
    int32_t streams, frame_h, frame_w, cell, max_tracks, forget_after, anchor, min_move;
} aic_heat_config;
int aic_heat_config_default(int streams, int frame_h, int frame_w, aic_heat_config* out);
int aic_heat_create(int device, const aic_heat_config* config, aic_heat** out);
int aic_heat_destroy(aic_heat* h);
int aic_heat_option(aic_heat* h, const char* key, int value);
int aic_heat_reset(aic_heat* h, int stream);
int aic_heat_update(aic_heat* h, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int32_t* n_final, int32_t* events,
                    int32_t* row_tags, int32_t* pending, int32_t* status);
int aic_heat_flush(aic_heat* h, int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status);
int aic_heat_export(aic_heat* h, int stream, int32_t* n, int32_t* events);
int aic_heat_decay(aic_heat* h, int stream, int layer_mask, int shift);
int aic_heat_export_layers(aic_heat* h, int stream, int layer_mask, int32_t* out);
int aic_heat_import_layers(aic_heat* h, int stream, int layer_mask, const int32_t* layers);
int aic_heat_set_lut(aic_heat* h, const uint8_t* bgr);
int aic_heat_lut(uint8_t* bgr);
int aic_heat_render(aic_heat* h, uint8_t* frames_bgr, int n_frames, int mem, const int32_t* cameras, int layer);
/* ---- proximity: ground plane, speed, pairs and parties per camera (csrc/prox.hpp) --------------------------------
 * A tracker-agnostic stage over the rows every tracker delivers (x1 y1 x2 y2 id cls, int32), for `streams` (1..256) cameras per call; no
 * frames.  A counted row (VALID, FIRST of its id, NONEMPTY, as for aic_heat_*) has the foot anchor fx = clamp(x1 + x2, 0, 2 W - 1), fy =
 * clamp(2 y2, 0, 2 H - 1) in doubled pixels and the height hc = clamp(y2 - y1, 1, 32767).  metric 0 (ground plane) places it at gx =
 * floor(((H0 fx + H1 fy + 2 H2) << shift) / den), gy from H3..H5, den = H6 fx + H7 fy + 2 H8, when den > 0 and |gx|, |gy| <= 2^24; with
 * |H[k]| <= 2^30 and shift <= 14 every intermediate fits int64 (|n| < 2^47, shifted < 2^61).  metric 1 (relative to body height) places
 * every counted row at (fx, fy).  Two placed rows are NEAR when dgx^2 + dgy^2 <= near^2 (metric 0), or when 256 max(hc) <=
 * height_ratio_q8 min(hc) and 1 000 000 (dfx^2 + dfy^2) <= near^2 (hc_i + hc_j)^2 (metric 1; all below 2^57).  A table of max_tracks
 * slots per stream holds each track's last place, its smoothed speed v_q8 (ground units, or per mille of body height, per tick; q8), its
 * gait (0 none yet, 1 still, 2 moving, 3 running), the distance it moved and its parties; a resident table holds linked / on / off /
 * since per PAIR of slots: a pair judged near link_ticks ticks in a row LINKS, a linked pair judged far unlink_ticks ticks in a row
 * UNLINKS, a pair with a row missing is frozen, and a slot taken by a new track inherits nothing.  Parties are the connected components
 * of the linked graph over the tick's placed rows.  tests/prox_oracle.py is the specification and the device equals it bit for bit.
 * aic_prox_config: frame_h, frame_w 1..16384; max_tracks 1..512; forget_after 0..2^24; metric 0 / 1; near 1..2^24 (metric 0) or 1..4096
 * (metric 1); height_ratio_q8 256..65536; link_ticks, unlink_ticks 1..32767; speed_shift 0..12; 0 <= still_speed <= run_speed <= 2^20.
 * aic_prox_config_default fills 128 tracks, forget_after 70, metric 1, near 700, height_ratio_q8 384, link_ticks 30, unlink_ticks 60,
 * speed_shift 2, still_speed 5, run_speed 70.  Resident memory: 32.8 KB of slot table per camera plus 8 bytes per slot pair, 4
 * max_tracks (max_tracks - 1) bytes per camera (65 KB at 128 tracks, 1.05 MB at 512).
 * Every argument error is AIC_ERR_INVALID before the device is touched; create, option, reset and set_ground never touch it.  Device
 * buffers are allocated by the first call that reaches the device; an allocation that does not fit fails that call with AIC_ERR_CAPACITY.
 * set_ground: H[9] (|H[k]| <= 2^30) and shift 0..14 of one stream or of all (-1); the default is the identity with shift 0.
 * update: counts[ticks * streams] and rows6 (tick-major; both host or both device, rows_mem), ticks 0..65536 (0 only drains), cap 0..4096,
 * cap_pairs 0..4096; a frame of more than 512 rows is AIC_ERR_CAPACITY before anything is staged.  Outputs (host): n_final[streams];
 * events[streams, cap, 16] = reason (0 LIVE, 1 EXPIRED, 2 FLUSHED), stream, id, cls, first_frame, last_seen, sightings, links, dist,
 * max_v_q8, v_q8, party_ticks, max_party, last gx, last gy, last gait -- only the n_final[s] first of a stream are written;
 * pending[streams]; status[streams] (may be NULL); records[ticks * streams, 16] = frame, n_counted, n_placed, n_near_pairs, largest_near,
 * n_linked_pairs, n_parties, n_singles, largest_party, n_units, n_running, n_still, n_link, n_unlink, 0, 0; row_tags[sum of counts, 8] =
 * gx, gy, v_q8 (-1 without a measurement), gait, party (the smallest id of the row's party, -1 when not placed), party_size, n_near, flags
 * (1 VALID, 2 FIRST, 4 NONEMPTY, 8 PLACED, 16 NEW); n_pair_events[ticks * streams] (the true counts); pair_events[ticks * streams,
 * cap_pairs, 8] = kind (1 LINK, 2 UNLINK), frame, id_lo, id_hi, duration, distance, on or off, 0, zero-filled.  The records and tags of
 * ticks a stopped stream did not walk are all -1.  A stream that needs more than max_tracks slots stops alone with AIC_ERR_CAPACITY.
 * flush, export (events[max_tracks, 16]), reset: as for aic_heat_*.  export_pairs: out6[max_tracks (max_tracks - 1) / 2, 6] = id_a id_b
 * linked on off since of the nonzero entries among live slots, in (slot_lo, slot_hi) order.
 * option: "forget_after", "metric", "near", "height_ratio_q8", "link_ticks", "unlink_ticks", "speed_shift", "still_speed", "run_speed"
 * (legal between calls), "ticks_per_launch", "launch_budget_mb": same results. */
typedef struct aic_prox aic_prox;
typedef struct {
    int32_t streams, frame_h, frame_w, max_tracks, forget_after, metric, near, height_ratio_q8, link_ticks, unlink_ticks, speed_shift, still_speed,
        run_speed;
} aic_prox_config;
int aic_prox_config_default(int streams, int frame_h, int frame_w, aic_prox_config* out);
int aic_prox_create(int device, const aic_prox_config* config, aic_prox** out);
int aic_prox_destroy(aic_prox* h);
int aic_prox_option(aic_prox* h, const char* key, int value);
int aic_prox_reset(aic_prox* h, int stream);
int aic_prox_set_ground(aic_prox* h, int stream, const int32_t* H, int shift);
int aic_prox_update(aic_prox* h, int ticks, const int32_t* counts, const int32_t* rows6, int rows_mem, int cap, int cap_pairs, int32_t* n_final,
                    int32_t* events, int32_t* pending, int32_t* status, int32_t* records, int32_t* row_tags, int32_t* n_pair_events,
                    int32_t* pair_events);
int aic_prox_flush(aic_prox* h, int stream, int cap, int32_t* n_final, int32_t* events, int32_t* pending, int32_t* status);
int aic_prox_export(aic_prox* h, int stream, int32_t* n, int32_t* events);
int aic_prox_export_pairs(aic_prox* h, int stream, int32_t* n, int32_t* out6);
/* ---- JPEG out: a bank of equally sized BGR24 images to complete JFIF files in one call (csrc/jpeg.hpp) ---------
 * Baseline sequential DCT, 8 bit, YCbCr full range, 4:2:0 (subsampling 420) or 4:4:4 (444), the Annex K Huffman tables, restart markers
 * always on (restart = MCUs per interval, 1..65535; 0 = one MCU row).  Integer arithmetic only; tests/jpeg_oracle.py is the
 * specification and the device's bytes equal it bit for bit.  Every file starts with the same 629 header bytes.
 * aic_jpeg_tables / aic_jpeg_header (host only, no device): the quantisation tables of a quality (1..100) in natural order; the header
 * (*n = 629; AIC_ERR_CAPACITY when cap is smaller).
 * Every argument error is AIC_ERR_INVALID before the device is touched; create, option and worst_case_bytes never touch it.
 * config: max_images 1..4096, height and width 1..16384, quality 1..100, restart 0..65535, subsampling 420 / 444, max_bytes >= 631 per
 * image (default 629 + 3 * padded_w * padded_h + 2 * intervals + 2; worst_case_bytes = 629 + 416 * blocks + 2 * intervals + 2 always fits).
 * encode: n (0..max_images) images [n, height, width, 3] in host or device memory (frames_mem; a device pointer of any alignment); the
 * files are packed back to back into out (out_mem; out_cap bytes): file i is out[offsets[i] .. offsets[i + 1]).  An image whose file is
 * larger than max_bytes gets status[i] = AIC_ERR_CAPACITY and zero length, its neighbours are unaffected.  When the packed total
 * exceeds out_cap the call returns AIC_ERR_CAPACITY with offsets and status filled and nothing written: the caller retries with room.
 * option: "quality", "restart" (legal between calls), "launch_budget_mb" (1..65536, default 1024): a bank is cut into launches whose
 * staged frames and coefficients each stay below it, one image at the least; same bytes.
 * coefficients (debugging): the quantised coefficients of n images, int16 [n, MCUs, blocks per MCU, 64] in zigzag order, to the host. */
typedef struct aic_jpeg aic_jpeg;
typedef struct {
    int32_t max_images, height, width, quality, restart, subsampling;
    int64_t max_bytes;
} aic_jpeg_config;
int aic_jpeg_tables(int quality, uint8_t luma[64], uint8_t chroma[64]);
int aic_jpeg_header(int height, int width, int quality, int restart, int subsampling, uint8_t* out, int cap, int* n);
int aic_jpeg_config_default(int height, int width, aic_jpeg_config* out);
int aic_jpeg_create(int device, const aic_jpeg_config* config, aic_jpeg** out);
int aic_jpeg_destroy(aic_jpeg* j);
int aic_jpeg_option(aic_jpeg* j, const char* key, int value);
int aic_jpeg_worst_case_bytes(aic_jpeg* j, int64_t* bytes);
int aic_jpeg_encode(aic_jpeg* j, const uint8_t* frames_bgr, int frames_mem, int n, uint8_t* out, int out_mem, int64_t out_cap,
                    int64_t* offsets, int32_t* status);
int aic_jpeg_coefficients(aic_jpeg* j, const uint8_t* frames_bgr, int frames_mem, int n, int16_t* out);
int aic_jpeg_counters(aic_jpeg* j, int64_t* images, int64_t* bytes_in, int64_t* bytes_out);
/* ---- JPEG in: a bank of JPEG files of one picture size to [n, height, width, 3] BGR24 in one call (csrc/jpegdec.hpp) --
 * Baseline sequential DCT (SOF0), 8 bit, one interleaved scan; 1 component (gray) or 3 (Y, Cb, Cr) at 4:4:4, 4:2:2 or 4:2:0; any 8-bit
 * quantisation tables, any Huffman tables (ids 0 and 1; a file without any DHT uses the Annex K tables), any restart interval; APPn and
 * COM are skipped.  Every image of a call may have its own tables, sampling and restart interval; only the picture size is the handle's.
 * Integer arithmetic only: tests/jpegdec_oracle.py is the specification and the device's pixels equal it byte for byte (libjpeg's ISLOW
 * inverse DCT, triangle upsampling and fixed-point colour conversion).
 * Anything else is refused per image: the call still returns AIC_OK, status[i] = AIC_ERR_FORMAT, reason[i] = an AIC_JPEGDEC_* value, the
 * output slot of that image is not written and its neighbours are unaffected.
 * Every argument error is AIC_ERR_INVALID before the device is touched (NULL, n outside 0..max_images, offsets not ascending, a file of
 * more than 64 MB, an unknown mem); create, option and probe never touch it; n = 0 succeeds without touching it.
 * config: max_images 1..4096, height and width 1..16384.
 * probe (host only): the header of one file; status / reason as decode would report them for the header alone (every other field zero
 * when refused; no size is asked for); intervals = the restart intervals the header implies.
 * decode: file i is files[offsets[i] .. offsets[i + 1]) in host or device memory (files_mem; offsets always in host memory); out_bgr in
 * host or device memory (out_mem; a device pointer of any alignment).
 * option: "launch_budget_mb" (1..65536, default 1024): a bank is cut into launches whose staged files and coefficients each stay below
 * it, one image at the least; same bytes.
 * coefficients (debugging): image `image` of the bank, int16 [MCUs, blocks per MCU, 64] in natural order, MCU-interleaved, to the host;
 * AIC_ERR_FORMAT for an image that decode would refuse.
 * aic_pipeline_upload_jpeg: the counterpart of aic_pipeline_upload -- decodes `count` files straight into ring slots slot .. slot + count
 * of a BGR24 pipeline whose frame size is the files'; a refused image leaves its slot as it was. */
#define AIC_JPEGDEC_TRUNCATED 1
#define AIC_JPEGDEC_NOT_JPEG 2
#define AIC_JPEGDEC_NOT_BASELINE 3
#define AIC_JPEGDEC_PRECISION 4
#define AIC_JPEGDEC_COMPONENTS 5
#define AIC_JPEGDEC_SAMPLING 6
#define AIC_JPEGDEC_SIZE_MISMATCH 7
#define AIC_JPEGDEC_BAD_TABLE 8
#define AIC_JPEGDEC_MISSING_TABLE 9
#define AIC_JPEGDEC_BAD_SCAN 10
#define AIC_JPEGDEC_RESTART_SEQUENCE 11
#define AIC_JPEGDEC_BAD_CODE 12
#define AIC_JPEGDEC_OVERRUN 13
typedef struct aic_jpegdec aic_jpegdec;
typedef struct {
    int32_t max_images, height, width;
} aic_jpegdec_config;
typedef struct {
    int32_t status, reason, width, height, components, sampling /* 400 444 422 420 */, restart, intervals;
    int64_t entropy_offset, entropy_bytes;
} aic_jpegdec_info;
int aic_jpegdec_probe(const uint8_t* file, int64_t bytes, aic_jpegdec_info* out);
int aic_jpegdec_create(int device, const aic_jpegdec_config* config, aic_jpegdec** out);
int aic_jpegdec_destroy(aic_jpegdec* d);
int aic_jpegdec_option(aic_jpegdec* d, const char* key, int value);
int aic_jpegdec_decode(aic_jpegdec* d, const uint8_t* files, int files_mem, const int64_t* offsets, int n, uint8_t* out_bgr, int out_mem,
                       int32_t* status, int32_t* reason);
int aic_jpegdec_coefficients(aic_jpegdec* d, const uint8_t* files, int files_mem, const int64_t* offsets, int n, int image, int16_t* out);
int aic_jpegdec_counters(aic_jpegdec* d, int64_t* images, int64_t* refused, int64_t* bytes_in, int64_t* bytes_out);
int aic_pipeline_upload_jpeg(aic_pipeline* p, int slot, const uint8_t* files, int files_mem, const int64_t* offsets, int count,
                             int32_t* status, int32_t* reason);
/* ---- 4:2:0 YUV frames in, NV12 out: pixel-format conversion of a bank of frames in one launch (csrc/yuv.hpp) -------
 * Decoders, RTSP stacks and camera SDKs deliver NV12 (sometimes I420) on pitched surfaces and encoders want the same back; everything else
 * in this library reads packed BGR24.  tests/yuv_oracle.py is the specification and the device equals it bit for bit in both directions:
 * int32 arithmetic on coefficients scaled by 2^20 (the standards' exact fractions, rounded half away from zero -- not OpenCV's
 * three-decimal constants, from which results may differ by one level), chroma replicated on decode (pixel (x, y) takes the chroma sample
 * of block (x/2, y/2)) and taken from the sums over each 2x2 block on encode.
 * Layout of one frame: AIC_PIX_NV12 = a Y plane of h rows of `pitch` bytes, then h/2 rows of `pitch` bytes holding U,V interleaved;
 * AIC_PIX_I420 = the Y plane, then a U plane of h/2 rows of pitch/2 bytes, then a V plane of the same shape.  Frame f starts at
 * f * frame_stride.  h and w even and in 2..16384; pitch >= w (even for I420), 0 = w; frame_stride >= pitch * h * 3 / 2, 0 = exactly that.
 * The BGR side is always [n_frames, h, w, 3], tight.  matrix: AIC_YUV_BT601 / AIC_YUV_BT709; range: AIC_YUV_LIMITED (luma 16..235,
 * chroma 16..240) / AIC_YUV_FULL.
 * aic_yuv_coeffs (host only): the decode coefficients cy cvr cvg cug cub, the encode coefficients yr yg yb ur ug ub vr vg vb and the
 * luma offset of a matrix / range pair.
 * aic_frames_to_bgr / aic_frames_from_bgr: src and dst both in host memory (AIC_HOST: uploaded, converted, downloaded) or both in the
 * device's HBM (AIC_DEVICE; any alignment -- 8-byte aligned bases with w, pitch and frame_stride multiples of 8 take the wide path, the
 * same bytes either way).  from_bgr writes only the bytes inside w: pitch padding and the tail of a frame_stride keep their contents.
 * Every argument error (odd or out-of-range h / w, pitch < w, an odd I420 pitch, a short frame_stride, format AIC_PIX_BGR24 or unknown,
 * unknown matrix / range / mem, NULL) is AIC_ERR_INVALID before the device is touched; n_frames = 0 succeeds without touching it.
 * One stream synchronise ends the call. */
#define AIC_PIX_BGR24 0
#define AIC_PIX_NV12 1
#define AIC_PIX_I420 2
#define AIC_YUV_BT601 0
#define AIC_YUV_BT709 1
#define AIC_YUV_LIMITED 0
#define AIC_YUV_FULL 1
int aic_yuv_coeffs(int matrix, int range, int32_t dec[5], int32_t enc[9], int32_t* y_offset);
int aic_frames_to_bgr(int device, const uint8_t* src, int n_frames, int h, int w, int format, int64_t pitch, int64_t frame_stride, int matrix,
                      int range, int mem, uint8_t* dst_bgr);
int aic_frames_from_bgr(int device, const uint8_t* src_bgr, int n_frames, int h, int w, int format, int64_t pitch, int64_t frame_stride,
                        int matrix, int range, int mem, uint8_t* dst);
/* A pipeline fed 4:2:0 frames: aic_pipeline_option "pixel_format" (AIC_PIX_*; default AIC_PIX_BGR24), "yuv_matrix", "yuv_range", legal
 * between calls (an odd frame_h or frame_w rejects a YUV format).  aic_pipeline_upload and aic_pipeline_run_from_host[_passes] then read
 * host frames of h * w * 3 / 2 bytes, tightly packed; they land in a YUV staging ring (one slot per ring slot, allocated on first use) and
 * are unpacked into the BGR ring slot on the copy stream, directly behind their copy.  The ring stays BGR: nothing after it changes.
 * aic_pipeline_read_frames: ring slots [slot, slot + count) as BGR [count, frame_h, frame_w, 3] to the host, between calls. */
int aic_pipeline_read_frames(aic_pipeline* p, int slot, int count, uint8_t* out_bgr);
int aic_host_register(void* ptr, size_t bytes);   /* hipHostRegister: page-lock caller memory */
int aic_host_unregister(void* ptr);
int aic_pipeline_tracker(aic_pipeline* p, aic_tracker** out);
/* Host wall-clock split since the last reset (seconds): issuing launch groups (producer thread), waiting for
 * a group's GPU work, walking its frames through the tracker (association recurrence). */
int aic_pipeline_stats(aic_pipeline* p, double* issue_s, double* wait_s, double* track_s, int64_t* frames, int reset);
/* Runtime options (tests / measurements). "taper": 1 (default) = the last launch group of a call is split into
 * shrinking groups so its un-overlapped tail is short, 0 = full groups only.  "group_frames": frames per launch group
 * (<= batch; 0 = batch).  "device_assoc": 2 = association on the device, k frames per launch (cascade, LSAP and
 * lifecycle in csrc/kernels_trk_dev.hip, no host round trip per frame); 0 = cost matrices on the device, cascade / LSAP /
 * lifecycle in host C++ (csrc/assoc_host.cpp, lsap.cpp), one launch + one sync per frame; 1 (default) = per launch group, on
 * the device while the assignment problems are at most 192 tracks x 192 detections (a few columns per lane of the wave
 * LSAP; unique optima never reach it), else on the host;
 * a group with a frame of more than 512 detections always takes the host chain ("device_assoc_limit": the 192 of the auto mode).  "device_filter" (inject = 0): 1 (default) = the
 * tracker's confidence / class filter runs on the device and ReID is sized from a device-side count, 0 = filter on the host.
 * "split_streams": 1 = crop + ReID of a launch group on a stream of their own beside the next group's detector (more frames/s; the
 * kernels of the two streams stretch each other, so per-launch durations no longer describe the kernels), 0 (default) = one stream.
 * "dual_lane_frames" (default 128): launch groups of at most that many frames alternate between TWO instances of each engine (the second
 * one built on first use: own activation arena, detector workspace and streams), so that the groups of the two chunk contexts run
 * side by side -- a small group is a chain of ~60 short dependent kernels that leaves most of the chip idle; 0 = one lane.
 * Same results in every mode.
 * "epoch_frames" (BoT-SORT pipelines and DeepSORT bank pipelines only; AIC_ERR_INVALID on any other): frames per epoch launch of the
 * tracker, 0..16 as aic_botsort_option / aic_deepsort_bank_option (0 = 16).  Same results either way.
 * "gmc" (a BoT-SORT pipeline only; AIC_ERR_INVALID on any other): 0 (default) = no camera-motion warp, 2 or 4 = the camera motion of
 * every frame is estimated on the device at that downscale (as aic_gmc_estimate_batch, the boxes being the detections handed to the
 * tracker) and warps the predicted tracks.  The gray levels are computed in the group's launch group, matching and fit run on the
 * tracker stream before the group's epochs; the stream's first frame gets the identity.  With 0 nothing of it is launched or allocated.
 * "streams" (ByteTrack and OC-SORT pipelines only; 1..256, default 1; set before the first run): the ring and every run range are
 * tick-major over that many camera streams, slot t * streams + s being tick t of stream s, and the tracker is a bank (one kernel block
 * per stream).  `batch` must be a multiple of it, as must slot and count of every run call; launch groups round to whole ticks. */
int aic_pipeline_option(aic_pipeline* p, const char* key, int value);
/* A pipeline with "streams", or one from aic_pipeline_create_botsort_bank or aic_pipeline_create_deepsort_bank: stream s as after create
 * (aic_bytetrack_bank_reset), a stop cleared, between run calls; with "gmc" the camera's carried gray level is forgotten as well.
 * AIC_ERR_INVALID on pipelines from aic_pipeline_create and aic_pipeline_create_botsort. */
int aic_pipeline_reset_stream(aic_pipeline* p, int stream);
/* The warps [n_frames, 6] (as aic_gmc_estimate_batch) of the most recently finished launch group of a pipeline with "gmc" set;
 * AIC_ERR_INVALID without it.  warps may be NULL; *n_frames is the group's frame count, at most cap_frames rows are written. */
int aic_pipeline_group_warps(aic_pipeline* p, float* warps, int cap_frames, int32_t* n_frames);
/* launch groups issued on the second lane since the pipeline was created */
int aic_pipeline_lane_groups(aic_pipeline* p, int64_t* lane1_groups);
/* Launch groups whose crop count outgrew the buffers sized from max_persons (handled, not dropped), and frames
 * whose confirmed tracks outnumbered the caller's max_persons rows (n_tracks reports the true count). */
int aic_pipeline_counters(aic_pipeline* p, int64_t* grown_groups, int64_t* clipped_frames);
/* inject = 0: launch groups whose detection filter (src/tracker/deepsort_tracker.py:88-101) ran on the device behind NMS (no host
 * synchronisation between YOLO and ReID) / on the host (one event wait per group), and the extra ReID rounds launched for groups
 * whose surviving detections outnumbered the ReID engine's max_items.  Any pointer may be NULL. */
int aic_pipeline_filter_counters(aic_pipeline* p, int64_t* device_groups, int64_t* host_groups, int64_t* overflow_rounds);
/* Frames, since creation, whose association (src/tracker/core/tracker_core.py:83-177) ran on the device in the epoch
 * kernels / on the host in C++: what the "device_assoc" auto mode actually chose. Either pointer may be NULL. */
int aic_pipeline_assoc_frames(aic_pipeline* p, int64_t* device_frames, int64_t* host_frames);
/* ReID embeddings of every crop of the most recently finished launch group, frame-major (parity tests of the
 * production-size kernel mix): emb[n_rows, dim] host, crops_per_frame[n_frames]. Any output pointer may be NULL. */
int aic_pipeline_group_embeddings(aic_pipeline* p, float* emb, int cap_rows, int32_t* crops_per_frame, int cap_frames,
                                  int32_t* n_rows, int32_t* n_frames, int32_t* dim);
/* Embeddings of the last processed frame (parity tests): emb[n,dim] host. */
int aic_pipeline_last_embeddings(aic_pipeline* p, float* emb, int cap_rows, int32_t* n, int32_t* dim);

/* ------------------------------------------------------------------ overlay (the step after the path)
 * draw_tracks / draw_detections / draw_info_panel (src/utils/visualization.py:9-124,170-228) as ONE kernel on the frame:
 * prims[n,8] = (kind, x0, y0, x1, y1, color B|G<<8|R<<16, text offset, text length | scale<<16); kind 0 = box outline of
 * thickness 2, 1 = filled rectangle (corners inclusive), 2 = 5x7 bitmap text with its top-left corner at (x0, y0).  Painter's
 * order = list order.  The frame (u8 BGR, host or device) is modified in place.  Pixel spec: csrc/kernels_overlay.hip. */
int aic_overlay(int device, uint8_t* frame_bgr, int h, int w, int mem, const int32_t* prims, int n, const uint8_t* text,
                int text_bytes);

/* ------------------------------------------------------------------ measurement
 * HIP-event timing of kernel classes on the streams they are launched on (bench.py roofline).
 * Classes: 0 conv_igemm (MFMA), 1 conv_direct (3-channel stems), 2 pool/upsample/misc,
 * 3 letterbox, 4 crop_resize, 5 decode+nms, 6 tracker kernels. */
#define AIC_PROF_CLASSES 7
/* class_mask: bit c set = time class c; 0 = off; -1 = all classes */
int aic_prof_enable(int device, int class_mask);
int aic_prof_reset(int device);
/* total ms, launches, algorithmic FLOPs and algorithmic bytes accumulated for a class. */
int aic_prof_read(int device, int cls, double* ms, int64_t* launches, double* flops, double* bytes);
/* length (ms, device clock) of the UNION of the class's bracketed intervals since aic_prof_reset: equal to aic_prof_read's ms while
 * one stream carries the class; with brackets open on two streams at once (aic_pipeline_option "split_streams") the overlap is
 * counted once.  -1 when cross-stream event timestamps are unavailable.  (bench.py's roofline denominator; no reference counterpart:
 * the reference times its loop with time.time(), src/aicamera_tracker.py:175,201.) */
int aic_prof_read_union(int device, int cls, double* ms_union);

#ifdef __cplusplus
}
#endif
#endif /* AICAM_H */
