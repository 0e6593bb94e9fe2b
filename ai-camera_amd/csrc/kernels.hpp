// kernels.hpp -- host-callable launchers of the gfx950 kernels (defined in the .hip files).
#pragma once
#include "common.hpp"
#include "conv_plan.hpp"

namespace aic {

typedef _Float16 half_t;

// ------------------------------------------------------------------ conv / graph ops (kernels_conv.hip)
void launch_conv_igemm(int dtype, const ConvArgs& a, hipStream_t s);
// the fused blocks, launched where plan_c64_block / plan_c2f16 (conv_plan.hpp) accept them (kernels_conv_block.hip, kernels_conv_c2f.hip)
void launch_c64_block(const ConvArgs& c1, const ConvArgs& c2, int ipb, hipStream_t s);
void launch_c2f16(const ConvArgs& cv1, const ConvArgs& m_cv1, const ConvArgs& m_cv2, const ConvArgs& cv2, hipStream_t s);

// letterbox + conv 3x3/2 (3->16) + SiLU fused (fp16 YOLOv8 stem); false = geometry not supported, nothing launched
struct LetterboxGeom;
bool launch_yolo_stem_fused(const uint8_t* frames, int n, const LetterboxGeom& g, const void* w, const float* bias, int Kp, void* y,
                            int y_cs, int y_coff, int Ho, int Wo, hipStream_t s, int win_y0 = 0, int win_rows = 0);   // win_*: ConvArgs::win_y0 / win_rows

// conv 3x3/1 (3->64) + ReLU + max-pool 3x3/2 fused (fp16, W == 64, H % 8 == 0): ReID stem
// in_stride: halves per input pixel, 8 (NHWC8) or 4 (NHWC4 = RGB0; only where reid_stem2_usable(H, W))
// frames != NULL: the fused fp16 ReID stem resamples every crop from the u8 frames itself (boxes [n,4] xyxy, frame_of[n] or NULL, valid[n] written)
struct CropSrc { const uint8_t* frames; int fh, fw; const float* boxes; const int* frame_of; int* valid; };
// n_dev: optional device-side crop count (see ConvArgs::n_dev)
void launch_reid_stem_pool(const void* x, const void* w, const float* bias, void* y, int n, int H, int W, int Kp, int y_cs,
                           int y_coff, int in_stride, hipStream_t s, const CropSrc* crop = nullptr, const int* n_dev = nullptr);
bool reid_stem2_usable(int H, int W);

struct EltArgs {
    const void* src; void* dst;
    int n, h, w, c;            // source extent, channels processed
    int s_cs, s_coff, d_cs, d_coff;
    const int* n_dev;          // optional device-side item count (n is then the bound the grid was sized for); NULL: n is exact
};
void launch_sppf_pool(int dtype, const EltArgs& a, hipStream_t s);     // writes 3 pooled copies at d_coff + k*c
void launch_upsample2x(int dtype, const EltArgs& a, hipStream_t s);
void launch_maxpool3s2(int dtype, const EltArgs& a, hipStream_t s);
void launch_avgpool(int dtype, const EltArgs& a, hipStream_t s);
void launch_l2norm(int dtype, const EltArgs& a, hipStream_t s);        // dst is float
// fp32 NCHW [n,3,h,w] -> NHWC8 (RGB + zeros) of the activation dtype
void launch_nchw_to_nhwc8(int dtype, const float* src, void* dst, int n, int h, int w, hipStream_t s);
// gather float NHWC buffer rows -> dense float [n, hw, c] (head export)
void launch_copy_f32(const float* src, float* dst, size_t count, hipStream_t s);

// ------------------------------------------------------------------ pre-processing (kernels_pre.hip)
struct LetterboxGeom {
    int src_h, src_w, out_h, out_w, unpad_h, unpad_w, top, left;
    float ratio, pad_w, pad_h;
};
LetterboxGeom letterbox_geometry(int h, int w, int out_h, int out_w);
// frames u8 [n,h,w,3] BGR (device). mode 0: fp32 NCHW RGB/255 ; mode 1: NHWC8 activation dtype
void launch_letterbox(const uint8_t* frames, int n, const LetterboxGeom& g, int mode, int dtype, void* out,
                      hipStream_t s);
void launch_letterbox_u8(const uint8_t* frame, const LetterboxGeom& g, const int color_bgr[3], uint8_t* out, hipStream_t s);
// boxes [n,4] xyxy (device), frame_of[n] (device, may be NULL = frame 0), frames u8 [*,h,w,3].
// n_dev (device int, may be NULL) caps the number of live crops. valid[n] written.
// slack: the caller owns >= 16 readable bytes behind the last frame (12-byte tap loads instead of byte loads; same bytes used)
void launch_crop_resize(const uint8_t* frames, int h, int w, const float* boxes, const int* frame_of, int n,
                        const int* n_dev, int out_h, int out_w, int mode, int dtype, void* out, int* valid,
                        hipStream_t s, bool slack = false);

// ------------------------------------------------------------------ detection head (kernels_det.hip)
struct HeadLevel { const float* box; const float* cls; int h, w, stride, a0; int cls_reduced, box_decoded; };   // cls_reduced / box_decoded: max_logit + labels / boxes of this level were written by the branch's own tail (ConvArgs::t_max / t_box)
struct DetArgs {
    HeadLevel lvl[4];
    int n_levels, n_anchors, nc, reg_max, batch;
    int fast_exp;      // fp16 engines: the DFL softmax's exponential as v_exp_f32(x log2 e), the form the box branches' tails use (tail_1x1); fp32 engines: expf
    float logit_thr, iou_thr;
    int max_det;
    // letterbox undo (K4)
    float pad_w, pad_h, ratio; int orig_w, orig_h;
    // outputs / workspace (device)
    float* boxes;      // [B,A,4]
    float* max_logit;  // [B,A]
    int* labels;       // [B,A]
    unsigned long long* keys;  // [B,A] sort keys
    int* n_cand;       // [B]
    int* num_dets;     // [B]
    float* out_boxes;  // [B,max_det,4] letterbox space
    float* out_boxes_orig;  // [B,max_det,4] original frame space (may be NULL)
    float* out_scores; // [B,max_det]
    int* out_labels;   // [B,max_det]
};
void launch_decode(const DetArgs& a, hipStream_t s);
// The candidate pass of the sparse box branches (three-level heads): from the max logits of a run, the pixels whose boxes NMS will read
// at logit_thr.  list[l], l < 3: level l's candidate pixels; list[3]: the in-map pixels of the 3 x 3 neighbourhoods of level 0's
// candidates, each once.  Entries are linear pixels img * h * w + cell of the level's full map (ConvArgs::pix_list), in no fixed order;
// count[4] (device) is zeroed and filled by the launch.  list[l] holds batch * h[l] * w[l] entries, list[3] as many as list[0].
struct BoxListArgs {
    const float* max_logit;        // [batch, n_anchors]
    float logit_thr;
    int batch, n_anchors;
    const int* n_dev;              // optional device-side live frame count: frames at or past it contribute nothing
    int h[3], w[3], a0[3];
    int* list[4];
    int* count;
};
void launch_box_candidates(const BoxListArgs& a, hipStream_t s);
// deepsort_tracker.py:88-101 on the device: order-preserving confidence / class filter of a launch group's NMS outputs, compacted
// into the arrays crop + ReID + the association epochs read (kernels_det.hip)
struct DetFilterArgs {
    const int* num_dets; const float* boxes; const float* scores; const int* labels;   // [B], [B,max_det,4] original-frame xyxy, [B,max_det] x 2
    int batch, max_det;
    float min_conf;
    unsigned long long mask[2];     // bit c = class c is tracked
    int cap;                        // rows the compact arrays hold (batch * max_det never overflows)
    int* rank;                      // scratch [B, max_det]
    int* frame_n; int* frame_d0;    // [B] kept detections of the frame, first row of the frame
    int* total;                     // [2]: rows present (<= cap), rows the filter passed
    float* xyxy; float* tlwh; float* conf; int* cls; int* frame_of;   // [cap, 4] x 2, [cap] x 3
};
void launch_det_filter(const DetFilterArgs& a, hipStream_t s);
void launch_select_sort_nms(const DetArgs& a, hipStream_t s);

// ------------------------------------------------------------------ tracker (kernels_trk.hip)
void launch_kf_initiate(const float* z, int n, float* mean, float* cov, hipStream_t s);
void launch_kf_predict(float* mean, float* cov, const int* slots, int n, hipStream_t s, float dt = 1.f);
void launch_kf_project(const float* mean, const float* cov, int n, float* pmean, float* pcov, hipStream_t s);
void launch_kf_update(float* mean, float* cov, const float* z, int n, hipStream_t s);
void launch_kf_gating(const float* mean, const float* cov, const int* slots, int n, const float* zs, int m,
                      int shared_z, int only_position, float* d2, hipStream_t s);
void launch_iou_cost(const float* trk_tlwh, const float* mean, const int* slots, int t, const float* det_tlwh,
                     int n, float* cost, hipStream_t s);
void launch_fill(float* p, float v, size_t n, hipStream_t s);
void launch_normalize_rows(const float* src, float* dst, int n, int dim, hipStream_t s, const int* n_dev = nullptr);

// fused per-frame tracker kernels
// galleries: base [slots][gmax][dim], rows normalised; per row t: slot index + valid length; det_n normalised rows.
void launch_cosine_min_mfma(const float* gal_n, const int* slots, const int* glen, int t, int gmax, int dim, const float* det_n,
                            const unsigned char* has_feat, int n, float* cost, hipStream_t s);
void launch_trk_assoc_all(float* mean, float* cov, const int* slots, const int* glen, int t, int do_predict, const float* det_tlwh,
                          const float* det_xyah, const float* gal_n, int gmax, int dim, const float* det_n,
                          const unsigned char* has_feat, int n, float* app, float* d2, float* iouc, hipStream_t s);
// the same launch preceded, per track, by the commit of the previous frame (Kalman update / initiate / gallery row);
// c_kind == nullptr: association only; n == 0: commit only
void launch_trk_step(float* mean, float* cov, const int* slots, const int* glen, int t, int do_predict, const float* det_tlwh,
                     const float* det_xyah, const float* gal_n, int gmax, int dim, const float* det_n,
                     const unsigned char* has_feat, int n, float* app, float* d2, float* iouc,
                     const int* c_kind, const int* c_det, const int* c_kout, const int* c_appos, const int* c_apdet,
                     const float* c_xyah, const float* c_feat, const float* c_feat_n, float* c_out_tlwh, float* c_gal_raw, float* c_gal_w,
                     hipStream_t s);
void launch_trk_commit(float* mean, float* cov, const int* lists, int M, int U, int A, const float* xyah, float* out_tlwh,
                       float* gal_raw, float* gal_n, int gmax, int dim, const float* feat, const float* feat_n, hipStream_t s);
// association on the device, k frames per launch (kernels_trk_dev.hip, trk_dev.hpp)
struct DevTrkHdr; struct DevTrack; struct TrkDevParams; struct EpochDets; struct EpochScratch; struct EpochOut;
void launch_trk_epoch_prep(const DevTrkHdr* hdr, const DevTrack* trk, const float* gal_n, int gmax, int dim, int cap, const float* featn,
                           int dn, int dn_pad, int k, float* sm, float* gram, hipStream_t s);
void launch_trk_epoch(DevTrkHdr* hdr, DevTrack* trk, int* free_slots, float* mean, float* cov, float* gal_raw, float* gal_n,
                      const TrkDevParams& prm, const EpochDets& dets, int f0, int k, int d_begin, int dn_pad, int nmax, int has_sm,
                      const EpochScratch& scr, const EpochOut& out, hipStream_t s);
struct EpochBankArgs;
void launch_trk_epoch_prep_bank(const EpochBankArgs& bk, int streams, const float* gal_n, int gmax, int dim, int cap, const float* featn,
                                int dn_pad_max, int f0, int k, float* sm, float* gram, hipStream_t s);
void launch_trk_epoch_bank(const EpochBankArgs& bk, int streams, float* mean, float* cov, float* gal_raw, float* gal_n, const TrkDevParams& prm,
                           const EpochDets& dets, int f0, int k, int nmax_call, const EpochScratch& scr, const EpochOut& out, hipStream_t s);
void launch_gallery_shard(const DevTrkHdr* hdr, const DevTrack* trk, const float* gal_n, int gmax, int dim, float* out, int t_max, hipStream_t s);
// configs[4] annotation pass: gathered [world, t_max, 2 + dim] -> per row (all ranks) track id or -1, nearest valid row of another rank or -1, its cosine distance
void launch_gallery_nearest(const float* gathered, int world, int t_max, int dim, int* ids, int* near_row, float* near_dist, hipStream_t s);
// cross-camera links inside a bank (kernels_xcam.hip, xcam.hpp): shards fp32 [streams, t_max, 2 + dim] in the layout of launch_gallery_shard,
// n_valid[streams] = the valid prefix of every stream's slice, flags[streams] (bit 0: valid rows not a prefix; bit 1: a track id >= 2^24)
constexpr int BANK_STREAMS_MAX_XCAM = 256;  // streams of one pass (= the nearest kernel's block: one thread per stream in its prefix sum)
constexpr int XCAM_KC = 32;                 // K-chunk of the nearest kernel's LDS tiles
constexpr int XCAM_SMALL_ROWS = 4096;       // streams * t_max below this: 32 x 32 tiles (2 x 2 per thread), else 64 x 64 (4 x 4 per thread)
void launch_xcam_pack_deepsort(const char* tbl, size_t tbl_stride, const float* gal_n, size_t gal_stride, int gmax, int dim, int streams, int t_max,
                               float* shards, int* n_valid, int* flags, hipStream_t s);
void launch_xcam_pack_botsort(char* bank, size_t table_stride, float* smooth, size_t smooth_stride, int cap, int dim, int streams, int t_max,
                              float* shards, int* n_valid, int* flags, hipStream_t s);
void launch_xcam_count(const float* shards, int streams, int t_max, int dim, int* n_valid, int* flags, hipStream_t s);
int xcam_tile_rows(int streams, int t_max, int tile);   // tile: 32 / 64 = that tile, anything else = by size
// the table of launch_gallery_nearest over [streams, t_max] rows (dim % 4 == 0, streams <= 256); best = [streams * t_max] scratch keys
void launch_xcam_nearest(const float* shards, const int* n_valid, int streams, int t_max, int dim, int tile, unsigned long long* best, int* ids,
                         int* near_row, float* near_dist, hipStream_t s);
void launch_trk_cascade_test(const TrkDevParams& prm, const EpochScratch& scr, int T, int n, const int* state, const int* tsu,
                             int* out_mdet, int* out_err, int stage1_only, hipStream_t s);
// the identity archive (kernels_archive.hip, archive.hpp): int8 rows at `pitch` bytes (dim rounded up to 64, zero padded), one scale a row,
// metadata per slot (key < 0 = free).  Every per-slot array is allocated for the capacity rounded up to 16 (rows: plus 128 bytes).
constexpr int ARCHIVE_MIN_BLOCK_ROWS = 64;
// put: row src_index[i] (device list; NULL: i) of src (row_stride floats apart, payload at + offset) -> slot slots[i] (NULL: i); keys[i] < 0 or slots[i] < 0 skips the row;
// mode 0 = check only.  *flag |= 1 for a row that has no code (all zero, non-finite).  key == NULL: no metadata (the queries' prologue)
void launch_archive_put(const float* src, const int* src_index, long row_stride, int offset, int dim, int pitch, int n, const int* slots, const long long* keys,
                        const int* cams, long long tick, int mode, signed char* rows, float* scale, int* camera, long long* t_last, long long* key,
                        int* flag, hipStream_t s);
int archive_block_rows(int hw, int n_queries);                 // R: the slots one block of the search owns (a multiple of 64)
size_t archive_partial_keys(int hw, int n_queries, int k);     // 64-bit keys of `part` below
void launch_archive_search(const signed char* rows, const float* scale, const int* camera, const long long* t_last, const long long* key, int hw,
                           int pitch, const signed char* qrows, const float* qscale, const aic_archive_filter* flt, int n_queries, int k,
                           unsigned long long* part, int* out_slot, float* out_dist, long long* out_key, hipStream_t s);


}  // namespace aic
