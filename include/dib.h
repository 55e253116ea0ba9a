/*
 * dib.h -- C ABI of libdib_hip.so: the MI355X (gfx950) implementation of detectInBlur's
 * data-parallel hot path (motion-blur augmentation feeding Faster R-CNN).
 *
 * The reference (mohammed-amr/detectInBlur) is pure Python; it has no FFI.  Each entry point
 * below replaces the body of one reference function and is what a ctypes binding inside the
 * reference would call.  Conventions:
 *   - plain pointers and sizes only; no torch / C++ types cross the boundary;
 *   - every `*_dev` pointer is device memory owned by the caller (e.g. a torch tensor's
 *     data_ptr()); host arrays are read during the call and may be freed on return;
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream); all work is
 *     enqueued on it, no entry point synchronises the host or allocates device memory;
 *   - return 0 on success, a negative DIB_E* code otherwise; dib_last_error() gives the text
 *     (thread-local).  No C++ exception crosses the boundary.
 */
#ifndef DIB_H_
#define DIB_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DIB_ABI_VERSION 7 /* 7: no kernel traps any more (later additions, new symbols only: dib_bn_mode_one_nhwc, dib_bn_mode_one_workspace_bytes, dib_augmix, dib_augmix_buffer_bytes, dib_augmix_workspace_bytes, the bf16 epilogues dib_bias_act_bf16_nhwc, dib_bias_act_mask_bf16_nhwc, dib_relu_mask_backward_bf16, dib_add_relu_mask_bf16, dib_scatter_add_bf16_nhwc, dib_fpn_topdown_merge_bf16_nhwc, dib_stem_pool_forward_bf16 / _backward_bf16, dib_squint_warp_forward / _backward, dib_overlay_rgb8, the deblurrer's dib_deblur_* entry points, dib_rl_deconvolve): DIB_ETIMEOUT, dib_device_status ("Device status" below); dib_blur_step takes an optional caller workspace through dib_blur_step_ws and bounds its private buffers; 6: + dib_sparse_blur_normalized (the blur with the input transform's float + normalise + zero-padded batch as its store phase); dib_blur_step runs compaction + blur as ONE launch where the shapes allow it (same results, same signature); 5: + dib_blur_step / dib_blur_step_release (DIB_ECAPTURE, DIB_STEP_PSFS_COMPLETE), dib_normalize_resize_pad, dib_fold_bn_multi, dib_scale_rows_multi, dib_box_match / _encode_matched / _decode / _pool / _labels, dib_topk_levels, dib_det_candidates, dib_bias_act_transpose, the large LDS window; 4: + dib_bias_act_mask_nhwc, dib_relu_mask_backward, dib_add_relu_mask, dib_scatter_add_nhwc, dib_fpn_topdown_merge_nhwc, dib_stem_pool_forward / _backward, dib_post_ops, dib_jpeg_roundtrip; 2: tap-table buffers carry no scheduler trailer any more; 3: tables carry a second
                             per-tap offset array (sizes come from dib_tap_table_bytes as before)          */

/* error codes */
#define DIB_OK 0
#define DIB_EINVAL (-1)  /* bad argument (NULL pointer, unsupported K / dtype, ...)            */
#define DIB_ESHAPE (-2)  /* reference would raise: reflect padding needs H,W > 64 (or < 64)    */
#define DIB_EHIP (-3)    /* a HIP runtime call failed; text in dib_last_error()                */
#define DIB_ENOT128 (-4) /* expand_targets on a PSF that is not 128 wide (utils.py:369-370)    */
#define DIB_ECAPTURE (-5) /* dib_blur_step on a stream under graph capture without caller tables */
#define DIB_ETIMEOUT (-6) /* an EARLIER dib_blur_step on this device gave up waiting inside its launch: see "Device status" */

/* element types */
#define DIB_F16 0
#define DIB_F32 1

/* accumulation modes of the sparse blur */
#define DIB_ACC_BITEXACT 0 /* reference arithmetic: round after every multiply and every add,
                              taps in row-major order (blur_functions.py:66-67)               */
#define DIB_ACC_FP32 1     /* fp32 accumulate, one final rounding (fp16 images only)           */
#define DIB_ACC_FMA16 2    /* fp16 accumulate with a fused multiply-add: one rounding per tap
                              instead of two; half the arithmetic, not the reference's (fp16 only) */
#define DIB_ACC_FAST16 3   /* the tolerance mode built for speed: DIB_ACC_FMA16's arithmetic (one fused fp16 multiply-add per
                              pixel and tap) with the taps of every window REORDERED into vertical runs -- taps of one PSF column
                              in consecutive rows share their LDS reads -- so the result differs from DIB_ACC_FMA16's in the last
                              bits (same stated tolerance against the reference: 1e-2 absolute on images in [0, 1]).  fp16 images,
                              K = 128, standard window (DIB_EINVAL otherwise); a table without the groups (compacted without
                              DIB_COMPACT_VRUNS, or a PSF of more than 4,096 taps) is blurred in row-major order: DIB_ACC_FMA16's
                              result */
/* The LARGE LDS window of the default fp16 tiles (segments of up to 21 PSF rows x 64 columns instead of 13 x 25; 39.9 KB,
 * four workgroups per CU instead of eight): fewer window refills for PSFs that span many columns or rows -- full-exposure
 * trajectories at batch 1, where the grid leaves most workgroup slots empty anyway.  Same results, bit for bit.  A table is
 * compacted for ONE geometry: pass DIB_COMPACT_LARGE_WINDOW (or-ed into `normalize`) to dib_psf_compact* and DIB_WINDOW_LARGE
 * (or-ed into `acc_mode`) to the dib_sparse_blur calls that read those tables, DIB_STEP_LARGE_WINDOW to dib_blur_step.
 * fp16 images with DIB_ACC_BITEXACT / DIB_ACC_FMA16 only (DIB_EINVAL otherwise). */
#define DIB_COMPACT_LARGE_WINDOW 8
#define DIB_WINDOW_LARGE 0x100
/* or-ed into `normalize` of dib_psf_compact*: also write the table's vertical-run groups, which DIB_ACC_FAST16 reads (fp16 PSFs,
 * K = 128, standard window; ~1 us more per compaction launch).  Tables without them serve every other mode as before. */
#define DIB_COMPACT_VRUNS 16

int dib_abi_version(void);
const char *dib_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Device status.  No kernel of this library traps (a trap ends the process's GPU context, i.e. the training job the blur runs
 * inside: reference engine.py:101 calls blur_image_list from a DDP rank).  Two conditions can only be seen from inside a launch:
 *   - the single launch of dib_blur_step hands its tap tables from the grid's first workgroups to the blur's workgroups behind
 *     them through memory.  Forward progress rests on the hardware dispatching a grid's workgroups lowest index first -- observed
 *     on gfx950, promised by nobody.  A blur workgroup that has polled ~1 s (2^20 polls) without seeing its tables gives up;
 *   - a tap table compacted for the other LDS window geometry (DIB_COMPACT_LARGE_WINDOW without DIB_WINDOW_LARGE or vice versa).
 * In both cases the workgroup leaves its tile unwritten, stores a code into a word of pinned host memory the library owns (one
 * per device) and ends.  The host never waits for that word: every dib_blur_step / dib_sparse_blur* call LOOKS at it first, and
 * the first call after such a launch returns DIB_ETIMEOUT (hand-off) or DIB_EINVAL (geometry) with the text in
 * dib_last_error(), launches nothing and clears the word -- the caller re-issues its batch (and knows that an earlier batch on
 * the device came out incomplete).  After a DIB_ETIMEOUT the device stays on compaction + blur as two ordinary launches for the
 * rest of the process.  dib_device_status(clear) looks at the current device's word without launching anything (e.g. behind a
 * hipStreamSynchronize): DIB_OK, DIB_ETIMEOUT or DIB_EINVAL; clear != 0 also consumes it as a call above would.
 * ------------------------------------------------------------------------------------- */
int dib_device_status(int clear);

/* ---------------------------------------------------------------------------------------
 * Tap tables.  A tap table is the device-side compacted form of one K x K PSF: header,
 * CSR row pointers and the row-major list of non-zero taps {row, col, weight}.  It is produced
 * once per PSF by dib_psf_compact and consumed by the blur and by the box growth, replacing the
 * two `psf/psf.sum()` + `psf.nonzero()` passes of the reference
 * (models/blur_functions.py:63,98 and utils.py:372-374) and their host synchronisations.
 * Layout (int32 words): [0]=ntaps [1]=rmin [2]=rmax [3]=cmin [4]=cmax [5]=K [6]=sum bits
 * [7]=nsegs | rowptr[K+1] | pad to x4 | taps[K*K] as {uint32 (row<<8|col), uint32 weight bits}
 * | segments[K*K] as {first tap, end tap, r_first<<8|r_last, cmin<<8|cmax} (runs of consecutive
 * taps with a bounding box of at most 13 rows x 25 columns: the unit staged in LDS by the blur)
 * | ltaps[K*K+8] one word per tap: byte offset of its source word in the blur's LDS window (low
 * 16 bits) and the fp16 weight bits (high 16 bits) | ltaps_q[K*K+8] the same for the window layout
 * of the default 128-wide tiles (8-byte elements {P[k], P[k+32], P[k+64], P[k+96]}).  With
 * DIB_COMPACT_LARGE_WINDOW the segments are runs of at most 21 rows x 64 columns and ltaps_q holds the
 * large window's offsets; word [5] carries the geometry in bit 16.
 * | vgroups[K*K] (16-byte records, behind the offsets; with DIB_COMPACT_VRUNS, word [5] bit 17 set when valid): per segment, its
 * taps regrouped into vertical runs of at most 4 taps of one PSF column in consecutive rows -- record g of a segment whose taps are
 * [t0, t1) sits at index t0 + g: {LDS offset | taps - 1 << 16 of the NEXT group, w0 | w1 << 16, w2 | w3 << 16, taps - 1 (| own offset
 * << 2 | groups of the segment << 18 in the segment's first record)}; what the DIB_ACC_FAST16 tap loop walks.
 * ------------------------------------------------------------------------------------- */
size_t dib_tap_table_bytes(int K); /* bytes of ONE table; K is 128 or 256 */
/* bytes of the buffer dib_psf_compact fills for B PSFs: B tables, dib_tap_table_bytes(K) apart */
size_t dib_tap_tables_bytes(int K, int B);

/* psf_dev: [B][K][K] of `dtype`.  normalize != 0 divides by the PSF's sum first, in the PSF's
 * dtype, exactly like `psf_GPU / psf_GPU.sum()` (blur_functions.py:98, utils.py:372); 0 takes the
 * weights as they are (manual_blur's contract, blur_functions.py:13).  tables_dev
 * (dib_tap_tables_bytes(K, B) bytes) receives B tables, dib_tap_table_bytes(K) apart. */
int dib_psf_compact(const void *psf_dev, int dtype, int B, int K, int normalize,
                    void *tables_dev, void *stream);
/* same, for PSFs that live in B separate device buffers (host array of B device pointers, each
 * 16-byte aligned): the reference's `psfs_GPU` list needs no stacking copy */
int dib_psf_compact_list(const void *const *psf_ptrs, int dtype, int B, int K, int normalize,
                         void *tables_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * Sparse PSF (x) image correlation: models/blur_functions.py:11-69 (`manual_blur`, both canvas
 * branches, post-ops excluded) for a whole batch in one launch; with tables built by
 * dib_psf_compact(normalize=1) it is `blur_image_list` (blur_functions.py:92-100).
 * Host arrays of length B: in/out device pointers (C x H x W planar, `dtype`, contiguous;
 * out must not alias in), C, H, W and table_index (which table of tables_dev image i uses;
 * < 0 = leave the image untouched, i.e. blur_dict["blurring"] == False).  tables_dev is the buffer
 * dib_psf_compact filled for num_tables PSFs (read only: any number of dib_sparse_blur calls, on any
 * streams, may share it).  Padding mode follows
 * the reference: K = 256 -> replicate; K = 128 -> zero if H < 64 or W < 64, else reflect.
 * Returns DIB_ESHAPE where the reference raises (K = 128 and H or W == 64).
 * ------------------------------------------------------------------------------------- */
int dib_sparse_blur(const void *const *in_dev, void *const *out_dev, const int *C, const int *H,
                    const int *W, const int *table_index, int B, int dtype,
                    void *tables_dev, int num_tables, int K, int acc_mode, void *stream);

/* ---------------------------------------------------------------------------------------
 * One blur step = dib_psf_compact_list + dib_sparse_blur behind ONE call: `blur_image_list`
 * (models/blur_functions.py:92-100) for a batch.  The first seven arguments are dib_psf_compact_list's (the batch's
 * blurring PSFs, in table order), the next ten dib_sparse_blur's (table_index[i] indexes those PSFs).
 *   tables_dev == NULL (the normal case): the tap tables live in two buffers per (device, stream) owned by the library
 *     and used alternately -- the ONE exception to "no entry point allocates device memory": grown to the largest batch
 *     seen on that stream, freed by dib_blur_step_release().  By default both launches are ordinary stream-ordered launches
 *     (the PSFs may be the product of work queued on `stream` before the call, e.g. an asynchronous upload).
 *     DIB_STEP_PSFS_COMPLETE in `flags` states that the PSF buffers are already complete when the call is made (resident
 *     PSFs; the reference's own `torch.HalfTensor(psf).to(device)` of engine.py:84, a synchronous copy from pageable
 *     memory): the compaction is then launched without a barrier in front of it (hipExtAnyOrderLaunch) and overlaps the
 *     kernel queued before it on `stream` -- the previous step's blur; the blur of this step waits for it as for any earlier
 *     launch.
 *   tables_dev != NULL: dib_tap_tables_bytes(K, num_psfs) bytes owned by the caller; two ordinary launches.  Required
 *     while `stream` is being captured into a HIP graph (a replay must not touch the library's buffers): without it the
 *     call returns DIB_ECAPTURE and launches nothing.
 * Results are those of the two separate calls, bit for bit.  No host synchronisation (except when a batch outgrows the
 * stream's table buffers: that call waits for the stream once).
 * ------------------------------------------------------------------------------------- */
#define DIB_STEP_PSFS_COMPLETE 1
#define DIB_STEP_LARGE_WINDOW 2 /* compact for and blur with the large LDS window (see DIB_WINDOW_LARGE) */
int dib_blur_step(const void *const *psf_ptrs, int psf_dtype, int num_psfs, int K, int normalize,
                  const void *const *in_dev, void *const *out_dev, const int *C, const int *H, const int *W,
                  const int *table_index, int B, int dtype, int acc_mode, void *tables_dev, int flags,
                  void *stream);
/* dib_blur_step with its nine host arrays packed into two (for callers that pay per array they marshal, e.g. ctypes):
 * ptrs = psf_ptrs[num_psfs] | in_dev[B] | out_dev[B];  ints = C[B] | H[B] | W[B] | table_index[B]. */
int dib_blur_step_packed(const void *const *ptrs, const int *ints, int psf_dtype, int num_psfs, int K, int normalize, int B,
                         int dtype, int acc_mode, void *tables_dev, int flags, void *stream);
int dib_blur_step_release(void);
/* The library's own table buffers are bounded: at most 8 streams per device keep a pair; a ninth stream takes over the least
 * recently used one's (behind one device synchronisation: that stream's last step may still be running, or the stream may be
 * gone).  A process that cycles through short-lived streams therefore holds at most 16 buffers per device.
 *
 * dib_blur_step_ws: the same step on a workspace the CALLER owns -- no allocation, no library state, usable from any number of
 * streams (one workspace per stream in flight).  workspace_dev: dib_blur_step_workspace_bytes(K, num_psfs) bytes of device
 * memory, 256-byte aligned (hand-off words first, the tables behind them; size it for the largest batch).  ws_state: ONE host word
 * per workspace, in / out: 0 before the workspace's first use -- that call clears the hand-off words with one
 * hipMemsetAsync on `stream` --, updated by every call.  All launches are ordinary stream-ordered ones, so one buffer
 * suffices: step n + 1's compaction cannot start before step n's blur has read its tables.  While `stream` is being captured
 * into a graph the call makes two ordinary launches into the workspace's table area (a replay cannot advance ws_state).
 * Everything else as dib_blur_step with tables_dev == NULL; results bit-identical. */
size_t dib_blur_step_workspace_bytes(int K, int num_psfs);
int dib_blur_step_ws(const void *const *psf_ptrs, int psf_dtype, int num_psfs, int K, int normalize,
                     const void *const *in_dev, void *const *out_dev, const int *C, const int *H, const int *W,
                     const int *table_index, int B, int dtype, int acc_mode, void *workspace_dev, size_t workspace_bytes,
                     unsigned long long *ws_state, int flags, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fused epilogue of the blur for the detector's input: `.float()` (engine.py:107-110), per-image
 * `(x - mean) / std` (models/net_transforms.py:112-121, :135-139) and the zero-padded batch
 * (net_transforms.py:238-247) in one pass, for batches whose images need no resize (scale factor 1).
 * in_dev: host array of B device pointers to 3 x H[i] x W[i] planar images of `dtype`; mean / std:
 * host arrays [B][3] (fp32: the values torch.as_tensor(row, dtype=float32) would hold);
 * out_dev: [B][3][Hp][Wp] fp32, planar (channels_last = 0) or stored channels-last, i.e. as
 * [B][Hp][Wp][3] (channels_last != 0); Hp >= H[i], Wp >= W[i]; pixels outside an image become 0.
 * Same arithmetic as the reference (fp32 subtract, IEEE divide): bit-identical results.
 * ------------------------------------------------------------------------------------- */
int dib_normalize_pad(const void *const *in_dev, int dtype, const int *H, const int *W, int B,
                      const float *mean, const float *std, float *out_dev, int Hp, int Wp,
                      int channels_last, void *stream);

/* The same epilogue for batches whose images need the detector's internal resize (every native-size COCO batch: the reference
 * blurs before the model resizes, engine.py:101 -> models/net_transforms.py:151-175): float conversion, per-image normalisation,
 * bilinear resize to Ho[i] x Wo[i] -- torch.nn.functional.interpolate(mode="bilinear", recompute_scale_factor=True,
 * align_corners=False) as ATen computes it on the GPU, the scale recomputed from the integer sizes -- and the zero-padded batch,
 * one launch.  Ho / Wo: host arrays, the output size of image i (the caller's int(H * scale), net_transforms.py:36-46,167);
 * an image with Ho == H and Wo == W is not interpolated (the reference skips the call at scale factor 1).  Everything else as
 * dib_normalize_pad.  Bit-identical to the unfused GPU path; within 2e-6 of the reference's CPU result. */
int dib_normalize_resize_pad(const void *const *in_dev, int dtype, const int *H, const int *W, const int *Ho, const int *Wo, int B,
                             const float *mean, const float *std, float *out_dev, int Hp, int Wp, int channels_last,
                             void *stream);

/* The estimator's input batch (engine_blur_estimator.py:221-258 and the ensemble router, engine.py:259-265, :354-366): the
 * arguments and the arithmetic of dib_normalize_resize_pad, then the TOP-LEFT CROP of models/net_transforms.py:226-236
 * (`crop_images`): out_dev is [B][3][Hc][Wc] fp32 (planar or channels-last as above) and holds rows 0..Hc-1, columns 0..Wc-1 of
 * every resized, normalised image.  Hc <= Ho[i] and Wc <= Wo[i] for every image, or DIB_EINVAL: nothing is ever padded.  B > 32
 * is split into launches of 32 images.  flags:
 *   DIB_EPILOGUE_QUANTIZE  (fp16 images only, else DIB_EINVAL) every source pixel first goes through the reference's
 *       `(img * 255).type(torch.uint8).type(torch.half) / 255` (engine_blur_estimator.py:217) as ATen evaluates it on Half:
 *       a = half(float(x) * 255.f), k = a truncated to an integer (uint8(int64(a))), q = half(float(k) / 255.f); IEEE divide, no
 *       contraction.  Domain: finite x >= 0 with half(x * 255) < 256 (every x <= 1.0029297); outside it the result is whatever the
 *       compiler's Half -> int64 -> uint8 conversion gives, as in ATen.
 *   DIB_EPILOGUE_PAD  the zero-padded batch of dib_normalize_resize_pad instead of the crop (Hc >= Ho[i], Wc >= Wo[i], pixels
 *       outside an image become 0): dib_normalize_resize_pad with flags, for DIB_EPILOGUE_QUANTIZE in the detector's batch mode.
 * Bit-identical to the unfused GPU path (quantise expression, .float(), normalize, interpolate, crop copy). */
#define DIB_EPILOGUE_QUANTIZE 1
#define DIB_EPILOGUE_PAD 2
int dib_normalize_resize_crop(const void *const *in_dev, int dtype, const int *H, const int *W, const int *Ho, const int *Wo, int B,
                              const float *mean, const float *std, float *out_dev, int Hc, int Wc, int channels_last, int flags,
                              void *stream);

/* The blur WITH that epilogue as its store phase: dib_sparse_blur + dib_normalize_pad in one launch, for batches whose images
 * need no resize (the model's internal scale factor is 1: BASELINE's synthetic 800 x 1333; the reference blurs, engine.py:101,
 * converts to float, :107-110, and normalises + pads inside the model, net_transforms.py:112-121, :238-247 -- the blurred fp16
 * image never has to exist).  in_dev: B device pointers to 3 x H[i] x W[i] fp16 images, table_index[i] >= 0 the table of
 * tables_dev image i uses; slot (may be NULL = identity): the batch position image i goes to (the caller may hand the images over
 * heaviest PSF first); mean / std: host [B][3] in the order of in_dev; out_dev: [B][3][Hp][Wp] fp32 planar or channels-last as
 * dib_normalize_pad, padding pixels are written as 0 by the launch.  acc_mode: every mode dib_sparse_blur serves on the standard
 * LDS window -- DIB_ACC_BITEXACT, DIB_ACC_FP32 (K = 128 and 256), DIB_ACC_FMA16, DIB_ACC_FAST16 (K = 128; on tables compacted without
 * DIB_COMPACT_VRUNS it runs DIB_ACC_FMA16's row-major loop, as in dib_sparse_blur) -- without DIB_WINDOW_LARGE: the large window is
 * not served here, tables compacted with DIB_COMPACT_LARGE_WINDOW go through dib_sparse_blur.
 * Returns DIB_OK, a negative error, or 1 = "not served, nothing launched" (an image that is not blurred, more than 32 images, a
 * padded extent the image's own tiles do not cover: Hp > ceil(H / 32) * 32 or Wp > ceil(W / 128) * 128, DIB_ACC_FAST16 at
 * K = 256): the caller then takes the two-launch path.  Bit-identical to dib_sparse_blur in the same mode followed by
 * dib_normalize_pad. */
int dib_sparse_blur_normalized(const void *const *in_dev, const int *H, const int *W, const int *table_index, const int *slot, int B,
                               void *tables_dev, int num_tables, int K, int acc_mode, const float *mean, const float *std,
                               float *out_dev, int Hp, int Wp, int channels_last, void *stream);

/* ---------------------------------------------------------------------------------------
 * Box growth and clamping: utils.py:360-392 (`expand_targets`, one image) and utils.py:395-434
 * (`fix_bounding_box_squeeze`).  boxes_dev: [N][4] float32 xyxy, updated in place.
 * ------------------------------------------------------------------------------------- */
int dib_expand_boxes(float *boxes_dev, int N, const void *table_dev, int H, int W, void *stream);
int dib_clamp_boxes(float *boxes_dev, int N, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------
 * PSF rasteriser: motion_blur/generate_PSF.py:31-83 (`PSF.fit`, single exposure fraction) and
 * :106-123 (`centerPSF`), then the centre crop of transforms.py:334-335, batched.
 * traj_dev: [B][iters] complex128 (re, im interleaved); fraction: host array [B].
 * canvas x canvas float64 accumulation in the reference's order (sample index ascending per
 * cell), so psf64_dev is bit-identical to the reference's float64 PSF.
 *   center != 0: roll the weighted centroid to the canvas centre;
 *   out_n: canvas, or 128 with canvas 256 for the [64:192] crop.
 * psf64_dev: [B][out_n][out_n] float64 (may be NULL); psf16_dev: same shape, float16 converted
 * as torch.HalfTensor(ndarray) does (float64 -> float32 -> float16; engine.py:84) (may be NULL).
 * workspace_dev: dib_psf_rasterize_workspace_bytes(B, iters, canvas) bytes.
 * Canvas border.  Low side: a coordinate below 1 (negative ones included) is clamped to cell 1
 * as the reference clamps it (:59, :61), and splats there with its (vanishing) triangle weights.
 * High side: a sample with floor(coord) >= canvas - 1 on either axis contributes only the cells
 * inside the canvas -- its splats on row or column `canvas` are dropped, and one further out
 * contributes nothing; the reference raises IndexError there (its accumulator has no such row),
 * whatever the sample's exposure weight, and so does the host path (dib_psf_fit returns -2).  A
 * kernel cannot raise without a synchronisation, so a caller that holds the trajectory on the
 * host checks it before the upload (blur_ops.rasterize_psfs does); device-resident input
 * follows the rule above.
 * B == 0 is DIB_OK and launches nothing; canvas outside {64, 128, 256}, any other out_n,
 * iters <= 0, B < 0, or a null traj_dev / fraction / workspace_dev with B > 0 is DIB_EINVAL.
 * ------------------------------------------------------------------------------------- */
size_t dib_psf_rasterize_workspace_bytes(int B, int iters, int canvas);
int dib_psf_rasterize(const double *traj_dev, int B, int iters, const double *fraction, int canvas,
                      int center, int out_n, double *psf64_dev, void *psf16_dev,
                      void *workspace_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * Detector ops the blurred batches feed (torchvision is not a dependency): RoIAlign as used by
 * torchvision.ops.MultiScaleRoIAlign(output_size=7, sampling_ratio=2) (reference
 * models/faster_rcnn.py:204-208) and NMS as used by RegionProposalNetwork / RoIHeads
 * (reference models/faster_rcnn.py:198-229).  fp32, NCHW.
 *   rois_dev: [K][5] = (batch index, x1, y1, x2, y2) in image coordinates.
 *   dib_roi_align_backward ACCUMULATES into grad_feat_dev (caller zero-fills it first).
 *   dib_nms: boxes [n][4] xyxy already sorted by descending score; keep_dev receives the kept
 *   indices (ascending = score order; entries past the count are 0), count_dev their number;
 *   workspace of dib_nms_workspace_bytes(n).
 * ------------------------------------------------------------------------------------- */
int dib_roi_align_forward(const float *feat_dev, const float *rois_dev, int K, int C, int H, int W,
                          float spatial_scale, int pooled, int sampling_ratio, int aligned,
                          float *out_dev, void *stream);
int dib_roi_align_backward(const float *grad_out_dev, const float *rois_dev, int K, int C, int H,
                           int W, float spatial_scale, int pooled, int sampling_ratio, int aligned,
                           float *grad_feat_dev, void *stream);
 /* Channels-last (NHWC) form over 1..4 pyramid levels in ONE launch: MultiScaleRoIAlign without the
 * per-level index_select / scatter (and their host syncs).  feat_dev / grad_feat_dev: host arrays of
 * n_levels device pointers to [N][H_l][W_l][C] fp32; H, W, scale: host arrays [n_levels];
 * level_dev: device int32 [K], the level of each RoI (may be NULL when n_levels == 1);
 * out / grad_out: [K][C][pooled][pooled] contiguous, as above.  pooled <= 7. */
int dib_roi_align_nhwc_forward(const float *const *feat_dev, const int *H, const int *W, const float *scale,
                               int n_levels, const float *rois_dev, const int *level_dev, int K, int C, int pooled,
                               int sampling_ratio, int aligned, float *out_dev, void *stream);
int dib_roi_align_nhwc_backward(const float *grad_out_dev, const int *H, const int *W, const float *scale,
                                int n_levels, const float *rois_dev, const int *level_dev, int K, int C, int pooled,
                                int sampling_ratio, int aligned, float *const *grad_feat_dev, void *stream);
size_t dib_nms_workspace_bytes(int n);
int dib_nms(const float *boxes_sorted_dev, int n, float iou_threshold, void *workspace_dev,
            long long *keep_dev, int *count_dev, void *stream);
/* B independent box sets of n boxes each in one launch pair (RPN: one set per image).  boxes [B][n][4],
 * keep [B][n] (entries past count[b] are 0), count [B]; valid_dev (may be NULL): [B][n] bytes, 0 = the
 * box takes no part (neither kept nor suppressing), which replaces a compaction + host sync in front
 * of the call; workspace: B * dib_nms_workspace_bytes(n). */
int dib_nms_batched(const float *boxes_sorted_dev, const unsigned char *valid_dev, int B, int n,
                    float iou_threshold, void *workspace_dev, long long *keep_dev, int *count_dev,
                    void *stream);

/* ---------------------------------------------------------------------------------------
 * Box bookkeeping of the training step (torchvision's box_iou + Matcher + BoxCoder as the reference's RPN / RoIHeads use
 * them, models/faster_rcnn.py:150-159, 198-229) for a whole batch per launch.  Ground truth is ragged: gt_cat_dev holds every
 * image's boxes back to back ([T][4] xyxy), gt_offset (HOST, N + 1 ints) where each image's boxes start; at most 32 images, at
 * most 256 boxes per image.  Candidates (anchors / proposals): cand_dev [N][M][4], or [M][4] shared by every image
 * (cand_shared != 0).  Same operations in the same order as the tensor expressions (IoU thresholds fall the same way).
 *   dib_box_match: match_dev [N][M] int64 = index (inside the image's list) of the ground truth of highest IoU, lowest index
 *     on ties; -1 where that IoU < low, -2 where low <= IoU < high; with allow_low_quality every candidate that realises some
 *     ground truth's best IoU keeps its index (best_dev: workspace of T unsigned).  Images without ground truth: -1.
 *   dib_box_encode_matched: targets_dev [N][M][4] = BoxCoder(weights).encode(gt[max(match, 0)], candidate) and / or
 *     matched_dev [N][M][4] = that ground-truth box (a zero box for images without ground truth); either may be NULL.
 *   dib_box_decode: out [R][4] = BoxCoder.decode(deltas [R][4], anchors [A][4]), row r against anchor r % A,
 *     dw / dh clamped at `clip` (log(1000 / 16)).
 * ------------------------------------------------------------------------------------- */
int dib_box_match(const float *gt_cat_dev, const int *gt_offset, int N, const float *cand_dev, int M, int cand_shared, float high,
                  float low, int allow_low_quality, unsigned *best_dev, long long *match_dev, void *stream);
int dib_box_encode_matched(const float *gt_cat_dev, const int *gt_offset, int N, const long long *match_dev, const float *cand_dev, int M,
                           int cand_shared, float wx, float wy, float ww, float wh, float *targets_dev, float *matched_dev, void *stream);
int dib_box_decode(const float *deltas_dev, const float *anchors_dev, long long R, int A, float wx, float wy, float ww, float wh,
                   float clip, float *out_dev, void *stream);
/* act(in + bias[c]) with the layout change between channels-last and planar in the same pass (inference: around the 3x3
 * convolutions that run through MIOpen's planar kernels).  to_planar = 1: in [N][HW][C] -> out [N][C][HW]; 0: in [N][C][HW] ->
 * out [N][HW][C].  Values identical to dib_bias_act_nhwc followed by a copy.  in_dev and out_dev must not alias. */
int dib_bias_act_transpose(const float *in_dev, const float *bias_dev, float *out_dev, int N, int C, long long HW, int to_planar, int relu,
                           void *stream);
/* Sorted top-k of every (image, level) row of scores in one launch (torchvision filter_proposals' per-level torch.topk + gather +
 * clip_boxes_to_image + the small-box test, reference models/faster_rcnn.py:198-207 sets the counts).  values_dev: [N][row_stride];
 * level l covers elements level_offset[l] .. level_offset[l + 1] of a row and yields its level_k[l] (<= K <= 2048) highest scores in
 * descending order -- equal scores in ascending index order, NaN first -- into out_scores_dev [N][L][K] (rows shorter than K end in
 * -inf), their level-relative indices into out_index_dev (optional).  With boxes_dev ([N][row_stride][4], same indexing): the
 * winners' boxes into out_boxes_dev [N][L][K][4], clipped to clip_wh_dev[n] = (width, height) when that is given, and
 * out_valid_dev [N][L][K] = score > -inf and both clipped sides >= min_size.  L <= 32.  (A long row is bound by the one compute unit
 * that sweeps it: callers split it into consecutive levels and merge the winners with a second call -- the order is the same.)
 * The order, pinned by tests/test_selection_gpu.py against a stable sort: -0 and +0 are equal scores (each keeps its sign in
 * out_scores_dev); denormals are numbers, above or below the zeros and never equal to them; NaN comes first, above +inf; equal
 * scores -- the zeros, NaNs among themselves, -inf when a level has fewer than level_k[l] numbers -- come out in ascending
 * level-relative index order, and when a run of equal scores straddles place level_k[l], its lowest indices are the ones taken.
 * Only columns level_offset[0] .. level_offset[L] of a row are read (level_offset[0] may be > 0, row_stride beyond the last level). */
int dib_topk_levels(const float *values_dev, long long row_stride, int N, const int *level_offset, const int *level_k, int L, int K,
                    const float *boxes_dev, const float *clip_wh_dev, float min_size, float *out_scores_dev, long long *out_index_dev,
                    float *out_boxes_dev, unsigned char *out_valid_dev, void *stream);
/* Detections of one image up to the NMS (torchvision RoIHeads.postprocess_detections; reference models/faster_rcnn.py:213-229): softmax
 * over the C <= 128 class logits of every RoI (ATen's operation order), per-class box decoding with BoxCoder weights (wx, wy, ww, wh)
 * and the log(1000 / 16) clip, clipping to the image, the score > score_thresh and side >= min_size tests.  logits_dev [R][C],
 * deltas_dev [R][4 C], rois_dev [R][4].  Class-major outputs without the background class: scores_cm_dev [C - 1][R] (-inf where the
 * candidate is dropped), boxes_cm_dev [C - 1][R][4]; stats_dev[0] = number of candidates kept, stats_dev[1] = bit pattern of the
 * largest coordinate among them (what batched_nms moves the classes apart by). */
int dib_det_candidates(const float *logits_dev, const float *deltas_dev, const float *rois_dev, int R, int C, float img_h, float img_w, float wx,
                       float wy, float ww, float wh, float clip, float score_thresh, float min_size, float *scores_cm_dev, float *boxes_cm_dev,
                       unsigned *stats_dev, void *stream);
/* RoI-head candidate pool: cands[n] = proposals[n] (P rows) ++ the ground truth of image n ++ [0, 0, 1, 1] rows up to P + Gpad
 * (torchvision RoIHeads.add_gt_proposals with a fixed shape).  cands_dev: [N][P + Gpad][4]. */
int dib_box_pool(const float *proposals_dev, int P, const float *gt_cat_dev, const int *gt_offset, int N, int Gpad, float *cands_dev, void *stream);
/* Class per pool row (RoIHeads.assign_targets_to_proposals): gt_labels[match] for match >= 0, 0 for -1, -1 for -2 and for padding
 * rows (proposal rows whose ok byte is 0 -- ok_dev may be null: all live --, ground-truth rows beyond the image's count).
 * match_dev / labels_dev: [N][M] int64, M >= P; gt_labels_cat_dev: int64, concatenated like the boxes. */
int dib_box_labels(const long long *match_dev, const long long *gt_labels_cat_dev, const int *gt_offset, int N, const unsigned char *ok_dev, int P,
                   int M, long long *labels_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * COCO box IoU: pycocotools' bbIou (reference cocoapi/common/maskApi.c:109-120), the inner loop of the
 * evaluation sweep's COCOeval.  dt_dev [m][4], gt_dev [n][4]: float64 (x, y, w, h); iscrowd_dev [n]
 * bytes or NULL; out_dev [n][m] float64 = intersection / union (union = detection area for crowd
 * ground truth), bit-identical to the C routine.
 * ------------------------------------------------------------------------------------- */
int dib_coco_box_iou(const double *dt_dev, const double *gt_dev, const unsigned char *iscrowd_dev, int m, int n,
                     double *out_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * Convolution epilogue of the ResNet-50 trunk with its frozen batch-norm folded into the weights
 * (reference models/faster_rcnn.py:367 builds the trunk with torchvision's FrozenBatchNorm2d):
 *   x = act(x + bias[c] (+ residual)), in place, channels-last fp32 (channel index fastest);
 * one pass instead of eager PyTorch's 2-4.  residual_dev may be NULL; relu != 0 applies ReLU as torch does (clamp_min(0)):
 * a NaN goes through, everything else that is not > 0 becomes +0.  The same ReLU is in dib_bias_act_transpose, in
 * dib_bn_mode_one_nhwc and in the bf16 forms below.
 * ------------------------------------------------------------------------------------- */
int dib_bias_act_nhwc(float *x_dev, const float *bias_dev, const float *residual_dev, long long n_elems,
                      int C, int relu, void *stream);

/* The ReLU form of the above that also leaves what its backward pass needs of the result: mask_dev[n_elems / 4],
 * one byte per 4 consecutive elements, bit k = element 4 i + k is > 0 -- a NaN element is stored as NaN and carries no bit
 * (C % 4 == 0, 16-byte aligned tensors).
 * dib_relu_mask_backward: grad_out = mask ? grad_in : 0 -- torch's threshold_backward(grad, y, 0) (the ReLU backward
 * behind every trunk convolution, reference models/faster_rcnn.py:367 / torchvision Bottleneck) at 8.25 instead of
 * 12 bytes per element; grad_out may alias grad_in. */
int dib_bias_act_mask_nhwc(float *x_dev, const float *bias_dev, const float *residual_dev, long long n_elems,
                           int C, unsigned char *mask_dev, void *stream);
int dib_relu_mask_backward(const float *grad_in_dev, const unsigned char *mask_dev, float *grad_out_dev,
                           long long n_elems, void *stream);
/* Gradient accumulation at a residual block's input (torchvision Bottleneck: the block input feeds conv1 AND the skip
 * connection, autograd adds the two gradients) fused with the ReLU backward of that input: a = (a + b), zeroed where the
 * mask bit is clear; mask_dev NULL = plain in-place accumulate. */
int dib_add_relu_mask(float *a_dev, const float *b_dev, const unsigned char *mask_dev, long long n_elems, void *stream);
/* The same accumulation for the first block of a ResNet stage, whose skip is a strided 1x1 convolution: the data gradient
 * of that convolution, computed densely on the strided pixels, is added in place into the data gradient of conv1:
 * a[n, ys * stride, xs * stride, :] += b[n, ys, xs, :] (channels-last fp32, C % 4 == 0) -- instead of a zero-filled
 * full-size gradient and a full-size add. */
int dib_scatter_add_nhwc(float *a_dev, const float *b_dev, int N, int H, int W, int Hs, int Ws, int C, int stride, void *stream);
/* FPN top-down merge (torchvision FeaturePyramidNetwork.forward: inner = lateral + interpolate(top, size, "nearest")) in one
 * in-place pass on the lateral convolution's output: x[n, h, w, :] += bias[:] + top[n, sh, sw, :], sh = min(int(floorf(h *
 * float(Ht) / H)), Ht - 1) (ATen's nearest index) -- instead of a bias add, an upsample that writes a full-size tensor and an
 * add that reads it back. */
int dib_fpn_topdown_merge_nhwc(float *x_dev, const float *bias_dev, const float *top_dev, int N, int H, int W, int Ht, int Wt, int C,
                               void *stream);
/* ResNet stem (torchvision resnet50: conv1 -> bn1 -> relu -> maxpool(3, stride 2, padding 1)) behind the folded convolution:
 * out[N, Ho, Wo, C] = max_pool2d(relu(x + bias)), Ho = (H - 1) / 2 + 1, in one pass; arg_dev: one unsigned short per 4 output
 * channels (4-bit window position of the winner, 15 = no gradient: the maximum is neither > 0 nor NaN).  ATen's selection: the
 * first maximum in row-major window order wins; a NaN beats every number and the LAST NaN of a window is the recorded one; the
 * pooled value of such a window is NaN (not 0) and its gradient goes to that position.  The backward pass turns grad_out + arg
 * into the dense gradient of x (max-pool backward and ReLU backward in one pass).  Channels-last fp32, C % 4 == 0, 16-byte
 * aligned. */
int dib_stem_pool_forward(const float *x_dev, const float *bias_dev, float *out_dev, unsigned short *arg_dev, int N, int H, int W, int C,
                          void *stream);
int dib_stem_pool_backward(const float *grad_out_dev, const unsigned short *arg_dev, float *grad_in_dev, int N, int H, int W, int C,
                           void *stream);

/* bfloat16 forms of the epilogues above (the trunk under `--amp`, models/backbone.py): activations, residuals and gradients are
 * channels-last bf16 (raw 16-bit words), bias vectors stay fp32.  Each upcasts, runs the fp32 kernel's arithmetic in its order
 * and rounds once to nearest even at the store (NaN stays NaN, +-inf stays): bit-identical to the torch expression evaluated in
 * fp32 and cast once.  8 elements per lane: C % 8 == 0 (n_elems % 8 == 0), 16-byte aligned tensors, no scalar variant.
 *   dib_bias_act_bf16_nhwc / _mask_:  x = bf16(act(float(x) + bias[c] (+ float(residual)))) in place; mask_dev[n_elems / 8], one byte
 *       per 8 consecutive elements, bit k = STORED element 8 i + k is > 0
 *   dib_relu_mask_backward_bf16:      grad_out = mask ? grad_in : +0 (may alias)
 *   dib_add_relu_mask_bf16:           a = bf16(float(a) + float(b)), then zeroed where the mask bit is clear (mask_dev NULL: plain add)
 *   dib_scatter_add_bf16_nhwc:        a[n, ys * stride, xs * stride, :] = bf16(float(a) + float(b[n, ys, xs, :]))
 *   dib_fpn_topdown_merge_bf16_nhwc:  x = bf16((float(x) + bias) + float(top at ATen's nearest source pixel)) in place
 *   dib_stem_pool_forward_bf16:       the stem's 7x7 convolution stays fp32 (3 input channels): x_dev fp32, out_dev bf16 =
 *       bf16(max_pool2d(relu(x + bias))), window order, tie rule and arg_dev exactly as dib_stem_pool_forward (C % 4 == 0)
 *   dib_stem_pool_backward_bf16:      grad_out_dev bf16 + arg -> grad_in_dev fp32 (summed in fp32 in dib_stem_pool_backward's order) */
int dib_bias_act_bf16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C, int relu, void *stream);
int dib_bias_act_mask_bf16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C,
                                unsigned char *mask_dev, void *stream);
int dib_relu_mask_backward_bf16(const void *grad_in_dev, const unsigned char *mask_dev, void *grad_out_dev, long long n_elems, void *stream);
int dib_add_relu_mask_bf16(void *a_dev, const void *b_dev, const unsigned char *mask_dev, long long n_elems, void *stream);
int dib_scatter_add_bf16_nhwc(void *a_dev, const void *b_dev, int N, int H, int W, int Hs, int Ws, int C, int stride, void *stream);
int dib_fpn_topdown_merge_bf16_nhwc(void *x_dev, const float *bias_dev, const void *top_dev, int N, int H, int W, int Ht, int Wt, int C,
                                    void *stream);
int dib_stem_pool_forward_bf16(const float *x_dev, const float *bias_dev, void *out_dev, unsigned short *arg_dev, int N, int H, int W, int C,
                               void *stream);
int dib_stem_pool_backward_bf16(const void *grad_out_dev, const unsigned short *arg_dev, float *grad_in_dev, int N, int H, int W, int C,
                                void *stream);

/* The IEEE Half form of dib_bias_act_nhwc, the only Half member of the family: the epilogue behind every convolution of the deblurrer
 * under `evaluate.py --deblur_first --deblur_precision half` (below).  x_dev and residual_dev are channels-last Half (raw 16-bit words),
 * bias_dev an fp32 vector of ANY fp32 values: the inference stage passes the reference's Half biases, upcast; the trainer under
 * `--amp` passes its fp32 master biases, which are never rounded to Half.  It reproduces torch's Half ops in their order, each
 * computed on the upcast values and rounded once to nearest even:
 *     bias only        x = half(x + b)
 *     bias + ReLU      x = relu(half(x + b))            a NaN stays a NaN, everything else that is not > 0 becomes +0
 *     bias + residual  x = half(half(x + b) + r)        TWO roundings: the reference's ResBlock is `res = body(x); res += x` on Half
 *                                                       tensors (with relu != 0: the ReLU of that)
 * A sum beyond 65504 becomes +-inf as torch's does; Half denormals are kept.  8 elements per lane where C % 8 == 0 and the tensors
 * are 16-byte aligned; one per lane otherwise, as dib_bias_act_nhwc (the deblurrer's coarser scales end in 3 channels).  n_elems not
 * a multiple of C, null pointers, tensors not aligned to their elements: DIB_EINVAL, nothing launched. */
int dib_bias_act_f16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C, int relu, void *stream);

/* Its ReLU form with the sign mask, for training (`train_deblurrer.py --amp`): the arithmetic, the roundings and the stored bits of
 * dib_bias_act_f16_nhwc(..., relu = 1), and mask_dev[n_elems / 8]: one byte per 8 consecutive elements, bit k = STORED element
 * 8 i + k is > 0 (dib_bias_act_mask_bf16_nhwc's contract; a NaN carries no bit).  Vector form only: C % 8 == 0 and x_dev, bias_dev,
 * residual_dev 16-byte aligned; anything else, a null x_dev, bias_dev or mask_dev: DIB_EINVAL, nothing launched. */
int dib_bias_act_mask_f16_nhwc(void *x_dev, const float *bias_dev, const void *residual_dev, long long n_elems, int C,
                               unsigned char *mask_dev, void *stream);

/* Frozen batch-norm folds of n trunk convolutions in one launch per 32 (torchvision's FrozenBatchNorm2d behind every ResNet
 * convolution, reference models/faster_rcnn.py:367; training re-folds every step because the weights move):
 *   scale = bn_w * rsqrt(var + eps);  shift = bn_b - mean * scale;  wf[co][...] = w[co][...] * scale[co]
 * -- the same operations in the same order as the tensor expressions, so bit-identical to them.  Host arrays of n device
 * pointers / sizes; w[k] is Co[k] x inner[k] dense with the output channel outermost (contiguous or channels-last weights);
 * wf[k] has w[k]'s element order; scale[k], shift[k]: Co[k] floats.  dib_scale_rows_multi is the backward of the weight
 * product: dw[k][co][...] = g[k][co][...] * scale[k][co]. */
int dib_fold_bn_multi(const float *const *w, const float *const *bn_w, const float *const *bn_b, const float *const *mean,
                      const float *const *var, const int *Co, const int *inner, int n, float eps, float *const *wf,
                      float *const *scale, float *const *shift, void *stream);
int dib_scale_rows_multi(const float *const *g, const float *const *scale, const int *Co, const int *inner, int n,
                         float *const *dw, void *stream);

/* ---------------------------------------------------------------------------------------
 * Post-blur corruption chain of manual_blur (reference models/blur_functions.py:72-81) in one pass:
 *   noise_var > 0:    out = clamp(in + N(0, noise_var), 0, 1)                    (:72-74, --add_noise)
 *   block_scale > 0:  out = nearest-up(nearest-down(., scale_factor = block_scale), size = original)   (:76-81, --add_block)
 * applied in that order (the noise of a source pixel travels with it into every block copy).  The block path equals
 * torch's two interpolate calls bit for bit; the noise field comes from a counter-based generator keyed by `seed`
 * (same distribution and rounding steps as torch's expression, not torch's sample values).  C x H x W planes of
 * DIB_F16 / DIB_F32; out must not alias in.  The host draws (variance, coin flip, scale factor) stay with the caller, in
 * the reference's order on numpy's global stream.
 * ------------------------------------------------------------------------------------- */
int dib_post_ops(const void *in_dev, void *out_dev, int C, int H, int W, int dtype, double noise_var,
                 unsigned long long seed, double block_scale, void *stream);

/* JPEG round trip of one image in one launch (reference transforms.py:467-493 around models/jpeg/DiffJPEG.py:
 * reflect-pad to a multiple of 16, RGB -> YCbCr 4:2:0 -> 8x8 DCT -> quantise with table x factor -> back -> crop).
 * in_dev: 3 x H x W planes of DIB_F16 / DIB_F32 in [0, 1]; out_dev: 3 x H x W planes of fp16 (the reference returns
 * `.half()`); q_luma / q_chroma: HOST pointers to the 8 x 8 tables already multiplied by the quality factor, row-major
 * [u][v].  fp32 arithmetic as the reference's; the DCT sums run in this kernel's order: results within one
 * quantisation step of the reference's (tests/test_jpeg.py), as torch's own GPU path is. */
int dib_jpeg_roundtrip(const void *in_dev, void *out_dev, int H, int W, int dtype, const float *q_luma,
                       const float *q_chroma, void *stream);

/* ---------------------------------------------------------------------------------------
 * Test-time batch-norm statistics, the reference's `--mode_one_norm` (models/batchnorm.py:159-184): every batch-norm layer
 * of the trunk normalises with its running statistics mixed with those of the batch it sees,
 *   mean = f * running_mean + g * mean_b,  var = f * running_var + g * var_b   (biased batch variance over N * H * W),
 *   f = float(n) / float(n + 1),  g = 1 / float(n + 1),  n = num_batches_tracked,
 *   x = act(x * scale[c] + shift[c] (+ residual)),  scale = w / sqrt(var + eps),  shift = b - mean * scale,
 * in place on a channels-last fp32 activation x_dev [n_pix][C] (C % 4 == 0; x, residual and workspace 16-byte aligned).
 * weight_dev / bias_dev may be NULL (1 and 0).  n comes from num_batches_dev (one int64 on the device, read there) or, when
 * that is NULL, from num_batches.  workspace_dev: dib_bn_mode_one_workspace_bytes(n_pix, C) bytes of device memory, no
 * initial contents needed (0: bad shape).  stats_dev, optional: [2][C] floats, the mixed mean and variance.  Three launches,
 * no atomics, no host synchronisation: deterministic and capturable into a graph.
 * ------------------------------------------------------------------------------------- */
size_t dib_bn_mode_one_workspace_bytes(long long n_pix, int C);
int dib_bn_mode_one_nhwc(float *x_dev, const float *residual_dev, long long n_pix, int C, const float *weight_dev, const float *bias_dev,
                         const float *running_mean_dev, const float *running_var_dev, const long long *num_batches_dev,
                         long long num_batches, float eps, int relu, void *workspace_dev, size_t workspace_bytes, float *stats_dev,
                         void *stream);

/* ---------------------------------------------------------------------------------------
 * Online batch-norm statistics, the reference layer's `acclimation_mode` (models/batchnorm.py:142-157; `evaluate.py
 * --acclimate_norm`): the layer first folds the statistics of the batch it sees into its running statistics, as
 * F.batch_norm(..., training=True, a) does, then normalises with the UPDATED running statistics, as
 * F.batch_norm(..., training=False) does.  Per channel, every product and sum rounded separately:
 *   n   = *num_batches_dev + (bump ? 1 : 0)                              (stored back when bump)
 *   a   = momentum >= 0 ? momentum : bump ? float(1.0 / double(n)) : 0   (negative momentum: cumulative average)
 *   rm' = (1 - a) * rm + a * mean_b,   rv' = (1 - a) * rv + a * M2 / (n_pix - 1)        (the UNBIASED batch variance)
 *   x   = act(x * scale[c] + shift[c] (+ residual)),  scale = w / sqrt(rv' + eps),  shift = b - rm' * scale.
 * Arguments as dib_bn_mode_one_nhwc (same layout, alignment and workspace: dib_bn_mode_one_workspace_bytes), except:
 * running_mean_dev / running_var_dev are WRITTEN (rm', rv'), each channel's pair by the one lane that read it;
 * num_batches_dev (one int64 on the device, 8-byte aligned; may be NULL without bump and with momentum >= 0) is written when
 * bump is set -- by one lane of the LAST of the three launches, while the old value is read in the second only, so no read can
 * follow the write; stats_dev, optional: [4][C] floats -- batch mean, unbiased batch variance, rm', rv'.
 * n_pix < 2 is DIB_EINVAL (torch raises for one value per channel in training mode).  Three launches, no atomics, no host
 * synchronisation, nothing kept between calls but the layer's own state: deterministic and capturable into a graph, whose
 * replays then carry the state forward.
 * ------------------------------------------------------------------------------------- */
int dib_bn_acclimate_nhwc(float *x_dev, const float *residual_dev, long long n_pix, int C, const float *weight_dev, const float *bias_dev,
                          float *running_mean_dev, float *running_var_dev, long long *num_batches_dev, int bump, float momentum,
                          float eps, int relu, void *workspace_dev, size_t workspace_bytes, float *stats_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * AugMix on the device (reference transforms.py:68-79, augmix/augment_and_mix.py:123-185), from plans drawn on the host
 * (transforms.AugMix): per image three chains of up to three ops, Pillow's semantics on uint8 images, then the reference's
 * float64 mix with the COCO mean (0.485, 0.456, 0.406) and std (0.229, 0.224, 0.225), written as fp16.
 * Op codes follow the reference's `augmentations` list; iparam: posterize bits (1..8) / solarize threshold (0..256); affine:
 * Pillow's inverse affine coefficients (a0..a5: source x = a0 (x + .5) + a1 (y + .5) + a2, y likewise) of a positional op.
 * src: 3 x H x W fp32 planes holding k / 255 (k = 0..255), mirrored left-right when flip != 0 (the result is then mirrored too);
 * dst: 3 x H x W fp16 planes, must not alias src.  buf_offset: byte offset of the image's uint8 stage images inside the
 * workspace's buffer area (dib_augmix_buffer_bytes(plan) bytes each; regions of different images must not overlap).
 * plans_host and plans_dev hold the same n records (the host copy is read during the call for validation and launch sizes).
 * norm_table_dev: [3][256] doubles (k / 255 - mean_c) / std_c; scale_table_dev: [256] doubles 255.0 / d (entry 0 unused);
 * half_table_dev: [256] fp16 bits of float(k) / 255.  workspace_dev: dib_augmix_workspace_bytes(n, sum of the buffer bytes)
 * bytes, no initial contents needed.  No atomics outside LDS, no host synchronisation: deterministic and capturable.
 * ------------------------------------------------------------------------------------- */
#define DIB_AUGMIX_WIDTH 3
#define DIB_AUGMIX_MAX_DEPTH 3
#define DIB_AUGMIX_AUTOCONTRAST 0
#define DIB_AUGMIX_EQUALIZE 1
#define DIB_AUGMIX_POSTERIZE 2
#define DIB_AUGMIX_ROTATE 3
#define DIB_AUGMIX_SOLARIZE 4
#define DIB_AUGMIX_SHEAR_X 5
#define DIB_AUGMIX_SHEAR_Y 6
#define DIB_AUGMIX_TRANSLATE_X 7
#define DIB_AUGMIX_TRANSLATE_Y 8
typedef struct dib_augmix_image {
  const float *src;
  void *dst;
  unsigned long long buf_offset;
  int H, W, flip;
  int n_ops[DIB_AUGMIX_WIDTH];
  int op[DIB_AUGMIX_WIDTH][DIB_AUGMIX_MAX_DEPTH];
  int iparam[DIB_AUGMIX_WIDTH][DIB_AUGMIX_MAX_DEPTH];
  double affine[DIB_AUGMIX_WIDTH][DIB_AUGMIX_MAX_DEPTH][6];
  float ws[DIB_AUGMIX_WIDTH];
  float m, one_minus_m;  /* m and float32(1 - m), as numpy computes them */
} dib_augmix_image;
unsigned long long dib_augmix_buffer_bytes(const dib_augmix_image *plan);
size_t dib_augmix_workspace_bytes(int n_images, unsigned long long buffer_bytes);
int dib_augmix(const dib_augmix_image *plans_host, const dib_augmix_image *plans_dev, int n_images, const double *norm_table_dev,
               const double *scale_table_dev, const unsigned short *half_table_dev, void *workspace_dev, size_t workspace_bytes,
               void *stream);

/* ---------------------------------------------------------------------------------------
 * "Squint" warp, the reference's `--warp_in_model` (models/warper.py:47-50: Half affine_grid + bilinear grid_sample, zeros
 * outside, align_corners False) as one launch on fp32 activations, with no grid tensor and no Half copy of the input.
 * Per output pixel (n, i, j), with m = mats_dev[n] (Half [2][3], READ ON THE DEVICE: a captured graph sees the values its
 * buffer holds at replay), bx = base_x_dev[j], by = base_y_dev[i] (Half tables: torch's own base grid,
 * linspace(-1, 1, W) * (W - 1) / W in Half, built by the caller -- the closed form does not reproduce its rounding):
 *   gx = half((m00 * bx + m01 * by) + m02),  gy = half((m10 * bx + m11 * by) + m12)       fp32, left to right, one rounding to Half
 *   ix = ((gx + 1) * W - 1) / 2,  iy = ((gy + 1) * H - 1) / 2                             fp32
 *   out = sum over the four corners (floor(ix) + {0, 1}, floor(iy) + {0, 1}) INSIDE the image of weight * in[corner]
 * A corner inside the image is multiplied and added even at weight 0 (a NaN / inf pixel reaches the output where torch's
 * grid_sample lets it); a corner outside is skipped.  The fp32 sum is stored as is (the reference rounds it to Half once more).
 * layout: DIB_WARP_NHWC (element order N, H, W, C; C % 4 == 0 with 16-byte aligned in / out: four channels per lane) or
 * DIB_WARP_NCHW (planar).  out must not alias in.  The backward pass ADDS the input gradient of the same warp into
 * grad_in_dev (zero-filled by the caller) with float atomic adds, one lane per element of grad_out: its sums depend on arrival
 * order in the last bits.  No gradient for the matrices or tables.  No host synchronisation: capturable into a graph.
 * ------------------------------------------------------------------------------------- */
#define DIB_WARP_NHWC 0
#define DIB_WARP_NCHW 1
int dib_squint_warp_forward(const float *in_dev, float *out_dev, int N, int C, int H, int W, int layout, const unsigned short *mats_dev,
                            const unsigned short *base_x_dev, const unsigned short *base_y_dev, void *stream);
int dib_squint_warp_backward(const float *grad_out_dev, float *grad_in_dev, int N, int C, int H, int W, int layout,
                             const unsigned short *mats_dev, const unsigned short *base_x_dev, const unsigned short *base_y_dev,
                             void *stream);

/* ---------------------------------------------------------------------------------------
 * Detection overlays: the picture the reference's `evaluate` saves of every image it scores (engine.py:382-383 around
 * utils.py:322-353, `overlay_boxes_torch`) -- the image as the detector saw it with the outline of every detection above 0.5 on
 * it -- as ONE launch for up to 32 images: planar fp16 / fp32 in, tight interleaved 8-bit RGB out, outlines already drawn.
 *   in_dev[i]:  3 x H[i] x W[i] planar, contiguous, DIB_F16 or DIB_F32;  out_dev[i]: H[i] x W[i] x 3 bytes, RGB interleaved, rows
 *   tight (what PIL.Image.fromarray takes);  H[i] * W[i] <= 2^30.
 *   boxes_dev: device array of dib_overlay_box; boxes box_offset[i] .. box_offset[i + 1] - 1 (HOST array of B + 1 ints, not
 *   decreasing) belong to image i, in drawing order.  boxes_dev may be NULL when there is no box.  rgb = R | G << 8 | B << 16 of the
 *   OUTPUT (the caller reproduces the reference's colour handling: detectinblur_amd/overlay.py).
 * Pixel value: k = trunc(float(x) * 255.0f), saturated to 0..255, NaN -> 0.  For 0 <= x < 256 / 255 that is torchvision's ToPILImage
 * on a float tensor (`pic.mul(255).byte()`, what utils.py:331 calls after `.float()`); outside that domain the reference WRAPS
 * (x = 1.01 -> 257 -> 1; negative values through the int conversion) where this saturates (1.01 -> 255, -0.2 -> 0).
 * Outline of a box, after xa = min(x0, x1), xb = max(x0, x1), ya, yb likewise (corners beyond +-2^30 are taken as +-2^30).  Pixel
 * (x, y) is painted iff all of
 *   xa - 1 <= x <= xb + 1 and ya - 1 <= y <= yb + 1;
 *   NOT (xa + 2 <= x <= xb - 2 and ya + 2 <= y <= yb - 2)                 (the interior);
 *   NOT (x in {xa - 1, xb + 1} and y in {ya - 1, yb + 1})                 (the four outermost corner pixels);
 *   the pixel lies inside the image (boxes are clipped; a box entirely outside paints nothing).
 * A degenerate box (xa == xb or ya == yb) follows the same rule.  Where outlines overlap, the LAST painting box in drawing order wins,
 * as a sequence of cv2.rectangle calls leaves it.  This rule is a reading of OpenCV's rectangle(thickness = 2) -- a closed polyline of
 * thick lines: every edge a filled quad one pixel either side of the line, every vertex a filled circle of radius 1, which OpenCV draws
 * as a plus.  It is the SPECIFICATION here and is NOT PINNED against cv2 (cv2 is not a dependency of this project and was not
 * available where this was written).
 * No atomics, no allocation, no host synchronisation: capturable into a graph.  B <= 32 (DIB_EINVAL beyond: split the list).
 * ------------------------------------------------------------------------------------- */
typedef struct dib_overlay_box { int x0, y0, x1, y1; unsigned int rgb; } dib_overlay_box;
int dib_overlay_rgb8(const void *const *in_dev, int dtype, const int *H, const int *W, int B, const dib_overlay_box *boxes_dev,
                     const int *box_offset, unsigned char *const *out_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * The deblur-first stage (reference engine.py:319-322, models/deblur/deblurInterface.py:42-63, `evaluate.py --deblur_first`):
 * everything around MSResNet's convolutions, on the device.  The convolutions themselves are MIOpen's, each followed by
 * dib_bias_act_nhwc.  n = n_scales, d = 2^(n - 1), Hp / Wp = H / W rounded up to multiples of d.
 *
 * dib_deblur_pyramid: in_dev planar [3][H][W] Half or fp32 in [0, 1] -> levels_dev[s] (HOST array of n device pointers), level s a
 *   channels-last fp32 [Hp >> s][Wp >> s][6] tensor whose channels 0..2 are written (3..5: dib_deblur_shuffle_concat), the coarsest
 *   level [..][3].  n launches.
 *     quantise  q = trunc(x * 255), the product rounded in the image's own dtype first (Half 0.50195312 -> 128), clamped to 0..255,
 *               NaN -> 0.  The reference's uint8 conversion of a value outside 0..255 is undefined; the clamp is this library's choice.
 *     pad       bottom and right, mode "edge".
 *     level s   level s - 1 smoothed per channel by a separable 7-tap Gaussian (sigma 2/3, weights exp(-x^2 / (2 sigma^2)) normalised in
 *               float64, rounded to fp32), down the columns first, then along the rows, boundary "reflect" (d c b a | a b c d, periodic
 *               when the halo is longer than the image); then the mean of each 2 x 2 block.  Products are accumulated from the first
 *               tap to the last, the block as 0.25 * ((a + b) + (c + d)).  This is a READING of scikit-image's
 *               pyramid_gaussian(img, n - 1, multichannel=True) on float32 (scipy.ndimage.gaussian_filter, then an order-1 resize
 *               without anti-aliasing at a factor of exactly 2); scikit-image was not available where this was written: NOT PINNED.
 *     store     every level minus 127.5 (MSResNet's mean shift).
 * dib_deblur_shuffle_concat: in_dev [h][w][12] (conv_end's convolution WITHOUT bias), out_dev [2h][2w][6]:
 *     out[2y + i][2x + j][3 + c] = in[y][x][4c + 2i + j] + bias[4c + 2i + j]          (bias + PixelShuffle(2) + cat, bit for bit)
 * dib_deblur_finish: in_dev [Hp][Wp][3] (the finest level's last convolution WITHOUT bias) -> out_dev planar fp32 [3][H][W]:
 *     out[c][y][x] = clamp(((in[y][x][c] + bias[c]) + 127.5) + 0.5, 0, 255) * (1.f / 255.f)    every step rounded in fp32, a NaN stays
 *     a NaN: bit for bit torch's `(conv + 127.5)[:H, :W].add_(0.5).clamp_(0, 255) / 255` ON A GPU, where the reference runs it (ATen
 *     divides a CUDA tensor by a scalar as a multiplication by the fp32 reciprocal; its CPU kernel divides: at most 1 ulp apart).
 * Padded images of more than 2^30 pixels, n outside 1..4, H or W < 1, null or misaligned pointers (levels, in_dev and out_dev of
 * shuffle_concat: 16 bytes): DIB_EINVAL, nothing launched.  No allocation, no host synchronisation: capturable into a graph.
 * ------------------------------------------------------------------------------------- */
int dib_deblur_pyramid(const void *in_dev, int dtype, int H, int W, int n_scales, float *const *levels_dev, void *stream);
int dib_deblur_shuffle_concat(const float *in_dev, const float *bias_dev, float *out_dev, int h, int w, void *stream);
int dib_deblur_finish(const float *in_dev, const float *bias_dev, float *out_dev, int H, int W, int Hp, int Wp, void *stream);

/* The same three steps for DeepDeblur's `--precision half` (reference models/deblur/deblurInterface.py:37,40,52-53: the model and the
 * pyramid are cast to Half, so every op of the network runs and rounds in Half; `evaluate.py --deblur_precision half`).  Levels,
 * convolution outputs and the image are IEEE Half (raw 16-bit words), biases fp32 vectors holding Half values; "half()" rounds to
 * nearest even; the convolutions are MIOpen's on Half tensors, each followed by dib_bias_act_f16_nhwc.  The same kernels as above,
 * templated over the stored type: same argument checks (DIB_EINVAL, nothing launched), same limits, capturable.
 *
 * dib_deblur_pyramid_f16: in_dev as above (Half or fp32 image) -> levels_dev[s], channels-last Half [Hp >> s][Wp >> s][6] (coarsest:
 *   [..][3]), 16-byte aligned, channels 0..2 written.  Quantise, pad and every level L_s are computed exactly as dib_deblur_pyramid
 *   computes them, in fp32 (the reference builds the pyramid on the host before it casts); stored is half(half(L_s) - 127.5): the
 *   upload's cast, then MSResNet's Half `x - 127.5`.  Level 0 holds integers and is exact.  A coarser level is filtered from the fp32
 *   values of the one above, not from its rounded ones: work_dev (16-byte aligned) receives fp32 [Hp >> s][Wp >> s][3] for
 *   s = 1 .. n - 2, back to back -- 0 bytes for n <= 2 (work_dev may be NULL), 3 Hp Wp bytes for n = 3, 3.75 Hp Wp for n = 4.
 * dib_deblur_shuffle_concat_f16: in_dev Half [h][w][12], out_dev Half [2h][2w][6], both 16-byte aligned:
 *     out[2y + i][2x + j][3 + c] = half(in[y][x][4c + 2i + j] + bias[4c + 2i + j])    bit for bit torch's Half bias add + PixelShuffle + cat
 * dib_deblur_finish_f16: in_dev Half [Hp][Wp][3] -> out_dev planar Half [3][H][W] (2-byte aligned; 8-byte vectors where they are):
 *     out[c][y][x] = half(clamp(half(half(half(in + bias) + 127.5) + 0.5), 0, 255) * (1.f / 255.f))
 *     every op of `(conv + 127.5)[:H, :W].add_(0.5).clamp_(0, 255) / 255` rounded to Half; the last product is formed in fp32 and
 *     rounded once, as ATen does for a Half tensor on a GPU.  A NaN stays a NaN.  No clamp anywhere else: a Half activation beyond
 *     65504 is inf and travels on as torch's would. */
int dib_deblur_pyramid_f16(const void *in_dev, int dtype, int H, int W, int n_scales, void *const *levels_dev, float *work_dev, void *stream);
int dib_deblur_shuffle_concat_f16(const void *in_dev, const float *bias_dev, void *out_dev, int h, int w, void *stream);
int dib_deblur_finish_f16(const void *in_dev, const float *bias_dev, void *out_dev, int H, int W, int Hp, int Wp, void *stream);

/* ---------------------------------------------------------------------------------------
 * Non-blind deconvolution with the blur's own forward model (this library's addition; `evaluate.py --deconvolve_first`): Richardson-
 * Lucy on one C x H x W planar image y_dev of `dtype` (the blurred, possibly corrupted image) with the tap table the blur read
 * (dib_psf_compact with normalize = 1; psf_dtype = the dtype of the PSF it was compacted from: fp16 or fp32 weight bits; either LDS
 * window geometry).  With o = K / 2 - 1 and the taps {(r_t, c_t, w_t)} of the table, not re-normalised:
 *     (A  x)[i, j] = sum_t w_t x[m (i - (r_t - o)), m (j - (c_t - o))]     dib_sparse_blur's operator: m is its padding rule (reflect /
 *                                                                          zero / replicate by K, H, W) with the wrap row and column
 *     (A* u)[i, j] = sum_t w_t u[m'(i + (r_t - o)), m'(j + (c_t - o))]     offsets negated; m' = the same rule without the wrap
 *     x_0 = y;   q = y / max(A x_k, eps);   x_{k+1} = clamp(x_k * (A* q), 0, 1);   out_dev = x_iterations, fp32 C x H x W
 * All arithmetic fp32 (y read as fp32), every sweep accumulates from 0 with fused multiply-adds, taps in table order.  A pixel with
 * y == 0 and A x == 0 gives q = 0: finite input never produces NaN or Inf.  Two launches per iteration on `stream` (sweep A with the
 * ratio as its epilogue, sweep A* with multiply and clamp); work_dev: 2 C H W floats (q and the spare plane x_k alternates through
 * with out_dev, so that the result ends in out_dev for odd and even counts).  No allocation, no host synchronisation, no atomics:
 * deterministic and capturable.  y_dev, out_dev and work_dev must not overlap.
 * DIB_EINVAL (nothing launched): null pointer, unknown dtype, K not 128 / 256, C, H or W < 1, iterations outside 1..1000, eps <= 0,
 * overlapping buffers.  DIB_ESHAPE: where dib_sparse_blur refuses the image (K = 128 and H or W == 64 with neither below 64), or
 * C H W >= 2^31 - 1.
 * ------------------------------------------------------------------------------------- */
int dib_rl_deconvolve(const void *y_dev, int dtype, float *out_dev, float *work_dev, int C, int H, int W, const void *table_dev,
                      int psf_dtype, int K, int iterations, float eps, void *stream);

/* ---------------------------------------------------------------------------------------
 * Total-variation regularised Richardson-Lucy (Dey et al. 2006, "RL-TV"; this library's addition; `evaluate.py --deconvolve_tv`): one
 * multiplicative factor per pixel and iteration in front of the plain update, which keeps the iteration from amplifying what A does
 * not explain (noise, block and JPEG residue).  Per plane x of H x W, planes independent, with beta > 0 and 0 < lambda <= 0.1:
 *     dx[i, j] = x[i, j + 1] - x[i, j]   (0 where j == W - 1)         dy[i, j] = x[i + 1, j] - x[i, j]   (0 where i == H - 1)
 *     n[i, j]  = sqrt(dx^2 + dy^2 + beta^2)                            p = dx / n,   r = dy / n
 *     div[i, j] = (p[i, j] - p[i, j - 1]) + (r[i, j] - r[i - 1, j])    with p[i, -1] = 0 and r[-1, j] = 0
 *     g = 1 / (1 - lambda * div)                                       tv_weight(x) = x * g
 *     q = y / max(A x_k, eps);   x_{k+1} = clamp((x_k * g_k) * (A* q), 0, 1);   x_0 = y
 * |p|, |r| < 1, so |div| < 4 and the denominator lies in (0.6, 1.4): g is finite and positive for finite input.  A flat neighbourhood
 * gives div = 0 and g = 1 exactly: black stays black, a constant stays constant, a 1 x 1 plane is returned unchanged.  The stencil is
 * seven points of x_k -- the centre, its four neighbours, (i + 1, j - 1) and (i - 1, j + 1) -- and never leaves the plane.  All fp32,
 * every sum, difference and product rounded on its own in the order written (the sum under the root as (dx dx + dy dy) + beta beta),
 * x_0 = y read as fp32; 1 / n and g are computed to 1 ulp each (the hardware's reciprocal square root and reciprocal, exact at 1),
 * p = dx (1 / n), r = dy (1 / n): the result agrees with an IEEE evaluation to rounding, not bit for bit.  A, A*, eps and the
 * boundary rules of the two sweeps are dib_rl_deconvolve's.  (x_k * g_k) is rounded first and then multiplied by A* q: sweep A*
 * runs as it is, with x_k * g_k as the plane its epilogue multiplies.
 *
 * dib_tv_weight: out_dev (fp32 C x H x W) = tv_weight of x_dev (`dtype`, C x H x W), one launch on `stream`, every pixel loaded and
 * stored once.  DIB_EINVAL (nothing launched): null pointer, unknown dtype, C, H or W < 1, tv_lambda outside (0, 0.1], tv_beta not
 * positive or not finite, overlapping buffers.  DIB_ESHAPE: C H W >= 2^31 - 1.
 * dib_rl_deconvolve_tv: dib_rl_deconvolve with the factor.  work_dev: 3 C H W floats (q, the spare plane, x_k * g_k); three launches
 * per iteration (the factor, sweep A, sweep A*); the result ends in out_dev for odd and even counts.  No allocation, no host
 * synchronisation, no atomics: deterministic and capturable.  Refusals: dib_rl_deconvolve's, and DIB_EINVAL for tv_lambda and tv_beta
 * as above.  dib_rl_deconvolve itself is unchanged: its launches, its 2-plane workspace, its bits.
 * ------------------------------------------------------------------------------------- */
int dib_tv_weight(const void *x_dev, int dtype, float *out_dev, int C, int H, int W, float tv_lambda, float tv_beta, void *stream);
int dib_rl_deconvolve_tv(const void *y_dev, int dtype, float *out_dev, float *work_dev, int C, int H, int W, const void *table_dev,
                         int psf_dtype, int K, int iterations, float eps, float tv_lambda, float tv_beta, void *stream);

/* ---------------------------------------------------------------------------------------
 * Restoration quality (this library's addition; quality.py, `train_deblurrer.py --validate_images`): how close image a is to image b.
 * a_dev, b_dev: planar C x H x W, contiguous, each DIB_F16 or DIB_F32 (any pairing), aligned to their element type only; L = data_range.
 * A stated reading (DeepDeblur reports PSNR and SSIM; its loss/ package is not in the reference tree): Wang et al. 2004 as
 * skimage.metrics.structural_similarity(gaussian_weights=True, sigma=1.5, use_sample_covariance=False, data_range=L, channel_axis=0).
 *     mse     = mean over all C H W of (a - b)^2
 *     psnr_db = 10 log10(L^2 / mse), +inf when mse == 0
 *     g       : 11 taps, g_k ~ exp(-(k - 5)^2 / (2 1.5^2)), normalised to sum 1, separable
 *     mu_a, mu_b, E[a a], E[b b], E[a b]: the VALID 11 x 11 correlation with g (x) g: no padding, (H - 10) x (W - 10) windows per channel
 *     var_a = E[a a] - mu_a^2,  var_b = E[b b] - mu_b^2,  cov = E[a b] - mu_a mu_b;  C1 = (0.01 L)^2,  C2 = (0.03 L)^2
 *     S       = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)(var_a + var_b + C2))
 *     ssim    = mean of S over all windows and channels
 * out_dev[3] = {mse, psnr_db, ssim}, fp32.
 * Arithmetic.  Pixels are read as fp32 and shifted by a pivot before the moments; variances and covariance do not depend on a shift
 * that all pixels of a window share, and the pivot is added back to the means.  WHICH pivot is implementation-defined and not part of
 * the contract: any per-window-constant shift meets the definition, and results of two implementations agree to rounding, not bit for
 * bit.  (This one takes the fp32 mean of the pixel tile a workgroup stages, per image: on a flat region that brings the cancellation
 * error of E[x x] - mu^2 from the order of ulp(L^2 / 4), what a fixed shift by L / 2 leaves, down to the order of ulp(var).)  Moments
 * (fused multiply-adds, rows left to right, then columns top to bottom) and S in fp32.  The eleven fp32 weights are multiples of 2^-24
 * that sum to exactly 1 (each within 2.2e-8 of the exact value).  (a - b)^2 is formed from the values as read; a lane adds a handful
 * of them, and of S, in fp32, everything beyond that is added in fp64: per-workgroup sums go to work_dev, a second small launch adds
 * those in a fixed order and writes out_dev.  No atomics, no allocation, no host synchronisation: the same bits from run to run of
 * one build, capturable.  A NaN pixel gives a NaN mse, psnr_db and ssim; nothing traps.  a == b in value gives exactly {0, +inf, 1}.
 * work_dev: dib_image_quality_workspace_bytes(C, H, W) bytes (0 for a shape the entry refuses), 8-byte aligned; nothing beyond is written.
 * DIB_EINVAL (nothing launched): null pointer, unknown dtype, C, H or W < 1, L <= 0 or not finite, a misaligned pointer (out_dev: 4
 * bytes), out_dev or work_dev overlapping an input or each other (a_dev and b_dev may overlap: they are only read).
 * DIB_ESHAPE: H < 11 or W < 11, or C H W >= 2^31 - 1.
 * ------------------------------------------------------------------------------------- */
size_t dib_image_quality_workspace_bytes(int C, int H, int W);
int dib_image_quality(const void *a_dev, int a_dtype, const void *b_dev, int b_dtype, int C, int H, int W, float data_range,
                      float *out_dev /* [3]: mse, psnr_db, ssim */, void *work_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * Restoration quality of K = 1 or 2 candidates against ONE sharp image, in one pass, folded into a per-cell accumulator on the device
 * (this library's addition; quality.py: restoration_quality, RestorationMeter; `evaluate.py --restoration_metrics`: the blurred image
 * and what --deblur_first / --deconvolve_first make of it, against the image before the blur).
 * ref_dev and cand_dev[k] (cand_dev, cand_dtype: HOST arrays of K entries): planar C x H x W, contiguous, each DIB_F16 or DIB_F32 in
 * any mix, aligned to their element type only.  The definition is dib_image_quality's (window, valid windows, population moments,
 * C1, C2), and with quantize8 == 0
 *     out_dev[3 k .. 3 k + 2] == what dib_image_quality(cand_dev[k], ref_dev, ..., data_range) writes, BIT FOR BIT:
 * both entries run the same device code per pair; this one reads the sharp image once and launches twice whatever K is.
 * quantize8 != 0: every image is replaced as it is read by its 8-bit grey levels rintf(clamp(255 x, 0, 255)) in fp32 (ties to even,
 * a NaN stays a NaN) and the metric runs on those with L = 255; data_range must then be 1.  Bit for bit dib_image_quality of images
 * quantised that way beforehand, with data_range 255.  (A pixel k / 255 held in Half comes back as exactly k.)
 * acc_dev (may be NULL): DIB_RQ_ACC_DOUBLES doubles per candidate, updated in place by one lane of the second launch:
 *     {n, n_identical, n_nonfinite, sum_mse, sum_psnr_db, sum_ssim}
 * from the figures AS WRITTEN to out_dev (fp32, widened): mse or ssim not finite -> n_nonfinite += 1 and nothing else;  mse == 0 ->
 * n, n_identical += 1, sum_ssim += ssim (its +inf dB stays out of sum_psnr_db: the mean PSNR is over n - n_identical images);
 * otherwise n += 1 and the three sums grow.  That is exactly what a host loop over the per-image out_dev rows would add, in order.
 * Calls on one stream are ordered; there are no atomics, no allocation, no host synchronisation: capturable, the same bytes from run
 * to run.  work_dev: dib_restoration_quality_workspace_bytes(K, C, H, W) bytes (0 for arguments the entry refuses), 8-byte aligned;
 * nothing beyond is written.
 * DIB_EINVAL (nothing launched): K outside 1..2, null pointer (acc_dev excepted), unknown dtype, C, H or W < 1, data_range <= 0 or not
 * finite, quantize8 with data_range != 1, a misaligned pointer (out_dev: 4 bytes, acc_dev and work_dev: 8), out_dev, acc_dev or
 * work_dev overlapping an input or each other (the inputs may overlap or be one another: they are only read).
 * DIB_ESHAPE: H < 11 or W < 11, or C H W >= 2^31 - 1.
 * ------------------------------------------------------------------------------------- */
#define DIB_RQ_ACC_DOUBLES 6
size_t dib_restoration_quality_workspace_bytes(int K, int C, int H, int W);
int dib_restoration_quality(const void *ref_dev, int ref_dtype, const void *const *cand_dev, const int *cand_dtype, int K, int C, int H,
                            int W, int quantize8, float data_range, float *out_dev /* [3 K]: mse, psnr_db, ssim per candidate */,
                            double *acc_dev, void *work_dev, void *stream);

/* ---------------------------------------------------------------------------------------
 * Training DeepDeblur's network (`python -m detectinblur_amd.train_deblurrer`, models/deblur_train.py; the reference vendors the
 * trainer as models/deblur/train.py, dataCommon.py): what runs around MIOpen's convolutions and is not above already.  HBM-bound
 * streams on `stream`; no allocation, no atomics, no host synchronisation: capturable, and bitwise reproducible from call to call.
 *
 * PATCHES.  in_dev: HOST array of B device pointers to planar [3][H[b]][W[b]] images of `dtype` (Half or fp32; sizes may differ);
 * out_dev: planar [B][3][ps][ps] of the same dtype.  Per image a crop origin (py, px) and a flags word:
 *     DIB_PATCH_HFLIP | DIB_PATCH_VFLIP | DIB_PATCH_ROT90 | order[0] << 4 | order[1] << 6 | order[2] << 8      (order[c] in 0..2)
 * in the order of the reference's dataCommon.py (crop :32-39, augment :76-81): the crop, then reverse x, then reverse y, then the
 * transpose, then out channel c = channel order[c].  Values are moved, never converted: bit-exact.  One launch; B <= 64.
 * DIB_EINVAL: null / misaligned pointer, unknown dtype, B outside 0..64, ps < 1, unknown flag bits or a channel index of 3.
 * DIB_ESHAPE: a patch that leaves its image.
 * ------------------------------------------------------------------------------------- */
#define DIB_PATCH_HFLIP 1u
#define DIB_PATCH_VFLIP 2u
#define DIB_PATCH_ROT90 4u
int dib_deblur_patches(const void *const *in_dev, int dtype, const int *H, const int *W, const int *py, const int *px,
                       const unsigned int *flags, int B, int ps, void *out_dev, void *stream);

/* PATCHES WITH THE VALUE AUGMENTATION (dataCommon.py: augment's change_saturation :72-87, add_noise :43-54; csrc/dib_deblur_augment.hip).
 * The arguments of dib_deblur_patches and the same data movement, plus per image a saturation factor, a noise sigma in grey levels and
 * the two key words of its noise field (keys: HOST array [B][2]); out_dev: planar fp32 [B][3][ps][ps] whatever `dtype` is.  Per pixel, in
 * fp32 on the 0..255 scale, every operation rounded on its own:
 *     q_c = the image's 8-bit level (dib_deblur_pyramid's quantisation: trunc(v * 255) clamped to 0..255, NaN -> 0; a Half product is
 *           rounded to Half first)
 *     x_c = clamp(m - saturation * (m - q_c), 0, 255),  m = max(q_0, q_1, q_2)       scaling S in HSV and converting back, without the hue
 *     x_c = clamp(x_c + sigma * n_i, 0, 255)  when sigma != 0                        n_i: the generator of dib_post_ops on element index
 *                                                                                    i = (c * ps + y) * ps + x of the image's output patch
 *     out = rint(x_c) / 255                                                          a grey level: dib_deblur_pyramid reads it back exactly
 * saturation == 1 and sigma == 0 give q_c / 255.  One launch; B <= 64.
 * DIB_EINVAL: as dib_deblur_patches; a saturation that is not finite or below 0; a sigma that is not finite; out_dev not 4-byte aligned.
 * DIB_ESHAPE: a patch that leaves its image.  Nothing is launched on either. */
int dib_deblur_patches_augment(const void *const *in_dev, int dtype, const int *H, const int *W, const int *py, const int *px,
                               const unsigned int *flags, const float *saturation, const float *sigma, const unsigned int *keys /* [B][2] */,
                               int B, int ps, float *out_dev, void *stream);

/* BIAS GRADIENT: the backward pass of dib_bias_act_nhwc / dib_bias_act_mask_nhwc in one pass over a channels-last fp32 gradient
 * [n_pix][C]:
 *     grad_out[p][c] = mask bit ? grad_in[p][c] : 0        the mask of dib_bias_act_mask_nhwc; bit-identical to dib_relu_mask_backward;
 *                                                          grad_out_dev may alias grad_in_dev
 *     bias_grad[c]   = sum over p of grad_out[p][c]        fp32
 * mask_dev NULL: no selection (any C >= 1), and grad_out_dev may be NULL too: the plain channel sum.  With a mask C % 4 == 0.
 * Tensors 16-byte aligned when C % 4 == 0, else 4-byte.  work_dev: dib_bias_grad_workspace_bytes(n_pix, C) bytes.
 * Two launches: per-slice partial sums into work_dev, then their sum in slice order; the order of every addition depends on
 * (n_pix, C) alone (csrc/dib_sliced_sum.h states it, with the depth of the tree for error bounds).  A NaN or inf gradient
 * reaches the sum of its own channel only.  DIB_EINVAL: n_pix or C < 1, n_pix * C > 2^40, null / misaligned pointer, a mask with
 * C % 4 != 0 or without grad_out_dev. */
size_t dib_bias_grad_workspace_bytes(long long n_pix, int C);
int dib_bias_grad_nhwc(const float *grad_in_dev, const unsigned char *mask_dev, float *grad_out_dev, long long n_pix, int C,
                       float *bias_grad_dev, void *work_dev, void *stream);

/* The same over a channels-last IEEE Half gradient [n_pix][C] (raw 16-bit words): the backward pass of dib_bias_act_f16_nhwc /
 * dib_bias_act_mask_f16_nhwc under `train_deblurrer.py --amp`.
 *     grad_out[p][c] = mask bit ? grad_in[p][c] : +0       the mask of dib_bias_act_mask_f16_nhwc (one byte per 8 elements); the 16
 *                                                          bits are moved, never converted; grad_out_dev may alias grad_in_dev
 *     bias_grad[c]   = sum over p of float(grad_out[p][c]) fp32: every Half is exact in fp32, only the additions round
 * The same kernels, templated over the stored type: the same summation order with 8 channels per lane (one 16-byte load) when
 * C % 8 == 0 and grad_in_dev / grad_out_dev are 16-byte aligned, else one channel per lane (2-byte aligned).  With a mask C % 8 == 0
 * and 16-byte alignment.  bias_grad_dev and work_dev: fp32, 4-byte aligned; dib_bias_grad_f16_workspace_bytes(n_pix, C) bytes (the
 * size of the one-channel-per-lane form, whose slices are the shorter ones: enough for either).  Argument errors as above. */
size_t dib_bias_grad_f16_workspace_bytes(long long n_pix, int C);
int dib_bias_grad_f16_nhwc(const void *grad_in_dev, const unsigned char *mask_dev, void *grad_out_dev, long long n_pix, int C,
                           float *bias_grad_dev, void *work_dev, void *stream);

/* L1 LOSS of one pyramid level (DeepDeblur's loss, sum over levels of mean |output - target|; its loss/ package is not in the
 * reference tree: a stated reading).  out_dev: the level's output, channels-last fp32 [n_pix][3]; target_dev: [n_pix][target_stride]
 * fp32 whose channels 0..2 are read (the layout dib_deblur_pyramid writes: stride 6, coarsest level 3).  With d = out - target:
 *     grad_dev[p][c] = sign(d) * k,  k = gscale / float(3 n_pix) (one fp32 division)      sign(+-0) = 0; a NaN d gives a NaN (torch.sign gives 0)
 *     *loss_dev     += (sum of |d|) / float(3 n_pix)                                     summed in csrc/dib_sliced_sum.h's order
 * The caller zeroes *loss_dev before the first level.  work_dev: dib_l1_pyramid_loss_workspace_bytes(n_pix) bytes.  Two launches.
 * DIB_EINVAL: n_pix < 1 or > 2^38, target_stride < 3, null / misaligned (4 bytes) pointer. */
size_t dib_l1_pyramid_loss_workspace_bytes(long long n_pix);
int dib_l1_pyramid_loss(const float *out_dev, const float *target_dev, int target_stride, long long n_pix, float gscale,
                        float *grad_dev, float *loss_dev, void *work_dev, void *stream);

/* ADVERSARIAL LOSS of the DeepDeblur trainer (`train_deblurrer.py --loss 1*L1+1*ADV`, models/deblur_adversarial.py;
 * csrc/dib_deblur_adv.hip).
 *
 * LeakyReLU in place on a convolution output of n_elems fp32 (dib_leaky_relu_mask) or IEEE Half (dib_leaky_relu_mask_f16, raw 16-bit
 * words; upcast, multiplied in fp32, rounded once) elements:
 *     x[i] = x[i] > 0 ? x[i] : x[i] * slope            NaN stays NaN; -0 stays -0 in fp32 and becomes +0 in the Half form, which
 *                                                        is what torch's Half kernel gives on gfx950 (csrc/dib_deblur_adv.hip, `leak`)
 *     mask[i / lane] bit (i % lane) = stored x[i] > 0    lane = 4 (fp32) / 8 (Half): dib_bias_act_mask_nhwc's layout; mask_dev may be NULL
 * and its backward from that mask (out_dev may alias grad_dev):
 *     out[i] = bit ? grad[i] : grad[i] * slope           Half: rounded once, and a -0 product becomes +0 as above
 * One launch each.  DIB_EINVAL, before any launch: slope not finite or <= 0 (only for slope > 0 is the mask of the result the mask
 * of the input); n_elems negative or no multiple of the lane; a null pointer (the forward's mask apart); x_dev / grad_dev / out_dev
 * not 16-byte aligned.  n_elems == 0: DIB_OK, nothing is launched. */
int dib_leaky_relu_mask(float *x_dev, long long n_elems, float slope, unsigned char *mask_dev, void *stream);
int dib_leaky_relu_mask_f16(void *x_dev, long long n_elems, float slope, unsigned char *mask_dev, void *stream);
int dib_leaky_relu_mask_backward(const float *grad_dev, const unsigned char *mask_dev, float slope, float *out_dev, long long n_elems,
                                 void *stream);
int dib_leaky_relu_mask_backward_f16(const void *grad_dev, const unsigned char *mask_dev, float slope, void *out_dev, long long n_elems,
                                     void *stream);

/* Binary cross-entropy with logits of n fp32 logits against a CONSTANT label (real_label 1: "real", 0: "fake"), mean over n.  With
 * z = -x for label 1 and z = x for label 0, e = exp(-|z|):
 *     *loss_dev  += (sum of max(z, 0) + log1p(e)) / float(n)                   ADDED: the caller zeroes it before the first call
 *     grad_dev[i] = (label 1: -1, label 0: +1) * (gscale / float(n)) * sigma(z)  sigma(z) = z >= 0 ? 1 / (1 + e) : e / (1 + e)
 * A NaN logit gives a NaN at its own gradient element and a NaN loss, nothing else.  +-inf follows the formulas (z = +inf: term inf,
 * sigma 1; z = -inf: term 0, sigma 0), where torch's binary_cross_entropy_with_logits gives NaN.  Two launches; the sum is taken in
 * dib_l1_pyramid_loss's order, fixed by n alone (csrc/dib_sliced_sum.h states it with its depth: the same kernels).  work_dev:
 * dib_adv_bce_loss_workspace_bytes(n) bytes.  DIB_EINVAL: n < 1 or > 2^40, real_label not 0 or 1, null / misaligned (4 bytes) pointer. */
size_t dib_adv_bce_loss_workspace_bytes(long long n);
int dib_adv_bce_loss(const float *logits_dev, long long n, int real_label, float gscale, float *grad_dev, float *loss_dev, void *work_dev,
                     void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DIB_H_ */
