/*
 * ct_hip.h -- C ABI of libct_hip.so: MI355X (gfx950) kernels for the per-frame
 * colour-transfer hot path of egorchistov/color-transfer.
 *
 * The reference is pure Python (numpy / scipy / scikit-image / torch) and has no
 * native layer; each entry point below replaces the numpy expression(s) cited next
 * to it (paths relative to the reference root).  A binding only needs ctypes (see
 * INTEGRATION.md).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller, except where the name
 *     says host; nothing is allocated, freed or synchronised inside (one exception:
 *     none -- the workspace comes from the caller, sized by ct_workspace_bytes());
 *   - every entry takes the hipStream_t to launch on (as void*; NULL = default stream)
 *     and returns immediately after enqueueing (asynchronous, graph-capturable);
 *   - images are interleaved HWC, C = 3, contiguous: pixel p of image b starts at
 *     base + (b * n_pixels + p) * 3 elements;
 *   - return value: 0 = CT_OK, negative = CT_E_* argument error, positive = hipError_t;
 *   - arithmetic is float64 internally (see ct_set_lab_mode for the table-driven float32-image path); "_f32"/"_f64" name the I/O element type.
 */
#ifndef CT_HIP_H
#define CT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CT_OK 0
#define CT_E_BADARG (-1)     /* null pointer, negative size, unknown enum */
#define CT_E_WORKSPACE (-2)  /* workspace too small / misaligned */
#define CT_E_ALIGN (-3)      /* image base not aligned to its element size */

/* bumped whenever an entry point changes its argument list (2: ct_attention_tokens_f32 gained kv_shift; 3: round 3; 4: ct_conv2d_split_rows_f32, res_pre_act, ct_linear_ws16_f32, layernorm partials, f16 form of ct_conv2d_split*;
 * 5: ct_reinhard_persist_*, ct_reinhard_psnr_u8, CT_WS_REINHARD_PERSIST; 6: ct_conv2d_split_f32 gained scratch / scratch_bytes;
 * 7: ct_device_status);
 * the ctypes binding refuses a library whose ct_abi_version() differs */
#define CT_ABI_VERSION 9

/* doubles per image in a stats record written by ct_lab_stats / ct_rgb_meancov */
#define CT_LAB_STATS_STRIDE 8  /* mean[3], std[3] (population, ddof 0), n, 0           */
#define CT_RGB_STATS_STRIDE 16 /* mean[3], cov[9] row-major (ddof 1), n, 0, 0, 0       */

enum ct_workspace_kind {
    CT_WS_LAB_STATS = 0, /* ct_lab_stats_*: n_images = number of images in the call    */
    CT_WS_RGB_MEANCOV = 1,
    CT_WS_REINHARD = 2,  /* ct_reinhard_*:  n_images = batch (pairs)                    */
    CT_WS_IDT = 3,       /* ct_idt_*:       n_images = batch (pairs)                    */
    CT_WS_REINHARD_PSNR = 4, /* ct_reinhard_psnr_f32: n_images = batch (pairs)          */
    CT_WS_REINHARD_PERSIST = 5, /* ct_reinhard_persist_f32 / ct_reinhard_psnr_u8: n_images = batch (pairs); 0 = frame size not supported */
    CT_WS_MK_U8 = 6      /* ct_mk_u8:       n_images = batch (pairs)                    */
};

int ct_abi_version(void);

/* Sticky status of the CURRENT device, for callers that never synchronise per call (video loops, graphs): a bit mask, 0 = all well.
 *   bit 0: a bounded spin of a persistent Reinhard launch gave up (a workgroup of its grid never became resident: that call's
 *          frames and PSNR records are NaN);
 *   bit 1: a stream-K consumer of ct_conv2d_split_f32 gave up waiting for its producer (that launch's tile is wrong).
 * Neither can happen while the launch's workgroups are all resident; both are bounded so that a queue never hangs.  clear != 0
 * resets the bits read.  Blocks the calling thread for two 4-byte copies and does NOT wait for running work: synchronise the
 * streams of interest first.  Returns -1 when the device cannot be read.  New in ABI 7; the reference has no counterpart
 * (its CPU path cannot fail this way). */
int ct_device_status(int clear);

/* Lab arithmetic of the float32 entries (ct_lab_stats_f32, ct_reinhard_*_f32, ct_reinhard_lab_f32):
 *   CT_LAB_TABLE (default)  the power functions of skimage's rgb2lab / lab2rgb (methods/linear.py:25,26,40) are LDS
 *                           look-ups + short polynomials; Lab agrees with the float64 path to ~5e-7, statistics to ~1e-7;
 *                           values outside [0,1], NaNs and degenerate statistics fall back to the exact code per wave;
 *   CT_LAB_EXACT            float64 arithmetic with hardware seeds and one Newton correction (~1e-11 relative).
 * float64 images always take the exact path.  ct_set_lab_mode: the process-wide default (atomic; env CT_HIP_LAB=exact presets
 * it).  ct_set_lab_mode_thread: an override for the CALLING thread only (-1 = back to the default) -- host threads that drive
 * different streams with different arithmetic each set their own; every entry reads the mode once, on the calling thread.
 * ct_get_lab_mode: what the calling thread's next call will use.                                                          */
#define CT_LAB_TABLE 0
#define CT_LAB_EXACT 1
int ct_set_lab_mode(int mode);
int ct_set_lab_mode_thread(int mode);
int ct_get_lab_mode(void);
/* The two table sweeps of ct_reinhard_f32 / ct_reinhard_psnr_f32 over CHUNKS of pairs (entries added under ABI 9, no argument list
 * changed): chunk k runs statistics(k) -> apply(k) on the caller's stream (even k) or on a library-owned non-blocking stream (odd k;
 * one per device and per calling thread, created on first use outside a stream capture and kept), which is forked from the
 * caller's stream with an event and joined back into it with an event; each launch is sized for half the chip, so the kernels
 * of the two lanes are resident side by side and one lane's ramp and drain run under the other's streaming.  The PSNR finish
 * runs once on the caller's stream.  Capturable in a graph once the stream exists (a first call inside a capture stays unpipelined).
 *   chunk_pairs  -1 the built-in plan (measured, DESIGN.md 4.1: chunks of about four pairs for calls of >= 8 pairs of >= 2 Mpixel,
 *                the whole-batch launches below), 0 off, > 0 that many pairs per chunk at any frame size and batch (tests, tuning);
 *   t_policy     how the statistics sweep of a chunk reads its TARGET tiles, which the chunk's apply sweep re-reads:
 *                CT_PIPE_T_NT non-temporal like every other access, CT_PIPE_T_PLAIN default cache policy; -1 = the built-in choice.
 * Whatever the setting, the two whole-batch launches are kept for CT_LAB_EXACT, float64 frames, an `out` that overlaps an input
 * other than out == target exactly, and while ct_profile_events is armed.  Results: bitwise reproducible run to run for a given
 * setting; against the whole-batch launches only the grouping of the statistics' partial sums differs (as it already does
 * between batch sizes).  ct_set_reinhard_pipeline: process-wide default (atomic); ct_set_reinhard_pipeline_thread: an override
 * for the CALLING thread (chunk_pairs -2 removes it); ct_get_reinhard_pipeline: the setting the calling thread's next call reads;
 * ct_reinhard_pipeline_chunk: the pairs per chunk that setting gives frames of n_pixels in a call of `batch` pairs (0 = whole batch). */
#define CT_PIPE_T_NT 0
#define CT_PIPE_T_PLAIN 1
int ct_set_reinhard_pipeline(int chunk_pairs, int t_policy);
int ct_set_reinhard_pipeline_thread(int chunk_pairs, int t_policy);
int ct_get_reinhard_pipeline(int *chunk_pairs, int *t_policy);
int ct_reinhard_pipeline_chunk(int64_t n_pixels, int batch);
/* Measurement hook: four hipEvent_t (or NULL = off) that the library records on the launch stream immediately before /
 * after moments_kernel<T,true> and reinhard_apply_kernel of the following ct_lab_stats / ct_reinhard* calls, so that a
 * caller can time exactly those kernels with hipEventElapsedTime (bench.py `roofline`).  When a call takes the persistent
 * launch, the first pair is recorded back to back and the second pair brackets reinhard_persist_kernel.  Per calling thread. */
void ct_profile_events(void *moments_start, void *moments_stop, void *apply_start, void *apply_stop);
/* Human readable text for a return code of this library (never NULL). */
const char *ct_error_string(int code);
/* Bytes of device workspace an entry of `kind` needs for `n_images` images of `n_pixels`. */
size_t ct_workspace_bytes(int kind, int64_t n_pixels, int n_images);

/* ---- A1: rgb2lab + np.mean/np.std  (methods/linear.py:25-26,33-36; skimage rgb2lab) ----
 * For image i in [0, n_images): stats[i*8 ..] = {mean L,a,b ; std L,a,b (ddof 0) ; n ; 0}.
 * Deterministic: fixed-shape tree reduction, no float atomics.                          */
int ct_lab_stats_f32(const float *rgb, int64_t n_pixels, int n_images, double *stats,
                     void *ws, size_t ws_bytes, void *stream);
int ct_lab_stats_f64(const double *rgb, int64_t n_pixels, int n_images, double *stats,
                     void *ws, size_t ws_bytes, void *stream);

/* ---- A2: (lab - mu_t) * sigma_r / sigma_t + mu_r ; lab2rgb   (methods/linear.py:38-40) ----
 * stats_t / stats_r: records written by ct_lab_stats (device memory, no host sync).
 * out may alias target.  Output clipped to [0,1] like skimage's xyz2rgb.                */
int ct_reinhard_apply_f32(const float *target, const double *stats_t, const double *stats_r,
                          float *out, int64_t n_pixels, int batch, void *stream);
int ct_reinhard_apply_f64(const double *target, const double *stats_t, const double *stats_r,
                          double *out, int64_t n_pixels, int batch, void *stream);
/* Same affine map but the result is left in Lab (parity probe for the 1e-4 Lab gate).   */
int ct_reinhard_lab_f32(const float *target, const double *stats_t, const double *stats_r,
                        float *out_lab, int64_t n_pixels, int batch, void *stream);

/* ---- a1 fused: methods.linear.color_transfer_between_images (methods/linear.py:8-42) ----
 * batch pairs per call: stats of all 2*batch images in one launch, finalize, apply.
 * ws: ct_workspace_bytes(CT_WS_REINHARD, n_pixels, batch).
 * stats_out: NULL, or device [2*batch][8] doubles receiving the Lab stats records
 * (targets first, then references) -- the per-frame metrics a caller may gather.       */
int ct_reinhard_f32(const float *target, const float *reference, float *out,
                    int64_t n_pixels, int batch, double *stats_out, void *ws, size_t ws_bytes,
                    void *stream);
int ct_reinhard_f64(const double *target, const double *reference, double *out,
                    int64_t n_pixels, int batch, double *stats_out, void *ws, size_t ws_bytes,
                    void *stream);
/* The same + the per-frame PSNR of Runner.test_step (methods/__init__.py:30-32,37) against ground-truth frames gt
 * ([batch][n_pixels][3] like the images): psnr_out[i] = {mse, 10 log10(1 / mse)} of the (clipped) result of pair i.
 * With the table arithmetic the squared error is accumulated by the apply sweep while it writes the result -- the result is
 * not read back from HBM.  ws: ct_workspace_bytes(CT_WS_REINHARD_PSNR, n_pixels, batch).                               */
int ct_reinhard_psnr_f32(const float *target, const float *reference, const float *gt, float *out, double *psnr_out,
                         int64_t n_pixels, int batch, double *stats_out, void *ws, size_t ws_bytes, void *stream);

/* ---- a1 as ONE persistent launch (csrc/reinhard_persist.hip): methods/linear.py:8-42 for `batch` pairs.  One workgroup per CU
 * owns 1 / CUs of every frame; the cube-root-domain image of (up to 18 of) its target tiles waits in LDS for the statistics of
 * the whole frame, which travel between the workgroups as 64-bit integer atomics one pair ahead of their use (the rest of its
 * target tiles are fetched a second time); no launch boundary, no finishing kernels, one pass over the reference.
 * Frame sizes: 256 pixels .. 16 Mpixel (ct_reinhard_persist_supported).  Measured at 1080p, 16 pairs per call: float32 frames
 * 39 - 41 k pairs/s (the two sweeps of ct_reinhard_psnr_f32: 41.5 - 43.6 k -- this form is bound by vector instruction issue and
 * executes more instructions, so the fused float32 entries keep the two sweeps unless CT_HIP_REINHARD_PERSIST=1);
 * uint8 frames 46.6 - 49.4 k pairs/s, which no other entry serves.
 * out must NOT overlap target, reference or gt (CT_E_BADARG): a tile with a pixel near a kink of the inverse is redone with the
 * exact code from the input frame AFTER its fast-path result has been stored (the two-sweep entries above do allow out == target).
 * gt = NULL: no metric (psnr_out unused); else psnr_out[i] = {mse, PSNR} like ct_reinhard_psnr_f32.
 * ws: ct_workspace_bytes(CT_WS_REINHARD_PERSIST, n_pixels, batch).  After the call has completed, the first 32-bit word of
 * ws is 0, or 1 when a workgroup of the grid never became resident within 2 s (results are then NaN).
 * Bitwise reproducible run to run and independent of `batch`.                                                           */
int ct_reinhard_persist_supported(int64_t n_pixels);
/* 1 when ct_reinhard_f32 / ct_reinhard_psnr_f32 take the persistent launch for frames of this size in the current Lab mode */
int ct_reinhard_takes_persist(int64_t n_pixels);
int ct_reinhard_persist_f32(const float *target, const float *reference, const float *gt, float *out, double *psnr_out,
                            int64_t n_pixels, int batch, double *stats_out, void *ws, size_t ws_bytes, void *stream);
/* uint8 frames as the reference's datasets deliver them (utils/data.py:84,106,125: `read_image(...).float() / 255`): the
 * kernel reads the bytes (a quarter of the float32 traffic) and takes k / 255 (IEEE float32 division) and its gamma
 * expansion from 256-entry tables filled by the float32 kernel's own functions: per pixel the arithmetic is that of
 * ct_reinhard_persist_f32 on `u8.float() / 255`; the frame statistics agree to their last float32 rounding (the moment terms
 * are added in another lane order), results within 2e-7.  out: float32.                                               */
int ct_reinhard_psnr_u8(const uint8_t *target, const uint8_t *reference, const uint8_t *gt, float *out, double *psnr_out,
                        int64_t n_pixels, int batch, double *stats_out, void *ws, size_t ws_bytes, void *stream);

/* ---- A3: np.mean(axis=0) + np.cov(x.T)   (methods/linear.py:64-67,103-106) ----
 * stats[i*16 ..] = {mean[3] ; cov[9] row-major, ddof 1 ; n ; 0 0 0}.                     */
int ct_rgb_meancov_f32(const float *rgb, int64_t n_pixels, int n_images, double *stats,
                       void *ws, size_t ws_bytes, void *stream);
int ct_rgb_meancov_f64(const double *rgb, int64_t n_pixels, int n_images, double *stats,
                       void *ws, size_t ws_bytes, void *stream);

/* ---- A4 (sync-free): the 3x3 algebra of monge_kantorovitch_color_transfer on the device (methods/linear.py:108-118) ----
 * stats_t / stats_r: records of ct_rgb_meancov; decomposition 0 "MK", 1 "sqrt", 2 "cholesky"; writes the 16-double coef
 * records ct_affine3x3_* consumes (T is applied as x @ T).  float64 Jacobi eigen-decomposition: the SPD matrix square root
 * is unique, so it equals scipy.linalg.sqrtm to rounding.  (Xiao's SVD-based matrix depends on LAPACK's sign
 * convention and is computed on the host.)
 * Degenerate covariances (where the reference raises from LAPACK): an all-zero TARGET covariance (a constant frame) gives a
 * T that is NaN in all nine entries, for every decomposition (0 * inf in the inverse square root / the inverted factor), so
 * that pair's output is NaN; an all-zero REFERENCE covariance gives T == 0 exactly (every pixel maps to mu_r); a singular
 * but non-zero target covariance (a grey frame: rank 1) is NaN or huge, as the sign of a rounding-level eigenvalue falls.
 * No record influences another one.                                                                                   */
int ct_mk_coef_f64(const double *stats_t, const double *stats_r, int decomposition, int batch, double *coef,
                   void *stream);

/* ---- a3 fused: methods.linear.monge_kantorovitch_color_transfer (methods/linear.py:85-124), batch pairs per call,
 * everything on the device (moments of all 2*batch images in one sweep, finishing kernel, ct_mk_coef, affine apply).
 * ws: ct_workspace_bytes(CT_WS_REINHARD, n_pixels, batch).  Output unclipped like the reference.                      */
int ct_mk_f32_f32(const float *target, const float *reference, float *out, int64_t n_pixels, int batch,
                  int decomposition, void *ws, size_t ws_bytes, void *stream);
int ct_mk_f32_f64(const float *target, const float *reference, double *out, int64_t n_pixels, int batch,
                  int decomposition, void *ws, size_t ws_bytes, void *stream);
int ct_mk_f64_f64(const double *target, const double *reference, double *out, int64_t n_pixels, int batch,
                  int decomposition, void *ws, size_t ws_bytes, void *stream);

/* ---- A5: (x - mu_t) @ A + mu_r   (methods/linear.py:80,122) ----
 * coef: device, 16 doubles per image: A[9] row-major such that out_j = sum_i (x_i-mu_t_i)*A[i][j]
 * (pass T for MK, T.T for Xiao), mu_t[3], mu_r[3], pad.  No clipping (the reference does
 * not clip either; the caller clamps, methods/__init__.py:30).                           */
int ct_affine3x3_f32_f64(const float *in, const double *coef, double *out, int64_t n_pixels,
                         int batch, void *stream);
int ct_affine3x3_f64_f64(const double *in, const double *coef, double *out, int64_t n_pixels,
                         int batch, void *stream);
int ct_affine3x3_f32_f32(const float *in, const double *coef, float *out, int64_t n_pixels,
                         int batch, void *stream);

/* ---- A3 / A5 / a3 on uint8 frames (csrc/linear_u8.hip): the image is k / 255, the scale skimage.img_as_float and the datasets
 * hand over (utils/data.py:84; utils/postprocess.py:138 is img_as_ubyte(mkct(img_as_float(..), img_as_float(..)).clip(0, 1))).
 * Added under ABI 9.
 *
 * ct_rgb_meancov_u8: the record of ct_rgb_meancov_f32.  Per image the sums of k and of k_i k_j are unsigned 64-bit integers, so the
 * record does not depend on the order of summation: bitwise reproducible, independent of the batch, and the covariance of a
 * constant frame is exactly 0.  cov_ij = (N sum k_i k_j - sum k_i sum k_j) / (N (N - 1)) / 255^2: the numerator exact in 128-bit
 * integers, three roundings (its conversion to double, the two divisions); mean_i = sum k_i / (255 N), one rounding.
 * n_pixels <= 94 906 265 (N (N - 1) <= 2^53, an exact double), else CT_E_BADARG; n_pixels < 2 gives the NaN of np.cov, like the
 * _f32 entry; ws: ct_workspace_bytes(CT_WS_RGB_MEANCOV, n_pixels, n_images).                                               */
int ct_rgb_meancov_u8(const uint8_t *rgb, int64_t n_pixels, int n_images, double *stats, void *ws, size_t ws_bytes,
                      void *stream);
/* ct_affine3x3_u8_*: x = (double)k / 255.0, then the arithmetic of ct_affine3x3_f64_f64 on x (the same fma order), rounded once to
 * float32: bitwise (float)ct_affine3x3_f64_f64(k / 255.0).  The _u8 form then applies ct_pack_u8_f32's rule to that float32 value
 * (rint(clamp(x, 0, 1) * 255), ties to even, NaN gives 0).                                                                    */
int ct_affine3x3_u8_f32(const uint8_t *in, const double *coef, float *out, int64_t n_pixels, int batch, void *stream);
int ct_affine3x3_u8_u8(const uint8_t *in, const double *coef, uint8_t *out, int64_t n_pixels, int batch, void *stream);
/* ct_mk_u8: monge_kantorovitch_color_transfer (methods/linear.py:85-124) for `batch` pairs of uint8 frames in four stream-ordered
 * launches: the moments of all 2 * batch images, their finishing launch, ct_mk_coef_f64, the apply sweep.  Bitwise the composition
 * ct_rgb_meancov_u8 -> ct_mk_coef_f64 -> ct_affine3x3_u8_*.  out_f32 (unclipped) and out_u8 are each optional; both NULL:
 * CT_E_BADARG.  With gt (uint8 frames like the images) and psnr_out, also psnr_out[i] = {mse, 10 log10(1 / mse)} like
 * ct_reinhard_psnr_u8: the float32 result clamped to [0,1] against gt as float32 k / 255 (IEEE float32 division), differences
 * formed and summed in float64 in a fixed order by the apply sweep while it writes (a fifth, one-workgroup launch finishes them;
 * the result is not read back).  A NaN result (constant target) gives mse = NaN.  gt == NULL: no metric, psnr_out unused.
 * ws: ct_workspace_bytes(CT_WS_MK_U8, n_pixels, batch).                                                                     */
int ct_mk_u8(const uint8_t *target, const uint8_t *reference, const uint8_t *gt, float *out_f32, uint8_t *out_u8,
             double *psnr_out, int64_t n_pixels, int batch, int decomposition, void *ws, size_t ws_bytes, void *stream);

/* ---- regrain: the second half of methods.iterative.automated_color_grading (methods/iterative.py:62-138) ----------------
 * img_in (the original target), img_col (the IDT result), out: device [height][width][3] float64, one frame per call; out
 * must not alias the inputs.  Multigrid as in the reference: both images are halved with skimage.transform.resize
 * semantics (Gaussian anti-aliasing sigma (factor-1)/2 with 'mirror' boundary, then bilinear sampling with 'reflect'
 * boundary; scikit-image 0.18.3) while (h+1)/2 > 20 and (w+1)/2 > 20 and nbits has entries left; on every level nbits[level]
 * Jacobi sweeps of iterative.py:106-115.  nbits: HOST array, the reference's default is {4, 16, 32, 64, 64, 64}.  The batch-1
 * call of the code behind ct_regrain_u8.
 * ws: ct_regrain_workspace_bytes(height, width) (16-byte aligned).                                                     */
size_t ct_regrain_workspace_bytes(int height, int width);
int ct_regrain_f64(const double *img_in, const double *img_col, double *out, int height, int width, const int *nbits,
                   int n_nbits, void *ws, size_t ws_bytes, void *stream);

/* ct_regrain_u8: the same regrain for `batch` frames of one size in the launches of one frame (every kernel has a frame axis), with
 * the original target as bytes: img_in uint8 [batch][height][width][3], img_col float64 of that shape.  Byte k stands for
 * (double)((float)k / 255.0f) (input_f32 = 1) or k / 255.0 (input_f32 = 0), looked up in ct_idt_u8's 256-entry table by the
 * kernels that read level 0's img_in (weights, level-0 sweeps, first down-resize); everything after the lookup is ct_regrain_f64's
 * float64 statements, so the float64 result is bitwise ct_regrain_f64 on that image, frame by frame.
 * Outputs, any non-empty subset (NULL = not wanted), written by the last level-0 launch: out_f64; out_f32 = that value rounded
 * once; out_u8 = ct_pack_u8_f32's rule on the float32 value (rint(clamp(x, 0, 1) * 255), ties to even, NaN -> 0).  Without
 * out_f64 no float64 image is stored.  With gt (uint8, the target's shape) psnr_out[batch][2] = (mse, PSNR) of the float32 result
 * clamped to [0, 1] against (float)k / 255.0f, in float64, one partial per workgroup of that last launch added in a fixed order
 * by one more launch; nothing is read back.  nbits[0] == 0 still writes every output.
 * n_nbits outside 1..8, a negative nbits entry, all outputs NULL, gt without psnr_out: CT_E_BADARG; img_col / out_f64 / out_f32 /
 * psnr_out off their element size: CT_E_ALIGN; ws missing, not 16-byte aligned or smaller than
 * ct_regrain_u8_workspace_bytes(batch, height, width, n_nbits): CT_E_WORKSPACE -- all before anything touches the device.
 * Workspace per frame, in doubles: 6 H W (resize scratch) + 8 H W (level 0: two iterates, weights) + 14 h w per further level
 * + one per workgroup of the last launch.  ct_regrain_u8_workspace_bytes is 0 for refused arguments (batch outside 1..65535,
 * height * width >= 2^31).  Added under ABI 9.                                                                              */
size_t ct_regrain_u8_workspace_bytes(int batch, int height, int width, int n_nbits);
int ct_regrain_u8(const uint8_t *img_in, const double *img_col, int batch, int height, int width, int input_f32,
                  const int *nbits, int n_nbits, double *out_f64, float *out_f32, uint8_t *out_u8, const uint8_t *gt,
                  double *psnr_out, void *ws, size_t ws_bytes, void *stream);

/* ct_acg_u8: methods.iterative.automated_color_grading (methods/iterative.py:118-138) for `batch` pairs of uint8 frames: ct_idt_u8
 * on the bytes (target [batch][height][width][3], reference [batch][n_r][3], rot / rinv [batch][n_iter][9], round_dr_f32 =
 * input_f32) with its float64 result left in the workspace, then ct_regrain_u8 with the target bytes as img_in and that result as
 * img_col.  Outputs, gt / psnr_out and nbits as for ct_regrain_u8.  The float64 result is bitwise ct_regrain_f64(image of the
 * target bytes, ct_idt_u8's float64 output) frame by frame.
 * Errors before anything touches the device, by ct_idt_u8's rules: n_iter < 1, bins outside 1..1024, n_nbits outside 1..8, all
 * outputs NULL, gt without psnr_out: CT_E_BADARG; CT_E_ALIGN and CT_E_WORKSPACE as above, against
 * ct_acg_u8_workspace_bytes = ct_idt_u8_workspace_bytes(batch, n_iter, bins, H W, 0) + 24 H W batch + ct_regrain_u8_workspace_bytes,
 * each rounded up to 16 (0 for refused arguments).  Added under ABI 9.                                                     */
size_t ct_acg_u8_workspace_bytes(int batch, int height, int width, int n_iter, int bins, int n_nbits);
int ct_acg_u8(const uint8_t *target, const uint8_t *reference, int64_t n_r, const uint8_t *gt, int batch, int height, int width,
              const double *rot, const double *rinv, int n_iter, int bins, int input_f32, const int *nbits, int n_nbits,
              double *out_f64, float *out_f32, uint8_t *out_u8, double *psnr_out, void *ws, size_t ws_bytes, void *stream);

/* ---- test-set distortions (utils/data.py:12-22,120-125): torchvision.transforms.functional.adjust_* on a uint8 frame ----
 * in: uint8 [3][height][width] (what read_image returns).  kind: 0 identity, 1 brightness, 2 contrast, 3 saturation
 * (param = factor >= 0), 4 hue (param = hue_factor in [-0.5, 0.5]), 5 gamma (param = gamma >= 0, gain 1).
 * out_u8 (optional): the distorted uint8 frame; out_f32 (optional): that frame / 255 as float32 [3][H][W] -- the
 * `target / 255` the dataset hands over.  torchvision's tensor-backend arithmetic restated (float32, truncating casts; the
 * Python-float factor and 1 - factor are each rounded to float32, hence the double parameter).
 * ws: >= 8 bytes, 8-byte aligned.                                                                                      */
int ct_distort_u8(const uint8_t *in, int height, int width, int kind, double param, uint8_t *out_u8, float *out_f32,
                  void *ws, size_t ws_bytes, void *stream);

/* ---- corrected frames -> bytes (utils/postprocess.py:138-144: img_as_ubyte(x.clip(0, 1)) before the PNGs are written) ----
 * in: float32, [n][height][width][3] (CT_PACK_HWC: what ct_reinhard_* / the Runner produce) or [n][3][height][width]
 * (CT_PACK_CHW: the CNN modules, the sample dicts).  out_hwc: uint8 [n][height][width][3] in both layouts.
 * q = rint(clamp(x, 0, 1) * 255): one float32 multiplication by 255.0f (no fma, no reciprocal), round to nearest with ties to
 * even; NaN, -inf and negatives give 0, +inf and values above 1 give 255 -- skimage's float32 branch of img_as_ubyte restated
 * (np.multiply(image, 255, dtype=float32), np.rint, np.clip; parity unpinned: skimage is absent offline).
 * Sizes and bases off the 16-byte grid take an element-wise path of the same rule; `in` not aligned to 4 bytes: CT_E_ALIGN;
 * n, height or width < 1, a null pointer or an unknown layout: CT_E_BADARG.  No workspace.  Added under ABI 9.            */
#define CT_PACK_HWC 0
#define CT_PACK_CHW 1
int ct_pack_u8_f32(const float *in, int layout, int n, int height, int width, uint8_t *out_hwc, void *stream);

/* ---- bicubic resampling (the reference's demo notebook, cell 24: F.interpolate(x, scale_factor=0.75, mode="bicubic") around
 * DCMCS3DI and F.interpolate(result, size=(H, W), mode="bicubic") after it; csrc/resize.hip) -------------------------------
 * in: float32 [planes][h][w] (NCHW with planes = n * c), out: float32 [planes][ho][wo]; element offsets are 64-bit.
 * torch.nn.functional.interpolate(mode="bicubic", align_corners=False) of torch 2.10: cubic convolution with A = -0.75 on the
 * taps floor(s) - 1 .. floor(s) + 2 clamped to the border, s = scale * (o + 0.5) - 0.5; the result is not clamped.
 * scale_h / scale_w: the source step per output pixel as torch derives it -- 1 / scale_factor when the caller gave a factor,
 * in / out when it gave a size -- in double: coordinates and weights are evaluated in float64 (torch's float32 kernel rounds s
 * to float32), and without antialias the 16 taps are accumulated in float64 and rounded once.
 * antialias != 0: F.interpolate(..., antialias=True) -- separable, columns then rows, filter support 2 * max(scale, 1), taps cut
 * at the border, A = -0.5, weights normalised per output pixel; float32 intermediate [planes][h][wo] in ws
 * (ct_bicubic_resize_workspace_bytes; 0 without antialias, ws may be NULL then).  A reduction beyond 31-fold on an axis (more than
 * 128 taps) is CT_E_BADARG with antialias.
 * wo % 4 == 0 and a 16-byte aligned out take 16-byte stores, anything else an element-wise path of the same rule.
 * A null pointer, a size < 1 or a scale that is not in (0, 1e9]: CT_E_BADARG; in / out not aligned to 4 bytes: CT_E_ALIGN; ws
 * missing, misaligned or too small with antialias: CT_E_WORKSPACE.  Deterministic.  Added under ABI 9.                          */
size_t ct_bicubic_resize_workspace_bytes(int64_t planes, int h, int wo, int antialias);
int ct_bicubic_resize_f32(const float *in, float *out, int64_t planes, int h, int w, int ho, int wo, double scale_h,
                          double scale_w, int antialias, void *ws, size_t ws_bytes, void *stream);

/* ---- per-frame metric (first step): PSNR as Runner.test_step logs it (methods/__init__.py:32,37) ----
 * a, b: [batch][n_elems] float32 (any layout, same for both); out[i] = {mse, 10 log10(1/mse)} (data range 1).
 * Deterministic float64 reduction.  ws: batch * 1024 doubles (ct_workspace_bytes(CT_WS_LAB_STATS, ., batch) suffices). */
int ct_frame_psnr_f32(const float *a, const float *b, int64_t n_elems, int batch, double *out, void *ws,
                      size_t ws_bytes, void *stream);

/* ---- per-frame SSIM and iCID, the other metrics of Runner.test_step (methods/__init__.py:33,35) --------------------------
 * a (result, already clamped to [0,1] by the caller like methods/__init__.py:30), b (ground truth): [batch][3][height][width]
 * float32, NCHW planes; out[i] = the metric of frame i.
 *   ct_frame_ssim_f32  piq.ssim defaults: average-pool by f = max(1, round(min(H,W)/256)), 11x11 Gaussian (sigma 1.5) on
 *                      "valid" windows, k1 0.01, k2 0.03, mean over channels and positions; needs min(H,W)/f >= 11
 *   ct_frame_icid_f32  utils/icid.py:28-152 (intent "perceptual", all seven maps, downsampling on): bilinear resize by 1/f,
 *                      Lab, eleven 11x11 sigma-2 Gaussian moments with reflect padding, 1 - mean(product of the maps)
 * One fused tile kernel per metric + a fixed-order finishing kernel; float32 arithmetic like the reference's torch code,
 * float64 sums.  ws: ct_metric_workspace_bytes(height, width, batch).                                                  */
size_t ct_metric_workspace_bytes(int height, int width, int batch);
int ct_frame_ssim_f32(const float *a, const float *b, int height, int width, int batch, double *out, void *ws,
                      size_t ws_bytes, void *stream);
int ct_frame_icid_f32(const float *a, const float *b, int height, int width, int batch, double *out, void *ws,
                      size_t ws_bytes, void *stream);

/* ---- SSIM, iCID and FSIM read from a frame group's own buffers (csrc/ct_frame_src.h).  Entries added under ABI 9 (no argument
 * list changed).  result_hwc: float32 [batch][height][width][3], what a grouped transfer writes: NOT clamped -- every value is
 * clamped to [0, 1] as it is read, and a NaN stays a NaN (a frame of NaNs, as a persistent launch that gave up leaves it, scores
 * NaN).  gt_hwc: uint8 [batch][height][width][3]; byte k stands for (float)k / 255.0f (IEEE division, from a 256-entry table in
 * LDS).  Any byte alignment of gt_hwc; result_hwc on 4 bytes.
 * Contract: ct_frame_X_hwc_u8(a, b) is bitwise ct_frame_X_f32(clamp(a, 0, 1) as NCHW, float32(b) / 255 as NCHW) -- the same
 * kernels instantiated on another frame source, the same statements in the same order, the same partial sums in the same slots.
 * Workspaces are the planar entries' (ct_metric_workspace_bytes, ct_fsim_workspace_bytes; 256-byte aligned for FSIM), the filter
 * bank and constants those of ct_fsim_setup_f32, and the return codes follow the planar entries case by case: CT_E_BADARG for a
 * null pointer, batch < 0 and a frame too small for the metric, CT_E_WORKSPACE for a missing or short workspace, CT_OK and
 * nothing launched for batch == 0.  15 bytes read per pixel and metric.                                                        */
int ct_frame_ssim_hwc_u8(const float *result_hwc, const uint8_t *gt_hwc, int height, int width, int batch, double *out,
                         void *ws, size_t ws_bytes, void *stream);
int ct_frame_icid_hwc_u8(const float *result_hwc, const uint8_t *gt_hwc, int height, int width, int batch, double *out,
                         void *ws, size_t ws_bytes, void *stream);
int ct_frame_fsim_hwc_u8(const float *result_hwc, const uint8_t *gt_hwc, double *out, int batch, int h, int w,
                         const float *filters, const double *consts, void *ws, size_t ws_bytes, void *stream);

/* ---- iCID with the other arguments of utils/icid.py:28-34.  Entries added under ABI 9 (no argument list changed).
 *   intent        CT_ICID_*: the weights of utils/icid.py:42-47, float32 constants as torch.tensor([...]) makes them --
 *                 perceptual (0.002, 10, 10, 0.002, 0.002, 10, 10); hue-preserving: weight 5 (hue difference) = 0.02; chromatic:
 *                 weights 4 (chroma difference) and 5 = 0.02
 *   omit_maps67   non-zero: maps 6 (chroma contrast) and 7 (chroma structure) get exponent 0, i.e. are dropped exactly; the
 *                 three blurred moments only they read are not computed
 *   downsampling  zero: the maps are taken at the frame's own size (f = 1) instead of after the bilinear resize by 1 / f
 * The frames, `out` and the two frame sources are those of ct_frame_icid_f32 / ct_frame_icid_hwc_u8, whose kernels these are:
 * (CT_ICID_PERCEPTUAL, 0, 1) gives their results bit for bit, and the hwc_u8 form is bitwise the f32 form on the converted
 * tensors under every option.  ws: ct_icid_workspace_bytes(height, width, batch, downsampling) -- one float64 per 32 x 16 tile of
 * the map grid; with downsampling off and min(height, width) >= 384 that is MORE than ct_metric_workspace_bytes.
 * CT_E_BADARG (nothing launched): a null pointer, batch < 0, intent outside 0..2, a map grid smaller than 6 x 6 (reflect padding
 * of 5).  CT_E_WORKSPACE (nothing launched): no workspace or ws_bytes < ct_icid_workspace_bytes(...).  batch == 0: CT_OK, nothing
 * launched.                                                                                                                    */
enum { CT_ICID_PERCEPTUAL = 0, CT_ICID_HUE_PRESERVING = 1, CT_ICID_CHROMATIC = 2 };
size_t ct_icid_workspace_bytes(int height, int width, int batch, int downsampling);
int ct_frame_icid_opt_f32(const float *a, const float *b, int height, int width, int batch, int intent, int omit_maps67,
                          int downsampling, double *out, void *ws, size_t ws_bytes, void *stream);
int ct_frame_icid_opt_hwc_u8(const float *result_hwc, const uint8_t *gt_hwc, int height, int width, int batch, int intent,
                             int omit_maps67, int downsampling, double *out, void *ws, size_t ws_bytes, void *stream);

/* ---- a4: methods.iterative.iterative_distribution_transfer (methods/iterative.py:8-59) ----
 * Per iteration: projection on the rotated axes (float64, fma chain), exact lo/hi, 2x3 histograms
 * with numpy's bin rule (LDS-binned integer atomics), cumulative LUT, np.interp apply with the
 * `left=0` quirk, back-rotation.  The rotation matrices are DATA drawn by the caller (the
 * reference draws them from numpy's global RNG, iterative.py:32):
 *   rot, rinv : device [batch][n_iter][9] float64 row-major, rinv = inverse(rot)
 *   out       : device [batch][n_t][3] float64 (the reference returns float64); also the working image
 *   round_dr_f32 : 1 reproduces `d_r = np.empty_like(target.T)` being float32 on iteration 0 for
 *                  float32 callers (iterative.py:36)
 *   bins <= 1024, n_iter >= 1;  ws: ct_idt_workspace_bytes(batch, n_iter, bins) bytes
 *   dbg  : NULL, or device buffers receiving the integer/LUT state (parity probes):
 *          hist [batch][n_iter][2][3][bins] u32 (0 = target, 1 = reference), lut [batch][n_iter][3][bins][2]
 *          (f, slope), par [batch][n_iter][3][4] (lo, hi, step, bins/(hi-lo)), binidx [batch][n_iter][3][n_t] u16 */
typedef struct ct_idt_debug {
    unsigned int *hist;
    double *lut;
    double *par;
    unsigned short *binidx;
} ct_idt_debug;

size_t ct_idt_workspace_bytes(int batch, int n_iter, int bins);
int ct_idt_f32(const float *target, int64_t n_t, const float *reference, int64_t n_r, int batch,
               const double *rot, const double *rinv, int n_iter, int bins, int round_dr_f32,
               double *out, void *ws, size_t ws_bytes, const ct_idt_debug *dbg, void *stream);
int ct_idt_f64(const double *target, int64_t n_t, const double *reference, int64_t n_r, int batch,
               const double *rot, const double *rinv, int n_iter, int bins, int round_dr_f32,
               double *out, void *ws, size_t ws_bytes, const ct_idt_debug *dbg, void *stream);

/* ct_idt_u8: the same transfer for `batch` pairs of uint8 frames (target [batch][n_t][3], reference [batch][n_r][3]), bytes in and
 * float64, float32 and / or bytes out, through the kernels of ct_idt_f32 / ct_idt_f64 reading one 256-entry float64 table:
 *   input_f32 = 1 : byte k stands for (double)((float)k / 255.0f), a correctly rounded float32 division -- the float32 tensor
 *                   `frame / 255` that a Runner feeds to ct_idt_f32;
 *   input_f32 = 0 : byte k stands for (double)k / 255.0 (img_as_float).
 * With input_f32 = round_dr_f32 = 1 every probe of dbg and out_f64 are bitwise what ct_idt_f32 gives on float32(k) / 255, with
 * input_f32 = round_dr_f32 = 0 bitwise what ct_idt_f64 gives on k / 255.0.  out_f32 is out_f64 rounded once; out_u8 is
 * ct_pack_u8_f32's rule on that float32 value (rint(clamp(x, 0, 1) * 255), ties to even, NaN gives 0).  Each of the three
 * outputs is optional, all three NULL: CT_E_BADARG.  Without out_f64 the float64 working image lives in the workspace
 * (state_in_ws = 1: 24 bytes per pixel and pair) and the last apply sweep does not store it.
 * With gt (uint8 [batch][n_t][3]) and psnr_out, also psnr_out[i] = {mse, 10 log10(1 / mse)} in ct_mk_u8's layout and by its
 * rule: the float32 result clamped to [0,1] against gt as float32 k / 255 (IEEE float32 division), differences formed and summed
 * in float64 in a fixed order by the last apply sweep while it writes, one partial per workgroup, finished by one more launch;
 * the result is not read back.  A NaN result gives mse = NaN.  gt without psnr_out: CT_E_BADARG; gt == NULL: no metric.
 * Plain stream-ordered launches.  n_iter >= 1, bins <= 1024, else CT_E_BADARG; out_f64 / out_f32 / psnr_out off their element
 * size: CT_E_ALIGN; ws missing, not 16-byte aligned or smaller than ct_idt_u8_workspace_bytes(batch, n_iter, bins, n_t,
 * out_f64 == NULL): CT_E_WORKSPACE -- all before anything touches the device.  ct_idt_u8_workspace_bytes is 0 for refused
 * arguments; state_in_ws adds exactly 24 * n_t * batch bytes rounded up to 16.  Added under ABI 9.                          */
size_t ct_idt_u8_workspace_bytes(int batch, int n_iter, int bins, int64_t n_t, int state_in_ws);
int ct_idt_u8(const uint8_t *target, int64_t n_t, const uint8_t *reference, int64_t n_r, const uint8_t *gt, int batch,
              const double *rot, const double *rinv, int n_iter, int bins, int input_f32, int round_dr_f32,
              double *out_f64, float *out_f32, uint8_t *out_u8, double *psnr_out,
              void *ws, size_t ws_bytes, const ct_idt_debug *dbg, void *stream);

/* ---- a5-a9: DCMCS3DI forward building blocks (methods/dcmcs3di.py:41-66, pasmnet/ *.py) ----
 * NCHW float32 tensors as the reference's modules exchange them; exact-f32 MFMA arithmetic.
 *
 * ct_conv2d_f32: torch.nn.Conv2d(cin, cout, ksize, padding=ksize/2) + bias, then optionally
 *   LeakyReLU(0.01) (act=1; pasmnet/backbone.py:10), `+ residual` (ResB skip, backbone.py:15),
 *   clamp to [0,1] (dcmcs3di.py:61).  ksize in {1,3}, cout <= 64.
 *   wp   : weights packed [ksize*ksize][ceil(cin/2)][2][32*ceil(cout/32)] (zero padded):
 *          wp[ky*ksize+kx][ci/2][ci%2][co] = weight[co][ci][ky][kx]
 *   bias : [32*ceil(cout/32)] zero padded
 *   *_bstride : elements between consecutive images of the batch (lets in/out be channel slices)   */
int ct_conv2d_f32(const float *in, const float *wp, const float *bias, const float *residual,
                  float *out, int n, int cin, int cout, int h, int w, int ksize,
                  long long in_bstride, long long out_bstride, long long res_bstride, int act,
                  int clamp, void *stream);

/* The same convolution family on the bf16 matrix pipe with float32-grade accuracy (csrc/conv_split.hip): every float32
 * operand is split into three bf16 pieces and a product is the sum of the six partial products above 2^-16 of the
 * leading one, accumulated in float32 (error ~ one float32 rounding per product; NOT bitwise the fmaf chain of
 * ct_conv2d_f32).  Stride 1, padding k/2, kernel (kh,kw) in {3x3, 1x1, 1x5, 5x1} (f16 form also 2x2 with padding 1 on the top / left
 * only: see ct_space_to_depth2_f32); w % 4 == 0; in / out / residual
 * 16-byte aligned with batch strides % 4 == 0 (CT_E_BADARG otherwise: use ct_conv2d_f32 / ct_gconv2d_f32 then).
 * wp_split: bf16 bit patterns [ceil(cout/64)][ceil(cin/16)][kh*kw][piece hi,mid,lo][m][k-half][cout%32][8 channels];
 * bias: zero padded to 64*ceil(cout/64).  act: 0 none, 1 LeakyReLU(0.01), 2 ReLU, 3 sigmoid, 4 tanh, 5 swish.
 * in2 != NULL: input channels [cin1, cin) come from in2 (cin1 % 16 == 0) -- torch.cat([a, b], dim=1) without the copy
 * (reg_refine.py:43,72,75: the GRU's hx / [r*h, x] and the motion encoder's [cor, flo]).
 * in3 != NULL (needs in2): channels [cin2, cin) come from in3 (cin2 % 16 == 0, cin1 < cin2 < cin): DCMCS3DI's
 * transfer[0] reads cat([fea_left, fea_warped, valid_left]) (methods/dcmcs3di.py:59,47) from its three tensors.
 * f16 != 0: wp_split is the TWO-piece fp16 image of weight * 2^w_exp instead (ct_hip.pack_conv_weight_split16: same index order
 * with [piece hi,lo]; three v_mfma_f32_32x32x16_f16 per product, 2^-22 relative dropped; every staged 16-channel input tile
 * carries a running power-of-two scale per output tile (exponent clamped to +-100), so inputs with |x| < 2^111 are in
 * range; a tile maximum at or above 2^112 overflows fp16: inf / NaN results) -- half the matrix work.
 * post_op (f16 form only; p1 / p2 dense tensors with out's strides): 1 = the activated result times p1 (the GRU's r * h,
 * reg_refine.py:50), 2 = (1 - p1) * p2 + p1 * result (its gate h = (1 - z) h + z q, reg_refine.py:47,55), before the clamp.
 * residual: added after the activation (ResB skip), or -- res_pre_act != 0 -- BEFORE it: a pre-computed partial convolution
 * (the SepConvGRU's loop-invariant `inp` channels, reg_refine.py:25-55: conv(cat([h, inp, motion])) = conv_inp(inp) + conv(rest)).
 * scratch (nullable; f16 form; 16-byte aligned, >= ct_conv_split_scratch_bytes(), ALL ZERO before its first use, then owned by
 * the launches of ONE stream: each launch leaves its flag words zero again): lets a launch whose (8x32-pixel, 64-channel) units
 * do not fill a whole number of rounds of the 512 resident workgroups share the units' input-channel loops between neighbouring
 * workgroups (stream-K: e.g. 544 units take 1.06 rounds instead of 2).  The float32 sums of a shared unit are added in a fixed
 * order, so results are deterministic; they differ from the scratch == NULL result by float32 rounding only.
 * CT_E_WORKSPACE: scratch misaligned or too small. */
size_t ct_conv_split_scratch_bytes(void);
int ct_conv2d_split_f32(const float *in, const float *in2, int cin1, const float *in3, int cin2, const void *wp_split,
                        const float *bias, const float *residual, float *out, int n, int cin, int cout, int h, int w, int kh,
                        int kw, long long in_bstride, long long in2_bstride, long long in3_bstride, long long out_bstride,
                        long long res_bstride, int act, int clamp, int res_pre_act, int f16, int w_exp, int post_op,
                        const float *p1, const float *p2, void *scratch, long long scratch_bytes, void *stream);

/* ct_conv2d_split_f32 of one input tensor with the result stored as TOKEN ROWS: out_rows[(n*h + y)*w + x][rows_c0 + co] of a
 * [n*h, w, rows_channels] tensor (rows_channels, rows_c0, cout multiples of 4; rows_c0 + cout <= rows_channels).  The query / key /
 * value 1x1 convolutions of the parallax attention (pasmnet/attention.py:39-40,44-45, dcmcs3di.py:58) write the layout
 * ct_attention_rows64_f32 reads, so their NCHW tensors and the transposes never exist.  No residual / clamp in this form. */
int ct_conv2d_split_rows_f32(const float *in, const void *wp_split, const float *bias, float *out_rows, int n, int cin, int cout,
                             int h, int w, int kh, int kw, long long in_bstride, int rows_channels, int rows_c0, int act,
                             int f16, int w_exp, void *stream);

/* The same for the 1x1 convolutions in front of the parallax attention (pasmnet/attention.py:39-40,44-45: query / key; dcmcs3di.py:58: value),
 * 64 input channels -> cout <= 64 (a multiple of 4), as a STREAMING kernel of its own (csrc/conv1x1_rows.hip; new in ABI 9): exact float32
 * products on the float32 matrix pipe (v_mfma_f32_32x32x2_f32), the 64 x 64 weights in a wave's registers, no LDS, no barrier -- a 1x1
 * convolution is HBM-bound by a factor of two even there.  weight: the Conv2d weight itself, float32 [cout][64]; bias [cout];
 * out_rows / rows_channels / rows_c0 / act (0 .. 4) as above; out_rows and weight 16-byte aligned. */
int ct_conv1x1_rows_f32(const float *in, const float *weight, const float *bias, float *out_rows, int n, int cin, int cout, int h, int w,
                        long long in_bstride, int rows_channels, int rows_c0, int act, void *stream);

/* The ResB convolutions (3x3, stride 1, padding 1, 32 < cin <= 64; reference pasmnet/backbone.py:8-15, unimatch/backbone.py
 * residual blocks) on the weight-stationary kernel of csrc/conv_ws.hip with float32 operands as TWO fp16 pieces and three
 * v_mfma_f32_32x32x16_f16 per 16-channel product (float32 accumulation; 2^-22 relative is dropped: float32-grade, not bitwise
 * the fmaf chain).  Every staged input row is scaled by a power of two of its own (exponent clamped to +-100), the
 * weights by 2^w_exp, so inputs with |x| < 2^111 are in range (a row maximum at or above 2^112 overflows fp16: inf / NaN
 * results; the bf16 three-piece and exact-f32 modes have no such bound); 64 * h * w must be below 2^32 (32-bit indexing).  wp16: fp16 bit patterns [ceil(cout/64)][ceil(cin/16)][9][piece hi/lo][m][k-half][cout%32][8]
 * of weight * 2^w_exp; bias zero-padded to 64 * ceil(cout/64); act / clamp / residual as ct_conv2d_split_f32. */
int ct_conv3x3_ws16_f32(const float *in, const void *wp16, int w_exp, const float *bias, const float *residual, float *out, int n,
                        int cin, int cout, int h, int w, long long in_bstride, long long out_bstride, long long res_bstride, int act,
                        int clamp, void *stream);

/* The same convolution as Winograd F(2x2, 3x3) on the two fp16 pieces (csrc/conv_wino.hip): 16 instead of 36 multiplications per
 * 2x2 output tile and channel pair, i.e. 2.25x fewer matrix instructions -- the weight-stationary kernel above runs at the chip's
 * power limit on real data.  Same arguments, bounds and float32-grade rounding (3e-7 of the output range against float64; results
 * are not bitwise those of ct_conv3x3_ws16_f32); every tile row of four input rows carries one power-of-two scale.
 * wq16: fp16 bit patterns [ceil(cout/64)][16 positions][4 cout blocks][2 cin chunks][piece hi/lo][64 lanes][8] of
 * (G g G^T) * 2^w_exp in the A-fragment order of v_mfma_f32_16x16x32_f16 (ct_hip.pack_conv_weight_wino16). */
int ct_conv3x3_wino16_f32(const float *in, const void *wq16, int w_exp, const float *bias, const float *residual, float *out, int n,
                          int cin, int cout, int h, int w, long long in_bstride, long long out_bstride, long long res_bstride, int act,
                          int clamp, void *stream);
/* Which kernel ct_conv3x3_wino16_f32 launches (new in ABI 9; process-wide, atomic; env CT_HIP_WINO_FORM=1 presets 1):
 *   0 (default)  csrc/conv_wino4.hip: four waves of 512 registers per CU, the transformed weights in the accumulation registers, the
 *                input transform of the next two output rows inside the matrix phase of the current ones (images of 64 * h * w * 4
 *                bytes below 2^30; larger ones take form 1 by themselves);
 *   1            csrc/conv_wino.hip: the eight-wave, three-phase kernel of round 5.
 * Both are float32-grade and deterministic; they sum the sixteen positions in different orders, so they agree to rounding, not bitwise. */
int ct_set_conv_wino_form(int form);

/* Parallax attention, one direction (pasmnet/attention.py:39-41, utils.py:30, utils.py:123-125):
 *   P = softmax_j( sum_c q[c][h][i] k[c][h][j] / c ) ;  out_v[c][h][i] = sum_j P[i][j] v[c][h][j],
 *   out_rgb likewise for the 3 channels of `rgb` (dcmcs3di.py:58,65).  att: NULL, or [n][h][w][w]
 *   receiving P (the API's att_right2left).  w <= ~1000 (one 32-query tile of S lives in LDS).    */
int ct_pam_attend_f32(const float *q, const float *k, const float *v, const float *rgb,
                      float *out_v, float *out_rgb, float *att, int n, int c, int cv, int h, int w,
                      void *stream);
/* valid mask of the opposite direction (utils.py:31,34-35): valid[n][0][h][j] = 1.0 if
 * sum_i softmax_j(q.k/c)[i][j] > 0.1 else 0.0; colsum (nullable) receives the sums themselves.
 * ws: ct_pam_workspace_bytes(n,h,w).  Column sums are added in a fixed order (deterministic).   */
size_t ct_pam_workspace_bytes(int n, int h, int w);
int ct_pam_valid_f32(const float *q, const float *k, float *valid, float *colsum, float *att,
                     int n, int c, int h, int w, void *ws, size_t ws_bytes, void *stream);

/* ---- a10-a16: GMFlow / UniMatch matcher building blocks (unimatch/ *.py, as called by methods/dmsct.py:85-94) ----
 * float32, exact-f32 MFMA for the contractions.  "tokens" = channels-last [batch][H*W][C] (the layout the
 * reference's transformer uses, transformer.py:238-239); everything else NCHW.
 *
 * ct_gconv2d_f32: Conv2d with any kernel / stride / padding / channel count (backbone.py:14-17,53,67;
 *   trident_conv.py:64-72; reg_refine.py:16-17,33-39,65-69,104-107; unimatch.py:59). act: 0 none, 1 LeakyReLU(0.01),
 *   2 ReLU, 3 sigmoid, 4 tanh.  wp: output channels in groups of 64, [ceil(cout/64)][kh*kw][ceil(cin/2)][2][64] (zero
 *   padded); bias padded to 64*ceil(cout/64), or NULL.  Stride-1 "same" convolutions with a 3x3 / 1x1 / 1x5 / 5x1
 *   kernel and a bias run on the LDS-tiled persistent kernel of ct_conv2d_f32, everything else on a generic one.  */
int ct_gconv2d_f32(const float *in, const float *wp, const float *bias, float *out, int n, int cin,
                   int cout, int h, int w, int kh, int kw, int stride, int pad_h, int pad_w,
                   long long in_bstride, long long out_bstride, int act, void *stream);
/* InstanceNorm2d(affine=False) over `planes` planes of `plane` elements (backbone.py:10,34-39):
 *   mode 0: IN(x)   1: relu(IN(x))   2: relu(skip + relu(IN(x))).  ws (nullable, 8-byte aligned,
 *   ct_instance_norm_workspace_bytes(planes)): lets few large planes be split over several workgroups each.       */
size_t ct_instance_norm_workspace_bytes(int planes);
int ct_instance_norm_f32(const float *x, const float *skip, float *y, int planes, int plane, float eps,
                         int mode, void *ws, size_t ws_bytes, void *stream);
/* Space-to-depth by 2 of an NCHW tensor (h even, w % 8 == 0, 16-byte aligned): out[n][(2 sy + sx) c_total + c][y][x] =
 * in[n][c][2y + sy][2x + sx], out dense [n][4c][h/2][w/2].  With it a stride-2 3x3 "same" convolution (unimatch/backbone.py:14-17,
 * 53,67; trident_conv.py:64-72) is ct_conv2d_split_f32 with kh = kw = 2 (taps at block offsets -1 / 0, f16 form only) over 4c
 * channels, and a stride-2 1x1 convolution is the 1x1 convolution of its first c channels. */
int ct_space_to_depth2_f32(const float *in, float *out, int n, int c, int h, int w, long long in_bstride, void *stream);
/* elementwise: op 0 a+b, 1 a*b, 2 (1-a)*b + a*c (GRU update, reg_refine.py:47,55), 3 normalize_img (utils.py:26-34),
 *   4 a*s0, 5 tanh on channels < split / relu on the rest (unimatch.py:320-323)                                   */
int ct_eltwise_f32(const float *a, const float *b, const float *c, float *y, long long n, int op,
                   int plane, int chans, int split, float s0, void *stream);
/* nn.Linear on tokens: out[t][n] = act(x[t][:] . w[n][:] + bias[n]); w in PyTorch layout [n][k]; k % 16 == 0;
 *   act 0 none, 6 exact GELU (transformer.py:26-41; attention.py:181-182).  x2 == NULL: x is [tokens][k], k1 == k.
 *   x2 != NULL: the input row is [x[t][0:k1] | x2[t][0:k-k1]], k1 % 32 == 0 -- torch.cat([source, message], -1) in
 *   front of the FFN (transformer.py:131) without materialising it.                                               */
int ct_linear_tokens_f32(const float *x, const float *x2, int k1, const float *w, const float *bias, float *out,
                         long long tokens, int k, int n, int act, void *stream);
/* the same layer on the bf16 matrix pipe with float32-grade accuracy (operands as three bf16 pieces, six MFMAs per product;
 *   csrc/conv_split.hip's arithmetic): wp = the weight pre-split on the host as bf16 bit patterns
 *   [ceil(n/128)][k/32][piece hi/mid/lo][8-channel group 0..3][feature row 0..127][8 channels], zero rows beyond n
 *   (ct_hip.pack_linear_weight_split).  k % 32 == 0.                                                              */
int ct_linear_tokens_split_f32(const float *x, const float *x2, int k1, const void *wp, const float *bias, float *out,
                               long long tokens, int k, int n, int act, void *stream);
/* The FFN-shaped linears (transformer.py:33-35,131-133: mlp = Linear(256 -> 1024) . GELU . Linear(1024 -> 128), no bias) with the
 * weight slice RESIDENT in LDS and float32 operands as two fp16 pieces (csrc/linear_ws16.hip; three MFMAs per product, float32
 * accumulation, 2^-22 relative dropped; power-of-two scales: one per layer on the weights, a running one per 32-token tile on the
 * activations).  Two shapes:
 *   k == 256, n % 128 == 0, n / 128 in {1,2,4,8}: out[tokens][n] = act(x' w^T + bias); x' = [x[t][0:128] | x2[t][0:128]] (k1 = 128)
 *        or x[t][0:256] (x2 = NULL, k1 = 256);
 *   n == 128, k % 256 == 0, k / 256 in {1,2,4,8}, x2 = NULL, act = 0: out = PARTIAL slabs [k/256][tokens][128] whose sum is the
 *        result (bias in slab 0) -- ct_layernorm128_f32(partials = k/256) adds them in slab order on its way in;
 *   k == 128, n % 128 == 0, n / 128 in {1,2,3,4}, x2 = NULL: several 128 -> 128 layers reading the same tokens in one launch (the
 *        q / k / v projections, transformer.py:26-31; w = their weights stacked): out = slabs [n/128][tokens][128], one per layer.
 * wp16: ct_hip.pack_linear_weight_ws16: fp16 bit patterns [slice][piece hi/lo][k step 0..15][lane half][feature 0..127][8 channels]
 * of w * 2^w_exp, channel of (step s, half h, j) = 128 h + 8 s + j within the slice (k == 128: 8 steps, 64 h + 8 s + j).
 * act: 0 none, 6 exact GELU.  ln_gamma / ln_beta != NULL (k = n = 128 only): out = [ln_residual +] LayerNorm_128(x w^T + bias) -- the
 * merge projection with norm1 and the skip of transformer.py:120-127,139-147 in one launch.                                   */
int ct_linear_ws16_f32(const float *x, const float *x2, int k1, const void *wp16, int w_exp, const float *bias, float *out,
                       long long tokens, int k, int n, int act, const float *ln_gamma, const float *ln_beta,
                       const float *ln_residual, void *stream);
/* LayerNorm(128, eps 1e-5, affine) on tokens, out = residual + LN(x) when residual != NULL (transformer.py:139-147);
 * partials > 1: x is [partials][tokens][128] and the normalised input is the sum of the slabs (added in slab order) */
int ct_layernorm128_f32(const float *x, const float *gamma, const float *beta, const float *residual,
                        float *out, long long tokens, int partials, void *stream);
/* single-head attention on tokens (C = 128), streaming softmax: out = softmax(q k^T * scale + mask) v.
 *   cv = 128 (swin window attention, attention.py:48-107) or 2 (global correlation -> expected coordinate,
 *   matching.py:10-39; flow propagation, attention.py:199-216).  region: NULL, or int32 [batch][len] ids;
 *   pairs with different ids get the additive -100 of the shifted-window mask (utils.py:87-111).
 *   rowmap: NULL (token (b, i) is row b*len + i of q/k/v/out), or int32 [batch][len] row indices into q/k/v/out: the
 *   (shifted) window partition of attention.py:60-92,100-107 as a gather/scatter table instead of roll + permute.
 *   nsplit > 1: the keys are split over nsplit workgroups per query tile and merged by a second kernel (same result up
 *   to float rounding); ws needs ct_attention_workspace_bytes(batch, len, cv, nsplit).  Use it when batch*len/128
 *   workgroups cannot fill the 256 CUs.
 *   kv_shift (rowmap launches; else 0): the keys / values of a token are read kv_shift rows further (mod batch*len) than
 *   its query -- the cross attention of transformer.py:281-287 attends every image to the other half of the batch
 *   (kv_shift = batch*len/2) without materialising torch.cat(chunk(2)[::-1]).
 *   Arithmetic (this entry and the two ct_attention_*64_f32 below): both products on the 16-bit matrix pipe with float32
 *   operands as two fp16 pieces and power-of-two scales per query row / staged key tile / running per value tile
 *   (csrc/attention16.hip; 2^-22 relative dropped; a probability below 2^-29 of its row's maximum keeps an absolute error of
 *   2^-40 of it); env CT_HIP_ATT16=0 selects the three-piece bf16 kernels of csrc/attention_tokens.hip.            */
size_t ct_attention_workspace_bytes(int batch, int len, int cv, int nsplit);
int ct_attention_tokens_f32(const float *q, const float *k, const float *v, const int *region, const int *rowmap,
                            float *out, int batch, int len, int cv, float scale, int nsplit, float *ws,
                            size_t ws_bytes, long long kv_shift, void *stream);
/* Streaming parallax attention on 64-channel row tokens (pasmnet/attention.py:39-46, utils.py:30-35,123-125), for
 * image widths whose score tile does not fit LDS (ct_pam_* need w <= 1983) and as the faster path in general:
 *   ct_attention_rows64_f32 : out[b][i][0:96] = softmax_j(q_i.k_j*scale) v[b][j][0:96]   (v != NULL), and/or the row
 *                             statistics stats[b][i] = (max, sum) of that softmax (v == NULL: statistics only)
 *   ct_attention_colsum64_f32: colsum[b][j] = sum_i exp(q_i.k_j*scale - max_i) / sum_i  (the valid-mask numerator),
 *                             fixed summation order.  batch = N*H rows, len = W, tokens channels-last.                */
/* layout moves for the row attention: rows[(b*h + y)*w + x][c0 + ch] = nchw[b][ch][y][x] for ch < c (row_channels
 * floats per token in `rows`), and back.  nchw_bstride: elements between images (channel slices are fine).           */
int ct_nchw_to_rows_f32(const float *nchw, float *rows, int batch, int c, int h, int w, long long nchw_bstride,
                        int row_channels, int c0, void *stream);
int ct_rows_to_nchw_f32(const float *rows, float *nchw, int batch, int c, int h, int w, long long nchw_bstride,
                        int row_channels, int c0, void *stream);
int ct_attention_rows64_f32(const float *q, const float *k, const float *v, float *out, float *stats,
                            int batch, int len, float scale, void *stream);
int ct_attention_colsum64_f32(const float *q, const float *k, const float *stats, float *colsum,
                              int batch, int len, float scale, void *stream);
/* Disparity of the parallax attention (pasmnet/utils.py:55-105, regress_disp; csrc/disparity.hip).  Argument checks return
 * CT_E_BADARG before anything touches the device: a negative size, a null pointer (unless the call is empty: batch / n*h*w == 0 is
 * a no-op that accepts nulls), w > 32768 (the fill entries).
 *   ct_attention_rows64_disp_f32: ct_attention_rows64_f32 plus disp_ini[b][i] = i - sum_j softmax_j(q_i.k_j*scale) j, [batch][len],
 *       accumulated as sum_j P_ij (j - i) inside the streaming pass.  v != NULL: `out` exactly as ct_attention_rows64_f32(q, k, v,
 *       out, NULL, ...) writes it under the same settings (CT_HIP_ATT16 included), in the same pass; v == NULL (out ignored): the
 *       expected index alone.  No statistics.
 *   ct_pam_disp_fill_f32: the occlusion fill of regress_disp (utils.py:85-105).  disp_ini, valid, disp: [n][1][h][w] float32,
 *       valid 0 / 1 (the mask ct_pam_valid_f32 / the streaming path produce).  disp = disp_ini where valid; an invalid pixel k
 *       pixels right of the last valid pixel p of its row: disp_ini[p] / (1 + 1e-4), k times in float32 (bitwise the reference's
 *       loops); left of the row's first valid pixel f: disp_ini[f] divided (f - x) times; a row without a valid pixel: 0.
 *       disp may be disp_ini (in place).
 *   ct_pam_regress_disp_f32: regress_disp of a materialised att [n][h][w][w] (P[i][j], rows need not sum to 1):
 *       disp_ini = i - sum_j att[i][j] j in a fixed order, then the fill above, into disp [n][1][h][w].                  */
int ct_attention_rows64_disp_f32(const float *q, const float *k, const float *v, float *out, float *disp_ini,
                                 int batch, int len, float scale, void *stream);
int ct_pam_disp_fill_f32(const float *disp_ini, const float *valid, float *disp, int n, int h, int w, void *stream);
int ct_pam_regress_disp_f32(const float *att, const float *valid, float *disp, int n, int h, int w, void *stream);
/* matching.py:42-86: flow[b][2][h][w] from the softmax over the (2r+1)^2 integer neighbourhood; f0,f1 tokens       */
int ct_local_corr_softmax_f32(const float *f0, const float *f1, float *flow, int batch, int h, int w,
                              int radius, void *stream);
/* matching.py:89-126: corr[b][(2r+1)^2][h][w] = f0 . bilinear(f1, pos + window + flow) / sqrt(128); radius <= 4   */
int ct_local_corr_flow_f32(const float *f0, const float *f1, const float *flow, float *corr, int batch,
                           int h, int w, int radius, void *stream);
/* attention.py:220-256: (2r+1)^2 local window attention of flow; q = q_proj(f), k = k_proj(f) as tokens          */
int ct_local_attn_prop_f32(const float *q, const float *k, const float *flow, float *out, int batch, int h,
                           int w, int radius, void *stream);
/* F.interpolate(bilinear, align_corners=True) to (ho, wo); channel 0 scaled by mul0, the others by mul1           */
int ct_bilinear_resize_f32(const float *in, float *out, int n, int c, int h, int w, int ho, int wo,
                           float mul0, float mul1, void *stream);
/* geometry.py:68-75 flow_warp: bilinear sample at (x,y)+flow, zeros padding, align_corners=True                   */
int ct_flow_warp_f32(const float *img, const float *flow, float *out, int n, int c, int h, int w,
                     void *stream);
/* utils.py:137-155 convex upsampling by `factor` (mask [b][9*factor^2][h][w])                                     */
int ct_convex_upsample_f32(const float *flow, const float *mask, float *out, int b, int h, int w,
                           int factor, void *stream);
/* geometry.py:78-99 given flow_warp(bwd, fwd) and flow_warp(fwd, bwd): occlusion masks as 0/1 [b][h][w]          */
int ct_fb_check_f32(const float *fwd, const float *bwd, const float *warped_bwd, const float *warped_fwd,
                    float *fwd_occ, float *bwd_occ, int b, int h, int w, float alpha, float beta,
                    void *stream);

/* piq.fsim(result, gt) of Runner.test_step (methods/__init__.py:34; FSIMc, piq defaults; third-party, restated: parity
 *   unpinned).  ct_fsim_setup_f32 builds, once per frame size, the log-Gabor filter bank ([16][hp*wp] float32,
 *   orientation-major; hp x wp = ct_fsim_pooled_size) and its three noise constants per orientation ([4][3] float64) on
 *   the device; ct_frame_fsim_f32 scores `batch` frames [batch][3][h][w] in [0,1]: out[b] float64.  The 1 + 16 FFTs per
 *   image run in this library's own batched 2-D transform (ct_fft2d_c2c_f32 below; no vendor FFT, no plan, no state);
 *   ws: 256-byte aligned, ct_fsim_workspace_bytes(batch, h, w) (0: pooled frame beyond 4096 points on an axis).       */
/* Batched in-place 2-D complex DFT (csrc/fft2d.hip): `planes` planes [hp][wp] of interleaved (re, im) float32 -- what
 *   torch.fft.fft2 (inverse = 0) and torch.fft.ifft2 x hp x wp (inverse = 1: unnormalised) compute inside piq.fsim.  Mixed-radix
 *   Stockham transforms of whole lines in LDS (radices 4, 2, 3, 5 in registers, any other prime factor as a plain butterfly):
 *   every size with both axes <= 4096; asynchronous, no workspace.                                                    */
int ct_fft2d_c2c_f32(void *data, int hp, int wp, int planes, int inverse, void *stream);
int ct_fsim_pooled_size(int h, int w, int *hp, int *wp);
size_t ct_fsim_workspace_bytes(int batch, int h, int w);
/* host only: byte offsets, inside the workspace of ct_frame_fsim_f32(batch, h, w), of what the call leaves there -- out[0] the I / Q
 *   planes [2 batch][2][hp*wp], out[1] the Scharr magnitude [2 batch][hp*wp], out[2] the phase-congruency map [2 batch][hp*wp],
 *   out[3] the noise thresholds [2 batch][4], all float32, image index 2 * pair + (0: a, 1: b)                           */
int ct_fsim_stage_offsets(int batch, int h, int w, size_t out[4]);
int ct_fsim_setup_f32(int h, int w, float *filters, double *consts, void *ws, size_t ws_bytes, void *stream);
int ct_frame_fsim_f32(const float *a, const float *b, double *out, int batch, int h, int w, const float *filters,
                      const double *consts, void *ws, size_t ws_bytes, void *stream);

/* ---- f4: DMSCT's colour-correction network (methods/dmsct.py:34-56,96-116): segmentation_models_pytorch's EfficientNet-B2
 * encoder (efficientnet_pytorch MBConv blocks), UnetDecoder and SegmentationHead.  Third-party, absent offline: the
 * structure is restated in oracle/smp_unet.py ("parity unpinned").  float32 NCHW.  The 1x1 / 3x3 convolutions of these
 * layers are ct_gconv2d_f32 / ct_conv2d_split_f32 with the BatchNorm folded into weight and bias (act 5 = swish).
 *
 * ct_gconv2d_pad_f32: ct_gconv2d_f32's generic kernel with explicit top / left zero padding and output size (the bottom /
 *   right padding is what the output size implies): efficientnet_pytorch's static TF-"SAME" padding, e.g. (0, 1) for the
 *   stride-2 stem (Conv2dStaticSamePadding).
 * ct_dwconv_f32: depthwise k x k convolution (k 3 / 5, stride 1 / 2), same padding convention, BatchNorm folded into
 *   w [c][k*k] and bias [c], act 0 / 5 (`swish(bn1(depthwise_conv(x)))`, MBConvBlock.forward).  tile_sums (nullable):
 *   [n][c][ct_dwconv_tiles(out_h, out_w)] receives the sum of every output tile -- the squeeze of the SE gate.
 * ct_se_gate_f32: gate[n][c] = sigmoid(se_expand(swish(se_reduce(mean)))) with mean = sum(tile_sums) / plane (float64,
 *   fixed order); w_reduce [nsq][c], w_expand [c][nsq].
 * ct_scale_planes_f32: x[p][:] *= gate[p], in place (`torch.sigmoid(x_squeezed) * x`).
 * ct_upsample2_concat_f32: DecoderBlock.forward's `cat([interpolate(x, scale_factor=2, mode="nearest"), skip], 1)`.    */
int ct_gconv2d_pad_f32(const float *in, const float *wp, const float *bias, float *out, int n, int cin, int cout, int h,
                       int w, int kh, int kw, int stride, int pad_top, int pad_left, int out_h, int out_w,
                       long long in_bstride, long long out_bstride, int act, void *stream);
int ct_dwconv_tiles(int out_h, int out_w);
int ct_dwconv_f32(const float *in, const float *w, const float *bias, float *out, int n, int c, int h, int wd, int k,
                  int stride, int pad_top, int pad_left, int out_h, int out_w, int act, float *tile_sums, void *stream);
int ct_se_gate_f32(const float *tile_sums, int tiles, int plane, const float *w_reduce, const float *b_reduce,
                   const float *w_expand, const float *b_expand, float *gate, int n, int c, int nsq, void *stream);
int ct_scale_planes_f32(float *x, const float *gate, int planes, int plane, void *stream);
int ct_upsample2_concat_f32(const float *x, const float *skip, float *out, int n, int cx, int cs, int h, int w,
                            void *stream);

/* ---- diagnostic views: the image panel of the reference's log_images (methods/dcmcs3di.py:116-144, methods/dmsct.py:148-184),
 * csrc/views.hip.  float32 NCHW in, as the models hold their tensors; entries added under ABI 9 (no argument list changed).
 *
 * ct_view_chess_mix_f32: utils/visualizations.py:9-21.  x, y, out [b][c][h][w]; block (i, j) of size x size pixels (ragged at the
 *   bottom / right edge) comes from x when i + j is even, else from y.  Bitwise a copy.
 * ct_view_scaled_plane_f32: the min-max family, out [b][3][h][w].
 *   CT_VIEW_RGBMSE (visualizations.py:24-36, rgbmse): m = ((d0*d0 + d1*d1) + d2*d2) / 3 with d = x - y over the three channels of
 *     x, y [b][3][h][w] (torch's channel mean, operation for operation); channel 0 = (m - lo) / (hi - lo) with lo / hi the
 *     frame's own min / max of m, channels 1 and 2 = 0.
 *   CT_VIEW_GRAY (no counterpart in the reference: how its logger shows a one-channel image): x [b][1][h][w], y unused (may be
 *     NULL); all three channels = (x - lo) / (hi - lo).
 *   hi == lo gives NaN (0 / 0, like the reference).  Finite inputs only: non-finite ones do not fault, their result is unspecified.
 * ct_flow_to_image_u8: utils/flow_viz.py:184-264 (flow_to_image, what pred_flow_viz calls).  flow [b][2][h][w] -> out_hwc
 *   [b][h][w][3] bytes.  Per frame: pixels with |u| or |v| > 1e7 are unknown -- zero flow for the maximum, black in the image; so
 *   are NaN pixels (a deviation: the reference's own maximum turns NaN and with it the whole frame); maxrad = max sqrt(u^2 + v^2)
 *   in float32; then, in float64 as numpy >= 2 promotes the reference's `u / (maxrad + eps)`: u, v /= maxrad + 2^-52, the angle
 *   picks two neighbours of the 55-entry Middlebury wheel, radius <= 1 fades towards white, else x 0.75, floor(255 col).  An
 *   all-zero flow is white.
 * ws: 4-byte aligned, ct_view_workspace_bytes(b) bytes (the per-frame statistics; its content is private to one call).
 * Three launches each for the last two (initialise, reduce, map); deterministic.                                          */
#define CT_VIEW_RGBMSE 0
#define CT_VIEW_GRAY 1
int ct_view_chess_mix_f32(const float *x, const float *y, float *out, int b, int c, int h, int w, int size, void *stream);
size_t ct_view_workspace_bytes(int b);
int ct_view_scaled_plane_f32(const float *x, const float *y, float *out, void *ws, size_t ws_bytes, int b, int h, int w,
                             int kind, void *stream);
int ct_flow_to_image_u8(const float *flow, uint8_t *out_hwc, void *ws, size_t ws_bytes, int b, int h, int w, void *stream);

/* ---- the error maps of utils/visualizations.py that rest on kornia (rgbssim l.55-60, labmse l.39-44, abmse l.47-52),
 * csrc/errmaps.hip.  Entries added under ABI 9 (no argument list changed).  x, y, out [b][3][h][w] float32; out as
 * ct_view_scaled_plane_f32(CT_VIEW_RGBMSE) writes it: channel 0 = (m - lo) / (hi - lo) with the frame's own extremes of the
 * map m, channels 1 and 2 = 0; hi == lo gives NaN.  kornia's arithmetic is restated from its published source (parity unpinned).
 *
 * ct_view_ssim_map_f32: m = 0.5 - mean_c(ssim_c) / 2, the channels added in their order and divided by 3.  Per channel, with
 *   the normalised 11-tap Gaussian exp(-k^2 / (2 * 1.5^2)) applied along the rows, then the columns, under reflect padding of 5
 *   (no edge repeat): mu1, mu2, E[x^2], E[y^2], E[xy]; s11 = E[x^2] - mu1^2, s22 = E[y^2] - mu2^2, s12 = E[xy] - mu1 mu2;
 *   ssim = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s11 + s22 + C2) + 1e-12), C1 = 0.01^2, C2 = 0.03^2.
 *   h and w must exceed 5 (the reflect padding).
 * ct_view_lab_map_f32: lab = kornia's rgb_to_lab of (x - y)^2 (sRGB 0.04045 / 2.4, XYZ, D65, 0.008856 / 7.787 / 4/29);
 *   CT_VIEW_LABMSE: m = ((L + a) + b) / 3, CT_VIEW_ABMSE: m = (a + b) / 2.
 * Both compute m once, into channel 0, and scale it in place.  ws as above.  CT_E_BADARG, before anything is launched, for a
 * null pointer, b, h or w < 1, ws_bytes < ct_view_workspace_bytes(b), an unknown kind and, for the SSIM map, h < 6 or w < 6.
 * Three launches each (initialise, map, scale); deterministic; float32 arithmetic throughout.                               */
#define CT_VIEW_LABMSE 2
#define CT_VIEW_ABMSE 3
int ct_view_ssim_map_f32(const float *x, const float *y, float *out, void *ws, size_t ws_bytes, int b, int h, int w, void *stream);
int ct_view_lab_map_f32(const float *x, const float *y, float *out, void *ws, size_t ws_bytes, int b, int h, int w, int kind,
                        void *stream);

/* ---- PNG serialisation: the compressed half of a PNG file, csrc/png.hip (the reference writes its frames as PNG files,
 * utils/postprocess.py:138-144).  Entries added under ABI 9 (no argument list changed).
 *
 * ct_png_deflate_u8: frames [n][h][w][3] bytes (what ct_pack_u8_f32 and the views produce) -> per frame ceil(h / rows_per_chunk)
 *   independent deflate streams (RFC 1951), one per chunk of rows_per_chunk rows (the last one may be short), each ending on a byte
 *   boundary with non-final blocks only, so that a frame's chunks concatenate to one stream that an empty final block
 *   (01 00 00 FF FF) closes.  Per row one PNG filter (0 .. 4) by the minimum sum of absolute values, the lowest type on a tie;
 *   Up / Average / Paeth read the previous RAW row of the frame (zeros above row 0).  Per chunk either one dynamic-Huffman block of
 *   literals only (code lengths <= 15 built on the device; one distance code of zero bits; header layout: csrc/png.hip) followed by
 *   an empty stored block, or, when that would not be smaller, stored blocks of at most 65 535 bytes.
 *   streams: slot (frame, chunk) at byte (frame * chunks + chunk) * capacity, any alignment; capacity >= ct_png_slot_capacity(h, w,
 *     rows_per_chunk) = F + 5 ceil(F / 65535) + 5 with F = min(rows_per_chunk, h) * (3 w + 1) filtered bytes: no chunk is larger,
 *     and bytes of a slot beyond its size are not written.
 *   sizes [n][chunks] int32: the bytes of each stream.  adler [n][chunks][2] uint32: Adler-32 (s1, s2) of the chunk's filtered bytes
 *     from the initial value 1; the host combines them (utils/png.py).
 *   The bytes of a frame depend on that frame alone.  One launch, one workgroup per chunk, no workspace, asynchronous.
 *   CT_E_BADARG: a null pointer, a size < 1, rows_per_chunk > 1024, w > 2^20 or a chunk of 2 GB (ct_png_slot_capacity returns 0
 *   for those); CT_E_WORKSPACE: capacity too small or above 2^31 - 1; CT_E_ALIGN: sizes / adler not on 4 bytes.            */
long long ct_png_slot_capacity(int h, int w, int rows_per_chunk);
int ct_png_deflate_u8(const uint8_t *frames, int n, int h, int w, int rows_per_chunk, uint8_t *streams, long long capacity,
                      int *sizes, unsigned int *adler, void *stream);

/* ---- PNG decoding: the other direction, csrc/png_decode.hip (+ csrc/ct_inflate.h, the serial core, which also compiles on the
 * host).  For the files the reference's datasets hold: 8 bits, colour type 2, no interlace; the container is host work
 * (utils/png.py: parse).  Entries added under ABI 9 (no argument list changed).
 *
 * Per-stream status, written by both kernels: */
#define CT_INFLATE_OK 0
#define CT_INFLATE_BAD_HEADER 1        /* zlib header: CM != 8, CINFO > 7, FDICT set or not divisible by 31 */
#define CT_INFLATE_BLOCK_TYPE 2        /* the reserved block type 3 */
#define CT_INFLATE_STORED_LEN 3        /* stored block: LEN != ~NLEN */
#define CT_INFLATE_OVERSUBSCRIBED 4    /* code lengths over-subscribed */
#define CT_INFLATE_INCOMPLETE 5        /* code lengths incomplete (one distance or literal code of one bit is allowed), no end-of-block code */
#define CT_INFLATE_REPEAT 6            /* repeat symbol with no previous length, or running past HLIT + HDIST */
#define CT_INFLATE_INVALID_SYMBOL 7    /* 286 / 287, distance 30 / 31, bits that are no code, HLIT > 286, HDIST > 30 */
#define CT_INFLATE_DISTANCE 8          /* distance beyond the start of the output */
#define CT_INFLATE_INPUT_EXHAUSTED 9
#define CT_INFLATE_OUTPUT_TOO_LARGE 10 /* the stream holds more than its slot (or the slot is above 2^31 - 1 bytes) */
#define CT_INFLATE_OUTPUT_TOO_SMALL 11 /* the stream ended before the slot was full */
#define CT_INFLATE_ADLER 12            /* Adler-32 mismatch */
#define CT_INFLATE_FILTER 13           /* ct_png_unfilter_u8: a filter-type byte above 4 */
#define CT_INFLATE_DIMS 14             /* ct_png_unfilter_u8: h or w < 1, w > CT_PNG_MAX_WIDTH, or sizes that are not h (1 + 3 w) / 3 h w */
#define CT_PNG_MAX_WIDTH 8192          /* a row of packed pixels is handed from band to band in LDS */
/* ct_png_inflate_u8: n zlib streams (RFC 1950) back to back in src, stream i = bytes [src_offsets[i], src_offsets[i + 1]) at any
 *   alignment, inflated into dst bytes [dst_offsets[i], dst_offsets[i + 1]): it must inflate to exactly that many (< 2^31).
 *   src_offsets, dst_offsets: int64 [n + 1] ON THE DEVICE.  status [n] int32 and adler_out [n] uint32 (the Adler-32 of what was
 *   written, compared on the device with the stream's trailer) are written for every stream.  Nothing outside a stream's bytes is
 *   read and nothing outside its slot written, whatever the bytes are; a slot of a stream that fails holds an unspecified prefix.
 *   One 64-lane workgroup per stream, 37.5 KB of LDS (the 32 KB window as a ring), no workspace, asynchronous, deterministic.
 * ct_png_unfilter_u8: stream i = h (1 + 3 w) filtered bytes at filtered + offsets[i] (dims [n][2] int32 = h, w; offsets and
 *   dst_offsets int64 [n + 1], all on the device) -> planar uint8 [3][h][w] at dst + dst_offsets[i].  All five filter types of
 *   the PNG specification.  A stream whose status is not 0 on entry is skipped; status is set to CT_INFLATE_FILTER / _DIMS.
 * Both: CT_E_BADARG: a null pointer or n < 1; CT_E_ALIGN: an int64 array off 8 bytes, status / adler_out / dims off 4.        */
int ct_png_inflate_u8(const uint8_t *src, const long long *src_offsets, int n, uint8_t *dst, const long long *dst_offsets, int *status,
                      unsigned int *adler_out, void *stream);
int ct_png_unfilter_u8(const uint8_t *filtered, const long long *offsets, const int *dims, int n, uint8_t *dst,
                       const long long *dst_offsets, int *status, void *stream);

/* ---- training / validation samples (utils/data.py:25-84: ArtificialTrainValDataset.__getitem__ + apply_uniform_distortions),
 * csrc/augment.hip.  Entries added under ABI 9 (no argument list changed).  One call makes a batch of n samples from n source
 * pairs gt, ref: uint8 [n][3][height][width].  Per sample (ct_augment_sample):
 *   crop both views at (top, left) to crop_h x crop_w; swap_hflip: the new gt is the mirrored crop of ref and the new ref the
 *   mirrored crop of gt; vflip: both upside down; target = the chain kind[0 .. n_ops - 1] applied to the new gt.
 *   kind 0 .. 5 and their parameters as for ct_distort_u8 (the same device functions); 6 = torchvision's adjust_sharpness
 *   (param = factor >= 0): the image passes unchanged when crop_h <= 2 or crop_w <= 2; else blend(img, degenerate, factor) with
 *   degenerate = img on the one-pixel border and round_half_even(sum w x) over the 3 x 3 neighbourhood inside (w = 5/13 at the
 *   centre, 1/13 elsewhere, float32), cast to uint8.  one_minus[i] = 1.0 - param[i], formed by the caller in float64.
 *   Every operation works on the uint8 result of the one before it.  Contrast in position k blends with the mean grey of the
 *   whole crop after operations 0 .. k - 1 (an exact integer sum).  A kind may appear more than once, sharpness at most once.
 * samples: n records in HOST memory, checked before anything is launched; samples_dev: the same n records in device memory,
 *   which the kernels read (they clamp what they index with, whatever it holds).
 * out_gt, out_ref, out_target: float32 [n][3][crop_h][crop_w] = value / 255 (a float32 division); out_target_u8 (optional): the
 *   uint8 target.  ws: ct_augment_workspace_bytes(n) bytes, 8-byte aligned (the grey sums).
 * Launches: one over all samples, preceded -- only when a chain has a contrast -- by the zeroing of ws and one grey-sum launch
 *   per contrast of the longest such chain (one for the dataset's chains).  Deterministic.
 * CT_E_BADARG: a null pointer (out_target_u8 excepted), n, a size or a crop size < 1, more than 65535 samples, a crop that
 *   leaves the source, a flag that is not 0 / 1, n_ops outside 0 .. 6, an unknown kind, hue outside [-0.5, 0.5], a negative (or
 *   NaN) factor, two sharpness operations in one chain; CT_E_WORKSPACE: ws missing, misaligned or too small; CT_E_ALIGN: a float
 *   output off 4 bytes, samples_dev off 8.                                                                                  */
#define CT_AUGMENT_MAX_OPS 6
#define CT_AUGMENT_SHARPNESS 6
typedef struct {
    int top, left, swap_hflip, vflip, n_ops;
    int kind[CT_AUGMENT_MAX_OPS];
    int reserved;
    double param[CT_AUGMENT_MAX_OPS];
    double one_minus[CT_AUGMENT_MAX_OPS];
} ct_augment_sample;
size_t ct_augment_workspace_bytes(int n);
int ct_augment_u8(const uint8_t *gt, const uint8_t *ref, int n, int height, int width, const ct_augment_sample *samples,
                  const ct_augment_sample *samples_dev, int crop_h, int crop_w, float *out_gt, float *out_ref, float *out_target,
                  uint8_t *out_target_u8, void *ws, size_t ws_bytes, void *stream);

/* ---- step losses (methods/dmsct.py:118-131, methods/dcmcs3di.py: l1_loss, mse_loss, kornia's ssim_loss(window_size=11)),
 * csrc/losses.hip.  Entries added under ABI 9 (no argument list changed).  a (result), b (ground truth): float32
 * [batch][3][h][w]; out: float64 [batch][3] = per frame mean |a - b|, mean (a - b)^2, mean clamp((1 - ssim_c) / 2, 0, 1) over
 * channels and positions, ssim_c the per-channel map of ct_view_ssim_map_f32 (the same device code).  Differences and the map in
 * float32, as torch computes them; sums in float64 in a fixed order (a tile launch and a finishing launch): deterministic.
 * kornia's ssim_loss with reduction="mean" restated (parity unpinned).  ws: ct_frame_losses_workspace_bytes(batch, h, w) bytes,
 * 8-byte aligned.  CT_E_BADARG: a null pointer, batch < 1 or > 65535, h < 6 or w < 6 (the reflect padding), more than two
 * million rows; CT_E_WORKSPACE: ws missing, misaligned or too small; CT_E_ALIGN: a or b off 4 bytes.                         */
size_t ct_frame_losses_workspace_bytes(int batch, int h, int w);
int ct_frame_losses_f32(const float *a, const float *b, double *out, void *ws, size_t ws_bytes, int batch, int h, int w,
                        void *stream);

/* ---- the parallax-attention losses of the reference's step (methods/dcmcs3di.py:68-92 through pasmnet/losses.py), csrc/pam_losses.hip.
 * Entries added under ABI 9 (no argument list changed).  Per-image float64 SUMS and counts over materialised attention maps
 * att [n][h][w][w] float32 (att[b][h][i][j]: query column i, key column j); mask [n][1][h][w] float32 0 / 1.  Every term is formed
 * in float32 as the reference's torch code forms it and widened to float64 before it is added; workgroup partials in ws, added in
 * a fixed order by a finishing launch: deterministic, no atomics.  Nothing is divided here: a zero count stays zero, and the
 * caller's sum / count gives the reference's 0 / 0 = NaN.
 *   ws: ct_pam_losses_workspace_bytes(n, h, w) bytes (enough for every entry below at that size), 8-byte aligned.
 *   ct_pam_cycle_l1_f32: out [n][2] = { sum_h sum_i mask[h][i] sum_k |(A_h . B_h)[i][k] - delta_ik|, sum mask }: loss_pam_cycle's
 *       numerator and count for the cycle map att_a . att_b, which is never stored (exact-f32 MFMA, float32 fma chain over k).
 *   ct_pam_map_sweep_f32: out [n][5] = { sum |att[h][i][j] - att[h+1][i][j]|                     (count (h-1) w w),
 *                                        sum |att[h][i][j] - att[h][i+1][j+1]|                   (count h (w-1) (w-1)),
 *                                        sum_c sum_h sum_i mask[h][i] |dst[c][h][i] - sum_j att[h][i][j] src[c][h][j]|,
 *                                        sum_h sum_i mask[h][i] sum_j |att[h][i][j] - delta_ij|,
 *                                        sum mask }
 *       src, dst [n][3][h][w] and mask are nullable and only switch terms off (their slots are 0): the third needs all three, the
 *       fourth and fifth the mask.  w <= 1024.
 *   ct_masked_l1_f32: out [n][2] = { sum |x - y| * mask, sum mask } for x, y [n][a][p][b] and mask [n][p] (broadcast over a and b):
 *       the reference's masked_l1_loss, a = 3, b = 1 for images [n][3][h][w], a = 1, b = w for maps [n][h][w][w], p = h w.
 *       ws: at least n * 64 * 8 bytes.
 * CT_E_BADARG: a null pointer that is not optional, n < 1 or > 65535, a size < 1, h > 65535 (cycle), w > 1024 (sweep), src without
 * dst or mask; CT_E_WORKSPACE: ws missing, misaligned or too small; CT_E_ALIGN: a tensor off its element size.  All before
 * anything touches the device.                                                                                              */
size_t ct_pam_losses_workspace_bytes(int n, int h, int w);
int ct_pam_cycle_l1_f32(const float *att_a, const float *att_b, const float *mask, double *out, void *ws, size_t ws_bytes, int n,
                        int h, int w, void *stream);
int ct_pam_map_sweep_f32(const float *att, const float *src, const float *dst, const float *mask, double *out, void *ws,
                         size_t ws_bytes, int n, int h, int w, void *stream);
int ct_masked_l1_f32(const float *x, const float *y, const float *mask, double *out, void *ws, size_t ws_bytes, int n, int64_t a,
                     int64_t p, int64_t b, void *stream);

/* ---- perspective warp of uint8 frames (utils/postprocess.py:97 cv2.flip(left, 1); :127-136 crop to bbox, cv2.warpPerspective
 * with INTER_LINEAR and a constant 0 border, dsize = the crop's own size, second crop; csrc/warp.hip) ------------------------
 * raw: uint8 [n][src_h][src_w][3]; out: uint8 [n][out_h][out_w][3].  The source image of the warp is the crop
 * (crop_x, crop_y, crop_w, crop_h) of the raw frame -- with flip_x != 0 of the raw frame mirrored left-right,
 * raw[r][src_w - 1 - c] -- and a tap outside the crop is 0 even where the raw frame has pixels.  The destination is
 * crop_w x crop_h; only its window (out_x, out_y, out_w, out_h) is computed and stored.
 * maps: device float64 [n][9], or [9] with shared != 0: the DESTINATION -> SOURCE matrix, row-major (cv2's M after its own
 * invert; inverting is the caller's job).
 * The rule is OpenCV's fixed-point bilinear path (imgwarp.cpp up to 4.10, INTER_BITS = 5) restated; parity unpinned: cv2 is
 * absent offline, no version is pinned, and OpenCV 4.11 replaced the path with a float one.  For destination (row r, column c):
 *   bh0 = min(16, crop_h), bw0 = min(1024 / bh0, crop_w), x0 = (c / bw0) * bw0, x1 = c - x0;
 *   float64, one rounding per operation, no fma, left to right:
 *   X0 = M0*x0 + M1*r + M2;  Y0 = M3*x0 + M4*r + M5;  W0 = M6*x0 + M7*r + M8
 *   W  = W0 + M6*x1;  W = (W != 0) ? 32 / W : 0
 *   fX = max(-2^31, min(2^31 - 1, (X0 + M0*x1) * W)), fY likewise with M3;  X = (int)rint(fX) (ties to even), Y likewise
 *   sx = sat16(X >> 5), sy = sat16(Y >> 5), a = X & 31, b = Y & 31
 *   out = ((32-a)(32-b) p[sy][sx] + a(32-b) p[sy][sx+1] + (32-a)b p[sy+1][sx] + ab p[sy+1][sx+1] + 512) >> 10   per channel.
 * path: CT_WARP_AUTO / CT_WARP_GLOBAL read every tap from memory (the faster one at 1080p), CT_WARP_STAGED stages each tile's
 * source rows in LDS (raw and its row pitch on the 16-byte grid, else global taps); the bytes are the same.  out may have any alignment and width: of every
 * row of a tile the 16-byte runs on the grid leave as vector stores, the up to 15 bytes at either end element-wise.
 * Memory-safe for ANY matrix (taps are bounds-checked after the integer conversion); with non-finite entries the pixel
 * values are unspecified.  Deterministic, no workspace.
 * CT_E_BADARG, before anything is launched: a null pointer, any size < 1, crop_w or crop_h > 32767, a crop that is not inside the
 * raw frame, a window that is not inside the destination, an unknown path.  CT_E_ALIGN: maps off 8 bytes.  Added under ABI 9. */
#define CT_WARP_AUTO 0
#define CT_WARP_STAGED 1
#define CT_WARP_GLOBAL 2
int ct_warp_perspective_u8(const uint8_t *raw, int n, int src_h, int src_w, int flip_x, int crop_x, int crop_y, int crop_w,
                           int crop_h, const double *maps, int shared, int out_x, int out_y, int out_w, int out_h, uint8_t *out,
                           int path, void *stream);

/* ---- 8-bit Y'CbCr 4:2:0 <-> RGB bytes (csrc/yuv.hip, csrc/ct_yuv.h): what cv2.VideoCapture + swscale do
 * on the host in the reference (utils/postprocess.py:78-103), here on the device so that the link carries 1.5 bytes per pixel.
 * A frame is a packed I420 buffer: the Y plane [height][width], then Cb and Cr [ch][cw], ch = ceil(height / 2), cw = ceil(width / 2);
 * frame f starts at yuv + f * frame_stride bytes, frame_stride >= height * width + 2 * ch * cw.  RGB is uint8 [n][height][width][3].
 * Both directions give the correctly rounded value, ties to even, of an exact rational expression, computed in integers:
 *   Kr, Kb: BT.601 299/1000, 114/1000; BT.709 2126/10000, 722/10000; Kg = 1 - Kr - Kb
 *   (Yoff, Ys, Cs): limited (16, 219, 224), encode clamps Y to 16..235 and C to 16..240; full (0, 255, 255); chroma offset 128
 *   siting: centre = chroma at luma (2i + 1/2, 2j + 1/2) (Y4M C420jpeg / C420); left = at (2i + 1/2, 2j) (C420mpeg2)
 *   decode: chroma at a luma position is the bilinear interpolation of the plane (indices clamped), an exact count of sixteenths
 *     C16; y' = (Y - Yoff) / Ys, c' = (C16 - 2048) / (16 Cs), R' = y' + 2 (1 - Kr) cr', B' = y' + 2 (1 - Kb) cb',
 *     G' = y' - (2 Kb (1 - Kb) / Kg) cb' - (2 Kr (1 - Kr) / Kg) cr';  byte = rint(255 clamp(., 0, 1)).  Every input byte is taken.
 *   encode: Y = clamp(rint(Yoff + Ys (Kr r + Kg g + Kb b) / 255)); chroma from the exact weighted mean over the footprint (centre:
 *     the 2x2 box; left: (1, 2, 1) / 4 on columns 2j - 1 .. 2j + 1, two rows averaged; luma indices clamped to the frame):
 *     Cb = clamp(rint(128 + Cs (b - y) / (255 * 2 (1 - Kb)))), Cr likewise with r and Kr.
 * swscale / cv2 parity is unpinned (neither is present offline).  Any alignment and odd sizes are taken: runs of 16 luma columns
 * whose addresses sit on the 16-byte grid move as vectors, the rest byte by byte.  No workspace, deterministic.
 * CT_E_BADARG, before anything is launched: a null pointer, n, height or width < 1, height * width * 3 >= 2^31, a stride smaller
 * than the frame, n * ch * ceil(width / 16) >= 2^31 - 2^21, an unknown matrix, range or siting.  Added under ABI 9.             */
#define CT_YUV_BT601 0
#define CT_YUV_BT709 1
#define CT_YUV_LIMITED 0
#define CT_YUV_FULL 1
#define CT_YUV_SITING_CENTER 0
#define CT_YUV_SITING_LEFT 1
int ct_yuv420_to_rgb_u8(const uint8_t *yuv, int64_t frame_stride, int n, int height, int width, int matrix, int range, int siting,
                        uint8_t *out_rgb, void *stream);
int ct_rgb_to_yuv420_u8(const uint8_t *rgb, int n, int height, int width, int matrix, int range, int siting, uint8_t *out_yuv,
                        int64_t frame_stride, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CT_HIP_H */
