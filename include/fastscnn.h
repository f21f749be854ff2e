/* fastscnn.h — C ABI of libfastscnn_hip.so, the MI355X (gfx950) Fast-SCNN hot path.
 *
 * Plain pointers and sizes only (no torch types).  Every function returns 0 on success or a
 * negative status (-1 invalid argument, -2 unsupported, -3 HIP error); fscnn_last_error()
 * returns the thread-local message of the last failure.  The library never allocates device
 * memory: the caller passes arenas and workspaces.  Launches go to the caller's hipStream_t
 * (passed as void*), so calls are graph-capturable and overlap with RCCL on other streams.
 *
 * dtype codes: 0 = fp32, 1 = bf16, 2 = fp16 (a plan's arithmetic, and image / logit dtypes).
 * Activations are NHWC; images and logits are NCHW.
 *
 * Thread safety: every entry point may be called concurrently from several host threads (the
 * reference's torch.nn.DataParallel, train.py:170-171, runs one replica per device from its own
 * worker thread); a plan may be shared by calls on the device it was first used on.  The launch
 * profiler (fscnn_prof_*) is process-global and meant for single-threaded measurement.
 *
 * Reference interfaces replaced (Shinokawa/Fast-SCNN-pytorch):
 *   fscnn_net_* / fscnn_plan_* / fscnn_forward   FastSCNN.__init__ / forward
 *                                                 (models/fast_scnn.py:16-46)
 *   fscnn_backward                                autograd backward of that forward
 *                                                 (train.py:273 / :280 loss.backward())
 *   fscnn_ce_fwd / fscnn_ce_bwd                   nn.CrossEntropyLoss(ignore_index=-1)
 *                                                 (utils/loss.py:103-124, train.py:191)
 *   fscnn_sgd                                     torch.optim.SGD.step (train.py:195-198,274)
 *   fscnn_adamw / fscnn_adamw_segments            torch.optim.AdamW.step under GradScaler
 *                                                 (train_bdd100k.py:183-188, 258-266)
 *   fscnn_conv0_fwd                               _ConvBNReLU(3,32,3,2) (models/fast_scnn.py:153)
 *   fscnn_dw3x3_*                                 nn.Conv2d(groups=C, k=3, pad=1) (:70, :86)
 *   fscnn_pw_gemm / fscnn_pw_wgrad                nn.Conv2d(k=1) (:73, :103, :107, :124-128,
 *                                                 :198, :202, :230)
 *   fscnn_bn_*                                    nn.BatchNorm2d (:56, :71, :74, :87, :108)
 *   fscnn_bilinear_ac_*                           F.interpolate(bilinear, align_corners=True)
 *                                                 (:40, :135, :212)
 *   fscnn_pyramid_pool_*                          AdaptiveAvgPool2d(1,2,3,6) (:130-132)
 */
#ifndef FASTSCNN_H
#define FASTSCNN_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fscnn_net fscnn_net;
typedef struct fscnn_plan fscnn_plan;

const char* fscnn_version(void);
const char* fscnn_last_error(void);

/* ---- network: layer table + arena layout ------------------------------------------------ */
int fscnn_net_create(int num_classes, int aux, fscnn_net** out);
void fscnn_net_destroy(fscnn_net* net);
/* parameter arena (fp32, 64-B aligned tensors, named_parameters() order) */
int fscnn_net_param_count(const fscnn_net* net, int* count, long long* total_floats);
int fscnn_net_param_info(const fscnn_net* net, int i, const char** name, long long* offset,
                         long long* numel);
/* buffer arena: running_mean / running_var in a fp32 arena, num_batches_tracked in an int64
 * arena (for those entries *offset is the index into the int64 arena) */
int fscnn_net_buffer_count(const fscnn_net* net, int* count, long long* total_floats, int* num_bn);
int fscnn_net_buffer_info(const fscnn_net* net, int i, const char** name, long long* offset,
                          long long* numel);
/* backward stage s (0..3) finalises the gradients of parameters [begin, end) of the arena */
int fscnn_net_stage_range(const fscnn_net* net, int stage, long long* begin, long long* end);

/* ---- plan: shapes + workspace sizes for one (N, H, W, dtype, mode) ----------------------
 * train: 0 inference (BatchNorm folded, fused blocks), 1 training (batch statistics, running-stat
 * update, Dropout, staged backward), 2 differentiable inference (the training dataflow with
 * running-statistics BatchNorm: model.eval() under autograd) */
int fscnn_plan_create(const fscnn_net* net, int N, int H, int W, int dtype, int train,
                      fscnn_plan** out);
void fscnn_plan_destroy(fscnn_plan* plan);
int fscnn_plan_workspace(const fscnn_plan* plan, long long* fwd_bytes, long long* bwd_bytes);
int fscnn_plan_shapes(const fscnn_plan* plan, int* dims /* 10: H1 W1 H2 W2 H3 W3 H4 W4 H5 W5 */);
/* debug / stage-level parity: location of a named activation (e.g. "c2pw.a", "g_logits") in
 * the forward (in_bws = 0) or backward (in_bws = 1) workspace; rows x cols with row stride ld */
int fscnn_plan_buffer(const fscnn_plan* plan, const char* name, long long* offset, long long* rows,
                      int* cols, int* ld, int* in_bws);

/* ---- whole-network forward / backward ----------------------------------------------------- */
int fscnn_forward(const fscnn_plan* plan, const void* x, int x_dtype, void* out, int out_dtype,
                  const float* params, float* running, long long* nbt, void* ws,
                  unsigned long long dropout_seed, float dropout_p, float momentum,
                  void* stream);
int fscnn_backward(const fscnn_plan* plan, const void* dout, const void* x, int x_dtype,
                   const float* params, float* grads, void* ws, void* bws,
                   unsigned long long dropout_seed, float dropout_p, int stage_from,
                   int stage_to, void* stream);

/* General backward (any of the three heads above) that can also return the gradient of the input
 * image: autograd of x through the whole network (models/fast_scnn.py:33-46; the reference module
 * is differentiable in its input like any nn.Module).  Exactly one of dout (d logits, with daux for
 * an aux net) or grad_loss + loss2 (the fused loss head) is given.  dx: NCHW [N][3][H][W] in
 * dx_dtype (0 fp32, 1 bf16, 2 fp16), written by the stage-3 call, or null.
 * Plans: train = 1 (train-mode BatchNorm, batch statistics) or 2 (eval-mode autograd: every
 * BatchNorm normalised by its running statistics, Dropout off, no running-stat update; the
 * reference's model.eval() with grad enabled, e.g. eval.py:43). */
int fscnn_backward_dx(const fscnn_plan* plan, const void* dout, const void* daux,
                      const float* grad_loss, const float* loss2, const void* x, int x_dtype,
                      void* dx, int dx_dtype, const float* params, float* grads, void* ws,
                      void* bws, unsigned long long dropout_seed, float dropout_p, int stage_from,
                      int stage_to, void* stream);

/* FastSCNN(aux=True) (models/fast_scnn.py:24-31, 42-45): the same forward / backward plus the
 * auxiliary head (3x3 conv 64->32 + BN + ReLU + Dropout + 1x1 on the LearningToDownsample output,
 * upsampled like the main logits).  aux_out / daux: NCHW [N][C][H][W] in out_dtype.  Plans of an
 * aux net must use these entry points (fscnn_forward / fscnn_backward return -1;
 * fscnn_forward_loss covers the main output only and returns -2). */
int fscnn_forward_aux(const fscnn_plan* plan, const void* x, int x_dtype, void* out, void* aux_out,
                      int out_dtype, const float* params, float* running, long long* nbt,
                      void* ws, unsigned long long dropout_seed, float dropout_p, float momentum,
                      void* stream);
int fscnn_backward_aux(const fscnn_plan* plan, const void* dout, const void* daux, const void* x,
                       int x_dtype, const float* params, float* grads, void* ws, void* bws,
                       unsigned long long dropout_seed, float dropout_p, int stage_from,
                       int stage_to, void* stream);

/* Eval prediction (eval.py:43-45, demo.py:43-48 consume only torch.argmax(outputs[0], 1)):
 * forward of an inference plan whose final bilinear upsample is fused with the argmax over classes;
 * labels [N][H][W] (label_dtype 0: int64 like torch.argmax, 1: uint8).  No logits are written. */
int fscnn_predict(const fscnn_plan* plan, const void* x, int x_dtype, void* labels,
                  int label_dtype, const float* params, float* running, long long* nbt, void* ws,
                  void* stream);
/* Validation step (Trainer.validation, train.py:370-439): forward of an inference plan that ends
 * in one fused head over the low-resolution logits instead of the upsample.  It forms every
 * full-resolution logit exactly as fscnn_forward stores it and leaves behind only
 *   loss[0]  (device float) the criterion of the main output: head 0 = cross entropy with
 *            ignore_index (NaN when no pixel is valid, like the mean over no element), head 1 =
 *            the Dice / Focal+Dice loss with the scalars of fscnn_forward_loss_dice; on an aux
 *            net with aux_weight != 0, plus aux_weight times the criterion of the aux output;
 *   counts   (int64 [2 + 3*num_classes], ACCUMULATED; may be null) the fscnn_seg_metric
 *            counters of argmax(main output) against target.
 * No logits and no labels are written; two calls on the same inputs give the same bits.
 * head_ws: fscnn_validate_ws_bytes(plan) bytes for the partial sums (negative, fscnn_last_error
 * set, unless the plan is an inference plan).  Returns -1 for training plans and -2 for
 * geometries the head does not take (num_classes above 32, Dice below 2, low-resolution rows
 * that do not fit its LDS staging): use fscnn_forward + the unfused criterion there. */
long long fscnn_validate_ws_bytes(const fscnn_plan* plan);
int fscnn_validate(const fscnn_plan* plan, const void* x, int x_dtype, const long long* target,
                   int head, long long ignore_index, float smooth, float dice_weight,
                   float focal_weight, float alpha, float gamma, float aux_weight, float* loss,
                   long long* counts, const float* params, float* running, long long* nbt,
                   void* ws, void* head_ws, void* stream);
/* Deployment pipeline (EndToEndFastSCNN, export_onnx_fixed.py:34-98; the host's argmax * 255 lane
 * mask, kuruma/core/preprocessing.py:53-79): raw 0..255 frames in, class probabilities out.
 * Every resampling here is F.interpolate(mode='bilinear', align_corners=False) without
 * antialiasing: output position o of an in -> out resize reads source position
 * max((o + 0.5) * in / out - 0.5, 0), taps floor(s) and min(floor(s) + 1, in - 1); the position
 * is evaluated exactly, as the rational ((2o + 1) in - out) / (2 out).  Every size is <= 16384.
 *
 * fscnn_e2e_pre: frames -> the backbone's input y, dense NCHW [N][3][base][base] in y_dtype
 *   (0 fp32, 1 bf16, 2 fp16): resize h x w -> base x base, / 255, then (v - mean[c]) / std[c]
 *   when both are given; fp32 lerp, one rounding at the store.  x: x_dtype 0 / 1 / 2 or
 *   FSCNN_DT_U8 (3); NCHW [N][3][h][w], or NHWC [N][h][w][3] with channels_last != 0; bgr != 0
 *   reads channel 2 - c for output channel c.  mean / std: HOST arrays of 3 floats (as
 *   fscnn_normalize_u8), both or neither null.  h, w >= 2; base >= 1.
 * fscnn_e2e_head: the low-resolution logits of an inference plan (NHWC [N][Hc][Wc][ldx], the
 *   buffer fscnn_predict's head reads) -> the pipeline's output at h_out x w_out.  For each
 *   output pixel the four taps of the base x base grid are formed exactly as fscnn_forward stores
 *   them (align_corners=True upsample, rounded to the logits dtype), combined in fp32, and then
 *   probs [N][C][h_out][w_out] in probs_dtype = their softmax over C (softmax != 0) or the
 *   resampled logits themselves; labels [N][h_out][w_out] uint8 = (argmax * label_scale) mod 256,
 *   ties to the lowest class.  Either output may be null.  Returns -2 (nothing launched) when
 *   C > 32 or the low-resolution window of an output tile does not fit the LDS staging.
 * fscnn_forward_e2e: front end, backbone and tail on `stream`; plan: an inference plan
 *   (train = 0) created for N x base x base, whose dtype is the backbone's arithmetic and the
 *   dtype of the front end's output.  ws: fscnn_e2e_ws_bytes(plan) bytes (negative for a training
 *   plan) = the plan's forward workspace followed by the front end's output; nothing else of full
 *   resolution is written.  Returns -2 before any launch where fscnn_e2e_head would. */
#define FSCNN_DT_U8 3
int fscnn_e2e_pre(const void* x, int x_dtype, int channels_last, int bgr, int N, int h, int w,
                  int base, const float* mean, const float* std, void* y, int y_dtype,
                  void* stream);
int fscnn_e2e_head(const void* logits, int dtype, int N, int Hc, int Wc, int C, int ldx, int base,
                   int h_out, int w_out, int softmax, void* probs, int probs_dtype,
                   unsigned char* labels, int label_scale, void* stream);
long long fscnn_e2e_ws_bytes(const fscnn_plan* plan);
int fscnn_forward_e2e(const fscnn_plan* plan, const void* x, int x_dtype, int channels_last,
                      int bgr, int h, int w, const float* mean, const float* std, int h_out,
                      int w_out, int softmax, void* probs, int probs_dtype, unsigned char* labels,
                      int label_scale, const float* params, float* running, long long* nbt,
                      void* ws, void* stream);
/* Bird's-eye tail of the deployment pipeline: what the reference's consumers do to the lane mask
 * before anything is steered -- the nearest-neighbour perspective warp to the bird's-eye view
 * (PerspectiveTransformer.transform_image_and_mask, kuruma/vision/transform.py:130-201) and the
 * per-row scan of the warped mask (PathPlanner.extract_centerline / extract_centerline_fast,
 * kuruma/vision/path_planning.py:188-293) -- in one launch, one workgroup per bird's-eye row.
 *
 * Coordinate law.  m[9]: HOST doubles, the destination -> source matrix (the inverse of the
 * matrix cv2.warpPerspective is given), all finite, otherwise -1.  For destination pixel (x, y),
 * in fp64, every operation rounded on its own (no fused multiply-add):
 *     X = (m0*x + m1*y) + m2      Y = (m3*x + m4*y) + m5      W = (m6*x + m7*y) + m8
 *     W = (W != 0) ? 1.0 / W : 0
 *     fx = max(INT_MIN, min(INT_MAX, X*W))  (a NaN product counts as INT_MAX)
 *     sx = rint(fx)  (half to even);  fy, sy the same from Y
 * The pixel takes the source value at (sx, sy) when 0 <= sx < w and 0 <= sy < h, else 0.  This is
 * the shape of OpenCV's classic nearest-neighbour perspective warp with a constant 0 border;
 * bit parity with a particular OpenCV build is not claimed.
 *
 * Outputs.  bev: uint8 [N][Hb][Wb], may be null.  rows: int32 [N][Hb][4] per bird's-eye row:
 *   [0], [1]  run_start, run_end (exclusive) of the longest run of non-zero pixels of length
 *             >= min_width, the leftmost of equally long runs; 0, 0 when there is none
 *             (centre of the exact centreline: (run_start + run_end) / 2, rounded down)
 *   [2], [3]  count of non-zero pixels and the sum of their column indices (the fast
 *             centreline: index_sum / count, rounded down, where count >= min_width)
 * Exact, deterministic, no atomics.
 * Limits: 1 <= N <= 65535, 1 <= Wb <= 8192, 1 <= Hb <= 65535, min_width >= 1; the logits source
 * additionally needs 1 <= C <= 32 and every size <= 16384.  Outside them: -2, nothing launched.
 *
 * fscnn_bev_mask: source (a), a uint8 mask [N][h][w] in device memory.
 * fscnn_e2e_bev: source (b), the low-resolution logits of an inference plan as fscnn_e2e_head
 *   takes them; the value at (sx, sy) is (argmax * label_scale) mod 256, evaluated exactly as
 *   fscnn_e2e_head evaluates its label at output pixel (sx, sy) of an h x w output (same code).
 *   The h x w mask itself is never written.
 * fscnn_forward_e2e_bev: front end, backbone and the bird's-eye tail on `stream`; plan, frames
 *   and ws (fscnn_e2e_ws_bytes) as fscnn_forward_e2e.  Returns -2 before any launch outside the
 *   limits above and when FSCNN_E2E_FUSED=0, like fscnn_forward_e2e. */
int fscnn_bev_mask(const unsigned char* mask, int N, int h, int w, const double* m, int Hb, int Wb,
                   int min_width, unsigned char* bev, int* rows, void* stream);
int fscnn_e2e_bev(const void* logits, int dtype, int N, int Hc, int Wc, int C, int ldx, int base,
                  int h, int w, int label_scale, const double* m, int Hb, int Wb, int min_width,
                  unsigned char* bev, int* rows, void* stream);
int fscnn_forward_e2e_bev(const fscnn_plan* plan, const void* x, int x_dtype, int channels_last,
                          int bgr, int h, int w, const float* mean, const float* std, int h_out,
                          int w_out, int label_scale, const double* m, int Hb, int Wb,
                          int min_width, unsigned char* bev, int* rows, const float* params,
                          float* running, long long* nbt, void* ws, void* stream);
/* Overlay tail of the deployment pipeline: the picture every consumer of the exported model builds
 * on the host from the frame and the lane mask (create_visualization,
 * kuruma/core/preprocessing.py:85-104: green where mask > 0, then cv2.addWeighted(frame, 1, green,
 * alpha, 0); the evaluation scripts blend a per-class colour image at 0.7 / 0.3 or 0.6 / 0.4),
 * after the nearest-neighbour resize of the mask back to the camera frame
 * (postprocess_matched_resolution, :53-79).  One launch: the frame is read once and the blended
 * uint8 frame is written once.  Bit parity with a particular OpenCV build is not claimed; the law
 * below is what is tested.
 *
 * The law.  For output pixel (n, y, x) of an h x w frame and channel k (channels in the frame's
 * own order; colours are given in that order, no BGR swap), with a mask of Hm x Wm:
 *   source   sx = (x * Wm) div w, sy = (y * Hm) div h in exact integer division -- cv2.INTER_NEAREST's
 *            floor(x * Wm / w) taken as a rational; the identity when both sizes agree.  Every
 *            size is <= 16384.
 *   label    L = the mask byte at (sy, sx).  From the logits: L = (argmax * label_scale) mod 256,
 *            evaluated exactly as fscnn_e2e_head evaluates its label at output pixel (sx, sy) of
 *            an h_out x w_out output (same code: strict >, the lowest class wins ties).
 *   lane     o_k = color[k] where L != 0, else 0.
 *   palette  id = the mask byte (mask in memory) or the argmax (logits);
 *            o_k = palette[id][k] if id < P, else 0; palette: uint8 [P][3], 1 <= P <= 256.
 *   blend    a = the frame value as fp32 (frames: dtype 0 fp32, 1 bf16, 2 fp16, 3 uint8);
 *            t = ((a * frame_weight) + (o_k * alpha)) + gamma, each of the four operations rounded
 *            to fp32 on its own (no fused multiply-add).
 *   store    out = uint8(min(max(rint(t), 0), 255)), round half to even, NaN -> 0
 *            (saturate_cast<uchar> of cv2.addWeighted).
 * out: uint8 in the layout of the frames ([N][h][w][3] with channels_last != 0, else [N][3][h][w]),
 * a buffer of its own: aliasing the frames is refused (-1).  mask_out: uint8 [N][h][w] = L of every
 * frame pixel (what postprocess_matched_resolution returns), may be null.  h, w >= 2.
 *
 * fscnn_overlay_mask: a uint8 mask [N][Hm][Wm] in device memory.  palette: DEVICE uint8 [P][3]
 *   (palette mode), or null for lane mode with color = HOST uint8[3].  -2 when a size exceeds the
 *   limit.
 * fscnn_e2e_overlay: the low-resolution logits of an inference plan as fscnn_e2e_head takes them.
 *   Both modes are one form here: colors = HOST uint8 [min(C, 32)][3], the colour of class id, and
 *   class_mask, whose bit id tells whether class id gets its colour (lane mode: color in every
 *   row, bit id = ((id * label_scale) mod 256 != 0); palette mode: the palette's rows, bit id =
 *   (id < P)).  Returns -2 (nothing launched) when C > 32, a size exceeds the limit or the
 *   low-resolution window of a 64 x 4 tile of frame pixels does not fit the LDS staging (a frame
 *   much smaller than h_out x w_out).
 * fscnn_forward_e2e_overlay: front end, backbone and the overlay tail on `stream`; plan, frames
 *   (x: both the front end's input and the blend's), mean / std and ws (fscnn_e2e_ws_bytes) as
 *   fscnn_forward_e2e.  Returns -2 before any launch where fscnn_e2e_overlay would and when
 *   FSCNN_E2E_FUSED=0, like fscnn_forward_e2e. */
int fscnn_overlay_mask(const void* frames, int frame_dtype, int channels_last, int N, int h, int w,
                       const unsigned char* mask, int Hm, int Wm, const unsigned char* color,
                       const unsigned char* palette, int P, float frame_weight, float alpha,
                       float gamma, unsigned char* out, unsigned char* mask_out, void* stream);
int fscnn_e2e_overlay(const void* logits, int dtype, int N, int Hc, int Wc, int C, int ldx,
                      int base, int h_out, int w_out, int label_scale, const void* frames,
                      int frame_dtype, int channels_last, int h, int w,
                      const unsigned char* colors, unsigned class_mask, float frame_weight,
                      float alpha, float gamma, unsigned char* out, unsigned char* mask_out,
                      void* stream);
int fscnn_forward_e2e_overlay(const fscnn_plan* plan, const void* x, int x_dtype,
                              int channels_last, int bgr, int h, int w, const float* mean,
                              const float* std, int h_out, int w_out, int label_scale,
                              const unsigned char* colors, unsigned class_mask,
                              float frame_weight, float alpha, float gamma, unsigned char* out,
                              unsigned char* mask_out, const float* params, float* running,
                              long long* nbt, void* ws, void* stream);
/* Colour bird's-eye view of the deployment pipeline: the other half of
 * PerspectiveTransformer.transform_image_and_mask (kuruma/vision/transform.py:174-180) -- the
 * camera frame warped to the bird's-eye view with cv2.INTER_LINEAR and a constant 0 border -- and,
 * in the same launch, the segmented bird's-eye picture (create_visualization of the warped frame
 * and the warped mask, kuruma/core/inference.py:275-287).  One workgroup per 256 pixels of a view
 * row.
 *
 * The law is the shape of OpenCV's fixed-point bilinear remap for 8-bit images as warpPerspective
 * drives it: 5 fractional coordinate bits, product weights.  Bit parity with a particular OpenCV
 * build is not claimed; the law below is what is tested.
 * m[9]: HOST doubles, destination -> source as for fscnn_bev_mask, all finite, otherwise -1.  For
 * view pixel (x, y), in fp64, every operation rounded on its own (no fused multiply-add):
 *     X = (m0*x + m1*y) + m2      Y = (m3*x + m4*y) + m5      W = (m6*x + m7*y) + m8
 *     W = (W != 0) ? 32.0 / W : 0
 *     fx = rint(max(INT_MIN, min(INT_MAX, X*W)))  (a NaN product counts as INT_MAX; half to even)
 *     sx = fx >> 5 (arithmetic), ax = fx & 31;  fy, sy, ay the same from Y
 * The four taps are p00 = (sx, sy), p10 = (sx+1, sy), p01 = (sx, sy+1), p11 = (sx+1, sy+1); a tap
 * outside 0 <= . < w, 0 <= . < h contributes 0, each tap on its own.  Per channel, in integers:
 *     S   = (32-ax)(32-ay)*p00 + ax(32-ay)*p10 + (32-ax)ay*p01 + ax*ay*p11
 *     out = (S + 512) >> 10
 * (the same integer as a 15-bit weight table with + 2^14 >> 15: product weights of 5-bit fractions
 * are exact multiples of 32).  Exact, deterministic, no atomics.
 *
 * frames: uint8 only, [N][h][w][3] with channels_last != 0, else [N][3][h][w]; channels are never
 * swapped.  image: the warped frames, uint8 in the layout of the frames ([N][Hb][Wb][3] or
 * [N][3][Hb][Wb]).  blended: the overlay law's lane mode and blend above applied to the warped
 * byte a: o_k = color[k] (HOST uint8[3], in the frames' channel order) where the byte of bev_mask
 * (uint8 [N][Hb][Wb], e.g. fscnn_bev_mask's) is not 0, else 0;
 * t = ((a * frame_weight) + (o_k * alpha)) + gamma in fp32, out = uint8(min(max(rint(t), 0), 255)),
 * NaN -> 0 (the same device function).  image and blended may each be null, not both (-1);
 * blended needs bev_mask and color (-1).  The outputs are buffers of their own: aliasing the
 * frames, the mask or each other is refused (-1).
 * Limits: 1 <= N <= 65535, 1 <= Wb <= 8192, 1 <= Hb <= 65535, 2 <= h, w <= 16384.  Outside them:
 * -2, nothing launched. */
int fscnn_bev_image(const unsigned char* frames, int channels_last, int N, int h, int w,
                    const double* m, int Hb, int Wb, unsigned char* image,
                    const unsigned char* bev_mask, const unsigned char* color /* HOST[3] */,
                    float frame_weight, float alpha, float gamma, unsigned char* blended,
                    void* stream);
/* Steering tail of the deployment pipeline: from the row table of the bird's-eye tail to the two
 * wheel commands, what the reference does on the host with PathPlanner.smooth_path /
 * generate_waypoints / plan_complete_path / _calculate_path_length
 * (kuruma/vision/path_planning.py:316-525) and VisualLateralErrorController.compute_wheel_pwm
 * (kuruma/control/visual_controller.py:72-207, 236-308).  One launch, one workgroup per frame, no
 * workspace, no atomics; the host reads nothing in between.
 *
 * The law, per frame, from rows[Hb][4] (run_start, run_end, count, index_sum); all arithmetic fp64.
 *   selection  fast != 0 (extract_centerline_fast): the rows y = Hb-1, Hb-1-skip_rows, ...
 *              (scan_from_bottom != 0) or y = 0, skip_rows, ... whose count >= min_width and > 0;
 *              pixel px = index_sum div count.  fast == 0 (extract_centerline): every row with
 *              run_end > run_start and run_end - run_start >= min_width; px = (run_start + run_end)
 *              div 2; skip_rows and scan_from_bottom are not read.  World point
 *              (x, y) = (min_x + px / pixels_per_unit, min_y + py / pixels_per_unit).
 *              plan_complete_path's fast mode passes min_width div 2, skip_rows 3 and
 *              degree = min(2, degree): those defaults are the caller's (path.py), not the kernel's.
 *   fit        weighted least squares x = f(y), degree d in 1 .. 3, every centreline point with
 *              weight 1; with force_bottom_center one more point (anchor_x, anchor_y) of weight 1e6,
 *              the weight multiplying the row [y^d .. y 1 | x] as in np.polyfit(..., w=).  No
 *              centreline point: no path (FSCNN_PATH_NO_CENTERLINE; the reference's early return,
 *              taken even where the anchor alone would be enough points).  Fewer than d + 1 points,
 *              anchor included: no path (FSCNN_PATH_TOO_FEW).  The system is solved by a QR
 *              factorisation (Givens rotations, rows in no particular order), never through the
 *              normal equations.  If a diagonal of the triangular factor is below npoints * 2^-52
 *              times the largest, the frame has no path (FSCNN_PATH_RANK_DEFICIENT); np.polyfit
 *              would return the truncated-SVD answer with a RankWarning there, which this law does
 *              not reproduce.
 *   waypoints  K values y_i = min_y + i * ((max_y - min_y) / (K - 1)), the last exactly max_y, y_0 =
 *              min_y when K = 1 (np.linspace); x_i by Horner from the highest coefficient, product
 *              and sum rounded separately (np.poly1d).  Path length = sum of the K - 1 segment
 *              lengths sqrt(dx*dx + dy*dy) (summed pairwise, not left to right).
 *   preview    among the waypoints with y_i < car_y, the one whose |sqrt((x_i - car_x)^2 +
 *              (y_i - car_y)^2) - preview_distance| is smallest, the first on ties; if none is
 *              ahead, the waypoint of smallest y, the first on ties (FSCNN_PATH_NONE_AHEAD).
 *              raw = control_x - car_x; with no path raw = 0.0 exactly and the control point is
 *              absent.
 *   EMA        with ema_state: e = raw and state = raw on a slot's first call (flag 0), afterwards
 *              e = state = ema_alpha * raw + (1 - ema_alpha) * state.  Without: e = raw.
 *   wheels     steering = steering_gain * e
 *              dynamic  = min(max(base_pwm / (1 + curvature_damping * |e|), min_pwm), max_pwm)
 *              left  = min(max(dynamic + steering, -1000), 1000)
 *              right = min(max(dynamic - steering, -1000), 1000)
 * Anchor and car position are both the reference's bottom-centre point: image pixel (320, 359, 1)
 * through view_params['image_to_world_matrix'] in float32 (_get_bottom_center_world_coord,
 * _get_car_position_world; the pixel is hard-coded there whatever the frame size).  The caller
 * computes it once on the host and passes it as doubles.
 *
 * out: double [N][FSCNN_PATH_REC + 2 * K] per frame, at the offsets below; then the K waypoints
 * (x_i, y_i).  Absent values (coefficients above d, and with no path every coefficient, the
 * control point and the waypoints) are NaN; with no path the length is 0 and FSCNN_PATH_NWAY is 0.
 * ema_state: DEVICE double [N][2] = (state, flag: 0 = not yet initialised), one batch slot per
 * camera stream, read and updated by the kernel; null = smoothing off.
 * Limits: K 1 .. 256, degree 1 .. 3, Hb 1 .. 65535, N 1 .. 65535, otherwise -2 and nothing is
 * launched.  Parameters that are not finite, pixels_per_unit == 0, skip_rows < 1 or min_width < 0:
 * -1. */
#define FSCNN_PATH_COEF 0        /* 4 slots: the d + 1 coefficients, highest power first */
#define FSCNN_PATH_NPOINTS 4     /* centreline points (the anchor not counted) */
#define FSCNN_PATH_STATUS 5      /* the bits below, as a double */
#define FSCNN_PATH_LENGTH 6
#define FSCNN_PATH_CONTROL_X 7
#define FSCNN_PATH_CONTROL_Y 8
#define FSCNN_PATH_RAW_ERROR 9   /* raw_lateral_error */
#define FSCNN_PATH_ERROR 10      /* lateral_error (after the EMA) */
#define FSCNN_PATH_STEERING 11   /* steering_adjustment */
#define FSCNN_PATH_DYNAMIC 12    /* dynamic_pwm */
#define FSCNN_PATH_PWM_LEFT 13
#define FSCNN_PATH_PWM_RIGHT 14
#define FSCNN_PATH_NWAY 15       /* number of waypoints: K, or 0 with no path */
#define FSCNN_PATH_REC 16
#define FSCNN_PATH_NO_CENTERLINE 1
#define FSCNN_PATH_TOO_FEW 2
#define FSCNN_PATH_RANK_DEFICIENT 4
#define FSCNN_PATH_NONE_AHEAD 8
typedef struct fscnn_path_params {
  int degree, num_waypoints;
  int fast, min_width, skip_rows, scan_from_bottom, force_bottom_center, reserved;
  double min_x, min_y, max_y, pixels_per_unit;  /* view_bounds, pixels_per_unit */
  double anchor_x, anchor_y, car_x, car_y;
  double steering_gain, base_pwm, curvature_damping, preview_distance, max_pwm, min_pwm;
  double ema_alpha;
} fscnn_path_params;
int fscnn_path_plan(const int* rows, int N, int Hb, const fscnn_path_params* p, double* ema_state,
                    double* out, void* stream);

/* SegmentationMetric counters (utils/metric.py:73-105, batch_pix_accuracy +
 * batch_intersection_union) of n predictions (pred_dtype 0 int64, 1 uint8) against int64 labels,
 * ACCUMULATED into counts[2 + 3*nclass] (int64): [correct, labeled, inter[C], area_pred[C],
 * area_lab[C]]; union = area_pred + area_lab - inter.  Exact integer counts. */
int fscnn_seg_metric(const void* pred, int pred_dtype, const long long* target, long long n,
                     int nclass, long long* counts, void* stream);

/* OHEM cross entropy (SoftmaxCrossEntropyOHEMLoss, utils/loss.py:127-176, the criterion of
 * train.py:190-191):
 * fscnn_ohem_prob: prob[i] = softmax probability of the label of pixel i (2.0 for ignored
 *   pixels); counts[0] += #labelled, counts[1] += #(prob <= thresh)  (device uint64 x 2).
 * fscnn_ohem_threshold: the whole threshold rule of utils/loss.py:159-170 on the device, from
 *   fscnn_ohem_prob's counters: *thr (device float) = inf when min_kept >= #labelled, else thresh,
 *   raised to the k-th smallest label probability (k = min(#labelled, min_kept)) when fewer than
 *   k labelled pixels have prob <= thresh.  work: 2056 uint32 device scratch.  No host sync
 *   (the reference's print of the label count on the first branch is not reproduced).
 * fscnn_ce_weighted_fwd / _bwd: nn.CrossEntropyLoss(weight, ignore_index) over the pixels with
 *   prob <= *thr (thr a device float; prob null: all labelled pixels; weight null: unweighted);
 *   out2 = (weighted mean loss, sum of weights); part as for fscnn_ce_fwd. */
int fscnn_ohem_prob(const void* logits, int dtype, const long long* target, int N, int C,
                    long long HW, long long ignore_index, float thresh, float* prob,
                    unsigned long long* counts, void* stream);
int fscnn_ohem_threshold(const float* prob, long long n, const unsigned long long* counts,
                         long long min_kept, float thresh, unsigned* work, float* thr, void* stream);
/* Deprecated (round 3): the host-driven k-th smallest of the OHEM rule was replaced by
 * fscnn_ohem_threshold, which keeps the threshold on the device.  Kept so old callers still link;
 * always returns -2 (unsupported) with a message naming the replacement. */
int fscnn_kth_smallest(const float* values, long long n, long long k, unsigned* hist, float* out,
                       void* stream);
int fscnn_ce_weighted_fwd(const void* logits, int dtype, const long long* target, int N, int C,
                          long long HW, long long ignore_index, const float* weight,
                          const float* prob, const float* thr, float* part, float* out2,
                          void* stream);
int fscnn_ce_weighted_bwd(const void* logits, int dtype, const long long* target, int N, int C,
                          long long HW, long long ignore_index, const float* weight,
                          const float* prob, const float* thr, const float* grad_out,
                          const float* out2, void* dlogits, void* stream);

/* Dice / Focal+Dice criteria (utils/loss.py:12-100; train.py:183-188, binary lane segmentation):
 * fscnn_dice_fwd writes stats[4] (device fp64) = (sum p1*t, sum p1, sum t, sum focal_i) with
 *   p1 = softmax(logits)[:, 1] (C > 1) or sigmoid (C == 1), t = float(target), focal_i =
 *   alpha (1 - pt)^gamma ce_i (only when focal != 0; C > 1); part: ce_parts(N, HW) * 4 floats.
 * fscnn_dice_bwd: d/dlogits of dice_weight * (1 - dice) + focal_weight * mean(focal), scaled by
 *   *grad_out (device). */
int fscnn_dice_fwd(const void* logits, int dtype, const long long* target, int N, int C,
                   long long HW, float alpha, float gamma, int focal, float* part, double* stats,
                   void* stream);
int fscnn_dice_bwd(const void* logits, int dtype, const long long* target, int N, int C,
                   long long HW, float alpha, float gamma, int focal, const double* stats,
                   const float* grad_out, float smooth, float dice_weight, float focal_weight,
                   void* dlogits, void* stream);

/* GPU input path.
 * fscnn_normalize_u8: transforms.ToTensor() + transforms.Normalize(mean, std) (train.py:104-107,
 *   eval.py:22-25, demo.py:37-40) of N uint8 HWC RGB images into the NCHW network input
 *   ((x / 255 - mean[c]) / std[c], torchvision's fp32 operation order); mean/std are HOST arrays
 *   of 3 floats; H*W must be a multiple of 4; out_dtype 0 fp32, 1 bf16.
 * fscnn_remap_labels: dataset label ids -> train ids through a device lookup table
 *   (data_loader/cityscapes.py:56-71 `_class_to_index` is lut = _key, offset = 1); ids outside
 *   the table become `invalid`. */
int fscnn_normalize_u8(const unsigned char* images, int N, int H, int W, const float* mean,
                       const float* std, void* out, int out_dtype, void* stream);
int fscnn_remap_labels(const unsigned char* labels, long long n, const long long* lut, int lut_size,
                       int offset, long long invalid, long long* out, void* stream);

/* GPU train / val augmentation (CitySegmentation._sync_transform / _val_sync_transform,
 * data_loader/cityscapes.py:93-150; the same code in tusimple.py): mirror, short-edge rescale
 * (PIL bilinear for the image, nearest for the mask), zero pad, crop, optional Gaussian blur,
 * ToTensor + Normalize and the label remap, one launch per batch, the same pixels as PIL.
 *
 * fscnn_sync_tables (host only, no GPU): PIL's resize tables of ONE axis of ONE sample for the
 *   `count` output positions start .. start+count-1 of a resize in_size -> out_size:
 *   bounds[count][2] = (first source index, taps), coef[count][kmax] = 22-bit fixed-point
 *   triangle-filter weights, nearest[count] = the mask's source index.  Positions >= out_size
 *   (the zero pad) get no taps and nearest -1.  *ksize = taps per position the resize needs
 *   (kmax must be >= it); with all three tables null the call only reports *ksize.
 *   in_size / out_size > 8 is E_INVALID.
 * fscnn_sync_blur_weights (host only): the two 24-bit weights of PIL's GaussianBlur(radius)
 *   box passes; radius must be in [0, 1) (all the reference draws), else E_INVALID.
 * fscnn_sync_transform: `blob` is N descriptors followed by their tables (int32; descriptor
 *   offsets count int32s from the blob's start), once in host memory (validated here: every
 *   table index is range-checked before the launch) and once, the same bytes, in device memory
 *   (what the kernel reads; the caller orders the copy before this call on `stream`).  Writes
 *   x [N,3,crop,crop] (out_dtype 0 fp32 / 1 bf16; (v/255 - mean[c])/std[c] as
 *   fscnn_normalize_u8), target [N,crop,crop] int64 = lut[id + lut_offset] (ids outside the
 *   table -> -1; pad -> id 0) and, unless null, crop_u8 [N,crop,crop,3].  lut is a device
 *   array, mean / std are host arrays of 3 floats. */
typedef struct fscnn_sync_desc {
  const unsigned char* image; /* device uint8 [H][W][3] */
  const unsigned char* mask;  /* device uint8 [H][W] */
  int H, W;
  int flip;                   /* read column W-1-x */
  int ow, oh, x1, y1;         /* resized size (before the pad) and the crop's origin */
  int blur;                   /* 0 / 1 */
  unsigned ww, fw;            /* fscnn_sync_blur_weights */
  int kx, ky;                 /* row stride of the coefficient tables */
  int off_xb, off_xk, off_yb, off_yk, off_nx, off_ny; /* bounds / coef / nearest, x and y axis */
} fscnn_sync_desc;
int fscnn_sync_tables(int in_size, int out_size, int start, int count, int kmax, int* bounds,
                      int* coef, int* nearest, int* ksize);
int fscnn_sync_blur_weights(float radius, unsigned* ww, unsigned* fw);
int fscnn_sync_transform(const void* host_blob, const void* device_blob, long long blob_bytes,
                         int N, int crop, const long long* lut, int lut_size, int lut_offset,
                         const float* mean, const float* std, void* x, int out_dtype,
                         long long* target, unsigned char* crop_u8, void* stream);

/* Fused training step head (train plans only): forward + bilinear upsample + CE(ignore_index)
 * evaluated at low resolution; loss2[0] = mean loss, loss2[1] = valid pixel count.  Computes
 * exactly criterion(model(x)[0], target) of train.py:270-271 without materialising the
 * full-resolution logits.  backward_loss then takes d(loss) (device scalar) instead of
 * d(logits). */
int fscnn_forward_loss(const fscnn_plan* plan, const void* x, int x_dtype, const long long* target,
                       long long ignore_index, float* loss2, const float* params, float* running,
                       long long* nbt, void* ws, unsigned long long dropout_seed, float dropout_p,
                       float momentum, void* stream);
int fscnn_backward_loss(const fscnn_plan* plan, const float* grad_loss, const float* loss2,
                        const void* x, int x_dtype, const float* params, float* grads, void* ws,
                        void* bws, unsigned long long dropout_seed, float dropout_p,
                        int stage_from, int stage_to, void* stream);

/* The same fused step head for the Dice / Focal+Dice criteria (utils/loss.py:12-100, the default
 * --loss-type of train.py:70): loss = dice_weight * (1 - (2 I + smooth) / (S + T + smooth)) +
 * focal_weight * F / (N H W) with, over the full-resolution pixels of the upsampled logits,
 * I = sum p1 t, S = sum p1, T = sum t, F = sum alpha (1 - pt)^gamma ce (p1 = softmax[:, 1],
 * t = float(target); targets outside [0, num_classes) count as 0; F only when focal_weight != 0).
 * DiceLoss / MixDiceLoss: dice_weight 1, focal_weight 0; FocalDiceLoss: dice_weight and
 * 1 - dice_weight.  loss_out (float[1]) and stats (double[4] = I, S, T, F) are device outputs;
 * nothing is read back by the host.  head_ws (fscnn_dice_head_ws_bytes, 256-B aligned) keeps
 * the low-resolution coefficient planes until fscnn_backward_loss_dice, which takes d(loss)
 * (device scalar) and the forward's stats and scalars.  num_classes 2 .. 32; an aux net
 * returns -2.  fscnn_dice_head_ws_bytes is negative (fscnn_last_error set) unless the plan
 * is a train = 1 plan; the plan's own workspace sizes do not include it. */
long long fscnn_dice_head_ws_bytes(const fscnn_plan* plan);
int fscnn_forward_loss_dice(const fscnn_plan* plan, const void* x, int x_dtype,
                            const long long* target, float smooth, float dice_weight,
                            float focal_weight, float alpha, float gamma, float* loss_out,
                            double* stats, const float* params, float* running, long long* nbt,
                            void* ws, void* head_ws, unsigned long long dropout_seed,
                            float dropout_p, float momentum, void* stream);
int fscnn_backward_loss_dice(const fscnn_plan* plan, const float* grad_loss, const double* stats,
                             float smooth, float dice_weight, float focal_weight, const void* x,
                             int x_dtype, const float* params, float* grads, void* ws, void* bws,
                             void* head_ws, unsigned long long dropout_seed, float dropout_p,
                             int stage_from, int stage_to, void* stream);

/* The same fused step head for the OHEM criterion (SoftmaxCrossEntropyOHEMLoss /
 * MixSoftmaxCrossEntropyOHEMLoss, utils/loss.py:127-206, what train.py:189-191 builds):
 * nn.CrossEntropyLoss(weight, ignore_index) over the kept pixels of the upsampled logits, a pixel
 * being kept when it is labelled and the softmax probability of its label is <= the threshold
 * of fscnn_ohem_threshold (inf, thresh, or the min_kept-th smallest label probability).  One
 * pass over the low-resolution logits writes prob[N*H*W] (fp32; 2.0 for ignored or out-of-range
 * targets, as fscnn_ohem_prob) and the two counters, and forms loss and gradient for the
 * threshold `thresh`; the threshold rule runs on the plane; a second pass, which returns at once
 * when *thr is bit-equal to thresh, redoes loss and gradient over prob[i] <= *thr.
 * loss2[0] = weighted mean loss over the kept pixels (NaN when none), loss2[1] = the sum of their
 * class weights (their count when weight is null): the CE head's format, so the backward is
 * fscnn_backward_loss / fscnn_backward_dx with this loss2.  weight: device float[num_classes] or
 * null.  prob, thr (float[1]), counts (uint64[2], zeroed by the call) and work (2056 uint32) are
 * caller-owned device buffers with the sizes of fscnn_ohem_prob / fscnn_ohem_threshold; nothing
 * is read back by the host.  num_classes 1 .. 32; more classes or an aux net return -2 before
 * anything is launched. */
int fscnn_forward_loss_ohem(const fscnn_plan* plan, const void* x, int x_dtype,
                            const long long* target, long long ignore_index, float thresh,
                            long long min_kept, const float* weight, float* loss2, float* prob,
                            float* thr, unsigned long long* counts, unsigned* work,
                            const float* params, float* running, long long* nbt, void* ws,
                            unsigned long long dropout_seed, float dropout_p, float momentum,
                            void* stream);

/* The fused step heads for an aux net (FastSCNN(aux=True), what train.py builds with --aux):
 * loss = L(out) + aux_weight * L(aux_out), the criteria of utils/loss.py:42-68 (MixDiceLoss),
 * :103-124 (MixSoftmaxCrossEntropyLoss) and :179-206 (MixSoftmaxCrossEntropyOHEMLoss), where L is
 * the single-output law of the heads above on each bilinearly upsampled output.  The head kernels
 * run once on the main and once on the aux low-resolution logits (the aux head stops there: no
 * full-resolution logits or gradient of either output exists); the OHEM head keeps a probability
 * plane, threshold and kept set per output, as the reference calls its single-output law once per
 * prediction.  loss_out (device float[3]) = (main + aux_weight * aux, main, aux), the last two
 * unweighted; only an output: the backward never reads it, so the caller may scale it in place.
 *
 * fscnn_aux_head: head 0 CE (ignore_index), 1 Dice (smooth and dice_weight as
 * fscnn_forward_loss_dice; plain Dice only, MixDiceLoss: focal_weight must be 0 -- the reference
 * has no two-output Focal+Dice criterion -- and alpha / gamma are then unused; a non-zero
 * focal_weight returns -2), 2 OHEM (ignore_index, thresh, min_kept, class_weight: device
 * float[num_classes] or null, as fscnn_forward_loss_ohem); the fields of the other heads are
 * ignored.  Pass the same values to the backward.
 *
 * head_ws (fscnn_aux_head_ws_bytes(plan, head) bytes, 256-B aligned, layout internal) is the one
 * caller buffer that survives from the forward to the backward: the aux head's gradient planes,
 * both heads' (mean, count) pairs / Dice sums and coefficient planes / OHEM planes, thresholds,
 * counters (zeroed inside the run) and select scratch; the plan's own workspace sizes do not
 * include it.  fscnn_aux_head_ws_bytes is negative (fscnn_last_error set) unless the plan is a
 * train = 1 plan of an aux net and head is 0 .. 2.
 *
 * fscnn_backward_loss_aux takes d(loss) (device scalar); stage 0 scales the main head's gradient
 * as fscnn_backward_loss does and the aux head's, times aux_weight, straight into the aux layer's
 * low-resolution entry point (no upsample backward).  dx: the input gradient [N][3][H][W] in
 * dx_dtype, or null (the Dice head does not form it: -1).  Null required pointers or inconsistent
 * arguments return -1, more than 32 classes (Dice: fewer than 2) -2, both before anything is
 * launched. */
typedef struct fscnn_aux_head {
  int head;                       /* 0 CE, 1 Dice, 2 OHEM */
  float aux_weight;
  long long ignore_index;         /* CE, OHEM */
  float smooth, dice_weight, focal_weight, alpha, gamma; /* Dice (focal_weight 0) */
  float thresh;                   /* OHEM */
  long long min_kept;
  const float* class_weight;
} fscnn_aux_head;
long long fscnn_aux_head_ws_bytes(const fscnn_plan* plan, int head);
/* Debugging / parity, like fscnn_plan_buffer: byte offset in head_ws of head `which`'s (0 main,
 * 1 aux) state `field` -- "pair" (float[2]: mean, count; Dice: float[1], the term), "stats"
 * (Dice: double[4]), "prob" (OHEM: float[N*H*W]), "thr" (float[1]), "counts" (uint64[2]) -- or
 * negative. */
long long fscnn_aux_head_ws_offset(const fscnn_plan* plan, int head, const char* field, int which);
int fscnn_forward_loss_aux(const fscnn_plan* plan, const void* x, int x_dtype,
                           const long long* target, const fscnn_aux_head* h, float* loss_out,
                           const float* params, float* running, long long* nbt, void* ws,
                           void* head_ws, unsigned long long dropout_seed, float dropout_p,
                           float momentum, void* stream);
int fscnn_backward_loss_aux(const fscnn_plan* plan, const float* grad_loss,
                            const fscnn_aux_head* h, const void* x, int x_dtype, void* dx,
                            int dx_dtype, const float* params, float* grads, void* ws, void* bws,
                            void* head_ws, unsigned long long dropout_seed, float dropout_p,
                            int stage_from, int stage_to, void* stream);

/* ---- fused blocks (inference) ---------------------------------------------------------------
 * fscnn_block_ir_fwd: one stride-1 LinearBottleneck (models/fast_scnn.py:95-115) with its three
 * BatchNorms folded (eval): y = BN_p(W_p * relu(BN_d(dw3x3(relu(BN_e(W_e * x)))))) (+ x when
 * residual, which needs cin == cout).  x, y NHWC [N][H][W] with row strides ldx / ldy elements
 * (ldy may exceed cout: the PPM concat buffer); w_expand [expand][cin] and w_project
 * [cout][expand] in dtype (the nn.Conv2d weight layouts); w_dw [expand][9] fp32; scale_* / shift_*
 * fp32 per channel (BN folded as gamma/sqrt(var+eps), beta - mean*scale).  cin in {64, 96, 128},
 * expand a multiple of 64, cout a multiple of 16 <= 128.  The 6x-expanded tensor stays in LDS.
 * Replaces the three conv+BN(+ReLU) modules of LinearBottleneck.block (:103-108) and the
 * shortcut add (:113-114). */
int fscnn_block_ir_fwd(const void* x, int ldx, int dtype, int N, int H, int W, int cin, int expand,
                       int cout, const void* w_expand, const float* w_dw, const void* w_project,
                       const float* scale_e, const float* shift_e, const float* scale_d,
                       const float* shift_d, const float* scale_p, const float* shift_p,
                       int residual, void* y, int ldy, void* stream);

/* fscnn_block_ir_s2_fwd: the stride-2 LinearBottleneck (models/fast_scnn.py:95-115 with
 * stride 2: bottleneck1.0 and bottleneck2.0, no shortcut) in one inference launch:
 * y = BN_p(W_p * relu(BN_d(dw3x3_s2_p1(relu(BN_e(W_e * x)))))), every BN folded.  x NHWC
 * [N][H][W] x cin (row stride ldx), y NHWC [N][(H-1)/2+1][(W-1)/2+1] x cout (row stride ldy);
 * weights and BN tables as fscnn_block_ir_fwd.  The expanded tensor never reaches memory; the
 * executor uses it for the two stride-2 blocks of every eval plan with >= 128 output tiles. */
int fscnn_block_ir_s2_fwd(const void* x, int ldx, int dtype, int N, int H, int W, int cin,
                          int expand, int cout, const void* w_expand, const float* w_dw,
                          const void* w_project, const float* scale_e, const float* shift_e,
                          const float* scale_d, const float* shift_d, const float* scale_p,
                          const float* shift_p, void* y, int ldy, void* stream);

/* fscnn_block_ltd_fwd: the inference LearningToDownsample stem up to dsconv1 in one launch
 * (models/fast_scnn.py:153-154): y = BN_p(W_p * relu(BN_d(dw3x3_s2_p1(relu(BN_0(conv3x3_s2_p0(x)))))))
 * followed by ReLU, every BN folded (scale, shift fp32 per channel).  x NCHW [N][3][H][W] of
 * x_dtype (0 fp32, 1 bf16, 2 fp16; 16-B aligned, W a multiple of 16 B / element size); w_conv
 * [32][3][3][3] fp32, w_dw [32][9] fp32, w_pw [48][32] in dtype (the plan's storage type);
 * y NHWC [N][H2][W2] x 48 channels with row stride ldy elements (>= 48, multiple of 4), where
 * H1 = (H-3)/2+1, H2 = (H1-1)/2+1 (same for W).  conv0's and the depthwise output never reach
 * memory.  Replaces LearningToDownsample.conv (_ConvBNReLU, :52) and .dsconv1 (_DSConv, :64-78);
 * the executor uses it for every eval plan whose image fits these constraints. */
int fscnn_block_ltd_fwd(const void* x, int x_dtype, int dtype, int N, int H, int W,
                        const float* w_conv, const float* scale_0, const float* shift_0,
                        const float* w_dw, const float* scale_d, const float* shift_d,
                        const void* w_pw, const float* scale_p, const float* shift_p, void* y,
                        int ldy, void* stream);

/* fscnn_block_dsconv_fwd: an inference _DSConv (models/fast_scnn.py:64-79; the Classifer's
 * dsconv1 / dsconv2, :228-231) in one launch: y = relu(BN_p(W_p * relu(BN_d(dw3x3_s1_p1(x))))),
 * every BN folded (scale, shift fp32 per channel).  x NHWC [N][H][W] x C in dtype (rows of C
 * contiguous elements, 16-B aligned); w_dw [C][9] fp32, w_pw [Co][C] in dtype; y NHWC with row
 * stride ldy elements (>= Co, multiple of 4, 16-B aligned).  C = Co = 128 (E_UNSUPPORTED
 * otherwise).  The depthwise output never reaches memory.  Replaces _DSConv's dw conv + BN + ReLU
 * and pw conv + BN + ReLU (two launches of the unfused eval path); the executor uses it for the
 * classifier's two DSConvs of every eval plan. */
int fscnn_block_dsconv_fwd(const void* x, int dtype, int N, int H, int W, int C, int Co,
                           const float* w_dw, const float* scale_d, const float* shift_d,
                           const void* w_pw, const float* scale_p, const float* shift_p, void* y,
                           int ldy, void* stream);

/* fscnn_block_dsconv_res_fwd: the same with a residual added after the pointwise BN, before the
 * final ReLU: y = relu(BN_p(W_p * relu(BN_d(dw3x3(up(x))))) + res) -- the FeatureFusionModule's
 * F.interpolate(scale 4, bilinear, align_corners) + dwconv + conv_lower_res + the high-res branch
 * (models/fast_scnn.py:207-218).  Hi > 0: x is [N][Hi][Wi] x C and up() its bilinear
 * align_corners resize to H x W, formed in LDS and never stored (same arithmetic as the unfused
 * up_nhwc); Hi = 0: up() is the identity and x is [N][H][W] x C.  res NHWC with row stride ldres
 * (>= Co, multiple of 4, 16-B aligned); res may alias y (each element is read before it is
 * written, by the same thread). */
int fscnn_block_dsconv_res_fwd(const void* x, int dtype, int N, int H, int W, int C, int Co,
                               int Hi, int Wi, const float* w_dw, const float* scale_d, const float* shift_d,
                               const void* w_pw, const float* scale_p, const float* shift_p,
                               const void* res, int ldres, void* y, int ldy, void* stream);

/* fscnn_block_cls_fwd: the inference Classifer (models/fast_scnn.py:221-237; Dropout is the
 * identity in eval) in two launches: tmp = dsconv1(x) (fscnn_block_dsconv_fwd), then dsconv2 and
 * the 1x1 classifier conv (+ bias) in one launch whose 128-channel dsconv2 output never reaches
 * memory: logits = W_cls * dsconv2(tmp) + b_cls.  x and tmp NHWC [N][H][W] x 128 in dtype
 * (16-B aligned); w_dw* [128][9] fp32, w_pw* [128][128] and w_cls [ncls][128] in dtype, b_cls
 * [ncls] fp32, every BN folded to (scale, shift) fp32; logits NHWC [N][H][W] x ncls with row
 * stride ldl (>= ncls; ncls <= 32), only the first ncls columns written.  Replaces the
 * Classifer's dw / pw / dw / pw / conv launches of the unfused eval path; bit-identical to them. */
int fscnn_block_cls_fwd(const void* x, int dtype, int N, int H, int W, const float* w_dw1,
                        const float* scale_d1, const float* shift_d1, const void* w_pw1,
                        const float* scale_p1, const float* shift_p1, const float* w_dw2,
                        const float* scale_d2, const float* shift_d2, const void* w_pw2,
                        const float* scale_p2, const float* shift_p2, const void* w_cls,
                        const float* b_cls, int ncls, void* tmp, void* logits, int ldl,
                        void* stream);

/* fscnn_block_ffm_fwd: the inference FeatureFusionModule (models/fast_scnn.py:200-218) in one
 * launch: y = relu(BN_l(W_l * relu(BN_d(dw3x3(up(low))))) + BN_h(W_h * high)).  low NHWC
 * [N][Hi][Wi] x 128 (the global feature extractor's output; up() its bilinear align_corners resize
 * to H x W, formed in LDS); high NHWC [N][H][W] x 64 with row stride ldhigh (>= 64, multiple of
 * 8, 16-B aligned; LearningToDownsample's output); w_dw [128][9] fp32, w_low [128][128] and
 * w_high [128][64] in dtype; every BN folded to (scale, shift) fp32.  Neither the upsampled
 * input, the depthwise output nor the high-res branch's output reaches memory.  Replaces
 * F.interpolate + dwconv + conv_lower_res + conv_higher_res + add + ReLU (four launches of the
 * unfused eval path); the executor uses it for the FFM of every eval plan (FSCNN_FFM_HI=0 keeps
 * the high-res branch as its own GEMM and fscnn_block_dsconv_res_fwd), bit-identical to them. */
int fscnn_block_ffm_fwd(const void* low, int dtype, int N, int Hi, int Wi, int H, int W,
                        const void* high, int ldhigh, const float* w_dw, const float* scale_d,
                        const float* shift_d, const void* w_low, const float* scale_l,
                        const float* shift_l, const void* w_high, const float* scale_h,
                        const float* shift_h, void* y, int ldy, void* stream);

/* ---- launch profiler (bench.py roofline, tools/layer_report.py) ----------------------------
 * kind: 1 conv0_fwd, 2 dw_fwd, 3 dw_dgrad, 4 dw_wgrad, 5 gemm_nt, 6 gemm_tn, 7 bn_apply,
 * 8 bn_bwd (apply), 9 upsample, 10 upsample_bwd, 11 cross_entropy / fused loss head,
 * 12 conv0_wgrad, 13 bn_bwd_reduce, 14 bn_finalize, 15 ppm_branches (the four pyramid-pooling
 * branch convs + BN + ReLU, one launch each way), 16 ir_block (fused inference bottleneck),
 * 17 ltd_stem (fused inference stem), 18 dsconv (fused inference DSConv);
 * 100 = every kind.
 * Between begin and end every launch of that kernel family is bracketed by hipEvents bound to its
 * dispatch (hipExtLaunchKernelGGL); end synchronises and returns summed kernel ms,
 * launch count and the algorithmic bytes
 * and flops of those launches (SURVEY.md §8(d) formulas); fscnn_prof_launch then returns launch
 * i's kind, ms, bytes, flops and layer (reference module name; issue order). */
int fscnn_prof_begin(int kind, int max_launches);
int fscnn_prof_end(double* total_ms, long long* launches, double* bytes, double* flops);
int fscnn_prof_launch(long long i, int* kind, float* ms, double* bytes, double* flops,
                      const char** layer);
const char* fscnn_prof_kind_name(int kind);
/* Debug: phase stamps of the next launches of the instrumented kernels (pointwise GEMMs, depthwise
 * forward / stride-1 dgrad): per-wave 100 MHz wall clock at fixed points of the kernel
 * (tools/stamp_probe.py).  Launch i writes buf + i * 262144 uint64 (8192 workgroups x 4 waves x
 * 8 slots), up to max_launches; null: off.  fscnn_debug_stamp_count / _tag: launches recorded and
 * each one's layer label.  Process-global, single-threaded measurement only. */
int fscnn_debug_stamps(void* buf, int max_launches);
int fscnn_debug_stamp_count(void);
const char* fscnn_debug_stamp_tag(int i);

/* ---- loss / optimizer ------------------------------------------------------------------- */
/* out2[0] = mean loss over valid pixels, out2[1] = valid count; part: ce_parts*2 floats */
long long fscnn_ce_parts(int N, long long HW);
int fscnn_ce_fwd(const void* logits, int dtype, const long long* target, int N, int C,
                 long long HW, long long ignore_index, float* part, float* out2, void* stream);
int fscnn_ce_bwd(const void* logits, int dtype, const long long* target, int N, int C,
                 long long HW, long long ignore_index, const float* grad_out,
                 const float* out2, void* dlogits, void* stream);
int fscnn_sgd(float* p, const float* g, float* buf, long long n, float lr, float momentum,
              float dampening, float weight_decay, int nesterov, int first, float grad_scale,
              void* stream);

/* torch.optim.AdamW.step (train_bdd100k.py:183-188, 258-266) in fp32, element by element:
 *   g = grad (negated if maximize; divided by *grad_scale if given);  p *= 1 - lr * weight_decay;
 *   m += (g - m) * (1 - beta1);  v = beta2 * v + (1 - beta2) * g * g;
 *   amsgrad: vmax = max(vmax, v), used in place of v;
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps),  t = step + 1.
 * The step count is a device fp32 scalar.  grad_scale / found_inf are device fp32 scalars or
 * null (what torch.amp.GradScaler hands an optimizer): when *found_inf != 0 the call changes
 * nothing, the step included; otherwise the step advances by one, in a one-thread launch behind
 * the update when `tick` is set (clear it on all but the last call that shares a step).
 * max_exp_avg_sq may be null unless amsgrad.
 *
 * fscnn_adamw: one span of n >= 0 elements, any 4-byte alignment. */
int fscnn_adamw(float* p, const float* g, float* exp_avg, float* exp_avg_sq,
                float* max_exp_avg_sq, long long n, double lr, double beta1, double beta2,
                double eps, double weight_decay, int amsgrad, int maximize, float* step, int tick,
                const float* grad_scale, const float* found_inf, void* stream);
/* fscnn_adamw_segments: one launch over every run of every parameter group of 16-byte aligned
 * arenas that share their offsets.  segs (device; host_segs: the same table in host memory, checked
 * when not null): nseg segments [begin, end) in elements, fewer than 2^31 each, begin a multiple
 * of 16, each with its index into `groups` and chunk0, the sum of
 * ceil((end - begin) / FSCNN_ADAMW_CHUNK) over the segments before it.  chunk_seg (device): for
 * each of the nchunks chunks its segment.  Elements
 * outside every segment are neither read nor written.  groups: up to FSCNN_ADAMW_MAX_GROUPS, read
 * from host memory at the call (nothing to upload when lr changes); step_slot indexes `steps`
 * (nslots device floats), all of which advance when `tick` is set. */
#define FSCNN_ADAMW_CHUNK 2048
#define FSCNN_ADAMW_MAX_GROUPS 8
typedef struct fscnn_adamw_seg {
  long long begin, end;
  int group;
  int chunk0;
} fscnn_adamw_seg;
typedef struct fscnn_adamw_group {
  double lr, beta1, beta2, eps, weight_decay;
  int amsgrad, maximize;
  int step_slot;
} fscnn_adamw_group;
int fscnn_adamw_segments(float* p, const float* g, float* exp_avg, float* exp_avg_sq,
                         float* max_exp_avg_sq, const fscnn_adamw_seg* segs,
                         const fscnn_adamw_seg* host_segs, int nseg, const int* chunk_seg,
                         int nchunks, const fscnn_adamw_group* groups, int ngroups, float* steps,
                         int nslots, int tick, const float* grad_scale, const float* found_inf,
                         void* stream);

/* ---- individual kernels (per-op parity tests) ------------------------- */
int fscnn_conv0_fwd(const void* x, int x_dtype, int N, int H, int W, const float* w,
                    const float* scale, const float* shift, int relu, void* y, int y_dtype,
                    void* stream);
/* dW [32][3][3][3] of the first conv from the NCHW image and NHWC dZ [N][Ho][Wo][32]
 * (autograd of models/fast_scnn.py:153); slab: fscnn_conv0_wgrad_slab_floats floats */
long long fscnn_conv0_wgrad_slab_floats(int N, int H, int W);
int fscnn_conv0_wgrad(const void* x, int x_dtype, int N, int H, int W, const void* dz,
                      int dz_dtype, float* slab, float* dw, void* stream);
int fscnn_dw3x3_fwd(const void* x, int dtype, int N, int H, int W, int C, int stride,
                    const float* w, const float* scale, const float* shift, int relu, void* y,
                    void* stream);
int fscnn_dw3x3_dgrad(const void* dy, int dtype, int N, int H, int W, int C, int stride,
                      const float* w, void* dx, void* stream);
long long fscnn_dw3x3_wgrad_slab_floats(int N, int H, int W, int C, int stride, int dtype);
int fscnn_dw3x3_wgrad(const void* x, const void* dy, int dtype, int N, int H, int W, int C,
                      int stride, float* slab, float* dw, void* stream);
/* C[M][N] = act((A[M][K] . B^T) * scale + shift (+ R)); B is [N][K] (b_trans=0) or [K][N].
 * stats_part (train BN statistics of the output, before R / relu): room for ceil(M/128)
 * records [P][3][N]; the call writes fscnn_pw_gemm_stats_parts(...) of them (pass that count as
 * P to fscnn_bn_finalize). */
int fscnn_pw_gemm_stats_parts(int M, int N, int K, int lda, int ldc, int dtype);
int fscnn_pw_gemm(int M, int N, int K, const void* A, int lda, const void* B, int ldb,
                  int b_trans, const float* scale, const float* shift, const void* R, int ldr,
                  int relu, void* C, int ldc, float* stats_part, int dtype, void* stream);
/* Training dgrad of a 1x1 conv whose output is the dy of a BatchNorm (the form the executor runs
 * for every LinearBottleneck expand dgrad, models/fast_scnn.py:103-104 autograd):
 *   dX[M][N] = D[M][K] . B^T (+ R), B [N][K] (the transposed conv weight, row stride ldb),
 * plus that BN's backward reduction over the STORED (rounded) dX, finished in the same call:
 *   dbeta[n] = sum_m dX*mask, dgamma[n] = sum_m dX*mask*(z - mean[n])*invstd[n],
 *   coef[n] = dbeta[n] / M, coef[N + n] = dgamma[n] / M,
 * mask = 1 (relu_mode 0) or (z*scale[n] + shift[n] > 0) (relu_mode 2: the BN feeds a ReLU).
 * z [M][N] (ld ldz) is the BN's forward input.  Scratch: part >= ceil(M/128)*2*N floats,
 * counters 512 zeroed uint32 (left zero), tsum 32*3*1024 doubles.  *path (nullable): 1 when the
 * streaming kernel ran (deep-K form for 16-bit K = 384 / 512 / 576 at M >= 131072), 0 tiled. */
int fscnn_pw_dgrad_bnbwd(int M, int N, int K, const void* D, int ldd, const void* B, int ldb,
                         const void* R, int ldr, void* dX, int lddx, const void* z, int ldz,
                         const float* mean, const float* invstd, const float* scale,
                         const float* shift, int relu_mode, float* part, unsigned* counters,
                         double* tsum, float* dgamma, float* dbeta, float* coef, int dtype,
                         int* path, void* stream);
long long fscnn_pw_wgrad_slab_floats(int M, int N, int K);
/* dW[N][K] = sum_m D[m][n] X[m][k] */
int fscnn_pw_wgrad(int M, int N, int K, const void* D, int ldd, const void* X, int ldx,
                   float* slab, float* dW, int dtype, void* stream);
/* part [P][3][C] is consumed (folded in place) */
int fscnn_bn_finalize(float* part, int P, int C, const float* gamma, const float* beta,
                      float* rmean, float* rvar, long long* nbt, float momentum, float* mean,
                      float* invstd, float* scale, float* shift, void* stream);
int fscnn_bilinear_ac_fwd(const void* x, int dtype, int N, int Hi, int Wi, int C, int Ho, int Wo,
                          void* y, int out_nchw, int out_dtype, void* stream);
/* NHWC grad wrt output [N][Ho][Wo][C] -> NHWC grad wrt input [N][Hi][Wi][C] (fp32 tmp) */
int fscnn_bilinear_ac_bwd(const void* dy, int dtype, int N, int Hi, int Wi, int C, int Ho, int Wo,
                          float* tmp, void* dx, void* stream);
int fscnn_pyramid_pool_fwd(const void* x, int dtype, int N, int H, int W, int C, int ldx,
                           void* pooled, void* stream);
int fscnn_pyramid_pool_bwd(const void* dpooled, int dtype, int N, int H, int W, int C, void* dx,
                           int lddx, int accumulate, void* stream);

/* ---- kernels that only a train step runs, in the executor's form (tests/test_gpu_train_kernels.py).
 * Every call refuses null or inconsistent arguments with a non-zero code before anything is
 * launched.  V below is the 16-byte vector width: 4 elements (fp32) or 8 (bf16 / fp16); C and
 * every row stride must be a multiple of it. */
/* y[M][C] (ldy) = act(z*scale + shift [+ z2*scale2 + shift2] [+ res]), act = ReLU when relu;
 * z2 (the FFM's second branch) and res (a shortcut) are optional. */
int fscnn_bn_apply(long long M, int C, const void* z, int ldz, const float* scale,
                   const float* shift, const void* z2, int ldz2, const float* scale2,
                   const float* shift2, const void* res, int ldres, int relu, void* y, int ldy,
                   int dtype, void* stream);
/* BatchNorm backward of dy[M][C] (lddy) through a BN with input z[M][C] (contiguous): the reduce,
 * finish and apply launches in the executor's order.
 *   dy_r = dy * mask;  relu_mode 0: no mask, 1: mask[M][C] (ldmask) > 0 (the saved ReLU output),
 *   2: z*scale + shift > 0 recomputed (mask null);
 *   dbeta = sum dy_r, dgamma = sum dy_r*xhat, xhat = (z - mean)*invstd;
 *   coef[0..C) = dbeta / M, coef[C..2C) = dgamma / M;  dz[M][C] = scale*(dy_r - coef0 - xhat*coef1).
 * frozen 1: a BN normalised with running statistics (the coefficients are zero, dz = scale*dy_r),
 * as eval-mode autograd runs it; frozen 2: the same with the apply kernel's own no-coefficient
 * form.  z2 (optional, relu_mode 1 only, C <= 512): a second BN on the same dy and mask (the
 * FFM), with mean2 / invstd2 / scale2, outputs dz2 / dgamma2 / dbeta2 and coef[2C..4C).
 * Scratch: part >= 2048*2*C floats (twice that when paired), counters 512 zeroed uint32 (left
 * zero).  *P / *rows_per_block (nullable): the reduce's record count and rows per record. */
int fscnn_bn_bwd(long long M, int C, const void* dy, int lddy, const void* mask, int ldmask,
                 const void* z, const float* mean, const float* invstd, const float* scale,
                 const float* shift, int relu_mode, int frozen, const void* z2,
                 const float* mean2, const float* invstd2, const float* scale2, float* part,
                 unsigned* counters, void* dz, void* dz2, float* dgamma, float* dbeta,
                 float* dgamma2, float* dbeta2, float* coef, int dtype, int* P,
                 int* rows_per_block, void* stream);
/* The PyramidPooling branch convs (1x1, K -> 32) + BN + ReLU of a train step, one launch each
 * way.  nb <= 4 branches of M[i] <= 512 rows (host array), packed branch after branch: x [sum M][K],
 * w [nb][32][K] (storage type), z [sum M][32], y [sum M][ldy]; gamma .. shift, dgamma, dbeta are
 * [nb][32], nbt [nb] (nullable), dw [nb][32][K] fp32, dx [sum M][K].  The forward writes the
 * batch statistics tables and updates the running ones; the backward recomputes the batch
 * statistics in fp64 from z and takes the ReLU mask from y > 0.  fscnn_ppm_branches_ok: whether
 * the launch takes branches of up to maxM rows (else both calls return an error). */
int fscnn_ppm_branches_ok(int maxM, int K, int dtype);
int fscnn_ppm_branches_fwd(int nb, const int* M, int K, const void* x, const void* w,
                           const float* gamma, const float* beta, float* rmean, float* rvar,
                           long long* nbt, float momentum, void* z, void* y, int ldy, float* mean,
                           float* invstd, float* scale, float* shift, int dtype, void* stream);
int fscnn_ppm_branches_bwd(int nb, const int* M, int K, const void* dy, int lddy, const void* y,
                           int ldy, const void* z, const float* mean, const float* invstd,
                           const float* scale, const float* gamma, const void* x, const void* w,
                           float* dgamma, float* dbeta, float* dw, void* dx, int dtype,
                           void* stream);
/* Bilinear (align_corners) upsample of the four PPM levels, feats bin-major [50][N][32], into
 * channels [coff, coff + 128) of the NHWC concat tensor y [N][H][W][ldy], and its backward from
 * the same slice of dy (H <= 80) to dfeats [50][N][32]. */
int fscnn_ppm_up_fwd(const void* feats, int dtype, int N, int H, int W, void* y, int ldy, int coff,
                     void* stream);
int fscnn_ppm_up_bwd(const void* dy, int dtype, int N, int H, int W, int ldy, int coff,
                     void* dfeats, void* stream);
/* Dropout of an NHWC tensor x [N][H][W] x C (ldx): y = keep ? v / (1 - p) : 0, the keep mask a
 * hash of (seed + seed_add, NCHW index); the seed by value, or read from the device slot
 * seed_slot when not null.  x_scale / x_shift (optional, together): x is a raw conv output and
 * v = relu(x*x_scale + x_shift) rounded to the storage type (bn_apply's output). */
int fscnn_dropout(const void* x, int ldx, int dtype, int N, int H, int W, int C,
                  unsigned long long seed, const unsigned long long* seed_slot,
                  unsigned long long seed_add, float p, const float* x_scale,
                  const float* x_shift, void* y, int ldy, void* stream);
/* Train forms of the depthwise 3x3 conv (pad 1, stride 1 or 2, x NHWC [N][H][W][C]).
 * fscnn_dw3x3_parts: BN records of the forward (dgrad 0) or of the dgrad (dgrad 1); -1 on bad
 * arguments.
 * fwd_train: z = conv(v), v = x or relu(x*in_scale + in_shift) (in_scale / in_shift together or
 * null; padding stays zero), plus the batch statistics of the stored z finished to mean / invstd /
 * scale / shift and the running statistics (nbt nullable).  part: parts*3*C floats.
 * dgrad_bn: dx = the conv's input gradient, plus the BN backward sums of the stored dx for the
 * BatchNorm whose output v was (its input z [N][H][W][C]; relu_mode 0 or 2 as in fscnn_bn_bwd)
 * finished to dgamma / dbeta / coef [2][C].  part: parts*2*C floats; w 16-byte aligned.
 * Both: counters 512 zeroed uint32 (left zero), tsum 32*3*1024 doubles; *in_kernel (nullable): 1
 * when the kernel's last workgroups ran the finish, 0 when it was a launch of its own. */
int fscnn_dw3x3_parts(int N, int H, int W, int C, int stride, int dtype, int dgrad);
/* Which depthwise tile kernels this shape's launches take (forward, weight gradient, stride-1
 * input gradient): the compile-time channel-chunk width 4, 6 or 8, or 0 for the run-time-width,
 * bounds-checked kernels (any other C, spans past 32 bits, FSCNN_DW_GENERIC=1); -1 on bad
 * arguments.  Both give the same bits (tests/test_gpu_dw_paths.py). */
int fscnn_dw3x3_ct_width(int N, int H, int W, int C, int stride, int dtype);
int fscnn_dw3x3_fwd_train(const void* x, int dtype, int N, int H, int W, int C, int stride,
                          const float* w, const float* in_scale, const float* in_shift, void* z,
                          float* part, unsigned* counters, double* tsum, const float* gamma,
                          const float* beta, float* rmean, float* rvar, long long* nbt,
                          float momentum, float* mean, float* invstd, float* scale, float* shift,
                          int* in_kernel, void* stream);
int fscnn_dw3x3_dgrad_bn(const void* dy, int dtype, int N, int H, int W, int C, int stride,
                         const float* w, void* dx, const void* z, const float* mean,
                         const float* invstd, const float* scale, const float* shift,
                         int relu_mode, float* part, unsigned* counters, double* tsum,
                         float* dgamma, float* dbeta, float* coef, int* in_kernel, void* stream);
/* fscnn_dw3x3_wgrad over a lazy input: x is a raw conv output and the operand is
 * relu(x*x_scale + x_shift) rounded to the storage type (x_scale / x_shift together, or both null:
 * x itself); padding stays zero.  slab: fscnn_dw3x3_wgrad_slab_floats floats; dw [C][3][3]. */
int fscnn_dw3x3_wgrad_train(const void* x, const void* dy, int dtype, int N, int H, int W, int C,
                            int stride, const float* x_scale, const float* x_shift, float* slab,
                            float* dw, void* stream);

/* ---- the pointwise (1x1) conv of a train step, in the executor's three GEMM forms
 * (tests/test_gpu_train_gemm.py).  Shared scratch: counters 512 zeroed uint32 (left zero), tsum
 * 32*3*1024 doubles.  *route (nullable) reports which kernel and which BatchNorm finish ran:
 * 0 the streaming kernel (its last workgroup finishes), 1 the tiled kernel finishing in its own
 * last workgroups, 2 the tiled kernel followed by a finalize launch; *records (nullable): the
 * BN records written (<= ceil(M/128)).  The *_route calls answer the same two questions on the
 * host alone (no launch; -1 on arguments the call itself would refuse).
 *
 * fwd_train: z[M][N] (ldc) = a[M][K] . B^T (+ bias[n]), B [N][K] (ldb), a = A (lda) or, with
 * a_scale / a_shift (together; K <= 768, K % V == 0), relu(A*a_scale[k] + a_shift[k]) rounded to
 * the storage type (bn_apply's output, never stored).  Plus the batch statistics of the STORED z,
 * finished in the same call: mean, invstd, scale = gamma*invstd, shift = beta - mean*scale, the
 * running statistics (momentum; unbiased variance) and *nbt += 1 (nullable).  part: room for
 * ceil(M/128)*3*N floats. */
int fscnn_pw_fwd_train_route(int M, int N, int K, int lda, int ldc, int lazy, int dtype,
                             int* records);
int fscnn_pw_fwd_train(int M, int N, int K, const void* A, int lda, const float* a_scale,
                       const float* a_shift, const void* B, int ldb, const float* bias, void* z,
                       int ldc, float* part, unsigned* counters, double* tsum, const float* gamma,
                       const float* beta, float* rmean, float* rvar, long long* nbt,
                       float momentum, float* mean, float* invstd, float* scale, float* shift,
                       int dtype, int* route, int* records, void* stream);
/* wgrad_train: dW[N][K] = sum_m D[m][n] x[m][k], x = X or its lazy BN+ReLU (x_scale / x_shift as
 * above), and, when dbias is given, dbias[n] = sum_m D[m][n] (bias_part: ceil(M/1024)*N floats,
 * given together with dbias).  slab: fscnn_pw_wgrad_slab_floats floats; *splits (nullable): the
 * row splits, each of ceil(ceil(M/splits)/64)*64 rows. */
int fscnn_pw_wgrad_train(int M, int N, int K, const void* D, int ldd, const void* X, int ldx,
                         const float* x_scale, const float* x_shift, float* slab, float* dW,
                         float* bias_part, float* dbias, int dtype, int* splits, void* stream);
/* dgrad_train: fscnn_pw_dgrad_bnbwd's call (same arguments, same sums) plus
 *  - tab [N][8] (16-byte aligned): that BN's backward as a per-channel operand transform,
 *    dz = al*mask*dy + gz*z + be with mask = (z*sc + sh > 0); tab[n] = (al, be, gz, sc, sh, ...),
 *    al = scale, gz = -scale*coef1*invstd, be = -scale*coef0 - gz*mean, (sc, sh) = the forward
 *    (scale, shift) in relu_mode 2 and (0, 1) in relu_mode 0;
 *  - an output dropout (drop_hw > 0: pixels per image, M % drop_hw == 0): the stored dX is
 *    fscnn_dropout's keep ? round(dX) / (1 - p) : 0 with the mask of NCHW index
 *    ((m / hw)*N + n)*hw + m % hw and seed (or *seed_slot) + seed_add, and the BN sums are those
 *    of the dropped dX.  Streaming kernel only (16-bit K <= 32, fp32 K <= 16, M >= 4096):
 *    refused otherwise. */
int fscnn_pw_dgrad_train_route(int M, int N, int K, int ldd, int lddx, int residual, int drop_hw,
                               int dtype, int* records);
int fscnn_pw_dgrad_train(int M, int N, int K, const void* D, int ldd, const void* B, int ldb,
                         const void* R, int ldr, void* dX, int lddx, const void* z, int ldz,
                         const float* mean, const float* invstd, const float* scale,
                         const float* shift, int relu_mode, float* part, unsigned* counters,
                         double* tsum, float* dgamma, float* dbeta, float* coef, float* tab,
                         int drop_hw, float drop_p, unsigned long long seed,
                         unsigned long long seed_add, const unsigned long long* seed_slot,
                         int dtype, int* route, int* records, void* stream);
/* The aux head's 3x3 conv as columns (pad 1, stride 1), x NHWC [N][H][W] (ldx >= C):
 * col[m][c*9 + kh*3 + kw] = x[n][h+kh-1][w+kw-1][c] or 0 (ldcol >= 9 C; columns past 9 C are not
 * written), and its transpose dx[m][c] (+)= sum_{kh,kw} dcol[n][h+1-kh][w+1-kw][c*9 + kh*3 + kw]
 * (accumulate: added to the stored dx). */
int fscnn_im2col3(const void* x, int ldx, int dtype, int N, int H, int W, int C, void* col,
                  int ldcol, void* stream);
int fscnn_col2im3(const void* dcol, int ldcol, int dtype, int N, int H, int W, int C, void* dx,
                  int lddx, int accumulate, void* stream);

#ifdef __cplusplus
}
#endif
#endif
