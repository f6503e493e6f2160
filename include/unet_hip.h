/*
 * unet_hip.h - C ABI of the MI355X-native U-Net lane-segmentation path (libunet_hip.so).
 *
 * The reference has no FFI: its seam is the Python model container
 * `RKNN_model_container` (reference src/py_utils/rknn_executor.py:4-42), whose
 * `run()` hands a uint8 NHWC frame to a vendor runtime (`rknn.inference`,
 * rknn_executor.py:36) and gets the mask tensor back.  These entry points are
 * what a binding for that seam needs: plain pointers and sizes, no torch or
 * numpy types.  Each function names the reference interface it stands in for.
 *
 * Conventions
 *   - every function returns UNET_OK (0) or a non-zero unet_status code;
 *     unet_last_error() gives the text of the last failure on that handle,
 *     unet_op_last_error() that of the calling thread's last failed call without one
 *     (reference: `exit(ret)` on init failure, rknn_executor.py:16-18);
 *   - `*_dev` pointers are caller-owned DEVICE pointers on the handle's HIP
 *     device; `*_host` pointers are host memory;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - the library owns only its packed-weight arena and its activation
 *     workspace; it never frees or reallocates caller memory;
 *   - calls on one handle are not re-entrant (the reference calls run() from a
 *     single rospy subscriber thread, src/unet_ros_node.py:280,313); they may
 *     come from any host thread (hipSetDevice is issued per call).
 */
#ifndef UNET_HIP_H
#define UNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct unet_ctx* unet_handle_t;

typedef enum unet_status {
  UNET_OK = 0,
  UNET_ERR_INVALID_ARG = 1, /* null pointer, bad enum, bad size */
  UNET_ERR_SHAPE = 2,       /* H or W not a multiple of 2^depth, numel mismatch */
  UNET_ERR_STATE = 3,       /* call order: params missing, not finalized, released */
  UNET_ERR_HIP = 4,         /* a HIP runtime call failed */
  UNET_ERR_NOMEM = 5,       /* device allocation failed */
  UNET_ERR_UNKNOWN_PARAM = 6,
  UNET_ERR_RANGE = 7        /* f16x3 tier: an activation left the fp16 range; re-run on the fp32 tier (unet_device_error) */
} unet_status;

#define UNET_MAX_DEPTH 6
#define UNET_MAX_CLASSES 8

/* Network description = constructor arguments of the reference's float model,
 * `UNet(in_channels, out_channels, features)` (reference README.md:1424). */
typedef struct unet_config {
  int32_t in_channels;              /* 3 */
  int32_t out_channels;             /* 1: the reference's lane head; 2..UNET_MAX_CLASSES: the multi-class head (below) */
  int32_t depth;                    /* len(features), 1..UNET_MAX_DEPTH */
  int32_t features[UNET_MAX_DEPTH]; /* e.g. {64,128,256,512} */
  int32_t device;                   /* HIP device index (reference: device_id string, rknn_executor.py:5) */
  float input_mean[3];              /* per-channel (u8 - mean) / std, reference README.md:3110-3111 */
  float input_std[3];
} unet_config;

/* ---- lifecycle: stands in for RKNN() + load_rknn + init_runtime (rknn_executor.py:6-21) ---- */
int unet_create(const unet_config* cfg, unet_handle_t* out);

/* Hand over one state_dict tensor in PyTorch layout (fp32, host memory):
 * conv (O,I,3,3), ConvTranspose (I,O,2,2), BatchNorm vectors, head (1,C,1,1).
 * `name` is the reference state_dict key (README.md:1424-1447), e.g.
 * "encoder_blocks.0.0.weight".  The integer num_batches_tracked counters are not
 * parameters of the forward pass and are not passed.  May be called again later to
 * overwrite a tensor (followed by unet_finalize). */
int unet_load_param(unet_handle_t h, const char* name, const float* data_host, size_t numel);

/* Fold eval-mode BatchNorm into per-channel scale/shift, repack weights into
 * MFMA fragment order and upload them.  Fails with UNET_ERR_STATE if a
 * tensor of the network is missing. */
int unet_finalize(unet_handle_t h);

/* Number of state_dict float tensors the network expects / name of the i-th. */
int unet_num_params(unet_handle_t h);
const char* unet_param_name(unet_handle_t h, int index);
size_t unet_param_numel(unet_handle_t h, int index);

/* Activation workspace the library allocates for a batch shape (bytes);
 * unet_reserve allocates it ahead of time so forward does no hipMalloc. */
size_t unet_workspace_bytes(unet_handle_t h, int n, int height, int width);
int unet_reserve(unet_handle_t h, int n, int height, int width);

/* ---- the hot path: stands in for rknn.inference(inputs=[u8 NHWC]) (rknn_executor.py:36) ----
 * frames_dev : (N,H,W,3) uint8 RGB, un-normalised (reference src/unet.py:30-42)
 * logits_dev : (N,1,H,W) float32 pre-sigmoid logits, or NULL
 * probs_dev  : (N,1,H,W) float32 sigmoid(logits) - what the deployed blob returns
 *              (its last op is ConvSigmoid), or NULL
 * mask_dev   : (N,H,W) uint8, 255 where logit > threshold_logit else 0, or NULL
 *              (reference src/unet.py:67 thresholds the probability; callers
 *              pass threshold_logit = log(t/(1-t)), 0 for t = 0.5) */
int unet_forward_u8(unet_handle_t h, const uint8_t* frames_dev, int n, int height, int width,
                    float* logits_dev, float* probs_dev, uint8_t* mask_dev, float threshold_logit,
                    void* stream);

/* forward(image)->logits of the float model (reference README.md:1460-1481):
 * image_dev is (N,3,H,W) float32, already normalised, NCHW like the PyTorch module. */
int unet_forward_f32(unet_handle_t h, const float* image_nchw_dev, int n, int height, int width,
                     float* logits_dev, float* probs_dev, uint8_t* mask_dev, float threshold_logit,
                     void* stream);

/* bf16 tier of the same forward (BASELINE.json configs[2]): bf16 activations and weights, fp32 accumulate,
 * fp32 BatchNorm/ReLU epilogue, fp32 logits out.  A separate accuracy tier: the 1e-3 fp32 logit bound does not
 * apply.  Needs every feature width to be a multiple of 32. */
int unet_forward_u8_bf16(unet_handle_t h, const uint8_t* frames_dev, int n, int height, int width,
                         float* logits_dev, float* probs_dev, uint8_t* mask_dev, float threshold_logit,
                         void* stream);

/* Split-operand ("f16x3") tier of the same forward: every fp32 operand is carried as fp16 hi + lo and every
 * product is formed by three fp16 MFMAs with fp32 accumulation (csrc/conv_x3_ws.h).  Same accuracy class as the
 * exact-fp32 tier - it passes the fp32 parity tests (logits within 2e-4 of the reference's, masks identical off
 * ties) - at 3/16 of its MFMA cost.  Same arguments and outputs as unet_forward_u8 / unet_forward_f32.  Needs
 * in_channels == 3, every feature width a multiple of 64 (<= 512) and activations below 65504 in magnitude. */
int unet_forward_u8_x3(unet_handle_t h, const uint8_t* frames_dev, int n, int height, int width,
                       float* logits_dev, float* probs_dev, uint8_t* mask_dev, float threshold_logit,
                       void* stream);
int unet_forward_f32_x3(unet_handle_t h, const float* image_nchw_dev, int n, int height, int width,
                        float* logits_dev, float* probs_dev, uint8_t* mask_dev, float threshold_logit,
                        void* stream);

/* Release device memory: stands in for rknn.release() (rknn_executor.py:40-42).
 * Idempotent on a live handle pointer set to NULL by the caller; after it every
 * other call on the handle is invalid. */
int unet_destroy(unet_handle_t h);

/* ---- per-launch timing (measurement aid, stands in for the reference's wall-clock around run(),
 * src/unet.py:80-83): when enabled, every kernel launch of a forward call is bracketed by a
 * hipEvent pair on the caller's stream.  unet_profile_count synchronises on the recorded events. */
int unet_profile_enable(unet_handle_t h, int on);
int unet_profile_count(unet_handle_t h);
int unet_profile_get(unet_handle_t h, int index, char* name, size_t name_cap, double* ms, double* flops,
                     double* bytes);

/* ---- training step (reference README.md:2060-2084: zero_grad, model(images) in train mode,
 * BCEWithLogitsLoss README.md:1694-1709, loss.backward(), optimizer.step() README.md:2173) ----
 * Parameters, gradients, Adam moments and BatchNorm running statistics live in caller-owned flat
 * device buffers: tensors in PyTorch layout back to back, in unet_param_name() order, the
 * running_mean / running_var entries in `bn_buffers_dev`, everything else in the other four.
 * unet_train_layout gives each entry's offset (in floats) and which buffer it lives in. */
size_t unet_train_param_numel(unet_handle_t h);
size_t unet_train_buffer_numel(unet_handle_t h);
int unet_train_layout(unet_handle_t h, int index, int* is_buffer, size_t* offset);
int unet_train_attach(unet_handle_t h, float* params_dev, float* grads_dev, float* exp_avg_dev,
                      float* exp_avg_sq_dev, float* bn_buffers_dev);
size_t unet_train_workspace_bytes(unet_handle_t h, int n, int height, int width);

/* Loss of the step.  mode 0 (default): BCEWithLogitsLoss, mean (reference README.md:1694-1709).
 * mode 1: the reference training script's BCEDiceLoss (README.md:1855-1893, :2169-2170):
 *   bce_weight * BCEWithLogits(pos_weight) + dice_weight * (1 - (2 sum(s t) + smooth) / (sum s + sum t + smooth));
 * loss_dev then receives three floats {total, bce, dice}. */
int unet_train_set_loss(unet_handle_t h, int mode, float bce_weight, float dice_weight, float pos_weight,
                        float smooth);

/* The loss as one structure.  mode 0 / 1: as unet_train_set_loss (focal_weight, alpha, gamma are ignored).
 * mode 2: the general loss of the reference's loss family (README.md:1694 BCELoss, :1781 DiceLoss, :1855 BCEDiceLoss,
 * :1914-1939 FocalLoss; table of which to use when :1942-1951, "Focal + Dice, gamma = 2.0" for masks under 5 % lane):
 *   L = bce_weight * BCEWithLogits(pos_weight) + focal_weight * Focal(alpha, gamma) + dice_weight * Dice(smooth)
 * with, per element (x the logit, t the target, any float in [0, 1]; p = sigmoid(x)),
 *   ce = max(x,0) - x t + log1p(exp(-|x|)),   q = p (1 - t) + (1 - p) t  [= 1 - p_t, formed without the subtraction],
 *   a_t = alpha t + (1 - alpha)(1 - t),   Focal = mean_i(a_t q^gamma ce).
 * All three terms are always computed and reported; the weights decide the total and the gradient. */
typedef struct unet_loss_config {
    int mode;
    float bce_weight, focal_weight, dice_weight, pos_weight, alpha, gamma, smooth;
} unet_loss_config;

/* Stands in for the `criterion = ...` line of a training script that picks a loss of that family (README.md:2169-2170).
 * loss_dev of unet_train_forward_backward_* then receives four floats {total, bce, dice, focal}; the profile record of
 * the mode-2 passes is "focal_loss_grad".  Modes 0 and 1 behave exactly like unet_train_set_loss.
 * Mode 2 accepts: every weight >= 0 and not all of them zero; pos_weight > 0; 0 <= alpha <= 1; smooth > 0; gamma == 0
 * (alpha-weighted BCE, no power is evaluated) or gamma >= 1.  Everything else, NaN and Inf included, is
 * UNET_ERR_INVALID_ARG - checked first, so the answer does not depend on the handle's state.  0 < gamma < 1 is rejected
 * on purpose: d/dx q^gamma is unbounded at q = 0, which a saturated logit reaches in fp32 (the reference's own autograd
 * returns NaN there).  Inside the domain no finite logit produces NaN or Inf.  UNET_ERR_STATE without
 * unet_train_attach. */
int unet_train_set_loss_cfg(unet_handle_t h, const unet_loss_config* cfg);

/* Forward in train mode (batch statistics, running stats updated with momentum 0.1), mean
 * BCE-with-logits against targets_dev (N,1,H,W float 0/1), full backward.  Writes every parameter
 * gradient into grads_dev (overwriting: this is zero_grad + backward), the scalar loss into
 * loss_dev[0] (loss_dev must hold 4 floats; see unet_train_set_loss) and, if not NULL, the logits into logits_dev.  No communication: a data-parallel
 * caller all-reduces grads_dev between this call and unet_train_adam_step. */
int unet_train_forward_backward_u8(unet_handle_t h, const uint8_t* frames_dev, const float* targets_dev, int n,
                                   int height, int width, float* loss_dev, float* logits_dev, void* stream);
int unet_train_forward_backward_f32(unet_handle_t h, const float* image_nchw_dev, const float* targets_dev, int n,
                                    int height, int width, float* loss_dev, float* logits_dev, void* stream);

/* torch.optim.Adam (decoupled = 0) or AdamW (decoupled = 1) on the flat buffers, `step` counted
 * from 1; gradients are multiplied by grad_scale first (1/world_size after a SUM all-reduce).
 * Re-derives the packed MFMA operands from the updated parameters. */
int unet_train_adam_step(unet_handle_t h, int step, float lr, float beta1, float beta2, float eps,
                         float weight_decay, int decoupled, float grad_scale, void* stream);

/* ---- the gradient pass: accumulation, global norm, non-finite count (csrc/grad_kernels.h) -------------------------
 * No reference counterpart in code: the reference's troubleshooting table names gradient accumulation
 * (README.md:2356); global-norm clipping and the non-finite guard have torch's semantics
 * (torch.nn.utils.clip_grad_norm_, GradScaler.step's skip).  The arithmetic is restated in tests/grad_model.py.
 *
 * unet_grad_accumulate_f32: one pass over flat fp32 device buffers of `numel` floats,
 *     dst[i] = a[i] + b[i]        one fp32 addition per element; b == NULL: dst[i] = a[i]
 * dst may be a or b (or lie apart from them; a partial overlap is refused).  dst == a with b == NULL stores nothing:
 * a pure reduction.  record (optional, two doubles on the device, 8-byte aligned) is OVERWRITTEN with a description of
 * the values written to - in the pure reduction read from - dst:
 *     record[0] = the sum of x * x over the finite elements, squares and sum formed in double
 *     record[1] = the number of non-finite elements (+-inf, NaN)
 * With a record, `work` (unet_grad_work_bytes bytes on the device, 8-byte aligned, the caller's) holds the blocks'
 * partial sums.  The reduction uses no atomics and a grid that depends on numel alone (at most 2048 blocks of 256
 * threads, on any device): per-thread partials in double, a fixed tree per block, and a one-block second launch that
 * adds the blocks' partials in a fixed order.  For given numel and given distances of dst, a and b from a 16-byte
 * boundary the record is the same bits on every run, every device and every rank; it differs from the exactly rounded
 * sum by at most numel * 2^-53, relative.  Pointers need 4-byte alignment only: the pass uses 16-byte accesses where
 * dst, a and b are equally far from a 16-byte boundary (a head and a tail of up to three floats are peeled) and 4-byte
 * accesses where they are not.  numel == 0 is valid and gives the record {0, 0}.  A bare device ordinal; the call only
 * enqueues on `stream`; bad arguments are refused with UNET_ERR_INVALID_ARG and a text for unet_op_last_error that
 * names the call, before any device is touched. */
size_t unet_grad_work_bytes(void);
int unet_grad_accumulate_f32(int device, float* dst, const float* a, const float* b, size_t numel, double* record,
                             double* work, void* stream);

/* unet_train_adam_step with the gradient multiplier taken from a record of unet_grad_accumulate_f32 over the attached
 * gradient buffer, on the device (the host reads nothing; the kernel reads the record with ordinary loads):
 *     coef = grad_scale * min(1, max_norm / (|grad_scale| * sqrt(record[0]) + 1e-6))
 * computed in double and rounded once to float: torch.nn.utils.clip_grad_norm_ applied to the gradient scaled by
 * grad_scale.  max_norm = +inf gives coef == grad_scale exactly; max_norm must be positive.  For an equal multiplier
 * the update is unet_train_adam_step's bit for bit.  If record[1] != 0 the optimiser kernel writes nothing: parameters
 * and both moments stay as they are, bit for bit (the repack of the MFMA operands still runs).  record_dev: 8-byte
 * aligned.  UNET_ERR_INVALID_ARG - before any device is touched - for a null or misaligned record, a handle without
 * unet_train_attach, step < 1 or a max_norm that is not positive. */
int unet_train_adam_step_rec(unet_handle_t h, int step, float lr, float beta1, float beta2, float eps,
                             float weight_decay, int decoupled, float grad_scale, float max_norm,
                             const double* record_dev, void* stream);

/* Data-parallel overlap (north_star: RCCL all-reduce of the gradients; the reference has no distributed code).  The
 * backward pass finishes the gradients of the decoder, the bottleneck and the head - the tail
 * [unet_train_grad_split, unet_train_param_numel) of the flat gradient buffer - before it starts on the encoder.  With a
 * communication stream set, unet_train_forward_backward_* makes that stream wait for the point where the tail is final,
 * so the caller's all-reduce of the tail, enqueued on that stream, overlaps the encoder's backward. */
int unet_train_set_comm_stream(unet_handle_t h, void* comm_stream);
size_t unet_train_grad_split(unet_handle_t h);

/* Process-wide switch for the training step's 3x3 convolutions: 1 (default) = forward, input gradient AND weight
 * gradient on the split-operand fp16 kernels (csrc/conv_x3_ws.h, conv_x3_r512.h, wgrad_x3_ws.h: fp16 hi + lo operands,
 * three MFMAs per product, fp32 accumulate) wherever Cin and Cout are multiples of 64 (environment
 * UNET_TRAIN_X3_WGRAD=0 keeps only the weight gradients on the exact-fp32 kernels); 0 = exact-fp32 MFMA kernels
 * everywhere.  BatchNorm and the loss are fp32 either way.  Accuracy: products carry ~2^-22 relative error while the
 * operands' lo parts are normal fp16 numbers; the training weight packs are not pre-scaled per channel (they are
 * re-derived on the device after every optimizer step), so for |w| < 2^-3 the lo part is subnormal and the product
 * error becomes an absolute ~2^-25 - inside the gradient tolerances of tests/test_train_gpu.py, which run in both
 * modes.  Returns the previous setting; environment UNET_TRAIN_X3=0 sets the initial value to 0. */
int unet_set_train_x3(int on);

/* Process-wide switch for WHERE the training step's f16x3 weight-gradient kernels run (no reference counterpart: the
 * reference's backward is torch autograd, README.md:2198-2201, which orders nothing beyond data dependence either).
 * 0 = in line on the caller's stream; 1 (default) = on a second, lower-priority stream owned by the handle, forked as
 * soon as the unit's dZ exists; 2 = forked behind the unit's input-gradient convolution, so that the weight gradient
 * runs beside the next unit's HBM-bound BatchNorm backward.  The side stream is joined back into the caller's stream before
 * the late-gradient event of unet_train_set_comm_stream and before unet_train_forward_backward_* returns its work to
 * the stream, so callers see no difference in ordering; results are bit-identical in all modes.  Ignored (in line) while
 * per-launch profiling or a debug snapshot is active.  mode outside 0..2 only queries.  Returns the previous mode;
 * environment UNET_TRAIN_SIDE sets the initial value. */
int unet_set_train_side(int mode);

/* Re-derive the packed MFMA operands from the attached parameter buffer after the caller overwrote it
 * (checkpoint load: reference README.md:2231 `model.load_state_dict`).  Unlike a second unet_train_attach it keeps
 * the loss configuration (unet_train_set_loss) and the workspace.  Synchronises the stream. */
int unet_train_repack(unet_handle_t h, void* stream);

/* Dice metric of the reference's validation loop (README.md:2115-2120 `compute_dice`, called at :2103-2104 with
 * pred = sigmoid(outputs) > 0.5): out_dev[0] = (2 sum(pred t) + smooth) / (sum pred + sum t + smooth) with
 * pred = logit > threshold_logit; out_dev[1..3] = the three sums.  logits/targets: `numel` floats each. */
int unet_dice_metric(int device, const float* logits_dev, const float* targets_dev, size_t numel,
                     float threshold_logit, float smooth, float* out_dev, void* stream);

/* Eval-mode forward on a training handle: `model.eval(); with torch.no_grad(): outputs = model(images)` of the
 * reference's validate() (README.md:2087-2099) on the parameters and BatchNorm buffers attached right now
 * (unet_train_attach) - no host round trip, no second copy of the weights.  BatchNorm uses the running statistics
 * (scale = gamma / sqrt(running_var + 1e-5), shift = beta - running_mean * scale, folded on the device at every call);
 * the convolutions run on the operand packs the training step keeps current, with the same kernel dispatch
 * (unet_set_train_x3).  Logits (N,1,H,W) go to logits_dev.  Uses the training workspace (unet_train_workspace_bytes) and
 * writes nothing a training step reads later: parameters, gradients, Adam moments, running statistics, the loss
 * configuration and the step's saved statistics stay as they are.  The fp16 range watch stays armed (unet_device_error).
 * UNET_ERR_STATE without unet_train_attach, UNET_ERR_SHAPE as the train entry points. */
int unet_train_eval_u8(unet_handle_t h, const uint8_t* frames_dev, int n, int height, int width, float* logits_dev,
                       void* stream);
int unet_train_eval_f32(unet_handle_t h, const float* image_nchw_dev, int n, int height, int width, float* logits_dev,
                        void* stream);

/* ---- multi-class segmentation: out_channels = K, 2 <= K <= UNET_MAX_CLASSES (csrc/multiclass_kernels.h) ----------
 * The reference's roadmap (multi-lane classification, lane + drivable area) on the network as it is: the 1x1 head has K
 * rows, a pixel's class is the argmax of its K logits, training minimises softmax cross-entropy (+ Dice).  A handle with
 * out_channels == 1 runs exactly what it ran before; every entry point below returns UNET_ERR_INVALID_ARG for it, and
 * the single-class entry points (the unet_forward_* family of every tier, the training step with float targets, the
 * unet_train_set_loss pair) return UNET_ERR_INVALID_ARG for a handle with K > 1, each with a text for unet_last_error,
 * before any device is touched.  The K-class forward exists on the fp32 and f16x3 tiers and on the int8 tier with its
 * hybrid units (the unet_i8_* section below: a quantised model is K-class when its head arrays have K rows), the training
 * step on the training handle (which dispatches its convolutions as for K == 1); the bf16 and f16q8 inference tiers are
 * single-class.
 *
 * Forward.  precision: 0 = the fp32 tier, 1 = the f16x3 tier (its last convolution stores operand planes and the K-way
 * head reads them; needs what unet_forward_u8_x3 needs, and the f16q8 switch off).  Every output is optional:
 *   logits_dev (N,K,H,W) fp32, NCHW like the torch module      probs_dev (N,K,H,W) = softmax over K
 *   labels_dev (N,H,W) uint8 = argmax (ties to the lowest class; a NaN logit never wins)
 *   mask_dev   (N,H,W) uint8 = 255 where the label is mask_class, else 0: the byte plane the lane-following, instance,
 *              lane-fit and video stages take. */
int unet_forward_classes_u8(unet_handle_t h, const uint8_t* frames_dev, int n, int height, int width, int precision,
                            float* logits_dev, float* probs_dev, uint8_t* labels_dev, int mask_class, uint8_t* mask_dev,
                            void* stream);
int unet_forward_classes_f32(unet_handle_t h, const float* image_nchw_dev, int n, int height, int width, int precision,
                             float* logits_dev, float* probs_dev, uint8_t* labels_dev, int mask_class, uint8_t* mask_dev,
                             void* stream);

/* The class loss.  A pixel is valid if its label is below K and is not ignore_index (-1: none).
 *   CE    = sum_valid cw[t] (logsumexp(z) - z_t) / sum_valid cw[t]       F.cross_entropy(weight=, ignore_index=), mean
 *   Dice  = 1 - mean_k (2 sum_valid p_k [t = k] + smooth) / (sum_valid p_k + sum_valid [t = k] + smooth),  p = softmax(z)
 *   total = ce_weight CE + dice_weight Dice
 * Deviations from torch, both on purpose: a label >= K that is not the ignore index is treated as ignored and counted
 * (torch raises); with no valid weight (the CE denominator is 0) the CE term and its gradient are 0 (torch gives NaN).
 * Domain: ce_weight, dice_weight >= 0 and not both 0; smooth > 0; class_weight[0..K) >= 0 and finite; ignore_index -1
 * or 0..255; NaN and Inf are rejected.  Inside it no finite logit produces NaN or Inf. */
typedef struct unet_class_loss_config {
    float ce_weight, dice_weight, smooth;
    float class_weight[UNET_MAX_CLASSES];
    int ignore_index;
} unet_class_loss_config;

/* The loss of a K-class training handle (default: ce_weight 1, dice_weight 0, smooth 1, class weights 1, no ignore
 * index).  The configuration is checked first (UNET_ERR_INVALID_ARG), then the state (UNET_ERR_STATE without
 * unet_train_attach). */
int unet_train_set_class_loss(unet_handle_t h, const unet_class_loss_config* cfg);

/* The training step of a K-class handle: as unet_train_forward_backward_u8 / _f32 with labels_dev (N,H,W) uint8 in place of
 * the float targets.  loss_dev receives four floats {total, ce, dice, number of out-of-range labels}; logits_dev
 * (optional) the (N,K,H,W) logits.  Profile records: "headk", "class_loss_grad", "headk_bwd".  On a K-class handle
 * unet_train_eval_u8 / _f32 write (N,K,H,W) logits. */
int unet_train_forward_backward_labels_u8(unet_handle_t h, const uint8_t* frames_dev, const uint8_t* labels_dev, int n,
                                          int height, int width, float* loss_dev, float* logits_dev, void* stream);
int unet_train_forward_backward_labels_f32(unet_handle_t h, const float* image_nchw_dev, const uint8_t* labels_dev, int n,
                                           int height, int width, float* loss_dev, float* logits_dev, void* stream);

/* Confusion matrix of one batch ADDED TO acc_dev: k * k unsigned 64-bit counts owned (and zeroed before the first batch)
 * by the caller, acc_dev[t * k + p] = pixels of true class t predicted as p, over the pixels whose true label is below k
 * and is not ignore_index and whose prediction is below k.  Integers throughout: exact.  work_dev: unet_confusion_work_bytes
 * bytes on the device, the caller's.  A bare device ordinal; only enqueues on `stream`; bad arguments are refused with
 * UNET_ERR_INVALID_ARG and a text for unet_op_last_error, before any device is touched.  numel at most 2^40. */
size_t unet_confusion_work_bytes(void);
int unet_confusion_accumulate(int device, const uint8_t* pred_dev, const uint8_t* truth_dev, size_t numel, int k,
                              int ignore_index, unsigned long long* acc_dev, void* work_dev, void* stream);

/* Labels and class mask of stored logits (n,k,pixels_per_image), e.g. those of unet_train_eval_*: the argmax and the byte
 * plane of the forward above; either output optional.  The class loss of stored logits against labels (n,
 * pixels_per_image) uint8: loss_dev[4] as the training step's, dlogits_dev (n,k,pixels_per_image) or NULL for the loss
 * alone (a validation loop); work_dev: unet_class_loss_work_bytes bytes on the device, 8-byte aligned, the caller's.  Both
 * take a bare device ordinal, only enqueue on `stream` and refuse bad arguments (a configuration outside its domain
 * included) with UNET_ERR_INVALID_ARG and a text for unet_op_last_error, before any device is touched. */
int unet_class_labels_f32(int device, const float* logits_dev, int n, int k, size_t pixels_per_image, uint8_t* labels_dev,
                          int mask_class, uint8_t* mask_dev, void* stream);
size_t unet_class_loss_work_bytes(void);
int unet_class_loss_grad(int device, const float* logits_dev, const uint8_t* labels_dev, int n, int k,
                         size_t pixels_per_image, const unet_class_loss_config* cfg, float* loss_dev, float* dlogits_dev,
                         void* work_dev, void* stream);

/* Test entry points of the multi-class kernels: weights and bias from host memory, scratch of the call's own, the stream
 * synchronised before they return.  x / a / d_a: (n*h*w, c) dense fp32, 16-byte aligned, c % 4 == 0, k * c <= 4096.
 * unet_op_headk: the outputs of the forward above, each optional.  unet_op_headk_backward: d_a[p,c] = sum_k
 * dl[k,p] w[k,c] (optional), d_w[k,c] = sum_p dl[k,p] a[p,c], d_b[k] = sum_p dl[k,p], all on the device. */
int unet_op_headk(int device, const float* x_dev, int n, int h, int w, int c, int k, const float* w_host,
                  const float* b_host, float* logits_dev, float* probs_dev, uint8_t* labels_dev, int mask_class,
                  uint8_t* mask_dev, void* stream);
/* ... and from the f16x3 tier's operand planes: x_dev = fp16 hi plane (n*h*w, c), the lo plane x_lo halfs behind it (the
 * layout of unet_op_head1x1_x3_planes); c % 8 == 0; the input is hi + lo. */
int unet_op_headk_x3_planes(int device, const uint16_t* x_dev, size_t x_lo, int n, int h, int w, int c, int k,
                            const float* w_host, const float* b_host, float* logits_dev, float* probs_dev,
                            uint8_t* labels_dev, int mask_class, uint8_t* mask_dev, void* stream);
int unet_op_headk_backward(int device, const float* dlogits_dev, const float* a_dev, const float* w_host, int n, int h,
                           int w, int c, int k, float* d_a_dev, float* d_w_dev, float* d_b_dev, void* stream);

/* Segmentation metrics and validation loss of one batch as one device reduction, added to running accumulators: the
 * body of the reference's validate() loop (README.md:2101-2110: criterion, compute_dice :2115-2120, per-batch values
 * averaged over the batches) and the confusion counts behind its published IoU / Dice / Precision / Recall / F1 /
 * pixel accuracy (README.md:4177-4184).  acc_dev: 16 doubles owned by the caller, zeroed by the caller before the first
 * batch:
 *   [0..3]  TP FP FN TN pixel counts over all batches so far, exact integers stored as doubles (exact below 2^53), with
 *           pred = logit > threshold_logit, truth = target > 0.5 (uint8 targets: target != 0)
 *   [4..6]  sum over the batches of the batch's (total, bce, dice) loss: loss_mode 0 = BCEWithLogits(mean) (total = bce,
 *           dice = 0), 1 = bce_weight * BCE(pos_weight) + dice_weight * Dice(smooth), as unet_train_set_loss
 *   [7]     sum over the batches of the batch's compute_dice(pred, target, smooth)
 *   [8]     number of batches      [9] number of pixels      [10..15] reserved
 * targets_dev: `numel` floats (0/1), or with targets_are_u8 `numel` bytes (0 / non-zero, e.g. 0 / 255 masks).  No host
 * synchronisation; takes a bare device index like unet_dice_metric, so it serves logits from any tier. */
int unet_seg_metrics_accumulate(int device, const float* logits_dev, const void* targets_dev, int targets_are_u8,
                                size_t numel, float threshold_logit, int loss_mode, float bce_weight, float dice_weight,
                                float pos_weight, float smooth, double* acc_dev, void* stream);
/* The same with the loss as a structure, so a validation pass (README.md:2101-2110) can report the general loss:
 * modes 0 and 1 are unet_seg_metrics_accumulate itself; with mode 2 slots [4..6] receive (total, bce, dice) of the
 * general loss and slot [10] the sum over the batches of the batch's focal term (README.md:1914-1939).  Slots [0..3],
 * [7..9] and [15] keep their meaning; [11..14] stay reserved.  The loss sums are formed by the code the training step
 * runs: the values equal what the step reports for the same logits. */
int unet_seg_metrics_accumulate_cfg(int device, const float* logits_dev, const void* targets_dev, int targets_are_u8,
                                    size_t numel, float threshold_logit, const unet_loss_config* cfg, double* acc_dev,
                                    void* stream);

/* Positive pixels per mask, the statistic behind the reference's two remedies for class imbalance (README.md:2514-2530
 * `calculate_pos_weight`: positive_pixels += (mask > 127).sum(); :2544-2553 `get_sample_weights`: the lane ratio of each
 * image): masks_dev holds n images of pixels_per_image bytes back to back, counts_dev[i] = number of pixels of image i
 * with mask > threshold (the reference binarises with > 127, README.md:2022, :2522).  One pass over the masks, integer
 * arithmetic: exact and deterministic.  No host synchronisation. */
int unet_mask_positive_counts(int device, const uint8_t* masks_dev, int n, size_t pixels_per_image, int threshold,
                              unsigned long long* counts_dev, void* stream);

const char* unet_last_error(unet_handle_t h);
/* The same for the entry points that take a device ordinal instead of a handle (unet_op_*, the loss, metric and camera
 * helpers, unet_augment_u8): the text of the last failure of such a call on the calling thread ("" if there was none).
 * Every non-zero status of such a call sets it, a refusal by the argument checks included; it is not cleared on success. */
const char* unet_op_last_error(void);
const char* unet_version(void);

/* Asynchronous kernel-side conditions, kept in a per-handle error block the kernels write to.
 *  - A kernel whose bounded wave-progress wait gives up (csrc/wino_f32.h) records it instead of continuing silently
 *    with stale data.  The next unet_forward_* / unet_train_forward_backward_* call that sees the record returns
 *    UNET_ERR_HIP (like an asynchronous HIP error the failing launch may be an earlier one) and clears it, so one
 *    transient failure is reported once.
 *  - The f16x3 tier stores activations as fp16 hi + lo planes: |v| <= 65504, where the reference's fp32 network
 *    (README.md:1449-1458) has no such bound.  Activations are stored scaled by a per-channel power of two chosen
 *    from the BatchNorm parameters so that four standard deviations sit near 2^10 (csrc/unet_x3.inc), which leaves
 *    the range only for inputs hundreds of standard deviations from the running statistics; a kernel that meets such a
 *    value records it.  Only unet_device_error reports that (UNET_ERR_RANGE): the results of the calls since the last
 *    unet_device_error are then not at fp32 parity and the caller re-runs them on the fp32 tier
 *    (py_utils/rknn_executor.py does).
 * unet_device_error synchronises the device, returns UNET_ERR_HIP / UNET_ERR_RANGE / UNET_OK for everything launched on
 * this handle since its last call, and clears the block.  The reference's container has no equivalent:
 * rknn.inference reports failure through its return value (rknn_executor.py:36). */
int unet_device_error(unet_handle_t h);
/* The same for a caller that launched everything on one stream: waits for that stream only (other streams of the
 * device - a camera stage, a second model - keep running), then reports and clears as unet_device_error does. */
int unet_device_error_on(unet_handle_t h, void* stream);
/* Data-parallel callers (trainer.py; the reference has no distributed code, BASELINE.json north_star asks for an RCCL
 * all-reduce of the gradients): enqueue on `stream` a one-thread kernel that writes 1.0f to the device float `dst` if the
 * error block holds any record of the launches before it on that stream, else 0.0f.  Nothing is synchronised or cleared.
 * The trainer puts `dst` in front of its flat gradient bucket, so the word is summed over the ranks by the SAME
 * all-reduce as the gradients and every rank learns whether ANY rank failed before any of them updates its parameters. */
int unet_device_status_to(unet_handle_t h, float* dst, void* stream);

/* Test hook: write `value` into word `word` (0 = kernel failure, 1 = fp16 range) of the handle's error block, as a
 * kernel would.  Lets the host-side recovery paths be exercised without a failing kernel. */
int unet_debug_set_error_block(unet_handle_t h, int word, unsigned value);
/* Test hook, host arithmetic only: the power-of-two scale the f16x3 tier stores a BatchNorm channel's activations with
 * (csrc/unet_x3.inc, ActScale): 4 |gamma| + |beta| lands in [512, 1024), the scale clamped to [2^-40, 2^40], 1 for a
 * channel whose magnitude is below 1e-30. */
float unet_debug_act_scale(float gamma, float beta);

/* Process-wide algorithm switch for 3x3 convolutions with Cin % 16 == 0 on even-sized maps:
 * 1 = Winograd F(2x2,3x3) on the fp32 MFMA pipe (default), 0 = direct implicit GEMM.
 * Returns the previous setting.  Environment UNET_NO_WINOGRAD=1 sets the initial value to 0. */
int unet_set_winograd(int on);

/* Process-wide kernel choice for the bf16 tier's 3x3 convolutions.  -1 = automatic (default): the wave-specialised
 * kernel (csrc/conv_bf16_ws.h) on wide maps with enough tiles per CU, the one-wave-per-SIMD kernel
 * (csrc/conv_bf16_r512.h) on maps whose width is a multiple of 28 (or 14) with Cout % 128 == 0 and a work item for
 * half the CUs, the 2x2-wave kernel (csrc/igemm_bf16.h) otherwise; 0 = the 2x2-wave kernel only; 1 = the
 * wave-specialised kernel whenever the layer shape allows it (Cin % 64 == 0, Cout % 64 == 0 and <= 512, H % 16 == 0);
 * 2 = the one-wave-per-SIMD kernel whenever the shape allows it.  All three accumulate chunk by chunk, tap by tap and
 * give bit-identical results (tests/test_bf16_gpu.py).  The tier's ConvTranspose2d follows the same switch: mode 1 its
 * wave-specialised kernel (csrc/upconv_bf16_ws.h), mode 2 - and automatically, once there is a work item for half of
 * the CUs - its one-wave-per-SIMD kernel (csrc/upconv_bf16_r512.h; Cin % 128 == 0).  Returns the previous setting. */
int unet_set_bf16_persistent(int mode);

/* ---- single operators, for parity tests against the oracle (tests/test_ops_gpu.py) ----
 * All tensors are dense NHWC float32 device buffers.  Weights are passed in
 * PyTorch layout on the HOST and packed internally (slow path, test only).
 * These and the other unet_op_* entry points below take a device ordinal, own their device scratch for the length of the
 * call (everything is freed on every return path), wait for `stream` before they return (all but unet_op_loss_grad,
 * which the training step's helper runs behind and which only enqueues) and leave the text of a failure for
 * unet_op_last_error(). */

/* y = relu?(conv3x3(x, w) * scale + shift), pad 1, stride 1 (reference README.md:1452-1457).
 * x (N,H,W,Cin) -> y (N,H,W,Cout); w_host (Cout,Cin,3,3); scale/shift host (Cout). */
int unet_op_conv3x3(int device, const float* x_dev, int n, int h, int w, int cin, const float* w_host,
                    const float* scale_host, const float* shift_host, int cout, int relu,
                    float* y_dev, void* stream);

/* ConvTranspose2d k=2 s=2 with bias (reference README.md:1442): x (N,H,W,Cin) -> y (N,2H,2W,Cout);
 * w_host (Cin,Cout,2,2). */
int unet_op_upconv2x2(int device, const float* x_dev, int n, int h, int w, int cin, const float* w_host,
                      const float* bias_host, int cout, float* y_dev, void* stream);

/* Plain 1x1 convolution without bias (the GEMM behind the ConvTranspose2d input gradient):
 * x (N,H,W,Cin) -> y (N,H,W,Cout); w_host (Cout,Cin). */
int unet_op_conv1x1(int device, const float* x_dev, int n, int h, int w, int cin, const float* w_host, int cout,
                    float* y_dev, void* stream);

/* MaxPool2d(2,2) (reference README.md:1429): x (N,H,W,C) -> y (N,H/2,W/2,C). */
int unet_op_maxpool2x2(int device, const float* x_dev, int n, int h, int w, int c, float* y_dev, void* stream);

/* 1x1 head with bias (reference README.md:1447): x (N,H,W,C) -> logits (N,H,W). */
int unet_op_head1x1(int device, const float* x_dev, int n, int h, int w, int c, const float* w_host,
                    float bias, float* logits_dev, void* stream);

/* The same two operators in the split-operand tier (fp32 NHWC in and out; converted to / from fp16 hi + lo planes
 * internally).  cin, cout multiples of 64.  tile_width: 0 = the dispatch's own choice, else one of the forced forms of
 * DESIGN.md section 4.15 ("The forced form"; csrc/unet_x3.inc, x3_decode_force); UNET_ERR_INVALID_ARG for any other value,
 * UNET_ERR_HIP if the forced form does not support the shape.
 * y_pool_dev: optional (N,H/2,W/2,Cout) MaxPool2d(2,2) output (reference README.md:1429). */
int unet_op_conv3x3_x3(int device, const float* x_dev, int n, int h, int w, int cin, const float* w_host,
                       const float* scale_host, const float* shift_host, int cout, int relu, int tile_width,
                       float* y_dev, float* y_pool_dev, void* stream);
/* The network's last two layers as the split-operand tier runs them (reference README.md:1456-1457, :1447, :1481): a
 * 3x3 convolution to 64 channels + scale/shift (+ ReLU) with the 1x1 head (64 -> 1, bias) fused into its epilogue; the
 * 64-channel activation is never stored.  x (N,H,W,cin) fp32 -> logits (N,H,W).  tile_width: of the forced forms
 *  only those with a fused-head instance, 0 / 16 / 32 / 628 / 632. */
int unet_op_conv3x3_x3_head(int device, const float* x_dev, int n, int h, int w, int cin, const float* w_host,
                            const float* scale_host, const float* shift_host, int relu, int tile_width,
                            const float* head_w_host, float head_bias, float* logits_dev, void* stream);
int unet_op_upconv2x2_x3(int device, const float* x_dev, int n, int h, int w, int cin, const float* w_host,
                         const float* bias_host, int cout, float* y_dev, void* stream);

/* The split-operand tier's operators on planes (test entry points, tests/test_x3_ops_gpu.py; the network runs the same
 * packing, dispatch and kernels).  An activation tensor is a caller-owned pair of fp16 NHWC planes (uint16 bit patterns):
 * the hi plane at the pointer, the lo plane `*_lo_off` elements behind it (a multiple of 8); the tensor stands for
 * hi + lo.  Weights, scale / shift, bias, head weights and activation scales are fp32 HOST arrays, packed and folded by the
 * functions the network's build uses.  ldo: pixel stride of y in elements (0 = cout), co_off: the first channel written
 * (multiples of 64, co_off + cout <= ldo); nothing outside those channels is touched.  range_out (optional int) receives
 * 1 if a kernel of the call reported a value outside the fp16 range (word 1 of an error block of the call's own), else 0.
 *
 * 3x3 convolution through the network's dispatch: x (N,H,W,cin) -> y channels [co_off, co_off + cout) of (N,H,W,ldo) =
 * out_act * relu?(conv3x3(x / in_act, w) * scale + shift).  tile_width as unet_op_conv3x3_x3 (not 428 / 414).  in_act
 * (cin) / out_act (cout): optional per-channel power-of-two activation scales.  split_k != 0: the call gets the split-K
 * scratch the forward hands over, so small maps run as partial sums + the finish kernel.  pool (optional): the 2x2
 * max-pool (N,H/2,W/2,cout), dense.  head_w_host (optional, cout == 64; y may then be NULL): the fused 1x1 head,
 * logits / probs (N,H,W) fp32 and mask uint8 = 255 where logit > head_thr, each optional.
 * path_out (optional int[8]): {structure (1 conv_x3_ws.h, 2 conv_x3_r512.h, 3 conv_x3_t448.h), pixel-tile width, epilogue
 * (0 planes, 1 planes + fused pool, 2 fused head), batch tiled as one tall image, kSplit (1 = no split-K), waves along the
 * pixels (structure 2) or channels (structure 3), pooled copy written by the separate pooling pass, 0}. */
int unet_op_conv3x3_x3_planes(int device, const uint16_t* x_dev, size_t x_lo_off, int n, int h, int w, int cin,
                              const float* w_host, const float* scale_host, const float* shift_host, int cout, int relu,
                              int tile_width, const float* in_act_host, const float* out_act_host, int split_k,
                              uint16_t* y_dev, size_t y_lo_off, int ldo, int co_off, uint16_t* pool_dev, size_t pool_lo_off,
                              const float* head_w_host, float head_bias, float head_thr, float* logits_dev,
                              float* probs_dev, uint8_t* mask_dev, int* path_out, int* range_out, void* stream);
/* ConvTranspose2d k=2 s=2 with bias: x (N,H,W,cin) -> y channels [co_off, co_off + cout) of (N,2H,2W,ldo); w_host
 * (cin,cout,2,2).  path_out (optional int[8]): {structure (1 upconv_x3_ws.h, 2 upconv_x3_r512.h, see
 * unet_set_x3_upconv_r512), 0, 0, 0, 1, work items per (a,b) split of structure 1, 0, 0}. */
int unet_op_upconv2x2_x3_planes(int device, const uint16_t* x_dev, size_t x_lo_off, int n, int h, int w, int cin,
                                const float* w_host, const float* bias_host, int cout, const float* in_act_host,
                                uint16_t* y_dev, size_t y_lo_off, int ldo, int co_off, int* path_out, int* range_out,
                                void* stream);
/* The first convolution: is_u8 != 0: uint8 (N,H,W,3) frames, normalised with mean_host / std_host (3 floats each);
 * else fp32 (N,3,H,W), already normalised -> y channels [0, cout) of (N,H,W,ldo); w_host (cout,3,3,3). */
int unet_op_conv_first_x3_planes(int device, const void* input_dev, int is_u8, int n, int h, int w, const float* w_host,
                                 const float* scale_host, const float* shift_host, int cout, int relu,
                                 const float* mean_host, const float* std_host, const float* out_act_host, uint16_t* y_dev,
                                 size_t y_lo_off, int ldo, int* range_out, void* stream);
/* MaxPool2d(2,2) on planes: channels [0, c) of x (N,H,W,ldi) -> dense y (N,H/2,W/2,c); c, ldi even (ldi 0 = c). */
int unet_op_maxpool2x2_x3_planes(int device, const uint16_t* x_dev, size_t x_lo_off, int n, int h, int w, int c, int ldi,
                                 uint16_t* y_dev, size_t y_lo_off, void* stream);
/* The unfused 1x1 head on dense planes (N,H,W,c): logits / probs / mask as unet_op_conv3x3_x3_planes. */
int unet_op_head1x1_x3_planes(int device, const uint16_t* x_dev, size_t x_lo_off, int n, int h, int w, int c,
                              const float* w_host, float bias, float thr, float* logits_dev, float* probs_dev,
                              uint8_t* mask_dev, void* stream);
/* fp32 -> planes: `count` (even) values, clamped to +-65504, hi = rn(v), lo = rn(v - hi). */
int unet_op_split_planes_x3(int device, const float* x_dev, size_t count, uint16_t* y_dev, size_t y_lo_off, int* range_out,
                            void* stream);

/* The bf16 tier's operators, one at a time (test entry points; the network runs the same packing, dispatch and kernels).
 * Activations are dense bf16 NHWC device tensors (uint16 bit patterns); weights, scale / shift, bias and head weights are
 * fp32 HOST arrays in PyTorch layout, packed internally by the functions the network's build uses.  cin, cout: multiples
 * of 32.  kernel: 0 = what the network picks for this shape under the current unet_set_bf16_persistent mode; 1 = the
 * 2x2-wave kernel (csrc/igemm_bf16.h); 2 = the wave-specialised kernel (csrc/conv_bf16_ws.h / csrc/upconv_bf16_ws.h);
 * 3 = the one-wave-per-SIMD kernel (csrc/conv_bf16_r512.h / csrc/upconv_bf16_r512.h).  A forced kernel that cannot take
 * the shape returns UNET_ERR_INVALID_ARG without launching anything.  path_out (optional, int[3]) receives {kernel that
 * ran (0 = none), 2x2 max-pool fused, 1x1 head fused}.  ldo: pixel stride of y in elements (0 = cout), co_off: the first
 * channel written (multiples of 32); channels outside [co_off, co_off + cout) are not touched.
 *
 * y = relu?(conv3x3(x, w) * scale + shift) rounded to bf16: x (N,H,W,cin) -> y (N,H,W,ldo); w_host (cout,cin,3,3);
 * y_pool (optional, dense (N,H/2,W/2,cout)): MaxPool2d(2,2) of y, written only where the kernel fuses it (path_out[1]). */
int unet_op_conv3x3_bf16(int device, const uint16_t* x_dev, int n, int h, int w, int cin, const float* w_host,
                         const float* scale_host, const float* shift_host, int cout, int relu, int kernel, int ldo,
                         int co_off, uint16_t* y_dev, uint16_t* y_pool_dev, int* path_out, void* stream);
/* The network's last convolution with the 1x1 head (cout -> 1, bias) fused into its epilogue where the kernel allows it
 * (path_out[2]); otherwise the activation is stored and the unfused head kernel runs, as in the forward.
 * logits / probs (N,H,W) fp32, mask (N,H,W) uint8 = 255 where logit > thr; each optional. */
int unet_op_conv3x3_bf16_head(int device, const uint16_t* x_dev, int n, int h, int w, int cin, const float* w_host,
                              const float* scale_host, const float* shift_host, int cout, int relu, int kernel,
                              const float* head_w_host, float head_bias, float thr, float* logits_dev, float* probs_dev,
                              uint8_t* mask_dev, int* path_out, void* stream);
/* ConvTranspose2d k=2 s=2 with bias: x (N,H,W,cin) -> y (N,2H,2W,ldo), channels [co_off, co_off + cout);
 * w_host (cin,cout,2,2). */
int unet_op_upconv2x2_bf16(int device, const uint16_t* x_dev, int n, int h, int w, int cin, const float* w_host,
                           const float* bias_host, int cout, int kernel, int ldo, int co_off, uint16_t* y_dev, int* path_out,
                           void* stream);
/* The first convolution: uint8 (N,H,W,3) frames -> (x - mean) / std -> 3x3 conv -> scale / shift (+ ReLU) -> dense
 * (N,H,W,cout) bf16.  mean_host / std_host: 3 floats each.  kernel: 0 = the forward's choice, 1 = csrc/conv_first_bf16x3.h
 * (H % 8 == 0, cout % 64 == 0), 2 = the fp32 kernel with a bf16 store. */
int unet_op_conv_first_bf16(int device, const uint8_t* frames_dev, int n, int h, int w, const float* w_host,
                            const float* scale_host, const float* shift_host, int cout, int relu, const float* mean_host,
                            const float* std_host, int kernel, uint16_t* y_dev, int* path_out, void* stream);
/* MaxPool2d(2,2) on bf16: x (N,H,W,ldi) channels [0,c) -> dense y (N,H/2,W/2,c); c, ldi multiples of 8 (ldi 0 = c). */
int unet_op_maxpool2x2_bf16(int device, const uint16_t* x_dev, int n, int h, int w, int c, int ldi, uint16_t* y_dev,
                            void* stream);
/* The unfused 1x1 head on dense bf16 (N,H,W,c) (c % 8 == 0): logits / probs / mask as unet_op_conv3x3_bf16_head. */
int unet_op_head1x1_bf16(int device, const uint16_t* x_dev, int n, int h, int w, int c, const float* w_host, float bias,
                         float thr, float* logits_dev, float* probs_dev, uint8_t* mask_dev, void* stream);

/* The exact-fp32 tier's operators on the paths the network runs (test entry points, tests/test_f32_ops_gpu.py; the
 * network runs the same packing, dispatch and kernels: csrc/igemm_f32.h, csrc/wino_f32.h, csrc/elementwise.h).
 * Activations are fp32 NHWC device tensors; weights, scale / shift and bias are fp32 HOST arrays in PyTorch layout.  cin,
 * cout: multiples of 4.  ldo: pixel stride of y in floats (0 = cout, dense), co_off: the first channel written; both
 * multiples of 4, co_off + cout <= ldo; channels outside [co_off, co_off + cout) are not touched.
 * path_out (optional int[8]) receives {algorithm that ran (1 direct, 2 Winograd), MS, NS, TH, TW (Winograd: 0, 0, THt,
 * TWt), grid blocks, coGroup, pool fused}.  The entry points that can launch the Winograd kernel read the device error
 * word back after the stream is synchronised: a bounded wave-progress wait that gave up is UNET_ERR_HIP (and says so in
 * unet_op_last_error); this holds for unet_op_conv3x3 as well.
 *
 * y = relu?(conv3x3(x, w) * scale + shift): x (N,H,W,cin) -> y (N,H,W,ldo); w_host (cout,cin,3,3).  algo: 0 = what the
 * forward picks (Winograd where cin % 16 == 0 and H, W are even, unless unet_set_winograd(0)), 1 = direct, 2 = Winograd;
 * a forced Winograd on a shape it does not take is UNET_ERR_INVALID_ARG and launches nothing.  y_pool (optional, H and
 * W even): dense (N,H/2,W/2,cout) MaxPool2d(2,2) of y - written from the output registers by the Winograd kernel, by the
 * pooling kernel reading y with pixel stride ldo after the direct kernel, as the forward's encoder does. */
int unet_op_conv3x3_f32(int device, const float* x_dev, int n, int h, int w, int cin, const float* w_host,
                        const float* scale_host, const float* shift_host, int cout, int relu, int algo, int ldo, int co_off,
                        float* y_dev, float* y_pool_dev, int* path_out, void* stream);
/* ConvTranspose2d k=2 s=2 with bias: x (N,H,W,cin) -> y (N,2H,2W,ldo), channels [co_off, co_off + cout);
 * w_host (cin,cout,2,2). */
int unet_op_upconv2x2_f32(int device, const float* x_dev, int n, int h, int w, int cin, const float* w_host,
                          const float* bias_host, int cout, int ldo, int co_off, float* y_dev, int* path_out, void* stream);
/* Plain 1x1 convolution (the training step's input gradient of the transposed convolution): w_host (cout,cin). */
int unet_op_conv1x1_f32(int device, const float* x_dev, int n, int h, int w, int cin, const float* w_host, int cout, int ldo,
                        int co_off, float* y_dev, int* path_out, void* stream);
/* MaxPool2d(2,2): channels [0, c) of x (N,H,W,ldi) -> dense y (N,H/2,W/2,c); c, ldi multiples of 4 (ldi 0 = c). */
int unet_op_maxpool2x2_f32(int device, const float* x_dev, int n, int h, int w, int c, int ldi, float* y_dev, void* stream);
/* The 1x1 head on dense (N,H,W,c): logits / probs (N,H,W) fp32, mask (N,H,W) uint8 = 255 where logit > thr; each
 * optional, at least one. */
int unet_op_head1x1_f32(int device, const float* x_dev, int n, int h, int w, int c, const float* w_host, float bias,
                        float thr, float* logits_dev, float* probs_dev, uint8_t* mask_dev, void* stream);
/* The input packers: is_u8 != 0: uint8 (N,H,W,3) frames -> (u8 - mean) / std; else fp32 (N,3,H,W) copied -> y (N,H,W,4)
 * fp32 with pad channel +0.0.  mean_host / std_host: 3 floats each (u8 only). */
int unet_op_pack_input_f32(int device, const void* src_dev, int is_u8, int n, int h, int w, const float* mean_host,
                           const float* std_host, float* y_dev, void* stream);
/* Test hook, host arithmetic only (no device call): the launch the fp32 tier makes for query[7] = {taps (9 = 3x3 conv,
 * 1 = transposed conv, 2 = plain 1x1), n, h, w, cin, cout, algo (as unet_op_conv3x3_f32; taps 9 only)} -> plan_out[8], the
 * fields of path_out (pool fused = 0).  The same functions decide the launches themselves. */
int unet_host_plan_conv_f32(const int* query, int n_query, int* plan_out, int n_plan);

/* One decoder step of the split-operand tier - ConvTranspose2d(2f -> f, k2, s2, bias) -> cat([skip, up]) ->
 * Conv3x3(2f -> f) -> scale/shift (+ ReLU) (reference README.md:1476-1479) - as the composed operator
 * (csrc/conv_x3_dec.h: the transposed convolution folded into the 3x3 convolution's up half on the host, float64).
 * skip (N,H,W,f) and x (N,H/2,W/2,2f) fp32 NHWC -> y (N,H,W,f); w_t (2f,f,2,2), b_t (f), w3 (f,2f,3,3), scale / shift (f)
 * on the host.  f 64, 128, 192 or 256 (more than 128: several channel groups per pixel tile, which the forward does not
 * use), W % 28 == 0, H even; UNET_ERR_INVALID_ARG otherwise.  Runs the block tile unet_set_x3_dec_form selects.  Not
 * bit-identical to the two-kernel path (a different summation). */
int unet_op_upcat_conv3x3_x3(int device, const float* skip_dev, const float* x_dev, int n, int h, int w, int f,
                             const float* wt_host, const float* bt_host, const float* w3_host, const float* scale_host,
                             const float* shift_host, int relu, float* y_dev, void* stream);
/* Test hook, host arithmetic only: the float64 composition behind unet_op_upcat_conv3x3_x3.  wp_out [4][f][2f][2][2]:
 * for output parity (a, b) = (p >> 1, p & 1) the 2 x 2 taps over x rows i + a - 1 + {0, 1}, columns j + b - 1 + {0, 1};
 * bias_out [9][f]: the transposed convolution's bias through the 3x3 up half for border class 3 * row class + column
 * class (0 = first row / column of the image, 1 = interior, 2 = last). */
int unet_host_compose_upcat(const float* wt_host, const float* bt_host, const float* w3_host, int f, double* wp_out,
                            double* bias_out);
/* Test hooks, host arithmetic only (no device is initialised): the plan the f16x3 dispatch makes (csrc/unet_x3.inc,
 * x3_plan_conv / x3_plan_upconv; DESIGN.md, "f16x3 dispatch").  Everything the decision depends on is in the query, the
 * A/B switches included, so the answer does not depend on the caller's environment.
 * 3x3 convolution, query[22]: n, h, w, cin, cout, epilogue asked for (0 planes, 1 planes + pooled copy, 2 fused head,
 *   3 fp32), tile_width, co_off, split-K scratch present, its size in floats, q-plane scratch present, fp8 fragments packed,
 *   in_is_q, want_out_q, pool_src_q, pool_dst_q, BatchNorm statistics wanted, then the switches UNET_X3_FLAT, UNET_X3_R512,
 *   UNET_X3_T448, UNET_X3_T448_C4 (1 = on, the default) and unet_set_x3_cross_fp8's mode.
 *   plan_out[24]: the seven ints of path_out; grid; rows of fused statistics (0 = none); planes_to_q8 pass first; pooling
 *   pass behind (0 none, 1 planes, 2 q8); split-K finish pass behind; the output's q plane written; valid (0: the forced
 *   form does not fit or a q-plane input meets another form - everything else is then 0); N, H, imgH, tilesX, tilesY,
 *   pixTiles, coTiles, coGroup, nChunks, kSplit as the kernel gets them.
 * Transposed convolution, query[9]: n, h, w, cin, cout, co_off, want_out_q, unet_set_x3_upconv_r512's mode, 1 = the plain
 *   GEMM of the backward pass on the same kernels (cin = K, cout = columns).  plan_out[16]: the first fourteen as above
 *   (path waves = the (a,b) split), then pixTiles, coTiles.
 * label_out (optional, label_cap >= 48): the profiler label of the plan's main kernel ("" where the caller names it).
 * UNET_ERR_INVALID_ARG: a wrong array size, a non-positive shape or a tile_width outside the table. */
int unet_host_plan_conv3x3_x3(const int* query, int n_query, int* plan_out, int n_plan, char* label_out, int label_cap);
int unet_host_plan_upconv2x2_x3(const int* query, int n_query, int* plan_out, int n_plan, char* label_out, int label_cap);
/* The same for one decoder step ConvTranspose2d -> cat -> Conv3x3 (x3_plan_dec_step): which form it runs in.
 * query[17]: n, h, w (the LOW-resolution map of x), f, unet_set_x3_compose's mode, unet_set_x3_compose_deep's switch,
 *   unet_set_x3_dec_form's mode, f16q8 scratch present, who asks (0 the forward, 1 an operator entry point, which forces
 *   its operator), the operators the asker holds (bit 0 composed, bit 1 deep: the forward 3, an entry point the one it
 *   built; the plan intersects it with those a step of width f can have), 1 = kernel 1 of the deep form alone (entry
 *   point), unet_set_x3_upconv_r512's mode (read by the two-kernel form's labels only), then the four switches and
 *   unet_set_x3_cross_fp8's mode as above.
 *   plan_out[16]: form (0 two kernels, 1 composed, 2 deep); composed: wco (64-channel tiles per block), tilesX, tilesY,
 *   pixTiles, coTiles, grid; [7] the launches of a composed / deep step; [8..15] deep: the eight ints of
 *   unet_host_plan_updeep_x3.  Whatever does not belong to the form is 0.
 * label_out (optional, label_cap >= 128): the profiler labels of the step's launches up to its second convolution, comma-
 *   separated; two kernels: those of the transposed and the first convolution as the forward launches them while no q
 *   plane is handed on, a split-K finish pass included. */
int unet_host_plan_dec_step_x3(const int* query, int n_query, int* plan_out, int n_plan, char* label_out, int label_cap);
/* Test hook, host arithmetic only: the packed fp16 hi / lo fragments of host weights times pre_host[cout] (powers of two),
 * as the operators upload them.  kind 0: 3x3 convolution, w (cout,cin,3,3) -> [cout/64][cin/32][tap row 3][plane 2][kx 3]
 * [cs 4][lane 64][8]; 1: transposed convolution, w (cin,cout,2,2) -> [cout/64][cin/32][plane 2][ab 4][cs 4][lane 64][8];
 * 2: first convolution, w (cout,3,3,3), cin = 3 -> [cout/64][cs 4][plane 2][lane 64][8] with k = tap * 3 + ci, k >= 27
 * zero; 3: composed decoder step, w = the skip half (f,f,3,3), wx_host = the window weights [parity 4][f][2f][tap 4],
 * cout = f, cin = 2f -> per 64-channel tile [f/32][tap 9][plane 2][cs 4][lane 64][8] then [2f/32][parity 4][tap 4][plane 2]
 * [cs 4][lane 64][8].  In every layout row j = lane & 15 of subtile cs of tile ct is channel 64 ct + 16 (j >> 2) + 4 cs +
 * (j & 3) and the lane's eight halfs are k = 32 chunk + 8 (lane >> 4) + e.  n_packed: the pack's size in halfs (checked). */
int unet_host_pack_x3(int kind, const float* w_host, const float* wx_host, int cout, int cin, const float* pre_host,
                      uint16_t* packed_out, size_t n_packed);
/* Process-wide switch for the composed decoder step in the f16x3 tier's forward (not the f16q8 tier, not training):
 * -1 = automatic (default) - the levels with f <= 128 on maps of width 28k with a work item for half of the CUs;
 * 0 = off: ConvTranspose2d + the 3x3 convolution as two kernels everywhere; 1 = wherever the shape rules allow.
 * Environment UNET_X3_COMPOSE=0 sets the initial value to 0.  A captured HIP graph keeps the setting it was captured
 * with.  Returns the previous setting. */
int unet_set_x3_compose(int mode);
/* Process-wide switch for the block tile of the composed decoder step (csrc/conv_x3_dec.h): -1 = automatic (default),
 * 1 = the 64-channel form everywhere, 2 = the 128-channel form wherever f % 128 == 0 (the 64-channel form elsewhere).
 * The two forms give bit-identical results (tests/test_x3_dec_forms_gpu.py).  Environment UNET_X3_DEC_FORM=1 or 2 sets
 * the initial value.  A captured HIP graph keeps the setting it was captured with.  Returns the previous setting. */
int unet_set_x3_dec_form(int mode);
/* Process-wide switch for the split form of the decoder step on the levels with f % 256 == 0 and a low-resolution map at
 * most 28 wide (csrc/upconv_x3_win.h + the addend epilogue of csrc/conv_x3_t448.h; DESIGN.md, "The decoder's composed
 * first convolution"): 1 = on (default; environment UNET_X3_COMPOSE_DEEP=0 makes it 0), 0 = those levels keep the
 * two-kernel path.  unet_set_x3_compose(0) turns it off together with the composed operator; unet_set_x3_compose(1) lifts
 * its work-item rule as well.  Returns the previous setting. */
int unet_set_x3_compose_deep(int on);
/* The two launches of that step on caller-owned planes (layouts as in "The split-operand tier's operators on planes").
 * wt_host (2f,f,2,2), bt_host (f), w3_host (f,2f,3,3); h, w: the low-resolution map of x, 4 <= w <= 28.
 * unet_op_updeep_window_x3_planes: kernel 1 alone.  x (N,h,w,2f) -> P, the up half of the 3x3 convolution with the
 *   border-class constants, into channels [co_off, co_off + f) of y (N,2h,2w,ldo); f a multiple of 64; in_act_host (2f)
 *   or NULL.
 * unet_op_updeep_conv3x3_x3_planes: both kernels.  cat (N,2h,2w,2f): the skip in channels [0,f) (read only), P is
 *   written to channels [f,2f); out (N,2h,2w,f) = relu?((conv3x3(skip) + P) scale + shift); f a multiple of 256;
 *   x_act_host (2f) / skip_act_host (f) or NULL.
 * UNET_ERR_INVALID_ARG for a shape neither kernel takes. */
int unet_op_updeep_window_x3_planes(int device, const uint16_t* x_dev, size_t x_lo_off, int n, int h, int w, int f,
                                    const float* wt_host, const float* bt_host, const float* w3_host,
                                    const float* in_act_host, uint16_t* y_dev, size_t y_lo_off, int ldo, int co_off,
                                    int* range_out, void* stream);
int unet_op_updeep_conv3x3_x3_planes(int device, const uint16_t* x_dev, size_t x_lo_off, int n, int h, int w, int f,
                                     const float* wt_host, const float* bt_host, const float* w3_host,
                                     const float* scale_host, const float* shift_host, int relu, const float* x_act_host,
                                     const float* skip_act_host, uint16_t* cat_dev, size_t cat_lo_off, uint16_t* out_dev,
                                     size_t out_lo_off, int* range_out, void* stream);
/* Test hooks, host arithmetic only.  unet_host_pack_updeep_x3: what kernel 1 is given - ordered_out: the float64 window
 * weights at the hi-plane positions of the pack [f/64][2f/32][tap = di * 2 + dj][plane 2][parity 4][cs 4][lane 64][8]
 * (row j = lane & 15 of subtile cs is channel 64 ct + 16 (j >> 2) + 4 cs + (j & 3), input channel 32 kc + 8 (lane >> 4)
 * + e), packed_out: the fp16 hi / lo planes of weight / x_act * pre, pre_out [f], cls_out [9][f] in float64 (the kernel
 * is given them rounded to fp32).
 * unet_host_plan_updeep_x3: query[7] = n, h, w, f, compose mode, deep switch, f16q8 on -> plan_out[8] = taken, kernel 1's
 * widest map / pixel tiles / channel tiles / grid, kernel 2's grid / flat tiling / pixel tiles (all 0: declined). */
int unet_host_pack_updeep_x3(const float* wt_host, const float* bt_host, const float* w3_host, int f, const float* x_act_host,
                             double* ordered_out, uint16_t* packed_out, float* pre_out, double* cls_out);
int unet_host_plan_updeep_x3(const int* query, int n_query, int* plan_out, int n_plan);

/* The first encoder block of the f16x3 tier as ONE kernel (csrc/conv_x3_enc1.h): enc1.conv1 is computed
 * per work item into the LDS halo image that enc1.conv2's 64-channel third-structure form reads, so the 64-channel tensor
 * between them is never stored.  Bit-identical to the two launches it replaces (tests/test_x3_enc1_gpu.py).
 * unet_set_x3_fuse_first: process-wide switch, 1 = on (default; environment UNET_X3_FUSE_FIRST=0 makes it 0), 0 = the
 *   block keeps its two launches.  A captured HIP graph keeps the setting it was captured with.  Returns the previous
 *   setting.
 * unet_host_plan_enc1_x3 (test hook, host arithmetic only): x3_plan_enc1.  query[13]: input is uint8, n, h, w, cout of
 *   the block, forced form of the second convolution (tile_width as unet_op_conv3x3_x3; 0 = none, as the forward asks),
 *   f16q8 scratch present, unet_set_x3_fuse_first's switch, then the four switches and unet_set_x3_cross_fp8's mode as
 *   for unet_host_plan_conv3x3_x3.  The plan takes the block exactly when the input is uint8, cout == 64, w % 28 == 0,
 *   no f16q8 scratch, the switch is on and unet_host_plan_conv3x3_x3's own answer for the second convolution (64 -> 64,
 *   pooled epilogue) is structure 3 on 28-wide tiles with one wave along the channels, the fused pool, no split-K and no
 *   tall-image tiling.  plan_out[8]: taken, grid, tiles along x, tiles along y, pixel tiles, 0, 0, 0 (all 0: declined).
 * unet_op_enc1_x3_planes (test entry point): frames (N,H,W,3) uint8 -> y channels [co_off, co_off + 64) of (N,H,W,ldo)
 *   and pool (N,H/2,W/2,64) dense, both as hi / lo planes, = the block's two convolutions + folded BN + ReLU with
 *   operators built by the functions the network's build uses.  w1_host (64,3,3,3), w2_host (64,64,3,3); act1_host /
 *   act2_host (64 each, optional): power-of-two activation scales of the two layers' outputs.  tile_width: the forced
 *   form of the second convolution (0 or 628); UNET_ERR_INVALID_ARG where the plan declines.  path_out (optional
 *   int[8]): the second convolution's path as unet_op_conv3x3_x3_planes reports it, [7] = 1: the fused kernel ran. */
int unet_set_x3_fuse_first(int on);
int unet_host_plan_enc1_x3(const int* query, int n_query, int* plan_out, int n_plan);
int unet_op_enc1_x3_planes(int device, const void* frames_dev, int n, int h, int w, const float* w1_host,
                           const float* scale1_host, const float* shift1_host, int relu1, const float* mean_host,
                           const float* std_host, const float* act1_host, const float* w2_host, const float* scale2_host,
                           const float* shift2_host, int relu2, const float* act2_host, int tile_width, uint16_t* y_dev,
                           size_t y_lo_off, int ldo, int co_off, uint16_t* pool_dev, size_t pool_lo_off, int* path_out,
                           int* range_out, void* stream);

/* Which kernel structure the split-operand tier's ConvTranspose2d (and the plain GEMMs of its training path) run on
 * (reference README.md:1442, :1476): -1 = automatic - the one-wave-per-SIMD kernel (csrc/upconv_x3_r512.h: 224-pixel
 * tiles, weights straight from L2) where Cin % 128 == 0 and there is a work item for at least half of the CUs, the
 * wave-specialised kernel (csrc/upconv_x3_ws.h) otherwise; 0 = the wave-specialised kernel only; 1 = the
 * one-wave-per-SIMD kernel whenever Cin % 128 == 0.  Both accumulate chunk by chunk in the same order and give
 * bit-identical results (tests/test_x3_gpu.py).  Returns the previous setting. */
int unet_set_x3_upconv_r512(int mode);

/* "f16q8": the split-operand tier with the two cross terms of every product (w_lo x_hi + w_hi x_lo, 2^-11 of the product)
 * formed on the fp8 matrix pipe (csrc/conv_q8_r512.h) in the 3x3 convolutions that suit it (Cin % 64 == 0,
 * Cout % 256 == 0, map width a multiple of 28 or 14, a work item for half of the CUs); the main term stays fp16 and
 * every other layer runs as in the f16x3 tier.  An accuracy tier of its own: logits within BASELINE.json's 1e-3 of the
 * reference's (measured on an MI355X, batch 256: 7.8e-4 against the reference's golden logits, 9.2e-4 against the f16x3
 * tier over 256 random frames - a 1.2x margin; binary masks differ from the f16x3 tier's in ~7 pixels per million, all at
 * logits within 1e-3 of zero), not the 2e-4 the f16x3 tier is held to (reference README.md:1449-1458 is plain fp32).
 * 0 = off (default), 1 = on for the following unet_forward_*_x3 calls of the CALLING THREAD (the switch is thread-local, so
 * a caller that sets it around one forward and restores it - UNetHIP.run_u8(precision="f16q8") - cannot change what another
 * thread's forward computes); the first call after switching it on rebuilds the handle's operators with the extra weight
 * fragments (it synchronises the device: do not mix with HIP graphs captured from the same handle).  Returns the previous
 * setting.
 * unet_op_conv3x3_x3 runs the kernel directly through the f16q8 forced forms of its tile_width. */
int unet_set_x3_cross_fp8(int mode);

/* Debug aid: during the next unet_train_forward_backward_* calls copy one internal buffer to dst_dev
 * (at most max_floats).  stage = 100+j: gradient w.r.t. the input of decoder step j's ConvTranspose2d;
 * 200+j: its space-to-depth gradient; 300+u / 400+u / 500+u: dZ, z and the saved BatchNorm statistics
 * of conv unit u (encoder, bottleneck, decoder order); -1 disables. */
int unet_train_debug_snapshot(unet_handle_t h, int stage, float* dst_dev, size_t max_floats);

/* Test entry for the general loss (mode 2 only; parameters checked as by unet_train_set_loss_cfg): what `criterion(pred,
 * masks)` and `total_loss.backward()` leave for the logits (README.md:1904-1906) - loss_terms_dev[0..3] = {total, bce,
 * dice, focal}, dlogits_dev = dL/dlogits - through the launch sequence the training step runs.  Any numel > 0; 128-bit
 * accesses where the three buffers are 16-byte aligned.  Two runs on the same inputs give the same bits. */
int unet_op_loss_grad(int device, const float* logits_dev, const float* targets_dev, size_t numel,
                      const unet_loss_config* cfg, float* loss_terms_dev, float* dlogits_dev, void* stream);

/* dW of a 3x3 convolution (training backward): dz (N,H,W,Cout), x (N,H,W,Cin) -> dw_dev (Cout,Cin,3,3). */
int unet_op_wgrad3x3(int device, const float* dz_dev, const float* x_dev, int n, int h, int w, int cin, int cout,
                     float* dw_dev, void* stream);
/* The same weight gradient on the split-operand fp16 kernel (every fp32 operand as fp16 hi + lo, three MFMAs per
 * product, pixels as the GEMM's K dimension through transposed LDS reads); cin, cout multiples of 64, h even.
 * scaled != 0: dz is brought into the fp16 range by a power of two first, as the training step does for gradients
 * (`loss.backward()` of README.md:2077 computes these sums in fp32). */
int unet_op_wgrad3x3_x3(int device, const float* dz_dev, const float* x_dev, int n, int h, int w, int cin, int cout,
                        float* dw_dev, int scaled, void* stream);

/* ---- The training step's f16x3 operators (test entry points) ---------------------------------------------------------
 * The MFMA operators of the training step on the launch sequences the step itself runs (the same run_* helpers), with
 * what feeds them: the device-side weight packers (fp32 device weights in PyTorch layout, as in the flat parameter
 * buffer; no pre-scaling), the power-of-two operand scaling of gradients and the fp32 epilogues.  Every call owns its
 * scratch, keys and range word, synchronises the stream before it returns and writes nothing outside the outputs named
 * here.  UNET_ERR_INVALID_ARG for what it cannot run (checked before a device is touched, except for a forced tile
 * width the shape does not fit).
 *
 * 3x3 convolution with fp32 output, y[p][off + co] (pixel stride ldo, 0 = cout; ldo, off multiples of 64).  cin / cout
 * are the channel counts of the convolution that runs (multiples of 64, <= 1024).  mode 0: the forward operator,
 * w_dev (cout, cin, 3, 3); mode 1: the input-gradient operator of the forward convolution whose weight w_dev
 * (cin, cout, 3, 3) is: channels swapped, taps flipped.  packer 0: pack_x3_kernel, 1: pack_x3_lds_multi_kernel (w_dev
 * 16-byte aligned).  Input: either x_planes (fp16 hi plane, the lo plane directly behind it: N*H*W*cin halfs each), or
 * x_f32 (N,H,W,cin) which the call splits - with scaled != 0 after scaling by the power of two that brings max |x| into
 * [2^13, 2^14) (absmax_key_kernel, split_planes_scaled_kernel), undone in the epilogue; *inv_out is 2^-k (1 unscaled).
 * tile_width / path_out (8 ints) as unet_op_conv3x3_x3_planes.  stat_partial_dev (optional, stat_cap_rows x 2 x cout
 * floats): handed to the epilogue as the step hands it its reduction scratch; it receives the raw rows [row][2][cout] of
 * per-channel sum / sum of squares and *stat_rows_out their count - 0 and the buffer untouched where the structure that
 * ran does not fuse them.  The grid is only known inside the dispatch, so the capacity must cover its largest (256
 * blocks x 4 rows = 1024 rows); less is UNET_ERR_INVALID_ARG with 1024 reported, before a device is touched. */
int unet_op_train_conv3x3_x3(int device, const uint16_t* x_planes, const float* x_f32, int scaled, int n, int h, int w,
                             int cin, int cout, const float* w_dev, int mode, int packer, int tile_width, float* y_dev,
                             int ldo, int off, float* stat_partial_dev, int stat_cap_rows, int* stat_rows_out,
                             float* inv_out, int* path_out, int* range_out, void* stream);
/* ConvTranspose2d(2f -> f, k2 s2) backward as the step runs it on the f16x3 kernels: dy_dev is the fp32 gradient
 * (N, 2h, 2w, ldd), f channels at offset offd (multiples of 4); in_planes the transposed convolution's input (N,h,w,2f)
 * as fp16 hi plane + lo plane directly behind; w_dev (2f, f, 2, 2).  Column sum + maximum, space-to-depth into scaled
 * operand planes, the 1x1 weight gradient and the input-gradient GEMM.  -> db_dev (f), dw_dev (2f, f, 2, 2), din_dev
 * (N,h,w,2f), *inv_out = 2^-k of the operand scaling, *structure_out = 1 (upconv_x3_ws.h) / 2 (upconv_x3_r512.h, see
 * unet_set_x3_upconv_r512) for the GEMM.  f a multiple of 64, <= 512. */
int unet_op_upconv_bwd_x3(int device, const float* dy_dev, int ldd, int offd, const uint16_t* in_planes,
                          const float* w_dev, int n, int h, int w, int f, float* db_dev, float* dw_dev, float* din_dev,
                          float* inv_out, int* structure_out, void* stream);
/* ConvTranspose2d forward of the training step: as unet_op_upconv2x2_x3_planes, but w_dev (cin, cout, 2, 2) and bias_dev
 * (cout) are fp32 device tensors and the operand comes from pack_upconv_x3_kernel (un-prescaled, unit scale). */
int unet_op_upconv_fwd_train_x3(int device, const uint16_t* x, size_t x_lo, int n, int h, int w, int cin,
                                const float* w_dev, const float* bias_dev, int cout, uint16_t* y, size_t y_lo, int ldo,
                                int co_off, int* path_out, int* range_out, void* stream);

/* ---- int8 tier of the deployed network ("model B") --------------------------------------
 * Stands in for the quantised .rknn blob behind rknn.inference (src/py_utils/rknn_executor.py:36): per-tensor
 * asymmetric int8 activations, per-output-channel asymmetric int8 weights as the reference configures its conversion
 * (README.md:3106-3116 `asymmetric_quantized-8` / `channel`; README.md:3370-3383), BatchNorm folded, sigmoid head, on
 * v_mfma_i32_16x16x64_i8.  The quantised model is a set of named arrays produced by unet_lane_detection_amd/quant.py
 * (int8 `<unit>.w_q`, int32 `<unit>.w_zp` / `.bias_q` / `.x_zp` / `.y_zp` / `.relu`, float32 `<unit>.mult`, the input
 * table `input.lut` int8[3][256] + `input.zp`; <unit> = the reference's state_dict prefixes such as
 * "encoder_blocks.0.0", "decoder_blocks.0", "output").  Integer-exact against oracle/int8_oracle.py; parity with the
 * Rockchip runtime itself is unpinned (its blobs cannot be executed here). */
typedef struct unet_i8_ctx* unet_i8_handle_t;
int unet_i8_create(int depth, const int* features, int device, unet_i8_handle_t* out);
int unet_i8_load(unet_i8_handle_t h, const char* name, const void* data_host, size_t bytes);
int unet_i8_finalize(unet_i8_handle_t h);
/* frames (N,H,W,3) uint8 as unet_forward_u8; logits = float32(int32 accumulator) * (x_scale * w_scale), probabilities
 * = sigmoid(logits) (what the blob's ConvSigmoid returns), mask as unet_forward_u8. */
int unet_i8_forward_u8(unet_i8_handle_t h, const uint8_t* frames_dev, int n, int height, int width, float* logits_dev,
                       float* probs_dev, uint8_t* mask_dev, float threshold_logit, void* stream);
/* Parity aid: copy one int8 activation tensor of the last forward to the host, dense NHWC with its real channels.
 * name: "im2col", "enc<l>.a", "cat<l>", "cat<l>.pool", "bott.a", "bott.b", "dec<j>.a", "dec<j>.b". */
int unet_i8_read_tensor(unet_i8_handle_t h, const char* name, int8_t* dst_host, size_t cap_bytes, int* channels);
/* Hybrid quantisation (README.md:3466-3474 "mixed precision"; unet_lane_detection_amd/quant.py states the arithmetic):
 * a unit whose arrays include `<unit>.hybrid` (int32 1) with `.w_h` (fp16 bits, shape of `.w_q`), `.gain`, `.bias_f`,
 * `.x_scale` (float32) and `.y_scale` runs on v_mfma_f32_16x16x32_f16 with fp32 accumulation; a tensor whose writers and
 * readers are all hybrid is stored as fp16, every other tensor stays int8 with its calibrated parameters.
 * unet_i8_set_hybrid(h, 0) before unet_i8_finalize runs the same arrays as pure int8 (1, the default, honours the marks).
 * unet_i8_tensor_dtype: 0 int8, 1 fp16, -1 unknown name or not finalized (names as unet_i8_read_tensor, plus "input").
 * unet_i8_read_tensor_f16 is unet_i8_read_tensor for fp16 tensors (fp16 bits out); each of the two returns
 * UNET_ERR_INVALID_ARG for a tensor of the other type. */
int unet_i8_set_hybrid(unet_i8_handle_t h, int on);
int unet_i8_tensor_dtype(unet_i8_handle_t h, const char* name);
int unet_i8_read_tensor_f16(unet_i8_handle_t h, const char* name, uint16_t* dst_host, size_t cap_bytes, int* channels);
/* K-class quantised models (csrc/i8_classes_kernels.h).  unet_i8_finalize takes the class count K from the entries of
 * `output.bias_q` (1 .. UNET_MAX_CLASSES) and requires `output.w_q` (K rows of features[0] weights), `output.w_zp` and
 * `output.mult` (K entries) - and for a hybrid head `output.w_h`, `.gain`, `.bias_f` - to agree with it: UNET_ERR_STATE
 * with a text for unet_i8_last_error otherwise, before any device is touched.  unet_i8_out_channels: K, 0 before the
 * first unet_i8_finalize.  A handle with K == 1 runs exactly what it ran before.
 *
 * unet_i8_forward_classes_u8: the forward of a handle with K >= 2.  Per pixel and class the single-class head's
 * arithmetic, logit_k = float32(int32 accumulator_k) * (x_scale * w_scale[k]), one IEEE multiplication (a hybrid head:
 * unet_lane_detection_amd/quant.py); every output is optional, at least one is required:
 *   logits_dev (N,K,H,W) fp32, probs_dev (N,K,H,W) = softmax over K          16-byte aligned
 *   labels_dev (N,H,W) uint8 = argmax, mask_dev (N,H,W) uint8 = 255 where the label is mask_class      4-byte aligned
 * with the tie and NaN rule of unet_forward_classes_u8.  With labels_dev or mask_dev alone the head writes one byte per
 * pixel.  UNET_ERR_INVALID_ARG with a text for a single-class handle, for no output at all, for mask_dev with mask_class
 * outside 0 .. K-1 and for a misaligned output; unet_i8_forward_u8 returns UNET_ERR_INVALID_ARG with a text for a handle
 * with K >= 2; all before any device is touched.
 *
 * unet_i8_run_head: the head alone on the last tensor of the handle's last forward (its n, height, width): the outputs
 * of unet_i8_forward_u8 for K == 1 (labels_dev, mask_class unused), those of unet_i8_forward_classes_u8 otherwise
 * (threshold_logit unused).  UNET_ERR_STATE when no forward has run since unet_i8_finalize. */
int unet_i8_out_channels(unet_i8_handle_t h);
int unet_i8_forward_classes_u8(unet_i8_handle_t h, const uint8_t* frames_dev, int n, int height, int width,
                               float* logits_dev, float* probs_dev, uint8_t* labels_dev, int mask_class, uint8_t* mask_dev,
                               void* stream);
int unet_i8_run_head(unet_i8_handle_t h, float* logits_dev, float* probs_dev, uint8_t* labels_dev, int mask_class,
                     uint8_t* mask_dev, float threshold_logit, void* stream);
int unet_i8_destroy(unet_i8_handle_t h);
const char* unet_i8_last_error(unet_i8_handle_t h);

/* Calibration pass on the FLOAT handle (README.md:3046-3078: min/max over calibration frames, algorithm 'normal'):
 * runs unet_forward_u8 and reports (min, max) of every activation tensor that carries quantisation parameters,
 * 2 floats per tensor in the order of quant.tensor_names(): input, per level {first encoder conv, concat tensor},
 * the two bottleneck convs, per decoder step its two convs.  Synchronises the stream. */
int unet_num_range_tensors(unet_handle_t h);
int unet_forward_u8_ranges(unet_handle_t h, const uint8_t* frames_dev, int n, int height, int width,
                           float* ranges_host, void* stream);
/* The same pass and the histogram pass below for a handle with out_channels >= 2 (UNET_ERR_INVALID_ARG with a text for a
 * single-class handle, as the two single-class entry points refuse a K-class one).  The range tensors are those of
 * quant.tensor_names() and none of them is the head's output: the record of a K-class model equals, bit for bit, that of
 * a single-class model with the same body. */
int unet_forward_classes_u8_ranges(unet_handle_t h, const uint8_t* frames_dev, int n, int height, int width,
                                   float* ranges_host, void* stream);
int unet_forward_classes_u8_histograms(unet_handle_t h, const uint8_t* frames_dev, int n, int height, int width,
                                       const float* spans_host, int bins, unsigned long long* hist_dev, void* stream);

/* Calibration beyond min/max (README.md:3407-3412 'mmse' / 'kl_divergence'): the distribution of every range tensor.
 * Binning rule (csrc/calib_kernels.cpp; quant.histogram_model restates it bit for bit): inv = float(bins) / (hi - lo)
 * in fp32; per element t = (v - lo) * inv, one fp32 subtraction and one fp32 multiplication; bin 0 for t < 0,
 * bins - 1 for t >= bins, else (int)t.  NaN is counted nowhere; an element equal to 0 is counted in no bin but in word
 * `bins`, so a histogram is bins + 1 64-bit words whose sum is the number of non-NaN elements.  bins: a power of two
 * from 64 to 4096.  The words are added to, never cleared.
 *
 * unet_op_histogram_f32: the kernel on its own (test entry point): x_dev is npix pixels of c channels at pixel stride
 * ld (floats).  UNET_ERR_INVALID_ARG for hi <= lo, a span that is not finite, unsupported bins, c > ld or null
 * pointers, before anything is launched.  Synchronises the stream.
 *
 * unet_forward_u8_histograms: the forward of unet_forward_u8_ranges with a histogram behind every layer instead:
 * spans_host holds (lo, hi) per tensor and hist_dev bins + 1 words per tensor, both in the order of
 * quant.tensor_names(); hist_dev accumulates across calls (clear it before the first).  Tensor 0, the input, is counted
 * over its 3 real channels.  No host synchronisation. */
int unet_op_histogram_f32(int device, const float* x_dev, size_t npix, int c, int ld, float lo, float hi, int bins,
                          unsigned long long* hist_dev, void* stream);
int unet_forward_u8_histograms(unet_handle_t h, const uint8_t* frames_dev, int n, int height, int width,
                               const float* spans_host, int bins, unsigned long long* hist_dev, void* stream);

/* The reference's acceptance check of a quantised model (README.md:3512-3565 `compare_outputs`): acc_dev[f] += the sum
 * over frame f of |pa - pb| for `frames` frames of per_frame floats each (probabilities of two tiers on the same
 * frames).  Every term is an fp32 value, the sums are float64 in a fixed order.  No host synchronisation. */
int unet_prob_mae_accumulate(int device, const float* pa_dev, const float* pb_dev, int frames, size_t per_frame,
                             double* acc_dev, void* stream);

/* ---- camera stage on the GPU ----------------------------------------------------
 * Replaces the OpenCV calls of the reference's ROS callback (src/unet_ros_node.py:296-311) and of
 * RKNNLaneInference.preprocess_image / postprocess_output (src/unet.py:33, :70).  Integer arithmetic restated from
 * OpenCV 4.x's 8-bit paths; parity against cv2 itself is unpinned (cv2 is not installed and the reference has no
 * fixture for this stage) - see oracle/camera_oracle.py.
 *
 * unet_ipm_prestage_u8: img_dev = the data field of a sensor_msgs/Image with encoding bgr8 (bgr_in = 1) or rgb8
 * (bgr_in = 0): `height` rows of `step` bytes.  Computes cv2.warpPerspective(img, M, (warp_w, warp_h)) [INTER_LINEAR,
 * constant border 0], the reference's same-size INTER_AREA resize (a copy), the conversion to RGB and
 * cv2.resize(.., (out_w, out_h)) [bilinear] in one pass; minv = M^-1 (row-major 3x3, destination -> source).
 * out_rgb_dev: (out_h, out_w, 3) uint8, ready for unet_forward_u8. */
int unet_ipm_prestage_u8(int device, const uint8_t* img_dev, int height, int width, int step, int bgr_in,
                         const double minv[9], int warp_w, int warp_h, int out_w, int out_h, uint8_t* out_rgb_dev,
                         void* stream);

/* cv2.resize(src, (out_w, out_h)) [bilinear] of an 8-bit image with `channels` interleaved channels: the mask's way
 * back to the warped size (src/unet.py:70). */
int unet_resize_u8(int device, const uint8_t* src_dev, int height, int width, int channels, int out_w, int out_h,
                   uint8_t* dst_dev, void* stream);

/* ---- training-time augmentation on the GPU ---------------------------------------------------------------------
 * The reference's train_transform (README.md:2035-2055, `get_transforms`): HorizontalFlip, Rotate,
 * RandomBrightnessContrast, HueSaturationValue and GaussianBlur of a batch gathered from a device-resident data set,
 * and the masks' targets (`mask > 127`, README.md:2022), in one launch.  The arithmetic is stated in
 * unet_lane_detection_amd/augment.py and reproduced bit for bit; parity against albumentations / cv2 themselves is
 * unpinned (neither is installed and the reference has no fixture for this stage).
 *
 * images_dev: (n_source, height, width, 3) uint8; masks_dev: (n_source, height, width) uint8, or NULL together with
 * targets_out_dev for images only.  params_dev: n_out records on the device, one per output sample, laid out as
 * augment.PARAMS_DTYPE (csrc/augment_kernels.h): source index, inverse affine, enable bits, colour parameters, blur
 * size.  images_out_dev: (n_out, height, width, 3) uint8; targets_out_dev: (n_out, 1, height, width) float 0/1.
 * The source index is clamped into [0, n_source) and every coordinate is folded into the frame, so no table reads
 * outside the data set; the Python layer rejects such tables before the launch.  height and width at least 8.
 * No host synchronisation. */
int unet_augment_u8(int device, const uint8_t* images_dev, const uint8_t* masks_dev, int n_source, int height, int width,
                    const void* params_dev, int n_out, int mask_threshold, uint8_t* images_out_dev,
                    float* targets_out_dev, void* stream);
/* The label mode of the same launch (multi-class training): labels_dev (n_source, height, width) uint8 class labels are
 * warped like the masks, and labels_out_dev (n_out, height, width) uint8 receives the nearest-sampled byte itself, no
 * threshold.  The images are what unet_augment_u8 writes, bit for bit.  Neither pointer may be NULL. */
int unet_augment_u8_labels(int device, const uint8_t* images_dev, const uint8_t* labels_dev, int n_source, int height,
                           int width, const void* params_dev, int n_out, uint8_t* images_out_dev,
                           uint8_t* labels_out_dev, void* stream);
/* sizeof one record, so a binding can check its layout against the library */
size_t unet_augment_param_bytes(void);

/* ---- video path on the GPU (csrc/video_kernels.h) --------------------------------------------------------------
 * The per-frame work of the reference's predict_video (src/unet.py:99-140; the webcam and single-image modes use the
 * same lines, :210-211, :251-252) around the network, a batch of frames at a time.  Integer resize as in the camera
 * stage above; parity against cv2 itself is unpinned.  Both calls only enqueue on `stream`.
 *
 * unet_resize_u8_batch: src_dev (n, height, width, channels) uint8, dense -> dst_dev (n, out_h, out_w, channels):
 * every image is what unet_resize_u8 gives for it, bit for bit (equal sizes are a copy).  channels is 1 or 3.  With
 * swap_rb (3 channels only) channels 0 and 2 are exchanged: cvtColor(BGR2RGB) followed by the resize of
 * preprocess_image (src/unet.py:121, :33).  A resize to more than 7680 columns is UNET_ERR_SHAPE. */
int unet_resize_u8_batch(int device, const uint8_t* src_dev, int n, int height, int width, int channels, int swap_rb,
                         int out_w, int out_h, uint8_t* dst_dev, void* stream);

/* unet_overlay_u8_batch: frames_dev (n, height, width, 3) uint8 and the network's masks masks_dev (n, mask_h, mask_w)
 * uint8 -> overlay_out_dev (n, height, width, 3), per frame and in one pass (src/unet.py:70, :125-126):
 *     m      = cv2.resize(mask, (width, height))                 values 0..255
 *     colour = lut[m]                                            applyColorMap; rows in the frame's channel order
 *     out[c] = clamp(rint(fl(fl(fl(frame[c] * alpha) + fl(colour[c] * beta)) + gamma)), 0, 255)        addWeighted
 * where every fl is one fp32 rounding (nothing is contracted into a fused multiply-add) and rint rounds half to
 * even.  lut_host: 256 * 3 bytes in host memory, consumed before the call returns.  mask_out_dev: NULL, or
 * (n, height, width) uint8 that receives m.  alpha, beta and gamma must be finite.  A frame wider than 7680 whose
 * mask has another size is UNET_ERR_SHAPE. */
int unet_overlay_u8_batch(int device, const uint8_t* frames_dev, int n, int height, int width, const uint8_t* masks_dev,
                          int mask_h, int mask_w, const uint8_t* lut_host, float alpha, float beta, float gamma,
                          uint8_t* overlay_out_dev, uint8_t* mask_out_dev, void* stream);

/* ---- checkpoint ensembles and threshold sweeps (csrc/ensemble_kernels.h) ---------------------------------------
 * Both sit between a head's output and the mask that leaves the device, take a bare device ordinal like
 * unet_seg_metrics_accumulate (so they serve every tier), only enqueue on `stream`, and refuse bad arguments with
 * UNET_ERR_INVALID_ARG and a text for unet_op_last_error that names the call, before any device is touched. */
#define UNET_ENSEMBLE_MAX 8
#define UNET_SWEEP_MAX 64

/* The reference's `ensemble_predict` ("model ensembling", README.md:2623-2647:
 * torch.stack([sigmoid(m(x)) for m in models]).mean(0) > 0.5) on the probability planes the members' heads wrote:
 * probs_dev is a HOST array of k device pointers, 1 <= k <= UNET_ENSEMBLE_MAX, each to `numel` floats; weights_host k
 * floats, finite and not negative, consumed before the call returns (NULL: (float)(1.0 / k) each).  Per element
 *     acc = w[0] * p0;   acc = acc + w[j] * pj   for j = 1 .. k-1, in that order
 * with every product and every sum rounded to fp32 on its own (nothing is contracted into a fused multiply-add), so
 * numpy float32 reproduces the result bit for bit.  probs_out_dev: NULL or `numel` floats that receive acc.
 * mask_out_dev: NULL or `numel` bytes that receive acc > threshold ? 255 : 0, the value the heads write and what the
 * reference's `> 0.5` yields (a NaN gives 0).  Not both NULL.  The inputs are probabilities and not logits: every tier
 * writes them from its head, so no exponential is repeated here and the mean is exact against its model. */
int unet_ensemble_combine(int device, const float* const* probs_dev, int k, const float* weights_host, size_t numel,
                          float threshold, float* probs_out_dev, uint8_t* mask_out_dev, void* stream);

/* Confusion counts of `numel` scores at n_thresholds thresholds in one pass: what choosing the operating point needs
 * (the reference's one knob, `predict(image, threshold=0.5)` src/unet.py:74, its advice to tune it README.md:4503-4524,
 * and the int8 model whose probabilities shift, README.md:3437, :3442-3474).  scores_dev: floats in any domain - logits,
 * probabilities, an ensemble's means; targets_dev: `numel` floats, positive iff != 0, or with targets_are_u8 `numel`
 * bytes, positive iff non-zero (for the 0/1 and 0/255 targets unet_seg_metrics_accumulate takes, the same classes).
 * thresholds_host: 1 <= n_thresholds <= UNET_SWEEP_MAX floats, strictly ascending, no NaN, -inf allowed first and +inf
 * last, consumed before the call returns.  Per element
 *     bin = #{ j : score > thresholds[j] }     0 .. n_thresholds; equal is not above; a NaN is above nothing (bin 0)
 *     counts_dev[cls * (n_thresholds + 1) + bin] += 1      cls = 1 for a positive target
 * counts_dev: 2 * (n_thresholds + 1) unsigned 64-bit integers owned by the caller, added to and never cleared, so
 * batches accumulate.  Predicted positive at thresholds[j] is bin > j: TP, FP, FN, TN at every threshold are suffix and
 * prefix sums of the two rows.  Integer arithmetic: exact and deterministic.  numel at most 2^41 - 1 (UNET_ERR_SHAPE). */
int unet_score_sweep_accumulate(int device, const float* scores_dev, const void* targets_dev, int targets_are_u8,
                                size_t numel, const float* thresholds_host, int n_thresholds,
                                unsigned long long* counts_dev, void* stream);
/* Process-wide kernel choice of unet_score_sweep_accumulate: 1 (default) = equal bins of a wave are combined with
 * ballots before they touch the block's LDS counters, 0 = every lane adds its own.  The counts are the same; the
 * switch is there for tools/ensemble_sweep_timing.py.  Returns the previous setting. */
int unet_set_sweep_combine(int on);

/* ---- lane following on the device (csrc/follow_kernels.h) ------------------------------------------------------
 * The two things the reference does with a frame besides the network: the HSV colour-threshold extractor the network
 * is measured against (`extract_white_lanes`, README.md:206-227) and the scan-row lane centre the mask is reduced to
 * (`LineFollower.find_lane_center`, README.md:4115-4126).  Both take a bare device ordinal, only enqueue on `stream`,
 * consume their host arrays before they return, and refuse bad arguments with UNET_ERR_INVALID_ARG and a text for
 * unet_op_last_error that names the call, before any device is touched.  The arithmetic is restated in
 * tests/follow_model.py and reproduced bit for bit; parity of the HSV conversion with cv2's own is unpinned.
 *
 * unet_hsv_lanes_u8_batch: frames_dev (n, height, width, 3) uint8, dense -> mask_out_dev (n, height, width) uint8
 * holding only 0 and 255, per frame and in one pass over the frames:
 *     (H, S, V) = the project's 8-bit HSV of the pixel (augment.rgb_to_hsv: integers, round-half-up, H in [0, 180));
 *                 with is_bgr channels 0 and 2 are exchanged first                            cvtColor(BGR2HSV)
 *     t         = 255 iff lower[c] <= (H, S, V)[c] <= upper[c] for c = 0, 1, 2, else 0       inRange
 *     mask      = dilate_ko(erode_ko(erode_kc(dilate_kc(t))))        morphologyEx CLOSE kc x kc, then OPEN ko x ko
 * Every dilate (erode) is the maximum (minimum) over a k x k all-ones box anchored at its centre, defined on the
 * whole image in turn; pixels outside the image never take part, at any of the four steps (OpenCV's default border
 * for erode and dilate).  close_ksize and open_ksize are one of 1, 3, 5, 7; 1 is the identity.  lower_host and
 * upper_host: 3 bytes each in host memory.  Any positive n, height, width with n * height * width < 2^31; no
 * alignment requirement on either pointer. */
int unet_hsv_lanes_u8_batch(int device, const uint8_t* frames_dev, int n, int height, int width, int is_bgr,
                            const uint8_t* lower_host, const uint8_t* upper_host, int close_ksize, int open_ksize,
                            uint8_t* mask_out_dev, void* stream);

/* unet_lane_center_u8_batch: masks_dev (n, height, width) uint8, any byte values; rows_host: n_rows row indices in
 * [0, height), 1 <= n_rows <= UNET_LANE_ROWS_MAX, passed to the kernel by value.  For frame i and row j
 *     out_dev[(i * n_rows + j) * 2 + 0] = #{ x : mask[i, rows[j], x] > level }
 *     out_dev[(i * n_rows + j) * 2 + 1] = the sum of those x
 * 0 <= level <= 255; width <= 65535, so the sum fits 32 bits.  No atomics: one wave per (frame, row).  The
 * reference's centre is sum / count (integer division) where count > 10 (follow.lane_centers). */
#define UNET_LANE_ROWS_MAX 64
int unet_lane_center_u8_batch(int device, const uint8_t* masks_dev, int n, int height, int width, const int* rows_host,
                              int n_rows, int level, uint32_t* out_dev, void* stream);

/* ---- lane fit on the device (csrc/lanefit_kernels.h) ------------------------------------------------------------
 * What the reference's bird's-eye warp is there for (README.md:3692: the IPM is in the node "to make the lane-line
 * fit that follows easy") and its roadmap still lists (README.md:5138-5148: lane-line fit, curvature output,
 * confidence output): the classic sliding-window search on the warped mask, reduced on the device to the moment sums
 * a least-squares x = a y^2 + b y + c needs.  The host solves the 3 x 3 normal equations from those exact integers
 * (unet_lane_detection_amd/lanefit.py).  The reference has no such code, so there is nothing outside to be equal to:
 * the arithmetic below is restated in tests/lanefit_model.py and reproduced bit for bit, and parity with any outside
 * implementation (cv2 / numpy tutorials of the same search) is unpinned.  Everything the device sums is an integer:
 * the records do not depend on the order of the reduction.
 *
 * unet_lane_fit_u8_batch: masks_dev (n, height, width) uint8, any byte values; a pixel is ON iff its byte is > level.
 * out_dev: n x 2 records of UNET_LANE_FIT_WORDS unsigned 64-bit words, 8-byte aligned; lane 0 is the left marking,
 * lane 1 the right one.  Every call overwrites all 16 words of every record.  A bare device ordinal; the call only
 * enqueues on `stream`; bad arguments are refused with UNET_ERR_INVALID_ARG and a text for unet_op_last_error that
 * names the call, before any device is touched; no alignment requirement on masks_dev.
 *
 * Window mode (prior_dev == NULL), per frame, all in integers:
 *     hist[x]  = #{ y in [height / 2, height) : mask[y, x] ON }
 *     mid      = width / 2; the left lane's range is [0, mid), the right lane's [mid, width)
 *     a lane whose range is empty or whose histogram maximum is 0 is ABSENT: flags, base, hit, tried and last centre
 *                are 0, the sums are 0, minimum y is `height`, maximum y is 0
 *     base     = the first column of the range at which the maximum is attained
 *     wh       = height / n_windows; window i (0 at the bottom) is rows [height - (i + 1) wh, height - i wh); rows
 *                above the top window belong to no window
 *     c = base; for i = 0 .. n_windows - 1:
 *         the window's columns are [max(c - margin, 0), min(c + margin, width))      half-open: x == c + margin is outside
 *         every ON pixel in it joins the lane's sums
 *         if the window's count is > min_pixels (equal does not recentre): c = (sum of its x) / count, hit += 1
 *     the two lanes' windows may overlap; such a pixel counts for both.
 * Prior mode (prior_dev: (n, 2, height) int32 on the device): no histogram, no windows.  A row y whose prior[y] is
 * negative is not searched; otherwise the ON pixels with prior[y] - margin <= x < prior[y] + margin and 0 <= x < width
 * join the sums.  The bounds are formed in 64 bits: any int32 prior is safe, INT_MAX included.  tried = the rows with
 * a non-negative prior, hit = those of them that contributed at least one pixel.
 *
 * Record words:
 *     [0]        flags; bit 0: the lane is present (window mode: a base was found; prior mode: tried > 0)
 *     [1]        base (0 in prior mode)
 *     [2], [3]   hit, tried (window mode: tried = n_windows, 0 for an absent lane)
 *     [4]        the last c (0 in prior mode)
 *     [5 + k]    S_k = sum of y^k over the lane's pixels, k = 0 .. 4
 *     [10 + k]   T_k = sum of x y^k, k = 0 .. 2
 *     [13], [14] minimum and maximum y of those pixels (`height` and 0 if there are none)
 *     [15]       0
 * The host solves [[S4,S3,S2],[S3,S2,S1],[S2,S1,S0]] (a,b,c) = (T2,T1,T0).
 *
 * Domain (anything else is refused): masks_dev and out_dev not null (prior_dev may be); n >= 1; 1 <= height <= 2048;
 * 1 <= width <= 8192; n * height * width < 2^31; 0 <= level <= 255; 1 <= n_windows <= min(height,
 * UNET_LANE_FIT_WINDOWS_MAX); 1 <= margin <= 512; min_pixels >= 0.
 * The bounds on height and margin keep every sum inside 64 bits.  A lane takes at most 2 margin <= 1024 pixels of a
 * row, so the largest sum is S_4 <= 1024 sum_{y < 2048} y^4 < 1024 * 2048^5 / 5 = 2^65 / 5 = 0.4 * 2^64 (exactly
 * 7 369 693 362 260 017 152 for 2048 rows, against 2^64 = 18 446 744 073 709 551 616), and
 * T_2 <= 1024 * 8191 * sum_{y < 2048} y^2 < 2^55. */
#define UNET_LANE_FIT_WORDS 16
#define UNET_LANE_FIT_WINDOWS_MAX 64
int unet_lane_fit_u8_batch(int device, const uint8_t* masks_dev, int n, int height, int width, int level,
                           int n_windows, int margin, int min_pixels, const int32_t* prior_dev,
                           unsigned long long* out_dev, void* stream);

/* ---- lane instances on the device (csrc/label_kernels.h) --------------------------------------------------------
 * Which pixels of a mask belong together: connected-component labelling of a mask batch, per-component integer
 * statistics and a component filter that writes a cleaned mask for the kernels above.  The reference lists
 * "multi-lane detection", "confidence output" and "instance segmentation" on its roadmap (README.md:5138-5153) and
 * names "lots of noise pixels" as a failure it can only answer by retraining or a higher threshold (README.md:4465,
 * 4601, 3902); it has no such code.  The arithmetic below is restated in tests/label_model.py and reproduced bit for
 * bit; the numbering is that of scipy.ndimage.label, which the model is held to.  Parity with cv2's label numbering
 * is unpinned: cv2 is not installed where this is tested.  Everything the device sums is an integer, so the records
 * do not depend on the order anything ran in.  All three take a bare device ordinal where they take one, only enqueue
 * on `stream`, refuse bad arguments with UNET_ERR_INVALID_ARG and a text for unet_op_last_error that names the call,
 * before any device is touched, have no alignment requirement on uint8 pointers, and overwrite all of their outputs.
 *
 * unet_label_work_bytes: a pure host function, the bytes of caller-owned device workspace unet_label_u8_batch needs
 * for (n, height, width); 0 for arguments outside that call's domain.  Nothing is allocated by either call.
 *
 * unet_label_u8_batch: masks_dev (n, height, width) uint8, any byte values; a pixel is ON iff its byte is > level.
 * connectivity 4: pixels that share an edge connect; 8: those that share a corner do too (cv2's default).
 *   labels_dev   (n, height, width) int32: 0 for an OFF pixel, else the id 1 .. K of its component.  Ids are in
 *                increasing order of the raster index y * width + x of the component's first pixel, per frame: a
 *                canonical numbering.  Components beyond max_components are still labelled; only their records are
 *                missing.
 *   header_dev   n records of four unsigned 64-bit words: [0] K, the true count even when it exceeds max_components;
 *                [1] the number of ON pixels; [2] min(K, max_components); [3] 0.
 *   records_dev  n x max_components records of UNET_LABEL_WORDS unsigned 64-bit words, 8-byte aligned; record c - 1
 *                of a frame describes component c:
 *     [0]        the area (= S_0)
 *     [1] .. [4] x_min, x_max, y_min, y_max
 *     [5]        T_0 = sum of x
 *     [6]        S_1 = sum of y
 *     [7] .. [9] S_2, S_3, S_4, S_k = sum of y^k
 *     [10], [11] T_1 = sum of x y, T_2 = sum of x y^2
 *     [12]       the raster index of the first pixel
 *     [13]       border flags: bit 0 touches row 0, bit 1 row height - 1, bit 2 column 0, bit 3 column width - 1
 *     [14], [15] 0
 *                Records at or beyond min(K, max_components) are all-zero.  S_0 .. S_4 and T_0 .. T_2 are the sums
 *                lanefit.solve takes: every component has a curve x = a y^2 + b y + c.
 *   work_dev     work_bytes >= unet_label_work_bytes(n, height, width) bytes, 4-byte aligned; contents are scratch.
 * Domain (anything else is refused): pointers not null; n >= 1; 1 <= height, width <= 2048; n * height * width <
 * 2^31; 0 <= level <= 255; connectivity 4 or 8; 1 <= max_components <= 65536; work_bytes as above; labels_dev 4-byte
 * aligned, header_dev and records_dev 8-byte aligned.
 * The bounds on height and width keep every sum inside 64 bits.  The largest is S_4 of a full 2048 x 2048 frame,
 * 2048 sum_{y < 2048} y^4 = 14 739 386 724 520 034 304 < 2^64 = 18 446 744 073 709 551 616 (the lane fit above has
 * 1024 sum y^4 = 7 369 693 362 260 017 152), and T_2 <= sum_{x < 2048} x * sum_{y < 2048} y^2 < 2^21 * 2^33 = 2^54.
 *
 * unet_keep_components_u8_batch: labels_dev, header_dev, records_dev and max_components as the call above left them.
 *   keep_out_dev (n, max_components) uint8: entry c - 1 is 1 iff component c has a record, its area is >= min_area,
 *                y_max - y_min + 1 >= min_height, x_max - x_min + 1 >= min_width and, if keep_largest > 0, fewer than
 *                keep_largest components of that frame that pass those thresholds precede it in the order "larger
 *                area first, lower id on equal area".  Else 0.
 *   mask_out_dev (n, height, width) uint8: 255 where the pixel's component is kept, else 0.  A component without a
 *                record (id > max_components) is never kept.  mask_out_dev may be the buffer the labels were
 *                computed from; it must not overlap labels_dev.
 * Domain: pointers not null; n, height, width, max_components as above; min_area, min_height, min_width,
 * keep_largest >= 0; labels_dev 4-byte aligned, header_dev and records_dev 8-byte aligned (keep_out_dev and
 * mask_out_dev: any).
 * What a large max_components costs: the label call clears all n x max_components records on every call (8 MB a frame
 * at 65536, spread over the whole grid), and with keep_largest > 0 a frame with more than 4096 recorded components
 * has its records read 41 times by one workgroup. */
#define UNET_LABEL_WORDS 16
size_t unet_label_work_bytes(int n, int height, int width);
int unet_label_u8_batch(int device, const uint8_t* masks_dev, int n, int height, int width, int level,
                        int connectivity, int32_t* labels_dev, int max_components, unsigned long long* header_dev,
                        unsigned long long* records_dev, void* work_dev, size_t work_bytes, void* stream);
int unet_keep_components_u8_batch(int device, const int32_t* labels_dev, int n, int height, int width,
                                  const unsigned long long* header_dev, const unsigned long long* records_dev,
                                  int max_components, int min_area, int min_height, int min_width, int keep_largest,
                                  uint8_t* keep_out_dev, uint8_t* mask_out_dev, void* stream);

/* ---- lane view on the device (csrc/laneview_kernels.h) -----------------------------------------------------------
 * The step that closes a sliding-window lane fit: the area between two fitted curves, the markings and the curves
 * themselves, all of which live in the bird's-eye image, drawn where the camera looks and blended onto the camera
 * frame.  The reference's own pictures of a result are such camera-view overlays (assets/demo/normal_unet.jpg), its
 * debugging advice is `visualize_output` (README.md:4563-4593: overlay[binary > 0] = [0, 255, 0]; blended =
 * cv2.addWeighted(img, 0.7, overlay, 0.3, 0)), and its roadmap lists "lane + drivable area" and an "end-to-end
 * interface" (README.md:5150-5153); it has no code that goes back through the IPM.  One kernel goes, per camera
 * pixel, forward through the perspective matrix, asks the curves and the mask what lies there, and blends.  The
 * arithmetic below is restated in tests/laneview_model.py and reproduced bit for bit; the mask layer is
 * cv2.warpPerspective(mask, inv(M), (width, height)) as oracle/camera_oracle.py restates it, thresholded, and parity
 * with cv2 itself is unpinned.  A bare device ordinal; the call only enqueues on `stream`; bad arguments are refused
 * with UNET_ERR_INVALID_ARG and a text for unet_op_last_error that names the call, before any device is touched; no
 * alignment requirement on uint8 pointers; every call overwrites all of its outputs.
 *
 * frames_dev: n frames of `height` rows of `step` bytes, 3 interleaved channels, step >= 3 * width; the last row may
 * end with its pixels.  The channel order is the caller's; colours are given in that order.  m: the perspective
 * matrix camera -> bird's-eye, row-major, in host memory: the matrix unet_ipm_prestage_u8's minv is the inverse of,
 * with the sign for which w below is positive on the ground (m and -m are one homography, but only one of them has
 * the ground below the horizon; laneview.orient chooses it).
 * masks_dev: (n, warp_h, warp_w) uint8 or NULL.  curves_dev: (n, k, UNET_LANE_VIEW_WORDS) signed 64-bit words on the
 * device, or NULL with k = 0.  style: host memory, consumed before the call returns; NULL is the default style (0.7,
 * 0.3, 0, both colours (0, 255, 0), thickness 4, both layers on).  view_out_dev: (n, height, width, 3) dense, or
 * NULL.  layers_out_dev: (n, height, width), or NULL.  Not both NULL.
 *
 * Per camera pixel (x, y), with nothing contracted and every operation one IEEE double operation in this order:
 *     w  = m6 x + m7 y + m8             a pixel with !(w > 0) is OUTSIDE: at or above the horizon, a NaN included
 *     fx = (m0 x + m1 y + m2) * (32 / w), fy = (m3 x + m4 y + m5) * (32 / w)
 *     fx, fy clamped to [-2^31, 2^31 - 1] (a NaN becomes -2^31); X = rint(fx), Y = rint(fy)      as the camera stage
 *     INSIDE iff 0 <= X < 32 warp_w and 0 <= Y < 32 warp_h       (X, Y: bird's-eye coordinates in 1/32 pixel)
 * Curve record i of a frame, i < k <= UNET_LANE_VIEW_MAX:
 *     [0]        flags; bit 0: present, bit 1: fill the area up to record i + 1, bit 2: draw the curve
 *     [1], [2]   y0 <= y1: the first and last row of the bird's-eye image the curve is valid on
 *     [3] .. [5] A = rint(a 2^27), B = rint(b 2^32), C = rint(c 2^37) for x = a y^2 + b y + c in pixels, so that
 *                A Y^2 + B Y + C is 2^32 times the curve's x in 1/32 pixel at the row Y / 32
 *     [6]        the curve's colour, byte c = channel c
 *     [7]        0
 * The kernel cannot have checked a record, so it clamps before use: A into +-(2^30 - 1), B into +-(2^45 - 1), C into
 * +-(2^57 - 1), y0 and y1 into [0, warp_h - 1].  An INSIDE pixel has 0 <= Y < 32 * 2048 = 2^16, so
 *     |A Y^2 + B Y + C| < 2^30 2^32 + 2^45 2^16 + 2^57 = 2^62 + 2^61 + 2^57 < 2^63:
 * no sum leaves 64 bits (7 061 468 290 635 333 631 at the extreme record against 2^63 = 9 223 372 036 854 775 808).
 *     x32_i(Y) = (A Y^2 + B Y + C) >> 32                  an arithmetic shift: the floor, also below zero
 *     curve i COVERS Y iff bit 0 is set and 32 y0 <= Y <= 32 y1 + 31
 * The layer of a pixel, highest first; 0 where nothing hits or the pixel is not INSIDE:
 *     3 + i   the lowest i with bit 2 set that covers Y and has |X - x32_i(Y)| <= 16 * thickness
 *     2       masks_dev != NULL, the marking layer is on, and the one-channel bilinear sample of the frame's mask at
 *             (X, Y) - integer pixel (X >> 5, Y >> 5), fractions X & 31 and Y & 31, taps outside the mask read 0,
 *             (sum + 2^14) >> 15: the camera stage's - is > level
 *     1       the area layer is on and there is an i with bit 1 set, i + 1 < k, records i and i + 1 both covering Y,
 *             and x32_i(Y) <= X <= x32_{i+1}(Y).  Curves that cross leave those rows empty.
 * layers_out_dev receives that number.  colour = the curve's, style->marking, style->area or, on layer 0, the frame's
 * own pixel, and on every pixel, whatever its layer,
 *     out[c] = clamp(rint(fl(fl(fl(frame[c] * alpha) + fl(colour[c] * beta)) + gamma)), 0, 255)
 * with fl one fp32 rounding and rint half to even: the addWeighted of unet_overlay_u8_batch.
 *
 * Domain (anything else is refused): frames_dev and m not null; n >= 1; 1 <= height, width <= 4096; step >= 3 * width;
 * n * height * step < 2^31; 1 <= warp_w <= 8192; 1 <= warp_h <= 2048; 0 <= level <= 255; 0 <= k <=
 * UNET_LANE_VIEW_MAX and k == 0 iff curves_dev == NULL; curves_dev 8-byte aligned; all nine m finite; alpha, beta and
 * gamma finite; 1 <= thickness <= 64 (bird's-eye pixels, measured along x); no unknown bit in style->layers; not
 * both outputs NULL. */
#define UNET_LANE_VIEW_WORDS 8
#define UNET_LANE_VIEW_MAX 8
#define UNET_LANE_VIEW_AREA 1u      /* unet_lane_view_style.layers: layer 1 is drawn */
#define UNET_LANE_VIEW_MARKING 2u   /* layer 2 is drawn */
typedef struct unet_lane_view_style {
  float alpha, beta, gamma;
  uint8_t area[3];      /* colour of layer 1 */
  uint8_t marking[3];   /* colour of layer 2 */
  uint8_t reserved[2];  /* ignored */
  int thickness;
  unsigned layers;      /* UNET_LANE_VIEW_AREA | UNET_LANE_VIEW_MARKING */
} unet_lane_view_style;
int unet_lane_view_u8_batch(int device, const uint8_t* frames_dev, int n, int height, int width, int step,
                            const double m[9], int warp_w, int warp_h, const uint8_t* masks_dev, int level,
                            const long long* curves_dev, int k, const unet_lane_view_style* style,
                            uint8_t* view_out_dev, uint8_t* layers_out_dev, void* stream);
/* sizeof(unet_lane_view_style), so a binding can check its layout against the library */
size_t unet_lane_view_style_bytes(void);

/* ---- frame and output diagnostics on the device (csrc/diagnose_kernels.h) ---------------------------------------
 * What the reference tells a user to look at first when "detection is poor": `diagnose_input_image`
 * (README.md:4476-4496: pixel range, mean brightness - it warns below 50 and above 200 - and the variance of
 * cv2.Laplacian(cvtColor(img, BGR2GRAY), CV_64F), warned about below 100) and `quick_test` (README.md:4615-4640: the
 * output's range, its mean and the share of pixels above the threshold), as a few integer words per frame.  Both take
 * a bare device ordinal, only enqueue on `stream`, and refuse bad arguments with UNET_ERR_INVALID_ARG and a text for
 * unet_op_last_error that names the call, before any device is touched.  Every call overwrites its output records, so
 * the caller clears nothing.  Everything summed is an integer: the records do not depend on the order of the
 * reduction.  The arithmetic is restated in tests/diagnose_model.py and reproduced bit for bit.  Parity with cv2
 * itself is unpinned: cv2 is not installed where this is tested and the reference ships no fixture.
 *
 * unet_frame_stats_u8_batch: frames_dev holds n frames of `height` rows of row_stride bytes each, row_stride >=
 * 3 * width, 0 = dense; the first 3 * width bytes of a row are pixels, the rest is padding that is never counted and
 * never read as pixels (a sensor_msgs/Image with its `step`).  The last row may end with its pixels.  out_dev: n
 * records of eight unsigned 64-bit words, 8-byte aligned:
 *     [0], [1], [2]   minimum, maximum and sum over all 3 * width * height pixel bytes   img.min(), img.max(), img.mean() * size
 *     [3]             S1 = sum of L over all pixels, two's complement
 *     [4]             S2 = sum of L * L
 *     [5] .. [7]      0
 *     Y      = (3735 B + 19235 G + 9798 R + 16384) >> 15      OpenCV 4's 8-bit BGR2GRAY; with is_bgr channel 0 is B, else R
 *     L(x,y) = Y(x-1,y) + Y(x+1,y) + Y(x,y-1) + Y(x,y+1) - 4 Y(x,y)                      cv2.Laplacian, ksize = 1
 * with neighbours outside the image taken by reflect-101 (index -1 is 1, index w is w - 2), and the pixel itself
 * where that dimension is 1: cv2's default border.  With N = width * height the host forms, from exact integers and
 * with one rounding to double each,
 *     mean = [2] / (3 N)          sharpness = (N S2 - S1^2) / N^2        the variance of L
 * Any positive n, height, width with n * height * width < 2^31; no alignment requirement on frames_dev. */
int unet_frame_stats_u8_batch(int device, const uint8_t* frames_dev, int n, int height, int width, int row_stride,
                              int is_bgr, unsigned long long* out_dev, void* stream);

/* unet_prob_stats_f32_batch: scores_dev (n, numel_per_frame) fp32 probabilities, as every tier's head writes them (no
 * exponential is evaluated here).  out_dev: n records of four unsigned 64-bit words, 8-byte aligned:
 *     [0]   low 32 bits: the fp32 bits of the minimum over the non-NaN values; high 32 bits: those of the maximum.
 *           -0.0 orders below +0.0; a frame of NaNs only gives +inf and -inf
 *     [1]   #{ s > threshold }: equal is not above and a NaN is above nothing, as in unet_score_sweep_accumulate
 *     [2]   the sum of floor(clamp(s, 0, 1) * 2^32); a NaN adds 0.  The product is exact in fp32, so the sum is an
 *           exact integer and [2] / 2^32 / numel_per_frame is the mean probability to within 2^-32, absolute
 *     [3]   the number of NaNs
 * 0 < numel_per_frame < 2^31; threshold is not a NaN. */
int unet_prob_stats_f32_batch(int device, const float* scores_dev, int n, size_t numel_per_frame, float threshold,
                              unsigned long long* out_dev, void* stream);

/* ---- frame correction on the device (csrc/correct_kernels.h) ----------------------------------------------------
 * The stage between "the message's rows are on the device" and "the warp reads them": a per-frame colour and contrast
 * correction decided from the frame's own histograms.  It answers the failure the reference is built around - the
 * white marking leaves HSV [0..180, 0..40, 185..255] under a colour cast, a shadow or glare (README.md:325-342,
 * :380-429) - which unet_frame_stats_u8_batch can only report.  The reference has no such code, and cv2 is not
 * installed where this is tested: parity with cv2.createCLAHE or any outside implementation is unpinned.  The
 * arithmetic below is restated in tests/correct_model.py and reproduced bit for bit.  A bare device ordinal; the call
 * only enqueues on `stream`; the caller supplies the work buffer; bad arguments are refused with UNET_ERR_INVALID_ARG
 * and a text for unet_op_last_error that names the call, before any device is touched; every output and every region
 * of the work buffer is overwritten by the call, so the caller clears nothing; no workgroup waits for another.
 *
 * frames_dev: n frames of `height` rows of row_stride bytes (0 = dense, otherwise >= 3 * width); the first 3 * width
 * bytes of a row are pixels, the rest is padding that is never read as pixels; the last row may end with its pixels.
 * is_bgr tells which of byte 0 (is_bgr) and byte 2 is blue; it only enters the gray value Y.  out_dev: the corrected
 * frames in rows of out_row_stride bytes (same rule); padding is never written.  out_dev == frames_dev with equal
 * strides is allowed: the apply pass reads a pixel before it writes it and reads no other pixel, and every histogram
 * pass has finished by then.  Any other overlap of the two is refused.  No alignment requirement on either; where both
 * bases and both strides are multiples of 16 the apply pass moves 16 bytes at a time, otherwise bytes - same bits.
 *
 * work_dev: work_bytes >= unet_correct_work_bytes(n, grid_x, grid_y) bytes, 4-byte aligned.  Frame i's part starts at
 * i * (3872 + 1280 * grid_x * grid_y) and holds, in this order,
 *     channel histograms   3 x 256 uint32      hist[c][v] = #{pixels whose byte c (memory order) equals v}
 *     plan words           8 uint32            [0] flags: bit 0 the frame is corrected, bit 1 the stretch is in effect,
 *                                              bit 2 CLAHE is in effect; [1..3] the gains g_0..g_2 (65536 = 1);
 *                                              [4], [5] lo, hi (0, 255 without a stretch); [6], [7] S, low and high half
 *     channel tables       3 x 256 bytes       lut[c][v]
 *     tile histograms      gy x gx x 256 uint32   zeros where CLAHE is not in effect
 *     tile tables          gy x gx x 256 bytes    the identity where CLAHE is not in effect
 *
 * Every `/` below is the floor division of non-negative integers.  N = height * width.
 * Plan, per frame.  S_c = sum of v * hist[c][v], S = S_0 + S_1 + S_2 (64 bits).
 *   gate     if cfg->only_flagged and dark_limit * 3 N <= S <= bright_limit * 3 N (the frame's mean is neither below
 *            dark_limit nor above bright_limit, the limits FrameStats applies to the same mean) the frame is not
 *            corrected: identity tables, flags 0, gains 65536, lo 0, hi 255, output bytes = input bytes.
 *   balance  white_balance 1 (gray world): g_c = clamp((S << 16) / (3 S_c), 65536 / max_gain, 65536 * max_gain);
 *            g_c = 65536 where S_c = 0 or white_balance is 0.  a_c(v) = min(255, (v g_c + 32768) >> 16).
 *   stretch  lo_bp, hi_bp in basis points of the 3 N samples, both 0 = off.  P[u] = sum over c and over the v with
 *            a_c(v) = u of hist[c][v]; lo = the smallest u whose cumulative count exceeds lo_bp * 3 N / 10000; hi = the
 *            smallest u whose cumulative count reaches 3 N - hi_bp * 3 N / 10000.  hi <= lo: no stretch (bit 1 clear,
 *            lo and hi are still recorded).  Otherwise s(u) = 0 for u < lo, else
 *            min(255, ((u - lo) * 255 + (hi - lo) / 2) / (hi - lo)).
 *   tone     cfg->tone, 256 bytes; the identity = off.  A gamma curve is a table the caller computes: no pow runs here.
 *   lut_c[v] = tone[s(a_c(v))].
 * CLAHE (cfg->clahe), OpenCV's scheme in integers.  th = ceil(height / grid_y), tw = ceil(width / grid_x); tile
 * (ty, tx) holds rows ty th .. min((ty + 1) th, height) - 1 and the columns likewise; a grid that leaves a tile empty,
 * (grid_y - 1) th >= height or (grid_x - 1) tw >= width, is refused.  With B', G', R' = lut_c[...] of the pixel,
 *     Y = (3735 B' + 19235 G' + 9798 R' + 16384) >> 15                       unet_frame_stats_u8_batch's gray value
 *   tile histogram: of Y over the tile's own pixels; A = their number (border tiles are smaller).
 *   tile table: L = max(1, clip_q8 * A / 65536) (clip_q8 = the clip limit times 256); E = sum of max(hist - L, 0);
 *     hist = min(hist, L) + E / 256; r = E % 256; if r > 0: step = max(256 / r, 1) and for (i = 0; i < 256 && r > 0;
 *     i += step) hist[i]++, r--.  T[i] = (255 cdf[i] + A / 2) / A with cdf the inclusive prefix sum.
 *   apply: X = 2 x + 1 - tw, tx0 = floor(X / (2 tw)) (X may be negative: a true floor, -1 at the least), wx = X - tx0 *
 *     2 tw, tx1 = tx0 + 1, then both clamped to [0, grid_x - 1]; ty0, ty1, wy likewise from y and th.
 *     Y2 = ((2 th - wy) ((2 tw - wx) T[ty0][tx0][Y] + wx T[ty0][tx1][Y])
 *           + wy ((2 tw - wx) T[ty1][tx0][Y] + wx T[ty1][tx1][Y]) + 2 tw th) / (4 tw th)
 *     out_c = Y2 if Y = 0, else min(255, (p_c Y2 + Y / 2) / Y) with p_c = lut_c[...]: the three channels are scaled by
 *     the luminance ratio, which keeps the hue.
 * Without CLAHE in effect out_c = lut_c[...].
 *
 * Domain (anything else is refused): no null pointer; n, height, width >= 1; height, width <= 16384; n * height * width
 * < 2^31; 1 <= grid_x, grid_y <= 16 and no empty tile (also when clahe is 0: the grid sizes the work buffer);
 * white_balance 0 or 1; 1 <= max_gain <= 8; lo_bp, hi_bp >= 0 with lo_bp + hi_bp < 10000; 1 <= clip_q8 <= 2^24;
 * 0 <= dark_limit <= bright_limit <= 255; work_dev 4-byte aligned and work_bytes as above. */
typedef struct unet_correct_config {
  int white_balance;          /* 0 = off, 1 = gray world */
  int max_gain;               /* 1 .. 8; default 4 */
  int lo_bp, hi_bp;           /* basis points clipped below and above; 0, 0 = off */
  int clahe;                  /* 0 = off */
  int grid_x, grid_y;         /* tiles across and down, 1 .. 16 */
  int clip_q8;                /* clip limit * 256; default 512 */
  int only_flagged;           /* correct only frames whose mean is below dark_limit or above bright_limit */
  int dark_limit, bright_limit; /* default 50, 200 */
  uint8_t tone[256];
} unet_correct_config;
/* sizeof(unet_correct_config), so a binding can check its layout against the library */
size_t unet_correct_config_bytes(void);
/* a pure host function: the bytes of caller-owned device work space; 0 for n < 1 or a grid outside 1 .. 16 */
size_t unet_correct_work_bytes(int n, int grid_x, int grid_y);
int unet_correct_u8_batch(int device, const uint8_t* frames_dev, int n, int height, int width, int row_stride,
                          int is_bgr, const unet_correct_config* cfg, uint8_t* out_dev, int out_row_stride,
                          void* work_dev, size_t work_bytes, void* stream);

/* ---- annotations on the device (csrc/annotate_kernels.h) --------------------------------------------------------
 * The step in front of a device-resident data set: an annotator's polygons rasterised into masks at whatever size a
 * stage trains at.  The reference does it with labelme_to_mask.py (README.md:1013-1052: np.array(points, np.int32) and
 * cv2.fillPoly(mask, [points], 255) per shape) and A.Resize on the stored mask (:1996-2055).  cv2 is not installed
 * where this is tested and the reference ships no fixture: parity with cv2.fillPoly itself is unpinned, and along
 * boundaries cv2's fixed-point edge walk and its line iterator give other pixels.  What is pinned is the rule below,
 * restated in tests/annotate_model.py and reproduced bit for bit.  A bare device ordinal; the call only enqueues on
 * `stream` (one launch, no host synchronisation, no atomics on global memory); every byte of masks_out_dev is written.
 *
 * Tables (CSR, all on the device): frame i owns the polygons frame_offsets[i] .. frame_offsets[i + 1] - 1, polygon j the
 * vertices poly_offsets[j] .. poly_offsets[j + 1] - 1 of vertices_dev, rows of (x, y), and the byte poly_values[j].
 * P = frame_offsets[n] and V = poly_offsets[P] are the lengths the arrays must have (P + 1 offsets, P values, V rows);
 * the kernel clamps every other offset into [0, P] or [0, V] and makes each range non-decreasing, and clamps every
 * coordinate to +-2^20, so that no table makes it read outside arrays of those lengths.  The Python layer refuses such
 * tables before the launch.  vertices_dev 8-byte aligned, the offsets 4-byte aligned.
 *
 * Rule.  Every quantity is an integer; `/` is the floor division of non-negative integers.  Output pixel (X, Y) of
 * frame i asks about the source point sx = X * src_w / out_w, sy = Y * src_h / out_h (equal sizes: the identity), which
 * is the same as rasterising at the source size and taking the nearest pixel.  Its byte is the value of the last
 * polygon of the frame, in order, that covers (sx, sy), and 0 if none does: successive fillPoly calls.  A polygon
 * covers a point if its parity or its outline does.  Its edges run from vertex k to vertex k + 1 and from the last to
 * the first; no vertices: skipped; one vertex: a dot; two: a line (the parities cancel).
 *   parity   even-odd at the pixel centre.  Edges with y0 == y1 are skipped; an edge is oriented so that y0 < y1 and
 *            counts if y0 <= sy < y1 and (x1 - x0) * (sy - y0) - (y1 - y0) * (sx - x0) > 0.  Odd count: covered.
 *   outline  an 8-connected line that does not depend on the edge's direction.  dx = x1 - x0, dy = y1 - y0.
 *            |dx| >= |dy|: oriented so that dx >= 0; dx == 0 is the single point (x0, y0); otherwise the point is on the
 *            line if x0 <= sx <= x1 and 0 <= 2 * (sx - x0) * dy + dx - 2 * dx * (sy - y0) < 2 * dx, which is
 *            y = y0 + floor((2 * (sx - x0) * dy + dx) / (2 * dx)) without a division.  |dx| < |dy|: oriented so that
 *            dy > 0, the same test with x and y exchanged.  A marking's far end is thinner than a pixel; without the
 *            outline it breaks into dots.
 *
 * Domain: no null pointer, n >= 1 (UNET_ERR_INVALID_ARG otherwise); 1 <= src_h, src_w, out_h, out_w <= 16384
 * (UNET_ERR_SHAPE otherwise); |x|, |y| <= 2^20, so that every expression above fits in 63 bits.  The cost grows with
 * output pixels times the edges whose rows meet a 64 x 64 tile of them; there is no cap on a frame's edges. */
int unet_fill_polygons_u8_batch(int device, const int32_t* vertices_dev, const int32_t* poly_offsets_dev,
                                const uint8_t* poly_values_dev, const int32_t* frame_offsets_dev, int n, int src_h,
                                int src_w, int out_h, int out_w, uint8_t* masks_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* UNET_HIP_H */
