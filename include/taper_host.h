/*
 * taper_host.h -- C ABI over the C++ host mirror (taper_amd/csrc/host): the
 * Tensor / Tape / nn::Module / loss / optim / data / train surface of the
 * reference (src/lib.rs:1-17 re-exports) as opaque handles, so that tests and
 * bench.py (Python, ctypes) -- or any other language -- can drive exactly the
 * code path a Rust host would.  Device work happens only through
 * include/taper_hip.h; this layer adds no arithmetic.
 *
 * Every function returns 0 on success; on failure the message is in
 * tp_last_error() (the reference panics instead: src/ops.rs:201-208 etc.).
 * Handles are owned by the caller and released with the matching *_free.
 */
#ifndef TAPER_HOST_H
#define TAPER_HOST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tp_tensor tp_tensor;
typedef struct tp_module tp_module;
typedef struct tp_optim tp_optim;
typedef struct tp_dataset tp_dataset;
typedef struct tp_loader tp_loader;
typedef struct tp_trainer tp_trainer;
typedef struct tp_sched tp_sched;
typedef struct tp_comm tp_comm;
typedef struct tp_qmodule tp_qmodule;

const char *tp_last_error(void);

/* ---- device / tape (src/tape.rs) ---- */
int tp_device_set(int device_id);
int tp_device_sync(void);
int tp_device_shutdown(void);
void *tp_device_ctx(void);                 /* the th_ctx* of this thread (for mixing with taper_hip.h calls) */
int tp_tape_reset(void);                   /* tape.rs:43-49 */
int tp_tape_len(size_t *out);
int tp_tape_set_compat_zero_sentinel(int on);   /* quirk Q1 */
int tp_set_full_backward(int on);               /* quirk Q2: 0 = faithful (default) */
int tp_set_conv_chain(int on);                  /* Trainer steps: 1 (default) = the conv front of a Sequential as one launch where compiled (th_conv_chain_fwd), 0 = layer by layer */
int tp_set_conv_chain_head(int on);             /* ... and the classifier behind such a front row by row in the same launch where compiled (th_conv_chain_head_fwd + th_wide_head_grads: the simple CNN's step is two launches); default 1 */

/* ---- Tensor (src/tensor.rs:470-541) ---- */
int tp_tensor_new(const float *h_data, const size_t *shape, int ndim, tp_tensor **out);
int tp_tensor_randn(const size_t *shape, int ndim, uint64_t seed, tp_tensor **out);
int tp_tensor_clone(const tp_tensor *t, tp_tensor **out);     /* Arc clone */
int tp_tensor_free(tp_tensor *t);
int tp_tensor_set_requires_grad(tp_tensor *t, int on);
int tp_tensor_requires_grad(const tp_tensor *t, int *out);
int tp_tensor_ndim(const tp_tensor *t, int *out);
int tp_tensor_shape(const tp_tensor *t, size_t *out4);
int tp_tensor_len(const tp_tensor *t, size_t *out);
int tp_tensor_data(const tp_tensor *t, float *h_out);          /* D2H copy of len floats */
int tp_tensor_set_data(tp_tensor *t, const float *h_in);
int tp_tensor_has_grad(const tp_tensor *t, int *out);
int tp_tensor_grad(const tp_tensor *t, float *h_out);          /* error if grad is None */
int tp_tensor_set_grad(tp_tensor *t, const float *h_in /* NULL -> None */);
int tp_tensor_tape_node(const tp_tensor *t, size_t *out);
int tp_tensor_dptr(const tp_tensor *t, void **d_out);          /* device pointer of the storage */
int tp_tensor_backward(tp_tensor *t);                          /* tensor.rs:520-529 */
int tp_tensor_zero_grad(tp_tensor *t);                         /* tensor.rs:531-533 */

/* ---- ops (src/ops.rs, src/tensor.rs); each returns a new handle ---- */
int tp_add(const tp_tensor *a, const tp_tensor *b, tp_tensor **out);
int tp_sub(const tp_tensor *a, const tp_tensor *b, tp_tensor **out);
int tp_mul(const tp_tensor *a, const tp_tensor *b, tp_tensor **out);
int tp_div(const tp_tensor *a, const tp_tensor *b, tp_tensor **out);
int tp_matmul(const tp_tensor *a, const tp_tensor *b, tp_tensor **out);
int tp_add_broadcast(const tp_tensor *a, const tp_tensor *b, tp_tensor **out);
int tp_sub_broadcast_rows(const tp_tensor *a, const tp_tensor *b, tp_tensor **out);
int tp_relu(const tp_tensor *x, tp_tensor **out);
int tp_sigmoid(const tp_tensor *x, tp_tensor **out);
int tp_transpose(const tp_tensor *x, tp_tensor **out);
int tp_exp(const tp_tensor *x, tp_tensor **out);
int tp_log(const tp_tensor *x, tp_tensor **out);
int tp_pow(const tp_tensor *x, float e, tp_tensor **out);
int tp_mean(const tp_tensor *x, tp_tensor **out);
int tp_sum(const tp_tensor *x, int dim /* -1 = all */, int keepdim, tp_tensor **out);
int tp_max(const tp_tensor *x, int dim /* -1 = all */, tp_tensor **values, tp_tensor **indices);
int tp_reshape(const tp_tensor *x, const size_t *shape, int ndim, tp_tensor **out);
int tp_flatten(const tp_tensor *x, int start_dim, tp_tensor **out);
int tp_squeeze(const tp_tensor *x, int dim /* -1 = all */, tp_tensor **out);
int tp_unsqueeze(const tp_tensor *x, int dim, tp_tensor **out);
int tp_linear(const tp_tensor *x, const tp_tensor *w, const tp_tensor *b /* nullable */, int relu, tp_tensor **out);
int tp_conv2d(const tp_tensor *x, const tp_tensor *w, const tp_tensor *b /* nullable */, int stride_h, int stride_w,
              int pad_h, int pad_w, int dil_h, int dil_w, int relu, tp_tensor **out);
/* tp_conv2d with a trailing flags word (0: exactly tp_conv2d).  Bit 0, TP_CONV_EXACT_STRIDE (not in the reference): the call must be 3x3,
 * stride (2, 2), padding (1, 1), dilation (1, 1); it runs the exact strided convolution (th_conv3x3_s2_fwd) instead of the reference's
 * general gather (Q9), and under tp_set_full_backward(1) its weight and input take gradients by the stride-1 rules.  Any other geometry
 * with the bit, and any unknown bit, is refused by name.  The same word is the last argument of tp_conv2d_new_ex (one group),
 * tp_basic_block_new_ex and tp_residual_block_new_ex; the blocks hand the bit to every conv of theirs whose stride is 2, change nothing
 * at stride 1 and refuse any other stride with it.  The flag is constructor state, not checkpoint content; tp_module_quantize* refuse a
 * model that holds such a conv. */
#define TP_CONV_EXACT_STRIDE 1
/* Value 16, TP_CONV_EXACT_POINTWISE (not in the reference; bits 2, 4 and 8 stay unknown): the call must be 1x1, stride (1, 1) or (2, 2),
 * padding (0, 0), dilation (1, 1); it runs the exact pointwise convolution (th_conv1x1_exact_fwd) instead of the reference's 1x1
 * reinterpretation (Q4: no convolution for c_in > 1, no stride, no gradient), and under tp_set_full_backward(1) its weight and input take
 * gradients.  Known to tp_conv2d_ex and tp_conv2d_new_ex (one group; with bit 0 as well -- 17 -- refused by name: a kernel is 3x3 or 1x1)
 * and to tp_residual_block_new_ex, where it means "pointwise shortcut" and combines with bit 0; tp_basic_block_new_ex refuses it as
 * unknown.  Constructor state, not checkpoint content; tp_module_quantize* refuse a model that holds such a conv. */
#define TP_CONV_EXACT_POINTWISE 16
int tp_conv2d_ex(const tp_tensor *x, const tp_tensor *w, const tp_tensor *b /* nullable */, int stride_h, int stride_w,
                 int pad_h, int pad_w, int dil_h, int dil_w, int relu, int flags, tp_tensor **out);
int tp_max_pool2d(const tp_tensor *x, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, tp_tensor **out);
int tp_avg_pool2d(const tp_tensor *x, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, tp_tensor **out);

/* ---- loss (src/loss.rs) ---- */
int tp_log_softmax(const tp_tensor *x, tp_tensor **out);
int tp_softmax(const tp_tensor *x, tp_tensor **out);
int tp_cross_entropy_loss(const tp_tensor *logits, const tp_tensor *targets, tp_tensor **out);
int tp_accuracy(const tp_tensor *pred, const tp_tensor *targets, float *out);
int tp_one_hot(const tp_tensor *idx, int num_classes, tp_tensor **out);
int tp_mse_loss(const tp_tensor *pred, const tp_tensor *targets, tp_tensor **out);
int tp_bce_loss(const tp_tensor *pred, const tp_tensor *targets, tp_tensor **out);                    /* loss.rs:6-73 */
int tp_cross_entropy_loss_onehot(const tp_tensor *logits, const tp_tensor *targets, tp_tensor **out); /* loss.rs:201-245 */

/* ---- nn (src/nn.rs, src/activation.rs) ---- */
int tp_linear_new(int in_features, int out_features, int with_bias, uint64_t seed, tp_module **out);
int tp_relu_new(tp_module **out);
int tp_sigmoid_new(tp_module **out);
int tp_conv2d_new(int in_ch, int out_ch, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, int with_bias,
                  int fuse_relu, uint64_t seed, tp_module **out);
int tp_conv2d_new_ex(int in_ch, int out_ch, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, int with_bias,
                     int fuse_relu, uint64_t seed, int flags, tp_module **out);   /* flags: see tp_conv2d_ex */
/* nn.rs:180-354 with groups > 1: weight [out, in/groups, k, k]; forward = slice_channels / slice_output_channels /
 * slice_1d, one conv2d per group, cat(dim 1) (nn.rs:289-332, 859-1014).  Like the reference's, the slices carry no tape
 * nodes: a grouped convolution is forward-only (nothing behind it, nor its own parameters, receives a gradient). */
int tp_conv2d_grouped_new(int in_ch, int out_ch, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, int groups,
                          int with_bias, int fuse_relu, uint64_t seed, tp_module **out);
int tp_slice_channels(const tp_tensor *x, size_t start, size_t end, tp_tensor **out);   /* nn.rs:862-886 */
int tp_cat(const tp_tensor *const *tensors, int n, size_t dim, tp_tensor **out);        /* nn.rs:928-1014: 2-D dim 0/1, 4-D dim 1 */
int tp_maxpool2d_new(int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, tp_module **out);
int tp_avgpool2d_new(int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, tp_module **out);
int tp_adaptive_avgpool2d_new(int out_h, int out_w, tp_module **out);
int tp_flatten_new(int start_dim, tp_module **out);
int tp_dropout_new(float p, uint64_t seed, tp_module **out);                 /* nn.rs:773-827 */
int tp_dropout_set_training(tp_module *m, int training);                     /* train() / eval() */
int tp_dropout_last_mask(const tp_module *m, tp_tensor **out);               /* mask of the latest training forward */
int tp_sequential_new(tp_module *const *layers, int n, int fuse_linear_relu, tp_module **out);
int tp_module_free(tp_module *m);
int tp_module_forward(const tp_module *m, const tp_tensor *x, tp_tensor **out);
int tp_module_num_parameters(const tp_module *m, int *out);
int tp_module_parameter(const tp_module *m, int i, tp_tensor **out);   /* shares storage with the model */
/* ---- BatchNorm2d / BasicBlock (nn.rs:829-857 announces both and writes neither: torch.nn.BatchNorm2d's semantics) ----
 * input [N, num_features, H, W]; parameters {gamma (ones), beta (zeros)}, buffers {running_mean (zeros), running_var (ones)}.  In
 * training mode (the layer's own flag, default on) the forward normalises with the batch's mean and biased variance and updates the
 * running pair on the device (momentum; unbiased variance); in eval mode it normalises with the running pair.  fuse_relu: max(y, 0) in
 * the same pass.  num_features <= 0, eps not finite or <= 0 and momentum outside [0, 1] fail before the device is touched; a training
 * forward of one value per channel fails with "Expected more than 1 value per channel when training". */
int tp_batchnorm2d_new(int num_features, float eps, float momentum, int fuse_relu, tp_module **out);
int tp_batchnorm2d_set_training(tp_module *m, int training);
int tp_batchnorm2d_is_training(const tp_module *m, int *out);
int tp_batchnorm2d_running_stats(const tp_module *m, float *h_mean, float *h_var);               /* each output nullable */
int tp_batchnorm2d_set_running_stats(tp_module *m, const float *h_mean, const float *h_var);
/* Conv2d::conv3x3(in, out, stride, 1) -> BatchNorm2d(out) with the ReLU fused; parameters(): the conv's, then gamma, beta */
int tp_basic_block_new(int in_channels, int out_channels, int stride, uint64_t seed, tp_module **out);
int tp_basic_block_new_ex(int in_channels, int out_channels, int stride, uint64_t seed, int flags, tp_module **out);   /* flags: see tp_conv2d_ex */
/* y = bn(x) + residual, then the layer's ReLU (fuse_relu: after the add), inside the normalisation's own launches: one tape
 * node whose backward also leaves the residual's gradient.  Statistics and the running update are tp_module_forward's.  Fails with
 * "BatchNorm2d::forward_add: ..." for a residual of another shape and for one that shares x's storage. */
int tp_batchnorm2d_forward_add(const tp_module *m, const tp_tensor *x, const tp_tensor *residual, tp_tensor **out);
/* conv3x3(in, out, stride, pad 1) -> BatchNorm2d + ReLU -> conv3x3(out, out, 1, pad 1) -> BatchNorm2d with the shortcut added and the ReLU
 * behind the add.  Shortcut: the input when in == out and stride == 1, else conv3x3(in, out, stride, pad 1) -> BatchNorm2d (a 3x3
 * projection: the float 1x1 path is not a usable one).  No conv has a bias; seeds: seed, seed + 1, seed + 2 (the projection).
 * parameters(): conv1 w, bn1 gamma beta, conv2 w, bn2 gamma beta, [shortcut conv w, gamma beta]; buffers: the running pairs in that order.
 * Non-positive arguments fail before the device is touched.  No quantized twin: tp_module_quantize* refuse the block. */
int tp_residual_block_new(int in_channels, int out_channels, int stride, uint64_t seed, tp_module **out);
/* flags: see tp_conv2d_ex.  With TP_CONV_EXACT_STRIDE and stride 2, conv1 and the projection are true convolutions that train under
 * tp_set_full_backward(1): the downsampling block to train with (the default block's strided convs keep the reference's gather and take
 * no gradient). */
int tp_residual_block_new_ex(int in_channels, int out_channels, int stride, uint64_t seed, int flags, tp_module **out);
/* With TP_CONV_EXACT_POINTWISE the projection is a 1x1 exact pointwise convolution(in, out, stride) -> BatchNorm2d in place of the 3x3 (same
 * seed + 2, no bias; strides 1 and 2 alone); with an identity shortcut the flag changes nothing.
 *
 * The bottleneck block: pointwise(in, mid) -> BatchNorm2d + ReLU -> conv3x3(mid, mid, stride, pad 1; the exact strided convolution at
 * stride 2) -> BatchNorm2d + ReLU -> pointwise(mid, out) -> BatchNorm2d + shortcut -> ReLU.  Shortcut: the input when in == out and stride
 * == 1, else pointwise(in, out, stride) -> BatchNorm2d.  Every 1x1 is the exact pointwise convolution, no conv has a bias, seeds seed ..
 * seed + 3 in that order; stride 1 or 2 (others refused by name).  parameters(): conv1 w, bn1 gamma beta, conv2 w, bn2 gamma beta, conv3 w,
 * bn3 gamma beta, [shortcut conv w, gamma beta]; buffers: the running pairs in that order.  No quantized twin. */
int tp_bottleneck_block_new(int in_channels, int mid_channels, int out_channels, int stride, uint64_t seed, tp_module **out);
/* saved-but-not-trained state (the running statistics), concatenated over a Sequential's / BasicBlock's / ResidualBlock's children; shares storage */
int tp_module_num_buffers(const tp_module *m, int *out);
int tp_module_buffer(const tp_module *m, int i, tp_tensor **out);
/* train() / eval() of every BatchNorm2d and every Dropout inside m */
int tp_module_set_training(tp_module *m, int on);

/* ---- post-training quantization (src/nn.rs:14-23, the quantized twins of nn.rs:62-504) ----
 * qtype: 0 Int8, 1 Float16; 2 Int4, 3 BFloat16 and 4 NF4 are placeholders in the reference (zeros) and are refused.  enabled == 0
 * gives Float16 whatever qtype says (tensor.rs:2085-2088).  Linear, Conv2d / Conv2dReLU, Sequential, the pools, Flatten, ReLU and
 * Sigmoid have twins; any other module (Dropout; BatchNorm2d and BasicBlock, which the static calls below take) fails with "Quantization not implemented for this module type" (nn.rs:15) before
 * anything is allocated.  The codes are made on the device; the source model is not touched and can keep training. */
int tp_module_quantize(const tp_module *m, int qtype, int enabled, tp_qmodule **out);
/* Static int8 quantization: weights and biases packed exactly as tp_module_quantize(m, 0, 1) packs them (tp_qmodule_tensor returns the same
 * bits), and every Linear additionally given ONE activation scale: the calibration tensors run through the plain float layers (a QAT layer:
 * its inner layer) and the finite min / max of each Linear's float input over all of them give max(|min|, |max|) / 127 (all zero ->
 * (0, 1), all equal to m -> (0.9 m, 1.1 m)), on the device.  A Linear's forward then quantizes its input with that scale and multiplies
 * int8 by int8 on the integer matrix cores with exact int32 sums (include/taper_hip.h, th_linear_q8q8_fwd), two launches at every batch
 * size; everything else runs as in the weight-only twin.  Refused before anything is allocated: a module tp_module_quantize refuses (same
 * message), n_calib < 1, a null calibration tensor, a Linear with in_features > 65 536.  The source model is only read; no tape node stays. */
int tp_module_quantize_static(const tp_module *m, const tp_tensor *const *calib, int n_calib, tp_qmodule **out);
/* tp_module_quantize_static with the convolutions static too: every 3x3, stride-1 Conv2d / Conv2dReLU with one group and no dilation (a
 * QAT conv: its inner layer) gets one activation scale from its float input in the same calibration pass, and its forward is two
 * launches -- channel-last int8 codes, then an implicit GEMM on the integer matrix cores (th_quantize_act_nhwc_int8, th_conv2d_q8q8_fwd)
 * with the layer's own or a following ReLU in the epilogue.  Any other conv (grouped, dilated, 1x1, strided or another kernel: the float
 * paths that are not plain convolutions) stays weight-only inside the same twin and has no scale.  tp_qmodule_tensor still returns the
 * packed codes of tp_module_quantize (the channel-last copy is internal); tp_qmodule_act_scales lists one scale per static layer, Linear
 * or conv, in layer order.  Refused in addition, before anything is allocated: in_channels * k_h * k_w > 65 536. */
int tp_module_quantize_static_conv(const tp_module *m, const tp_tensor *const *calib, int n_calib, tp_qmodule **out);
/* tp_module_quantize_static_conv with the activations int8 from one static conv to the next: calibration, packing, refusals, tensors, scales
 * and storage bytes are the same, and so is every output bit on finite activations; only the launches differ.  A link is a static conv A
 * of at most th_qconv_i8_chain_max_cout() output channels (its own or a following ReLU folded in), optionally ONE MaxPool2d, then a
 * static conv B inside the same Sequential: A's product writes B's codes (th_conv2d_q8q8_fwd_codes with B's scale), the pool runs on the
 * codes (th_maxpool2d_nhwc_int8) and B skips its codec -- no f32 tensor exists at the boundary.  Anything else between two convs (a ReLU
 * behind the pool, a second pool, any other layer, a weight-only conv, a wider A) runs as in tp_module_quantize_static_conv's twin. */
int tp_module_quantize_static_chain(const tp_module *m, const tp_tensor *const *calib, int n_calib, tp_qmodule **out);
/* The three calls above as one, by flags, and per-channel weight pairs: TP_QSTATIC_CONVS is tp_module_quantize_static_conv, with
 * TP_QSTATIC_CHAIN tp_module_quantize_static_chain (CHAIN without CONVS, and any unknown bit, is refused).  TP_QSTATIC_PER_CHANNEL gives the
 * weight of every static layer one {min_val, scale} pair per output channel instead of one for the tensor -- a Linear's rows; a static
 * conv's effective output channels, the columns of its buffer as the float kernels read it ([c_in k_h k_w][c_out]) -- each pair from the
 * finite min / max of that channel alone (th_quantize_int8_channels), and the products read them (th_linear_q8q8_fwd_pc,
 * th_conv2d_q8q8_fwd_pc, th_conv2d_q8q8_fwd_codes_pc).  Biases and every layer that stays weight-only keep one pair; calibration, scales,
 * links and refusals are those of the per-tensor twin.
 * TP_QSTATIC_LINKS keeps the activations int8 through the classifier as well: a static Linear A, optionally a ReLU, then a static Linear
 * B directly behind in the same Sequential is a link -- A's product writes B's codes with B's scale (th_linear_q8q8_fwd_link), B skips its
 * codec and sums its rows from the codes it reads.  With CONVS and CHAIN also set, the last stage of a static conv run of at most
 * th_qconv_i8_chain_max_cout() output channels c, optionally ONE MaxPool2d, Flatten(1), then a static Linear with in_features = c * HW
 * and HW * th_qconv_i8_cpitch(c) <= th_q8q8_max_k() is a link too: the Linear keeps its weight rows re-laid [HW][cpitch] and reads the
 * channel-last codes the conv (or the pool) writes with its scale.  LINKS alone is valid (Linear links only) and combines with the three
 * flags above.  Calibration, packing, tensors, scales and every output bit are those of the same flags without LINKS; only the launches
 * differ, and tp_qmodule_storage_bytes counts the re-laid rows of a Linear behind a Flatten link.  The value is 16: bit 8 stays an unknown
 * bit and is refused, like -1.
 * TP_QBLOCKS (32; needs CONVS, refused by name without it) quantizes residual models.  Without it every refusal stands:
 * ResidualBlock, BottleneckBlock and every exact_stride / exact_pointwise conv are refused with their messages.  With it the exact convs
 * (3x3 stride 2 pad 1; 1x1 stride 1 or 2) are static convs like the stride-1 3x3, bare, in a BasicBlock or in a block, and a ResidualBlock /
 * BottleneckBlock whose convs are all such convolutions gets a twin: its main branch as static stages with each BatchNorm2d in its
 * conv's epilogue, and the skip connection r added in f32 in the last conv's epilogue (th_conv2d_q8q8_fwd_residual / _codes_residual),
 *     y = max(((v * a) + b) + r, 0)   (each operation rounded once, in this order).
 * Identity shortcut: r = (float)code * scale from the codes of the block's input as its first conv reads them.  Projected shortcut: the
 * projection is one more static stage on the same codes (its calibrated scale equals the first conv's bit for bit), its BatchNorm2d in
 * its epilogue, no ReLU, and r is its f32 map.  A block that holds a default strided or 1x1 conv (no convolution: SURVEY Q4 / Q9) is
 * refused by name before anything is allocated: build it with exact_stride / pointwise_shortcut.  With CHAIN a block is a stage of the
 * enclosing Sequential's run and the boundaries inside its main branch are links (the 128-channel rule applies; the identity residual
 * is no boundary); the scales, tensors and every output bit are those of the same flags without CHAIN / LINKS.  tp_qmodule_tensor
 * lists conv1, conv2, [conv3], [projection]; the scales follow that order; tp_qmodule_affine lists bn1, bn2, [bn3], [the shortcut's].
 * tp_module_quantize keeps refusing blocks; blocks wider than 128 channels at a link run through f32; int8 training is out of scope. */
#define TP_QSTATIC_CONVS 1
#define TP_QSTATIC_CHAIN 2
#define TP_QSTATIC_PER_CHANNEL 4
#define TP_QSTATIC_LINKS 16
#define TP_QBLOCKS 32
int tp_module_quantize_static_ex(const tp_module *m, const tp_tensor *const *calib, int n_calib, int flags, tp_qmodule **out);
/* tp_module_quantize_static_ex with the rule that turns the calibration tensors into each static layer's activation scale.  `flags`: the
 * TP_QSTATIC_* flags above, their rules unchanged; every twin form, the BatchNorm folds and the QAT inner layers combine with either
 * method -- only the value of each layer's scale differs.  method = TP_CALIB_MINMAX: tp_module_quantize_static_ex itself (keep_ppm and
 * num_bins are not read; nothing more runs or is allocated).  method = TP_CALIB_PERCENTILE: the calibration set is shown twice -- the
 * range pass, then every static layer adds its float inputs to its own histogram of |x| with num_bins bins over [0, max(|min|, |max|)]
 * (th_act_hist_update) -- and each scale becomes T / 127, T the upper edge of the first bin at which keep_ppm millionths of the layer's
 * finite input elements are kept (th_act_scale_from_hist; its fallbacks leave the min / max scale).  keep_ppm = 1 000 000 gives the
 * min / max scales bit for bit.  The histograms are released before the call returns.  Refused by name before the model or the device is
 * touched: flags as above, a method that is neither, and with TP_CALIB_PERCENTILE keep_ppm outside [1, 1 000 000] or num_bins outside
 * [16, th_act_hist_max_bins()]; then tp_module_quantize_static's refusals.
 * tp_qmodule_calibration: static layer i in tp_qmodule_act_scales order, of any static twin -- out4 = {finite min, finite max, threshold,
 * scale}, stats4 = {bin, total, kept, bin_count}: the bin the threshold ends, the finite elements counted, those at or below the
 * threshold's bin, and that bin's own count (all 0 for a min / max twin, whose threshold is max(|min|, |max|)). */
#define TP_CALIB_MINMAX 0
#define TP_CALIB_PERCENTILE 1
int tp_module_quantize_static_cal(const tp_module *m, const tp_tensor *const *calib, int n_calib, int flags, int method, int keep_ppm, int num_bins,
                                  tp_qmodule **out);
int tp_qmodule_calibration(const tp_qmodule *q, int i, float *out4, uint64_t *stats4);
/* the layer boundaries a forward crosses in int8 (the links above: conv -> conv, Flatten, Linear -> Linear); 0 for a twin made without
 * TP_QSTATIC_CHAIN and TP_QSTATIC_LINKS */
int tp_qmodule_chain_links(const tp_qmodule *q, int *out);
/* the calibrated activation scales in layer order: *n = their count (0 for a weight-only twin), the first min(*n, cap) into h_scales (nullable) */
int tp_qmodule_act_scales(const tp_qmodule *q, float *h_scales, int cap, int *n);
int tp_qmodule_free(tp_qmodule *q);
/* QuantizedModule::forward: records no tape node; the output does not require a gradient */
int tp_qmodule_forward(const tp_qmodule *q, const tp_tensor *x, tp_tensor **out);
/* code bytes of every tensor (a static twin's Linear weights with their row padding; behind a Flatten link of TP_QSTATIC_LINKS the re-laid
 * rows of out_features * HW * cpitch bytes the twin holds instead), plus 8 bytes of {min_val, scale} per int8 tensor
 * (per channel of a per-channel tensor), 4 bytes per activation scale and 8 bytes per channel of a frozen BatchNorm2d */
int tp_qmodule_storage_bytes(const tp_qmodule *q, size_t *out);
/* the packed tensors in the order of the source's parameters() without those of a BatchNorm2d (its gamma and beta are not packed: see
 * tp_qmodule_affine): length, then codes (n int8 or n uint16; h_codes nullable),
 * {min_val, scale} (int8; {0, 0} for Float16; nullable) and the qtype (nullable) */
int tp_qmodule_num_tensors(const tp_qmodule *q, int *out);
int tp_qmodule_tensor_len(const tp_qmodule *q, int i, size_t *out);
int tp_qmodule_tensor(const tp_qmodule *q, int i, void *h_codes, float *h_params, int *qtype);
/* Per-channel tensors (TP_QSTATIC_PER_CHANNEL): element k of channel c is code c * chan_stride + k * elem_stride of the packed tensor; a
 * tensor with one pair returns 1, 0, 1.  tp_qmodule_tensor_params: *n_pairs = the tensor's pairs (its channels; 1 for a per-tensor int8
 * tensor, 0 for Float16), the first min(*n_pairs, cap_pairs) as {min_val, scale} into h_pairs (nullable).  tp_qmodule_tensor refuses a
 * non-null h_params on a per-channel tensor; its codes and qtype work as before. */
int tp_qmodule_tensor_channels(const tp_qmodule *q, int i, size_t *channels, size_t *chan_stride, size_t *elem_stride);
int tp_qmodule_tensor_params(const tp_qmodule *q, int i, float *h_pairs, size_t cap_pairs, size_t *n_pairs);
/* BatchNorm2d and BasicBlock in the four tp_module_quantize_static* calls above (tp_module_quantize keeps the reference's refusal: without
 * TP_QSTATIC_CONVS the convs of such a model stay weight-only inside a static twin).  A BatchNorm2d's twin keeps a snapshot of the layer on its running pair,
 * whatever its training flag says: per channel {a, b} with invstd = 1 / sqrt(running_var + eps), a = gamma * invstd,
 * b = beta - running_mean * a, made on the device (th_fold_batchnorm2d), and its forward is y = x * a + b, then max(y, 0) where the layer
 * fuses a ReLU -- each operation rounded once.  The weights are not touched: every code of tp_qmodule_tensor is that of the same call on
 * the same model.  A BasicBlock gives its conv twin and its BatchNorm2d twin inline to the enclosing Sequential's twin (alone: a Sequential
 * twin of the two).  Right behind a static conv that has no ReLU of its own the layer runs in that conv's epilogue
 * (th_conv2d_q8q8_fwd_affine / _codes_affine) with its own or a following ReLU folded in behind it, so a link of TP_QSTATIC_CHAIN is static
 * conv, [BatchNorm2d], [ReLU], [one MaxPool2d], static conv; behind anything else (a weight-only conv such as a BasicBlock's with stride
 * 2) it is one launch of th_channel_affine_fwd.  Calibration runs the float layer in eval mode.  Nothing of the source is modified.
 * tp_qmodule_num_affines: the frozen layers of the twin; tp_qmodule_affine: layer i in layer order -- *n_pairs = its channels, the first
 * min(*n_pairs, cap_pairs) pairs {a, b} into h_pairs (nullable). */
int tp_qmodule_num_affines(const tp_qmodule *q, int *out);
int tp_qmodule_affine(const tp_qmodule *q, int i, float *h_pairs, size_t cap_pairs, size_t *n_pairs);

/* ---- quantization-aware training (src/quantization/{qat_config,qat_layers,qat_manager}.rs) ----
 * config: qtype 0 Int8 / 1 Float16 (2..4 refused like tp_module_quantize), activations (fake-quantize each layer's output, before any
 * ReLU), symmetric (must be 1) and per_channel (must be 0) -- a refused config fails before the device is touched.  module_id: the
 * qat_manager key (nullable: "linear_<in>" / "conv2d_<in>_<out>" as qat_layers.rs names them).  Initial weights are those of
 * tp_linear_new / tp_conv2d_new with the same seed; parameters() are the inner layer's; tp_module_quantize packs the inner layer.
 * While active a layer runs on the codec's round trip of its weight AND bias (what tp_module_quantize packs) and, with activations, of
 * its output; gradients pass straight through to the f32 masters. */
int tp_qat_linear_new(int in_features, int out_features, int with_bias, int qtype, int activations, int symmetric, int per_channel,
                      const char *module_id, uint64_t seed, tp_module **out);
/* groups 1 only; fuse_relu: a QAT Conv2dReLU (the ReLU follows the activation fake-quant) */
int tp_qat_conv2d_new(int in_ch, int out_ch, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, int with_bias, int fuse_relu,
                      int qtype, int activations, int symmetric, int per_channel, const char *module_id, uint64_t seed, tp_module **out);
/* the process-wide state (qat_manager.rs global::): QAT enabled (default 0), training mode (default 1); a QAT layer fake-quantizes
 * while both are on and its own flag is (tp_qat_module_set_enabled also sets the manager's entry of its id) */
int tp_qat_enable(int on);
int tp_qat_set_training(int on);
int tp_qat_is_training(int *out);
int tp_qat_module_set_enabled(tp_module *m, int on);
int tp_qat_status(int *global_enabled, int *training_mode, size_t *module_count, size_t *enabled_modules);
/* observer readout: {weight min_val, weight scale, activation scale} of the layer's last fake-quantized forward (int8; zeros before) */
int tp_qat_module_observed(const tp_module *m, float *out3);
/* the round trip of the layer's weight (which 0) or bias (1) that its last active forward ran with (a copy; no gradient) */
int tp_qat_module_fake_quantized(const tp_module *m, int which, tp_tensor **out);

/* ---- quantization observers (src/quantization/observers.rs) ----
 * Statistics of the tensors an observer is shown, kept on the device: tp_observer_observe only enqueues work (no synchronisation, nothing
 * read back), the read-outs wait.  kind TP_OBSERVER_MINMAX: the running min / max PER ELEMENT of the flat data (the first observation
 * fixes the length; later ones update the first min(m, len) elements); TP_OBSERVER_HISTOGRAM: num_bins >= 1 64-bit counts between
 * num_bins + 1 edges that the first observation fixes (0 bins fail before the device is touched; num_bins is ignored for MINMAX).  A
 * disabled observer ignores observations and does not count them; reset returns every device buffer and the next observation is a
 * first one again.  A read-out of the other kind's group fails. */
#define TP_OBSERVER_MINMAX 0
#define TP_OBSERVER_HISTOGRAM 1
typedef struct tp_observer tp_observer;
typedef struct tp_observer_manager tp_observer_manager;
int tp_observer_new(int kind, size_t num_bins, tp_observer **out);
int tp_observer_free(tp_observer *o);
int tp_observer_set_enabled(tp_observer *o, int on);
int tp_observer_is_enabled(const tp_observer *o, int *out);
int tp_observer_observe(tp_observer *o, const tp_tensor *t);
int tp_observer_num_observations(const tp_observer *o, size_t *out);
int tp_observer_reset(tp_observer *o);
/* MinMax read-outs: the vectors' length (0 before the first observation), the vectors (each nullable), and get_stats -- global_min /
 * global_max are the NaN-ignoring folds from +inf / -inf, made on the device; range = global_max - global_min (-inf when empty) */
int tp_observer_minmax_len(const tp_observer *o, size_t *out);
int tp_observer_minmax_values(const tp_observer *o, float *h_min, float *h_max);
int tp_observer_minmax_stats(const tp_observer *o, size_t *num_observations, float *global_min, float *global_max, float *range);
/* Histogram read-outs: num_bins counts, the edges (tp_observer_hist_num_edges: num_bins + 1, or 0 while there are none), and get_stats:
 * mean_bin = (sum of i * count) as f32 / total_count as f32, 0 when empty */
int tp_observer_hist_num_bins(const tp_observer *o, size_t *out);
int tp_observer_hist_bins(const tp_observer *o, uint64_t *h_bins);
int tp_observer_hist_num_edges(const tp_observer *o, size_t *out);
int tp_observer_hist_edges(const tp_observer *o, float *h_edges);
int tp_observer_hist_stats(const tp_observer *o, size_t *num_observations, uint64_t *total_count, float *mean_bin, uint64_t *max_bin_count);
/* ObserverManager (observers.rs:268-345): observers by name, one map per kind; adding an existing name replaces the observer with a
 * fresh one; observing an unknown name does nothing, asking its stats sets *found = 0 -- neither is an error.  tp_observer_manager_names:
 * the minmax names then the histogram names, each sorted, '\n'-separated and NUL-terminated into buf (truncated to cap; nullable),
 * *n_names their number and *needed the bytes the whole list takes with its NUL. */
int tp_observer_manager_new(tp_observer_manager **out);
int tp_observer_manager_free(tp_observer_manager *m);
int tp_observer_manager_add_minmax(tp_observer_manager *m, const char *name);
int tp_observer_manager_add_histogram(tp_observer_manager *m, const char *name, size_t num_bins);
int tp_observer_manager_observe_minmax(tp_observer_manager *m, const char *name, const tp_tensor *t);
int tp_observer_manager_observe_histogram(tp_observer_manager *m, const char *name, const tp_tensor *t);
int tp_observer_manager_minmax_stats(const tp_observer_manager *m, const char *name, int *found, size_t *num_observations, float *global_min,
                                     float *global_max, float *range);
int tp_observer_manager_histogram_stats(const tp_observer_manager *m, const char *name, int *found, size_t *num_observations,
                                        uint64_t *total_count, float *mean_bin, uint64_t *max_bin_count);
int tp_observer_manager_reset_all(tp_observer_manager *m);
int tp_observer_manager_names(const tp_observer_manager *m, char *buf, size_t cap, size_t *n_names, size_t *needed);

/* ---- optim (src/optim.rs) ---- */
int tp_adam_new(tp_tensor *const *params, int n, float lr, float beta1, float beta2, float eps, float weight_decay,
                tp_optim **out);
int tp_sgd_new(tp_tensor *const *params, int n, float lr, tp_optim **out);
int tp_adamw_new(tp_tensor *const *params, int n, float lr, float beta1, float beta2, float eps, float weight_decay,
                 tp_optim **out);                                            /* optim.rs:130-180 */
int tp_optim_free(tp_optim *o);
int tp_optim_step(tp_optim *o);
int tp_optim_zero_grad(tp_optim *o);
int tp_adam_set_lr(tp_optim *o, float lr);
int tp_adam_get_lr(const tp_optim *o, float *out);
int tp_adam_t(const tp_optim *o, int *out);
int tp_adam_moments(const tp_optim *o, float *h_m, float *h_v);  /* concatenated in parameter order */
int tp_optim_total(const tp_optim *o, int64_t *out);             /* padded arena length (all-reduce size) */
int tp_adam_load_state(tp_optim *o, int t, const float *h_m, const float *h_v);  /* inverse of tp_adam_t / tp_adam_moments */

/* ---- LR schedulers (src/optim.rs:183-352) ---- */
int tp_sched_step_lr(float base_lr, size_t step_size, float gamma, tp_sched **out);
int tp_sched_exponential(float base_lr, float gamma, tp_sched **out);
int tp_sched_cosine(float base_lr, size_t t_max, float min_lr, tp_sched **out);
int tp_sched_plateau(float initial_lr, float factor, size_t patience, float min_lr, int mode_max, tp_sched **out);
int tp_sched_step(tp_sched *s, const float *metric /* NULL = None */);
int tp_sched_get_lr(const tp_sched *s, float *out);
int tp_sched_free(tp_sched *s);

/* ---- data (src/data/mnist.rs) ---- */
int tp_dataset_from_host(const float *h_images, const float *h_labels, size_t n, int train, tp_dataset **out);
int tp_dataset_from_idx(const char *images_path, const char *labels_path, int train, tp_dataset **out);
int tp_dataset_synthetic(size_t n, uint64_t seed, int train, tp_dataset **out);
int tp_dataset_len(const tp_dataset *d, size_t *out);
int tp_dataset_tensors(const tp_dataset *d, tp_tensor **images, tp_tensor **labels);
int tp_dataset_free(tp_dataset *d);
int tp_loader_new(const tp_dataset *d, size_t batch_size, int shuffle, uint64_t seed, tp_loader **out);
int tp_loader_reset(tp_loader *l);
int tp_loader_num_batches(const tp_loader *l, size_t *out);
int tp_loader_next(tp_loader *l, tp_tensor **images, tp_tensor **labels, int *has_batch);
int tp_loader_free(tp_loader *l);

/* ---- data parallel (new) ---- */
int tp_comm_unique_id(uint8_t out_id[128]);
int tp_comm_new(int n_ranks, int rank, const uint8_t id[128], tp_comm **out);
/* peer-to-peer communicator (th_comm_init_p2p): new -> export_arena(optimizer) -> ship all 192-byte blobs to all ranks ->
 * connect(blobs in rank order); the Trainer then runs all-reduce + Adam as one launch */
int tp_comm_new_p2p(int n_ranks, int rank, tp_comm **out);
/* The exchange inside the gradient launch (th_mlp_tail_dp; include/taper_hip.h): a Trainer over a peer-to-peer communicator takes it for
 * the Linear + ReLU + Linear step whenever tp_comm_tail_exchange_ok says the shapes and the placement of the ranks allow it
 * (tp_comm_set_inkernel(c, 0): never -- the three-launch form, for A/B runs).  tp_comm_new_loopback: W = 2 with this process as its own
 * peer -- the whole protocol through local memory, results bit-identical to the single-GPU step; what a 1-GPU box can time of it. */
int tp_comm_new_loopback(tp_comm **out);
int tp_comm_set_inkernel(tp_comm *c, int on);
int tp_comm_inkernel_launches(tp_comm *c, int64_t *out);
int tp_comm_exchange_selftest(tp_comm *c, int slots, int rounds, int *out_bad);   /* collective */
int tp_comm_ranks_on_this_device(tp_comm *c, int *out);
int tp_comm_exchange_form(tp_comm *c, int *out);   /* th_comm_exchange_form: 0 none, 1 one-shot, 2 two-shot */
int tp_comm_tail_exchange_ok(tp_comm *c, int batch, int in_features, int hidden, int classes, int *out);
int tp_comm_export_arena(tp_comm *c, tp_optim *optimizer, uint8_t out_blob[192]);
int tp_comm_connect(tp_comm *c, const uint8_t *blobs, size_t n_bytes);
/* fine_grained != 0: the optimizer's gradient arena is first moved into fine-grained device memory (coherent across agents, never cached
 * in a peer's L2): the fallback when the self-check fails on the pooled, coarse-grained arena.  The communicator keeps the registered
 * arenas alive; free it on every rank before the optimizer. */
int tp_comm_export_arena_ex(tp_comm *c, tp_optim *optimizer, int fine_grained, uint8_t out_blob[192]);
/* collective self-test (every rank calls it, before training): 3 (or `rounds`) all-reduces of patterns that differ per rank, round and
 * element through the SAME addresses of the optimizer's gradient arena, through the in-place kernel and then through the fused
 * all-reduce + Adam kernel (p / m / v against the closed form of optim.rs:83-113; state restored) */
int tp_comm_self_check(tp_comm *c, tp_optim *optimizer, int *ok);
int tp_comm_self_check_rounds(tp_comm *c, tp_optim *optimizer, int rounds, int *ok);
int tp_comm_timed_out(tp_comm *c, int *out);   /* synchronises the stream */
int tp_comm_failed(tp_comm *c, int *out);      /* the same verdict from the host-visible error word, no synchronisation; the Trainer throws on it after every epoch / eager step */
int tp_comm_set_timeout_ms(tp_comm *c, int64_t ms);   /* bound of the in-kernel waits for a peer (default 120 s; TAPER_P2P_TIMEOUT_MS) */
int tp_comm_set_fuse_adam(tp_comm *c, int on);        /* p2p: 1 (default) all-reduce + Adam in one launch, 0 all-reduce in place then Adam::step */
int tp_comm_stats(tp_comm *c, int64_t out2[2]);   /* {in-place, fused} one-shot launches enqueued or captured */
int tp_comm_free(tp_comm *c);
int tp_comm_allreduce_mean(tp_comm *c, void *d_buf, size_t n);
int tp_comm_count(tp_comm *c, int *out_ranks);                     /* th_comm_count: for RCCL, what ncclCommCount reports */
/* `reps` gradient exchanges + Adam as a Trainer step issues them, timed with events on the stream; collective (every rank calls it);
 * the optimizer state moves: for benchmarks, after the timed run */
int tp_comm_time_exchange(tp_comm *c, tp_optim *adam, int reps, float *us_per_exchange);

/* ---- train (src/train.rs, examples/train_mnist*.rs) ---- */
int tp_trainer_new(tp_module *model, tp_optim *adam, tp_trainer **out);
int tp_trainer_set_sample_shape(tp_trainer *t, const size_t *shape, int ndim);  /* e.g. {1,28,28} for the CNN */
int tp_trainer_set_comm(tp_trainer *t, tp_comm *c /* nullable */);
/* graph-path knobs: steps per hipGraph replay; fuse_head 1 = classifier head (last Linear + cross-entropy)
 * as one launch, 2 = additionally the backward of a Linear+ReLU layer in front of it in the same launch
 * (th_mlp_tail; falls back to 1 where unsupported), 0 = off; Adam updates in the epilogues of the
 * gradient kernels (ignored with a communicator) */
int tp_trainer_set_options(tp_trainer *t, int graph_chunk, int fuse_head, int fuse_adam);
int tp_trainer_free(tp_trainer *t);
/* one reference-literal step (examples/train_mnist.rs:89-121); reads loss / accuracy back */
int tp_trainer_train_step(tp_trainer *t, const tp_tensor *images, const tp_tensor *labels, float *loss, float *acc);
/* mode 0 = eager train_epoch (train.rs:98-144), 1 = hipGraph replay, 2 = evaluate (train.rs:147-172).
 * per_step (nullable) receives 2*num_batches floats {loss, n_correct}; max_steps 0 = whole epoch. */
int tp_trainer_run_epoch(tp_trainer *t, tp_loader *l, int mode, size_t max_steps, float *avg_loss, float *accuracy,
                         size_t *total_correct, size_t *total_samples, size_t *num_batches, float *per_step,
                         size_t per_step_cap);
/* What the last mode-1 call did, in order, as (kind, steps) pairs: 0 the state reset launched on its own, 1 steps enqueued eagerly (the
 * last, partial batch: a trailing (1, 1)), 2 / 3 a step graph captured / replayed, 4 / 5 a whole-call graph (reset + steps) captured /
 * replayed.  A read-only query, as the plan queries: n_out (nullable) receives the number of pairs, pairs (nullable) at most cap_pairs. */
int tp_trainer_last_replays(const tp_trainer *t, int64_t *pairs, size_t cap_pairs, size_t *n_out);

/* train.rs:175-261: fit = epochs of train + evaluate + scheduler.step(Some(val_loss)) + metrics + early
 * stop at val_acc > 0.99; graph != 0 trains through the captured step */
int tp_trainer_set_scheduler(tp_trainer *t, tp_sched *s /* nullable; shared with the caller's handle */);
int tp_trainer_fit(tp_trainer *t, tp_loader *train, tp_loader *val, size_t epochs, int verbose, int graph);
/* Metrics (train.rs:9-71): which = 0 train_loss, 1 train_acc, 2 val_loss, 3 val_acc, 4 epoch_times */
int tp_trainer_metrics(const tp_trainer *t, int which, float *h_out, size_t cap, size_t *n_out);
/* which = 0: the print_last line, 1: the plot_summary text (NUL-terminated, truncated to cap) */
int tp_trainer_metrics_text(const tp_trainer *t, int which, char *buf, size_t cap);
/* train.rs:264-292 text checkpoint and its inverse; the optimizer-state pair is an extension */
int tp_trainer_save_checkpoint(const tp_trainer *t, const char *path);
int tp_trainer_load_checkpoint(tp_trainer *t, const char *path);
int tp_trainer_save_optimizer_state(const tp_trainer *t, const char *path);
int tp_trainer_load_optimizer_state(tp_trainer *t, const char *path);
/* an f32 as Rust's `{}` prints it (the checkpoint's number format) */
int tp_format_f32(float v, char *buf, size_t cap);

#ifdef __cplusplus
}
#endif
#endif /* TAPER_HOST_H */
