/* taper_hip_debug.h -- test hooks of libtaper_hip.so.  NOT part of the drop-in boundary (include/taper_hip.h): a host binding never needs
 * them.  The parity tests use them to assert WHICH kernel instance / step form a call took, and the measurement tools to force one. */
#ifndef TAPER_HIP_DEBUG_H
#define TAPER_HIP_DEBUG_H

#include "taper_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* how many th_mlp3_xent / th_mlp2_xent calls this thread has enqueued (which form a Trainer step took) */
int th_debug_mlp3_calls(int64_t *out);
int th_debug_mlp2_calls(int64_t *out);
/* measurement hook: 1 / 2 / 3 = th_mlp2_xent enqueues only that launch (rows / dW1 / finish) on this thread, so that each can be timed with
 * events on its own (the pool hands the same workspace back from call to call: launches 2 and 3 read what an earlier full call left); 0 = the step */
int th_debug_mlp2_only(int which);
/* 1 .. 8 = th_mlp2_xent splits a 16-row block's k chunks over that many workgroups on this thread whatever the cap says (the repro tests
 * walk the hand-off's forms); 0 = the default choice */
int th_debug_mlp2_ksplit(int ksplit);
/* 1 = conv chains over more than 256 images run as min(n, 256) workgroups that WALK the images (r05: bit-identical, measured 3 - 5 % slower
 * than one workgroup per image, off by default); 0 / -1 = default */
int th_debug_set_chain_loop(int on);
/* 1: th_conv_chain_mlp3_xent enqueues its first launch (the chain with the classifier's rows) alone -- per-launch timing; 0: both */
int th_debug_chain_mlp3_only(int which);
/* 1 = the compiled chain instances are not used on this thread (their nets take the run-time-described kernel, id 3); 0 = default */
int th_debug_set_chain_generic(int on);
/* launch configuration of the most recent matrix-core 3x3 convolution this thread enqueued (the parity
 * tests assert which kernel instance a shape takes): out6 = {16-channel tiles per workgroup (1/2/4), 1 if the
 * operands are staged by LDS-DMA (2 / 4: the image-resident kernel, generic / compiled patch geometry; 6: a conv chain, out6[0] = its instance id), waves per workgroup / 4, grid.x, grid.y, 1 if the epilogue is the fused 2x2 pool}. */
int th_debug_last_conv_config(th_ctx *ctx, int *out6);
/* which matrix-core kernel takes a 3x3 launch.  -1 (default): the image-resident kernel (whole images per
 * workgroup, every output tile in registers; out6[1] == 2 in th_debug_last_conv_config, out6[2] = pixel tiles per wave,
 * out6[4] = images per unit) when the launch has at least one unit per two CUs, the 128-pixel kernel otherwise; 0: never;
 * 1: whenever the shape fits it. */
int th_debug_set_conv_img(th_ctx *ctx, int mode);
/* what a 3x3 convolution entry point would do with this shape -- pure host code, no context, the function the launch itself consumes
 * (csrc/conv_plan.h: ConvPlan, copied out field by field).  op: 0 th_conv3x3_fwd, 1 _pool2_fwd, 2 _gap_fwd, 3 _bwd_input, 4 _bwd_weight;
 * relu_bias = relu + 2 * (bias present) (ops 0 - 2); accumulate: ops 3 and 4; w_misalign_bytes: the weight pointer (op 4: the gradient's)
 * off a 16-byte boundary; img_mode as th_debug_set_conv_img.  out32 = {family (0: the call is refused before any allocation or launch;
 * 1 conv1 / conv1_pool2; 2 conv3x3_kernel; 3 conv3x3_rows_kernel; 4 conv3x3_mfma_kernel; 5 conv3x3_img_kernel; 6 conv_layer_chain_kernel;
 * 7 conv3x3_wgrad_mfma_kernel; 8 conv_wgrad_img_kernel; 9 conv1_wgrad_kernel; 10 conv3x3_bwd_weight_kernel), CT (wgrad image form: CTW),
 * ACC, CIT, POOL, WH, DMA, TPW, compiled WP, compiled CIS, PX, 1 if the weights go through conv3x3_prep_weights (0: read in place),
 * images per workgroup, rows per band, bands, grid x, y, z, tile_store, gap, LDS bytes, the LDS limit of that launch, chain post, chain LIN,
 * G, partial slabs (0: none), reduce ending (0 none; 1 slab_sum_kernel; 2 th_colsum; 3 th_colsum_accum; 4 th_colsum + wgrad_scatter_kernel),
 * PQ (wgrad image form: PS), pixel blocks, slab channel pitch, refusal (1 plane over the LDS tile, 2 no gap plan, 3 no pool plan,
 * 4 pad, 5 weight-gradient limits), h_out, w_out}.  Nonsense geometry is an error that names it; a shape the entry point refuses is family 0. */
int th_debug_conv3x3_plan(int op, int n, int c_in, int h, int w, int c_out, int pad, int weight_layout, int relu_bias, int accumulate,
                          int w_misalign_bytes, int img_mode, int *out32);
/* what a stride-2 3x3 convolution entry point would do with this shape -- pure host code, no context, the function the launch itself
 * consumes (csrc/conv_s2_plan.h: ConvS2Plan, copied out field by field).  op: 0 th_conv3x3_s2_fwd, 1 _bwd_input, 2 _bwd_weight; h, w: the
 * input's; relu_bias = relu + 2 * (bias present) (op 0); accumulate: ops 1 and 2; w_misalign_bytes: the gradient pointer of op 2 off a
 * 16-byte boundary (the weights are read element by element: their alignment decides nothing).  out21 = {op, CT (16-channel tiles per
 * workgroup), accumulate, images, output rows, output columns per workgroup tile, row bands, column blocks, grid x, y, z, LDS bytes, the
 * LDS limit of that launch, G, partial slabs, reduce ending (as th_debug_conv3x3_plan), pixel blocks, slab channel pitch, refusal (0: the
 * call launches; 1 grid over the device limit, 2 weight gradient of maps of 2 GiB and more), h_out, w_out}. */
int th_debug_conv3x3_s2_plan(int op, int n, int c_in, int h, int w, int c_out, int weight_layout, int relu_bias, int accumulate,
                             int w_misalign_bytes, int *out21);
/* what this thread's most recent th_conv3x3_s2_* call launched: out8 = {op, CT, accumulate, grid x, y, z, LDS bytes, reduce ending}
 * (op -1: none yet) */
int th_debug_last_conv_s2_config(th_ctx *ctx, int *out8);
/* what an exact pointwise convolution entry point would do with this shape -- pure host code, no context, the function the launch itself
 * consumes (csrc/conv_pw_plan.h: ConvPwPlan, copied out field by field).  op: 0 th_conv1x1_exact_fwd, 1 _bwd_input, 2 _bwd_weight; h, w: the
 * input's; relu_bias = relu + 2 * (bias present) (op 0); accumulate: ops 1 and 2; w_misalign_bytes: the gradient pointer of op 2 off a
 * 16-byte boundary.  out20 = {op, CT (16-channel tiles per workgroup), accumulate, stride, pixels of the flat (image, oh, ow) axis per
 * workgroup tile, the most images one tile touches (ops 0, 1), tiles, grid x, y, z, LDS bytes, the LDS limit of that launch, G, partial
 * slabs, reduce ending (as th_debug_conv3x3_plan), input channels per slab (op 2), slab channel pitch, refusal (0: the call launches; 1 grid
 * over the device limit or 2^31 output pixels and more, 2 operand of 2 GiB and more behind one descriptor), h_out, w_out}. */
int th_debug_conv1x1_exact_plan(int op, int n, int c_in, int h, int w, int c_out, int stride, int weight_layout, int relu_bias, int accumulate,
                                int w_misalign_bytes, int *out20);
/* what this thread's most recent th_conv1x1_exact_* call launched: out9 = {op, CT, accumulate, stride, grid x, y, z, LDS bytes, reduce
 * ending} (op -1: none yet) */
int th_debug_last_conv_pw_config(th_ctx *ctx, int *out9);
/* what th_linear_q8_fwd (qtype TH_QTYPE_INT8) / th_linear_h16_fwd (TH_QTYPE_F16) would do with this shape and these pointers
 * (x / w: bytes off a 16-byte boundary) -- pure host code, no context, the function the launch itself consumes: out8 = {1 if the weight-
 * streaming kernel takes it (0: the dequantize workspace and th_linear_fwd; the rest is 0 then), 1 if its vector-load instance, batch tile
 * (1 / 2 / 4 / 8), k positions per slice, slices (grid.y; > 1: a combine launch follows), grid.x, slices asked for, k steps of a wave over
 * a whole row}. */
int th_debug_qlinear_plan(int qtype, int batch, int in_features, int out_features, int x_misalign_bytes, int w_misalign_bytes, int *out8);
/* what th_linear_q8q8_fwd would do with this shape -- pure host code, the function the launch itself consumes: out4 = {1 if the few-rows
 * form takes it (a workgroup per 32 x 32 tile, K split over its four waves; 0: the 128 x 128 form through LDS), tile rows, tile columns,
 * workgroups} */
int th_debug_q8q8_plan(int batch, int in_features, int out_features, int *out4);
/* what th_conv2d_q8q8_fwd would do with this shape -- pure host code, the function the launch itself consumes: out8 = {32-channel MFMA
 * tiles per workgroup (1 / 2 / 4, by c_out alone), pixels per workgroup tile (128), channels per workgroup tile (32 times the first),
 * pixel tiles, channel tiles, workgroups, h_out, w_out}.  Refuses what the launch refuses of a shape, and n < 1. */
int th_debug_qconv_plan(int n, int c_in, int h, int w, int c_out, int k_h, int k_w, int s_h, int s_w, int pad_h, int pad_w, int *out8);
/* what th_sgemm / th_linear_fwd (trans 0, 1) would do with this shape, layout and pointers (a / b / c: bytes off a 16-byte boundary: 0, 4,
 * 8 or 12) under a plain epilogue -- pure host code, no context, the function gemm_dispatch itself launches from: out12 = {tile class (16 /
 * 64 / 128), load form (0: 16 x 16 tiles straight from L2; 1: whole tiles by LDS-DMA; 2: LDS-DMA with the edge quads zeroed by the
 * descriptor's range; 3: clamped float4 register loads; 4: scalar register loads), waves per workgroup, a_vec, b_vec (16-tiles: float4 loads
 * of that operand; else both = 16-byte rows and whole quads), K slices, k positions per slice, workgroups, 1 if a split launch hands its
 * slices to the XCDs one by one, reduce pass (0: none; 1: splitk_reduce4; 2: splitk_reduce), tile rows, tile columns}.  k == 0 is a shape. */
int th_debug_sgemm_plan(int trans_a, int trans_b, int m, int n, int k, int a_misalign_bytes, int b_misalign_bytes, int c_misalign_bytes, int *out12);
/* what th_linear_fwd_ex would launch for this shape with the context's sub-tile switch on (1) or off (0) -- pure host code, no context, the
 * function the launch itself consumes: out8 = {1 if the one-launch path takes it (0: slices, tick and th_linear_fwd as launches of their own;
 * the rest is 0 then), sub-tile rows, sub-tile columns (16 x 16: the whole MFMA tile), waves per workgroup, K chunks per wave (1), grid.x
 * (sub-tile columns), grid.y (sub-tile rows + the spare row), 1 if every XCD takes the sub-tiles of one 32 x 32 block of the output}. */
int th_debug_linear_fwd_ex_plan(int batch, int in_features, int out_features, int subtiles, int *out8);

/* post-mortem of the in-launch exchange (csrc/dp_dev.h) on stderr: the communicator's state words and, per parity and source block of the
 * receive region, the slots that hold words.  Trainer::check_comm calls it under TAPER_DP_POSTMORTEM=1 when a time-out is reported. */
int th_comm_debug_dump(th_comm *comm, th_ctx *ctx);
#ifdef __cplusplus
}
#endif

#endif /* TAPER_HIP_DEBUG_H */
