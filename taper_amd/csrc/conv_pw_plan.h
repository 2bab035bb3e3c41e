// conv_pw_plan.h -- which kernel instance an exact pointwise (1x1) convolution call takes (th_conv1x1_exact_fwd / _bwd_input / _bwd_weight),
// as plain host data in the manner of conv_s2_plan.h: one host function per entry point fills a ConvPwPlan, the launch code in conv_pw.hip
// reads it and decides nothing itself, and th_debug_conv1x1_exact_plan (include/taper_hip_debug.h) hands the same plan to the tests.
#ifndef TAPER_CONV_PW_PLAN_H
#define TAPER_CONV_PW_PLAN_H

namespace th {

// (2 GiB: what a buffer descriptor with 32-bit byte offsets covers -- the images one pixel tile can touch (forward: of x, input gradient:
// of gy), the whole maps of the weight gradient.  GRID: a launch grid over the device limit, or 2^31 output pixels and more.)
enum ConvPwRefusal { CONV_PW_OK = 0, CONV_PW_REFUSED_GRID = 1, CONV_PW_REFUSED_2GIB = 2 };

// every field is an int: th_debug_conv1x1_exact_plan copies the struct out as it stands (kConvPwPlanInts of them, in this order)
struct ConvPwPlan {
    int op;           // 0 forward, 1 input gradient, 2 weight gradient
    int ct;           // 16-channel tiles per workgroup (CT: 1 / 2 / 4) -- output channels (ops 0, 2), input channels (op 1)
    int acc;          // the call accumulates into its output (a kernel argument for op 1, the reduce ending for op 2)
    int stride;       // 1 or 2
    int px_t;         // pixels of the flat (image, oh, ow) axis per workgroup tile (ops 0, 1) or pixel block (op 2)
    int span;         // ops 0, 1: the most images one tile touches (what its buffer descriptor covers)
    int tiles;        // ceil(n h_out w_out / px_t)
    int grid_x, grid_y, grid_z;
    int lds;          // LDS bytes of the launch
    int lds_limit;    // what the launch may request for this kernel
    int G;            // op 2: pixel-block classes (grid.x)
    int slabs;        // op 2: partial slabs wgrad_reduce adds
    int reduce;       // op 2: ConvReduce (conv_plan.h)
    int ci_slab;      // op 2: input channels per slab (grid.y = ceil(c_in / ci_slab))
    int co_ld;        // op 2: channel pitch of a partial slab
    int refused;      // ConvPwRefusal
    int h_out, w_out;
};
constexpr int kConvPwPlanInts = (int)(sizeof(ConvPwPlan) / sizeof(int));

void conv_pw_fwd_plan(ConvPwPlan *p, int n, int c_in, int h, int w, int c_out, int stride);
void conv_pw_bwd_input_plan(ConvPwPlan *p, int n, int c_in, int h, int w, int c_out, int stride, bool accumulate);
void conv_pw_bwd_weight_plan(ConvPwPlan *p, int n, int c_in, int h, int w, int c_out, int stride, int layout, bool accumulate, bool gw_aligned);

}  // namespace th

#endif
