// conv_s2_plan.h -- which kernel instance a stride-2 3x3 convolution call takes (th_conv3x3_s2_fwd / _bwd_input / _bwd_weight), as plain
// host data in the manner of conv_plan.h: one host function per entry point fills a ConvS2Plan, the launch code in conv_s2.hip reads it
// and decides nothing itself, and th_debug_conv3x3_s2_plan (include/taper_hip_debug.h) hands the same plan to the tests.  These kernels
// never go through conv3x3_plan.
#ifndef TAPER_CONV_S2_PLAN_H
#define TAPER_CONV_S2_PLAN_H

namespace th {

// (2 GiB: the whole maps of the weight gradient, one image's input (forward) or gradient (input gradient): what a buffer descriptor with
// 32-bit byte offsets covers)
enum ConvS2Refusal { CONV_S2_OK = 0, CONV_S2_REFUSED_GRID = 1, CONV_S2_REFUSED_2GIB = 2 };

// every field is an int: th_debug_conv3x3_s2_plan copies the struct out as it stands (kConvS2PlanInts of them, in this order)
struct ConvS2Plan {
    int op;           // 0 forward, 1 input gradient, 2 weight gradient
    int ct;           // 16-channel tiles per workgroup (CT: 1 / 2 / 4) -- output channels (ops 0, 2), input channels (op 1)
    int acc;          // the call accumulates into its output (a kernel argument for op 1, the reduce ending for op 2)
    int img_t;        // images per workgroup tile
    int rows_t;       // output rows per workgroup tile
    int cols_t;       // output columns per workgroup tile (w_out when one column block holds the row)
    int bands;        // ceil(h_out / rows_t)
    int cblks;        // ceil(w_out / cols_t)
    int grid_x, grid_y, grid_z;
    int lds;          // dynamic LDS bytes of the launch
    int lds_limit;    // what the launch may request for this kernel
    int G;            // op 2: pixel-block classes (grid.x)
    int slabs;        // op 2: partial slabs wgrad_reduce adds
    int reduce;       // op 2: ConvReduce (conv_plan.h)
    int n_pb;         // op 2: pixel blocks
    int co_ld;        // op 2: channel pitch of a partial slab
    int refused;      // ConvS2Refusal
    int h_out, w_out;
};
constexpr int kConvS2PlanInts = (int)(sizeof(ConvS2Plan) / sizeof(int));

void conv3x3_s2_fwd_plan(ConvS2Plan *p, int n, int c_in, int h, int w, int c_out);
void conv3x3_s2_bwd_input_plan(ConvS2Plan *p, int n, int c_in, int h, int w, int c_out, bool accumulate);
void conv3x3_s2_bwd_weight_plan(ConvS2Plan *p, int n, int c_in, int h, int w, int c_out, int layout, bool accumulate, bool gw_aligned);

}  // namespace th

#endif
