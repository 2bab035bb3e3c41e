// conv_plan.h -- which kernel instance a 3x3 convolution call takes, as plain host data.  Every decision of th_conv3x3_fwd / _pool2_fwd /
// _gap_fwd / _bwd_input / _bwd_weight (c_in, c_out, plane, batch, workgroup counts, pointer alignment, th_debug_set_conv_img) is taken by
// the host functions declared here, which fill a ConvPlan; the launch code reads the plan and decides nothing itself, and
// th_debug_conv3x3_plan (include/taper_hip_debug.h) hands the same plan to the tests.  No device call anywhere in them.
#ifndef TAPER_CONV_PLAN_H
#define TAPER_CONV_PLAN_H

namespace th {

enum ConvFamily {
    CONV_F_REFUSED = 0,       // the call returns an error before any allocation or launch (ConvPlan::refused says why)
    CONV_F_CONV1 = 1,         // conv1_kernel / conv1_pool2_kernel (pool = 1): one input channel, taper layout, plane <= 48 KB
    CONV_F_TILE = 2,          // conv3x3_kernel<ACC>: 2 x 4 pixel tiles on the vector ALUs
    CONV_F_ROWS = 3,          // conv3x3_rows_kernel<PX, ACC>
    CONV_F_MFMA = 4,          // conv3x3_mfma_kernel<CT, ACC, CIT, POOL, WH, DMA>
    CONV_F_IMG = 5,           // conv3x3_img_kernel<CT, TPW, POOL, WP, CIS>
    CONV_F_CHAIN = 6,         // conv_layer_chain_kernel<S, C_IN, C_OUT, POST, LIN>
    CONV_F_WGRAD_MFMA = 7,    // conv3x3_wgrad_mfma_kernel<CT, PQ>
    CONV_F_WGRAD_IMG = 8,     // conv_wgrad_img_kernel (three compiled shapes)
    CONV_F_WGRAD_CONV1 = 9,   // conv1_wgrad_kernel
    CONV_F_WGRAD_VEC = 10,    // conv3x3_bwd_weight_kernel, slabs == 0: straight into gw; slabs > 0: image slabs
};
enum ConvReduce { CONV_R_NONE = 0, CONV_R_SLAB_SUM = 1, CONV_R_COLSUM = 2, CONV_R_COLSUM_ACCUM = 3, CONV_R_SCATTER = 4 };
enum ConvRefusal { CONV_OK = 0, CONV_REFUSED_LDS = 1, CONV_REFUSED_GAP = 2, CONV_REFUSED_POOL = 3, CONV_REFUSED_PAD = 4, CONV_REFUSED_WGRAD = 5 };

// every field is an int: th_debug_conv3x3_plan copies the struct out as it stands (kConvPlanInts of them, in this order)
struct ConvPlan {
    int family;
    int ct;           // MFMA / IMG / WGRAD_MFMA: 16-channel tiles per workgroup (CT); WGRAD_IMG: CTW
    int acc;          // the ACC instance (accumulate into the output)
    int cit;          // MFMA: input channels per pass (8, or 1)
    int pool;         // fused 2x2 max pool (MFMA / IMG POOL instance, conv1_pool2_kernel, chain post 1)
    int wh;           // MFMA: WH (1 / 2); other families 0
    int dma;          // MFMA: the DMA instance
    int tpw;          // IMG: pixel tiles per wave (4 / 7 / 13)
    int wp, cis;      // IMG: compiled patch geometry (0, 0: the generic instance)
    int px;           // ROWS: PX (4 / 2 / 1)
    int prep;         // 1: weights go through conv3x3_prep_weights into a pool allocation; 0: read in place
    int img_t;        // images per workgroup (WGRAD_IMG: IPW)
    int rows_t;       // MFMA / WGRAD_MFMA: output rows per workgroup band
    int bands;        // MFMA / WGRAD_MFMA: ceil(h_out / rows_t); WGRAD_IMG: BANDS
    int grid_x, grid_y, grid_z;
    int tile_store;   // IMG: plain output through an LDS tile
    int gap;          // fused global average pool (IMG gap mode, chain post 2)
    int lds;          // dynamic LDS bytes of the launch
    int lds_limit;    // what the launch may request for this kernel
    int post;         // CHAIN: 0 / 1 / 2
    int lin;          // CHAIN: the LIN instance (no bias, no ReLU)
    int G;            // WGRAD_MFMA: pixel-block classes (grid.x)
    int slabs;        // op 4: partial slabs wgrad_reduce adds (0: none, the kernel writes gw itself)
    int reduce;       // op 4: ConvReduce
    int pq;           // WGRAD_MFMA: PQ (1 / 2); WGRAD_IMG: PS
    int n_pb;         // WGRAD_MFMA: pixel blocks
    int co_ld;        // op 4: channel pitch of a partial slab
    int refused;      // ConvRefusal
    int h_out, w_out;
};
constexpr int kConvPlanInts = (int)(sizeof(ConvPlan) / sizeof(int));

// conv_chain.hip: true if a compiled one-stage chain takes the layer (fills family, ct, post, lin, grid, lds, lds_limit)
bool conv_layer_chain_plan(int n, int c_in, int hw, int c_out, int post, bool linear, ConvPlan *p);
// conv_mfma.hip: the matrix-core forward (chain, image-resident or 128-pixel kernel); weights [9 c_in][w_ld].  img_mode as g_conv_img_mode
void conv3x3_mfma_plan(ConvPlan *p, int n, int c_in, int h, int w_in, int c_out, int pad, int w_ld, int w_cols, bool relu, bool has_bias,
                       bool accum, bool pool, bool gap, int img_mode);
// conv_mfma.hip: the matrix-core weight gradient (image-resident or slab kernel) and its reduce ending
void conv3x3_wgrad_mfma_plan(ConvPlan *p, int n, int c_in, int h, int w_in, int c_out, int pad, int layout, bool accumulate, bool gw_aligned);
int wgrad_reduce_plan(int G, int kt, int c_out, int co_ld, int layout, bool accumulate, bool aligned);
// conv_pool.hip: the vector-ALU forward
void conv3x3_vec_plan(ConvPlan *p, int n, int in_ch, int h, int w, int out_ch, int co_pad, int pad, bool accum);
// conv_pool.hip: a whole entry point.  op: 0 fwd, 1 pool2 fwd, 2 gap fwd, 3 bwd_input, 4 bwd_weight; w_aligned: the weight pointer (op 4: gw)
// is 16-byte aligned.  The geometry is the entry point's own (already checked).
void conv3x3_plan(ConvPlan *p, int op, int n, int c_in, int h, int w, int c_out, int pad, int weight_layout, bool relu, bool has_bias,
                  bool accumulate, bool w_aligned, int img_mode);
extern int g_conv_img_mode;

}  // namespace th

#endif
