// fwd_tick.hip -- th_linear_fwd_ex's one-launch kernel (gemm.hip: fwd_ex_plan chooses its form): the (sub-)tiles of H = relu(X . W^T + b)
// on the grid's tile rows, and on the spare row ONE workgroup that applies the carried Adam slices with the step counter as it stands and
// then opens the next step (t += 1).
//
// A translation unit of its own because of its ARGUMENTS.  The launch is latency-bound, and a tile wave can ask for X and W1 only when it
// holds their addresses.  So the signature opens with what the operand requests need, as flat scalars (ten dwords, the first cache line of
// the argument block), and everything else follows in one struct; the tile path uses neither gridDim nor any other hidden argument, and it
// asks for X and W before it needs the struct.  As SmallArgs + AdamSlices + tick (0x228 bytes, the form sgemm_small16 keeps) a tile wave
// stood at six scalar waits over four cache lines before its first operand request (profiles/mlp_fwd_args.md).  Ten leading scalars are also
// what kernel-argument preload (-mllvm -amdgpu-kernarg-preload-count=10) hands a wave in SGPRs at launch: measured, no gain that clears the
// project's rule on top of this form, so the object is built without it (experiments/README.md).
// The body is small16_dev.h's: the same MFMAs over the same chunks, the same wave-ordered sums, the same epilogue arithmetic as sgemm_small16.
#include "small16_dev.h"

namespace th {

constexpr int kFwdAVec = 1, kFwdBVec = 2, kFwdXcd = 4;   // `flags`: 16-byte loads of X / of W, the XCD map

struct FwdTickRest {
    float *C;
    const float *bias;   // nullable
    int relu;
    int32_t *tick;       // nullable
    AdamSlices x;        // (carries the update guard)
};

// grid = (grid_x, tile_rows + 1); block = 64 * NW.  The tiles are this launch's tail, not the spare workgroup: measured in situ it adds
// 0.08-0.11 us to the step over plain tiles (tools/step_tails_probe.py, profiles/mlp_step_tails.md).
template <int NW, int RM, int RN>
__global__ __launch_bounds__(64 * NW) void sgemm_small16_tick(const float *X, const float *W, int m, int n, int k, int tile_rows, int grid_x,
                                                              int flags, FwdTickRest r) {
#ifdef TH_PROFILE
    __builtin_amdgcn_sched_barrier(0);
    const long long t_entry = wall_clock64();   // in front of any argument use
    __builtin_amdgcn_sched_barrier(0);
#endif
    __shared__ float red[NW][64][4];
    if ((int)blockIdx.y < tile_rows) {
        int tm = blockIdx.y, tn = blockIdx.x;
        const int b = blockIdx.x + grid_x * blockIdx.y;
        if (flags & kFwdXcd) {
            // 64 x 128 outputs (the MNIST MLP's layer 1 at batch 64): block b runs on XCD b % 8; give every XCD the (sub-)tiles of one 32 x 32
            // block of H instead of a column of them, so its L2 fetches 32 rows of X and 32 of W (200 KB) instead of all of X and 16 of W (250 KB)
            constexpr int SBM = 32 / RM, SBN = 32 / RN;
            static_assert(SBN == 2 || SBN == 4, "sub-tiles of 16 or 8 columns");
            const int q = b & 7, j = b >> 3;
            tm = SBM * (q >> 2) + (j >> (SBN == 4 ? 2 : 1));
            tn = SBN * (q & 3) + (j & (SBN - 1));
        }
        // X [m][k] and W [n][k], both k-contiguous; no K split between workgroups; alpha 1, beta 0, no fused update
        const SmallArgs p{X, nullptr, W, r.C, nullptr, m, n, k, k, 1, 1, k, (k + 15) / 16 * 16, flags & kFwdAVec, flags & kFwdBVec,
                          Epilogue{1.0f, 0.0f, r.bias, r.relu, AdamDev{nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, 0.f, 0.f}, nullptr, nullptr}};
        // the operand requests go out first; bias (and later C) come from `r`, whose fetch lies under them
#ifdef TH_PROFILE
        small16_body<true, true, NW, false, RM, RN, true, true>(p, tm, tn, 0, red, t_entry, b);
#else
        small16_body<true, true, NW, false, RM, RN, false, true>(p, tm, tn, 0, red);
#endif
        return;
    }
    if (blockIdx.x == 0) adam_slices_then_tick(r.x, r.tick);
}

int fwd_tick_launch(th_ctx *ctx, const FwdTickLaunch &q, const float *d_x, const float *d_w, const float *d_b, float *d_y, int m, int n, int k,
                    int relu, const AdamSlices &x, int32_t *d_tick) {
    const FwdTickRest r{d_y, d_b, relu, d_tick, x};
    const int flags = (q.a_vec ? kFwdAVec : 0) | (q.b_vec ? kFwdBVec : 0) | (q.xcd_blocks ? kFwdXcd : 0);
    const dim3 grid(q.grid_x, q.grid_y, 1);
    const int tile_rows = q.grid_y - 1;
    if (q.rm == 8) hipLaunchKernelGGL((sgemm_small16_tick<16, 8, 8>), grid, dim3(1024), 0, ctx->stream, d_x, d_w, m, n, k, tile_rows, q.grid_x, flags, r);
    else if (q.waves == 16) hipLaunchKernelGGL((sgemm_small16_tick<16, 16, 16>), grid, dim3(1024), 0, ctx->stream, d_x, d_w, m, n, k, tile_rows, q.grid_x, flags, r);
    else hipLaunchKernelGGL((sgemm_small16_tick<4, 16, 16>), grid, dim3(256), 0, ctx->stream, d_x, d_w, m, n, k, tile_rows, q.grid_x, flags, r);
    TH_LAUNCH_CHECK();
    return 0;
}

}  // namespace th

#ifdef TH_PROFILE
extern "C" int th_debug_fwd_prof(th_ctx *ctx, long long *h_out, int n_blocks) {
    TH_REQUIRE(ctx && h_out && n_blocks >= 1 && n_blocks <= th::kFwdProfBlocks, "th_debug_fwd_prof: bad argument");
    TH_HIP(hipStreamSynchronize(ctx->stream));
    TH_HIP(hipMemcpyFromSymbol(h_out, HIP_SYMBOL(th::g_fwd_prof), (size_t)n_blocks * 2 * th::kFwdProfStamps * sizeof(long long)));
    return 0;
}
#endif
