// small16_dev.h -- the small / latency-bound sgemm body: one workgroup per 16 x 16 MFMA tile (or a sub-tile of it), operands straight
// from L2, the waves split K.  Shared by gemm.hip (sgemm_small16, linear_bwd_small, mlp3_grads_kernel) and fwd_tick.hip (th_linear_fwd_ex's
// one-launch kernel): one source, so every caller sums the same chunks in the same order.
#pragma once
#include "adam_dev.h"

namespace th {

typedef float floatx4 __attribute__((ext_vector_type(4)));

struct Epilogue {
    float alpha, beta;
    const float *bias;  // per output column (n), nullable
    int relu;
    AdamDev adam;       // adam.p != nullptr: C is a complete gradient and the Adam update of the
                        // parameter at the same index runs right here (th_linear_bwd_adam)
    // sgemm_tile, unsplit launches only (th_linear_bwd_adam_ex2): the backward of the fused Linear + ReLU IN FRONT of a layer, folded into that
    // layer's dX product -- C <- C * [mask > 0] (mask: the layer's input, [m][n] like C; ops.rs:358-369) and colpart [tiles_m][n] (nullable):
    // column sums of the stored tile rows, which th_colsum over the tile rows turns into the bias gradient of the layer in front (tensor.rs:686-691)
    const float *mask;
    float *colpart;
};

// ------------------------------------------------------------------------
// small / latency-bound kernel
// ------------------------------------------------------------------------
// One workgroup (NW waves) per 16x16 output tile; wave w covers its share of
// [kbeg_slice, kend_slice).  Lane l: r = l & 15 (row of A / col of B),
// g = l >> 4 (which 4-wide k group).  In MFMA step s the lane supplies
// k = kk + 4*g + s for BOTH operands, so every k is used exactly once.
// MASKED: A values are multiplied by (Amask[same index] > 0) on the fly -- the
// ReLU backward (ops.rs:358-369) folded into the operand load of the two
// backward GEMMs of a Linear layer.
struct SmallArgs {
    const float *A, *Amask, *B;
    float *C, *partial;
    int m, n, k;
    long a_rs, a_cs, b_rs, b_cs;
    int kslice, a_vec, b_vec;
    Epilogue ep;
    int xcd_blocks = 0;   // unused (the forward launch's XCD map is an argument of its own kernel, fwd_tick.hip); kept for the layout
};

// th_linear_fwd_ex's one-launch path: gemm.hip decides (fwd_ex_plan, the alignment of X and W), fwd_tick.hip launches
struct FwdTickLaunch {
    int rm, waves, grid_x, grid_y, xcd_blocks;
    bool a_vec, b_vec;   // 16-byte operand loads: the pointer 16-byte aligned and k a multiple of 4
};
int fwd_tick_launch(th_ctx *ctx, const FwdTickLaunch &q, const float *d_x, const float *d_w, const float *d_b, float *d_y, int m, int n, int k,
                    int relu, const AdamSlices &x, int32_t *d_tick);

#ifdef TH_PROFILE
// stamps 0..5 of th_linear_fwd_ex's launch (tools/prof_fwd.py): per workgroup, lane 0 of wave 0 ([0]) and of the last wave that owns a whole
// chunk ([1]); 100 MHz wall clock.  Slot 6: the kernel's true entry, read in front of any argument use (fwd_tick.hip).  Nothing else reads the
// buffer; it belongs to the translation unit that launches the stamped instance.
constexpr int kFwdProfBlocks = 320;
constexpr int kFwdProfStamps = 8;
static __device__ __attribute__((unused)) long long g_fwd_prof[kFwdProfBlocks][2][kFwdProfStamps];
#define FWD_STAMP(i)                                                                          \
    do {                                                                                      \
        if constexpr (STAMPED) {                                                              \
            __builtin_amdgcn_sched_barrier(0);                                                \
            if (stamp_slot >= 0) g_fwd_prof[stamp_blk][stamp_slot][i] = wall_clock64();       \
            __builtin_amdgcn_sched_barrier(0);                                                \
        }                                                                                     \
    } while (0)
// the value must be in its register: the compiler waits for the load (or the MFMA) that writes it in front of this point
#define FWD_LANDED(v) do { if constexpr (STAMPED) asm volatile("" ::"v"(v)); } while (0)
#else
#define FWD_STAMP(i) do { } while (0)
#define FWD_LANDED(v) do { } while (0)
#endif

// RM x RN (powers of two up to 16): the workgroup owns that SUB-TILE of a 16 x 16 MFMA tile (th_linear_fwd_ex).  Every output element of
// v_mfma_f32_16x16x4_f32 is its own FMA chain over k (experiments/mfma_fma_chain.hip), so feeding RM rows of A and RN of B into the same
// MFMAs over the same chunks, and dropping the C/D elements outside, gives the bits of the 16 x 16 form.  Lanes past the sub-tile alias one of
// its rows (no further cache line) and supply zeros; the C/D elements outside the sub-tile are neither summed nor stored.
// EP_LATE: what the epilogue needs from memory is requested BEHIND the first round of operand loads instead of in front of it -- for a caller
// whose operand addresses are known before its epilogue pointers are (fwd_tick.hip); the same requests, the same arithmetic.
// stamp_entry / stamp_blk: profile build only (the caller's entry reading and workgroup number).
#define SMALL16_REQUEST_EPILOGUE()                                                    \
    do {                                                                              \
        if (e_ok) {                                                                   \
            if (p.ep.beta != 0.0f && !p.partial) e_cold = p.C[e_ix];                  \
            if (fuse_adam) {                                                          \
                e_p = p.ep.adam.p[e_ix];                                              \
                e_m = p.ep.adam.m[e_ix];                                              \
                e_v = p.ep.adam.v[e_ix];                                              \
                e_step = adam_dev_step(p.ep.adam);                                    \
            }                                                                         \
            if (p.ep.bias) e_bias = p.ep.bias[ecol];                                  \
        }                                                                             \
    } while (0)
template <bool A_KC, bool B_KC, int NW, bool MASKED, int RM = 16, int RN = 16, bool STAMPED = false, bool EP_LATE = false>
__device__ __forceinline__ void small16_body(const SmallArgs &p, int tile_row, int tile_col, int zslice, float (*red)[64][4],
                                             long long stamp_entry = 0, int stamp_blk_arg = -1) {
    constexpr bool SUB = RM < 16 || RN < 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, g = lane >> 4;
    const int row0 = tile_row * RM, col0 = tile_col * RN;
    const int kbeg_slice = zslice * p.kslice;
    const int kend_slice = min(p.k, kbeg_slice + p.kslice);
    // split the slice between the NW waves in multiples of 16
    const int kwave = ((kend_slice - kbeg_slice + 16 * NW - 1) / (16 * NW)) * 16;
    const int kbeg = kbeg_slice + wave * kwave;
    const int kend = min(kend_slice, kbeg + kwave);
#ifdef TH_PROFILE
    const int stamp_blk = stamp_blk_arg >= 0 ? stamp_blk_arg : blockIdx.x + gridDim.x * blockIdx.y;
    const int stamp_last = max((kend_slice - kbeg_slice) / kwave - 1, 0) % NW;
    const int stamp_slot = (lane != 0 || stamp_blk >= kFwdProfBlocks) ? -1 : wave == 0 ? 0 : wave == stamp_last ? 1 : -1;
    if constexpr (STAMPED)
        if (stamp_slot >= 0) g_fwd_prof[stamp_blk][stamp_slot][6] = stamp_entry;
#endif
    FWD_STAMP(0);

    const int arow = row0 + (SUB ? r & (RM - 1) : r), bcol = col0 + (SUB ? r & (RN - 1) : r);
    const bool a_ok = (!SUB || r < RM) && arow < p.m, b_ok = (!SUB || r < RN) && bcol < p.n;
    const long a_off = (long)(a_ok ? arow : SUB ? row0 : 0) * p.a_rs;
    const float *ap = p.A + a_off;
    const float *mp = MASKED ? p.Amask + a_off : nullptr;
    const float *bp = p.B + (long)(b_ok ? bcol : SUB ? col0 : 0) * p.b_cs;

    // These shapes are latency-bound: after a kernel boundary every dependent
    // global round trip costs ~0.5-1 us.  So (a) everything the epilogue will
    // need from memory -- bias, the old C for beta != 0, the Adam state of a fused
    // update -- is requested by wave 0 NOW, under the operand loads; (b) the
    // operand loads of CH k-steps (64 k per wave) are all issued before the
    // first MFMA consumes any.
    // Epilogue work is spread over waves 0..3: wave e finishes output element e of every lane (row
    // 4*(lane>>4) + e of the tile), so the p / m / v traffic of a fused Adam update and the final adds
    // run on four SIMDs instead of one.
    const int ecol = col0 + (lane & 15);
    const bool fuse_adam = p.ep.adam.p != nullptr && p.partial == nullptr;
    const int erow = row0 + (lane >> 4) * 4 + wave;     // meaningful for wave < 4
    const bool e_sub = !SUB || ((lane >> 4) * 4 + wave < RM && (lane & 15) < RN);   // the C/D elements of the sub-tile
    const bool e_ok = wave < 4 && erow < p.m && ecol < p.n && e_sub;
    const long e_ix = e_ok ? (long)erow * p.n + ecol : 0;
    float e_bias = 0.f, e_cold = 0.f, e_p = 0.f, e_m = 0.f, e_v = 0.f, e_step = 0.f;
    if constexpr (!EP_LATE) {
        SMALL16_REQUEST_EPILOGUE();
    }
    constexpr int CH = 4;
    floatx4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int kk0 = kbeg; kk0 < kend; kk0 += 16 * CH) {
        float av[CH][4], bv[CH][4];
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int kb = kk0 + 16 * c + g * 4;
            if (A_KC && p.a_vec && kb + 4 <= kend) {
                float4 t = *reinterpret_cast<const float4 *>(ap + kb);
                av[c][0] = t.x; av[c][1] = t.y; av[c][2] = t.z; av[c][3] = t.w;
                if (MASKED) {
                    float4 q = *reinterpret_cast<const float4 *>(mp + kb);
                    av[c][0] = q.x > 0.f ? av[c][0] : 0.f; av[c][1] = q.y > 0.f ? av[c][1] : 0.f;
                    av[c][2] = q.z > 0.f ? av[c][2] : 0.f; av[c][3] = q.w > 0.f ? av[c][3] : 0.f;
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const bool in = kb + s < kend;
                    float v = in ? ap[(long)(kb + s) * p.a_cs] : 0.f;
                    if (MASKED) v = (in && mp[(long)(kb + s) * p.a_cs] > 0.f) ? v : 0.f;
                    av[c][s] = v;
                }
            }
            if (B_KC && p.b_vec && kb + 4 <= kend) {
                float4 t = *reinterpret_cast<const float4 *>(bp + kb);
                bv[c][0] = t.x; bv[c][1] = t.y; bv[c][2] = t.z; bv[c][3] = t.w;
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) bv[c][s] = (kb + s < kend) ? bp[(long)(kb + s) * p.b_rs] : 0.f;
            }
        }
        if (kk0 == kbeg) {
            FWD_STAMP(1);
            FWD_LANDED(av[0][0]);
            FWD_LANDED(bv[0][0]);
            FWD_STAMP(2);
        }
        if constexpr (EP_LATE) {
            if (kk0 == kbeg) SMALL16_REQUEST_EPILOGUE();
        }
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (kk0 + 16 * c >= kend) break;  // wave-uniform
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float a = a_ok ? av[c][s] : 0.f;
                const float b = b_ok ? bv[c][s] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
            }
        }
    }
    if constexpr (EP_LATE) {
        if (kbeg >= kend) SMALL16_REQUEST_EPILOGUE();   // a wave without a chunk of K still finishes its output elements
    }
    FWD_LANDED(acc[0]);
    FWD_STAMP(3);

    // deterministic in-workgroup reduction: every wave parks its 4 partial sums; wave e adds element e
    // of waves 0..NW-1 in wave order
    if (!SUB || (g * 4 < RM && r < RN)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) red[wave][lane][i] = acc[i];
    }
    __syncthreads();
    FWD_STAMP(4);
    if (wave < 4 && e_sub) {
        float sum = red[0][lane][wave];
        for (int w = 1; w < NW; ++w) sum += red[w][lane][wave];
        // C/D map of 16x16x4: col = lane & 15, row = (lane >> 4) * 4 + i  (here i = wave)
        if (e_ok) {
            if (p.partial) {
                p.partial[(long)zslice * p.m * p.n + e_ix] = sum;
            } else {
                float out = p.ep.alpha * sum;
                if (p.ep.beta != 0.0f) out += p.ep.beta * e_cold;
                if (p.ep.bias) out += e_bias;
                if (p.ep.relu) out = out > 0.0f ? out : 0.0f;
                p.C[e_ix] = out;
                if (fuse_adam) {  // th_linear_bwd_adam: C is a complete gradient (optim.rs:99-110)
                    const AdamDev &ad = p.ep.adam;
                    const AdamMV x = adam_moments(ad, e_p, e_m, e_v, out);
                    ad.m[e_ix] = x.m;
                    ad.v[e_ix] = x.v;
                    ad.p[e_ix] = adam_param(ad, e_p, x, e_step);
                }
            }
        }
    }
#ifdef TH_PROFILE
    if constexpr (STAMPED) __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): stamp 5 is the store's return, not its issue
#endif
    FWD_STAMP(5);
}

}  // namespace th
