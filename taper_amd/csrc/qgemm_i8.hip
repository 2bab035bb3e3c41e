// qgemm_i8.hip -- calibrated int8 inference: int8 activation codes times int8 weight codes on the integer matrix cores
// (v_mfma_i32_32x32x32_i8), exact int32 accumulation, one f32 epilogue.
//
//   th_quantize_act_int8  f32 [rows, k] -> symmetric int8 codes [rows, pitch] (th_fake_quant_act's codec with a scale fixed beforehand)
//                         and the int32 sum of each row's codes; one launch, a wave per row
//   th_pad_rows_int8      packed [rows, k] codes -> [rows, pitch] with zero padding (once per weight): the conv weight pack with one tap
//   th_linear_q8q8_fwd    y = sx * (sw * (float)(acc + 128 rs) + mw * (float)rs) [+ deq(bias)] [ReLU], acc = sum_k qx qw from the MFMA;
//                         two forms: 128 x 128 tiles through LDS, and a workgroup per 32 x 32 tile with K split over its waves for few rows
//   th_linear_q8q8_fwd_pc the same with one {mw, sw} per output row: the same kernels, a template flag in store_tile
//   th_linear_q8q8_fwd_link  either product with a destination -- f32, or the next layer's int8 codes from the epilogue -- and, without
//                         row sums given, its own from the x codes it reads anyway: template flags beside the per-channel one
//   th_act_range_update   calibration: the finite min / max of a tensor folded into a running device pair, and the scale they give
//
// The piece of 16 codes, the LDS image of a stage, the fragment pairing and the epilogue's arithmetic are qi8_dev.h's, shared with
// qconv_i8.hip; rs is the sum of the row's activation codes.  A row's result depends on that row alone: nothing of the tiling reaches
// the arithmetic.
#include "common.h"
#include "qi8_dev.h"
#include "stream_dev.h"

namespace th {

constexpr int kQ8Tile = 128;       // macro-tile: 128 rows of x by 128 rows of W, four waves of 2 x 2 MFMA tiles
constexpr int kQ8KStep = 64;       // bytes of K per LDS stage: two 32-k MFMA steps
constexpr int kQ8Raster = 8;       // tile rows per group of the tile order (gemm.hip's sgemm_tile)
constexpr int kQ8SkinnyMaxBatch = 256;   // up to here a workgroup per 32 x 32 tile with K split over its waves (measured: profiles/quant_static.md)

// ---- activations -> codes ----
// A wave per row, four rows per workgroup; a lane takes 16 k positions at a time: four float4 loads, one 16-byte store.  Positions
// k .. pitch - 1 get the code 0.  VEC: x rows and code rows are 16-byte aligned (the host says).
template <bool VEC>
__global__ __launch_bounds__(256) void quantize_act_kernel(const float *__restrict__ x, int rows, int k, const float *__restrict__ d_scale,
                                                           int8_t *__restrict__ q, int pitch, int *__restrict__ rowsum) {
    const int lane = threadIdx.x & 63;
    const float scale = d_scale[0];
    for (long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += (long)gridDim.x * 4) {
        const float *xr = x + (size_t)row * k;
        int8_t *qr = q + (size_t)row * pitch;
        int sum = 0;
        for (int k0 = lane * 16; k0 < pitch; k0 += 64 * 16) {
            int c[16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int kk = k0 + 4 * i;
                float v[4];
                if (VEC && kk + 4 <= k) {
                    const float4 f = *(const float4 *)(xr + kk);
                    v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = kk + j < k ? xr[kk + j] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    c[4 * i + j] = kk + j < k ? act_code(v[j], scale) : 0;
                    sum += c[4 * i + j];
                }
            }
            const uint4 p = piece_pack(c);
            if (VEC) {
                *(uint4 *)(qr + k0) = p;
            } else {
#pragma unroll
                for (int i = 0; i < 16; ++i) qr[k0 + i] = (int8_t)piece_code(p, i);
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);   // integers: any order gives the same bits
        if (lane == 0) rowsum[row] = sum;
    }
}

// what the epilogue of either form needs
struct Q8Epilogue {
    const int *rowsum;
    const float *xscale, *wparams;
    const int8_t *qb;
    const float *bparams;
    int relu, M, N;
    float *y;
};

// One 32 x 32 accumulator tile out: this lane holds column n (a row of W) of rows row_base + (e & 3) + 8 (e >> 2) (row_base includes the
// lane half's 4 h), each through q8_value.  PC: wparams holds one {mw, sw} per column, this lane's at 2 n; else one for all.
template <bool PC>
__device__ __forceinline__ void store_tile(const intx16 &acc, int row_base, int n, const Q8Epilogue &ep) {
    if (n >= ep.N) return;
    const float sx = ep.xscale[0], mw = ep.wparams[PC ? 2 * (size_t)n : 0], sw = ep.wparams[PC ? 2 * (size_t)n + 1 : 1];
    const float bias = ep.qb ? dequant_int8(ep.qb[n], ep.bparams[1], ep.bparams[0]) : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int row = row_base + (e & 3) + 8 * (e >> 2);
        if (row >= ep.M) continue;
        const int rs = ep.rowsum[row];
        ep.y[(size_t)row * ep.N + n] = q8_value(acc[e], rs, q8_rterm(mw, rs), sx, sw, ep.qb != nullptr, [&] { return bias; }, ep.relu);
    }
}

// ---- the link forms ----
// th_linear_q8q8_fwd_link's two template flags beside PC.  CODES: the epilogue's value goes through the activation codec with the next
// layer's scale and leaves as a row of that layer's codes; OWN: the kernel sums the x codes it reads into the row sums it needs.
struct Q8Link {
    const float *yscale;   // CODES: the next layer's activation scale
    int8_t *qy;            // CODES: [M][pitch_y] codes, bytes N .. pitch_y - 1 of every row written 0
    int pitch_y;
};

// the sum of the 16 codes of a piece: four signed dot products with 1 (integers: exact)
__device__ __forceinline__ int piece_sum4(const uint4 &p) {
    int s = __builtin_amdgcn_sdot4((int)p.x, 0x01010101, 0, false);
    s = __builtin_amdgcn_sdot4((int)p.y, 0x01010101, s, false);
    s = __builtin_amdgcn_sdot4((int)p.z, 0x01010101, s, false);
    return __builtin_amdgcn_sdot4((int)p.w, 0x01010101, s, false);
}

// store_tile for the link forms: rs_of(local row, row) gives the row sum (from memory, or from the workgroup's own sums; whatever it
// gives for a row past M is never stored); the f32 form stores as store_tile does, the CODES form puts the code of every (row, column)
// of the tile -- 0 at a column past N -- at tile[local row * tpitch + local column] in LDS, from where whole pieces go out (codes_out).
// lrow_base / lcol: the lane's place inside the workgroup's tile.
template <bool PC, bool CODES, class RowSum>
__device__ __forceinline__ void store_tile_link(const intx16 &acc, int row_base, int n, int lrow_base, int lcol, const Q8Epilogue &ep, const Q8Link &lk,
                                                RowSum rs_of, int8_t *tile, int tpitch) {
    const bool live = n < ep.N;   // (a lane past N stays to the end: rs_of may be a lane exchange)
    const int nn = live ? n : 0;
    const float sx = ep.xscale[0], mw = ep.wparams[PC ? 2 * (size_t)nn : 0], sw = ep.wparams[PC ? 2 * (size_t)nn + 1 : 1];
    const float bias = ep.qb ? dequant_int8(ep.qb[nn], ep.bparams[1], ep.bparams[0]) : 0.f;
    const float sy = CODES ? lk.yscale[0] : 0.f;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int lrow = lrow_base + (e & 3) + 8 * (e >> 2), row = row_base + (e & 3) + 8 * (e >> 2);
        const int rs = rs_of(lrow, row);
        const float v = q8_value(acc[e], rs, q8_rterm(mw, rs), sx, sw, ep.qb != nullptr, [&] { return bias; }, ep.relu);
        if constexpr (CODES) {
            tile[lrow * tpitch + lcol] = (int8_t)(live ? act_code(v, sy) : 0);
        } else {
            if (live && row < ep.M) ep.y[(size_t)row * ep.N + n] = v;
        }
    }
}

// The codes of a workgroup's tile (rows x cols bytes at `tile`, row pitch tpitch, complete and visible) to their rows of qy, 16 bytes a
// store; the LAST column tile also writes the zero pieces from its end to pitch_y, so that every byte of a row of qy is written once.
// Threads t of nt take pieces t, t + nt, ...
__device__ __forceinline__ void codes_out(const int8_t *tile, int tpitch, int rows, int cols, int row0, int col0, bool last_n, int M, const Q8Link &lk, int t,
                                          int nt) {
    const int p0 = col0 >> 4, p1 = last_n ? lk.pitch_y >> 4 : (col0 + cols) >> 4, np = p1 - p0;   // (not last: the tile lies inside N <= pitch_y)
    for (long i = t; i < (long)rows * np; i += nt) {
        const int r = (int)(i / np), p = (int)(i - (long)r * np);
        if (row0 + r >= M) continue;
        const uint4 v = p * 16 < cols ? *(const uint4 *)(tile + r * tpitch + p * 16) : make_uint4(0, 0, 0, 0);
        *(uint4 *)(lk.qy + (size_t)(row0 + r) * lk.pitch_y + (size_t)(p0 + p) * 16) = v;
    }
}

// ---- the product ----
// Each operand's stage is 128 rows in qi8_dev.h's image; x is the MFMA's A operand and W its B: C/D column = lane & 31 is a row of W,
// C/D row = (reg & 3) + 8 (reg >> 2) + 4 h a row of x.
//
// CODES / OWN (the link forms; both false: th_linear_q8q8_fwd's kernel, nothing of them is compiled in).  OWN: thread t sums the
// x pieces it fetches -- piece t & 3 of rows t >> 2 and + 64, every K step, so the four threads of a row see the row's whole K -- and the
// 128 sums are parked in LDS behind the loop's last barrier.  CODES: the tile's codes go through the stage LDS, free by then, and leave
// as 16-byte pieces.
template <bool PC, bool CODES, bool OWN>
__device__ __forceinline__ void qgemm_i8_tile(const int8_t *__restrict__ qx, int pitch_x, int K, const int8_t *__restrict__ qw, int pitch_w, const Q8Epilogue &ep,
                                              const Q8Link &lk, int tiles_m, int tiles_n) {
    const int M = ep.M, N = ep.N;
    __shared__ uint4 lds[2][2][kQ8Tile * 4];   // [stage][x / W][slot]: 32 KB

    // tile order: block b runs on XCD b % 8; every XCD takes a contiguous run of the tile list, and the list walks groups of 8 tile rows
    // column by column, so the tiles an XCD has in flight share their operand panels in its L2 (gemm.hip, sgemm_tile)
    const int nwg = tiles_m * tiles_n, bid = blockIdx.x;
    const int xcd = bid % kNumXCD, per = nwg / kNumXCD, rmd = nwg % kNumXCD;
    const int tile = (xcd < rmd ? xcd * (per + 1) : rmd * (per + 1) + (xcd - rmd) * per) + bid / kNumXCD;
    const int grp = tile / (kQ8Raster * tiles_n), first = grp * kQ8Raster, gh = min(kQ8Raster, tiles_m - first), in = tile - grp * kQ8Raster * tiles_n;
    const int row0 = (first + in % gh) * kQ8Tile, col0 = (in / gh) * kQ8Tile;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64, li = lane & 31, h = lane >> 5;

    // staging: thread t brings piece t & 3 of rows (t >> 2) and (t >> 2) + 64 of each operand; rows past M / N re-read the last row (never
    // stored), pieces that begin at or past K are zero (pitch >= K rounded up to 16: every piece that is read lies inside its row)
    const int srow = t >> 2, piece = t & 3, pieces = (K + 15) >> 4;
    const int8_t *pa[2], *pb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        pa[i] = qx + (size_t)min(row0 + srow + 64 * i, M - 1) * pitch_x + piece * 16;
        pb[i] = qw + (size_t)min(col0 + srow + 64 * i, N - 1) * pitch_w + piece * 16;
    }
    const int nk = (K + kQ8KStep - 1) / kQ8KStep;
    uint4 ga[2], gb[2];
    int own[2] = {0, 0};   // OWN: the sums of this thread's pieces of its two x rows
    auto fetch = [&](int kt) {
        const bool in_k = kt * 4 + piece < pieces;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            ga[i] = in_k ? *(const uint4 *)(pa[i] + (size_t)kt * kQ8KStep) : make_uint4(0, 0, 0, 0);
            gb[i] = in_k ? *(const uint4 *)(pb[i] + (size_t)kt * kQ8KStep) : make_uint4(0, 0, 0, 0);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            lds[buf][0][stage_slot(srow + 64 * i, piece)] = ga[i];
            lds[buf][1][stage_slot(srow + 64 * i, piece)] = gb[i];
            if constexpr (OWN) own[i] += piece_sum4(ga[i]);   // (every fetched stage is staged exactly once)
        }
    };

    intx16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0;

    fetch(0);
    stage(0);
    lds_barrier();
    int buf = 0;
    for (int kt = 0; kt < nk; ++kt) {
        if (kt + 1 < nk) fetch(kt + 1);   // in flight under this stage's MFMAs
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            intx4 a[2], b[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                a[i] = stage_frag(lds[buf][0], wm + 32 * i + li, s, h);
                b[i] = stage_frag(lds[buf][1], wn + 32 * i + li, s, h);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if (kt + 1 < nk) stage(buf ^ 1);   // (read last in step kt - 1: every wave passed that step's barrier)
        lds_barrier();
        buf ^= 1;
    }

    if constexpr (!CODES && !OWN) {
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) store_tile<PC>(acc[i][j], row0 + wm + 32 * i + 4 * h, col0 + wn + 32 * j + li, ep);
    } else {
        __shared__ int rsum[OWN ? kQ8Tile : 1];
        int8_t *tile = reinterpret_cast<int8_t *>(&lds[0][0][0]);   // CODES: [128][128] codes in the stage LDS (every wave is past the loop's last barrier)
        if constexpr (OWN) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                int sum = own[i];
                sum += __shfl_xor(sum, 1, 64);   // the four threads of a row (integers: any order gives the same bits)
                sum += __shfl_xor(sum, 2, 64);
                if (piece == 0) rsum[srow + 64 * i] = sum;
            }
            lds_barrier();
        }
        auto rs_of = [&](int lrow, int row) { return OWN ? rsum[OWN ? lrow : 0] : ep.rowsum[min(row, M - 1)]; };
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                store_tile_link<PC, CODES>(acc[i][j], row0 + wm + 32 * i + 4 * h, col0 + wn + 32 * j + li, wm + 32 * i + 4 * h, wn + 32 * j + li, ep, lk, rs_of, tile,
                                           kQ8Tile);
        if constexpr (CODES) {
            lds_barrier();
            codes_out(tile, kQ8Tile, kQ8Tile, kQ8Tile, row0, col0, col0 + kQ8Tile >= N, M, lk, t, 256);
        }
    }
}

template <bool PC>
__global__ __launch_bounds__(256) void qgemm_i8_kernel(const int8_t *__restrict__ qx, int pitch_x, int K, const int8_t *__restrict__ qw, int pitch_w,
                                                       Q8Epilogue ep, int tiles_m, int tiles_n) {
    qgemm_i8_tile<PC, false, false>(qx, pitch_x, K, qw, pitch_w, ep, Q8Link{}, tiles_m, tiles_n);
}

template <bool PC, bool CODES, bool OWN>
__global__ __launch_bounds__(256) void qgemm_i8_link_kernel(const int8_t *__restrict__ qx, int pitch_x, int K, const int8_t *__restrict__ qw, int pitch_w,
                                                            Q8Epilogue ep, Q8Link lk, int tiles_m, int tiles_n) {
    qgemm_i8_tile<PC, CODES, OWN>(qx, pitch_x, K, qw, pitch_w, ep, lk, tiles_m, tiles_n);
}

// Few rows (batch <= kQ8SkinnyMaxBatch): the 128 x 128 form would leave most CUs idle and walk K in one long chain of dependent
// stages.  Here a workgroup owns ONE 32 x 32 tile and its four waves split K: wave v takes the 64-byte chunks v, v + 4, ... of both
// operands straight from memory into its fragments (a lane's two 16-byte loads per row are 32 consecutive bytes; no LDS staging, no
// barrier inside the loop, so the loads of several chunks are in flight at once), and the four int32 partial tiles are added through LDS
// -- integers: the order does not matter -- before the same epilogue.  ceil(N / 32) * ceil(M / 32) workgroups.
//
// CODES / OWN (the link forms; both false: th_linear_q8q8_fwd's kernel).  OWN: a lane sums the pieces of row li that it loads -- its
// half's of its wave's chunks -- and the halves and waves are added through LDS beside the partial tiles.  CODES: wave 0 passes the
// tile's 32 x 32 codes through LDS, and each of its lanes stores one 16-byte piece.
template <bool PC, bool CODES, bool OWN>
__device__ __forceinline__ void qgemm_i8_skinny_tile(const int8_t *__restrict__ qx, int pitch_x, int K, const int8_t *__restrict__ qw, int pitch_w,
                                                     const Q8Epilogue &ep, const Q8Link &lk, int tiles_m) {
    __shared__ int red[3][16][64];   // 12 KB
    // block b runs on XCD b % 8: every XCD takes a contiguous run of the tile list, row tiles fastest, so the row tiles of one W panel
    // read it through one L2
    const int nwg = gridDim.x, bid = blockIdx.x, xcd = bid % kNumXCD, per = nwg / kNumXCD, rmd = nwg % kNumXCD;
    const int tile = (xcd < rmd ? xcd * (per + 1) : rmd * (per + 1) + (xcd - rmd) * per) + bid / kNumXCD;
    const int row0 = (tile % tiles_m) * 32, col0 = (tile / tiles_m) * 32;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, li = lane & 31, h = lane >> 5;
    const int8_t *pa = qx + (size_t)min(row0 + li, ep.M - 1) * pitch_x + h * 16;
    const int8_t *pb = qw + (size_t)min(col0 + li, ep.N - 1) * pitch_w + h * 16;
    const int pieces = (K + 15) >> 4, nk = (K + kQ8KStep - 1) / kQ8KStep;   // 16-byte pieces that begin before K; 64-byte chunks
    intx16 acc;
    int own = 0;   // OWN: the sum of the x pieces this lane loads
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0;
    for (int kt0 = wave; kt0 < nk; kt0 += 16) {   // four chunks a trip, their sixteen loads issued before the first MFMA (a chunk past K loads nothing)
        uint4 va[4][2], vb[4][2];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int kt = kt0 + 4 * u;
                const bool in_k = kt * 4 + 2 * s + h < pieces;
                va[u][s] = in_k ? *(const uint4 *)(pa + (size_t)kt * kQ8KStep + 32 * s) : make_uint4(0, 0, 0, 0);
                vb[u][s] = in_k ? *(const uint4 *)(pb + (size_t)kt * kQ8KStep + 32 * s) : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(as_frag(va[u][s]), as_frag(vb[u][s]), acc, 0, 0, 0);
                if constexpr (OWN) own += piece_sum4(va[u][s]);
            }
    }
    __shared__ int part[OWN ? 4 : 1][OWN ? 64 : 1];   // OWN: every wave's sums, a lane each
    if constexpr (OWN) part[wave][lane] = own;
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) red[wave - 1][e][lane] = acc[e];
    }
    __syncthreads();
    if (wave > 0) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] += red[0][e][lane] + red[1][e][lane] + red[2][e][lane];
    if constexpr (!CODES && !OWN) {
        store_tile<PC>(acc, row0 + 4 * h, col0 + li, ep);
    } else {
        __shared__ __attribute__((aligned(16))) int8_t tile[CODES ? 32 * 32 : 16];
        int total = 0;   // OWN: the sum of row li, in both lanes li and li + 32 (integers: any order gives the same bits)
        if constexpr (OWN) {
#pragma unroll
            for (int w = 0; w < 4; ++w) total += part[OWN ? w : 0][OWN ? li : 0] + part[OWN ? w : 0][OWN ? li + 32 : 0];
        }
        auto rs_of = [&](int lrow, int row) { return OWN ? __shfl(total, lrow, 64) : ep.rowsum[min(row, ep.M - 1)]; };
        store_tile_link<PC, CODES>(acc, row0 + 4 * h, col0 + li, 4 * h, li, ep, lk, rs_of, tile, 32);
        if constexpr (CODES) {   // wave 0 alone is left: its LDS writes and reads stay in order, the fence keeps the compiler to that
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
            codes_out(tile, 32, 32, 32, row0, col0, col0 + 32 >= ep.N, ep.M, lk, lane, 64);
        }
    }
}

template <bool PC>
__global__ __launch_bounds__(256) void qgemm_i8_skinny_kernel(const int8_t *__restrict__ qx, int pitch_x, int K, const int8_t *__restrict__ qw,
                                                              int pitch_w, Q8Epilogue ep, int tiles_m) {
    qgemm_i8_skinny_tile<PC, false, false>(qx, pitch_x, K, qw, pitch_w, ep, Q8Link{}, tiles_m);
}

template <bool PC, bool CODES, bool OWN>
__global__ __launch_bounds__(256) void qgemm_i8_skinny_link_kernel(const int8_t *__restrict__ qx, int pitch_x, int K, const int8_t *__restrict__ qw,
                                                                   int pitch_w, Q8Epilogue ep, Q8Link lk, int tiles_m) {
    qgemm_i8_skinny_tile<PC, CODES, OWN>(qx, pitch_x, K, qw, pitch_w, ep, lk, tiles_m);
}

// ---- calibration ----
// range = {finite min, finite max} seen so far (first: this tensor's alone); scale by fq_act_int8_kernel's rule from the running pair
__global__ __launch_bounds__(kStreamThreads) void act_range_fold_kernel(const float *__restrict__ part, int nb, int first, float *__restrict__ range,
                                                                        float *__restrict__ d_scale) {
    __shared__ float s[8];
    float mn, mx;
    fold_parts(part, nb, &mn, &mx, s);
    if (threadIdx.x != 0) return;
    if (!first) {
        mn = fminf(mn, range[0]);
        mx = fmaxf(mx, range[1]);
    }
    range[0] = mn;
    range[1] = mx;
    if (mn == mx) {
        if (mn == 0.0f) {
            mn = 0.0f;
            mx = 1.0f;
        } else {
            const float m = mn;
            mn = m * 0.9f;
            mx = m * 1.1f;
        }
    }
    d_scale[0] = fmaxf(fabsf(mn), fabsf(mx)) / 127.0f;
}

// every host decision of the product (th_linear_q8q8_fwd launches from it, th_debug_q8q8_plan reports it)
struct Q8Plan {
    int skinny, tiles_m, tiles_n, grid;
};
static Q8Plan q8q8_plan(int B, int N) {
    Q8Plan p{};
    p.skinny = B <= kQ8SkinnyMaxBatch;
    const int ts = p.skinny ? 32 : kQ8Tile;
    p.tiles_m = ceil_div(B, ts);
    p.tiles_n = ceil_div(N, ts);
    p.grid = p.tiles_m * p.tiles_n;
    return p;
}

// the link kernel of a form for (pc, codes, own); (codes, own) = (false, false) is th_linear_q8q8_fwd's own kernel, not one of these
template <bool SKINNY, bool PC>
static auto q8q8_link_kernel(bool codes, bool own) {
    if constexpr (SKINNY)
        return codes ? (own ? qgemm_i8_skinny_link_kernel<PC, true, true> : qgemm_i8_skinny_link_kernel<PC, true, false>) : qgemm_i8_skinny_link_kernel<PC, false, true>;
    else
        return codes ? (own ? qgemm_i8_link_kernel<PC, true, true> : qgemm_i8_link_kernel<PC, true, false>) : qgemm_i8_link_kernel<PC, false, true>;
}

constexpr int kRangeParts = 512;
constexpr int64_t kRangePartMin = 4 * 256 * 8;

}  // namespace th

using namespace th;

extern "C" {

int th_quantize_act_int8(th_ctx *ctx, const float *d_x, int rows, int k, const float *d_scale, int8_t *d_q, int pitch, int *d_rowsum) {
    TH_REQUIRE(ctx && d_x && d_scale && d_q && d_rowsum, "th_quantize_act_int8: null argument");
    TH_REQUIRE(rows >= 0 && k > 0 && pitch >= k && pitch % 16 == 0, "th_quantize_act_int8: bad shape rows=%d k=%d pitch=%d (pitch >= k, a multiple of 16)",
               rows, k, pitch);
    if (rows == 0) return 0;
    const dim3 grid(std::min(ceil_div(rows, 4), kNumCU * 16));
    const bool vec = k % 4 == 0 && (((uintptr_t)d_x | (uintptr_t)d_q) & 15) == 0;
    hipLaunchKernelGGL(vec ? quantize_act_kernel<true> : quantize_act_kernel<false>, grid, dim3(256), 0, ctx->stream, d_x, rows, k, d_scale, d_q, pitch, d_rowsum);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_pad_rows_int8(th_ctx *ctx, const int8_t *d_src, int rows, int k, int8_t *d_dst, int pitch) {
    TH_REQUIRE(ctx && d_src && d_dst, "th_pad_rows_int8: null argument");
    TH_REQUIRE(rows >= 0 && k > 0 && pitch >= k && pitch % 16 == 0 && ((uintptr_t)d_dst & 15) == 0,
               "th_pad_rows_int8: bad shape rows=%d k=%d pitch=%d (pitch >= k, a multiple of 16) or a destination off a 16-byte boundary", rows, k, pitch);
    if (rows == 0) return 0;
    hipLaunchKernelGGL(pack_conv_weight_kernel<false>, dim3(ew_grid((size_t)rows * (pitch / 16), 256)), dim3(256), 0, ctx->stream, d_src, (long)rows, k, 1, d_dst,
                       pitch);
    TH_LAUNCH_CHECK();
    return 0;
}

// Every product: its checks (fn: the caller's name for the message), then the launch; pc: d_wparams holds a pair per output row.  link:
// th_linear_q8q8_fwd_link's call -- d_rowsum may be null (the kernel sums its own rows), and the destination is d_y or the codes d_qy
// [batch][pitch_y] made with *d_yscale, exactly one of the two.
static int q8q8_run(const char *fn, bool pc, bool link, th_ctx *ctx, const int8_t *d_qx, int pitch_x, const int *d_rowsum, const float *d_xscale, int batch,
                    int in_features, const int8_t *d_qw, int pitch_w, int out_features, const float *d_wparams, const int8_t *d_qb, const float *d_bparams, int relu,
                    float *d_y, const float *d_yscale = nullptr, int8_t *d_qy = nullptr, int pitch_y = 0) {
    TH_REQUIRE(ctx && d_qx && (link || d_rowsum) && d_xscale && d_qw && d_wparams && (link || d_y) && (!d_qb || d_bparams), "%s: null argument", fn);
    if (link) {
        TH_REQUIRE((d_y != nullptr) != (d_qy != nullptr), "%s: exactly one destination, d_y or d_qy, must be set", fn);
        TH_REQUIRE(!d_qy || d_yscale, "%s: a codes destination needs d_yscale", fn);
    }
    TH_REQUIRE(batch >= 0 && in_features > 0 && out_features > 0, "%s: bad shape B=%d K=%d N=%d", fn, batch, in_features, out_features);
    TH_REQUIRE(in_features <= kQ8MaxK, "%s: in_features %d is above %d, where the int32 sum can overflow", fn, in_features, kQ8MaxK);
    TH_REQUIRE((((uintptr_t)d_qx | (uintptr_t)d_qw) & 15) == 0, "%s: the code pointers must be 16-byte aligned", fn);
    TH_REQUIRE(pitch_x % 16 == 0 && pitch_w % 16 == 0 && pitch_x >= in_features && pitch_w >= in_features,
               "%s: pitches %d / %d must be multiples of 16 and at least in_features %d", fn, pitch_x, pitch_w, in_features);
    if (d_qy) {
        TH_REQUIRE(((uintptr_t)d_qy & 15) == 0, "%s: the codes destination must be 16-byte aligned", fn);
        TH_REQUIRE(pitch_y % 16 == 0 && pitch_y >= out_features, "%s: pitch_y %d must be a multiple of 16 and at least out_features %d", fn, pitch_y, out_features);
    }
    if (batch == 0) return 0;
    const Q8Plan p = q8q8_plan(batch, out_features);
    const Q8Epilogue ep{d_rowsum, d_xscale, d_wparams, d_qb, d_bparams, relu, batch, out_features, d_y};
    const bool codes = d_qy != nullptr, own = d_rowsum == nullptr;
    const Q8Link lk{d_yscale, d_qy, pitch_y};
    if (codes || own) {
        if (p.skinny) {
            const auto kernel = pc ? q8q8_link_kernel<true, true>(codes, own) : q8q8_link_kernel<true, false>(codes, own);
            hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(256), 0, ctx->stream, d_qx, pitch_x, in_features, d_qw, pitch_w, ep, lk, p.tiles_m);
        } else {
            const auto kernel = pc ? q8q8_link_kernel<false, true>(codes, own) : q8q8_link_kernel<false, false>(codes, own);
            hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(256), 0, ctx->stream, d_qx, pitch_x, in_features, d_qw, pitch_w, ep, lk, p.tiles_m, p.tiles_n);
        }
    } else if (p.skinny)
        hipLaunchKernelGGL(pc ? qgemm_i8_skinny_kernel<true> : qgemm_i8_skinny_kernel<false>, dim3(p.grid), dim3(256), 0, ctx->stream, d_qx, pitch_x, in_features, d_qw,
                           pitch_w, ep, p.tiles_m);
    else
        hipLaunchKernelGGL(pc ? qgemm_i8_kernel<true> : qgemm_i8_kernel<false>, dim3(p.grid), dim3(256), 0, ctx->stream, d_qx, pitch_x, in_features, d_qw, pitch_w, ep,
                           p.tiles_m, p.tiles_n);
    TH_LAUNCH_CHECK();
    return 0;
}

int th_linear_q8q8_fwd(th_ctx *ctx, const int8_t *d_qx, int pitch_x, const int *d_rowsum, const float *d_xscale, int batch, int in_features,
                       const int8_t *d_qw, int pitch_w, int out_features, const float *d_wparams, const int8_t *d_qb, const float *d_bparams, int relu,
                       float *d_y) {
    return q8q8_run("th_linear_q8q8_fwd", false, false, ctx, d_qx, pitch_x, d_rowsum, d_xscale, batch, in_features, d_qw, pitch_w, out_features, d_wparams, d_qb, d_bparams,
                    relu, d_y);
}

int th_linear_q8q8_fwd_pc(th_ctx *ctx, const int8_t *d_qx, int pitch_x, const int *d_rowsum, const float *d_xscale, int batch, int in_features,
                          const int8_t *d_qw, int pitch_w, int out_features, const float *d_wparams, const int8_t *d_qb, const float *d_bparams, int relu,
                          float *d_y) {
    return q8q8_run("th_linear_q8q8_fwd_pc", true, false, ctx, d_qx, pitch_x, d_rowsum, d_xscale, batch, in_features, d_qw, pitch_w, out_features, d_wparams, d_qb, d_bparams,
                    relu, d_y);
}

int th_linear_q8q8_fwd_link(th_ctx *ctx, const int8_t *d_qx, int pitch_x, const int *d_rowsum, const float *d_xscale, int batch, int in_features,
                            const int8_t *d_qw, int pitch_w, int out_features, const float *d_wparams, int per_channel, const int8_t *d_qb, const float *d_bparams,
                            int relu, float *d_y, const float *d_yscale, int8_t *d_qy, int pitch_y) {
    return q8q8_run("th_linear_q8q8_fwd_link", per_channel != 0, true, ctx, d_qx, pitch_x, d_rowsum, d_xscale, batch, in_features, d_qw, pitch_w, out_features,
                    d_wparams, d_qb, d_bparams, relu, d_y, d_yscale, d_qy, pitch_y);
}

int th_debug_q8q8_plan(int batch, int in_features, int out_features, int *out4) {
    TH_REQUIRE(out4 && batch >= 1 && in_features > 0 && in_features <= kQ8MaxK && out_features > 0, "th_debug_q8q8_plan: null argument or bad shape B=%d K=%d N=%d",
               batch, in_features, out_features);
    const Q8Plan p = q8q8_plan(batch, out_features);
    const int out[4] = {p.skinny, p.tiles_m, p.tiles_n, p.grid};
    std::copy(out, out + 4, out4);
    return 0;
}

int th_qlinear_i8_kstep(void) { return kQ8KStep; }
int th_q8q8_max_k(void) { return kQ8MaxK; }

int th_act_range_update(th_ctx *ctx, const float *d_x, int64_t n, int first, float *d_range2, float *d_scale) {
    TH_REQUIRE(ctx && n >= 0 && (n == 0 || d_x) && d_range2 && d_scale, "th_act_range_update: null argument");
    const int nb = std::max(n <= 0 ? 0 : stream_grid(n, kRangePartMin, kRangeParts), 1);
    void *part = nullptr;
    if (th_malloc(ctx, (size_t)nb * 2 * sizeof(float), &part)) return 1;
    hipLaunchKernelGGL((minmax_parts_kernel<MinMaxFinite, true>), dim3(nb), dim3(kStreamThreads), 0, ctx->stream, d_x, d_x, n, (float *)part);
    TH_LAUNCH_CHECK();
    hipLaunchKernelGGL(act_range_fold_kernel, dim3(1), dim3(kStreamThreads), 0, ctx->stream, (const float *)part, nb, first, d_range2, d_scale);
    TH_LAUNCH_CHECK();
    return th_free(ctx, part);
}

}  // extern "C"
