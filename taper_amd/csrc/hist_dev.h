// hist_dev.h -- what the two counting passes share (observers.hip's th_obs_hist_count against an edge table, qcalib.hip's
// th_act_hist_update with one multiply per element): a workgroup of kHistThreads lanes with 32-bit counters in LDS, the hot bin a wave
// counts by ballot, the walk of a tensor by whole waves, and the merge of the workgroup's counters into the 64-bit global bins.  A
// value's bin is each pass's own.
#pragma once
#include "common.h"
#include "stream_dev.h"

namespace th {

constexpr int kObsLdsMaxBins = 8192;               // (8193 table entries + 8192 counters) * 4 B = 64 KiB + 4: two such workgroups fit a CU's 160 KiB
constexpr int kHistThreads = 1024;                 // 16 waves share a table and a set of counters: half the merges of two 8-wave workgroups
constexpr int kHistGrid = 256;                     // one workgroup per CU
constexpr int64_t kHistWgMin = 4 * 1024 * 4;       // elements per counting workgroup at least: a small tensor pays few table loads and merges

// The wave's hot bin: elements that fall into it are counted by ballot into hot_n (wave-uniform) and skip the LDS add.  After each
// round of loads a wave that caught few elements that way looks for a better candidate among the lanes of the round's last element.
// Every call is made by the whole wave (the ballots see 64 lanes); a bin is in [0, nb), or negative for a lane that counts nothing.
struct HotBin {
    unsigned *cnt;   // the workgroup's counters in LDS
    int hot = 0;
    unsigned hot_n = 0, hot_seen = 0;   // hot_seen: hot_n at the last retarget

    __device__ __forceinline__ void tally(int k) {   // k >= 0
        hot_n += __popcll(__ballot(k == hot));
        if (k != hot) atomicAdd(&cnt[k], 1u);
    }
    __device__ __forceinline__ void count(int k) {   // k < 0: nothing
        hot_n += __popcll(__ballot(k == hot));
        if (k >= 0 && k != hot) atomicAdd(&cnt[k], 1u);
    }
    // seen: elements the wave counted since the last call; last: each lane's latest bin (>= 0)
    __device__ __forceinline__ void retarget(int last, unsigned seen) {
        if ((hot_n - hot_seen) * 8 < seen) {
            unsigned long long rest = __ballot(last != hot);
            for (int tries = 0; tries < 3 && rest; ++tries) {
                const int cand = __builtin_amdgcn_readfirstlane(__shfl(last, __ffsll((long long)rest) - 1, 64));
                const unsigned long long same = __ballot(last == cand);
                if (__popcll(same) >= 8) {
                    flush();
                    hot_n = 0;
                    hot = cand;
                    break;
                }
                rest &= ~same;
            }
        }
        hot_seen = hot_n;
    }
    __device__ __forceinline__ void flush() {   // (the caller zeroes hot_n, or is done)
        if (hot_n && (threadIdx.x & 63) == 0) atomicAdd(&cnt[hot], hot_n);
    }
};

// x[0, n) by whole waves: with a 16-byte aligned x in float4s, four loads in flight per lane -- four(a) for each, then round() -- and
// the rest one load at a time, then the scalar tail: one(v, valid), where a lane past the end has valid = false.  Every trip count is
// wave-uniform (jw is the wave's first index), so a HotBin stays uniform and every ballot sees 64 lanes -- which is why this walk is
// written out here and is not stream_dev.h's span_walk, whose lanes stop one by one.
template <class Four, class Round, class One>
__device__ __forceinline__ void hist_wave_walk(const float *__restrict__ x, int64_t n, Four four, Round round, One one) {
    const int64_t t0 = (int64_t)blockIdx.x * kHistThreads + threadIdx.x, stride = (int64_t)gridDim.x * kHistThreads;
    int64_t head = 0;
    if (((uintptr_t)x & 15) == 0) {
        const float4 *x4 = (const float4 *)x;
        const int64_t n4 = n >> 2;
        int64_t jw = t0 - (threadIdx.x & 63);
        for (; jw + 3 * stride + 63 < n4; jw += 4 * stride) {
            const int64_t j = jw + (threadIdx.x & 63);
            const float4 a = x4[j], b = x4[j + stride], c = x4[j + 2 * stride], d = x4[j + 3 * stride];
            four(a); four(b); four(c); four(d);
            round();
        }
        for (int64_t jj = jw; jj < n4; jj += stride) {
            const int64_t mine = jj + (threadIdx.x & 63);
            const bool valid = mine < n4;
            const float4 a = valid ? x4[mine] : make_float4(0.f, 0.f, 0.f, 0.f);
            one(a.x, valid); one(a.y, valid); one(a.z, valid); one(a.w, valid);
        }
        head = n4 << 2;
    }
    {
        const int64_t iw = head + t0 - (threadIdx.x & 63);
        for (int64_t ii = iw; ii < n; ii += stride) {
            const int64_t mine = ii + (threadIdx.x & 63);
            const bool valid = mine < n;
            one(valid ? x[mine] : 0.0f, valid);
        }
    }
}

// the workgroup's nb counters (complete and visible) into the global bins: non-zero counters only, each workgroup from a bin of its own
__device__ __forceinline__ void hist_merge(const unsigned *cnt, int nb, unsigned long long *__restrict__ bins) {
    const int start = (int)(((long long)blockIdx.x * nb) / gridDim.x);
    for (int i = threadIdx.x; i < nb; i += kHistThreads) {
        int k = i + start;
        if (k >= nb) k -= nb;
        const unsigned c = cnt[k];
        if (c) atomicAdd(&bins[k], (unsigned long long)c);
    }
}

}  // namespace th
