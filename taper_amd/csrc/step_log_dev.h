// step_log_dev.h -- the step log every fused step form ends with (th_log_step, include/taper_hip.h), stated once.
//
// One thread of the step's last launch appends {loss, n_correct} to the metrics ring at slot state[0] mod capacity, then advances the
// step number (state[0] += 1) and the sample cursor (state[1] += advance).  Four stores, in that order; the record is a copy of two
// floats and two integer additions, so every site that calls these functions writes the same bits.
#pragma once
#include "common.h"

namespace th {

// the four step-log arguments of the C ABI as a kernel argument (reduce.hip's loss kernels), with the Adam tick that rides with them
struct StepLog {  // th_log_step folded into the loss kernel (nullable metrics)
    float *metrics;
    int64_t capacity;
    int64_t *state;
    int64_t advance;
    int32_t *adam_tick;  // nullable: Adam's t += 1 (optim.rs:84) for a step whose updates run fused
};

// The slot for step number state0: state0 mod capacity.  Contract: state0 >= 0, capacity > 0 (the launchers check the capacity, the
// step number starts at 0 and only this file advances it), both workgroup-uniform.  Below the capacity it is state0 itself; past it,
// a 32-bit remainder when both fit -- the 64-bit remainder is a 140-instruction routine.
__device__ __forceinline__ int64_t step_log_slot(int64_t state0, int64_t capacity) {
    if (state0 < capacity) return state0;
    if ((((uint64_t)state0 | (uint64_t)capacity) >> 32) == 0) return (int64_t)((uint32_t)state0 % (uint32_t)capacity);
    return state0 % capacity;
}

// the record, for a site that formed the slot and the next state words early (under its operand loads)
__device__ __forceinline__ void step_log_write(float *metrics, int64_t slot, float loss, float ncorrect, int64_t *state,
                                               int64_t state0_next, int64_t state1_next) {
    metrics[2 * slot] = loss;
    metrics[2 * slot + 1] = ncorrect;
    state[0] = state0_next;
    state[1] = state1_next;
}

// ... and for a site that reads the state where it logs
__device__ __forceinline__ void step_log_write(float *metrics, int64_t capacity, int64_t *state, int64_t advance, float loss,
                                               float ncorrect) {
    const int64_t s0 = state[0], s1 = state[1];
    step_log_write(metrics, step_log_slot(s0, capacity), loss, ncorrect, state, s0 + 1, s1 + advance);
}

// launcher side: every entry point that takes d_metrics, metrics_capacity, d_state, advance runs this under its own name
#define TH_REQUIRE_STEP_LOG(NAME) \
    TH_REQUIRE(!d_metrics || (d_state && metrics_capacity > 0), NAME ": metrics need d_state and a capacity")

}  // namespace th
