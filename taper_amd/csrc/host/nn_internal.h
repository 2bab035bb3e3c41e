// nn_internal.h -- what modules.cpp / optim.cpp / comm.cpp / trainer.cpp share beyond taper.h (host mirror internals; not installed).
#pragma once
#include "taper.h"

#define TH(call) th_check((call), #call)

namespace taper {
// modules.cpp, used by the Trainer's choice of step form (trainer.cpp)
// From this batch on a Linear + ReLU + Linear classifier steps through th_mlp2_xent: the crossover measured with bench.py --batch B (r05, with
// a knob since retired; HISTORY.md) -- launch-per-layer forms 24.9 us at 448 rows, 30.8 at 512; th_mlp2_xent 25.5 / 28.3
constexpr size_t kMlp2MinBatch = 480;
bool mlp2_shapes_ok(size_t batch, const std::vector<Tensor> &w, int64_t n_rows);
}  // namespace taper
