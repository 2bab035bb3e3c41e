// trainer.cpp -- dataset, loader and the step drivers (src/data/mnist.rs, src/train.rs, examples/train_mnist*.rs).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "nn_internal.h"
#include "../../../include/taper_hip_debug.h"   // (th_comm_debug_dump: the post-mortem under TAPER_DP_POSTMORTEM)

namespace taper {
// ---------------------------------------------------------------- data
MNISTDataset MNISTDataset::from_host(const std::vector<float> &images, const std::vector<float> &labels, bool train) {
    TAPER_ASSERT(images.size() == labels.size() * 784, "MNISTDataset: images must be [N,784]");
    MNISTDataset d;
    d.images = Tensor(images, {labels.size(), 784});
    d.labels = Tensor(labels, {labels.size()});
    d.train = train;
    return d;
}

MNISTDataset MNISTDataset::from_u8(const std::vector<uint8_t> &pixels, const std::vector<uint8_t> &labels, bool train) {
    TAPER_ASSERT(pixels.size() == labels.size() * 784, "MNISTDataset: pixels must be [N,784]");
    th_ctx *ctx = Device::ctx();
    MNISTDataset d;
    d.images = Tensor::empty({labels.size(), 784});
    auto staging = Buffer::alloc((pixels.size() + 3) / 4);
    TH(th_memcpy_h2d(ctx, staging->d, pixels.data(), pixels.size()));
    TH(th_u8_to_unit_f32(ctx, reinterpret_cast<const uint8_t *>(staging->d), d.images.dptr(), pixels.size()));  // mnist.rs:226
    std::vector<float> lf(labels.begin(), labels.end());  // mnist.rs:268
    d.labels = Tensor(lf, {labels.size()});
    d.train = train;
    Device::sync();
    return d;
}

static uint32_t be32(const unsigned char *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

MNISTDataset MNISTDataset::from_idx_files(const std::string &images_path, const std::string &labels_path, bool train) {
    auto slurp = [](const std::string &path) {
        std::ifstream f(path, std::ios::binary);
        if (!f) throw Error("Failed to open " + path);
        return std::vector<unsigned char>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    };
    std::vector<unsigned char> ib = slurp(images_path), lb = slurp(labels_path);
    // mnist.rs:185-233
    TAPER_ASSERT(ib.size() >= 16, "File " + images_path + " is too small");
    TAPER_ASSERT(be32(ib.data()) == 0x00000803, "Invalid magic number for images");
    const size_t n = be32(ib.data() + 4), rows = be32(ib.data() + 8), cols = be32(ib.data() + 12);
    TAPER_ASSERT(rows == 28 && cols == 28, "Unexpected image size");
    TAPER_ASSERT(ib.size() == 16 + n * 784, "File size mismatch (images)");
    // mnist.rs:236-274
    TAPER_ASSERT(lb.size() >= 8, "File " + labels_path + " is too small");
    TAPER_ASSERT(be32(lb.data()) == 0x00000801, "Invalid magic number for labels");
    const size_t nl = be32(lb.data() + 4);
    TAPER_ASSERT(lb.size() == 8 + nl, "File size mismatch (labels)");
    TAPER_ASSERT(nl == n, "image / label count mismatch");
    return from_u8(std::vector<uint8_t>(ib.begin() + 16, ib.end()), std::vector<uint8_t>(lb.begin() + 8, lb.end()), train);
}

static inline uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

MNISTDataset MNISTDataset::synthetic(size_t n, uint64_t seed, bool train) {
    std::vector<uint8_t> px(n * 784), lb(n);
    uint64_t s = seed;
    for (size_t i = 0; i < px.size(); i += 8) {
        uint64_t r = splitmix64(s);
        for (size_t j = 0; j < 8 && i + j < px.size(); ++j) px[i + j] = (uint8_t)(r >> (8 * j));
    }
    for (size_t i = 0; i < n; ++i) lb[i] = (uint8_t)(splitmix64(s) % 10);
    return from_u8(px, lb, train);
}

std::pair<Tensor, Tensor> MNISTDataset::get_batch(const std::vector<size_t> &indices) const {  // mnist.rs:277-310
    std::vector<int32_t> idx(indices.begin(), indices.end());
    th_ctx *ctx = Device::ctx();
    auto d_idx = Buffer::alloc(idx.size());
    TH(th_memcpy_h2d(ctx, d_idx->d, idx.data(), idx.size() * sizeof(int32_t)));
    Tensor xb = Tensor::empty({idx.size(), 784}), yb = Tensor::empty({idx.size()});
    TH(th_gather_batch(ctx, images.dptr(), labels.dptr(), reinterpret_cast<const int32_t *>(d_idx->d), (int64_t)idx.size(), nullptr,
                       (int)idx.size(), 784, xb.dptr(), yb.dptr()));
    return {xb, yb};
}

DataLoader::DataLoader(MNISTDataset dataset, size_t batch_size, bool shuffle, uint64_t seed)
    : ds_(std::move(dataset)), bs_(batch_size), shuffle_(shuffle), rng_(seed) {  // mnist.rs:335-353
    TAPER_ASSERT(batch_size > 0, "DataLoader: batch_size must be positive");
    indices_.resize(ds_.len());
    for (size_t i = 0; i < indices_.size(); ++i) indices_[i] = (int32_t)i;
    if (shuffle_) std::shuffle(indices_.begin(), indices_.end(), rng_);
    d_idx_ = Buffer::alloc(std::max<size_t>(indices_.size(), 1));
    upload_indices();
}

void DataLoader::upload_indices() {
    TH(th_memcpy_h2d(Device::ctx(), d_idx_->d, indices_.data(), indices_.size() * sizeof(int32_t)));
}

void DataLoader::reset() {  // mnist.rs:355-363
    cur_ = 0;
    if (shuffle_) {
        std::shuffle(indices_.begin(), indices_.end(), rng_);
        upload_indices();
    }
}

size_t DataLoader::num_batches() const { return (ds_.len() + bs_ - 1) / bs_; }  // mnist.rs:365-367

bool DataLoader::next(Tensor *images, Tensor *labels) {  // mnist.rs:373-385 (keeps the last partial batch)
    if (cur_ >= ds_.len()) return false;
    const size_t end = std::min(cur_ + bs_, ds_.len()), b = end - cur_;
    *images = Tensor::empty({b, 784});
    *labels = Tensor::empty({b});
    TH(th_gather_batch(Device::ctx(), ds_.images.dptr(), ds_.labels.dptr(), d_indices() + cur_, (int64_t)b, nullptr, (int)b, 784,
                       images->dptr(), labels->dptr()));
    cur_ = end;
    return true;
}

// ---------------------------------------------------------------- trainer
static Tensor shape_input(const Tensor &images, const Shape &sample_shape) {
    if (sample_shape.empty()) return images;
    Shape s{images.shape()[0]};
    s.insert(s.end(), sample_shape.begin(), sample_shape.end());
    return images.reshape(s);  // train_mnist_cnn.rs:161-162
}

static void reduce_grads(Trainer &t) {
    // (the Adam step behind a peer-to-peer all-reduce skips itself on the device when that all-reduce timed out)
    t.optimizer->set_step_guard(t.comm && t.comm->is_p2p() ? t.comm->error_word() : nullptr);
    if (!t.comm) return;
    FlatParams &fp = t.optimizer->flat();
    fp.zero_missing();  // grad None contributes zeros; the has_grad mask is rank-invariant
    t.comm->allreduce_mean(fp.g_arena->d, (size_t)fp.total);
}

void Trainer::train_step(const Tensor &images, const Tensor &labels, float *loss_out, float *acc_out) {
    Tape::reset();                                              // train_mnist.rs:91
    check_batchnorm_comm();
    if (has_qat()) {
        TAPER_ASSERT(!comm, "QAT: data-parallel training of a QAT model is not supported");
        qat_pass_.run(*model);                                  // every active QAT layer's weights: one launch pair
    }
    Tensor logits = model->forward(shape_input(images, sample_shape));  // :101
    Tensor loss = cross_entropy_loss(logits, labels);           // :107
    const float acc = accuracy(logits, labels);                 // :110
    loss.backward();                                            // :115
    if (!(comm && optimizer->step_reduced(*comm))) {
        reduce_grads(*this);
        optimizer->step();                                      // :118
    }
    optimizer->zero_grad();                                     // :119
    if (loss_out) *loss_out = loss.data()[0];                   // :121
    if (acc_out) *acc_out = acc;
    check_comm();                                               // (the read-back above synchronised the stream)
}

void Trainer::check_comm() const {
    // a peer that never arrived at an all-reduce: the launch applied nothing and every later one is a no-op (th_comm_error_peek) -- the
    // replicas are no longer in step, and the run must end here, loudly, not train on
    if (comm && comm->is_p2p() && comm->failed()) {
        if (const char *e = std::getenv("TAPER_DP_POSTMORTEM"); e && atoi(e)) th_comm_debug_dump(comm->handle(), Device::ctx());
        int d[4] = {-1, 0, 0, 0};
        th_comm_timeout_detail(comm->handle(), Device::ctx(), d);
        std::string where;
        if (d[0] >= 0) {
            where = "; first wait to run out: slot " + std::to_string(d[0]) + " of exchange step " + std::to_string(d[1]) + ", nothing from rank(s)";
            for (int s = 0; s < comm->n_ranks; ++s)
                if (d[2] >> s & 1) where += " " + std::to_string(s);
        }
        throw Error("data-parallel all-reduce timed out waiting for a peer (rank " + std::to_string(comm->rank) + " of " +
                    std::to_string(comm->n_ranks) + "): no update was applied from that step on; the replicas are out of step" + where);
    }
}

EpochResult Trainer::train_epoch(DataLoader &loader) {  // train.rs:98-144
    EpochResult r;
    float total_loss = 0.f;
    loader.reset();
    r.num_batches = loader.num_batches();
    Tensor images, labels;
    while (loader.next(&images, &labels)) {
        float loss, acc;
        train_step(images, labels, &loss, &acc);
        const size_t b = images.shape()[0];
        r.total_correct += (size_t)(acc * (float)b);  // train.rs:117 (truncating cast, Q13)
        r.total_samples += b;
        total_loss += loss;
        r.losses.push_back(loss);
        r.ncorrect.push_back(acc * (float)b);
    }
    r.avg_loss = total_loss / (float)r.num_batches;                    // train.rs:140
    r.accuracy = (float)r.total_correct / (float)r.total_samples;      // train.rs:141
    return r;
}

// A log of {loss, n_correct} per batch -> the epoch's figures (evaluate, train_epoch_graph): the first n_full batches have bs rows, the one
// behind them last_rows.
static EpochResult epoch_result(const float *log, size_t nb, size_t n_full, size_t bs, size_t last_rows) {
    EpochResult r;
    r.num_batches = nb;
    float total_loss = 0.f;
    for (size_t s = 0; s < nb; ++s) {
        const size_t b = s < n_full ? bs : last_rows;
        const float acc = log[2 * s + 1] / (float)b;      // loss.rs:289
        r.total_correct += (size_t)(acc * (float)b);      // train.rs:117, :160 (truncating cast, Q13)
        r.total_samples += b;
        total_loss += log[2 * s];
        r.losses.push_back(log[2 * s]);
        r.ncorrect.push_back(log[2 * s + 1]);
    }
    r.avg_loss = total_loss / (float)nb;
    r.accuracy = (float)r.total_correct / (float)r.total_samples;
    return r;
}

EpochResult Trainer::evaluate(DataLoader &loader) {  // train.rs:147-172
    // Same formulas, no per-batch read-back: the loss kernel appends {loss, n_correct} of every batch to a device
    // log (as in the graph-replayed training epoch) and the host reads the log once at the end.
    loader.reset();
    const size_t nb = loader.num_batches();
    if (nb == 0) return EpochResult{};
    // BatchNorm2d layers run on their running statistics for the duration; each gets its own flag back (Dropout is left as it is)
    struct EvalMode {
        std::vector<std::pair<BatchNorm2d *, bool>> was;
        explicit EvalMode(Module &m) {
            std::vector<BatchNorm2d *> bns;
            batchnorm_modules(m, &bns);
            for (BatchNorm2d *b : bns) {
                was.emplace_back(b, b->is_training());
                b->eval();
            }
        }
        ~EvalMode() {
            for (auto &w : was) w.first->set_training(w.second);
        }
    } eval_mode(*model);
    th_ctx *ctx = Device::ctx();
    auto log = Buffer::alloc(2 * nb), st = Buffer::alloc(4);
    TH(th_fill_f32(ctx, st->d, 0.f, 4));
    Tensor images, labels;
    // nothing is differentiated here: a Sequential's conv front may take the launches that never write the full-resolution maps
    // (conv + pool pairs, the one-launch conv chain from batch 96 up) exactly as inside a training step
    // (the same condition as a training step's; NoGradScope: no count buffers, no bias tape nodes for gradients nobody will ask for)
    PoolBiasScope pool_scope(fuse_head && dynamic_cast<Sequential *>(model.get()) != nullptr);
    NoGradScope no_grad;
    while (loader.next(&images, &labels)) {
        Tape::reset();
        const size_t b = images.shape()[0];
        StepLogSink sink{log->d, (int64_t)nb, reinterpret_cast<int64_t *>(st->d), (int64_t)b, nullptr};
        Tensor logits = model->forward(shape_input(images, sample_shape));
        Tensor ncorrect;
        cross_entropy_loss(logits, labels, &ncorrect, &sink);   // loss.rs:136-195 + the count of loss.rs:271-290
    }
    Tape::reset();
    std::vector<float> mt(2 * nb);
    TH(th_memcpy_d2h(ctx, mt.data(), log->d, mt.size() * sizeof(float)));
    const size_t bs = loader.batch_size(), n_full = loader.dataset().len() / bs;   // (DataLoader::next: full batches, then what is left)
    return epoch_result(mt.data(), nb, n_full, bs, loader.dataset().len() - n_full * bs);
}

// The captured form of a step: identical arithmetic, but nothing is read back.  The batches
// come from the device-resident dataset through the device cursor (ONE gather launch for a
// whole chunk of steps), and the loss kernel itself appends {loss, n_correct} to the device
// log and advances the step / cursor state.

static const char *const step_form_names[] = {"mlp2_rows", "chain_mlp3", "mlp3", "chain_head", "mlp_tail", "linear_head", "linear_wide", "layered"};
static_assert(sizeof step_form_names / sizeof *step_form_names == (size_t)StepForm::Layered + 1, "one name per StepForm");

void StepPlan::key(std::vector<uintptr_t> *out) const {
    out->push_back((uintptr_t)form);
    out->push_back((uintptr_t)prefix);
    out->push_back((uintptr_t)fused_adam | (uintptr_t)pool_bias << 1 | (uintptr_t)conv_chain << 2 | (uintptr_t)exchange << 3);
}

// The form of a step of `batch` rows, chosen on EVERYTHING the step will ask for -- the model's structure, the parameters' state (every one
// trains, no gradient already present, aligned storage), the switches and the communicator -- so that no form has to fall back to another
// once launches are enqueued (a frozen layer or gradients left by a manual backward take a slower form, they do not fail inside the step).
// The fused ops keep their own TAPER_ASSERTs on the same predicates as the guard.  A predicate that reads the fused part's input is given a
// stand-in of its shape: the step's rows in front of the first layer, else the [batch, in] output of the prefix, which is fresh and
// requires a gradient exactly when a parameter in front of it does.
StepPlan Trainer::plan_step(size_t batch, int64_t n_rows) const {
    StepPlan p;
    auto *seq = dynamic_cast<Sequential *>(model.get());
    const size_t nl = seq ? seq->layers.size() : 0;
    p.pool_bias = fuse_head && seq;
    p.conv_chain = conv_chain_enabled();
    auto linear = [&](size_t i) { return dynamic_cast<Linear *>(seq->layers[i].get()); };
    auto relu = [&](size_t i) { return dynamic_cast<ReLU *>(seq->layers[i].get()) != nullptr; };
    auto flatten = [&](size_t i) { auto *f = dynamic_cast<Flatten *>(seq->layers[i].get()); return f && f->start_dim == 1; };
    const Tensor xin = shape_input(Tensor::from_device(nullptr, {batch, 784}), sample_shape);
    auto input_of = [&](size_t i, size_t width) {
        if (i == 0) return xin;
        bool needs_grad = false;
        for (size_t j = 0; j < i; ++j)
            for (const Tensor &q : seq->layers[j]->parameters()) needs_grad = needs_grad || q.get_requires_grad();
        Tensor h = Tensor::from_device(nullptr, {batch, width});
        h.set_requires_grad(needs_grad);
        return h;
    };
    // data parallel: the steps whose gradient launch can exchange with the peers keep their fused Adam epilogues, which apply the mean
    const bool dp = comm && comm->is_p2p() && comm->fuse_adam && fuse_adam;
    auto take = [&](StepForm f, size_t prefix, std::initializer_list<Linear *> ls, bool exchange = false) {
        p.form = f;
        p.prefix = prefix;
        std::copy(ls.begin(), ls.end(), p.linear);
        p.exchange = exchange;
        // Adam updates ride in the epilogues of the kernels that produce the gradients -- unless the gradients still have to be all-reduced
        // across ranks first, by a launch of their own
        p.fused_adam = fuse_adam && (!comm || exchange);
        return p;
    };
    check_batchnorm_comm();
    // a QAT model trains layer by layer: its layers fake-quantize their weights and outputs, which no fused form does
    if (has_qat()) {
        TAPER_ASSERT(!comm, "QAT: data-parallel training of a QAT model is not supported");
        return take(StepForm::Layered, nl, {});
    }
    // a tied layer trains layer by layer too, and Adam runs behind the whole backward: the node of the layer's LATER use finds the gradient
    // slot empty and would apply (or defer) the update on that use's share alone, the earlier use would then read the updated weight for its
    // dX and add a dW that Adam::step skips as already applied -- and no fused form is written for one weight in two places
    if (has_shared_parameter()) {
        take(StepForm::Layered, nl, {});
        p.fused_adam = false;
        return p;
    }
    // the exact pointwise convolution belongs to no fused form (the conv chain's stages are 3x3 rows): such a model trains layer by layer
    if (holds_exact_pointwise(*model)) return take(StepForm::Layered, nl, {});
    Linear *last = (fuse_head && nl) ? linear(nl - 1) : nullptr;
    Linear *hidden = (last && fuse_head >= 2 && seq->fuse && nl >= 3 && relu(nl - 2)) ? linear(nl - 3) : nullptr;
    Linear *hidden0 = (hidden && nl >= 5 && relu(nl - 4)) ? linear(nl - 5) : nullptr;   // a three-layer classifier: th_mlp3_xent, two launches
    // the conv rows in front of the classifier as one launch with the classifier's rows in its last epilogue
    const bool chain_head = fuse_head >= 2 && seq && seq->fuse && conv_chain_enabled() && conv_chain_head_enabled() && xin.shape().size() == 4;

    // Linear + ReLU (+ Linear + ReLU) + Linear on the loader's 784-wide rows (BASELINE's 784-128-10, examples/train_mnist.rs:40-48's
    // 784-128-64-10) at large batch: three launches for the whole step, the rows read in place
    if (hidden && sample_shape.empty() && batch >= kMlp2MinBatch && (nl == 3 || (nl == 5 && relu(1) && linear(0)))) {
        std::vector<Tensor> w, b;
        for (size_t i = 0; i < nl; i += 2) {
            w.push_back(linear(i)->weight);
            b.push_back(linear(i)->bias);
        }
        // Two hidden layers: below ~1 800 rows the two-launch classifier (th_mlp3_xent behind a gather) is the faster step where it applies --
        // 26.7 / 30.3 / 32.8 / 39.2 us at 512 / 768 / 1 024 / 1 536 rows against 34.4 / 35.8 / 37.7 / 42.0 for th_mlp2_xent_deep, whose 16-row
        // blocks each leave a whole [h2][h1] share of dW2 behind; 47.5 against 43.7 at 2 048 (r05, with a probe and a knob since retired;
        // HISTORY.md)
        constexpr size_t kDeepMinBatch = 1792;
        const bool mlp3_faster = nl == 5 && batch < kDeepMinBatch &&
                                 th_mlp3_supported((int)batch, (int)w[0].shape()[1], (int)w[0].shape()[0], (int)w[1].shape()[0], (int)w[2].shape()[0]);
        if (w[0].shape()[1] == 784 && mlp2_params_ok(w, b) && mlp2_shapes_ok(batch, w, n_rows) && !mlp3_faster)
            return nl == 3 ? take(StepForm::Mlp2Rows, 0, {hidden, last}) : take(StepForm::Mlp2Rows, 0, {linear(0), hidden, last});
    }
    // Linear + ReLU + Linear + ReLU + Linear + cross-entropy: two launches for the whole classifier (th_mlp3_xent)
    if (hidden0) {
        const Tensor w3[3] = {hidden0->weight, hidden->weight, last->weight}, b3[3] = {hidden0->bias, hidden->bias, last->bias};
        // the reference CNN whole (conv rows + pools, global average pool, Flatten, this classifier): its rows in the chain launch
        if (chain_head && nl >= 8 && flatten(nl - 6) && seq->conv_stages_at(0, nl - 6, &p.stages) == nl - 6 &&
            conv_chain_mlp3_supported(xin, p.stages, w3, b3))
            return take(StepForm::ChainMlp3, 0, {hidden0, hidden, last});
        p.stages.clear();
        const size_t in_f = hidden0->weight.shape()[1];
        // (parameters th_mlp3_xent cannot take -- a frozen layer, a Linear without a bias: the classifier runs layer by layer, unfused)
        if (th_mlp3_supported((int)batch, (int)in_f, (int)w3[0].shape()[0], (int)w3[1].shape()[0], (int)w3[2].shape()[0]))
            return mlp3_supported(input_of(nl - 5, in_f), w3, b3) ? take(StepForm::Mlp3, nl - 5, {hidden0, hidden, last})
                                                                  : take(StepForm::Layered, nl - 5, {});
    }
    // conv rows + Flatten + Linear + cross-entropy (the simple CNN): two launches per step
    if (last && !hidden && chain_head && nl >= 3 && flatten(nl - 2) && seq->conv_stages_at(0, nl - 2, &p.stages) == nl - 2 &&
        conv_chain_head_supported(xin, p.stages, last->weight, last->bias)) {
        // (data parallel: the compiled simple chain, whose tick carries the step number, and the batch sums' launch can take the exchange)
        const bool exchange = dp && xin.conv_chain_head_supported(p.stages, (int)last->weight.shape()[0]) == 2 &&
                              comm->wide_exchange_ok((int)batch, (int)last->weight.shape()[1], (int)last->weight.shape()[0],
                                                     (int)p.stages.back().weight.shape()[0]);
        return take(StepForm::ChainHead, 0, {last}, exchange);
    }
    p.stages.clear();
    if (!last) return take(StepForm::Layered, nl, {});
    // Linear + ReLU + Linear + cross-entropy: two launches per step
    if (hidden && mlp_tail_supported(input_of(nl - 3, hidden->weight.shape()[1]), hidden->weight, hidden->bias, last->weight, last->bias)) {
        // (data parallel: straight on the loader's rows with both biases, and the communicator can exchange the slices inside the launch)
        const bool exchange = dp && nl == 3 && sample_shape.empty() && hidden->bias.defined() && last->bias.defined() &&
                              comm->tail_exchange_ok((int)batch, 784, (int)hidden->weight.shape()[0], (int)last->weight.shape()[0]);
        return take(StepForm::MlpTail, nl - 3, {hidden, last}, exchange);
    }
    const Tensor h = input_of(nl - 1, last->weight.shape()[1]);
    if (linear_cross_entropy_supported(h, last->weight) && !last->weight.has_grad() && !(last->bias.defined() && last->bias.has_grad()))
        return take(StepForm::LinearHead, nl - 1, {last});
    if (fuse_head >= 2 && linear_cross_entropy_wide_supported(h, last->weight, last->bias)) return take(StepForm::LinearWide, nl - 1, {last});
    return take(StepForm::Layered, nl, {});
}

void Trainer::enqueue_compute(const StepPlan &plan, float *d_xb, float *d_yb, size_t batch, const th_row_source *rows) {
    int64_t *state = reinterpret_cast<int64_t *>(state_->d);
    FusedAdamScope scope(plan.fused_adam ? optimizer.get() : nullptr);
    PoolBiasScope pool_scope(plan.pool_bias);
    Tape::reset();
    StepLogSink sink{metrics_->d, (int64_t)metrics_cap_, state, (int64_t)batch, plan.fused_adam ? optimizer->d_tick() : nullptr,
                     plan.exchange ? comm.get() : nullptr};
    // this function ends in zero_grad(), so a gradient an epilogue has applied is dead unless a communicator reads the gradient arena
    // (reduce_grads, step_reduced, the in-launch exchange) or a second use of the parameter adds to the slot -- and a model with a shared
    // parameter never takes this form: plan_step trains it layer by layer (has_shared_parameter)
    sink.drop_applied_grads = plan.form == StepForm::MlpTail && plan.fused_adam && !comm;
    Adam *adam = optimizer.get();
    auto *seq = dynamic_cast<Sequential *>(model.get());
    Linear *const *L = plan.linear;
    Tensor ncorrect, loss, xin, y;
    if (!rows) {
        xin = shape_input(Tensor::from_device(d_xb, {batch, 784}), sample_shape);
        y = Tensor::from_device(d_yb, {batch});
    }
    switch (plan.form) {
        case StepForm::Mlp2Rows: {   // (every step ends with zero_grad: the parameters' state plan_step saw holds for each)
            std::vector<Tensor> w, b;
            for (Linear *l : plan.linear)
                if (l) {
                    w.push_back(l->weight);
                    b.push_back(l->bias);
                }
            loss = mlp2_cross_entropy(*rows, batch, w, b, &ncorrect, &sink);
            break;
        }
        case StepForm::ChainMlp3:
        case StepForm::Mlp3: {
            const Tensor w3[3] = {L[0]->weight, L[1]->weight, L[2]->weight}, b3[3] = {L[0]->bias, L[1]->bias, L[2]->bias};
            loss = plan.form == StepForm::ChainMlp3 ? conv_chain_mlp3_cross_entropy(xin, plan.stages, w3, b3, y, &ncorrect, &sink)
                                                    : mlp3_cross_entropy(seq->forward_prefix(xin, plan.prefix), w3, b3, y, &ncorrect, &sink);
            break;
        }
        case StepForm::ChainHead:
            loss = conv_chain_head_cross_entropy(xin, plan.stages, L[0]->weight, L[0]->bias, y, &ncorrect, &sink);
            break;
        case StepForm::MlpTail: {
            Tensor xh = seq->forward_prefix(xin, plan.prefix);
            if (plan.fused_adam) adam->set_carry_deferred(true);   // flushed by enqueue_steps
            loss = mlp_tail_cross_entropy(xh, L[0]->weight, L[0]->bias, L[1]->weight, L[1]->bias, y, &ncorrect, &sink);
            break;
        }
        case StepForm::LinearHead:
        case StepForm::LinearWide: {
            // updates a previous tail step left for its successor must run with ITS counter: before this step's tick
            adam->flush_deferred();
            Tensor h = seq->forward_prefix(xin, plan.prefix);
            loss = plan.form == StepForm::LinearHead ? linear_cross_entropy(h, L[0]->weight, L[0]->bias, y, &ncorrect, &sink)
                                                     : linear_cross_entropy_wide(h, L[0]->weight, L[0]->bias, y, &ncorrect, &sink);
            break;
        }
        case StepForm::Layered: {
            adam->flush_deferred();
            qat_pass_.run(*model);   // (after the flush: this step's fake-quantized weights are made from the updated masters)
            Tensor h = seq ? seq->forward_prefix(xin, plan.prefix) : model->forward(xin);
            for (size_t i = plan.prefix; seq && i < seq->layers.size(); ++i) h = seq->layers[i]->forward(h);
            loss = cross_entropy_loss(h, y, &ncorrect, &sink);
            break;
        }
    }
    loss.backward();
    if (plan.exchange) {
        optimizer->step();   // (nothing is left: every update ran in an epilogue, on the mean gradient, or waits for the next step's first launch)
    } else if (!(comm && optimizer->step_reduced(*comm))) {   // peer-to-peer communicator: all-reduce + Adam in one launch
        reduce_grads(*this);
        optimizer->step();
        optimizer->set_step_guard(nullptr);   // (the guard is the communicator's word: it must not outlive this call in the optimizer -- ADVICE r04)
    }
    optimizer->zero_grad();
    adam->set_carry_deferred(false);
}

void Trainer::enqueue_steps(const float *d_images, const float *d_labels, const int32_t *d_indices, int64_t n_indices,
                            size_t batch, size_t steps) {
    int64_t *state = reinterpret_cast<int64_t *>(state_->d);
    // behind a failed exchange of a peer-to-peer communicator nothing may move: the launches that apply deferred updates or tick Adam's
    // counter (the next step's first launch, the flush below) look at its error word first
    // (and every tick of Adam's counter advances the exchange's step number with it: th_ctx_set_update_guard)
    struct Guard {
        Guard(const uint32_t *w, uint32_t *step) { TH(th_ctx_set_update_guard(Device::ctx(), w, step)); }
        ~Guard() { th_ctx_set_update_guard(Device::ctx(), nullptr, nullptr); }
    } guard(comm && comm->is_p2p() ? comm->error_word() : nullptr, comm && comm->is_p2p() ? comm->step_word() : nullptr);
    // ranks sharing this device: their waiting workgroups occupy CUs, and the forward launch's sub-tile forms were measured on a free chip only
    TH(th_linear_fwd_ex_set_subtiles(Device::ctx(), !(comm && comm->ranks_on_this_device() > 1)));
    const StepPlan plan = plan_step(batch, d_indices ? n_indices : (int64_t)batch);
    if (plan.form == StepForm::Mlp2Rows) {
        // the step reads its rows where they lie: through the index vector at the device cursor (every step's log advances it), or the
        // dataset itself for the one-step epoch in index order -- no gather launch, no staging buffer
        const th_row_source rows{d_images, d_labels, d_indices, d_indices ? state + 1 : nullptr, d_indices ? n_indices : 0,
                                 d_indices ? n_indices : (int64_t)batch};
        for (size_t s = 0; s < steps; ++s) enqueue_compute(plan, nullptr, nullptr, batch, &rows);
    } else if (d_indices == nullptr) {
        // one step over the whole dataset in index order: the "gathered" batch IS the dataset (no copy)
        enqueue_compute(plan, const_cast<float *>(d_images), const_cast<float *>(d_labels), batch);
    } else {
        TH(th_gather_batch(Device::ctx(), d_images, d_labels, d_indices, n_indices, state + 1, (int)(batch * steps), 784, xb_->d,
                           yb_->d));
        for (size_t s = 0; s < steps; ++s) enqueue_compute(plan, xb_->d + s * batch * 784, yb_->d + s * batch, batch);
    }
    // a tail step leaves the head's W / b updates for its successor's first launch; the last one's run here
    optimizer->flush_deferred();
}

void Trainer::check_batchnorm_comm() const {
    if (!comm) return;
    // per-rank batch statistics: the replicas' running pairs -- and, through the normalised activations, their gradients' meaning -- would
    // drift apart; synchronised statistics are not implemented
    std::vector<BatchNorm2d *> bns;
    batchnorm_modules(*model, &bns);
    TAPER_ASSERT(bns.empty(), "BatchNorm2d: data-parallel training of a model with batch normalisation is not supported (statistics are per rank)");
}

bool Trainer::has_qat() const {
    std::vector<const QATModule *> mods;
    qat_modules(*model, &mods, false);
    // the same layer twice: its backward launches would both accumulate into one master gradient, and a fused Adam update deferred by the
    // first could ride in the second (Adam::take_deferred recognises a shared weight by the pointer the launch reads: here the round trip)
    for (size_t i = 0; i < mods.size(); ++i)
        for (size_t j = i + 1; j < mods.size(); ++j)
            TAPER_ASSERT(mods[i] != mods[j], "QAT: the model holds the same QAT layer twice; the Trainer does not train a shared QAT layer");
    return !mods.empty();
}

bool Trainer::has_shared_parameter() const {
    const std::vector<Tensor> ps = model->parameters();
    for (size_t i = 0; i < ps.size(); ++i)
        for (size_t j = i + 1; j < ps.size(); ++j)
            if (ps[i].dptr() == ps[j].dptr()) return true;
    return false;
}

// ---- StepGraphs: policy, the one capture path, replay (taper.h)
void StepGraphs::drop() {
    for (auto &g : steps_) th_graph_destroy(g.second);
    steps_.clear();
    for (auto &g : whole_) th_graph_destroy(g.second);
    whole_.clear();
    whole_failed_.clear();
}

void StepGraphs::begin_call(std::vector<uintptr_t> key) {
    events_.clear();
    call_key_ = std::move(key);
    if (!steps_.empty() && !current()) drop();
}

static bool power_of_two(size_t v) { return (v & (v - 1)) == 0; }

std::vector<size_t> StepGraphs::ladder_to_record(size_t chunk, size_t n_full) const {
    std::vector<size_t> want;
    if (n_full == 0 || off_) return want;
    for (size_t s = chunk; s >= 1; s /= 2)
        if ((s == 1 || n_full >= s + 1) && !have(s)) want.push_back(s);
    return want;
}

bool StepGraphs::wants_remainder(size_t tail) const {
    size_t exact = 0;
    for (auto &g : steps_) exact += power_of_two(g.first) ? 0 : 1;
    return tail > 2 && !power_of_two(tail) && !have(tail) && have(1) && exact < 4 && !off_ && current();
}

bool StepGraphs::wants_whole(size_t n_full) const {
    return n_full >= 2 && have(n_full) && whole_.size() < 4 && !off_ &&
           std::find(whole_failed_.begin(), whole_failed_.end(), n_full) == whole_failed_.end() && current();
}

bool StepGraphs::capture(Kind kind, size_t steps, Adam &optimizer, bool rethrow, const std::function<void()> &body) {
    th_ctx *ctx = Device::ctx();
    TH(th_graph_begin(ctx));
    th_graph *g = nullptr;
    try {
        body();
        TH(th_graph_end(ctx, &g));
    } catch (const std::exception &e) {
        if (!g) th_graph_end(ctx, &g);
        if (g) th_graph_destroy(g);
        optimizer.set_carry_deferred(false);
        optimizer.drop_step_bookkeeping();
        optimizer.zero_grad();
        Tape::reset();
        switch (kind) {
            case Kind::Ladder:
                fprintf(stderr, "taper: step capture with the communicator failed (%s); running data-parallel steps eagerly\n", e.what());
                off_ = true;
                break;
            case Kind::Remainder:
                fprintf(stderr, "taper: capturing a %zu-step remainder graph failed (%s); the ladder graphs serve it\n", steps, e.what());
                break;
            case Kind::Whole:
                fprintf(stderr, "taper: capturing a whole-call graph of %zu steps failed (%s); reset + replay stay two launches\n", steps, e.what());
                whole_failed_.push_back(steps);
                break;
        }
        if (rethrow) throw;
        return false;
    }
    if (kind == Kind::Whole) {
        whole_.emplace_back(steps, g);
    } else {
        steps_.insert(std::find_if(steps_.begin(), steps_.end(), [&](const auto &x) { return x.first < steps; }), {steps, g});   // largest first
        if (kind == Kind::Ladder) key_ = call_key_;
    }
    note(kind == Kind::Whole ? kCaptureWhole : kCapture, steps);
    return true;
}

void StepGraphs::replay_whole(size_t n_full) {
    TH(th_graph_launch(Device::ctx(), find(whole_, n_full)));
    note(kReplayWhole, n_full);
}

size_t StepGraphs::replay_largest(size_t left) {
    for (auto &g : steps_)
        if (g.first <= left) {
            TH(th_graph_launch(Device::ctx(), g.second));
            note(kReplay, g.first);
            return g.first;
        }
    return 0;
}

static bool env_is_1(const char *name) {   // read on every call: a process may set and unset the operator overrides between calls
    const char *e = std::getenv(name);
    return e && e[0] == '1';
}

// QAT: the descriptor buffer the steps read is uploaded in front of any step of a call, and graph_key then keys on its generation -- a
// buffer replaced since (an eager train_step after a layer switched) has gone back to the pool, and the graphs that read it must not replay
void Trainer::sync_qat_descriptors() {
    std::vector<const QATModule *> active;
    qat_modules(*model, &active, true);
    qat_pass_.sync(active);
}

// Everything a captured step bakes in: the kernel arguments and what the layered path reads -- the dataset and index buffers (two loaders
// over one dataset share the images but own their index vectors), the epoch length the gather wraps at, the label buffer, the input
// reshape, the communicator, the optimizer's arenas -- then the full batch's plan (the choice of launch sequence, and every switch it read:
// a communicator's inkernel / fuse_adam included).  (nullptr indices = the zero-copy full-batch form, a different graph.)  Any
// mismatch re-records.  (The last, partial batch is never captured -- enqueue_steps plans it afresh every call -- and a call cut short
// by max_steps has none: keying on its plan would re-record the graphs whenever such calls alternate with whole epochs.)
std::vector<uintptr_t> Trainer::graph_key(const StepPlan &plan, const float *d_img, const float *d_lab, const int32_t *d_idx, size_t n, size_t bs) const {
    std::vector<uintptr_t> key{(uintptr_t)d_img, (uintptr_t)d_lab, (uintptr_t)d_idx, (uintptr_t)n, (uintptr_t)bs, (uintptr_t)comm.get(),
                               (uintptr_t)model.get(), (uintptr_t)optimizer.get(), (uintptr_t)optimizer->flat().p_arena->d,
                               (uintptr_t)optimizer->flat().g_arena->d, (uintptr_t)(xb_ ? xb_->d : nullptr), (uintptr_t)metrics_->d};
    plan.key(&key);
    for (size_t d : sample_shape) key.push_back((uintptr_t)d);
    // beta1 / beta2 / eps / weight decay are kernel arguments BY VALUE (only lr and t live in device memory)
    for (float h : {optimizer->beta1(), optimizer->beta2(), optimizer->eps(), optimizer->weight_decay()}) {
        uint32_t bits;
        std::memcpy(&bits, &h, sizeof bits);
        key.push_back(bits);
    }
    key.push_back((uintptr_t)full_backward());
    // which parameters train, as the layered path's tape bakes it in (freezing a layer behind a capture re-records -- ADVICE r05)
    {
        uintptr_t h = 1469598103934665603ull;
        for (const Tensor &p : optimizer->flat().params) h = (h ^ (uintptr_t)(p.get_requires_grad() ? 2 : 1)) * 1099511628211ull;
        key.push_back(h);
    }
    // QAT: whether each layer fake-quantizes (the global switch, training mode, every layer's own flag) and its codec and activation switch,
    // and the generation of the descriptor buffer (sync_qat_descriptors)
    {
        std::vector<const QATModule *> mods;
        qat_modules(*model, &mods, false);
        if (!mods.empty()) {
            key.push_back((uintptr_t)qat::enabled() | (uintptr_t)qat::is_training() << 1);
            key.push_back((uintptr_t)qat_pass_.generation());
        }
        for (const QATModule *q : mods)
            key.push_back((uintptr_t)q->active() | (uintptr_t)q->config.activations << 1 | (uintptr_t)q->config.qtype << 2);
    }
    // BatchNorm2d: each layer's mode (a captured step bakes in which statistics it normalises with and whether it updates the running pair)
    {
        std::vector<BatchNorm2d *> bns;
        batchnorm_modules(*model, &bns);
        for (const BatchNorm2d *b : bns) key.push_back((uintptr_t)0xb0 | (uintptr_t)b->is_training());
    }
    return key;
}

static bool trace_epoch() {   // TAPER_TRACE_EPOCH: host-side timeline of one call (stderr), a measurement probe
    static const bool on = std::getenv("TAPER_TRACE_EPOCH") != nullptr;
    return on;
}

EpochResult Trainer::train_epoch_graph(DataLoader &loader, size_t max_steps) {
    th_ctx *ctx = Device::ctx();
    const auto t_enter = std::chrono::steady_clock::now();
    auto us_since = [&](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(); };
    // ---- sizes and plans
    loader.reset();
    const MNISTDataset &ds = loader.dataset();
    const size_t n = ds.len(), bs = loader.batch_size();
    size_t nb = loader.num_batches();
    if (max_steps && max_steps < nb) nb = max_steps;
    const size_t n_full = std::min(nb, n / bs);
    // the forms of the full and the last, partial batch; steps per replay: graph_chunk, capped so that the gathered batches of one chunk stay
    // within 256 MB (steps that read their rows in place gather nothing)
    const size_t rem_rows = nb > n_full ? n - n_full * bs : 0;   // the last, partial batch (mnist.rs:373-385 keeps it)
    const StepPlan plan = plan_step(bs, (int64_t)n), rem_plan = rem_rows ? plan_step(rem_rows, (int64_t)n) : StepPlan{};
    const bool full_in_place = plan.form == StepForm::Mlp2Rows;
    const size_t chunk = full_in_place ? std::max<size_t>(graph_chunk, 1) : std::max<size_t>(std::min<size_t>(graph_chunk, ((size_t)1 << 26) / (bs * 784)), 1);
    const float *d_img = ds.images.dptr(), *d_lab = ds.labels.dptr();
    // full batch, index order (mnist.rs:355-363 without shuffle): the gather would be an identity copy of 188 MB
    const int32_t *d_idx = (!loader.shuffled() && bs >= n && nb == 1) ? nullptr : loader.d_indices();
    // ---- staging and log buffers (the captured graphs hold their addresses: a new buffer drops the graphs)
    // staging rows for the gathered forms: a chunk of full batches, and / or the last partial batch when it is too small for the in-place form
    const size_t stage_rows = std::max(full_in_place ? (size_t)0 : chunk * bs, (rem_rows && rem_plan.form != StepForm::Mlp2Rows) ? rem_rows : (size_t)0);
    if (d_idx && stage_rows && (!xb_ || xb_->n < stage_rows * 784)) {   // (the zero-copy forms read the dataset in place: no staging buffers)
        drop_graphs();
        xb_ = Buffer::alloc(stage_rows * 784);
        yb_ = Buffer::alloc(stage_rows);
    }
    if (!state_) state_ = Buffer::alloc(4);
    // the step log is sized for the loader's whole epoch even when this call stops early (max_steps): the captured graphs
    // hold its address, and a short first call followed by a full epoch would otherwise drop and re-record every graph
    if (metrics_cap_ < loader.num_batches() + 1) {
        drop_graphs();
        metrics_cap_ = loader.num_batches() + 1;
        // pinned host memory: the loss kernels write {loss, n_correct} of every step straight into it (8 B per step, posted writes), and the
        // host reads it after ONE stream synchronisation -- a staged device-to-host copy costs a short run (the contract's 20 steps) ~20 us
        metrics_ = Buffer::alloc_host(2 * metrics_cap_);
    }
    // ---- key
    sync_qat_descriptors();
    graphs_.begin_call(graph_key(plan, d_img, d_lab, d_idx, n, bs));

    // ---- schedule: what is recorded and what replays is StepGraphs' policy (taper.h); here is the order of a call
    auto reset_state = [&] { TH(th_fill_f32(ctx, state_->d, 0.f, 4)); };   // step = 0, cursor = 0
    auto steps_of = [&](size_t batch, size_t steps) { enqueue_steps(d_img, d_lab, d_idx, (int64_t)n, batch, steps); };
    auto eager = [&](size_t batch, size_t steps) {
        steps_of(batch, steps);
        graphs_.note(StepGraphs::kEager, steps);
    };
    auto capture = [&](StepGraphs::Kind kind, size_t steps, const std::function<void()> &body) {
        return graphs_.capture(kind, steps, *optimizer, !comm, body);
    };
    // operator override: TAPER_NO_GRAPH=1 enqueues every step's op list eagerly instead of replaying captured graphs -- same kernels, same
    // results, one host launch per kernel (rocprofv3 on ROCm 7.2 crashes inside hipGraphLaunch once several instantiated graphs are replayed
    // back to back: profiling runs use this)
    if (env_is_1("TAPER_NO_GRAPH")) graphs_.latch_off();
    size_t done = 0;
    const bool whole = !rem_rows && graphs_.serves_whole(n_full);
    const double us_prep = us_since(t_enter);
    if (!whole) {
        reset_state();
        graphs_.note(StepGraphs::kReset, 0);
    }
    const double us_fill = us_since(t_enter);
    if (whole) {
        graphs_.replay_whole(n_full);
        done = n_full;
    }
    // operator override: TAPER_DP_EAGER=1 keeps data-parallel steps out of hipGraphs (collectives launched eagerly)
    // (read behind a whole-call replay, as it always was: the call that first sees it may still be served by one)
    if (comm && env_is_1("TAPER_DP_EAGER")) graphs_.latch_off();
    if (!whole) {
        const std::vector<size_t> ladder = graphs_.ladder_to_record(chunk, n_full);
        if (!ladder.empty()) {
            // step 0 runs eagerly (pool warm-up, has_grad mask upload); then the SAME host code
            // is run under stream capture to record the op list of 1 step and of a chunk of
            // steps (one hipGraphLaunch per chunk amortises the ~10 us host cost of a replay)
            eager(bs, 1);
            done = 1;
            for (size_t steps : ladder)
                if (!capture(StepGraphs::Kind::Ladder, steps, [&] { steps_of(bs, steps); })) break;
        }
        const size_t tail = (n_full - done) % chunk;
        if (graphs_.wants_remainder(tail)) capture(StepGraphs::Kind::Remainder, tail, [&] { steps_of(bs, tail); });
        // ... a whole-call graph serves the very call that records it (a second reset in front of the steps changes nothing): a graph's
        // FIRST replay pays its upload, which must not fall into a later, timed call
        if (done == 0 && !rem_rows && graphs_.wants_whole(n_full) &&
            capture(StepGraphs::Kind::Whole, n_full, [&] { reset_state(); steps_of(bs, n_full); })) {
            graphs_.replay_whole(n_full);
            done = n_full;
        }
    }
    while (done < n_full) {
        const size_t steps = graphs_.replay_largest(n_full - done);
        if (!steps) eager(bs, 1);   // no graph fits (e.g. n_full == 1 on a later call): run the step eagerly
        done += steps ? steps : 1;
    }
    if (rem_rows) eager(rem_rows, 1);
    loader.advance(std::min(n, nb * bs));

    // ---- synchronise
    const double us_enqueued = us_since(t_enter);
    Device::sync();
    check_comm();
    if (trace_epoch()) fprintf(stderr, "taper trace: train_epoch_graph %zu steps (%s%s%s): state reset enqueued at %.1f - %.1f us, all enqueued after %.1f us, stream idle after %.1f us\n", nb,
                               step_form_names[(int)plan.form], rem_rows ? ", last batch " : "", rem_rows ? step_form_names[(int)rem_plan.form] : "", us_prep, us_fill, us_enqueued, us_since(t_enter));
    // ---- result: the log is host-visible (th_host_malloc); every step's entry has landed once the stream is idle
    return epoch_result(metrics_->d, nb, n_full, bs, rem_rows);
}

}  // namespace taper
