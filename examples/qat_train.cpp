// Quantization-aware training on MI355X -- counterpart of the reference's examples/qat_example.rs: train the reference CNN
// (train_mnist_cnn.rs:35-100; --model mlp: 784-128-64-10) with int8 fake quantization of weights and activations (QATConv2d / QATLinear,
// Adam(1e-3), batch 64), evaluate it with training mode off, then quantize() it to int8 and print the QAT model's accuracy, the packed
// model's accuracy and both sizes.  MNIST IDX files under --data-dir when present, synthetic rows otherwise; --steps bounds the training
// steps (default: the reference's five epochs).
#include <chrono>

#include "common.h"

using namespace taper;

static size_t storage_bytes(const QuantizedModule &q) {
    std::vector<const QTensor *> ts;
    q.tensors(&ts);
    size_t s = 0;
    for (const QTensor *t : ts) s += t->storage_bytes();
    return s;
}

template <class F>
static float evaluate(DataLoader &loader, const Shape &sample, F forward) {
    size_t correct = 0, total = 0;
    loader.reset();
    Tensor images, labels;
    while (loader.next(&images, &labels)) {
        Tape::reset();
        const size_t b = images.shape()[0];
        Shape s{b};
        s.insert(s.end(), sample.begin(), sample.end());
        const Tensor logits = forward(sample.empty() ? images : images.reshape(s));
        correct += (size_t)(accuracy(logits, labels) * (float)b);
        total += b;
    }
    Tape::reset();
    return total ? (float)correct / (float)total : 0.f;
}

int main(int argc, char **argv) {
    size_t steps = 0;
    bool mlp = false;
    bool batch_given = false;
    int kept = 1;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--batch-size")) batch_given = true;
        if (!strcmp(argv[i], "--steps") && i + 1 < argc) steps = strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--model") && i + 1 < argc) mlp = !strcmp(argv[++i], "mlp");
        else argv[kept++] = argv[i];
    }
    ex::Args args = ex::parse(kept, argv);
    if (args.epochs == 0) args.epochs = 5;                               // qat_example.rs: `for epoch in 1..=5`
    if (!batch_given) args.batch_size = 64;                             // qat_example.rs: DataLoader::new(.., 64, ..)
    try {
        printf("Quantization-Aware Training (QAT) Example\nThis example demonstrates QAT training and deployment.\n\n");
        MNISTDataset train_ds = ex::load(args, true), test_ds = ex::load(args, false);
        printf("Training set: %zu samples\nTest set: %zu samples\n\n", train_ds.len(), test_ds.len());
        DataLoader train_loader(train_ds, args.batch_size, true), test_loader(test_ds, args.batch_size, false);

        QATConfig cfg;   // int8, symmetric, per tensor, activations fake-quantized too
        printf("QAT Configuration:\n  Quantization Type: Int8\n  Per-Channel: false\n  Symmetric: true\n  Activations: true\n\n");
        std::shared_ptr<Sequential> model;
        Shape sample;
        if (mlp) {
            printf("Building QAT-aware MLP model...\n");
            model = std::make_shared<Sequential>(std::vector<std::shared_ptr<Module>>{
                std::make_shared<QATLinear>(784, 128, true, cfg, "fc1", 1), std::make_shared<ReLU>(),
                std::make_shared<QATLinear>(128, 64, true, cfg, "fc2", 2), std::make_shared<ReLU>(),
                std::make_shared<QATLinear>(64, 10, true, cfg, "fc3", 3)});
        } else {
            printf("Building QAT-aware CNN model...\n");
            auto conv = [&](size_t ci, size_t co, const char *id, uint64_t seed) {
                return std::make_shared<QATConv2d>(ci, co, std::make_pair(3, 3), std::make_pair(1, 1), std::make_pair(1, 1), true, true, cfg, id, seed);
            };
            auto pool = [] { return std::make_shared<MaxPool2d>(std::make_pair(2, 2), std::make_pair(2, 2), std::make_pair(0, 0)); };
            model = std::make_shared<Sequential>(std::vector<std::shared_ptr<Module>>{
                conv(1, 32, "conv1", 1), conv(32, 32, "conv2", 2), pool(), conv(32, 64, "conv3", 3), conv(64, 64, "conv4", 4), pool(),
                conv(64, 128, "conv5", 5), std::make_shared<AdaptiveAvgPool2d>(std::make_pair(1, 1)), std::make_shared<Flatten>(1),
                std::make_shared<QATLinear>(128, 128, true, cfg, "fc1", 6), std::make_shared<ReLU>(),
                std::make_shared<QATLinear>(128, 64, true, cfg, "fc2", 7), std::make_shared<ReLU>(),
                std::make_shared<QATLinear>(64, 10, true, cfg, "fc3", 8)});
            sample = {1, 28, 28};
        }
        size_t n_params = 0;
        for (const Tensor &p : model->parameters()) n_params += p.len();
        printf("Total parameters: %zu\n", n_params);
        auto optimizer = std::make_shared<Adam>(model->parameters(), 0.001f);
        Trainer trainer(model, optimizer);
        trainer.sample_shape = sample;

        qat::enable();   // qat_example.rs: global::enable_qat(); global::set_training_mode(true)
        qat::set_training_mode(true);
        const qat::Status st = qat::status();
        printf("QAT Status: enabled=%s training=%s\n", st.global_enabled ? "true" : "false", st.training_mode ? "true" : "false");

        const std::string rule(60, '=');
        printf("\n%s\n\nStep 1: QAT training...\n", rule.c_str());
        size_t left = steps;
        for (size_t epoch = 1; epoch <= args.epochs && (steps == 0 || left > 0); ++epoch) {
            const auto t0 = std::chrono::steady_clock::now();
            qat::set_training_mode(true);
            const EpochResult tr = trainer.train_epoch_graph(train_loader, steps ? left : 0);
            if (steps) left -= std::min(left, tr.num_batches);
            qat::set_training_mode(false);   // evaluation: the plain f32 forward
            const float val = evaluate(test_loader, sample, [&](const Tensor &x) { return model->forward(x); });
            const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            printf("Epoch %zu complete:\n   Train Loss: %.4f | Train Acc: %.2f%%\n   Val Acc: %.2f%% | Time: %.2fs\n\n", epoch, tr.avg_loss,
                   tr.accuracy * 100.f, val * 100.f, secs);
        }

        printf("%s\n\nStep 2: Evaluating the QAT model (training mode off)...\n", rule.c_str());
        qat::set_training_mode(false);
        const float acc_qat = evaluate(test_loader, sample, [&](const Tensor &x) { return model->forward(x); });
        printf("QAT model accuracy (eval): %.2f%%\n", acc_qat * 100.f);

        printf("\n%s\n\nStep 3: Deploying: quantize(Int8)...\n", rule.c_str());
        auto q8 = quantize(*model, QType::Int8, true);
        const float acc8 = evaluate(test_loader, sample, [&](const Tensor &x) { return q8->forward(x); });
        printf("Int8 model accuracy: %.2f%%\n", acc8 * 100.f);
        const size_t size32 = n_params * 4, size8 = storage_bytes(*q8);
        printf("\n%s\n\nQAT Summary:\n", rule.c_str());
        printf("Float32 size: %zu bytes\n", size32);
        printf("Int8 size: %zu bytes (%.2fx smaller), accuracy change %.2f points\n", size8, (double)size32 / size8, (acc8 - acc_qat) * 100.f);
        printf("QAT Complete!\n");
        qat::disable();
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
