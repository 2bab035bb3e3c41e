// Post-training quantization on MI355X -- counterpart of the reference's examples/ptq_quantize.rs: train the reference CNN
// (train_mnist_cnn.rs:35-100; Adam(1e-2, wd 1e-4), batch 64), quantize it to Int8 and to Float16 (Module::quantize), evaluate all
// three on the test set and print sizes, compression ratios and accuracy drops.  MNIST IDX files under --data-dir when present,
// synthetic rows otherwise; --steps bounds the training steps (default: two epochs, as the reference's loop runs).
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

// test accuracy of `forward` over the loader (the reference's per-batch truncation of acc * batch, ptq_quantize.rs)
template <class F>
static float evaluate(DataLoader &loader, F forward) {
    size_t correct = 0, total = 0;
    loader.reset();
    Tensor images, labels;
    while (loader.next(&images, &labels)) {
        Tape::reset();
        const size_t b = images.shape()[0];
        const Tensor logits = forward(images.reshape({b, 1, 28, 28}));
        correct += (size_t)(accuracy(logits, labels) * (float)b);
        total += b;
    }
    Tape::reset();
    return total ? (float)correct / (float)total : 0.f;
}

int main(int argc, char **argv) {
    size_t steps = 0;
    int kept = 1;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--steps") && i + 1 < argc) steps = strtoul(argv[++i], nullptr, 10);
        else argv[kept++] = argv[i];
    }
    ex::Args args = ex::parse(kept, argv);
    if (args.epochs == 0) args.epochs = 2;   // ptq_quantize.rs: `for epoch in 1..=2`
    args.batch_size = args.batch_size == 256 ? 64 : args.batch_size;   // ptq_quantize.rs: DataLoader::new(.., 64, ..)
    try {
        printf("Model Quantization Example\nThis example shows how to train a model and then quantize it for inference.\n\n");
        MNISTDataset train_ds = ex::load(args, true), test_ds = ex::load(args, false);
        printf("Training set: %zu samples\nTest set: %zu samples\n\n", train_ds.len(), test_ds.len());
        DataLoader train_loader(train_ds, args.batch_size, true), test_loader(test_ds, args.batch_size, false);

        printf("Building CNN model...\n");
        auto conv = [](size_t ci, size_t co, uint64_t seed) {
            return std::make_shared<Conv2dReLU>(ci, co, std::make_pair(3, 3), std::make_pair(1, 1), std::make_pair(1, 1), true, seed);
        };
        auto pool = [] { return std::make_shared<MaxPool2d>(std::make_pair(2, 2), std::make_pair(2, 2), std::make_pair(0, 0)); };
        auto model = std::make_shared<Sequential>(std::vector<std::shared_ptr<Module>>{
            conv(1, 32, 1), conv(32, 32, 2), pool(), conv(32, 64, 3), conv(64, 64, 4), pool(), conv(64, 128, 5),
            std::make_shared<AdaptiveAvgPool2d>(std::make_pair(1, 1)), std::make_shared<Flatten>(1),
            std::make_shared<Linear>(128, 128, true, 6), std::make_shared<ReLU>(),
            std::make_shared<Linear>(128, 64, true, 7), std::make_shared<ReLU>(), std::make_shared<Linear>(64, 10, true, 8)});
        size_t n_params = 0;
        for (const Tensor &p : model->parameters()) n_params += p.len();
        printf("Total parameters: %zu\n", n_params);
        auto optimizer = std::make_shared<Adam>(model->parameters(), 0.01f, 0.9f, 0.999f, 1e-8f, 0.0001f);
        Trainer trainer(model, optimizer);
        trainer.sample_shape = {1, 28, 28};

        const std::string rule(60, '=');
        printf("\n%s\n\nStep 1: Training the model...\n", rule.c_str());
        size_t left = steps;
        for (size_t epoch = 1; epoch <= args.epochs && (steps == 0 || left > 0); ++epoch) {
            const auto t0 = std::chrono::steady_clock::now();
            const EpochResult tr = trainer.train_epoch_graph(train_loader, steps ? left : 0);
            if (steps) left -= std::min(left, tr.num_batches);
            const float val = evaluate(test_loader, [&](const Tensor &x) { return model->forward(x); });
            const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            printf("Epoch %zu complete:\n   Train Loss: %.4f | Train Acc: %.2f%%\n   Val Acc: %.2f%% | Time: %.2fs\n\n", epoch, tr.avg_loss,
                   tr.accuracy * 100.f, val * 100.f, secs);
        }

        printf("%s\n\nStep 2: Quantizing the trained model...\n", rule.c_str());
        auto t0 = std::chrono::steady_clock::now();
        auto q8 = quantize(*model, QType::Int8, true);
        Device::sync();
        printf("Int8 quantization completed in %.2fms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        t0 = std::chrono::steady_clock::now();
        auto q16 = quantize(*model, QType::Float16, true);
        Device::sync();
        printf("Float16 quantization completed in %.2fms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());

        printf("\n%s\n\nStep 3: Testing quantized models on the full test set...\n", rule.c_str());
        const float acc32 = evaluate(test_loader, [&](const Tensor &x) { return model->forward(x); });
        const float acc8 = evaluate(test_loader, [&](const Tensor &x) { return q8->forward(x); });
        const float acc16 = evaluate(test_loader, [&](const Tensor &x) { return q16->forward(x); });
        printf("Original model accuracy: %.2f%%\nInt8 model accuracy: %.2f%%\nFloat16 model accuracy: %.2f%%\n", acc32 * 100.f, acc8 * 100.f,
               acc16 * 100.f);

        const size_t size32 = n_params * 4, size8 = storage_bytes(*q8), size16 = storage_bytes(*q16);
        printf("\n%s\n\nQuantization Summary:\n", rule.c_str());
        printf("Original size: %zu bytes\n", size32);
        printf("Int8 size: %zu bytes (%.2fx smaller), accuracy drop %.2f points\n", size8, (double)size32 / size8, (acc32 - acc8) * 100.f);
        printf("Float16 size: %zu bytes (%.2fx smaller), accuracy drop %.2f points\n", size16, (double)size32 / size16, (acc32 - acc16) * 100.f);
        printf("Quantization Complete!\n");
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
