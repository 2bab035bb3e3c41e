// Looking at a trained model before choosing a quantization -- the observers of src/quantization/observers.rs on MI355X: train the
// 784-128-10 MLP for a few steps, then run calibration batches through it layer by layer, show every layer's output to a MinMax and a
// Histogram observer and every weight to the same pair, and print one line of statistics per observer.  The statistics stay on the
// device; only the printed numbers come back.  MNIST IDX files under --data-dir when present, synthetic rows otherwise; --steps bounds
// the training steps (default 20), --calib the calibration batches (default 4), --bins the histogram bins (default 64).
#include "common.h"

using namespace taper;

int main(int argc, char **argv) {
    size_t steps = 20, calib = 4, bins = 64;
    int kept = 1;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--steps") && i + 1 < argc) steps = strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--calib") && i + 1 < argc) calib = strtoul(argv[++i], nullptr, 10);
        else if (!strcmp(argv[i], "--bins") && i + 1 < argc) bins = strtoul(argv[++i], nullptr, 10);
        else argv[kept++] = argv[i];
    }
    ex::Args args = ex::parse(kept, argv);
    args.batch_size = args.batch_size == 256 ? 64 : args.batch_size;
    try {
        printf("Observer calibration example\n");
        MNISTDataset train_ds = ex::load(args, true);
        DataLoader loader(train_ds, args.batch_size, true);
        auto model = std::make_shared<Sequential>(std::vector<std::shared_ptr<Module>>{
            std::make_shared<Linear>(784, 128, true, 1), std::make_shared<ReLU>(), std::make_shared<Linear>(128, 10, true, 2)});
        auto optimizer = std::make_shared<Adam>(model->parameters(), 0.001f, 0.9f, 0.999f, 1e-8f, 0.0f);
        Trainer trainer(model, optimizer);
        const EpochResult tr = trainer.train_epoch_graph(loader, steps);
        printf("Trained %zu steps: loss %.4f, accuracy %.2f%%\n", tr.num_batches, tr.avg_loss, tr.accuracy * 100.f);

        ObserverManager observers;
        std::vector<std::string> names;
        auto add = [&](const std::string &name) {
            observers.add_minmax_observer(name);
            observers.add_histogram_observer(name, bins);
            names.push_back(name);
        };
        const char *layer_names[] = {"linear1.out", "relu.out", "linear2.out"};
        for (const char *n : layer_names) add(n);
        const char *param_names[] = {"linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias"};
        const std::vector<Tensor> params = model->parameters();
        for (size_t i = 0; i < params.size(); ++i) {
            add(param_names[i]);
            observers.observe_minmax(param_names[i], params[i]);
            observers.observe_histogram(param_names[i], params[i]);
        }

        // calibration: nothing below waits for the device until the statistics are asked for
        loader.reset();
        Tensor images, labels;
        size_t batches = 0;
        while (batches < calib && loader.next(&images, &labels)) {
            Tape::reset();
            Tensor x = images;
            for (size_t l = 0; l < model->layers.size(); ++l) {
                x = model->layers[l]->forward(x);
                observers.observe_minmax(layer_names[l], x);
                observers.observe_histogram(layer_names[l], x);
            }
            ++batches;
        }
        Tape::reset();
        printf("Calibrated on %zu batches of %zu\n\n", batches, args.batch_size);

        for (const std::string &n : names) {
            ObserverStats mm{};
            HistogramStats h{};
            if (!observers.get_minmax_stats(n, &mm) || !observers.get_histogram_stats(n, &h)) throw Error("observer " + n + " not found");
            printf("observer %-15s obs %zu  min %+.6f  max %+.6f  range %.6f  | %zu bins: count %llu  mean bin %.3f  fullest %llu\n", n.c_str(),
                   mm.num_observations, mm.global_min, mm.global_max, mm.range, bins, (unsigned long long)h.total_count, h.mean_bin,
                   (unsigned long long)h.max_bin_count);
        }
        printf("\nObservers: %zu names\n", observers.get_observer_names().size());
    } catch (const std::exception &e) {
        fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
