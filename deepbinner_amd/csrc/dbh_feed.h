// dbh_feed.h — a training-data set resident on the device and the kernel that assembles a batch
// from it (dbh_feed.hip; include/deepbinner_hip.h, "training: device-fed batches"; DESIGN.md
// section 19).  What dbh_trainer.hip needs of a data set: where its arrays lie, and the launch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dbh_feed {

// the layer numbers of dbh_train.h's hash that the feed uses (dropout has 1..7, the noise 0; the
// random signals of dbh_random_core.h take 11..14: kLayerSignal, kLayerSegment, kLayerDraw,
// kLayerGradient)
constexpr uint32_t kLayerChance = 8, kLayerKey = 9, kLayerOrder = 10;

struct View {
    int64_t n = 0;
    int input_size = 0, n_classes = 0;
    const int16_t* samples = nullptr;    // [n][input_size], as the file holds them
    const int32_t* labels = nullptr;     // [n]
    const double* mean = nullptr;        // [n]
    const double* std = nullptr;         // [n]: 0 for a constant window
};

// floor((1 - 1 / augmentation) * 2^24) in double; augmentation < 1 or not a number: false
bool augment_threshold(double augmentation, uint32_t* threshold);

// Queued on `stream`, nothing synchronised: slot w of x_dev [n_windows][input_size] and labels_dev
// takes sample indices_dev[w] (indices_dev null: sample first + w), normalised, and augmented where
// the slot's draw of `seed` lies under `threshold`.  An index outside [0, n) gives a window of NaN
// and the label -1.
hipError_t assemble(const View& ds, const int64_t* indices_dev, int64_t first, int64_t n_windows,
                    uint32_t threshold, uint64_t seed, float* x_dev, int32_t* labels_dev,
                    hipStream_t stream);

}  // namespace dbh_feed

const dbh_feed::View* dbh_dataset_view(const struct dbh_dataset* ds);
