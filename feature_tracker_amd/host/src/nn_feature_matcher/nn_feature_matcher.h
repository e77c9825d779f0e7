// nn_feature_matcher.h — feature_tracker::NNFeatureMatcher with the reference's class shape (src/nn_feature_matcher/nn_feature_matcher.h:
// Options, ModelType, options(), Initialize, the Match template and its two instantiations) and ONE difference: the onnxruntime
// members (session, tensors, names) are replaced by a seam, SetInference, through which the caller supplies the network with whatever
// runtime it has.  Everything Match does after the network (nn_feature_matcher.cpp:155-216) runs on the device through the C ABI
// (ftk_nn_match_*).  The LightGlue network and its .onnx files are not part of this project.
#ifndef _NN_FEATURE_MATCHER_H_
#define _NN_FEATURE_MATCHER_H_

#include <cstdint>
#include <functional>
#include <vector>

#include "basic_type.h"
#include "feature_tracker.h"
#include "nn_feature_point_detector.h"

namespace feature_tracker {

using feature_detector::DiskDescriptorType;
using feature_detector::SuperpointDescriptorType;

/* Class NNFeatureMatcher Declaration. */
class NNFeatureMatcher {

public:
    enum class ModelType : uint8_t {
        kLightglueForSuperpointScoreMat = 0,
        kLightglueForSuperpointMatches = 1,
        kLightglueForDiskScoreMat = 2,
        kLightglueForDiskMatches = 3,
    };

    struct Options {
        int32_t kMaxNumberOfMatches = 300;  // sizes the reference's warm-up inference only (:57-70): carried for source compatibility, unused
        float kMinValidMatchScore = -3.0f;
        ModelType kModelType = ModelType::kLightglueForSuperpointScoreMat;
    };

    // What the network returned: a score matrix (the reference's one-output models) or a match list (its two-output models), in host
    // memory that stays valid until Match returns.  (A caller whose network leaves its output in device memory calls the device
    // entries of include/ftk.h itself — ftk_nn_match_scores_device / _list_device / ftk_nn_fill_pixels_device on its own stream and
    // buffers: this host layer owns no device allocator.)
    struct InferenceOutput {
        bool is_match_list = false;
        // score matrix: scores(i, j) at scores[i * row_stride + j], i < n_ref, j < n_cur (row_stride >= n_cur: LightGlue's tensor
        // with its dustbin row and column is passed as it is, with row_stride = n_cur + 1)
        const float *scores = nullptr;
        int64_t row_stride = 0;
        // match list: n_matches rows of (idx_ref, idx_cur)
        const int64_t *matches = nullptr;
        int32_t n_matches = 0;
    };
    // descriptors: n x dim floats, row-major (the vectors' own storage).  Returns false when the inference failed.
    using InferenceFunction = std::function<bool(ModelType model, const float *descriptors_ref, int32_t n_ref, const float *descriptors_cur, int32_t n_cur,
                                                 int32_t dim, const std::vector<Vec2> &pixel_uv_ref, const std::vector<Vec2> &pixel_uv_cur,
                                                 InferenceOutput &output)>;

public:
    NNFeatureMatcher();
    virtual ~NNFeatureMatcher() = default;

    // The reference loads its model here; this class has none to load: it warms the device kernels up and returns true.
    bool Initialize();
    // The network.  Without one Match returns false, as the reference does without a session (:94).
    void SetInference(InferenceFunction inference) { inference_ = std::move(inference); }
    template <typename NNFeatureDescriptorType>
    bool Match(const std::vector<NNFeatureDescriptorType> &descriptors_ref, const std::vector<NNFeatureDescriptorType> &descriptors_cur,
               const std::vector<Vec2> &pixel_uv_ref, const std::vector<Vec2> &pixel_uv_cur, std::vector<Vec2> &matched_pixel_uv_cur,
               std::vector<uint8_t> &status);

    // Reference for member variables.
    Options &options() { return options_; }
    // Const reference for member variables.
    const Options &options() const { return options_; }

private:
    bool PostProcess(const InferenceOutput &output, const std::vector<Vec2> &pixel_uv_ref, const std::vector<Vec2> &pixel_uv_cur,
                     std::vector<Vec2> &matched_pixel_uv_cur, std::vector<uint8_t> &status);

private:
    Options options_;
    InferenceFunction inference_;
    std::vector<int32_t> match_index_;
};

}  // namespace feature_tracker

#endif  // end of _NN_FEATURE_MATCHER_H_
