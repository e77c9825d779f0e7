// nn_feature_matcher.cpp — NNFeatureMatcher over the C ABI: the caller's network through the SetInference seam, then the reference's
// post-processing (src/nn_feature_matcher/nn_feature_matcher.cpp:155-216) on the device.
#include "nn_feature_matcher.h"

#include <string>

#include "device_runtime.h"
#include "ftk.h"
#include "slam_log_reporter.h"
#include "slam_operations.h"

namespace feature_tracker {

NNFeatureMatcher::NNFeatureMatcher() { device::WarmUp(FTK_WARM_COSINE); }

bool NNFeatureMatcher::Initialize() {
    device::WarmUp(FTK_WARM_COSINE);
    return true;
}

template bool NNFeatureMatcher::Match<SuperpointDescriptorType>(const std::vector<SuperpointDescriptorType> &descriptors_ref,
                                                                const std::vector<SuperpointDescriptorType> &descriptors_cur,
                                                                const std::vector<Vec2> &pixel_uv_ref, const std::vector<Vec2> &pixel_uv_cur,
                                                                std::vector<Vec2> &matched_pixel_uv_cur, std::vector<uint8_t> &status);
template bool NNFeatureMatcher::Match<DiskDescriptorType>(const std::vector<DiskDescriptorType> &descriptors_ref,
                                                          const std::vector<DiskDescriptorType> &descriptors_cur, const std::vector<Vec2> &pixel_uv_ref,
                                                          const std::vector<Vec2> &pixel_uv_cur, std::vector<Vec2> &matched_pixel_uv_cur,
                                                          std::vector<uint8_t> &status);
template <typename NNFeatureDescriptorType>
bool NNFeatureMatcher::Match(const std::vector<NNFeatureDescriptorType> &descriptors_ref, const std::vector<NNFeatureDescriptorType> &descriptors_cur,
                             const std::vector<Vec2> &pixel_uv_ref, const std::vector<Vec2> &pixel_uv_cur, std::vector<Vec2> &matched_pixel_uv_cur,
                             std::vector<uint8_t> &status) {
    // the reference's InferenceSession checks (:92-94); no inference function stands for its null session
    RETURN_FALSE_IF(descriptors_ref.empty());
    RETURN_FALSE_IF(descriptors_cur.size() != pixel_uv_cur.size() || descriptors_ref.size() != pixel_uv_ref.size());
    RETURN_FALSE_IF(!inference_);
    static_assert(sizeof(NNFeatureDescriptorType) % sizeof(float) == 0, "descriptors are plain float vectors");
    InferenceOutput output;
    RETURN_FALSE_IF(!inference_(options_.kModelType, reinterpret_cast<const float *>(descriptors_ref.data()), static_cast<int32_t>(descriptors_ref.size()),
                                descriptors_cur.empty() ? nullptr : reinterpret_cast<const float *>(descriptors_cur.data()),
                                static_cast<int32_t>(descriptors_cur.size()), static_cast<int32_t>(sizeof(NNFeatureDescriptorType) / sizeof(float)),
                                pixel_uv_ref, pixel_uv_cur, output));
    return PostProcess(output, pixel_uv_ref, pixel_uv_cur, matched_pixel_uv_cur, status);
}

bool NNFeatureMatcher::PostProcess(const InferenceOutput &output, const std::vector<Vec2> &pixel_uv_ref, const std::vector<Vec2> &pixel_uv_cur,
                                   std::vector<Vec2> &matched_pixel_uv_cur, std::vector<uint8_t> &status) {
    std::string error;
    ftk_context *ctx = device::SharedContext(&error);
    if (ctx == nullptr) {
        ReportError("[NNFeatureMatcher] " << error);
        return false;
    }
    const int32_t n_ref = static_cast<int32_t>(pixel_uv_ref.size()), n_cur = static_cast<int32_t>(pixel_uv_cur.size());
    status.assign(pixel_uv_ref.size(), static_cast<uint8_t>(TrackStatus::kLargeResidual));  // :156
    matched_pixel_uv_cur = pixel_uv_cur;                                                    // :157
    match_index_.assign(pixel_uv_ref.size(), -1);
    int ok = 0;
    const int rc = output.is_match_list
                       ? ftk_nn_match_list(ctx, output.matches, output.n_matches, n_ref, n_cur, match_index_.data(), status.data(), &ok)
                       : ftk_nn_match_scores(ctx, output.scores, 1, n_ref, n_cur, output.row_stride, 0, options_.kMinValidMatchScore, match_index_.data(),
                                             status.data(), &ok);
    if (rc != FTK_OK) {
        ReportError("[NNFeatureMatcher] " << ftk_last_error(ctx));
        return false;
    }
    RETURN_FALSE_IF(!ok);
    // :171 / :213 — a matched row beyond the n_cur entries of matched_pixel_uv_cur keeps its status and writes no pixel
    for (int32_t i = 0; i < n_ref && i < n_cur; ++i) {
        const int32_t j = match_index_[i];
        if (j >= 0 && j < n_cur) {
            matched_pixel_uv_cur[i] = pixel_uv_cur[j];
        }
    }
    return true;
}

}  // namespace feature_tracker
