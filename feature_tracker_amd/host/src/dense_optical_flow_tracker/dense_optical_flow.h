// dense_optical_flow.h — feature_tracker::DenseOpticalFlow with the reference's surface
// (src/dense_optical_flow_tracker/dense_optical_flow.h:12-65): Options, options(), both Track overloads and
// OpticalFlowMethodName().
//
// Where the work runs: every pixel of every level on the MI355X (ftk_dense_flow / ftk_dense_flow_level, include/ftk.h):
// the moment images, the per-pixel Gauss-Newton refinement and the 3x3 median are kernels; the flow planes come back as
// column-major Mat like the reference's.  The object keeps the Gaussian kernel's k2 / k4 / k22 between calls as the
// reference's does (a half patch of 0 does not recompute them, dense_optical_flow.cpp:95-98).
#ifndef _DENSE_OPTICAL_FLOW_TRACKER_H
#define _DENSE_OPTICAL_FLOW_TRACKER_H

#include <array>
#include <string>

#include "basic_type.h"
#include "datatype_image.h"
#include "datatype_image_pyramid.h"
#include "slam_basic_math.h"

namespace feature_tracker {

/* Class DenseOpticalFlow Declaration. */
class DenseOpticalFlow {

public:
    struct Options {
        int32_t kMaxIteration = 10;
        int32_t kHalfPatchSize = 2;
        float kMaxConvergeStep = 1e-6f;
        float kMaxDeltaFlowStep = 1.0f;
    };

public:
    DenseOpticalFlow() = default;
    virtual ~DenseOpticalFlow() = default;

    bool Track(const ImagePyramid &ref_pyramid, const ImagePyramid &cur_pyramid, std::array<Mat, 2> &flow_rc);
    bool Track(const GrayImage &ref_image, const GrayImage &cur_image, std::array<Mat, 2> &flow_rc);

    std::string OpticalFlowMethodName() const { return "Gunnar Farneback"; }

    // Reference for parameters.
    Options &options() { return options_; }
    // Const reference for parameters.
    const Options &options() const { return options_; }

    // Not in the reference: text of the last failure (no device, ...).
    const std::string &last_error() const { return last_error_; }

private:
    void FillOptions(void *native) const;
    void RememberKernelMoments();

private:
    Options options_;
    // the reference object's gaussian_kernel_.k2 / k4 / k22 (dense_optical_flow.h:45-50)
    float k_moments_[3] = {0.0f, 0.0f, 0.0f};
    std::string last_error_;
};

}  // namespace feature_tracker

#endif  // end of _DENSE_OPTICAL_FLOW_TRACKER_H
