// dense_optical_flow.cpp — marshals DenseOpticalFlow::Track into the C ABI.  Replaces the reference's per-pixel loops
// (dense_optical_flow.cpp:7-85) with the device entries; the planes are converted between the ABI's row-major layout and Mat's
// column-major one here.
#include "dense_optical_flow.h"

#include <vector>

#include "device_runtime.h"
#include "ftk.h"
#include "slam_log_reporter.h"
#include "slam_operations.h"

namespace feature_tracker {

namespace {

void ToRowMajor(const Mat &m, std::vector<float> &out) {
    out.resize(static_cast<size_t>(m.rows()) * m.cols());
    for (int32_t r = 0; r < m.rows(); ++r) {
        for (int32_t c = 0; c < m.cols(); ++c) {
            out[static_cast<size_t>(r) * m.cols() + c] = m(r, c);
        }
    }
}

void FromRowMajor(const std::vector<float> &in, int32_t rows, int32_t cols, Mat &m) {
    m.resize(rows, cols);
    for (int32_t r = 0; r < rows; ++r) {
        for (int32_t c = 0; c < cols; ++c) {
            m(r, c) = in[static_cast<size_t>(r) * cols + c];
        }
    }
}

}  // namespace

void DenseOpticalFlow::FillOptions(void *native) const {
    ftk_dense_flow_options &opt = *static_cast<ftk_dense_flow_options *>(native);
    ftk_default_dense_flow_options(&opt);
    opt.max_iteration = options_.kMaxIteration;
    opt.half_patch = options_.kHalfPatchSize;
    opt.max_converge_step = options_.kMaxConvergeStep;
    opt.max_delta_flow_step = options_.kMaxDeltaFlowStep;
    for (int i = 0; i < 3; ++i) {
        opt.k_moments[i] = k_moments_[i];
    }
}

// InitializeGaussianKernel's k2 / k4 / k22 as the object keeps them (recomputed for a half patch > 0, :119-131)
void DenseOpticalFlow::RememberKernelMoments() {
    if (options_.kHalfPatchSize > 0) {
        (void)ftk_dense_flow_gaussian(options_.kHalfPatchSize, nullptr, k_moments_);
    }
}

bool DenseOpticalFlow::Track(const GrayImage &ref_image, const GrayImage &cur_image, std::array<Mat, 2> &flow_rc) {
    RETURN_FALSE_IF(ref_image.data() == nullptr);  // :9-10
    RETURN_FALSE_IF(cur_image.data() == nullptr);
    RETURN_FALSE_IF(options_.kHalfPatchSize < 0);  // :12 InitializeGaussianKernel
    last_error_.clear();
    ftk_context *ctx = device::SharedContext(&last_error_);
    if (ctx == nullptr) {
        ReportError("[DenseOpticalFlow] " << last_error_);
        return false;
    }
    const ftk_image ref_level = {ref_image.data(), ref_image.rows(), ref_image.cols()};
    const ftk_image cur_level = {cur_image.data(), cur_image.rows(), cur_image.cols()};
    ftk_pyramid *ref_dev = nullptr, *cur_dev = nullptr;
    int rc = ftk_pyramid_upload(ctx, &ref_level, 1, &ref_dev);
    if (rc == FTK_OK) {
        rc = ftk_pyramid_upload(ctx, &cur_level, 1, &cur_dev);
    }
    // :18-23: each plane is the initial guess when it is ref-sized, otherwise reset to zero
    std::vector<float> planes[2];
    int32_t valid = 0;
    for (int k = 0; k < 2; ++k) {
        if (flow_rc[k].rows() == ref_image.rows() && flow_rc[k].cols() == ref_image.cols()) {
            ToRowMajor(flow_rc[k], planes[k]);
            valid |= 1 << k;
        } else {
            planes[k].assign(static_cast<size_t>(ref_image.rows()) * ref_image.cols(), 0.0f);
        }
    }
    if (rc == FTK_OK) {
        ftk_dense_flow_options opt;
        FillOptions(&opt);
        rc = ftk_dense_flow_level(ctx, &opt, ref_dev, cur_dev, 0, planes[0].data(), planes[1].data(), valid);
    }
    if (rc != FTK_OK) {
        last_error_ = ftk_last_error(ctx);
    }
    ftk_pyramid_destroy(ref_dev);
    ftk_pyramid_destroy(cur_dev);
    if (rc != FTK_OK) {
        ReportError("[DenseOpticalFlow] " << last_error_);
        return false;
    }
    RememberKernelMoments();
    FromRowMajor(planes[0], ref_image.rows(), ref_image.cols(), flow_rc[0]);
    FromRowMajor(planes[1], ref_image.rows(), ref_image.cols(), flow_rc[1]);
    return true;
}

bool DenseOpticalFlow::Track(const ImagePyramid &ref_pyramid, const ImagePyramid &cur_pyramid, std::array<Mat, 2> &flow_rc) {
    RETURN_FALSE_IF(ref_pyramid.data() == nullptr);  // :37-39
    RETURN_FALSE_IF(cur_pyramid.data() == nullptr);
    RETURN_FALSE_IF(ref_pyramid.level() != cur_pyramid.level());
    RETURN_FALSE_IF(ref_pyramid.level() == 0);
    last_error_.clear();
    ftk_context *ctx = device::SharedContext(&last_error_);
    if (ctx == nullptr) {
        ReportError("[DenseOpticalFlow] " << last_error_);
        return false;
    }
    ftk_pyramid *ref_dev = device::PyramidTwin(ctx, ref_pyramid, &last_error_);
    ftk_pyramid *cur_dev = ref_dev ? device::PyramidTwin(ctx, cur_pyramid, &last_error_) : nullptr;
    if (ref_dev == nullptr || cur_dev == nullptr) {
        ReportError("[DenseOpticalFlow] " << last_error_);
        return false;
    }
    ftk_image level0;
    (void)ftk_pyramid_level(ref_dev, 0, &level0);
    std::vector<float> planes[2];
    planes[0].resize(static_cast<size_t>(level0.rows) * level0.cols);
    planes[1].resize(planes[0].size());
    ftk_dense_flow_options opt;
    FillOptions(&opt);
    const int rc = ftk_dense_flow(ctx, &opt, ref_dev, cur_dev, planes[0].data(), planes[1].data());
    if (rc != FTK_OK) {
        last_error_ = ftk_last_error(ctx);
        ReportError("[DenseOpticalFlow] " << last_error_);
        return false;
    }
    RememberKernelMoments();
    FromRowMajor(planes[0], level0.rows, level0.cols, flow_rc[0]);
    FromRowMajor(planes[1], level0.rows, level0.cols, flow_rc[1]);
    return true;
}

}  // namespace feature_tracker
