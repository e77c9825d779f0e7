// dense_flow_cli — what the reference's test/test_dense_optical_flow.cpp does, headless: load an image pair, build 5-level
// pyramids, DenseOpticalFlow with kHalfPatchSize = 2 and kMaxIteration = 20, Track; print the call time and write both
// flow planes (row-major float32, rows x cols of the ref image) instead of drawing them.
//   dense_flow_cli <ref.png|pgm> <cur.png|pgm> <flow_r.f32> <flow_c.f32>
#include <cstdio>
#include <string>
#include <vector>

#include "dense_optical_flow.h"
#include "slam_log_reporter.h"
#include "slam_memory.h"
#include "tick_tock.h"
#include "visualizor_2d.h"

using namespace slam_visualizor;

static bool WritePlane(const std::string &path, const Mat &m) {
    std::vector<float> row_major(static_cast<size_t>(m.rows()) * m.cols());
    for (int32_t r = 0; r < m.rows(); ++r) {
        for (int32_t c = 0; c < m.cols(); ++c) {
            row_major[static_cast<size_t>(r) * m.cols() + c] = m(r, c);
        }
    }
    FILE *f = std::fopen(path.c_str(), "wb");
    if (f == nullptr) {
        return false;
    }
    const size_t n = std::fwrite(row_major.data(), sizeof(float), row_major.size(), f);
    std::fclose(f);
    return n == row_major.size();
}

int main(int argc, char **argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: dense_flow_cli ref cur flow_r.f32 flow_c.f32\n");
        return 2;
    }
    GrayImage ref_image, cur_image;
    if (!Visualizor2D::LoadImage(argv[1], ref_image) || !Visualizor2D::LoadImage(argv[2], cur_image)) {
        std::fprintf(stderr, "cannot load the images\n");
        return 2;
    }
    ImagePyramid ref_pyramid, cur_pyramid;
    ref_pyramid.SetPyramidBuff((uint8_t *)SlamMemory::Malloc(sizeof(uint8_t) * ref_image.rows() * ref_image.cols()), true);
    cur_pyramid.SetPyramidBuff((uint8_t *)SlamMemory::Malloc(sizeof(uint8_t) * cur_image.rows() * cur_image.cols()), true);
    ref_pyramid.SetRawImage(ref_image.data(), ref_image.rows(), ref_image.cols());
    cur_pyramid.SetRawImage(cur_image.data(), cur_image.rows(), cur_image.cols());
    ref_pyramid.CreateImagePyramid(5);
    cur_pyramid.CreateImagePyramid(5);

    feature_tracker::DenseOpticalFlow solver;
    solver.options().kHalfPatchSize = 2;
    solver.options().kMaxIteration = 20;
    std::array<Mat, 2> flow_rc;
    TickTock timer;
    const bool ok = solver.Track(ref_pyramid, cur_pyramid, flow_rc);
    const float ms = timer.TockTickInMillisecond();
    std::printf("%s ok %d, %d x %d flow, %.3f ms\n", solver.OpticalFlowMethodName().c_str(), ok ? 1 : 0, flow_rc[0].rows(), flow_rc[0].cols(), ms);
    if (!ok) {
        std::printf("error: %s\n", solver.last_error().c_str());
        return 1;
    }
    if (!WritePlane(argv[3], flow_rc[0]) || !WritePlane(argv[4], flow_rc[1])) {
        std::fprintf(stderr, "cannot write the flow planes\n");
        return 2;
    }
    return 0;
}
