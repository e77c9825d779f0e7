// nn_match_cli — drives feature_tracker::NNFeatureMatcher with a stand-in for the network: the "inference" hands back a score matrix
// (or a match list) read from a file, which is how a caller wires its own runtime into the SetInference seam.
//
//   nn_match_cli scores <n_ref> <n_cur> <row_stride> <min_score as 8 hex digits> <scores.f32>   raw float32, (n_ref - 1) * row_stride + n_cur values
//   nn_match_cli list   <n_ref> <n_cur> <n_matches> <matches.i64>                               raw int64, 2 * n_matches values
//   nn_match_cli none   <n_ref> <n_cur>                                                         no inference function set
//
// cur pixel j is (j + 0.25, 1000 - j); output: "ok <0|1>", then per reference row "status" and per entry of matched_pixel_uv_cur
// "u_bits v_bits".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "nn_feature_matcher.h"

template <class T>
static std::vector<T> ReadRaw(const char *path, size_t count) {
    std::vector<T> v(count);
    std::ifstream in(path, std::ios::binary);
    in.read(reinterpret_cast<char *>(v.data()), static_cast<std::streamsize>(sizeof(T) * count));
    if (static_cast<size_t>(in.gcount()) != sizeof(T) * count) {
        std::fprintf(stderr, "nn_match_cli: %s holds fewer than %zu values\n", path, count);
        std::exit(2);
    }
    return v;
}

int main(int argc, char **argv) {
    if (argc < 4) {
        return 2;
    }
    using feature_tracker::NNFeatureMatcher;
    const std::string mode = argv[1];
    const int32_t n_ref = std::atoi(argv[2]), n_cur = std::atoi(argv[3]);
    NNFeatureMatcher matcher;
    matcher.Initialize();
    std::vector<float> scores;
    std::vector<int64_t> matches;
    if (mode == "scores" && argc >= 7) {
        const int64_t row_stride = std::atoll(argv[4]);
        const uint32_t bits = static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 16));
        std::memcpy(&matcher.options().kMinValidMatchScore, &bits, 4);
        scores = ReadRaw<float>(argv[6], n_ref > 0 ? static_cast<size_t>((n_ref - 1) * row_stride + n_cur) : 0);
        matcher.SetInference([&scores, row_stride](NNFeatureMatcher::ModelType, const float *, int32_t, const float *, int32_t, int32_t, const std::vector<Vec2> &,
                                                   const std::vector<Vec2> &, NNFeatureMatcher::InferenceOutput &out) {
            out.scores = scores.data();
            out.row_stride = row_stride;
            return true;
        });
    } else if (mode == "list" && argc >= 6) {
        const int32_t n_matches = std::atoi(argv[4]);
        matches = ReadRaw<int64_t>(argv[5], 2 * static_cast<size_t>(n_matches));
        matcher.options().kModelType = NNFeatureMatcher::ModelType::kLightglueForSuperpointMatches;
        matcher.SetInference([&matches, n_matches](NNFeatureMatcher::ModelType, const float *, int32_t, const float *, int32_t, int32_t, const std::vector<Vec2> &,
                                                   const std::vector<Vec2> &, NNFeatureMatcher::InferenceOutput &out) {
            out.is_match_list = true;
            out.matches = matches.data();
            out.n_matches = n_matches;
            return true;
        });
    } else if (mode != "none") {
        return 2;
    }
    std::vector<feature_tracker::SuperpointDescriptorType> ref(n_ref), cur(n_cur);
    std::vector<Vec2> ref_uv(n_ref), cur_uv(n_cur), matched;
    for (int32_t j = 0; j < n_cur; ++j) {
        cur_uv[j] = Vec2(j + 0.25f, 1000.0f - j);
    }
    std::vector<uint8_t> status;
    const bool ok = matcher.Match(ref, cur, ref_uv, cur_uv, matched, status);
    std::printf("ok %d\n", ok ? 1 : 0);
    if (ok) {
        for (size_t i = 0; i < status.size(); ++i) {
            std::printf("%d\n", status[i]);
        }
        for (size_t t = 0; t < matched.size(); ++t) {
            uint32_t ub = 0, vb = 0;
            std::memcpy(&ub, &matched[t].x(), 4);
            std::memcpy(&vb, &matched[t].y(), 4);
            std::printf("%08x %08x\n", ub, vb);
        }
    }
    return ok ? 0 : 1;
}
