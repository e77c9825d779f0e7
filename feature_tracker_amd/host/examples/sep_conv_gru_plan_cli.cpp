// sep_conv_gru_plan_cli — prints the launch plan of the SepConvGru kernels (csrc/sep_conv_gru_plan.h) without a device.  One case per
// line on stdin:
//   h_channels in_channels kernel_size vertical gates B H W
// one line of key=value pairs per case on stdout.  tests/test_sep_conv_gru_cpu.py drives it.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "sep_conv_gru_plan.h"

int main() {
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream line(text);
        long long v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (long long &e : v) {
            line >> e;
        }
        ftk::SepConvGruPlanInput in{};
        in.h_channels = (int32_t)v[0], in.in_channels = (int32_t)v[1], in.kernel_size = (int32_t)v[2], in.vertical = (int32_t)v[3], in.gates = (int32_t)v[4];
        in.B = (int32_t)v[5], in.H = (int32_t)v[6], in.W = (int32_t)v[7];
        const ftk::SepConvGruPlan p = ftk::sep_conv_gru_plan(in);
        printf("refused=%s", ftk::gru_refusal_name(p.refused));
        if (p.refused == ftk::GruRefusal::None) {
            printf(" out_channels=%d m_tiles=%d wm=%d wn=%d m_groups=%d tile_w=%d tile_h=%d tiles_x=%d tiles_y=%d chunk=%d chunks=%d steps_per_chunk=%d k_steps=%d"
                   " pitch=%d lds=%zu lds_static=%zu packed=%lld grid=%ux%u block=%ux%u mfma=%s",
                   p.out_channels, p.m_tiles, p.wm, p.wn, p.m_groups, p.tile_w, p.tile_h, p.tiles_x, p.tiles_y, ftk::kGruChunk, p.chunks, p.steps_per_chunk,
                   p.k_steps, p.pitch, p.lds, sizeof(float) * ftk::kGruLdsFloats,
                   (long long)ftk::sep_conv_gru_packed_elements(p.out_channels, in.in_channels, in.kernel_size), p.grid.x, p.grid.y, p.block.x, p.block.y,
                   p.mfma);
        }
        printf("\n");
    }
    return 0;
}
