// klt_plan_cli — prints the launch plan of KLT calls (csrc/klt_plan.h) without a device: which kernel form and instantiation a call
// runs, its grid, block and LDS size, and the launch-shape fields of its argument block.  One case per line on stdin:
//   model method half_rows half_cols n max_extent luminance tree long_tail waves group lssd_chunked spill
// (the last four are the parsed FTK_KLT_WAVES / FTK_KLT_GROUP / FTK_LSSD_CHUNKED / FTK_KLT_SPILL overrides, -1 = not set);
// one line of key=value pairs per case on stdout.  tests/test_klt_plan_cpu.py drives it.
#include <cstdio>
#include <cstring>

#include "klt_plan.h"

// `klt_plan_cli inside`: the staging rule of the pipelined kernel's byte windows (ftk_device.h klt_byte_window_inside).  One case per
// line on stdin: im_rows im_cols wrows pitch lo margin; one line of '0' / '1' per case on stdout, the rule's answer for every window origin
// r_lo in [lo, im_rows + margin) (outer) and c_lo in [lo, im_cols + margin) (inner).
static int inside_mode() {
    int im_rows, im_cols, wrows, pitch, lo, margin;
    while (scanf("%d %d %d %d %d %d", &im_rows, &im_cols, &wrows, &pitch, &lo, &margin) == 6) {
        for (int r_lo = lo; r_lo < im_rows + margin; ++r_lo) {
            for (int c_lo = lo; c_lo < im_cols + margin; ++c_lo) {
                putchar(ftk::klt_byte_window_inside(im_rows, im_cols, r_lo, c_lo, wrows, pitch) ? '1' : '0');
            }
        }
        putchar('\n');
    }
    return 0;
}

// `klt_plan_cli units`: where the 8-byte units of a byte window come from (ftk_device.h klt_byte_unit_offset, the function the kernel's
// staging uses).  One case per line on stdin: im_cols wrows pitch; one line per case on stdout: the image byte offset of every unit
// idx in [0, wrows * pitch / 8) relative to the window's origin, which is also LDS byte 8 * idx of the window.
static int units_mode() {
    int im_cols, wrows, pitch;
    while (scanf("%d %d %d", &im_cols, &wrows, &pitch) == 3) {
        const int shift = ftk::klt_byte_units_shift(pitch);
        for (int idx = 0; idx < (wrows << shift); ++idx) {
            printf("%u ", ftk::klt_byte_unit_offset((uint32_t)idx, shift, (uint32_t)im_cols));
        }
        putchar('\n');
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "inside") == 0) {
        return inside_mode();
    }
    if (argc > 1 && strcmp(argv[1], "units") == 0) {
        return units_mode();
    }
    static const char *const forms[] = {"pipelined", "one_wave_fast", "generic", "generic_spill"};
    ftk::KltPlanInput in;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d", &in.model, &in.method, &in.half_rows, &in.half_cols, &in.n, &in.max_extent, &in.consider_luminance,
                 &in.tree, &in.long_tail, &in.waves, &in.group, &in.lssd_chunked, &in.spill) == 13) {
        ftk::KltParams p, again;
        ftk::KltPlan plan = {}, plan_again = {};
        size_t spill_floats = 0;
        memset(&p, 0, sizeof(p));
        memset(&again, 0, sizeof(again));
        p.n = again.n = in.n;  // (the call's own fields the pickers read)
        p.consider_luminance = again.consider_luminance = in.consider_luminance;
        const int rc = ftk::klt_plan(in, &p, &plan, &spill_floats);
        const int rc_again = ftk::klt_plan(in, &again, &plan_again, &spill_floats);
        if (rc != ftk::kKltPlanOk) {
            printf("rc=%d\n", rc);
            continue;
        }
        const bool stable = rc_again == rc && memcmp(&p, &again, sizeof(p)) == 0 && plan.form == plan_again.form && plan.lds_bytes == plan_again.lds_bytes &&
                            plan.grid == plan_again.grid && plan.block == plan_again.block;
        const ftk::KltKernel k = ftk::klt_pick(plan, in.model, in.method, p);
        printf("rc=0 stable=%d form=%s lds_bytes=%zu grid=%u block=%u kernel=%d family=%s half=%d solo=%d k_tree=%d k_lum=%d k_spill=%d k_row_chunks=%d k_cur_units=%d k_ref_units=%d", stable ? 1 : 0,
               forms[(int)plan.form], plan.lds_bytes, plan.grid, plan.block, k.entry != nullptr, k.family ? k.family : "-", k.half, k.solo, k.tree, k.lum, k.spill, k.row_chunks, k.cur_units, k.ref_units);
        printf(" waves_per_feature=%d features_per_group=%d group_lds_stride=%d px_floats=%d terms_floats=%d a0_floats=%d lssd_chunked=%d quad_chain=%d"
               " pb_enabled=%d fk_enabled=%d spill=%d tree=%d long_tail=%d spill_stride_floats=%u rwin_rows=%d rwin_cols=%d cwin_rows=%d cwin_cols=%d P=%d"
               " pb_rwin_rows=%d pb_rwin_cols=%d pb_rwin_pitch=%d pb_cwin_pitch=%d byte_windows_ok=%d\n",
               p.waves_per_feature, p.features_per_group, p.group_lds_stride, p.px_floats, p.terms_floats, p.a0_floats, p.lssd_chunked, p.quad_chain, p.pb_enabled,
               p.fk_enabled, p.spill, p.tree, p.long_tail, p.spill_stride_floats, p.rwin_rows, p.rwin_cols, p.cwin_rows, p.cwin_cols, p.P,
               p.pb_rwin_rows, p.pb_rwin_cols, p.pb_rwin_pitch, p.pb_cwin_pitch, ftk::klt_byte_windows_ok(p) ? 1 : 0);
    }
    return 0;
}
