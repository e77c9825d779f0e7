// klt_plan_cli — prints the launch plan of KLT calls (csrc/klt_plan.h) without a device: which kernel form and instantiation a call
// runs, its grid, block and LDS size, and the launch-shape fields of its argument block.  One case per line on stdin:
//   model method half_rows half_cols n max_extent luminance tree long_tail waves group lssd_chunked spill
// (the last four are the parsed FTK_KLT_WAVES / FTK_KLT_GROUP / FTK_LSSD_CHUNKED / FTK_KLT_SPILL overrides, -1 = not set);
// one line of key=value pairs per case on stdout.  tests/test_klt_plan_cpu.py drives it.
#include <cstdio>
#include <cstring>

#include "klt_plan.h"

int main() {
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
        printf("rc=0 stable=%d form=%s lds_bytes=%zu grid=%u block=%u kernel=%d family=%s half=%d solo=%d k_tree=%d k_lum=%d k_spill=%d k_row_chunks=%d", stable ? 1 : 0,
               forms[(int)plan.form], plan.lds_bytes, plan.grid, plan.block, k.entry != nullptr, k.family ? k.family : "-", k.half, k.solo, k.tree, k.lum, k.spill, k.row_chunks);
        printf(" waves_per_feature=%d features_per_group=%d group_lds_stride=%d px_floats=%d terms_floats=%d a0_floats=%d lssd_chunked=%d quad_chain=%d"
               " pb_enabled=%d fk_enabled=%d spill=%d tree=%d long_tail=%d spill_stride_floats=%u rwin_rows=%d rwin_cols=%d cwin_rows=%d cwin_cols=%d P=%d\n",
               p.waves_per_feature, p.features_per_group, p.group_lds_stride, p.px_floats, p.terms_floats, p.a0_floats, p.lssd_chunked, p.quad_chain, p.pb_enabled,
               p.fk_enabled, p.spill, p.tree, p.long_tail, p.spill_stride_floats, p.rwin_rows, p.rwin_cols, p.cwin_rows, p.cwin_cols, p.P);
    }
    return 0;
}
