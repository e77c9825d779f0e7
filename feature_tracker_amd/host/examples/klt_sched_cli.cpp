// klt_sched_cli — walks the trackers' two state machines (csrc/klt_sched.h: launch order and tail class) without a device.
// One command per line on stdin, one line of key=value pairs on stdout for every command except `new`, `set` and `fail`:
//   new                          fresh states
//   set sched_call|tail_call V   put a counter where a test wants it
//   call n n_track model waves long_tail capturing ref_untouched sched sched_min have_grid have_claim have_pred
//                                one tracker call through klt_sched_step (sched / sched_min: parsed switches, -1 = not set)
//   fail                         the launch of the last call failed: klt_sched_reset
//   tail model method seen_word  klt_tail_class_step
//   launch model method          klt_tail_next_call
//   word grid|claim|flag|tail A B   pack (A, B), then unpack
// tests/test_klt_sched_cpu.py drives it.
#include <cstdio>
#include <cstring>

#include "klt_sched.h"

int main() {
    static const char *const orders[] = {"none", "index", "position"};
    ftk::KltSchedState sched;
    ftk::KltTailState tail;
    char line[512], what[32];
    while (fgets(line, sizeof(line), stdin)) {
        ftk::KltSchedInput in = {};
        int model = 0, method = 0, capturing = 0, ref_untouched = 0, have_grid = 0, have_claim = 0, have_pred = 0;
        unsigned a = 0, b = 0;
        if (strncmp(line, "new", 3) == 0) {
            sched = ftk::KltSchedState();
            tail = ftk::KltTailState();
        } else if (sscanf(line, "set %31s %u", what, &a) == 2) {
            (strcmp(what, "sched_call") == 0 ? sched.call : tail.call) = a;
        } else if (strncmp(line, "fail", 4) == 0) {
            ftk::klt_sched_reset(sched);
        } else if (sscanf(line, "call %d %u %d %d %d %d %d %d %d %d %d %d", &in.n, &in.n_track, &in.model, &in.waves_per_feature, &in.long_tail, &capturing,
                          &ref_untouched, &in.sched, &in.sched_min, &have_grid, &have_claim, &have_pred) == 12) {
            in.capturing = capturing != 0;
            in.ref_untouched = ref_untouched != 0;
            in.have_grid = have_grid != 0;
            in.have_claim = have_claim != 0;
            in.have_pred = have_pred != 0;
            const ftk::KltSchedStep s = ftk::klt_sched_step(sched, in);
            printf("active=%d grow_to=%zu wipe=%d iters_buf=%d sort_from=%d sort_reads_ref_uv=%d order=%s order_buf=%d recording=%d sched_call=%u trades=%d"
                   " state_recorded=%u state_call=%u state_capacity=%zu state_n=%d state_calls=%u\n",
                   s.active, s.grow_to, s.wipe_claims_and_grid, s.iters_buf, s.sort_from, s.sort_reads_ref_uv, orders[(int)s.order], s.order_buf, s.recording,
                   s.sched_call, s.trades, sched.recorded, sched.call, sched.capacity, sched.n, sched.calls);
        } else if (sscanf(line, "tail %d %d %u", &model, &method, &a) == 3) {
            printf("long_tail=%d\n", ftk::klt_tail_class_step(tail, model, method, a));
        } else if (sscanf(line, "launch %d %d", &model, &method) == 2) {
            bool wipe = false;
            const uint32_t call = ftk::klt_tail_next_call(tail, model, method, &wipe);
            printf("tail_call=%u wipe=%d\n", call, wipe);
        } else if (sscanf(line, "word %31s %u %u", what, &a, &b) == 3) {
            if (strcmp(what, "grid") == 0) {
                printf("word=%u call=%u low=%u\n", ftk::sched_grid_pack(a, b), ftk::sched_grid_call(ftk::sched_grid_pack(a, b)), ftk::sched_grid_iters(ftk::sched_grid_pack(a, b)));
            } else if (strcmp(what, "claim") == 0) {
                printf("word=%u call=%u low=%u\n", ftk::sched_claim_pack(a, b), ftk::sched_claim_call(ftk::sched_claim_pack(a, b)), ftk::sched_claim_code(ftk::sched_claim_pack(a, b)));
            } else if (strcmp(what, "flag") == 0) {
                printf("word=%u call=%u low=%u\n", ftk::sched_flag_pack(a, b), ftk::sched_flag_call(ftk::sched_flag_pack(a, b)), ftk::sched_flag_flat(ftk::sched_flag_pack(a, b)));
            } else {
                printf("word=%u call=%u low=%u\n", ftk::tail_word_pack(a, b), ftk::tail_word_call(ftk::tail_word_pack(a, b)), ftk::tail_word_iters(ftk::tail_word_pack(a, b)));
            }
        } else {
            fprintf(stderr, "klt_sched_cli: cannot read '%s'\n", line);
            return 1;
        }
    }
    return 0;
}
