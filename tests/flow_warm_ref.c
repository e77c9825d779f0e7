/* flow_warm_ref.c — scalar CPU restatement of the warm start of RAFT on video as DESIGN.md 5.18 states it: a coarse flow pushed forward
 * along itself, the nearest valid landing per target pixel (upstream RAFT's forward_interpolate, which asks scipy's
 * griddata(method="nearest") on the host).  TEST INFRASTRUCTURE ONLY: independent code, it includes nothing from feature_tracker_amd/ and
 * nothing there may use it.  Compile with -ffp-contract=off: every operation is one correctly rounded float32 operation, the fused one is
 * written as fmaf.
 *
 * `variant` is a test-only argument: 0 the contract; 1 a mutant in which the HIGHEST source index wins among equal distances; 2 a mutant
 * whose validity test is x1 >= 0 && x1 <= W && y1 >= 0 && y1 <= H; 3 a mutant that measures a landing (x1, y1) from the target as if it
 * were (y1, x1). */
#include <math.h>
#include <stdint.h>

/* flow [B][2][H][W] -> out [B][2][H][W]; chosen (or NULL) [B][H][W]: the winning source index of each target, -1 without one */
int fwr_warm(const float *flow, int32_t B, int32_t H, int32_t W, int32_t variant, float *out, int32_t *chosen) {
    if (!flow || !out || B < 1 || H < 1 || W < 1 || (int64_t)H * W > (1 << 20) || variant < 0 || variant > 3) {
        return -1;
    }
    const int64_t HW = (int64_t)H * W;
    const float w = (float)W, h = (float)H;
    for (int64_t b = 0; b < B; ++b) {
        const float *fx = flow + b * 2 * HW, *fy = fx + HW;
        for (int64_t t = 0; t < HW; ++t) {
            const float tx = (float)(t % W), ty = (float)(t / W);
            float best = 0.0f;
            int64_t best_s = -1;
            for (int64_t s = 0; s < HW; ++s) {
                const float x1 = (float)(s % W) + fx[s], y1 = (float)(s / W) + fy[s];
                const int valid = variant == 2 ? (x1 >= 0.0f && x1 <= w && y1 >= 0.0f && y1 <= h) : (x1 > 0.0f && x1 < w && y1 > 0.0f && y1 < h);
                if (!valid) {
                    continue;
                }
                const float ex = tx - (variant == 3 ? y1 : x1), ey = ty - (variant == 3 ? x1 : y1);
                const float d2 = fmaf(ey, ey, ex * ex);
                if (best_s < 0 || d2 < best || (variant == 1 && d2 == best)) {
                    best = d2;
                    best_s = s;
                }
            }
            out[b * 2 * HW + t] = best_s < 0 ? 0.0f : fx[best_s];
            out[b * 2 * HW + HW + t] = best_s < 0 ? 0.0f : fy[best_s];
            if (chosen) {
                chosen[b * HW + t] = (int32_t)best_s;
            }
        }
    }
    return 0;
}
