/* raft_conv_ref.c — scalar CPU restatement of the stock layers of RAFT's UpdateBlock (src/nn_optical_flow_tracker/raft/update_block.py:4-67)
 * as DESIGN.md 5.14 states them, and of the whole block around the GRU restatement of tests/sep_conv_gru_ref.c (compiled together with
 * this file).  TEST INFRASTRUCTURE ONLY: independent code, it includes nothing from feature_tracker_amd/ and nothing there may use it.
 * Compile with -ffp-contract=off: every operation below is one correctly rounded float32 operation, the fused ones are written as fmaf.
 *
 * One layer: acc = bias[co]; for k = (c * ks + ty) * ks + tx ascending (c over the concatenation of the parts: the memory order of torch's
 * weight tensor) acc = fmaf(w[co][c][ty][tx], in[c][y + ty - pad][x + tx - pad], acc).  A tap outside the image is +0.0f and is MULTIPLIED,
 * not skipped, as sep_conv_gru_ref.c treats its padding: fmaf(w, +0, acc) turns an accumulator of -0 into +0 and an infinite or NaN
 * weight into NaN.  Then, in this order: v = (acc < 0) ? +0 : acc if relu (a NaN and -0 pass through), and out = scale * v.
 *
 * `variant` is a test-only argument: 0 the contract, and six mutants that the float64 comparison of tests/test_update_block_cpu.py must
 * reject: 1 taps flipped (convolution instead of correlation: tap (ty, tx) reads the pixel shifted by (pad - ty, pad - tx)); 2 ty and tx
 * transposed; 3 a tap outside the image reads the clamped edge pixel instead of +0; 4 every ReLU dropped; 5 temp_flow before
 * temp_correlation in out_conv's input; 6 the flow head fed the old net instead of the new one (5 and 6: rc_update_block only). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* tests/sep_conv_gru_ref.c */
int scg_forward(const float *const *parts, const int32_t *part_channels, int32_t n_parts, const float *h, const float *const *weights,
                const float *const *biases, int32_t Ch, int32_t ks, int32_t B, int32_t H, int32_t W, int32_t variant, float *out);

int rc_conv2d(const float *const *parts, const int32_t *part_channels, int32_t n_parts, const float *weight, const float *bias, int32_t Cout, int32_t ks,
              int32_t relu, float scale, int32_t B, int32_t H, int32_t W, int32_t variant, float *out) {
    if (!parts || !part_channels || n_parts < 1 || !weight || !bias || !out || Cout < 1 || (ks != 1 && ks != 3 && ks != 7) || B < 1 || H < 1 || W < 1 ||
        variant < 0 || variant > 6) {
        return -1;
    }
    int32_t Cin = 0;
    for (int32_t i = 0; i < n_parts; ++i) {
        if (part_channels[i] < 1 || !parts[i]) {
            return -1;
        }
        Cin += part_channels[i];
    }
    const int32_t pad = ks / 2;
    const int64_t HW = (int64_t)H * W, K = (int64_t)Cin * ks * ks;
    for (int64_t b = 0; b < B; ++b) {
        for (int32_t co = 0; co < Cout; ++co) {
            const float *w = weight + co * K;
            for (int32_t y = 0; y < H; ++y) {
                for (int32_t x = 0; x < W; ++x) {
                    float acc = bias[co];
                    int32_t c = 0;
                    for (int32_t i = 0; i < n_parts; ++i) {
                        for (int32_t cp = 0; cp < part_channels[i]; ++cp, ++c) {
                            const float *p = parts[i] + (b * part_channels[i] + cp) * HW;
                            for (int32_t ty = 0; ty < ks; ++ty) {
                                for (int32_t tx = 0; tx < ks; ++tx) {
                                    int32_t dy = ty - pad, dx = tx - pad;
                                    if (variant == 1) {
                                        dy = -dy, dx = -dx;
                                    } else if (variant == 2) {
                                        const int32_t t = dy;
                                        dy = dx, dx = t;
                                    }
                                    int32_t yy = y + dy, xx = x + dx;
                                    float v;
                                    if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
                                        v = p[(int64_t)yy * W + xx];
                                    } else if (variant == 3) {
                                        yy = yy < 0 ? 0 : (yy >= H ? H - 1 : yy);
                                        xx = xx < 0 ? 0 : (xx >= W ? W - 1 : xx);
                                        v = p[(int64_t)yy * W + xx];
                                    } else {
                                        v = 0.0f;
                                    }
                                    acc = fmaf(w[((int64_t)c * ks + ty) * ks + tx], v, acc);
                                }
                            }
                        }
                    }
                    float v = acc;
                    if (relu && variant != 4) {
                        v = (acc < 0.0f) ? 0.0f : acc;
                    }
                    out[(b * Cout + co) * HW + (int64_t)y * W + x] = scale * v;
                }
            }
        }
    }
    return 0;
}

/* sizes: net, inp, corr_in, corr_hidden, corr_out, flow_hidden, flow_out, motion_out, head_hidden, mask_hidden, mask_out, gru_ks, B, H, W.
 * conv_w / conv_b: correlation_conv.0, correlation_conv.2, flow_conv.0, flow_conv.2, out_conv.0, flow_head.conv1, flow_head.conv2, mask.0,
 * mask.2; gru_w / gru_b as scg_forward takes them; features: NULL or [B][motion_out - 2][H][W], the motion encoder's `out`.  update_block.py:61-67 with :36-43 and :10-14. */
int rc_update_block(const float *net, const float *inp, const float *correlation, const float *flow, const float *const *conv_w, const float *const *conv_b,
                    const float *const *gru_w, const float *const *gru_b, const int32_t *sizes, int32_t variant, float *new_net, float *mask,
                    float *delta_flow, float *features) {
    if (!net || !inp || !correlation || !flow || !conv_w || !conv_b || !gru_w || !gru_b || !sizes || !new_net || !mask || !delta_flow || variant < 0 ||
        variant > 6) {
        return -1;
    }
    const int32_t Cnet = sizes[0], Cinp = sizes[1], corr_in = sizes[2], corr_hidden = sizes[3], corr_out = sizes[4], flow_hidden = sizes[5],
                  flow_out = sizes[6], motion_out = sizes[7], head_hidden = sizes[8], mask_hidden = sizes[9], mask_out = sizes[10], gru_ks = sizes[11],
                  B = sizes[12], H = sizes[13], W = sizes[14];
    if (motion_out < 3) {
        return -1;
    }
    const int32_t cv = variant <= 4 ? variant : 0; /* the variant of every layer */
    const size_t px = (size_t)B * H * W;
    int32_t widest = corr_hidden;
    const int32_t widths[] = {corr_out, flow_hidden, flow_out, motion_out, head_hidden, mask_hidden};
    for (size_t i = 0; i < sizeof widths / sizeof widths[0]; ++i) {
        widest = widths[i] > widest ? widths[i] : widest;
    }
    float *t0 = malloc(px * widest * sizeof(float)), *tc = malloc(px * corr_out * sizeof(float)), *tf = malloc(px * flow_out * sizeof(float)),
          *mo = malloc(px * (motion_out - 2) * sizeof(float));
    int rc = (t0 && tc && tf && mo) ? 0 : -2;
    const int32_t one_corr[] = {corr_in}, one_ch[] = {corr_hidden}, one_flow[] = {2}, one_fh[] = {flow_hidden};
    /* MotionEncoder.forward, :37-40 */
    const float *in1[] = {correlation};
    rc = rc ? rc : rc_conv2d(in1, one_corr, 1, conv_w[0], conv_b[0], corr_hidden, 1, 1, 1.0f, B, H, W, cv, t0);
    in1[0] = t0;
    rc = rc ? rc : rc_conv2d(in1, one_ch, 1, conv_w[1], conv_b[1], corr_out, 3, 1, 1.0f, B, H, W, cv, tc);
    in1[0] = flow;
    rc = rc ? rc : rc_conv2d(in1, one_flow, 1, conv_w[2], conv_b[2], flow_hidden, 7, 1, 1.0f, B, H, W, cv, t0);
    in1[0] = t0;
    rc = rc ? rc : rc_conv2d(in1, one_fh, 1, conv_w[3], conv_b[3], flow_out, 3, 1, 1.0f, B, H, W, cv, tf);
    const float *temp[] = {tc, tf};
    int32_t temp_ch[] = {corr_out, flow_out};
    if (variant == 5) {
        temp[0] = tf, temp[1] = tc;
        temp_ch[0] = flow_out, temp_ch[1] = corr_out;
    }
    rc = rc ? rc : rc_conv2d(temp, temp_ch, 2, conv_w[4], conv_b[4], motion_out - 2, 3, 1, 1.0f, B, H, W, cv, mo);
    if (!rc && features) { /* MotionEncoder.forward's `out`, before :41's cat with flow */
        memcpy(features, mo, px * (motion_out - 2) * sizeof(float));
    }
    /* :62-64: the GRU over cat[inp, cat[out, flow]] */
    const float *x[] = {inp, mo, flow};
    const int32_t x_ch[] = {Cinp, motion_out - 2, 2};
    rc = rc ? rc : scg_forward(x, x_ch, 3, net, gru_w, gru_b, Cnet, gru_ks, B, H, W, 0, new_net);
    /* :65-66 */
    const int32_t one_net[] = {Cnet}, one_hh[] = {head_hidden}, one_mh[] = {mask_hidden};
    in1[0] = variant == 6 ? net : new_net;
    rc = rc ? rc : rc_conv2d(in1, one_net, 1, conv_w[5], conv_b[5], head_hidden, 3, 1, 1.0f, B, H, W, cv, t0);
    in1[0] = t0;
    rc = rc ? rc : rc_conv2d(in1, one_hh, 1, conv_w[6], conv_b[6], 2, 3, 0, 1.0f, B, H, W, cv, delta_flow);
    in1[0] = new_net;
    rc = rc ? rc : rc_conv2d(in1, one_net, 1, conv_w[7], conv_b[7], mask_hidden, 3, 1, 1.0f, B, H, W, cv, t0);
    in1[0] = t0;
    rc = rc ? rc : rc_conv2d(in1, one_mh, 1, conv_w[8], conv_b[8], mask_out, 1, 0, 0.25f, B, H, W, cv, mask);
    free(t0), free(tc), free(tf), free(mo);
    return rc;
}
