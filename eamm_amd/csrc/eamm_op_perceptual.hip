// The perceptual loss's operators that are no convolutions (perceptual.hip): one pyramid level in conv1_1's layout, ReLU with
// MaxPool2d(2, 2), the weighted L1 mean of a feature pair -- each with its backward.  Every refusal names its entry and its argument.
#include "op_common.h"

namespace {

constexpr int VGG_IN_C = 32;   // conv1_1's input: three channels padded to the convolution kernels' granule (CONV_BK)

#define PERC_REFUSE(cond, msg) \
    if (cond) return fail(nullptr, EAMM_ERR_ARG, msg)

}  // namespace

extern "C" {

int eamm_op_vgg_input(int device, const float* image, const float* aa_weight, const float* mean, const float* std_, int B, int H, int W,
                      int inv_scale, float* out_nhwc, float* level_nchw, void* stream_) {
    PERC_REFUSE(!image, "eamm_op_vgg_input: image is null");
    PERC_REFUSE(!out_nhwc && !level_nchw, "eamm_op_vgg_input: out_nhwc and level_nchw are both null");
    PERC_REFUSE(out_nhwc && (!mean || !std_), "eamm_op_vgg_input: mean / std are null (needed for out_nhwc)");
    PERC_REFUSE(!op_count_ok(B, H, W, VGG_IN_C), "eamm_op_vgg_input: B, H, W must be positive with B * H * W * 32 below 2^31");
    PERC_REFUSE(inv_scale < 1 || H % inv_scale || W % inv_scale, "eamm_op_vgg_input: inv_scale must be an integer >= 1 dividing H and W");
    PERC_REFUSE(inv_scale != 1 && !aa_weight, "eamm_op_vgg_input: aa_weight (the [3,1,13,13] buffer) is null with inv_scale > 1");
    PERC_REFUSE(out_nhwc && !op_aligned16(out_nhwc), "eamm_op_vgg_input: out_nhwc is not 16-byte aligned");
    OP_ENTRY(false, "");
    OP_DONE(vgg_input_launch(image, aa_weight, mean, std_, B, H, W, inv_scale, out_nhwc, level_nchw, s), "eamm_op_vgg_input");
}

int eamm_op_vgg_input_backward(int device, const float* grad_nhwc, int grad_channels, const float* grad_level, const float* aa_weight,
                               const float* std_, int B, int H, int W, int inv_scale, float* grad_image, void* stream_) {
    PERC_REFUSE(!grad_nhwc && !grad_level, "eamm_op_vgg_input_backward: grad_nhwc and grad_level are both null");
    PERC_REFUSE(!grad_image, "eamm_op_vgg_input_backward: grad_image is null");
    PERC_REFUSE(grad_nhwc && !std_, "eamm_op_vgg_input_backward: std is null (needed for grad_nhwc)");
    PERC_REFUSE(grad_nhwc && (grad_channels < 4 || (grad_channels & 3) || !op_aligned16(grad_nhwc)),
                "eamm_op_vgg_input_backward: grad_nhwc needs a channel count that is a multiple of 4 and a 16-byte aligned address");
    PERC_REFUSE(!op_count_ok(B, H, W, grad_nhwc ? grad_channels : 3),
                "eamm_op_vgg_input_backward: B, H, W must be positive with fewer than 2^31 elements");
    PERC_REFUSE(inv_scale < 1 || H % inv_scale || W % inv_scale,
                "eamm_op_vgg_input_backward: inv_scale must be an integer >= 1 dividing H and W");
    PERC_REFUSE(inv_scale != 1 && !aa_weight, "eamm_op_vgg_input_backward: aa_weight (the [3,1,13,13] buffer) is null with inv_scale > 1");
    OP_ENTRY(false, "");
    OP_DONE(vgg_input_backward_launch(grad_nhwc, grad_channels, grad_level, aa_weight, std_, B, H, W, inv_scale, grad_image, s),
            "eamm_op_vgg_input_backward");
}

int eamm_op_relu_pool(int device, float* x, int B, int H, int W, int C, float* pooled, void* stream_) {
    PERC_REFUSE(!x, "eamm_op_relu_pool: x is null");
    PERC_REFUSE(C < 32 || C % 32 || !op_count_ok(B, H, W, C),
                "eamm_op_relu_pool: B, H, W must be positive, C a multiple of 32, fewer than 2^31 elements");
    PERC_REFUSE(pooled && (H < 2 || W < 2), "eamm_op_relu_pool: a map below 2 x 2 has no pooling window (pooled must be null)");
    PERC_REFUSE(!op_aligned16(x) || !op_aligned16(pooled), "eamm_op_relu_pool: x / pooled are not 16-byte aligned");
    OP_ENTRY(false, "");
    OP_DONE(relu_pool_launch(x, B, H, W, C, pooled, s), "eamm_op_relu_pool");
}

int eamm_op_relu_pool_backward(int device, const float* y, const float* dy, const float* dp, int B, int H, int W, int C, float* dx,
                               void* stream_) {
    PERC_REFUSE(!y || !dx, "eamm_op_relu_pool_backward: y / dx is null");
    PERC_REFUSE(!dy && !dp, "eamm_op_relu_pool_backward: dy and dp are both null");
    PERC_REFUSE(C < 32 || C % 32 || !op_count_ok(B, H, W, C),
                "eamm_op_relu_pool_backward: B, H, W must be positive, C a multiple of 32, fewer than 2^31 elements");
    PERC_REFUSE(dp && (H < 2 || W < 2), "eamm_op_relu_pool_backward: a map below 2 x 2 has no pooling window (dp must be null)");
    PERC_REFUSE(!op_aligned16(y) || !op_aligned16(dy) || !op_aligned16(dp) || !op_aligned16(dx),
                "eamm_op_relu_pool_backward: y / dy / dp / dx are not 16-byte aligned");
    OP_ENTRY(false, "");
    OP_DONE(relu_pool_backward_launch(y, dy, dp, B, H, W, C, dx, s), "eamm_op_relu_pool_backward");
}

size_t eamm_op_l1_pair_workspace_floats(long long n) { return n < 1 ? 0 : (size_t)2 * l1_pair_partials(n); }

int eamm_op_l1_pair(int device, const float* a, const float* b, long long n, float weight, float* value, float* grad, float* workspace,
                    size_t workspace_floats, void* stream_) {
    PERC_REFUSE(!a || !b || !value || !grad, "eamm_op_l1_pair: a / b / value / grad is null");
    PERC_REFUSE(n < 1, "eamm_op_l1_pair: n must be positive");
    PERC_REFUSE(!op_aligned16(a) || !op_aligned16(b) || !op_aligned16(grad), "eamm_op_l1_pair: a / b / grad are not 16-byte aligned");
    PERC_REFUSE(!op_workspace_ok(workspace, workspace_floats, eamm_op_l1_pair_workspace_floats(n), true),
                "eamm_op_l1_pair: workspace of eamm_op_l1_pair_workspace_floats(n) floats, 16-byte aligned");
    OP_ENTRY(false, "");
    OP_DONE(l1_pair_launch(a, b, n, weight, value, grad, reinterpret_cast<double*>(workspace), s), "eamm_op_l1_pair");
}

int eamm_op_l1_pair_backward(int device, const float* grad, long long n, const float* grad_value, float* out, void* stream_) {
    PERC_REFUSE(!grad || !grad_value || !out, "eamm_op_l1_pair_backward: grad / grad_value / out is null");
    PERC_REFUSE(n < 1, "eamm_op_l1_pair_backward: n must be positive");
    PERC_REFUSE(!op_aligned16(grad) || !op_aligned16(out), "eamm_op_l1_pair_backward: grad / out are not 16-byte aligned");
    OP_ENTRY(false, "");
    OP_DONE(l1_pair_backward_launch(grad, n, grad_value, out, s), "eamm_op_l1_pair_backward");
}

}  // extern "C"
