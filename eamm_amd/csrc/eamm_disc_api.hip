// The discriminator's operators as entries of their own family, eamm_disc_* (include/eamm_hip.h): the valid 4x4 convolution with its
// data and weight gradients (disc_conv4.hip) and InstanceNorm + LeakyReLU + AvgPool with its backward (disc_norm.hip).  The operator
// convention: device index first, (workspace, workspace_floats) before the stream, stream last, errors through eamm_last_error(NULL).
// Every refusal names its entry and its reason.
#include "op_common.h"

namespace {

constexpr float DISC_EPS = 1e-5f;   // nn.InstanceNorm2d's default

#define DISC_REFUSE(cond, ...) \
    if (cond) return fail(nullptr, EAMM_ERR_ARG, __VA_ARGS__)

}  // namespace

extern "C" {

size_t eamm_disc_conv4_workspace_floats(int B, int H, int W, int Cin, int Cout, int pad, int transposed, int thin) {
    return disc_conv4_workspace_floats(B, H, W, Cin, Cout, pad, transposed, thin);
}

int eamm_disc_conv4(int device, const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, int pad,
                    int transposed, int thin, float* out, float* workspace, size_t workspace_floats, void* stream_) {
    DISC_REFUSE(!x || !weight || !out, "eamm_disc_conv4: x / weight / out is null");
    if (const char* why = disc_conv4_refusal(B, H, W, Cin, Cout, pad, transposed, thin)) return fail(nullptr, EAMM_ERR_ARG, "eamm_disc_conv4: %s", why);
    DISC_REFUSE(!op_aligned16(x) || !op_aligned16(out), "eamm_disc_conv4: x / out are not 16-byte aligned");
    const size_t need = disc_conv4_workspace_floats(B, H, W, Cin, Cout, pad, transposed, thin);
    DISC_REFUSE(!op_workspace_ok(workspace, workspace_floats, need, true),
                "eamm_disc_conv4: workspace too small or misaligned (%zu floats needed, 16-byte aligned)", need);
    OP_ENTRY(false, "");
    OP_DONE(disc_conv4_launch(x, B, H, W, Cin, weight, bias, Cout, pad, transposed, thin, out, workspace, s), "eamm_disc_conv4");
}

size_t eamm_disc_conv4_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout) {
    return disc_conv4_wgrad_workspace_floats(B, H, W, Cin, Cout);
}

int eamm_disc_conv4_wgrad(int device, const float* x, const float* grad_out, int B, int H, int W, int Cin, int Cout, float* grad_weight,
                          float* grad_bias, float* workspace, size_t workspace_floats, void* stream_) {
    DISC_REFUSE(!x || !grad_out, "eamm_disc_conv4_wgrad: x / grad_out is null");
    DISC_REFUSE(!grad_weight && !grad_bias, "eamm_disc_conv4_wgrad: grad_weight and grad_bias are both null");
    if (const char* why = disc_conv4_wgrad_refusal(B, H, W, Cin, Cout)) return fail(nullptr, EAMM_ERR_ARG, "eamm_disc_conv4_wgrad: %s", why);
    DISC_REFUSE(!op_aligned16(x) || !op_aligned16(grad_out), "eamm_disc_conv4_wgrad: x / grad_out are not 16-byte aligned");
    const size_t need = disc_conv4_wgrad_workspace_floats(B, H, W, Cin, Cout);
    DISC_REFUSE(!op_workspace_ok(workspace, workspace_floats, need, true),
                "eamm_disc_conv4_wgrad: workspace too small or misaligned (%zu floats needed, 16-byte aligned)", need);
    OP_ENTRY(false, "");
    OP_DONE(disc_conv4_wgrad_launch(x, grad_out, B, H, W, Cin, Cout, grad_weight, grad_bias, workspace, s), "eamm_disc_conv4_wgrad");
}

size_t eamm_disc_norm_act_pool_workspace_floats(int B, int H, int W, int C, int norm) { return disc_norm_workspace_floats(B, H, W, C, norm, 0); }

int eamm_disc_norm_act_pool(int device, const float* x, const float* gamma, const float* beta, int B, int H, int W, int C, int norm, int pool,
                            double* stats, float* out, float* workspace, size_t workspace_floats, void* stream_) {
    DISC_REFUSE(!x || !out, "eamm_disc_norm_act_pool: x / out is null");
    DISC_REFUSE((norm != 0 && norm != 1) || (pool != 0 && pool != 1), "eamm_disc_norm_act_pool: norm and pool are 0 or 1");
    if (const char* why = disc_norm_refusal(B, H, W, C, norm, pool)) return fail(nullptr, EAMM_ERR_ARG, "eamm_disc_norm_act_pool: %s", why);
    DISC_REFUSE(norm && (!gamma || !beta || !stats), "eamm_disc_norm_act_pool: gamma / beta / stats is null (needed with norm)");
    DISC_REFUSE(!op_aligned16(x) || !op_aligned16(out) || !op_aligned16(gamma) || !op_aligned16(beta),
                "eamm_disc_norm_act_pool: x / out / gamma / beta are not 16-byte aligned");
    const size_t need = disc_norm_workspace_floats(B, H, W, C, norm, 0);
    DISC_REFUSE(norm && !op_workspace_ok(workspace, workspace_floats, need, true),
                "eamm_disc_norm_act_pool: workspace too small or misaligned (%zu floats needed, 16-byte aligned)", need);
    OP_ENTRY(false, "");
    OP_DONE(disc_norm_act_pool_launch(x, gamma, beta, B, H, W, C, norm, pool, DISC_EPS, stats, out, workspace, s), "eamm_disc_norm_act_pool");
}

size_t eamm_disc_norm_act_pool_backward_workspace_floats(int B, int H, int W, int C, int norm) {
    return disc_norm_workspace_floats(B, H, W, C, norm, 1);
}

int eamm_disc_norm_act_pool_backward(int device, const float* x, const double* stats, const float* gamma, const float* beta,
                                     const float* grad_out, int B, int H, int W, int C, int norm, int pool, float* grad_x, float* grad_gamma,
                                     float* grad_beta, float* workspace, size_t workspace_floats, void* stream_) {
    DISC_REFUSE(!x || !grad_out, "eamm_disc_norm_act_pool_backward: x / grad_out is null");
    DISC_REFUSE(!grad_x && !grad_gamma && !grad_beta, "eamm_disc_norm_act_pool_backward: grad_x, grad_gamma and grad_beta are all null");
    DISC_REFUSE((norm != 0 && norm != 1) || (pool != 0 && pool != 1), "eamm_disc_norm_act_pool_backward: norm and pool are 0 or 1");
    if (const char* why = disc_norm_refusal(B, H, W, C, norm, pool)) return fail(nullptr, EAMM_ERR_ARG, "eamm_disc_norm_act_pool_backward: %s", why);
    DISC_REFUSE(norm && (!gamma || !beta || !stats), "eamm_disc_norm_act_pool_backward: gamma / beta / stats is null (needed with norm)");
    DISC_REFUSE(!norm && (grad_gamma || grad_beta || !grad_x), "eamm_disc_norm_act_pool_backward: without norm there is grad_x alone");
    DISC_REFUSE(!op_aligned16(x) || !op_aligned16(grad_out) || !op_aligned16(grad_x) || !op_aligned16(gamma) || !op_aligned16(beta),
                "eamm_disc_norm_act_pool_backward: x / grad_out / grad_x / gamma / beta are not 16-byte aligned");
    const size_t need = disc_norm_workspace_floats(B, H, W, C, norm, 1);
    DISC_REFUSE(norm && !op_workspace_ok(workspace, workspace_floats, need, true),
                "eamm_disc_norm_act_pool_backward: workspace too small or misaligned (%zu floats needed, 16-byte aligned)", need);
    OP_ENTRY(false, "");
    OP_DONE(disc_norm_act_pool_backward_launch(x, stats, gamma, beta, grad_out, B, H, W, C, norm, pool, grad_x, grad_gamma, grad_beta, workspace, s),
            "eamm_disc_norm_act_pool_backward");
}

}  // extern "C"
