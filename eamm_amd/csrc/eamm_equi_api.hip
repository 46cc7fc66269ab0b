// The equivariance transform's operators as entries of their own family, eamm_equi_* (include/eamm_hip.h; kernels in equivariance.hip):
// the frame warp with reflection sampling, the coordinate warp with its jacobian, and the coordinate gradient of both.  The operator
// convention: device index first, stream last, errors through eamm_last_error(NULL).  Every refusal names its entry and its reason.
#include "op_common.h"

namespace {

constexpr int EQUI_MAX_POINTS = 16;   // control points per side
constexpr int EQUI_MAX_C = 6;         // as num_channels

#define EQUI_REFUSE(cond, msg) \
    if (cond) return fail(nullptr, EAMM_ERR_ARG, msg)

bool equi_points_ok(int P) { return P == 0 || (P >= 2 && P <= EQUI_MAX_POINTS); }

}  // namespace

extern "C" {

int eamm_equi_tps_warp_frame(int device, const float* frame, const float* theta, const float* control_params, int points, int B, int C,
                             int H, int W, float* out, void* stream_) {
    EQUI_REFUSE(!frame || !theta || !out, "eamm_equi_tps_warp_frame: frame / theta / out is null");
    EQUI_REFUSE(!equi_points_ok(points), "eamm_equi_tps_warp_frame: points must be 0 (affine only) or 2..16");
    EQUI_REFUSE(points && !control_params, "eamm_equi_tps_warp_frame: control_params is null with points > 0");
    EQUI_REFUSE(C < 1 || C > EQUI_MAX_C, "eamm_equi_tps_warp_frame: C must be 1..6");
    EQUI_REFUSE(H < 2 || W < 2, "eamm_equi_tps_warp_frame: H and W must be at least 2 (the coordinate grid divides by n - 1)");
    EQUI_REFUSE(!op_count_ok(B, C, H, W) || B > OP_GRID_YZ,
                "eamm_equi_tps_warp_frame: B must be 1..65535 with fewer than 2^31 elements in the frame");
    EQUI_REFUSE(frame == out, "eamm_equi_tps_warp_frame: out must not be the frame (every pixel gathers from others)");
    OP_ENTRY(false, "");
    OP_DONE(tps_warp_frame_launch(frame, theta, control_params, points, B, C, H, W, out, s), "eamm_equi_tps_warp_frame");
}

int eamm_equi_tps_warp_points(int device, const float* coords, int coords_batch, const float* theta, const float* control_params, int points,
                              int B, int N, float* out, float* jac, void* stream_) {
    EQUI_REFUSE(!coords || !theta || !out, "eamm_equi_tps_warp_points: coords / theta / out is null");
    EQUI_REFUSE(!equi_points_ok(points), "eamm_equi_tps_warp_points: points must be 0 (affine only) or 2..16");
    EQUI_REFUSE(points && !control_params, "eamm_equi_tps_warp_points: control_params is null with points > 0");
    EQUI_REFUSE(!op_count_ok(B, N, 4), "eamm_equi_tps_warp_points: B and N must be positive with B * N * 4 below 2^31");
    EQUI_REFUSE(coords_batch != 1 && coords_batch != B, "eamm_equi_tps_warp_points: coords_batch must be 1 or B");
    OP_ENTRY(false, "");
    OP_DONE(tps_warp_points_launch(coords, coords_batch, theta, control_params, points, B, N, out, jac, s), "eamm_equi_tps_warp_points");
}

int eamm_equi_tps_warp_points_backward(int device, const float* coords, int coords_batch, const float* theta, const float* control_params,
                                       int points, int B, int N, const float* grad_out, const float* grad_jac, float* grad_coords,
                                       void* stream_) {
    EQUI_REFUSE(!coords || !theta || !grad_coords, "eamm_equi_tps_warp_points_backward: coords / theta / grad_coords is null");
    EQUI_REFUSE(!grad_out && !grad_jac, "eamm_equi_tps_warp_points_backward: grad_out and grad_jac are both null");
    EQUI_REFUSE(!equi_points_ok(points), "eamm_equi_tps_warp_points_backward: points must be 0 (affine only) or 2..16");
    EQUI_REFUSE(points && !control_params, "eamm_equi_tps_warp_points_backward: control_params is null with points > 0");
    EQUI_REFUSE(!op_count_ok(B, N, 4), "eamm_equi_tps_warp_points_backward: B and N must be positive with B * N * 4 below 2^31");
    EQUI_REFUSE(coords_batch != 1 && coords_batch != B, "eamm_equi_tps_warp_points_backward: coords_batch must be 1 or B");
    OP_ENTRY(false, "");
    OP_DONE(tps_warp_points_backward_launch(coords, coords_batch, theta, control_params, points, B, N, grad_out, grad_jac, grad_coords, s),
            "eamm_equi_tps_warp_points_backward");
}

}  // extern "C"
