// The equivariance constraint's random transform (reference modules/model.py:71-152, class Transform): an affine map theta [B,2,3]
// plus a thin-plate term on a P x P grid of control points with one weight per image and point,
//     out = theta[:, :2] c + theta[:, 2] + (r, r),   r = sum_p w[b,p] U(d_p),   d_p = |x - cx_p| + |y - cy_p|,   U(d) = d^2 log(d + 1e-6)
// (the L1 distance and ONE r for both components are the reference's).  P = 0: the affine map alone.
//   * tps_warp_frame_kernel           every output pixel warps its own grid point and samples all C planes there as
//                                     F.grid_sample(padding_mode='reflection') does (pointwise.h sample_pos_reflect): no grid tensor,
//                                     no [B, H W, P^2] distance tensor -- one read and one write of the frames.  blockIdx.y is the
//                                     image, so theta and the weights are wave-uniform loads.
//   * tps_warp_points_kernel          coords [Bc,N,2] (Bc = 1: one set for every image) -> out [B,N,2] and, where asked, the
//                                     jacobian d out / d c = theta[:, :2] + (g; g), g = sum_p w U'(d_p) sign(c - c_p): what autograd
//                                     gives the reference (sign(0) = 0 as torch.abs).
//   * tps_warp_points_backward_kernel grad_c[k] = sum_i gout[i] jac[i][k] + sum_ij gjac[i][j] Hs[j][k], Hs = sum_p w U''(d_p) s s^T:
//                                     the jacobian is differentiated again, as the reference's create_graph=True allows.  One
//                                     thread per coordinate; with Bc = 1 it adds the images' terms in index order.
// logf, not the fast intrinsic; sums over p ascending; no atomics: the same bits from run to run.
#include "pointwise.h"

namespace eamm {

namespace {

constexpr int TPS_THREADS = 256;
constexpr float TPS_EPS = 1e-6f;

// U, U', U'' of d >= 0 (log(d + eps) is finite at d = 0, and every term that multiplies it is zero there)
__device__ __forceinline__ float tps_u(float d) { return d * d * logf(d + TPS_EPS); }
__device__ __forceinline__ void tps_u12(float d, float& u1, float& u2, bool second) {
    const float e = d + TPS_EPS, l = logf(e);
    u1 = 2.f * d * l + d * d / e;
    u2 = 0.f;
    if (second) u2 = 2.f * l + 2.f * d / e + (d * d + 2.f * d * TPS_EPS) / (e * e);
}
__device__ __forceinline__ float sign0(float v) { return v > 0.f ? 1.f : (v < 0.f ? -1.f : 0.f); }

// r of the point (x, y) under the weights w[P * P], control points row-major on the P x P coordinate grid
__device__ __forceinline__ float tps_value(const float* __restrict__ w, int P, float x, float y) {
    float r = 0.f;
    for (int py = 0; py < P; ++py) {
        const float dy = fabsf(y - grid_coord(py, P));
        for (int px = 0; px < P; ++px) r += tps_u(fabsf(x - grid_coord(px, P)) + dy) * w[py * P + px];
    }
    return r;
}

}  // namespace

__global__ __launch_bounds__(256) void tps_warp_frame_kernel(const float* __restrict__ frame, const float* __restrict__ theta,
                                                             const float* __restrict__ params, int P, int C, int H, int W,
                                                             float* __restrict__ out) {
    const int b = blockIdx.y;
    const int pix = blockIdx.x * TPS_THREADS + threadIdx.x;
    const float* t = theta + b * 6;
    const float t00 = t[0], t01 = t[1], t02 = t[2], t10 = t[3], t11 = t[4], t12 = t[5];
    if (pix >= H * W) return;
    const int j = pix % W, i = pix / W;
    const float x = grid_coord(j, W), y = grid_coord(i, H);
    float gx = fmaf(t01, y, t00 * x) + t02, gy = fmaf(t11, y, t10 * x) + t12;
    if (P) {
        const float r = tps_value(params + (size_t)b * P * P, P, x, y);
        gx += r;
        gy += r;
    }
    const SamplePos p = sample_pos_reflect(gx, gy, W, H);
    const bool east = p.x0 + 1 < W, south = p.y0 + 1 < H;
    const float wnw = (1.f - p.ax) * (1.f - p.ay), wne = p.ax * (1.f - p.ay), wsw = (1.f - p.ax) * p.ay, wse = p.ax * p.ay;
    const size_t plane = (size_t)H * W, at = (size_t)p.y0 * W + p.x0;
    for (int c = 0; c < C; ++c) {
        const float* src = frame + ((size_t)b * C + c) * plane + at;
        float v = src[0] * wnw;
        if (east) v += src[1] * wne;
        if (south) v += src[W] * wsw;
        if (east && south) v += src[W + 1] * wse;
        out[((size_t)b * C + c) * plane + pix] = v;
    }
}

__global__ __launch_bounds__(256) void tps_warp_points_kernel(const float* __restrict__ coords, int Bc, const float* __restrict__ theta,
                                                              const float* __restrict__ params, int P, int B, int N,
                                                              float* __restrict__ out, float* __restrict__ jac) {
    const int idx = blockIdx.x * TPS_THREADS + threadIdx.x;
    if (idx >= B * N) return;
    const int b = idx / N, n = idx - b * N;
    const float* c = coords + 2 * (size_t)(Bc == 1 ? n : idx);
    const float x = c[0], y = c[1];
    const float* t = theta + b * 6;
    const float* w = params + (size_t)b * P * P;
    float r = 0.f, g0 = 0.f, g1 = 0.f;
    for (int py = 0; py < P; ++py) {
        const float ey = y - grid_coord(py, P);
        for (int px = 0; px < P; ++px) {
            const float ex = x - grid_coord(px, P), d = fabsf(ex) + fabsf(ey), wp = w[py * P + px];
            r += tps_u(d) * wp;
            if (jac) {
                float u1, u2;
                tps_u12(d, u1, u2, false);
                g0 += wp * u1 * sign0(ex);
                g1 += wp * u1 * sign0(ey);
            }
        }
    }
    out[2 * (size_t)idx] = fmaf(t[1], y, t[0] * x) + t[2] + r;
    out[2 * (size_t)idx + 1] = fmaf(t[4], y, t[3] * x) + t[5] + r;
    if (jac) {
        float* q = jac + 4 * (size_t)idx;
        q[0] = t[0] + g0;
        q[1] = t[1] + g1;
        q[2] = t[3] + g0;
        q[3] = t[4] + g1;
    }
}

__global__ __launch_bounds__(256) void tps_warp_points_backward_kernel(const float* __restrict__ coords, int Bc,
                                                                       const float* __restrict__ theta, const float* __restrict__ params,
                                                                       int P, int B, int N, const float* __restrict__ gout,
                                                                       const float* __restrict__ gjac, float* __restrict__ gcoords) {
    const int idx = blockIdx.x * TPS_THREADS + threadIdx.x;
    if (idx >= Bc * N) return;
    const int n = idx % N;
    const float x = coords[2 * (size_t)idx], y = coords[2 * (size_t)idx + 1];
    const int b_lo = Bc == 1 ? 0 : idx / N, b_hi = Bc == 1 ? B : b_lo + 1;
    float acc0 = 0.f, acc1 = 0.f;
    for (int b = b_lo; b < b_hi; ++b) {
        const float* t = theta + b * 6;
        const float* w = params + (size_t)b * P * P;
        const size_t at = (size_t)b * N + n;
        float g0 = 0.f, g1 = 0.f, hxx = 0.f, hxy = 0.f, hyy = 0.f;
        for (int py = 0; py < P; ++py) {
            const float ey = y - grid_coord(py, P), sy = sign0(ey);
            for (int px = 0; px < P; ++px) {
                const float ex = x - grid_coord(px, P), sx = sign0(ex), wp = w[py * P + px];
                float u1, u2;
                tps_u12(fabsf(ex) + fabsf(ey), u1, u2, gjac != nullptr);
                g0 += wp * u1 * sx;
                g1 += wp * u1 * sy;
                hxx += wp * u2 * sx * sx;
                hxy += wp * u2 * sx * sy;
                hyy += wp * u2 * sy * sy;
            }
        }
        float d0 = 0.f, d1 = 0.f;
        if (gout) {
            const float o0 = gout[2 * at], o1 = gout[2 * at + 1];
            d0 = o0 * (t[0] + g0) + o1 * (t[3] + g0);
            d1 = o0 * (t[1] + g1) + o1 * (t[4] + g1);
        }
        if (gjac) {
            const float* q = gjac + 4 * at;
            const float G0 = q[0] + q[2], G1 = q[1] + q[3];      // sum over i of gjac[i][j]
            d0 += G0 * hxx + G1 * hxy;
            d1 += G0 * hxy + G1 * hyy;
        }
        acc0 += d0;
        acc1 += d1;
    }
    gcoords[2 * (size_t)idx] = acc0;
    gcoords[2 * (size_t)idx + 1] = acc1;
}

hipError_t tps_warp_frame_launch(const float* frame, const float* theta, const float* params, int P, int B, int C, int H, int W, float* out,
                                 hipStream_t s) {
    const dim3 grid((unsigned)((H * W + TPS_THREADS - 1) / TPS_THREADS), (unsigned)B);
    hipLaunchKernelGGL(tps_warp_frame_kernel, grid, dim3(TPS_THREADS), 0, s, frame, theta, params, P, C, H, W, out);
    return hipGetLastError();
}

hipError_t tps_warp_points_launch(const float* coords, int Bc, const float* theta, const float* params, int P, int B, int N, float* out,
                                  float* jac, hipStream_t s) {
    hipLaunchKernelGGL(tps_warp_points_kernel, dim3((unsigned)((B * N + TPS_THREADS - 1) / TPS_THREADS)), dim3(TPS_THREADS), 0, s, coords, Bc,
                       theta, params, P, B, N, out, jac);
    return hipGetLastError();
}

hipError_t tps_warp_points_backward_launch(const float* coords, int Bc, const float* theta, const float* params, int P, int B, int N,
                                           const float* gout, const float* gjac, float* gcoords, hipStream_t s) {
    hipLaunchKernelGGL(tps_warp_points_backward_kernel, dim3((unsigned)((Bc * N + TPS_THREADS - 1) / TPS_THREADS)), dim3(TPS_THREADS), 0, s,
                       coords, Bc, theta, params, P, B, N, gout, gjac, gcoords);
    return hipGetLastError();
}

}  // namespace eamm
