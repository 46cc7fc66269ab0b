// What the operator translation units share (eamm_op_conv.hip, eamm_op_train_conv.hip, eamm_op_train.hip, eamm_op_infer.hip,
// eamm_op_perceptual.hip, eamm_disc_api.hip, eamm_equi_api.hip; the
// eamm_op_*, eamm_disc_* and eamm_equi_* entries of include/eamm_hip.h): each entry runs ONE kernel family of the path -- or one operator of the differentiable
// training graph -- on caller-provided device buffers, without a handle.  Included by those files only.
#pragma once
#include "eamm_ctx.h"
#include <algorithm>
#include <mutex>

namespace {

// `iters` back-to-back run()s between two HIP events on `s`; *avg_ms gets their mean only when every step succeeded
template <typename Run>
hipError_t time_launches(hipStream_t s, int iters, float* avg_ms, Run run) {
    if (iters <= 0 || !avg_ms) return hipSuccess;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipEventRecord(e0, s);
    for (int i = 0; i < iters && e == hipSuccess; ++i) e = run();
    if (e == hipSuccess) e = hipEventRecord(e1, s);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
    if (e == hipSuccess) *avg_ms = ms / iters;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return e;
}

// An operator call's temporary device buffers (dev_alloc / upload): freed on every path, once the caller's stream is done
// with them.  Errors land in `err`; the entry hands them on to eamm_last_error(NULL).
struct OpBuffers : CtxBase {
    hipStream_t s;
    OpBuffers(int dev, hipStream_t st) : s(st) { device = dev; }
    ~OpBuffers() {
        if (owned.empty()) return;
        (void)hipStreamSynchronize(s);
        for (void* p : owned) (void)hipFree(p);
    }
};

constexpr int OP_GRID_YZ = 65535;   // a grid's y / z extent
bool op_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
bool op_count_ok(long long a, long long b, long long c = 1, long long d = 1) {   // positive factors, product below 2^31
    if (a < 1 || b < 1 || c < 1 || d < 1) return false;
    const long long lim = 1ll << 31;
    return a < lim && b < lim && c < lim && d < lim && a * b < lim && a * b * c < lim && a * b * c * d < lim;
}

// the caller's workspace: there, of at least `need` floats, and 16-byte aligned where the entry asks for that (the entries whose
// size query answers 0 for an unsupported shape refuse `need == 0` themselves)
bool op_workspace_ok(const float* workspace, size_t have, size_t need, bool aligned16) {
    return workspace && have >= need && (!aligned16 || op_aligned16(workspace));
}

// the register-staged implicit GEMM's layer for a filter that is packed on the device (w and bias: the caller's sections)
ConvLayer plain_conv_layer(int kh, int kw, int Cin, int Cout) {
    ConvLayer L;
    L.kh = kh;
    L.kw = kw;
    L.C0 = Cin;
    L.Cout = Cout;
    L.BN = conv_tile_n(Cout);
    L.ntiles = (Cout + L.BN - 1) / L.BN;
    L.nchunks = kh * kw * (Cin / CONV_BK);
    return L;
}

int op_done(hipError_t e, const char* name) {
    return e == hipSuccess ? EAMM_OK : fail(nullptr, EAMM_ERR_HIP, "%s failed: %s", name, hipGetErrorString(e));
}

}  // namespace

// The preamble and return of an eamm_op_* entry: argument check, the device made current for the call, the caller's stream; then the
// launch's status (evaluated once) as the entry's return
#define OP_ENTRY(cond, msg)                                                                      \
    if (cond) return fail(nullptr, EAMM_ERR_ARG, msg);                                           \
    DeviceGuard guard(device);                                                                   \
    if (guard.status != hipSuccess) return fail(nullptr, EAMM_ERR_HIP, "hipSetDevice failed");   \
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_)
#define OP_DONE(e, name) return op_done(e, name)
