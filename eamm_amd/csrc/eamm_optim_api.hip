// The optimiser step as entries of their own family, eamm_optim_* (include/eamm_hip.h; kernel in optim.hip): Adam over a list of
// tensors.  The operator convention: device index first, stream last, errors through eamm_last_error(NULL); every refusal names its
// entry and its reason, and comes before anything touches a device.  eamm_optim_adam allocates nothing, synchronises nothing and reads
// nothing back: the host arrays are copied into the launches' kernel arguments and may be freed as soon as it returns.
#include "op_common.h"

namespace {

#define OPTIM_REFUSE(cond, ...) \
    if (cond) return fail(nullptr, EAMM_ERR_ARG, __VA_ARGS__)

bool optim_aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

int optim_check_lengths(const char* entry, int n, const long long* numel) {
    OPTIM_REFUSE(n < 0, "%s: n = %d tensors", entry, n);
    OPTIM_REFUSE(!numel, "%s: numel is null", entry);
    for (int i = 0; i < n; ++i)
        OPTIM_REFUSE(numel[i] < 0 || numel[i] > ADAM_MAX_NUMEL, "%s: numel[%d] = %lld is not in 0 .. 2^36", entry, i, numel[i]);
    return EAMM_OK;
}

}  // namespace

extern "C" {

int eamm_optim_adam_table_capacity(void) { return ADAM_TABLE; }
int eamm_optim_adam_block_elems(void) { return ADAM_BLOCK_ELEMS; }

int eamm_optim_adam_plan(int n, const long long* numel, int max_launches, int* launch_first, int* launch_count, int* launch_blocks,
                         long long* elems_per_block) {
    if (int rc = optim_check_lengths("eamm_optim_adam_plan", n, numel)) return rc;
    OPTIM_REFUSE(max_launches < 0, "eamm_optim_adam_plan: max_launches = %d", max_launches);
    OPTIM_REFUSE(max_launches > 0 && (!launch_first || !launch_count || !launch_blocks),
                 "eamm_optim_adam_plan: launch_first / launch_count / launch_blocks is null with max_launches > 0");
    std::vector<AdamLaunch> launches((size_t)max_launches);
    const int need = adam_plan(n, numel, launches.data(), max_launches);
    for (int l = 0; l < std::min(need, max_launches); ++l) {
        launch_first[l] = launches[l].first;
        launch_count[l] = launches[l].count;
        launch_blocks[l] = launches[l].blocks;
        if (elems_per_block)
            for (int i = launches[l].first; i < launches[l].first + launches[l].count; ++i) elems_per_block[i] = numel[i] ? launches[l].chunk : 0;
    }
    return need;
}

int eamm_optim_adam(int device, int n, float* const* p, const float* const* g, float* const* m, float* const* v, const long long* numel,
                    const float* step_size, const float* bc2_sqrt, double beta1, double beta2, double eps, double weight_decay,
                    void* stream_) {
    OPTIM_REFUSE(!p || !g || !m || !v || !step_size || !bc2_sqrt, "eamm_optim_adam: p / g / m / v / step_size / bc2_sqrt is null");
    if (int rc = optim_check_lengths("eamm_optim_adam", n, numel)) return rc;
    OPTIM_REFUSE(!std::isfinite(beta1) || !std::isfinite(beta2) || !std::isfinite(eps) || !std::isfinite(weight_decay),
                 "eamm_optim_adam: beta1 / beta2 / eps / weight_decay is not finite");
    OPTIM_REFUSE(beta1 < 0 || beta1 >= 1 || beta2 < 0 || beta2 >= 1 || eps < 0 || weight_decay < 0,
                 "eamm_optim_adam: beta1 and beta2 must be in [0, 1), eps and weight_decay not negative");
    for (int i = 0; i < n; ++i) {
        if (numel[i] == 0) continue;
        OPTIM_REFUSE(!p[i] || !g[i] || !m[i] || !v[i], "eamm_optim_adam: tensor %d has a null address and %lld elements", i, numel[i]);
        OPTIM_REFUSE(!optim_aligned4(p[i]) || !optim_aligned4(g[i]) || !optim_aligned4(m[i]) || !optim_aligned4(v[i]),
                     "eamm_optim_adam: tensor %d has an address that is not 4-byte aligned", i);
        OPTIM_REFUSE(!std::isfinite(step_size[i]) || !std::isfinite(bc2_sqrt[i]) || !(bc2_sqrt[i] > 0.f),
                     "eamm_optim_adam: step_size[%d] / bc2_sqrt[%d] is not finite, or bc2_sqrt is not positive", i, i);
    }
    OP_ENTRY(false, "");
    // the weights as ATen's scalar kernels see them: the Python float rounded to fp32 once (lerp's 1 - weight is taken in fp32)
    const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2);
    AdamLaunch launches[16];
    AdamTable table;
    for (int first = 0; first < n;) {     // the plan, sixteen launches at a time
        const int made = std::min(16, adam_plan(n - first, numel + first, launches, 16));
        for (int l = 0; l < made; ++l) {
            const AdamLaunch& L = launches[l];
            int blocks = 0;
            for (int k = 0; k <= ADAM_TABLE; ++k) {
                if (k < L.count) {
                    const int i = first + L.first + k;
                    table.p[k] = p[i];
                    table.g[k] = g[i];
                    table.m[k] = m[i];
                    table.v[k] = v[i];
                    table.n[k] = numel[i];
                    table.step_size[k] = step_size[i];
                    table.bc2_sqrt[k] = bc2_sqrt[i];
                } else if (k < ADAM_TABLE) {
                    table.p[k] = table.m[k] = table.v[k] = nullptr;
                    table.g[k] = nullptr;
                    table.n[k] = 0;
                    table.step_size[k] = 0.f;
                    table.bc2_sqrt[k] = 1.f;
                }
                table.first_block[k] = blocks;
                if (k < L.count) blocks += (int)((numel[first + L.first + k] + L.chunk - 1) / L.chunk);
            }
            table.count = L.count;
            table.chunk = L.chunk;
            if (const hipError_t e = adam_launch(table, 1.f - omb1, omb1, (float)beta2, omb2, (float)eps, (float)weight_decay, s))
                return op_done(e, "eamm_optim_adam");
        }
        first += launches[made - 1].first + launches[made - 1].count;
    }
    return EAMM_OK;
}

}  // extern "C"
