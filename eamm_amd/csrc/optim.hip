// Adam over a list of tensors (torch.optim.Adam's update, the optimiser of every stage of the reference's train.py), fp32:
//     g' = g + weight_decay p                     (only when weight_decay != 0; L2 as torch.optim.Adam, not AdamW)
//     m  = lerp(m, g', 1 - beta1)                 (ATen's lerp: g' - (g' - m) beta1 where 1 - beta1 >= 0.5, else m + (1 - beta1)(g' - m))
//     v  = beta2 v + (1 - beta2) g' g'
//     p  = p - step_size m / (sqrt(v) / bc2_sqrt + eps)
// in torch's single-tensor order, with step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) per TENSOR.
//
// One pass reads p, g, m, v and writes p, m, v: 28 bytes per element, and nothing else to do -- a streaming kernel.  Geometry:
//   * a workgroup of 256 threads owns ONE chunk of one tensor (no grid stride: the tensors of a list run from one element to tens of
//     millions, and a chunk per workgroup lets the hardware balance them); the chunk is `mult` tiles of E = 4096 elements, mult = 1
//     unless the launch would exceed ADAM_GRID_CAP workgroups (adam_plan);
//   * a full tile is four float4 per thread and array: all sixteen loads are issued before the first result is needed;
//   * float4 accesses where all four addresses of the tensor are 16-byte aligned (a chunk starts a multiple of 4096 elements in, so the
//     tensor's alignment is every chunk's); a tensor with any address off that boundary, and the last 1..3 elements of a length that
//     is no multiple of four, take the scalar path;
//   * the tensor list arrives BY VALUE (AdamTable, kernels.h): the kernel arguments are read with scalar loads, and the workgroup's
//     tensor is found by a binary search over the prefix of workgroup counts, uniform over the workgroup.
// No LDS, no atomics: every element is computed by one thread from its own four values, so the result does not depend on the cut.
#include "kernels.h"

#include <algorithm>

namespace eamm {

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_VEC_PER_THREAD = ADAM_BLOCK_ELEMS / (4 * ADAM_THREADS);
static_assert(ADAM_VEC_PER_THREAD * 4 * ADAM_THREADS == ADAM_BLOCK_ELEMS, "a tile is whole float4 rounds of the workgroup");
static_assert(sizeof(AdamTable) + 6 * sizeof(float) <= 4096, "the table travels in the kernel arguments");

struct AdamScalars {
    float beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay, step_size, bc2_sqrt;
};

__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const AdamScalars& c) {
    if (c.weight_decay != 0.f) g = g + c.weight_decay * p;
    const float d = g - m;
    m = c.one_minus_beta1 < 0.5f ? m + c.one_minus_beta1 * d : g - d * c.beta1;   // beta1 = 1 - (1 - beta1), as ATen writes 1 - weight
    v = v * c.beta2 + c.one_minus_beta2 * g * g;
    const float denom = sqrtf(v) / c.bc2_sqrt + c.eps;
    p = p - c.step_size * (m / denom);
}

__device__ __forceinline__ void adam_vec(float4& p, const float4& g, float4& m, float4& v, const AdamScalars& c) {
    adam_element(p.x, g.x, m.x, v.x, c);
    adam_element(p.y, g.y, m.y, v.y, c);
    adam_element(p.z, g.z, m.z, v.z, c);
    adam_element(p.w, g.w, m.w, v.w, c);
}

}  // namespace

__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamTable t, float beta1, float one_minus_beta1, float beta2,
                                                         float one_minus_beta2, float eps, float weight_decay) {
    const int b = (int)blockIdx.x;
    // the tensor of workgroup b: the last i with first_block[i] <= b (a length-0 tensor repeats its neighbour's entry and is never found)
    int lo = 0, hi = t.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (t.first_block[mid] <= b) lo = mid;
        else hi = mid;
    }
    const int i = lo;
    const long long n = t.n[i];
    const long long begin = (long long)(b - t.first_block[i]) * t.chunk;
    if (begin >= n) return;                      // (never: the plan gives a tensor ceil(n / chunk) workgroups)
    const long long len = n - begin < t.chunk ? n - begin : (long long)t.chunk;
    float* __restrict__ p = t.p[i] + begin;
    const float* __restrict__ g = t.g[i] + begin;
    float* __restrict__ m = t.m[i] + begin;
    float* __restrict__ v = t.v[i] + begin;
    const AdamScalars c{beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay, t.step_size[i], t.bc2_sqrt[i]};
    const int tid = (int)threadIdx.x;
    const bool aligned = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
                           reinterpret_cast<uintptr_t>(v)) & 15) == 0;
    if (!aligned) {
        for (long long k = tid; k < len; k += ADAM_THREADS) {
            float pk = p[k], mk = m[k], vk = v[k];
            adam_element(pk, g[k], mk, vk, c);
            p[k] = pk;
            m[k] = mk;
            v[k] = vk;
        }
        return;
    }
    long long done = 0;
    for (; done + ADAM_BLOCK_ELEMS <= len; done += ADAM_BLOCK_ELEMS) {      // full tiles: sixteen loads in flight per thread
        float4* p4 = reinterpret_cast<float4*>(p + done);
        const float4* g4 = reinterpret_cast<const float4*>(g + done);
        float4* m4 = reinterpret_cast<float4*>(m + done);
        float4* v4 = reinterpret_cast<float4*>(v + done);
        float4 pr[ADAM_VEC_PER_THREAD], gr[ADAM_VEC_PER_THREAD], mr[ADAM_VEC_PER_THREAD], vr[ADAM_VEC_PER_THREAD];
#pragma unroll
        for (int r = 0; r < ADAM_VEC_PER_THREAD; ++r) {
            const int k = r * ADAM_THREADS + tid;
            pr[r] = p4[k];
            gr[r] = g4[k];
            mr[r] = m4[k];
            vr[r] = v4[k];
        }
#pragma unroll
        for (int r = 0; r < ADAM_VEC_PER_THREAD; ++r) {
            const int k = r * ADAM_THREADS + tid;
            adam_vec(pr[r], gr[r], mr[r], vr[r], c);
            p4[k] = pr[r];
            m4[k] = mr[r];
            v4[k] = vr[r];
        }
    }
    const long long rest = len - done;            // below one tile: whole float4 first, then 1..3 single elements
    const int nvec = (int)(rest >> 2);
    {
        float4* p4 = reinterpret_cast<float4*>(p + done);
        const float4* g4 = reinterpret_cast<const float4*>(g + done);
        float4* m4 = reinterpret_cast<float4*>(m + done);
        float4* v4 = reinterpret_cast<float4*>(v + done);
        for (int k = tid; k < nvec; k += ADAM_THREADS) {
            float4 pk = p4[k], mk = m4[k], vk = v4[k];
            adam_vec(pk, g4[k], mk, vk, c);
            p4[k] = pk;
            m4[k] = mk;
            v4[k] = vk;
        }
    }
    const long long k = done + 4ll * nvec + tid;
    if (k < len) {
        float pk = p[k], mk = m[k], vk = v[k];
        adam_element(pk, g[k], mk, vk, c);
        p[k] = pk;
        m[k] = mk;
        v[k] = vk;
    }
}

int adam_plan(int n, const long long* numel, AdamLaunch* launches, int cap) {
    int made = 0;
    for (int first = 0; first < n;) {
        const int count = std::min(ADAM_TABLE, n - first);
        long long tiles = 0;
        for (int i = first; i < first + count; ++i) tiles += (numel[i] + ADAM_BLOCK_ELEMS - 1) / ADAM_BLOCK_ELEMS;
        const long long mult = std::min<long long>(ADAM_MAX_MULT, std::max<long long>(1, (tiles + ADAM_GRID_CAP - 1) / ADAM_GRID_CAP));
        const long long chunk = mult * ADAM_BLOCK_ELEMS;
        long long blocks = 0;
        for (int i = first; i < first + count; ++i) blocks += (numel[i] + chunk - 1) / chunk;
        if (made < cap) launches[made] = AdamLaunch{first, count, (int)blocks, (int)chunk};
        ++made;
        first += count;
    }
    return made;
}

hipError_t adam_launch(const AdamTable& table, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                       float weight_decay, hipStream_t s) {
    const int blocks = table.first_block[table.count];
    if (blocks <= 0) return hipSuccess;
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)blocks), dim3(ADAM_THREADS), 0, s, table, beta1, one_minus_beta1, beta2,
                       one_minus_beta2, eps, weight_decay);
    return hipGetLastError();
}

}  // namespace eamm
