// the Adam step of many tensors in one launch (fp32, in place).
//
// The trainer ends every step with `self.optimizer.step()` on two torch.optim.Adam objects that hold one parameter group per tensor
// (6 for the scene, 9 groups / 36 tensors for the human): about a dozen elementwise launches per group, each a pass over the group's
// memory.  Here the per-tensor records -- four pointers, a length and six scalars -- travel BY VALUE in the kernel argument, next to a
// prefix array of chunk counts: no device allocation, no copy, no event, nothing to wait for.  One workgroup takes one chunk of
// ADAM_CHUNK elements of one tensor; it finds its tensor by a search over the prefix array on blockIdx.x, which is wave-uniform, so the
// search and the record's fetch run on the scalar unit.  A tensor whose four pointers are 16-byte aligned moves as float4 (every chunk
// starts a multiple of 16 bytes into its tensor); any other -- a view at an odd element offset: 4-byte alignment is all torch
// guarantees -- moves element by element.  Either way a thread first issues all its loads, then computes, then stores: each element is
// read once (p, g, m, v) and written once (p, m, v), 28 bytes, and the kernel is judged against the copy rate.
//
// Arithmetic: the library is built with -ffp-contract=off and correctly rounded divide / sqrt, so adam_one() does what it spells.
#include <math.h>

#include "hgs_common.h"

namespace {

constexpr int ADAM_TENSORS = 56;                         // records per launch
constexpr int ADAM_PREFIX = 64;                          // prefix entries: a power of two above ADAM_TENSORS (the search takes 6 fixed steps)
constexpr int ADAM_THREADS = 256, ADAM_UNROLL = 4;
constexpr int ADAM_CHUNK = ADAM_THREADS * 4 * ADAM_UNROLL;   // elements per workgroup: 4 096 (112 KB of traffic)
// blocks per launch: the grid's thread count stays below 2^32
constexpr uint32_t ADAM_MAX_BLOCKS = (1u << 24) - 1u;

struct AdamTable {
    hgs_adam_tensor t[ADAM_TENSORS];
    // prefix[i] = chunks of the tensors before i; prefix[count] = the grid; entries behind that 0xFFFFFFFF
    uint32_t prefix[ADAM_PREFIX];
};
static_assert(sizeof(hgs_adam_tensor) == 64, "hgs_adam_tensor layout");
static_assert(sizeof(AdamTable) <= 4096, "the table must fit a 4 KB kernel argument");
static_assert(ADAM_TENSORS >= 48 && ADAM_TENSORS < ADAM_PREFIX && (ADAM_PREFIX & (ADAM_PREFIX - 1)) == 0, "table sizes");

struct AdamScalars {
    float w1, b2, w2, eps, step, bc2;
};

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamScalars& s)
{
    m = m + (g - m) * s.w1;
    v = v * s.b2 + s.w2 * g * g;
    p = p - s.step * (m / (sqrtf(v) / s.bc2 + s.eps));
}

__global__ void __launch_bounds__(ADAM_THREADS) adam_multi_tensor_kernel(const AdamTable tab)
{
    const uint32_t b = blockIdx.x;
    // the last i with prefix[i] <= b (prefix[0] = 0, non-decreasing, the unused tail is 0xFFFFFFFF)
    uint32_t ti = 0;
#pragma unroll
    for (uint32_t s = ADAM_PREFIX / 2; s; s >>= 1)
        if (tab.prefix[ti + s] <= b) ti += s;
    ti = ti < (uint32_t)ADAM_TENSORS ? ti : 0u;   // (never taken on a table the host built: keeps the record fetch in bounds)
    const hgs_adam_tensor& r = tab.t[ti];
    const AdamScalars sc = {r.one_minus_beta1, r.beta2, r.one_minus_beta2, r.eps, r.step_size, r.bc2_sqrt};
    const size_t start = (size_t)(b - tab.prefix[ti]) * ADAM_CHUNK;
    if ((int64_t)start >= r.numel) return;
    const size_t left = (size_t)r.numel - start;
    const uint32_t n = left < (size_t)ADAM_CHUNK ? (uint32_t)left : (uint32_t)ADAM_CHUNK;   // elements of this chunk
    float* const p = r.param + start;
    const float* const g = r.grad + start;
    float* const m = r.exp_avg + start;
    float* const v = r.exp_avg_sq + start;
    const uint32_t tid = threadIdx.x;

    if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
        const uint32_t nv = n >> 2;   // whole float4s
        float4* const p4 = reinterpret_cast<float4*>(p);
        const float4* const g4 = reinterpret_cast<const float4*>(g);
        float4* const m4 = reinterpret_cast<float4*>(m);
        float4* const v4 = reinterpret_cast<float4*>(v);
        float4 P[ADAM_UNROLL], G[ADAM_UNROLL], M[ADAM_UNROLL], V[ADAM_UNROLL];
#pragma unroll
        for (int k = 0; k < ADAM_UNROLL; ++k) {
            const uint32_t i = tid + k * ADAM_THREADS;
            if (i < nv) P[k] = p4[i], G[k] = g4[i], M[k] = m4[i], V[k] = v4[i];
        }
#pragma unroll
        for (int k = 0; k < ADAM_UNROLL; ++k) {
            const uint32_t i = tid + k * ADAM_THREADS;
            if (i < nv) {
                adam_one(P[k].x, G[k].x, M[k].x, V[k].x, sc);
                adam_one(P[k].y, G[k].y, M[k].y, V[k].y, sc);
                adam_one(P[k].z, G[k].z, M[k].z, V[k].z, sc);
                adam_one(P[k].w, G[k].w, M[k].w, V[k].w, sc);
                p4[i] = P[k], m4[i] = M[k], v4[i] = V[k];
            }
        }
        const uint32_t i = (nv << 2) + tid;   // the tensor's last one to three elements
        if (i < n) {
            float pp = p[i], mm = m[i], vv = v[i];
            adam_one(pp, g[i], mm, vv, sc);
            p[i] = pp, m[i] = mm, v[i] = vv;
        }
    } else {
        constexpr int E = 4 * ADAM_UNROLL;
#pragma unroll
        for (int h = 0; h < E; h += ADAM_UNROLL) {
            float P[ADAM_UNROLL], G[ADAM_UNROLL], M[ADAM_UNROLL], V[ADAM_UNROLL];
#pragma unroll
            for (int k = 0; k < ADAM_UNROLL; ++k) {
                const uint32_t i = tid + (h + k) * ADAM_THREADS;
                if (i < n) P[k] = p[i], G[k] = g[i], M[k] = m[i], V[k] = v[i];
            }
#pragma unroll
            for (int k = 0; k < ADAM_UNROLL; ++k) {
                const uint32_t i = tid + (h + k) * ADAM_THREADS;
                if (i < n) {
                    adam_one(P[k], G[k], M[k], V[k], sc);
                    p[i] = P[k], m[i] = M[k], v[i] = V[k];
                }
            }
        }
    }
}

int fail_adam(const char* what)
{
    hgs::set_last_error(what);
    return HGS_ERR_INVALID_ARGUMENT;
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

extern "C" void hgs_adam_limits(int32_t* tensors_per_launch, int32_t* chunk_elems)
{
    if (tensors_per_launch) *tensors_per_launch = ADAM_TENSORS;
    if (chunk_elems) *chunk_elems = ADAM_CHUNK;
}

extern "C" int32_t hgs_adam_step(const hgs_adam_tensor* tensors, int32_t n, void* stream)
{
    if (n < 0) return fail_adam("adam_step: n < 0");
    if (n == 0) return HGS_OK;
    if (!tensors) return fail_adam("adam_step: null `tensors`");
    for (int32_t i = 0; i < n; ++i) {
        const hgs_adam_tensor& t = tensors[i];
        if (t.numel < 0) return fail_adam("adam_step: numel < 0");
        if (!isfinite(t.one_minus_beta1) || !isfinite(t.beta2) || !isfinite(t.one_minus_beta2) || !isfinite(t.eps) || !isfinite(t.step_size) ||
            !isfinite(t.bc2_sqrt))
            return fail_adam("adam_step: non-finite scalar (one_minus_beta1, beta2, one_minus_beta2, eps, step_size or bc2_sqrt)");
        if (!(t.bc2_sqrt > 0.0f)) return fail_adam("adam_step: bc2_sqrt <= 0");
        if (t.numel == 0) continue;
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) return fail_adam("adam_step: null pointer (param, grad, exp_avg or exp_avg_sq)");
        if (!aligned4(t.param) || !aligned4(t.grad) || !aligned4(t.exp_avg) || !aligned4(t.exp_avg_sq))
            return fail_adam("adam_step: pointer not 4-byte aligned");
        if (((uint64_t)t.numel + ADAM_CHUNK - 1) / ADAM_CHUNK > ADAM_MAX_BLOCKS) return fail_adam("adam_step: numel beyond one launch's grid (2^36 elements)");
    }
    AdamTable tab;
    int32_t i = 0;
    while (i < n) {
        int count = 0;
        uint32_t blocks = 0;
        for (; i < n && count < ADAM_TENSORS; ++i) {
            if (tensors[i].numel == 0) continue;
            const uint32_t chunks = (uint32_t)(((uint64_t)tensors[i].numel + ADAM_CHUNK - 1) / ADAM_CHUNK);
            if (count && chunks > ADAM_MAX_BLOCKS - blocks) break;   // the grid is full: this tensor opens the next launch
            tab.t[count] = tensors[i];
            tab.prefix[count] = blocks;
            blocks += chunks;
            ++count;
        }
        if (!count) break;   // only empty tensors were left
        tab.prefix[count] = blocks;
        for (int k = count + 1; k < ADAM_PREFIX; ++k) tab.prefix[k] = 0xFFFFFFFFu;
        for (int k = count; k < ADAM_TENSORS; ++k) tab.t[k] = tab.t[0];   // (never read: defined bytes in the argument)
        hipLaunchKernelGGL(adam_multi_tensor_kernel, dim3(blocks), dim3(ADAM_THREADS), 0, (hipStream_t)stream, tab);
        if (hipGetLastError() != hipSuccess) {
            hgs::set_last_error("adam_step: kernel launch failed");
            return HGS_ERR_HIP;
        }
    }
    return HGS_OK;
}
