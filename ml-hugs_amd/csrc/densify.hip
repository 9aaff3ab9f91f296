// the trainer-side consumers of the rasterizer's outputs, fused.
// The reference runs, every training step, four boolean-indexed torch ops
//   max_radii2D[vis] = max(max_radii2D[vis], radii[vis])                     gs_trainer.py:407-410 / 430-433
//   xyz_gradient_accum[vis] += || viewspace_points.grad[:n][vis, :2] ||      scene.py:460-462 / hugs_trimlp.py:880-882
//   denom[vis] += 1
// (each a gather + scatter with a host-visible nonzero()); here it is one pass over the n Gaussians.
#include <cstdio>

#include "hgs_common.h"

namespace {
__global__ void __launch_bounds__(256)
densification_stats_kernel(int n, const float* __restrict__ grad2d /*[>=n,3]*/, const int32_t* __restrict__ radii,
                           const uint8_t* __restrict__ visible, float* __restrict__ max_radii2D,
                           float* __restrict__ xyz_gradient_accum, float* __restrict__ denom)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !visible[i]) return;
    max_radii2D[i] = fmaxf(max_radii2D[i], (float)radii[i]);
    const float gx = grad2d[3 * (size_t)i], gy = grad2d[3 * (size_t)i + 1];
    xyz_gradient_accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.0f;
}
}  // namespace

extern "C" int32_t hgs_densification_stats(int32_t n, const float* viewspace_grad, const int32_t* radii,
                                           const uint8_t* visibility_filter, float* max_radii2D,
                                           float* xyz_gradient_accum, float* denom, void* stream)
{
    if (n < 0 || (n > 0 && (!viewspace_grad || !radii || !visibility_filter || !max_radii2D || !xyz_gradient_accum || !denom)))
    {
        hgs::set_last_error("densification_stats: n must be >= 0 and all six arrays non-null");
        return HGS_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return HGS_OK;
    hipLaunchKernelGGL(densification_stats_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, viewspace_grad,
                       radii, visibility_filter, max_radii2D, xyz_gradient_accum, denom);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        char msg[256];
        snprintf(msg, sizeof msg, "densification_stats: %s", hipGetErrorString(e));
        hgs::set_last_error(msg);
        return HGS_ERR_HIP;
    }
    return HGS_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the densification round itself (clone, split, prune) as a stream compaction.
//
// The reference runs `densify_and_prune` (scene.py:441-458, hugs_trimlp.py:857-878) as clone -> cat, split -> cat -> prune, prune:
// three cats and two boolean-index prunes over every parameter, both Adam moments and the statistics.  The final row list is a pure
// function of per-source-row predicates (the header spells them out), so here a round is
//   densify_classify_kernel   one pass over the predicates' inputs: a kind byte per row, four counts per workgroup of DR_ROWS rows
//   densify_partials_kernel   ONE workgroup turns the per-workgroup counts into exclusive prefixes and writes the five totals
//   (the host reads the totals back and allocates the results)
//   densify_scatter_kernel    grid (row blocks, tensors): a workgroup rebuilds its rows' destinations in LDS from the kind bytes and its
//                             prefix -- an in-block rescan, nothing per row is stored between the passes -- and then walks the flat
//                             elements of its DR_ROWS x width slab: the read is contiguous, the writes are contiguous wherever
//                             neighbouring rows survive (row widths 1, 3, 4, 9, 45: dword accesses throughout)
// No workgroup ever waits for another one: the scan's only cross-workgroup step is the single-workgroup launch in the middle.
namespace {

constexpr int DR_THREADS = 256, DR_PER_THREAD = 4;
constexpr int DR_ROWS = DR_THREADS * DR_PER_THREAD;   // rows per workgroup of the classify and scatter passes: 1 024
constexpr int DR_TENSORS = 32;                        // records per scatter launch (768 bytes of kernel argument)
constexpr int DR_MAX_LAUNCHES = 16;
constexpr int DR_MAX_WIDTH = 1024;                    // the reciprocal row index below is exact while DR_ROWS * width^2 < 2^32
constexpr uint32_t DR_NONE = 0xFFFFFFFFu;
enum : uint32_t { K_KEEP = 1, K_CLONE = 2, K_SPLIT = 4, K_SELECTED = 8 };
static_assert(sizeof(hgs_densify_tensor) == 24, "hgs_densify_tensor layout");
static_assert((uint64_t)DR_ROWS * DR_MAX_WIDTH * DR_MAX_WIDTH < (1ull << 32), "row index by reciprocal");
static_assert(DR_ROWS < 65536, "four 16-bit counts in one 64-bit word");

struct U4 {
    uint32_t keep, clone, split, sel;
};
__device__ __forceinline__ U4 operator+(U4 a, U4 b) { return {a.keep + b.keep, a.clone + b.clone, a.split + b.split, a.sel + b.sel}; }

// the four counts of up to DR_ROWS rows, 16 bits each
__device__ __forceinline__ uint64_t pack_kind(uint32_t k)
{
    return (uint64_t)(k & 1u) | ((uint64_t)((k >> 1) & 1u) << 16) | ((uint64_t)((k >> 2) & 1u) << 32) | ((uint64_t)((k >> 3) & 1u) << 48);
}
__device__ __forceinline__ U4 unpack(uint64_t p)
{
    return {(uint32_t)(p & 0xFFFF), (uint32_t)((p >> 16) & 0xFFFF), (uint32_t)((p >> 32) & 0xFFFF), (uint32_t)(p >> 48)};
}

// Exclusive prefix of v over the workgroup's DR_THREADS threads (Hillis-Steele in LDS), the workgroup's sum in `total`.
// Every thread of the workgroup calls it; `lds` holds DR_THREADS values and is free again on return.
template <class T>
__device__ __forceinline__ T block_scan_exclusive(T v, T* lds, T zero, T& total)
{
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
#pragma unroll
    for (int d = 1; d < DR_THREADS; d <<= 1) {
        T x = lds[t];
        if (t >= d) x = x + lds[t - d];
        __syncthreads();
        lds[t] = x;
        __syncthreads();
    }
    total = lds[DR_THREADS - 1];
    const T before = t ? lds[t - 1] : zero;
    __syncthreads();
    return before;
}

struct PlanArgs {
    int32_t n, densify, use_screen;
    float max_grad, min_opacity, small_max, max_screen_size, big_max;
};

template <int FLAVOUR>
__device__ __forceinline__ uint32_t classify_row(const PlanArgs& a, float accum, float den, float radius, float s0, float s1, float s2, float op)
{
    float g = accum / den;
    if (g != g) g = 0.0f;
    if (FLAVOUR == HGS_DENSIFY_SCENE) {
        s0 = expf(s0), s1 = expf(s1), s2 = expf(s2);
        op = 1.0f / (1.0f + expf(-op));
    }
    const float m = fmaxf(fmaxf(s0, s1), s2);
    const bool low = op < a.min_opacity;
    if (!a.densify) {
        const bool gone = low || (a.use_screen && (radius > a.max_screen_size || m > a.big_max));
        return gone ? 0u : K_KEEP;
    }
    const bool small = m <= a.small_max;
    const bool clone = fabsf(g) >= a.max_grad && small;
    bool split = g >= a.max_grad && !small;
    if (FLAVOUR == HGS_DENSIFY_HUMAN) {
        const float med = fmaxf(fminf(s0, s1), fminf(fmaxf(s0, s1), s2));   // the middle one of three
        split = split && ((s0 - med) / med >= 1.0f || (s1 - med) / med >= 1.0f || (s2 - med) / med >= 1.0f);
    }
    // (the statistics were reset by the clone's and the split's postfix: max_radii2D is 0 at prune time)
    const bool screen0 = a.use_screen && 0.0f > a.max_screen_size;
    const bool gone = low || screen0 || (a.use_screen && m > a.big_max);
    uint32_t k = 0;
    if (!split && !gone) k |= K_KEEP;
    if (clone && !gone) k |= K_CLONE;
    if (split) {
        k |= K_SELECTED;
        float m2 = m;   // human: scales_tmp of a copy is the source row's
        if (FLAVOUR == HGS_DENSIFY_SCENE) m2 = fmaxf(fmaxf(expf(logf(s0 / 1.6f)), expf(logf(s1 / 1.6f))), expf(logf(s2 / 1.6f)));
        if (!(low || screen0 || (a.use_screen && m2 > a.big_max))) k |= K_SPLIT;
    }
    return k;
}

template <int FLAVOUR>
__global__ void __launch_bounds__(DR_THREADS)
densify_classify_kernel(const PlanArgs a, const float* __restrict__ accum, const float* __restrict__ denom, const float* __restrict__ radii,
                        const float* __restrict__ scales, const float* __restrict__ opacity, uint8_t* __restrict__ kind, U4* __restrict__ partials)
{
    __shared__ uint64_t lds[DR_THREADS];
    const uint32_t row0 = blockIdx.x * (uint32_t)DR_ROWS + threadIdx.x * DR_PER_THREAD;
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < DR_PER_THREAD; ++j) {
        const uint32_t i = row0 + j;
        if (i < (uint32_t)a.n) {
            const uint32_t k = classify_row<FLAVOUR>(a, accum[i], denom[i], radii[i], scales[3 * (size_t)i], scales[3 * (size_t)i + 1],
                                                     scales[3 * (size_t)i + 2], opacity[i]);
            kind[i] = (uint8_t)k;
            sum += pack_kind(k);
        }
    }
    uint64_t total;
    block_scan_exclusive<uint64_t>(sum, lds, 0ull, total);
    if (threadIdx.x == 0) partials[blockIdx.x] = unpack(total);
}

// counts per workgroup -> exclusive prefixes, in place; totals[5].  One workgroup walks the array DR_THREADS entries at a time.
__global__ void __launch_bounds__(DR_THREADS) densify_partials_kernel(uint32_t blocks, U4* __restrict__ partials, uint32_t* __restrict__ totals)
{
    __shared__ U4 lds[DR_THREADS];
    const U4 zero = {0, 0, 0, 0};
    U4 carry = zero;
    for (uint32_t base = 0; base < blocks; base += DR_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const U4 v = i < blocks ? partials[i] : zero;
        U4 total;
        const U4 before = block_scan_exclusive<U4>(v, lds, zero, total);
        if (i < blocks) partials[i] = carry + before;
        carry = carry + total;
    }
    if (threadIdx.x == 0) {
        totals[0] = carry.keep, totals[1] = carry.clone, totals[2] = carry.split, totals[3] = carry.split, totals[4] = carry.sel;
    }
}

struct ScatterTable {
    hgs_densify_tensor t[DR_TENSORS];
};
static_assert(sizeof(ScatterTable) <= 1024, "the table travels in the kernel argument");

// row `c` of the rotation of source row i applied to noise * std
template <int FLAVOUR>
__device__ __forceinline__ float split_offset(size_t i, uint32_t c, const float* __restrict__ scales, const float* __restrict__ rotation, const float* __restrict__ nz)
{
    float s0 = scales[3 * i], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];
    float r0, r1, r2;
    if (FLAVOUR == HGS_DENSIFY_SCENE) {
        s0 = expf(s0), s1 = expf(s1), s2 = expf(s2);
        float w = rotation[4 * i], x = rotation[4 * i + 1], y = rotation[4 * i + 2], z = rotation[4 * i + 3];
        const float norm = sqrtf(w * w + x * x + y * y + z * z);   // build_rotation, general.py:177-198
        w = w / norm, x = x / norm, y = y / norm, z = z / norm;
        if (c == 0) r0 = 1.0f - 2.0f * (y * y + z * z), r1 = 2.0f * (x * y - w * z), r2 = 2.0f * (x * z + w * y);
        else if (c == 1) r0 = 2.0f * (x * y + w * z), r1 = 1.0f - 2.0f * (x * x + z * z), r2 = 2.0f * (y * z - w * x);
        else r0 = 2.0f * (x * z - w * y), r1 = 2.0f * (y * z + w * x), r2 = 1.0f - 2.0f * (x * x + y * y);
    } else {
        s0 = fmaxf(s0, 0.0f), s1 = fmaxf(s1, 0.0f), s2 = fmaxf(s2, 0.0f);
        r0 = rotation[9 * i + 3 * c], r1 = rotation[9 * i + 3 * c + 1], r2 = rotation[9 * i + 3 * c + 2];
    }
    return r0 * (nz[0] * s0) + r1 * (nz[1] * s1) + r2 * (nz[2] * s2);
}

template <int FLAVOUR>
__global__ void __launch_bounds__(DR_THREADS)
densify_scatter_kernel(uint32_t n, const uint8_t* __restrict__ kind, const U4* __restrict__ partials, const uint32_t* __restrict__ totals,
                       const ScatterTable tab, const float* __restrict__ scales, const float* __restrict__ rotation, const float* __restrict__ noise)
{
    __shared__ uint64_t lds[DR_THREADS];
    __shared__ uint32_t to_keep[DR_ROWS], to_clone[DR_ROWS], to_split[DR_ROWS], split_rank[DR_ROWS];
    const uint32_t tid = threadIdx.x;
    const uint32_t row0 = blockIdx.x * (uint32_t)DR_ROWS;
    const uint32_t rows = n - row0 < (uint32_t)DR_ROWS ? n - row0 : (uint32_t)DR_ROWS;

    // the block's row -> destination map, from the plan
    uint32_t k[DR_PER_THREAD];
    uint64_t sum = 0;
#pragma unroll
    for (int j = 0; j < DR_PER_THREAD; ++j) {
        const uint32_t r = tid * DR_PER_THREAD + j;
        k[j] = r < rows ? kind[row0 + r] : 0u;
        sum += pack_kind(k[j]);
    }
    uint64_t total;
    U4 at = unpack(block_scan_exclusive<uint64_t>(sum, lds, 0ull, total));
    const U4 base = partials[blockIdx.x];
    const uint32_t n_keep = totals[0], n_clone = totals[1], n_split = totals[2], n_sel = totals[4];
#pragma unroll
    for (int j = 0; j < DR_PER_THREAD; ++j) {
        const uint32_t r = tid * DR_PER_THREAD + j;
        to_keep[r] = (k[j] & K_KEEP) ? base.keep + at.keep : DR_NONE;
        to_clone[r] = (k[j] & K_CLONE) ? n_keep + base.clone + at.clone : DR_NONE;
        to_split[r] = (k[j] & K_SPLIT) ? n_keep + n_clone + base.split + at.split : DR_NONE;
        split_rank[r] = base.sel + at.sel;
        at = at + unpack(pack_kind(k[j]));
    }
    __syncthreads();

    const hgs_densify_tensor rec = tab.t[blockIdx.y < (uint32_t)DR_TENSORS ? blockIdx.y : 0u];
    const uint32_t w = (uint32_t)rec.width, mode = (uint32_t)rec.mode;
    const uint32_t magic = w > 1 ? 0xFFFFFFFFu / w + 1u : 0u;   // e / w == umulhi(e, magic) for e < DR_ROWS * w, w <= DR_MAX_WIDTH
    const uint32_t elems = rows * w;
    const float* const src = rec.src + (size_t)row0 * w;
    float* const dst = rec.dst;
    constexpr int U = 4;
    for (uint32_t e0 = tid; e0 < elems; e0 += U * DR_THREADS) {
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t e = e0 + u * DR_THREADS;
            v[u] = (e < elems && mode != HGS_DENSIFY_ZERO) ? src[e] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const uint32_t e = e0 + u * DR_THREADS;
            if (e >= elems) continue;
            const uint32_t r = w > 1 ? __umulhi(e, magic) : e;
            const uint32_t c = e - r * w;
            const uint32_t dk = to_keep[r], dc = to_clone[r], ds = to_split[r];
            if (dk != DR_NONE) dst[(size_t)dk * w + c] = v[u];
            if (dc != DR_NONE) dst[(size_t)dc * w + c] = mode == HGS_DENSIFY_MOMENT ? 0.0f : v[u];
            if (ds != DR_NONE) {
                float a = v[u], b = v[u];
                if (mode == HGS_DENSIFY_MOMENT) a = b = 0.0f;
                else if (mode == HGS_DENSIFY_DIV_SPLIT) a = b = v[u] / 1.6f;
                else if (mode == HGS_DENSIFY_LOG_SCALE_SPLIT) a = b = logf(expf(v[u]) / 1.6f);
                else if (mode == HGS_DENSIFY_XYZ_SPLIT) {
                    const size_t i = (size_t)row0 + r, rank = split_rank[r];
                    a = split_offset<FLAVOUR>(i, c, scales, rotation, noise + 3 * rank) + v[u];
                    b = split_offset<FLAVOUR>(i, c, scales, rotation, noise + 3 * ((size_t)n_sel + rank)) + v[u];
                }
                dst[(size_t)ds * w + c] = a;
                dst[((size_t)ds + n_split) * w + c] = b;
            }
        }
    }
}

int fail_densify(const char* what)
{
    hgs::set_last_error(what);
    return HGS_ERR_INVALID_ARGUMENT;
}

int launched(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return HGS_OK;
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", what, hipGetErrorString(e));
    hgs::set_last_error(msg);
    return HGS_ERR_HIP;
}

}  // namespace

extern "C" void hgs_densify_limits(int32_t* rows_per_workgroup, int32_t* tensors_per_launch)
{
    if (rows_per_workgroup) *rows_per_workgroup = DR_ROWS;
    if (tensors_per_launch) *tensors_per_launch = DR_TENSORS;
}

extern "C" int32_t hgs_densify_plan(int32_t flavour, int32_t n, int32_t densify, const float* xyz_gradient_accum, const float* denom,
                                    const float* max_radii2D, const float* scales, const float* opacity, float max_grad, float min_opacity,
                                    float small_max, int32_t use_screen, float max_screen_size, float big_max, uint8_t* kind,
                                    uint32_t* partials, uint32_t* totals, void* stream)
{
    if (flavour != HGS_DENSIFY_SCENE && flavour != HGS_DENSIFY_HUMAN) return fail_densify("densify_plan: unknown flavour");
    if (n < 0) return fail_densify("densify_plan: n < 0");
    if (!totals) return fail_densify("densify_plan: null `totals`");
    if (n > 0 && (!xyz_gradient_accum || !denom || !max_radii2D || !scales || !opacity || !kind || !partials))
        return fail_densify("densify_plan: null pointer (xyz_gradient_accum, denom, max_radii2D, scales, opacity, kind or partials) with n > 0");
    if (((uintptr_t)partials & 15) != 0 || ((uintptr_t)totals & 3) != 0) return fail_densify("densify_plan: partials must be 16-byte aligned, totals 4-byte");
    const uint32_t blocks = ((uint32_t)n + DR_ROWS - 1) / DR_ROWS;
    const PlanArgs a ={n, densify, use_screen, max_grad, min_opacity, small_max, max_screen_size, big_max};
    if (blocks) {
        if (flavour == HGS_DENSIFY_SCENE)
            hipLaunchKernelGGL(densify_classify_kernel<HGS_DENSIFY_SCENE>, dim3(blocks), dim3(DR_THREADS), 0, (hipStream_t)stream, a,
                               xyz_gradient_accum, denom, max_radii2D, scales, opacity, kind, reinterpret_cast<U4*>(partials));
        else
            hipLaunchKernelGGL(densify_classify_kernel<HGS_DENSIFY_HUMAN>, dim3(blocks), dim3(DR_THREADS), 0, (hipStream_t)stream, a,
                               xyz_gradient_accum, denom, max_radii2D, scales, opacity, kind, reinterpret_cast<U4*>(partials));
        if (const int err = launched("densify_plan (classify)")) return err;
    }
    hipLaunchKernelGGL(densify_partials_kernel, dim3(1), dim3(DR_THREADS), 0, (hipStream_t)stream, blocks, reinterpret_cast<U4*>(partials), totals);
    return launched("densify_plan (scan)");
}

extern "C" int32_t hgs_densify_scatter(int32_t flavour, int32_t n, const uint8_t* kind, const uint32_t* partials, const uint32_t* totals,
                                       const hgs_densify_tensor* tensors, int32_t count, const float* scales, const float* rotation,
                                       const float* noise, void* stream)
{
    if (flavour != HGS_DENSIFY_SCENE && flavour != HGS_DENSIFY_HUMAN) return fail_densify("densify_scatter: unknown flavour");
    if (n < 0) return fail_densify("densify_scatter: n < 0");
    if (count < 0) return fail_densify("densify_scatter: count < 0");
    if (count > DR_TENSORS * DR_MAX_LAUNCHES) return fail_densify("densify_scatter: more tensors than 16 launches take");
    if (count > 0 && !tensors) return fail_densify("densify_scatter: null `tensors`");
    if (n > 0 && (!kind || !partials || !totals)) return fail_densify("densify_scatter: null pointer (kind, partials or totals) with n > 0");
    if (((uintptr_t)partials & 15) != 0 || ((uintptr_t)totals & 3) != 0) return fail_densify("densify_scatter: partials must be 16-byte aligned, totals 4-byte");
    for (int32_t i = 0; i < count; ++i) {
        const hgs_densify_tensor& t = tensors[i];
        if (t.mode < HGS_DENSIFY_COPY || t.mode > HGS_DENSIFY_DIV_SPLIT) return fail_densify("densify_scatter: unknown mode");
        if (t.width < 0 || t.width > DR_MAX_WIDTH) return fail_densify("densify_scatter: width must be 0 .. 1024");
        if (t.width == 0 || n == 0) continue;
        if (!t.dst || (!t.src && t.mode != HGS_DENSIFY_ZERO)) return fail_densify("densify_scatter: null pointer (src or dst) with n > 0");
        if ((((uintptr_t)t.src | (uintptr_t)t.dst) & 3) != 0) return fail_densify("densify_scatter: pointer not 4-byte aligned");
        if (t.mode == HGS_DENSIFY_XYZ_SPLIT) {
            if (t.width != 3) return fail_densify("densify_scatter: XYZ_SPLIT needs width 3");
            if (!scales || !rotation || !noise) return fail_densify("densify_scatter: XYZ_SPLIT needs scales, rotation and noise");
        }
    }
    if (n == 0) return HGS_OK;
    const uint32_t blocks = ((uint32_t)n + DR_ROWS - 1) / DR_ROWS;
    ScatterTable tab;
    int32_t i = 0;
    while (i < count) {
        int filled = 0;
        for (; i < count && filled < DR_TENSORS; ++i)
            if (tensors[i].width > 0) tab.t[filled++] = tensors[i];
        if (!filled) break;   // only empty tensors were left
        for (int k2 = filled; k2 < DR_TENSORS; ++k2) tab.t[k2] = tab.t[0];   // (never read: defined bytes in the argument)
        if (flavour == HGS_DENSIFY_SCENE)
            hipLaunchKernelGGL(densify_scatter_kernel<HGS_DENSIFY_SCENE>, dim3(blocks, filled), dim3(DR_THREADS), 0, (hipStream_t)stream, (uint32_t)n, kind,
                               reinterpret_cast<const U4*>(partials), totals, tab, scales, rotation, noise);
        else
            hipLaunchKernelGGL(densify_scatter_kernel<HGS_DENSIFY_HUMAN>, dim3(blocks, filled), dim3(DR_THREADS), 0, (hipStream_t)stream, (uint32_t)n, kind,
                               reinterpret_cast<const U4*>(partials), totals, tab, scales, rotation, noise);
        if (const int err = launched("densify_scatter")) return err;
    }
    return HGS_OK;
}
