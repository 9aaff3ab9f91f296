// Accumulated-alpha and depth maps of a rendered frame, with gradients:
//     alpha(pixel) = sum_i w_i,    depth(pixel) = sum_i w_i z_i,    w_i = alpha_i T_i,
// over exactly the colour pass's contributors, z_i the view-space z of the Gaussian's Splat record.  Three passes of their own
// over what the forward left behind -- the per-quad compacted lists, the splat records, final_T and n_contrib -- so no kernel of
// the colour path changes:
//   maps_forward_kernel   one wave per (tile, quad) walks the quad's list from the front up to each pixel's recorded last contributor
//   maps_backward_kernel  the same wave walks it from the back from final_T, as the colour backward does: the computation is linear
//                         in (c . g), so it IS the colour backward with c . g replaced by z gD + gA and S started at 0.  Per entry
//                         one cross-lane reduction of seven sums -- the six raw moments of u (slots 0..5 of the [P][12] accumulator,
//                         where they add to the colour backward's) and g_z = sum w gD (pad slot 9) -- and one global_atomic_add_f32
//   maps_finish_kernel    one thread per Gaussian, after the per-Gaussian backward: dL/dmeans3D += g_z (V[2], V[6], V[10])
// The alpha of an entry is evaluated with the instruction sequence of fwd_accumulate (blend_fwd.h) / bwd_pixel (blend.hip): the
// skip below 1/255 must fall as the colour pass's did.  Compiled with -ffp-contract=off like them; the FMAs are explicit.
#include "hgs_common.h"
#include "blend_fwd.h"

namespace hgs {

namespace {

struct MapRec {  // wave-uniform (SGPRs): the geometry half of SplatRec and the Gaussian's view-space z
    float x, y, A, B, C, L, z;
};

// (the index is clamped for the same reason as in load_rec: the pipelines read a few entries past either end of a list)
__device__ __forceinline__ MapRec load_map_rec(const Splat* splats, uint32_t entry_low, uint32_t last_gaussian)
{
    const uint32_t gid = min(entry_low & GID_MASK, last_gaussian);
    const_f4p p = (const_f4p)((const char*)splats + gid * 64u);
    const v4f h0 = p[0];
    const float lc = ((const_f32p)p)[4], l2o = ((const_f32p)p)[5];   // (one s_load_dwordx2)
    const float z = ((const_f32p)p)[9];                              // Splat::depth
    MapRec s;
    s.x = h0.x, s.y = h0.y;
    s.A = h0.z, s.B = h0.w, s.C = lc;
    s.L = l2o, s.z = z;
    return s;
}

// What a lane knows of its pixel before the walk.
struct MapPixel {
    int px, py;
    bool inside;
    size_t pix;
    uint32_t last;  // 1-based list position of the pixel's last contributor (n_contrib without its clamp flags); 0: none
};

__device__ __forceinline__ MapPixel map_pixel(const Camera& cam, int tile, int w, int lane, const uint32_t* __restrict__ n_contrib)
{
    MapPixel m;
    m.px = (tile % cam.gx) * TILE + (w & 1) * 8 + (lane & 7);
    m.py = (tile / cam.gx) * TILE + (w >> 1) * 8 + (lane >> 3);
    m.inside = m.px < cam.W && m.py < cam.H;
    m.pix = m.inside ? (size_t)m.py * cam.W + m.px : 0;
    const uint32_t ld = n_contrib[m.pix];  // (out-of-image lanes read a clamped address and are masked)
    m.last = m.inside ? (ld & GID_MASK) : 0u;
    return m;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return __builtin_amdgcn_readfirstlane(v);
}

// Entries of the list (ascending positions) with pos1 <= wmax: binary search with scalar loads, as the colour backward's.
__device__ __forceinline__ uint32_t entries_up_to(const uint64_t* first, uint32_t n, uint32_t wmax)
{
    if (n == 0 || wmax == 0) return 0;
    if ((uint32_t)(((const_u64p)first)[n - 1] >> 32) <= wmax) return n;
    uint32_t lo = 0, hi = n - 1;  // invariant: entries [0, lo) have pos1 <= wmax, entry hi has pos1 > wmax
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint32_t)(((const_u64p)first)[mid] >> 32) <= wmax) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One list entry applied to the wave's 64 pixels, fully predicated.  A contributor of a pixel is an entry at or in front of the
// pixel's recorded last one whose alpha reaches 1/255 -- the transmittance stop is already in `last`.
__device__ __forceinline__ void maps_accumulate(const MapRec& s, uint32_t pos1, float pxf, float pyf, uint32_t last, float& T, float& A,
                                                float& D)
{
    const float dx = s.x - pxf, dy = s.y - pyf;
    const float tq = __builtin_fmaf(s.A, dx, s.B * dy), uq = s.C * dy;
    const float e = __builtin_fmaf(-tq, tq, __builtin_fmaf(-uq, uq, s.L));   // == log2_alpha(s, dx, dy)
    const float alpha = fminf(ALPHA_MAX, __builtin_amdgcn_exp2f(e));
    const bool take = alpha >= ALPHA_MIN && pos1 <= last;
    const float wgt = take ? alpha * T : 0.0f;
    A += wgt;
    D = __builtin_fmaf(s.z, wgt, D);
    T = take ? T * (1.0f - alpha) : T;
}

}  // namespace

// Workgroup b = tile b, one wave per quad.  Either output may be NULL.
__global__ void __launch_bounds__(256)
maps_forward_kernel(Camera cam, uint32_t lastg, const uint2* __restrict__ ranges, const uint64_t* __restrict__ act, size_t act_stride,
                    const uint32_t* __restrict__ act_count, const Splat* __restrict__ splats, const uint32_t* __restrict__ n_contrib,
                    const uint32_t* __restrict__ n_total, float* __restrict__ out_alpha, float* __restrict__ out_depth)
{
    if (((const_u32p)n_total)[1]) return;  // the frame did not fit its binning buffer: nothing of it is valid
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x;
    const MapPixel m = map_pixel(cam, tile, w, lane, n_contrib);
    const float pxf = (float)m.px, pyf = (float)m.py;
    const v2u range = ((const_u2p)ranges)[tile];
    const uint32_t wmax = range.y > range.x ? wave_max(m.last) : 0u;
    const uint64_t* list = act + (size_t)w * act_stride + range.x;
    const uint32_t n = entries_up_to(list, wmax ? ((const_u32p)act_count)[tile * NUM_LISTS + w] : 0u, wmax);
    float T = 1.0f, A = 0.0f, D = 0.0f;
    if (n) {
        // the forward blend's software pipeline (blend_fwd.h): two entries per half-iteration, two register sets
        v4u eA = load_pair(list, 0);
        MapRec rA0 = load_map_rec(splats, eA.x, lastg), rA1 = load_map_rec(splats, eA.z, lastg);
        v4u eB = load_pair(list, 2);
        for (uint32_t j = 0; j < n; j += 4) {
            const MapRec rB0 = load_map_rec(splats, eB.x, lastg), rB1 = load_map_rec(splats, eB.z, lastg);
            const v4u eA2 = load_pair(list, j + 4);
            maps_accumulate(rA0, eA.y, pxf, pyf, m.last, T, A, D);
            if (j + 1 < n) maps_accumulate(rA1, eA.w, pxf, pyf, m.last, T, A, D);
            if (j + 2 >= n) break;
            rA0 = load_map_rec(splats, eA2.x, lastg), rA1 = load_map_rec(splats, eA2.z, lastg);
            const v4u eB2 = load_pair(list, j + 6);
            maps_accumulate(rB0, eB.y, pxf, pyf, m.last, T, A, D);
            if (j + 3 < n) maps_accumulate(rB1, eB.w, pxf, pyf, m.last, T, A, D);
            eA = eA2, eB = eB2;
        }
        // (as in blend_forward_walk: keeping the next pair's records alive past the loop pins their loads in the middle of the body,
        //  where they fly while the second pair is blended, instead of in front of the wait at the loop's top)
        asm volatile("" ::"s"(rA0.x), "s"(rA0.L), "s"(rA0.z), "s"(rA1.x), "s"(rA1.L), "s"(rA1.z));
    }
    if (m.inside) {
        if (out_alpha) out_alpha[m.pix] = A;
        if (out_depth) out_depth[m.pix] = D;
    }
}

// ------------------------------------------------------------------------------------------------
namespace {

// (every DPP move is evaluated with all 64 lanes active and only then selected: blend.hip)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
constexpr int DPP_QUAD_XOR1 = 0xB1;         // quad_perm:[1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;         // quad_perm:[2,3,0,1]
constexpr int DPP_ROW_HALF_MIRROR = 0x141;  // lane i <- lane 7-i of its half-row

// Per-wave LDS region of the reduction: [entry of the pair][sum 0..7][lane]; the eighth row is never written (seven sums) and the
// lane group that reads it adds nothing anywhere.
constexpr int MAPS_RED_FLOATS = 2 * 8 * 64;
constexpr int MAPS_SUMS = 7;

struct MapBwd {
    float pxf, pyf;
    float T;       // running transmittance, in front of the entry being processed once divided by 1 - alpha
    float S;       // sum over deeper contributors j of (z_j gD + gA) alpha_j T_j; the background adds nothing: starts at 0
    float gA, gD;  // dL/dalpha map, dL/ddepth map at the pixel
    uint32_t last;
};

}  // namespace

__global__ void __launch_bounds__(256)
maps_backward_kernel(Camera cam, uint32_t lastg, const uint2* __restrict__ ranges, const uint64_t* __restrict__ act, size_t act_stride,
                     const uint32_t* __restrict__ act_count, const Splat* __restrict__ splats, const float* __restrict__ final_T,
                     const uint32_t* __restrict__ n_contrib, const uint32_t* __restrict__ n_total, const float* __restrict__ dL_dalpha_map,
                     const float* __restrict__ dL_ddepth_map, float* __restrict__ grad_accum)
{
    __shared__ float red_all[4 * MAPS_RED_FLOATS];
    if (((const_u32p)n_total)[1]) return;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int tile = (int)blockIdx.x;
    const v2u range = ((const_u2p)ranges)[tile];
    if (range.y <= range.x) return;
    const MapPixel m = map_pixel(cam, tile, w, lane, n_contrib);
    // (all loads issued before any is consumed; out-of-image lanes read pixel 0 and are masked)
    const float ld_T = final_T[m.pix];
    const float ld_gA = dL_dalpha_map ? dL_dalpha_map[m.pix] : 0.0f;
    const float ld_gD = dL_ddepth_map ? dL_ddepth_map[m.pix] : 0.0f;
    MapBwd p;
    p.pxf = (float)m.px, p.pyf = (float)m.py;
    p.T = m.inside ? ld_T : 0.0f;
    p.S = 0.0f;
    p.gA = m.inside ? ld_gA : 0.0f, p.gD = m.inside ? ld_gD : 0.0f;
    p.last = m.last;
    const uint32_t wmax = wave_max(m.last);
    if (wmax == 0) return;
    const uint64_t* first = act + (size_t)w * act_stride + range.x;
    const uint32_t n = entries_up_to(first, ((const_u32p)act_count)[tile * NUM_LISTS + w], wmax);
    if (n == 0) return;
    const uint64_t* top = first + n;  // one past the deepest entry to visit

    // The reduction of blend.hip: lane group g = lanes 8g..8g+7 sums v_g.  Lane 8g+i reads the eight partials of lanes 8i..8i+7 with
    // two ds_read_b128 (the odd groups the two halves in the other order: 64 distinct banks per b128 lane group), adds them, and
    // three in-half-row DPP adds finish group g's total.  Lane 8g adds total g into slot g of the Gaussian's record for g = 0..5,
    // lane 48 adds g_z into pad slot 9: seven addresses, one atomic instruction.
    float* const red = red_all + w * MAPS_RED_FLOATS;
    const int grp = lane >> 3;
    const int rd = grp * 64 + (lane & 7) * 8 + (grp & 1) * 4;  // (floats) first read; the second at rd ^ 4
    const int slot_of_lane = (lane & 7) != 0 || grp >= MAPS_SUMS ? -1 : (grp == 6 ? 9 : grp);

    // Per entry: the pixel work and the seven sums stored to the entry's LDS buffer e at [sum][lane].  Returns whether any lane took
    // the entry (else nothing was stored and no reduction or atomic is due).
    auto backward_entry = [&](const MapRec& s, uint32_t pos1, int e) -> bool {
        const float dy = s.y - p.pyf, bdy = s.B * dy, cdy = s.C * dy, q = __builtin_fmaf(-cdy, cdy, s.L);
        const float dx = s.x - p.pxf;
        const float t = __builtin_fmaf(s.A, dx, bdy);
        const float ex = __builtin_fmaf(-t, t, q);  // == log2_alpha(s, dx, dy), same rounding
        const float alpha_uncapped = __builtin_amdgcn_exp2f(ex);
        const float alpha = fminf(ALPHA_MAX, alpha_uncapped);
        const bool act_lane = alpha >= ALPHA_MIN && pos1 <= p.last;
        if (__builtin_amdgcn_ballot_w64(act_lane) == 0ull) return false;
        float v[MAPS_SUMS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (act_lane) {
            const float inv = __builtin_amdgcn_rcpf(1.0f - alpha);
            p.T = p.T * inv;  // transmittance in front of this entry
            const float cg = __builtin_fmaf(s.z, p.gD, p.gA);
            // alpha map + depth map = sum_j (gA + z_j gD) alpha_j T_j, every T_j behind this entry carries (1 - alpha):
            //   dL/dalpha = T cg - S / (1 - alpha)
            const float dL_dalpha = __builtin_fmaf(p.T, cg, -(p.S * inv));
            const float dch = alpha * p.T;
            p.S = __builtin_fmaf(cg, dch, p.S);
            const float u = alpha_uncapped * dL_dalpha;  // straight-through alpha cap, as the colour backward
            const float ux = u * dx, uy = u * dy;
            v[0] = ux;
            v[1] = uy;
            v[2] = ux * dx;
            v[3] = ux * dy;
            v[4] = uy * dy;
            v[5] = u;
            v[6] = dch * p.gD;
        }
        float* const buf = red + e * (8 * 64);
#pragma unroll
        for (int k = 0; k < MAPS_SUMS; ++k) buf[k * 64 + lane] = v[k];
        return true;
    };
    auto backward_finish = [&](uint32_t val, int e) {
        const float* const buf = red + e * (8 * 64);
        // (wave-scope fences: no instruction, they only keep the compiler from moving the reads above the stores; DS operations of a
        //  wave execute in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const float4 ra = *(const float4*)(buf + rd);
        const float4 rb = *(const float4*)(buf + (rd ^ 4));
        float y = ((ra.x + ra.y) + (ra.z + ra.w)) + ((rb.x + rb.y) + (rb.z + rb.w));
        y += dpp_mov<DPP_QUAD_XOR1>(y);
        y += dpp_mov<DPP_QUAD_XOR2>(y);
        y += dpp_mov<DPP_ROW_HALF_MIRROR>(y);
        if (slot_of_lane >= 0) atomicAdd(grad_accum + (size_t)(val & GID_MASK) * 12u + slot_of_lane, y);
        // (the buffer's next store must not overtake these reads in the compiler's schedule either)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    };

    // The colour backward's pipeline: pair k = entries top[-2k-2] (shallower) and top[-2k-1] (deeper); the front pad of `act` makes the
    // read below the list's start by the last, half-used pair harmless.  Two register sets: while one is consumed the other's records
    // and the next pair of entries are in flight.
    v4u eA = load_pair(top - 2, 0);
    MapRec rA0 = load_map_rec(splats, eA.z, lastg), rA1 = load_map_rec(splats, eA.x, lastg);  // rA0: deeper, first
    v4u eB = load_pair(top - 4, 0);
    for (uint32_t j = 0; j < n; j += 4) {
        __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): before the next set's loads are issued (scalar loads return out of order)
        const MapRec rB0 = load_map_rec(splats, eB.z, lastg), rB1 = load_map_rec(splats, eB.x, lastg);
        const v4u eA2 = load_pair(top - 6 - j, 0);
        const bool tA0 = backward_entry(rA0, eA.w, 0);
        const bool tA1 = j + 1 < n && backward_entry(rA1, eA.y, 1);
        if (tA0) backward_finish(eA.z, 0);
        if (tA1) backward_finish(eA.x, 1);
        if (j + 2 >= n) break;
        rA0 = load_map_rec(splats, eA2.z, lastg), rA1 = load_map_rec(splats, eA2.x, lastg);
        const v4u eB2 = load_pair(top - 8 - j, 0);
        const bool tB0 = backward_entry(rB0, eB.w, 0);
        const bool tB1 = j + 3 < n && backward_entry(rB1, eB.y, 1);
        if (tB0) backward_finish(eB.z, 0);
        if (tB1) backward_finish(eB.x, 1);
        eA = eA2, eB = eB2;
    }
}

// After the per-Gaussian backward (which writes dL/dmeans3D whole): z_view = x V[2] + y V[6] + z V[10] + V[14].
__global__ void __launch_bounds__(256)
maps_finish_kernel(int P1, int P, const float* __restrict__ V, const float* __restrict__ grad_accum, const uint32_t* __restrict__ n_total,
                   float* __restrict__ dL_dmeans3D, float* __restrict__ seg2_dL_dmeans3D)
{
    if (((const_u32p)n_total)[1]) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    const float gz = grad_accum[12 * (size_t)i + 9];
    if (gz == 0.0f) return;
    float* const d = i < P1 ? dL_dmeans3D + 3 * (size_t)i : seg2_dL_dmeans3D + 3 * (size_t)(i - P1);
    d[0] += gz * V[2], d[1] += gz * V[6], d[2] += gz * V[10];
}

void launch_maps_forward(const Camera& cam, int P, const uint2* ranges, const uint64_t* act, size_t act_stride, const uint32_t* act_count,
                         const Splat* splats, const uint32_t* n_contrib, const uint32_t* n_total, float* out_alpha, float* out_depth,
                         hipStream_t st)
{
    hipLaunchKernelGGL(maps_forward_kernel, dim3(cam.gx * cam.gy), dim3(256), 0, st, cam, (uint32_t)(P - 1), ranges, act, act_stride,
                       act_count, splats, n_contrib, n_total, out_alpha, out_depth);
}

void launch_maps_backward(const Camera& cam, int P, const uint2* ranges, const uint64_t* act, size_t act_stride, const uint32_t* act_count,
                          const Splat* splats, const float* final_T, const uint32_t* n_contrib, const uint32_t* n_total,
                          const float* dL_dalpha, const float* dL_ddepth, float* grad_accum, hipStream_t st)
{
    hipLaunchKernelGGL(maps_backward_kernel, dim3(cam.gx * cam.gy), dim3(256), 0, st, cam, (uint32_t)(P - 1), ranges, act, act_stride,
                       act_count, splats, final_T, n_contrib, n_total, dL_dalpha, dL_ddepth, grad_accum);
}

void launch_maps_finish(int P1, int P, const float* V, const float* grad_accum, const uint32_t* n_total, float* dL_dmeans3D,
                        float* seg2_dL_dmeans3D, hipStream_t st)
{
    hipLaunchKernelGGL(maps_finish_kernel, dim3((P + 255) / 256), dim3(256), 0, st, P1, P, V, grad_accum, n_total, dL_dmeans3D,
                       seg2_dL_dmeans3D);
}

}  // namespace hgs
