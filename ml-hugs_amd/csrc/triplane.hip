// Row f-8 (the statement that opens every human step): TriPlane.forward, /root/reference/hugs/models/modules/triplane.py:26-40,
// called at /root/reference/hugs/models/hugs_trimlp.py:206,408 --
//   x = (x - center) / scale + 0.5;  x = x * 2 - 1                                   (:27,:30)
//   feat_xy = grid_sample(plane_xy, coords[..., [0, 1]], align_corners=True)          (:35; bilinear, zeros padding)
//   feat_xz = grid_sample(plane_xz, coords[..., [0, 2]], ...)   feat_yz = grid_sample(plane_yz, coords[..., [1, 2]], ...)
//   feat = cat([feat_xy, feat_xz, feat_yz], dim=1)                                    (:38)
// grid[..., 0] indexes a plane's LAST axis: on plane_xy [1,F,resX,resY] x runs along the axis of size resY and y along resX, on
// plane_xz [1,F,resX,resZ] x along resZ and z along resX, on plane_yz [1,F,resY,resZ] y along resZ and z along resY.
//
// Mapping: 32 lanes per point, lane = channel, the three planes one after the other; a wave holds two points.  The planes are
// addressed through element strides.  Stored texel-major (torch.channels_last: channel stride 1) a texel's 32 channels are one
// 128-byte segment: a corner read is one segment per point, and a wave-instruction of the backward's scatter is two 128-byte
// segments of float atomics -- the shape that runs at the chip's full atomic rate.  NCHW planes (channel stride H * W) run
// through the same code with every lane in a row of its own: correct, and slow.
// dL/dx needs no atomics: a point's three coordinates collect from two planes each over the 32 channels, all inside its 32 lanes.
#include "hgs_common.h"

namespace {

struct PlaneGeo {
    const float* value;   // [F,H,W] through the strides below (backward without dL/dx: may be NULL)
    float* grad;          // backward only: same strides, zero on entry, or NULL
    long long sc, sh, sw; // element strides: channel, row (H), column (W)
    int H, W;
};
struct TriGeo {
    PlaneGeo p[3];        // xy, xz, yz
    float center, scale;
};

// which coordinate runs along W (grid[..., 0]) and which along H (grid[..., 1]) of plane p
__device__ __forceinline__ constexpr int axis_w(int p) { return p == 2 ? 1 : 0; }
__device__ __forceinline__ constexpr int axis_h(int p) { return p == 0 ? 1 : 2; }

// One bilinear cell as grid_sample forms it (align_corners=True): ix = ((g + 1) / 2) * (W - 1), nw = floor, the four weights from
// the differences to the opposite corner.  A corner is used only when it lies inside the plane; the test is made on the floats, so
// a non-finite or far-away coordinate selects no corner and no index is ever formed from it.
struct Cell {
    float tx0, tx1, ty0, ty1;   // ix - ix_nw, ix_se - ix, iy - iy_nw, iy_se - iy
    int x0, y0;
    bool in_x0, in_x1, in_y0, in_y1;
};
__device__ __forceinline__ Cell locate(float gu, float gv, int W, int H)
{
    Cell c;
    const float ix = ((gu + 1.0f) / 2.0f) * (float)(W - 1);
    const float iy = ((gv + 1.0f) / 2.0f) * (float)(H - 1);
    const float fx = floorf(ix), fy = floorf(iy);
    c.tx0 = ix - fx, c.tx1 = (fx + 1.0f) - ix;
    c.ty0 = iy - fy, c.ty1 = (fy + 1.0f) - iy;
    c.in_x0 = fx >= 0.0f && fx <= (float)(W - 1);
    c.in_x1 = fx >= -1.0f && fx <= (float)(W - 2);
    c.in_y0 = fy >= 0.0f && fy <= (float)(H - 1);
    c.in_y1 = fy >= -1.0f && fy <= (float)(H - 2);
    c.x0 = (c.in_x0 || c.in_x1) ? (int)fx : 0;
    c.y0 = (c.in_y0 || c.in_y1) ? (int)fy : 0;
    return c;
}

__device__ __forceinline__ void normalized(const float* __restrict__ x, size_t pt, float center, float scale, float q[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = ((x[3 * pt + k] - center) / scale + 0.5f) * 2.0f - 1.0f;
}

constexpr int F32 = 32, POINTS_PER_BLOCK = 256 / F32;

__global__ void __launch_bounds__(256)
triplane_forward_kernel(int n, TriGeo g, const float* __restrict__ x, float* __restrict__ feat)
{
    const int c = threadIdx.x & (F32 - 1);
    const size_t pt = (size_t)blockIdx.x * POINTS_PER_BLOCK + (threadIdx.x >> 5);
    if (pt >= (size_t)n) return;
    float q[3];
    normalized(x, pt, g.center, g.scale, q);
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const PlaneGeo& P = g.p[p];
        const Cell k = locate(q[axis_w(p)], q[axis_h(p)], P.W, P.H);
        const float* base = P.value + (long long)c * P.sc + (long long)k.y0 * P.sh + (long long)k.x0 * P.sw;
        const bool nw = k.in_x0 && k.in_y0, ne = k.in_x1 && k.in_y0, sw = k.in_x0 && k.in_y1, se = k.in_x1 && k.in_y1;
        const float v_nw = nw ? base[0] : 0.0f, v_ne = ne ? base[P.sw] : 0.0f;
        const float v_sw = sw ? base[P.sh] : 0.0f, v_se = se ? base[P.sh + P.sw] : 0.0f;
        float acc = 0.0f;
        if (nw) acc += v_nw * (k.tx1 * k.ty1);
        if (ne) acc += v_ne * (k.tx0 * k.ty1);
        if (sw) acc += v_sw * (k.tx1 * k.ty0);
        if (se) acc += v_se * (k.tx0 * k.ty0);
        feat[pt * (3 * F32) + p * F32 + c] = acc;
    }
}

// DP: scatter into the planes' gradients; DX: dL/dx (reads the planes' values)
template <bool DX, bool DP>
__global__ void __launch_bounds__(256)
triplane_backward_kernel(int n, TriGeo g, const float* __restrict__ x, const float* __restrict__ dL_dfeat, float* __restrict__ dL_dx)
{
    const int c = threadIdx.x & (F32 - 1);
    const size_t pt = (size_t)blockIdx.x * POINTS_PER_BLOCK + (threadIdx.x >> 5);
    if (pt >= (size_t)n) return;
    float q[3];
    normalized(x, pt, g.center, g.scale, q);
    float dq[3] = {0.0f, 0.0f, 0.0f};   // this channel's part of dL/d(normalized coordinate)
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const PlaneGeo& P = g.p[p];
        const Cell k = locate(q[axis_w(p)], q[axis_h(p)], P.W, P.H);
        const long long at = (long long)c * P.sc + (long long)k.y0 * P.sh + (long long)k.x0 * P.sw;
        const bool nw = k.in_x0 && k.in_y0, ne = k.in_x1 && k.in_y0, sw = k.in_x0 && k.in_y1, se = k.in_x1 && k.in_y1;
        const float go = dL_dfeat[pt * (3 * F32) + p * F32 + c];
        if (DP && P.grad) {
            float* gp = P.grad + at;
            if (nw) atomicAdd(gp, (k.tx1 * k.ty1) * go);
            if (ne) atomicAdd(gp + P.sw, (k.tx0 * k.ty1) * go);
            if (sw) atomicAdd(gp + P.sh, (k.tx1 * k.ty0) * go);
            if (se) atomicAdd(gp + P.sh + P.sw, (k.tx0 * k.ty0) * go);
        }
        if (DX) {
            const float* base = P.value + at;
            const float v_nw = nw ? base[0] : 0.0f, v_ne = ne ? base[P.sw] : 0.0f;
            const float v_sw = sw ? base[P.sh] : 0.0f, v_se = se ? base[P.sh + P.sw] : 0.0f;
            float gix = 0.0f, giy = 0.0f;
            if (nw) gix -= v_nw * k.ty1 * go, giy -= v_nw * k.tx1 * go;
            if (ne) gix += v_ne * k.ty1 * go, giy -= v_ne * k.tx0 * go;
            if (sw) gix -= v_sw * k.ty0 * go, giy += v_sw * k.tx1 * go;
            if (se) gix += v_se * k.ty0 * go, giy += v_se * k.tx0 * go;
            dq[axis_w(p)] += gix * ((float)(P.W - 1) / 2.0f);
            dq[axis_h(p)] += giy * ((float)(P.H - 1) / 2.0f);
        }
    }
    if (DX) {
        // sum over the point's 32 channels (its own half of the wave), then d(normalized)/dx = 2 / scale
#pragma unroll
        for (int d = F32 / 2; d >= 1; d >>= 1) {
#pragma unroll
            for (int j = 0; j < 3; ++j) dq[j] += __shfl_xor(dq[j], d, F32);
        }
        if (c < 3) dL_dx[3 * pt + c] = ((c == 0 ? dq[0] : c == 1 ? dq[1] : dq[2]) * 2.0f) / g.scale;
    }
}

int fail_triplane(const char* what)
{
    hgs::set_last_error(what);
    return HGS_ERR_INVALID_ARGUMENT;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// res = (resX, resY, resZ): plane_xy is [F,resX,resY], plane_xz [F,resX,resZ], plane_yz [F,resY,resZ]
void fill_geometry(TriGeo& g, const int32_t res[3], const int64_t strides[3][3], float center, float scale)
{
    const int H[3] = {res[0], res[0], res[1]}, W[3] = {res[1], res[2], res[2]};
    for (int p = 0; p < 3; ++p) {
        g.p[p].value = nullptr, g.p[p].grad = nullptr;
        g.p[p].sc = strides[p][0], g.p[p].sh = strides[p][1], g.p[p].sw = strides[p][2];
        g.p[p].H = H[p], g.p[p].W = W[p];
    }
    g.center = center, g.scale = scale;
}

const char* check_geometry(int32_t n, int32_t F, const int32_t* res, const int64_t (*strides)[3])
{
    if (n < 0) return "need n >= 0";
    if (F != F32) return "only F = 32 features per plane is implemented (the reference's configuration)";
    if (!res || !strides) return "null pointer";
    for (int k = 0; k < 3; ++k) if (res[k] < 2) return "every plane resolution must be at least 2";
    for (int p = 0; p < 3; ++p) for (int k = 0; k < 3; ++k) if (strides[p][k] < 0) return "negative stride";
    return nullptr;
}

}  // namespace

extern "C" int32_t hgs_triplane_forward(int32_t n, int32_t F, const int32_t res[3], const int64_t strides[3][3], float center, float scale,
                                        const float* x, const float* plane_xy, const float* plane_xz, const float* plane_yz,
                                        float* feat, void* stream)
{
    static thread_local char msg[160];
    if (const char* why = check_geometry(n, F, res, strides)) {
        snprintf(msg, sizeof msg, "triplane_forward: %s", why);
        return fail_triplane(msg);
    }
    if (n == 0) return HGS_OK;
    if (!x || !plane_xy || !plane_xz || !plane_yz || !feat) return fail_triplane("triplane_forward: null pointer");
    if (!aligned16(feat)) return fail_triplane("triplane_forward: feat must be 16-byte aligned");
    TriGeo g;
    fill_geometry(g, res, strides, center, scale);
    g.p[0].value = plane_xy, g.p[1].value = plane_xz, g.p[2].value = plane_yz;
    const dim3 grid((unsigned)(((size_t)n + POINTS_PER_BLOCK - 1) / POINTS_PER_BLOCK));
    hipLaunchKernelGGL(triplane_forward_kernel, grid, dim3(256), 0, (hipStream_t)stream, n, g, x, feat);
    if (hipGetLastError() != hipSuccess) {
        hgs::set_last_error("triplane_forward: kernel launch failed");
        return HGS_ERR_HIP;
    }
    return HGS_OK;
}

extern "C" int32_t hgs_triplane_backward(int32_t n, int32_t F, const int32_t res[3], const int64_t strides[3][3], float center, float scale,
                                         const float* x, const float* const planes[3], const float* dL_dfeat, float* dL_dx,
                                         float* const dL_dplanes[3], void* stream)
{
    static thread_local char msg[160];
    if (const char* why = check_geometry(n, F, res, strides)) {
        snprintf(msg, sizeof msg, "triplane_backward: %s", why);
        return fail_triplane(msg);
    }
    if (n == 0) return HGS_OK;
    if (!x || !dL_dfeat) return fail_triplane("triplane_backward: null pointer");
    if (dL_dx && (!planes || !planes[0] || !planes[1] || !planes[2])) return fail_triplane("triplane_backward: dL_dx needs the three planes");
    if (!aligned16(dL_dfeat)) return fail_triplane("triplane_backward: dL_dfeat must be 16-byte aligned");
    TriGeo g;
    fill_geometry(g, res, strides, center, scale);
    bool any_plane = false;
    for (int p = 0; p < 3; ++p) {
        g.p[p].value = dL_dx ? planes[p] : nullptr;
        g.p[p].grad = dL_dplanes ? dL_dplanes[p] : nullptr;
        any_plane = any_plane || g.p[p].grad;
    }
    if (!dL_dx && !any_plane) return HGS_OK;   // nothing asked for
    const dim3 grid((unsigned)(((size_t)n + POINTS_PER_BLOCK - 1) / POINTS_PER_BLOCK));
    if (dL_dx && any_plane) hipLaunchKernelGGL((triplane_backward_kernel<true, true>), grid, dim3(256), 0, (hipStream_t)stream, n, g, x, dL_dfeat, dL_dx);
    else if (dL_dx) hipLaunchKernelGGL((triplane_backward_kernel<true, false>), grid, dim3(256), 0, (hipStream_t)stream, n, g, x, dL_dfeat, dL_dx);
    else hipLaunchKernelGGL((triplane_backward_kernel<false, true>), grid, dim3(256), 0, (hipStream_t)stream, n, g, x, dL_dfeat, dL_dx);
    if (hipGetLastError() != hipSuccess) {
        hgs::set_last_error("triplane_backward: kernel launch failed");
        return HGS_ERR_HIP;
    }
    return HGS_OK;
}
