// Row f-5 with HumanSceneLoss's masks (hugs/losses/loss.py:46-162): the reference never calls l1_loss and ssim on the bare images
// in its `human` and `scene` configs, it calls them on composites it builds with full-image torch statements,
//   human:  x = pred,            y = gt * m + bg_c * (1 - m)        (loss.py:71; again for the human-only render, :130)
//   scene:  x = pred * (1 - m),  y = gt * (1 - m)                   (loss.py:78-80)
// and scales both terms with the mask's area.  Here the composite is applied while a tile is loaded into LDS (loss_tile.h): the
// kernels are loss.hip's with one more input plane, no composited image is written to memory, and sum(m) rides on channel 0's tiles.
//   l1        = sum |x - y| / sum(m)                                 (loss.py:89,91 -> utils.py:57)
//   ssim_term = (1 - mean(ssim map of x, y)) * sum(m) / (H W)        (loss.py:99-103)
// BOTH modes use the sum of the human mask m: in `scene` the reference inverts the mask (:78) and inverts it again where it divides
// (:91) and where it scales (:103) -- reproduced, not repaired.  sum(m) = 0 divides by zero on the device as it does there.
// Backward: dL/dpred = s [ gs (w*m1 + 2 x (w*m2) + y (w*m3)) + gl sign(x - y) ], s = 1 (human) or 1 - m (scene); gs and gl follow from
// the two upstream gradients and forward's sum(m), all read on the device.
#include "loss_tile.h"

static_assert(LOSS_HUMAN == HGS_MASKED_HUMAN && LOSS_SCENE == HGS_MASKED_SCENE, "the header's modes are the template's");

namespace {

template <int MODE, bool WITH_MAPS>
__global__ void __launch_bounds__(256)
masked_loss_forward_kernel(Plane p, const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                           const float* __restrict__ bg, float* __restrict__ maps, float4* __restrict__ partial)
{
    ssim_l1_forward_tile<MODE, WITH_MAPS>(p, pred, gt, mask, bg, maps, partial);
}

// out[0] = l1, out[1] = ssim_term, out[2] = sum(m), out[3] = mean of the SSIM map; the three sums in a fixed order in double
__global__ void __launch_bounds__(256)
masked_loss_reduce_kernel(int blocks, const float4* __restrict__ partial, double count, double pixels, float* __restrict__ out)
{
    __shared__ double sa[256], sb[256], sc[256];
    double a = 0.0, b = 0.0, c = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) {
        const float4 v = partial[i];
        a += (double)v.x, b += (double)v.y, c += (double)v.z;
    }
    sa[threadIdx.x] = a, sb[threadIdx.x] = b, sc[threadIdx.x] = c;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d)
            sa[threadIdx.x] += sa[threadIdx.x + d], sb[threadIdx.x] += sb[threadIdx.x + d], sc[threadIdx.x] += sc[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double mean = sa[0] / count, area = sc[0];
        out[0] = (float)(sb[0] / area), out[1] = (float)((1.0 - mean) * area / pixels), out[2] = (float)area, out[3] = (float)mean;
    }
}

template <int MODE>
__global__ void __launch_bounds__(256)
masked_loss_backward_kernel(Plane p, const float* __restrict__ pred, const float* __restrict__ gt, const float* __restrict__ mask,
                            const float* __restrict__ bg, const float* __restrict__ maps, const float* __restrict__ terms,
                            const float* __restrict__ g_l1, const float* __restrict__ g_ssim_term, float* __restrict__ dL_dpred)
{
    ssim_l1_backward_tile<MODE>(p, pred, gt, mask, bg, maps, g_ssim_term, g_l1, terms, dL_dpred);
}

}  // namespace

extern "C" size_t hgs_masked_loss_workspace(int32_t C, int32_t H, int32_t W)
{
    if (C < 1 || H < 1 || W < 1) return 0;
    return sizeof(float4) * (size_t)loss_tiles(C, H, W);
}

extern "C" int32_t hgs_masked_loss_forward(int32_t mode, int32_t C, int32_t H, int32_t W, const float* pred, const float* gt,
                                           const float* mask, const float* bg, float* maps, void* workspace, float* out, void* stream)
{
    if (mode != HGS_MASKED_HUMAN && mode != HGS_MASKED_SCENE) return fail_loss("masked_loss_forward: unknown mode (HGS_MASKED_HUMAN or HGS_MASKED_SCENE)");
    if (C < 1 || H < 1 || W < 1 || C > 65535) return fail_loss("masked_loss_forward: need 1 <= C <= 65535, H >= 1, W >= 1");
    if (!pred || !gt || !mask || !workspace || !out) return fail_loss("masked_loss_forward: null pointer");
    if (mode == HGS_MASKED_HUMAN && !bg) return fail_loss("masked_loss_forward: the human mode needs bg");
    if (((uintptr_t)workspace & 15) != 0) return fail_loss("masked_loss_forward: the workspace must be 16-byte aligned");
    const int64_t tiles = loss_tiles(C, H, W);
    if (tiles > (1ll << 30)) return fail_loss("masked_loss_forward: image too large");
    const dim3 g = loss_grid(tiles);
    const Plane p{C, H, W};
    hipStream_t st = (hipStream_t)stream;
    float4* part = (float4*)workspace;
    if (mode == HGS_MASKED_HUMAN) {
        if (maps) hipLaunchKernelGGL((masked_loss_forward_kernel<LOSS_HUMAN, true>), g, dim3(256), 0, st, p, pred, gt, mask, bg, maps, part);
        else hipLaunchKernelGGL((masked_loss_forward_kernel<LOSS_HUMAN, false>), g, dim3(256), 0, st, p, pred, gt, mask, bg, maps, part);
    } else {
        if (maps) hipLaunchKernelGGL((masked_loss_forward_kernel<LOSS_SCENE, true>), g, dim3(256), 0, st, p, pred, gt, mask, bg, maps, part);
        else hipLaunchKernelGGL((masked_loss_forward_kernel<LOSS_SCENE, false>), g, dim3(256), 0, st, p, pred, gt, mask, bg, maps, part);
    }
    hipLaunchKernelGGL(masked_loss_reduce_kernel, dim3(1), dim3(256), 0, st, (int)tiles, (const float4*)workspace, (double)C * H * W,
                       (double)H * W, out);
    if (hipGetLastError() != hipSuccess) {
        hgs::set_last_error("masked_loss_forward: kernel launch failed");
        return HGS_ERR_HIP;
    }
    return HGS_OK;
}

extern "C" int32_t hgs_masked_loss_backward(int32_t mode, int32_t C, int32_t H, int32_t W, const float* pred, const float* gt,
                                            const float* mask, const float* bg, const float* maps, const float* terms,
                                            const float* g_l1, const float* g_ssim_term, float* dL_dpred, void* stream)
{
    if (mode != HGS_MASKED_HUMAN && mode != HGS_MASKED_SCENE) return fail_loss("masked_loss_backward: unknown mode (HGS_MASKED_HUMAN or HGS_MASKED_SCENE)");
    if (C < 1 || H < 1 || W < 1 || C > 65535) return fail_loss("masked_loss_backward: need 1 <= C <= 65535, H >= 1, W >= 1");
    if (!pred || !gt || !mask || !terms || !dL_dpred) return fail_loss("masked_loss_backward: null pointer");
    if (mode == HGS_MASKED_HUMAN && !bg) return fail_loss("masked_loss_backward: the human mode needs bg");
    if (g_ssim_term && !maps) return fail_loss("masked_loss_backward: a gradient of the SSIM term needs forward's maps");
    const int64_t tiles = loss_tiles(C, H, W);
    if (tiles > (1ll << 30)) return fail_loss("masked_loss_backward: image too large");
    const dim3 g = loss_grid(tiles);
    const Plane p{C, H, W};
    const float* m = g_ssim_term ? maps : nullptr;
    if (mode == HGS_MASKED_HUMAN)
        hipLaunchKernelGGL(masked_loss_backward_kernel<LOSS_HUMAN>, g, dim3(256), 0, (hipStream_t)stream, p, pred, gt, mask, bg, m, terms,
                           g_l1, g_ssim_term, dL_dpred);
    else
        hipLaunchKernelGGL(masked_loss_backward_kernel<LOSS_SCENE>, g, dim3(256), 0, (hipStream_t)stream, p, pred, gt, mask, bg, m, terms,
                           g_l1, g_ssim_term, dL_dpred);
    if (hipGetLastError() != hipSuccess) {
        hgs::set_last_error("masked_loss_backward: kernel launch failed");
        return HGS_ERR_HIP;
    }
    return HGS_OK;
}
