// Row f-5 (the consumer on the other side of the rasterizer's output): the photometric loss of every training step,
//   l1_loss(pred, gt)            /root/reference/hugs/losses/utils.py:54-58
//   ssim(pred, gt)               /root/reference/hugs/losses/utils.py:65-108 (11x11 Gaussian window, sigma 1.5, zero padding,
//                                groups = channels, C1 = 0.01^2, C2 = 0.03^2, mean over everything)
// called on the full render and again on the human-only render (hugs/losses/loss.py:88-107,128-137).  The reference spends
// five depthwise 11x11 conv2d + ~15 elementwise kernels on it forward and the same again backward, on 1080p images: more GPU
// time than the rasterizer's own forward + backward.  Here: one forward kernel (both images read once, the five windowed
// moments through LDS, separable: 11 + 11 taps instead of 121), one 256-thread reduction, one backward kernel.
//
// Forward, per pixel (mu1 = w*x, mu2 = w*y, E11 = w*x^2, E22 = w*y^2, E12 = w*xy; * = zero-padded correlation):
//   A = 2 mu1 mu2 + C1,  B = 2 (E12 - mu1 mu2) + C2,  Cc = mu1^2 + mu2^2 + C1,  D = (E11 - mu1^2) + (E22 - mu2^2) + C2
//   map = A B / (Cc D)
// and, for the backward (x = pred is the only differentiable input, as at every reference call site), the three partials
//   m1 = dmap/dmu1 = 2 mu2 (B - A)/(Cc D) - 2 mu1 map (1/Cc - 1/D),   m2 = dmap/dE11 = -map / D,   m3 = dmap/dE12 = 2 A/(Cc D)
// are stored; backward is the adjoint of the three correlations (the window is symmetric):
//   dL/dx = g_ssim/(C H W) [ w*m1 + 2 x (w*m2) + y (w*m3) ] + g_l1 sign(x - y)
// Tiles of 64 x 16 pixels per 256-thread workgroup, halo 5.  Both kernels move ~4 bytes per pixel and quantity once; the
// arithmetic (110 FMAs per pixel forward) and the LDS traffic are what the time goes into, not HBM.
// Sums: per-workgroup partials, added up in a fixed order in double by the reduction kernel (no float atomics: the same loss
// bit for bit on every run).
#include "loss_tile.h"

namespace {

template <bool WITH_MAPS>
__global__ void __launch_bounds__(256)
ssim_l1_forward_kernel(Plane p, const float* __restrict__ img1, const float* __restrict__ img2, float* __restrict__ maps,
                       float2* __restrict__ partial)
{
    ssim_l1_forward_tile<LOSS_PLAIN, WITH_MAPS>(p, img1, img2, nullptr, nullptr, maps, partial);
}

// out[0] = mean of the SSIM map, out[1] = mean |x - y|, out[2] = sum |x - y| (l1_loss with a mask divides it by mask.sum())
__global__ void __launch_bounds__(256) ssim_l1_reduce_kernel(int blocks, const float2* __restrict__ partial, double count, float* __restrict__ out)
{
    __shared__ double sa[256], sb[256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 256) a += (double)partial[i].x, b += (double)partial[i].y;
    sa[threadIdx.x] = a, sb[threadIdx.x] = b;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) sa[threadIdx.x] += sa[threadIdx.x + d], sb[threadIdx.x] += sb[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(sa[0] / count), out[1] = (float)(sb[0] / count), out[2] = (float)sb[0];
}

__global__ void __launch_bounds__(256)
ssim_l1_backward_kernel(Plane p, const float* __restrict__ img1, const float* __restrict__ img2, const float* __restrict__ maps,
                        const float* __restrict__ g_ssim_mean, const float* __restrict__ g_l1_sum, float* __restrict__ dL_dimg1)
{
    ssim_l1_backward_tile<LOSS_PLAIN>(p, img1, img2, nullptr, nullptr, maps, g_ssim_mean, g_l1_sum, nullptr, dL_dimg1);
}

}  // namespace

extern "C" size_t hgs_ssim_l1_workspace(int32_t C, int32_t H, int32_t W)
{
    if (C < 1 || H < 1 || W < 1) return 0;
    return sizeof(float2) * (size_t)loss_tiles(C, H, W);
}

extern "C" int32_t hgs_ssim_l1_forward(int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, float* maps,
                                       void* workspace, float* out, void* stream)
{
    if (C < 1 || H < 1 || W < 1 || C > 65535) return fail_loss("ssim_l1_forward: need 1 <= C <= 65535, H >= 1, W >= 1");
    if (!img1 || !img2 || !workspace || !out) return fail_loss("ssim_l1_forward: null pointer");
    if (((uintptr_t)workspace & 7) != 0) return fail_loss("ssim_l1_forward: the workspace must be 8-byte aligned");
    const int64_t tiles = loss_tiles(C, H, W);
    if (tiles > (1ll << 30)) return fail_loss("ssim_l1_forward: image too large");
    const dim3 g = loss_grid(tiles);
    const Plane p{C, H, W};
    hipStream_t st = (hipStream_t)stream;
    if (maps) hipLaunchKernelGGL(ssim_l1_forward_kernel<true>, g, dim3(256), 0, st, p, img1, img2, maps, (float2*)workspace);
    else hipLaunchKernelGGL(ssim_l1_forward_kernel<false>, g, dim3(256), 0, st, p, img1, img2, maps, (float2*)workspace);
    hipLaunchKernelGGL(ssim_l1_reduce_kernel, dim3(1), dim3(256), 0, st, (int)tiles, (const float2*)workspace,
                       (double)C * H * W, out);
    if (hipGetLastError() != hipSuccess) {
        hgs::set_last_error("ssim_l1_forward: kernel launch failed");
        return HGS_ERR_HIP;
    }
    return HGS_OK;
}

extern "C" int32_t hgs_ssim_l1_backward(int32_t C, int32_t H, int32_t W, const float* img1, const float* img2, const float* maps,
                                        const float* g_ssim_mean, const float* g_l1_sum, float* dL_dimg1, void* stream)
{
    if (C < 1 || H < 1 || W < 1 || C > 65535) return fail_loss("ssim_l1_backward: need 1 <= C <= 65535, H >= 1, W >= 1");
    if (!img1 || !img2 || !dL_dimg1) return fail_loss("ssim_l1_backward: null pointer");
    if (g_ssim_mean && !maps) return fail_loss("ssim_l1_backward: a gradient of the SSIM term needs forward's maps");
    const int64_t tiles = loss_tiles(C, H, W);
    if (tiles > (1ll << 30)) return fail_loss("ssim_l1_backward: image too large");
    const dim3 g = loss_grid(tiles);
    hipLaunchKernelGGL(ssim_l1_backward_kernel, g, dim3(256), 0, (hipStream_t)stream, Plane{C, H, W}, img1, img2,
                       g_ssim_mean ? maps : nullptr, g_ssim_mean, g_l1_sum, dL_dimg1);
    if (hipGetLastError() != hipSuccess) {
        hgs::set_last_error("ssim_l1_backward: kernel launch failed");
        return HGS_ERR_HIP;
    }
    return HGS_OK;
}
