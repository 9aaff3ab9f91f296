// The device code of row f-5 that loss.hip (l1_loss + ssim on the images as they are) and masked_loss.hip (the same two terms on
// HumanSceneLoss's masked composites) share: the tile geometry, the XCD banding, the tile loaders and the two kernel bodies, with
// the composite as a template parameter.  LOSS_PLAIN instantiates exactly the statements loss.hip had before the masks came.
#pragma once
#include "hgs_common.h"

namespace {

// what a tile holds once it is in LDS (x from the render `pred`, y from the target `gt`, m the [H,W] mask, bg one colour per channel):
//   LOSS_PLAIN   x = pred,            y = gt
//   LOSS_HUMAN   x = pred,            y = gt * m + bg_c * (1 - m)          hugs/losses/loss.py:71,130
//   LOSS_SCENE   x = pred * (1 - m),  y = gt * (1 - m)                     hugs/losses/loss.py:78-80
// (the two masked values equal HGS_MASKED_HUMAN / HGS_MASKED_SCENE of the header)
enum { LOSS_PLAIN = 0, LOSS_HUMAN = 1, LOSS_SCENE = 2 };

constexpr int SSIM_R = 5, SSIM_TW = 64, SSIM_TH = 16, SSIM_IW = SSIM_TW + 2 * SSIM_R, SSIM_IH = SSIM_TH + 2 * SSIM_R;
constexpr int SSIM_SEG = 8;  // columns per thread in the horizontal pass
// gauss(11, 1.5) / sum, in fp32 as the reference builds it (utils.py:65-67)
__host__ __device__ constexpr float ssim_w(int k)  // (a function, so that the unrolled loops see literals)
{
    constexpr float W[6] = {1.028380124e-03f, 7.598758209e-03f, 3.600077331e-02f, 1.093606874e-01f, 2.130055279e-01f, 2.660117149e-01f};
    return W[k < 6 ? k : 10 - k];
}

struct Plane {
    int C, H, W;
    __device__ __forceinline__ size_t at(int c, int y, int x) const { return ((size_t)c * H + y) * W + x; }
};

// LDS tile: rows of SSIM_LW floats, image column x0 - SSIM_PAD + c at position c -- the halo (5) is padded to 8 so that a row
// starts on a 16-byte boundary of the image row and is fetched as float4s (when W is a multiple of 4 and the plane is 16-byte
// aligned; x0 is a multiple of 64)
constexpr int SSIM_PAD = 8, SSIM_LW = SSIM_TW + 2 * SSIM_PAD, SSIM_OFF = SSIM_PAD - SSIM_R;  // 80 columns; the window starts at column 3
typedef float TileRow[SSIM_LW + 1];

// Workgroup -> tile.  Consecutive workgroups are dealt round-robin to the 8 XCDs, each with its own L2; a tile shares 5-pixel halos
// with its neighbours, so every XCD gets a contiguous BAND of the (channel, row, column) tile order instead of every 8th tile:
// workgroup b works on tile (b % 8) * ceil(T / 8) + b / 8 (the grid is 8 * ceil(T / 8) workgroups; the surplus leaves at once).
// 1080p: forward 57.7 -> 53.5 us, backward 49.1 -> 37.4 us.
struct TileId { int ch, x0, y0, linear; bool valid; };
__device__ __forceinline__ TileId tile_of_workgroup(int tiles_x, int tiles_y, int C)
{
    const int T = tiles_x * tiles_y * C, per = (T + 7) / 8;
    const int t = (int)(blockIdx.x & 7u) * per + (int)(blockIdx.x >> 3);
    const int ch = t / (tiles_x * tiles_y), r = t - ch * (tiles_x * tiles_y), ty = r / tiles_x;
    return {ch, (r - ty * tiles_x) * SSIM_TW, ty * SSIM_TH, t, t < T && (int)(blockIdx.x >> 3) < per};
}

// loads the tile + halo of one channel (`src`: the channel's H x W plane) into LDS, zero outside the image
__device__ __forceinline__ void load_tile(TileRow* dst, int x0, int y0, int H, int W, const float* __restrict__ src)
{
    if ((W & 3) == 0 && ((uintptr_t)src & 15) == 0) {
        for (int idx = threadIdx.x; idx < SSIM_IH * (SSIM_LW / 4); idx += 256) {
            const int r = idx / (SSIM_LW / 4), c = (idx - r * (SSIM_LW / 4)) * 4;
            const int gy = y0 - SSIM_R + r, gx = x0 - SSIM_PAD + c;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *reinterpret_cast<const float4*>(src + (size_t)gy * W + gx);
            dst[r][c] = v.x, dst[r][c + 1] = v.y, dst[r][c + 2] = v.z, dst[r][c + 3] = v.w;
        }
    } else {
        for (int idx = threadIdx.x; idx < SSIM_IH * SSIM_IW; idx += 256) {
            const int r = idx / SSIM_IW, c = idx - r * SSIM_IW;
            const int gy = y0 - SSIM_R + r, gx = x0 - SSIM_R + c;
            dst[r][c + SSIM_OFF] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? src[(size_t)gy * W + gx] : 0.0f;
        }
    }
}

// one pixel of a masked composite, every product and the sum rounded on its own as the reference's eager statements round them (the
// library is built with -ffp-contract=off: nothing here becomes an FMA).  KIND = LOSS_HUMAN is the target's composite, LOSS_SCENE
// either image's.
template <int KIND>
__device__ __forceinline__ float composite(float v, float m, float bg)
{
    const float inv = 1.0f - m;
    if constexpr (KIND == LOSS_HUMAN) {
        const float a = v * m, b = bg * inv;
        return a + b;
    } else {
        return v * inv;
    }
}

// load_tile with the composite applied on the way into LDS: no composited image exists in memory.  `msk` is the [H,W] mask plane.  A
// halo pixel outside the image is 0 (conv2d's zero padding of the composited image), not bg.  The float4 path needs the mask plane
// to meet the images' condition too; the scalar path stores the same values.
template <int KIND>
__device__ __forceinline__ void load_tile_masked(TileRow* dst, int x0, int y0, int H, int W, const float* __restrict__ src,
                                                 const float* __restrict__ msk, float bg)
{
    if ((W & 3) == 0 && (((uintptr_t)src | (uintptr_t)msk) & 15) == 0) {
        for (int idx = threadIdx.x; idx < SSIM_IH * (SSIM_LW / 4); idx += 256) {
            const int r = idx / (SSIM_LW / 4), c = (idx - r * (SSIM_LW / 4)) * 4;
            const int gy = y0 - SSIM_R + r, gx = x0 - SSIM_PAD + c;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const float4 v = *reinterpret_cast<const float4*>(src + (size_t)gy * W + gx);
                const float4 m = *reinterpret_cast<const float4*>(msk + (size_t)gy * W + gx);
                o = make_float4(composite<KIND>(v.x, m.x, bg), composite<KIND>(v.y, m.y, bg), composite<KIND>(v.z, m.z, bg),
                                composite<KIND>(v.w, m.w, bg));
            }
            dst[r][c] = o.x, dst[r][c + 1] = o.y, dst[r][c + 2] = o.z, dst[r][c + 3] = o.w;
        }
    } else {
        for (int idx = threadIdx.x; idx < SSIM_IH * SSIM_IW; idx += 256) {
            const int r = idx / SSIM_IW, c = idx - r * SSIM_IW;
            const int gy = y0 - SSIM_R + r, gx = x0 - SSIM_R + c;
            float o = 0.0f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) o = composite<KIND>(src[(size_t)gy * W + gx], msk[(size_t)gy * W + gx], bg);
            dst[r][c + SSIM_OFF] = o;
        }
    }
}

// The forward of one tile.  LOSS_PLAIN: `partial` is float2 per tile {sum of the SSIM map, sum |x - y|}.  Masked: float4 per tile, .z =
// the sum of the mask over the tile's pixels on the tiles of channel 0 and 0 on the others (sum(m) is taken once, not once per
// channel), .w = 0.
template <int MODE, bool WITH_MAPS>
__device__ __forceinline__ void ssim_l1_forward_tile(Plane p, const float* __restrict__ img1, const float* __restrict__ img2,
                                                     const float* __restrict__ mask, const float* __restrict__ bg,
                                                     float* __restrict__ maps, void* __restrict__ partial)
{
    // the two image tiles stay in LDS; the five windowed moments go one at a time through ONE row-sum buffer (24 KB of LDS
    // instead of 51, registers for one moment at a time: six workgroups per CU instead of three)
    __shared__ TileRow sx[SSIM_IH], sy[SSIM_IH];
    __shared__ float hq[SSIM_IH][SSIM_TW + 1];
    __shared__ float2 wsum[4];
    __shared__ float wmask[MODE != LOSS_PLAIN ? 4 : 1];  // (LOSS_PLAIN never touches it: not allocated)
    const TileId tile = tile_of_workgroup((p.W + SSIM_TW - 1) / SSIM_TW, (p.H + SSIM_TH - 1) / SSIM_TH, p.C);
    if (!tile.valid) return;  // (uniform)
    const int ch = tile.ch, x0 = tile.x0, y0 = tile.y0, tid = threadIdx.x;
    if constexpr (MODE == LOSS_PLAIN) {
        load_tile(sx, x0, y0, p.H, p.W, img1 + (size_t)ch * p.H * p.W);
        load_tile(sy, x0, y0, p.H, p.W, img2 + (size_t)ch * p.H * p.W);
    } else if constexpr (MODE == LOSS_HUMAN) {
        load_tile(sx, x0, y0, p.H, p.W, img1 + (size_t)ch * p.H * p.W);
        load_tile_masked<LOSS_HUMAN>(sy, x0, y0, p.H, p.W, img2 + (size_t)ch * p.H * p.W, mask, bg[ch]);
    } else {
        load_tile_masked<LOSS_SCENE>(sx, x0, y0, p.H, p.W, img1 + (size_t)ch * p.H * p.W, mask, 0.0f);
        load_tile_masked<LOSS_SCENE>(sy, x0, y0, p.H, p.W, img2 + (size_t)ch * p.H * p.W, mask, 0.0f);
    }
    const int col = tid & (SSIM_TW - 1), r0 = (tid / SSIM_TW) * 4;
    if constexpr (MODE != LOSS_PLAIN) {
        // sum(m) over the tile's own pixels, on channel 0's tiles only -- here, before the moments, where no register is scarce (in
        // the epilogue it cost the kernel a wave per SIMD); the rows were fetched for the tile a moment ago
        float mask_sum = 0.f;
        if (ch == 0) {  // (uniform)
#pragma unroll
            for (int o = 0; o < 4; ++o)
                if (x0 + col < p.W && y0 + r0 + o < p.H) mask_sum += mask[(size_t)(y0 + r0 + o) * p.W + x0 + col];
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mask_sum += __shfl_xor(mask_sum, d, 64);
        if ((tid & 63) == 0) wmask[tid >> 6] = mask_sum;
    }
    float acc[5][4];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        __syncthreads();  // (the tiles are loaded / the previous moment's vertical pass is done with hq)
        // horizontal pass: a thread = one row, 8 adjacent columns (18 inputs in registers)
        if (tid < SSIM_IH * (SSIM_TW / SSIM_SEG)) {
            const int row = tid / (SSIM_TW / SSIM_SEG), c0 = (tid - row * (SSIM_TW / SSIM_SEG)) * SSIM_SEG;
            float v[SSIM_SEG + 2 * SSIM_R];
#pragma unroll
            for (int j = 0; j < SSIM_SEG + 2 * SSIM_R; ++j) {
                const float xv = sx[row][c0 + j + SSIM_OFF], yv = sy[row][c0 + j + SSIM_OFF];
                v[j] = q == 0 ? xv : q == 1 ? yv : q == 2 ? xv * xv : q == 3 ? yv * yv : xv * yv;
            }
#pragma unroll
            for (int o = 0; o < SSIM_SEG; ++o) {
                float t = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) t = __builtin_fmaf(ssim_w(k), v[o + k], t);
                hq[row][c0 + o] = t;
            }
        }
        __syncthreads();
        // vertical pass: a thread = one column, 4 adjacent rows
        float v[4 + 2 * SSIM_R];
#pragma unroll
        for (int j = 0; j < 4 + 2 * SSIM_R; ++j) v[j] = hq[r0 + j][col];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < 11; ++k) t = __builtin_fmaf(ssim_w(k), v[o + k], t);
            acc[q][o] = t;
        }
    }
    const float C1 = 0.0001f, C2 = 0.0009f;
    float ssim_sum = 0.f, l1_sum = 0.f;
    const int gx = x0 + col;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = y0 + r0 + o;
        if (gx < p.W && gy < p.H) {
            const float mu1 = acc[0][o], mu2 = acc[1][o], mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = acc[2][o] - mu1_sq, s2 = acc[3][o] - mu2_sq, s12 = acc[4][o] - mu12;
            const float A = 2.0f * mu12 + C1, B = 2.0f * s12 + C2, Cc = mu1_sq + mu2_sq + C1, D = s1 + s2 + C2;
            const float map = (A * B) / (Cc * D);
            ssim_sum += map;
            l1_sum += fabsf(sx[r0 + o + SSIM_R][col + SSIM_PAD] - sy[r0 + o + SSIM_R][col + SSIM_PAD]);
            if (WITH_MAPS) {
                // (the map itself is the reference's expression, correctly rounded; its partials take the 1-ulp reciprocals)
                const float inv_c = __builtin_amdgcn_rcpf(Cc), inv_d = __builtin_amdgcn_rcpf(D), inv_cd = inv_c * inv_d;
                const size_t at = p.at(ch, gy, gx), plane = (size_t)p.C * p.H * p.W;
                maps[at] = 2.0f * mu2 * (B - A) * inv_cd - 2.0f * mu1 * map * (inv_c - inv_d);
                maps[plane + at] = -map * inv_d;
                maps[2 * plane + at] = 2.0f * A * inv_cd;
            }
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) ssim_sum += __shfl_xor(ssim_sum, d, 64), l1_sum += __shfl_xor(l1_sum, d, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = make_float2(ssim_sum, l1_sum);
    if constexpr (MODE != LOSS_PLAIN) {
        __syncthreads();
        if (tid == 0)
            static_cast<float4*>(partial)[tile.linear] =
                make_float4((wsum[0].x + wsum[1].x) + (wsum[2].x + wsum[3].x), (wsum[0].y + wsum[1].y) + (wsum[2].y + wsum[3].y),
                            (wmask[0] + wmask[1]) + (wmask[2] + wmask[3]), 0.0f);
    } else {
        __syncthreads();
        if (tid == 0) {
            const float2 s = make_float2((wsum[0].x + wsum[1].x) + (wsum[2].x + wsum[3].x), (wsum[0].y + wsum[1].y) + (wsum[2].y + wsum[3].y));
            static_cast<float2*>(partial)[tile.linear] = s;
        }
    }
}

// The backward of one tile: dL/dimg1 = s [ gs (w*m1 + 2 x (w*m2) + y (w*m3)) + gl sign(x - y) ], x and y recomposed from the inputs in
// the epilogue; s = d x / d img1 = 1, or 1 - m in LOSS_SCENE.  `maps` may be null when g_ssim is (no gradient of the SSIM term).
template <int MODE>
__device__ __forceinline__ void ssim_l1_backward_tile(Plane p, const float* __restrict__ img1, const float* __restrict__ img2,
                                                      const float* __restrict__ mask, const float* __restrict__ bg,
                                                      const float* __restrict__ maps, const float* __restrict__ g_ssim,
                                                      const float* __restrict__ g_l1, const float* __restrict__ terms,
                                                      float* __restrict__ dL_dimg1)
{
    // one quantity at a time through ONE tile and ONE row-sum buffer (15 KB of LDS instead of 46: eight workgroups per CU instead
    // of three -- this kernel waits on memory, not on arithmetic)
    __shared__ TileRow sm[SSIM_IH];
    __shared__ float hq[SSIM_IH][SSIM_TW + 1];
    const TileId tile = tile_of_workgroup((p.W + SSIM_TW - 1) / SSIM_TW, (p.H + SSIM_TH - 1) / SSIM_TH, p.C);
    if (!tile.valid) return;  // (uniform)
    const int ch = tile.ch, x0 = tile.x0, y0 = tile.y0, tid = threadIdx.x;
    const size_t plane = (size_t)p.C * p.H * p.W;
    // gs: the factor of the SSIM map's SUM, gl: of sum |x - y| -- from the upstream gradients, DEVICE scalars, either may be null (= 0).
    // LOSS_PLAIN: g_ssim is the gradient of the map's mean, g_l1 of the l1 sum.  Masked: they are the gradients of the two terms
    // ssim_term = (1 - mean) sum(m) / (H W) and l1 = sum |x - y| / sum(m), and terms[2] is forward's sum(m).
    float gs, gl;
    if constexpr (MODE == LOSS_PLAIN) {
        gs = g_ssim ? g_ssim[0] / (float)((double)p.C * p.H * p.W) : 0.0f, gl = g_l1 ? g_l1[0] : 0.0f;
    } else {
        const float area = terms[2];
        gs = g_ssim ? g_ssim[0] * -(area / (float)((double)p.H * p.W)) / (float)((double)p.C * p.H * p.W) : 0.0f;
        gl = g_l1 ? g_l1[0] / area : 0.0f;
    }
    const int col = tid & (SSIM_TW - 1), r0 = (tid / SSIM_TW) * 4;
    float acc[3][4] = {};
    if (maps) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            load_tile(sm, x0, y0, p.H, p.W, maps + q * plane + (size_t)ch * p.H * p.W);
            __syncthreads();  // (also: the previous quantity's vertical pass is done with hq)
            if (tid < SSIM_IH * (SSIM_TW / SSIM_SEG)) {
                const int row = tid / (SSIM_TW / SSIM_SEG), c0 = (tid - row * (SSIM_TW / SSIM_SEG)) * SSIM_SEG;
                float v[SSIM_SEG + 2 * SSIM_R];
#pragma unroll
                for (int j = 0; j < SSIM_SEG + 2 * SSIM_R; ++j) v[j] = sm[row][c0 + j + SSIM_OFF];
#pragma unroll
                for (int o = 0; o < SSIM_SEG; ++o) {
                    float t = 0.f;
#pragma unroll
                    for (int k = 0; k < 11; ++k) t = __builtin_fmaf(ssim_w(k), v[o + k], t);
                    hq[row][c0 + o] = t;
                }
            }
            __syncthreads();  // (also: the horizontal pass is done with sm, the next quantity may overwrite it)
            float v[4 + 2 * SSIM_R];
#pragma unroll
            for (int j = 0; j < 4 + 2 * SSIM_R; ++j) v[j] = hq[r0 + j][col];
#pragma unroll
            for (int o = 0; o < 4; ++o) {
                float t = 0.f;
#pragma unroll
                for (int k = 0; k < 11; ++k) t = __builtin_fmaf(ssim_w(k), v[o + k], t);
                acc[q][o] = t;
            }
        }
    }
    const int gx = x0 + col;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int gy = y0 + r0 + o;
        if (gx < p.W && gy < p.H) {
            const size_t at = p.at(ch, gy, gx);
            float x = img1[at], y = img2[at];
            if constexpr (MODE == LOSS_HUMAN) y = composite<LOSS_HUMAN>(y, mask[(size_t)gy * p.W + gx], bg[ch]);
            float s = 1.0f;
            if constexpr (MODE == LOSS_SCENE) {
                const float m = mask[(size_t)gy * p.W + gx];
                x = composite<LOSS_SCENE>(x, m, 0.0f), y = composite<LOSS_SCENE>(y, m, 0.0f), s = 1.0f - m;
            }
            const float d = x - y;
            const float sign = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
            const float g = gs * (acc[0][o] + 2.0f * x * acc[1][o] + y * acc[2][o]) + gl * sign;
            dL_dimg1[at] = MODE == LOSS_SCENE ? s * g : g;
        }
    }
}

int fail_loss(const char* what)
{
    hgs::set_last_error(what);
    return HGS_ERR_INVALID_ARGUMENT;
}

// number of tiles, and the 1-D grid that covers them in XCD bands (tile_of_workgroup)
int64_t loss_tiles(int C, int H, int W) { return (int64_t)((W + SSIM_TW - 1) / SSIM_TW) * ((H + SSIM_TH - 1) / SSIM_TH) * C; }
dim3 loss_grid(int64_t tiles) { return dim3((unsigned)(((tiles + 7) / 8) * 8)); }

}  // namespace
