// Row f-9 (the three decoders behind the triplane features): /root/reference/hugs/models/modules/decoders.py:24-111, called at
// /root/reference/hugs/models/hugs_trimlp.py:409-410,430 -- a TRUNK of 1..3 Linear + exact GELU layers and, off its last activation,
// 1..3 HEADS (one Linear each, activation none / exact GELU / sigmoid), as one kernel forward and one backward, fp32 throughout on
// v_mfma_f32_32x32x2_f32 (exact f32: a k-ordered fmaf chain).
//
// Mapping.  A workgroup of 4 waves takes a tile of MLP_TILE = 32 points at a time.  Everything on chip is CHANNEL-major,
// buf[channel][point] with a row stride of 33 floats, so that all three products read both operands with conflict-free ds_read_b32:
//   forward   Z[o][p]  = sum_c W[o][c] a[c][p]     A = W (LDS, natural [o][c] layout, odd row stride), B = a rows c
//   backward  G[c][p]  = sum_o W[o][c] gz[o][p]    A = W read down a column,                           B = gz rows o
//   weights   dW[o][c] = sum_p gz[o][p] a[c][p]    A = gz read along a row (stride 33: bank = row + p), B = a along a row
// 32x32x2: lane l supplies A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31] and holds D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31]
// in result register r.  A result tile therefore has the POINT on the lane (forward, backward) and goes back to LDS as 32 consecutive
// floats per register.  Wave w owns output tile w of a layer (rows 32 w ..); a 64-wide layer leaves waves 2 and 3 without a product.
// Weights come through LDS in chunks of 64 of the summed index.  The backward recomputes the trunk keeping, per layer, the activation
// a = gelu(z) and the derivative d = gelu'(z) (one erf and one exp per element, once), turns d into gz = d * G in place, and keeps
// every dW tile in accumulator registers ACROSS the tiles a workgroup walks (the grid is one workgroup per CU): one flush of float
// atomics per workgroup at the end, 32 consecutive floats (one 128-byte segment) per wave half and instruction.
#include "hgs_common.h"

namespace {

typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int MLP_TILE = 32;          // points per tile
constexpr int S = MLP_TILE + 1;       // row stride of the channel-major buffers
constexpr int KC = 64;                // summed-index chunk of a staged weight block
constexpr int BUF = 128 * S;          // one activation buffer (up to 128 channels)
constexpr int HB = 64 * S;            // the heads' buffer (up to 64 concatenated head columns)
constexpr int WB = 128 * (KC + 1);    // staged weights: 128 rows x 64 columns (stride 65) or 64 rows x 128 columns (stride 129)
constexpr int MAXL = HGS_MLP_MAX_TRUNK, MAXH = HGS_MLP_MAX_HEADS;

struct MlpParams {
    int n, in, nheads, ho, ho_pad;    // ho: head columns in all; ho_pad: rounded up to 32
    int off[MAXH + 1];                // first concatenated row of each head
    int act[MAXH];
    const float* W[MAXL]; const float* b[MAXL]; const float* Wh[MAXH]; const float* bh[MAXH];
    const float* x;
    float* out[MAXH];                 // forward
    const float* gy[MAXH];            // backward: upstream gradients (NULL: that head is unused)
    float* dx; float* dW[MAXL]; float* db[MAXL]; float* dWh[MAXH]; float* dbh[MAXH];
    bool any_dwh;
};

__device__ __forceinline__ int drow(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }
__device__ __forceinline__ v16f mfma(float a, float b, v16f c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }

constexpr float SQRT1_2 = 0.70710678118654752440f, INV_SQRT_2PI = 0.39894228040143267794f;
// a = gelu(z) = z Phi(z), d = gelu'(z) = Phi(z) + z phi(z)
__device__ __forceinline__ void gelu(float z, float& a, float& d)
{
    const float cdf = 0.5f * (1.0f + erff(z * SQRT1_2));
    a = z * cdf;
    d = cdf + z * (expf(-0.5f * z * z) * INV_SQRT_2PI);
}
__device__ __forceinline__ void head_act(int code, float z, float& y, float& d)
{
    if (code == HGS_MLP_ACT_GELU) gelu(z, y, d);
    else if (code == HGS_MLP_ACT_SIGMOID) { y = 1.0f / (1.0f + expf(-z)); d = y * (1.0f - y); }
    else { y = z; d = 1.0f; }
}

// q / m for the m = ncols / 32 in {1, 2, 3, 4} the supported widths give (q < 2^15)
__device__ __forceinline__ int div_m(int q, int m) { return m == 1 ? q : m == 2 ? q >> 1 : m == 4 ? q >> 2 : (q * 43691) >> 17; }

// rows [row0, row0 + nrows) x columns [col0, col0 + ncols) of a row-major matrix of row length ld -> wb[r * ws + c]; ncols a multiple of 32.
// Eight loads per thread in flight before the first LDS write (a loop of one load and one write each waits out every L2 round trip).
__device__ __forceinline__ void stage(float* wb, int ws, const float* __restrict__ W, int ld, int row0, int nrows, int col0, int ncols, int tid)
{
    const int m = ncols >> 5, total = nrows * ncols;
    const float* src = W + (size_t)row0 * ld + col0;
    for (int e0 = tid; e0 < total; e0 += 256 * 8) {
        float v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + 256 * k, r = div_m(e >> 5, m), c = e - r * ncols;
            v[k] = e < total ? src[r * ld + c] : 0.0f;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int e = e0 + 256 * k, r = div_m(e >> 5, m), c = e - r * ncols;
            if (e < total) wb[r * ws + c] = v[k];
        }
    }
}
// the heads' weights as ONE block of ho_pad rows (rows past the last head: zero)
__device__ __forceinline__ void stage_heads(float* wb, int ws, const MlpParams& P, int ld, int col0, int ncols, int tid)
{
    for (int hd = 0; hd < P.nheads; ++hd) stage(wb + P.off[hd] * ws, ws, P.Wh[hd], ld, 0, P.off[hd + 1] - P.off[hd], col0, ncols, tid);
    const int c32 = tid & 31;
    for (int r = P.ho + (tid >> 5); r < P.ho_pad; r += 8)
        for (int c = c32; c < ncols; c += 32) wb[r * ws + c] = 0.0f;
}
__device__ __forceinline__ int head_of(const MlpParams& P, int o) { return o < P.off[1] ? 0 : o < P.off[2] ? 1 : 2; }

// Z[o0 + i][p] += sum_{k < kw} wb[(o0 + i) ws + k] act[k S + p]
__device__ __forceinline__ void prod_f(v16f& acc, const float* wb, int ws, int o0, const float* act, int kw, int lane)
{
    const int i = lane & 31, h = lane >> 5;
    const float* pa = wb + (o0 + i) * ws + h;
    const float* pb = act + h * S + i;
    for (int s0 = 0; s0 < kw / 2; s0 += 8)   // kw is a multiple of 32
#pragma unroll
        for (int s = s0; s < s0 + 8; ++s) acc = mfma(pa[2 * s], pb[2 * s * S], acc);
}
// G[c0 + i][p] += sum_{o < kw} wb[o ws + c0 + i] gz[o S + p]
__device__ __forceinline__ void prod_b(v16f& acc, const float* wb, int ws, int c0, const float* gz, int kw, int lane)
{
    const int i = lane & 31, h = lane >> 5;
    const float* pa = wb + h * ws + c0 + i;
    const float* pb = gz + h * S + i;
    for (int s0 = 0; s0 < kw / 2; s0 += 8)
#pragma unroll
        for (int s = s0; s < s0 + 8; ++s) acc = mfma(pa[2 * s * ws], pb[2 * s * S], acc);
}
// dW[o0 + i][c0 + j] += sum_{p < 32} gz[(o0 + i) S + p] a[(c0 + j) S + p]
__device__ __forceinline__ void prod_w(v16f& acc, const float* gz, int o0, const float* a, int c0, int lane)
{
    const int i = lane & 31, h = lane >> 5;
    const float* pa = gz + (o0 + i) * S + h;
    const float* pb = a + (c0 + i) * S + h;
#pragma unroll 1
    for (int s0 = 0; s0 < MLP_TILE / 2; s0 += 8)
#pragma unroll
        for (int s = s0; s < s0 + 8; ++s) acc = mfma(pa[2 * s], pb[2 * s], acc);
}
// sum over the tile's points of row `row`
__device__ __forceinline__ float row_sum(const float* buf, int row)
{
    float acc = 0.0f;
#pragma unroll 8
    for (int p = 0; p < MLP_TILE; ++p) acc += buf[row * S + p];
    return acc;
}

constexpr int lds_floats(int L, bool bwd) { return (bwd ? (1 + 2 * L) : 2) * BUF + HB + WB; }

// H: trunk width (64 or 128), L: trunk layers.  LDS: xb | per layer a, d (forward: two buffers in all) | hb | wb
template <int H, int L, bool BWD>
__global__ void __launch_bounds__(256)
mlp_kernel(const MlpParams P)
{
    extern __shared__ __align__(16) float lds[];
    constexpr int NH = H / 32, LOG_NH = H == 128 ? 2 : 1;
    constexpr int EPI = BWD ? 2 : 4;   // activations evaluated side by side (independent chains; registers bound it in the backward)
    float* const xb = lds;
    auto ab = [&](int l) { return lds + BUF * (BWD ? 1 + 2 * l : (l + 1) & 1); };   // forward: x and the activations alternate between two buffers
    auto db = [&](int l) { return lds + BUF * (2 + 2 * l); };   // backward only
    float* const hb = lds + BUF * (BWD ? 1 + 2 * L : 2);
    float* const wb = hb + HB;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, i = lane & 31, h = lane >> 5;
    const int c32 = tid & 31, rgrp = tid >> 5;
    const int NHO = P.ho_pad >> 5;   // 1 or 2 head tiles

    // dW tiles this wave owns: tile t = w + 4 j of a layer is (output tile t % NH, input tile t / NH); of the heads (t % NHO, t / NHO)
    // (at most NH input tiles -> NH tiles per wave in layer 0, NH NH / 4 above it, NH / 2 of the heads)
    constexpr int J0 = NH, JL = NH * NH / 4, JH = NH / 2;
    v16f aw0[J0], awl[L > 1 ? L - 1 : 1][JL], ah[JH];
    float bsum[L], bhsum = 0.0f;
    if (BWD) {
#pragma unroll
        for (int l = 0; l < L; ++l) {
            bsum[l] = 0.0f;
#pragma unroll
            for (int j = 0; j < JL; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) if (l) awl[l ? l - 1 : 0][j][r] = 0.0f;
        }
#pragma unroll
        for (int j = 0; j < J0; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) aw0[j][r] = 0.0f;
#pragma unroll
        for (int j = 0; j < JH; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) ah[j][r] = 0.0f;
    }

    const int tiles = (P.n + MLP_TILE - 1) / MLP_TILE;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const size_t p0 = (size_t)tile * MLP_TILE;
        __syncthreads();   // the last tile's readers of xb / hb are done
        {   // the tile's rows of x are one contiguous run of 32 in floats
            const int m = P.in >> 5, total = MLP_TILE * P.in;
            const float* src = P.x + p0 * P.in;
            const size_t left = ((size_t)P.n - p0) * P.in;
            for (int e0 = tid; e0 < total; e0 += 256 * 8) {
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int e = e0 + 256 * k;
                    v[k] = e < total && (size_t)e < left ? src[e] : 0.0f;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int e = e0 + 256 * k, p = div_m(e >> 5, m), c = e - p * P.in;
                    if (e < total) xb[c * S + p] = v[k];
                }
            }
        }
        for (int p = rgrp; p < MLP_TILE; p += 8) {
            const bool ok = p0 + p < (size_t)P.n;
            if (BWD) {
                for (int hd = 0; hd < P.nheads; ++hd) {
                    const int wh = P.off[hd + 1] - P.off[hd];
                    for (int o = c32; o < wh; o += 32) hb[(P.off[hd] + o) * S + p] = ok && P.gy[hd] ? P.gy[hd][(p0 + p) * wh + o] : 0.0f;
                }
            }
        }

        // ---- the trunk, forward
#pragma unroll
        for (int l = 0; l < L; ++l) {
            const int C = l ? H : P.in;
            const float* in = l ? ab(l - 1) : xb;
            v16f acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            for (int kc = 0; kc < C; kc += KC) {
                const int kw = C - kc < KC ? C - kc : KC;
                __syncthreads();
                stage(wb, KC + 1, P.W[l], C, 0, H, kc, kw, tid);
                __syncthreads();
                if (w < NH) prod_f(acc, wb, KC + 1, 32 * w, in + kc * S, kw, lane);
            }
            if (w < NH) {
                // z to LDS from the registers, then the activation in a loop unrolled only EPI times over the same elements (each lane re-reads what
                // it wrote): sixteen erf evaluations unrolled side by side cost ~150 VGPRs
                float* za = ab(l);
#pragma unroll
                for (int r = 0; r < 16; ++r) za[(32 * w + drow(r, h)) * S + i] = acc[r];
#pragma unroll EPI
                for (int r = 0; r < 16; ++r) {
                    const int o = 32 * w + drow(r, h);
                    float a, d;
                    gelu(za[o * S + i] + P.b[l][o], a, d);
                    za[o * S + i] = a;
                    if (BWD) db(l)[o * S + i] = d;
                }
            }
        }

        // ---- the heads
        {
            const float* in = ab(L - 1);
            v16f acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            for (int kc = 0; kc < H; kc += KC) {
                __syncthreads();
                stage_heads(wb, KC + 1, P, H, kc, KC, tid);
                __syncthreads();
                if (w < NHO) prod_f(acc, wb, KC + 1, 32 * w, in + kc * S, KC, lane);
            }
            if (w < NHO) {
                float* zh = wb + WB - HB;   // z through LDS as in the trunk: the tail of wb, past the 64 rows x 65 the heads' block takes
#pragma unroll
                for (int r = 0; r < 16; ++r) zh[(32 * w + drow(r, h)) * S + i] = acc[r];
#pragma unroll EPI
                for (int r = 0; r < 16; ++r) {
                    const int o = 32 * w + drow(r, h);
                    if (o < P.ho) {
                        const int hd = head_of(P, o);
                        float y, d;
                        head_act(P.act[hd], zh[o * S + i] + P.bh[hd][o - P.off[hd]], y, d);
                        if (BWD) hb[o * S + i] *= d;   // gz = dL/dy * act'(z)
                        else hb[o * S + i] = y;
                    } else if (BWD) hb[o * S + i] = 0.0f;
                }
            }
            __syncthreads();
        }

        if (!BWD) {
            for (int p = rgrp; p < MLP_TILE; p += 8) {
                if (p0 + p >= (size_t)P.n) continue;
                for (int hd = 0; hd < P.nheads; ++hd) {
                    const int wh = P.off[hd + 1] - P.off[hd];
                    for (int o = c32; o < wh; o += 32) P.out[hd][(p0 + p) * wh + o] = hb[(P.off[hd] + o) * S + p];
                }
            }
            continue;
        }

        // ---- backward: the heads' parameter gradients, then dL/d(last activation)
        if (P.any_dwh) {
#pragma unroll
            for (int j = 0; j < JH; ++j) {
                const int t = w + 4 * j;
                if (t < NHO * NH) prod_w(ah[j], hb, 32 * (t & (NHO - 1)), ab(L - 1), 32 * (t >> (NHO - 1)), lane);
            }
            if (tid < P.ho) bhsum += row_sum(hb, tid);
        }
        stage_heads(wb, H + 1, P, H, 0, H, tid);
        __syncthreads();
        if (w < NH) {
            v16f acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            prod_b(acc, wb, H + 1, 32 * w, hb, P.ho_pad, lane);
#pragma unroll
            for (int r = 0; r < 16; ++r) db(L - 1)[(32 * w + drow(r, h)) * S + i] *= acc[r];
        }

        // ---- backward through the trunk: db(l) holds gz_l
#pragma unroll
        for (int l = L - 1; l >= 0; --l) {
            const int C = l ? H : P.in, CT = C >> 5;
            const float* src = l ? ab(l - 1) : xb;
            __syncthreads();
            if (P.dW[l]) {
#pragma unroll
                for (int j = 0; j < (l ? JL : J0); ++j) {
                    const int t = w + 4 * j;
                    if (t < NH * CT) prod_w(l ? awl[l ? l - 1 : 0][j < JL ? j : 0] : aw0[j < J0 ? j : 0], db(l), 32 * (t & (NH - 1)), src, 32 * (t >> LOG_NH), lane);
                }
            }
            if (P.db[l] && tid < H) bsum[l] += row_sum(db(l), tid);
            if (l > 0 || P.dx) {
                v16f acc;
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
                for (int ob = 0; ob < H; ob += KC) {
                    __syncthreads();
                    stage(wb, C + 1, P.W[l], C, ob, KC, 0, C, tid);
                    __syncthreads();
                    if (w < CT) prod_b(acc, wb, C + 1, 32 * w, db(l) + ob * S, KC, lane);
                }
                if (w < CT) {
                    float* dst = l ? db(l - 1) : ab(0);   // l == 0: dL/dx (a_0's last reader was the product for dW of the layer above)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int at = (32 * w + drow(r, h)) * S + i;
                        dst[at] = l ? dst[at] * acc[r] : acc[r];
                    }
                }
            }
        }
        if (P.dx) {
            __syncthreads();
            const float* g0 = ab(0);
            for (int p = rgrp; p < MLP_TILE; p += 8) {
                if (p0 + p >= (size_t)P.n) continue;
                for (int c = c32; c < P.in; c += 32) P.dx[(p0 + p) * P.in + c] = g0[c * S + p];
            }
        }
    }

    if (!BWD) return;
    // ---- flush: one float atomic per element and workgroup, 32 consecutive floats per wave half
#pragma unroll
    for (int l = 0; l < L; ++l) {
        const int C = l ? H : P.in, CT = C >> 5;
        if (P.dW[l]) {
#pragma unroll
            for (int j = 0; j < (l ? JL : J0); ++j) {
                const int t = w + 4 * j;
                if (t >= NH * CT) continue;
                const v16f& acc = l ? awl[l ? l - 1 : 0][j < JL ? j : 0] : aw0[j < J0 ? j : 0];
                const int o0 = 32 * (t & (NH - 1)), c0 = 32 * (t >> LOG_NH);
#pragma unroll
                for (int r = 0; r < 16; ++r) unsafeAtomicAdd(&P.dW[l][(size_t)(o0 + drow(r, h)) * C + c0 + i], acc[r]);
            }
        }
        if (P.db[l] && tid < H) unsafeAtomicAdd(&P.db[l][tid], bsum[l]);
    }
    if (P.any_dwh) {
#pragma unroll
        for (int j = 0; j < JH; ++j) {
            const int t = w + 4 * j;
            if (t >= NHO * NH) continue;
            const int o0 = 32 * (t & (NHO - 1)), c0 = 32 * (t >> (NHO - 1));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = o0 + drow(r, h);
                if (o >= P.ho) continue;
                const int hd = head_of(P, o);
                if (P.dWh[hd]) unsafeAtomicAdd(&P.dWh[hd][(size_t)(o - P.off[hd]) * H + c0 + i], ah[j][r]);
            }
        }
        if (tid < P.ho) {
            const int hd = head_of(P, tid);
            if (P.dbh[hd]) unsafeAtomicAdd(&P.dbh[hd][tid - P.off[hd]], bhsum);
        }
    }
}

int fail_mlp(const char* what)
{
    hgs::set_last_error(what);
    return HGS_ERR_INVALID_ARGUMENT;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the description's own consistency (no pointers beyond the weights): NULL if fine
const char* check_net(int32_t n, const hgs_mlp_desc* net)
{
    if (n < 0) return "need n >= 0";
    if (!net) return "null network description";
    if (net->in_width < 32 || net->in_width > 128 || net->in_width % 32) return "input width must be a multiple of 32 up to 128";
    if (net->n_trunk < 1 || net->n_trunk > MAXL) return "1 to 3 trunk layers";
    for (int l = 0; l < net->n_trunk; ++l) {
        if (net->trunk_width[l] != 64 && net->trunk_width[l] != 128) return "trunk widths must be 64 or 128";
        if (net->trunk_width[l] != net->trunk_width[0]) return "all trunk layers must have the same width";
    }
    if (net->n_heads < 1 || net->n_heads > MAXH) return "1 to 3 heads";
    int total = 0;
    for (int k = 0; k < net->n_heads; ++k) {
        if (net->head_width[k] < 1) return "every head needs at least one column";
        if (net->head_act[k] != HGS_MLP_ACT_NONE && net->head_act[k] != HGS_MLP_ACT_GELU && net->head_act[k] != HGS_MLP_ACT_SIGMOID)
            return "unknown activation code";
        total += net->head_width[k] > 64 ? 65 : net->head_width[k];
    }
    if (total > 64) return "at most 64 head columns in total";
    return nullptr;
}
const char* check_weights(const hgs_mlp_desc* net)
{
    for (int l = 0; l < net->n_trunk; ++l) if (!net->trunk_weight[l] || !net->trunk_bias[l]) return "null trunk weight or bias";
    for (int k = 0; k < net->n_heads; ++k) if (!net->head_weight[k] || !net->head_bias[k]) return "null head weight or bias";
    return nullptr;
}

void fill(MlpParams& P, int32_t n, const hgs_mlp_desc* net, const float* x)
{
    P = MlpParams{};
    P.n = n, P.in = net->in_width, P.nheads = net->n_heads, P.x = x;
    for (int l = 0; l < net->n_trunk; ++l) P.W[l] = net->trunk_weight[l], P.b[l] = net->trunk_bias[l];
    int at = 0;
    for (int k = 0; k < MAXH; ++k) {
        P.off[k] = at;
        if (k < net->n_heads) {
            P.Wh[k] = net->head_weight[k], P.bh[k] = net->head_bias[k], P.act[k] = net->head_act[k];
            at += net->head_width[k];
        }
    }
    P.off[MAXH] = at;
    P.ho = at, P.ho_pad = (at + 31) / 32 * 32;
}

int num_cus()
{
    static const int cus = [] {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256;
        return v;
    }();
    return cus;
}

template <int H, int L, bool BWD>
bool launch_one(const MlpParams& P, int grid, hipStream_t st)
{
    constexpr int bytes = lds_floats(L, BWD) * (int)sizeof(float);
    static_assert(bytes <= 160 * 1024, "LDS of a gfx950 CU");
    static const bool attr = hipFuncSetAttribute((const void*)mlp_kernel<H, L, BWD>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess;
    if (!attr) (void)hipGetLastError();   // (the launch reports what matters)
    hipLaunchKernelGGL((mlp_kernel<H, L, BWD>), dim3(grid), dim3(256), bytes, st, P);
    return hipGetLastError() == hipSuccess;
}
template <bool BWD>
bool launch(const MlpParams& P, int H, int L, hipStream_t st)
{
    // backward: one workgroup per CU walks its tiles and flushes its parameter gradients once; forward: two fit a CU
    const int tiles = (P.n + MLP_TILE - 1) / MLP_TILE, cap = num_cus() * (BWD ? 1 : 2), grid = tiles < cap ? tiles : cap;
    if (H == 128) return L == 1 ? launch_one<128, 1, BWD>(P, grid, st) : L == 2 ? launch_one<128, 2, BWD>(P, grid, st) : launch_one<128, 3, BWD>(P, grid, st);
    return L == 1 ? launch_one<64, 1, BWD>(P, grid, st) : L == 2 ? launch_one<64, 2, BWD>(P, grid, st) : launch_one<64, 3, BWD>(P, grid, st);
}

}  // namespace

extern "C" int32_t hgs_mlp_tile(void) { return MLP_TILE; }

extern "C" int32_t hgs_mlp_forward(int32_t n, const hgs_mlp_desc* net, const float* x, float* const head_out[HGS_MLP_MAX_HEADS], void* stream)
{
    static thread_local char msg[160];
    if (const char* why = check_net(n, net)) {
        snprintf(msg, sizeof msg, "mlp_forward: %s", why);
        return fail_mlp(msg);
    }
    if (n == 0) return HGS_OK;
    if (const char* why = check_weights(net)) {
        snprintf(msg, sizeof msg, "mlp_forward: %s", why);
        return fail_mlp(msg);
    }
    if (!x || !head_out) return fail_mlp("mlp_forward: null pointer");
    if (!aligned16(x)) return fail_mlp("mlp_forward: x must be 16-byte aligned");
    for (int k = 0; k < net->n_heads; ++k) {
        if (!head_out[k]) return fail_mlp("mlp_forward: null head output");
        if (!aligned16(head_out[k])) return fail_mlp("mlp_forward: every head output must be 16-byte aligned");
    }
    MlpParams P;
    fill(P, n, net, x);
    for (int k = 0; k < net->n_heads; ++k) P.out[k] = head_out[k];
    if (!launch<false>(P, net->trunk_width[0], net->n_trunk, (hipStream_t)stream)) {
        hgs::set_last_error("mlp_forward: kernel launch failed");
        return HGS_ERR_HIP;
    }
    return HGS_OK;
}

extern "C" int32_t hgs_mlp_backward(int32_t n, const hgs_mlp_desc* net, const float* x, const float* const dL_dhead[HGS_MLP_MAX_HEADS],
                                    float* dL_dx, const hgs_mlp_grads* grads, void* stream)
{
    static thread_local char msg[160];
    if (const char* why = check_net(n, net)) {
        snprintf(msg, sizeof msg, "mlp_backward: %s", why);
        return fail_mlp(msg);
    }
    if (n == 0) return HGS_OK;
    if (const char* why = check_weights(net)) {
        snprintf(msg, sizeof msg, "mlp_backward: %s", why);
        return fail_mlp(msg);
    }
    if (!x || !dL_dhead) return fail_mlp("mlp_backward: null pointer");
    if (!aligned16(x)) return fail_mlp("mlp_backward: x must be 16-byte aligned");
    if (!aligned16(dL_dx)) return fail_mlp("mlp_backward: dL_dx must be 16-byte aligned");
    MlpParams P;
    fill(P, n, net, x);
    bool any_up = false, any_out = dL_dx != nullptr;
    for (int k = 0; k < net->n_heads; ++k) {
        if (!aligned16(dL_dhead[k])) return fail_mlp("mlp_backward: every head gradient must be 16-byte aligned");
        P.gy[k] = dL_dhead[k];
        any_up = any_up || dL_dhead[k];
    }
    P.dx = dL_dx;
    if (grads) {
        for (int l = 0; l < net->n_trunk; ++l) {
            P.dW[l] = grads->trunk_weight[l], P.db[l] = grads->trunk_bias[l];
            any_out = any_out || P.dW[l] || P.db[l];
        }
        for (int k = 0; k < net->n_heads; ++k) {
            P.dWh[k] = grads->head_weight[k], P.dbh[k] = grads->head_bias[k];
            P.any_dwh = P.any_dwh || P.dWh[k] || P.dbh[k];
        }
        any_out = any_out || P.any_dwh;
    }
    if (!any_out) return HGS_OK;   // nothing asked for
    if (!any_up) {                 // no head is used: every gradient is zero; the parameter gradients already are
        if (dL_dx && hipMemsetAsync(dL_dx, 0, sizeof(float) * (size_t)n * net->in_width, (hipStream_t)stream) != hipSuccess) {
            hgs::set_last_error("mlp_backward: memset failed");
            return HGS_ERR_HIP;
        }
        return HGS_OK;
    }
    if (!launch<true>(P, net->trunk_width[0], net->n_trunk, (hipStream_t)stream)) {
        hgs::set_last_error("mlp_backward: kernel launch failed");
        return HGS_ERR_HIP;
    }
    return HGS_OK;
}
