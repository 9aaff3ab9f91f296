// the SMPL body model's forward, from (betas, pose, transl) to vertices and joint transforms, fused.
//   SMPL.forward, /root/reference/hugs/models/modules/smpl_layer.py:411-519 (called every human step, hugs_trimlp.py:458), into
//   lbs(), /root/reference/hugs/models/modules/lbs.py:76-187: shape blend (:129-130), joint regression (:134), 24 Rodrigues
//   rotations and the pose feature (:141-144), the pose-corrective product (:149-150, :162), the kinematic chain (:170, a Python
//   loop over the joints), the skinning (:174-185) and the translation of smpl_layer.py:498-504.
// The reference spends on the order of a hundred small torch kernels on this forward and more in autograd's backward; the arithmetic
// is tiny (one 17 MB stream of posedirs at V = 6 890) and the cost is launch count.  Here it is three kernels forward:
//   shape  (one thread per vertex)    shape_offsets, v_shaped, per-workgroup partial sums of J_regressor . v_shaped
//   chain  (one workgroup)            finishes J in a fixed order, Rodrigues, pose feature, the chain; R, J, G, A0 stay in the workspace
//   skin   (64 vertices / workgroup)  pose_offsets (four waves split the P rows, posedirs read once, coalesced), v_posed, T, verts
// and backward the mirror image: lbs.hip's skinning backward (dL/dA on the matrix cores, dL/dv_posed), a per-vertex kernel with the
// partial sums of dL/dpose_feature and of the translation's per-vertex terms, a one-workgroup kernel that reduces them and walks
// the chain in reverse through Rodrigues to dL/dpose, dL/dJ and dL/dtransl, a per-vertex kernel that adds J_regressor^T dL/dJ and
// forms the partial sums of dL/dbetas, and their ordered finish.  Every reduction is per-workgroup partials summed in a fixed
// order: no float atomics, two calls on the same inputs return the same bits.  fp32 throughout, one batch element per call.
#include <math.h>

#include "hgs_common.h"

namespace {

typedef const __attribute__((address_space(4))) float* const_f32p;

constexpr int SMPL_MAX_J = 32, SMPL_MAX_NB = 16;
constexpr int SHAPE_VERTS = 256;                  // vertices per workgroup of the two shape kernels (one per thread)
constexpr int SKIN_VERTS = 64;                    // vertices per workgroup of the two posedirs kernels (256 threads: 4 waves split the rows)
constexpr int SKIN_ELEMS = 3 * SKIN_VERTS;
constexpr int JP = 3 * SMPL_MAX_J;                // stride of one workgroup's partial joint sums

struct Parents {
    int32_t p[SMPL_MAX_J];
};

// What the forward leaves at the head of the workspace for its backward (offsets in floats).
constexpr int WS_R = 0;                           // [32][9]  joint rotations
constexpr int WS_J = WS_R + 9 * SMPL_MAX_J;       // [32][3]  rest joints
constexpr int WS_G = WS_J + 3 * SMPL_MAX_J;       // [32][12] world transforms of the chain, rows of [R | t]
constexpr int WS_A0 = WS_G + 12 * SMPL_MAX_J;     // [32][16] A before the translation
constexpr int WS_PF = WS_A0 + 16 * SMPL_MAX_J;    // [288]    pose feature
constexpr int WS_HEAD = WS_PF + 288;
static_assert(9 * (SMPL_MAX_J - 1) <= 288, "pose feature");

struct Layout {  // byte offsets of the scratch behind the head
    size_t jpart, dA0, dJ, dvp, dvskin, dW, skin_ws, dpf_part, tr_part, beta_part, total;
    int nb_shape, nb_skin;
    Layout(int V, int J, int NB)
    {
        const size_t v = V < 1 ? 1 : (size_t)V;
        nb_shape = (int)((v + SHAPE_VERTS - 1) / SHAPE_VERTS);
        nb_skin = (int)((v + SKIN_VERTS - 1) / SKIN_VERTS);
        const int P = 9 * (J - 1);
        size_t o = hgs::align_up(sizeof(float) * WS_HEAD);
        jpart = o;     o = hgs::align_up(o + sizeof(float) * JP * (size_t)nb_shape);
        dA0 = o;       o = hgs::align_up(o + sizeof(float) * 16 * SMPL_MAX_J);
        dJ = o;        o = hgs::align_up(o + sizeof(float) * 3 * SMPL_MAX_J);
        dvp = o;       o = hgs::align_up(o + sizeof(float) * 3 * v);
        dvskin = o;    o = hgs::align_up(o + sizeof(float) * 3 * v);
        dW = o;        o = hgs::align_up(o + sizeof(float) * (size_t)J * v);
        skin_ws = o;   o = hgs::align_up(o + hgs_lbs_skin_backward_workspace((int32_t)v, J));
        dpf_part = o;  o = hgs::align_up(o + sizeof(float) * (size_t)P * nb_skin);
        tr_part = o;   o = hgs::align_up(o + sizeof(float) * 3 * (size_t)nb_skin);
        beta_part = o; o = hgs::align_up(o + sizeof(float) * SMPL_MAX_NB * (size_t)nb_shape);
        total = o;
        (void)NB;
    }
};

__device__ inline float wave_sum(float x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);  // a butterfly: every lane ends with the same bits
    return x;
}

// R = I + sin a K + (1 - cos a) K^2 with a = |r + 1e-8|, K = hat(r / a): the published formula, epsilon inside the norm.
__device__ inline void rodrigues(const float r[3], float R[9])
{
    const float ex = r[0] + 1e-8f, ey = r[1] + 1e-8f, ez = r[2] + 1e-8f;
    const float a = sqrtf((ex * ex + ey * ey) + ez * ez);
    const float x = r[0] / a, y = r[1] / a, z = r[2] / a;
    const float s = sinf(a), c1 = 1.0f - cosf(a);
    const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float k2 = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
            R[3 * i + j] = ((i == j ? 1.0f : 0.0f) + s * K[3 * i + j]) + c1 * k2;
        }
}

// dL/dr of the formula above given dL/dR.  At r = 0: n = 0, K = 0 and dr = (sin a / a) * (the antisymmetric part of dR): finite.
__device__ inline void rodrigues_backward(const float r[3], const float dR[9], float dr[3])
{
    const float ex = r[0] + 1e-8f, ey = r[1] + 1e-8f, ez = r[2] + 1e-8f;
    const float a = sqrtf((ex * ex + ey * ey) + ez * ez);
    const float x = r[0] / a, y = r[1] / a, z = r[2] / a;
    const float s = sinf(a), c = cosf(a), c1 = 1.0f - c;
    const float K[9] = {0.f, -z, y, z, 0.f, -x, -y, x, 0.f};
    float K2[9], dK[9];
    float dRK = 0.f, dRK2 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            K2[3 * i + j] = (K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j]) + K[3 * i + 2] * K[6 + j];
            dRK += dR[3 * i + j] * K[3 * i + j];
            dRK2 += dR[3 * i + j] * K2[3 * i + j];
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            // d(K K)/dK:  dR K^T + K^T dR
            const float u = (dR[3 * i] * K[3 * j] + dR[3 * i + 1] * K[3 * j + 1]) + dR[3 * i + 2] * K[3 * j + 2];
            const float w = (K[i] * dR[j] + K[3 + i] * dR[3 + j]) + K[6 + i] * dR[6 + j];
            dK[3 * i + j] = s * dR[3 * i + j] + c1 * (u + w);
        }
    const float dn[3] = {dK[7] - dK[5], dK[2] - dK[6], dK[3] - dK[1]};
    float da = c * dRK + s * dRK2;                                  // through sin a and 1 - cos a
    da -= ((dn[0] * r[0] + dn[1] * r[1]) + dn[2] * r[2]) / (a * a);  // n = r / a
    dr[0] = dn[0] / a + da * (ex / a);                               // a = |r + eps|
    dr[1] = dn[1] / a + da * (ey / a);
    dr[2] = dn[2] / a + da * (ez / a);
}

// ---------------------------------------------------------------------------------------------------------------- forward

__global__ void __launch_bounds__(SHAPE_VERTS)
smpl_shape_kernel(int V, int J, int NB, const float* __restrict__ betas, const float* __restrict__ v_template,
                  const float* __restrict__ shapedirs, const float* __restrict__ J_regressor, float* __restrict__ v_shaped,
                  float* __restrict__ shape_offsets, float* __restrict__ jpart /*[gridDim.x][JP]*/)
{
    __shared__ float red[4][JP];
    const int v = blockIdx.x * SHAPE_VERTS + threadIdx.x;
    const bool ok = v < V;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const_f32p b = (const_f32p)betas;
    float vs[3] = {0.f, 0.f, 0.f};
    if (ok) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float* s = shapedirs + (3 * (size_t)v + k) * NB;
            float acc = 0.0f;
            for (int l = 0; l < NB; ++l) acc = __builtin_fmaf(s[l], b[l], acc);
            shape_offsets[3 * (size_t)v + k] = acc;
            vs[k] = v_template[3 * (size_t)v + k] + acc;
            v_shaped[3 * (size_t)v + k] = vs[k];
        }
    }
    for (int j = 0; j < J; ++j) {
        const float wj = ok ? J_regressor[(size_t)j * V + v] : 0.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float s = wave_sum(wj * vs[k]);
            if (lane == 0) red[w][3 * j + k] = s;
        }
    }
    __syncthreads();
    const int e = threadIdx.x;
    if (e < 3 * J) jpart[(size_t)blockIdx.x * JP + e] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
}

__global__ void __launch_bounds__(64)
smpl_chain_kernel(int J, int nblocks, Parents par, const float* __restrict__ pose, const float* __restrict__ transl,
                  const float* __restrict__ jpart, float* __restrict__ ws, float* __restrict__ A_out, float* __restrict__ Jtr_out)
{
    __shared__ float Rs[SMPL_MAX_J][9], Js[SMPL_MAX_J][3], Gs[SMPL_MAX_J][12];
    __shared__ int ps[SMPL_MAX_J];
    const int t = threadIdx.x;
    for (int e = t; e < 3 * J; e += 64) {
        float acc = 0.0f;
        for (int b = 0; b < nblocks; ++b) acc += jpart[(size_t)b * JP + e];
        Js[e / 3][e % 3] = acc;
        ws[WS_J + e] = acc;
    }
    if (t < J) {
        ps[t] = par.p[t];
        const float r[3] = {pose[3 * t], pose[3 * t + 1], pose[3 * t + 2]};
        float R[9];
        rodrigues(r, R);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            Rs[t][i] = R[i];
            ws[WS_R + 9 * t + i] = R[i];
            if (t >= 1) ws[WS_PF + 9 * (t - 1) + i] = R[i] - (i % 4 == 0 ? 1.0f : 0.0f);  // (R - I), row-major per joint
        }
    }
    __syncthreads();
    if (t == 0) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) Gs[0][4 * r + c] = Rs[0][3 * r + c];
            Gs[0][4 * r + 3] = Js[0][r];
        }
        for (int j = 1; j < J; ++j) {
            const int p = ps[j];
            float Gp[12], Rj[9], d[3];
#pragma unroll
            for (int i = 0; i < 12; ++i) Gp[i] = Gs[p][i];
#pragma unroll
            for (int i = 0; i < 9; ++i) Rj[i] = Rs[j][i];
#pragma unroll
            for (int i = 0; i < 3; ++i) d[i] = Js[j][i] - Js[p][i];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    Gs[j][4 * r + c] = (Gp[4 * r] * Rj[c] + Gp[4 * r + 1] * Rj[3 + c]) + Gp[4 * r + 2] * Rj[6 + c];
                Gs[j][4 * r + 3] = ((Gp[4 * r] * d[0] + Gp[4 * r + 1] * d[1]) + Gp[4 * r + 2] * d[2]) + Gp[4 * r + 3];
            }
        }
    }
    __syncthreads();
    if (t < J) {
        const float tr[3] = {transl ? transl[0] : 0.0f, transl ? transl[1] : 0.0f, transl ? transl[2] : 0.0f};
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const float* g = &Gs[t][4 * r];
            const float a3 = g[3] - ((g[0] * Js[t][0] + g[1] * Js[t][1]) + g[2] * Js[t][2]);  // the rest joint removed
#pragma unroll
            for (int c = 0; c < 4; ++c) ws[WS_G + 12 * t + 4 * r + c] = g[c];
#pragma unroll
            for (int c = 0; c < 3; ++c) ws[WS_A0 + 16 * t + 4 * r + c] = g[c], A_out[16 * t + 4 * r + c] = g[c];
            ws[WS_A0 + 16 * t + 4 * r + 3] = a3;
            A_out[16 * t + 4 * r + 3] = a3 + tr[r];
            Jtr_out[3 * t + r] = g[3] + tr[r];
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) ws[WS_A0 + 16 * t + 12 + c] = A_out[16 * t + 12 + c] = c == 3 ? 1.0f : 0.0f;
    }
}

__global__ void __launch_bounds__(256)
smpl_skin_kernel(int V, int J, int P /* 0: posedirs disabled, not read */, const float* __restrict__ ws,
                 const float* __restrict__ transl, const float* __restrict__ posedirs, const float* __restrict__ v_shaped,
                 const float* __restrict__ W, float* __restrict__ pose_offsets, float* __restrict__ v_posed,
                 float* __restrict__ T_out, float* __restrict__ verts)
{
    __shared__ float part[4][SKIN_ELEMS];
    __shared__ float vp[SKIN_ELEMS];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t E = 3 * (size_t)V, e0 = (size_t)blockIdx.x * SKIN_ELEMS;
    if (P > 0) {
        const_f32p pf = (const_f32p)(ws + WS_PF);
        float acc[3] = {0.f, 0.f, 0.f};
        const bool in0 = e0 + lane < E, in1 = e0 + 64 + lane < E, in2 = e0 + 128 + lane < E;
        for (int p = w; p < P; p += 4) {
            const float f = pf[p];
            const float* row = posedirs + (size_t)p * E + e0;
            if (in0) acc[0] = __builtin_fmaf(f, row[lane], acc[0]);
            if (in1) acc[1] = __builtin_fmaf(f, row[64 + lane], acc[1]);
            if (in2) acc[2] = __builtin_fmaf(f, row[128 + lane], acc[2]);
        }
#pragma unroll
        for (int t = 0; t < 3; ++t) part[w][64 * t + lane] = acc[t];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < SKIN_ELEMS && e0 + t < E) {
        const float po = P > 0 ? ((part[0][t] + part[1][t]) + part[2][t]) + part[3][t] : 0.0f;
        const float x = v_shaped[e0 + t] + po;
        pose_offsets[e0 + t] = po;
        v_posed[e0 + t] = x;
        vp[t] = x;
    }
    __syncthreads();
    const size_t v = (size_t)blockIdx.x * SKIN_VERTS + t;
    if (t >= SKIN_VERTS || v >= (size_t)V) return;
    const_f32p As = (const_f32p)(ws + WS_A0);
    float T[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) T[k] = 0.0f;
    const float* wv = W + v * J;
    for (int j = 0; j < J; ++j) {
        const float wj = wv[j];
#pragma unroll
        for (int k = 0; k < 16; ++k) T[k] = __builtin_fmaf(wj, As[16 * j + k], T[k]);
    }
    const float x = vp[3 * t], y = vp[3 * t + 1], z = vp[3 * t + 2];
    const float tr[3] = {transl ? transl[0] : 0.0f, transl ? transl[1] : 0.0f, transl ? transl[2] : 0.0f};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        verts[3 * v + r] = (((T[4 * r] * x + T[4 * r + 1] * y) + T[4 * r + 2] * z) + T[4 * r + 3]) + tr[r];
        T[4 * r + 3] += tr[r];
    }
    float4* To = reinterpret_cast<float4*>(T_out + 16 * v);
#pragma unroll
    for (int r = 0; r < 4; ++r) To[r] = make_float4(T[4 * r], T[4 * r + 1], T[4 * r + 2], T[4 * r + 3]);
}

// --------------------------------------------------------------------------------------------------------------- backward

// Per vertex element e = 3 v + k: dL/dv_posed (skinning's part + the output's own cotangent), this workgroup's partial sums of
// dL/dpose_feature[p] = sum_e posedirs[p, e] (dL/dv_posed + dL/dpose_offsets)[e], and of the translation's per-vertex terms.
__global__ void __launch_bounds__(256)
smpl_bwd_vertex_kernel(int V, int P /* 0: posedirs disabled */, const float* __restrict__ posedirs,
                       const float* __restrict__ dv_skin, const float* __restrict__ g_vposed, const float* __restrict__ g_po,
                       const float* __restrict__ g_verts, const float* __restrict__ g_T, float* __restrict__ dvp_out,
                       float* __restrict__ dpf_part /*[gridDim.x][P]*/, float* __restrict__ tr_part /*[gridDim.x][3]*/)
{
    __shared__ float dsh[SKIN_ELEMS], csh[SKIN_ELEMS];
    const int t = threadIdx.x;
    const size_t E = 3 * (size_t)V, e0 = (size_t)blockIdx.x * SKIN_ELEMS;
    if (t < SKIN_ELEMS) {
        float d = 0.0f, c = 0.0f;
        const size_t e = e0 + t;
        if (e < E) {
            const float dvp = (dv_skin ? dv_skin[e] : 0.0f) + (g_vposed ? g_vposed[e] : 0.0f);
            dvp_out[e] = dvp;
            d = dvp + (g_po ? g_po[e] : 0.0f);
            if (g_verts) c = g_verts[e];
            if (g_T) c += g_T[16 * (e / 3) + 4 * (e % 3) + 3];
        }
        dsh[t] = d;
        csh[t] = c;
    }
    __syncthreads();
    const int lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    if (w < 3) {  // SKIN_ELEMS is a multiple of 3: element 3 i + w of the workgroup is component w of its vertex i
        const float s = wave_sum(csh[3 * lane + w]);
        if (lane == 0) tr_part[(size_t)blockIdx.x * 3 + w] = s;
    }
    if (P > 0) {
        const float d0 = dsh[lane], d1 = dsh[64 + lane], d2 = dsh[128 + lane];
        const bool in0 = e0 + lane < E, in1 = e0 + 64 + lane < E, in2 = e0 + 128 + lane < E;
        for (int p = w; p < P; p += 4) {
            const float* row = posedirs + (size_t)p * E + e0;
            float s = 0.0f;
            if (in0) s = __builtin_fmaf(d0, row[lane], s);
            if (in1) s = __builtin_fmaf(d1, row[64 + lane], s);
            if (in2) s = __builtin_fmaf(d2, row[128 + lane], s);
            s = wave_sum(s);
            if (lane == 0) dpf_part[(size_t)blockIdx.x * P + p] = s;
        }
    }
}

// One workgroup: the ordered finish of the partial sums, the chain in reverse, Rodrigues' backward.
__global__ void __launch_bounds__(256)
smpl_bwd_chain_kernel(int J, int P /* rows of dpf_part; 0: none */, int nb_skin /* workgroups of the vertex kernel; 0: it did not run */,
                      Parents par, const float* __restrict__ pose, const float* __restrict__ ws, const float* __restrict__ dA0,
                      const float* __restrict__ g_A, const float* __restrict__ g_Jtr, const float* __restrict__ dpf_part,
                      const float* __restrict__ tr_part, float* __restrict__ dJ_out, float* __restrict__ dpose,
                      float* __restrict__ dtransl)
{
    __shared__ float Rs[SMPL_MAX_J][9], Js[SMPL_MAX_J][3], Gs[SMPL_MAX_J][12];
    __shared__ float dRg[SMPL_MAX_J][9], dRl[SMPL_MAX_J][9], dt[SMPL_MAX_J][3], dJ[SMPL_MAX_J][3];
    __shared__ float dpf[288];
    __shared__ int ps[SMPL_MAX_J];
    const int t = threadIdx.x;
    for (int p = t; p < 288; p += 256) {
        float acc = 0.0f;
        if (p < P)
            for (int b = 0; b < nb_skin; ++b) acc += dpf_part[(size_t)b * P + p];
        dpf[p] = acc;
    }
    for (int e = t; e < 9 * J; e += 256) Rs[e / 9][e % 9] = ws[WS_R + e];
    for (int e = t; e < 12 * J; e += 256) Gs[e / 12][e % 12] = ws[WS_G + e];
    for (int e = t; e < 3 * J; e += 256) Js[e / 3][e % 3] = ws[WS_J + e];
    __syncthreads();
    if (t < J) {
        ps[t] = par.p[t];
        float dAt[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            dAt[r] = (dA0 ? dA0[16 * t + 4 * r + 3] : 0.0f) + (g_A ? g_A[16 * t + 4 * r + 3] : 0.0f);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float dAr = (dA0 ? dA0[16 * t + 4 * r + c] : 0.0f) + (g_A ? g_A[16 * t + 4 * r + c] : 0.0f);
                dRg[t][3 * r + c] = dAr - dAt[r] * Js[t][c];  // A's translation is t - Rg J
            }
            dt[t][r] = dAt[r] + (g_Jtr ? g_Jtr[3 * t + r] : 0.0f);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) dJ[t][c] = -((Gs[t][c] * dAt[0] + Gs[t][4 + c] * dAt[1]) + Gs[t][8 + c] * dAt[2]);
    }
    __syncthreads();
    if (t == 0) {
        for (int j = J - 1; j >= 1; --j) {  // parents[j] < j: joint j's sums are final when it is reached
            const int p = ps[j];
            float Rp[9], g[9], Rj[9], tj[3], d[3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) Rp[3 * r + c] = Gs[p][4 * r + c];
#pragma unroll
            for (int i = 0; i < 9; ++i) g[i] = dRg[j][i], Rj[i] = Rs[j][i];
#pragma unroll
            for (int i = 0; i < 3; ++i) tj[i] = dt[j][i], d[i] = Js[j][i] - Js[p][i];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    dRl[j][3 * r + c] = (Rp[r] * g[c] + Rp[3 + r] * g[3 + c]) + Rp[6 + r] * g[6 + c];                          // Rg_p^T dRg_j
                    dRg[p][3 * r + c] += ((g[3 * r] * Rj[3 * c] + g[3 * r + 1] * Rj[3 * c + 1]) + g[3 * r + 2] * Rj[3 * c + 2])  // dRg_j R_j^T
                                         + tj[r] * d[c];
                }
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float u = (Rp[c] * tj[0] + Rp[3 + c] * tj[1]) + Rp[6 + c] * tj[2];  // Rg_p^T dt_j
                dJ[j][c] += u;
                dJ[p][c] -= u;
                dt[p][c] += tj[c];
            }
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) dRl[0][i] = dRg[0][i];
#pragma unroll
        for (int c = 0; c < 3; ++c) dJ[0][c] += dt[0][c];
    }
    __syncthreads();
    if (t < J) {
        float dR[9], dr[3];
#pragma unroll
        for (int i = 0; i < 9; ++i) dR[i] = dRl[t][i] + (t >= 1 ? dpf[9 * (t >= 1 ? t - 1 : 0) + i] : 0.0f);
        const float r[3] = {pose[3 * t], pose[3 * t + 1], pose[3 * t + 2]};
        rodrigues_backward(r, dR, dr);
#pragma unroll
        for (int c = 0; c < 3; ++c) dpose[3 * t + c] = dr[c], dJ_out[3 * t + c] = dJ[t][c];
    }
    const int lane = t & 63, w = __builtin_amdgcn_readfirstlane(t >> 6);
    if (w < 3 && dtransl) {  // wave w: component w
        float acc = lane < J ? (g_A ? g_A[16 * lane + 4 * w + 3] : 0.0f) + (g_Jtr ? g_Jtr[3 * lane + w] : 0.0f) : 0.0f;  // J <= 32 lanes: the joints' terms
        for (int b = lane; b < nb_skin; b += 64) acc += tr_part[(size_t)b * 3 + w];
        acc = wave_sum(acc);
        if (lane == 0) dtransl[w] = acc;
    }
}

// Per vertex: dL/dv_shaped = dL/dv_posed + its own cotangent + J_regressor^T dL/dJ; partial sums of dL/dbetas.
__global__ void __launch_bounds__(SHAPE_VERTS)
smpl_bwd_shape_kernel(int V, int J, int NB, const float* __restrict__ shapedirs, const float* __restrict__ J_regressor,
                      const float* __restrict__ dJ, const float* __restrict__ dvp, const float* __restrict__ g_vshaped,
                      const float* __restrict__ g_so, float* __restrict__ beta_part /*[gridDim.x][16]*/)
{
    __shared__ float red[4][SMPL_MAX_NB];
    const int v = blockIdx.x * SHAPE_VERTS + threadIdx.x;
    const bool ok = v < V;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const_f32p dJs = (const_f32p)dJ;
    float d[3] = {0.f, 0.f, 0.f};
    if (ok) {
        float a[3] = {0.f, 0.f, 0.f};
        for (int j = 0; j < J; ++j) {
            const float wj = J_regressor[(size_t)j * V + v];
#pragma unroll
            for (int k = 0; k < 3; ++k) a[k] = __builtin_fmaf(wj, dJs[3 * j + k], a[k]);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const size_t e = 3 * (size_t)v + k;
            d[k] = ((a[k] + (dvp ? dvp[e] : 0.0f)) + (g_vshaped ? g_vshaped[e] : 0.0f)) + (g_so ? g_so[e] : 0.0f);
        }
    }
    for (int l = 0; l < NB; ++l) {
        float s = 0.0f;
        if (ok) {
            const float* sd = shapedirs + 3 * (size_t)v * NB + l;
            s = (sd[0] * d[0] + sd[NB] * d[1]) + sd[2 * (size_t)NB] * d[2];
        }
        s = wave_sum(s);
        if (lane == 0) red[w][l] = s;
    }
    __syncthreads();
    const int l = threadIdx.x;
    if (l < NB) beta_part[(size_t)blockIdx.x * SMPL_MAX_NB + l] = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
}

__global__ void __launch_bounds__(64)
smpl_bwd_beta_kernel(int NB, int nblocks, const float* __restrict__ beta_part, float* __restrict__ dbetas)
{
    const int l = threadIdx.x;
    if (l >= NB) return;
    float acc = 0.0f;
    for (int b = 0; b < nblocks; ++b) acc += beta_part[(size_t)b * SMPL_MAX_NB + l];
    dbetas[l] = acc;
}

int fail_smpl(const char* what)
{
    hgs::set_last_error(what);
    return HGS_ERR_INVALID_ARGUMENT;
}

int check_launch(const char* what)
{
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return HGS_OK;
    char msg[256];
    snprintf(msg, sizeof msg, "%s: %s", what, hipGetErrorString(e));
    hgs::set_last_error(msg);
    return HGS_ERR_HIP;
}

// sizes and the kinematic tree; 0 = fine
int check_model(const char* who, int32_t V, int32_t J, int32_t NB, const int32_t* parents, Parents* out)
{
    char msg[256];
    if (V < 0 || J < 2 || J > SMPL_MAX_J || NB < 1 || NB > SMPL_MAX_NB) {
        snprintf(msg, sizeof msg, "%s: need V >= 0 vertices, 2 <= J <= 32 joints and 1 <= NB <= 16 shape coefficients (got V=%d J=%d NB=%d)",
                 who, V, J, NB);
        return fail_smpl(msg);
    }
    if (!parents) {
        snprintf(msg, sizeof msg, "%s: null pointer (parents)", who);
        return fail_smpl(msg);
    }
    for (int j = 0; j < SMPL_MAX_J; ++j) out->p[j] = 0;
    for (int j = 0; j < J; ++j) {
        const int32_t p = parents[j];
        if (j == 0 ? p != -1 : (p < 0 || p >= j)) {
            snprintf(msg, sizeof msg, "%s: bad parents array: need parents[0] = -1 and 0 <= parents[j] < j (parents[%d] = %d)", who, j, p);
            return fail_smpl(msg);
        }
        out->p[j] = p;
    }
    return HGS_OK;
}

}  // namespace

extern "C" size_t hgs_smpl_workspace(int32_t V, int32_t J, int32_t NB)
{
    if (V <= 0 || J < 2 || J > SMPL_MAX_J || NB < 1 || NB > SMPL_MAX_NB) return 0;
    return Layout(V, J, NB).total;
}

extern "C" int32_t hgs_smpl_forward(int32_t V, int32_t J, int32_t NB, const int32_t* parents, const float* betas, const float* pose,
                                    const float* transl, const float* v_template, const float* shapedirs, const float* posedirs,
                                    const float* J_regressor, const float* lbs_weights, int32_t disable_posedirs, float* verts,
                                    float* J_transformed, float* A, float* T, float* v_posed, float* v_shaped, float* shape_offsets,
                                    float* pose_offsets, void* workspace, void* stream)
{
    Parents par;
    if (const int rc = check_model("smpl_forward", V, J, NB, parents, &par)) return rc;
    if (V == 0) return HGS_OK;
    if (!betas || !pose || !v_template || !shapedirs || !J_regressor || !lbs_weights || !verts || !J_transformed || !A || !T || !v_posed ||
        !v_shaped || !shape_offsets || !pose_offsets || !workspace)
        return fail_smpl("smpl_forward: null pointer");
    if (!disable_posedirs && !posedirs) return fail_smpl("smpl_forward: null pointer (posedirs may be NULL only with disable_posedirs)");
    if ((((uintptr_t)T | (uintptr_t)workspace) & 15) != 0) return fail_smpl("smpl_forward: T and workspace must be 16-byte aligned");
    const Layout L(V, J, NB);
    hipStream_t st = (hipStream_t)stream;
    float* ws = (float*)workspace;
    float* jpart = (float*)((char*)workspace + L.jpart);
    hipLaunchKernelGGL(smpl_shape_kernel, dim3(L.nb_shape), dim3(SHAPE_VERTS), 0, st, V, J, NB, betas, v_template, shapedirs, J_regressor,
                       v_shaped, shape_offsets, jpart);
    hipLaunchKernelGGL(smpl_chain_kernel, dim3(1), dim3(64), 0, st, J, L.nb_shape, par, pose, transl, jpart, ws, A, J_transformed);
    hipLaunchKernelGGL(smpl_skin_kernel, dim3(L.nb_skin), dim3(256), 0, st, V, J, disable_posedirs ? 0 : 9 * (J - 1), ws, transl, posedirs,
                       v_shaped, lbs_weights, pose_offsets, v_posed, T, verts);
    return check_launch("smpl_forward");
}

extern "C" int32_t hgs_smpl_backward(int32_t V, int32_t J, int32_t NB, const int32_t* parents, const float* pose, const float* shapedirs,
                                     const float* posedirs, const float* J_regressor, const float* lbs_weights, int32_t disable_posedirs,
                                     const float* v_posed, const float* T, const float* dL_dverts, const float* dL_dJ_transformed,
                                     const float* dL_dA, const float* dL_dT, const float* dL_dv_posed, const float* dL_dv_shaped,
                                     const float* dL_dshape_offsets, const float* dL_dpose_offsets, float* dL_dbetas, float* dL_dpose,
                                     float* dL_dtransl, void* workspace, void* stream)
{
    Parents par;
    if (const int rc = check_model("smpl_backward", V, J, NB, parents, &par)) return rc;
    if (!dL_dbetas || !dL_dpose) return fail_smpl("smpl_backward: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (V == 0) {  // the forward was a no-op: nothing depends on the parameters
        if (hipMemsetAsync(dL_dbetas, 0, sizeof(float) * NB, st) != hipSuccess || hipMemsetAsync(dL_dpose, 0, sizeof(float) * 3 * J, st) != hipSuccess ||
            (dL_dtransl && hipMemsetAsync(dL_dtransl, 0, sizeof(float) * 3, st) != hipSuccess))
            return check_launch("smpl_backward");
        return HGS_OK;
    }
    if (!pose || !shapedirs || !J_regressor || !lbs_weights || !v_posed || !T || !workspace) return fail_smpl("smpl_backward: null pointer");
    if (!disable_posedirs && !posedirs) return fail_smpl("smpl_backward: null pointer (posedirs may be NULL only with disable_posedirs)");
    if ((((uintptr_t)T | (uintptr_t)workspace | (uintptr_t)dL_dT) & 15) != 0)
        return fail_smpl("smpl_backward: T, dL_dT and workspace must be 16-byte aligned");
    const Layout L(V, J, NB);
    char* base = (char*)workspace;
    float* ws = (float*)workspace;
    float* dA0 = (float*)(base + L.dA0);
    float* dJ = (float*)(base + L.dJ);
    float* dvp = (float*)(base + L.dvp);
    float* dvskin = (float*)(base + L.dvskin);
    float* dpf_part = (float*)(base + L.dpf_part);
    float* tr_part = (float*)(base + L.tr_part);
    float* beta_part = (float*)(base + L.beta_part);
    const bool has_skin = dL_dverts || dL_dT;
    const bool has_vertex = has_skin || dL_dv_posed || dL_dpose_offsets;
    const int P = disable_posedirs ? 0 : 9 * (J - 1);
    if (has_skin) {  // dL/dA0 (matrix cores, fixed-order reduction) and skinning's dL/dv_posed: lbs.hip
        const int rc = hgs_lbs_skin_backward(V, J, ws + WS_A0, lbs_weights, v_posed, nullptr, T, dL_dverts, dL_dT, nullptr, dA0,
                                             (float*)(base + L.dW), dvskin, nullptr, base + L.skin_ws, stream);
        if (rc < 0) return rc;
    }
    if (has_vertex)
        hipLaunchKernelGGL(smpl_bwd_vertex_kernel, dim3(L.nb_skin), dim3(256), 0, st, V, P, posedirs, has_skin ? dvskin : nullptr, dL_dv_posed,
                           dL_dpose_offsets, dL_dverts, dL_dT, dvp, dpf_part, tr_part);
    hipLaunchKernelGGL(smpl_bwd_chain_kernel, dim3(1), dim3(256), 0, st, J, has_vertex ? P : 0, has_vertex ? L.nb_skin : 0, par, pose, ws,
                       has_skin ? dA0 : nullptr, dL_dA, dL_dJ_transformed, dpf_part, tr_part, dJ, dL_dpose, dL_dtransl);
    hipLaunchKernelGGL(smpl_bwd_shape_kernel, dim3(L.nb_shape), dim3(SHAPE_VERTS), 0, st, V, J, NB, shapedirs, J_regressor, dJ,
                       has_vertex ? dvp : nullptr, dL_dv_shaped, dL_dshape_offsets, beta_part);
    hipLaunchKernelGGL(smpl_bwd_beta_kernel, dim3(1), dim3(64), 0, st, NB, L.nb_shape, beta_part, dL_dbetas);
    return check_launch("smpl_backward");
}
