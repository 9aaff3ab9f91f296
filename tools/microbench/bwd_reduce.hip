// The backward's per-(tile, entry) cross-lane reduction of nine per-lane sums (blend.hip), in isolation: SIMD time per
// reduction on gfx950 at 1..8 waves per SIMD on every CU.  Each wave makes nine sums per "entry" with FMA filler, two entries
// per iteration (a pair, as the walk does), and reduces them in one of these forms:
//   (a) the permlane / DPP transpose-reduce the backward used through round 6 (v_permlane32_swap / v_permlane16_swap, a select
//       step, DPP adds; blue by its own DPP chain with two row_bcast adds);
//   (b) the wave-private LDS transpose: v0..v7 stored at [v][lane] (ds_write2st64_b32), read back transposed by two
//       ds_read_b128 per lane, 7 adds + 3 in-half-row DPP adds; blue by the same DPP chain as (a).  Both entries are stored,
//       then each is read and finished behind its own lgkmcnt(0) (the shipped order);
//   (c) as (b), both entries' reads issued before ONE wait (16 read registers live at once).
// The filler-only loop is subtracted; the result is ns of SIMD time per reduction.  Atomics are left out (identical in all
// forms: one instruction, nine lanes).
#include <hip/hip_runtime.h>
#include <cstdio>

typedef uint32_t pair_t __attribute__((ext_vector_type(2)));
template <int CTRL> __device__ __forceinline__ float dpp_mov(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
template <int W> __device__ __forceinline__ float swap_add(float a, float b)
{
    pair_t r = W == 32 ? __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), false, false)
                       : __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, a), __builtin_bit_cast(uint32_t, b), false, false);
    const uint32_t r0 = r.x, r1 = r.y;
    return __builtin_bit_cast(float, r0) + __builtin_bit_cast(float, r1);
}
template <int CTRL> __device__ __forceinline__ float pair_step(float a, float b, bool hi)
{
    const float keep = hi ? b : a, send = hi ? a : b;
    return keep + dpp_mov<CTRL>(send);
}
__device__ __forceinline__ float blue_chain(float v8)
{
    float vb = v8 + dpp_mov<0xB1>(v8);
    vb += dpp_mov<0x4E>(vb);
    vb += dpp_mov<0x141>(vb);
    vb += dpp_mov<0x140>(vb);
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:15 row_mask:0xa bank_mask:0xf" : "+v"(vb));
    asm volatile("s_nop 1\n\tv_add_f32_dpp %0, %0, %0 row_bcast:31 row_mask:0xc bank_mask:0xf" : "+v"(vb));
    return vb;
}
__device__ __forceinline__ float reduce_a(const float (&v)[9], bool b3, bool sel, bool l63)
{
    const float s0 = swap_add<32>(v[0], v[1]), s1 = swap_add<32>(v[2], v[3]);
    const float s2 = swap_add<32>(v[4], v[5]), s3 = swap_add<32>(v[6], v[7]);
    const float t0 = swap_add<16>(s0, s1), t1 = swap_add<16>(s2, s3);
    float y = pair_step<0x128>(t0, t1, b3);
    y += dpp_mov<0x141>(y);
    y += dpp_mov<0x4E>(y);
    y += dpp_mov<0xB1>(y);
    const float vb = blue_chain(v[8]);
    return sel ? (l63 ? vb : y) : 0.0f;
}
__device__ __forceinline__ void lds_store(float* buf, int lane, const float (&v)[9])
{
#pragma unroll
    for (int k = 0; k < 8; ++k) buf[k * 64 + lane] = v[k];
}
__device__ __forceinline__ void lds_read(const float* buf, int rd, float4& ra, float4& rb)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    ra = *(const float4*)(buf + rd);
    rb = *(const float4*)(buf + (rd ^ 4));
}
__device__ __forceinline__ float lds_finish(const float4& ra, const float4& rb, float vb, bool sel, bool l63)
{
    float y = ((ra.x + ra.y) + (ra.z + ra.w)) + ((rb.x + rb.y) + (rb.z + rb.w));
    y += dpp_mov<0xB1>(y);
    y += dpp_mov<0x4E>(y);
    y += dpp_mov<0x141>(y);
    return sel ? (l63 ? vb : y) : 0.0f;
}

constexpr int FILL = 16;  // FMAs of filler per entry on top of the nine sums
template <int MODE> __global__ void __launch_bounds__(256) k(float* out, float a, float b, int iters)
{
    __shared__ float red[4][2 * 8 * 64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    float* const buf = red[w];
    const int grp = lane >> 3, rd = grp * 64 + (lane & 7) * 8 + (grp & 1) * 4;
    const bool sel_a = lane == 63 || (lane & 7) == 0, sel_b = sel_a, b3 = lane & 8, l63 = lane == 63;
    float x[FILL], v0[9], v1[9], acc = 0.f;
#pragma unroll
    for (int i = 0; i < FILL; ++i) x[i] = threadIdx.x * 1e-3f + i;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            float (&v)[9] = e ? v1 : v0;
#pragma unroll
            for (int i = 0; i < FILL; ++i) x[i] = __builtin_fmaf(x[i], a, b);
#pragma unroll
            for (int q = 0; q < 9; ++q) v[q] = __builtin_fmaf(x[q], a, x[q + 1]);
            if (MODE == 1) acc += reduce_a(v, b3, sel_a, l63);
            if (MODE >= 2) lds_store(buf + e * 512, lane, v);
        }
        if (MODE == 0) {
#pragma unroll
            for (int q = 0; q < 9; ++q) acc += v0[q] * v1[q];   // (keeps the sums alive)
        }
        if (MODE == 2) {
            const float vb0 = blue_chain(v0[8]), vb1 = blue_chain(v1[8]);
            float4 ra, rb;
            lds_read(buf, rd, ra, rb);
            acc += lds_finish(ra, rb, vb0, sel_b, l63);
            lds_read(buf + 512, rd, ra, rb);
            acc += lds_finish(ra, rb, vb1, sel_b, l63);
        }
        if (MODE == 3) {
            const float vb0 = blue_chain(v0[8]), vb1 = blue_chain(v1[8]);
            float4 ra0, rb0, ra1, rb1;
            lds_read(buf, rd, ra0, rb0);
            lds_read(buf + 512, rd, ra1, rb1);
            acc += lds_finish(ra0, rb0, vb0, sel_b, l63) + lds_finish(ra1, rb1, vb1, sel_b, l63);
        }
    }
    float s = acc;
#pragma unroll
    for (int i = 0; i < FILL; ++i) s += x[i];
    out[blockIdx.x * 256 + threadIdx.x] = s;
}

template <int MODE> double run(int wps, int iters)
{
    static float* d = nullptr;
    if (!d) (void)hipMalloc(&d, 256 * 8 * 256 * 4);
    hipEvent_t e0, e1;
    (void)hipEventCreate(&e0), (void)hipEventCreate(&e1);
    const int blocks = 256 * wps;   // a 256-thread workgroup puts one wave on each SIMD of its CU; 256 CUs
    k<MODE><<<blocks, 256>>>(d, 0.9999f, 1e-4f, 10);
    (void)hipEventRecord(e0);
    k<MODE><<<blocks, 256>>>(d, 0.9999f, 1e-4f, iters);
    (void)hipEventRecord(e1);
    (void)hipEventSynchronize(e1);
    float ms;
    (void)hipEventElapsedTime(&ms, e0, e1);
    return ms * 1e6 / ((double)wps * iters);   // ns of SIMD time per iteration (= per pair of entries)
}

int main()
{
    const int iters = 20000;
    printf("ns of SIMD time per reduction (two entries per iteration, filler-only loop subtracted)\n");
    for (int wps : {1, 2, 4, 8}) {
        const double base = run<0>(wps, iters);
        const double ta = run<1>(wps, iters), tb = run<2>(wps, iters), tc = run<3>(wps, iters);
        printf("%d w/SIMD: filler %6.2f ns/pair | (a) permlane/DPP %6.2f | (b) LDS, wait per entry %6.2f | (c) LDS, one wait per pair %6.2f"
               " | (b)/(a) %.3f (c)/(a) %.3f\n",
               wps, base, (ta - base) / 2, (tb - base) / 2, (tc - base) / 2, (tb - base) / (ta - base), (tc - base) / (ta - base));
    }
    return 0;
}
