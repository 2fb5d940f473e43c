// Palette lookup: the map from the indexed model's (N,H,W,256) probabilities and a palette to an RGBA image, and its
// VJP.  With t_k = palette_k / 127.5f - 1.0f per channel (the two f32 operations of p2p_palette_snap's image_out; with `blacken` a
// slot of alpha 0 is (-1,-1,-1,-1)):
//   soft forward   out_p = sum_k probs_pk t_k          (linear: nothing assumes that a row sums to 1)
//   hard forward   out_p = t_argmax_k probs_pk         (ties: the lowest k, the rule of p2p_argmax_lastdim)
//   backward       dprobs_pk = ((g_p0 t_k0 + g_p1 t_k1) + g_p2 t_k2) + g_p3 t_k3, every operation rounded to f32 on its own
// Streaming kernels: a pixel is 256 consecutive floats, one float4 per lane of a wave, so one wave owns one pixel per load and lane
// l owns slots 4l .. 4l+3 of every pixel it meets.  A workgroup stays inside one image (grid chunks x N), so a lane converts its
// four palette rows once and keeps the sixteen t values in registers.  No LDS, no workspace, no atomics: the soft forward reduces a
// pixel with four FMAs per channel and lane (ascending slot) and the xor butterfly of wave_sum (offsets 32, 16, .., 1), the same
// lanes in the same order for every pixel, so a pixel's bits depend on nothing but its 256 probabilities and its image's palette.
// The number of pixels a workgroup walks is a launch parameter (small batches get more, shorter workgroups); it moves no bit.
#include "p2p_common.hpp"

#define PLK_K 256
#define PLK_THREADS 256
#define PLK_PIX 4                           // pixels a wave has in flight: their loads are issued before the first reduction
#define PLK_ITERS 8                         // groups of PLK_PIX consecutive pixels per wave: 128 pixels per workgroup ...
#define PLK_ITERS_SMALL 2                   // ... or 32 while that leaves fewer than PLK_WANT_WGS workgroups
#define PLK_WANT_WGS 2048

__device__ __forceinline__ float4 plk_colour(const int4& q, int blacken) {
    const bool clear = blacken && q.w == 0;          // dataset_utils.blacken_transparent_pixels, applied to the palette
    const float r = clear ? 0.f : (float)q.x, g = clear ? 0.f : (float)q.y, b = clear ? 0.f : (float)q.z;
    return make_float4(__fsub_rn(__fdiv_rn(r, 127.5f), 1.0f), __fsub_rn(__fdiv_rn(g, 127.5f), 1.0f),
                       __fsub_rn(__fdiv_rn(b, 127.5f), 1.0f), __fsub_rn(__fdiv_rn((float)q.w, 127.5f), 1.0f));
}

// the lane's four slots of image b
__device__ __forceinline__ void plk_load(const int* __restrict__ palette, int b, int lane, int blacken, float4 (&t)[4]) {
    const int4* row = (const int4*)(palette + ((long long)b * PLK_K + 4 * lane) * 4);
#pragma unroll
    for (int s = 0; s < 4; ++s) t[s] = plk_colour(row[s], blacken);
}

// One channel of the pixel's sum per lane: lane l returns channel l >> 4.  The tree is wave_sum's (pairs at xor offsets 32, 16, 8, 4,
// 2, 1, addition being commutative), but a lane stops carrying the channels it will not return: at offset 32 lanes 0..31 keep x and
// y and hand z and w over, at offset 16 one of the two remaining goes -- 7 shuffles per pixel instead of 24, the same bits.
__device__ __forceinline__ float plk_dot(const float4& v, const float4 (&t)[4], int lane) {
    float4 a;
    a.x = __fmaf_rn(v.w, t[3].x, __fmaf_rn(v.z, t[2].x, __fmaf_rn(v.y, t[1].x, __fmaf_rn(v.x, t[0].x, 0.f))));
    a.y = __fmaf_rn(v.w, t[3].y, __fmaf_rn(v.z, t[2].y, __fmaf_rn(v.y, t[1].y, __fmaf_rn(v.x, t[0].y, 0.f))));
    a.z = __fmaf_rn(v.w, t[3].z, __fmaf_rn(v.z, t[2].z, __fmaf_rn(v.y, t[1].z, __fmaf_rn(v.x, t[0].z, 0.f))));
    a.w = __fmaf_rn(v.w, t[3].w, __fmaf_rn(v.z, t[2].w, __fmaf_rn(v.y, t[1].w, __fmaf_rn(v.x, t[0].w, 0.f))));
    const bool hi5 = (lane & 32) != 0, hi4 = (lane & 16) != 0;
    const float r0 = __shfl_xor(hi5 ? a.x : a.z, 32, 64), r1 = __shfl_xor(hi5 ? a.y : a.w, 32, 64);
    const float u0 = (hi5 ? a.z : a.x) + r0, u1 = (hi5 ? a.w : a.y) + r1;          // lanes 0..31: x, y;  lanes 32..63: z, w
    float s = (hi4 ? u1 : u0) + __shfl_xor(hi4 ? u0 : u1, 16, 64);                 // lanes 0..15 x, 16..31 y, 32..47 z, 48..63 w
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}

// the pixel's argmax in every lane: strict '>' inside the lane, then the butterfly on (value, index) with the lowest index on ties
__device__ __forceinline__ int plk_argmax(const float4& v, int lane) {
    float best = v.x;
    int bi = 4 * lane;
    if (v.y > best) { best = v.y; bi = 4 * lane + 1; }
    if (v.z > best) { best = v.z; bi = 4 * lane + 2; }
    if (v.w > best) { best = v.w; bi = 4 * lane + 3; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
    }
    return bi;
}

template <bool HARD>
__global__ __launch_bounds__(PLK_THREADS) void palette_lookup_fwd_kernel(int HW, const float* __restrict__ probs, const int* __restrict__ palette,
                                                                         int blacken, int iters, float* __restrict__ out) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float4 t[4];
    plk_load(palette, b, lane, blacken, t);
    const long long base = (long long)b * HW;
    const int first = (blockIdx.x * (PLK_THREADS / 64) + wave) * PLK_PIX * iters;
    for (int i = 0; i < iters; ++i) {
        const int p0 = first + i * PLK_PIX;
        if (p0 >= HW) break;                         // wave-uniform
        float4 v[PLK_PIX];
#pragma unroll
        for (int j = 0; j < PLK_PIX; ++j) {
            const int p = p0 + j < HW ? p0 + j : HW - 1;          // past the image: its last pixel once more, result dropped
            v[j] = *(const float4*)(probs + (base + p) * PLK_K + 4 * lane);
        }
        if (HARD) {
#pragma unroll
            for (int j = 0; j < PLK_PIX; ++j) {
                const int bi = p0 + j < HW ? plk_argmax(v[j], lane) : -1;
#pragma unroll
                for (int s = 0; s < 4; ++s)          // the slot's owner has its colour in a register (static index: no scratch)
                    if (bi == 4 * lane + s) *(float4*)(out + (base + p0 + j) * 4) = t[s];
            }
        } else {
            float o = 0.f;
#pragma unroll
            for (int j = 0; j < PLK_PIX; ++j) {
                const float r = plk_dot(v[j], t, lane);
                if ((lane & 15) == j) o = r;
            }
            // lane 16 c + j holds channel c of pixel p0 + j: sixteen lanes store the group's 64 consecutive bytes
            if ((lane & 15) < PLK_PIX && p0 + (lane & 15) < HW) out[(base + p0 + (lane & 15)) * 4 + (lane >> 4)] = o;
        }
    }
}

// four products and three sums, each rounded to f32: the pragma keeps the compiler from contracting a product into the sum that
// follows it.  (hipcc contracts by default, and __fmul_rn / __fadd_rn are no protection: they are inline functions of a plain * and
// a plain +, compiled under that default, and fuse once inlined; the operators have to stand in the pragma's own scope.)
__device__ __forceinline__ float plk_vjp(const float4& g, const float4& t) {
#pragma clang fp contract(off)
    const float a = g.x * t.x, b = g.y * t.y, c = g.z * t.z, d = g.w * t.w;
    return ((a + b) + c) + d;
}

// a pure write stream: g_p is one wave-uniform 16-byte read, every lane stores the float4 of its four slots
__global__ __launch_bounds__(PLK_THREADS) void palette_lookup_bwd_kernel(int HW, const float* __restrict__ g, const int* __restrict__ palette,
                                                                         int blacken, int iters, float* __restrict__ dprobs) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float4 t[4];
    plk_load(palette, b, lane, blacken, t);
    const long long base = (long long)b * HW;
    const int first = (blockIdx.x * (PLK_THREADS / 64) + wave) * PLK_PIX * iters;
    for (int i = 0; i < iters; ++i) {
        const int p0 = first + i * PLK_PIX;
        if (p0 >= HW) break;                         // wave-uniform
        float4 u[PLK_PIX];
#pragma unroll
        for (int j = 0; j < PLK_PIX; ++j) {
            const int p = p0 + j < HW ? p0 + j : HW - 1;
            u[j] = *(const float4*)(g + (base + p) * 4);
        }
#pragma unroll
        for (int j = 0; j < PLK_PIX; ++j) {
            if (p0 + j >= HW) break;                 // wave-uniform
            *(float4*)(dprobs + (base + p0 + j) * PLK_K + 4 * lane) =
                make_float4(plk_vjp(u[j], t[0]), plk_vjp(u[j], t[1]), plk_vjp(u[j], t[2]), plk_vjp(u[j], t[3]));
        }
    }
}

static int plk_check(const char* who, int N, int H, int W, int K, const void* in, const void* palette, int blacken, const void* outp) {
    P2P_REQUIRE(K == PLK_K, "%s: K = %d, only the 256-slot palette is supported", who, K);
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && (long long)H * W <= (1LL << 30) && N <= 65535, "%s: bad shape %d x %d x %d (H * W <= 2^30, N <= 65535)",
                who, N, H, W);
    P2P_REQUIRE(blacken == 0 || blacken == 1, "%s: blacken = %d, expected 0 or 1", who, blacken);
    P2P_REQUIRE(in && palette && outp, "%s: null pointer", who);
    P2P_REQUIRE(((uintptr_t)in % 16) == 0 && ((uintptr_t)palette % 16) == 0 && ((uintptr_t)outp % 16) == 0, "%s: every pointer must be 16-byte aligned",
                who);
    return 0;
}

// pixels per wave and the grid: (iters, chunks x N).  H * W <= 2^30: the chunk count and every pixel index fit an int.
static inline int plk_iters(int N, int H, int W) {
    const long long chunks = ((long long)H * W + (PLK_THREADS / 64) * PLK_PIX * PLK_ITERS - 1) / ((PLK_THREADS / 64) * PLK_PIX * PLK_ITERS);
    return chunks * N >= PLK_WANT_WGS ? PLK_ITERS : PLK_ITERS_SMALL;
}

static inline dim3 plk_grid(int N, int H, int W, int iters) {
    const long long chunk = (long long)(PLK_THREADS / 64) * PLK_PIX * iters;
    return dim3((unsigned)(((long long)H * W + chunk - 1) / chunk), (unsigned)N);
}

extern "C" int p2p_palette_lookup_fwd(int N, int H, int W, int K, const float* probs, const int* palette, int hard, int blacken, float* out,
                                      void* stream) {
    if (plk_check("p2p_palette_lookup_fwd", N, H, W, K, probs, palette, blacken, out)) return -1;
    P2P_REQUIRE(hard == 0 || hard == 1, "p2p_palette_lookup_fwd: hard = %d, expected 0 (expected colour) or 1 (argmax)", hard);
    const int iters = plk_iters(N, H, W);
    const dim3 grid = plk_grid(N, H, W, iters);
    if (hard) palette_lookup_fwd_kernel<true><<<grid, PLK_THREADS, 0, (hipStream_t)stream>>>(H * W, probs, palette, blacken, iters, out);
    else palette_lookup_fwd_kernel<false><<<grid, PLK_THREADS, 0, (hipStream_t)stream>>>(H * W, probs, palette, blacken, iters, out);
    return p2p_check_launch("p2p_palette_lookup_fwd");
}

extern "C" int p2p_palette_lookup_bwd(int N, int H, int W, int K, const float* g, const int* palette, int blacken, float* dprobs, void* stream) {
    if (plk_check("p2p_palette_lookup_bwd", N, H, W, K, g, palette, blacken, dprobs)) return -1;
    const int iters = plk_iters(N, H, W);
    palette_lookup_bwd_kernel<<<plk_grid(N, H, W, iters), PLK_THREADS, 0, (hipStream_t)stream>>>(H * W, g, palette, blacken, iters, dprobs);
    return p2p_check_launch("p2p_palette_lookup_bwd");
}
