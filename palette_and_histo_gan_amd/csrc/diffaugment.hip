// Differentiable augmentation of an RGBA batch in front of the discriminator, and its VJP (DESIGN.md "differentiable augmentation";
// Zhao et al., "Differentiable Augmentation for Data-Efficient GAN Training", NeurIPS 2020).  Per image, from one row of two small
// device tables -- color (b, s, k) and geometry (ty, tx, y0, x0) -- and in this order:
//   colour       channels 0..2 of every pixel: u = x + b;  v = (u - mean_c u) s + mean_c u;  y = (v - m) k + m with m the mean of v over
//                the image, which is mean_rgb(x) + b in real arithmetic: ONE per-image sum of the raw input
//   translation  out[r][c] = y[r - ty][c - tx] where that pixel exists, else `fill` in all four channels
//   cutout       out[r][c] = `fill` for y0 <= r < y0 + ch, x0 <= c < x0 + cw
// Memory bound: 16 bytes read and 16 written per pixel, one RGBA pixel per lane and access (global_load/store_dwordx4).
// Two launches when the colour stage is on, one otherwise:
//   da_sum_kernel    grid (chunks of 1024 pixels, N): lane partials over 4 pixels, wave butterfly, the 4 waves through LDS; one float
//                    per workgroup into the workspace.
//   da_fwd / da_bwd  the same grid; every workgroup adds its image's chunk partials again (lane-strided, then the same wave and
//                    workgroup tree), so nothing is handed from one workgroup to another inside a launch.
// No float atomics and no dependence on N or on the image's position in the batch: the chunking is a function of H * W alone, so an
// image's sum has the same bits alone and in any batch.  Without the colour bit no arithmetic touches a value: copy, move or fill.
#include "p2p_common.hpp"

#define DA_THREADS 256
#define DA_PIX 4                              // pixels per lane
#define DA_CHUNK (DA_THREADS * DA_PIX)        // pixels per workgroup: 16 KiB in, 16 KiB out
#define DA_COLOR 1
#define DA_TRANSLATION 2
#define DA_CUTOUT 4

struct DaGeom {
    int ty, tx, y0, x0, ch, cw;
};

// the image's geometry row with the stages that are switched off neutralised (wave-uniform address: scalar loads)
__device__ __forceinline__ DaGeom da_geom(const int* __restrict__ geometry, int b, int ch, int cw, int bits) {
    DaGeom g = {0, 0, 0, 0, 0, 0};
    if (bits & DA_TRANSLATION) { g.ty = geometry[b * 4 + 0]; g.tx = geometry[b * 4 + 1]; }
    if (bits & DA_CUTOUT) { g.y0 = geometry[b * 4 + 2]; g.x0 = geometry[b * 4 + 3]; g.ch = ch; g.cw = cw; }
    return g;
}

// is OUTPUT pixel (r, c) inside the cutout box?  (64-bit differences: a table may hold any int32)
__device__ __forceinline__ bool da_cut(const DaGeom& g, int r, int c) {
    const long long dr = (long long)r - g.y0, dc = (long long)c - g.x0;
    return dr >= 0 && dr < g.ch && dc >= 0 && dc < g.cw;
}

// sum of an image's chunk partials, valid in every lane: lane-strided, then wave butterfly, then the waves in order
__device__ __forceinline__ float da_total(const float* __restrict__ ws, int b, int chunks, float* red) {
    const float* in = ws + (long long)b * chunks;
    float s = 0.f;
    for (int i = threadIdx.x; i < chunks; i += DA_THREADS) s += in[i];
    return block_sum(s, red);
}

// ws[b][chunk] = sum over the chunk's pixels of the three colour channels of t.  MASKED (backward): t is the gradient of the
// OUTPUT; a pixel that the forward filled (no source pixel, or inside the box) does not count.
template <bool MASKED>
__global__ __launch_bounds__(DA_THREADS) void da_sum_kernel(int H, int W, const float* __restrict__ t, const int* __restrict__ geometry,
                                                            int ch, int cw, int bits, float* __restrict__ ws) {
    __shared__ float red[16];
    const int b = blockIdx.y, tid = threadIdx.x, HW = H * W;
    DaGeom g = {0, 0, 0, 0, 0, 0};
    if (MASKED) g = da_geom(geometry, b, ch, cw, bits);
    const float* in = t + (long long)b * HW * 4;
    float4 v[DA_PIX];
#pragma unroll
    for (int j = 0; j < DA_PIX; ++j) {          // all of the lane's loads are issued before the first value is used
        const int p = (blockIdx.x * DA_PIX + j) * DA_THREADS + tid;
        bool counts = p < HW;
        if (MASKED) {
            const int r = p / W, c = p - r * W;
            const long long sr = (long long)r - g.ty, sc = (long long)c - g.tx;
            counts = counts && sr >= 0 && sr < H && sc >= 0 && sc < W && !da_cut(g, r, c);
        }
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (counts) v[j] = *(const float4*)(in + (long long)p * 4);
    }
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < DA_PIX; ++j) acc += (v[j].x + v[j].y) + v[j].z;
    acc = block_sum(acc, red);
    if (tid == 0) ws[(long long)b * gridDim.x + blockIdx.x] = acc;
}

// one OUTPUT pixel per lane and step: fill, or the (colour-transformed) source pixel
__global__ __launch_bounds__(DA_THREADS) void da_fwd_kernel(int H, int W, const float* __restrict__ img, const float* __restrict__ color,
                                                            const int* __restrict__ geometry, int ch, int cw, int bits, float fill,
                                                            const float* __restrict__ ws, float* __restrict__ out) {
    __shared__ float red[16];
    const int b = blockIdx.y, tid = threadIdx.x, HW = H * W;
    const DaGeom g = da_geom(geometry, b, ch, cw, bits);
    const bool colour = bits & DA_COLOR;
    float cb = 0.f, cs = 1.f, ck = 1.f, m = 0.f;
    if (colour) {
        cb = color[b * 3 + 0]; cs = color[b * 3 + 1]; ck = color[b * 3 + 2];
        m = da_total(ws, b, gridDim.x, red) / (3.f * (float)HW) + cb;
    }
    const float* in = img + (long long)b * HW * 4;
    float* o = out + (long long)b * HW * 4;
    // all of the lane's loads are issued before the first value is used
    float4 v[DA_PIX];
    bool kept[DA_PIX];
#pragma unroll
    for (int j = 0; j < DA_PIX; ++j) {
        const int p = (blockIdx.x * DA_PIX + j) * DA_THREADS + tid;
        const int r = p / W, c = p - r * W;
        const long long sr = (long long)r - g.ty, sc = (long long)c - g.tx;
        kept[j] = p < HW && sr >= 0 && sr < H && sc >= 0 && sc < W && !da_cut(g, r, c);
        v[j] = make_float4(fill, fill, fill, fill);
        if (kept[j]) v[j] = *(const float4*)(in + (sr * W + sc) * 4);
    }
#pragma unroll
    for (int j = 0; j < DA_PIX; ++j) {
        const int p = (blockIdx.x * DA_PIX + j) * DA_THREADS + tid;
        if (p >= HW) continue;
        if (colour && kept[j]) {
            const float u0 = v[j].x + cb, u1 = v[j].y + cb, u2 = v[j].z + cb;
            const float sbar = ((u0 + u1) + u2) / 3.f;
            v[j].x = ((u0 - sbar) * cs + sbar - m) * ck + m;
            v[j].y = ((u1 - sbar) * cs + sbar - m) * ck + m;
            v[j].z = ((u2 - sbar) * cs + sbar - m) * ck + m;
        }
        *(float4*)(o + (long long)p * 4) = v[j];
    }
}

// one INPUT pixel per lane and step.  g' = the output gradient at the pixel's destination (r + ty, c + tx), 0 where the forward wrote
// `fill` there or the destination lies outside; with Gamma the image's sum of g' over pixels and colour channels (da_sum_kernel<true>):
//   dv = k g' + (1 - k) Gamma / N,   dx_c = s dv_c + (1 - s) / 3 sum_c' dv_c'   (c < 3),   dx_3 = g'_3.
__global__ __launch_bounds__(DA_THREADS) void da_bwd_kernel(int H, int W, const float* __restrict__ gout, const float* __restrict__ color,
                                                            const int* __restrict__ geometry, int ch, int cw, int bits,
                                                            const float* __restrict__ ws, float* __restrict__ gimg) {
    __shared__ float red[16];
    const int b = blockIdx.y, tid = threadIdx.x, HW = H * W;
    const DaGeom g = da_geom(geometry, b, ch, cw, bits);
    const bool colour = bits & DA_COLOR;
    float cs = 1.f, ck = 1.f, shift = 0.f;
    if (colour) {
        cs = color[b * 3 + 1]; ck = color[b * 3 + 2];
        shift = (1.f - ck) * (da_total(ws, b, gridDim.x, red) / (3.f * (float)HW));
    }
    const float* in = gout + (long long)b * HW * 4;
    float* o = gimg + (long long)b * HW * 4;
    float4 v[DA_PIX];
#pragma unroll
    for (int j = 0; j < DA_PIX; ++j) {
        const int p = (blockIdx.x * DA_PIX + j) * DA_THREADS + tid;
        const int r = p / W, c = p - r * W;
        const long long dr = (long long)r + g.ty, dc = (long long)c + g.tx;
        v[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p < HW && dr >= 0 && dr < H && dc >= 0 && dc < W && !da_cut(g, (int)dr, (int)dc)) v[j] = *(const float4*)(in + (dr * W + dc) * 4);
    }
#pragma unroll
    for (int j = 0; j < DA_PIX; ++j) {
        const int p = (blockIdx.x * DA_PIX + j) * DA_THREADS + tid;
        if (p >= HW) continue;
        if (colour) {
            const float d0 = ck * v[j].x + shift, d1 = ck * v[j].y + shift, d2 = ck * v[j].z + shift;
            const float mean = ((d0 + d1) + d2) / 3.f;
            v[j].x = (d0 - mean) * cs + mean;
            v[j].y = (d1 - mean) * cs + mean;
            v[j].z = (d2 - mean) * cs + mean;
        }
        *(float4*)(o + (long long)p * 4) = v[j];
    }
}

static inline int da_chunks(int H, int W) { return (int)(((long long)H * W + DA_CHUNK - 1) / DA_CHUNK); }

static int da_check(const char* who, int N, int H, int W, const void* in, const float* color, const int* geometry, int ch, int cw,
                    int bits, const void* out, const float* workspace) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && (long long)H * W <= (1LL << 28) && N <= 65535,
                "%s: bad shape %d x %d x %d (H * W <= 2^28, N <= 65535)", who, N, H, W);
    P2P_REQUIRE((bits & ~(DA_COLOR | DA_TRANSLATION | DA_CUTOUT)) == 0, "%s: policy_bits = %d (1 colour, 2 translation, 4 cutout)", who, bits);
    P2P_REQUIRE(in && out && in != out, "%s: null pointer, or input and output are one buffer (the translation reads other pixels)", who);
    P2P_REQUIRE(((uintptr_t)in % 16) == 0 && ((uintptr_t)out % 16) == 0, "%s: the images must be 16-byte aligned", who);
    P2P_REQUIRE(!(bits & DA_COLOR) || (color && workspace), "%s: the colour stage needs the color table and the workspace", who);
    P2P_REQUIRE(!(bits & (DA_TRANSLATION | DA_CUTOUT)) || geometry, "%s: translation and cutout need the geometry table", who);
    P2P_REQUIRE(!(bits & DA_CUTOUT) || (ch >= 0 && cw >= 0), "%s: cutout box %d x %d", who, ch, cw);
    return 0;
}

extern "C" long long p2p_diffaug_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (long long)N * da_chunks(H, W) * (long long)sizeof(float);
}

extern "C" int p2p_diffaug_fwd(int N, int H, int W, const float* img, const float* color, const int* geometry, int ch, int cw,
                               int policy_bits, float fill, float* out, float* workspace, void* stream) {
    if (da_check("p2p_diffaug_fwd", N, H, W, img, color, geometry, ch, cw, policy_bits, out, workspace)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(da_chunks(H, W), N);
    if (policy_bits & DA_COLOR) da_sum_kernel<false><<<grid, DA_THREADS, 0, st>>>(H, W, img, geometry, ch, cw, policy_bits, workspace);
    da_fwd_kernel<<<grid, DA_THREADS, 0, st>>>(H, W, img, color, geometry, ch, cw, policy_bits, fill, workspace, out);
    return p2p_check_launch("p2p_diffaug_fwd");
}

extern "C" int p2p_diffaug_bwd(int N, int H, int W, const float* grad_out, const float* color, const int* geometry, int ch, int cw,
                               int policy_bits, float fill, float* grad_img, float* workspace, void* stream) {
    (void)fill;          // the gradient does not depend on the fill value
    if (da_check("p2p_diffaug_bwd", N, H, W, grad_out, color, geometry, ch, cw, policy_bits, grad_img, workspace)) return -1;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(da_chunks(H, W), N);
    if (policy_bits & DA_COLOR) da_sum_kernel<true><<<grid, DA_THREADS, 0, st>>>(H, W, grad_out, geometry, ch, cw, policy_bits, workspace);
    da_bwd_kernel<<<grid, DA_THREADS, 0, st>>>(H, W, grad_out, color, geometry, ch, cw, policy_bits, workspace, grad_img);
    return p2p_check_launch("p2p_diffaug_bwd");
}
