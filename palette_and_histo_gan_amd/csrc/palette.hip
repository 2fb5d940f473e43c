// Soft palette histogram and conformance of an RGBA image under a palette, their VJP, and the palette of an image
// (DESIGN.md "palette loss").  With x_p = img_p * 0.5 + 0.5 (four channels), c_k = pal_k / 255 and n valid slots:
//   d_pk = sum_c (x_pc - c_kc)^2,   w_pk = softmax_k(-(d_pk - min_j d_pj) / tau),
//   h_k = mean_p w_pk,   m = mean_p sum_k w_pk d_pk.
// Vector-ALU and exponential bound (H*W*K pair evaluations per image), no matrix work.  The image's palette sits in LDS as one
// float4 per slot (4 KB); the slot loops read it at a wave-uniform address (broadcast, one ds_read_b128 per slot shared by the
// lane's pixels); every lane owns its own pixels.  All reductions run in a fixed order (no float atomics): bit-reproducible.
// p2p_palette_snap, further down, is the hard counterpart in integer arithmetic (nearest slot, lowest index on ties);
// p2p_palette_project_fwd / _bwd, after it, replace every pixel by a palette colour, differentiably.
#include "p2p_common.hpp"

#define PAL_MAX 256
#define PAL_THREADS 256
#define PAL_FWD_PIX 4                       // pixels per lane, forward
#define PAL_BWD_PIX 2                       // pixels per lane, backward
#define PAL_WS_STRIDE 260                   // floats per (image, chunk) partial: 256 slot sums, the conformance sum, padding

__device__ __forceinline__ float pal_dist(const float4& x, const float4& c) {
    const float dx = x.x - c.x, dy = x.y - c.y, dz = x.z - c.z, dw = x.w - c.w;
    // spelled out: the passes over the slots must reproduce each other's d bit for bit (d - min is 0 at the nearest slot)
    return __fmaf_rn(dw, dw, __fmaf_rn(dz, dz, __fmaf_rn(dy, dy, __fmul_rn(dx, dx))));
}

__device__ __forceinline__ float4 pal_x(const float* __restrict__ img, long long pix) {
    const float4 v = *(const float4*)(img + pix * 4);
    return make_float4(__fmaf_rn(v.x, 0.5f, 0.5f), __fmaf_rn(v.y, 0.5f, 0.5f), __fmaf_rn(v.z, 0.5f, 0.5f), __fmaf_rn(v.w, 0.5f, 0.5f));
}

// the image's valid slots as float4 colours in LDS; returns their count (0: nothing to do)
__device__ __forceinline__ int pal_load(const int* __restrict__ palette, const int* __restrict__ sizes, int b, int K, float4* c) {
    int n = sizes[b];
    n = n < 0 ? 0 : (n > K ? K : n);
    for (int k = threadIdx.x; k < n; k += blockDim.x) {
        const int4 q = *(const int4*)(palette + ((long long)b * K + k) * 4);
        c[k] = make_float4((float)q.x / 255.f, (float)q.y / 255.f, (float)q.z / 255.f, (float)q.w / 255.f);
    }
    __syncthreads();
    return n;
}

// Forward, grid (chunks, N): a workgroup owns PAL_THREADS * PAL_FWD_PIX consecutive pixels of one image and writes the sums of
// its pixels' weights per slot and of their conformance to ws[image][chunk][PAL_WS_STRIDE].
//   pass 1: min_k d;  pass 2: S = sum_k e_k and sum_k e_k (d_k - min), e_k = exp2((d_k - min) * nscale), nscale = -log2(e) / tau;
//   pass 3: per slot, e_k / S summed over the lane's pixels, across the wave (butterfly), then across the waves through LDS.
__global__ __launch_bounds__(PAL_THREADS) void soft_palette_fwd_kernel(int HW, const float* __restrict__ img, const int* __restrict__ palette,
                                                                       const int* __restrict__ sizes, int K, float nscale,
                                                                       float* __restrict__ ws) {
    __shared__ float4 c[PAL_MAX];
    __shared__ float part[PAL_THREADS / 64][PAL_MAX];
    __shared__ float red[16];
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float* out = ws + ((long long)b * gridDim.x + blockIdx.x) * PAL_WS_STRIDE;
    const int n = pal_load(palette, sizes, b, K, c);
    if (n == 0) {                           // the whole workgroup: an image without a palette contributes nothing
        for (int k = tid; k < PAL_WS_STRIDE; k += PAL_THREADS) out[k] = 0.f;
        return;
    }
    float4 x[PAL_FWD_PIX];
    float mn[PAL_FWD_PIX], inv[PAL_FWD_PIX];
    bool valid[PAL_FWD_PIX];
#pragma unroll
    for (int j = 0; j < PAL_FWD_PIX; ++j) {
        const int p = (blockIdx.x * PAL_FWD_PIX + j) * PAL_THREADS + tid;
        valid[j] = p < HW;
        x[j] = valid[j] ? pal_x(img, (long long)b * HW + p) : make_float4(0.f, 0.f, 0.f, 0.f);
        mn[j] = INFINITY;
    }
    for (int k = 0; k < n; ++k) {
        const float4 ck = c[k];
#pragma unroll
        for (int j = 0; j < PAL_FWD_PIX; ++j) mn[j] = fminf(mn[j], pal_dist(x[j], ck));
    }
    float S[PAL_FWD_PIX], D[PAL_FWD_PIX];
#pragma unroll
    for (int j = 0; j < PAL_FWD_PIX; ++j) S[j] = D[j] = 0.f;
    for (int k = 0; k < n; ++k) {
        const float4 ck = c[k];
#pragma unroll
        for (int j = 0; j < PAL_FWD_PIX; ++j) {
            const float t = pal_dist(x[j], ck) - mn[j];
            const float e = __builtin_amdgcn_exp2f(t * nscale);
            S[j] += e;
            D[j] = __fmaf_rn(e, t, D[j]);
        }
    }
    float conf = 0.f;
#pragma unroll
    for (int j = 0; j < PAL_FWD_PIX; ++j) {
        inv[j] = valid[j] ? 1.f / S[j] : 0.f;                 // S >= 1: the nearest slot contributes exp2(0)
        conf += valid[j] ? mn[j] + D[j] * inv[j] : 0.f;       // sum_k w_k d_k = min + sum_k w_k (d_k - min)
    }
    for (int k = 0; k < n; ++k) {
        const float4 ck = c[k];
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < PAL_FWD_PIX; ++j) {
            const float t = pal_dist(x[j], ck) - mn[j];
            acc = __fmaf_rn(__builtin_amdgcn_exp2f(t * nscale), inv[j], acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) part[wave][k] = acc;
    }
    __syncthreads();
    for (int k = tid; k < PAL_MAX; k += PAL_THREADS) {
        float s = 0.f;
        if (k < n)
            for (int w = 0; w < PAL_THREADS / 64; ++w) s += part[w][k];
        out[k] = s;
    }
    conf = block_sum(conf, red);
    if (tid == 0) out[PAL_MAX] = conf;
}

// hist[b][k] = (sum over the image's chunks, in chunk order) / HW; conf[b] likewise.  Grid N.
__global__ __launch_bounds__(PAL_THREADS) void soft_palette_finish_kernel(int HW, int chunks, int K, const float* __restrict__ ws,
                                                                          float* __restrict__ hist, float* __restrict__ conf) {
    const int b = blockIdx.x;
    const float* in = ws + (long long)b * chunks * PAL_WS_STRIDE;
    for (int k = threadIdx.x; k <= PAL_MAX; k += PAL_THREADS) {
        if (k >= K && k != PAL_MAX) continue;
        float s = 0.f;
        for (int ch = 0; ch < chunks; ++ch) s += in[(long long)ch * PAL_WS_STRIDE + k];
        s = s / (float)HW;
        if (k == PAL_MAX) conf[b] = s;
        else hist[(long long)b * K + k] = s;
    }
}

// VJP, grid (chunks, N), one dimg pixel per lane and step.  With r the nearest slot of the pixel, a_k = gh_k + gm d_k (times 1/HW)
// and E[.] the mean under w:  sum_k w_k (a_k - E a) c_k = E[(a - a_r)(c - c_r)] - E[a - a_r] E[c - c_r]  -- the covariance taken
// about slot r.  Where one colour dominates, a_k - E a cancels to rounding in f32; about r every term of the dominant slot is
// exactly 0 and the rest is small times small, so no wide arithmetic is needed.  x - E c = (x - c_r) - E[c - c_r] likewise.
//   pass 1: min_k d and its first index r;  pass 2: one exponential per pair and the ten running sums.
// TV (p2p_soft_palette_tv_bwd): the upstream gradient of the total-variation and conformance means is formed here instead of read
// from a table -- gh is h_fake and gm is h_real, g_k = w_tv sgn(h_fake_k - h_real_k) (sgn 0 = 0: tf.abs) and the conformance weight
// is w_conf for every image.  Everything behind the two loads is the one body: the same f32 operations on the same values.
template <bool TV>
__global__ __launch_bounds__(PAL_THREADS) void soft_palette_bwd_kernel(int HW, const float* __restrict__ img, const int* __restrict__ palette,
                                                                       const int* __restrict__ sizes, int K, float nscale, float two_over_tau,
                                                                       const float* __restrict__ gh, const float* __restrict__ gm,
                                                                       float w_tv, float w_conf, float* __restrict__ dimg) {
    __shared__ float4 c[PAL_MAX];
    __shared__ float g[PAL_MAX];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = pal_load(palette, sizes, b, K, c);
    int pix[PAL_BWD_PIX];
    bool valid[PAL_BWD_PIX];
#pragma unroll
    for (int j = 0; j < PAL_BWD_PIX; ++j) {
        pix[j] = (blockIdx.x * PAL_BWD_PIX + j) * PAL_THREADS + tid;
        valid[j] = pix[j] < HW;
    }
    if (n == 0) {
#pragma unroll
        for (int j = 0; j < PAL_BWD_PIX; ++j)
            if (valid[j]) *(float4*)(dimg + ((long long)b * HW + pix[j]) * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    for (int k = tid; k < n; k += PAL_THREADS) {
        const long long e = (long long)b * K + k;
        if (TV) {
            const float d = gh[e] - gm[e];
            g[k] = d > 0.f ? w_tv : (d < 0.f ? -w_tv : 0.f);
        } else {
            g[k] = gh[e];
        }
    }
    __syncthreads();
    const float gmb = TV ? w_conf : gm[b];
    float4 x[PAL_BWD_PIX];
    float mn[PAL_BWD_PIX];
    int r[PAL_BWD_PIX];
#pragma unroll
    for (int j = 0; j < PAL_BWD_PIX; ++j) {
        x[j] = valid[j] ? pal_x(img, (long long)b * HW + pix[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        mn[j] = INFINITY;
        r[j] = 0;
    }
    for (int k = 0; k < n; ++k) {
        const float4 ck = c[k];
#pragma unroll
        for (int j = 0; j < PAL_BWD_PIX; ++j) {
            const float d = pal_dist(x[j], ck);
            if (d < mn[j]) { mn[j] = d; r[j] = k; }
        }
    }
    float4 cr[PAL_BWD_PIX], Ec[PAL_BWD_PIX], Eac[PAL_BWD_PIX];
    float gr[PAL_BWD_PIX], S[PAL_BWD_PIX], Ea[PAL_BWD_PIX];
#pragma unroll
    for (int j = 0; j < PAL_BWD_PIX; ++j) {
        cr[j] = c[r[j]];
        gr[j] = g[r[j]];
        S[j] = Ea[j] = 0.f;
        Ec[j] = Eac[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int k = 0; k < n; ++k) {
        const float4 ck = c[k];
        const float gk = g[k];
#pragma unroll
        for (int j = 0; j < PAL_BWD_PIX; ++j) {
            const float t = pal_dist(x[j], ck) - mn[j];
            const float e = __builtin_amdgcn_exp2f(t * nscale);
            const float ea = e * __fmaf_rn(gmb, t, gk - gr[j]);              // e (a_k - a_r), HW left out
            const float cx = ck.x - cr[j].x, cy = ck.y - cr[j].y, cz = ck.z - cr[j].z, cw = ck.w - cr[j].w;
            S[j] += e;
            Ea[j] += ea;
            Ec[j].x = __fmaf_rn(e, cx, Ec[j].x); Ec[j].y = __fmaf_rn(e, cy, Ec[j].y);
            Ec[j].z = __fmaf_rn(e, cz, Ec[j].z); Ec[j].w = __fmaf_rn(e, cw, Ec[j].w);
            Eac[j].x = __fmaf_rn(ea, cx, Eac[j].x); Eac[j].y = __fmaf_rn(ea, cy, Eac[j].y);
            Eac[j].z = __fmaf_rn(ea, cz, Eac[j].z); Eac[j].w = __fmaf_rn(ea, cw, Eac[j].w);
        }
    }
    const float inv_hw = 1.f / (float)HW;
#pragma unroll
    for (int j = 0; j < PAL_BWD_PIX; ++j) {
        if (!valid[j]) continue;
        const float is = 1.f / S[j];
        const float ea = Ea[j] * is;
        const float s1 = 0.5f * two_over_tau * inv_hw, s2 = gmb * inv_hw;    // 0.5: d x / d img
        float4 o;
        o.x = s1 * (Eac[j].x * is - ea * (Ec[j].x * is)) + s2 * ((x[j].x - cr[j].x) - Ec[j].x * is);
        o.y = s1 * (Eac[j].y * is - ea * (Ec[j].y * is)) + s2 * ((x[j].y - cr[j].y) - Ec[j].y * is);
        o.z = s1 * (Eac[j].z * is - ea * (Ec[j].z * is)) + s2 * ((x[j].z - cr[j].z) - Ec[j].z * is);
        o.w = s1 * (Eac[j].w * is - ea * (Ec[j].w * is)) + s2 * ((x[j].w - cr[j].w) - Ec[j].w * is);
        *(float4*)(dimg + ((long long)b * HW + pix[j]) * 4) = o;
    }
}

// The two loss values of a batch from its soft histograms (fused step): per image tv_b = 0.5 sum_{k < n_b} |h_fake - h_real|
// added in ascending k, then inv_batch * sum_b tv_b and inv_batch * sum_b conf_fake_b added in ascending b (an image with n_b <= 0
// is left out of both).  One workgroup: PAL_LOSS_IMGS images at a time, their |differences| staged through LDS with coalesced loads
// (rows padded to 257 floats: lane j walks row j without bank conflicts), one lane per image for the sum over the slots, lane 0 for
// the sum over the images.  Every sum has one order whatever B is: an image's term does not depend on its neighbours, two launches
// give the same bits.
#define PAL_LOSS_IMGS 32

__global__ __launch_bounds__(PAL_THREADS) void palette_loss_kernel(int B, int K, const float* __restrict__ h_real, const float* __restrict__ h_fake,
                                                                   const float* __restrict__ conf_fake, const int* __restrict__ sizes,
                                                                   float inv_batch, float* __restrict__ out_tv, float* __restrict__ out_conf) {
    __shared__ float diff[PAL_LOSS_IMGS][PAL_MAX + 1];
    __shared__ float tv[PAL_LOSS_IMGS], cf[PAL_LOSS_IMGS];
    const int tid = threadIdx.x;
    float sum_tv = 0.f, sum_cf = 0.f;                        // lane 0
    for (int b0 = 0; b0 < B; b0 += PAL_LOSS_IMGS) {
        const int nb = B - b0 < PAL_LOSS_IMGS ? B - b0 : PAL_LOSS_IMGS;
        for (int i = tid; i < nb * K; i += PAL_THREADS) {
            const int j = i / K, k = i - j * K;
            const long long e = (long long)b0 * K + i;
            diff[j][k] = fabsf(h_fake[e] - h_real[e]);
        }
        __syncthreads();
        if (tid < nb) {
            int n = sizes[b0 + tid];
            n = n < 0 ? 0 : (n > K ? K : n);
            float s = 0.f;
            for (int k = 0; k < n; ++k) s += diff[tid][k];
            tv[tid] = 0.5f * s;
            cf[tid] = n > 0 ? conf_fake[b0 + tid] : 0.f;
        }
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < nb; ++j) {
                sum_tv += tv[j];
                sum_cf += cf[j];
            }
    }
    if (tid == 0) {
        *out_tv = inv_batch * sum_tv;
        *out_conf = inv_batch * sum_cf;
    }
}

// Palette of an image: its distinct quantised RGBA colours in ascending order of r + 256 g + 65536 b + 2^24 a.  One workgroup per
// image: an open-addressing hash set in LDS (integer atomics only), then a rank sort of the occupied slots.  A slot is 64 bits wide
// because every 32-bit value is a key (opaque white is 0xFFFFFFFF): EMPTY lies outside the key space.  More than `cap` colours:
// size -1, zeroed row.  Every insertion past the cap raises `over`, which every lane reads before its next pixel, so at most
// cap + PAL_THREADS keys are ever stored in the PAL_TABLE slots: a probe always finds a free slot, and is bounded by the table
// size regardless.
#define PAL_TABLE 1024
#define PAL_EMPTY 0xFFFFFFFFFFFFFFFFull

__device__ __forceinline__ unsigned pal_quant(float v) {
    // clamp(floor((v * 0.5 + 0.5) * 255 + 0.5), 0, 255), every step rounded to f32 on its own
    const float q = floorf(__fadd_rn(__fmul_rn(__fmaf_rn(v, 0.5f, 0.5f), 255.f), 0.5f));
    return (unsigned)fminf(fmaxf(q, 0.f), 255.f);          // fmaxf(NaN, 0) = 0
}

// The hash set as device functions (palette_extract_kernel and palette_quantize_kernel share them): clear, then a barrier; insert
// from any lane; after a barrier `over` says whether more than cap keys arrived, and if not pal_set_rows writes the sorted rows.
struct PalSet {
    unsigned long long table[PAL_TABLE];
    unsigned keys[PAL_MAX];
    int count, over, m, pad;
};

__device__ __forceinline__ void pal_set_clear(PalSet* s) {
    for (int i = threadIdx.x; i < PAL_TABLE; i += PAL_THREADS) s->table[i] = PAL_EMPTY;
    if (threadIdx.x == 0) { s->count = 0; s->over = 0; s->m = 0; }
}

__device__ __forceinline__ void pal_set_insert(PalSet* s, unsigned key, int cap) {
    unsigned slot = (key * 2654435761u) >> 22;          // Fibonacci hash, top 10 bits
    for (int probe = 0; probe < PAL_TABLE; ++probe) {
        const unsigned long long seen = atomicCAS(&s->table[slot], PAL_EMPTY, (unsigned long long)key);
        if (seen == (unsigned long long)key) break;     // already there
        if (seen == PAL_EMPTY) {                         // this lane inserted it
            if (atomicAdd(&s->count, 1) + 1 > cap) atomicExch(&s->over, 1);
            break;
        }
        slot = (slot + 1) & (PAL_TABLE - 1);
    }
}

// The whole workgroup, with over == 0: the set's keys in ascending order as int32 RGBA rows row[0 .. n), zero rows up to `rows`;
// returns n.  Holds a barrier.
__device__ __forceinline__ int pal_set_rows(PalSet* s, int cap, int rows, int* __restrict__ row) {
    const int tid = threadIdx.x;
    for (int i = tid; i < PAL_TABLE; i += PAL_THREADS) {
        const unsigned long long e = s->table[i];
        if (e != PAL_EMPTY) {
            const int at = atomicAdd(&s->m, 1);               // any order: the ranks below do not depend on it
            if (at < PAL_MAX) s->keys[at] = (unsigned)e;
        }
    }
    __syncthreads();
    const int n = s->m < cap ? s->m : cap;                   // m == count <= cap <= PAL_MAX here
    for (int i = n + tid; i < rows; i += PAL_THREADS) *(int4*)(row + 4 * i) = make_int4(0, 0, 0, 0);
    if (tid < n) {
        const unsigned key = s->keys[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += s->keys[j] < key ? 1 : 0;      // keys are distinct
        *(int4*)(row + 4 * rank) = make_int4((int)(key & 255u), (int)((key >> 8) & 255u), (int)((key >> 16) & 255u), (int)(key >> 24));
    }
    return n;
}

__global__ __launch_bounds__(PAL_THREADS) void palette_extract_kernel(int HW, const float* __restrict__ img, int cap, int* __restrict__ pal_out,
                                                                      int* __restrict__ sizes_out) {
    __shared__ PalSet set;
    const int b = blockIdx.x, tid = threadIdx.x;
    pal_set_clear(&set);
    __syncthreads();
    for (int p = tid; p < HW; p += PAL_THREADS) {
        if (*(volatile int*)&set.over) break;
        const float4 v = *(const float4*)(img + ((long long)b * HW + p) * 4);
        pal_set_insert(&set, pal_quant(v.x) | (pal_quant(v.y) << 8) | (pal_quant(v.z) << 16) | (pal_quant(v.w) << 24), cap);
    }
    __syncthreads();
    int* row = pal_out + (long long)b * cap * 4;
    if (set.over) {
        for (int i = tid; i < cap * 4; i += PAL_THREADS) row[i] = 0;
        if (tid == 0) sizes_out[b] = -1;
        return;
    }
    const int n = pal_set_rows(&set, cap, cap, row);
    if (tid == 0) sizes_out[b] = n;
}

// Hard counterpart of the soft histogram: every pixel's nearest palette slot, in integers (DESIGN.md "palette snap").  A pixel is
// quantised with pal_quant and packed into one word q; a slot sits in LDS as its packed bytes c_k and the word
// ((|c_k|^2 + PAL_SNAP_BIAS) << 8) | k.  key_pk = word_k - (dot4(q, c_k) << 9) is ((|c_k|^2 - 2 q.c_k + BIAS) << 8) | k: the bias
// 2 * 4 * 255^2 keeps the score non-negative (it is at most 3 * 4 * 255^2 = 780300 < 2^20, so the shifted score fits 28 bits), and
// one unsigned min over k yields the nearest slot and, among equals, the lowest k.  dist = (key >> 8) - BIAS + |q|^2.
// Grid (chunks, N): a workgroup owns PAL_THREADS * PAL_SNAP_PIX consecutive pixels of one image, counts its pixels per slot in LDS
// and adds the non-zero counts and its two sums to global memory with integer atomics (any order gives the same bits);
// palette_snap_clear_kernel zeroes those outputs first.
#define PAL_SNAP_PIX 4
#define PAL_SNAP_BIAS 520200u

// The packed-key code that p2p_palette_snap and the hard forward of p2p_palette_project_fwd share, so that their bits cannot drift
// apart: the pixel's packed bytes, the slots in LDS (returns the clamped slot count; the caller synchronises), one step of the
// unsigned min, and the normalised colour of a slot's packed bytes.
__device__ __forceinline__ unsigned pal_snap_quant(const float4& v) {
    return pal_quant(v.x) | (pal_quant(v.y) << 8) | (pal_quant(v.z) << 16) | (pal_quant(v.w) << 24);
}

__device__ __forceinline__ uint2 pal_snap_slot(unsigned pk, int k) {
    return make_uint2(pk, ((__builtin_amdgcn_udot4(pk, pk, 0u, false) + PAL_SNAP_BIAS) << 8) | (unsigned)k);
}

__device__ __forceinline__ int pal_snap_load(const int* __restrict__ palette, const int* __restrict__ sizes, int b, int K, uint2* slot) {
    int n = sizes[b];
    n = n < 0 ? 0 : (n > K ? K : n);
    for (int k = threadIdx.x; k < n; k += PAL_THREADS) {
        const int4 c = *(const int4*)(palette + ((long long)b * K + k) * 4);
        const unsigned cx = (unsigned)c.x & 255u, cy = (unsigned)c.y & 255u, cz = (unsigned)c.z & 255u, cw = (unsigned)c.w & 255u;
        slot[k] = pal_snap_slot(cx | (cy << 8) | (cz << 16) | (cw << 24), k);
    }
    return n;
}

__device__ __forceinline__ unsigned pal_snap_min(unsigned key, unsigned q, const uint2& s) {
    const unsigned k2 = s.y - (__builtin_amdgcn_udot4(q, s.x, 0u, false) << 9);
    return k2 < key ? k2 : key;
}

__device__ __forceinline__ float4 pal_snap_colour(unsigned c) {
    return make_float4(__fsub_rn(__fdiv_rn((float)(c & 255u), 127.5f), 1.0f), __fsub_rn(__fdiv_rn((float)((c >> 8) & 255u), 127.5f), 1.0f),
                       __fsub_rn(__fdiv_rn((float)((c >> 16) & 255u), 127.5f), 1.0f), __fsub_rn(__fdiv_rn((float)(c >> 24), 127.5f), 1.0f));
}

__global__ __launch_bounds__(PAL_THREADS) void palette_snap_clear_kernel(long long n_counts, int* __restrict__ counts, long long n_stats,
                                                                         long long* __restrict__ stats) {
    const long long i = (long long)blockIdx.x * PAL_THREADS + threadIdx.x;
    if (i < n_counts) counts[i] = 0;
    if (i < n_stats) stats[i] = 0;
}

__global__ __launch_bounds__(PAL_THREADS) void palette_snap_kernel(int HW, const float* __restrict__ img, const int* __restrict__ palette,
                                                                   const int* __restrict__ sizes, int K, int* __restrict__ index_out,
                                                                   float* __restrict__ image_out, int* __restrict__ dist_out,
                                                                   int* __restrict__ counts, long long* __restrict__ stats) {
    __shared__ uint2 slot[PAL_MAX];          // x: packed bytes, y: key word
    __shared__ int cnt[PAL_MAX];
    __shared__ unsigned sums[2];             // off-palette pixels and summed distances of the workgroup (<= 1024 * 260100 < 2^32)
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = pal_snap_load(palette, sizes, b, K, slot);
    for (int k = tid; k < n; k += PAL_THREADS) cnt[k] = 0;
    if (tid < 2) sums[tid] = 0u;
    __syncthreads();
    const long long base = (long long)b * HW;
    unsigned q[PAL_SNAP_PIX], key[PAL_SNAP_PIX];
    bool valid[PAL_SNAP_PIX];
#pragma unroll
    for (int j = 0; j < PAL_SNAP_PIX; ++j) {
        const int p = (blockIdx.x * PAL_SNAP_PIX + j) * PAL_THREADS + tid;
        valid[j] = p < HW;
        q[j] = 0u;
        key[j] = 0xFFFFFFFFu;
        if (!valid[j]) continue;
        const float4 v = *(const float4*)(img + (base + p) * 4);
        if (n == 0) {                        // nothing to snap to: the pixel passes through bit for bit
            index_out[base + p] = -1;
            if (dist_out) dist_out[base + p] = 0;
            if (image_out) *(float4*)(image_out + (base + p) * 4) = v;
        }
        q[j] = pal_snap_quant(v);
    }
    if (n == 0) return;                      // the whole workgroup; counts and stats stay 0
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
        const uint2 s = slot[k];             // wave-uniform address: one broadcast ds_read_b64 for the lane's pixels
#pragma unroll
        for (int j = 0; j < PAL_SNAP_PIX; ++j) key[j] = pal_snap_min(key[j], q[j], s);
    }
    unsigned off = 0u, dsum = 0u;
#pragma unroll
    for (int j = 0; j < PAL_SNAP_PIX; ++j) {
        if (!valid[j]) continue;
        const int p = (blockIdx.x * PAL_SNAP_PIX + j) * PAL_THREADS + tid;
        const int idx = (int)(key[j] & 255u);
        const unsigned d = (key[j] >> 8) - PAL_SNAP_BIAS + __builtin_amdgcn_udot4(q[j], q[j], 0u, false);
        index_out[base + p] = idx;
        if (dist_out) dist_out[base + p] = (int)d;
        if (image_out) *(float4*)(image_out + (base + p) * 4) = pal_snap_colour(slot[idx].x);
        atomicAdd(&cnt[idx], 1);
        off += d > 0u ? 1u : 0u;
        dsum += d;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        off += __shfl_xor(off, o, 64);
        dsum += __shfl_xor(dsum, o, 64);
    }
    if ((tid & 63) == 0) {
        atomicAdd(&sums[0], off);
        atomicAdd(&sums[1], dsum);
    }
    __syncthreads();
    for (int k = tid; k < n; k += PAL_THREADS)
        if (cnt[k]) atomicAdd(counts + (long long)b * K + k, cnt[k]);
    if (tid < 2 && sums[tid]) atomicAdd((unsigned long long*)(stats + (long long)b * 2 + tid), (unsigned long long)sums[tid]);
}

// A palette of at most `colours` colours FOR an image, derived from the image itself (the contract is the comment of
// p2p_palette_quantize in p2pgan.h): farthest-point starting slots, then Lloyd passes, all in integers.  One workgroup per image and
// everything in dynamic LDS: the scratch below, then the image's packed keys (4 B per pixel) and the running minimum m_p of the
// farthest-point selection (4 B per pixel) -- 17.1 KB + 8 HW bytes: 49 KB at 64 x 64 (three workgroups per CU), 145 KB at 128 x 128.
//   exact path:      the bounded hash set of palette_extract_kernel with cap = colours; `over` is read after a barrier.
//   farthest point:  per step one sweep over the pixels (m_p = min(m_p, D(q_p, C[j-1])), best = max of (m_p << 32) | ~key, i.e. the
//                    largest m_p and among equals the lowest key), a wave64 butterfly and one barrier: red[] is double-buffered by
//                    the step's parity, and every lane takes the maximum of the four wave results itself.  Step 0 runs on
//                    m_p = 2^32 - 1 everywhere, so it returns the lowest key.
//   Lloyd pass:      the snap's packed-key minimum over slot[] (pal_snap_min), PAL_SNAP_PIX pixels per lane and sweep; per-slot count
//                    and channel sums are LDS integer atomics.  A sprite is mostly one colour, so lanes that share their slot with
//                    the first pending lane are summed across the wave first (up to PAL_Q_ROUNDS such groups per sweep, a group of
//                    fewer than PAL_Q_GROUP lanes is not worth the butterfly) and one lane adds the totals; integer sums, so the
//                    grouping cannot change a bit.  Then one lane per slot rounds the centroid, raises changed[t & 1] if it moved
//                    and clears the sums; all lanes read the flag behind a barrier and leave together.
// Every loop is bounded by HW, colours, iterations or a constant; no barrier stands under a condition that differs between lanes.
#define PAL_Q_MAXPIX (1 << 14)
#define PAL_Q_ROUNDS 3
#define PAL_Q_GROUP 8

struct PalQuantScratch {
    PalSet set;
    uint2 slot[PAL_MAX];                                   // x: packed bytes, y: key word (pal_snap_slot)
    unsigned acc[5][PAL_MAX];                              // n_k and the four channel sums S_k
    unsigned first[PAL_MAX];                               // 1 where no lower slot holds the same colour
    unsigned long long red[2][PAL_THREADS / 64];
    int changed[2], pad[2];
};
static_assert(sizeof(PalQuantScratch) % 16 == 0, "the keys behind the scratch stay 16-byte aligned");

__device__ __forceinline__ unsigned pal_q_wave_sum(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// adds pixel q to slot k's count and sums for every lane with `valid`; the whole wave calls it
__device__ __forceinline__ void pal_q_add(unsigned (*acc)[PAL_MAX], bool valid, unsigned k, unsigned q) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(valid), direct = 0ull;
#pragma unroll
    for (int round = 0; round < PAL_Q_ROUNDS; ++round) {
        if (todo == 0ull) break;                           // wave-uniform, as everything that steers this loop
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned lk = __shfl(k, leader, 64);
        const bool mine = ((todo >> lane) & 1ull) && k == lk;
        const unsigned long long match = __ballot(mine);
        todo &= ~match;
        if (__popcll(match) < PAL_Q_GROUP) {
            direct |= match;
            continue;
        }
        // two channels per word: 64 lanes * 255 < 2^16
        const unsigned rg = pal_q_wave_sum(mine ? (q & 255u) | (((q >> 8) & 255u) << 16) : 0u);
        const unsigned ba = pal_q_wave_sum(mine ? ((q >> 16) & 255u) | ((q >> 24) << 16) : 0u);
        if (lane == leader) {
            atomicAdd(&acc[0][lk], (unsigned)__popcll(match));
            atomicAdd(&acc[1][lk], rg & 0xFFFFu);
            atomicAdd(&acc[2][lk], rg >> 16);
            atomicAdd(&acc[3][lk], ba & 0xFFFFu);
            atomicAdd(&acc[4][lk], ba >> 16);
        }
    }
    if (((todo | direct) >> lane) & 1ull) {
        atomicAdd(&acc[0][k], 1u);
        atomicAdd(&acc[1][k], q & 255u);
        atomicAdd(&acc[2][k], (q >> 8) & 255u);
        atomicAdd(&acc[3][k], (q >> 16) & 255u);
        atomicAdd(&acc[4][k], q >> 24);
    }
}

__global__ __launch_bounds__(PAL_THREADS) void palette_quantize_kernel(int HW, const float* __restrict__ img, int colours, int iterations,
                                                                       const int* __restrict__ init_palette, const int* __restrict__ init_sizes,
                                                                       int K, int* __restrict__ pal_out, int* __restrict__ sizes_out,
                                                                       int* __restrict__ iters_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pal_q_lds[];
    PalQuantScratch* s = (PalQuantScratch*)pal_q_lds;
    unsigned* keys = (unsigned*)(pal_q_lds + sizeof(PalQuantScratch));      // [HW]
    unsigned* far = keys + HW;                                               // [HW]
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int* row = pal_out + (long long)b * K * 4;
    // 0: quantise; the set stops taking keys once it holds more than `colours`
    pal_set_clear(&s->set);
    if (tid < 2) s->changed[tid] = 0;
    __syncthreads();
    for (int p = tid; p < HW; p += PAL_THREADS) {
        const unsigned key = pal_snap_quant(*(const float4*)(img + ((long long)b * HW + p) * 4));
        keys[p] = key;
        far[p] = 0xFFFFFFFFu;
        if (!*(volatile int*)&s->set.over) pal_set_insert(&s->set, key, colours);
    }
    __syncthreads();
    // 1: at most `colours` colours: they are the palette
    if (!s->set.over) {                                    // the whole workgroup
        const int n = pal_set_rows(&s->set, colours, K, row);
        if (tid == 0) {
            sizes_out[b] = n;
            if (iters_out) iters_out[b] = 0;
        }
        return;
    }
    // 2: starting slots
    int n0 = 0;
    if (init_palette) {
        n0 = init_sizes[b];
        n0 = n0 < 0 ? 0 : (n0 > K ? K : n0);
    }
    int n;
    if (n0 > 0) {                                          // the whole workgroup
        n = n0 < colours ? n0 : colours;
        for (int k = tid; k < n; k += PAL_THREADS) {
            const int4 c = *(const int4*)(init_palette + ((long long)b * K + k) * 4);
            s->slot[k] = pal_snap_slot(((unsigned)c.x & 255u) | (((unsigned)c.y & 255u) << 8) | (((unsigned)c.z & 255u) << 16) |
                                           (((unsigned)c.w & 255u) << 24), k);
        }
    } else {
        n = colours;
        unsigned c = 0u, cc = 0u;                          // the slot chosen last, in every lane's registers
        for (int j = 0; j < n; ++j) {
            unsigned long long best = 0ull;
            for (int p = tid; p < HW; p += PAL_THREADS) {
                const unsigned q = keys[p];
                unsigned m = far[p];
                if (j > 0) {
                    const unsigned d = __builtin_amdgcn_udot4(q, q, 0u, false) + cc - 2u * __builtin_amdgcn_udot4(q, c, 0u, false);
                    m = d < m ? d : m;
                    far[p] = m;
                }
                const unsigned long long cand = ((unsigned long long)m << 32) | (unsigned long long)(~q);
                best = cand > best ? cand : best;
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const unsigned long long other = __shfl_xor(best, o, 64);
                best = other > best ? other : best;
            }
            if (lane == 0) s->red[j & 1][wave] = best;
            __syncthreads();
#pragma unroll
            for (int w = 0; w < PAL_THREADS / 64; ++w) best = s->red[j & 1][w] > best ? s->red[j & 1][w] : best;
            c = ~(unsigned)best;
            cc = __builtin_amdgcn_udot4(c, c, 0u, false);
            if (tid == 0) s->slot[j] = pal_snap_slot(c, j);
        }
    }
    for (int k = tid; k < n; k += PAL_THREADS)
#pragma unroll
        for (int a = 0; a < 5; ++a) s->acc[a][k] = 0u;
    __syncthreads();
    // 3: Lloyd passes
    int iters = 0;
    for (int t = 1; t <= iterations; ++t) {
        for (int p0 = 0; p0 < HW; p0 += PAL_THREADS * PAL_SNAP_PIX) {
            unsigned q[PAL_SNAP_PIX], key[PAL_SNAP_PIX];
            bool valid[PAL_SNAP_PIX];
#pragma unroll
            for (int j = 0; j < PAL_SNAP_PIX; ++j) {
                const int p = p0 + j * PAL_THREADS + tid;
                valid[j] = p < HW;
                q[j] = valid[j] ? keys[p] : 0u;
                key[j] = 0xFFFFFFFFu;
            }
#pragma unroll 4
            for (int k = 0; k < n; ++k) {
                const uint2 sl = s->slot[k];               // wave-uniform address: one broadcast read for the lane's pixels
#pragma unroll
                for (int j = 0; j < PAL_SNAP_PIX; ++j) key[j] = pal_snap_min(key[j], q[j], sl);
            }
#pragma unroll
            for (int j = 0; j < PAL_SNAP_PIX; ++j) pal_q_add(s->acc, valid[j], key[j] & 255u, q[j]);
        }
        __syncthreads();
        if (tid < n) {                                     // n <= PAL_MAX = PAL_THREADS: one lane per slot
            const unsigned cnt = s->acc[0][tid];
            if (cnt) {                                     // floor((2 S + n_k) / (2 n_k)); a slot without pixels keeps its colour
                unsigned pk = 0u;
#pragma unroll
                for (int a = 0; a < 4; ++a) pk |= ((2u * s->acc[1 + a][tid] + cnt) / (2u * cnt)) << (8 * a);
                if (pk != s->slot[tid].x) {
                    s->slot[tid] = pal_snap_slot(pk, tid);
                    s->changed[t & 1] = 1;
                }
            }
#pragma unroll
            for (int a = 0; a < 5; ++a) s->acc[a][tid] = 0u;
        }
        if (tid == 0) s->changed[(t + 1) & 1] = 0;         // read by every lane before the barrier above, raised after the next one
        __syncthreads();
        iters = t;
        if (!s->changed[t & 1]) break;                     // the whole workgroup
    }
    // 4: the distinct colours of the slots in ascending key order
    unsigned key = 0u;
    if (tid < n) {
        key = s->slot[tid].x;
        unsigned f = 1u;
        for (int j = 0; j < tid; ++j) f = s->slot[j].x == key ? 0u : f;
        s->first[tid] = f;
    }
    __syncthreads();
    int size = 0, rank = 0;
    for (int j = 0; j < n; ++j) {
        const int f = (int)s->first[j];
        size += f;
        rank += (f && s->slot[j].x < key) ? 1 : 0;
    }
    if (tid < n && s->first[tid])
        *(int4*)(row + 4 * rank) = make_int4((int)(key & 255u), (int)((key >> 8) & 255u), (int)((key >> 16) & 255u), (int)(key >> 24));
    for (int i = size + tid; i < K; i += PAL_THREADS) *(int4*)(row + 4 * i) = make_int4(0, 0, 0, 0);
    if (tid == 0) {
        sizes_out[b] = size;
        if (iters_out) iters_out[b] = iters;
    }
}

// Differentiable palette projection (DESIGN.md "palette projection"): every pixel replaced by a colour of its image's palette, on the
// grid of the kernels above (a workgroup owns PAL_THREADS * PAL_PROJ_PIX consecutive pixels of one image).  Purely per pixel: no
// workspace, no atomics, no cross-lane traffic, so a pixel's bits depend on nothing but the pixel and its image's palette.
//   soft forward: y = 2 sum_k w_k c_k - 1 with the w of the soft histogram; sum_k w_k c_k is taken as c_r + E[c - c_r] about the
//                 nearest slot r (first index of min_k d), so a pixel on a palette colour returns that colour to rounding;
//   hard forward: the snap's packed key (pal_snap_* above) and nothing else: the bits of p2p_palette_snap's image_out;
//   backward:     dimg = (2 / tau) Cov_w(c) g at the raw image (the 0.5 of x = img 0.5 + 0.5 and the 2 of y cancel), the 4 x 4 covariance
//                 about r: E[(c - c_r)(c - c_r)^T] - E[c - c_r] E[c - c_r]^T.  About r the dominant slot's terms are exactly 0 and the
//                 rest is small times small, as in soft_palette_bwd_kernel; the covariance as written cancels to rounding in f32.
// An image without valid slots passes through: the forward copies img, the backward copies g, bit for bit.
#define PAL_PROJ_PIX 4

__global__ __launch_bounds__(PAL_THREADS) void palette_project_soft_kernel(int HW, const float* __restrict__ img, const int* __restrict__ palette,
                                                                           const int* __restrict__ sizes, int K, float nscale,
                                                                           float* __restrict__ out) {
    __shared__ float4 c[PAL_MAX];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = pal_load(palette, sizes, b, K, c);
    const long long base = (long long)b * HW;
    int pix[PAL_PROJ_PIX];
    bool valid[PAL_PROJ_PIX];
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        pix[j] = (blockIdx.x * PAL_PROJ_PIX + j) * PAL_THREADS + tid;
        valid[j] = pix[j] < HW;
    }
    if (n == 0) {                            // the whole workgroup
#pragma unroll
        for (int j = 0; j < PAL_PROJ_PIX; ++j)
            if (valid[j]) *(float4*)(out + (base + pix[j]) * 4) = *(const float4*)(img + (base + pix[j]) * 4);
        return;
    }
    float4 x[PAL_PROJ_PIX];
    float mn[PAL_PROJ_PIX];
    int r[PAL_PROJ_PIX];
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        x[j] = valid[j] ? pal_x(img, base + pix[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        mn[j] = INFINITY;
        r[j] = 0;
    }
    for (int k = 0; k < n; ++k) {
        const float4 ck = c[k];
#pragma unroll
        for (int j = 0; j < PAL_PROJ_PIX; ++j) {
            const float d = pal_dist(x[j], ck);
            if (d < mn[j]) { mn[j] = d; r[j] = k; }
        }
    }
    float4 cr[PAL_PROJ_PIX], Ec[PAL_PROJ_PIX];
    float S[PAL_PROJ_PIX];
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        cr[j] = c[r[j]];
        S[j] = 0.f;
        Ec[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int k = 0; k < n; ++k) {
        const float4 ck = c[k];
#pragma unroll
        for (int j = 0; j < PAL_PROJ_PIX; ++j) {
            const float e = __builtin_amdgcn_exp2f((pal_dist(x[j], ck) - mn[j]) * nscale);
            S[j] += e;
            Ec[j].x = __fmaf_rn(e, ck.x - cr[j].x, Ec[j].x); Ec[j].y = __fmaf_rn(e, ck.y - cr[j].y, Ec[j].y);
            Ec[j].z = __fmaf_rn(e, ck.z - cr[j].z, Ec[j].z); Ec[j].w = __fmaf_rn(e, ck.w - cr[j].w, Ec[j].w);
        }
    }
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        if (!valid[j]) continue;
        const float is = 1.f / S[j];                              // S >= 1: the nearest slot contributes exp2(0)
        *(float4*)(out + (base + pix[j]) * 4) =
            make_float4(__fmaf_rn(2.f, __fmaf_rn(Ec[j].x, is, cr[j].x), -1.f), __fmaf_rn(2.f, __fmaf_rn(Ec[j].y, is, cr[j].y), -1.f),
                        __fmaf_rn(2.f, __fmaf_rn(Ec[j].z, is, cr[j].z), -1.f), __fmaf_rn(2.f, __fmaf_rn(Ec[j].w, is, cr[j].w), -1.f));
    }
}

__global__ __launch_bounds__(PAL_THREADS) void palette_project_hard_kernel(int HW, const float* __restrict__ img, const int* __restrict__ palette,
                                                                           const int* __restrict__ sizes, int K, float* __restrict__ out) {
    __shared__ uint2 slot[PAL_MAX];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = pal_snap_load(palette, sizes, b, K, slot);
    __syncthreads();
    const long long base = (long long)b * HW;
    unsigned q[PAL_PROJ_PIX], key[PAL_PROJ_PIX];
    bool valid[PAL_PROJ_PIX];
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        const int p = (blockIdx.x * PAL_PROJ_PIX + j) * PAL_THREADS + tid;
        valid[j] = p < HW;
        q[j] = 0u;
        key[j] = 0xFFFFFFFFu;
        if (!valid[j]) continue;
        const float4 v = *(const float4*)(img + (base + p) * 4);
        if (n == 0) *(float4*)(out + (base + p) * 4) = v;
        q[j] = pal_snap_quant(v);
    }
    if (n == 0) return;                      // the whole workgroup
#pragma unroll 4
    for (int k = 0; k < n; ++k) {
        const uint2 s = slot[k];
#pragma unroll
        for (int j = 0; j < PAL_PROJ_PIX; ++j) key[j] = pal_snap_min(key[j], q[j], s);
    }
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        if (!valid[j]) continue;
        const int p = (blockIdx.x * PAL_PROJ_PIX + j) * PAL_THREADS + tid;
        *(float4*)(out + (base + p) * 4) = pal_snap_colour(slot[key[j] & 255u].x);
    }
}

// centred second moments of a pixel, the upper triangle of a symmetric 4 x 4 matrix
struct PalMoments { float xx, xy, xz, xw, yy, yz, yw, zz, zw, ww; };

__global__ __launch_bounds__(PAL_THREADS) void palette_project_bwd_kernel(int HW, const float* __restrict__ img, const int* __restrict__ palette,
                                                                          const int* __restrict__ sizes, int K, float nscale, float two_over_tau,
                                                                          const float* __restrict__ g, float* __restrict__ dimg) {
    __shared__ float4 c[PAL_MAX];
    const int b = blockIdx.y, tid = threadIdx.x;
    const int n = pal_load(palette, sizes, b, K, c);
    const long long base = (long long)b * HW;
    int pix[PAL_PROJ_PIX];
    bool valid[PAL_PROJ_PIX];
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        pix[j] = (blockIdx.x * PAL_PROJ_PIX + j) * PAL_THREADS + tid;
        valid[j] = pix[j] < HW;
    }
    if (n == 0) {                            // the whole workgroup: the forward was a copy
#pragma unroll
        for (int j = 0; j < PAL_PROJ_PIX; ++j)
            if (valid[j]) *(float4*)(dimg + (base + pix[j]) * 4) = *(const float4*)(g + (base + pix[j]) * 4);
        return;
    }
    float4 x[PAL_PROJ_PIX];
    float mn[PAL_PROJ_PIX];
    int r[PAL_PROJ_PIX];
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        x[j] = valid[j] ? pal_x(img, base + pix[j]) : make_float4(0.f, 0.f, 0.f, 0.f);
        mn[j] = INFINITY;
        r[j] = 0;
    }
    for (int k = 0; k < n; ++k) {
        const float4 ck = c[k];
#pragma unroll
        for (int j = 0; j < PAL_PROJ_PIX; ++j) {
            const float d = pal_dist(x[j], ck);
            if (d < mn[j]) { mn[j] = d; r[j] = k; }
        }
    }
    float4 cr[PAL_PROJ_PIX], m1[PAL_PROJ_PIX];
    PalMoments m2[PAL_PROJ_PIX];
    float S[PAL_PROJ_PIX];
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        cr[j] = c[r[j]];
        S[j] = 0.f;
        m1[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        m2[j] = PalMoments{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    }
    for (int k = 0; k < n; ++k) {
        const float4 ck = c[k];
#pragma unroll
        for (int j = 0; j < PAL_PROJ_PIX; ++j) {
            const float e = __builtin_amdgcn_exp2f((pal_dist(x[j], ck) - mn[j]) * nscale);
            const float cx = ck.x - cr[j].x, cy = ck.y - cr[j].y, cz = ck.z - cr[j].z, cw = ck.w - cr[j].w;
            const float ex = e * cx, ey = e * cy, ez = e * cz, ew = e * cw;
            S[j] += e;
            m1[j].x += ex; m1[j].y += ey; m1[j].z += ez; m1[j].w += ew;
            m2[j].xx = __fmaf_rn(ex, cx, m2[j].xx); m2[j].xy = __fmaf_rn(ex, cy, m2[j].xy); m2[j].xz = __fmaf_rn(ex, cz, m2[j].xz);
            m2[j].xw = __fmaf_rn(ex, cw, m2[j].xw); m2[j].yy = __fmaf_rn(ey, cy, m2[j].yy); m2[j].yz = __fmaf_rn(ey, cz, m2[j].yz);
            m2[j].yw = __fmaf_rn(ey, cw, m2[j].yw); m2[j].zz = __fmaf_rn(ez, cz, m2[j].zz); m2[j].zw = __fmaf_rn(ez, cw, m2[j].zw);
            m2[j].ww = __fmaf_rn(ew, cw, m2[j].ww);
        }
    }
#pragma unroll
    for (int j = 0; j < PAL_PROJ_PIX; ++j) {
        if (!valid[j]) continue;
        const float is = 1.f / S[j];
        const float ax = m1[j].x * is, ay = m1[j].y * is, az = m1[j].z * is, aw = m1[j].w * is;
        const PalMoments& m = m2[j];
        const float vxx = m.xx * is - ax * ax, vxy = m.xy * is - ax * ay, vxz = m.xz * is - ax * az, vxw = m.xw * is - ax * aw;
        const float vyy = m.yy * is - ay * ay, vyz = m.yz * is - ay * az, vyw = m.yw * is - ay * aw;
        const float vzz = m.zz * is - az * az, vzw = m.zw * is - az * aw, vww = m.ww * is - aw * aw;
        const float4 u = *(const float4*)(g + (base + pix[j]) * 4);
        *(float4*)(dimg + (base + pix[j]) * 4) =
            make_float4(two_over_tau * (vxx * u.x + vxy * u.y + vxz * u.z + vxw * u.w), two_over_tau * (vxy * u.x + vyy * u.y + vyz * u.z + vyw * u.w),
                        two_over_tau * (vxz * u.x + vyz * u.y + vzz * u.z + vzw * u.w), two_over_tau * (vxw * u.x + vyw * u.y + vzw * u.z + vww * u.w));
    }
}

static inline int pal_chunks(int H, int W, int per_lane) {
    const long long per = (long long)PAL_THREADS * per_lane;
    return (int)(((long long)H * W + per - 1) / per);
}

static int pal_check(const char* who, int N, int H, int W, const void* img, const void* palette, const void* sizes, int K, float tau) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && (long long)H * W <= (1LL << 30) && N <= 65535, "%s: bad shape %d x %d x %d (H * W <= 2^30, N <= 65535)", who, N, H, W);
    P2P_REQUIRE(K >= 1 && K <= PAL_MAX, "%s: K = %d, a palette has 1..%d slots", who, K, PAL_MAX);
    P2P_REQUIRE(tau >= 1e-30f && tau <= 3.0e38f, "%s: the temperature must be positive and finite (>= 1e-30)", who);
    P2P_REQUIRE(img && palette && sizes, "%s: null pointer", who);
    P2P_REQUIRE(((uintptr_t)img % 16) == 0 && ((uintptr_t)palette % 16) == 0, "%s: img and palette must be 16-byte aligned", who);
    return 0;
}

extern "C" long long p2p_soft_palette_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (long long)N * pal_chunks(H, W, PAL_FWD_PIX) * PAL_WS_STRIDE * (long long)sizeof(float);
}

extern "C" int p2p_soft_palette_fwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau,
                                    float* hist, float* conf, float* workspace, void* stream) {
    if (pal_check("p2p_soft_palette_fwd", N, H, W, img, palette, sizes, K, tau)) return -1;
    P2P_REQUIRE(hist && conf && workspace, "p2p_soft_palette_fwd: null pointer");
    const int chunks = pal_chunks(H, W, PAL_FWD_PIX);
    hipStream_t st = (hipStream_t)stream;
    const float nscale = (float)(-1.4426950408889634 / (double)tau);
    soft_palette_fwd_kernel<<<dim3(chunks, N), PAL_THREADS, 0, st>>>(H * W, img, palette, sizes, K, nscale, workspace);
    soft_palette_finish_kernel<<<N, PAL_THREADS, 0, st>>>(H * W, chunks, K, workspace, hist, conf);
    return p2p_check_launch("p2p_soft_palette_fwd");
}

extern "C" int p2p_soft_palette_bwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau,
                                    const float* gh, const float* gm, float* dimg, void* stream) {
    if (pal_check("p2p_soft_palette_bwd", N, H, W, img, palette, sizes, K, tau)) return -1;
    P2P_REQUIRE(gh && gm && dimg && ((uintptr_t)dimg % 16) == 0, "p2p_soft_palette_bwd: null or unaligned pointer");
    const float nscale = (float)(-1.4426950408889634 / (double)tau);
    soft_palette_bwd_kernel<false><<<dim3(pal_chunks(H, W, PAL_BWD_PIX), N), PAL_THREADS, 0, (hipStream_t)stream>>>(
        H * W, img, palette, sizes, K, nscale, (float)(2.0 / (double)tau), gh, gm, 0.f, 0.f, dimg);
    return p2p_check_launch("p2p_soft_palette_bwd");
}

extern "C" int p2p_soft_palette_tv_bwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau,
                                       const float* h_real, const float* h_fake, float w_tv, float w_conf, float* dimg, void* stream) {
    if (pal_check("p2p_soft_palette_tv_bwd", N, H, W, img, palette, sizes, K, tau)) return -1;
    P2P_REQUIRE(h_real && h_fake && dimg && ((uintptr_t)dimg % 16) == 0, "p2p_soft_palette_tv_bwd: null or unaligned pointer");
    const float nscale = (float)(-1.4426950408889634 / (double)tau);
    soft_palette_bwd_kernel<true><<<dim3(pal_chunks(H, W, PAL_BWD_PIX), N), PAL_THREADS, 0, (hipStream_t)stream>>>(
        H * W, img, palette, sizes, K, nscale, (float)(2.0 / (double)tau), h_fake, h_real, w_tv, w_conf, dimg);
    return p2p_check_launch("p2p_soft_palette_tv_bwd");
}

extern "C" int p2p_palette_loss(int B, int K, const float* h_real, const float* h_fake, const float* conf_fake, const int* sizes,
                                float inv_batch, float* out_tv, float* out_conf, void* stream) {
    P2P_REQUIRE(B > 0, "p2p_palette_loss: bad batch %d", B);
    P2P_REQUIRE(K >= 1 && K <= PAL_MAX, "p2p_palette_loss: K = %d, a palette has 1..%d slots", K, PAL_MAX);
    P2P_REQUIRE(h_real && h_fake && conf_fake && sizes && out_tv && out_conf, "p2p_palette_loss: null pointer");
    palette_loss_kernel<<<1, PAL_THREADS, 0, (hipStream_t)stream>>>(B, K, h_real, h_fake, conf_fake, sizes, inv_batch, out_tv, out_conf);
    return p2p_check_launch("p2p_palette_loss");
}

extern "C" int p2p_palette_snap(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, int* index_out,
                                float* image_out, int* dist_out, int* counts_out, long long* stats_out, void* stream) {
    if (pal_check("p2p_palette_snap", N, H, W, img, palette, sizes, K, 1.f)) return -1;
    P2P_REQUIRE(index_out && counts_out && stats_out, "p2p_palette_snap: null pointer");
    P2P_REQUIRE(((uintptr_t)image_out % 16) == 0, "p2p_palette_snap: image_out must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long long n_counts = (long long)N * K, n_stats = (long long)N * 2;
    const long long n_clear = n_counts > n_stats ? n_counts : n_stats;          // K = 1: more stats than counts
    palette_snap_clear_kernel<<<(int)((n_clear + PAL_THREADS - 1) / PAL_THREADS), PAL_THREADS, 0, st>>>(n_counts, counts_out, n_stats, stats_out);
    palette_snap_kernel<<<dim3(pal_chunks(H, W, PAL_SNAP_PIX), N), PAL_THREADS, 0, st>>>(H * W, img, palette, sizes, K, index_out, image_out,
                                                                                          dist_out, counts_out, stats_out);
    return p2p_check_launch("p2p_palette_snap");
}

extern "C" int p2p_palette_quantize(int N, int H, int W, const float* img, int colours, int iterations, const int* init_palette,
                                    const int* init_sizes, int K, int* palette_out, int* sizes_out, int* iters_out, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0, "p2p_palette_quantize: bad shape %d x %d x %d", N, H, W);
    P2P_REQUIRE((long long)H * W <= PAL_Q_MAXPIX, "p2p_palette_quantize: %d x %d pixels, an image has at most 2^14 (128 x 128): its keys stay in LDS",
                H, W);
    P2P_REQUIRE(K >= 1 && K <= PAL_MAX, "p2p_palette_quantize: K = %d, a palette has 1..%d slots", K, PAL_MAX);
    P2P_REQUIRE(colours >= 1 && colours <= K, "p2p_palette_quantize: colours = %d, expected 1..K = %d", colours, K);
    P2P_REQUIRE(iterations >= 0 && iterations <= 64, "p2p_palette_quantize: iterations = %d, expected 0..64", iterations);
    P2P_REQUIRE((init_palette == nullptr) == (init_sizes == nullptr), "p2p_palette_quantize: init_palette and init_sizes are given together or not at all");
    P2P_REQUIRE(img && palette_out && sizes_out, "p2p_palette_quantize: null pointer");
    P2P_REQUIRE(((uintptr_t)img % 16) == 0 && ((uintptr_t)palette_out % 16) == 0 && ((uintptr_t)init_palette % 16) == 0,
                "p2p_palette_quantize: img, palette_out and init_palette must be 16-byte aligned");
    const int lds = (int)sizeof(PalQuantScratch) + 8 * H * W;
    static bool attr_done = false;
    if (!attr_done) attr_done = p2p_allow_lds((const void*)palette_quantize_kernel, 160 * 1024, "palette_quantize_kernel");
    palette_quantize_kernel<<<N, PAL_THREADS, lds, (hipStream_t)stream>>>(H * W, img, colours, iterations, init_palette, init_sizes, K, palette_out,
                                                                          sizes_out, iters_out);
    return p2p_check_launch("p2p_palette_quantize");
}

extern "C" int p2p_palette_project_fwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau, int hard,
                                       float* out, void* stream) {
    if (pal_check("p2p_palette_project_fwd", N, H, W, img, palette, sizes, K, tau)) return -1;
    P2P_REQUIRE(hard == 0 || hard == 1, "p2p_palette_project_fwd: hard = %d, expected 0 (soft) or 1 (snap)", hard);
    P2P_REQUIRE(out && ((uintptr_t)out % 16) == 0, "p2p_palette_project_fwd: out is a null pointer or not 16-byte aligned");
    const dim3 grid(pal_chunks(H, W, PAL_PROJ_PIX), N);
    hipStream_t st = (hipStream_t)stream;
    if (hard) palette_project_hard_kernel<<<grid, PAL_THREADS, 0, st>>>(H * W, img, palette, sizes, K, out);
    else palette_project_soft_kernel<<<grid, PAL_THREADS, 0, st>>>(H * W, img, palette, sizes, K, (float)(-1.4426950408889634 / (double)tau), out);
    return p2p_check_launch("p2p_palette_project_fwd");
}

extern "C" int p2p_palette_project_bwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau,
                                       const float* g, float* dimg, void* stream) {
    if (pal_check("p2p_palette_project_bwd", N, H, W, img, palette, sizes, K, tau)) return -1;
    P2P_REQUIRE(g && dimg && ((uintptr_t)g % 16) == 0 && ((uintptr_t)dimg % 16) == 0,
                "p2p_palette_project_bwd: g or dimg is a null pointer or not 16-byte aligned");
    palette_project_bwd_kernel<<<dim3(pal_chunks(H, W, PAL_PROJ_PIX), N), PAL_THREADS, 0, (hipStream_t)stream>>>(
        H * W, img, palette, sizes, K, (float)(-1.4426950408889634 / (double)tau), (float)(2.0 / (double)tau), g, dimg);
    return p2p_check_launch("p2p_palette_project_bwd");
}

extern "C" int p2p_palette_extract(int N, int H, int W, const float* img, int cap, int* palette_out, int* sizes_out, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && (long long)H * W <= (1LL << 30), "p2p_palette_extract: bad shape %d x %d x %d", N, H, W);
    P2P_REQUIRE(cap >= 1 && cap <= PAL_MAX, "p2p_palette_extract: cap = %d, a palette has 1..%d slots", cap, PAL_MAX);
    P2P_REQUIRE(img && palette_out && sizes_out && ((uintptr_t)img % 16) == 0 && ((uintptr_t)palette_out % 16) == 0,
                "p2p_palette_extract: null or unaligned pointer");
    palette_extract_kernel<<<N, PAL_THREADS, 0, (hipStream_t)stream>>>(H * W, img, cap, palette_out, sizes_out);
    return p2p_check_launch("p2p_palette_extract");
}
