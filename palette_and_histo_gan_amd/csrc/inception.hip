// InceptionV3 (Keras, include_top=False, pooling="avg", inference) behind the FID evaluation (reference
// frechet_inception_distance.py): the resize + preprocess_input of the images, the 94 Conv2D + BatchNorm(scale=False) + ReLU
// blocks as exact-f32 MFMA implicit GEMMs, the two pooling forms and the global average.  Everything f32 in / f32 accumulate,
// every sum in a fixed order (no float atomics): a second launch is bit-identical.  The layer table and the launch sequence are
// in palette_and_histo_gan_amd/inception.py.
#include "p2p_common.hpp"

// ---- resize (scikit-image 0.19 resize(order=0)) + preprocess_input ("tf" mode) ---------------------------------------------

// mm[2n] / mm[2n+1] = min / max of image n (the clip bounds resize takes from its input); min and max are exact in any order
__global__ __launch_bounds__(256) void inc_minmax_kernel(const float* __restrict__ img, long long per_image, float* __restrict__ mm) {
    __shared__ float lo_s[4], hi_s[4];
    const float* p = img + (long long)blockIdx.x * per_image;
    float lo = INFINITY, hi = -INFINITY;
    for (long long i = threadIdx.x; i < per_image; i += blockDim.x) {
        const float v = p[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    if ((threadIdx.x & 63) == 0) { lo_s[threadIdx.x >> 6] = lo; hi_s[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { lo = fminf(lo_s[0], lo_s[w]); hi = fmaxf(hi_s[0], hi_s[w]); lo_s[0] = lo; hi_s[0] = hi; }
        mm[2 * blockIdx.x] = lo_s[0];
        mm[2 * blockIdx.x + 1] = hi_s[0];
    }
}

// One output pixel per thread.  With `filter` the channel axis first goes through scipy.ndimage.gaussian_filter (3 taps, mode
// "mirror"), evaluated as scipy's symmetric correlate1d does it in f64 -- x[c] w0 + (x[c-1] + x[c+1]) w1, no fused multiply-add --
// and stored as f32.  Then the nearest-neighbour pick through the host's index tables (scipy.ndimage.zoom of an index ramp), the
// clip to the image's [min, max], and x / 127.5 - 1 as two f32 operations.
__global__ __launch_bounds__(256) void inc_prep_kernel(int N, int H, int W, int C, const float* __restrict__ img,
                                                       const int* __restrict__ rows, const int* __restrict__ cols,
                                                       const int* __restrict__ chans, int OH, int OW, double w0, double w1,
                                                       int filter, const float* __restrict__ mm, TView out) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= (long long)N * OH * OW) return;
    const int ox = (int)(m % OW);
    const long long t = m / OW;
    const int oy = (int)(t % OH);
    const int n = (int)(t / OH);
    const float* px = img + (((long long)n * H + rows[oy]) * W + cols[ox]) * C;
    const float lo = mm[2 * n], hi = mm[2 * n + 1];
    float* o = (float*)out.ptr + out.off(n, oy, ox);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int c = chans[q];
        float v;
        if (filter) {
            const int l = c > 0 ? c - 1 : 1, r = c < C - 1 ? c + 1 : C - 2;      // "mirror": -1 -> 1, C -> C - 2
            double s = __dmul_rn((double)px[c], w0);
            s = __dadd_rn(s, __dmul_rn(__dadd_rn((double)px[l], (double)px[r]), w1));
            v = (float)s;
        } else {
            v = px[c];
        }
        v = fminf(fmaxf(v, lo), hi);
        v = __fdiv_rn(v, 127.5f);
        o[q] = __fsub_rn(v, 1.0f);
    }
}

extern "C" int p2p_inc_prep(int N, int H, int W, int C, const float* images, const int* rows, const int* cols, const int* chans,
                            int OH, int OW, double w0, double w1, int filter, const p2p_tensor* out, float* minmax, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && OH > 0 && OW > 0 && (C == 3 || C == 4), "p2p_inc_prep: bad shape N=%d H=%d W=%d C=%d -> %dx%d",
                N, H, W, C, OH, OW);
    P2P_REQUIRE(C == 4 || !filter, "p2p_inc_prep: the channel filter needs 4 input channels");
    P2P_REQUIRE(images && rows && cols && chans && out && out->ptr && minmax, "p2p_inc_prep: null pointer");
    P2P_REQUIRE(out->ld >= 3, "p2p_inc_prep: output view needs 3 channels, ld = %d", out->ld);
    hipStream_t st = (hipStream_t)stream;
    inc_minmax_kernel<<<N, 256, 0, st>>>(images, (long long)H * W * C, minmax);
    const long long M = (long long)N * OH * OW;
    inc_prep_kernel<<<dim3((unsigned)((M + 255) / 256)), 256, 0, st>>>(N, H, W, C, images, rows, cols, chans, OH, OW, w0, w1, filter,
                                                                       minmax, make_view(out));
    return p2p_check_launch("p2p_inc_prep");
}

// ---- Conv2D (no bias) + BatchNorm(scale=False, inference) + ReLU: implicit GEMM on v_mfma_f32_32x32x2_f32 -------------------
// C[m][co] = sum_k A[m][k] W[k][co], m = (n, oy, ox), k = (ky, kx, ci) with ci fastest (the HWIO kernel flattened row-major),
// A[m][k] = in[n, oy s - pt + ky, ox s - pl + kx, ci] or 0 outside the image (predicated loads: inputs carry no halo).
// Epilogue relu(acc * scale[co] + shift[co]) into a channel slice of the output view.  Block tile (32 WM) x (32 WN), one 32x32
// accumulator per wave (WM x WN = 4 waves), K in blocks of 16 staged through LDS with the next block's loads in flight during the
// MFMAs.  Each output is one k-ordered f32 fma chain: bit-reproducible.
struct IncConvArgs {
    int N, H, W, Cin, kh, kw, stride, pt, pl, OH, OW, Cout, K, M;
    TView in;
    const float* w;
    const float* scale;
    const float* shift;
    TView out;
};

constexpr int INC_BK = 16;

template <int WM, int WN, bool VEC>
__global__ __launch_bounds__(256) void inc_conv_kernel(IncConvArgs a) {
    constexpr int BM = 32 * WM, BN = 32 * WN;
    constexpr int APAD = 4;
    constexpr int A_VEC = BM / 64;                 // float4 pieces of A per thread (VEC): BM rows x 4 pieces / 256 threads
    constexpr int A_SCL = BM * INC_BK / 256;        // scalars of A per thread (generic gather)
    constexpr int B_PIECES = INC_BK * BN / 4;       // float4 pieces of B per block
    __shared__ float As[INC_BK][BM + APAD];
    __shared__ float Bs[INC_BK][BN];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const float* in = (const float*)a.in.ptr;

    // the A rows this thread loads: VEC: rows (tid >> 2) + 64 i, piece tid & 3; generic: row tid % BM, k slots tid / BM + (256 / BM) j
    constexpr int ROWS = VEC ? A_VEC : 1;
    int rn[ROWS], ry[ROWS], rx[ROWS];
    bool rv[ROWS];
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        const int r = VEC ? (tid >> 2) + 64 * i : tid % BM;
        const int m = m0 + r;
        rv[i] = m < a.M;
        const int mm = rv[i] ? m : 0;
        const int ox = mm % a.OW, t = mm / a.OW;
        const int oy = t % a.OH;
        rn[i] = t / a.OH;
        ry[i] = oy * a.stride - a.pt;
        rx[i] = ox * a.stride - a.pl;
    }

    f32x4 ra[VEC ? A_VEC : 1];
    float rs[VEC ? 1 : A_SCL];
    f32x4 rb;
    const int bp_row = tid / (BN / 4), bp_col = (tid % (BN / 4)) * 4;

    auto load = [&](int kb) {
        const int k0 = kb * INC_BK;
        if constexpr (VEC) {
            const int tap = k0 / a.Cin, ci = k0 - tap * a.Cin;
            const int ky = tap / a.kw, kx = tap - ky * a.kw;
#pragma unroll
            for (int i = 0; i < A_VEC; ++i) {
                const int iy = ry[i] + ky, ix = rx[i] + kx;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (rv[i] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    v = *(const f32x4*)(in + a.in.off(rn[i], iy, ix) + ci + (tid & 3) * 4);
                ra[i] = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < A_SCL; ++j) {
                const int k = k0 + tid / BM + (256 / BM) * j;
                float v = 0.f;
                if (rv[0] && k < a.K) {
                    const int tap = k / a.Cin, ci = k - tap * a.Cin;
                    const int ky = tap / a.kw, kx = tap - ky * a.kw;
                    const int iy = ry[0] + ky, ix = rx[0] + kx;
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = in[a.in.off(rn[0], iy, ix) + ci];
                }
                rs[j] = v;
            }
        }
        if (tid < B_PIECES) {
            const int k = k0 + bp_row, co = n0 + bp_col;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k < a.K && co < a.Cout) v = *(const f32x4*)(a.w + (long long)k * a.Cout + co);
            rb = v;
        }
    };
    auto stash = [&]() {
        if constexpr (VEC) {
#pragma unroll
            for (int i = 0; i < A_VEC; ++i) {
                const int r = (tid >> 2) + 64 * i, kq = (tid & 3) * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) As[kq + e][r] = ra[i][e];
            }
        } else {
#pragma unroll
            for (int j = 0; j < A_SCL; ++j) As[tid / BM + (256 / BM) * j][tid % BM] = rs[j];
        }
        if (tid < B_PIECES) *(f32x4*)&Bs[bp_row][bp_col] = rb;
    };

    f32x16 acc;
    const float z = p2p_valu_zero();
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = z;

    const int nkb = (a.K + INC_BK - 1) / INC_BK;
    const int ar = wm * 32 + (lane & 31), bc = wn * 32 + (lane & 31), kh = lane >> 5;
    load(0);
    for (int kb = 0; kb < nkb; ++kb) {
        __syncthreads();
        stash();
        __syncthreads();
        if (kb + 1 < nkb) load(kb + 1);
#pragma unroll
        for (int kk = 0; kk < INC_BK; kk += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + kh][ar], Bs[kk + kh][bc], acc, 0, 0, 0);
    }

    // C/D map of the 32x32 tile: column lane & 31, row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int co = n0 + bc;
    if (co >= a.Cout) return;
    const float sc = a.scale[co], sh = a.shift[co];
    float* out = (float*)a.out.ptr;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (m >= a.M) continue;
        const int ox = m % a.OW, t = m / a.OW;
        const int oy = t % a.OH, n = t / a.OH;
        out[a.out.off(n, oy, ox) + co] = fmaxf(fmaf(acc[r], sc, sh), 0.f);
    }
}

extern "C" int p2p_inc_conv(int N, int H, int W, int Cin, int kh, int kw, int stride, int pad_top, int pad_left, int OH, int OW,
                            int Cout, const p2p_tensor* in, const float* w, const float* scale, const float* shift,
                            const p2p_tensor* out, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && kh > 0 && kw > 0 && stride > 0 && OH > 0 && OW > 0 && Cout > 0,
                "p2p_inc_conv: bad shape N=%d %dx%dx%d k=%dx%d/%d -> %dx%dx%d", N, H, W, Cin, kh, kw, stride, OH, OW, Cout);
    // every gather is predicated on the image bounds, so any padding / output size reads inside the input view
    P2P_REQUIRE(pad_top >= 0 && pad_left >= 0 && (long long)N * OH * OW < (1LL << 31) && (long long)kh * kw * Cin < (1LL << 31),
                "p2p_inc_conv: bad geometry (pads %d, %d)", pad_top, pad_left);
    P2P_REQUIRE(in && in->ptr && out && out->ptr && w && scale && shift, "p2p_inc_conv: null pointer");
    P2P_REQUIRE(in->ld >= Cin && out->ld >= Cout, "p2p_inc_conv: view ld smaller than the channel count (in %d < %d or out %d < %d)",
                in->ld, Cin, out->ld, Cout);
    P2P_REQUIRE(Cout % 4 == 0 && ((uintptr_t)w % 16) == 0, "p2p_inc_conv: weights must be 16-byte aligned rows (Cout %% 4 == 0)");
    IncConvArgs a;
    a.N = N; a.H = H; a.W = W; a.Cin = Cin; a.kh = kh; a.kw = kw; a.stride = stride; a.pt = pad_top; a.pl = pad_left;
    a.OH = OH; a.OW = OW; a.Cout = Cout; a.K = kh * kw * Cin; a.M = N * OH * OW;
    a.in = make_view(in); a.w = w; a.scale = scale; a.shift = shift; a.out = make_view(out);
    // float4 gathers when every 16-wide K block lies inside one tap and starts 16-byte aligned
    const bool vec = Cin % INC_BK == 0 && in->ld % 4 == 0 && ((uintptr_t)in->ptr % 16) == 0;
    hipStream_t st = (hipStream_t)stream;
    const bool wide = Cout % 64 == 0;       // 64 x 64 tiles; otherwise 128 x 32 (Cout = 32, 48, 80, 96, 160 waste less)
    const unsigned gm = (unsigned)((a.M + (wide ? 63 : 127)) / (wide ? 64 : 128));
    const unsigned gn = (unsigned)((Cout + (wide ? 63 : 31)) / (wide ? 64 : 32));
    if (wide) {
        if (vec) inc_conv_kernel<2, 2, true><<<dim3(gm, gn), 256, 0, st>>>(a);
        else inc_conv_kernel<2, 2, false><<<dim3(gm, gn), 256, 0, st>>>(a);
    } else {
        if (vec) inc_conv_kernel<4, 1, true><<<dim3(gm, gn), 256, 0, st>>>(a);
        else inc_conv_kernel<4, 1, false><<<dim3(gm, gn), 256, 0, st>>>(a);
    }
    return p2p_check_launch("p2p_inc_conv");
}

// ---- pooling --------------------------------------------------------------------------------------------------------------
// kind 0: MaxPooling2D 3x3 / 2 "valid"; kind 1: AveragePooling2D 3x3 / 1 "same" (TF divides by the number of taps inside the
// image), taps summed row by row.  One output element per thread.
__global__ __launch_bounds__(256) void inc_pool_kernel(int kind, int N, int H, int W, int C, int OH, int OW, TView in, TView out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)N * OH * OW * C) return;
    const int c = (int)(e % C);
    long long t = e / C;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH), n = (int)(t / OH);
    const float* p = (const float*)in.ptr;
    float v;
    if (kind == 0) {
        v = -INFINITY;
        for (int dy = 0; dy < 3; ++dy)
            for (int dx = 0; dx < 3; ++dx) v = fmaxf(v, p[in.off(n, 2 * oy + dy, 2 * ox + dx) + c]);
    } else {
        float s = 0.f;
        int cnt = 0;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int y = oy + dy, x = ox + dx;
                if (y < 0 || y >= H || x < 0 || x >= W) continue;
                s += p[in.off(n, y, x) + c];
                ++cnt;
            }
        v = s / (float)cnt;
    }
    ((float*)out.ptr)[out.off(n, oy, ox) + c] = v;
}

extern "C" int p2p_inc_pool(int kind, int N, int H, int W, int C, const p2p_tensor* in, const p2p_tensor* out, void* stream) {
    P2P_REQUIRE(kind == 0 || kind == 1, "p2p_inc_pool: kind %d (0 = max 3x3/2 valid, 1 = average 3x3/1 same)", kind);
    P2P_REQUIRE(N > 0 && C > 0 && H > 0 && W > 0 && (kind == 1 || (H >= 3 && W >= 3)), "p2p_inc_pool: bad shape N=%d %dx%dx%d (kind %d)",
                N, H, W, C, kind);
    P2P_REQUIRE(in && in->ptr && out && out->ptr && in->ld >= C && out->ld >= C, "p2p_inc_pool: bad views");
    const int OH = kind == 0 ? (H - 3) / 2 + 1 : H, OW = kind == 0 ? (W - 3) / 2 + 1 : W;
    const long long total = (long long)N * OH * OW * C;
    inc_pool_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, (hipStream_t)stream>>>(kind, N, H, W, C, OH, OW, make_view(in),
                                                                                            make_view(out));
    return p2p_check_launch("p2p_inc_pool");
}

// GlobalAveragePooling2D: out[n][c] = (sum over the map, row by row) / (H W); one thread per (n, c)
__global__ __launch_bounds__(256) void inc_gap_kernel(int N, int H, int W, int C, TView in, float* __restrict__ out) {
    const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= (long long)N * C) return;
    const int c = (int)(e % C), n = (int)(e / C);
    const float* p = (const float*)in.ptr;
    float s = 0.f;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) s += p[in.off(n, y, x) + c];
    out[e] = s / (float)(H * W);
}

extern "C" int p2p_inc_gap(int N, int H, int W, int C, const p2p_tensor* in, float* out, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, "p2p_inc_gap: bad shape N=%d %dx%dx%d", N, H, W, C);
    P2P_REQUIRE(in && in->ptr && in->ld >= C && out, "p2p_inc_gap: bad arguments");
    const long long total = (long long)N * C;
    inc_gap_kernel<<<dim3((unsigned)((total + 255) / 256)), 256, 0, (hipStream_t)stream>>>(N, H, W, C, make_view(in), out);
    return p2p_check_launch("p2p_inc_gap");
}
