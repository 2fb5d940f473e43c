// Keras Adam over the flat parameter buffer, weight-copy preparation and batch packing.
// Reference: tf.keras.optimizers.Adam(0.0002, beta_1=0.5) applied at pix2pix_model.py:28-29,81-83
// (OptimizerV2 formulation: eps added to sqrt(v) outside the bias correction);
// batch value contract dataset_utils.py:39-48,209-246.
#include "p2p_common.hpp"
#include <math.h>
#include <stdlib.h>

__global__ void adam_flat_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                 float* __restrict__ v, long long n, float lr_t, float b1, float b2, float eps,
                                 float gscale) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        float gi = g[i] * gscale;
        float mi = b1 * m[i] + (1.f - b1) * gi;
        float vi = b2 * v[i] + (1.f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        p[i] = p[i] - lr_t * mi / (sqrtf(vi) + eps);
    }
}

extern "C" int p2p_adam_flat(float* p, const float* g, float* m, float* v, long long n, int t, float lr, float beta1,
                             float beta2, float eps, float gscale, void* stream) {
    P2P_REQUIRE(p && g && m && v && n > 0 && t >= 1, "p2p_adam_flat: bad args");
    double lr_t = (double)lr * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t));
    long long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    adam_flat_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(p, g, m, v, n, (float)lr_t, beta1, beta2,
                                                                             eps, gscale);
    return p2p_check_launch("p2p_adam_flat");
}

// Device-resident step state, so that a whole train step can be captured once in a hipGraph and replayed: the Adam
// iteration count / bias-corrected step size and the dropout counter live in HBM and are advanced by these kernels.
__global__ void adam_tick_kernel(int* __restrict__ t, float* __restrict__ lr_t, float lr, float b1, float b2) {
    int tt = t[0] + 1;
    t[0] = tt;
    lr_t[0] = (float)((double)lr * sqrt(1.0 - pow((double)b2, (double)tt)) / (1.0 - pow((double)b1, (double)tt)));
}

// One element of the Keras Adam step with its roundings spelled out: m' = fma(1 - b1, g, b1 * m), v' = fma(b2, v, ((1 - b2) * g) * g).
// That is what the compiler's contraction made of the vector loop of the first flat kernel; left to the compiler, a scalar copy of
// the same expressions (a tail, a vector cut by an excluded range) came out with other fusions and other last bits.  Every path
// of adam_kernel goes through here, so the five entry points it serves agree bit for bit by construction.
__device__ __forceinline__ void adam_update(float& p, float g, float& m, float& v, float lr_t, float b1, float b2, float eps,
                                            float gscale) {
#pragma clang fp contract(off)
    const float gg = g * gscale;
    m = __builtin_fmaf(1.f - b1, gg, b1 * m);
    v = __builtin_fmaf(b2, v, ((1.f - b2) * gg) * gg);
    p = p - lr_t * m / (sqrtf(v) + eps);
}

// Exponential moving average of the generator's masters: e' = e + (1 - beta_t) * (p' - e) with
// beta_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay and t = the Adam iteration p2p_adam_tick left in t_dev.  Three correctly
// rounded f32 operations per element and no contraction: a NumPy float32 restatement gives the same bits, and p' == e leaves e
// as it is.  Every path of the two kernels that average (vector body, straddling vectors, tails) goes through here.
struct EmaArgs { float* e; const int* t_dev; float decay; int warmup; };

__device__ __forceinline__ float ema_one_minus_beta(const EmaArgs& a) {
#pragma clang fp contract(off)
    float beta = a.decay;
    if (a.warmup) {
        const float t = (float)a.t_dev[0];
        beta = fminf(a.decay, __fdiv_rn(1.f + t, 10.f + t));
    }
    return 1.f - beta;
}

__device__ __forceinline__ void ema_update(float& e, float p, float omb) {
#pragma clang fp contract(off)
    const float d = p - e;
    const float s = omb * d;
    e = e + s;
}

// The gradient options of p2p_adam_step, in front of adam_update: the clamp first, then the device scale.
// Both are exact no-ops when off (g * 1.0f == g).
struct GradOpts { const float* gscale_dev; float clipvalue; };

__device__ __forceinline__ float grad_clamp(float g, float c) { return c > 0.f ? fminf(fmaxf(g, -c), c) : g; }

// What one launch holds fixed for every element.
struct AdamCoef { float lr_t, b1, b2, eps, gscale, clip, omb; };

// The live element j, and the whole 16-byte vector at i: the only two places of the flat pass that touch an element.
template <bool EMA, bool OPTS>
__device__ __forceinline__ void adam_element(float* p, const float* g, float* m, float* v, float* e, long long j,
                                             const AdamCoef& c) {
    adam_update(p[j], OPTS ? grad_clamp(g[j], c.clip) : g[j], m[j], v[j], c.lr_t, c.b1, c.b2, c.eps, c.gscale);
    if constexpr (EMA) ema_update(e[j], p[j], c.omb);
}

template <bool EMA, bool OPTS>
__device__ __forceinline__ void adam_vector(float* p, const float* g, float* m, float* v, float* e, long long i,
                                            const AdamCoef& c) {
    f32x4 gi = *(const f32x4*)(g + i), mi = *(const f32x4*)(m + i), vi = *(const f32x4*)(v + i), pi = *(const f32x4*)(p + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float pk = pi[k], mk = mi[k], vk = vi[k];
        adam_update(pk, OPTS ? grad_clamp(gi[k], c.clip) : gi[k], mk, vk, c.lr_t, c.b1, c.b2, c.eps, c.gscale);
        pi[k] = pk; mi[k] = mk; vi[k] = vk;
    }
    *(f32x4*)(m + i) = mi; *(f32x4*)(v + i) = vi; *(f32x4*)(p + i) = pi;
    if constexpr (EMA) {
        f32x4 ei = *(const f32x4*)(e + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float ek = ei[k];
            ema_update(ek, pi[k], c.omb);
            ei[k] = ek;
        }
        *(f32x4*)(e + i) = ei;
    }
}

// The flat Adam pass behind p2p_adam_flat_dev, _excl, p2p_adam_ema_flat_dev, _excl and p2p_adam_step.
//   HOLE  elements [ex_lo, ex_hi) are neither read nor written.  The 16-byte vectors that lie wholly inside the hole are taken out
//         of the index space (every lane keeps a whole share of live vectors); a vector that straddles an end of the hole is
//         updated element by element.  HOLE = false is the plain index space and its register footprint: the early Adam over
//         the generator's head buckets runs beside the weight-gradient stream's last kernels and must leave them room.
//   EMA   the moving average of the live elements in the same pass (e has the hole too): the fresh p is still in registers, so
//         the average costs one read and one write of e (8 bytes per element) and no launch.
//   OPTS  the gradient options, read from `o`; without them `gscale` is the by-value scale of the flat entry points and no
//         instruction of the options is compiled in (the option-carrying form costs the batch-256 step
//         time that its arithmetic does not explain, so the default step does not run it).
template <bool EMA, bool HOLE, bool OPTS>
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            long long n, long long ex_lo, long long ex_hi, const float* __restrict__ lr_t_dev, float b1, float b2,
                            float eps, float gscale, GradOpts o, EmaArgs ema) {
    AdamCoef c = {lr_t_dev[0], b1, b2, eps, gscale, 0.f, 0.f};
    if constexpr (OPTS) {
        c.gscale = o.gscale_dev ? o.gscale_dev[0] : 1.0f;
        c.clip = o.clipvalue;
    }
    if constexpr (EMA) c.omb = ema_one_minus_beta(ema);
    const long long hv_lo = HOLE ? (ex_lo + 3) / 4 : 0, hv_hi = HOLE ? ex_hi / 4 : 0;
    const long long hole = hv_hi > hv_lo ? hv_hi - hv_lo : 0;
    const long long live = n / 4 - hole;
    long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    if constexpr (!HOLE && !OPTS) {
        // the vectors the loop below visits with an empty hole.  The default step runs this form beside the weight-gradient
        // stream, and its timings were taken with this loop's code: kept apart from the optioned one
        for (long long i = q * 4; i + 3 < n; i += stride * 4) adam_vector<EMA, OPTS>(p, g, m, v, ema.e, i, c);
    } else {
        for (; q < live; q += stride) {
            const long long i = (!HOLE || q < hv_lo ? q : q + hole) * 4;
            if (!HOLE || i + 4 <= ex_lo || i >= ex_hi) adam_vector<EMA, OPTS>(p, g, m, v, ema.e, i, c);
            else
                for (long long j = i; j < i + 4; ++j)
                    if (j < ex_lo || j >= ex_hi) adam_element<EMA, OPTS>(p, g, m, v, ema.e, j, c);
        }
    }
    // tail (n is padded to a multiple of 4 by the host layout, kept for safety)
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long j = n / 4 * 4; j < n; ++j)
            if (!HOLE || j < ex_lo || j >= ex_hi) adam_element<EMA, OPTS>(p, g, m, v, ema.e, j, c);
}

// Grid of a pass in which thread q takes the 16-byte vectors q, q + grid * 256, ...: one thread per vector up to 8192 workgroups.
static inline dim3 vector_grid(long long nvec) {
    const long long blocks = (nvec + 255) / 256;
    return dim3((unsigned)(blocks > 8192 ? 8192 : blocks < 1 ? 1 : blocks));
}

template <typename... P>
static inline bool aligned16(const P*... ptrs) {
    return ((((uintptr_t)ptrs) | ...) % 16) == 0;
}

// Every check, the grid and the choice of instantiation for the five entry points; `who` names the one that was called.
// `gscale` is the by-value scale of the four flat entry points.  OPTS only where an option is on: p2p_adam_step with both off
// runs the code of the flat entry points.
static int adam_launch(const p2p_adam_args& a, const p2p_adam_hyper& h, float gscale, bool ema, const char* who, void* stream) {
    P2P_REQUIRE(a.p && a.g && a.m && a.v && a.n > 0 && a.lr_t_dev, "%s: bad args", who);
    P2P_REQUIRE(!ema || (a.e && a.t_dev), "%s: the moving average needs e and t_dev", who);
    P2P_REQUIRE(0 <= a.ex_lo && a.ex_lo <= a.ex_hi && a.ex_hi <= a.n, "%s: the excluded range must lie inside [0, n)", who);
    P2P_REQUIRE(aligned16(a.p, a.g, a.m, a.v, a.e), "%s: buffers must be 16-byte aligned", who);
    const long long hv_lo = (a.ex_lo + 3) / 4, hv_hi = a.ex_hi / 4;
    const long long live = a.n / 4 - (hv_hi > hv_lo ? hv_hi - hv_lo : 0);
    const dim3 grid = vector_grid(live);
    const GradOpts o = {a.gscale_dev, h.clipvalue};
    const EmaArgs avg = ema ? EmaArgs{a.e, a.t_dev, h.ema_decay, a.ema_warmup} : EmaArgs{nullptr, nullptr, 0.f, 0};
    const bool hole = a.ex_hi > a.ex_lo, opts = a.gscale_dev || h.clipvalue > 0.f;
#define ADAM_CASE(EMA, HOLE, OPTS)                                                                                                \
    if (ema == EMA && hole == HOLE && opts == OPTS)                                                                                \
        adam_kernel<EMA, HOLE, OPTS><<<grid, 256, 0, (hipStream_t)stream>>>(a.p, a.g, a.m, a.v, a.n, a.ex_lo, a.ex_hi, a.lr_t_dev, \
                                                                          h.beta1, h.beta2, h.eps, gscale, o, avg)
    ADAM_CASE(false, false, false); ADAM_CASE(true, false, false); ADAM_CASE(false, true, false); ADAM_CASE(true, true, false);
    ADAM_CASE(false, false, true);  ADAM_CASE(true, false, true);  ADAM_CASE(false, true, true);  ADAM_CASE(true, true, true);
#undef ADAM_CASE
    return p2p_check_launch(who);
}

extern "C" int p2p_adam_tick(int* t_dev, float* lr_t_dev, float lr, float beta1, float beta2, void* stream) {
    P2P_REQUIRE(t_dev && lr_t_dev, "p2p_adam_tick: null pointer");
    adam_tick_kernel<<<1, 1, 0, (hipStream_t)stream>>>(t_dev, lr_t_dev, lr, beta1, beta2);
    return p2p_check_launch("p2p_adam_tick");
}

extern "C" int p2p_adam_flat_dev(float* p, const float* g, float* m, float* v, long long n, const float* lr_t_dev,
                                 float beta1, float beta2, float eps, float gscale, void* stream) {
    const p2p_adam_args a = {p, g, m, v, nullptr, n, 0, 0, lr_t_dev, nullptr, nullptr, nullptr, 0, 0};
    return adam_launch(a, {beta1, beta2, eps, 0.f, 0.f}, gscale, false, "p2p_adam_flat_dev", stream);
}

extern "C" int p2p_adam_ema_flat_dev(float* p, const float* g, float* m, float* v, float* e, long long n, const float* lr_t_dev,
                                     float beta1, float beta2, float eps, float gscale, const int* t_dev, float decay, int warmup,
                                     void* stream) {
    const p2p_adam_args a = {p, g, m, v, e, n, 0, 0, lr_t_dev, nullptr, t_dev, nullptr, warmup, 0};
    return adam_launch(a, {beta1, beta2, eps, 0.f, decay}, gscale, true, "p2p_adam_ema_flat_dev", stream);
}

extern "C" int p2p_adam_flat_dev_excl(float* p, const float* g, float* m, float* v, long long n, long long ex_lo, long long ex_hi,
                                      const float* lr_t_dev, float beta1, float beta2, float eps, float gscale, void* stream) {
    const p2p_adam_args a = {p, g, m, v, nullptr, n, ex_lo, ex_hi, lr_t_dev, nullptr, nullptr, nullptr, 0, 0};
    return adam_launch(a, {beta1, beta2, eps, 0.f, 0.f}, gscale, false, "p2p_adam_flat_dev_excl", stream);
}

extern "C" int p2p_adam_ema_flat_dev_excl(float* p, const float* g, float* m, float* v, float* e, long long n, long long ex_lo,
                                          long long ex_hi, const float* lr_t_dev, float beta1, float beta2, float eps, float gscale,
                                          const int* t_dev, float decay, int warmup, void* stream) {
    const p2p_adam_args a = {p, g, m, v, e, n, ex_lo, ex_hi, lr_t_dev, nullptr, t_dev, nullptr, warmup, 0};
    return adam_launch(a, {beta1, beta2, eps, 0.f, decay}, gscale, true, "p2p_adam_ema_flat_dev_excl", stream);
}

// The moving average as a pass of its own, for the steps whose Adam runs in another kernel (p2p_adam_prep_batched): reads the
// updated p and e, writes e.  ema_update's arithmetic: the same bits as the fused forms.
__global__ void ema_flat_kernel(const float* __restrict__ p, long long n, EmaArgs ema) {
    const float omb = ema_one_minus_beta(ema);
    long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    long long stride = (long long)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        const f32x4 pi = *(const f32x4*)(p + i);
        f32x4 ei = *(const f32x4*)(ema.e + i);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float ek = ei[k];
            ema_update(ek, pi[k], omb);
            ei[k] = ek;
        }
        *(f32x4*)(ema.e + i) = ei;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long j = n / 4 * 4; j < n; ++j) ema_update(ema.e[j], p[j], omb);
}

extern "C" int p2p_ema_flat(float* e, const float* p, long long n, const int* t_dev, float decay, int warmup, void* stream) {
    P2P_REQUIRE(e && p && n > 0 && t_dev, "p2p_ema_flat: bad args");
    P2P_REQUIRE(aligned16(e, p), "p2p_ema_flat: buffers must be 16-byte aligned");
    ema_flat_kernel<<<vector_grid(n / 4), 256, 0, (hipStream_t)stream>>>(p, n, EmaArgs{e, t_dev, decay, warmup});
    return p2p_check_launch("p2p_ema_flat");
}

// ---- optimizer options --------------------------------------------------------------------------------
// Learning-rate schedules of Keras 2.9 (tf.keras.optimizers.schedules: ExponentialDecay, PiecewiseConstantDecay, PolynomialDecay,
// CosineDecay) and the build-added LinearDecay, restated in f64 and evaluated at `step` = the iteration count before the increment
// (OptimizerV2._decayed_lr evaluates the schedule at `iterations`; apply_gradients increments afterwards).  Definitions:
// include/p2pgan.h p2p_lr_schedule; host restatement: palette_and_histo_gan_amd/schedules.py.
__device__ __forceinline__ double lr_schedule(const p2p_lr_schedule& s, double step) {
    double lr = s.initial;
    switch (s.kind) {
    case P2P_LR_EXPONENTIAL: {      // ExponentialDecay.__call__: initial * decay_rate ^ (step / decay_steps), floor under staircase
        double p = step / s.decay_steps;
        if (s.flag) p = floor(p);
        lr = s.initial * pow(s.rate, p);
        break;
    }
    case P2P_LR_PIECEWISE: {        // PiecewiseConstantDecay.__call__: the boundaries are inclusive on the right
        int i = 0;
        while (i < s.nbounds && step > s.bounds[i]) ++i;
        lr = s.values[i];
        break;
    }
    case P2P_LR_POLYNOMIAL: {       // PolynomialDecay.__call__
        double d = s.decay_steps, g = step;
        if (s.flag) d = s.decay_steps * (step == 0.0 ? 1.0 : ceil(step / s.decay_steps));
        else g = fmin(step, s.decay_steps);
        lr = (s.initial - s.end) * pow(1.0 - g / d, s.power) + s.end;
        break;
    }
    case P2P_LR_COSINE: {           // CosineDecay.__call__ (alpha = rate)
        const double c = 0.5 * (1.0 + cos(3.14159265358979323846 * (fmin(step, s.decay_steps) / s.decay_steps)));
        lr = s.initial * ((1.0 - s.rate) * c + s.rate);
        break;
    }
    case P2P_LR_LINEAR:             // LinearDecay: constant, then linear, then `end`
        if (step >= s.hold_steps + s.decay_steps) lr = s.end;
        else if (step >= s.hold_steps) lr = s.initial + (s.end - s.initial) * ((step - s.hold_steps) / s.decay_steps);
        break;
    default: break;
    }
    if (s.warmup_steps > 0.0 && step < s.warmup_steps) lr = lr * ((step + 1.0) / s.warmup_steps);
    return lr;
}

__global__ void adam_tick_sched_kernel(int* __restrict__ t, float* __restrict__ lr_t, p2p_lr_schedule s, float b1, float b2) {
    int tt = t[0] + 1;
    t[0] = tt;
    const double lr = lr_schedule(s, (double)(tt - 1));
    lr_t[0] = (float)(lr * sqrt(1.0 - pow((double)b2, (double)tt)) / (1.0 - pow((double)b1, (double)tt)));
}

extern "C" int p2p_adam_tick_sched(int* t_dev, float* lr_t_dev, const p2p_lr_schedule* sched, float beta1, float beta2,
                                   void* stream) {
    P2P_REQUIRE(t_dev && lr_t_dev && sched, "p2p_adam_tick_sched: null pointer");
    P2P_REQUIRE(sched->kind >= P2P_LR_CONSTANT && sched->kind <= P2P_LR_LINEAR, "p2p_adam_tick_sched: unknown schedule kind %d",
                sched->kind);
    P2P_REQUIRE(sched->kind != P2P_LR_PIECEWISE || (sched->nbounds >= 1 && sched->nbounds <= 8),
                "p2p_adam_tick_sched: a piecewise schedule holds 1..8 boundaries, got %d", sched->nbounds);
    P2P_REQUIRE(sched->kind == P2P_LR_CONSTANT || sched->kind == P2P_LR_PIECEWISE || sched->decay_steps > 0.0,
                "p2p_adam_tick_sched: decay_steps must be positive");
    adam_tick_sched_kernel<<<1, 1, 0, (hipStream_t)stream>>>(t_dev, lr_t_dev, *sched, beta1, beta2);
    return p2p_check_launch("p2p_adam_tick_sched");
}

// Global gradient norm in a fixed order (include/p2pgan.h p2p_sumsq_partials: lane, vector component, wave tree, block partial;
// p2p_clip_scale: lane-strided serial sums of the partials, wave tree).  Every add and multiply is a rounded f32 operation.
__device__ __forceinline__ float wave_tree_sum(float acc) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_down(acc, off, 64);
    return acc;         // lane 0: the tree's root; the other lanes hold sums nobody reads
}

__global__ void __launch_bounds__(256) sumsq_partials_kernel(const float* __restrict__ g, long long n, long long ex_lo, long long ex_hi,
                                                             float* __restrict__ partials) {
#pragma clang fp contract(off)
    __shared__ float wsum[4];
    const long long nvec = n / 4;
    const long long stride = (long long)gridDim.x * 256;
    float acc = 0.f;
    for (long long j = (long long)blockIdx.x * 256 + threadIdx.x; j < nvec; j += stride) {
        const long long i = j * 4;
        if (i >= ex_lo && i + 4 <= ex_hi) continue;             // wholly inside the hole: four zeros, acc unchanged
        const f32x4 gi = *(const f32x4*)(g + i);
        const bool whole = i + 4 <= ex_lo || i >= ex_hi;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float gk = (whole || i + k < ex_lo || i + k >= ex_hi) ? gi[k] : 0.f;
            const float sq = gk * gk;
            acc = acc + sq;
        }
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long j = nvec * 4; j < n; ++j) {
            const float gk = (j < ex_lo || j >= ex_hi) ? g[j] : 0.f;
            const float sq = gk * gk;
            acc = acc + sq;
        }
    acc = wave_tree_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

static inline int sumsq_blocks(long long n) {
    long long nb = (n / 4 + 255) / 256;
    if (nb < 1) nb = 1;
    if (nb > P2P_SUMSQ_MAX_PARTS) nb = P2P_SUMSQ_MAX_PARTS;
    return (int)nb;
}

extern "C" int p2p_sumsq_partials(const float* g, long long n, long long ex_lo, long long ex_hi, float* partials, int* nparts_out,
                                  void* stream) {
    P2P_REQUIRE(g && partials && nparts_out && n > 0, "p2p_sumsq_partials: bad args");
    P2P_REQUIRE(0 <= ex_lo && ex_lo <= ex_hi && ex_hi <= n, "p2p_sumsq_partials: the excluded range must lie inside [0, n)");
    P2P_REQUIRE(aligned16(g), "p2p_sumsq_partials: the gradient must be 16-byte aligned");
    const int nb = sumsq_blocks(n);
    sumsq_partials_kernel<<<dim3((unsigned)nb), 256, 0, (hipStream_t)stream>>>(g, n, ex_lo, ex_hi, partials);
    *nparts_out = nb;
    return p2p_check_launch("p2p_sumsq_partials");
}

struct ClipBufs { const float* p[P2P_CLIP_MAX_BUFS]; int n[P2P_CLIP_MAX_BUFS]; int nbuf; };

__global__ void __launch_bounds__(64) clip_scale_kernel(ClipBufs b, float clipnorm, float* __restrict__ scale, float* __restrict__ norm_out) {
#pragma clang fp contract(off)
    float acc = 0.f;
    int base = 0;           // index of the buffer's first partial in the concatenated list
    for (int k = 0; k < b.nbuf; ++k) {
        // lane l takes the list entries l, l + 64, ...: inside buffer k those are its entries i with (base + i) % 64 == l
        for (int i = ((int)threadIdx.x - base % 64 + 64) % 64; i < b.n[k]; i += 64) acc = acc + b.p[k][i];
        base += b.n[k];
    }
    acc = wave_tree_sum(acc);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(acc);              // correctly rounded, as in adam_update (the _rn intrinsic is the native, approximate one)
        float s = 1.0f;
        if (!isfinite(norm)) s = __builtin_nanf("");                    // tf.clip_by_global_norm: non-finite norm -> NaN everywhere
        else if (norm > clipnorm) s = __fdiv_rn(clipnorm, norm);
        scale[0] = s;
        norm_out[0] = norm;
    }
}

extern "C" int p2p_clip_scale(const float* const* partials, const int* nparts, int nbuf, float clipnorm, float* scale_dev,
                              float* norm_dev, void* stream) {
    P2P_REQUIRE(partials && nparts && scale_dev && norm_dev && nbuf >= 1 && nbuf <= P2P_CLIP_MAX_BUFS, "p2p_clip_scale: bad args");
    P2P_REQUIRE(clipnorm > 0.f, "p2p_clip_scale: the threshold must be positive");
    ClipBufs b;
    b.nbuf = nbuf;
    for (int k = 0; k < P2P_CLIP_MAX_BUFS; ++k) {
        b.p[k] = k < nbuf ? partials[k] : nullptr;
        b.n[k] = k < nbuf ? nparts[k] : 0;
        P2P_REQUIRE(k >= nbuf || (b.p[k] && b.n[k] >= 1 && b.n[k] <= P2P_SUMSQ_MAX_PARTS), "p2p_clip_scale: buffer %d: bad partials", k);
    }
    clip_scale_kernel<<<1, 64, 0, (hipStream_t)stream>>>(b, clipnorm, scale_dev, norm_dev);
    return p2p_check_launch("p2p_clip_scale");
}

extern "C" int p2p_adam_step(const p2p_adam_args* a, void* stream) {
    P2P_REQUIRE(a && a->hyper, "p2p_adam_step: null argument struct");
    return adam_launch(*a, *a->hyper, 1.0f, a->e != nullptr, "p2p_adam_step", stream);
}

__global__ void counter_add_kernel(long long* c, long long inc) { c[0] += inc; }

extern "C" int p2p_counter_add(long long* counter_dev, long long inc, void* stream) {
    P2P_REQUIRE(counter_dev, "p2p_counter_add: null pointer");
    counter_add_kernel<<<1, 1, 0, (hipStream_t)stream>>>(counter_dev, inc);
    return p2p_check_launch("p2p_counter_add");
}

// f32 gradient sum of a GradientTape (tape.py): a network's weight gradients over several calls, the two terms of a generator
// call's d(source).  dst = src for the first contribution, dst += src for every further one.  One thread per 16-byte chunk, no atomics: each element is one add in call
// order, so the sum is bit-reproducible.
__global__ void grad_accumulate_kernel(float* __restrict__ dst, const float* __restrict__ src, long long n, int first) {
    long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    long long stride = (long long)gridDim.x * blockDim.x * 4;
    for (; i + 3 < n; i += stride) {
        f32x4 s = *(const f32x4*)(src + i);
        if (!first) {
            f32x4 d = *(const f32x4*)(dst + i);
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = d[k] + s[k];
        }
        *(f32x4*)(dst + i) = s;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (long long j = n / 4 * 4; j < n; ++j) dst[j] = first ? src[j] : dst[j] + src[j];
}

extern "C" int p2p_grad_accumulate(float* dst, const float* src, long long n, int first, void* stream) {
    P2P_REQUIRE(dst && src && n > 0, "p2p_grad_accumulate: bad args");
    P2P_REQUIRE(aligned16(dst, src), "p2p_grad_accumulate: buffers must be 16-byte aligned");
    grad_accumulate_kernel<<<vector_grid(n / 4), 256, 0, (hipStream_t)stream>>>(dst, src, n, first);
    return p2p_check_launch("p2p_grad_accumulate");
}

// wn[t][g][d] = T(w[t][g][d]) for g < wn_rows, d < wn_cols;  wt[t][d][g] = T(w[t][g][d]) for d < wt_rows,
// g < wt_cols; entries outside the real [Cg][Cd] block are written as zeros (channel padding of the edge
// layers).  32x32 LDS tile transpose per tap.
template <typename T>
__device__ __forceinline__ void weight_prep_tile(const float* __restrict__ w, int Cg, int Cd, T* __restrict__ wn, int wn_rows,
                                                 int wn_cols, T* __restrict__ wt, int wt_rows, int wt_cols, int t, int g0, int d0,
                                                 float (*tile)[33]) {
    const float* wp = w + (long long)t * Cg * Cd;
    int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
    for (int r = ty; r < 32; r += 8) {
        int g = g0 + r, d = d0 + tx;
        float val = (g < Cg && d < Cd) ? wp[(long long)g * Cd + d] : 0.f;
        tile[r][tx] = val;
        if (wn && g < wn_rows && d < wn_cols) wn[((long long)t * wn_rows + g) * wn_cols + d] = from_f32<T>(val);
    }
    __syncthreads();
    if (wt) {
        for (int r = ty; r < 32; r += 8) {
            int d = d0 + r, g = g0 + tx;
            if (d < wt_rows && g < wt_cols) wt[((long long)t * wt_rows + d) * wt_cols + g] = from_f32<T>(tile[tx][r]);
        }
    }
}

template <typename T>
__global__ void weight_prep_kernel(const float* __restrict__ w, int Cg, int Cd, T* __restrict__ wn, int wn_rows,
                                   int wn_cols, T* __restrict__ wt, int wt_rows, int wt_cols) {
    __shared__ float tile[32][33];
    weight_prep_tile<T>(w, Cg, Cd, wn, wn_rows, wn_cols, wt, wt_rows, wt_cols, blockIdx.z, blockIdx.y * 32, blockIdx.x * 32, tile);
}

// Batched form: one launch re-derives the copies of every layer after an optimizer step.  Workgroup b serves the
// task whose [first_block, first_block + 16 * tiles_g * tiles_d) range holds b (<= 64 tasks, scanned linearly).
// 64x64 tiles with 16-byte reads and 4-element stores for the unpadded layers whose channel counts are multiples of 64
// (every encoder/decoder block but up6): a quarter of the workgroups, whole 128/256-byte rows per wave access.
static __host__ __device__ inline bool prep_tile64(int Cg, int Cd, int wn_rows, int wn_cols, int wt_rows, int wt_cols,
                                                   bool have_wn, bool have_wt) {
    return Cg % 64 == 0 && Cd % 64 == 0 && (!have_wn || (wn_rows == Cg && wn_cols == Cd)) &&
           (!have_wt || (wt_rows == Cd && wt_cols == Cg));
}

template <typename T>
__device__ __forceinline__ void weight_prep_tile64(const float* __restrict__ w, int Cg, int Cd, T* __restrict__ wn,
                                                   T* __restrict__ wt, int t, int g0, int d0, float (*tile)[65]) {
    typedef __attribute__((__vector_size__(4 * sizeof(T)))) T vec4_t;
    const float* wp = w + (long long)t * Cg * Cd;
    const int c4 = (threadIdx.x & 15) * 4, r0 = threadIdx.x >> 4;         // 16 column quads x 16 rows per pass
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + 16 * i;
        const f32x4 v = *(const f32x4*)(wp + (long long)(g0 + r) * Cd + d0 + c4);
        tile[r][c4] = v[0]; tile[r][c4 + 1] = v[1]; tile[r][c4 + 2] = v[2]; tile[r][c4 + 3] = v[3];
        if (wn) {
            vec4_t q;
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = from_f32<T>(v[k]);
            *(vec4_t*)(wn + ((long long)t * Cg + g0 + r) * Cd + d0 + c4) = q;
        }
    }
    __syncthreads();
    if (wt) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int d = r0 + 16 * i;
            vec4_t q;
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = from_f32<T>(tile[c4 + k][d]);
            *(vec4_t*)(wt + ((long long)t * Cd + d0 + d) * Cg + g0 + c4) = q;
        }
    }
}

template <typename T>
__global__ void weight_prep_batched_kernel(const p2p_prep_task* __restrict__ tasks, int ntasks) {
    __shared__ float tile[64][65];
    const long long b = blockIdx.x;
    int ti = 0;
    while (ti + 1 < ntasks && tasks[ti + 1].first_block <= b) ++ti;
    const p2p_prep_task k = tasks[ti];
    const int local = (int)(b - k.first_block);
    const int per_tap = k.tiles_g * k.tiles_d;
    const int t = local / per_tap, rem = local - t * per_tap;
    const int gy = rem / k.tiles_d, dx = rem - gy * k.tiles_d;
    if (prep_tile64(k.Cg, k.Cd, k.wn_rows, k.wn_cols, k.wt_rows, k.wt_cols, k.wn != nullptr, k.wt != nullptr)) {
        weight_prep_tile64<T>(k.w, k.Cg, k.Cd, (T*)k.wn, (T*)k.wt, t, gy * 64, dx * 64, tile);
        return;
    }
    weight_prep_tile<T>(k.w, k.Cg, k.Cd, (T*)k.wn, k.wn_rows, k.wn_cols, (T*)k.wt, k.wt_rows, k.wt_cols, t, gy * 32, dx * 32,
                        (float (*)[33])tile);
}

// ---- Adam + weight copies in one pass (SURVEY.md 2.3 K18 "also emits the bf16 weight copy") -------------------------------
// The same tiling as the batched weight prep, but the master tile is UPDATED on the way: theta, g, m, v are read, the Keras
// Adam step of p2p_adam_flat_dev is applied (the same expressions, but written out in ADAM_ONE and contracted as the compiler sees
// fit, not adam_update's spelled-out roundings: the masters may differ from the flat pass in the last bit, which is what
// tests/test_train_step_gpu.py allows this pair), theta, m, v are written back and the fresh value goes straight into the two operand copies.  Saves the second read of the 117 MB master.  Every master element
// lies in exactly one tile of its task; the caller lists every kernel ONCE.
struct AdamCtx { float* p0; const float* g0; float* m0; float* v0; const float* lr_t; float b1, b2, eps; };

#define ADAM_ONE(p, g, m, v)                                   \
    do {                                                       \
        m = c.b1 * (m) + (1.f - c.b1) * (g);                   \
        v = c.b2 * (v) + (1.f - c.b2) * (g) * (g);             \
        p = (p) - lr_t * (m) / (sqrtf(v) + c.eps);             \
    } while (0)

template <typename T>
__global__ void adam_prep_batched_kernel(const p2p_prep_task* __restrict__ tasks, int ntasks, AdamCtx c) {
    typedef __attribute__((__vector_size__(4 * sizeof(T)))) T vec4_t;
    __shared__ float tile[64][65];
    const long long b = blockIdx.x;
    int ti = 0;
    while (ti + 1 < ntasks && tasks[ti + 1].first_block <= b) ++ti;
    const p2p_prep_task k = tasks[ti];
    const int local = (int)(b - k.first_block);
    const int per_tap = k.tiles_g * k.tiles_d;
    const int t = local / per_tap, rem = local - t * per_tap;
    const int gy = rem / k.tiles_d, dx = rem - gy * k.tiles_d;
    const float lr_t = c.lr_t[0];
    const long long base = (k.w - c.p0) + (long long)t * k.Cg * k.Cd;        // element index of this tap in the flat buffers
    T* wn = (T*)k.wn;
    T* wt = (T*)k.wt;
    if (prep_tile64(k.Cg, k.Cd, k.wn_rows, k.wn_cols, k.wt_rows, k.wt_cols, wn != nullptr, wt != nullptr)) {
        const int g0 = gy * 64, d0 = dx * 64;
        const int c4 = (threadIdx.x & 15) * 4, r0 = threadIdx.x >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int r = r0 + 16 * i;
            const long long e = base + (long long)(g0 + r) * k.Cd + d0 + c4;
            f32x4 pv = *(const f32x4*)(c.p0 + e), mv = *(const f32x4*)(c.m0 + e), vv = *(const f32x4*)(c.v0 + e);
            const f32x4 gv = *(const f32x4*)(c.g0 + e);
#pragma unroll
            for (int q = 0; q < 4; ++q) ADAM_ONE(pv[q], gv[q], mv[q], vv[q]);
            *(f32x4*)(c.p0 + e) = pv; *(f32x4*)(c.m0 + e) = mv; *(f32x4*)(c.v0 + e) = vv;
            tile[r][c4] = pv[0]; tile[r][c4 + 1] = pv[1]; tile[r][c4 + 2] = pv[2]; tile[r][c4 + 3] = pv[3];
            if (wn) {
                vec4_t q4;
#pragma unroll
                for (int q = 0; q < 4; ++q) q4[q] = from_f32<T>(pv[q]);
                *(vec4_t*)(wn + ((long long)t * k.Cg + g0 + r) * k.Cd + d0 + c4) = q4;
            }
        }
        __syncthreads();
        if (wt) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int d = r0 + 16 * i;
                vec4_t q4;
#pragma unroll
                for (int q = 0; q < 4; ++q) q4[q] = from_f32<T>(tile[c4 + q][d]);
                *(vec4_t*)(wt + ((long long)t * k.Cd + d0 + d) * k.Cg + g0 + c4) = q4;
            }
        }
        return;
    }
    float (*t32)[33] = (float (*)[33])tile;
    const int g0 = gy * 32, d0 = dx * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int r = ty; r < 32; r += 8) {
        const int g = g0 + r, d = d0 + tx;
        float val = 0.f;
        if (g < k.Cg && d < k.Cd) {
            const long long e = base + (long long)g * k.Cd + d;
            float pv = c.p0[e], mv = c.m0[e], vv = c.v0[e];
            const float gv = c.g0[e];
            ADAM_ONE(pv, gv, mv, vv);
            val = pv;
            c.p0[e] = pv; c.m0[e] = mv; c.v0[e] = vv;
        }
        t32[r][tx] = val;
        if (wn && g < k.wn_rows && d < k.wn_cols) wn[((long long)t * k.wn_rows + g) * k.wn_cols + d] = from_f32<T>(val);
    }
    __syncthreads();
    if (wt) {
        for (int r = ty; r < 32; r += 8) {
            const int d = d0 + r, g = g0 + tx;
            if (d < k.wt_rows && g < k.wt_cols) wt[((long long)t * k.wt_rows + d) * k.wt_cols + g] = from_f32<T>(t32[tx][r]);
        }
    }
}

extern "C" int p2p_adam_prep_batched(int dtype, long long n_elems, const p2p_prep_task* tasks_dev, int ntasks, long long total_blocks,
                                     float* params, const float* grads, float* m, float* v, const float* lr_t_dev, float beta1,
                                     float beta2, float eps, void* stream) {
    P2P_REQUIRE(tasks_dev && ntasks >= 1 && ntasks <= 64 && total_blocks >= 1 && total_blocks < (1LL << 31) && n_elems > 0,
                "p2p_adam_prep_batched: bad args");
    P2P_REQUIRE(params && grads && m && v && lr_t_dev, "p2p_adam_prep_batched: null pointer");
    P2P_REQUIRE(aligned16(params, grads, m, v), "p2p_adam_prep_batched: buffers must be 16-byte aligned");
    AdamCtx c = {params, grads, m, v, lr_t_dev, beta1, beta2, eps};
    P2P_DISPATCH_DTYPE(dtype, (adam_prep_batched_kernel<T><<<dim3((unsigned)total_blocks), 256, 0, (hipStream_t)stream>>>(tasks_dev, ntasks, c)));
    return p2p_check_launch("p2p_adam_prep_batched");
}

extern "C" long long p2p_weight_prep_task_blocks(int Cg, int Cd, int wn_rows, int wn_cols, int wt_rows, int wt_cols,
                                                 int have_wn, int have_wt, int* tiles_g, int* tiles_d) {
    int gmax = Cg, dmax = Cd;
    if (have_wn) { gmax = gmax > wn_rows ? gmax : wn_rows; dmax = dmax > wn_cols ? dmax : wn_cols; }
    if (have_wt) { gmax = gmax > wt_cols ? gmax : wt_cols; dmax = dmax > wt_rows ? dmax : wt_rows; }
    const int ts = prep_tile64(Cg, Cd, wn_rows, wn_cols, wt_rows, wt_cols, have_wn != 0, have_wt != 0) ? 64 : 32;
    const int tg = (gmax + ts - 1) / ts, td = (dmax + ts - 1) / ts;
    if (tiles_g) *tiles_g = tg;
    if (tiles_d) *tiles_d = td;
    return 16LL * tg * td;
}

extern "C" int p2p_weight_prep_batched(int dtype, const p2p_prep_task* tasks_dev, int ntasks, long long total_blocks, void* stream) {
    P2P_REQUIRE(tasks_dev && ntasks >= 1 && ntasks <= 64 && total_blocks >= 1 && total_blocks < (1LL << 31),
                "p2p_weight_prep_batched: bad args");
    P2P_DISPATCH_DTYPE(dtype, (weight_prep_batched_kernel<T><<<dim3((unsigned)total_blocks), 256, 0, (hipStream_t)stream>>>(tasks_dev, ntasks)));
    return p2p_check_launch("p2p_weight_prep_batched");
}

extern "C" int p2p_weight_prep_pad(int dtype, const float* w, int Cg, int Cd, void* wn, int wn_rows, int wn_cols,
                                   void* wt, int wt_rows, int wt_cols, void* stream) {
    P2P_REQUIRE(w && Cg > 0 && Cd > 0 && (wn || wt), "p2p_weight_prep: bad args");
    int gmax = Cg, dmax = Cd;
    if (wn) { gmax = gmax > wn_rows ? gmax : wn_rows; dmax = dmax > wn_cols ? dmax : wn_cols; }
    if (wt) { gmax = gmax > wt_cols ? gmax : wt_cols; dmax = dmax > wt_rows ? dmax : wt_rows; }
    dim3 grid((dmax + 31) / 32, (gmax + 31) / 32, 16);
    P2P_DISPATCH_DTYPE(dtype, (weight_prep_kernel<T><<<grid, 256, 0, (hipStream_t)stream>>>(
                                  w, Cg, Cd, (T*)wn, wn_rows, wn_cols, (T*)wt, wt_rows, wt_cols)));
    return p2p_check_launch("p2p_weight_prep");
}

extern "C" int p2p_weight_prep(int dtype, const float* w, int Cg, int Cd, void* wn, void* wt, void* stream) {
    return p2p_weight_prep_pad(dtype, w, Cg, Cd, wn, Cg, Cd, wt, Cd, Cg, stream);
}

template <typename T>
__global__ void pack_input_kernel(int N, PixDec dec, int C, const void* __restrict__ src, int src_is_int, TView dst) {
    const unsigned npix = (unsigned)N * dec.H * dec.W;
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
        int n, y, x;
        dec(p, n, y, x);
        T* d = (T*)dst.ptr + dst.off(n, y, x);
        const long long e = (long long)p * C;
        for (int c = 0; c < C; ++c) {
            float v = src_is_int ? (float)((const int*)src)[e + c] : ((const float*)src)[e + c];
            d[c] = from_f32<T>(v);
        }
    }
}

// One launch scatters a dense batch into up to 4 views (the source image feeds down1, the last skip connection and
// both discriminator inputs; networks.py:45,92-94): read once, write everywhere.
struct PackDst { TView v[4]; int n; };

template <typename T>
__global__ void pack_multi_kernel(int N, PixDec dec, int C, const void* __restrict__ src, int src_is_int, PackDst dst) {
    const unsigned npix = (unsigned)N * dec.H * dec.W;
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
        int n, y, x;
        dec(p, n, y, x);
        if (C == 4 && !src_is_int) {      // RGBA pixel: one 16-byte read, one 4-channel vector store per view
            typedef __attribute__((__vector_size__(4 * sizeof(T)))) T vec4_t;
            f32x4 v = *(const f32x4*)((const float*)src + (long long)p * 4);
            vec4_t q;
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = from_f32<T>(v[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < dst.n) *(vec4_t*)((T*)dst.v[k].ptr + dst.v[k].off(n, y, x)) = q;
            continue;
        }
        const long long e = (long long)p * C;
        for (int c = 0; c < C; ++c) {
            float v = src_is_int ? (float)((const int*)src)[e + c] : ((const float*)src)[e + c];
            T q = from_f32<T>(v);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < dst.n) ((T*)dst.v[k].ptr)[dst.v[k].off(n, y, x) + c] = q;
        }
    }
}

// The RGBA batch of a train step in ONE launch (dataset_utils.py:209-229 -> networks.py:45,92-94): per pixel one 16-byte read
// of the source and of the target, and whole 16-byte pixel stores wherever the destination pixel is complete:
//   v_src   [source | 0 0 0 0]            down1's input
//   v_c6    [source | 0 0 0 0]            channels 32..39 of the last concat buffer
//   v_dreal [target | source]             discriminator input, real half
//   v_dfake [  ...  | source]             discriminator input, fake half: only the source half (the generator writes the rest)
template <typename T>
__global__ void pack_pair_kernel(int N, PixDec dec, const float* __restrict__ source, const float* __restrict__ target, TView v_src,
                                 TView v_c6, TView v_dreal, TView v_dfake) {
    typedef __attribute__((__vector_size__(4 * sizeof(T)))) T vec4_t;
    typedef __attribute__((__vector_size__(8 * sizeof(T)))) T vec8_t;
    const unsigned npix = (unsigned)N * dec.H * dec.W;
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
        int n, y, x;
        dec(p, n, y, x);
        const f32x4 s4 = *(const f32x4*)(source + (long long)p * 4), t4 = *(const f32x4*)(target + (long long)p * 4);
        vec4_t sq;
        vec8_t sz, ts;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            sq[k] = from_f32<T>(s4[k]);
            sz[k] = sq[k]; sz[4 + k] = from_f32<T>(0.f);
            ts[k] = from_f32<T>(t4[k]); ts[4 + k] = sq[k];
        }
        *(vec8_t*)((T*)v_src.ptr + v_src.off(n, y, x)) = sz;
        if (v_c6.ptr) *(vec8_t*)((T*)v_c6.ptr + v_c6.off(n, y, x)) = sz;
        *(vec8_t*)((T*)v_dreal.ptr + v_dreal.off(n, y, x)) = ts;
        if (v_dfake.ptr) *(vec4_t*)((T*)v_dfake.ptr + v_dfake.off(n, y, x) + 4) = sq;
    }
}

extern "C" int p2p_pack_pair(int dtype, int N, int H, int W, const float* source, const float* target, const p2p_tensor* v_src,
                             const p2p_tensor* v_c6, const p2p_tensor* v_dreal, const p2p_tensor* v_dfake, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && source && target && v_src && v_dreal, "p2p_pack_pair: bad args");
    P2P_REQUIRE((long long)N * H * W < (1LL << 31), "p2p_pack_pair: too many pixels");
    const int esz = dtype == P2P_BF16 ? 2 : 4;
    // v_c6 / v_dfake may be NULL: those two stores are PARTIAL pixels (16 of 80 bytes, 8 of 16), and the train step leaves them
    // to the kernels that write the rest of the pixel (p2p_norm_act_fwd_tail, p2p_tanh_l1_fwd_pair)
    const p2p_tensor* vs[4] = {v_src, v_c6, v_dreal, v_dfake};
    for (int k = 0; k < 4; ++k)
        P2P_REQUIRE(!vs[k] || (vs[k]->ptr && vs[k]->ld % 8 == 0 && ((uintptr_t)vs[k]->ptr % (8 * esz)) == 0),
                    "p2p_pack_pair: views must start on an 8-channel boundary (whole 16/32-byte pixels)");
    TView none;
    none.ptr = nullptr; none.img = 0; none.row = 0; none.ld = 0;
    const TView vc = v_c6 ? make_view(v_c6) : none, vd = v_dfake ? make_view(v_dfake) : none;
    P2P_REQUIRE(((uintptr_t)source % 16) == 0 && ((uintptr_t)target % 16) == 0, "p2p_pack_pair: batches must be 16-byte aligned");
    long long blocks = ((long long)N * H * W + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    P2P_DISPATCH_DTYPE(dtype, (pack_pair_kernel<T><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(
                                  N, PixDec::make(H, W), source, target, make_view(v_src), vc, make_view(v_dreal), vd)));
    return p2p_check_launch("p2p_pack_pair");
}

// The palette-index batch of a train step (Pix2PixIndexedModel: one int32 index per pixel, dataset_utils.py:232-246) in one
// launch, WHOLE 8-channel pixels everywhere (a 2-byte store into a 16-byte pixel is a partial sector write):
//   v_src   [source 0 0 0 0 0 0 0]      down1's input
//   v_c6    the same pixel               channels 32..39 of the last concat buffer (NULL: left to p2p_norm_act_fwd_tail)
//   v_dreal [target source 0 ...]        discriminator input, real half
//   v_dfake [0      source 0 ...]        fake half: channel 0 is written later by the head (argmax)
template <typename T>
__global__ void pack_pair_idx_kernel(int N, PixDec dec, const int* __restrict__ source, const int* __restrict__ target, TView v_src,
                                     TView v_c6, TView v_dreal, TView v_dfake) {
    typedef __attribute__((__vector_size__(8 * sizeof(T)))) T vec8_t;
    const unsigned npix = (unsigned)N * dec.H * dec.W;
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < npix; p += gridDim.x * blockDim.x) {
        int n, y, x;
        dec(p, n, y, x);
        const T sq = from_f32<T>((float)source[p]), tq = from_f32<T>((float)target[p]), z = from_f32<T>(0.f);
        vec8_t a, b, c;
#pragma unroll
        for (int k = 0; k < 8; ++k) { a[k] = z; b[k] = z; c[k] = z; }
        a[0] = sq;
        b[0] = tq; b[1] = sq;
        c[1] = sq;
        *(vec8_t*)((T*)v_src.ptr + v_src.off(n, y, x)) = a;
        if (v_c6.ptr) *(vec8_t*)((T*)v_c6.ptr + v_c6.off(n, y, x)) = a;
        *(vec8_t*)((T*)v_dreal.ptr + v_dreal.off(n, y, x)) = b;
        *(vec8_t*)((T*)v_dfake.ptr + v_dfake.off(n, y, x)) = c;
    }
}

extern "C" int p2p_pack_pair_idx(int dtype, int N, int H, int W, const int* source, const int* target, const p2p_tensor* v_src,
                                 const p2p_tensor* v_c6, const p2p_tensor* v_dreal, const p2p_tensor* v_dfake, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && source && target && v_src && v_dreal && v_dfake, "p2p_pack_pair_idx: bad args");
    P2P_REQUIRE((long long)N * H * W < (1LL << 31), "p2p_pack_pair_idx: too many pixels");
    const int esz = dtype == P2P_BF16 ? 2 : 4;
    const p2p_tensor* vs[4] = {v_src, v_c6, v_dreal, v_dfake};
    for (int k = 0; k < 4; ++k)
        P2P_REQUIRE(!vs[k] || (vs[k]->ptr && vs[k]->ld % 8 == 0 && ((uintptr_t)vs[k]->ptr % (8 * esz)) == 0),
                    "p2p_pack_pair_idx: views must start on an 8-channel boundary (whole 16/32-byte pixels)");
    TView none;
    none.ptr = nullptr; none.img = 0; none.row = 0; none.ld = 0;
    long long blocks = ((long long)N * H * W + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    P2P_DISPATCH_DTYPE(dtype, (pack_pair_idx_kernel<T><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(
                                  N, PixDec::make(H, W), source, target, make_view(v_src), v_c6 ? make_view(v_c6) : none,
                                  make_view(v_dreal), make_view(v_dfake))));
    return p2p_check_launch("p2p_pack_pair_idx");
}

extern "C" int p2p_pack_input_multi(int dtype, int N, int H, int W, int C, const void* src, int src_is_int,
                                    const p2p_tensor* dsts, int ndst, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && src && dsts && ndst >= 1 && ndst <= 4, "p2p_pack_input_multi: bad args");
    PackDst d;
    d.n = ndst;
    for (int k = 0; k < 4; ++k) d.v[k] = make_view(&dsts[k < ndst ? k : 0]);
    if (C == 4 && !src_is_int) {      // the vector path needs 4-channel-aligned views
        const int esz = dtype == P2P_BF16 ? 2 : 4;
        for (int k = 0; k < ndst; ++k)
            P2P_REQUIRE(((uintptr_t)dsts[k].ptr % (4 * esz)) == 0 && (dsts[k].ld % 4) == 0 && ((uintptr_t)src % 16) == 0,
                        "p2p_pack_input_multi: RGBA views must be aligned to 4 channels");
    }
    long long total = (long long)N * H * W;
    P2P_REQUIRE(total < (1LL << 31), "p2p_pack_input_multi: too many pixels");
    long long blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    P2P_DISPATCH_DTYPE(dtype, (pack_multi_kernel<T><<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(N, PixDec::make(H, W), C, src, src_is_int, d)));
    return p2p_check_launch("p2p_pack_input_multi");
}

// out[0..6] = [g_total, g_adv, g_l1, g_aux, d_total, d_real, d_fake] from the loss slots (pix2pix_model.py:44-56,
// 242-250,273-278): g_total = adv + lambda_l1 * l1 + lambda_aux * aux, d_total = real + fake.
__global__ void finish_losses_kernel(const float* __restrict__ l, int aux_slot, int l1_slot, float lambda_l1, float lambda_aux,
                                     float* __restrict__ out) {
    float adv = l[2], l1 = l[l1_slot], aux = aux_slot >= 0 ? l[aux_slot] : 0.f;
    out[0] = adv + lambda_l1 * l1 + lambda_aux * aux;
    out[1] = adv; out[2] = l1; out[3] = aux;
    out[4] = l[0] + l[1]; out[5] = l[0]; out[6] = l[1];
}

extern "C" int p2p_finish_losses(const float* slots, int aux_slot, int l1_slot, float lambda_l1, float lambda_aux, float* out,
                                 void* stream) {
    P2P_REQUIRE(slots && out && l1_slot >= 0, "p2p_finish_losses: bad args");
    finish_losses_kernel<<<1, 1, 0, (hipStream_t)stream>>>(slots, aux_slot, l1_slot, lambda_l1, lambda_aux, out);
    return p2p_check_launch("p2p_finish_losses");
}

// As finish_losses_kernel for a generator loss of five terms (the fused palette step): out[3] reports the first of the two extra ones.
__global__ void finish_losses2_kernel(const float* __restrict__ l, int aux_slot, int aux2_slot, int l1_slot, float lambda_l1,
                                      float lambda_aux, float lambda_aux2, float* __restrict__ out) {
    float adv = l[2], l1 = l[l1_slot], aux = l[aux_slot], aux2 = l[aux2_slot];
    out[0] = adv + lambda_l1 * l1 + lambda_aux * aux + lambda_aux2 * aux2;
    out[1] = adv; out[2] = l1; out[3] = aux;
    out[4] = l[0] + l[1]; out[5] = l[0]; out[6] = l[1];
}

extern "C" int p2p_finish_losses2(const float* slots, int aux_slot, int aux2_slot, int l1_slot, float lambda_l1, float lambda_aux,
                                  float lambda_aux2, float* out, void* stream) {
    P2P_REQUIRE(slots && out && l1_slot >= 0 && aux_slot >= 0 && aux2_slot >= 0, "p2p_finish_losses2: bad args");
    finish_losses2_kernel<<<1, 1, 0, (hipStream_t)stream>>>(slots, aux_slot, aux2_slot, l1_slot, lambda_l1, lambda_aux, lambda_aux2, out);
    return p2p_check_launch("p2p_finish_losses2");
}

template <typename T>
__global__ void unpack_kernel(int N, int H, int W, int C, TView src, float* __restrict__ dst) {
    long long total = (long long)N * H * W * C;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        int c = (int)(i % C);
        long long p = i / C;
        int x = (int)(p % W);
        int y = (int)((p / W) % H);
        int n = (int)(p / ((long long)W * H));
        dst[i] = to_f32(((const T*)src.ptr)[src.off(n, y, x) + c]);
    }
}

static inline unsigned grid_for(long long total) {
    long long b = (total + 255) / 256;
    return (unsigned)(b < 4096 ? (b < 1 ? 1 : b) : 4096);
}

extern "C" int p2p_pack_input(int dtype, int N, int H, int W, int C, const void* src, int src_is_int,
                              const p2p_tensor* dst, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && src && dst && dst->ptr, "p2p_pack_input: bad args");
    P2P_REQUIRE((long long)N * H * W < (1LL << 31), "p2p_pack_input: too many pixels");
    P2P_DISPATCH_DTYPE(dtype, (pack_input_kernel<T><<<dim3(grid_for((long long)N * H * W)), 256, 0, (hipStream_t)stream>>>(
                                  N, PixDec::make(H, W), C, src, src_is_int, make_view(dst))));
    return p2p_check_launch("p2p_pack_input");
}

extern "C" int p2p_unpack(int dtype, int N, int H, int W, int C, const p2p_tensor* src, float* dst, void* stream) {
    P2P_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && src && src->ptr && dst, "p2p_unpack: bad args");
    P2P_DISPATCH_DTYPE(dtype, (unpack_kernel<T><<<dim3(grid_for((long long)N * H * W * C)), 256, 0, (hipStream_t)stream>>>(
                                  N, H, W, C, make_view(src), dst)));
    return p2p_check_launch("p2p_unpack");
}

// Bernoulli(0.5) keep mask of keras Dropout(0.5) (networks.py:31-32): counter-based (splitmix64 of
// seed, call counter, element index), one byte per element, 8 elements per hash.
__global__ void dropout_mask_kernel(unsigned char* __restrict__ mask, long long n, unsigned long long seed,
                                    unsigned long long counter, const long long* __restrict__ counter_dev, long long group0) {
    if (counter_dev) counter += (unsigned long long)counter_dev[0] * 16ull;      // device step counter (graph replay)
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    long long stride = (long long)gridDim.x * blockDim.x;
    for (; i * 8 < n; i += stride) {
        // the stream is keyed by the GLOBAL element index (group0 = 8-element groups in front of this shard): an N-rank
        // data-parallel step draws the masks of the single-process global batch
        unsigned long long z = seed * 0x9E3779B97F4A7C15ull + counter * 0xD1B54A32D192ED03ull + (unsigned long long)(i + group0);
        z += 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z = z ^ (z >> 31);
        for (int k = 0; k < 8 && i * 8 + k < n; ++k) mask[i * 8 + k] = (unsigned char)((z >> (8 * k + 3)) & 1ull);
    }
}

extern "C" int p2p_dropout_mask(unsigned char* mask, long long n, long long seed, long long counter, void* stream) {
    P2P_REQUIRE(mask && n > 0, "p2p_dropout_mask: bad args");
    long long blocks = (n / 8 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    dropout_mask_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(mask, n, (unsigned long long)seed,
                                                                                (unsigned long long)counter, nullptr, 0);
    return p2p_check_launch("p2p_dropout_mask");
}

// same, with the call counter = counter_dev[0] * 16 + salt read on the device (one salt per dropout layer)
extern "C" int p2p_dropout_mask_dev(unsigned char* mask, long long n, long long seed, const long long* counter_dev,
                                    long long salt, long long elem_offset, void* stream) {
    P2P_REQUIRE(mask && n > 0 && counter_dev, "p2p_dropout_mask_dev: bad args");
    P2P_REQUIRE(elem_offset >= 0 && elem_offset % 8 == 0, "p2p_dropout_mask_dev: elem_offset must be a non-negative multiple of 8");
    long long blocks = (n / 8 + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    if (blocks < 1) blocks = 1;
    dropout_mask_kernel<<<dim3((unsigned)blocks), 256, 0, (hipStream_t)stream>>>(mask, n, (unsigned long long)seed,
                                                                                (unsigned long long)salt, counter_dev, elem_offset / 8);
    return p2p_check_launch("p2p_dropout_mask_dev");
}
