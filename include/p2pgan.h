/*
 * p2pgan.h -- C ABI of libp2pgan_hip.so: the MI355X (gfx950) kernels behind the Pix2Pix side2side
 * training step of fegemo/palette-and-histo-gan.
 *
 * The reference has no FFI seam: its hot path bottoms out in TensorFlow/Keras ops called from Python
 * (SURVEY.md section 8b).  Each entry point below replaces the TF op(s) at the cited reference call
 * site; the Python host in palette_and_histo_gan_amd/ re-creates the reference class API
 * (Pix2PixModel.train_step etc.) on top of them through ctypes.
 *
 * Conventions (all entry points):
 *   - raw DEVICE pointers; the library never allocates or frees, workspaces are passed in;
 *   - tensors are NHWC "views" (p2p_tensor): a pointer to element (n=0,y=0,x=0,c=0) of the view plus
 *     pixel strides.  Activation buffers are allocated with a zero halo of 2 pixels around every image
 *     so kernels read the SAME-padding taps without bounds checks, and several views may alias one
 *     buffer with different channel offsets (concat-by-slice, networks.py:45,94);
 *   - dtype selects the storage/MFMA-input type of activations and weight copies: P2P_F32 (parity
 *     mode, exact-f32 MFMA) or P2P_BF16 (throughput mode, bf16 in / f32 accumulate).  Master weights,
 *     gradients, optimizer state, statistics and loss partials are always f32;
 *   - no entry point reads outside the pixels of the views it is given: where a tile row of an edge layer is wider than
 *     a pixel (4/8/36/33-channel tensors) the surplus slots re-read bytes of the same pixel.  What a view must provide is
 *     its zero halo: the stride-2 kernels gather rows/columns -1 .. 2*LH (hi) and -1 .. LH (lo) of every image, the
 *     stride-1 heads -1 .. H+1 (p2p_view_halo_pixels() = 2 pixels on every side covers all of them);
 *   - `stream` is a hipStream_t passed as void*; all work is stream-ordered, no hidden syncs;
 *   - return 0 on success, otherwise a hipError_t / negative argument-check code; the message is
 *     available from p2p_last_error() (thread-local).
 *
 * Stride-2 4x4 layers are described once by (hi, lo, W[16][Cg][Cd]):
 *   Conv2D          (networks.py:10-16): hi = input  (2LH x 2LW x Cg), lo = output, W = HWIO kernel
 *   Conv2DTranspose (networks.py:26-27): hi = output (2LH x 2LW x Cg), lo = input,  W = (kh,kw,Cout,Cin)
 * so the Keras layouts of both layer kinds are the same [tap][Cg][Cd] array and
 *   op G (hi -> lo): lo[n,y,x,d]  = sum_{kh,kw,g} hi[n,s*y+kh-1,s*x+kw-1,g] W[kh,kw,g,d]   conv fwd / convT dgrad
 *   op P (lo -> hi): hi[n,Y,X,g]  = sum_{Y=s*y+kh-1, X=s*x+kw-1, d} lo[n,y,x,d] W[kh,kw,g,d] convT fwd / conv dgrad
 *   op W           : dW[kh,kw,g,d] = sum_{n,y,x} hi[n,s*y+kh-1,s*x+kw-1,g] lo[n,y,x,d]     weight gradient
 * The stride-1 layers (networks.py:47-48,75-78; TF SAME pad 1 before / 2 after) use the same forms with s=1.
 */
#ifndef P2PGAN_H
#define P2PGAN_H

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { P2P_F32 = 0, P2P_BF16 = 1 } p2p_dtype;
typedef enum { P2P_OP_G = 0, P2P_OP_P = 1, P2P_OP_W = 2 } p2p_convop;
typedef enum { P2P_ACT_NONE = 0, P2P_ACT_LEAKY = 1, P2P_ACT_RELU = 2 } p2p_act;

typedef struct {
    void* ptr;            /* element (0,0,0,0) of the view */
    long long img_stride; /* pixels between images */
    int row_stride;       /* pixels between rows */
    int ld;               /* elements between pixels (channels of the underlying buffer) */
} p2p_tensor;

/* A gradient source read pointwise at (pixel, channel): kind 0 = absent, 1 = activation dtype,
 * 2 = f32, possibly `nslabs` split-K slabs `slab_stride` elements apart that are summed on load.
 * Dense [pixels][ld] layout, channel offset coff. */
typedef struct {
    const void* ptr;
    int kind;
    int nslabs;
    long long slab_stride;
    int ld;
    int coff;
} p2p_gsrc;

const char* p2p_last_error(void);
int p2p_version(void);
/* Zero halo (pixels on every side of every image) that the gathering kernels rely on; see Conventions. */
int p2p_view_halo_pixels(void);

/* ---- convolutions -------------------------------------------------------------------------- */

/* Direct (non-MFMA) 4x4 convolution, any channel counts, stride 1 or 2: the edge layers
 * (Cin 1..8, Cout 1..4; networks.py:46-48,57,75-78) and the on-device cross-check of the MFMA paths.
 * op G/P write the output view in `dtype`; op W writes f32 dW[16][Cg][Cd] (and dbias[Cd] if non-null,
 * = sum of lo).  `w` is the [16][Cg][Cd] weight copy in `dtype`; `bias` (f32[Cd], op G only) may be null. */
int p2p_conv_direct(int op, int stride, int dtype, int N, int LH, int LW, int Cg, int Cd,
                    const p2p_tensor* hi, const p2p_tensor* lo, const void* w, const float* bias,
                    float* dw, float* dbias, void* stream);

/* MFMA implicit-GEMM for the stride-2 blocks (networks.py:7-36), op G or P.
 * Requires Cg % 32 == 0 and Cd % 32 == 0.  `w` is Wt[16][Cd][Cg] for op G and Wn[16][Cg][Cd] for op P
 * (both produced by p2p_weight_prep).  The input view must carry the zero halo.  With splitk == 1 the
 * result is written to the output view in `dtype`; with splitk > 1 (a divisor of 16 for G, of 4 for P)
 * f32 partial slabs [splitk][pixels][Cout] are written to `slabs` and summed by the consumer
 * (p2p_norm_act_fwd / p2p_gsrc). */
int p2p_igemm(int op, int dtype, int N, int LH, int LW, int Cg, int Cd,
              const p2p_tensor* hi, const p2p_tensor* lo, const void* w,
              int splitk, float* slabs, float* stat_part, void* stream);
/* InstanceNorm statistics fused into the epilogue (splitk == 1): stat_part[N][slots][Cout][2] receives, per image and
 * slot, the mean and the centred sum of squares of an equal share of that image's output pixels;
 * slots = p2p_igemm_stat_slots(op, N, LH, LW, Cout) (0 = this shape cannot fuse them: pass stat_part = null and let
 * p2p_norm_act_fwd compute them).  p2p_norm_act_fwd consumes them with ws = stat_part, nsplit = -slots. */
int p2p_igemm_stat_slots(int op, int N, int LH, int LW, int ncols);

/* Block-resident form of p2p_igemm for the wide maps (bf16, LH == LW in {8,16,32,64}, splitk == 1; op P: Cd % 32 == 0 and
 * Cg % 64 == 0, op G: Cg % 16 == 0 and Cd % 256 == 0): a workgroup keeps the input block of 256 lo pixels (with halo) in
 * LDS, all taps / sub-pixel phases read it there and only the weights stream (csrc/brig.hip).  p2p_igemm takes this path
 * by itself whenever p2p_brig_ok says the shape qualifies (environment P2P_BRIG=0 keeps the im2col kernel);
 * p2p_igemm_layer_stat_slots is the statistics-slot query that matches the kernel p2p_igemm will use for the layer. */
int p2p_brig_ok(int op, int dtype, int N, int LH, int LW, int Cg, int Cd);
/* The whole block of networks.py:7-21 / 24-36 (without dropout) in ONE launch where a workgroup holds whole images (lo maps up
 * to 16x16): convolution, InstanceNorm statistics, normalisation and LeakyReLU / ReLU.  Writes the rounded convolution result
 * to the output view of the op (dense raw tensor: the backward pass reads it), (mean, rstd) to stats[N][Cout][2] and
 * act(gamma * (x - mean) * rstd + beta) into the (haloed, channel-sliced) view act_out.  p2p_igemm_norm_act_ok tells whether
 * the shape qualifies; otherwise p2p_igemm + p2p_norm_act_fwd do the same in two launches. */
int p2p_igemm_norm_act_ok(int op, int dtype, int N, int LH, int LW, int Cg, int Cd);
int p2p_igemm_norm_act(int op, int dtype, int N, int LH, int LW, int Cg, int Cd, const p2p_tensor* hi, const p2p_tensor* lo,
                       const void* w, const float* gamma, const float* beta, float eps, int act, float alpha,
                       const p2p_tensor* act_out, float* stats, void* stream);
int p2p_brig_stat_slots(int op, int dtype, int N, int LH, int LW, int Cg, int Cd);
int p2p_igemm_layer_stat_slots(int op, int dtype, int N, int LH, int LW, int Cg, int Cd);

/* Edge-layer form of the same kernel (Cin 1..8, the 36/33-channel concat, Cout 1..4; networks.py:46-48,57,75-78):
 * stride 1 or 2, any contraction width that fills whole 16-byte chunks (`cin_pad` = channels of the gathered
 * view as padded in HBM and in `w`), output columns masked to `ncols` (launched in 32-wide tiles; `w_rows`, a
 * multiple of 32 >= those tiles, = rows per tap slab of `w`), optional f32 bias[ncols] and LeakyReLU fused in
 * the epilogue.  `w` is [16][w_rows][cin_pad] in `dtype` (p2p_weight_prep_pad). */
int p2p_igemm_edge(int op, int stride, int dtype, int N, int LH, int LW, int cin_pad, int ncols, int w_rows,
                   const p2p_tensor* in, const p2p_tensor* out, const void* w, const float* bias,
                   int act, float alpha, void* stream);

/* LDS-strip form of p2p_igemm for the widest-map block (Cg == 32, Cd == 128, bf16: up6 forward = op P, its data gradient
 * = op G; networks.py:26-27,66-73): the input strip is staged once, the weights live in registers, the four waves split
 * the phases (op P) or the output channels (op G); persistent workgroups prefetch the next strip into registers.  Same
 * tensors and weight copies as p2p_igemm (wn for op P, wt for op G), no split-K.  op P optionally writes InstanceNorm
 * statistics like p2p_igemm: stat_part [N][slots][32][2] with slots = p2p_conv_strip_stat_slots (0 = not available).
 * p2p_conv_strip_ok tells whether the shape is supported. */
int p2p_conv_strip_ok(int op, int dtype, int N, int LH, int LW, int Cg, int Cd);
int p2p_conv_strip_stat_slots(int op, int dtype, int N, int LH, int LW, int Cg, int Cd);
int p2p_conv_strip(int op, int dtype, int N, int LH, int LW, int Cg, int Cd,
                   const p2p_tensor* hi, const p2p_tensor* lo, const void* w, float* stat_part, void* stream);

/* Few-output form (ncols <= 4, 32 < cin_pad <= 64; op G stride 1 or op P stride 2): the generator's 36 -> 4 head, the
 * discriminator's 64 -> 1 head and d(D first conv)/d(fake image) 64 -> 4 (networks.py:46,57,75-78).  Contracts the
 * channels first (rows = 16 taps x outputs, no padding of the 1..4 outputs to a 32-row tile, every input pixel read
 * once), then sums the 16 shifted taps out of LDS in a fixed order.  Same arguments and semantics as p2p_igemm_edge;
 * p2p_conv_fewout_ok tells whether the shape is supported. */
int p2p_conv_fewout_ok(int op, int stride, int dtype, int N, int LH, int LW, int cin_pad, int ncols);
int p2p_conv_fewout(int op, int stride, int dtype, int N, int LH, int LW, int cin_pad, int ncols, int w_rows,
                    const p2p_tensor* in, const p2p_tensor* out, const void* w, const float* bias,
                    int act, float alpha, void* stream);

/* Few-input form (cin_pad == 8: one 16-byte pixel, bf16 only; op G stride 1/2 or op P stride 1; ncols <= 64): the first
 * convolution of both networks and the data gradients of the two stride-1 heads (networks.py:10-16,45-46,57,75-78).
 * Weights live in registers, a strip of input rows in LDS, one MFMA K step = two taps, LDS-transposed 16-byte stores.
 * Same arguments and semantics as p2p_igemm_edge; p2p_conv_fewin_ok tells whether the shape is supported. */
int p2p_conv_fewin_ok(int op, int stride, int dtype, int N, int LH, int LW, int cin_pad, int ncols);
int p2p_conv_fewin(int op, int stride, int dtype, int N, int LH, int LW, int cin_pad, int ncols, int w_rows,
                   const p2p_tensor* in, const p2p_tensor* out, const void* w, const float* bias,
                   int act, float alpha, void* stream);

/* p2p_conv_fewin followed by the backward of the LeakyReLU in front of the layer, in one launch: out = conv(in) * (gate > 0 ?
 * 1 : alpha) with `gate` = the activation output of that block (same shape as out; whole 16-byte channel runs).  Bit-identical
 * to p2p_conv_fewin + p2p_act_bwd; the gradient tensor between them is never written (reference: the tape gradient through
 * the discriminator's first block, networks.py:45-48, pix2pix_model.py:78-79). */
int p2p_conv_fewin_actbwd(int op, int stride, int dtype, int N, int LH, int LW, int cin_pad, int ncols, int w_rows,
                          const p2p_tensor* in, const p2p_tensor* out, const void* w, const p2p_tensor* gate, float alpha,
                          void* stream);

/* MFMA weight gradient of a stride-2 block: dw[16][Cg][Cd] (f32) = sum over pixels.  The pixel sum is
 * split over `msplit` workgroups per tile; partial slabs go to `workspace`
 * (p2p_wgemm_workspace_bytes) and are reduced deterministically. */
long long p2p_wgemm_workspace_bytes(int N, int LH, int LW, int Cg, int Cd, int msplit);
int p2p_wgemm(int dtype, int N, int LH, int LW, int Cg, int Cd,
              const p2p_tensor* hi, const p2p_tensor* lo, float* dw,
              int msplit, void* workspace, void* stream);

/* Edge-layer form: stride 1 or 2, any Cg/Cd (store masked to the real counts); both views must have 16-byte
 * pixels (pad the channel count) and a zero halo. */
int p2p_wgemm_edge(int dtype, int stride, int N, int LH, int LW, int Cg, int Cd,
                   const p2p_tensor* hi, const p2p_tensor* lo, float* dw,
                   int msplit, void* workspace, void* stream);

/* LDS-resident form for the edge layers (Cg, Cd <= 64 with at most two 32x32 tiles, LW in {16,32,64}): every strip of
 * pixels is staged once and all 16 taps are contracted out of LDS, so HBM traffic = the algorithmic bytes.
 * p2p_wgrad_small_blocks returns the number of f32 slabs of 16*Cg*Cd floats the call needs in `workspace` (one partial
 * per workgroup plus the intermediate slabs of the two-level fixed-order sum), or 0 if the shape is not supported
 * (use p2p_wgemm_edge). */
int p2p_wgrad_small_blocks(int dtype, int stride, int N, int LH, int LW, int Cg, int Cd, int hi_ld, int lo_ld);
int p2p_wgrad_small(int dtype, int stride, int N, int LH, int LW, int Cg, int Cd,
                    const p2p_tensor* hi, const p2p_tensor* lo, float* dw, void* workspace, void* stream);

/* out[c] = sum over all pixels of v[n,y,x,c] (f32): bias gradients of the stride-1 heads.  One partial per workgroup and
 * channel goes to `workspace` (p2p_view_colsum_workspace_bytes), the partials are added in workgroup order: bit-reproducible. */
long long p2p_view_colsum_workspace_bytes(int dtype, int N, int H, int W, int C, const p2p_tensor* v);
int p2p_view_colsum(int dtype, int N, int H, int W, int C, const p2p_tensor* v, float* out, float* workspace, void* stream);

/* ---- route queries: which kernel a launcher would start -------------------------------------- */

/* The launchers above and p2p_norm_act_fwd / _bwd below choose among template instantiations and kernel forms from their
 * arguments and from A/B switches read once per process from the environment (README, "Tuning / A-B switches").  Each query
 * here takes the launch's arguments (views need their geometry only; pointers their null-ness and 16-byte alignment), calls
 * the SAME decision function as its launcher, starts nothing and needs no GPU.  It returns a small code composed by the macro
 * next to it, or -1 where the launcher would refuse the arguments.  The P2P_*_ARMS lists name every arm the launchers'
 * dispatch has, as X(fields of the macro): tests/test_switch_routes_cpu.py requires each to be run by a GPU test or named
 * unreachable with a reason. */

/* p2p_igemm (p2p_igemm_route; P2P_IGEMM_ROUTE_BRIG: the block-resident kernel takes the layer, see p2p_brig_route) and
 * p2p_igemm_edge: kernel family, BM x BN tile, K groups per tile, LDS stages, block order (w_major: blocks that share a
 * weight tile are neighbours). */
#define P2P_IGEMM_FAM_R03 1      /* igemm_kernel<GEN = false>: power-of-two K bytes, no bias / activation / column mask */
#define P2P_IGEMM_FAM_GEN 2      /* igemm_kernel<GEN = true> */
#define P2P_IGEMM_FAM_PIPE_G 3   /* igemm_pipe_kernel<MODE 0>: software-pipelined, op G */
#define P2P_IGEMM_FAM_PIPE_P 4   /* igemm_pipe_kernel<MODE 1>: op P */
#define P2P_IGEMM_TILE_128x128 0
#define P2P_IGEMM_TILE_256x128 1
#define P2P_IGEMM_TILE_128x64 2
#define P2P_IGEMM_TILE_256x64 3
#define P2P_IGEMM_TILE_128x32 4
#define P2P_IGEMM_TILE_256x32 5
#define P2P_IGEMM_ROUTE(family, tile, kgroups, stages, w_major) \
    ((family) | ((tile) << 3) | (((kgroups) - 1) << 6) | (((stages) - 2) << 7) | ((w_major) << 9))
#define P2P_IGEMM_ROUTE_BRIG 0
/* X(family, tile, K groups, stages); every arm exists with w_major 0 and 1 */
#define P2P_IGEMM_ARMS(X) \
    X(1, 0, 1, 2) X(1, 0, 1, 3) X(1, 1, 1, 2) X(1, 1, 1, 3) X(1, 2, 1, 2) X(1, 2, 1, 3) \
    X(1, 3, 1, 2) X(1, 3, 1, 3) X(1, 4, 1, 2) X(1, 4, 1, 3) X(1, 5, 1, 2) X(1, 5, 1, 3) \
    X(2, 0, 1, 2) X(2, 0, 1, 3) X(2, 1, 1, 2) X(2, 1, 1, 3) X(2, 2, 1, 2) X(2, 2, 1, 3) \
    X(2, 3, 1, 2) X(2, 3, 1, 3) X(2, 4, 1, 2) X(2, 4, 1, 3) X(2, 5, 1, 2) X(2, 5, 1, 3) \
    X(3, 1, 1, 3) X(3, 0, 2, 4) X(3, 0, 1, 2) X(4, 1, 1, 3) X(4, 0, 2, 4) X(4, 0, 1, 2)
int p2p_igemm_route(int op, int dtype, int N, int LH, int LW, int Cg, int Cd, const p2p_tensor* hi, const p2p_tensor* lo,
                    int splitk, int with_stats);
int p2p_igemm_edge_route(int op, int stride, int dtype, int N, int LH, int LW, int cin_pad, int ncols, int w_rows,
                         const p2p_tensor* in, const p2p_tensor* out, int with_bias, int act);

/* brig_launch, through p2p_igemm (fused 0) or p2p_igemm_norm_act (fused 1): op, output channels per wave (cbw 1: 32, 2: 64),
 * DMA issue order of waves 4-7 (stagger), fused InstanceNorm + activation epilogue.  P2P_BRIG_ROUTE_NONE: the kernel (fused 1:
 * its fused epilogue) is not offered for the shape. */
#define P2P_BRIG_ROUTE(op_p, cbw, stagger, fused) (1 | ((op_p) << 1) | (((cbw) - 1) << 2) | ((stagger) << 3) | ((fused) << 4))
#define P2P_BRIG_ROUTE_NONE 0
/* X(op P, cbw, stagger, fused) */
#define P2P_BRIG_ARMS(X) \
    X(0, 1, 0, 0) X(0, 1, 0, 1) X(0, 1, 1, 0) X(0, 1, 1, 1) X(0, 2, 0, 0) X(0, 2, 0, 1) X(0, 2, 1, 0) X(0, 2, 1, 1) \
    X(1, 1, 0, 0) X(1, 1, 0, 1) X(1, 1, 1, 0) X(1, 1, 1, 1) X(1, 2, 0, 0) X(1, 2, 0, 1) X(1, 2, 1, 0) X(1, 2, 1, 1)
int p2p_brig_route(int op, int dtype, int N, int LH, int LW, int Cg, int Cd, int fused);

/* p2p_wgemm / p2p_wgemm_edge: the software-pipelined bf16 kernel, or wgemm_kernel on a BG x BD tile */
#define P2P_WGEMM_ROUTE_PIPE 0
#define P2P_WGEMM_ROUTE_128x128 1
#define P2P_WGEMM_ROUTE_64x128 2
#define P2P_WGEMM_ROUTE_32x128 3
#define P2P_WGEMM_ROUTE_64x64 4
#define P2P_WGEMM_ROUTE_32x64 5
#define P2P_WGEMM_ROUTE_64x32 6
#define P2P_WGEMM_ROUTE_32x32 7
#define P2P_WGEMM_ARMS(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7)
int p2p_wgemm_route(int dtype, int stride, int N, int LH, int LW, int Cg, int Cd, const p2p_tensor* hi, const p2p_tensor* lo,
                    int msplit);

/* p2p_wgrad_small: stride, GT x DT window of 32x32 tiles, waves per workgroup (16: one tap each, 8: two taps each), packing of
 * few-channel pixels (0 none, 1 the hi side, 2 the lo side), bank swizzle of the transposing LDS reads (1: a mask is in force on
 * either side) */
#define P2P_WS_TILE_1x1 0
#define P2P_WS_TILE_1x2 1
#define P2P_WS_TILE_1x4 2
#define P2P_WS_TILE_2x1 3
#define P2P_WS_TILE_2x2 4
#define P2P_WS_ROUTE(stride, tile, waves, pack, swizzle) \
    (((stride) - 1) | ((tile) << 1) | (((waves) >> 4) << 4) | ((pack) << 5) | ((swizzle) << 7))
/* X(stride, tile, waves, pack, swizzle): unpacked windows in both wave counts with and without the swizzle; packed layers (8 waves,
 * no swizzle): pack 1 on the 1x2 window, pack 2 on the 2x1 window at stride 1 */
#define P2P_WS_ARMS(X) \
    X(1, 0, 8, 0, 0) X(1, 0, 8, 0, 1) X(1, 0, 16, 0, 0) X(1, 0, 16, 0, 1) X(1, 1, 8, 0, 0) X(1, 1, 8, 0, 1) X(1, 1, 16, 0, 0) X(1, 1, 16, 0, 1) \
    X(1, 2, 8, 0, 0) X(1, 2, 8, 0, 1) X(1, 2, 16, 0, 0) X(1, 2, 16, 0, 1) X(1, 3, 8, 0, 0) X(1, 3, 8, 0, 1) X(1, 3, 16, 0, 0) X(1, 3, 16, 0, 1) \
    X(1, 4, 8, 0, 0) X(1, 4, 8, 0, 1) X(1, 4, 16, 0, 0) X(1, 4, 16, 0, 1) \
    X(2, 0, 8, 0, 0) X(2, 0, 8, 0, 1) X(2, 0, 16, 0, 0) X(2, 0, 16, 0, 1) X(2, 1, 8, 0, 0) X(2, 1, 8, 0, 1) X(2, 1, 16, 0, 0) X(2, 1, 16, 0, 1) \
    X(2, 2, 8, 0, 0) X(2, 2, 8, 0, 1) X(2, 2, 16, 0, 0) X(2, 2, 16, 0, 1) X(2, 3, 8, 0, 0) X(2, 3, 8, 0, 1) X(2, 3, 16, 0, 0) X(2, 3, 16, 0, 1) \
    X(2, 4, 8, 0, 0) X(2, 4, 8, 0, 1) X(2, 4, 16, 0, 0) X(2, 4, 16, 0, 1) \
    X(1, 1, 8, 1, 0) X(2, 1, 8, 1, 0) X(1, 3, 8, 2, 0)
int p2p_wgrad_small_route(int dtype, int stride, int N, int LH, int LW, int Cg, int Cd, int hi_ld, int lo_ld);

/* p2p_norm_act_fwd / _fwd_tail / _bwd: the form (lane groups on maps of <= 16 pixels; register-resident; the workgroup forms:
 * one pass, statistics pass + apply pass over a pixel split, apply-only over statistics slots of a conv epilogue; the scalar
 * kernel), pixels per thread of the small / register forms, the f32-slab loader instantiation (forward: raw_kind 2, backward:
 * a gradient source of kind 2) and log2 of the channel group (a launch argument, not an instantiation: P2P_NORM_ROUTE_ARM
 * strips it). */
#define P2P_NORM_FORM_SCALAR 0
#define P2P_NORM_FORM_SMALL 1
#define P2P_NORM_FORM_REG 2
#define P2P_NORM_FORM_VEC0 3
#define P2P_NORM_FORM_VEC12 4
#define P2P_NORM_FORM_VEC3 5
#define P2P_NORM_ROUTE(form, ppl, slabs, lg_cg) ((form) | ((ppl) << 3) | ((slabs) << 7) | ((lg_cg) << 8))
#define P2P_NORM_ROUTE_ARM(code) ((code) & 0xff)
/* X(form, pixels per thread, slab loader) */
#define P2P_NORM_FWD_ARMS(X) \
    X(0, 0, 0) X(1, 1, 0) X(1, 1, 1) X(1, 2, 0) X(1, 2, 1) X(1, 4, 0) X(1, 4, 1) \
    X(2, 1, 0) X(2, 1, 1) X(2, 2, 0) X(2, 2, 1) X(2, 4, 0) X(2, 4, 1) X(2, 8, 0) X(2, 8, 1) X(3, 0, 0) X(4, 0, 0) X(5, 0, 0)
#define P2P_NORM_BWD_ARMS(X) \
    X(0, 0, 0) X(1, 1, 0) X(1, 1, 1) X(1, 2, 0) X(1, 2, 1) X(1, 4, 0) X(1, 4, 1) \
    X(2, 1, 0) X(2, 1, 1) X(2, 2, 0) X(2, 2, 1) X(2, 4, 0) X(2, 4, 1) X(2, 8, 0) X(2, 8, 1) X(3, 0, 0) X(4, 0, 0)
int p2p_norm_act_fwd_route(int dtype, int N, int H, int W, int C, const void* raw, int raw_kind, int nslabs,
                           long long slab_stride, const float* gamma, const float* beta, const p2p_tensor* out,
                           void* raw_out, float* stats, float* ws, long long ws_bytes, int nsplit,
                           const p2p_tensor* tail, int tail_ch);
int p2p_norm_act_bwd_route(int dtype, int N, int H, int W, int C, const void* raw, const float* stats, const float* gamma,
                           const float* beta, const p2p_gsrc* g1, const p2p_gsrc* g2, const p2p_tensor* draw,
                           float* dgamma_part, float* dbeta_part, float* ws, long long ws_bytes, int nsplit);

/* ---- InstanceNorm + activation + dropout (networks.py:18-19,29-34), fused ---------------------- */

/* raw: conv output, dense [N*H*W][C]; raw_kind 1 = `dtype`, 2 = f32 with nslabs split-K slabs.
 * gamma/beta null => no normalisation (down1, D.down: networks.py:46,58).
 * y = act(drop(gamma*(x-mu)*rsqrt(var+eps)+beta)), dropout keep-mask `mask` (u8 dense [N*H*W][C], may be
 * null) scales kept values by 2.  Writes y into the (haloed, possibly channel-sliced) view `out`,
 * mean/rstd into stats[N][C][2] and, if raw_out != null, the summed raw tensor in `dtype`.
 * nsplit > 1 splits every image's pixel range over nsplit workgroups (two launches: partial sums to the f32
 * workspace ws, >= N*nsplit*C*2*4 bytes, then apply); nsplit in {0, 1} or ws == null = one launch;
 * nsplit < 0: ws holds -nsplit statistics slots per image written by p2p_igemm's epilogue (apply only). */
int p2p_norm_act_fwd(int dtype, int N, int H, int W, int C,
                     const void* raw, int raw_kind, int nslabs, long long slab_stride,
                     const float* gamma, const float* beta, float eps, int act, float alpha,
                     const unsigned char* mask, const p2p_tensor* out, void* raw_out, float* stats,
                     float* ws, long long ws_bytes, int nsplit, void* stream);
/* As p2p_norm_act_fwd, and copies tail_ch channels per pixel from the view `tail` (same N, H, W) into the channels that
 * FOLLOW this layer's C channels in `out`: the last concat of the generator is [up6 | input image] (networks.py:92-94) and
 * written this way every pixel of the concat buffer leaves one wave complete (no partial 32-byte sectors: the separate
 * copy cost 41 of 71 us with cold caches).  Workgroup (vector) form only: H*W > 16, C % 8 == 0, tail_ch whole 16-byte vectors. */
int p2p_norm_act_fwd_tail(int dtype, int N, int H, int W, int C,
                          const void* raw, int raw_kind, int nslabs, long long slab_stride,
                          const float* gamma, const float* beta, float eps, int act, float alpha,
                          const unsigned char* mask, const p2p_tensor* out, void* raw_out, float* stats,
                          float* ws, long long ws_bytes, int nsplit, const p2p_tensor* tail, int tail_ch, void* stream);

/* Backward of the fused block: dact = g1 + g2 (pointwise gradient sources), through dropout/activation
 * (sign recomputed from raw+stats) and the InstanceNorm closed form.  Writes d(raw)
 * into the haloed view `draw` and per-image partials dgamma_part/dbeta_part [N][C] (f32).  ws/nsplit as above;
 * maps of up to 64x64 pixels whose (image, channel group) slice fits a workgroup's registers take one launch that
 * reads every operand once, whatever nsplit says (the same holds for p2p_norm_act_fwd without conv-epilogue statistics).
 * nsplit | 0x100 (nsplit > 0, forward and backward): the two-pass forms only, whose order of the per-channel sums does
 * not depend on N -- an image's result then does not depend on the batch it sits in (the engine's f32 parity mode);
 * nsplit | 0x200: the one-launch forms with the geometry they would pick for N = 256 (wide channel groups, several
 * pixels per thread), so that tests reach those variants with a small batch. */
int p2p_norm_act_bwd(int dtype, int N, int H, int W, int C,
                     const void* raw, const float* stats, const float* gamma, const float* beta,
                     int act, float alpha, const unsigned char* mask,
                     const p2p_gsrc* g1, const p2p_gsrc* g2,
                     const p2p_tensor* draw, float* dgamma_part, float* dbeta_part,
                     float* ws, long long ws_bytes, int nsplit, void* stream);

/* InstanceNorm block over a 1x1 map (H = W = 1; the generator's bottleneck at 64x64 inputs).  x - mean(x) is 0 over one pixel,
 * so the output is act(drop(0 * gamma + beta)) whatever the convolution produced, d(raw) and dgamma are 0 and dbeta_part is
 * d(yhat) = (g1 + g2) * slope * keep.  The forward form reads no convolution result and writes no statistics, the backward form
 * reads neither and writes no d(raw); out, dbeta_part and dgamma_part (= 0) are bit-identical to p2p_norm_act_fwd /
 * p2p_norm_act_bwd at H = W = 1 (mask, views and gradient sources as there).  C % 8 == 0 and 16-byte aligned pixels. */
int p2p_norm_act_fwd_1x1(int dtype, int N, int C, const float* gamma, const float* beta, int act, float alpha,
                         const unsigned char* mask, const p2p_tensor* out, void* stream);
int p2p_norm_act_bwd_1x1(int dtype, int N, int C, const float* gamma, const float* beta, int act, float alpha,
                         const unsigned char* mask, const p2p_gsrc* g1, const p2p_gsrc* g2, float* dgamma_part,
                         float* dbeta_part, void* stream);

/* Backward of a LeakyReLU that was fused into a conv epilogue (only its OUTPUT is stored):
 * draw = (g1 + g2) * (act_out > 0 ? 1 : alpha). */
int p2p_act_bwd(int dtype, int N, int H, int W, int C, const p2p_tensor* act_out, const p2p_gsrc* g1,
                const p2p_gsrc* g2, float alpha, const p2p_tensor* draw, void* stream);

/* out[c] = scale * sum_r part[r][c] (f32): batch reduction of dgamma/dbeta partials, loss partials. */
int p2p_colsum(const float* part, int rows, int cols, float scale, float* out, void* stream);

/* Batched form: task t sums the dense [rows][cols] block at part + table[t][0] over rows into out + table[t][3];
 * table = device int32[ntasks][4] = {part_off, rows, cols, out_off}.  One launch reduces the dgamma/dbeta
 * partials of every InstanceNorm layer of a backward pass. */
int p2p_colsum_batched(const float* part, const int* table, int ntasks, int max_cols, float* out, void* stream);

/* ---- losses (pix2pix_model.py:44-56) ------------------------------------------------------------ */

/* Loss sums are deterministic: the loss kernels launch P2P_LOSS_BLOCKS workgroups and write one partial per workgroup
 * and loss term, partials[k * P2P_LOSS_BLOCKS + b]; p2p_loss_partials_sum adds K consecutive rows in workgroup order,
 * out[k] = sum_b partials[k * P2P_LOSS_BLOCKS + b] (one launch for all loss terms of a step). */
#define P2P_LOSS_BLOCKS 256
int p2p_loss_partials_sum(const float* partials, int K, float* out, void* stream);

/* logits: view [N2][H][W][1]; images [0,n_real) are D(real), the rest D(fake).
 * partials rows 0..2 = BCE(1,real), BCE(0,fake), BCE(1,fake) scaled by inv_count.
 * dlogits_d (all N2 images): d(real+fake loss)/dlogit; dlogits_g (fake images only): d(adv)/dlogit. */
int p2p_bce_logits(int dtype, int N2, int n_real, int H, int W, const p2p_tensor* logits,
                   float inv_count, const p2p_tensor* dlogits_d, const p2p_tensor* dlogits_g,
                   float* partials, void* stream);
/* As p2p_bce_logits for gradient views of 8-channel pixels [g | 7 padding channels] (the operand layout of the few-channel
 * convolution kernels): whole pixels are stored -- a 2-byte store into a 16-byte pixel is a partial sector write. */
int p2p_bce_logits_pad8(int dtype, int N2, int n_real, int H, int W, const p2p_tensor* logits,
                        float inv_count, const p2p_tensor* dlogits_d, const p2p_tensor* dlogits_g,
                        float* partials, void* stream);

/* fake = tanh(z) written to `fake` view; partials row 0 = inv_count * sum |real - fake| over all C channels.
 * fake_f32 (may be null): dense f32 [N*H*W][C] copy of tanh(z) before rounding to `dtype` -- the histogram loss reads its
 * images in f32 in every mode (log-chroma of dark colours does not survive 8 significant bits). */
int p2p_tanh_l1_fwd(int dtype, int N, int H, int W, int C, const p2p_tensor* z, const p2p_tensor* real,
                    const p2p_tensor* fake, float inv_count, float* partials, float* fake_f32, void* stream);
/* The train step's form for 4-channel images whose discriminator inputs are 8-channel pixels [image | source]
 * (networks.py:45): real_pair = [target | source] is read whole and the WHOLE fake pixel [tanh(z) | source] is written. */
int p2p_tanh_l1_fwd_pair(int dtype, int N, int H, int W, const p2p_tensor* z, const p2p_tensor* real_pair,
                         const p2p_tensor* fake_pair, float inv_count, float* partials, float* fake_f32, void* stream);

/* dz = (g_d + g_extra + lambda_l1*inv_count*sign(fake-real)) * (1 - fake^2) into the haloed view dz. */
int p2p_tanh_l1_bwd(int dtype, int N, int H, int W, int C, const p2p_tensor* fake, const p2p_tensor* real,
                    const p2p_gsrc* g_d, const p2p_gsrc* g_extra, float l1_scale,
                    const p2p_tensor* dz, void* stream);
/* As p2p_tanh_l1_bwd (C = 4) for a dz view of 8-channel pixels [dz | 4 padding channels]: whole-pixel stores. */
int p2p_tanh_l1_bwd_pad8(int dtype, int N, int H, int W, const p2p_tensor* fake, const p2p_tensor* real,
                         const p2p_gsrc* g_d, const p2p_gsrc* g_extra, float l1_scale, const p2p_tensor* dz,
                         void* stream);

/* ---- RGB-uv histogram + Hellinger loss (histogram.py:4-89, pix2pix_model.py:242-250) ------------------------- */

/* The histogram entry points take `dtype` = the element type of the IMAGE view they read; the engine always hands them f32
 * views (the f32 input batch for the real image, p2p_tanh_l1_fwd's fake_f32 for the generated one), also in bf16 mode.
 * Raw (unnormalised) histogram of the RGB channels of `img` ([-1,1] images): hist[N][3][64][64] f32 with
 * hist[n][c][i][j] = sum_p Iy[p] k(u_p - d_i) k(v_p - d_j) for component c (the reference's (B,64,64,3) tensor
 * transposed and before its division by the per-image total, histogram.py:75-79). */
int p2p_rgbuv_hist_fwd(int dtype, int N, int H, int W, const p2p_tensor* img, float* hist, void* stream);
/* The same with the reference function's other arguments (histogram.py:36): hist[N][3][size][size], size 2..128, bin centres
 * linspace(-3, 3, size), method 0 = "inverse-quadratic", 1 = "RBF", 2 = any other string (the reference then applies no kernel
 * function: histogram.py:20-27 has no third branch), sigma > 0.  General f32 kernel for evaluation code; no reference call site
 * leaves the defaults, which the specialised kernels serve. */
int p2p_rgbuv_hist_general(int dtype, int N, int H, int W, const p2p_tensor* img, int size, int method, float sigma, float* hist,
                           void* stream);

/* The same raw histograms [N][3][64][64], all three colour components of an image from THREE shared kernel rows per pixel
 * (the components' (u, v) are (a, b), (-a, c), (-b, -c) of three log-chroma differences and the bin grid is symmetric,
 * histogram.py:54-55,72-74), contracted over the image's pixels or -- where `points`/`npoints` (p2p_rgbuv_points) list them
 * -- over its DISTINCT colours weighted by their pixel counts (identical up to f32 summation order).  workspace:
 * p2p_rgbuv_hist_fwd3_workspace_bytes(N) bytes (partial histograms of the pixel ranges, summed in fixed order). */
long long p2p_rgbuv_hist_fwd3_workspace_bytes(int N);
int p2p_rgbuv_hist_fwd3(int dtype, int N, int H, int W, const p2p_tensor* img, const float* points, const int* npoints, int cap,
                        float* hist, float* workspace, void* stream);
/* Distinct colours of every image with their pixel counts: points[n][k] = (r, g, b, count) for k < npoints[n], in order of
 * first appearance within tiles of 1024 pixels (bitwise equality of the f32 / bf16 RGB values; colours of different tiles
 * are not merged).  npoints[n] = -1 where the list would exceed `cap` entries (the image is then contracted densely).
 * Deterministic (integer LDS atomics only).  points: f32 [N][cap][4], 16-byte aligned. */
int p2p_rgbuv_points(int dtype, int N, int H, int W, const p2p_tensor* img, int cap, float* points, int* npoints, void* stream);

/* out[N][64][64][3] = raw[N][3][64][64] transposed and divided by the per-image total (histogram.py:75-79). */
int p2p_hist_normalize(const float* raw, int N, float* out, void* stream);

/* Per-image totals of both raw histograms and the LOCAL Hellinger sum of squares
 * sq_sum[0] = sum_{n,c,i,j} (sqrt(pred/tot_pred) - sqrt(true/tot_true))^2 (histogram.py:88-89): one partial per image in
 * sq_part[N], added in image order (bit-reproducible, no float atomics).  Under data parallelism sq_sum is all-reduced
 * (SUM) before the two calls below. */
int p2p_hellinger_fwd(const float* hist_true, const float* hist_pred, int N, float* tot_true, float* tot_pred,
                      float* sq_part, float* sq_sum, void* stream);
/* loss_out[0] = sqrt(sq_sum) / (sqrt(2) * B_global). */
int p2p_hellinger_finish(const float* sq_sum, float inv_global_batch, float* loss_out, void* stream);
/* d(coef' * hellinger)/d(fake image) with coef = lambda_hist / (2*sqrt(2)*B_global): writes three f32 slabs
 * dimg[3][N*H*W][4] (one per colour component, alpha gradient 0) that the consumer sums; gh_ws is a
 * [N][3][64][64] f32 workspace. */
int p2p_rgbuv_hist_hellinger_bwd(int dtype, int N, int H, int W, const p2p_tensor* fake, const float* hist_true,
                                 const float* hist_pred, const float* tot_true, const float* tot_pred,
                                 const float* sq_sum, float coef, float* gh_ws, float* dimg, void* stream);
/* The same gradient, the three colour components evaluated together from three shared kernel rows per pixel and summed in
 * the kernel: ONE f32 slab [N*H*W][4] is written to `dimg` (consumer: p2p_tanh_l1_bwd with a one-slab gradient source). */
int p2p_rgbuv_hist_hellinger_bwd3(int dtype, int N, int H, int W, const p2p_tensor* fake, const float* hist_true,
                                  const float* hist_pred, const float* tot_true, const float* tot_pred, const float* sq_sum,
                                  float coef, float* gh_ws, float* dimg, void* stream);

/* Backward of the standalone histogram (histogram.calculate_rgbuv_histogram under torch autograd), in two steps.
 * 1. The normalisation and transpose: raw[N][3][size][size] as the forward kernels write it, grad_out = dL/d(normalised
 *    histogram) in the reference's [N][size][size][3] layout, size 2..128; with T_n = sum raw_n and Hn = raw / T:
 *    gh[n][c][i][j] = (grad_out[n][i][j][c] - sum_{c,i,j} grad_out[n] * Hn[n]) / T_n   (one workgroup per image, fixed order). */
int p2p_hist_normalize_bwd(const float* raw, const float* grad_out, int N, int size, float* gh, void* stream);
/* 2. d(sum gh * raw)/d(img) for an ARBITRARY raw-histogram gradient gh[N][3][64][64] at the reference's arguments (64 bins,
 *    inverse-quadratic, sigma 0.02): the kernel of p2p_rgbuv_hist_hellinger_bwd3 without its Hellinger prep.  Writes ONE f32
 *    slab dimg[N*H*W][4] (alpha gradient 0), 16-byte aligned. */
int p2p_rgbuv_hist_bwd(int dtype, int N, int H, int W, const p2p_tensor* img, const float* gh, float* dimg, void* stream);
/*    The same for p2p_rgbuv_hist_general's arguments (size 2..128, method 0..2, sigma > 0; same codes): gh[N][3][size][size],
 *    dimg[N*H*W][4] f32, the three components summed in the kernel.  Deterministic: every pixel is reduced by a fixed set of
 *    lanes in a fixed order (no float atomics).  f32 vector arithmetic, for evaluation code. */
int p2p_rgbuv_hist_general_bwd(int dtype, int N, int H, int W, const p2p_tensor* img, int size, int method, float sigma,
                               const float* gh, float* dimg, void* stream);

/* ---- soft palette histogram and conformance (build-added, DESIGN.md "palette loss") ------------------------------ */
/* f32 only; img: dense [N][H][W][4] in [-1, 1], 16-byte aligned, any H, W >= 1 (H * W <= 2^30, N <= 65535).  palette: int32
 * [N][K][4] RGBA rows in 0..255, 16-byte aligned, K <= 256; sizes[n] = valid slots of image n (clamped to K; <= 0: the image
 * contributes zeros).  With x_p = img_p * 0.5 + 0.5 (all four channels), c_k = palette[n][k] / 255 and tau > 0:
 *   d_pk = sum_c (x_pc - c_kc)^2,   w_pk = exp(-(d_pk - min_j d_pj) / tau) / sum_j exp(-(d_pj - min_j d_pj) / tau)   (j, k < sizes[n])
 *   hist[n][k] = (1 / HW) sum_p w_pk   (0 for k >= sizes[n]),      conf[n] = (1 / HW) sum_p sum_k w_pk d_pk.
 * workspace: p2p_soft_palette_workspace_bytes(N, H, W) bytes of per-workgroup partial sums, added in workgroup order (no float
 * atomics: bit-reproducible). */
long long p2p_soft_palette_workspace_bytes(int N, int H, int W);
int p2p_soft_palette_fwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau,
                         float* hist, float* conf, float* workspace, void* stream);
/* Its VJP for upstream gradients gh[N][K] and gm[N] (the weights are recomputed): with a_k = (gh_k + gm d_pk) / HW,
 *   dL/dx_p = (2 / tau) sum_k w_pk (a_k - sum_j w_pj a_j) c_k + (2 gm / HW) (x_p - sum_k w_pk c_k),   dimg = 0.5 dL/dx,
 * alpha included; dimg: dense f32 [N][H][W][4], 16-byte aligned, every pixel written.  The weighted differences are taken about
 * the pixel's nearest slot, so they do not cancel where one colour dominates. */
int p2p_soft_palette_bwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau,
                         const float* gh, const float* gm, float* dimg, void* stream);
/* The same VJP for the loss of the fused palette step, with the upstream gradient formed in the kernel from the two histograms
 * h_real[N][K] and h_fake[N][K] (what p2p_soft_palette_fwd wrote) instead of read from a table:
 *   gh[n][k] = w_tv * sgn(h_fake[n][k] - h_real[n][k]) for k < sizes[n] (sgn 0 = 0), 0 beyond;   gm[n] = w_conf.
 * Equals p2p_soft_palette_bwd handed that table bit for bit (one kernel body). */
int p2p_soft_palette_tv_bwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau,
                            const float* h_real, const float* h_fake, float w_tv, float w_conf, float* dimg, void* stream);
/* The two loss values of B images from their soft histograms and conformances (f32, dense; K <= 256):
 *   tv_b = 0.5 sum_{k < min(sizes[b], K)} |h_fake[b][k] - h_real[b][k]|, added in ascending k (0 for sizes[b] <= 0),
 *   out_tv[0] = inv_batch * sum_b tv_b,   out_conf[0] = inv_batch * sum_{b: sizes[b] > 0} conf_fake[b], added in ascending b.
 * With inv_batch = 1 / global batch a rank writes its own images' share of the two batch means: the SUM over the ranks is the
 * global value.  One workgroup, fixed-order sums, no float atomics: bit-reproducible, and an image's term does not depend on B. */
int p2p_palette_loss(int B, int K, const float* h_real, const float* h_fake, const float* conf_fake, const int* sizes,
                     float inv_batch, float* out_tv, float* out_conf, void* stream);
/* Palette of every image: q = clamp(floor((img * 0.5 + 0.5) * 255 + 0.5), 0, 255) per channel (each step rounded to f32), key =
 * r + 256 g + 65536 b + 2^24 a (unsigned); palette_out[n][0 .. sizes_out[n]) = the image's distinct keys in ascending order
 * (transparent black first), unpacked to int32 RGBA, remaining rows 0.  More than `cap` (1..256) distinct colours:
 * sizes_out[n] = -1 and a zeroed row.  One workgroup per image (LDS hash set, integer atomics, bounded probing). */
int p2p_palette_extract(int N, int H, int W, const float* img, int cap, int* palette_out, int* sizes_out, void* stream);
/* Nearest palette slot of every pixel, in integers (DESIGN.md "palette snap").  img, palette, sizes as for the soft histogram.
 * With q_p the pixel quantised per channel as p2p_palette_extract quantises it (NaN -> 0) and n = clamp(sizes[n], 0, K):
 *   D_pk = sum_c (q_pc - palette[k][c])^2 (0..260100),   index_out[p] = argmin_{k < n} D_pk (ties: the lowest k),
 *   dist_out[p] = D_p,index,   image_out[p] = palette[index] / 127.5f - 1.0f (two f32 operations; 16-byte aligned),
 *   counts_out[n][k] = #{p : index = k} (0 for k >= n),   stats_out[n] = { #{p : dist > 0}, sum_p dist }.
 * n = 0: index -1, dist 0, image_out = img bit for bit, counts and stats 0.  image_out and dist_out may be NULL; every element of
 * every other output is written (the call clears counts_out and stats_out itself; integer atomics across workgroups, so two calls
 * give identical bits).  No workspace, no allocation. */
int p2p_palette_snap(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, int* index_out,
                     float* image_out, int* dist_out, int* counts_out, long long* stats_out, void* stream);
/* A palette of at most `colours` colours for every image, derived from the image itself by an integer k-means.
 * img: dense f32 [N][H][W][4] in [-1, 1], 16-byte aligned; palette_out: int32 [N][K][4], 16-byte aligned; sizes_out: int32 [N];
 * iters_out: int32 [N] or NULL; init_palette int32 [N][K][4] (16-byte aligned) and init_sizes int32 [N]: both given or both NULL.
 * 1 <= colours <= K <= 256, 0 <= iterations <= 64, H * W <= 2^14 (128 x 128: an image's keys stay in LDS; larger maps are refused);
 * anything else returns a negative code and sets p2p_last_error before any launch.  Per image n, with
 * D(a, b) = sum_c (a_c - b_c)^2 over the four channels, in integers:
 *   0. q_p = the pixel quantised as p2p_palette_extract / p2p_palette_snap quantise it (NaN -> 0), key = r + 256 g + 65536 b + 2^24 a,
 *      U = the set of distinct keys of the image.
 *   1. |U| <= colours: palette_out = the colours of U in ascending key order, sizes_out = |U|, iters_out = 0 -- the bits
 *      p2p_palette_extract writes with cap = K -- whether or not an initial palette was given.
 *   2. Starting slots C[0 .. m).  With n0 = clamp(init_sizes[n], 0, K) > 0: m = min(n0, colours), C[k] = init_palette[n][k] & 255 per
 *      channel (duplicate rows allowed).  Otherwise m = colours by farthest-point selection: C[0] = the colour of the smallest key
 *      of U; for j = 1 .. m-1 with m_p = min_{i<j} D(q_p, C[i]): C[j] = the colour of a pixel that maximises m_p, among equal maxima
 *      the one with the lowest key (|U| > colours: every maximum is > 0 and the C[j] are distinct).
 *   3. Lloyd passes t = 1 .. iterations: a_p = argmin_{k<m} D(q_p, C[k]), ties to the lowest k (p2p_palette_snap's rule, same device
 *      code); n_k = #{p : a_p = k}, S_kc = sum_{a_p = k} q_pc; C'[k][c] = floor((2 S_kc + n_k) / (2 n_k)) if n_k > 0, a slot without
 *      pixels keeps its colour; C' = C stops.  iters_out = the number of assignment passes made up to and including the one that
 *      found the fixed point (`iterations` if none did, 0 for iterations = 0).
 *   4. palette_out = the distinct keys of the final C in ascending order, unpacked to int32 RGBA rows (rounded centroids can
 *      coincide and duplicates given in init stay duplicates: possibly fewer than m), sizes_out = their number, rows from sizes_out
 *      to K zero.  Every element of every output is written.
 * Integer arithmetic throughout (sums <= 2^14 * 255): the result depends only on the multiset of the image's quantised colours --
 * not on the order of the pixels, on N, on the image's place in the batch or on how the work is split between lanes -- and two calls
 * give identical bits.  The centroids are not re-assigned: snap with p2p_palette_snap, which also yields the index image, the
 * counts and the quantisation error.  One workgroup per image, 17.1 KB + 8 H W bytes of LDS; no workspace, no allocation. */
int p2p_palette_quantize(int N, int H, int W, const float* img, int colours, int iterations, const int* init_palette,
                         const int* init_sizes, int K, int* palette_out, int* sizes_out, int* iters_out, void* stream);

/* Differentiable palette projection (DESIGN.md "palette projection"): every pixel replaced by a colour of its image's palette.
 * img, palette, sizes, K, tau and w_pk as for the soft histogram; n = clamp(sizes[n], 0, K); out: dense f32 [N][H][W][4], 16-byte
 * aligned, every pixel written.
 *   hard = 0:  out_p = 2 sum_k w_pk c_k - 1 in all four channels, the sum taken as c_r + sum_k w_pk (c_k - c_r) about the pixel's
 *              nearest slot r (a min pass, then one exponential per pair);
 *   hard = 1:  out_p = palette[argmin_k D_pk] / 127.5f - 1.0f by the integer rule of p2p_palette_snap (same device code): the bits
 *              of its image_out.  tau is checked and otherwise unused.
 *   n = 0:     out = img bit for bit.
 * Purely per pixel: no workspace, no atomics, no cross-lane reduction; a pixel's bits depend on neither N nor its image's place. */
int p2p_palette_project_fwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau, int hard,
                            float* out, void* stream);
/* The VJP of the SOFT projection at img for an upstream gradient g [N][H][W][4] (whichever forward ran: with hard = 1 it is the
 * surrogate gradient of the snap):   dimg_p = (2 / tau) Cov_w(c) g_p,   Cov_w(c) = sum_k w_pk c_k c_k^T - (sum_k w_pk c_k)(sum_k w_pk c_k)^T,
 * a symmetric 4 x 4 matrix per pixel, alpha included (the 0.5 of x and the 2 of out cancel).  The covariance is taken about the
 * nearest slot, E[(c - c_r)(c - c_r)^T] - E[c - c_r] E[c - c_r]^T, so it does not cancel where one colour dominates.  n = 0:
 * dimg = g bit for bit.  g, dimg: dense f32, 16-byte aligned; every pixel of dimg written.  Per pixel, as the forward. */
int p2p_palette_project_bwd(int N, int H, int W, const float* img, const int* palette, const int* sizes, int K, float tau,
                            const float* g, float* dimg, void* stream);

/* Palette lookup: the RGBA image of the indexed model's probabilities.  probs, dprobs: dense f32 [N][H][W][K];
 * palette: int32 [N][K][4], RGBA rows in 0..255; out, g: dense f32 [N][H][W][4]; every pointer 16-byte aligned; any H, W >= 1
 * (H * W <= 2^30, N <= 65535); K must be 256, as for p2p_softmax_bwd; hard and blacken are 0 or 1.  Anything else returns a negative
 * code before any launch.  With t_k = palette[n][k] / 127.5f - 1.0f per channel (the two f32 operations of p2p_palette_snap's
 * image_out) and, with blacken = 1, the RGB of a slot whose alpha is 0 set to 0 first (t_k = (-1, -1, -1, -1):
 * dataset_utils.blacken_transparent_pixels applied to the palette):
 *   hard = 0:  out_p = sum_k probs_pk t_k.  Linear: no offset, nothing assumes that a row sums to 1; a one-hot row (an exact 1.0f and
 *              zeros) returns the bits of t_k.  One wave reduces one pixel: four FMAs per channel in every lane (slots 4 lane ..
 *              4 lane + 3, ascending), then an xor butterfly (offsets 32, 16, .., 1) over the 64 lanes.  The same lanes in the same
 *              order for every pixel; no atomics, no workspace: a pixel's bits depend on neither N, nor its image's place in the
 *              batch, nor a second launch.
 *   hard = 1:  out_p = t_argmax_k probs_pk, ties to the lowest k (the rule of p2p_argmax_lastdim): bit-equal to a gather.
 * Every pixel of out is written. */
int p2p_palette_lookup_fwd(int N, int H, int W, int K, const float* probs, const int* palette, int hard, int blacken,
                           float* out, void* stream);
/* Its VJP with respect to probs for an upstream gradient g -- the same for both forwards (for hard = 1 the straight-through
 * surrogate); the palette is not differentiable and probs is not needed:
 *   dprobs_pk = ((g_p0 t_k0 + g_p1 t_k1) + g_p2 t_k2) + g_p3 t_k3,
 * every product and every sum rounded to f32 on its own (no FMA contraction), so a float32 restatement matches bit for bit.  Every
 * element of dprobs is written: a 1 KB-per-pixel write stream. */
int p2p_palette_lookup_bwd(int N, int H, int W, int K, const float* g, const int* palette, int blacken,
                           float* dprobs, void* stream);

/* ---- differentiable augmentation (build-added, DESIGN.md "differentiable augmentation") --------------------------- */
/* DiffAugment (Zhao et al., NeurIPS 2020) of dense f32 RGBA images [N][H][W][4], 16-byte aligned, any H, W >= 1 (H * W <= 2^28,
 * N <= 65535).  color: f32 [N][3] = brightness offset b, saturation factor s, contrast factor k; geometry: int32 [N][4] = ty, tx,
 * y0, x0 (any int32); both in device memory.  policy_bits: 1 colour | 2 translation | 4 cutout; a stage whose bit is clear does not
 * read its table (color / geometry may then be NULL).  Per image, in this order:
 *   colour       channels 0..2 of every pixel: u = x + b;  v = (u - mean_c u) s + mean_c u;  y = (v - m) k + m, where m, the mean of v
 *                over the image's H W 3 values, is taken as mean_rgb(x) + b (equal in real arithmetic).  Alpha is untouched.
 *   translation  out[r][c] = y[r - ty][c - tx] where that pixel exists, else `fill` in all four channels.
 *   cutout       out[r][c] = fill for y0 <= r < y0 + ch and x0 <= c < x0 + cw (the box may hang over the border; ch, cw >= 0).
 * Without the colour bit the result is a bit-exact copy / move / fill.  out must not be img.  workspace:
 * p2p_diffaug_workspace_bytes(N, H, W) bytes, needed by the colour stage only (one partial sum per 1024 pixels; the sums are
 * tree-shaped, in a fixed order, without float atomics, and an image's sum does not depend on N or on its place in the batch). */
long long p2p_diffaug_workspace_bytes(int N, int H, int W);
int p2p_diffaug_fwd(int N, int H, int W, const float* img, const float* color, const int* geometry, int ch, int cw,
                    int policy_bits, float fill, float* out, float* workspace, void* stream);
/* Its VJP with respect to img (the tables are not differentiable; img itself is not needed).  With g' = grad_out carried back to
 * the source positions, 0 where the output was a fill, Gamma = sum of g' over the image's pixels and three colour channels and
 * M = 3 H W:   dv = k g' + (1 - k) Gamma / M,   grad_img_c = s dv_c + (1 - s) / 3 sum_c' dv_c' (c < 3),   grad_img_3 = g'_3.
 * Every element of grad_img is written.  `fill` is ignored (one argument list serves both calls); workspace as above. */
int p2p_diffaug_bwd(int N, int H, int W, const float* grad_out, const float* color, const int* geometry, int ch, int cw,
                    int policy_bits, float fill, float* grad_img, float* workspace, void* stream);

/* ---- palette-index head (pix2pix_model.py:261-325) ------------------------------------------------------------ */

/* z: logits view [N][H][W][C]; target: view holding the real palette index of every pixel (as a value of `dtype`).
 * Writes argmax(softmax(z)) (ties -> lowest index) into fake_idx as a value of `dtype`, optionally
 * dz = grad_scale * (softmax(z) - onehot(target)) and the f32 probabilities; loss_out[0] = inv_count * sum CCE with
 * CCE = log(sum_c exp(z_c - max)) - (z_target - max) (the logits form Keras 2.9 uses for a softmax-activated output,
 * finite for every input), loss_out[1] = inv_count / C * sum |onehot - p|.  loss_part: workspace of
 * 2 * P2P_SOFTMAX_MAX_BLOCKS floats (one partial per workgroup, summed in workgroup order: bit-reproducible).
 * 1 <= C <= 512 in f32, 1 <= C <= 256 in bf16: the indices travel as values of `dtype`, and indices above 256 are not bf16
 * values (257 would be read and stored as 256).  Anything else returns a negative code and sets p2p_last_error before any launch. */
#define P2P_SOFTMAX_MAX_BLOCKS 8192
int p2p_softmax_cce_argmax(int dtype, int N, int H, int W, int C, const p2p_tensor* z, const p2p_tensor* target,
                           const p2p_tensor* fake_idx, float grad_scale, float inv_count, const p2p_tensor* dz,
                           float* probs_out, float* loss_part, float* loss_out, void* stream);
/* VJP of softmax over the last dimension, plus an optional direct logits gradient (the loss hooks of the indexed train step):
 *   dz[n,y,x,c] = scale * ( gz[m,c] + p[m,c] * (gp[m,c] - sum_k p[m,k] * gp[m,k]) ),   m = (n*H + y)*W + x
 * probs, gp, gz: dense f32 [N*H*W][C], 16-byte aligned; gp or gz may be NULL (absent = 0; probs is only read with gp).  dz: view
 * in `dtype` (16-byte aligned pixels, written only at the view's own pixels and channels, halo untouched).  C == 256 (anything
 * else: negative return code + p2p_last_error).  f32 arithmetic, except sum_k p*gp and gp - sum_k p*gp in f64 (they cancel where
 * one class dominates).  Deterministic: every pixel is reduced by a fixed set of lanes in a fixed order, no atomics. */
int p2p_softmax_bwd(int dtype, int N, int H, int W, int C, const float* probs, const float* gp, const float* gz,
                    float scale, const p2p_tensor* dz, void* stream);
/* tf.argmax(probs, axis=-1, output_type=int32) on dense f32 probabilities [M][C]; ties -> lowest index. */
int p2p_argmax_lastdim(const float* probs, long long M, int C, int* out, void* stream);

/* The palette-index head in one launch (bf16, IMG_SIZE 64: query p2p_head_softmax_ok): Conv2D(256, 4, stride 1, SAME, bias) of
 * the haloed concat view `in` (pixels of cin_pad = 40 channels: [up6 32 | source | zero pad], networks.py:75-78,92-94) with
 * the op-G weight copy wt[16][256][40], softmax over the 256 palette slots, argmax (ties -> lowest index) written as an
 * activation-dtype value into `fake_idx`, CategoricalCrossentropy against the index image `target` in the log-sum-exp form,
 * and its gradient grad_scale * (probs - onehot) into the haloed view `dz` (256-channel pixels) -- what p2p_igemm_edge +
 * p2p_softmax_cce_argmax + p2p_view_colsum compute, without ever writing the logits (pix2pix_model.py:268,273-293,300-301).
 * loss_out[0] = inv_count * sum of -log p_target, loss_out[1] = inv_count / 256 * sum |onehot - p|; dbias (may be NULL) =
 * column sums of dz.  workspace: p2p_head_softmax_workspace_bytes(N, H) bytes (per-workgroup partials, summed in order). */
int p2p_head_softmax_ok(int dtype, int N, int H, int W, int cin_pad, int ncls);
long long p2p_head_softmax_workspace_bytes(int N, int H);
int p2p_head_softmax_cce(int dtype, int N, int H, int W, int cin_pad, int ncls, const p2p_tensor* in, const void* wt,
                         const float* bias, const p2p_tensor* target, const p2p_tensor* fake_idx, float grad_scale,
                         float inv_count, const p2p_tensor* dz, float* dbias, float* workspace, float* loss_out, void* stream);
/* Data gradient of that head through its first 32 input channels (the up6 slice of the concat; the source image has no
 * gradient): op P, stride 1, out[n,y,x,g] = sum_{kh,kw,d} dz[n,y+1-kh,x+1-kw,d] * W[kh][kw][g][d], g < 32, with the op-P weight
 * copy wn[16][w_rows][256] (bf16, IMG_SIZE 64: query p2p_head_dgrad_ok).  dz: haloed view of 256-channel pixels (zero halo of
 * 2 pixels); out: view with >= 32 channels per pixel, channels [0, 32) are written. */
int p2p_head_dgrad_ok(int dtype, int N, int H, int W, int ncls, int cout, int w_rows, int dz_ld, int out_ld);
int p2p_head_dgrad(int dtype, int N, int H, int W, int ncls, int cout, const p2p_tensor* dz, const void* wn, int w_rows,
                   const p2p_tensor* out, void* stream);

/* ---- optimizer / parameter plumbing (pix2pix_model.py:28-29,81-83) ------------------------------- */

/* Keras Adam over a flat f32 buffer; t = iteration AFTER increment; grads are multiplied by gscale first. */
int p2p_adam_flat(float* p, const float* g, float* m, float* v, long long n, int t,
                  float lr, float beta1, float beta2, float eps, float gscale, void* stream);

/* Device-resident step state (lets a whole step be captured in a hipGraph and replayed): t_dev[0] += 1 and
 * lr_t_dev[0] = lr*sqrt(1-beta2^t)/(1-beta1^t); p2p_adam_flat_dev reads the step size from lr_t_dev. */
int p2p_adam_tick(int* t_dev, float* lr_t_dev, float lr, float beta1, float beta2, void* stream);
int p2p_adam_flat_dev(float* p, const float* g, float* m, float* v, long long n, const float* lr_t_dev,
                      float beta1, float beta2, float eps, float gscale, void* stream);
/* p2p_adam_flat_dev that leaves the elements [ex_lo, ex_hi) of all four buffers alone (neither read nor written; any alignment)
 * in ONE launch: a tensor whose gradient is identically 0 (and whose moments are 0) does not move under Adam.  Bit-identical to
 * p2p_adam_flat_dev outside the range. */
int p2p_adam_flat_dev_excl(float* p, const float* g, float* m, float* v, long long n, long long ex_lo, long long ex_hi,
                           const float* lr_t_dev, float beta1, float beta2, float eps, float gscale, void* stream);
/* Exponential moving average e of the masters p, fused into the Adam pass.  p, m, v come out as from
 * p2p_adam_flat_dev[_excl], bit for bit; then, per element, in f32 without contraction,
 *     e' = e + (1 - beta_t) * (p' - e),    beta_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay,    t = (float)t_dev[0]
 * (the Adam iteration as p2p_adam_tick left it: the kernel reads it, so a recorded or captured step serves every step number).
 * Where p' == e, e' == e exactly.  e: n floats, 16-byte aligned like the others; the _excl form leaves [ex_lo, ex_hi) of e alone
 * too.  p2p_ema_flat is the same update as a pass of its own over an already updated p (for p2p_adam_prep_batched steps). */
int p2p_adam_ema_flat_dev(float* p, const float* g, float* m, float* v, float* e, long long n, const float* lr_t_dev,
                          float beta1, float beta2, float eps, float gscale, const int* t_dev, float decay, int warmup, void* stream);
int p2p_adam_ema_flat_dev_excl(float* p, const float* g, float* m, float* v, float* e, long long n, long long ex_lo, long long ex_hi,
                               const float* lr_t_dev, float beta1, float beta2, float eps, float gscale, const int* t_dev, float decay,
                               int warmup, void* stream);
int p2p_ema_flat(float* e, const float* p, long long n, const int* t_dev, float decay, int warmup, void* stream);
int p2p_counter_add(long long* counter_dev, long long inc, void* stream);

/* ---- optimizer options: learning-rate schedules, gradient clipping ------------------------------- */

/* A learning-rate schedule, evaluated on the DEVICE from the step counter: lr(step) in f64 with the formulas of Keras 2.9's
 * tf.keras.optimizers.schedules (names below), step = the iteration count BEFORE the increment (Keras evaluates a schedule at
 * `iterations`, then increments).  A HOST struct, read when the call is issued (it travels to the kernel by value).
 *   P2P_LR_CONSTANT     lr = initial
 *   P2P_LR_EXPONENTIAL  ExponentialDecay: p = step / decay_steps; flag (staircase): p = floor(p); lr = initial * rate^p
 *   P2P_LR_PIECEWISE    PiecewiseConstantDecay: values[0] if step <= bounds[0]; values[i] if bounds[i-1] < step <= bounds[i];
 *                       values[nbounds] if step > bounds[nbounds-1]        (nbounds <= 8)
 *   P2P_LR_POLYNOMIAL   PolynomialDecay: flag (cycle): d = decay_steps * (step == 0 ? 1 : ceil(step / decay_steps)), s = step;
 *                       else d = decay_steps, s = min(step, decay_steps);  lr = (initial - end) * (1 - s / d)^power + end
 *   P2P_LR_COSINE       CosineDecay: s = min(step, decay_steps); lr = initial * ((1 - rate) * 0.5 * (1 + cos(pi * s / decay_steps)) + rate)
 *                       (rate = alpha)
 *   P2P_LR_LINEAR       build-added LinearDecay (the pix2pix recipe): initial while step < hold_steps, `end` from
 *                       step >= hold_steps + decay_steps on, initial + (end - initial) * (step - hold_steps) / decay_steps between
 * warmup_steps > 0 multiplies any kind by (step + 1) / warmup_steps while step < warmup_steps. */
enum { P2P_LR_CONSTANT = 0, P2P_LR_EXPONENTIAL = 1, P2P_LR_PIECEWISE = 2, P2P_LR_POLYNOMIAL = 3, P2P_LR_COSINE = 4,
       P2P_LR_LINEAR = 5 };
typedef struct p2p_lr_schedule {
    int kind, flag, nbounds, pad_;
    double initial, decay_steps, rate, end, power, hold_steps, warmup_steps;
    double bounds[8], values[9];
} p2p_lr_schedule;
/* p2p_adam_tick with the rate taken from a schedule: t_dev[0] += 1 (-> t), lr = sched(t - 1) in f64,
 * lr_t_dev[0] = (float)(lr * sqrt(1 - beta2^t) / (1 - beta1^t)).  P2P_LR_CONSTANT without warm-up, initial = (double)(float)lr:
 * the bits of p2p_adam_tick.  The device's f64 pow and cos are not correctly rounded: other kinds may differ from a host
 * evaluation by 1 ulp of the f32 result. */
int p2p_adam_tick_sched(int* t_dev, float* lr_t_dev, const p2p_lr_schedule* sched, float beta1, float beta2, void* stream);

/* Global L2 norm of a flat f32 gradient and the scale tf.clip_by_global_norm applies, in a FIXED summation order that depends
 * on n alone (not on the batch, the resident grid or the stream; no atomics), every operation a correctly rounded f32 one
 * without contraction (sq = g * g rounded, then acc + sq), so a NumPy float32 restatement reproduces the bits
 * (tests/optimizer_oracle.py):
 *   p2p_sumsq_partials   V = n / 4 whole 16-byte vectors, NB = min(max(ceil(V / 256), 1), P2P_SUMSQ_MAX_PARTS) workgroups of
 *       256 threads.  Thread q = 256 * b + tid starts with acc = 0 and walks the vectors j = q, q + 256 * NB, ... in rising
 *       order, within a vector the components 0, 1, 2, 3 in order: acc = acc + g * g.  An element inside the hole
 *       [ex_lo, ex_hi) counts as 0 (a vector wholly inside is not read).  Thread 0 of workgroup 0 then adds the n % 4 tail
 *       elements in rising order.  Wave tree: for off = 32, 16, 8, 4, 2, 1: acc[l] = acc[l] + acc[l + off] (lane 0 holds the
 *       wave's sum).  Workgroup: ((w0 + w1) + w2) + w3 over its four waves -> partials[b].  *nparts_out = NB (HOST int, written
 *       when the call is issued).  partials: room for P2P_SUMSQ_MAX_PARTS floats.
 *   p2p_clip_scale       the partials of nbuf (<= 8) buffers, concatenated in argument order into one list c[0 .. M): one wave;
 *       lane l: acc = 0, then acc = acc + c[i] for i = l, l + 64, ... rising; the same wave tree; norm = sqrt(lane 0's sum);
 *       scale = norm > clipnorm ? clipnorm / norm (one correctly rounded division) : 1.0f -- EXACTLY 1 at and below the
 *       threshold, where TF's clip_norm * min(1 / norm, 1 / clip_norm) may be 1 ulp off 1; a non-finite norm gives a NaN
 *       scale, as tf.clip_by_global_norm does.  scale_dev[0] = scale, norm_dev[0] = norm (kept for logging without a sync).
 *       `partials` and `nparts` are HOST arrays (of device pointers / of counts), read when the call is issued. */
enum { P2P_SUMSQ_MAX_PARTS = 1024, P2P_CLIP_MAX_BUFS = 8 };
int p2p_sumsq_partials(const float* g, long long n, long long ex_lo, long long ex_hi, float* partials, int* nparts_out,
                       void* stream);
int p2p_clip_scale(const float* const* partials, const int* nparts, int nbuf, float clipnorm, float* scale_dev, float* norm_dev,
                   void* stream);

/* One Adam launch over a flat buffer with every option as a field: what p2p_adam_flat_dev, _excl, p2p_adam_ema_flat_dev and
 * _excl do (e null: no moving average; ex_lo == ex_hi: no hole), plus
 *   gscale_dev   device scalar the gradient is multiplied by (p2p_clip_scale's; null: 1)
 *   clipvalue    hyper->clipvalue > 0: g = fminf(fmaxf(g, -c), c) before everything else (<= 0: off)
 * Both are HOST structs read when the call is issued; `hyper` is shared by every launch of one optimizer.  The five entry points
 * are one kernel behind one launcher (csrc/optim.hip adam_kernel, adam_launch): with both options off this call runs the very
 * code of the entry point it stands for, and with them on the element still goes through the same update. */
typedef struct p2p_adam_hyper {
    float beta1, beta2, eps, clipvalue, ema_decay;
} p2p_adam_hyper;
typedef struct p2p_adam_args {
    float* p;
    const float* g;
    float* m;
    float* v;
    float* e;
    long long n, ex_lo, ex_hi;
    const float* lr_t_dev;
    const float* gscale_dev;
    const int* t_dev;
    const p2p_adam_hyper* hyper;
    int ema_warmup, pad_;
} p2p_adam_args;
int p2p_adam_step(const p2p_adam_args* a, void* stream);

/* f32 gradient sum of a GradientTape (tape.py): a network's weight gradients over several calls, the two terms of a generator
 * call's d(source).  dst = src when `first` is set (the first contribution), dst += src otherwise; n floats, 16-byte aligned,
 * no atomics (bit-reproducible). */
int p2p_grad_accumulate(float* dst, const float* src, long long n, int first, void* stream);

/* master f32 W[16][Cg][Cd] -> wn (dtype, same layout; may be null) and wt (dtype, [16][Cd][Cg]; may be null). */
int p2p_weight_prep(int dtype, const float* w, int Cg, int Cd, void* wn, void* wt, void* stream);

/* Padded variant for the edge layers: wn is [16][wn_rows][wn_cols], wt is [16][wt_rows][wt_cols]; entries
 * outside the real [Cg][Cd] block are zero. */
int p2p_weight_prep_pad(int dtype, const float* w, int Cg, int Cd, void* wn, int wn_rows, int wn_cols,
                        void* wt, int wt_rows, int wt_cols, void* stream);

/* Batched form: one launch for every layer.  `tasks_dev` is a DEVICE array of ntasks (<= 64) descriptors with the
 * arguments of p2p_weight_prep_pad (null wn / wt = not wanted); tiles_g, tiles_d and the task's workgroup count come from
 * p2p_weight_prep_task_blocks, first_block is the running sum of the preceding tasks' counts, total_blocks the sum. */
typedef struct p2p_prep_task {
    const float* w;
    void* wn;
    void* wt;
    int Cg, Cd, wn_rows, wn_cols, wt_rows, wt_cols, tiles_g, tiles_d;
    long long first_block;
} p2p_prep_task;
long long p2p_weight_prep_task_blocks(int Cg, int Cd, int wn_rows, int wn_cols, int wt_rows, int wt_cols,
                                      int have_wn, int have_wt, int* tiles_g, int* tiles_d);
int p2p_weight_prep_batched(int dtype, const p2p_prep_task* tasks_dev, int ntasks, long long total_blocks, void* stream);
/* Keras Adam step (as p2p_adam_flat_dev, same expressions) on the masters of the listed layers AND their operand copies in one
 * pass (tf.keras.optimizers.Adam.apply_gradients, pix2pix_model.py:81-83, followed by what p2p_weight_prep_batched derives):
 * every task's master `w` lies inside `params`; grads / m / v are the flat buffers parallel to it.  Each kernel tensor must be
 * listed ONCE; n_elems = sum of 16 * Cg * Cd over the tasks.  The small tensors (gamma, beta, bias) go through
 * p2p_adam_flat_dev. */
int p2p_adam_prep_batched(int dtype, long long n_elems, const p2p_prep_task* tasks_dev, int ntasks, long long total_blocks,
                          float* params, const float* grads, float* m, float* v, const float* lr_t_dev, float beta1, float beta2,
                          float eps, void* stream);


/* dense f32 (or i32 if src_is_int) [N][H][W][C] host-layout batch -> view in `dtype` (dataset_utils.py:39-48 contract). */
int p2p_pack_input(int dtype, int N, int H, int W, int C, const void* src, int src_is_int,
                   const p2p_tensor* dst, void* stream);
/* same batch into ndst (1..4) views with one read (dsts = array of p2p_tensor). */
int p2p_pack_input_multi(int dtype, int N, int H, int W, int C, const void* src, int src_is_int,
                         const p2p_tensor* dsts, int ndst, void* stream);
/* The RGBA (4-channel) batch of a train step in one launch: source and target read once, whole-pixel stores into
 * down1's input [source|0], channels 32..39 of the last concat buffer [source|0], the real half of the discriminator
 * input [target|source] and the source half of its fake half.  Every view starts on an 8-channel boundary.
 * v_c6 and v_dfake may be NULL: those two are PARTIAL-pixel stores (16 of 80 bytes, 8 of 16), which the train step leaves to
 * the kernels that write the rest of the pixel (p2p_norm_act_fwd_tail, p2p_tanh_l1_fwd_pair). */
int p2p_pack_pair(int dtype, int N, int H, int W, const float* source, const float* target,
                  const p2p_tensor* v_src, const p2p_tensor* v_c6, const p2p_tensor* v_dreal, const p2p_tensor* v_dfake,
                  void* stream);
/* The palette-index batch of a train step (one int32 index per pixel, dataset_utils.py:232-246; 8-channel pixels): whole-pixel
 * stores of [source 0..] into v_src (and v_c6 unless NULL), [target source 0..] into v_dreal, [0 source 0..] into v_dfake
 * (its channel 0 is written later by the head's argmax). */
int p2p_pack_pair_idx(int dtype, int N, int H, int W, const int* source, const int* target,
                      const p2p_tensor* v_src, const p2p_tensor* v_c6, const p2p_tensor* v_dreal, const p2p_tensor* v_dfake,
                      void* stream);
/* out[7] = [g_total, g_adv, g_l1, g_aux, d_total, d_real, d_fake] from the loss slots written by the loss kernels:
 * slots[0..2] = BCE(1,real), BCE(0,fake), BCE(1,fake); slots[l1_slot] = L1; slots[aux_slot] = histogram /
 * segmentation loss (aux_slot < 0: none); g_total = adv + lambda_l1*l1 + lambda_aux*aux. */
int p2p_finish_losses(const float* slots, int aux_slot, int l1_slot, float lambda_l1, float lambda_aux, float* out,
                      void* stream);
/* The same result vector for a generator loss of five terms (the fused palette step): g_total = adv + lambda_l1*l1 +
 * lambda_aux*slots[aux_slot] + lambda_aux2*slots[aux2_slot]; out[3] = slots[aux_slot]. */
int p2p_finish_losses2(const float* slots, int aux_slot, int aux2_slot, int l1_slot, float lambda_l1, float lambda_aux,
                       float lambda_aux2, float* out, void* stream);
/* view in `dtype` -> dense f32 [N][H][W][C] (for generate()/tests). */
int p2p_unpack(int dtype, int N, int H, int W, int C, const p2p_tensor* src, float* dst, void* stream);

/* Bernoulli(0.5) keep mask of Dropout(0.5) (networks.py:31-32): counter-based RNG, one byte per element. */
int p2p_dropout_mask(unsigned char* mask, long long n, long long seed, long long counter, void* stream);
/* same with the call counter = counter_dev[0]*16 + salt read on the device; the random stream is indexed by
 * elem_offset + i (elem_offset = elements of this layer's mask that belong to the samples in front of the shard, a
 * multiple of 8), so the ranks of a data-parallel step draw the masks of the single-process global batch. */
int p2p_dropout_mask_dev(unsigned char* mask, long long n, long long seed, const long long* counter_dev,
                         long long salt, long long elem_offset, void* stream);

/* ---- collectives (RCCL over xGMI; build-added data parallelism) ----------------------------------- */

/* For hosts without PyTorch (the Python host of this repository reaches the same RCCL through torch.distributed).  Rank 0
 * obtains 128 opaque bytes with p2p_comm_unique_id and distributes them; every rank (one process per GPU, hipSetDevice done)
 * calls p2p_comm_init with them.  p2p_comm_allreduce_sum: in-place SUM of n f32 values, stream-ordered -- per step the flat
 * generator gradient buffer in buckets, the tail [small tensors | discriminator gradients | loss slots] and, for the
 * histogram model, the one Hellinger scalar between p2p_hellinger_fwd and p2p_hellinger_finish.  librccl.so is loaded on the
 * first call (no link-time dependency). */
int p2p_comm_unique_id(void* id_out_128_bytes);
int p2p_comm_init(const void* id_128_bytes, int rank, int world, void** comm_out);
int p2p_comm_allreduce_sum(void* comm, float* buf, long long n, void* stream);
int p2p_comm_destroy(void* comm);

/* ---- stream ordering (the drop-in's own schedule; the reference's train_step is one tf.function, pix2pix_model.py:63-87) ---
 * Events that order kernels of ONE device between the engine's HIP streams (weight gradients and histograms run beside the
 * data-gradient chain).  Created with hipEventDisableTiming | hipEventDisableSystemFence: no host-visible release, so a record
 * does not write back / invalidate L2.  Not for host synchronisation (use the stream's own synchronise for that). */
int p2p_event_create(void** ev_out);
int p2p_event_destroy(void* ev);
int p2p_event_record(void* ev, void* stream);            /* marks the work issued so far on `stream` */
int p2p_stream_wait_event(void* stream, void* ev);       /* later work on `stream` waits for the event's latest record */
/* A record costs the recording stream a packet of its own between two kernels.  p2p_arm_stop_event(ev) instead hands `ev` to the
 * LAST kernel that the next supporting entry point of this thread launches (p2p_norm_act_bwd, p2p_act_bwd: the calls the weight-
 * gradient forks follow), as that dispatch's completion signal: equivalent to p2p_event_record(ev, stream) right behind the call.
 * p2p_disarm_stop_event(&was_pending) afterwards tells whether the event is still unclaimed (record it the ordinary way then). */
int p2p_arm_stop_event(void* ev);
int p2p_disarm_stop_event(int* was_pending);

/* ---- step replay (the reference runs train_step as ONE traced tf.function, pix2pix_model.py:62: a step costs the host one
 * call, not one per op; side2side_model.py:73,114 is the loop that issues it) -------------------------------------------------
 * A train step is ~105 kernel entry points and ~40 stream operations whose arguments do not change from step to step (persistent
 * buffers, explicit stream handles).  The host records them once as an array of p2p_replay_call and re-issues the whole step
 * with ONE p2p_replay call: the same entry points, in the same order, on the same streams -- bit-identical results, no
 * interpreter between two launches.  `fn` = p2p_replay_fn_index(name of an entry point of this header that returns int and takes
 * only scalars and pointers); a[k] = argument k in an 8-byte slot (ints and floats in the low bytes, little endian).  Bit k of
 * `ind64` / `ind32` set: a[k] is the ADDRESS of a host variable of 8 / 4 bytes that is read when the call is replayed (the batch
 * pointers, the result pointer, the optimizer's hyper-parameters: what may change between two steps of one recording).
 * Structures passed by pointer (p2p_tensor, p2p_gsrc) are read at replay time like any other pointer argument: the host keeps
 * them alive.  Returns 0, or the first failing call's code with p2p_last_error() naming the call's index and entry point. */
#define P2P_REPLAY_MAX_ARGS 24
typedef struct {
    int fn;
    int nargs;
    unsigned ind64;
    unsigned ind32;
    unsigned long long a[P2P_REPLAY_MAX_ARGS];
} p2p_replay_call;
int p2p_replay_fn_index(const char* name);      /* -1: not a replayable entry point */
int p2p_replay_fn_nargs(int fn);
int p2p_replay(const p2p_replay_call* calls, int n);

/* ---- input pipeline (reference dataset_utils.py:11-20,39-49,66-120,209-246) ---------------------------- */

/* Host helper (no GPU): undo the PNG scanline filters of an inflated IDAT stream (height rows of 1 + row_bytes bytes, 8-bit
 * samples, bpp bytes per pixel) into out[height][row_bytes].  Replaces libpng behind tf.image.decode_png (dataset_utils.py:68). */
int p2p_png_unfilter(const unsigned char* filtered, int height, int row_bytes, int bpp, unsigned char* out);

/* One RGBA train/test batch from the HBM-resident sprite set `sprites` (uint8 [n_sprites][S][S][4], S a power of two).
 * src_idx/tgt_idx: device int32 [B] sprite numbers; aug: device f32 [B][4] = (apply != 0, hue delta in turns, dy, dx in
 * pixels) or NULL (test set / augment=False).  Per pixel: translate (nearest, fill 0) -> blacken alpha == 0
 * (dataset_utils.py:11-20) -> hue rotation of RGB (tf.image.adjust_hue semantics, :80-84) -> x / 127.5 - 1 if `normalise`
 * (:39-49) -> source/target f32 [B][S][S][4], the two tensors train_step takes (pix2pix_model.py:63-64). */
int p2p_sprites_rgba_batch(const void* sprites, int n_sprites, int S, const int* src_idx, const int* tgt_idx, const float* aug,
                           int B, int normalise, float* source, float* target, void* stream);

/* Row gather out[b] = table[sel[b]] (rows of row_ints int32, row_ints % 4 == 0): indexed batches are rows of the index maps
 * and palettes extracted once at load time (dataset_utils.py:123-164). */
int p2p_gather_rows_i32(const int* table, int n_rows, int row_ints, const int* sel, int B, int* out, void* stream);

/* palette_ordering = "shuffled" (io_utils.py:53-55 calls tf.random.shuffle inside the dataset map: a new permutation of the
 * palette's colours every time a sample is loaded).  Re-labels one gathered indexed batch: src_out/tgt_out[b][i] =
 * inv[b][idx[b][i]] over the n index values of each sample, pal_out[b][j] = palette[b][perm[b][j]] over the P palette rows of C
 * ints; perm/inv: device int32 [B][P], inverse of each other (the padding rows map to themselves).  The decoded image
 * indexed_to_rgba(idx, palette) (io_utils.py:96-103) is unchanged. */
int p2p_palette_relabel_batch(const int* src_idx, const int* tgt_idx, const int* palette, const int* perm, const int* inv,
                              int B, int n, int P, int C, int* src_out, int* tgt_out, int* pal_out, void* stream);

/* ---- FID evaluation: InceptionV3 (Keras, include_top=False, pooling="avg", inference; reference frechet_inception_distance.py)
 * All f32 in / f32 accumulate, fixed-order sums (bit-reproducible).  Views are NHWC p2p_tensor WITHOUT a halo: the convolution and
 * the average pool predicate their taps on the image bounds.  Layer table and launch order: palette_and_histo_gan_amd/inception.py. */

/* resize(image, (OH, OW, 3), order=0) of scikit-image 0.19 + preprocess_input ("tf" mode) of dense f32 images [N][H][W][C],
 * C = 3 or 4: with `filter` (C = 4) the channel axis is smoothed by the 3-tap gaussian w1, w0, w1 (mode "mirror", in f64 as
 * scipy evaluates it, stored f32); then out[n, o, p, q] = img[n, rows[o], cols[p], chans[q]] (device int32 index tables built on
 * the host with scipy.ndimage.zoom), clipped to image n's [min, max], / 127.5, - 1.  minmax: device workspace of 2 N floats. */
int p2p_inc_prep(int N, int H, int W, int C, const float* images, const int* rows, const int* cols, const int* chans, int OH,
                 int OW, double w0, double w1, int filter, const p2p_tensor* out, float* minmax, void* stream);
/* Conv2D (no bias, kernel kh x kw, stride, top/left zero padding) + BatchNorm(scale=False) + ReLU:
 * out[n, oy, ox, co] = relu(scale[co] * sum_{ky,kx,ci} in[n, oy s - pad_top + ky, ox s - pad_left + kx, ci] w[(ky kw + kx) Cin + ci][co]
 *                      + shift[co]),  scale = rsqrt(var + eps), shift = beta - mean scale (host, f64 -> f32).
 * w: f32 [kh kw Cin][Cout], 16-byte aligned, Cout % 4 == 0.  `out` may be a channel slice of a wider buffer (any ld). */
int p2p_inc_conv(int N, int H, int W, int Cin, int kh, int kw, int stride, int pad_top, int pad_left, int OH, int OW, int Cout,
                 const p2p_tensor* in, const float* w, const float* scale, const float* shift, const p2p_tensor* out, void* stream);
/* kind 0: max 3x3 / 2 "valid" (OH = (H - 3) / 2 + 1); kind 1: average 3x3 / 1 "same" over the taps inside the image (OH = H) */
int p2p_inc_pool(int kind, int N, int H, int W, int C, const p2p_tensor* in, const p2p_tensor* out, void* stream);
/* global average pool: out f32 [N][C] = mean over the H x W map */
int p2p_inc_gap(int N, int H, int W, int C, const p2p_tensor* in, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
