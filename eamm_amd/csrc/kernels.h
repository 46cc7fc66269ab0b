// Internal (non-ABI) declarations shared by the HIP translation units of libeamm_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace eamm {

constexpr int CONV_BK = 32;           // K-chunk: 32 input channels of one filter tap
constexpr int CONV_LDK = CONV_BK + 4; // LDS row stride (dwords): +16 B keeps ds_read_b128 conflict-free
inline size_t round64(size_t n) { return (n + 63) / 64 * 64; }   // 256-byte aligned sections of a workspace
constexpr int KP_STRIDE = 8;          // per (frame, keypoint) record: kd.xy, ks.xy, J00 J01 J10 J11

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_SIGMOID = 2 };

// Executed-MFMA accounting for bench.py's roofline: every launcher of a matrix-core kernel adds the multiply-adds its grid
// really issues (padded tile dimensions, Winograd / polyphase point counts -- not the reference convolution's) x 2 to a
// per-host-thread counter; eamm_forward_frames folds it into the profile totals while profiling is on.
void note_mfma_flops(double flops);
double take_mfma_flops();   // returns the counter and resets it
double total_mfma_flops();  // process-wide monotonic total (all host threads)

// Tuning knobs: every EAMM_* environment variable the library reads goes through knob_int(), which records the name, the value
// in effect and whether the environment set it -- eamm_knobs_json() reports the table, so a benchmark line can carry the
// configuration it was measured under (bench.py `knobs`).  DOCUMENTED knobs are listed in include/eamm_hip.h.
long long knob_int(const char* name, long long dflt);
int knobs_json(char* buf, int cap);   // {"EAMM_X": {"value": v, "set": 0|1}, ...}; returns the length needed (excl. NUL)

// One convolution launch. Activations are NHWC fp32; the GEMM view is
//   M = B*H*W pixels (2x2-quad order), N = Cout, K = taps * (C0 + C1).
struct ConvArgs {
    const float* in0;      // [B,H,W,C0]
    const float* in1;      // [B,H,W,C1] second half of a channel concatenation, or null
    int C0, C1;            // multiples of CONV_BK
    unsigned in0_bytes, in1_bytes, w_bytes;  // buffer-descriptor ranges
    int H, W;              // input size (even); phase mode writes a 2H x 2W output
    int linear;            // 1: pixels enumerated in raster order (odd H or W; never with pool) instead of 2x2 quads
    int nphase;            // 1, or 4 = collapsed "nearest x2 + 3x3" (one 2x2 filter per output parity)
    int M;                 // B*H*W
    const float* w;        // packed [nphase][ntiles][nchunks][BN][BK], BatchNorm already folded in
    const float* bias;     // [ntiles*BN]
    int Cout;              // real output channels (= output stride)
    int nchunks;           // taps * (C0+C1)/BK
    int mtiles, ntiles;
    int chunks_per_split;  // K range of one split-K slice
    int Mpad, Npad;        // partial slab dims
    float* partial;        // non-null: split-K, raw accumulators to [split][phase][Mpad][Npad]
    int act;               // Act
    int pool;              // avgpool2x2 after the activation
    int nchw;              // write out as [B,Cout,H,W] instead of NHWC
    const float* resid;    // NHWC, added before the activation
    float* out;            // NHWC [B,H,W,Cout] (pooled: [B,H/2,W/2,Cout]; phase: [B,2H,2W,Cout])
    float* out2;           // optional second output relu(out*s2 + t2): the next res-block's pre-activation
    const float* s2;
    const float* t2;
    int split_n;           // > 0 (round 6, the private DeconvTail -> KPDetector_a hand-over): channels n < split_n go to `out` as NHWC with
                           // a split_n-float pixel stride, channels split_n <= n < Cout to `out2` as one float4 per pixel (Cout <= split_n + 4)
};

// Packed convolution weights resident on the device.
struct ConvLayer {
    int kh = 0, kw = 0, C0 = 0, C1 = 0, Cout = 0;
    bool phase = false;     // UpBlock2d: nearest x2 + 3x3 as four 2x2 phase filters
    int BM = 128, BN = 0, ntiles = 0, nchunks = 0;
    int dma_cfg = 0;        // 0: register-staged 128 x BN kernel; >0: LDS-DMA big-tile kernel (conv_mfma_dma.hip)
    float* w = nullptr;     // device
    float* bias = nullptr;  // device, [ntiles*BN]
};

int conv_tile_n(int Cout);
size_t conv_packed_elems(int taps, int cin_packed, int Cout, int BN, int nphase);
// Host-side repack: [Cout][Cin][kh*kw] (BatchNorm folded by the caller) -> [nphase][ntiles][nchunks][BN][BK].
// cin_map[c] = original input channel of packed channel c, or -1 for zero padding.  phase = true takes
// 3x3 weights and emits the four collapsed 2x2 filters.
void conv_pack_host(const float* w, int Cout, int Cin, int kh, int kw, const int* cin_map, int cin_packed, int BN,
                    bool phase, bool swizzle, float* dst);
// Same packing from four explicit 2x2 phase filters wph [4][Cout][Cin][4] (ConvTranspose2d k4 s2 p1, conv_mfma.hip).
void conv_pack_phases_host(const float* wph, int Cout, int Cin, const int* cin_map, int cin_packed, int BN, bool swizzle,
                           float* dst);
// LDS-DMA tile configurations: id -> (BM, BN); returns false for an unknown id.
bool conv_dma_tile(int dma_cfg, int* BM, int* BN);
struct ConvArgs;
hipError_t conv_dma_launch_kernel(const ConvLayer& L, const ConvArgs& a, int blocks, hipStream_t stream);

struct ConvPlan {           // launch geometry of one layer at one problem size
    int mtiles, ntiles, splits, chunks_per_split, Mpad, Npad;
    size_t partial_elems;   // 0 when splits == 1
};
ConvPlan conv_plan(const ConvLayer& L, int M, int force_splits = 0);

struct ConvIO {
    const float* in0; const float* in1;
    int B, Hin, Win;
    int act, pool, nchw;
    const float* resid;
    float* out; float* out2; const float* s2; const float* t2;
    float* partial;         // split-K workspace
    size_t partial_cap;     // its capacity in floats (the slice count is clamped to fit)
    int split_n;            // ConvArgs::split_n
};
hipError_t conv_launch(const ConvLayer& L, const ConvIO& io, hipStream_t stream, int force_splits = 0);

// ---- spatial-patch (halo in LDS) kernel for the collapsed UpBlock2d convolution (conv_mfma_patch.hip)
struct PatchLayer {
    int C0 = 0, C1 = 0, Cout = 0;
    float* w = nullptr;     // device, packed [ntile][cchunk][phase][tap][64][32]
    float* w_poly = nullptr;  // device, polyphase minimal-filtering form [ntile 32][cchunk][point 9][32][32] (conv_mfma_patch_poly.hip)
    float* w_poly3 = nullptr; // device, layers whose whole-tile launches run the split-bf16 product form: the same U as three bf16
                              // planes (patch_poly_pack_split_host); nullptr: fp32 form only
    float* bias = nullptr;  // device, [ntiles*64]
};
size_t patch_packed_elems(int Cin_packed, int Cout);
size_t patch_poly_packed_elems(int Cin_packed, int Cout);
void patch_poly_pack_host(const float* w_oihw_3x3, int Cout, int Cin, const int* cin_map, int cin_packed, float* dst);
// U as three bf16 planes whose sum is patch_poly_pack_host's float exactly; patch_poly_split_packed_elems: its size in FLOATS (x 1.5)
size_t patch_poly_split_packed_elems(int Cin_packed, int Cout);
void patch_poly_pack_split_host(const float* w_oihw_3x3, int Cout, int Cin, const int* cin_map, int cin_packed, uint16_t* dst);
// splits > 1: the channel reduction split over that many workgroups per tile, raw sums into partial[splits][B,2H,2W,Cout]
// (partial_cap floats), finished by patch_poly_reduce_kernel; patch_poly_splits picks the split for a launch
hipError_t patch_poly_launch(const PatchLayer& L, const float* in0, const float* in1, int B, int H, int W, int act,
                             float* out, hipStream_t stream, int splits = 1, float* partial = nullptr, size_t partial_cap = 0);
int patch_poly_splits(const PatchLayer& L, int B, int H, int W, int max_splits, int cus);
void patch_pack_host(const float* w_oihw_3x3, int Cout, int Cin, const int* cin_map, int cin_packed, float* dst);
hipError_t patch_phase_launch(const PatchLayer& L, const float* in0, const float* in1, int B, int H, int W, int act,
                              float* out, hipStream_t stream);

// ---- column-patch kernel for the 7x1 convolution of the final layer (conv_col7.hip): in [B,H,W,C] (C = 32 or 64),
// w = conv_pack_host(..., kh 7, kw 1, BN 32, swizzle) image [C/32][7][32][32], out [B,H,W,32]
hipError_t conv_col7_launch(const float* in, int C, int B, int H, int W, const float* w_swizzled, float* out,
                            hipStream_t stream);
// the same with the horizontal gather, bias and sigmoid in the tile epilogue: out_nchw [B,3,H,W] = sigmoid(conv7x7 + bias)
// (weights: the row-split image above built from a 3-output-channel 7x7 filter, bias [3] on the device)
// w_split: the same weights as three bf16 planes (col7_pack_split_host), with which the products run in the split-bf16 form
// (fp32-exact to 2^-24 relative); nullptr: fp32 MFMA products
hipError_t conv_col7_fused_launch(const float* in, int C, int B, int H, int W, const float* w_swizzled, const float* bias,
                                  float* out_nchw, hipStream_t stream, const float* w_split = nullptr);
// the row-split weights [Cout <= 21][Cin][7] as three bf16 planes whose sum is the fp32 weight exactly; col7_split_packed_elems: the
// image's size in FLOATS
size_t col7_split_packed_elems(int cin_packed);
void col7_pack_split_host(const float* w_rowsplit, int Cout, int Cin, const int* cin_map, int cin_packed, uint16_t* dst);

// the plain form's second half: the seven horizontal taps gathered, bias, sigmoid
hipError_t final_shift_sum_launch(const float* part /*[n,H,W,32]: channel dx*3+co*/, const float* bias /*[3] dev*/,
                                  int n, int H, int W, float* out /*[n,3,H,W]*/, hipStream_t s);
// streamed-weight variant for the row-split flow head: two concatenated inputs, N = ntile32*32 (3 -> 96), weights packed with
// conv_pack_host(..., kh 7, kw 1, BN 96, swizzle); out [B,H,W,pixel_stride]
hipError_t conv_col7s_launch(const float* in0, int C0, const float* in1, int C1, int B, int H, int W, const float* w_swizzled,
                             int ntile32, float* out, int pixel_stride, hipStream_t stream);

// ---- Winograd paths for the bottleneck convolutions: F(2x2,3x3) (conv_winograd.hip), F(4x4,3x3) (conv_winograd4.hip)
struct WinoLayer {
    int Cin = 0, Cout = 0, BN = 128, ntiles = 0;
    int tile = 2;           // output tile side: 2 -> 16 transform points, BN 128; 4 -> 36 points, BN 64
    float* u = nullptr;     // device, packed [ntiles][(tile+2)^2*Cin/32][BN][32]
    float* u3 = nullptr;    // device, tile 4 and Cin % 128 == 0 (host-packed layers): the same U as three bf16 planes
                            // (wino4_pack_split_host) for the split-bf16 product form; nullptr: fp32 form only
    float* bias = nullptr;  // device, [ntiles*BN]
};
size_t wino_packed_elems(int Cout, int Cin, int BN);
void wino_pack_host(const float* w_oihw, int Cout, int Cin, int BN, float* dst);
// V[16][B*H/2*W/2][C] = B^T d B of x (optionally of relu(x*s + t))
hipError_t wino_transform_launch(const float* x, const float* s, const float* t, int B, int H, int W, int C, float* V,
                                 hipStream_t stream);
hipError_t wino_gemm_launch(const WinoLayer& L, const float* V, int B, int H, int W, int act, const float* resid,
                            float* out, hipStream_t stream);

size_t wino4_packed_elems(int Cout, int Cin, int BN);
void wino4_pack_host(const float* w_oihw, int Cout, int Cin, int BN, float* dst);
// U as three bf16 planes whose sum is wino4_pack_host's float exactly; wino4_split_packed_elems: its size in FLOATS (x 1.5)
size_t wino4_split_packed_elems(int Cout, int Cin, int BN);
void wino4_pack_split_host(const float* w_oihw, int Cout, int Cin, int BN, uint16_t* dst);
// V[36][B*H/4*W/4][C] = B^T d B of x (optionally of relu(x*s + t)); H, W multiples of 4
hipError_t wino4_transform_launch(const float* x, const float* s, const float* t, int B, int H, int W, int C, float* V,
                                  hipStream_t stream);
// variant: the GEMM's software pipeline, 0 | 3 | 6 (conv_winograd4.hip)
// groups in {1,2,3,6}: > 1 splits the six rows of transform points over that many workgroups per tile (few tiles) and
// finishes with wino4_output_transform_kernel; zbuf: [24][B*H/4*W/4][Cout] floats; pool (groups > 1 only): 2x2 average
// after the activation, out is [B,H/2,W/2,Cout]
hipError_t wino4_gemm_launch(const WinoLayer& L, const float* V, int B, int H, int W, int act, const float* resid,
                             float* out, hipStream_t stream, int variant = 0, int groups = 1, float* zbuf = nullptr, int pool = 0);

// ---- the generator's first block: 7x7 conv 3 -> Cout (+ folded BatchNorm, ReLU) from the NCHW source (conv_first.hip)
bool first7_supported(int Cout);
void first7_pack_host(const float* w_oihw_7x7_folded, int Cout, float* dst /*[196][Cout]*/);
hipError_t first7_launch(const float* src /*[ns,3,H,W]*/, const float* w_packed, const float* bias, int ns, int H, int W,
                         int Cout, float* out /*[ns,H,W,Cout]*/, hipStream_t stream);

// ---- dense-motion kernels: key-point records, front end, flow head, source preparation; layout and format changes (motion.hip)
hipError_t kp_prepare_launch(const float* kd_val, const float* kd_jac, const float* ks_val, const float* ks_jac,
                             int n, int ns, int K, float* kp_rec, int* bad_flag, hipStream_t s);
hipError_t motion_front_launch(const float* kp_rec, const float* src_small /*[ns,h,w,4]*/, int n, int ns, int K,
                               int h, int w, float variance, int Cpad, float* hg_in /*[n,h,w,Cpad]*/,
                               float* sparse_deformed /*[n,K+1,channels,h,w] or null*/, hipStream_t s, int groups = 1,
                               int channels = 3, size_t group_stride = 0);   // groups of three image channels
hipError_t motion_head_launch(const float* logits /*[n,h,w,32]*/, const float* kp_rec, int n, int K, int h, int w,
                              int has_occ, float* deformation /*[n,h,w,2]*/, float* occlusion /*[n,h,w]*/,
                              float* mask_out /*[n,K+1,h,w] or null*/, float* occ_out /*[n,1,h,w] or null*/,
                              hipStream_t s);
// the training entry's form: mask logits [n,h,w,ld] (channels 0..K), occlusion logit [n,h,w,ldo] (channel 0) or null
hipError_t motion_head_forward_launch(const float* lm, int ld, const float* lo, int ldo, const float* rec, int n, int K, int h, int w,
                                      float* mask, float* deformation, float* occlusion, hipStream_t s);
hipError_t motion_head_rowsplit_launch(const float* part /*[n,h,w,PS]: channel dx*NC+co*/, int PS, int NC,
                                       const float* bias /*[NC] dev*/, const float* kp_rec, int n, int K, int h, int w,
                                       int has_occ, float* deformation, float* occlusion, float* mask_out,
                                       float* occ_out, hipStream_t s);
hipError_t broadcast_features_launch(const float* feat /*[ns,hf,wf,C]*/, int n, int ns, int hf, int wf, int C, float* out,
                                     float* out2, const float* s2, const float* t2, hipStream_t s);
hipError_t source_prepare_launch(const float* src /*[ns,3,H,W]*/, const float* aa_w /*[3,13,13] dev*/, int ns, int H,
                                 int W, int inv_scale, int Cpad, float* src_nhwc /*[ns,H,W,Cpad]*/,
                                 float* src_small /*[ns,h,w,4]*/, hipStream_t s);
hipError_t antialias_down_launch(const float* src /*[ns,3,H,W]*/, const float* aa_w, int ns, int H, int W,
                                 int inv_scale, int Cpad, float* dst /*[ns,h,w,Cpad]: RGB + zeros*/, hipStream_t s,
                                 int src_planes = 3, int first_channel = 0, int channels = 3, int slot = 0);
hipError_t nchw_to_nhwc_pad_launch(const float* src /*[B,planes,H,W]*/, int B, int C, int H, int W, int Cpad,
                                   float* dst /*[B,H,W,Cpad]*/, hipStream_t s, int planes = 0 /*0: = C; else the first C of them*/);
hipError_t to_u8_launch(const float* pred /*[n,3,H,W]*/, int n, int H, int W, uint8_t* out /*[n,H,W,3]*/,
                        hipStream_t s);
// ---- the key-point heads' reduction, forward and backward (kp_head.hip)
hipError_t kp_head_launch(const float* logits /*[B,h,w,Cs]*/, int B, int K, int njm, int h, int w, int Cs, int pad,
                          float temperature, float* value /*[B,K,2]*/, float* jacobian /*[B,K,2,2] or null*/,
                          float* heatmap /*[B,K,h-6+2pad,w-6+2pad] or null*/, hipStream_t s,
                          float* ws = nullptr /* kp_head_workspace_floats(B, K) floats: batched calls run the pixel-sliced form */,
                          float* stats = nullptr /*[B,K,2]: the softmax's (maximum, denominator), what the backward reads*/);
constexpr int KP_HEAD_SLICES = 8;
size_t kp_head_workspace_floats(int B, int K);
// its backward: any of the three gradients may be null; grad_logits is fully written
constexpr int KP_HEAD_BWD_SLICES = 32;
size_t kp_head_backward_workspace_floats(int B, int K);
hipError_t kp_head_backward_launch(const float* logits /*[B,h,w,Cs]*/, const float* stats /*[B,K,2]*/, const float* value /*[B,K,2]*/,
                                   const float* jacobian /*[B,K,2,2] or null*/, const float* g_value, const float* g_jacobian,
                                   const float* g_heatmap, int B, int K, int njm, int h, int w, int Cs, int pad, float temperature,
                                   float* grad_logits /*[B,h,w,Cs]*/, float* ws /* kp_head_backward_workspace_floats(B, K) */, hipStream_t s);
// ---- the warps by the flow (warp.hip); the backward ACCUMULATES its three gradients into zeroed buffers
hipError_t warp_features_launch(const float* feat /*[ns,hf,wf,C]*/, const float* deformation /*[n,h,w,2]*/,
                                const float* occlusion /*[n,h,w] or null*/, int n, int ns, int hf, int wf, int C,
                                int h, int w, float* out, float* out2, const float* s2, const float* t2,
                                hipStream_t s);
hipError_t warp_image_launch(const float* src /*[ns,3,H,W]*/, const float* deformation /*[n,h,w,2]*/, int n, int ns,
                             int H, int W, int h, int w, float* out /*[n,channels,H,W]*/, hipStream_t s, int src_planes = 3,
                             int channels = 3);
hipError_t warp_features_backward_launch(const float* feat, const float* defo, const float* occ, const float* dout, int n, int ns,
                                         int hf, int wf, int C, float* dfeat, float* ddefo, float* docc, hipStream_t s);
// ---- training-mode BatchNorm forward (batchnorm.hip; SURVEY.md 8f row N4, first slice)
size_t bn_workspace_floats(int N, int C, int HW);
hipError_t bn_local_sums_launch(const float* x /*[N,C,HW]*/, int N, int C, int HW, float* sums /*[6C+2]*/, float* workspace,
                                hipStream_t s);
hipError_t bn_finalize_launch(const float* sums, int C, float eps, float momentum, int mode, const float* weight,
                              float* running_mean, float* running_var, float* mean, float* scale, float* inv_std /*[C] or null*/,
                              hipStream_t s);
// backward (round 3): sums in the forward's packed layout [6C+2]; coef [3C] = S1/N, S2*inv_std^2/N, weight*inv_std
hipError_t bn_bwd_sums_launch(const float* x, const float* dy, const float* mean, int N, int C, int HW, float* sums, float* workspace,
                              hipStream_t s);
hipError_t bn_bwd_finalize_launch(const float* local, const float* reduced, int C, const float* inv_std, const float* weight, float eps,
                                  int mode, float* dweight, float* dbias, float* coef, hipStream_t s);
hipError_t bn_bwd_apply_launch(const float* x, const float* dy, const float* mean, const float* coef, int N, int C, int HW, float* dx,
                               hipStream_t s);
hipError_t bn_apply_launch(const float* x, const float* mean, const float* scale, const float* bias, int N, int C, int HW,
                           float* y, hipStream_t s);
// NHWC variants for the engine's training-mode forward (batchnorm_nhwc.hip); sums / finalize as above
// The finalize step of one replica folded into bn_combine_kernel (kind 1: bn_finalize_kernel's modes 0 / 1; kind 2:
// bn_bwd_finalize_kernel's with reduced == local): nothing is exchanged in between and the step reads only its own channel's totals.
struct BnFuse {
    int kind = 0, mode = 1;
    float eps = 0.f, momentum = 0.f;
    const float* weight = nullptr;
    float *running_mean = nullptr, *running_var = nullptr, *mean = nullptr, *scale = nullptr, *inv_std_out = nullptr;   // kind 1
    const float* inv_std = nullptr;                                                                                   // kind 2
    float *dweight = nullptr, *dbias = nullptr, *coef = nullptr;
};
hipError_t bn_combine_launch(const double* partial /*[C][P][2]*/, int C, int P, long long count, float* sums /*[6C+2]*/, hipStream_t s,
                             const BnFuse* fuse = nullptr);
size_t bn_nhwc_workspace_floats(long long M, int C);
hipError_t bn_nhwc_sums_launch(const float* x /*[M,C]*/, long long M, int C, float* sums /*[6C+2]*/, float* workspace, hipStream_t s,
                               const BnFuse* fuse = nullptr);
hipError_t bn_nhwc_apply_launch(const float* x /*[B,H,W,C]*/, const float* mean, const float* scale, const float* bias, int B, int H,
                                int W, int C, int relu, int pool, float* y, hipStream_t s);
// backward of the fused tail y = [avgpool2x2](act(BatchNorm(x))) on NHWC: packed sums like bn_bwd_sums_launch, then dx with
// bn_bwd_finalize_launch's coefficients (the ReLU mask is recomputed from x)
hipError_t bn_nhwc_bwd_sums_launch(const float* x, const float* dy, const float* mean, const float* scale, const float* bias, int B, int H,
                                   int W, int C, int relu, int pool, float* sums, float* workspace, hipStream_t s,
                                   const BnFuse* fuse = nullptr);
hipError_t bn_nhwc_bwd_apply_launch(const float* x, const float* dy, const float* mean, const float* scale, const float* bias,
                                    const float* coef, int B, int H, int W, int C, int relu, int pool, float* dx, hipStream_t s);

// backward.hip: gradients of a stride-1 "same" convolution's weights and bias (NHWC activations, OIHW gradient)
size_t conv_wgrad_workspace_floats(int B, int H, int W, int Cin, int Cout, int kh, int kw);
hipError_t conv_wgrad_launch(const float* x, const float* dy, int B, int H, int W, int Cin, int Cout, int kh, int kw, float* dweight,
                             float* dbias, float* workspace, size_t workspace_floats, hipStream_t s, const float* x_transformed = nullptr);
bool conv_wgrad_takes_transformed(int B, int H, int W, int Cin, int Cout, int kh, int kw);
// dW [Cout,Cin,taps] = the pixel-split slabs partial[splits][taps][Mpad][Npad] added in slice order (also the stride-2 weight gradient's)
hipError_t conv_wgrad_reduce_launch(const float* partial, int splits, int taps, int Mpad, int Npad, int Cout, int Cin, float* dw, hipStream_t s);
// The weight gradient of a stride-2 pair of maps (backward.hip's strided_wgrad_kernel): dW[r][c][ky][kx] = sum over the pixels (y, x) of
// dense [B,H,W,rows] of dense[y, x][r] * gathered[2y + ky - pad, 2x + kx - pad][c], gathered [B,2H,2W,cols] (zeros outside), ks x ks taps;
// one GEMM per tap, split over the pixels, the slabs summed in slice order into dweight [rows][cols][ks][ks].  workspace: the query's
// floats (P = B*H*W), 16-byte aligned.  conv_s2_wgrad_launch: dense = dY, gathered = x, pad = ks / 2; deconv4s2_wgrad_launch: dense = x,
// gathered = dY, ks = 4, pad = 1.  With `stride`, `Hg`, `Wg` given the gathered map is [B,Hg,Wg,cols] read at (stride y + ky - pad,
// stride x + kx - pad): disc_conv4_wgrad_launch has stride 1, pad 0, Hg = H + 3, Wg = W + 3.
size_t strided_wgrad_workspace_floats(int P, int rows, int cols, int ks);
hipError_t strided_wgrad_launch(const float* dense, const float* gathered, int B, int H, int W, int rows, int cols, int ks, int pad,
                                float* dweight, float* workspace, hipStream_t s, int stride = 2, int Hg = 0, int Wg = 0);
// db[Cout] = sum over the P pixels of dy [P][Cout] (Cout a multiple of 4, <= 1024), two fixed-order stages; workspace: the query's floats
size_t conv_bias_grad_workspace_floats(int Cout);
hipError_t conv_bias_grad_launch(const float* dy, long long P, int Cout, float* dbias, float* workspace, hipStream_t s);

// disc_conv4.hip: the discriminator's valid 4x4 convolution (NHWC, OIHW device filter packed into `workspace` on every call).
// pad = 0, transposed = 0: the forward; pad = 3, transposed = 1: the data gradient (x = dY, weight = the forward filter).  thin = 4 | 8 |
// 16: the side with few channels is [.,thin] floats per pixel (forward: the input, Cin = the filter's channels <= thin; data gradient:
// the output, Cout = the filter's channels <= thin, zeros above).  *_refusal: null, or why the shape is refused.
const char* disc_conv4_refusal(int B, int H, int W, int Cin, int Cout, int pad, int transposed, int thin);
size_t disc_conv4_workspace_floats(int B, int H, int W, int Cin, int Cout, int pad, int transposed, int thin);
hipError_t disc_conv4_launch(const float* x, int B, int H, int W, int Cin, const float* weight, const float* bias, int Cout, int pad,
                             int transposed, int thin, float* out, float* workspace, hipStream_t s);
// x [B,H,W,Cx] (Cx 4 | 8 | 16 | a multiple of 32), dy [B,H-3,W-3,Cout] -> dweight [Cout,Cx,4,4], dbias [Cout] or null
const char* disc_conv4_wgrad_refusal(int B, int H, int W, int Cx, int Cout);
size_t disc_conv4_wgrad_workspace_floats(int B, int H, int W, int Cx, int Cout);
hipError_t disc_conv4_wgrad_launch(const float* x, const float* dy, int B, int H, int W, int Cx, int Cout, float* dweight, float* dbias,
                                   float* workspace, hipStream_t s);
// disc_norm.hip: InstanceNorm2d(affine) (norm = 1) + LeakyReLU(0.2) + AvgPool2d(2) (pool = 1, floor sizes) on x [B,H,W,C], and its
// backward from the saved x and stats [B,C,2] doubles = (mean, rstd).  workspace: disc_norm_workspace_floats floats, 16-byte aligned.
const char* disc_norm_refusal(int B, int H, int W, int C, int norm, int pool);
size_t disc_norm_workspace_floats(int B, int H, int W, int C, int norm, int backward);
hipError_t disc_norm_act_pool_launch(const float* x, const float* gamma, const float* beta, int B, int H, int W, int C, int norm, int pool,
                                     float eps, double* stats, float* out, float* workspace, hipStream_t s);
hipError_t disc_norm_act_pool_backward_launch(const float* x, const double* stats, const float* gamma, const float* beta, const float* dout,
                                              int B, int H, int W, int C, int norm, int pool, float* dx, float* dgamma, float* dbeta,
                                              float* workspace, hipStream_t s);

// conv_pack_dev.hip: the packings of conv_pack_host (register-staged kernel) and wino4_pack_host from a DEVICE OIHW tensor;
// transposed = 1 reads the forward filter [Cin][Cout][kh][kw] transposed and flipped (the data gradient's filter)
hipError_t conv_pack_dev_launch(const float* w, int Cout, int Cin, int T, int BN, int transposed, float* dst, hipStream_t s);
hipError_t wino4_pack_dev_launch(const float* w, int Cout, int Cin, int BN, int transposed, float* dst, hipStream_t s);
hipError_t bias_pad_dev_launch(const float* b, int Cout, int n, float* dst, hipStream_t s);
hipError_t col7_pack_dev_launch(const float* w_3c77, int C, float* dst /*[7*C/32][32][32]*/, hipStream_t s);

// conv7_thin.hip: the 7x7 layers with three channels on one side (training path); thin tensors are [B,H,W,4] (4th channel 0)
size_t conv7_thin_workspace_floats(int B, int H, int W, int N);
hipError_t conv7_thin_in_launch(const float* thin, const float* w, const float* bias, int B, int H, int W, int N, int transposed,
                                float* out, float* workspace, hipStream_t s);
hipError_t conv7_thin_wgrad_launch(const float* thin, const float* wide, int B, int H, int W, int N, int thin_is_input, float* dw,
                                   float* workspace, hipStream_t s);

// ---- backward of the dense-motion kernels (motion_backward.hip)
hipError_t antialias_down_backward_launch(const float* dsmall /*[B,h,w,4]*/, const float* aa_w, int B, int H, int W, int inv_scale,
                                          float* dsrc /*[B,3,H,W]*/, hipStream_t s);
hipError_t kp_records_backward_launch(const float* kd_jac, const float* ks_jac, const float* drec, int n, int K, float* dkd_val,
                                      float* dks_val, float* dkd_jac, float* dks_jac, hipStream_t s);
size_t motion_backward_workspace_floats(int n, int K, int h, int w);
hipError_t motion_front_backward_launch(const float* rec, const float* src_small, int n, int K, int h, int w, float variance, int Cpad,
                                        const float* dhg, const float* dsd, float* dsrc_small, float* drec, float* workspace,
                                        hipStream_t s);
hipError_t motion_head_backward_launch(const float* mask, const float* occlusion, const float* rec, int n, int K, int h, int w,
                                       const float* dmask, const float* ddef, const float* docc, float* dlm, int ld, float* dlo, int ldo,
                                       float* drec, float* workspace, hipStream_t s);

// One-Euro smoothing of [T,E] sequences along T (keypoints.hip; reference filter1.py:13-47 as driven by demo.py:241-250).
// Emotion detector Emotion_k (conv_s2.hip, emotion.hip).  conv_s2_launch: a stride-2 KSxKS convolution (KS 1 or 3, pad KS/2) of a
// plain pack_conv layer on NHWC [B,Hin,Win,C0] (Hin, Win even) -> [B,Hin/2,Win/2,Cout], bias + resid + act epilogue, split-K through
// `partial` (at most partial_cap floats; conv_s2_partial_elems: the plan's need).
size_t conv_s2_partial_elems(const ConvLayer& L, int B, int Hin, int Win);
hipError_t conv_s2_launch(const ConvLayer& L, const float* in, int B, int Hin, int Win, int act, const float* resid, float* out,
                          float* partial, size_t partial_cap, hipStream_t stream);
hipError_t emo_maxpool_launch(const float* in /*[B,H,W,C]*/, int B, int H, int W, int C, float* out /*[B,H/2,W/2,C]*/, hipStream_t s);
hipError_t emo_avgpool_launch(const float* in /*[B,P,C]*/, int B, int P, int C, float* out /*[B,C]*/, hipStream_t s);
hipError_t emo_embed_launch(const float* value /*[B,10,2]*/, const float* jacobian /*[B,10,2,2]*/, int B, float* out /*[B,1260]*/,
                            hipStream_t s);
hipError_t emo_linear_launch(const float* x0, int K0, const float* x1, int K1, const float* wt /*[K0+K1][O]*/, const float* bias, int O,
                             int B, int relu, float* out /*[B,O]*/, hipStream_t s);
hipError_t emo_final_launch(const float* a /*[B,64]*/, const float* w /*98 floats*/, int B, float* value, float* jacobian, hipStream_t s);

// conv_s2_backward.hip: data and weight gradient of the stride-2 convolution above from DEVICE tensors (OIHW filter [Cout,Cin,ks,ks],
// ks 1 | 3, no bias; Hin, Win even; Cin, Cout multiples of 32).  *_workspace_floats is 0 for an unsupported shape; the data
// gradient packs its filter into the workspace, the weight gradient keeps its pixel-split slabs there.  dx / dweight fully written.
bool conv_s2_backward_supported(int B, int Hin, int Win, int Cin, int Cout, int ks);
size_t conv_s2_dgrad_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int ks);
hipError_t conv_s2_dgrad_launch(const float* dy /*[B,Hin/2,Win/2,Cout]*/, const float* weight, int B, int Hin, int Win, int Cin, int Cout,
                                int ks, float* dx /*[B,Hin,Win,Cin]*/, float* workspace, size_t workspace_floats, hipStream_t s);
size_t conv_s2_wgrad_workspace_floats(int B, int Hin, int Win, int Cin, int Cout, int ks);
hipError_t conv_s2_wgrad_launch(const float* x /*[B,Hin,Win,Cin]*/, const float* dy /*[B,Hin/2,Win/2,Cout]*/, int B, int Hin, int Win, int Cin,
                                int Cout, int ks, float* dweight /*[Cout,Cin,ks,ks]*/, float* workspace, size_t workspace_floats, hipStream_t s);
// emotion_backward.hip: MaxPool2d(3, 2, 1) backward (the winner recomputed from the saved input, ATen's first-maximum rule) and the
// backward of emo_final_kernel: da [B,64], dw [98] summed over the frames in their order (workspace: B * 98 floats)
hipError_t emo_maxpool_backward_launch(const float* in /*[B,H,W,C]*/, const float* dy /*[B,H/2,W/2,C]*/, int B, int H, int W, int C,
                                       float* dx /*[B,H,W,C]*/, hipStream_t s);
size_t emo_final_backward_workspace_floats(int B);
hipError_t emo_final_backward_launch(const float* a /*[B,64]*/, const float* w /*98 floats*/, const float* g_value /*[B,4,2] or null*/,
                                     const float* g_jacobian /*[B,4,2,2] or null*/, int B, float* da /*[B,64]*/, float* dw /*[98]*/,
                                     float* workspace, hipStream_t s);

// Audio network AT_net2 (audio.hip): the first audio convolution 1 -> 64 (BatchNorm folded: w [9][64], b [64]) + ReLU from the raw
// [F,H,W] MFCC windows to NHWC [F,H,W,64]; MaxPool2d(3, (sy, sx)) without padding on NHWC (C % 4 == 0); x *= scale.
hipError_t audio_conv1_launch(const float* x, const float* w, const float* b, int F, int H, int W, float* out, hipStream_t s);
hipError_t audio_maxpool_launch(const float* in, int F, int H, int W, int C, int sy, int sx, float* out, hipStream_t s);
hipError_t audio_scale_launch(float* x, size_t n, float scale, hipStream_t s);
// One LSTM layer (hidden 256, gates i f g o) over S steps for N <= 8 clips in one persistent launch of LSTM_WG workgroups.
constexpr int LSTM_WG = 16;
struct LstmArgs {
    const float* whh;            // lstm_pack_whh_host image [16][256][64]
    const float* xproj;          // [N*S][1024] input projection of step s of clip n at row n*S + s, biases included
    const float* clipb;          // [N][1024] added to every step of clip n, or null
    int N, S;
    const float* h0;             // [N][256] h before the first step
    float* hT;                   // [N][256] h after the last step (must not overlap h0)
    float* c;                    // [N][256] cell state: read first, overwritten with the state after the last step
    float* y;                    // h of step s of clip n at y[n * ystride + s * 256]
    long long ystride;
    unsigned long long* gran;    // [2][8][256] tagged hand-off words
    unsigned epoch0;             // tag of the first step (step s: epoch0 + s); tags must never repeat on one gran buffer
    unsigned long long limit;    // wall-clock ticks one wait may take before the error word is set
    int* err;                    // host-visible error word
};
void lstm_pack_whh_host(const float* whh /*[1024][256]*/, float* dst /*[16][256][64]*/);
hipError_t lstm_rec_launch(const LstmArgs& a, hipStream_t s);
// lstm_backward.hip: what the differentiable LSTM operator needs around lstm_rec_kernel.  lstm_pack_whh_dev_launch:
// lstm_pack_whh_host on a DEVICE W_hh.  lstm_scan_launch: gate pre-activations [N,T,1024] -> activated gates in place + c [N,T,256].
// lstm_bwd_launch: the backward recurrence (one persistent launch of LSTM_WG workgroups), dx = the gate gradients [N,T,1024].
struct LstmBwdArgs {
    const float* whh;            // W_hh [1024][256] as nn.LSTM keeps it
    const float* acts;           // [N,T,1024] activated gates i f g o (lstm_scan_launch)
    const float* c;              // [N,T,256] cell states (lstm_scan_launch)
    const float* dy;             // [N,T,256] gradient of the layer's output
    float* dx;                   // [N,T,1024] gradient of the input projection, fully written (NaN after a timed-out wait)
    int N, T;
    unsigned long long* gran;    // [2][8][1024] tagged hand-off words, ZEROED before the launch (tags are 1 .. T)
    unsigned long long limit;    // wall-clock ticks one wait may take before the error word is set
    int* err;                    // host-visible error word
};
hipError_t lstm_pack_whh_dev_launch(const float* whh /*[1024][256]*/, float* dst /*[16][256][64]*/, hipStream_t s);
hipError_t lstm_scan_launch(float* gates, int N, int T, float* c, hipStream_t s);
hipError_t lstm_bwd_launch(const LstmBwdArgs& a, hipStream_t s);
// audio_backward.hip: MaxPool2d(3, (sy, sx)) backward (each window's winner recomputed, first maximum in row-major order; a gather
// per input pixel, no atomics) and ConvTranspose2d(k4, s2, p1) on NHWC with the reference's filter [Cin,Cout,4,4] ON THE DEVICE
// (Cin, Cout multiples of 32): forward (+ bias, nullable), data gradient, weight (+ bias, nullable) gradient.  *_workspace_floats
// is 0 for an unsupported shape.
hipError_t audio_maxpool_backward_launch(const float* in, const float* dy, int F, int H, int W, int C, int sy, int sx, float* dx, hipStream_t s);
size_t deconv4s2_workspace_floats(int B, int H, int W, int Cin, int Cout, int which /*0 forward, 1 data gradient, 2 weight gradient*/);
hipError_t deconv4s2_forward_launch(const float* x, const float* weight, const float* bias, int B, int H, int W, int Cin, int Cout, float* out,
                                    float* workspace, size_t workspace_floats, hipStream_t s);
hipError_t deconv4s2_dgrad_launch(const float* dy, const float* weight, int B, int H, int W, int Cin, int Cout, float* dx, float* workspace,
                                  size_t workspace_floats, hipStream_t s);
hipError_t deconv4s2_wgrad_launch(const float* x, const float* dy, int B, int H, int W, int Cin, int Cout, float* dweight, float* dbias,
                                  float* workspace, size_t workspace_floats, hipStream_t s);

// perceptual.hip: the pyramid perceptual loss around its convolutions.  vgg_input: one pyramid level of src [B,3,H,W] (inv 1: a copy)
// -> out [B,h,w,32] = (level - mean) / std in channels 0..2, zeros above, and / or level [B,3,h,w] (either may be null); its backward
// gathers g [B,h,w,Cg] (channels 0..2, divided by std) and / or glevel [B,3,h,w] -> dsrc [B,3,H,W].  relu_pool: x = relu(x) in place,
// pooled (or null) = MaxPool2d(2, 2) of it, sizes floored; backward dx = (y > 0) * (dy + dp at its window's first maximum), dy / dp
// nullable.  l1_pair: value[0] = weight * mean|a - b| through l1_pair_partials(n) doubles, g = (weight / n) sign(a - b).
hipError_t vgg_input_launch(const float* src, const float* aa_w, const float* mean, const float* stdv, int B, int H, int W, int inv,
                            float* out, float* level, hipStream_t s);
hipError_t vgg_input_backward_launch(const float* g, int Cg, const float* glevel, const float* aa_w, const float* stdv, int B, int H, int W,
                                     int inv, float* dsrc, hipStream_t s);
hipError_t relu_pool_launch(float* x /*[B,H,W,C]*/, int B, int H, int W, int C, float* pooled /*[B,H/2,W/2,C]*/, hipStream_t s);
hipError_t relu_pool_backward_launch(const float* y, const float* dy, const float* dp, int B, int H, int W, int C, float* dx, hipStream_t s);
int l1_pair_partials(long long n);
hipError_t l1_pair_launch(const float* a, const float* b, long long n, float weight, float* value, float* g, double* partial, hipStream_t s);
hipError_t l1_pair_backward_launch(const float* g, long long n, const float* grad_value, float* out, hipStream_t s);

// equivariance.hip: the equivariance constraint's Transform (affine theta [B,2,3] + thin-plate term, params [B,P*P], P = 0: none).
// tps_warp_frame: out [B,C,H,W] = grid_sample(frame, warp(grid), reflection) without a grid tensor.  tps_warp_points: coords
// [Bc,N,2] (Bc 1 or B) -> out [B,N,2], jac [B,N,2,2] (or null); its backward: gout / gjac (each nullable) -> gcoords [Bc,N,2].
hipError_t tps_warp_frame_launch(const float* frame, const float* theta, const float* params, int P, int B, int C, int H, int W, float* out,
                                 hipStream_t s);
hipError_t tps_warp_points_launch(const float* coords, int Bc, const float* theta, const float* params, int P, int B, int N, float* out,
                                  float* jac, hipStream_t s);
hipError_t tps_warp_points_backward_launch(const float* coords, int Bc, const float* theta, const float* params, int P, int B, int N,
                                           const float* gout, const float* gjac, float* gcoords, hipStream_t s);

// optim.hip: Adam over a LIST of tensors, a few launches for the whole list.  A launch carries its tensors BY VALUE in the kernel
// arguments (AdamTable: no device-side table, nothing that depends on host memory staying alive); a workgroup owns one chunk of
// `chunk` elements of one tensor and finds the tensor by a wave-uniform search over the table's prefix of workgroup counts.
constexpr int ADAM_TABLE = 64;             // tensors per launch: 64 x 52 bytes + the scalars stay below the 4 KiB of kernel arguments
constexpr int ADAM_BLOCK_ELEMS = 4096;     // E, the elements of a workgroup's chunk at multiplier 1: 256 threads x 4 float4
constexpr int ADAM_GRID_CAP = 8192;        // a launch whose chunks at E would be more than this many gets larger ones ...
constexpr int ADAM_MAX_MULT = 8;           // ... of up to 8 E elements
constexpr long long ADAM_MAX_NUMEL = 1ll << 36;   // per tensor: a full table's workgroup count stays below 2^31
struct AdamTable {
    float* p[ADAM_TABLE];
    const float* g[ADAM_TABLE];
    float* m[ADAM_TABLE];
    float* v[ADAM_TABLE];
    long long n[ADAM_TABLE];
    float step_size[ADAM_TABLE];           // lr / (1 - beta1^step), per tensor
    float bc2_sqrt[ADAM_TABLE];            // sqrt(1 - beta2^step), per tensor
    int first_block[ADAM_TABLE + 1];       // prefix of workgroup counts; entries beyond `count` repeat the total
    int count;
    int chunk;                             // elements per workgroup in this launch, a multiple of E
};
struct AdamLaunch {
    int first, count, blocks, chunk;       // tensors [first, first + count) of the list, `blocks` workgroups of `chunk` elements
};
// How a list of n lengths (each 0 .. ADAM_MAX_NUMEL) is cut into launches, in list order: at most ADAM_TABLE tensors each, a length-0
// tensor takes a table slot and no workgroup.  Writes at most `cap` launches; returns how many the list needs.
int adam_plan(int n, const long long* numel, AdamLaunch* launches, int cap);
hipError_t adam_launch(const AdamTable& table, float beta1, float one_minus_beta1, float beta2, float one_minus_beta2, float eps,
                       float weight_decay, hipStream_t s);

hipError_t one_euro_launch(const float* x, int T, int E, float mincutoff, float beta, float dcutoff, float freq, float scale,
                           float* out, hipStream_t stream, float* state = nullptr, int resume = 0);

// mfcc.hip: python_speech_features.mfcc(signal, 16000, winstep=0.01) of n_clips clips [n_clips][clip_stride] of n_samples each,
// padded virtually with `pad` zeros on each side -> out [n_clips][mfcc_frames(n_samples, pad)][13]
long long mfcc_frames(long long n_samples, int pad);
hipError_t mfcc_launch(const float* pcm, long long n_samples, int n_clips, long long clip_stride, int pad, float* out,
                       hipStream_t stream);

// video_prep.hip: the emotion video's resize (S0), similarity alignment (S1) and fused augmentation (S2..S6); 256 x 256 outputs
constexpr int VIDEO_MAX_RADIUS = 32;                 // Gaussian radius < 32 per axis: input sides up to about 4000 pixels
struct VideoResizeTaps {                             // normalised Gaussian taps, index i + r for offset i = -r .. r (r = 0: {1})
    double wy[2 * VIDEO_MAX_RADIUS - 1];
    double wx[2 * VIDEO_MAX_RADIUS - 1];
    int ry, rx;
};
struct VideoAugParams {
    double rot[6];                                   // S4: input (x', y') = [rot0 rot1 rot2; rot3 rot4 rot5] (x, y, 1)
    unsigned long long noise_seed;                   // device-hash seed (when no explicit noise is passed)
    int flip;                                        // S3: horizontal flip of the clip
    int mouth_x, mouth_y, mouth_w, mouth_h;          // S2: the noise rectangle (columns mouth_x .., rows mouth_y ..)
};
hipError_t resize_aa_launch(const unsigned char* in, int n, int H, int W, int C, const VideoResizeTaps& taps, unsigned char* out,
                            hipStream_t stream);
hipError_t similarity_warp_launch(const unsigned char* in, int n, int H, int W, int C, const double* maps, int mode, void* out,
                                  hipStream_t stream);
hipError_t emotion_augment_launch(const float* aligned, long long n_src, long long t0, int count, const double* hinv, const float* noise,
                                  const VideoAugParams& p, float* out, hipStream_t stream);

}  // namespace eamm
