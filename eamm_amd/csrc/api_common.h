// Shared internals of the C-ABI translation units (eamm_api.hip and its siblings, eamm_kp_api.hip, ...): handle base class, error
// reporting, device allocation, and the state_dict -> BatchNorm-folded, MFMA-packed layer builders.
#pragma once
#include "../../include/eamm_hip.h"
#include "kernels.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

namespace eamm {

// The text behind every *_last_error(NULL): the last failure, on this thread, of an entry that has no handle to report
// through (a create, an eamm_op_* operator).  ONE per thread for the whole library (an inline variable, unlike the helpers
// in the anonymous namespace below, of which every translation unit has its own copy): the generator's entries are spread
// over several translation units and eamm_last_error(NULL) must see all of them.
inline thread_local std::string g_create_error;

namespace {

struct HostTensor {
    std::vector<int64_t> shape;
    std::vector<float> data;
    size_t numel() const {
        size_t n = 1;
        for (auto s : shape) n *= (size_t)s;
        return n;
    }
};

// A convolution layer packed for the register-staged 128 x BN kernel and, where it pays, also for an LDS-DMA
// big-tile kernel; conv launches pick by problem size (see pick()).
struct LayerSet {
    ConvLayer base, dma, big;
    ConvLayer skinny32, skinny64;   // S.dma's weights (N tile 128) behind the 32- / 64-row LDS-DMA tiles: M <= 32 / 64
    bool has_skinny = false;
    PatchLayer patch;           // UpBlock2d layers only: spatial-patch kernel (conv_mfma_patch.hip)
    bool has_dma = false, has_big = false, has_patch = false;
};



// What every handle type carries: device, last error, the raw state_dict until finalisation, owned device memory
// and the convolution-tile tuning knobs (environment, read at create).
struct CtxBase {
    int device = 0;
    std::string err;
    std::map<std::string, HostTensor> sd;
    bool finalized = false;
    std::vector<void*> owned;   // every device allocation, freed by free_owned()
    int dma_min_m = 4608;       // smallest per-phase M for which an LDS-DMA tile is preferred (1024 until round 3: the 512x64 tile left the
                                // last hourglass decoder level at 8-32 workgroups for calls of 1-4 frames; one frame 1044 -> 1076 frames/s)
    int big_min_m = 49152;      // ... and for which Cout % 256 == 0 layers use the 256x256 tile (>= 192 M tiles)
    int dma_cfg_n256 = 2, dma_cfg_n128 = 2, dma_cfg_n64 = 3;
    int patch_poly = 1;         // up blocks on the patch kernel in the polyphase minimal-filtering form (EAMM_PATCH_POLY; 0: collapsed-phase form)
    int skinny_max_m = 16384;   // largest per-phase pixel count served by the 32- / 64-row tiles (EAMM_SKINNY_MAX_M; 0 = off):
                                // 64x128 tiles need no split-K where 256x128 ones do (measured 256x256: 1 frame 753 -> 785, 4 frames 1969 -> 2067,
                                // 8 frames 2756 -> 2782 frames/s; 16 frames unchanged)
    int patch_split_max = 4;    // largest split of the channel reduction of the polyphase kernel over workgroups (EAMM_PATCH_SPLIT_MAX; 1 = off)
    int patch_min_blocks = 128; // fewest workgroups for which UpBlock2d layers use the spatial-patch kernel (< 0: never)
};

// Every C entry point that touches the device runs under one of these: the handle's device becomes current for
// the call and the caller's current device is restored on return (PyTorch reads the current device from the HIP
// runtime, so a library that leaves another device selected would silently redirect the caller's later work).
struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t status = hipSuccess;
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != device) {
            status = hipSetDevice(device);
            switched = status == hipSuccess && prev >= 0;
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};

int fail(CtxBase* c, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

#define HIP_TRY(c, expr)                                                                        \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess)                                                                   \
            return fail((c), EAMM_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), \
                        __FILE__, __LINE__);                                                    \
    } while (0)

template <typename T>
int dev_alloc(CtxBase* c, T** p, size_t elems) {
    void* q = nullptr;
    HIP_TRY(c, hipMalloc(&q, std::max<size_t>(elems, 1) * sizeof(T)));
    c->owned.push_back(q);
    *p = reinterpret_cast<T*>(q);
    return 0;
}

int upload(CtxBase* c, float** dst, const std::vector<float>& src) {
    int rc = dev_alloc(c, dst, src.size());
    if (rc) return rc;
    HIP_TRY(c, hipMemcpy(*dst, src.data(), src.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

const HostTensor* find(const CtxBase* c, const std::string& key) {
    auto it = c->sd.find(key);
    return it == c->sd.end() ? nullptr : &it->second;
}

// y = ((conv(x) + b) - mean) * gamma / sqrt(var + eps) + beta   (sync_batchnorm/batchnorm.py:48-53, eps 1e-5): eval-mode
// BatchNorm (key prefix `norm`, may be empty) folded into per-channel scale and bias (fp64) of the convolution `conv`
int fold_norm(CtxBase* c, const std::string& conv, const std::string& norm, int Cout, std::vector<double>* scale,
              std::vector<double>* bias) {
    const HostTensor* bt = find(c, conv + ".bias");
    if (!bt || (int)bt->numel() != Cout) return fail(c, EAMM_ERR_KEY, "%s.bias missing or mis-shaped", conv.c_str());
    scale->assign(Cout, 1.0);
    bias->resize(Cout);
    for (int o = 0; o < Cout; ++o) (*bias)[o] = bt->data[o];
    if (norm.empty()) return EAMM_OK;
    const HostTensor *g = find(c, norm + ".weight"), *be = find(c, norm + ".bias"), *mu = find(c, norm + ".running_mean"),
                     *var = find(c, norm + ".running_var");
    if (!g || !be || !mu || !var || (int)g->numel() != Cout || (int)be->numel() != Cout || (int)mu->numel() != Cout ||
        (int)var->numel() != Cout)
        return fail(c, EAMM_ERR_KEY, "BatchNorm entries of %s missing or mis-shaped", norm.c_str());
    for (int o = 0; o < Cout; ++o) {
        const double s = (double)g->data[o] / std::sqrt((double)var->data[o] + 1e-5);
        (*scale)[o] = s;
        (*bias)[o] = ((*bias)[o] - (double)mu->data[o]) * s + (double)be->data[o];
    }
    return EAMM_OK;
}

// A convolution with its BatchNorm folded in, on the host: weights [Cout][Cin][kh][kw] (MODE_PHASES: four explicit 2x2
// phase filters [4][Cout][Cin][4]), bias [Cout].  What every packer below takes.
struct HostConv {
    int Cout = 0, Cin = 0, kh = 0, kw = 0;
    std::vector<float> w, b;
};

struct FoldSpec {
    std::string conv;            // key prefix holding .weight / .bias
    std::string norm;            // key prefix holding BatchNorm stats, or empty
};

// The ks x ks convolutions `parts` (Cin inputs each), BatchNorm folded, stacked along Cout (the flow head stacks mask +
// occlusion into one convolution, the key-point detector kp + jacobian)
int fold_conv(CtxBase* c, const std::vector<FoldSpec>& parts, int ks, int Cin, HostConv* f) {
    f->Cin = Cin;
    f->kh = f->kw = ks;
    f->Cout = 0;
    for (auto& ps : parts) {
        const HostTensor* wt = find(c, ps.conv + ".weight");
        if (!wt || wt->shape.size() != 4 || wt->shape[1] != Cin || wt->shape[2] != ks || wt->shape[3] != ks)
            return fail(c, EAMM_ERR_KEY, "state_dict entry %s.weight missing or mis-shaped (expected [*,%d,%d,%d])",
                        ps.conv.c_str(), Cin, ks, ks);
        f->Cout += (int)wt->shape[0];
    }
    const size_t per = (size_t)Cin * ks * ks;
    f->w.resize((size_t)f->Cout * per);
    f->b.resize(f->Cout);
    int o0 = 0;
    for (auto& ps : parts) {
        const HostTensor* wt = find(c, ps.conv + ".weight");
        const int co = (int)wt->shape[0];
        std::vector<double> s, b;
        if (int rc = fold_norm(c, ps.conv, ps.norm, co, &s, &b)) return rc;
        for (int o = 0; o < co; ++o) {
            f->b[o0 + o] = (float)b[o];
            for (size_t i = 0; i < per; ++i) f->w[(o0 + o) * per + i] = (float)((double)wt->data[o * per + i] * s[o]);
        }
        o0 += co;
    }
    return EAMM_OK;
}

// MODE_ROWSPLIT: the ks x ks filter as a ks x 1 one with N = (dx, co), w'[dx*Cout+co][c][dy] = w[co][c][dy][dx] -- the
// horizontal taps become output channels, gathered afterwards (final_shift_sum, the column-patch kernels).  The bias moves
// out (returned: the gather applies it); the new one is zero.
std::vector<float> to_rowsplit(HostConv* f) {
    const int ks = f->kh, Cout = f->Cout, Cin = f->Cin;
    std::vector<float> wr((size_t)ks * Cout * Cin * ks);
    for (int dx = 0; dx < ks; ++dx)
        for (int co = 0; co < Cout; ++co)
            for (int ci = 0; ci < Cin; ++ci)
                for (int dy = 0; dy < ks; ++dy)
                    wr[((size_t)(dx * Cout + co) * Cin + ci) * ks + dy] = f->w[((size_t)co * Cin + ci) * ks * ks + dy * ks + dx];
    f->w.swap(wr);
    f->Cout = ks * Cout;
    f->kw = 1;
    std::vector<float> row_bias(f->Cout, 0.f);
    f->b.swap(row_bias);
    return row_bias;
}

// Packed input channel -> channel of the filter: the C0_real + C1_real inputs of a concatenation [in0 | in1] whose halves
// are stored C0_packed / C1_packed wide (-1: a zero padding channel)
std::vector<int> channel_map(int C0_real, int C0_packed, int C1_real, int C1_packed) {
    std::vector<int> map(C0_packed + C1_packed, -1);
    for (int i = 0; i < C0_real; ++i) map[i] = i;
    for (int i = 0; i < C1_real; ++i) map[C0_packed + i] = C0_real + i;
    return map;
}

enum LayerMode { MODE_PLAIN = 0, MODE_PHASE = 1, MODE_ROWSPLIT = 2, MODE_PHASES = 3 };

// bias zero-padded to n floats -> device
int upload_bias(CtxBase* c, float** dst, const std::vector<float>& b, size_t n) {
    std::vector<float> pad(n, 0.f);
    std::copy(b.begin(), b.end(), pad.begin());
    return upload(c, dst, pad);
}

// Weights image of the implicit-GEMM kernels for an N tile of BN (swizzle: the LDS-DMA layout).  map: null, or
// channel_map()'s cin_packed entries.  MODE_PHASE collapses a 3x3 filter into the four 2x2 phase filters of "nearest x2 +
// 3x3"; MODE_PHASES takes those four filters as they are.
int upload_conv_image(CtxBase* c, float** dst, const HostConv& f, const int* map, int cin_packed, int BN, LayerMode mode,
                      bool swizzle) {
    const bool phase = mode == MODE_PHASE || mode == MODE_PHASES;
    std::vector<float> packed(conv_packed_elems(phase ? 4 : f.kh * f.kw, cin_packed, f.Cout, BN, phase ? 4 : 1));
    if (mode == MODE_PHASES)
        conv_pack_phases_host(f.w.data(), f.Cout, f.Cin, map, cin_packed, BN, swizzle, packed.data());
    else
        conv_pack_host(f.w.data(), f.Cout, f.Cin, f.kh, f.kw, map, cin_packed, BN, phase, swizzle, packed.data());
    return upload(c, dst, packed);
}

// The three-plane bf16 image of a row-split final layer (f: to_rowsplit's 7x1 filter with N = 21) for the split-bf16 form of the
// fused column-patch kernel (conv_col7.hip)
int upload_col7_split(CtxBase* c, float** dst, const HostConv& f, const int* map, int cin_packed) {
    std::vector<float> planes(col7_split_packed_elems(cin_packed));
    col7_pack_split_host(f.w.data(), f.Cout, f.Cin, map, cin_packed, reinterpret_cast<uint16_t*>(planes.data()));
    return upload(c, dst, planes);
}

// -> ConvLayer: the register-staged 128 x BN kernel (BN 0: conv_tile_n's), or (dma_cfg > 0) an LDS-DMA tile (conv_dma_tile)
int pack_conv(CtxBase* c, const HostConv& f, const int* map, int C0_packed, int C1_packed, LayerMode mode, int dma_cfg,
              ConvLayer* L, int BN = 0) {
    const bool phase = mode == MODE_PHASE || mode == MODE_PHASES;
    L->kh = f.kh;
    L->kw = f.kw;
    L->phase = phase;
    L->C0 = C0_packed;
    L->C1 = C1_packed;
    L->Cout = f.Cout;
    L->BM = 128;
    L->BN = BN ? BN : conv_tile_n(f.Cout);
    L->dma_cfg = dma_cfg;
    if (dma_cfg > 0 && !conv_dma_tile(dma_cfg, &L->BM, &L->BN)) return fail(c, EAMM_ERR_ARG, "unknown dma tile %d", dma_cfg);
    L->ntiles = (f.Cout + L->BN - 1) / L->BN;
    L->nchunks = (phase ? 4 : f.kh * f.kw) * ((C0_packed + C1_packed) / CONV_BK);
    if (int rc = upload_conv_image(c, &L->w, f, map, C0_packed + C1_packed, L->BN, mode, dma_cfg > 0)) return rc;
    return upload_bias(c, &L->bias, f.b, (size_t)L->ntiles * L->BN);
}

// -> PatchLayer: the spatial-patch kernel of the UpBlock2d convolution (3x3), polyphase or collapsed-phase form;
// split_planes: also the three-plane bf16 image of the polyphase form (a layer that only runs split over workgroups needs none)
int pack_patch(CtxBase* c, const HostConv& f, const int* map, int C0_packed, int C1_packed, bool poly, PatchLayer* P,
               bool split_planes = false) {
    const int cin_packed = C0_packed + C1_packed;
    P->C0 = C0_packed;
    P->C1 = C1_packed;
    P->Cout = f.Cout;
    std::vector<float> packed(poly ? patch_poly_packed_elems(cin_packed, f.Cout) : patch_packed_elems(cin_packed, f.Cout));
    if (poly)
        patch_poly_pack_host(f.w.data(), f.Cout, f.Cin, map, cin_packed, packed.data());
    else
        patch_pack_host(f.w.data(), f.Cout, f.Cin, map, cin_packed, packed.data());
    if (int rc = upload(c, poly ? &P->w_poly : &P->w, packed)) return rc;
    if (poly && split_planes) {   // the whole-tile launches of such a layer run the split-bf16 form (conv_mfma_patch_poly.hip)
        std::vector<float> planes(patch_poly_split_packed_elems(cin_packed, f.Cout));
        patch_poly_pack_split_host(f.w.data(), f.Cout, f.Cin, map, cin_packed, reinterpret_cast<uint16_t*>(planes.data()));
        if (int rc = upload(c, &P->w_poly3, planes)) return rc;
    }
    return upload_bias(c, &P->bias, f.b, (size_t)((f.Cout + 63) / 64) * 64);
}

// -> WinoLayer: Winograd-domain weights U = G g G^T of a 3x3 convolution, F(2x2,3x3) (tile 2) or F(4x4,3x3) (tile 4);
// split_planes: also the three-plane bf16 image of a tile-4 layer (a layer that only runs split over workgroups needs none)
int pack_wino(CtxBase* c, const HostConv& f, int tile, WinoLayer* L, bool split_planes = true) {
    L->Cin = f.Cin;
    L->Cout = f.Cout;
    L->tile = tile;
    L->BN = tile == 4 ? 64 : 128;
    L->ntiles = (f.Cout + L->BN - 1) / L->BN;
    std::vector<float> packed(tile == 4 ? wino4_packed_elems(f.Cout, f.Cin, L->BN) : wino_packed_elems(f.Cout, f.Cin, L->BN));
    if (tile == 4)
        wino4_pack_host(f.w.data(), f.Cout, f.Cin, L->BN, packed.data());
    else
        wino_pack_host(f.w.data(), f.Cout, f.Cin, L->BN, packed.data());
    if (int rc = upload(c, &L->u, packed)) return rc;
    if (split_planes && tile == 4 && f.Cin % (4 * CONV_BK) == 0) {   // the whole-tile launches of such a layer run the split-bf16 form (conv_winograd4.hip)
        std::vector<float> planes(wino4_split_packed_elems(f.Cout, f.Cin, L->BN));
        wino4_pack_split_host(f.w.data(), f.Cout, f.Cin, L->BN, reinterpret_cast<uint16_t*>(planes.data()));
        if (int rc = upload(c, &L->u3, planes)) return rc;
    }
    return upload_bias(c, &L->bias, f.b, (size_t)L->ntiles * L->BN);
}

// conv (+ optional BatchNorm folded behind it) -> packed device layer.
// MODE_PLAIN: ks x ks convolution.  MODE_ROWSPLIT: ks x 1 convolution with N = (dx, co) (to_rowsplit); the bias is
// returned in *row_bias instead of being applied by the convolution.  w_swizzled: a second image of the same weights in
// the LDS-DMA (XOR-swizzled) layout for an N tile of w_swizzled_bn (0: the layer's), the consumer kernel's.  w_col7_split (a
// row-split final layer): a third image, upload_col7_split's.
int build_layer(CtxBase* c, const std::vector<FoldSpec>& parts, int ks, int C0_real, int C0_packed, int C1_real,
                int C1_packed, ConvLayer* L, LayerMode mode = MODE_PLAIN, std::vector<float>* row_bias = nullptr,
                int dma_cfg = 0, float** w_swizzled = nullptr, int w_swizzled_bn = 0, float** w_col7_split = nullptr) {
    if (mode != MODE_PLAIN && mode != MODE_ROWSPLIT) return fail(c, EAMM_ERR_ARG, "build_layer: plain or row-split layers only");
    HostConv f;
    if (int rc = fold_conv(c, parts, ks, C0_real + C1_real, &f)) return rc;
    if (mode == MODE_ROWSPLIT) {
        std::vector<float> rb = to_rowsplit(&f);
        if (row_bias) row_bias->swap(rb);
    }
    const std::vector<int> map = channel_map(C0_real, C0_packed, C1_real, C1_packed);
    if (int rc = pack_conv(c, f, map.data(), C0_packed, C1_packed, MODE_PLAIN, dma_cfg, L)) return rc;
    if (w_col7_split)
        if (int rc = upload_col7_split(c, w_col7_split, f, map.data(), C0_packed + C1_packed)) return rc;
    if (!w_swizzled) return EAMM_OK;
    return upload_conv_image(c, w_swizzled, f, map.data(), C0_packed + C1_packed, w_swizzled_bn ? w_swizzled_bn : L->BN,
                             MODE_PLAIN, true);
}

// A 3x3 layer (MODE_PLAIN, or MODE_PHASE: the layer consumes the low-resolution input of an UpBlock2d and evaluates
// "nearest x2 + 3x3" as four 2x2 phase filters) packed for every kernel that may run it (pick(), launch_up());
// patch_split_planes: pack_patch's split_planes
int build_set(CtxBase* c, const std::vector<FoldSpec>& parts, int C0_real, int C0_packed, int C1_real, int C1_packed,
              LayerSet* S, LayerMode mode, bool patch_split_planes = false) {
    HostConv f;
    int rc = fold_conv(c, parts, 3, C0_real + C1_real, &f);
    if (rc) return rc;
    const std::vector<int> map = channel_map(C0_real, C0_packed, C1_real, C1_packed);
    if ((rc = pack_conv(c, f, map.data(), C0_packed, C1_packed, mode, 0, &S->base))) return rc;
    const int Cout = S->base.Cout;
    int cfg = 0;
    if (Cout % 256 == 0) cfg = c->dma_cfg_n256;
    else if (Cout % 128 == 0) cfg = c->dma_cfg_n128;
    else if (Cout == 64) cfg = c->dma_cfg_n64;
    if (cfg > 0 && c->dma_min_m >= 0) {
        if ((rc = pack_conv(c, f, map.data(), C0_packed, C1_packed, mode, cfg, &S->dma))) return rc;
        S->has_dma = true;
        if (S->dma.BN == 128 && c->skinny_max_m > 0) {   // same packed weights, small-M tiles (conv_dma_tile ids 4, 5)
            S->skinny32 = S->dma;
            S->skinny64 = S->dma;
            S->skinny32.dma_cfg = 4;
            S->skinny64.dma_cfg = 5;
            conv_dma_tile(4, &S->skinny32.BM, &S->skinny32.BN);
            conv_dma_tile(5, &S->skinny64.BM, &S->skinny64.BN);
            S->has_skinny = true;
        }
        if (Cout % 256 == 0 && cfg != 1 && c->big_min_m >= 0) {
            if ((rc = pack_conv(c, f, map.data(), C0_packed, C1_packed, mode, 1, &S->big))) return rc;
            S->has_big = true;
        }
    }
    if (mode == MODE_PHASE && parts.size() == 1 && !parts[0].norm.empty() && (Cout & 3) == 0 && c->patch_min_blocks >= 0) {
        if ((rc = pack_patch(c, f, map.data(), C0_packed, C1_packed, c->patch_poly != 0, &S->patch, patch_split_planes))) return rc;
        S->has_patch = true;
    }
    return 0;
}

// the largest split-K slab any of the set's kernels asks for at M pixels
size_t set_partial_elems(const LayerSet& S, size_t M) {
    size_t n = conv_plan(S.base, (int)M).partial_elems;
    if (S.has_dma) n = std::max(n, conv_plan(S.dma, (int)M).partial_elems);
    if (S.has_big) n = std::max(n, conv_plan(S.big, (int)M).partial_elems);
    if (S.has_skinny) n = std::max({n, conv_plan(S.skinny32, (int)M).partial_elems, conv_plan(S.skinny64, (int)M).partial_elems});
    return n;
}

// conv (+ folded BatchNorm) of C -> C channels -> Winograd-domain weights (pack_wino)
int build_wino(CtxBase* c, const std::string& conv, const std::string& norm, int C, WinoLayer* L, int tile = 2) {
    HostConv f;
    if (int rc = fold_conv(c, {{conv, norm}}, 3, C, &f)) return rc;
    if (f.Cout != C) return fail(c, EAMM_ERR_KEY, "%s mis-shaped for the Winograd path", conv.c_str());
    return pack_wino(c, f, tile, L);
}

// F(4x4,3x3) packing of a convolution whose input and output widths differ (hourglass DownBlock2d: conv -> BatchNorm
// folded; reference modules/util.py:903-921); input channels Cin_real sit first in a Cin_packed-wide activation
int build_wino4_rect(CtxBase* c, const std::string& conv, const std::string& norm, int Cin_real, int Cin_packed, WinoLayer* L) {
    if (Cin_packed < Cin_real || Cin_packed % 64) return fail(c, EAMM_ERR_KEY, "%s mis-shaped for the Winograd path", conv.c_str());
    HostConv f;
    if (int rc = fold_conv(c, {{conv, norm}}, 3, Cin_real, &f)) return rc;
    HostConv p = f;   // zero filters on the padding channels
    p.Cin = Cin_packed;
    p.w.assign((size_t)f.Cout * Cin_packed * 9, 0.f);
    for (int o = 0; o < f.Cout; ++o)
        std::copy_n(f.w.begin() + (size_t)o * Cin_real * 9, (size_t)Cin_real * 9, p.w.begin() + (size_t)o * Cin_packed * 9);
    return pack_wino(c, p, 4, L, false);   // the hourglass encoder's launches are variant 0: fp32 form
}

// Tile choice per launch (measured on MI355X, profiles/r01_convbench_*): M is the per-phase pixel count.
const ConvLayer& pick(const CtxBase* c, const LayerSet& S, size_t M) {
    // skinny GEMMs (deep hourglass levels at small batches): the weight stream is the cost, so tiles without padding rows
    if (S.has_skinny && M <= (size_t)c->skinny_max_m) return M <= 32 ? S.skinny32 : S.skinny64;
    if (S.has_big && M >= (size_t)c->big_min_m) return S.big;
    return (S.has_dma && M >= (size_t)c->dma_min_m) ? S.dma : S.base;
}

// UpBlock2d launch: the spatial-patch kernel when its 16x16-pixel tiles fill the chip, else the im2col-style kernels
int launch_up(CtxBase* c, const LayerSet& S, const ConvIO& io, hipStream_t s) {
    if (S.has_patch) {
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device);
        int splits = 1;
        if (S.patch.w_poly) {
            splits = patch_poly_splits(S.patch, io.B, io.Hin, io.Win, c->patch_split_max, cus);
            if ((size_t)splits * io.B * 4 * io.Hin * io.Win * S.patch.Cout > io.partial_cap) splits = 1;
        }
        const int blocks = ((io.Hin + 15) / 16) * ((io.Win + 15) / 16) * io.B * ((S.patch.Cout + 31) / 32) * splits;   // of the polyphase kernel
        if (blocks >= c->patch_min_blocks && io.Hin >= 16 && io.Win >= 16 && io.act == ACT_RELU && !io.resid && !io.out2 && !io.pool && !io.nchw) {
            if (S.patch.w_poly)
                HIP_TRY(c, patch_poly_launch(S.patch, io.in0, io.in1, io.B, io.Hin, io.Win, io.act, io.out, s, splits, io.partial,
                                             io.partial_cap));
            else
                HIP_TRY(c, patch_phase_launch(S.patch, io.in0, io.in1, io.B, io.Hin, io.Win, io.act, io.out, s));
            return EAMM_OK;
        }
    }
    HIP_TRY(c, conv_launch(pick(c, S, (size_t)io.B * io.Hin * io.Win), io, s));
    return EAMM_OK;
}

int env_int(const char* name, int dflt) { return (int)knob_int(name, dflt); }   // recorded: eamm_knobs_json

int round_up(int v, int m) { return (v + m - 1) / m * m; }

bool is_pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }


inline void read_tile_knobs(CtxBase* c) {
    // tuning knobs (defaults measured on MI355X, profiles/): EAMM_DMA_MIN_M < 0 disables the LDS-DMA kernels
    c->dma_min_m = env_int("EAMM_DMA_MIN_M", c->dma_min_m);
    c->big_min_m = env_int("EAMM_BIG_MIN_M", c->big_min_m);
    c->patch_poly = env_int("EAMM_PATCH_POLY", c->patch_poly);
    c->dma_cfg_n256 = env_int("EAMM_DMA_CFG_N256", c->dma_cfg_n256);
    c->dma_cfg_n128 = env_int("EAMM_DMA_CFG_N128", c->dma_cfg_n128);
    c->dma_cfg_n64 = env_int("EAMM_DMA_CFG_N64", c->dma_cfg_n64);
    c->patch_min_blocks = env_int("EAMM_PATCH_MIN_BLOCKS", c->patch_min_blocks);
    c->patch_split_max = env_int("EAMM_PATCH_SPLIT_MAX", c->patch_split_max);
    c->skinny_max_m = env_int("EAMM_SKINNY_MAX_M", c->skinny_max_m);
}

inline void free_owned(CtxBase* c) {
    DeviceGuard guard(c->device);
    (void)hipDeviceSynchronize();
    for (void* p : c->owned) (void)hipFree(p);
    c->owned.clear();
}

inline int store_tensor(CtxBase* c, const char* key, const float* host, const int64_t* shape, int ndim) {
    if (!c || !key || !host || ndim < 0 || (ndim > 0 && !shape)) return fail(c, EAMM_ERR_ARG, "null argument");
    if (c->finalized) return fail(c, EAMM_ERR_STATE, "weights already finalised; create a new handle to reload");
    HostTensor t;
    t.shape.assign(shape, shape + ndim);
    t.data.assign(host, host + t.numel());
    c->sd[key] = std::move(t);
    return EAMM_OK;
}

// strict key-set check, like load_state_dict(strict=True) (reference demo.py:91)
inline int check_keys(CtxBase* c, const std::vector<std::string>& want) {
    std::string missing, unexpected;
    for (auto& k : want)
        if (!c->sd.count(k)) missing += (missing.empty() ? "" : ", ") + k;
    for (auto& kv : c->sd) {
        const std::string& k = kv.first;
        if (k.size() > 20 && k.compare(k.size() - 20, 20, ".num_batches_tracked") == 0) continue;
        if (std::find(want.begin(), want.end(), k) == want.end()) unexpected += (unexpected.empty() ? "" : ", ") + k;
    }
    if (!missing.empty() || !unexpected.empty())
        return fail(c, EAMM_ERR_KEY, "state_dict mismatch. Missing key(s): [%s]. Unexpected key(s): [%s].",
                    missing.substr(0, 400).c_str(), unexpected.substr(0, 400).c_str());
    return EAMM_OK;
}

inline void block_keys(const std::string& p, std::vector<std::string>* keys) {   // conv + BatchNorm block
    keys->push_back(p + ".conv.weight");
    keys->push_back(p + ".conv.bias");
    for (const char* s : {".norm.weight", ".norm.bias", ".norm.running_mean", ".norm.running_var"}) keys->push_back(p + s);
}

}  // namespace
}  // namespace eamm
