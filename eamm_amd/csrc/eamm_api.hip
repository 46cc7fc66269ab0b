// C ABI of libeamm_hip.so (see include/eamm_hip.h), the generator handle: create / destroy, strict state_dict intake,
// padding of odd widths, BatchNorm folding and weight repacking, the workspace, and the frame-invariant half of
// OcclusionAwareGenerator.forward (reference modules/generator.py:59-97):
//   eamm_encode_source  -- first 7x7 block, down blocks, anti-alias down-sampling (+ export / import of what it caches)
// The per-frame half, eamm_forward_frames, and its launch plan are in eamm_forward.hip; the eamm_op_* entries in the four eamm_op_*.hip.
#include "eamm_ctx.h"

namespace {

void expected_keys(const eamm_ctx* c, std::vector<std::string>* keys) {
    auto block = [&](const std::string& p) { block_keys(p, keys); };
    const std::string dm = "dense_motion_network.";
    for (int i = 0; i < c->nb; ++i) block(dm + "hourglass.encoder.down_blocks." + std::to_string(i));
    for (int i = 0; i < c->nb; ++i) block(dm + "hourglass.decoder.up_blocks." + std::to_string(i));
    if (c->nb > 0) {
        keys->push_back(dm + "mask.weight");
        keys->push_back(dm + "mask.bias");
        if (c->cfg.estimate_occlusion_map) {
            keys->push_back(dm + "occlusion.weight");
            keys->push_back(dm + "occlusion.bias");
        }
        if (c->cfg.dm_inv_scale != 1) keys->push_back(dm + "down.weight");
    }
    block("first");
    for (int i = 0; i < c->nd; ++i) block("down_blocks." + std::to_string(i));
    for (int i = 0; i < c->nd; ++i) block("up_blocks." + std::to_string(i));
    for (int i = 0; i < c->cfg.num_bottleneck_blocks; ++i) {
        const std::string r = "bottleneck.r" + std::to_string(i);
        for (const char* s : {".conv1.weight", ".conv1.bias", ".conv2.weight", ".conv2.bias", ".norm1.weight",
                              ".norm1.bias", ".norm1.running_mean", ".norm1.running_var", ".norm2.weight",
                              ".norm2.bias", ".norm2.running_mean", ".norm2.running_var"})
            keys->push_back(r + s);
    }
    keys->push_back("final.weight");
    keys->push_back("final.bias");
}

double conv_flops(int ks, int cin, int cout, double pixels) { return 2.0 * ks * ks * (double)cin * cout * pixels; }

// ---- widths that are not multiples of 32 (reference modules/generator.py:14-48 accepts any): the state_dict is padded into
// the equivalent network whose widths are the next multiples of 32 -- extra output channels get zero filters and a zero bias,
// their BatchNorm is the identity (weight 1, bias 0, mean 0, variance 1), extra input channels get zero filter columns -- so
// the extra channels carry exact zeros through ReLU, pooling, the residual adds and the warps, and every layer builder and
// kernel below runs unchanged on multiples of 32.
struct PadPart { int real, packed; };
int pad_conv(eamm_ctx* c, const std::string& conv, int co_r, int co_p, const std::vector<PadPart>& in) {
    auto wi = c->sd.find(conv + ".weight");
    auto bi = c->sd.find(conv + ".bias");
    if (wi == c->sd.end() || bi == c->sd.end()) return fail(c, EAMM_ERR_KEY, "state_dict entry %s.weight / .bias missing", conv.c_str());
    HostTensor& w = wi->second;
    int cin_r = 0, cin_p = 0;
    for (auto& p : in) { cin_r += p.real; cin_p += p.packed; }
    if (w.shape.size() != 4 || w.shape[0] != co_r || w.shape[1] != cin_r || (int)bi->second.numel() != co_r)
        return fail(c, EAMM_ERR_KEY, "state_dict entry %s.weight mis-shaped (expected [%d,%d,k,k])", conv.c_str(), co_r, cin_r);
    const int T = (int)(w.shape[2] * w.shape[3]);
    HostTensor nw;
    nw.shape = {co_p, cin_p, w.shape[2], w.shape[3]};
    nw.data.assign((size_t)co_p * cin_p * T, 0.f);
    for (int o = 0; o < co_r; ++o) {
        int src = 0, dst = 0;
        for (auto& p : in) {
            std::copy(w.data.begin() + ((size_t)o * cin_r + src) * T, w.data.begin() + ((size_t)o * cin_r + src + p.real) * T,
                      nw.data.begin() + ((size_t)o * cin_p + dst) * T);
            src += p.real;
            dst += p.packed;
        }
    }
    w = std::move(nw);
    HostTensor& b = bi->second;
    b.data.resize(co_p, 0.f);
    b.shape = {co_p};
    return 0;
}
int pad_norm(eamm_ctx* c, const std::string& norm, int c_r, int c_p) {
    for (const char* leaf : {".weight", ".bias", ".running_mean", ".running_var"}) {
        auto it = c->sd.find(norm + leaf);
        if (it == c->sd.end() || (int)it->second.numel() != c_r)
            return fail(c, EAMM_ERR_KEY, "BatchNorm entry %s%s missing or mis-shaped (expected %d)", norm.c_str(), leaf, c_r);
        const bool one = !strcmp(leaf, ".weight") || !strcmp(leaf, ".running_var");
        it->second.data.resize(c_p, one ? 1.f : 0.f);
        it->second.shape = {c_p};
    }
    return 0;
}

int pad_state_dict(eamm_ctx* c) {
    const std::string dm = "dense_motion_network.";
    const int nb = c->nb, nd = c->nd;
    // the hourglass input line: per motion (heat-map, image channels) -- C + 1 values of the reference land in the kernels' four
    const std::vector<PadPart> motion_line((size_t)c->K + 1, PadPart{c->Cimg + 1, 4 * c->G});
    int rc;
#define PAD_TRY(e) if ((rc = (e))) return rc
    for (int i = 0; i < nb; ++i) {
        const std::string p = dm + "hourglass.encoder.down_blocks." + std::to_string(i);
        const std::vector<PadPart> in = i == 0 ? motion_line : std::vector<PadPart>{PadPart{c->enc_r[i - 1], c->enc_c[i - 1]}};
        PAD_TRY(pad_conv(c, p + ".conv", c->enc_r[i], c->enc_c[i], in));
        PAD_TRY(pad_norm(c, p + ".norm", c->enc_r[i], c->enc_c[i]));
    }
    for (int i = 0; i < nb; ++i) {
        const std::string p = dm + "hourglass.decoder.up_blocks." + std::to_string(i);
        std::vector<PadPart> in;
        if (i == 0) in = {{c->enc_r[nb - 1], c->enc_c[nb - 1]}};
        else in = {{c->dec_r[i - 1], c->dec_c[i - 1]}, {c->enc_r[nb - 1 - i], c->enc_c[nb - 1 - i]}};
        PAD_TRY(pad_conv(c, p + ".conv", c->dec_r[i], c->dec_c[i], in));
        PAD_TRY(pad_norm(c, p + ".norm", c->dec_r[i], c->dec_c[i]));
    }
    if (nb > 0) {
        std::vector<PadPart> in = {{c->dec_r.back(), c->dec_c.back()}};
        in.insert(in.end(), motion_line.begin(), motion_line.end());
        PAD_TRY(pad_conv(c, dm + "mask", c->K + 1, c->K + 1, in));
        if (c->cfg.estimate_occlusion_map) PAD_TRY(pad_conv(c, dm + "occlusion", 1, 1, in));
        if (c->cfg.dm_inv_scale != 1 && c->Cimg != 3) {   // anti-alias buffer [C,1,13,13] (util.py:1038): one filter per channel
            auto it = c->sd.find(dm + "down.weight");
            if (it == c->sd.end() || (int)it->second.numel() != c->Cimg * 169)
                return fail(c, EAMM_ERR_KEY, "%sdown.weight must be [%d,1,13,13]", dm.c_str(), c->Cimg);
            it->second.data.resize((size_t)c->Cpl * 169, 0.f);
            it->second.shape = {c->Cpl, 1, 13, 13};
        }
    }
    PAD_TRY(pad_conv(c, "first.conv", c->down_r[0], c->down_c[0], {{c->Cimg, c->Cpl}}));
    PAD_TRY(pad_norm(c, "first.norm", c->down_r[0], c->down_c[0]));
    for (int i = 0; i < nd; ++i) {
        const std::string p = "down_blocks." + std::to_string(i);
        PAD_TRY(pad_conv(c, p + ".conv", c->down_r[i + 1], c->down_c[i + 1], {{c->down_r[i], c->down_c[i]}}));
        PAD_TRY(pad_norm(c, p + ".norm", c->down_r[i + 1], c->down_c[i + 1]));
    }
    for (int i = 0; i < c->cfg.num_bottleneck_blocks; ++i) {
        const std::string r = "bottleneck.r" + std::to_string(i);
        for (const char* k : {".conv1", ".conv2"}) PAD_TRY(pad_conv(c, r + k, c->Cb_r, c->Cb, {{c->Cb_r, c->Cb}}));
        for (const char* k : {".norm1", ".norm2"}) PAD_TRY(pad_norm(c, r + k, c->Cb_r, c->Cb));
    }
    for (int i = 0; i < nd; ++i) {
        const std::string p = "up_blocks." + std::to_string(i);
        const PadPart in = i == 0 ? PadPart{c->Cb_r, c->Cb} : PadPart{c->up_r[i - 1], c->up_c[i - 1]};
        PAD_TRY(pad_conv(c, p + ".conv", c->up_r[i], c->up_c[i], {in}));
        PAD_TRY(pad_norm(c, p + ".norm", c->up_r[i], c->up_c[i]));
    }
    // (more than three image channels: `final` keeps its C outputs and runs on the generic kernel, see eamm_finalize_weights)
    PAD_TRY(pad_conv(c, "final", c->Cimg, c->Cimg > 3 ? c->Cimg : 3, {{c->up_r.back(), c->up_c.back()}}));
#undef PAD_TRY
    return 0;
}

}  // namespace

// -------------------------------------------------------------------------------------------------
extern "C" {

int eamm_abi_version(void) { return EAMM_ABI_VERSION; }

const char* eamm_last_error(const eamm_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int eamm_create(const eamm_config* cfg, int device, eamm_ctx** out) {
    if (!cfg || !out) return fail(nullptr, EAMM_ERR_ARG, "null argument");
    *out = nullptr;
    const eamm_config& g = *cfg;
    if (g.num_channels < 1 || g.num_channels > 6)
        return fail(nullptr, EAMM_ERR_ARG, "num_channels must be 1 .. 6 (got %d): the motion kernels keep a pixel's image channels in "
                    "groups of three (one float4 beside its heat-map value per group), two groups at most", g.num_channels);
    if (g.num_kp < 1 || g.num_kp + 2 > 32)
        return fail(nullptr, EAMM_ERR_ARG, "num_kp must be 1 .. 30 (got %d): the flow head keeps the K + 1 motions' softmax and the "
                    "occlusion logit of a pixel in one 32-lane group", g.num_kp);
    // dm_num_blocks == 0: a generator without a motion network (dense_motion_params=None, generator.py:22-23)
    const bool has_dm = g.dm_num_blocks > 0;
    if (g.dm_num_blocks < 0) return fail(nullptr, EAMM_ERR_ARG, "dm_num_blocks < 0");
    if (has_dm && (!is_pow2(g.dm_inv_scale) || g.dm_inv_scale > 4 || g.dm_inv_scale == 3))
        return fail(nullptr, EAMM_ERR_ARG, "1/scale_factor must be 1, 2 or 4");
    if (!has_dm && g.estimate_occlusion_map) return fail(nullptr, EAMM_ERR_ARG, "estimate_occlusion_map needs a motion network");
    if (g.block_expansion < 1 || g.max_features < 1 || (has_dm && (g.dm_block_expansion < 1 || g.dm_max_features < 1)))
        return fail(nullptr, EAMM_ERR_ARG, "channel widths must be positive");
    if (g.num_down_blocks < 1 || g.num_bottleneck_blocks < 1)
        return fail(nullptr, EAMM_ERR_ARG, "need at least one down block and one bottleneck block");
    if (g.max_frames < 1 || g.max_sources < 1) return fail(nullptr, EAMM_ERR_ARG, "max_frames / max_sources < 1");
    const int div_g = 1 << g.num_down_blocks, div_m = has_dm ? g.dm_inv_scale << g.dm_num_blocks : 1;
    if (g.height % div_g || g.width % div_g || g.height % div_m || g.width % div_m)
        return fail(nullptr, EAMM_ERR_ARG, "frame %dx%d not divisible for %d down blocks / %d hourglass levels",
                    g.height, g.width, g.num_down_blocks, g.dm_num_blocks);
    {   // the kernels address tensors through 32-bit buffer descriptors: every activation must stay below 4 GiB
        const double hw = (double)g.height * g.width, F = g.max_frames;
        const double biggest = std::max({F * hw * 32.0,                                  // final-conv partial products
                                         F * hw * (double)round_up(g.block_expansion, 32),   // last up-block output
                                         4.0 * F * (hw / (1 << (2 * g.num_down_blocks))) *
                                             round_up(std::min(g.max_features, g.block_expansion << g.num_down_blocks), 32)}) * 4.0;
        if (biggest >= 4294967280.0)
            return fail(nullptr, EAMM_ERR_ARG, "max_frames=%d at %dx%d needs a %.1f GiB activation tensor; the limit is 4 GiB "
                        "per tensor -- lower max_frames", g.max_frames, g.height, g.width, biggest / 1073741824.0);
    }
    {   // validate the device without leaving it selected in the caller's thread
        DeviceGuard probe(device);
        if (probe.status != hipSuccess) return fail(nullptr, EAMM_ERR_HIP, "hipSetDevice(%d) failed", device);
    }

    eamm_ctx* c = new eamm_ctx();
    c->cfg = g;
    c->device = device;
    c->H = g.height;
    c->W = g.width;
    if (!has_dm) c->cfg.dm_inv_scale = 1;
    c->h = c->H / c->cfg.dm_inv_scale;
    c->w = c->W / c->cfg.dm_inv_scale;
    c->nd = g.num_down_blocks;
    c->nb = g.dm_num_blocks;
    c->K = g.num_kp;
    c->hf = c->H >> c->nd;
    c->wf = c->W >> c->nd;
    c->Cimg = g.num_channels;
    c->G = c->Cimg > 3 ? 2 : 1;            // groups of three image channels (motion.hip: motion_front_kernel)
    c->Cpl = 3 * c->G;                     // planes of the zero-extended source copy
    c->Cp0 = round_up((c->K + 1) * 4 * c->G, 32);
    // hourglass channel plan (reference modules/util.py:941-987)
    for (int i = 0; i < c->nb; ++i) c->enc_r.push_back(std::min(g.dm_max_features, g.dm_block_expansion << (i + 1)));
    for (int i = c->nb - 1; i >= 0; --i) c->dec_r.push_back(std::min(g.dm_max_features, g.dm_block_expansion << i));
    // generator channel plan (reference modules/generator.py:27-44)
    c->down_r.push_back(g.block_expansion);
    for (int i = 0; i < c->nd; ++i) c->down_r.push_back(std::min(g.max_features, g.block_expansion << (i + 1)));
    for (int i = 0; i < c->nd; ++i) c->up_r.push_back(std::min(g.max_features, g.block_expansion << (c->nd - i - 1)));
    c->Cb_r = c->down_r.back();
    // the kernels' widths: the 32-channel granule of the MFMA operand loaders (any width the reference accepts is taken)
    auto pad32 = [&](const std::vector<int>& r, std::vector<int>* p) {
        for (int v : r) {
            p->push_back(round_up(v, 32));
            c->padded_widths |= p->back() != v;
        }
    };
    pad32(c->enc_r, &c->enc_c);
    pad32(c->dec_r, &c->dec_c);
    pad32(c->down_r, &c->down_c);
    pad32(c->up_r, &c->up_c);
    c->Cb = c->down_c.back();
    read_tile_knobs(c);
    c->wino_min_m = env_int("EAMM_WINO_MIN_M", c->wino_min_m);   // (< 0 disables the Winograd bottleneck)
    c->wino4_min_m = env_int("EAMM_WINO4_MIN_M", c->wino4_min_m);
    c->wino_tile = env_int("EAMM_WINO_TILE", c->wino_tile);
    c->col7 = env_int("EAMM_COL7", c->col7);
    c->final_fused = env_int("EAMM_FINAL_FUSED", c->final_fused);
    c->final_fused_min_rows = env_int("EAMM_FINAL_FUSED_MIN_ROWS", c->final_fused_min_rows);
    c->bneck_chains = env_int("EAMM_BNECK_CHAINS", c->bneck_chains);
    c->pass_chains = env_int("EAMM_PASS_CHAINS", c->pass_chains);
    // clamped ONCE, here: negative = off (as the other knobs), at most four chains; the split-K slab count and the runtime
    // chain count both derive from this value
    c->pass_chains = c->pass_chains < 0 ? 1 : std::min(c->pass_chains, 4);
    c->bneck_chains = std::max(1, std::min(c->bneck_chains, 16));
    if (getenv("EAMM_WARP_JOINT") && atoi(getenv("EAMM_WARP_JOINT")) != 0) {   // (a benchmark record labelled from it would be wrong)
        delete c;
        return fail(nullptr, EAMM_ERR_ARG, "EAMM_WARP_JOINT was removed: one feature-warp launch for all chains' frames measured "
                    "-0.8 %% frames/s (DESIGN.md section 12, profiles/r04_experiments.txt section 3); unset it");
    }
    c->wino4_variant = env_int("EAMM_WINO4_VARIANT", c->wino4_variant);
    c->wino4_variant_pinned = getenv("EAMM_WINO4_VARIANT") != nullptr;   // an explicit choice holds for every call size
    {   // read ONCE here, not per call (a device query in every forward_view of the per-frame path)
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) c->cus = cus;
        else (void)hipGetLastError();
    }
#ifdef EAMM_EXPERIMENTS
    c->epi_v = env_int("EAMM_WINO4_EPI_V", c->epi_v);
#else
    // timing experiments that compute wrong results exist only in a -DEAMM_EXPERIMENTS build (make EXPERIMENTS=1): the product
    // library refuses to run with their knobs set rather than ignoring them silently (or, worse, obeying them)
    for (const char* bad : {"EAMM_WINO4_EPI_V", "EAMM_COL7_DBG"})
        if (getenv(bad) && atoi(getenv(bad)) != 0) {
            delete c;
            return fail(nullptr, EAMM_ERR_ARG, "%s is a wrong-results timing experiment: it needs a library built with make EXPERIMENTS=1", bad);
        }
    if (c->wino4_variant == 10 || c->wino4_variant == 16 || c->wino4_variant == 17 || c->wino4_variant == 50) {
        const int v = c->wino4_variant;
        delete c;
        return fail(nullptr, EAMM_ERR_ARG, "EAMM_WINO4_VARIANT=%d is a wrong-results timing experiment: it needs make EXPERIMENTS=1", v);
    }
    if (c->wino4_variant != 0 && c->wino4_variant != 3 && c->wino4_variant != 6) {   // (wino4_gemm_launch knows no other: every forward would fail)
        const int v = c->wino4_variant;
        delete c;
        return fail(nullptr, EAMM_ERR_ARG, "EAMM_WINO4_VARIANT=%d: the F(4x4) GEMM has the pipeline variants 0, 3 and 6", v);
    }
#endif
    c->pass_chains_min_frames = env_int("EAMM_PASS_CHAINS_MIN_FRAMES", c->pass_chains_min_frames);
    c->pass_chains_min_blocks = env_int("EAMM_PASS_CHAINS_MIN_BLOCKS", c->pass_chains_min_blocks);
    c->head_col7_min_tiles = env_int("EAMM_HEAD_COL7_MIN_TILES", c->head_col7_min_tiles);
    c->enc_wino = env_int("EAMM_ENC_WINO", c->enc_wino);
    c->first7 = env_int("EAMM_FIRST7", c->first7);
    c->enc_wino_min_mflop = env_int("EAMM_ENC_WINO_MIN_MFLOP", c->enc_wino_min_mflop);
    c->enc_wino_min_tiles = env_int("EAMM_ENC_WINO_MIN_TILES", c->enc_wino_min_tiles);
    *out = c;
    return EAMM_OK;
}

void eamm_destroy(eamm_ctx* c) {
    if (!c) return;
    DeviceGuard guard(c->device);
    free_owned(c);
    for (auto& e : c->prof.events) (void)hipEventDestroy(e);
    for (auto& e : c->prof.chain_ev) (void)hipEventDestroy(e);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    for (auto& e : c->ev_join) (void)hipEventDestroy(e);
    for (auto& st : c->own_streams) (void)hipStreamDestroy(st);   // (drains the stream's work first; the pool's streams stay)
    delete c;
}

int eamm_load_tensor(eamm_ctx* c, const char* key, const float* host, const int64_t* shape, int ndim) {
    return store_tensor(c, key, host, shape, ndim);
}

int eamm_finalize_weights(eamm_ctx* c) {
    if (!c) return EAMM_ERR_ARG;
    if (c->finalized) return fail(c, EAMM_ERR_STATE, "weights already finalised");
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    const eamm_config& g = c->cfg;
    {
        std::vector<std::string> want;
        expected_keys(c, &want);
        if (int krc = check_keys(c, want)) return krc;
    }
    if (c->padded_widths || c->Cimg != 3) {
        if (c->train_mode)
            return fail(c, EAMM_ERR_ARG, "a training-mode handle needs three image channels and channel widths that are multiples of 32 "
                        "(its BatchNorm kernels read the module's own statistics tensors); the module takes the operator composition "
                        "for such a generator");
        if (int prc = pad_state_dict(c)) return prc;
    }
    const std::string dm = "dense_motion_network.";
    int rc;
    // training mode (eamm_set_training): batch statistics cannot be folded -- every convolution is packed with its raw
    // weights and the BatchNorm runs as its own kernels (eamm_train_api.hip)
    const bool tr = c->train_mode;
    auto nm = [&](const std::string& norm) { return tr ? std::string() : norm; };
    // hourglass encoder: e_0 = 44-channel motion tensor (padded to Cp0), e_i = DownBlock2d_i(e_{i-1})
    c->hg_enc.resize(c->nb);
    const int cin0 = (c->K + 1) * 4 * c->G;
    for (int i = 0; i < c->nb; ++i) {
        const std::string p = dm + "hourglass.encoder.down_blocks." + std::to_string(i);
        const int cr = i == 0 ? cin0 : c->enc_c[i - 1], cp = i == 0 ? c->Cp0 : c->enc_c[i - 1];
        if ((rc = build_set(c, {{p + ".conv", nm(p + ".norm")}}, cr, cp, 0, 0, &c->hg_enc[i], MODE_PLAIN))) return rc;
    }
    // hourglass decoder: u_i = UpBlock2d_i(cat[u_{i-1}, e_{nb-i}])  (util.py:981-987)
    c->hg_dec.resize(c->nb);
    for (int i = 0; i < c->nb; ++i) {
        const std::string p = dm + "hourglass.decoder.up_blocks." + std::to_string(i);
        const int c0 = i == 0 ? c->enc_c[c->nb - 1] : c->dec_c[i - 1];
        const int c1 = i == 0 ? 0 : c->enc_c[c->nb - 1 - i];
        if ((rc = build_set(c, {{p + ".conv", nm(p + ".norm")}}, c0, c0, c1, c1, &c->hg_dec[i], MODE_PHASE))) return rc;
    }
    // flow head: mask (K+1) and occlusion (1) 7x7 convolutions share one launch (dense_motion.py:98,110)
    if (c->nb > 0) {
        std::vector<FoldSpec> parts = {{dm + "mask", ""}};
        if (g.estimate_occlusion_map) parts.push_back({dm + "occlusion", ""});
        const int nc = c->K + 1 + (g.estimate_occlusion_map ? 1 : 0);
        if (7 * nc <= 128 && env_int("EAMM_HEAD_ROWSPLIT", 1)) {
            // 7x1 MFMA convolution with N = (dx, co) + horizontal gather in the head kernel: pads N to 7*nc (84) of
            // 128 instead of nc (12) of 32 -> 2.3x fewer executed MACs
            std::vector<float> hb;
            const bool col7s_ok = c->col7 && 7 * nc <= 96 && c->dec_c.back() % 32 == 0 && c->Cp0 % 32 == 0;
            if ((rc = build_layer(c, parts, 7, c->dec_c.back(), c->dec_c.back(), cin0, c->Cp0, &c->head, MODE_ROWSPLIT, &hb, 0,
                                  col7s_ok ? &c->head_w_swz : nullptr, 96)))
                return rc;
            if ((rc = upload(c, &c->head_bias, hb))) return rc;
            c->head_nc = nc;
        } else if ((rc = build_layer(c, parts, 7, c->dec_c.back(), c->dec_c.back(), cin0, c->Cp0, &c->head))) {
            return rc;
        }
    }
    // generator encoder
    if ((rc = build_layer(c, {{"first.conv", nm("first.norm")}}, 7, c->Cpl, c->Csrc, 0, 0, &c->first))) return rc;
    // K = 147 (196 with the zero rows) instead of 49 x 32; a first layer of another width keeps the generic kernel
    if (c->first7 && c->Cpl == 3 && first7_supported(c->down_c[0]) && c->first.Cout == c->down_c[0]) {
        HostConv f;   // (build_layer has just checked these keys: first7 is off in training mode, where nm() drops the norm)
        if ((rc = fold_conv(c, {{"first.conv", "first.norm"}}, 7, 3, &f))) return rc;
        std::vector<float> packed((size_t)196 * f.Cout);
        first7_pack_host(f.w.data(), f.Cout, packed.data());
        if ((rc = upload(c, &c->first7_w, packed))) return rc;
        if ((rc = upload(c, &c->first7_bias, f.b))) return rc;
    }
    c->down.resize(c->nd);
    for (int i = 0; i < c->nd; ++i) {
        const std::string p = "down_blocks." + std::to_string(i);
        if ((rc = build_set(c, {{p + ".conv", nm(p + ".norm")}}, c->down_c[i], c->down_c[i], 0, 0, &c->down[i], MODE_PLAIN)))
            return rc;
    }
    // bottleneck: conv1 absorbs norm2 (conv1 -> norm2 -> relu), norm1 becomes the producer's second output
    const int nr = g.num_bottleneck_blocks;
    c->res1.resize(nr);
    c->res2.resize(nr);
    c->pre_s.resize(nr);
    c->pre_t.resize(nr);
    for (int i = 0; i < nr; ++i) {
        const std::string r = "bottleneck.r" + std::to_string(i);
        if ((rc = build_set(c, {{r + ".conv1", nm(r + ".norm2")}}, c->Cb, c->Cb, 0, 0, &c->res1[i], MODE_PLAIN))) return rc;
        if ((rc = build_set(c, {{r + ".conv2", ""}}, c->Cb, c->Cb, 0, 0, &c->res2[i], MODE_PLAIN))) return rc;
        if (c->wino_min_m >= 0 && c->Cb % 64 == 0) {
            c->wres1.resize(nr);
            c->wres2.resize(nr);
            if ((rc = build_wino(c, r + ".conv1", r + ".norm2", c->Cb, &c->wres1[i]))) return rc;
            if ((rc = build_wino(c, r + ".conv2", "", c->Cb, &c->wres2[i]))) return rc;
            if (c->wino_tile == 4) {
                c->w4res1.resize(nr);
                c->w4res2.resize(nr);
                if ((rc = build_wino(c, r + ".conv1", r + ".norm2", c->Cb, &c->w4res1[i], 4))) return rc;
                if ((rc = build_wino(c, r + ".conv2", "", c->Cb, &c->w4res2[i], 4))) return rc;
            }
        }
        const HostTensor *gm = find(c, r + ".norm1.weight"), *bt = find(c, r + ".norm1.bias"),
                         *mu = find(c, r + ".norm1.running_mean"), *vr = find(c, r + ".norm1.running_var");
        if ((int)gm->numel() != c->Cb || (int)bt->numel() != c->Cb || (int)mu->numel() != c->Cb ||
            (int)vr->numel() != c->Cb)
            return fail(c, EAMM_ERR_KEY, "%s.norm1 mis-shaped", r.c_str());
        // (not fold_norm with a zero conv bias: (0 - mu) * s + beta is +0 where beta - mu * s is -0, for mu = +0 and
        // beta = -0; everywhere else the two agree bit for bit)
        std::vector<float> s(c->Cb), t(c->Cb);
        for (int ch = 0; ch < c->Cb; ++ch) {
            const double sc = (double)gm->data[ch] / std::sqrt((double)vr->data[ch] + 1e-5);
            s[ch] = (float)sc;
            t[ch] = (float)((double)bt->data[ch] - (double)mu->data[ch] * sc);
        }
        if ((rc = upload(c, &c->pre_s[i], s))) return rc;
        if ((rc = upload(c, &c->pre_t[i], t))) return rc;
    }
    // hourglass encoder levels in F(4x4,3x3) form: they borrow the bottleneck's V / Z workspaces (a frame's share must fit)
    if (c->enc_wino && !c->w4res1.empty()) {
        c->w4enc.resize(c->nb);
        const size_t hw_l = (size_t)c->h * c->w, hwf_l = (size_t)c->hf * c->wf;
        for (int i = 0; i < c->nb; ++i) {
            const int cr = i == 0 ? cin0 : c->enc_c[i - 1], cp = i == 0 ? c->Cp0 : c->enc_c[i - 1], co = c->enc_c[i];
            const size_t tiles = (hw_l >> (2 * i)) / 16;
            if (((c->h >> i) & 3) || ((c->w >> i) & 3) || cp % 64 || (co & 3) || 36 * tiles * cp > 4 * hwf_l * c->Cb ||
                tiles * co > (hwf_l / 16) * c->Cb ||
                (size_t)g.max_frames * tiles < (size_t)c->enc_wino_min_tiles * (144.0 * cp * co > 100e6 ? 4 : 1))
                continue;   // (the last: never used at any call size -- do not pack 36 / 9 x the weights for nothing)
            const std::string p = dm + "hourglass.encoder.down_blocks." + std::to_string(i);
            if ((rc = build_wino4_rect(c, p + ".conv", p + ".norm", cr, cp, &c->w4enc[i]))) return rc;
        }
    }
    if (c->enc_wino && !c->w4res1.empty()) {   // the source encoder's down blocks likewise (workspaces sized for them below)
        c->w4down.resize(c->nd);
        for (int i = 0; i < c->nd; ++i) {
            const int ci = c->down_c[i], co = c->down_c[i + 1];
            if (((c->H >> i) & 3) || ((c->W >> i) & 3) || ci % 64 || (co & 3)) continue;
            const std::string p = "down_blocks." + std::to_string(i);
            if ((rc = build_wino4_rect(c, p + ".conv", p + ".norm", ci, ci, &c->w4down[i]))) return rc;
        }
    }
    c->up.resize(c->nd);
    for (int i = 0; i < c->nd; ++i) {
        const std::string p = "up_blocks." + std::to_string(i);
        const int ci = i == 0 ? c->Cb : c->up_c[i - 1];
        if ((rc = build_set(c, {{p + ".conv", nm(p + ".norm")}}, ci, ci, 0, 0, &c->up[i], MODE_PHASE, true))) return rc;
    }
    if (c->Cimg > 3) {   // more than three outputs: the plain 7x7 kernel (N padded to its 32-column tile), sigmoid and the NCHW
        // store in its epilogue -- correct for any channel count, ten times the minimal work: RGBA is not the shipped case
        if ((rc = build_layer(c, {{"final", ""}}, 7, c->up_c.back(), c->up_c.back(), 0, 0, &c->final_conv))) return rc;
    } else {   // final 7x7 (Cout = 3): 7x1 MFMA convolution over (dx, co) + horizontal gather
        std::vector<float> fb;
        const bool col7_ok = c->col7 && c->up_c.back() % 32 == 0 && c->up_c.back() <= 64;
        if ((rc = build_layer(c, {{"final", ""}}, 7, c->up_c.back(), c->up_c.back(), 0, 0, &c->final_conv,
                              MODE_ROWSPLIT, &fb, 0, col7_ok ? &c->final_w_swz : nullptr, 0, col7_ok ? &c->final_w3 : nullptr)))
            return rc;
        if (c->final_conv.Cout != 21) return fail(c, EAMM_ERR_KEY, "final.weight must have 3 output channels");
        if ((rc = upload(c, &c->final_bias, fb))) return rc;
    }
    // anti-alias buffer [planes,1,13,13]
    {
        std::vector<float> aa((size_t)c->Cpl * 169, 0.f);
        if (g.dm_inv_scale != 1) {
            const HostTensor* t = find(c, dm + "down.weight");
            if (!t || (int)t->numel() != c->Cpl * 169) return fail(c, EAMM_ERR_KEY, "%sdown.weight must be [%d,1,13,13]", dm.c_str(), c->Cimg);
            aa = t->data;
        }
        if ((rc = upload(c, &c->aa_w, aa))) return rc;
    }

    // ---- workspace --------------------------------------------------------------------------
    const size_t S = g.max_sources, F = g.max_frames;
    const size_t HW = (size_t)c->H * c->W, hw = (size_t)c->h * c->w, hwf = (size_t)c->hf * c->wf;
    if ((rc = dev_alloc(c, &c->feat, S * hwf * c->Cb))) return rc;
    if ((rc = dev_alloc(c, &c->src_small, (size_t)c->G * S * hw * 4))) return rc;     // [group][source][h][w][4]
    if ((rc = dev_alloc(c, &c->src_full, S * c->Cpl * HW))) return rc;
    if (c->Cimg != 3)    // the channels a source does not have stay zero for the handle's life (eamm_encode_source copies only the real ones)
        HIP_TRY(c, hipMemset(c->src_full, 0, S * c->Cpl * HW * sizeof(float)));
    if (c->Cimg < 3) {   // one or two channels: the three-channel kernels write staging tensors (four and more write the caller's)
        if ((rc = dev_alloc(c, &c->stage_pred, F * 3 * HW))) return rc;
        if (c->nb > 0 && (rc = dev_alloc(c, &c->stage_deformed, F * 3 * HW))) return rc;
        if (c->nb > 0 && (rc = dev_alloc(c, &c->stage_sparse, F * (c->K + 1) * 3 * hw))) return rc;
    }
    if ((rc = dev_alloc(c, &c->src_nhwc, S * HW * c->Csrc))) return rc;
    c->enc_tmp.resize(c->nd);
    for (int i = 0; i < c->nd; ++i)  // enc_tmp[0] = first output @HxW; enc_tmp[i] = down[i-1] output
        if ((rc = dev_alloc(c, &c->enc_tmp[i], S * (HW >> (2 * i)) * c->down_c[i]))) return rc;
    if ((rc = dev_alloc(c, &c->kp_rec, F * c->K * KP_STRIDE))) return rc;
    if ((rc = dev_alloc(c, &c->bad_flag, 1))) return rc;
    HIP_TRY(c, hipMemset(c->bad_flag, 0, sizeof(int)));
    if (c->nb > 0 && (rc = dev_alloc(c, &c->hg_in, F * hw * c->Cp0))) return rc;
    c->e_buf.resize(c->nb);
    c->u_buf.resize(c->nb);
    for (int i = 0; i < c->nb; ++i) {
        if ((rc = dev_alloc(c, &c->e_buf[i], F * (hw >> (2 * (i + 1))) * c->enc_c[i]))) return rc;
        if ((rc = dev_alloc(c, &c->u_buf[i], F * (hw >> (2 * (c->nb - 1 - i))) * c->dec_c[i]))) return rc;
    }
    if (c->nb > 0 && (rc = dev_alloc(c, &c->logits, F * hw * (c->head_nc ? 128 : 32)))) return rc;
    if (c->nb > 0 && (rc = dev_alloc(c, &c->deformation, F * hw * 2))) return rc;
    if (c->nb > 0 && (rc = dev_alloc(c, &c->occlusion, F * hw))) return rc;
    if ((rc = dev_alloc(c, &c->xa, F * hwf * c->Cb))) return rc;
    if ((rc = dev_alloc(c, &c->xb, F * hwf * c->Cb))) return rc;
    if ((rc = dev_alloc(c, &c->act, F * hwf * c->Cb))) return rc;
    if ((rc = dev_alloc(c, &c->tmp, F * hwf * c->Cb))) return rc;
    if ((rc = dev_alloc(c, &c->final_part, F * HW * 32))) return rc;
    size_t v_elems = 4 * F * hwf * c->Cb, z_elems = 24 * ((F * hwf + 15) / 16) * c->Cb;
    for (size_t i = 0; i < c->w4down.size(); ++i)   // the encoder's down blocks in F(4x4) form borrow the same workspaces
        if (c->w4down[i].Cout) {   // ... for as many sources per call as the 32-bit descriptors allow (more take the direct kernels)
            size_t ns_fit = S;
            while (ns_fit > 0 && !wino4_fits(ns_fit * (HW >> (2 * i)) / 16, c->w4down[i].Cin, c->w4down[i].Cout)) --ns_fit;
            const size_t tiles = ns_fit * (HW >> (2 * i)) / 16;
            v_elems = std::max(v_elems, 36 * tiles * c->w4down[i].Cin);
            z_elems = std::max(z_elems, 24 * tiles * c->w4down[i].Cout);
        }
    if (!c->wres1.empty() && (rc = dev_alloc(c, &c->wino_v, v_elems))) return rc;
    c->wino_z_elems = z_elems;
    if (!c->w4res1.empty() && (rc = dev_alloc(c, &c->wino_z, z_elems))) return rc;
    if (c->epi_v && !c->w4res1.empty() && (rc = dev_alloc(c, &c->epi_scratch, (size_t)3 * c->cfg.max_frames * c->hf * c->wf * c->Cb))) return rc;
    c->up_buf.resize(c->nd);
    for (int i = 0; i < c->nd; ++i)
        if ((rc = dev_alloc(c, &c->up_buf[i], F * (hwf << (2 * (i + 1))) * c->up_c[i]))) return rc;
    if (tr) {   // pre-BatchNorm convolution outputs (DownBlock2d: at the un-pooled size) and the statistics of the site in flight
        size_t raw_elems = F * HW * c->down_c[0];
        int cmax = std::max(c->down_c[0], c->Cb);
        for (int i = 0; i < c->nd; ++i) {
            raw_elems = std::max(raw_elems, F * (HW >> (2 * i)) * c->down_c[i + 1]);
            raw_elems = std::max(raw_elems, F * (hwf << (2 * (i + 1))) * c->up_c[i]);
            cmax = std::max({cmax, c->down_c[i + 1], c->up_c[i]});
        }
        for (int i = 0; i < c->nb; ++i) {
            raw_elems = std::max(raw_elems, F * (hw >> (2 * i)) * c->enc_c[i]);
            raw_elems = std::max(raw_elems, F * (hw >> (2 * (c->nb - 1 - i))) * c->dec_c[i]);
            cmax = std::max({cmax, c->enc_c[i], c->dec_c[i]});
        }
        if (cmax > 1024 || (cmax & 3)) return fail(c, EAMM_ERR_ARG, "training mode: BatchNorm sites of up to 1024 channels (got %d)", cmax);
        if (S < F) return fail(c, EAMM_ERR_ARG, "training mode needs max_sources >= max_frames (one source per frame of the batch)");
        c->train_cmax = cmax;
        if ((rc = dev_alloc(c, &c->raw, raw_elems))) return rc;
        if ((rc = dev_alloc(c, &c->train_stat, (size_t)2 * cmax))) return rc;
        if ((rc = dev_alloc(c, &c->bn_work, (size_t)cmax * 1024 * 4))) return rc;
    }
    // split-K slab: the largest any layer asks for at any batch size up to the maximum (a smaller batch
    // can pick more K slices than the full one); conv_launch also clamps its slice count to the slab.
    {
        size_t need = 0;
        auto upd1 = [&](const ConvLayer& L, size_t M) { need = std::max(need, conv_plan(L, (int)M).partial_elems); };
        auto upd = [&](const LayerSet& S, size_t M) { need = std::max(need, set_partial_elems(S, M)); };
        for (size_t f = 1; f <= S; ++f) {
            upd1(c->first, f * HW);
            for (int i = 0; i < c->nd; ++i) upd(c->down[i], f * (HW >> (2 * i)));
        }
        const int cus = c->cus;
        auto upd_poly = [&](const LayerSet& S, size_t f, int Hin, int Win) {   // split polyphase launches: raw slabs of the output
            if (!S.has_patch || !S.patch.w_poly || Hin < 16 || Win < 16) return;
            const int sp = patch_poly_splits(S.patch, (int)f, Hin, Win, c->patch_split_max, cus);
            if (sp > 1) need = std::max(need, (size_t)sp * f * 4 * Hin * Win * S.patch.Cout);
        };
        for (size_t f = 1; f <= F; ++f) {
            for (int i = 0; i < c->nb; ++i) {
                upd(c->hg_enc[i], f * (hw >> (2 * i)));
                upd(c->hg_dec[i], f * (hw >> (2 * (c->nb - i))));
                upd_poly(c->hg_dec[i], f, c->h >> (c->nb - i), c->w >> (c->nb - i));
            }
            for (int i = 0; i < c->nd; ++i) upd_poly(c->up[i], f, c->hf << i, c->wf << i);
            if (c->nb > 0) upd1(c->head, f * hw);
            upd(c->res1[0], f * hwf);
            for (int i = 0; i < c->nd; ++i) upd(c->up[i], f * (hwf << (2 * i)));
            upd1(c->final_conv, f * HW);
        }
        c->partial_elems = need;   // one slab per whole-pass chain
        if ((rc = dev_alloc(c, &c->partial, c->partial_elems * (size_t)max_pass_chains(c)))) return rc;
    }

    // ---- algorithmic FLOPs (reference layer shapes, real channel counts)
    {
        const int cin0_r = (c->K + 1) * (c->Cimg + 1);
        double fe = conv_flops(7, c->Cimg, c->down_r[0], (double)HW);
        for (int i = 0; i < c->nd; ++i) fe += conv_flops(3, c->down_r[i], c->down_r[i + 1], (double)(HW >> (2 * i)));
        c->flops_encode = fe;
        double ff = 0;
        for (int i = 0; i < c->nb; ++i) {
            ff += conv_flops(3, i == 0 ? cin0_r : c->enc_r[i - 1], c->enc_r[i], (double)(hw >> (2 * i)));
            const int ci = i == 0 ? c->enc_r[c->nb - 1] : c->dec_r[i - 1] + c->enc_r[c->nb - 1 - i];
            ff += conv_flops(3, ci, c->dec_r[i], (double)(hw >> (2 * (c->nb - 1 - i))));
        }
        if (c->nb > 0) ff += conv_flops(7, c->dec_r.back() + cin0_r, c->K + 1 + (g.estimate_occlusion_map ? 1 : 0), (double)hw);
        ff += 2.0 * nr * conv_flops(3, c->Cb_r, c->Cb_r, (double)hwf);
        for (int i = 0; i < c->nd; ++i)
            ff += conv_flops(3, i == 0 ? c->Cb_r : c->up_r[i - 1], c->up_r[i], (double)(hwf << (2 * (i + 1))));
        ff += conv_flops(7, c->up_r.back(), c->Cimg, (double)HW);
        if (c->nb > 0) ff += 9.0 * hwf * c->Cb_r;  // bilinear feature warp + occlusion multiply
        c->flops_frame = ff;
    }
    const int max_chains = std::max(c->bneck_chains, max_pass_chains(c));
    c->private_streams = env_int("EAMM_PRIVATE_STREAMS", 0);
    if (max_chains > 1) {
        HIP_TRY(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        for (int k = 1; k < max_chains; ++k) {
            hipStream_t st = chain_stream(c->device, k - 1);
            hipEvent_t ev = nullptr;
            if (!st) return fail(c, EAMM_ERR_HIP, "hipStreamCreate failed for chain %d", k);
            c->pool_streams.push_back(st);
            HIP_TRY(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            c->ev_join.push_back(ev);
            // the private twin (StreamLease): created here, outside any graph capture; idle unless a call needs it
            hipStream_t own = nullptr;
            HIP_TRY(c, hipStreamCreateWithFlags(&own, hipStreamNonBlocking));
            c->own_streams.push_back(own);
        }
    }
    c->side_streams = c->pool_streams;   // (plan queries count them; every call picks its set: StreamLease)
    c->sd.clear();
    HIP_TRY(c, hipDeviceSynchronize());
    c->finalized = true;
    return EAMM_OK;
}

int eamm_encode_source(eamm_ctx* c, const float* source, int ns, void* stream_) {
    if (!c || !source) return fail(c, EAMM_ERR_ARG, "null argument");
    if (!c->finalized) return fail(c, EAMM_ERR_STATE, "call eamm_finalize_weights first");
    if (ns < 1 || ns > c->cfg.max_sources) return fail(c, EAMM_ERR_ARG, "ns=%d outside [1,%d]", ns, c->cfg.max_sources);
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    const size_t HW = (size_t)c->H * c->W;
    if (c->Cimg == 3) {
        HIP_TRY(c, hipMemcpyAsync(c->src_full, source, (size_t)ns * 3 * HW * sizeof(float), hipMemcpyDeviceToDevice, s));
    } else {   // [ns,C,H,W] into the first C planes of [ns,3,H,W]; the kernels below read the zero-extended copy
        HIP_TRY(c, hipMemcpy2DAsync(c->src_full, c->Cpl * HW * sizeof(float), source, c->Cimg * HW * sizeof(float), c->Cimg * HW * sizeof(float),
                                    (size_t)ns, hipMemcpyDeviceToDevice, s));
        source = c->src_full;
    }
    if (c->G == 1) {
        HIP_TRY(c, source_prepare_launch(source, c->aa_w, ns, c->H, c->W, c->cfg.dm_inv_scale, c->Csrc, c->src_nhwc,
                                         c->src_small, s));
    } else {   // two groups of three planes: the padded NHWC copy for `first`, one down-sampled float4 image per group
        HIP_TRY(c, nchw_to_nhwc_pad_launch(source, ns, c->Cpl, c->H, c->W, c->Csrc, c->src_nhwc, s));
        for (int g = 0; g < c->G; ++g)
            HIP_TRY(c, antialias_down_launch(source, c->aa_w, ns, c->H, c->W, c->cfg.dm_inv_scale, 4,
                                             c->src_small + (size_t)g * c->cfg.max_sources * c->h * c->w * 4, s, c->Cpl, 3 * g));
    }
    if (c->first7_w)                                              // SameBlock2d 7x7   generator.py:61
        HIP_TRY(c, first7_launch(source, c->first7_w, c->first7_bias, ns, c->H, c->W, c->down_c[0], c->enc_tmp[0], s));
    else
        HIP_TRY(c, conv_launch(c->first, conv_io(c->src_nhwc, ns, c->H, c->W, ACT_RELU, c->enc_tmp[0], c->partial, c->partial_elems), s));
    for (int i = 0; i < c->nd; ++i) {                             // DownBlock2d       generator.py:62-63
        ConvIO d = conv_io(c->enc_tmp[i], ns, c->H >> i, c->W >> i, ACT_RELU, (i == c->nd - 1) ? c->feat : c->enc_tmp[i + 1], c->partial,
                           c->partial_elems);
        d.pool = 1;
        // F(4x4) form as the hourglass encoder levels, by the source side's rule (eamm_ctx.h: Wino4Pooled)
        if (i < (int)c->w4down.size() && wino4_pooled_pays(c, c->w4down[i], ns * (d.Hin / 4) * (d.Win / 4), Wino4Pooled::SOURCE)) {
            if (int rc = launch_wino4_pooled(c, c->w4down[i], d.in0, ns, d.Hin, d.Win, d.out, c->wino_v, c->wino_z, s)) return rc;
            continue;
        }
        HIP_TRY(c, conv_launch(pick(c, c->down[i], (size_t)ns * d.Hin * d.Win), d, s));
    }
    c->ns_cached = ns;
    return EAMM_OK;
}

int eamm_check_numeric(eamm_ctx* c, void* stream_) {
    if (!c) return EAMM_ERR_ARG;
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    int flag = 0;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    HIP_TRY(c, hipMemcpyAsync(&flag, c->bad_flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    if (flag) {
        HIP_TRY(c, hipMemsetAsync(c->bad_flag, 0, sizeof(int), s));
        return fail(c, EAMM_ERR_NUMERIC, "singular key-point jacobian (torch.inverse would raise, dense_motion.py:56)");
    }
    return EAMM_OK;
}

size_t eamm_source_cache_bytes(const eamm_ctx* c, int ns) {
    if (!c) return 0;
    const size_t per = (size_t)c->hf * c->wf * c->Cb + (size_t)c->G * c->h * c->w * 4 + (size_t)c->Cpl * c->H * c->W;
    return per * (size_t)ns * sizeof(float);
}

int eamm_export_source_cache(eamm_ctx* c, void* dst, int ns, void* stream_) {
    if (!c || !dst) return fail(c, EAMM_ERR_ARG, "null argument");
    if (ns < 1 || ns > c->ns_cached) return fail(c, EAMM_ERR_STATE, "only %d sources are cached", c->ns_cached);
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    const size_t a = (size_t)ns * c->hf * c->wf * c->Cb, b = (size_t)ns * c->h * c->w * 4, d = (size_t)ns * c->Cpl * c->H * c->W;
    const size_t gstride = (size_t)c->cfg.max_sources * c->h * c->w * 4;   // src_small is [group][max_sources][h][w][4]
    float* p = reinterpret_cast<float*>(dst);
    HIP_TRY(c, hipMemcpyAsync(p, c->feat, a * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int g = 0; g < c->G; ++g)
        HIP_TRY(c, hipMemcpyAsync(p + a + g * b, c->src_small + g * gstride, b * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(p + a + c->G * b, c->src_full, d * sizeof(float), hipMemcpyDeviceToDevice, s));
    return EAMM_OK;
}

int eamm_import_source_cache(eamm_ctx* c, const void* src, int ns, void* stream_) {
    if (!c || !src) return fail(c, EAMM_ERR_ARG, "null argument");
    if (!c->finalized) return fail(c, EAMM_ERR_STATE, "call eamm_finalize_weights first");
    if (ns < 1 || ns > c->cfg.max_sources) return fail(c, EAMM_ERR_ARG, "ns=%d outside [1,%d]", ns, c->cfg.max_sources);
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    const size_t a = (size_t)ns * c->hf * c->wf * c->Cb, b = (size_t)ns * c->h * c->w * 4, d = (size_t)ns * c->Cpl * c->H * c->W;
    const size_t gstride = (size_t)c->cfg.max_sources * c->h * c->w * 4;
    const float* p = reinterpret_cast<const float*>(src);
    HIP_TRY(c, hipMemcpyAsync(c->feat, p, a * sizeof(float), hipMemcpyDeviceToDevice, s));
    for (int g = 0; g < c->G; ++g)
        HIP_TRY(c, hipMemcpyAsync(c->src_small + g * gstride, p + a + g * b, b * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(c, hipMemcpyAsync(c->src_full, p + a + c->G * b, d * sizeof(float), hipMemcpyDeviceToDevice, s));
    c->ns_cached = ns;
    return EAMM_OK;
}

double eamm_flops_per_frame(const eamm_ctx* c) { return c ? c->flops_frame : 0.0; }

int eamm_build_experiments(void) {
#ifdef EAMM_EXPERIMENTS
    return 1;
#else
    return 0;
#endif
}
int eamm_knobs_json(char* buf, int cap) { return knobs_json(buf, cap); }
double eamm_total_mfma_flops(void) { return total_mfma_flops(); }
double eamm_encode_flops(const eamm_ctx* c) { return c ? c->flops_encode : 0.0; }

}  // extern "C"
