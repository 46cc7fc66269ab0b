// C ABI of the emotion detector Emotion_k (reference modules/util.py:1223-1527; demo.py:68-70 builds it with --type linear_3 and
// demo.py:221-228 calls forward + feature once per frame of the emotion video):
//   image -> anti-alias down -> Hourglass (hourglass_common.h, the key-point detector's)            util.py:1498-1501
//         -> conv1 3x3 (35 -> 64) + bn1 + ReLU (MFMA convolution, concat in the loader) -> MaxPool2d(3, 2, 1)   :1502-1505
//         -> layer1 .. layer4 (BasicBlock x 2 each; stride-1 3x3 on the path's MFMA kernels with the residual add and ReLU in
//            the epilogue, stride-2 3x3 and 1x1 shortcut on conv_s2.hip) -> AdaptiveAvgPool2d(1) = `feature`     :1507-1512
//         -> classify.last_fc = fake; embed(value, jacobian) -> fc_p; fc_all(cat(out, ner)) -> final -> value, jacobian :1513-1525
// All BatchNorms are folded into the convolutions at finalize (fold_conv); the trunk's bias-free convolutions get zero biases.
#include "hourglass_common.h"

using namespace eamm;

namespace {

struct EmoBlock {          // one BasicBlock (util.py:1069-1099)
    LayerSet c1, c2;       // stride-1 convolutions (c1 unused when s2)
    ConvLayer c1s2, ds;    // stride-2 3x3 conv1 and the 1x1 stride-2 downsample
    bool s2 = false;
    int cin = 0, cout = 0;
};

struct Linear {            // nn.Linear, weight transposed [K][O]
    float *wt = nullptr, *b = nullptr;
    int K = 0, O = 0;
};

}  // namespace

struct eamm_emo_ctx : eamm::CtxBase {
    eamm_emo_config cfg{};
    int H = 0, W = 0, h = 0, w = 0;
    int Cin_pad = 32;
    Hourglass hg;
    LayerSet stem;                  // conv1 + bn1 on [hourglass out | x_in]
    EmoBlock blocks[8];
    Linear fake, fcp0, fcp2, fa0, fa2, fa4;
    float* final_w = nullptr;       // `final`'s three Conv1d (emo_final_kernel's layout)
    float *aa_w = nullptr, *img_stage = nullptr, *x_in = nullptr;
    float* stem_out = nullptr;      // [F,h,w,64]
    float* act[4] = {};             // trunk activations, [F,h/2,w/2,64] floats each (the largest level)
    float *feat = nullptr, *emb = nullptr, *h1 = nullptr, *ner = nullptr, *a1 = nullptr, *a2 = nullptr, *a3 = nullptr;
    float* partial = nullptr;
    size_t partial_elems = 0;
};

namespace {

const char* kLayer[4] = {"layer1", "layer2", "layer3", "layer4"};
const int kWidth[4] = {64, 128, 256, 512};

std::string blk_name(int i) { return std::string(kLayer[i / 2]) + "." + std::to_string(i % 2); }

void bn_keys(const std::string& p, std::vector<std::string>* keys) {
    for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"}) keys->push_back(p + s);
}

void wb_keys(const std::string& p, std::vector<std::string>* keys) {
    keys->push_back(p + ".weight");
    keys->push_back(p + ".bias");
}

// the bias-free convolutions get an explicit zero bias so that fold_conv folds their BatchNorm like every other
int zero_bias(eamm_emo_ctx* c, const std::string& conv) {
    const HostTensor* w = find(c, conv + ".weight");
    if (!w || w->shape.empty()) return fail(c, EAMM_ERR_KEY, "state_dict entry %s.weight missing", conv.c_str());
    HostTensor b;
    b.shape = {w->shape[0]};
    b.data.assign((size_t)w->shape[0], 0.f);
    c->sd[conv + ".bias"] = std::move(b);
    return EAMM_OK;
}

int build_linear(eamm_emo_ctx* c, const std::string& p, int K, int O, Linear* L) {
    const HostTensor *w = find(c, p + ".weight"), *b = find(c, p + ".bias");
    if (!w || w->shape.size() != 2 || w->shape[0] != O || w->shape[1] != K || !b || (int)b->numel() != O)
        return fail(c, EAMM_ERR_KEY, "state_dict entry %s mis-shaped (expected weight [%d,%d], bias [%d])", p.c_str(), O, K, O);
    std::vector<float> wt((size_t)K * O);
    for (int o = 0; o < O; ++o)
        for (int k = 0; k < K; ++k) wt[(size_t)k * O + o] = w->data[(size_t)o * K + k];
    L->K = K;
    L->O = O;
    if (int rc = upload(c, &L->wt, wt)) return rc;
    return upload(c, &L->b, b->data);
}

int append_conv1d(eamm_emo_ctx* c, const std::string& p, int co, int ci, int k, std::vector<float>* out) {
    const HostTensor *w = find(c, p + ".weight"), *b = find(c, p + ".bias");
    if (!w || w->shape.size() != 3 || w->shape[0] != co || w->shape[1] != ci || w->shape[2] != k || !b || (int)b->numel() != co)
        return fail(c, EAMM_ERR_KEY, "state_dict entry %s mis-shaped (expected weight [%d,%d,%d], bias [%d])", p.c_str(), co, ci, k, co);
    out->insert(out->end(), w->data.begin(), w->data.end());
    out->insert(out->end(), b->data.begin(), b->data.end());
    return EAMM_OK;
}

int conv(eamm_emo_ctx* c, const LayerSet& S, const float* in0, const float* in1, int B, int Hs, int Ws, int act, const float* resid,
         float* out, hipStream_t s) {
    ConvIO io{};
    io.in0 = in0;
    io.in1 = in1;
    io.B = B;
    io.Hin = Hs;
    io.Win = Ws;
    io.act = act;
    io.resid = resid;
    io.out = out;
    io.partial = c->partial;
    io.partial_cap = c->partial_elems;
    HIP_TRY(c, conv_launch(pick(c, S, (size_t)B * Hs * Ws), io, s));
    return EAMM_OK;
}

}  // namespace

extern "C" {

const char* eamm_emo_last_error(const eamm_emo_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int eamm_emo_create(const eamm_emo_config* cfg, int device, eamm_emo_ctx** out) {
    if (!cfg || !out) return fail(nullptr, EAMM_ERR_ARG, "null argument");
    *out = nullptr;
    const eamm_emo_config& g = *cfg;
    if (g.num_channels < 1 || g.num_channels > 8) return fail(nullptr, EAMM_ERR_ARG, "num_channels must be 1 .. 8 (got %d)", g.num_channels);
    if (g.block_expansion % 32 || g.max_features % 32 || g.num_blocks < 1)
        return fail(nullptr, EAMM_ERR_ARG, "channel widths must be multiples of 32");
    if (g.inv_scale != 1 && g.inv_scale != 2 && g.inv_scale != 4) return fail(nullptr, EAMM_ERR_ARG, "1/scale_factor must be 1, 2 or 4");
    if (g.num_classes < 1 || g.num_classes > 4096) return fail(nullptr, EAMM_ERR_ARG, "num_classes must be 1 .. 4096 (got %d)", g.num_classes);
    if (g.max_batch < 1) return fail(nullptr, EAMM_ERR_ARG, "max_batch < 1");
    const int div = g.inv_scale << std::max(g.num_blocks, 4);   // hourglass levels; the trunk halves the map four times
    if (g.height < div || g.width < div || g.height % div || g.width % div)
        return fail(nullptr, EAMM_ERR_ARG, "frame %dx%d not divisible for scale 1/%d, %d hourglass levels and the trunk's 16x reduction",
                    g.height, g.width, g.inv_scale, g.num_blocks);
    {
        DeviceGuard probe(device);
        if (probe.status != hipSuccess) return fail(nullptr, EAMM_ERR_HIP, "hipSetDevice(%d) failed", device);
    }
    eamm_emo_ctx* c = new eamm_emo_ctx();
    c->cfg = g;
    c->device = device;
    c->H = g.height;
    c->W = g.width;
    c->h = c->H / g.inv_scale;
    c->w = c->W / g.inv_scale;
    c->Cin_pad = (g.num_channels + 31) / 32 * 32;
    hg_channels(&c->hg, g.block_expansion, g.max_features, g.num_blocks);
    read_tile_knobs(c);
    *out = c;
    return EAMM_OK;
}

void eamm_emo_destroy(eamm_emo_ctx* c) {
    if (!c) return;
    free_owned(c);
    delete c;
}

int eamm_emo_load_tensor(eamm_emo_ctx* c, const char* key, const float* host, const int64_t* shape, int ndim) {
    return store_tensor(c, key, host, shape, ndim);
}

int eamm_emo_finalize_weights(eamm_emo_ctx* c) {
    if (!c) return EAMM_ERR_ARG;
    if (c->finalized) return fail(c, EAMM_ERR_STATE, "weights already finalised");
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    const eamm_emo_config& g = c->cfg;
    {   // the reference's whole key set (load_state_dict(strict=True), demo.py:95); fc / fc_n / final_4 / final_10 are ignored
        std::vector<std::string> want;
        hg_keys("predictor", c->hg.nb, &want);
        if (g.inv_scale != 1) want.push_back("down.weight");
        want.push_back("conv1.weight");
        bn_keys("bn1", &want);
        for (int i = 0; i < 8; ++i) {
            const std::string p = blk_name(i);
            want.push_back(p + ".conv1.weight");
            bn_keys(p + ".bn1", &want);
            want.push_back(p + ".conv2.weight");
            bn_keys(p + ".bn2", &want);
            if (i % 2 == 0 && i > 0) {
                want.push_back(p + ".downsample.0.weight");
                bn_keys(p + ".downsample.1", &want);
            }
        }
        for (const char* p : {"fc", "fc_p.0", "fc_p.2", "fc_n.0", "fc_n.2", "fc_all.0", "fc_all.2", "fc_all.4", "final.0", "final.3",
                              "final.5", "final_4.0", "final_4.3", "final_10.0", "final_10.3", "classify.last_fc"})
            wb_keys(p, &want);
        if (int rc = check_keys(c, want)) return rc;
    }
    int rc;
    const int cin = g.num_channels;
    if ((rc = hg_build(c, &c->hg, "predictor", cin, c->Cin_pad))) return rc;
    if ((rc = hg_build_input(c, g.num_channels, g.inv_scale, c->H, c->W, g.max_batch, &c->aa_w, &c->img_stage))) return rc;
    // stem: conv1 over cat[hourglass out (block_expansion), image (num_channels, stored Cin_pad wide)]      util.py:1502-1504
    if ((rc = zero_bias(c, "conv1"))) return rc;
    const int be = c->hg.dec_c.back();
    if ((rc = build_set(c, {{"conv1", "bn1"}}, be, be, cin, c->Cin_pad, &c->stem, MODE_PLAIN))) return rc;
    if (c->stem.base.Cout != 64) return fail(c, EAMM_ERR_KEY, "conv1 must have 64 output channels");
    int inplanes = 64;
    for (int i = 0; i < 8; ++i) {
        EmoBlock& B = c->blocks[i];
        const std::string p = blk_name(i);
        B.cin = inplanes;
        B.cout = kWidth[i / 2];
        B.s2 = i % 2 == 0 && i > 0;
        for (const char* cv : {".conv1", ".conv2"})
            if ((rc = zero_bias(c, p + cv))) return rc;
        if (B.s2) {
            HostConv f;
            if ((rc = fold_conv(c, {{p + ".conv1", p + ".bn1"}}, 3, B.cin, &f))) return rc;
            if ((rc = pack_conv(c, f, nullptr, B.cin, 0, MODE_PLAIN, 0, &B.c1s2))) return rc;
            if ((rc = zero_bias(c, p + ".downsample.0"))) return rc;
            HostConv d;
            if ((rc = fold_conv(c, {{p + ".downsample.0", p + ".downsample.1"}}, 1, B.cin, &d))) return rc;
            if ((rc = pack_conv(c, d, nullptr, B.cin, 0, MODE_PLAIN, 0, &B.ds))) return rc;
            if (B.c1s2.Cout != B.cout || B.ds.Cout != B.cout) return fail(c, EAMM_ERR_KEY, "%s has the wrong channel count", p.c_str());
        } else {
            if ((rc = build_set(c, {{p + ".conv1", p + ".bn1"}}, B.cin, B.cin, 0, 0, &B.c1, MODE_PLAIN))) return rc;
            if (B.c1.base.Cout != B.cout) return fail(c, EAMM_ERR_KEY, "%s.conv1 has the wrong channel count", p.c_str());
        }
        if ((rc = build_set(c, {{p + ".conv2", p + ".bn2"}}, B.cout, B.cout, 0, 0, &B.c2, MODE_PLAIN))) return rc;
        if (B.c2.base.Cout != B.cout) return fail(c, EAMM_ERR_KEY, "%s.conv2 has the wrong channel count", p.c_str());
        inplanes = B.cout;
    }
    // head                                                                                                   util.py:1513-1525
    if ((rc = build_linear(c, "classify.last_fc", 512, g.num_classes, &c->fake))) return rc;
    if ((rc = build_linear(c, "fc_p.0", 1260, 1024, &c->fcp0))) return rc;
    if ((rc = build_linear(c, "fc_p.2", 1024, 512, &c->fcp2))) return rc;
    if ((rc = build_linear(c, "fc_all.0", 1024, 512, &c->fa0))) return rc;
    if ((rc = build_linear(c, "fc_all.2", 512, 256, &c->fa2))) return rc;
    if ((rc = build_linear(c, "fc_all.4", 256, 64, &c->fa4))) return rc;
    {
        std::vector<float> fw;
        if ((rc = append_conv1d(c, "final.0", 2, 1, 4, &fw)) || (rc = append_conv1d(c, "final.3", 4, 2, 4, &fw)) ||
            (rc = append_conv1d(c, "final.5", 4, 4, 3, &fw)))
            return rc;
        if ((rc = upload(c, &c->final_w, fw))) return rc;
    }

    const size_t F = g.max_batch, hw = (size_t)c->h * c->w, hw2 = hw / 4;
    if ((rc = dev_alloc(c, &c->x_in, F * hw * c->Cin_pad))) return rc;
    if ((rc = dev_alloc(c, &c->stem_out, F * hw * 64))) return rc;
    for (auto& a : c->act)
        if ((rc = dev_alloc(c, &a, F * hw2 * 64))) return rc;
    if ((rc = dev_alloc(c, &c->feat, F * 512)) || (rc = dev_alloc(c, &c->emb, F * 1260)) || (rc = dev_alloc(c, &c->h1, F * 1024)) ||
        (rc = dev_alloc(c, &c->ner, F * 512)) || (rc = dev_alloc(c, &c->a1, F * 512)) || (rc = dev_alloc(c, &c->a2, F * 256)) ||
        (rc = dev_alloc(c, &c->a3, F * 64)))
        return rc;
    size_t need = 0;
    if ((rc = hg_alloc(c, &c->hg, F, hw, &need))) return rc;
    for (size_t f = 1; f <= F; ++f) {
        need = std::max(need, set_partial_elems(c->stem, f * hw));
        int hs = c->h / 2, ws = c->w / 2;
        for (int i = 0; i < 8; ++i) {
            const EmoBlock& B = c->blocks[i];
            if (B.s2) {
                need = std::max({need, conv_s2_partial_elems(B.c1s2, (int)f, hs, ws), conv_s2_partial_elems(B.ds, (int)f, hs, ws)});
                hs /= 2;
                ws /= 2;
            } else {
                need = std::max(need, set_partial_elems(B.c1, f * hs * ws));
            }
            need = std::max(need, set_partial_elems(B.c2, f * hs * ws));
        }
    }
    c->partial_elems = need;
    if ((rc = dev_alloc(c, &c->partial, need))) return rc;
    c->sd.clear();
    HIP_TRY(c, hipDeviceSynchronize());
    c->finalized = true;
    return EAMM_OK;
}

int eamm_emo_detect(eamm_emo_ctx* c, const float* image, const float* kp_value, const float* kp_jacobian, int B,
                    const eamm_emo_outputs* o, void* stream_) {
    if (!c || !image || !o) return fail(c, EAMM_ERR_ARG, "null argument");
    if (!c->finalized) return fail(c, EAMM_ERR_STATE, "call eamm_emo_finalize_weights first");
    if (B < 1 || B > c->cfg.max_batch) return fail(c, EAMM_ERR_ARG, "batch %d outside [1,%d]", B, c->cfg.max_batch);
    const bool want_kp = o->value || o->jacobian;
    if (want_kp && (!kp_value || !kp_jacobian)) return fail(c, EAMM_ERR_ARG, "value / jacobian requested without the input key points");
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    const int h = c->h, w = c->w;
    int rc;
    // feature_map = predictor(down(x))                                                                      util.py:1499-1501
    if ((rc = hg_input(c, image, c->aa_w, c->img_stage, B, c->cfg.num_channels, c->H, c->W, c->cfg.inv_scale, c->Cin_pad, c->x_in, s)))
        return rc;
    if ((rc = hg_run(c, c->hg, c->x_in, B, h, w, c->partial, c->partial_elems, s))) return rc;
    // relu(bn1(conv1(feature_map))) -> maxpool                                                               util.py:1502-1505
    if ((rc = conv(c, c->stem, c->hg.u_buf[c->hg.nb - 1], c->x_in, B, h, w, ACT_RELU, nullptr, c->stem_out, s))) return rc;
    HIP_TRY(c, emo_maxpool_launch(c->stem_out, B, h, w, 64, c->act[0], s));
    // layer1 .. layer4                                                                                       util.py:1507-1510
    int xi = 0, hs = h / 2, ws = w / 2;
    for (int i = 0; i < 8; ++i) {
        const EmoBlock& Bk = c->blocks[i];
        int others[3], n = 0;
        for (int j = 0; j < 4; ++j)
            if (j != xi) others[n++] = j;
        float *x = c->act[xi], *t = c->act[others[0]], *d = c->act[others[1]], *y = c->act[others[2]];
        if (Bk.s2) {
            HIP_TRY(c, conv_s2_launch(Bk.c1s2, x, B, hs, ws, ACT_RELU, nullptr, t, c->partial, c->partial_elems, s));
            HIP_TRY(c, conv_s2_launch(Bk.ds, x, B, hs, ws, ACT_NONE, nullptr, d, c->partial, c->partial_elems, s));
            hs /= 2;
            ws /= 2;
            if ((rc = conv(c, Bk.c2, t, nullptr, B, hs, ws, ACT_RELU, d, y, s))) return rc;
        } else {
            if ((rc = conv(c, Bk.c1, x, nullptr, B, hs, ws, ACT_RELU, nullptr, t, s))) return rc;
            if ((rc = conv(c, Bk.c2, t, nullptr, B, hs, ws, ACT_RELU, x, y, s))) return rc;
        }
        xi = others[2];
    }
    // avgpool -> out [B,512]                                                                                 util.py:1511-1512
    HIP_TRY(c, emo_avgpool_launch(c->act[xi], B, hs * ws, 512, c->feat, s));
    if (o->feature) HIP_TRY(c, hipMemcpyAsync(o->feature, c->feat, sizeof(float) * B * 512, hipMemcpyDeviceToDevice, s));
    if (o->fake)                                                                                            // util.py:1513
        HIP_TRY(c, emo_linear_launch(c->feat, 512, nullptr, 0, c->fake.wt, c->fake.b, c->fake.O, B, 0, o->fake, s));
    if (!want_kp) return EAMM_OK;
    // embed(cat(value, jacobian)) -> fc_p -> fc_all(cat(out, ner)) -> final                                  util.py:1514-1525
    HIP_TRY(c, emo_embed_launch(kp_value, kp_jacobian, B, c->emb, s));
    HIP_TRY(c, emo_linear_launch(c->emb, 1260, nullptr, 0, c->fcp0.wt, c->fcp0.b, 1024, B, 1, c->h1, s));
    HIP_TRY(c, emo_linear_launch(c->h1, 1024, nullptr, 0, c->fcp2.wt, c->fcp2.b, 512, B, 1, c->ner, s));
    HIP_TRY(c, emo_linear_launch(c->feat, 512, c->ner, 512, c->fa0.wt, c->fa0.b, 512, B, 1, c->a1, s));
    HIP_TRY(c, emo_linear_launch(c->a1, 512, nullptr, 0, c->fa2.wt, c->fa2.b, 256, B, 1, c->a2, s));
    HIP_TRY(c, emo_linear_launch(c->a2, 256, nullptr, 0, c->fa4.wt, c->fa4.b, 64, B, 1, c->a3, s));
    HIP_TRY(c, emo_final_launch(c->a3, c->final_w, B, o->value, o->jacobian, s));
    return EAMM_OK;
}

}  // extern "C"
