// C ABI of the audio network AT_net2 up to its LSTM (reference modules/util.py:514-600; demo.py:497 calls it through
// test_auido, demo.py:286-354):
//   example_image -> down_blocks (8 x DownBlock2d, MFMA convolution with the AvgPool2d(2) epilogue) = image_feature [N,512]  :577-581
//   audio [N,T,28,12] -> audio_eocder: conv 1->64 (audio.hip, direct) -> 64->128 (MFMA, 28x12) -> MaxPool2d(3,(1,2)) ->
//                        128->256, 256->256, 256->512 (MFMA, 26x5, raster pixel order) -> MaxPool2d(3,(2,2)) = [12,2,512]      :589
//                     -> audio_eocder_fc: 12288->2048->256 (MFMA as 1x1 convolutions; columns permuted to NHWC at load) * weight :591-593
//   pose [N,T,6] -> pose_encoder 6->128->256 (emo_linear)                                                                       :594
//   lstm_input = [image_feature, audio, pose]: W_ih_l0[:, :512] image_feature + b_ih_l0 + b_hh_l0 once per clip (clipb); the
//   K = 512 rest as one GEMM over the steps; layers 1, 2: W_ih_l x + b_ih_l + b_hh_l as one GEMM each; the recurrences on
//   lstm_rec_kernel (audio.hip)                                                                                                   :596-598
// Every convolution's BatchNorm folds at finalize (fold_conv).  Results are independent of how steps are grouped into passes
// and calls: the GEMMs of the per-step path run with a fixed split-K (1, or FC1_SPLITS for audio_eocder_fc.0), so a frame's
// values do not depend on the pass size, and the recurrence carries (h, c) exactly.
#include "api_common.h"

using namespace eamm;

namespace {

constexpr int MAXN = 8, HID = 256, GATES = 1024, IMG = 256, FC1_SPLITS = 4;
constexpr int AH = 28, AW = 12, PH = 26, PW = 5, QH = 12, QW = 2;   // MFCC window; after the first pool; after the second
const int kDown[9] = {3, 4, 8, 16, 32, 64, 128, 256, 512};

struct Linear {            // nn.Linear, weight transposed [K][O] (emo_linear_launch)
    float *wt = nullptr, *b = nullptr;
};

}  // namespace

struct eamm_audio_ctx : eamm::CtxBase {
    eamm_audio_config cfg{};
    ConvLayer down[8];
    int down_splits[8] = {};         // split-K of each DownBlock at one clip, used for every clip count (a clip's values then do
                                     // not depend on how many clips share the call)
    ConvLayer ac[4];                 // audio_eocder.1, .3, .4, .5
    ConvLayer fc1, fc2, xp[3];       // audio_eocder_fc.0 / .2; the LSTM input projections
    float *c1_w = nullptr, *c1_b = nullptr;
    Linear pose0, pose2, img_proj;
    float* whh[3] = {};
    float *img_pad = nullptr, *img_a = nullptr, *img_b = nullptr, *img_feat = nullptr, *clipb = nullptr;
    float *st_audio = nullptr, *st_pose = nullptr, *buf_a = nullptr, *buf_b = nullptr, *afeat = nullptr, *pfeat = nullptr,
          *pose_h = nullptr, *xproj = nullptr, *y[2] = {};
    float *hs[2] = {}, *cs = nullptr;   // [3][N][256] recurrent state (h ping-pong between launches)
    unsigned long long* gran = nullptr;
    unsigned epoch = 1;
    int* err_host = nullptr;            // pinned, device-mapped: the recurrence's timeout word
    int* err_dev = nullptr;
    unsigned long long limit = 0;
    float* partial = nullptr;
    size_t partial_elems = 0;
};

namespace {

void bn_keys(const std::string& p, std::vector<std::string>* keys) {
    for (const char* s : {".weight", ".bias", ".running_mean", ".running_var"}) keys->push_back(p + s);
}

void wb_keys(const std::string& p, std::vector<std::string>* keys) {
    keys->push_back(p + ".weight");
    keys->push_back(p + ".bias");
}

const HostTensor* need(eamm_audio_ctx* c, const std::string& key, std::vector<int64_t> shape) {
    const HostTensor* t = find(c, key);
    if (!t || t->shape != shape) {
        std::string s;
        for (auto v : shape) s += (s.empty() ? "" : ",") + std::to_string(v);
        fail(c, EAMM_ERR_KEY, "state_dict entry %s missing or mis-shaped (expected [%s])", key.c_str(), s.c_str());
        return nullptr;
    }
    return t;
}

int zero_bias(eamm_audio_ctx* c, const std::string& conv, int cout) {
    HostTensor b;
    b.shape = {cout};
    b.data.assign((size_t)cout, 0.f);
    c->sd[conv + ".bias"] = std::move(b);
    return EAMM_OK;
}

// nn.Linear weight [O][Kfull] (columns k0 .. k0+K) transposed for emo_linear_launch, with the given bias
int build_linear(eamm_audio_ctx* c, const std::string& wkey, int K, int O, const std::vector<float>& bias, Linear* L, int k0 = 0,
                 int Kfull = -1) {
    if (Kfull < 0) Kfull = K;
    const HostTensor* w = need(c, wkey, {O, Kfull});
    if (!w) return EAMM_ERR_KEY;
    std::vector<float> wt((size_t)K * O);
    for (int o = 0; o < O; ++o)
        for (int k = 0; k < K; ++k) wt[(size_t)k * O + o] = w->data[(size_t)o * Kfull + k0 + k];
    if (int rc = upload(c, &L->wt, wt)) return rc;
    return upload(c, &L->b, bias);
}

int build_linear(eamm_audio_ctx* c, const std::string& p, int K, int O, Linear* L) {
    const HostTensor* b = need(c, p + ".bias", {O});
    if (!b) return EAMM_ERR_KEY;
    return build_linear(c, p + ".weight", K, O, b->data, L);
}

// a dense layer [O][Kfull] (columns k0 .. k0+K) as a 1x1 convolution on [M,1,1,K], or on the concatenation of [M,1,1,K-C1]
// and [M,1,1,C1]; perm (optional): packed column j reads source column perm[j]
int build_dense(eamm_audio_ctx* c, const std::string& wkey, int O, int Kfull, int k0, int K, const std::vector<float>& bias,
                const std::vector<int>* perm, ConvLayer* L, int C1 = 0) {
    const HostTensor* w = need(c, wkey, {O, Kfull});
    if (!w) return EAMM_ERR_KEY;
    HostConv f;
    f.Cout = O;
    f.Cin = K;
    f.kh = f.kw = 1;
    f.w.resize((size_t)O * K);
    for (int o = 0; o < O; ++o)
        for (int j = 0; j < K; ++j) f.w[(size_t)o * K + j] = w->data[(size_t)o * Kfull + k0 + (perm ? (*perm)[j] : j)];
    f.b = bias;
    return pack_conv(c, f, nullptr, K - C1, C1, MODE_PLAIN, 0, L);
}

int conv(eamm_audio_ctx* c, const ConvLayer& L, const float* in0, const float* in1, int B, int H, int W, int act, int pool, float* out,
         hipStream_t s, int force_splits) {
    ConvIO io{};
    io.in0 = in0;
    io.in1 = in1;
    io.B = B;
    io.Hin = H;
    io.Win = W;
    io.act = act;
    io.pool = pool;
    io.out = out;
    io.partial = c->partial;
    io.partial_cap = c->partial_elems;
    HIP_TRY(c, conv_launch(L, io, s, force_splits));
    return EAMM_OK;
}

int image_features(eamm_audio_ctx* c, const float* image, int N, hipStream_t s) {
    HIP_TRY(c, nchw_to_nhwc_pad_launch(image, N, 3, IMG, IMG, 32, c->img_pad, s));
    const float* in = c->img_pad;
    int side = IMG;
    for (int i = 0; i < 8; ++i) {
        float* out = i == 7 ? c->img_feat : (i % 2 == 0 ? c->img_a : c->img_b);
        if (int rc = conv(c, c->down[i], in, nullptr, N, side, side, ACT_RELU, 1, out, s, c->down_splits[i])) return rc;
        in = out;
        side /= 2;
    }
    // W_ih_l0[:, :512] image_feature + b_ih_l0 + b_hh_l0                                                          util.py:595-598
    HIP_TRY(c, emo_linear_launch(c->img_feat, 512, nullptr, 0, c->img_proj.wt, c->img_proj.b, GATES, N, 0, c->clipb, s));
    return EAMM_OK;
}

// audio_eocder -> audio_eocder_fc * weight, pose_encoder, layer-0 input projection of F staged frames          util.py:588-596
int step_inputs(eamm_audio_ctx* c, int F, float weight, hipStream_t s) {
    int rc;
    HIP_TRY(c, audio_conv1_launch(c->st_audio, c->c1_w, c->c1_b, F, AH, AW, c->buf_a, s));
    if ((rc = conv(c, c->ac[0], c->buf_a, nullptr, F, AH, AW, ACT_RELU, 0, c->buf_b, s, 1))) return rc;
    HIP_TRY(c, audio_maxpool_launch(c->buf_b, F, AH, AW, 128, 1, 2, c->buf_a, s));
    if ((rc = conv(c, c->ac[1], c->buf_a, nullptr, F, PH, PW, ACT_RELU, 0, c->buf_b, s, 1))) return rc;
    if ((rc = conv(c, c->ac[2], c->buf_b, nullptr, F, PH, PW, ACT_RELU, 0, c->buf_a, s, 1))) return rc;
    if ((rc = conv(c, c->ac[3], c->buf_a, nullptr, F, PH, PW, ACT_RELU, 0, c->buf_b, s, 1))) return rc;
    HIP_TRY(c, audio_maxpool_launch(c->buf_b, F, PH, PW, 512, 2, 2, c->buf_a, s));
    if ((rc = conv(c, c->fc1, c->buf_a, nullptr, F, 1, 1, ACT_RELU, 0, c->buf_b, s, FC1_SPLITS))) return rc;
    if ((rc = conv(c, c->fc2, c->buf_b, nullptr, F, 1, 1, ACT_RELU, 0, c->afeat, s, 1))) return rc;
    HIP_TRY(c, audio_scale_launch(c->afeat, (size_t)F * 256, weight, s));
    HIP_TRY(c, emo_linear_launch(c->st_pose, 6, nullptr, 0, c->pose0.wt, c->pose0.b, 128, F, 1, c->pose_h, s));
    HIP_TRY(c, emo_linear_launch(c->pose_h, 128, nullptr, 0, c->pose2.wt, c->pose2.b, 256, F, 1, c->pfeat, s));
    return conv(c, c->xp[0], c->afeat, c->pfeat, F, 1, 1, ACT_NONE, 0, c->xproj, s, 1);
}

int recur(eamm_audio_ctx* c, int layer, int N, int S, int cur, const float* clipb, float* y, long long ystride, hipStream_t s) {
    LstmArgs a{};
    a.whh = c->whh[layer];
    a.xproj = c->xproj;
    a.clipb = clipb;
    a.N = N;
    a.S = S;
    a.h0 = c->hs[cur] + (size_t)layer * N * HID;
    a.hT = c->hs[cur ^ 1] + (size_t)layer * N * HID;
    a.c = c->cs + (size_t)layer * N * HID;
    a.y = y;
    a.ystride = ystride;
    a.gran = c->gran;
    a.epoch0 = c->epoch;
    a.limit = c->limit;
    a.err = c->err_dev;
    c->epoch += (unsigned)S;
    HIP_TRY(c, lstm_rec_launch(a, s));
    return EAMM_OK;
}

}  // namespace

extern "C" {

const char* eamm_audio_last_error(const eamm_audio_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int eamm_audio_create(const eamm_audio_config* cfg, int device, eamm_audio_ctx** out) {
    if (!cfg || !out) return fail(nullptr, EAMM_ERR_ARG, "null argument");
    *out = nullptr;
    if (cfg->max_batch < MAXN || cfg->max_batch > 4096)
        return fail(nullptr, EAMM_ERR_ARG, "max_batch must be %d .. 4096 (got %d)", MAXN, cfg->max_batch);
    {
        DeviceGuard probe(device);
        if (probe.status != hipSuccess) return fail(nullptr, EAMM_ERR_HIP, "hipSetDevice(%d) failed", device);
    }
    eamm_audio_ctx* c = new eamm_audio_ctx();
    c->cfg = *cfg;
    c->device = device;
    *out = c;
    return EAMM_OK;
}

void eamm_audio_destroy(eamm_audio_ctx* c) {
    if (!c) return;
    free_owned(c);
    if (c->err_host) {
        DeviceGuard guard(c->device);
        (void)hipHostFree(c->err_host);
    }
    delete c;
}

int eamm_audio_load_tensor(eamm_audio_ctx* c, const char* key, const float* host, const int64_t* shape, int ndim) {
    return store_tensor(c, key, host, shape, ndim);
}

int eamm_audio_finalize_weights(eamm_audio_ctx* c) {
    if (!c) return EAMM_ERR_ARG;
    if (c->finalized) return fail(c, EAMM_ERR_STATE, "weights already finalised");
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    {   // the keys this handle uses (AudioFeatureNet keeps decon.* for its DeconvTail and generator.* to itself)
        std::vector<std::string> want;
        for (int i = 0; i < 8; ++i) block_keys("down_blocks." + std::to_string(i), &want);
        for (const char* p : {"pose_encoder.0", "pose_encoder.2", "audio_eocder_fc.0", "audio_eocder_fc.2"}) wb_keys(p, &want);
        for (int idx : {0, 1, 3, 4, 5}) {
            const std::string p = "audio_eocder." + std::to_string(idx);
            want.push_back(p + ".0.weight");
            bn_keys(p + ".1", &want);
        }
        for (int l = 0; l < 3; ++l)
            for (const char* k : {"weight_ih_l", "weight_hh_l", "bias_ih_l", "bias_hh_l"}) want.push_back("lstm." + std::string(k) + std::to_string(l));
        if (int rc = check_keys(c, want)) return rc;
    }
    int rc;
    // image encoder: channels below 32 are zero-padded on both sides (zero filters, zero bias: the padding carries zeros)
    for (int i = 0; i < 8; ++i) {
        const std::string p = "down_blocks." + std::to_string(i);
        const int ci = kDown[i], co = kDown[i + 1], cip = std::max(32, ci), cop = std::max(32, co);
        HostConv f;
        if ((rc = fold_conv(c, {{p + ".conv", p + ".norm"}}, 3, ci, &f))) return rc;
        if (f.Cout != co) return fail(c, EAMM_ERR_KEY, "%s.conv must have %d output channels", p.c_str(), co);
        f.w.resize((size_t)cop * ci * 9, 0.f);
        f.b.resize(cop, 0.f);
        f.Cout = cop;
        const std::vector<int> map = channel_map(ci, cip, 0, 0);
        if ((rc = pack_conv(c, f, map.data(), cip, 0, MODE_PLAIN, 0, &c->down[i]))) return rc;
    }
    // audio_eocder: bias-free convolutions + BatchNorm                                                           util.py:539-546
    const int acin[5] = {1, 64, 128, 256, 256}, acout[5] = {64, 128, 256, 256, 512}, aidx[5] = {0, 1, 3, 4, 5};
    for (int j = 0; j < 5; ++j) {
        const std::string p = "audio_eocder." + std::to_string(aidx[j]);
        if ((rc = zero_bias(c, p + ".0", acout[j]))) return rc;
        HostConv f;
        if ((rc = fold_conv(c, {{p + ".0", p + ".1"}}, 3, acin[j], &f))) return rc;
        if (f.Cout != acout[j]) return fail(c, EAMM_ERR_KEY, "%s.0 must have %d output channels", p.c_str(), acout[j]);
        if (j == 0) {   // [64][1][3][3] -> [9][64]
            std::vector<float> w(9 * 64);
            for (int o = 0; o < 64; ++o)
                for (int t = 0; t < 9; ++t) w[t * 64 + o] = f.w[o * 9 + t];
            if ((rc = upload(c, &c->c1_w, w)) || (rc = upload(c, &c->c1_b, f.b))) return rc;
        } else if ((rc = pack_conv(c, f, nullptr, acin[j], 0, MODE_PLAIN, 0, &c->ac[j - 1]))) {
            return rc;
        }
    }
    // audio_eocder_fc: the reference flattens NCHW [512,12,2]; the activations here are NHWC [12,2,512]          util.py:590-591
    {
        const HostTensor* b0 = need(c, "audio_eocder_fc.0.bias", {2048});
        const HostTensor* b2 = need(c, "audio_eocder_fc.2.bias", {256});
        if (!b0 || !b2) return EAMM_ERR_KEY;
        std::vector<int> perm(12288);
        for (int y = 0; y < QH; ++y)
            for (int x = 0; x < QW; ++x)
                for (int ch = 0; ch < 512; ++ch) perm[(y * QW + x) * 512 + ch] = ch * QH * QW + y * QW + x;
        if ((rc = build_dense(c, "audio_eocder_fc.0.weight", 2048, 12288, 0, 12288, b0->data, &perm, &c->fc1))) return rc;
        if ((rc = build_dense(c, "audio_eocder_fc.2.weight", 256, 2048, 0, 2048, b2->data, nullptr, &c->fc2))) return rc;
    }
    if ((rc = build_linear(c, "pose_encoder.0", 6, 128, &c->pose0)) || (rc = build_linear(c, "pose_encoder.2", 128, 256, &c->pose2)))
        return rc;
    // LSTM: input projections (layer 0: the image columns per clip, the audio + pose columns per step) and W_hh images
    for (int l = 0; l < 3; ++l) {
        const std::string L = std::to_string(l);
        const HostTensor *bi = need(c, "lstm.bias_ih_l" + L, {GATES}), *bh = bi ? need(c, "lstm.bias_hh_l" + L, {GATES}) : nullptr;
        const HostTensor* whh = bh ? need(c, "lstm.weight_hh_l" + L, {GATES, HID}) : nullptr;
        if (!whh) return EAMM_ERR_KEY;
        std::vector<float> bsum(GATES);
        for (int o = 0; o < GATES; ++o) bsum[o] = (float)((double)bi->data[o] + (double)bh->data[o]);
        if (l == 0) {
            if ((rc = build_linear(c, "lstm.weight_ih_l0", 512, GATES, bsum, &c->img_proj, 0, 1024))) return rc;
            if ((rc = build_dense(c, "lstm.weight_ih_l0", GATES, 1024, 512, 512, std::vector<float>(GATES, 0.f), nullptr, &c->xp[0], 256)))
                return rc;
        } else if ((rc = build_dense(c, "lstm.weight_ih_l" + L, GATES, HID, 0, HID, bsum, nullptr, &c->xp[l]))) {
            return rc;
        }
        std::vector<float> packed((size_t)LSTM_WG * HID * 64);
        lstm_pack_whh_host(whh->data.data(), packed.data());
        if ((rc = upload(c, &c->whh[l], packed))) return rc;
    }
    // workspaces
    const size_t F = c->cfg.max_batch;
    const size_t act = std::max<size_t>((size_t)AH * AW * 128, (size_t)PH * PW * 512);
    if ((rc = dev_alloc(c, &c->img_pad, (size_t)MAXN * IMG * IMG * 32)) || (rc = dev_alloc(c, &c->img_a, (size_t)MAXN * 128 * 128 * 32)) ||
        (rc = dev_alloc(c, &c->img_b, (size_t)MAXN * 64 * 64 * 32)) || (rc = dev_alloc(c, &c->img_feat, (size_t)MAXN * 512)) ||
        (rc = dev_alloc(c, &c->clipb, (size_t)MAXN * GATES)) || (rc = dev_alloc(c, &c->st_audio, F * AH * AW)) ||
        (rc = dev_alloc(c, &c->st_pose, F * 6)) || (rc = dev_alloc(c, &c->buf_a, F * act)) || (rc = dev_alloc(c, &c->buf_b, F * act)) ||
        (rc = dev_alloc(c, &c->afeat, F * 256)) || (rc = dev_alloc(c, &c->pfeat, F * 256)) || (rc = dev_alloc(c, &c->pose_h, F * 128)) ||
        (rc = dev_alloc(c, &c->xproj, F * GATES)) || (rc = dev_alloc(c, &c->y[0], F * HID)) || (rc = dev_alloc(c, &c->y[1], F * HID)) ||
        (rc = dev_alloc(c, &c->hs[0], (size_t)3 * MAXN * HID)) || (rc = dev_alloc(c, &c->hs[1], (size_t)3 * MAXN * HID)) ||
        (rc = dev_alloc(c, &c->cs, (size_t)3 * MAXN * HID)) || (rc = dev_alloc(c, &c->gran, (size_t)2 * MAXN * HID)))
        return rc;
    HIP_TRY(c, hipMemset(c->gran, 0, sizeof(unsigned long long) * 2 * MAXN * HID));
    size_t need_p = 0;
    {
        int side = IMG;
        for (int i = 0; i < 8; ++i, side /= 2) {
            c->down_splits[i] = conv_plan(c->down[i], side * side).splits;
            need_p = std::max(need_p, conv_plan(c->down[i], MAXN * side * side, c->down_splits[i]).partial_elems);
        }
    }
    need_p = std::max(need_p, conv_plan(c->fc1, (int)F, FC1_SPLITS).partial_elems);
    c->partial_elems = need_p;
    if ((rc = dev_alloc(c, &c->partial, need_p))) return rc;
    HIP_TRY(c, hipHostMalloc(reinterpret_cast<void**>(&c->err_host), sizeof(int), hipHostMallocMapped | hipHostMallocCoherent));
    *c->err_host = 0;
    HIP_TRY(c, hipHostGetDevicePointer(reinterpret_cast<void**>(&c->err_dev), c->err_host, 0));
    {   // a wait may take 10 s of wall clock: far beyond any step, long enough for a loaded chip to dispatch every workgroup
        int khz = 100000;
        if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->device) != hipSuccess || khz <= 0) khz = 100000;
        c->limit = (unsigned long long)khz * 1000ull * 10ull;
    }
    c->sd.clear();
    HIP_TRY(c, hipDeviceSynchronize());
    c->finalized = true;
    return EAMM_OK;
}

int eamm_audio_check(eamm_audio_ctx* c, void* stream) {
    if (!c) return fail(c, EAMM_ERR_ARG, "null argument");
    if (stream) {
        DeviceGuard guard(c->device);
        if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
        HIP_TRY(c, hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    }
    if (c->err_host && __atomic_load_n(c->err_host, __ATOMIC_ACQUIRE))
        return fail(c, EAMM_ERR_HIP, "an LSTM recurrence timed out waiting for another workgroup: its results are invalid and the handle "
                                     "is unusable");
    return EAMM_OK;
}

int eamm_audio_lstm_features(eamm_audio_ctx* c, const float* image, const float* audio, const float* pose, int N, int T, float weight,
                             const float* h0, const float* c0, float* h_out, float* c_out, float* clip_bias, float* out, void* stream_) {
    if (!c || !audio || !pose || !out) return fail(c, EAMM_ERR_ARG, "null argument");
    if (!image && !clip_bias) return fail(c, EAMM_ERR_ARG, "neither an image nor a clip bias from an earlier call");
    if (!c->finalized) return fail(c, EAMM_ERR_STATE, "call eamm_audio_finalize_weights first");
    if (N < 1 || N > MAXN) return fail(c, EAMM_ERR_ARG, "clips %d outside [1,%d]", N, MAXN);
    if (T < 1) return fail(c, EAMM_ERR_ARG, "steps %d < 1", T);
    if (__atomic_load_n(c->err_host, __ATOMIC_ACQUIRE))
        return fail(c, EAMM_ERR_HIP, "an earlier LSTM recurrence timed out waiting for another workgroup; the handle is unusable");
    DeviceGuard guard(c->device);
    if (guard.status != hipSuccess) return fail(c, EAMM_ERR_HIP, "hipSetDevice(%d) failed", c->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream_);
    const size_t state = (size_t)3 * N * HID;
    if (h0) HIP_TRY(c, hipMemcpyAsync(c->hs[0], h0, sizeof(float) * state, hipMemcpyDeviceToDevice, s));
    else HIP_TRY(c, hipMemsetAsync(c->hs[0], 0, sizeof(float) * state, s));
    if (c0) HIP_TRY(c, hipMemcpyAsync(c->cs, c0, sizeof(float) * state, hipMemcpyDeviceToDevice, s));
    else HIP_TRY(c, hipMemsetAsync(c->cs, 0, sizeof(float) * state, s));
    int rc;
    const float* clipb = clip_bias;
    if (image) {   // the image encoder, once per clip: a chunked clip passes its first call's clip_bias on instead
        if ((rc = image_features(c, image, N, s))) return rc;
        clipb = c->clipb;
        if (clip_bias) HIP_TRY(c, hipMemcpyAsync(clip_bias, c->clipb, sizeof(float) * N * GATES, hipMemcpyDeviceToDevice, s));
    }
    const int chunk = c->cfg.max_batch / N;
    int cur = 0;
    for (int s0 = 0; s0 < T; s0 += chunk) {
        const int S = std::min(chunk, T - s0), F = N * S;
        // this chunk's steps of every clip, clip-major: frame n * S + s
        HIP_TRY(c, hipMemcpy2DAsync(c->st_audio, sizeof(float) * S * AH * AW, audio + (size_t)s0 * AH * AW, sizeof(float) * T * AH * AW,
                                    sizeof(float) * S * AH * AW, N, hipMemcpyDeviceToDevice, s));
        HIP_TRY(c, hipMemcpy2DAsync(c->st_pose, sizeof(float) * S * 6, pose + (size_t)s0 * 6, sizeof(float) * T * 6, sizeof(float) * S * 6,
                                    N, hipMemcpyDeviceToDevice, s));
        if ((rc = step_inputs(c, F, weight, s))) return rc;
        if ((rc = recur(c, 0, N, S, cur, clipb, c->y[0], (long long)S * HID, s))) return rc;
        if ((rc = conv(c, c->xp[1], c->y[0], nullptr, F, 1, 1, ACT_NONE, 0, c->xproj, s, 1))) return rc;
        if ((rc = recur(c, 1, N, S, cur, nullptr, c->y[1], (long long)S * HID, s))) return rc;
        if ((rc = conv(c, c->xp[2], c->y[1], nullptr, F, 1, 1, ACT_NONE, 0, c->xproj, s, 1))) return rc;
        if ((rc = recur(c, 2, N, S, cur, nullptr, out + (size_t)s0 * HID, (long long)T * HID, s))) return rc;
        cur ^= 1;
    }
    if (h_out) HIP_TRY(c, hipMemcpyAsync(h_out, c->hs[cur], sizeof(float) * state, hipMemcpyDeviceToDevice, s));
    if (c_out) HIP_TRY(c, hipMemcpyAsync(c_out, c->cs, sizeof(float) * state, hipMemcpyDeviceToDevice, s));
    return EAMM_OK;
}

}  // extern "C"
