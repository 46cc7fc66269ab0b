// The `predictor` front of the image detectors (KPDetector, keypoint_detector.py:77-81; Emotion_k, util.py:1498-1501), shared
// by eamm_kp_api.hip and eamm_emo_api.hip: AntiAliasInterpolation2d down-sampling to NHWC, then the Hourglass (util.py:941-1002)
// as the path's fp32-MFMA convolutions (pool in the encoder's epilogue, collapsed up-conv, concat in the loader).
// The output is the pair (u_buf.back() [B,h,w,block_expansion], x_in [B,h,w,Cin_pad]): the consumer's loader concatenates them.
#pragma once
#include "api_common.h"

namespace eamm {
namespace {

struct Hourglass {
    int nb = 0;
    std::vector<int> enc_c, dec_c;
    std::vector<LayerSet> enc, dec;
    std::vector<float*> e_buf, u_buf;
};

inline void hg_channels(Hourglass* hg, int block_expansion, int max_features, int num_blocks) {
    hg->nb = num_blocks;
    hg->enc_c.clear();
    hg->dec_c.clear();
    for (int i = 0; i < num_blocks; ++i) hg->enc_c.push_back(std::min(max_features, block_expansion << (i + 1)));
    for (int i = num_blocks - 1; i >= 0; --i) hg->dec_c.push_back(std::min(max_features, block_expansion << i));
}

inline void hg_keys(const std::string& prefix, int nb, std::vector<std::string>* want) {
    for (int i = 0; i < nb; ++i) block_keys(prefix + ".encoder.down_blocks." + std::to_string(i), want);
    for (int i = 0; i < nb; ++i) block_keys(prefix + ".decoder.up_blocks." + std::to_string(i), want);
}

// cin real input channels stored cin_pad wide
inline int hg_build(CtxBase* c, Hourglass* hg, const std::string& prefix, int cin, int cin_pad) {
    int rc;
    hg->enc.resize(hg->nb);
    hg->dec.resize(hg->nb);
    for (int i = 0; i < hg->nb; ++i) {
        const std::string p = prefix + ".encoder.down_blocks." + std::to_string(i);
        const int cr = i == 0 ? cin : hg->enc_c[i - 1], cp = i == 0 ? cin_pad : hg->enc_c[i - 1];
        if ((rc = build_set(c, {{p + ".conv", p + ".norm"}}, cr, cp, 0, 0, &hg->enc[i], MODE_PLAIN))) return rc;
    }
    for (int i = 0; i < hg->nb; ++i) {
        const std::string p = prefix + ".decoder.up_blocks." + std::to_string(i);
        const int c0 = i == 0 ? hg->enc_c[hg->nb - 1] : hg->dec_c[i - 1];
        const int c1 = i == 0 ? 0 : hg->enc_c[hg->nb - 1 - i];
        if ((rc = build_set(c, {{p + ".conv", p + ".norm"}}, c0, c0, c1, c1, &hg->dec[i], MODE_PHASE))) return rc;
    }
    return EAMM_OK;
}

// activations for up to F frames of h x w = hw pixels; *need: raised to the largest split-K slab of any layer
inline int hg_alloc(CtxBase* c, Hourglass* hg, size_t F, size_t hw, size_t* need) {
    int rc;
    hg->e_buf.resize(hg->nb);
    hg->u_buf.resize(hg->nb);
    for (int i = 0; i < hg->nb; ++i) {
        if ((rc = dev_alloc(c, &hg->e_buf[i], F * (hw >> (2 * (i + 1))) * hg->enc_c[i]))) return rc;
        if ((rc = dev_alloc(c, &hg->u_buf[i], F * (hw >> (2 * (hg->nb - 1 - i))) * hg->dec_c[i]))) return rc;
    }
    for (size_t f = 1; f <= F; ++f)
        for (int i = 0; i < hg->nb; ++i)
            *need = std::max({*need, set_partial_elems(hg->enc[i], f * (hw >> (2 * i))),
                              set_partial_elems(hg->dec[i], f * (hw >> (2 * (hg->nb - i))))});
    return EAMM_OK;
}

// The anti-alias buffer (`down.weight`, zero filters for planes an image lacks) and, for one / two channel images, the
// zero-extended three-plane staging buffer the anti-alias kernel reads
inline int hg_build_input(CtxBase* c, int num_channels, int inv_scale, int H, int W, int max_batch, float** aa_w, float** img_stage) {
    int rc;
    std::vector<float> aa((size_t)std::max(3, num_channels) * 169, 0.f);
    if (inv_scale != 1) {
        const HostTensor* t = find(c, "down.weight");
        if (!t || (int)t->numel() != num_channels * 169)
            return fail(c, EAMM_ERR_KEY, "down.weight must be [%d,1,13,13]", num_channels);
        std::copy(t->data.begin(), t->data.end(), aa.begin());   // (the planes an image does not have keep zero filters)
    }
    if ((rc = upload(c, aa_w, aa))) return rc;
    if (num_channels < 3) {   // one / two image channels: the hourglass's first block has filters for those only
        const size_t n = (size_t)max_batch * 3 * H * W;
        if ((rc = dev_alloc(c, img_stage, n))) return rc;
        HIP_TRY(c, hipMemset(*img_stage, 0, n * sizeof(float)));
    }
    return EAMM_OK;
}

// x = down(x): [B,C,H,W] image -> anti-aliased NHWC [B,h,w,Cin_pad], zero-padded channels        keypoint_detector.py:79-80
inline int hg_input(CtxBase* c, const float* image, const float* aa_w, float* img_stage, int B, int C, int H, int W, int inv_scale,
                    int cin_pad, float* x_in, hipStream_t s) {
    if (img_stage) {   // [B,C,H,W] into the first C planes of [B,3,H,W]
        const size_t HW = (size_t)H * W * sizeof(float);
        HIP_TRY(c, hipMemcpy2DAsync(img_stage, 3 * HW, image, (size_t)C * HW, (size_t)C * HW, (size_t)B, hipMemcpyDeviceToDevice, s));
        image = img_stage;
    }
    if (C <= 3) {
        HIP_TRY(c, antialias_down_launch(image, aa_w, B, H, W, inv_scale, cin_pad, x_in, s));
    } else {   // four to eight channels: four per float4 slot, straight from the caller's [B,C,H,W] (real channels stay contiguous)
        for (int g0 = 0, slot = 0; g0 < C; g0 += 4, ++slot)
            HIP_TRY(c, antialias_down_launch(image, aa_w, B, H, W, inv_scale, cin_pad, x_in, s, C, g0, std::min(4, C - g0), slot));
    }
    return EAMM_OK;
}

// encoder + decoder on x_in [B,h,w,*]; the result is hg.u_buf[nb-1]
inline int hg_run(CtxBase* c, const Hourglass& hg, const float* x_in, int B, int h, int w, float* partial, size_t partial_elems,
                  hipStream_t s) {
    for (int i = 0; i < hg.nb; ++i) {   // hourglass encoder                      util.py:956-960
        ConvIO io{};
        io.in0 = i == 0 ? x_in : hg.e_buf[i - 1];
        io.B = B;
        io.Hin = h >> i;
        io.Win = w >> i;
        io.act = ACT_RELU;
        io.pool = 1;
        io.out = hg.e_buf[i];
        io.partial = partial;
        io.partial_cap = partial_elems;
        HIP_TRY(c, conv_launch(pick(c, hg.enc[i], (size_t)B * io.Hin * io.Win), io, s));
    }
    for (int i = 0; i < hg.nb; ++i) {   // hourglass decoder                      util.py:981-987
        ConvIO io{};
        io.in0 = i == 0 ? hg.e_buf[hg.nb - 1] : hg.u_buf[i - 1];
        io.in1 = i == 0 ? nullptr : hg.e_buf[hg.nb - 1 - i];
        io.B = B;
        io.Hin = h >> (hg.nb - i);
        io.Win = w >> (hg.nb - i);
        io.act = ACT_RELU;
        io.out = hg.u_buf[i];
        io.partial = partial;
        io.partial_cap = partial_elems;
        if (int urc = launch_up(c, hg.dec[i], io, s)) return urc;
    }
    return EAMM_OK;
}

}  // namespace
}  // namespace eamm
