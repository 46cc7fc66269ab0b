"""Checkpoint layout of the generator and seeded synthetic weights / inputs.

``state_dict_spec(cfg)`` derives, from the constructor kwargs alone, the exact key set and
shapes that ``generator.load_state_dict(checkpoint['generator'])`` expects in the reference
(reference demo.py:91; key set listed in SURVEY.md section 8b): conv weights are OIHW, every
``norm`` carries ``weight, bias, running_mean, running_var, num_batches_tracked`` and the
dense-motion network owns the ``down.weight`` anti-alias buffer.

No pretrained checkpoint ships with the reference (README.md:21 is a download link), so parity is
pinned with synthetic weights produced by a frozen ``numpy.random.RandomState`` stream: He-scaled
convolutions and non-trivial BatchNorm statistics (PyTorch's default init makes the prediction
almost constant, which would let a broken kernel pass).  The same generator is used in the
container (to drive the imported reference) and on the GPU box, so 182 MB of weights never have to
be committed.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import numpy as np
import torch


# ----------------------------------------------------------------------------------------------
# layout
# ----------------------------------------------------------------------------------------------
def _block(prefix, cin, cout, k, spec, gain):
    spec.append((prefix + ".conv.weight", (cout, cin, k, k), "conv_w", gain))
    spec.append((prefix + ".conv.bias", (cout,), "conv_b", None))
    _norm(prefix + ".norm", cout, spec)


def _norm(prefix, c, spec):
    spec.append((prefix + ".weight", (c,), "bn_w", None))
    spec.append((prefix + ".bias", (c,), "bn_b", None))
    spec.append((prefix + ".running_mean", (c,), "bn_mean", None))
    spec.append((prefix + ".running_var", (c,), "bn_var", None))
    spec.append((prefix + ".num_batches_tracked", (), "nbt", None))


def hourglass_channels(block_expansion, in_features, num_blocks, max_features):
    """(encoder [(cin, cout)], decoder [(cin, cout)], out_filters) -- reference util.py:941-987."""
    enc = []
    for i in range(num_blocks):
        cin = in_features if i == 0 else min(max_features, block_expansion * (2 ** i))
        cout = min(max_features, block_expansion * (2 ** (i + 1)))
        enc.append((cin, cout))
    dec = []
    for i in reversed(range(num_blocks)):
        mult = 1 if i == num_blocks - 1 else 2
        cin = mult * min(max_features, block_expansion * (2 ** (i + 1)))
        cout = min(max_features, block_expansion * (2 ** i))
        dec.append((cin, cout))
    return enc, dec, block_expansion + in_features


def generator_channels(cfg):
    """Encoder / decoder channel plan of the generator (reference generator.py:25-46)."""
    be, mf, nd = cfg["block_expansion"], cfg["max_features"], cfg["num_down_blocks"]
    down = [(min(mf, be * 2 ** i), min(mf, be * 2 ** (i + 1))) for i in range(nd)]
    up = [(min(mf, be * 2 ** (nd - i)), min(mf, be * 2 ** (nd - i - 1))) for i in range(nd)]
    return down, up, min(mf, be * 2 ** nd)


def state_dict_spec(cfg):
    """Ordered [(key, shape, kind, gain)] in the reference's registration order."""
    spec = []
    nc, nk = cfg["num_channels"], cfg["num_kp"]
    dm = cfg.get("dense_motion_params")
    if dm is not None:
        enc, dec, out_filters = hourglass_channels(
            dm["block_expansion"], (nk + 1) * (nc + 1), dm["num_blocks"], dm["max_features"])
        p = "dense_motion_network."
        for i, (ci, co) in enumerate(enc):
            _block(f"{p}hourglass.encoder.down_blocks.{i}", ci, co, 3, spec, 2.0)
        for i, (ci, co) in enumerate(dec):
            _block(f"{p}hourglass.decoder.up_blocks.{i}", ci, co, 3, spec, 2.0)
        spec.append((p + "mask.weight", (nk + 1, out_filters, 7, 7), "conv_w", 4.0))
        spec.append((p + "mask.bias", (nk + 1,), "conv_b", None))
        if cfg.get("estimate_occlusion_map", False):
            spec.append((p + "occlusion.weight", (1, out_filters, 7, 7), "conv_w", 4.0))
            spec.append((p + "occlusion.bias", (1,), "conv_b", None))
        if dm.get("scale_factor", 1) != 1:
            spec.append((p + "down.weight", (nc, 1, 13, 13), "aa", None))
    down, up, bott = generator_channels(cfg)
    _block("first", nc, cfg["block_expansion"], 7, spec, 2.0)
    for i, (ci, co) in enumerate(down):
        _block(f"down_blocks.{i}", ci, co, 3, spec, 2.0)
    for i, (ci, co) in enumerate(up):
        _block(f"up_blocks.{i}", ci, co, 3, spec, 2.0)
    for i in range(cfg["num_bottleneck_blocks"]):
        r = f"bottleneck.r{i}"
        spec.append((r + ".conv1.weight", (bott, bott, 3, 3), "conv_w", 1.0))
        spec.append((r + ".conv1.bias", (bott,), "conv_b", None))
        spec.append((r + ".conv2.weight", (bott, bott, 3, 3), "conv_w", 1.0))
        spec.append((r + ".conv2.bias", (bott,), "conv_b", None))
        _norm(r + ".norm1", bott, spec)
        _norm(r + ".norm2", bott, spec)
    spec.append(("final.weight", (nc, cfg["block_expansion"], 7, 7), "conv_w", 1.0))
    spec.append(("final.bias", (nc,), "conv_b", None))
    return spec


def kp_state_dict_spec(cfg):
    """Checkpoint layout of KPDetector / KPDetector_a (reference keypoint_detector.py:12-37, 115-141): the
    `predictor` hourglass (unused by KPDetector_a.forward but present in its checkpoint), the 7x7 `kp` and
    `jacobian` heads and the anti-alias buffer."""
    spec = []
    in_features = cfg.get("num_channels_a", cfg["num_channels"])
    enc, dec, out_filters = hourglass_channels(cfg["block_expansion"], in_features, cfg["num_blocks"], cfg["max_features"])
    for i, (ci, co) in enumerate(enc):
        _block(f"predictor.encoder.down_blocks.{i}", ci, co, 3, spec, 2.0)
    for i, (ci, co) in enumerate(dec):
        _block(f"predictor.decoder.up_blocks.{i}", ci, co, 3, spec, 2.0)
    k = cfg["num_kp"]
    spec.append(("kp.weight", (k, out_filters, 7, 7), "conv_w", 1.0))
    spec.append(("kp.bias", (k,), "conv_b", None))
    if cfg.get("estimate_jacobian", False):
        njm = 1 if cfg.get("single_jacobian_map", False) else k
        spec.append(("jacobian.weight", (4 * njm, out_filters, 7, 7), "conv_w", 1.0))
        spec.append(("jacobian.bias", (4 * njm,), "conv_b", None))
    if cfg.get("scale_factor", 1) != 1:
        spec.append(("down.weight", (cfg["num_channels"], 1, 13, 13), "aa", None))
    return spec


def emotion_state_dict_spec(cfg):
    """Checkpoint layout of Emotion_k (reference util.py:1223-1318), in its registration order: the `predictor` hourglass, the
    anti-alias buffer, the bias-free 3x3 stem + BatchNorm, layer1..layer4 of BasicBlocks (util.py:1069-1082; a 1x1 `downsample`
    + BatchNorm where the width or the stride changes), then the linear / Conv1d heads -- `fc`, `fc_n`, `final_4`, `final_10`
    included, which forward does not use (223 entries for the demo's arguments)."""
    spec = []
    enc, dec, out_filters = hourglass_channels(cfg["block_expansion"], cfg["num_channels"], cfg["num_blocks"], cfg["max_features"])
    for i, (ci, co) in enumerate(enc):
        _block(f"predictor.encoder.down_blocks.{i}", ci, co, 3, spec, 2.0)
    for i, (ci, co) in enumerate(dec):
        _block(f"predictor.decoder.up_blocks.{i}", ci, co, 3, spec, 2.0)
    if cfg.get("scale_factor", 1) != 1:
        spec.append(("down.weight", (cfg["num_channels"], 1, 13, 13), "aa", None))
    spec.append(("conv1.weight", (64, out_filters, 3, 3), "conv_w", 2.0))
    _norm("bn1", 64, spec)
    cin = 64
    for li, planes in enumerate((64, 128, 256, 512)):
        for bi in range(2):
            p = f"layer{li + 1}.{bi}"
            ci = cin if bi == 0 else planes
            spec.append((p + ".conv1.weight", (planes, ci, 3, 3), "conv_w", 2.0))
            _norm(p + ".bn1", planes, spec)
            spec.append((p + ".conv2.weight", (planes, planes, 3, 3), "conv_w", 1.0))
            _norm(p + ".bn2", planes, spec)
            if bi == 0 and li > 0:
                spec.append((p + ".downsample.0.weight", (planes, ci, 1, 1), "conv_w", 1.0))
                _norm(p + ".downsample.1", planes, spec)
        cin = planes

    def lin(name, shape, gain=2.0):
        spec.append((name + ".weight", shape, "fc_w", gain))
        spec.append((name + ".bias", (shape[0],), "conv_b", None))
    lin("fc", (cfg.get("num_classes", 8), 512), 1.0)
    lin("fc_p.0", (1024, 1260))
    lin("fc_p.2", (512, 1024))
    lin("fc_n.0", (128, 60))
    lin("fc_n.2", (512, 128))
    lin("fc_all.0", (512, 1024))
    lin("fc_all.2", (256, 512))
    lin("fc_all.4", (64, 256))
    lin("final.0", (2, 1, 4))
    lin("final.3", (4, 2, 4))
    lin("final.5", (4, 4, 3), 1.0)
    lin("final_4.0", (4, 4, 3))
    lin("final_4.3", (4, 4, 3), 1.0)
    lin("final_10.0", (8, 4, 3))
    lin("final_10.3", (10, 8, 3), 1.0)
    lin("classify.last_fc", (8, 512), 1.0)
    return spec


DECONV_CHANNELS = (256, 256, 128, 128, 128, 35)   # AT_net2.decon, reference util.py:559-574


def deconv_state_dict_spec(channels=DECONV_CHANNELS):
    """Checkpoint layout of the nn.Sequential `AT_net2.decon` (reference util.py:559-576): ConvTranspose2d at index
    3i ([Cin,Cout,k,k], k = 6 for the first layer, 4 after), BatchNorm2d at 3i+1 for every layer but the last."""
    spec = []
    n = len(channels) - 1
    for i in range(n):
        k = 6 if i == 0 else 4
        # "conv_w" draws with fan_in = shape[1]*k*k; a stride-2 transposed conv sums k*k/4 taps of shape[0] inputs
        spec.append((f"{3 * i}.weight", (channels[i], channels[i + 1], k, k), "convT_w", 2.0))
        spec.append((f"{3 * i}.bias", (channels[i + 1],), "conv_b", None))
        if i + 1 < n:
            _norm(f"{3 * i + 1}", channels[i + 1], spec)
    return spec


def antialias_kernel(channels: int, sigma: float = 1.5) -> torch.Tensor:
    """The fixed 13x13 Gaussian buffer of the anti-alias down-sampler.

    Reference util.py:1009-1035: sigma is hard-coded to 1.5 regardless of the scale, the window is
    2*round(4*sigma)+1 = 13 taps, normalised to sum 1, replicated per channel as a depthwise weight.
    """
    size = 2 * round(sigma * 4) + 1
    ax = torch.arange(size, dtype=torch.float32)
    mean = (size - 1) / 2
    g = torch.exp(-(ax - mean) ** 2 / (2 * sigma ** 2))
    k2 = g[:, None] * g[None, :]
    k2 = k2 / torch.sum(k2)
    return k2.view(1, 1, size, size).repeat(channels, 1, 1, 1).contiguous()


# ----------------------------------------------------------------------------------------------
# seeded synthetic weights and inputs (frozen RandomState stream)
# ----------------------------------------------------------------------------------------------
def synthetic_state_dict(cfg, seed: int = 1234, spec=None) -> "OrderedDict[str, torch.Tensor]":
    rs = np.random.RandomState(seed)
    sd = OrderedDict()
    for key, shape, kind, gain in (state_dict_spec(cfg) if spec is None else spec):
        if kind == "conv_w":
            fan_in = shape[1] * shape[2] * shape[3]
            v = rs.standard_normal(shape) * math.sqrt(gain / fan_in)
        elif kind == "fc_w":        # nn.Linear [O,K] / nn.Conv1d [O,C,k]
            fan_in = int(np.prod(shape[1:]))
            v = rs.standard_normal(shape) * math.sqrt(gain / fan_in)
        elif kind == "convT_w":
            fan_in = shape[0] * shape[2] * shape[3] / 4.0
            v = rs.standard_normal(shape) * math.sqrt(gain / fan_in)
        elif kind == "conv_b":
            v = 0.1 * rs.standard_normal(shape)
        elif kind == "bn_w":
            v = rs.uniform(0.75, 1.25, shape)
        elif kind in ("bn_b", "bn_mean"):
            v = 0.1 * rs.standard_normal(shape)
        elif kind == "bn_var":
            v = rs.uniform(0.75, 1.25, shape)
        elif kind == "nbt":
            sd[key] = torch.tensor(1000, dtype=torch.int64)
            continue
        elif kind == "aa":
            sd[key] = antialias_kernel(shape[0])
            continue
        elif kind == "lstm":       # U(-1/4, 1/4): 4x nn.LSTM's default bound 1/sqrt(256), whose three stacked layers shrink
            v = rs.uniform(-0.25, 0.25, shape)   # lstm_out to std 0.04; here std ~0.25 and no |h| > 0.99 (the fixtures record both)
        elif kind == "style_w":    # StyleGAN2 entries (unused by the 'cnn' branch): any finite values
            v = rs.standard_normal(shape)
        elif kind == "zero":
            v = np.zeros(shape)
        elif kind == "buf":
            v = np.full(shape, 1.0 / np.prod(shape))
        else:  # pragma: no cover
            raise ValueError(kind)
        sd[key] = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return sd


def adversarial_state_dict(cfg, seed: int = 1234, bn_stats=None) -> "OrderedDict[str, torch.Tensor]":
    """Seeded synthetic generator weights with the statistics of a badly conditioned TRAINED checkpoint (VERDICT r04 item 6;
    the benign `synthetic_state_dict` keeps BatchNorm variance and gain in [0.75, 1.25]):
      * every convolution in front of a BatchNorm has per-output-channel scales 10^U(-2, 0.5) (pre-normalisation standard
        deviations 0.01 .. 3.2, variances 1e-4 .. 10) and twice the He gain in the weights (a gain of 4 in variance);
      * 3 % of those channels are DEAD: weights x 1e-3 with the bias kept, i.e. a constant plus a fluctuation a thousand times
        smaller, which BatchNorm then amplifies by gamma / sqrt(var + eps) ~ 100 .. 300 (reference batchnorm.py:48-53);
      * BatchNorm gains 10^U(-0.6, 0.6) = 0.25 .. 4, one in ten negative; shifts 0.3 N(0, 1).
    The running statistics cannot be drawn at random -- activations would explode or vanish through 30 layers; a trained
    network's statistics are those of its own activations -- so they come from ``bn_stats`` ({norm prefix: (mean, var)}):
    the fixture generator (make_golden.py) calibrates them with one batch-statistics pass of the reference-equivalent forward on the fixture's
    inputs, perturbs the variances by 10^U(-0.3, 0.3) and stores them IN the fixture (a few hundred kB), so that the GPU box
    rebuilds exactly these weights from the seed + the fixture.  Without ``bn_stats``: mean 0, variance 1 (calibration input)."""
    sd = synthetic_state_dict(cfg, seed=seed)
    rs = np.random.RandomState(seed + 4242)
    pairs = []   # (convolution prefix, norm prefix)
    for key in sd:
        if key.endswith(".conv.weight"):
            pairs.append((key[:-len(".weight")], key[:-len(".conv.weight")] + ".norm"))
        elif key.endswith(".conv1.weight"):
            pairs.append((key[:-len(".weight")], key[:-len(".conv1.weight")] + ".norm2"))
    for conv, norm in pairs:
        w, b = sd[conv + ".weight"], sd[conv + ".bias"]
        co = w.shape[0]
        scale = 10.0 ** rs.uniform(-2.0, 0.5, co)
        dead = rs.uniform(size=co) < 0.03
        wscale = np.where(dead, 1e-3, 2.0 * scale).astype(np.float32)
        sd[conv + ".weight"] = w * torch.from_numpy(wscale)[:, None, None, None]
        sd[conv + ".bias"] = b * torch.from_numpy(np.where(dead, 1.0, scale).astype(np.float32))
    for key in list(sd):
        if key.endswith(".running_var"):
            norm = key[:-len(".running_var")]
            c = sd[key].numel()
            gamma = 10.0 ** rs.uniform(-0.6, 0.6, c) * np.where(rs.uniform(size=c) < 0.1, -1.0, 1.0)
            sd[norm + ".weight"] = torch.from_numpy(gamma.astype(np.float32))
            sd[norm + ".bias"] = torch.from_numpy((0.3 * rs.standard_normal(c)).astype(np.float32))
            if bn_stats is None:
                sd[norm + ".running_mean"] = torch.zeros(c)
                sd[norm + ".running_var"] = torch.ones(c)
            else:
                mean, var = bn_stats[norm]
                sd[norm + ".running_mean"] = torch.as_tensor(mean, dtype=torch.float32).clone()
                sd[norm + ".running_var"] = torch.as_tensor(var, dtype=torch.float32).clone()
    return sd


def adversarial_inputs(size: int, frames: int, num_kp: int = 10, channels: int = 3):
    """Inputs for the adversarial fixtures: a SATURATED source (every pixel exactly 0 or 1) and key points on or just inside the
    frame border (|coordinate| in [0.9, 1.0]; a few at exactly +-1), jacobians I + 0.3 N(0,1)."""
    rs = np.random.RandomState(77)
    src = torch.from_numpy((rs.uniform(size=(1, channels, size, size)) > 0.5).astype(np.float32))

    def kps(n, seed):
        r = np.random.RandomState(seed)
        v = r.uniform(0.9, 1.0, (n, num_kp, 2)) * np.where(r.uniform(size=(n, num_kp, 2)) < 0.5, -1.0, 1.0)
        v[:, 0] = np.sign(v[:, 0])                       # key point 0 sits exactly in a corner
        v[:, 1:4] *= r.uniform(0.0, 1.0, (n, 3, 2))      # a few stay inside, or nothing of the source would be sampled
        j = np.eye(2)[None, None] + 0.3 * r.standard_normal((n, num_kp, 2, 2))
        return {"value": torch.from_numpy(v.astype(np.float32)), "jacobian": torch.from_numpy(j.astype(np.float32))}
    return src, kps(1, 300), kps(frames, 301)


def trained_like_kp_state_dict(cfg, seed: int) -> "OrderedDict[str, torch.Tensor]":
    """Synthetic key-point-detector weights with the jacobian head near its trained shape: the reference initialises that head to
    zero weights and an identity bias (modules/keypoint_detector.py:27-28) and training keeps the jacobians near I; He-scaled
    random weights instead give jacobians with |det| ~ 0.01, whose inverse (normalize_kp, demo.py:128; dense_motion.py:56)
    amplifies every rounding difference a hundredfold -- fine for a detector's own parity test, useless for a chain through the
    generator.  Here: the seeded random head scaled by 0.05 plus bias = identity + 0.05 N(0,1)."""
    sd = synthetic_state_dict(cfg, seed=seed, spec=kp_state_dict_spec(cfg))
    if "jacobian.weight" in sd:
        rs = np.random.RandomState(seed + 1000)
        n = sd["jacobian.bias"].numel() // 4
        sd["jacobian.weight"] = sd["jacobian.weight"] * 0.05
        sd["jacobian.bias"] = torch.from_numpy((np.tile([1.0, 0.0, 0.0, 1.0], n) + 0.05 * rs.standard_normal(4 * n)).astype(np.float32))
    return sd


def synthetic_lstm_features(frames: int, channels: int = 256, seed: int = 5) -> torch.Tensor:
    """[T,C] stand-in for the audio network's LSTM output (AT_net2, util.py:600-607): a random pose plus a slow random walk,
    so that consecutive frames' key points move like a talking head's (the One-Euro filter then has something to smooth)."""
    rs = np.random.RandomState(seed)
    base = 0.3 * rs.standard_normal((1, channels))
    walk = 0.05 * np.cumsum(rs.standard_normal((frames, channels)), axis=0)
    return torch.from_numpy((base + walk).astype(np.float32))


def synthetic_source(size: int, seed: int = 1, batch: int = 1, channels: int = 3) -> torch.Tensor:
    """uniform[0,1) RGB source, float32 [batch,3,size,size]; ``channels``: grey-scale / two-channel variants."""
    rs = np.random.RandomState(seed)
    return torch.from_numpy(rs.uniform(0.0, 1.0, (batch, channels, size, size)).astype(np.float32))


def synthetic_keypoints(n: int, num_kp: int = 10, seed: int = 0, jacobian: bool = True) -> dict:
    """n keypoint sets: value ~ U[-0.8, 0.8], jacobian = I + 0.1 N(0,1) (well conditioned).

    Frame t of a clip uses seed 2+t, the source keypoints seed 0; each
    frame draws from its own stream so that a shard of a clip is reproducible in isolation.
    """
    vals, jacs = [], []
    for i in range(n):
        rs = np.random.RandomState(seed + i)
        vals.append(rs.uniform(-0.8, 0.8, (num_kp, 2)))
        jacs.append(np.eye(2)[None] + 0.1 * rs.standard_normal((num_kp, 2, 2)))
    kp = {"value": torch.from_numpy(np.stack(vals).astype(np.float32))}
    if jacobian:
        kp["jacobian"] = torch.from_numpy(np.stack(jacs).astype(np.float32))
    return kp


def _stylegan2_spec(prefix, size=64, style_dim=256, n_mlp=8, out_channels=35):
    """Key layout of the StyleGAN2 `Generator(64, 256, 8)` that AT_net2 holds as `generator` (its jaco_net='gan' branch, unused
    by the demo's 'cnn' configuration): names, shapes and which entries are buffers ("buf": the blur / up-sampling kernels and
    the fixed noises).  Held only so that a strict load of the reference's checkpoint works."""
    spec = []

    def lin(name, o, i):
        spec.append((f"{prefix}.{name}.weight", (o, i), "fc_w", 1.0))
        spec.append((f"{prefix}.{name}.bias", (o,), "conv_b", None))

    def styled(name, cin, cout, k, up=False, noise=True):
        spec.append((f"{prefix}.{name}.conv.weight", (1, cout, cin, k, k), "style_w", None))
        if up:
            spec.append((f"{prefix}.{name}.conv.blur.kernel", (4, 4), "buf", None))
        lin(f"{name}.conv.modulation", cin, style_dim)
        if noise:
            spec.append((f"{prefix}.{name}.noise.weight", (1,), "zero", None))
            spec.append((f"{prefix}.{name}.activate.bias", (1, cout, 1, 1), "zero", None))

    def to_rgb(name, cin, up):
        spec.append((f"{prefix}.{name}.bias", (1, out_channels, 1, 1), "zero", None))
        if up:
            spec.append((f"{prefix}.{name}.upsample.kernel", (4, 4), "buf", None))
        styled(name, cin, out_channels, 1, noise=False)

    for i in range(1, n_mlp + 1):
        lin(f"style.{i}", style_dim, style_dim)
    ch = {4: 256, 8: 256, 16: 128, 32: 64, 64: 32}
    spec.append((f"{prefix}.input.input", (1, ch[4], 4, 4), "style_w", None))
    styled("conv1", ch[4], ch[4], 3)
    to_rgb("to_rgb1", ch[4], False)
    log_size = int(math.log2(size))
    cin, j = ch[4], 0
    for i in range(3, log_size + 1):
        cout = ch[2 ** i]
        styled(f"convs.{j}", cin, cout, 3, up=True)
        styled(f"convs.{j + 1}", cout, cout, 3)
        j += 2
        cin = cout
    for i in range(3, log_size + 1):
        to_rgb(f"to_rgbs.{i - 3}", ch[2 ** i], True)
    for k in range((log_size - 2) * 2 + 1):
        side = 2 ** ((k + 5) // 2)
        spec.append((f"{prefix}.noises.noise_{k}", (1, 1, side, side), "buf", None))
    return spec


AUDIO_DOWN_CHANNELS = (3, 4, 8, 16, 32, 64, 128, 256, 512)   # AT_net2.down_blocks, reference util.py:518-523


def audio_feature_state_dict_spec():
    """Checkpoint layout of AT_net2 (reference util.py:514-582), in its registration order: the image encoder's eight DownBlock2d,
    `pose_encoder`, `audio_eocder` (conv2d = bias-free conv + BatchNorm + ReLU, at Sequential indices 0, 1, 3, 4, 5),
    `audio_eocder_fc`, the three-layer `lstm`, `decon` and the unused StyleGAN2 `generator` -- 235 entries.  The LSTM draws
    U(+-1/4) ("lstm"), which keeps its gates away from both saturation and zero."""
    spec = []
    for i in range(8):
        _block(f"down_blocks.{i}", AUDIO_DOWN_CHANNELS[i], AUDIO_DOWN_CHANNELS[i + 1], 3, spec, 2.0)

    def lin(name, o, i, gain=2.0):
        spec.append((name + ".weight", (o, i), "fc_w", gain))
        spec.append((name + ".bias", (o,), "conv_b", None))
    lin("pose_encoder.0", 128, 6)
    lin("pose_encoder.2", 256, 128)
    for idx, (ci, co) in zip((0, 1, 3, 4, 5), ((1, 64), (64, 128), (128, 256), (256, 256), (256, 512))):
        spec.append((f"audio_eocder.{idx}.0.weight", (co, ci, 3, 3), "conv_w", 2.0))
        _norm(f"audio_eocder.{idx}.1", co, spec)
    lin("audio_eocder_fc.0", 2048, 12288)
    lin("audio_eocder_fc.2", 256, 2048)
    for layer in range(3):
        spec.append((f"lstm.weight_ih_l{layer}", (1024, 1024 if layer == 0 else 256), "lstm", None))
        spec.append((f"lstm.weight_hh_l{layer}", (1024, 256), "lstm", None))
        spec.append((f"lstm.bias_ih_l{layer}", (1024,), "lstm", None))
        spec.append((f"lstm.bias_hh_l{layer}", (1024,), "lstm", None))
    spec += [("decon." + k, s, kind, g) for k, s, kind, g in deconv_state_dict_spec()]
    spec += _stylegan2_spec("generator")
    return spec


def synthetic_audio_inputs(clips: int, steps: int, seed: int = 21, size: int = 256):
    """AT_net2.forward's inputs for `clips` clips of `steps` steps: example_image [N,3,size,size] uniform [0,1), audio [N,T,28,12]
    (MFCC windows, demo.py:326-332: coefficients 1..12 of 28 rows; N(0, 4^2) like real MFCCs' spread) and pose [N,T,6]
    (demo.py:297; small rotations and translations, U(-0.3, 0.3))."""
    rs = np.random.RandomState(seed)
    image = rs.uniform(0.0, 1.0, (clips, 3, size, size))
    audio = 4.0 * rs.standard_normal((clips, steps, 28, 12))
    pose = rs.uniform(-0.3, 0.3, (clips, steps, 6))
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    return f32(image), f32(audio), f32(pose)
