"""Drop-in ``AT_net2`` (reference modules/util.py:514-612) whose forward pass runs in libeamm_hip.so.

The reference's ``test_auido`` (demo.py:286-354) calls ``audio_feature(example_image, input_mfcc, pose, 'cnn', 1.6)``: the image
encoder, then per time step (batch 1) the audio CNN, ``audio_eocder_fc`` and the pose MLP, one sequential three-layer
``nn.LSTM``, and ``decon`` per step.  Here one ``eamm_audio_lstm_features`` call computes ``lstm_out`` for whole clips: the image
encoder once per clip, the per-step encoders batched over ``max_batch`` frames, and each LSTM layer's recurrence as one persistent
launch.  ``decon`` is the existing ``DeconvTail`` (so ``animate_from_features(..., deconv_tail=net.decon)`` keeps working).  Same
``state_dict`` keys as the reference (its 235 entries, the 99 of the unused StyleGAN2 ``generator`` included, held only so that a
strict load works).  The sub-modules only hold parameters; there is no PyTorch fallback.

Training.  ``AT_net2`` is what the reference's first stage trains together with ``KPDetector_a`` (train.py ``train_part1``, an L1
distance between the audio-driven and the image-driven key points, modules/model.py:187-221).  The parameters are frozen at
construction and a frozen network runs the graph-free engine whatever ``.training`` says (a fresh ``nn.Module`` is in training
mode); ``mod.requires_grad_(True)`` opts in.  ``forward`` and ``lstm_features`` then take the GRAPH ROUTE when the module is in
``.train()``, or gradients are enabled and an input or a parameter requires one: util.py:580-614 as a composition of differentiable
HIP operators -- ``train_graph._Graph.down_block`` eight times; per step ``train_graph.conv`` + ``_Graph.norm`` (plain
``nn.BatchNorm2d``) + ``audio_ops.maxpool3_nhwc``; three ``audio_ops.lstm_layer`` (persistent forward and backward recurrences);
``DeconvTail``'s graph route -- with the linear layers, the ``* weight`` scale and the LSTM's input projections as torch-ROCm ops
with their own autograd.  In ``.train()`` every BatchNorm of ``audio_eocder`` and ``decon`` takes its batch statistics over the N
clips of ONE step and updates its running statistics T times in step order, as the reference's per-step calls do (the
convolutions are batched over N x T); in ``.eval()`` every BatchNorm uses its running statistics.  Under ``torch.no_grad()`` in
``.train()`` the route is the same composition without a graph.  ``state=`` (chunked clips) is an inference feature: with the graph
route it raises ``ValueError`` (no truncated back-propagation through time).  The op-level composition, not a tuned path.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib
from ._handle import HandleOwner, ptr, refuse_silent_detach, stream_ptr, weights_key
from .deconv_tail import DeconvTail
from .weights import AUDIO_DOWN_CHANNELS, _stylegan2_spec

MAX_CLIPS = 8
HIDDEN = 256
IMAGE_SIZE = 256
MFCC_SHAPE = (28, 12)     # demo.py:326-332: 28 rows of coefficients 1..12; audio_eocder_fc takes 512 x 12 x 2 = 12288 inputs
POSE_DIM = 6


class _DownBlock(nn.Module):
    """Parameter holder named like DownBlock2d (util.py:903-921)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, 3, padding=1)
        self.norm = nn.BatchNorm2d(cout)


def _conv2d_block(cin, cout):
    """util.py:1740-1753 ``conv2d``: bias-free 3x3 convolution, BatchNorm2d, ReLU."""
    return nn.Sequential(nn.Conv2d(cin, cout, 3, 1, 1, bias=False), nn.BatchNorm2d(cout), nn.ReLU(True))


def _holder(prefix: str, spec) -> nn.Module:
    """A module tree that only holds the entries ``spec`` lists (names relative to ``prefix``), registered in that order."""
    root = nn.Module()
    for key, shape, kind, _ in spec:
        path = key[len(prefix) + 1:].split(".")
        m = root
        for part in path[:-1]:
            if part not in m._modules:
                m.add_module(part, nn.Module())
            m = m._modules[part]
        t = torch.zeros(shape)
        if kind == "buf":
            m.register_buffer(path[-1], t)
        else:
            m.register_parameter(path[-1], nn.Parameter(t, requires_grad=False))
    return root


class AudioFeatureNet(HandleOwner, nn.Module):
    """reference util.py:514 ``AT_net2`` (forward = util.py:578-612), ``jaco_net='cnn'``; trainable after ``requires_grad_(True)``."""
    _prefix = "eamm_audio_"

    def __init__(self, max_batch: int = 256):
        super().__init__()
        ch = AUDIO_DOWN_CHANNELS
        self.down_blocks = nn.ModuleList([_DownBlock(ch[i], ch[i + 1]) for i in range(8)])
        self.pose_encoder = nn.Sequential(nn.Linear(6, 128), nn.ReLU(True), nn.Linear(128, 256), nn.ReLU(True))
        self.audio_eocder = nn.Sequential(_conv2d_block(1, 64), _conv2d_block(64, 128), nn.MaxPool2d(3, stride=(1, 2)),
                                          _conv2d_block(128, 256), _conv2d_block(256, 256), _conv2d_block(256, 512),
                                          nn.MaxPool2d(3, stride=(2, 2)))
        self.audio_eocder_fc = nn.Sequential(nn.Linear(1024 * 12, 2048), nn.ReLU(True), nn.Linear(2048, 256), nn.ReLU(True))
        self.lstm = nn.LSTM(256 * 4, 256, 3, batch_first=True)
        self.decon = DeconvTail()
        self.generator = _holder("generator", _stylegan2_spec("generator"))
        if not 8 <= int(max_batch) <= 4096:
            raise ValueError(f"AudioFeatureNet: max_batch must be 8 .. 4096 (got {max_batch})")
        self.max_batch = int(max_batch)
        # what train_graph._Graph reads for the image encoder's BatchNorms (as KPDetector: None = one process's statistics)
        self.process_group = None
        self.sync_batchnorm: Optional[bool] = None
        for p in self.parameters():          # frozen: training is opted into with mod.requires_grad_(True)
            p.requires_grad_(False)

    # -- handle management ----------------------------------------------------------------------------------
    def _keyed_tensors(self, dev):
        """The entries the library reads -- all but the unused StyleGAN2 ``generator`` and ``decon`` (a ``DeconvTail`` with its own
        handle) -- and the handle's key over them."""
        named = [(name, t) for name, t in self.state_dict(keep_vars=True).items() if not name.startswith(("generator.", "decon."))]
        return (dev, weights_key(t for _, t in named), self.max_batch), named

    def _ensure(self):
        dev = self._inference_device(self.lstm.weight_hh_l0)
        key, named = self._keyed_tensors(dev)
        if self._has_handle(key):
            return
        cs = _lib.EammAudioConfig()
        cs.max_batch = self.max_batch
        self._rebuild_handle(key, self.max_batch, cs, dev, named)

    # -- forward ----------------------------------------------------------------------------------------------
    @staticmethod
    def check_inputs(example_image, audio, pose):
        """Refuses, by name, every input the reference's layers would not accept (and clip counts beyond 8)."""
        if not torch.is_tensor(example_image) or example_image.dim() != 4 or tuple(example_image.shape[1:]) != (3, IMAGE_SIZE, IMAGE_SIZE):
            raise ValueError(f"AudioFeatureNet: example_image must be [N,3,{IMAGE_SIZE},{IMAGE_SIZE}] (eight DownBlock2d down to "
                             f"512x1x1), got {tuple(getattr(example_image, 'shape', ()))}")
        n = example_image.shape[0]
        if not 1 <= n <= MAX_CLIPS:
            raise ValueError(f"AudioFeatureNet: 1 to {MAX_CLIPS} clips per call, got N = {n}")
        if not torch.is_tensor(audio) or audio.dim() != 4 or tuple(audio.shape[2:]) != MFCC_SHAPE or audio.shape[0] != n:
            raise ValueError(f"AudioFeatureNet: audio must be [N,T,28,12] MFCC windows with N = {n} (audio_eocder_fc takes "
                             f"512 x 12 x 2 = 12288 inputs), got {tuple(getattr(audio, 'shape', ()))}")
        t = audio.shape[1]
        if t < 1:
            raise ValueError("AudioFeatureNet: audio has no time steps (T = 0)")
        if not torch.is_tensor(pose) or pose.dim() != 3 or tuple(pose.shape) != (n, t, POSE_DIM):
            raise ValueError(f"AudioFeatureNet: pose must be [N,T,6] = [{n},{t},6], got {tuple(getattr(pose, 'shape', ()))}")
        return n, t

    def lstm_features(self, example_image: torch.Tensor, audio: torch.Tensor, pose: torch.Tensor, weight: float = 1.6,
                      state: Optional[Dict[str, torch.Tensor]] = None) -> torch.Tensor:
        """util.py:578-598 up to the LSTM -> ``lstm_out`` [N,T,256] (what ``animate_from_features`` consumes).

        ``state`` (optional dict): ``'h'`` / ``'c'`` [3,N,256] start the recurrence instead of zeros when present, and are
        replaced by the state after the last step; ``'clip'`` [N,1024] holds the image's share of the layer-0 gates, computed by
        the first call with that dict (the image encoder runs once per clip; later calls ignore ``example_image``'s values).  A
        clip computed in consecutive chunks with one dict is bit-identical to one call over the whole clip.

        The call does not wait for the device.  A recurrence that timed out (a workgroup waited longer than the limit for
        another) is reported by ``check()``, which ``forward`` and ``animate_from_features`` call at their end."""
        if self._wants_graph(example_image, audio, pose):
            n, t = self.check_inputs(example_image, audio, pose)
            if state is not None:
                raise ValueError("AudioFeatureNet: state= (chunked clips) is an inference feature; the differentiable route has no "
                                 "truncated back-propagation through time")
            return self._lstm_features_graph(example_image, audio, pose, weight)
        refuse_silent_detach(self, example_image)
        n, t = self.check_inputs(example_image, audio, pose)
        self._ensure()
        dev = self.lstm.weight_hh_l0.device
        f32 = lambda x: x.to(dev, torch.float32).contiguous()
        img, aud, pos = f32(example_image), f32(audio), f32(pose)
        out = torch.empty(n, t, HIDDEN, device=dev)
        h0 = c0 = None
        if state is not None and "h" in state:
            h0, c0 = f32(state["h"]), f32(state["c"])
            if tuple(h0.shape) != (3, n, HIDDEN) or tuple(c0.shape) != (3, n, HIDDEN):
                raise ValueError(f"AudioFeatureNet: state h / c must be [3,{n},256], got {tuple(h0.shape)} / {tuple(c0.shape)}")
        clip = img_arg = None
        if state is not None and "clip" in state:
            clip = state["clip"]
            if tuple(clip.shape) != (n, 4 * HIDDEN) or clip.device != dev:
                raise ValueError(f"AudioFeatureNet: state['clip'] must be [{n},1024] on {dev}, got {tuple(clip.shape)}")
        else:
            img_arg = img
            if state is not None:
                clip = torch.empty(n, 4 * HIDDEN, device=dev)
        h1 = torch.empty(3, n, HIDDEN, device=dev) if state is not None else None
        c1 = torch.empty(3, n, HIDDEN, device=dev) if state is not None else None
        with torch.no_grad():
            self._handle.call("lstm_features", ptr(img_arg), ptr(aud), ptr(pos), n, t, float(weight), ptr(h0), ptr(c0), ptr(h1), ptr(c1),
                              ptr(clip), ptr(out), stream_ptr(dev))
        if state is not None:
            state["h"], state["c"], state["clip"] = h1, c1, clip
        return out

    def _wants_graph(self, *inputs) -> bool:
        """Opted in (``requires_grad_(True)``: a parameter requires a gradient) and either in ``.train()`` or with gradients enabled
        (the parameter requires one).  A frozen network never takes the graph route, whatever ``.training`` says."""
        return any(p.requires_grad for p in self.parameters()) and (self.training or torch.is_grad_enabled())

    def _lstm_features_graph(self, example_image, audio, pose, weight) -> torch.Tensor:
        """util.py:580-598 as a composition of differentiable operators (NHWC between the convolutions) -> ``lstm_out`` [N,T,256]."""
        from . import audio_ops, train_graph
        dev = self.lstm.weight_hh_l0.device
        if dev.type != "cuda":
            raise RuntimeError("eamm_amd.AudioFeatureNet runs only on a ROCm GPU (no CPU fallback): call .cuda()")
        n, t = audio.shape[:2]
        f32 = lambda x: x.to(dev, torch.float32)
        g = train_graph._Graph(self)
        out = f32(example_image).permute(0, 2, 3, 1)                                    # util.py:583-587
        for blk in self.down_blocks:
            out = g.down_block(out, blk)
        image_feature = out.reshape(n, -1)                                               # [N,512] (1x1 map)
        # the per-step encoders on a TIME-MAJOR batch (row s * N + clip): the convolutions see all N * T frames at once; in
        # .train() each BatchNorm call sees the N clips of one step, in step order (util.py:589-591 runs audio_eocder per step)
        per_step = g.training and t > 1

        def norm(y, holder):
            if not per_step:
                return g.norm(y, holder, relu=True)
            return torch.cat([g.norm(y[s * n:(s + 1) * n], holder, relu=True) for s in range(t)], dim=0)

        a = f32(audio).transpose(0, 1).reshape(t * n, MFCC_SHAPE[0], MFCC_SHAPE[1], 1)
        for idx in range(7):
            layer = self.audio_eocder[idx]
            if isinstance(layer, nn.MaxPool2d):
                a = audio_ops.maxpool3_nhwc(a, *layer.stride)
            else:
                a = norm(train_graph.conv(a, layer[0], feeds_norm=g.training), layer[1])
        a = a.permute(0, 3, 1, 2).reshape(t * n, -1)                                     # the reference flattens NCHW [512,12,2]
        for i in (0, 2):
            a = torch.relu(F.linear(a, self.audio_eocder_fc[i].weight, self.audio_eocder_fc[i].bias))
        a = a * float(weight)                                                            # util.py:593
        pf = f32(pose).transpose(0, 1).reshape(t * n, POSE_DIM)
        for i in (0, 2):
            pf = torch.relu(F.linear(pf, self.pose_encoder[i].weight, self.pose_encoder[i].bias))
        x = torch.cat([image_feature[None].expand(t, n, image_feature.shape[1]), a.view(t, n, -1), pf.view(t, n, -1)], dim=2)
        x = x.transpose(0, 1)                                                            # [N,T,1024]: batch_first
        for l in range(3):                                                               # util.py:598, from the zero state
            w_ih, w_hh = getattr(self.lstm, f"weight_ih_l{l}"), getattr(self.lstm, f"weight_hh_l{l}")
            bias = getattr(self.lstm, f"bias_ih_l{l}") + getattr(self.lstm, f"bias_hh_l{l}")
            x = audio_ops.lstm_layer(F.linear(x, w_ih, bias), w_hh)
        return x

    def check(self):
        """Waits for the current stream and raises ``EammError`` if a recurrence of this module timed out (its results are then
        invalid, and so is every later call) -- the engine's, or an ``audio_ops.lstm_layer`` of the graph route."""
        if self._handle is not None and self._handle.ptr is not None:
            self._handle.call("check", stream_ptr(self._handle.device))
        dev = self.lstm.weight_hh_l0.device
        if dev.type == "cuda":
            from . import audio_ops
            audio_ops.lstm_check(dev)

    def forward(self, example_image: torch.Tensor, audio: torch.Tensor, pose: torch.Tensor, jaco_net: str, weight: float) -> torch.Tensor:
        """util.py:578-612 -> ``deco_out`` [N,T,35,64,64]."""
        if jaco_net == "gan":
            raise NotImplementedError("AudioFeatureNet: the StyleGAN2 branch (jaco_net='gan', AT_net2.generator) is not implemented; "
                                      "its weights are held only for a strict state_dict load")
        if jaco_net != "cnn":
            raise Exception("jaco_net type wrong")   # the reference's own error (util.py:610)
        lstm_out = self.lstm_features(example_image, audio, pose, weight)
        n, t = lstm_out.shape[:2]
        if self._wants_graph(example_image, audio, pose):
            # decon per step (util.py:601-607): time-major rows, so that a .train() BatchNorm call sees one step's N clips
            deco = self.decon._forward_graph(lstm_out.transpose(0, 1).reshape(t * n, HIDDEN), steps=t)
            self.check()
            return deco.view(t, n, *deco.shape[1:]).transpose(0, 1)
        deco = self.decon(lstm_out.reshape(n * t, HIDDEN))
        self.check()
        return deco.view(n, t, *deco.shape[1:])
