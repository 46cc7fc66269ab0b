"""Drop-in ``AT_net2`` (reference modules/util.py:514-612) whose forward pass runs in libeamm_hip.so.

The reference's ``test_auido`` (demo.py:286-354) calls ``audio_feature(example_image, input_mfcc, pose, 'cnn', 1.6)``: the image
encoder, then per time step (batch 1) the audio CNN, ``audio_eocder_fc`` and the pose MLP, one sequential three-layer
``nn.LSTM``, and ``decon`` per step.  Here one ``eamm_audio_lstm_features`` call computes ``lstm_out`` for whole clips: the image
encoder once per clip, the per-step encoders batched over ``max_batch`` frames, and each LSTM layer's recurrence as one persistent
launch.  ``decon`` is the existing ``DeconvTail`` (so ``animate_from_features(..., deconv_tail=net.decon)`` keeps working).  Same
``state_dict`` keys as the reference (its 235 entries, the 99 of the unused StyleGAN2 ``generator`` included, held only so that a
strict load works).  The sub-modules only hold parameters; there is no PyTorch fallback.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
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
    """reference util.py:514 ``AT_net2`` (forward = util.py:578-612), inference only, ``jaco_net='cnn'``."""
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
        for p in self.parameters():
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

    def check(self):
        """Waits for the current stream and raises ``EammError`` if a recurrence of this module timed out (its results are then
        invalid, and so is every later call)."""
        if self._handle is not None and self._handle.ptr is not None:
            self._handle.call("check", stream_ptr(self._handle.device))

    def forward(self, example_image: torch.Tensor, audio: torch.Tensor, pose: torch.Tensor, jaco_net: str, weight: float) -> torch.Tensor:
        """util.py:578-612 -> ``deco_out`` [N,T,35,64,64]."""
        if jaco_net == "gan":
            raise NotImplementedError("AudioFeatureNet: the StyleGAN2 branch (jaco_net='gan', AT_net2.generator) is not implemented; "
                                      "its weights are held only for a strict state_dict load")
        if jaco_net != "cnn":
            raise Exception("jaco_net type wrong")   # the reference's own error (util.py:610)
        lstm_out = self.lstm_features(example_image, audio, pose, weight)
        n, t = lstm_out.shape[:2]
        deco = self.decon(lstm_out.reshape(n * t, HIDDEN))
        self.check()
        return deco.view(n, t, *deco.shape[1:])
