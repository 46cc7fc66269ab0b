"""The training convolutions' results, bit for bit: the stride-2 convolution (``eamm_op_conv_s2`` / ``_dgrad`` / ``_wgrad``), the 4x4
stride-2 transposed convolution (``eamm_op_deconv4s2`` / ``_dgrad`` / ``_wgrad`` with its bias gradient) and the stride-1 weight
gradient (``eamm_op_conv_wgrad``, one case per route) on inputs from a seeded CPU generator, each output's sha256 against the table
below.  The table was recorded from the library as it stood BEFORE these kernels were moved onto the shared gather-GEMM loop
(conv_gather_gemm.h) and the shared strided weight-gradient kernel: a change of any product's place in its sum shows here.  Every
kernel involved sums in a fixed order (no atomics), so the digests do not depend on the run or the card.  Accuracy is not this
file's business: tests/test_gpu_emotion_backward.py, test_gpu_audio_backward.py and test_gpu_backward.py compare the same operators
with float64 ATen.

The inference path's register-staged kernel (conv_mfma.hip, ``eamm_op_conv`` / ``eamm_op_conv_ex`` tile code 0) runs the same loop.
tests/test_gpu_conv_modes.py and tests/test_gpu_ops.py compare its modes with float64 and with one another, but not with an earlier
build, so its modes are pinned here too: every filter shape it is compiled for in the three tile widths, two concatenated inputs,
phase mode, split-K, the pooled epilogue, the NCHW store and the second output (CONV_CASES).

Outputs and workspaces are pre-filled with NaN, so an element that a kernel leaves unwritten (or a slab it reads without having
written it) changes the digest too.

The transposed convolution goes through ``audio_ops.conv_transpose4s2_nhwc`` and autograd, which pad the channels to the kernels'
granule of 32 in front of the entries (Cout = 35 runs as 64 columns of which 29 are zero filters) and call all three of them.
"""
import functools
import hashlib

import pytest
import torch

from eamm_amd import _lib, _op, audio_ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# (B, Hin, Win, Cin, Cout): M below one tile; an M tail with two pixel splits in the weight gradient; several N tiles; deep K
S2_SHAPES = [(1, 2, 2, 32, 32), (9, 10, 6, 32, 32), (2, 6, 10, 64, 128), (1, 4, 4, 256, 512)]
# (B, H, W, Cin, Cout): one pixel; a channel tail at 35; rows != columns of the weight gradient with the operands' roles swapped
T4_SHAPES = [(1, 1, 1, 32, 32), (3, 4, 4, 64, 35), (2, 5, 3, 256, 128)]
# (B, H, W, Cin, Cout): the per-tap kernel (a width that is no multiple of 32), the filter-row kernel, and the F(3x3,4x4) route at its
# smallest size (512 tiles = the default EAMM_WGRAD_WINO4_MIN_TILES): the per-tap kernel on 36 planes
WGRAD_CASES = {"per_tap": (2, 9, 20, 64, 32), "row": (1, 4, 32, 64, 64), "wino4_planes": (2, 64, 64, 32, 32)}

# eamm_op_conv_ex, tile code 0: B, H, W, C0, Cout and what differs from a plain 3x3 (ks = (kh, kw))
CONV_CASES = {
    "3x3_two_inputs_resid_relu_bn128": dict(B=1, H=8, W=8, C0=64, C1=32, Cout=128, resid=True, act=1),
    "3x3_odd_raster_ntail_bn64":       dict(B=2, H=5, W=7, C0=32, Cout=40),
    "3x3_pool_bn32":                   dict(B=1, H=8, W=8, C0=32, Cout=32, act=1, pool=1),
    "3x3_splitk3_resid":               dict(B=1, H=8, W=8, C0=96, Cout=128, resid=True, splitk=3),
    "3x3_second_output":               dict(B=1, H=8, W=8, C0=64, Cout=64, resid=True, second=True),
    "phase_bn64":                      dict(B=1, H=4, W=6, C0=64, Cout=64, up=1),
    "phase_two_inputs_splitk2_bn32":   dict(B=2, H=4, W=4, C0=32, C1=32, Cout=32, up=1, splitk=2),
    "phase_nchw_bn128":                dict(B=1, H=5, W=7, C0=64, Cout=72, up=1, nchw=1),
    "7x7_sigmoid_nchw":                dict(B=2, H=8, W=12, C0=32, Cout=3, ks=(7, 7), act=2, nchw=1),
    "7x7_bn128":                       dict(B=1, H=8, W=8, C0=32, Cout=96, ks=(7, 7)),
    "7x7_bn64":                        dict(B=1, H=6, W=6, C0=32, Cout=48, ks=(7, 7), act=1),
    "7x1_two_inputs_bn64":             dict(B=2, H=9, W=6, C0=32, C1=32, Cout=64, ks=(7, 1)),
    "7x1_bn128":                       dict(B=1, H=8, W=8, C0=32, Cout=128, ks=(7, 1)),
    "7x1_bn32":                        dict(B=1, H=7, W=5, C0=64, Cout=32, ks=(7, 1), act=1),
    "1x1_two_inputs_bn64":             dict(B=5, H=1, W=1, C0=96, C1=32, Cout=40, ks=(1, 1)),
    "1x1_splitk4_bn128":               dict(B=8, H=1, W=1, C0=512, Cout=256, ks=(1, 1), act=1, splitk=4),
    "1x1_pointwise_bn32":              dict(B=2, H=6, W=10, C0=32, Cout=32, ks=(1, 1)),
}

DIGESTS = {
    "conv_s2 k1 (1, 2, 2, 32, 32)": {
        "forward": "915efcb79fab4af97cef658ff13c67dce5429eb88ca562bba1e5d1ee85aaba5d",
        "dgrad": "4c92cc7222ad4457dbdca1a420cdae304bd8e541fa7bbef85308a0fc424e313b",
        "wgrad": "744e446a27c848b126c67eba6d6c17ce8f91ba65718f82d2c7fb642eafd1a716",
    },
    "conv_s2 k1 (9, 10, 6, 32, 32)": {
        "forward": "5ff617ce556d0c2d33eaa32541de23003526a28c96beb14413df1dcc270574e5",
        "dgrad": "1af4a530aefcaad25d8d555cea9033022773f2bb07a946a16faa7394f972ee12",
        "wgrad": "22a18fb4d617c54a036e070c342eed164e18704d7a90e72b202370e8e00e4d30",
    },
    "conv_s2 k1 (2, 6, 10, 64, 128)": {
        "forward": "05cfaa5ee798cae0112c58bc46879eb865aa25ed100f60685d1a5c9687977c97",
        "dgrad": "2c6649a2eed320124817bdbc72b89d2bd22e6b1b553cf7eca6136782c0efd160",
        "wgrad": "f65069278587e8a7572e8f8635c812a979fcb4adca53779cc14f335efaff4788",
    },
    "conv_s2 k1 (1, 4, 4, 256, 512)": {
        "forward": "ba61685b95618647f2b598f02636d654c90a141f6f0f6ae1254f43e23c15f39a",
        "dgrad": "829057b88b9668e37a09bb1d484637a33418785ce227f531c5db41375f821d64",
        "wgrad": "67ad503f0d784fbf60790f9202304d67d8d92aaed2f52126e6ecdaaf60a23814",
    },
    "conv_s2 k3 (1, 2, 2, 32, 32)": {
        "forward": "57fb3ea35c0faa50e3075c896690f34caead5aa818325f6def1cbd21307b3036",
        "dgrad": "e39610249848f8ae13bad2b154c3d7cc6392df2d1704fd40d7a437e946b5868e",
        "wgrad": "b7c066a8eee9332fb623e6a3d23327f4271241a87d5c610e24d8e98f12ef3c19",
    },
    "conv_s2 k3 (9, 10, 6, 32, 32)": {
        "forward": "708e121831306afa94b49245b52a00b2aac2c50839bbac89bb6df11a0e7058d3",
        "dgrad": "02895c6ec5bd05403344daefc5f0877f428c60d1d8121cafb1d96deb903d9b5e",
        "wgrad": "3dd219918bbd025d8ccf3c2748ab2ef78904e6aadc29ec2efe01bc363730bc8e",
    },
    "conv_s2 k3 (2, 6, 10, 64, 128)": {
        "forward": "32cb5f6f91d57db2060b6085f304507fb62d3cb10c377c38883079ee083eceb0",
        "dgrad": "b8a04bc50c56f04df79b9d2238ea145b35f55b9cf7b2a1bb61c566063139718f",
        "wgrad": "0e9ddd578335ed8a139f20d5409cc2845dcf7488088fdfb5e236dabab3853ac6",
    },
    "conv_s2 k3 (1, 4, 4, 256, 512)": {
        "forward": "fb1a22128396455e534feee8a2ba634fe7f58ed43e1e228ec29935b4f3377b4c",
        "dgrad": "4b805ed5cfdc236cb19c7e02e81339f6cf1aae4cb1e3ea9392a376a38f015c0a",
        "wgrad": "371763d62c8aba9450e5f4a6e5b70545d2bd117fb703de3d1ae943b7afca9774",
    },
    "deconv4s2 (1, 1, 1, 32, 32)": {
        "forward": "de36d28bd00a7cb35eccbe7b94f68cfbb73dc49060b8db847d4014a813f3f131",
        "dgrad": "e6ce1cd875af704776f3bddcd9410387d40ae3047c036d2292f6aa840cb02792",
        "wgrad": "ed215f7637ed10e145c8505b69e7fe7e5ed2587a97dcb0378eb303516d5a14fb",
        "bias_grad": "2adea15b3f2e087f69431d44792f66940e0256e8c6f289e28f2c566624ddae92",
    },
    "deconv4s2 (3, 4, 4, 64, 35)": {
        "forward": "d93fd855e1b40b70c7e945f73e9d3d8b3074355701f866424581367511dbbdc0",
        "dgrad": "1749a80d52ec10c8a929d7012cf83448a9f778a773759b54e0441fdef2f3a9e0",
        "wgrad": "1e7d1ac674708d77ab1492aa436b1f3bde27f70f6639ca49a89b2a351ff28d81",
        "bias_grad": "b2b6bd0d5a6f8b3a95f432925a2a35976a65a65e82f4244dfd010ec99dd5fdfb",
    },
    "deconv4s2 (2, 5, 3, 256, 128)": {
        "forward": "954d536c924e81ef689ec2025c4da3d4c7c6d236ee3cdb3cc60d69c51c2bdd71",
        "dgrad": "bbac9a64b1da2ca643a10d70a23ca310e3c1f77a6e212f6dd9b69588d6887028",
        "wgrad": "67e4c64c1d881f58aaed57db6c917fef4248875a299af1cf0b245993730b2a68",
        "bias_grad": "91ad9ffefa74a26612bd12b1c66bb1d32d381be47754c985b7bb84cb16d9fa3f",
    },
    "conv_wgrad per_tap": {
        "wgrad": "9e7f4386aae6afe3834ea421f732a6c63ff65debd006495ad001e7711c5d9985",
        "bias_grad": "7b84a7f67e73cbfbc4b28a8164c38a490423002dc24861c1b86b7bc30cb1bdee",
    },
    "conv_wgrad row": {
        "wgrad": "12dec11e1f0dd83716ae0ea8f48a8f44c7ccb60e61c609e28c3bae70cc89fed6",
        "bias_grad": "c2b4e232e2316599f1a63820380b4235183a1e85b1af53b87a0f37daebf33269",
    },
    "conv_wgrad wino4_planes": {
        "wgrad": "2be97248f36fd1b501e3f92af430150ec1ae60f23eb7e5714886c9dfcd4860b3",
        "bias_grad": "3ee3cde218c10e6dedcd61fd36a1a056095896d1b5f4fe5be4788902efc85a1a",
    },
    "conv 3x3_two_inputs_resid_relu_bn128": {
        "out": "6a74e3ae0ce3b5e0cc192ad8689456364c54ed5b628d282ff8f3b86c06ff9af7",
    },
    "conv 3x3_odd_raster_ntail_bn64": {
        "out": "c5da7764c5621ecd853f70517df7f03e544d0ce0c5dc77cf815afb78e8db5884",
    },
    "conv 3x3_pool_bn32": {
        "out": "7601bc68d5dc3119af6ce7cd092c482674a2d023974499d6399b0e0d1ea0bf4c",
    },
    "conv 3x3_splitk3_resid": {
        "out": "2dcdd67eb9b714bcc9b4f22e4baeffd53f3d5ee24ecb226c9fd15444fa73bf96",
    },
    "conv 3x3_second_output": {
        "out": "4aa5cd10ef6d13af07f315a43ab1f938d8a67ee0de77922b8f8f19566483cb6b",
        "out2": "4dd3516f063b2788e93b10a72cab26c1f87d54a8b3df1bc30eab2c1b007082c0",
    },
    "conv phase_bn64": {
        "out": "f98aa41ecf310ff14e057510421d943949d477038f7a4624acf8636fd1f306ff",
    },
    "conv phase_two_inputs_splitk2_bn32": {
        "out": "a42d4a893d37776af41816a14e62e462646e685c97bdfd113be720e6c22b446a",
    },
    "conv phase_nchw_bn128": {
        "out": "d33f019918d56030a030c5978c4b00fa7302724993efdc22db333668c493fc2e",
    },
    "conv 7x7_sigmoid_nchw": {
        "out": "8b6b7f3ec20a61697e8d2ae5e8c06b076f5eb9a46393ea54bb520115aaeb45f7",
    },
    "conv 7x7_bn128": {
        "out": "da91047f8a885691a8add2c5221e576be97006014d8fd229987a96bd895deff5",
    },
    "conv 7x7_bn64": {
        "out": "b01b76e3f6ec51724d1d98338201f46a093ae69184659f19f988cd624a3b62bc",
    },
    "conv 7x1_two_inputs_bn64": {
        "out": "d33179a636e6bee585f1a9fc322747db4637cac9f30d02fbd7cca3e5db930b3d",
    },
    "conv 7x1_bn128": {
        "out": "33d56a1708cf791b8c99b2d4ec0ce0ea94969e98eadd9aabfea06b2a3f3a5744",
    },
    "conv 7x1_bn32": {
        "out": "023ac5a395f9dce83291d2e40fb957ed1b128751526a6edd0c01c361ec924e1b",
    },
    "conv 1x1_two_inputs_bn64": {
        "out": "918cf81f79aa2b0799ee4382c7496135b7305cd2c3c25afa3f3947322c4e643f",
    },
    "conv 1x1_splitk4_bn128": {
        "out": "5339eb3ed2e16db448f28068550125d34c5fd2da044dca503857deb55277f078",
    },
    "conv 1x1_pointwise_bn32": {
        "out": "17ceff293be726d38b870d41970d528a2ccd607d11f000579e2507e6d603b067",
    },
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def poisoned(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def work(name, *dims):
    n = getattr(_lib.lib(), f"eamm_op_{name}_workspace_floats")(*dims)
    assert n > 0, (name, dims)
    return poisoned(n)


@functools.lru_cache(maxsize=None)
def s2_digests(k, shape):
    b, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(5000 + 100 * k + sum(shape))
    x = torch.randn(b, h, w, cin, generator=g).to(DEV)
    wt = (torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5).to(DEV)
    gy = torch.randn(b, h // 2, w // 2, cout, generator=g).to(DEV)
    y, dx, dw = poisoned(b, h // 2, w // 2, cout), poisoned(b, h, w, cin), poisoned(cout, cin, k, k)
    dims = (b, h, w, cin, cout, k)
    _op.call("conv_s2", DEV, x, b, h, w, cin, wt, cout, k, y, work=work("conv_s2", *dims))
    _op.call("conv_s2_dgrad", DEV, gy, b, h, w, cin, wt, cout, k, dx, work=work("conv_s2_dgrad", *dims))
    _op.call("conv_s2_wgrad", DEV, x, gy, b, h, w, cin, cout, k, dw, work=work("conv_s2_wgrad", *dims))
    torch.cuda.synchronize()
    return {"forward": sha(y), "dgrad": sha(dx), "wgrad": sha(dw)}


@functools.lru_cache(maxsize=None)
def t4_digests(shape):
    b, h, w, cin, cout = shape
    g = torch.Generator().manual_seed(6000 + sum(shape))
    x = torch.randn(b, h, w, cin, generator=g).to(DEV).requires_grad_()
    wt = (torch.randn(cin, cout, 4, 4, generator=g) / (4 * cin) ** 0.5).to(DEV).requires_grad_()
    bias = (0.1 * torch.randn(cout, generator=g)).to(DEV).requires_grad_()
    gy = torch.randn(b, 2 * h, 2 * w, cout, generator=g).to(DEV)
    y = audio_ops.conv_transpose4s2_nhwc(x, wt, bias)
    y.backward(gy)
    torch.cuda.synchronize()
    return {"forward": sha(y), "dgrad": sha(x.grad), "wgrad": sha(wt.grad), "bias_grad": sha(bias.grad)}


@functools.lru_cache(maxsize=None)
def wgrad_digests(name):
    b, h, w, cin, cout = WGRAD_CASES[name]
    g = torch.Generator().manual_seed(7000 + sum(WGRAD_CASES[name]))
    x = torch.randn(b, h, w, cin, generator=g).to(DEV)
    gy = torch.randn(b, h, w, cout, generator=g).to(DEV)
    dw, db = poisoned(cout, cin, 3, 3), poisoned(cout)
    _op.call("conv_wgrad", DEV, x, gy, b, h, w, cin, cout, 3, 3, dw, db, work=work("conv_wgrad", b, h, w, cin, cout, 3, 3))
    torch.cuda.synchronize()
    return {"wgrad": sha(dw), "bias_grad": sha(db)}


@functools.lru_cache(maxsize=None)
def conv_digests(name):
    c = dict(CONV_CASES[name])
    b, h, w, c0, cout = (c[k] for k in ("B", "H", "W", "C0", "Cout"))
    c1, up, (kh, kw) = c.get("C1", 0), c.get("up", 0), c.get("ks", (3, 3))
    g = torch.Generator().manual_seed(8000 + list(CONV_CASES).index(name))
    x0 = torch.randn(b, h, w, c0, generator=g).to(DEV)
    x1 = torch.randn(b, h, w, c1, generator=g).to(DEV) if c1 else None
    wt = (torch.randn(cout, c0 + c1, kh, kw, generator=g) * (2.0 / ((c0 + c1) * kh * kw)) ** 0.5).contiguous()     # host
    bias = (0.1 * torch.randn(cout, generator=g)).contiguous()                                                       # host
    ho, wo = h << up, w << up
    res = torch.randn(b, ho, wo, cout, generator=g).to(DEV) if c.get("resid") else None
    s2, t2 = ((0.3 + 0.8 * torch.randn(cout, generator=g)).to(DEV), (0.2 + 0.7 * torch.randn(cout, generator=g)).to(DEV)) \
        if c.get("second") else (None, None)
    pool, nchw = c.get("pool", 0), c.get("nchw", 0)
    out = poisoned(b, cout, ho, wo) if nchw else poisoned(b, ho >> pool, wo >> pool, cout)
    out2 = poisoned(b, ho, wo, cout) if c.get("second") else None
    _op.call("conv_ex", DEV, x0, c0, x1, c1, b, h, w, up, wt, bias, cout, kh, kw, c.get("act", 0), pool, res,
             c.get("splitk", 0), 0, out, 0, None, None, None, out2, s2, t2, nchw, 0)
    torch.cuda.synchronize()
    return {"out": sha(out), **({"out2": sha(out2)} if out2 is not None else {})}


def all_digests():
    """{case id: {output: sha256}}: what DIGESTS holds"""
    out = {}
    for k in (1, 3):
        for shape in S2_SHAPES:
            out[f"conv_s2 k{k} {shape}"] = s2_digests(k, shape)
    for shape in T4_SHAPES:
        out[f"deconv4s2 {shape}"] = t4_digests(shape)
    for name in WGRAD_CASES:
        out[f"conv_wgrad {name}"] = wgrad_digests(name)
    for name in CONV_CASES:
        out[f"conv {name}"] = conv_digests(name)
    return out


def check(case, got):
    print(case, got)
    assert case in DIGESTS, f"no recorded digests for {case}"
    assert got == DIGESTS[case], (case, {k: (v, DIGESTS[case].get(k)) for k, v in got.items() if v != DIGESTS[case].get(k)})


@pytest.mark.parametrize("shape", S2_SHAPES)
@pytest.mark.parametrize("k", [1, 3])
def test_conv_s2_bits(k, shape):
    check(f"conv_s2 k{k} {shape}", s2_digests(k, shape))


@pytest.mark.parametrize("shape", T4_SHAPES)
def test_deconv4s2_bits(shape):
    check(f"deconv4s2 {shape}", t4_digests(shape))


@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_conv_wgrad_bits(name):
    check(f"conv_wgrad {name}", wgrad_digests(name))


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_register_staged_conv_bits(name):
    check(f"conv {name}", conv_digests(name))
