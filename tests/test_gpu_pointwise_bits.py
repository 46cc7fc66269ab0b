"""The element-wise and gather operators' results, bit for bit: key-point records, dense-motion front end, flow head (training entry
and both inference forms), feature and image warps, the key-point heads' reduction, anti-alias down-sampling, the final layer's
shift-sum and the NCHW BatchNorm sums, forward and backward, on inputs from seeded CPU generators, each output's sha256 against the
table below.  The table was recorded from the library as it stood BEFORE these kernels were moved onto csrc/pointwise.h (one
sampling position, one sparse motion, one coordinate grid, one set of wave / block reductions) and sorted into one file per operator
(csrc/warp.hip, csrc/kp_head.hip): a changed rounding, a product that moved within its sum or the sign of a zero shows here.

Only outputs that are summed in a fixed order are pinned.  The gradients that float atomics accumulate (``grad_small`` of the front
end, ``grad_features`` of the warp) stay with the tolerance tests (test_gpu_motion_ops*.py, test_gpu_backward.py); the warp's flow and
occlusion gradients are pinned at a power-of-two channel-group count, where one lane per pixel adds once into a zeroed buffer.
Outputs and workspaces are pre-filled with NaN, and so are the logit channels no kernel may read: an element left unwritten or a
stray read changes a digest.  Accuracy is not this file's business.

One assertion is no digest: on the same logits and records the training entry ``eamm_op_motion_head`` and the inference entry
``eamm_op_motion_head_infer`` give bit-equal mask, deformation and occlusion (test_motion_head_training_equals_inference).

``PYTHONPATH=. python tests/test_gpu_pointwise_bits.py`` prints the table of the library it runs on.
"""
import ctypes as C
import functools
import hashlib

import pytest
import torch

from eamm_amd import OcclusionAwareGenerator, _lib, _op, tiny_config
from eamm_amd._handle import ptr, stream_ptr
from eamm_amd.weights import antialias_kernel, synthetic_keypoints, synthetic_source, synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NAN = float("nan")

# ---- the cases: each the smallest shape that reaches the edge its comment names ---------------------------------------------------
KS = (1, 10, 30)                                  # one motion; the shipped count; K = 30: the occlusion logit is slot 31 of the line
GRIDS = [(2, 12, 20), (1, 17, 19)]                # (n, h, w): one partial block of 240 pixels; 323 = 256 + a 67-thread tail block
KP_RECORDS = [(k, jac) for k in (1, 30) for jac in (False, True)]
MOTION_FRONT = [(g, k) for g in GRIDS for k in KS]
ENGINE_CHANNELS = (3, 4)                          # one cached source for all frames (ns = 1); 4: two channel groups per motion
# (occlusion logit, K, ld, grid): a convolution of its own, none, channel K + 1 of the mask logits' rows; ld = 32 and a wider line
MOTION_HEAD = [(occ, k, ld, grid) for occ in ("separate", "absent", "stacked") for k in KS for ld, grid in ((32, GRIDS[0]), (64, GRIDS[1]))]
HEAD_INFER = [(g, k) for g in [(1, 17, 19), (2, 16, 16)] for k in KS]
HEAD_PARITY = [(k, occ) for k in KS for occ in (0, 1)]
ROWSPLIT = [(w, occ) for w in (5, 64, 70) for occ in (0, 1)]       # narrower than the halo; one whole tile; a seam; 7 NC = 84 | 77
# n, ns, hf, wf, C, h, w, occlusion, out2: hf == h and hf == 4 h (the resized flow); one source and one per frame
WARP = {
    "c32_one_source":          (2, 1, 8, 12, 32, 8, 12, True, False),
    "c256_per_frame_out2":     (2, 2, 8, 12, 256, 8, 12, True, True),
    "c32_resized_flow_out2":   (2, 1, 16, 16, 32, 4, 4, True, True),
    "c256_resized_no_occ":     (1, 1, 16, 16, 256, 4, 4, False, False),
}
WARP_IMAGE = [(2, 1, 32, 48, 8, 12, 3, 3), (2, 2, 8, 12, 8, 12, 6, 4)]    # n, ns, H, W, h, w, src_planes, channels
WARP_BACKWARD = [(2, 1, 8, 12, 32), (2, 2, 5, 7, 32)]                     # n, ns, hf, wf, C: C / 4 = 8 lanes per pixel
# B = 1: one block per key point; B = 9: the pixel-slice form.  K = 15: a tail of five in the second group of ten.  njm 0 | 1 | K.
KP_HEAD = [(b, k, njm, geo) for b in (1, 9) for k in (10, 15) for njm in ("0", "1", "K") for geo in ((16, 16, 0), (17, 19, 3))]
ANTIALIAS = [(1, 8, 8, 4), (1, 20, 12, 4), (2, 12, 20, 1)]                # B, H, W, 1 / scale
FINAL_SHIFT_SUM = [5, 128, 131]                                           # W: narrower than the halo; one tile; a 3-pixel second tile
BATCHNORM = [(2, 3, 5, 7), (2, 4, 8, 8)]                                  # N, C, H, W: HW % 4 != 0 (scalar loads); the 16-byte loads

DIGESTS = {
    "kp_records 1 False": {
        "records": "855afb493efdf0c4f3b7eba82dcfbe1cf9ad66bcc506551477f28c0e1ae62abd",
        "singular": "df3f619804a92fdb4057192dc43dd748ea778adc52bc498ce80524c014b81119",
        "grad_kd_value": "1a064a6eeec788ce414cdbac5b2b0966a9e5b2fc2fc85d995e6871f65ee7b6f1",
        "grad_ks_value": "8d2302365b87c64b8d803260e48e4f2b63d12f0fc584c575852012067d124152",
    },
    "kp_records 1 True": {
        "records": "2063391d54646b5345908b52aeb0cb053af20ee5252eaf6df59a6a729fccf5de",
        "singular": "df3f619804a92fdb4057192dc43dd748ea778adc52bc498ce80524c014b81119",
        "grad_kd_value": "50f554d107bc006d1dc0e56ba6ad73ec9a0656f3bd390be092587d9eb77642c4",
        "grad_ks_value": "cbd7d179ac0980c727f836902a94108fb4c14831d93823c3308f16aa6e0d6a05",
        "grad_kd_jacobian": "26e0f15714e8179ed7cc1192bec7e7653d02f59793977f730aede8b9db7ca8b9",
        "grad_ks_jacobian": "88ff2e2e515dc8bcd5e4ea21d04fddd87551df2cb81d73bc94975ae964816896",
    },
    "kp_records 30 False": {
        "records": "1105c952c1e3028435f6f2883696756309ae3ec191e962a82f62b7f52e328b27",
        "singular": "df3f619804a92fdb4057192dc43dd748ea778adc52bc498ce80524c014b81119",
        "grad_kd_value": "0a5a7d6a88a9f5f43656d4f7e80ae5cdef04cd202e0c974fe52ac5fac58b7969",
        "grad_ks_value": "486f676ed10fb3e7125d3cab70d5223f0bca01100dab3a946391c4aa0005344f",
    },
    "kp_records 30 True": {
        "records": "4a9777d1d0966692ec24b7ecad187c6c7d80f6db135998f18f40a30b1944170d",
        "singular": "df3f619804a92fdb4057192dc43dd748ea778adc52bc498ce80524c014b81119",
        "grad_kd_value": "0358afd6811131c048dda6ed8c27bb01c16b99e5c0aede1ed7d6035194fd9528",
        "grad_ks_value": "6880d7ae40405a7869aed8395ff31acbaa1b0227fe28ca401433bb686a63f9db",
        "grad_kd_jacobian": "b12db6c9010a5c476dc03aa3f6a8304cd4b2984563b8425088711353687cd252",
        "grad_ks_jacobian": "203fa819e15c6af53c064a65fd329a9d12ebcc4918f06b5690f74d4464f0662b",
    },
    "motion_front (2, 12, 20) 1": {
        "hourglass_in": "7404e11c02072cab331e4fdad427a6842b664bfb9614f5ee0e7671949afc02ae",
        "sparse_deformed": "c6be3bd00c6551cf6bfa16191b2aa59675d6481eab3163c785190f9a069add74",
        "grad_records": "3fe8f8d8a76d6207aa11fb7d1107b3d11d84aa1abcdf90ab4eca9e8259edbdde",
    },
    "motion_front (2, 12, 20) 10": {
        "hourglass_in": "e954da0123d697c73a0bd9a9a8e936cbaab0431d00f661deeee94b5897eeb808",
        "sparse_deformed": "9de7531e7488e3f53e4f1775de018601cd654de91445534b4dc23d67b39ad3a4",
        "grad_records": "72dd072067c5fa39ec1208b21ae7e77f3fb0eeb29173d92bba77bf406a80edf2",
    },
    "motion_front (2, 12, 20) 30": {
        "hourglass_in": "3960dbf1baa1ebf72ae0a1a14337a721cf2155fa471aafb2e38d1feb018f3f07",
        "sparse_deformed": "9158dfb83695b5ffd941ac70b05483643a8329eecc7569271243d0a3e4a9fde3",
        "grad_records": "d4f875e9010e984c6f1117d1ad63f24d1fbd4b20654f98bd8a7ffb65aee3bc33",
    },
    "motion_front (1, 17, 19) 1": {
        "hourglass_in": "a25b06367196205c24b02b235e74d5fc897d872a9eedfe3fa6b81ffe39a9eb30",
        "sparse_deformed": "e2250360b5770e038652fccb15a4bd3c4e0e987055e273a404a1a0f0daef61af",
        "grad_records": "54a3b5903aea665d79354af6679ae81c393a0b88e5c8d064901f7bdcc7749f33",
    },
    "motion_front (1, 17, 19) 10": {
        "hourglass_in": "9d5e5aba964e4038a7d790cb929c8da54e3cad6f07503361136d95c3733d5c78",
        "sparse_deformed": "f6b62105058d5d15d017521027e19d9bcd0ebd9b29db05d955a4b7b95a3b838d",
        "grad_records": "9c0ef6ecedae650fac1419325ec44882ba8a90bff8a9eaa1e622d4102b2e7dd1",
    },
    "motion_front (1, 17, 19) 30": {
        "hourglass_in": "4732a83fada9a5f23deb9bebc4a2783258edcdb2214622b1bef4170764ff48ef",
        "sparse_deformed": "23360a472e3a09d5a6e4178a4847d7fea1184ee913a237674568e0a505240bf5",
        "grad_records": "c1f43ddbd182ec858532c4d1a54c76237eba4c1b7a56f7b42656c7bfde60bb19",
    },
    "engine_front 3": {
        "sparse_deformed": "6f2ca215f5c7bb79101c38dde42761d8f44e96bbd57482ced71511377d21ed61",
    },
    "engine_front 4": {
        "sparse_deformed": "c9bfc6fab43913207320d86a2f58ea7c8a91c7b786c109ec33bab59f8aa00c9d",
    },
    "motion_head separate 1 32 (2, 12, 20)": {
        "mask": "971c629ebd9eec67586c3090ddb39d98ff216c3637d44518cc406ceee23960a4",
        "deformation": "4d763e17ae0fbda0efdf75bf6d503b69a13d38125806d42810e22c4204493503",
        "occlusion": "0834d889eb7f0fbab715409a04af72b3975c4fd20af2ed8b076c0c8a4ffd3e60",
        "grad_mask_logits": "a75871a20c842a3b3fcc0f6c6e7959f1febae8ab6ab5dfc043a2f4ca353bd158",
        "grad_occlusion_logits": "f3a066338f9e12dee0d0c4599a3dc9b1827f2f396b7c1bebe93e6aa8aef1d734",
        "grad_records": "cd9ab3d39162e3265d80aaeed9ff3fa8df4fb72def8e1382b8c79469444246ce",
    },
    "motion_head separate 1 64 (1, 17, 19)": {
        "mask": "aaf2c683f2dc9a03e9002cb335763122763219de604b1da12fdc230f3809f037",
        "deformation": "38a1bd00988515f05c2c9b12cc8bc5ded2cb117bf0c91a93cbd8e12ea6ed05af",
        "occlusion": "87bce8fa295f07dc2b5536a3234e3fca1e7c6c7e97cd7f2fa9c9c5f67cdc89b3",
        "grad_mask_logits": "74faa577adc57c7131dd1d5eddbc7a740508c566949b37b4d0e4de4562fe67e3",
        "grad_occlusion_logits": "1dd8f3a878a90d5fa2e963bc6b1d48fc06762d52435d476e0a25c72442ae5488",
        "grad_records": "7775ff3e2a058f22d98bae1007d74790bc6d2db458c39ddf070ed5be612f753b",
    },
    "motion_head separate 10 32 (2, 12, 20)": {
        "mask": "edd7f319a574e8d626841d8f3d5888e47b3a4beaf6030259c8679a0450f7d9d7",
        "deformation": "b7de19085ee2bfbb34d1bf1a3717d5cb09036cd4f8d33804175ceada8af6640a",
        "occlusion": "3eb189c0c9692a7eb17e9fd9d686ec8c931d068c9fefc87d18595782e765fd12",
        "grad_mask_logits": "c2424d1bbbc6ca63c5d968fd6d1377e6ff168d4a344c4e5fa065e3d461b03abd",
        "grad_occlusion_logits": "8bccc4ce7d02af3c43597b2e7177b02450b86d91c20858e0e6f9737deca175f4",
        "grad_records": "bb5d5732acbce071df153a6a68685209e4ed23153eba171b24a408cd2890e128",
    },
    "motion_head separate 10 64 (1, 17, 19)": {
        "mask": "2db69991593f95f0b6dfb5ad9a027ff423cbfaedbb3d6b853a76c895dbb57be3",
        "deformation": "2be28d28c673a25b94de6397cde88145adfbe2f2b032f342c9e857af3625c966",
        "occlusion": "da3d5772c91cfbee20085d74cd42909373487c9598f0ce4049263b93ee881ebf",
        "grad_mask_logits": "1417d5437caa0716ae0dff143c059c8940ec26ed27ac0ea9cd0ddadb0709f7be",
        "grad_occlusion_logits": "6309eb16dd5aefb1a8065d27c81cffa7b3f4ced2657c9dad1f10e17150254d27",
        "grad_records": "bb09a02a8180c57a6e9dc4719fedf1dc7f515d936d3ae8b392f148da08e852df",
    },
    "motion_head separate 30 32 (2, 12, 20)": {
        "mask": "3d7dde4e5e0756648f38adb91b5036f7138cb889d34d9f3a98d2cda8dde42814",
        "deformation": "c9fb88f5b3a3f774e767ba8b920a82ea306549190179eb0d29eb84eeda0800fa",
        "occlusion": "94d207ddb309d46cee6471eeb6bfd198334c08d59c4eec265c635c841bbc7ecf",
        "grad_mask_logits": "83fa06501d6f2d2bb6721ea9b06f063897943928beb2b5149d0cfa02f886ca0b",
        "grad_occlusion_logits": "91c1c2bda594f7226b509069f455443a4d6349bfd98f9cc5e0102769d0a40e1c",
        "grad_records": "f65faca16072edef5ca5a090361002b2ee2a599e7f4820ac5f055f668b42698c",
    },
    "motion_head separate 30 64 (1, 17, 19)": {
        "mask": "19b6fba93435d8e0cd23c0493d7ac6c56907a0379d7e157a1b5daa5e5f8fe502",
        "deformation": "4d6ade55b41f39ffc9ae3704419aa20c4fe2cb5c80eb007b9d8fb581f16ca9fa",
        "occlusion": "42901f326cba8822141efc2fdef88826b6a641ee72f9fef8844a672d1a4555ee",
        "grad_mask_logits": "78d174eee99a471b8473851018b0b714d9098eabef503984d81afc49290e23df",
        "grad_occlusion_logits": "9e36e75c9924984df91697a4cb150860153233cb31bfe812f0e50f0c372573bc",
        "grad_records": "f193d9ffb132134d235d9806e2fc6128e081f24cc6c5b4eef1559f8ce17398ee",
    },
    "motion_head absent 1 32 (2, 12, 20)": {
        "mask": "125a6f1d32e5dd3fa3ec48db95827b34498e6ff59f9420a767affa149b0f2990",
        "deformation": "6dc66542000db0d8f26fe20c46573f2256c92854dca1d080c7159c402d10b421",
        "grad_mask_logits": "daf5b866a164121cd88dbf3b7b1bc7c8b36b039ff8f376e6686dede6224c8954",
        "grad_records": "57d74d66987af78ffe05bae0cc5a13207c4956c0eb1bd47d3f7363e5af80dc23",
    },
    "motion_head absent 1 64 (1, 17, 19)": {
        "mask": "66a48eabc848e01e8a7cc7e1381e4107dbe973f0b9aa2bb6acf45c9ff6e511bf",
        "deformation": "641a67338545b2ade91fa3e2fe962ec430691ef130006a46d459531c4e7fbaac",
        "grad_mask_logits": "bf6ef7265f9c141a7daed13ed3d3b4b76b8cca4cd615c8cff4e834152817997c",
        "grad_records": "52369352070f09d6d8cb62b897945a060c7108795ca5791e45dfb275ce225980",
    },
    "motion_head absent 10 32 (2, 12, 20)": {
        "mask": "b1bf0ddc1630069abc77a0cde8aad80770865e1e3a127a726d7c72b8ceed7706",
        "deformation": "4ee10031822bdda054a30dee09a71f7bdaf7afd62459112a6440c83619196853",
        "grad_mask_logits": "6192c9722c0549f02a0932b72678aaedb01373df2fbdecf6a8c2a54ea6a8f838",
        "grad_records": "352fe9988c6a756168e38c1e278ffeddd337a8a6e52f7325658ba43fe18cd35c",
    },
    "motion_head absent 10 64 (1, 17, 19)": {
        "mask": "59a0dabd227b88ca243edeefccf535f9756949104ecb38f58f8e1b186abd4d4e",
        "deformation": "fe767dd3f274facd2e83a630b7f7f142f968b0f5975fdcfeb99dd2abec007e80",
        "grad_mask_logits": "fafe6536ab4e0250224866ceec0d9da9970c32594dde0f0367d01bb99f8918bf",
        "grad_records": "2ce577e7d7404a320fdbfadc1fcce001fcee43f2794a8692dc35855ca1b4a178",
    },
    "motion_head absent 30 32 (2, 12, 20)": {
        "mask": "d3d2021d96f1a7fd4fde567d913c75145aba1d6811eafbd540133b85213efb0c",
        "deformation": "77347d8a573ae0db7a0e94f895f60f317e53dbf0c4934007ff62bb8815810d0e",
        "grad_mask_logits": "a40663c1c4f7667f9dccb64974354137b328c88b0851b19407324158eed1a6f1",
        "grad_records": "980a0025333afe5ae341e49ee16e079bbda60a5880bcb735ba0ea01a19d1792b",
    },
    "motion_head absent 30 64 (1, 17, 19)": {
        "mask": "bb16b884a44838aba511c4aa4b2c6602f8211a9bdf412ad2836607ae04a52a1a",
        "deformation": "6bb7ca6e50b80967ea44181a0341e92bfa45eada1267b7ae4d82c3409205b930",
        "grad_mask_logits": "466520d194e0e785efce9faed2d7bd5d43022b8c19b675bd07cbdebc7b039bdf",
        "grad_records": "82f79763a326b3d4ee5a00d315698fec02263bceb063d803baf68775011cfcae",
    },
    "motion_head stacked 1 32 (2, 12, 20)": {
        "mask": "702ad1704c267a1b094289e369476568bc6546735856924dab87f554bc07dce5",
        "deformation": "9c0f9287e0b1e3f0e9ec40b6c25ace279e3bcb6a52bb8e3ae2960bcca48902dd",
        "occlusion": "c359f23221f9f077b25dbb54968a9351984f60c0432d89ebb7044204a6299cbd",
        "grad_mask_logits": "c6f3b029722748640d9e6154ca49abf95cef48aac93fbc156df67703b9615663",
        "grad_records": "210b96e5447c6f37f125d27134080a90a11dc91c9d21f0e91a440d7581e96afb",
    },
    "motion_head stacked 1 64 (1, 17, 19)": {
        "mask": "cf3f51fde8e4bd1f6285da4d40fc2290385e9dc47af409c0aa2798074c6a59c9",
        "deformation": "cd9b77a9b836cb1db44afa866ec40c4ac340baf818bbc3e11842e03d837eb9e8",
        "occlusion": "0776c881d097479a273ebd8464a972d00fb70ceed28b67b276df6397ee344208",
        "grad_mask_logits": "a1b4760eba816667ea58cc8b553423a5f38b815d40833883e662bdc7a9be4164",
        "grad_records": "55fbed87851ed1d262382a36927d0fcb47c163cff198a4d07d6693ea5e4f641e",
    },
    "motion_head stacked 10 32 (2, 12, 20)": {
        "mask": "272b2804ba184434ccce6450177349777e4904c3ba7e200fec982687b977513f",
        "deformation": "424ace2669bb86492c1a8cacece7be218ef945acdd9fffe022fb14b11d5f8d9b",
        "occlusion": "9728ebf41ddeeb6db7d0bb9be3738c829df561211bb7c4a5d9e845b459172880",
        "grad_mask_logits": "5c752531f0a6ecddac38e18cfa01646c87c28c32d9b35f827e247c2f0a904fc2",
        "grad_records": "8c8beefee9852a2d6b01e00c198923017760355d2e18a78e320fc56bcd4c72fb",
    },
    "motion_head stacked 10 64 (1, 17, 19)": {
        "mask": "93ffe0acf7ea85ac4631c6de326bb93b3a5990148c4aa737ba7c88d0a22bf413",
        "deformation": "d2bdb82de3ab7872627ada9680dad42c43a9b1cd2ea79ea3144d6fe9cf828c2b",
        "occlusion": "d201647b675bfe4a50f8aae032aac0cb57dc3fe7df9475fbd4a957c93d616c56",
        "grad_mask_logits": "76a7688463dd97be7c4e201cf877cebed46b28e38836f3e70392edcf9d45cf4d",
        "grad_records": "b6682cbb3d660a0177a2b5eb2bcc2cd19b6e9120428bb190123747c3acc311ca",
    },
    "motion_head stacked 30 32 (2, 12, 20)": {
        "mask": "b34c78b727271e6bbf52b1ef93162846e6c87f2535a26b6a5434daf6b271f549",
        "deformation": "00c0909c2ccf6b764c3dd95243510d9415f8669db2606cd2a95e4fe5204b0a98",
        "occlusion": "74f403152fbb1eb1bbc67920b266a905dec5174b482d6c943b4903805813a5fc",
        "grad_mask_logits": "59a523af75235186aeea01c82aa19cd45f532b00cb7f2704d49975fbad9d6849",
        "grad_records": "08621ca7ac10c1a2fd8c3af0bb080bf9371f411ca3f2262e84d67d251e09e7ab",
    },
    "motion_head stacked 30 64 (1, 17, 19)": {
        "mask": "ee1a2f69053c146622918e60af2f2904db11296912bee275c3731c7852180a01",
        "deformation": "38ddb9d5facc845a6d9cffc6895b48e4d866fc4c4358c08bd83d04248b980fb6",
        "occlusion": "3bae4b4dfa4dbbd108550cb4a95ff75dc2a021aabc3d399449c0c51852ad3dea",
        "grad_mask_logits": "1f98f34579e7b7c803490ea264ced077b1aa24e1595edab0f91062f034e92a42",
        "grad_records": "ce8dddade56a13d518cd77c317558ee3a3ff68bf978f3fbd346eaa7d075f8be2",
    },
    "motion_head_infer (1, 17, 19) 1": {
        "deformation_occ0": "fae9e9c98f58c18a8b56faa90595efbc6bccdb57320a24cf081b6651431aaead",
        "occlusion_occ0": "f3ec7c3e3686b9547639820dc786abdcd6031496696544a18c661cbfe1cf1c2b",
        "mask_occ0": "efd3a18eeb294287dc7b42d41655b2b4573c083cd3369294960697ceb3f345ce",
        "occ_out_occ0": "f3ec7c3e3686b9547639820dc786abdcd6031496696544a18c661cbfe1cf1c2b",
        "deformation_occ1": "1b4f38678472e6933d159832dde34aa5c1c07309c674d112740023a7fd2b8dd5",
        "occlusion_occ1": "c055df6f2872abc631dfeba67918600e6198ac72025814a9de8a4b54f603594d",
        "mask_occ1": "5f5380e9a7d678de9d7b1c23703d5af69ff33210e5e732b81c174199471511fb",
        "occ_out_occ1": "c055df6f2872abc631dfeba67918600e6198ac72025814a9de8a4b54f603594d",
    },
    "motion_head_infer (1, 17, 19) 10": {
        "deformation_occ0": "319654cd42a7131677805e4dc865802571dc9feec34e1fa311449f0a6cbebe21",
        "occlusion_occ0": "f3ec7c3e3686b9547639820dc786abdcd6031496696544a18c661cbfe1cf1c2b",
        "mask_occ0": "40fe8380c2da6ab83b7694880996d9e49507c1c93a06101d5a2ea752fbc186df",
        "occ_out_occ0": "f3ec7c3e3686b9547639820dc786abdcd6031496696544a18c661cbfe1cf1c2b",
        "deformation_occ1": "0bb96b3625c4aeeb7c43c2d9f0e3d0aa5733d1e4227bbc5b62174b91c2522a5d",
        "occlusion_occ1": "be5c2ba9664090003606819f4d858d4537c506de277c278bbcaea01b3bbceff3",
        "mask_occ1": "3b3987a0278eab5894e9b6ed09462cfa8eb582489f0c88904687690cae4232f6",
        "occ_out_occ1": "be5c2ba9664090003606819f4d858d4537c506de277c278bbcaea01b3bbceff3",
    },
    "motion_head_infer (1, 17, 19) 30": {
        "deformation_occ0": "fb7758befdd7efb8c1125f7af794cbad71596f01b8f08bb6241b4de28640ba91",
        "occlusion_occ0": "f3ec7c3e3686b9547639820dc786abdcd6031496696544a18c661cbfe1cf1c2b",
        "mask_occ0": "295bd47a55967b7df70d5080c44479513fee21372d2dab44292d178f5ef25dc3",
        "occ_out_occ0": "f3ec7c3e3686b9547639820dc786abdcd6031496696544a18c661cbfe1cf1c2b",
        "deformation_occ1": "04299d10215bb5aebd7e8812d694452a6fe638d809c9461762511ce41c3f26f3",
        "occlusion_occ1": "0a9712ce6d72dfbff7b760f7f70595af1771927a45daf872efdb91f7e1d4e2ab",
        "mask_occ1": "d95f99709bfcee3f2a731209728c5adb36475a9a0ee1156ffb30b958a75705f1",
        "occ_out_occ1": "0a9712ce6d72dfbff7b760f7f70595af1771927a45daf872efdb91f7e1d4e2ab",
    },
    "motion_head_infer (2, 16, 16) 1": {
        "deformation_occ0": "07412209977478d7805bce3c88f518822fecedd4b75518bcc06d59fd0d96e382",
        "occlusion_occ0": "34f4b3efd43fd77d16449c5a4fbf63efdf2ed14022e3f5619f8f3ced7a50e104",
        "mask_occ0": "52bc17f9a2ed0932c4a3cf5c6829762f6e9548afa0934ba33c73c9c1963aabe9",
        "occ_out_occ0": "34f4b3efd43fd77d16449c5a4fbf63efdf2ed14022e3f5619f8f3ced7a50e104",
        "deformation_occ1": "a671afba03a94d9d940f4d64af48aaf90c1b3e8ead7e3d9a79f13f7af90895f9",
        "occlusion_occ1": "e3eccdbca8ca1de60221d6e977fa4387bcb304f8277cdf621188198640cc2635",
        "mask_occ1": "a02bfa75ca26412936b05d8f9819d18eecff7c26a230d58a4b9adcb58622c89e",
        "occ_out_occ1": "e3eccdbca8ca1de60221d6e977fa4387bcb304f8277cdf621188198640cc2635",
    },
    "motion_head_infer (2, 16, 16) 10": {
        "deformation_occ0": "bd1d6cb6a3ce7d49079a9b39fc4465a0781bc82e6f6fa069edbbcbce2c0ed45a",
        "occlusion_occ0": "34f4b3efd43fd77d16449c5a4fbf63efdf2ed14022e3f5619f8f3ced7a50e104",
        "mask_occ0": "cdeae56fd3e6d69f70514aeccf3d50997b66d797857e1f3140a5a5da481c9eae",
        "occ_out_occ0": "34f4b3efd43fd77d16449c5a4fbf63efdf2ed14022e3f5619f8f3ced7a50e104",
        "deformation_occ1": "f7cfdeb574c4bd648d789350c2f33b46433b50ba63be927452819d5ca3c32579",
        "occlusion_occ1": "c259bfeef3fa16255f1836c5e6954c7eec5c4ee45a4148cd5e5b970f7d6557b8",
        "mask_occ1": "c16104d2415f1c854955ed12aee8007209ed5c1631f852fcbffd301cbe150fe4",
        "occ_out_occ1": "c259bfeef3fa16255f1836c5e6954c7eec5c4ee45a4148cd5e5b970f7d6557b8",
    },
    "motion_head_infer (2, 16, 16) 30": {
        "deformation_occ0": "0df61a9e68a23884978128e6ece36197935c5c164dd63888a33d824e537f3d6f",
        "occlusion_occ0": "34f4b3efd43fd77d16449c5a4fbf63efdf2ed14022e3f5619f8f3ced7a50e104",
        "mask_occ0": "9f9ed7dc5aea4ac16d4481e5e45b2b209c5d134da95bfd5a80ee01c808eab957",
        "occ_out_occ0": "34f4b3efd43fd77d16449c5a4fbf63efdf2ed14022e3f5619f8f3ced7a50e104",
        "deformation_occ1": "446e19f300d0f839c65d832dd16477aef1cbc46632fb70d15ee462d5447916a9",
        "occlusion_occ1": "e877d822a1417be66f00bcf09988c1374b724242e3757914ba1c3e4219b0e80f",
        "mask_occ1": "6fcef3538af8c899f12bed1b90c8c4bb9f30fb4bfa15582dbf189ee3068da7aa",
        "occ_out_occ1": "e877d822a1417be66f00bcf09988c1374b724242e3757914ba1c3e4219b0e80f",
    },
    "motion_head_rowsplit 5 0": {
        "deformation": "66d66c13c29c435cac9aee36c0c5b6a657218f1d903ef5c7417144f7bf591b21",
        "occlusion": "62d05a2dbcc1643ab5e2d33eaa816d26ebd81a3453c75a0f31413ca9de3f6b03",
        "mask": "724b1110c11e8b8b695f48377ca71a46c5b6e3d072b1c9d5b14597f918fcd3f9",
        "occ_out": "62d05a2dbcc1643ab5e2d33eaa816d26ebd81a3453c75a0f31413ca9de3f6b03",
    },
    "motion_head_rowsplit 5 1": {
        "deformation": "575a59ce6bac230655e4ac1783f5de3d8dbc7e404464ce6f60889dce774a9b8c",
        "occlusion": "bb5fa38ed6ac65bccbe17e729bc098444009e5f8358da560ea6fd29be9e22189",
        "mask": "5be38bfe82406f87bc945a5b65656465988ed05d03d6f8a4e40d0a85dd9486e5",
        "occ_out": "bb5fa38ed6ac65bccbe17e729bc098444009e5f8358da560ea6fd29be9e22189",
    },
    "motion_head_rowsplit 64 0": {
        "deformation": "f4e4e4b0f1a16af6aec7496ed0083dc5fe4873f389da8f1b3dbd5042ecaba9d8",
        "occlusion": "0f8639910d797fccbd3b2132030a6ecec4c40ca2ac220049ca97e941e81d67d5",
        "mask": "74428744f9b7a5856bcb7767e71cc73a011b639101f9f44811ae3417202540b8",
        "occ_out": "0f8639910d797fccbd3b2132030a6ecec4c40ca2ac220049ca97e941e81d67d5",
    },
    "motion_head_rowsplit 64 1": {
        "deformation": "a51f7d3bf01df6ce67e15bfe477ec4cbb8a13acb089c4090686e326af00ab005",
        "occlusion": "e26bc91a819fc692e2f4e632e62dcc8c8da69a8e7e62f6174f9939caa9590c8e",
        "mask": "895f66b43096375a945863bdf175f12d3455bd2ada195f9cd330ebe8cee1a05f",
        "occ_out": "e26bc91a819fc692e2f4e632e62dcc8c8da69a8e7e62f6174f9939caa9590c8e",
    },
    "motion_head_rowsplit 70 0": {
        "deformation": "9a70a1e43a7725845a98018106c576ecc4b4c7501f2fd2c6baa04ee8ca903d86",
        "occlusion": "a0bb9a01df3a2ead0fa750963877d2b85cff0df4ba55baf87a5d7e76fd620ee1",
        "mask": "649d5c9aa32961a0a48bca861b8fd36a4564a5efcd45fb611f0d9bdbb6bd0b90",
        "occ_out": "a0bb9a01df3a2ead0fa750963877d2b85cff0df4ba55baf87a5d7e76fd620ee1",
    },
    "motion_head_rowsplit 70 1": {
        "deformation": "1d91ad073cb3d27ea85b6ff548c878e0ad81527723f7eba407b8cca97c51cec8",
        "occlusion": "70f42063b13506c087351e18d527bc9b3a138742e25a508366a10146cf192b33",
        "mask": "0129a26a01d6265b86a7251f8cf83827c1fe4eaf9d8e691a717cc5cce9158f58",
        "occ_out": "70f42063b13506c087351e18d527bc9b3a138742e25a508366a10146cf192b33",
    },
    "warp c32_one_source": {
        "out": "c2e2af406a2328cc125da8b7fdb7061bcdc1970d4e07b32743f0333c4ba5b455",
    },
    "warp c256_per_frame_out2": {
        "out": "4d482d50e933513827a45f8e526276d239bee5c9a1b18a3bdf4c5f8db17e15fa",
        "out2": "8f1b18fb974be29d55babb9efea9694fb27ea38026f63a9994898b6473ed9e84",
    },
    "warp c32_resized_flow_out2": {
        "out": "8ad7556bb2f5618c44f8b6f199f8beeb31307429459d135d193aa9b3b2389f8d",
        "out2": "9cec98c767a6f34538849b7fbf61fefe7d8f3252a73a655cce7e2458788fee41",
    },
    "warp c256_resized_no_occ": {
        "out": "7a702820351378b208a4002b42527809948e4a969d08fd7216e7068f1396e6ba",
    },
    "warp_image (2, 1, 32, 48, 8, 12, 3, 3)": {
        "out": "414759f81634b688afcd708cd3cee903f916bb0181c6c2e2612e41be74419343",
    },
    "warp_image (2, 2, 8, 12, 8, 12, 6, 4)": {
        "out": "4daad1043d59aca3bf0070455368760e943979a1581ee7c0a51594c5015b7345",
    },
    "warp_backward (2, 1, 8, 12, 32)": {
        "grad_deformation": "e5cbec286a75b73112a4fa7b34a20ceaeece9f24e1ddd68268147f01944cfc45",
        "grad_occlusion": "f737d74e9514e79f1786b814040ee8715f30f55e2bf085286fded5a03d60fdb5",
    },
    "warp_backward (2, 2, 5, 7, 32)": {
        "grad_deformation": "630a5a84a70c85366e30f0c25a21648afd370c4a8422f2f17b82b4c049eac4b3",
        "grad_occlusion": "efe38856eecebb16220f860567ecd0baf3e8ee6b196acb5c04a8d072d145fdac",
    },
    "kp_head 1 10 0 (16, 16, 0)": {
        "value": "807ac5197a1d5291e63b83dd24dbde4ba1740dfcb2a3589bdfe220481b796ec3",
        "heatmap": "5ef7d997f7be65d5599a00534846550bd319e6cd3b4500eb280723eabddf24fe",
        "stats": "75ecfae50c2f23167d74ed4783523aa4fdedf774395356016f8c47b8ee0a41df",
        "grad_logits": "d4903c320af5db3b06a1a6b4ceed6ef2c0fe4aed9b3ebf29db3b680bebce6acc",
        "grad_logits_with_heatmap": "3234c2f5b90994dc50b823bed27a6af09bd23de5476e7619e095619e933d42e0",
    },
    "kp_head 1 10 0 (17, 19, 3)": {
        "value": "8560f39357d74a44ff6ef61a4a9c439bb8421666b3aa2a9b71d91acb577dac03",
        "heatmap": "96781ea3607a7a59123fff95cbb0acb33a3a91b38e2ff026cbd99ae3178f2d02",
        "stats": "c85b670e29b3fc703f19b06532bce27dae968259d38b523b78bdd967b7136f44",
        "grad_logits": "652714de2731438d1994e1f1ebd6e740bf7562bb2501cc014109bdc41a6018c5",
        "grad_logits_with_heatmap": "8b0ddf9eb0bdfd5b8b63d0e1a4d0359cbaa5e568e10f6667f64931fffdb366d0",
    },
    "kp_head 1 10 1 (16, 16, 0)": {
        "value": "d6a34bd5125b46407e9e8bdb7da65f0c534a5d6931595479fefdad6f4ecf4a86",
        "jacobian": "96348d915a78cb48c2016d66b8ec0964a4b2652fc53540c6ed4030e99f29aee6",
        "heatmap": "62ccacffd4c4da3d2903238778c04f6590d30755f27bc2b4f303ab7350744f05",
        "stats": "b7efcc3ae6cdf8f1516c24fd53cfd3b5a356c0c1d074e83dccf976dc7f729f77",
        "grad_logits": "c4e1fa03035376866e8c88e4293a6154c700ce7d0f61f48e662aaf8f46241993",
        "grad_logits_with_heatmap": "d0fc64ba7674d7f29b2301d57af520a0ee36d01c60a7ac8610789f3a3ec1de06",
    },
    "kp_head 1 10 1 (17, 19, 3)": {
        "value": "b0cf690916309d544e0c8bc856afad43ab00754f92d6b991b2a9363140eff3b1",
        "jacobian": "be325419dba99e484d4676bd7ee24f80e8eb2c45bc3411fdc58eadab8f931358",
        "heatmap": "5c1139d6ccb3d95e3e3a21060474c1162d14ffeee06891fc1535eb1b462488dc",
        "stats": "27d7d2b6fb42a8d3d6da629ff3a55ee950991ba06eb3830c32ac87358f653638",
        "grad_logits": "a2c6dd13ddd4f0cf0fb54017007994080e4f276d94c4393c7c0ff3f63bc918cb",
        "grad_logits_with_heatmap": "880467a0476e32c9a80e71cd50d46093f84740268b6b96086cd7745099cd2ec1",
    },
    "kp_head 1 10 K (16, 16, 0)": {
        "value": "4a81110bfcadb6a0233aec5aed68fa278be6027cecc9ec1b0a6b82c39488031a",
        "jacobian": "1c11b540b8895256a3b5efdcb77297dfd5be4eb72a806e2e0981b45b2aea9166",
        "heatmap": "7b99d525407479a345d09ad7d6e4054f33953132d02f017f2d9254d08559ed87",
        "stats": "5d9dfa41b49c7e24a64b0e21dbe862d3a1430a7891bdac52b85d37b910e58314",
        "grad_logits": "4cb641daa0db2abe1b893cc10367dd4c6275d8ae30204ae7397de561a61b6797",
        "grad_logits_with_heatmap": "74944fc4116520bfe2f9dd8cc87fa8cc080a2acdf23f8eed730a215545567938",
    },
    "kp_head 1 10 K (17, 19, 3)": {
        "value": "5066ebe7c28789177d181603948b8139a7efde2397d4275d0a348e156f2d4c3c",
        "jacobian": "fbca12647704d41a5d7ab8b2fdd823bad8ab8a83004b09cc3b08122f731f9ed1",
        "heatmap": "69163face7ce046a9e3cd9a6750f5a2461f335ca97181c081f88a25e95eb04a3",
        "stats": "c6bea5471abbaaf2ecf2f3e6a4fd9ea7510c83ee3320dc416bb64a4b78d1628b",
        "grad_logits": "0cae6f8db933f3f295a851cfc74089c4c2f2237254eda0e556dfcbf735655805",
        "grad_logits_with_heatmap": "1a868ae594cea0282a7541446b7df6a61319ae73e93008b6c308e71c92f95b47",
    },
    "kp_head 1 15 0 (16, 16, 0)": {
        "value": "71e0662b2b690f9702c07e49a6fbc0376ada7aed54096bf27a29460f92688552",
        "heatmap": "0b9cf53d3c83a9c063dbff90ac26a52935c17448cd35db1cdf774e6631b593e4",
        "stats": "f2eae9e6b2fa5f9ae26066e200c1cc2aa6b5c2afbef8c0084f9e73531d2a9de0",
        "grad_logits": "ba87f574c8f7f8b28de733e3c3ef281e4907da5b508a2155b3d6e595abddeaf4",
        "grad_logits_with_heatmap": "7e1b40f78d5ac44fa4baf5b92bccedbc939a61c69044be6f1315d0f7dba30d31",
    },
    "kp_head 1 15 0 (17, 19, 3)": {
        "value": "94502cba141e684f7488c797e06f85b092b4da017957540dbfe1c7d74e245ec1",
        "heatmap": "299d53b05b1713d918f448e1e53ef20f836a6552cf3b86c18f6747f6b6061c48",
        "stats": "a825b41db9c4e551b30f4f2de7c6544774fb89f8749689e38374fbe2855721a3",
        "grad_logits": "240da5805b6e3e8dd1b6709f7ed03b234f4a8a40614d59d7573b1498b5fd5392",
        "grad_logits_with_heatmap": "b82b0f3c4b5b968ecc596d8f2fe8c76a85084056a54c9be663f47efa7fc7e534",
    },
    "kp_head 1 15 1 (16, 16, 0)": {
        "value": "56828527b040aa99dbda32a07759f93a7ce8ef932dc1e3129a7392d63f6d99bd",
        "jacobian": "b1102f6f4dbc0acd7c08794aef6ce9cd8a321c2a5e62bb46f830ddeb3d140809",
        "heatmap": "c33a48e711a05f488e50839be2fe67747939d4ce727c74ed661394f077b41ca0",
        "stats": "e549d52aaa4bea486a76ddc8b41ad5e06dda0fb98e92cf40025b758f5e5b0663",
        "grad_logits": "8184059cb3770708a67904972b1c088a0c8ba255d4e5b758b2ed77b7e2291281",
        "grad_logits_with_heatmap": "3e909b85381a21229d81b98d3a44323604dd809ffed1bf8e294644eb9c949099",
    },
    "kp_head 1 15 1 (17, 19, 3)": {
        "value": "18679318b5e8dec4a647bed1890cf9835647b74c8846246a7af5ce3e73f07686",
        "jacobian": "c6b2247aaa2abef70c35700415322c6031a15f4a039afc1adfe2471fb2695fda",
        "heatmap": "ae11e6c6fe6e48e0c2c209a5ca42a4166a587281f0f39667279803c9df441b1f",
        "stats": "97b68d82ae3fc0639d8051fc3b08baa8a1276e0ea850a3e053a00bca6a795a97",
        "grad_logits": "8db7de78050ad9007b0e5727b72e0f5f77cf0971e3da7c1ca4035f55c8eeab2f",
        "grad_logits_with_heatmap": "77cdfee6e4895b1c680737a183547da8ad48b4219afa64824f8225bea7e8578a",
    },
    "kp_head 1 15 K (16, 16, 0)": {
        "value": "9149a8d78a122178154f8f897d09f3813d5cb45a9416a011fb914ca883bddf0f",
        "jacobian": "7ef1fd1aebd1baf22d716b09d05bc347ac3c234ff76e00cd0b6d530f1ae27e88",
        "heatmap": "d6f7078a02a21270bcd61cb52859703af8c5a89602d17cbee270e89ebaaafece",
        "stats": "27da00bc27b59a53289cd1b2ff2b22457f34411b5671182e83beb84beeb18cc0",
        "grad_logits": "97ed60acf9a1734762de1f19a9db6730bfe63e79102e4bd8e519f8b8536ef9ed",
        "grad_logits_with_heatmap": "3c2da5132b611859a86ecb42c79af1f71f0ab9867427fdb895557587b812d26a",
    },
    "kp_head 1 15 K (17, 19, 3)": {
        "value": "8a0123849bc74db07fa4a7ef3682b69b784765ecc54631ff0708eea2cb5bf4a8",
        "jacobian": "6a55e5c4b7a118380dd4b2cfe7c56e71d6c5bd0dface8ad0ee9d3226faf8cefa",
        "heatmap": "ff7f335deaefa4ac753fae5e83144e5a54a520a41445d806fb12ccaa37ace5ab",
        "stats": "bc9af7695c6dfeea31d65338dc246300a32cd572e0c8cd4f236db30920fc4cce",
        "grad_logits": "d363b09cf8051d380e307d3281fb4318dd7cba6434127d91debcd232eeec3469",
        "grad_logits_with_heatmap": "06465ae0af2aa9f9df0845f076c7aec68e2ea7389680c517e9694755d3e28b79",
    },
    "kp_head 9 10 0 (16, 16, 0)": {
        "value": "67bb5c5209f2e1ce5c06c3167acac3288ba53fd5392863f3078c235846e69f91",
        "heatmap": "dd9e844bb4db197b6df10accae225aae11113ab6845276b74799afc949203172",
        "stats": "9c275940e625ba7da53073f0946d971bf1f9439d0bf83d5af2fd0869b5b4aebb",
        "grad_logits": "9538f1d33583a8bb0f889ba971baf1aa2e4354f73b7c9e4aacfc55815c5f006b",
        "grad_logits_with_heatmap": "04ae3826e8efd3a57668371742fe637f780c7b60b421c2ad48c42fa29328758d",
    },
    "kp_head 9 10 0 (17, 19, 3)": {
        "value": "db303f59f01f1f120ea471f07e243b9947d330c0cb7ae9b229f338f60adad05b",
        "heatmap": "2d89b58235dc3c0175ccb5d5d40b47aebe0d22bd5c157ac04280e6e4ba4cec25",
        "stats": "456640d9d2e8dfd4f002c668050d1ce5266f919b471c404da6d5a245ea61b843",
        "grad_logits": "79d0d847b08d30d37fcf1f4f40fdab6c39bdf612cecd6a8d68872dffdc3da3f9",
        "grad_logits_with_heatmap": "bc393ae895edfe35975b85028b6e701a2c29e49cde1f6c3f527f3ed71f27505b",
    },
    "kp_head 9 10 1 (16, 16, 0)": {
        "value": "9c6af1cbbc420ad7aec50c7bd7b4b9b405548b4227ff007ac82c16382e346555",
        "jacobian": "def12c1d927fed1e04879a75379f171193d63274d37cf3d9ea485fc8c74b436c",
        "heatmap": "6d60802d3c7965657aa7b84c90f857b4b91db5099c5cf3299574228fcbc25607",
        "stats": "7f3be8ea213cae807a077b581f489ee23b98b379bad93111fdbcad29159a8b65",
        "grad_logits": "f60e680f47202261d07d5f2ae81d254e4519825c427c5bc150b58442b6f596e8",
        "grad_logits_with_heatmap": "fa9680355e81f31a0faf52e3651b49c4b8c0d519abc6aa9e30109dbda2b714c5",
    },
    "kp_head 9 10 1 (17, 19, 3)": {
        "value": "38568f5c460dffe31c82315b7b4b4730c1f3c3a15a29c80910c13a69028f6cd2",
        "jacobian": "690421442223048c35b0dbb38ef787f873df5a348002787682b3d5b2fcecd2cd",
        "heatmap": "f1cff251062d7f5d064b511adcd002e8fa2bf326061d5ee5892107828d18a389",
        "stats": "7ef122e90eec93f31609f04cb9e22e01c419c69f44896160949384225a087a15",
        "grad_logits": "fd043f0091b95e783d729f52ce02613982f0499e82f67ab8e4cb5f75164db20a",
        "grad_logits_with_heatmap": "820cccda93502e93813b18a8172ebb00c5e7496d4f126e6990d68fce71a1b58a",
    },
    "kp_head 9 10 K (16, 16, 0)": {
        "value": "2212fb832fa04dccba7ea2e2b5006f7a38c8219581de6418312ee49042c0549f",
        "jacobian": "9a4e1a23893aa8d8aac5b0839305c0a374874a44d007555cf3c0f9f2bb4ddedb",
        "heatmap": "c08834d694296f7b77f9ecf42632bdff51d205cbedbb1ae00eb2c57317e76c2e",
        "stats": "32527ffe9673abf00d7683cf89cf8da569bdbfa8f5e82369a58fdd92a30addd8",
        "grad_logits": "1cb157f024b24801927c37d9992e344bd7f07b5186c6dfe27bf32871384f15fb",
        "grad_logits_with_heatmap": "67d348b9fdd1a7627abed9ec6d7bef1f5d77c4df35a54f5a37c4df8a68002047",
    },
    "kp_head 9 10 K (17, 19, 3)": {
        "value": "4a95cae5e9600743f822af61ef3332af9276612546f5a5d5f4fc45750a80293c",
        "jacobian": "db2e5f79309566a10ec10d9a0302c41c235fddf053f4de00ed55b00246a57603",
        "heatmap": "8ee189f73912fa2d34336513498920d410eca97403bb4f61ed1ba29c0a0b807f",
        "stats": "88f9dedb4d99883a227a1ca59451a78cd64705c002cea68db66e659201da12fb",
        "grad_logits": "c269c57dcda77664711447f0d76300ea848249887777f44431757f72bb3eb3a3",
        "grad_logits_with_heatmap": "a13f3416db70699c8eb81852763dbdd7c830842e883fc812ee8a725268783706",
    },
    "kp_head 9 15 0 (16, 16, 0)": {
        "value": "6d9b842ea2cf1617603da58a0a8fe88f8841f58e5b992760dabd4ec94d69a7a6",
        "heatmap": "1fe7bec24da772751f58be562d04cf4aded694f4d14e5511f00c0a56fb87a89f",
        "stats": "df9f6d016db16501d386b2618ac57a5156a86ff6615d4e2411861b2246555a50",
        "grad_logits": "9987d7386f6ed94b8c8d558ca94fa447805e8ead84e4941da621881e8732d7dd",
        "grad_logits_with_heatmap": "c78fb0faac95b06eccec4bb66023676ffe047bc2265f87523af88822a2ac8af1",
    },
    "kp_head 9 15 0 (17, 19, 3)": {
        "value": "75aad60122a60b774279b23857707ad4c4c0694bf95e5ca46fb73ff1268a211f",
        "heatmap": "c896bdd3f1ce0b4a5cdf01fa35a3f05b862d749b92bc0d55a10452a845fe95c5",
        "stats": "88a5b30042144977a72c396f3d3cbfefd7adb737e2c0053f6f00aca262fdbc0d",
        "grad_logits": "b0183d5f2f7ae5f5387ec002df48edf9d1ecc13840d6a8455b4023d4d32db927",
        "grad_logits_with_heatmap": "10776f2dcd6ddf51e70ab2db00ce4b0264ee60deb31b062a6c578af3acebfd43",
    },
    "kp_head 9 15 1 (16, 16, 0)": {
        "value": "9e02acad9e1faaea928fb9793d66a93425e76a63999547c49eae6b49608d604e",
        "jacobian": "0efc0e7b45447d4e2ad27158679324955b0e77c9532ea6529e0c772e2eed86e9",
        "heatmap": "73b9943b561c02ff7e55677012a125311c71ffca432ae3b9507874d5773e9c31",
        "stats": "881ebc8c862ad75f843685130488bb2daa8a45928f8f0f5f83d4557bd94219cc",
        "grad_logits": "8b8c7f8c29b5bcd37d0f78d2eb5a15b1a13dd1676fd7db34afdf277566c3745a",
        "grad_logits_with_heatmap": "5dbcc9eb0989acaabf3db4ffbc72ccbcca70928b2041246c408452429271b0e8",
    },
    "kp_head 9 15 1 (17, 19, 3)": {
        "value": "1c31175c61f89027c48583b97bc358ddf67da6fadba2d8c4a8c0316fade6e3b3",
        "jacobian": "d4b9d28245188af9303db7342097d628e9bd04e792503c5ad33d24630cb31420",
        "heatmap": "21382f46f5c0e7bd5903359f5174465e9600f9a5c8ce1844bbe864cbecf86726",
        "stats": "c849eb46f9d9786c00dcd7156453011c154056430b2872af9e70d2ceb45157ad",
        "grad_logits": "f4c2cb20c3c09bd4e0822706e68a07a336621fb978bf4a876b8641510dc1a79b",
        "grad_logits_with_heatmap": "7eec7113af126a4073534510d9a0bc321c5d95aac0aabab61a91810d31c50563",
    },
    "kp_head 9 15 K (16, 16, 0)": {
        "value": "69f0ffcf8ab5303ecbd8986ee4836b4b2681efe859413c934672d819ce0f5c82",
        "jacobian": "1f2d06d2967066f1c8547d8d2a3f705ee0e68a3d1766b6b36b172f176a14f83c",
        "heatmap": "5c134fb64c8d75ae0a696b08167dd6b6dbdb3da96703bb765aeef44ec1b577af",
        "stats": "34fd0f06c1a3ef2c9261812facf3324505f9dd9f83003c3fdf328948935b7fff",
        "grad_logits": "69353c4126115d64810d5419544a1a945fbaf1afc03ced847cabb36a9d2cef72",
        "grad_logits_with_heatmap": "3fc537362ab380a3d026ea3987cd65aad90275cc930557be4321be82f604ed18",
    },
    "kp_head 9 15 K (17, 19, 3)": {
        "value": "9f6c48e47b97f02faa9e572f01f5d2f88873a06663a08b5a54f317f116f91e98",
        "jacobian": "146335547e4035a303890078f93bdb7c3580accc3c9f078b4009b19afbb7da08",
        "heatmap": "b7adba65797b7d3e5b8dbd0a6f3b817104d0df6255c60e7f24c5d8b963083051",
        "stats": "1a17ce6b3e45f2740312f1d34284cbd604b53eabb7853ed4f90f75b29505aa89",
        "grad_logits": "925c1f4f6329b90933b573f5fa59e78a36609891460909e43feba34894730586",
        "grad_logits_with_heatmap": "6bee63fa4bf88d374b04595a08d9ffeb65a1400dd157f92d0a12be403ce71545",
    },
    "antialias_down (1, 8, 8, 4)": {
        "small": "0a47b3e93f29d3bb2af4cf2094e720461f2b15f380a7ceee5295992ad939ab8f",
        "grad_source": "75336617643f34fb7d89a8375b5ecae1b0950fa426bdfb681a47a859130aa770",
    },
    "antialias_down (1, 20, 12, 4)": {
        "small": "626a83dd92f67b3c473e6e4985f35f7203bf1943fa492e60a7373f6dc89507f8",
        "grad_source": "993a881a2c74c33ccb2a75e9d96f2172e492209cec4d46f20ff51e260a32d883",
    },
    "antialias_down (2, 12, 20, 1)": {
        "small": "fb51147aa57839bb6d4ad7dad94bab1f18bd44a2436ba4f02010f4668ec109b9",
        "grad_source": "4b1829532e327f119f03be970342e055ffa48db1d2127e3df0169ae1314aaaa6",
    },
    "final_shift_sum 5": {
        "out": "28f40900ad2272fb5451771a170b7ce26a7668e9c8a100f970e9b297269476c0",
    },
    "final_shift_sum 128": {
        "out": "74f24ff30c35e10b05addf7f4a7472727522a28c926e4f009e08ac6cd3a23ee2",
    },
    "final_shift_sum 131": {
        "out": "1b831bef863d7a11fdac080325e041a45a4112334cd6fca64d9ce3e30e9eb213",
    },
    "batchnorm_nchw (2, 3, 5, 7)": {
        "local_sums": "5533b6dd96ce43c1c52c76683aab998c9503e6487019e7d915f19713c102f5d5",
        "backward_sums": "a82a2d877e44cd626af9eef3628b6d399cf93506d85fadbd9d945c7c87a9f31d",
    },
    "batchnorm_nchw (2, 4, 8, 8)": {
        "local_sums": "0eb0b0ab0f11d43c58e25efdae4c0ab248e14b9df152fdf335d4b455a17868fa",
        "backward_sums": "8ef69aaddd69705de5cd3f9fdf76986e4dc10823ed09facbe8dd1669a4251be6",
    },
}


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def poisoned(*shape):
    return torch.full(shape, NAN, device=DEV)


def gen(*seed):
    return torch.Generator().manual_seed(sum(int(s) * 131 ** i for i, s in enumerate(seed)) + 90001)


def digests_of(**outs):
    torch.cuda.synchronize()
    return {k: sha(v) for k, v in outs.items() if v is not None}


def keypoints(n, k, seed, jacobian=True):
    return {a: b.to(DEV) for a, b in synthetic_keypoints(n, k, seed=seed, jacobian=jacobian).items()}


def records(n, k):
    kd, ks = keypoints(n, k, 4), keypoints(n, k, 6)
    rec, flag = poisoned(n, k, 8), torch.zeros(1, dtype=torch.int32, device=DEV)
    _op.call("kp_records", DEV, kd["value"], kd["jacobian"], ks["value"], ks["jacobian"], n, k, rec, flag)
    return rec


def wild_flow(n, h, w, g):
    """the identity grid + noise: samples beyond both borders, two far outside, one NaN"""
    ident = torch.stack(torch.meshgrid(torch.linspace(-1, 1, h), torch.linspace(-1, 1, w), indexing="ij")[::-1], -1)
    defo = ident[None] + 0.5 * torch.randn(n, h, w, 2, generator=g)
    defo[0, 0, 1] = torch.tensor([-3.0, -3.0])
    defo[0, 0, 2] = torch.tensor([3.0, 3.0])
    defo[0, 1, 0] = torch.tensor([NAN, 0.0])
    return defo.contiguous()


@functools.lru_cache(maxsize=None)
def kp_records_digests(k, jac):
    n = 2
    kd, ks = keypoints(n, k, 4, jac), keypoints(n, k, 6, jac)
    rec, flag = poisoned(n, k, 8), torch.zeros(1, dtype=torch.int32, device=DEV)
    _op.call("kp_records", DEV, kd["value"], kd.get("jacobian"), ks["value"], ks.get("jacobian"), n, k, rec, flag)
    g_rec = torch.randn(n, k, 8, generator=gen(1, k, jac)).to(DEV)
    g_kdv, g_ksv = poisoned(n, k, 2), poisoned(n, k, 2)
    g_kdj, g_ksj = (poisoned(n, k, 2, 2), poisoned(n, k, 2, 2)) if jac else (None, None)
    _op.call("kp_records_backward", DEV, kd.get("jacobian"), ks.get("jacobian"), g_rec, n, k, g_kdv, g_ksv, g_kdj, g_ksj)
    return digests_of(records=rec, singular=flag, grad_kd_value=g_kdv, grad_ks_value=g_ksv, grad_kd_jacobian=g_kdj, grad_ks_jacobian=g_ksj)


@functools.lru_cache(maxsize=None)
def motion_front_digests(grid, k):
    n, h, w = grid
    g = gen(2, k, h)
    rec = records(n, k)
    cpad = _op.round_up(4 * (k + 1), 32)              # (beyond the K + 1 records: the zero fill)
    small = torch.rand(n, h, w, 4, generator=g).to(DEV)
    hg, sd = poisoned(n, h, w, cpad), poisoned(n, k + 1, 3, h, w)
    _op.call("motion_front", DEV, rec, small, n, k, h, w, 0.01, cpad, hg, sd)
    g_hg, g_sd = torch.randn(n, h, w, cpad, generator=g).to(DEV), torch.randn(n, k + 1, 3, h, w, generator=g).to(DEV)
    g_small, g_rec = poisoned(n, h, w, 4), poisoned(n, k, 8)
    ws = poisoned(_lib.lib().eamm_op_motion_workspace_floats(n, k, h, w))
    _op.call("motion_front_backward", DEV, rec, small, n, k, h, w, 0.01, cpad, g_hg, g_sd, g_small, g_rec, work=ws)
    return digests_of(hourglass_in=hg, sparse_deformed=sd, grad_records=g_rec)


@functools.lru_cache(maxsize=None)
def engine_front_digests(channels):
    """``sparse_deformed`` of the frozen engine: source preparation, records and front end with ONE source for both frames"""
    cfg = {**tiny_config(), "num_channels": channels}
    net = OcclusionAwareGenerator(**cfg)
    net.load_state_dict(synthetic_state_dict(cfg, seed=1234), strict=True)
    net = net.to(DEV).eval()
    engine = net.encode_source(synthetic_source(64, seed=1, channels=channels).to(DEV))
    out = engine.forward_frames(keypoints(2, 10, 2), keypoints(1, 10, 0), outputs=("prediction", "sparse_deformed"))
    return digests_of(sparse_deformed=out["sparse_deformed"])


def head_logits(n, h, w, k, ld, used, g):
    logits = torch.randn(n, h, w, ld, generator=g)
    logits[..., used:] = NAN
    return logits.to(DEV)


@functools.lru_cache(maxsize=None)
def motion_head_digests(occ, k, ld, grid):
    n, h, w = grid
    g = gen(3, k, ld, len(occ))
    rec = records(n, k)
    lm = head_logits(n, h, w, k, ld, k + 1 + (occ == "stacked"), g)
    lo = head_logits(n, h, w, k, ld, 1, g) if occ == "separate" else None
    has_occ = occ != "absent"
    lo_arg = C.c_void_p(lm.data_ptr() + 4 * (k + 1)) if occ == "stacked" else lo
    mask, defo, occl = poisoned(n, k + 1, h, w), poisoned(n, h, w, 2), poisoned(n, h, w) if has_occ else None
    _op.call("motion_head", DEV, lm, ld, lo_arg, ld if has_occ else 0, rec, n, k, h, w, mask, defo, occl)
    g_mask, g_defo = torch.randn(n, k + 1, h, w, generator=g).to(DEV), torch.randn(n, h, w, 2, generator=g).to(DEV)
    g_occ = torch.randn(n, h, w, generator=g).to(DEV) if has_occ else None
    g_lm, g_lo, g_rec = poisoned(n, h, w, ld), poisoned(n, h, w, ld) if occ == "separate" else None, poisoned(n, k, 8)
    g_lo_arg = C.c_void_p(g_lm.data_ptr() + 4 * (k + 1)) if occ == "stacked" else g_lo
    ws = poisoned(_lib.lib().eamm_op_motion_workspace_floats(n, k, h, w))
    _op.call("motion_head_backward", DEV, mask, occl, rec, n, k, h, w, g_mask, g_defo, g_occ, g_lm, ld, g_lo_arg, ld if has_occ else 0, g_rec,
             work=ws)
    return digests_of(mask=mask, deformation=defo, occlusion=occl, grad_mask_logits=g_lm, grad_occlusion_logits=g_lo, grad_records=g_rec)


def head_infer(logits, rec, n, k, h, w, has_occ):
    bufs = poisoned(n, h, w, 2), poisoned(n, h, w), poisoned(n, k + 1, h, w), poisoned(n, 1, h, w)
    _op.call("motion_head_infer", DEV, logits, rec, n, k, h, w, has_occ, *bufs)
    return bufs


@functools.lru_cache(maxsize=None)
def head_infer_digests(grid, k):
    n, h, w = grid
    g = gen(4, k, h)
    rec = records(n, k)
    out = {}
    for has_occ in (0, 1):
        defo, occ, mask, occ_out = head_infer(head_logits(n, h, w, k, 32, k + 1 + has_occ, g), rec, n, k, h, w, has_occ)
        out.update(digests_of(**{f"deformation_occ{has_occ}": defo, f"occlusion_occ{has_occ}": occ, f"mask_occ{has_occ}": mask,
                                 f"occ_out_occ{has_occ}": occ_out}))
    return out


@functools.lru_cache(maxsize=None)
def rowsplit_digests(w, has_occ):
    n, h, k, ps = 2, 3, 10, 128
    nc = k + 1 + has_occ
    g = gen(5, w, has_occ)
    part = 0.5 * torch.randn(n, h, w, ps, generator=g)
    part[..., 7 * nc:] = NAN
    bias = torch.randn(nc, generator=g).to(DEV)
    defo, occ, mask, occ_out = poisoned(n, h, w, 2), poisoned(n, h, w), poisoned(n, k + 1, h, w), poisoned(n, 1, h, w)
    _op.call("motion_head_rowsplit", DEV, part.to(DEV), ps, nc, bias, records(n, k), n, k, h, w, has_occ, defo, occ, mask, occ_out)
    return digests_of(deformation=defo, occlusion=occ, mask=mask, occ_out=occ_out)


@functools.lru_cache(maxsize=None)
def warp_digests(name):
    n, ns, hf, wf, c, h, w, occ, second = WARP[name]
    g = gen(6, list(WARP).index(name))
    feat = torch.randn(ns, hf, wf, c, generator=g).to(DEV)
    defo = wild_flow(n, h, w, g).to(DEV)
    om = torch.rand(n, h, w, generator=g).to(DEV) if occ else None
    s2, t2 = ((0.3 + 0.8 * torch.randn(c, generator=g)).to(DEV), (0.2 + 0.7 * torch.randn(c, generator=g)).to(DEV)) if second else (None, None)
    out, out2 = poisoned(n, hf, wf, c), poisoned(n, hf, wf, c) if second else None
    if second:
        _op.call("warp_ex", DEV, feat, defo, om, n, ns, hf, wf, c, h, w, out, 0, None, out2, s2, t2)
    else:
        _op.call("warp", DEV, feat, defo, om, n, ns, hf, wf, c, h, w, out, 0, None)
    return digests_of(out=out, out2=out2)


@functools.lru_cache(maxsize=None)
def warp_image_digests(case):
    n, ns, hh, ww, h, w, planes, channels = case
    g = gen(7, hh, planes)
    src = torch.rand(ns, planes, hh, ww, generator=g).to(DEV)
    defo = wild_flow(n, h, w, g).to(DEV)
    out = poisoned(n, channels, hh, ww)
    _op.call("warp_image", DEV, src, defo, n, ns, hh, ww, h, w, planes, channels, out)
    return digests_of(out=out)


@functools.lru_cache(maxsize=None)
def warp_backward_digests(case):
    n, ns, hf, wf, c = case
    g = gen(8, ns, hf)
    feat = torch.randn(ns, hf, wf, c, generator=g).to(DEV)
    defo = wild_flow(n, hf, wf, g).to(DEV)
    om = torch.rand(n, hf, wf, generator=g).to(DEV)
    g_out = torch.randn(n, hf, wf, c, generator=g).to(DEV)
    g_feat, g_defo, g_occ = poisoned(ns, hf, wf, c), poisoned(n, hf, wf, 2), poisoned(n, hf, wf)
    _op.call("warp_backward", DEV, feat, defo, om, g_out, n, ns, hf, wf, c, g_feat, g_defo, g_occ)
    return digests_of(grad_deformation=g_defo, grad_occlusion=g_occ)


@functools.lru_cache(maxsize=None)
def kp_head_digests(b, k, njm_name, geo):
    h, w, pad = geo
    njm = {"0": 0, "1": 1, "K": k}[njm_name]
    cs = _op.round_up(k + 4 * njm, 4) + 4
    g = gen(9, b, k, njm, h)
    logits = torch.randn(b, h, w, cs, generator=g)
    logits[..., k + 4 * njm:] = NAN
    logits = logits.to(DEV)
    oh, ow = h - 6 + 2 * pad, w - 6 + 2 * pad
    value, jac, heat, stats = poisoned(b, k, 2), poisoned(b, k, 2, 2) if njm else None, poisoned(b, k, oh, ow), poisoned(b, k, 2)
    ws = poisoned(_lib.lib().eamm_op_kp_head_workspace_floats(b, k))
    _op.call("kp_head", DEV, logits, b, k, njm, h, w, cs, pad, 0.1, value, jac, heat, stats, work=ws)
    out = digests_of(value=value, jacobian=jac, heatmap=heat, stats=stats)
    g_value = torch.randn(b, k, 2, generator=g).to(DEV)
    g_jac = torch.randn(b, k, 2, 2, generator=g).to(DEV) if njm else None
    g_heat = torch.randn(b, k, oh, ow, generator=g).to(DEV)
    for name, gh in (("grad_logits", None), ("grad_logits_with_heatmap", g_heat)):
        grad = poisoned(b, h, w, cs)
        ws = poisoned(_lib.lib().eamm_op_kp_head_workspace_floats(b, k))
        _op.call("kp_head_backward", DEV, logits, stats, value, jac, g_value, g_jac, gh, b, k, njm, h, w, cs, pad, 0.1, grad, work=ws)
        out.update(digests_of(**{name: grad}))
    return out


@functools.lru_cache(maxsize=None)
def antialias_digests(case):
    b, hh, ww, inv = case
    g = gen(10, hh, inv)
    src = torch.rand(b, 3, hh, ww, generator=g).to(DEV)
    weight = antialias_kernel(3).to(DEV) if inv != 1 else None
    small = poisoned(b, hh // inv, ww // inv, 4)
    _op.call("antialias_down", DEV, src, weight, b, hh, ww, inv, small)
    g_small = torch.randn(b, hh // inv, ww // inv, 4, generator=g).to(DEV)
    g_src = poisoned(b, 3, hh, ww)
    _op.call("antialias_down_backward", DEV, g_small, weight, b, hh, ww, inv, g_src)
    return digests_of(small=small, grad_source=g_src)


@functools.lru_cache(maxsize=None)
def final_shift_sum_digests(w):
    n, h = 2, 3
    g = gen(11, w)
    part = torch.randn(n, h, w, 32, generator=g)
    part[..., 21:] = NAN
    bias = torch.randn(3, generator=g).to(DEV)
    out = poisoned(n, 3, h, w)
    _op.call("final_shift_sum", DEV, part.to(DEV), bias, n, h, w, out)
    return digests_of(out=out)


@functools.lru_cache(maxsize=None)
def batchnorm_digests(case):
    n, c, h, w = case
    g = gen(12, c, h)
    x = (1.5 + torch.randn(n, c, h, w, generator=g)).to(DEV)
    dy = torch.randn(n, c, h, w, generator=g).to(DEV)
    mean = x.cpu().mean(dim=(0, 2, 3)).to(DEV)
    lib = _lib.lib()
    out = {}
    for name in ("local_sums", "backward_sums"):
        sums, ws = poisoned(6 * c + 2), poisoned(max(1, lib.eamm_bn_workspace_floats(n, c, h * w)))
        if name == "local_sums":
            rc = lib.eamm_bn_local_sums(ptr(x), n, c, h * w, ptr(sums), ptr(ws), stream_ptr(DEV, None))
        else:
            rc = lib.eamm_bn_backward_sums(ptr(x), ptr(dy), ptr(mean), n, c, h * w, ptr(sums), ptr(ws), stream_ptr(DEV, None))
        _lib.check(rc, None)
        out.update(digests_of(**{name: sums}))
    return out


FAMILIES = [      # (name, digest function, its cases)
    ("kp_records", kp_records_digests, KP_RECORDS),
    ("motion_front", motion_front_digests, MOTION_FRONT),
    ("engine_front", engine_front_digests, [(c,) for c in ENGINE_CHANNELS]),
    ("motion_head", motion_head_digests, MOTION_HEAD),
    ("motion_head_infer", head_infer_digests, HEAD_INFER),
    ("motion_head_rowsplit", rowsplit_digests, ROWSPLIT),
    ("warp", warp_digests, [(name,) for name in WARP]),
    ("warp_image", warp_image_digests, [(c,) for c in WARP_IMAGE]),
    ("warp_backward", warp_backward_digests, [(c,) for c in WARP_BACKWARD]),
    ("kp_head", kp_head_digests, KP_HEAD),
    ("antialias_down", antialias_digests, [(c,) for c in ANTIALIAS]),
    ("final_shift_sum", final_shift_sum_digests, [(w,) for w in FINAL_SHIFT_SUM]),
    ("batchnorm_nchw", batchnorm_digests, [(c,) for c in BATCHNORM]),
]
CASES = [(name, fn, tuple(case)) for name, fn, cases in FAMILIES for case in cases]


def case_id(name, case):
    return f"{name} {' '.join(str(c) for c in case)}"


@pytest.mark.parametrize("name,fn,case", CASES, ids=[case_id(name, case) for name, _, case in CASES])
def test_pointwise_bits(name, fn, case):
    key, got = case_id(name, case), fn(*case)
    print(key, got)
    assert key in DIGESTS, f"no recorded digests for {key}"
    assert got == DIGESTS[key], (key, {k: (v, DIGESTS[key].get(k)) for k, v in got.items() if v != DIGESTS[key].get(k)})


@pytest.mark.parametrize("k,has_occ", HEAD_PARITY)
def test_motion_head_training_equals_inference(k, has_occ):
    """One softmax, flow combine and sigmoid: the training entry (stacked occlusion logit, line of 32) and the inference entry agree
    in every bit on the same logits and records."""
    n, h, w = GRIDS[1]
    rec = records(n, k)
    logits = head_logits(n, h, w, k, 32, k + 1 + has_occ, gen(13, k, has_occ))
    defo_i, occ_i, mask_i, _ = head_infer(logits, rec, n, k, h, w, has_occ)
    mask, defo, occ = poisoned(n, k + 1, h, w), poisoned(n, h, w, 2), poisoned(n, h, w) if has_occ else None
    lo = C.c_void_p(logits.data_ptr() + 4 * (k + 1)) if has_occ else None
    _op.call("motion_head", DEV, logits, 32, lo, 32 if has_occ else 0, rec, n, k, h, w, mask, defo, occ)
    torch.cuda.synchronize()
    same = {"mask": torch.equal(mask, mask_i), "deformation": torch.equal(defo, defo_i), "occlusion": not has_occ or torch.equal(occ, occ_i)}
    print(f"training vs inference head K {k} occ {has_occ}: {same}")
    assert all(same.values()), same


if __name__ == "__main__":
    print("DIGESTS = {")
    for name_, fn_, case_ in CASES:
        print(f'    "{case_id(name_, case_)}": {{')
        for out_, digest_ in fn_(*case_).items():
            print(f'        "{out_}": "{digest_}",')
        print("    },")
    print("}")
