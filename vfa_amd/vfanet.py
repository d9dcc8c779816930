"""``VFANet`` -- the caller of the projector, with the reference's interface (``vfa/model/vfanet.py:14-149``).

Only the camera loop (:64-82) is the hot path; it is replaced by one batched ``aggregate_views`` call (HIP
kernels).  Backbone, laterals and BEV heads are stock convolutions / GroupNorm and stay PyTorch (MIOpen on ROCm):
they are laid out with the reference's sub-module names so that its checkpoints (``model_state_dict``) load
key-for-key.  GroupNorm is per sample, so running the laterals on all cameras at once is numerically the
per-camera computation of the reference.

Multi-GPU (``distributed=True``): each rank runs backbone + laterals + projection for ITS cameras
(``camera_shard``) and the partial BEV maps are summed with one RCCL all-reduce; heads run replicated.

``view_reduce="max"`` fuses the cameras by an elementwise maximum instead of the reference's sum (``aggregate_views``; DESIGN.md
4.9).  It is a plain attribute, not a buffer: the ``state_dict`` keys stay the reference's.

``head_convs="hip"`` (a plain attribute too; default ``"library"``) runs the dense 3x3 convolutions of the BEV heads at inference on
the HIP kernels of ``csrc/vfa_conv.hip`` from the same parameters (``heads``).

``head_convs_train="hip"`` (the same kind of attribute; default ``"library"``) runs the four 256 -> 256 convolutions of the heads
WITH gradients on ``ops.conv3x3_train`` -- HIP forward, input-gradient and weight-gradient kernels (``csrc/vfa_conv_grad.hip``), the
same bits on every run -- while the norms, the ReLUs and the few-output layers stay the modules they are (``heads``).

``trunk_convs="hip"`` (the same kind of attribute; default ``"library"``) runs the residual stages ``layer1`` .. ``layer4`` of the
ResNet trunk at inference on the HIP kernels of ``csrc/vfa_trunk.hip`` from the same parameters (``trunk``).

``trunk_stem="hip"`` (independent of ``trunk_convs``; default ``"library"``) runs the trunk's stem -- the 7 x 7 stride-2 convolution,
GroupNorm, ReLU and the max pooling -- at inference on the HIP kernels of ``csrc/vfa_stem.hip`` (``trunk``).  With
``trunk_stem = trunk_convs = head_convs = "hip"`` no library convolution runs between the camera bytes and the detections.

``trunk_convs_train="hip"`` (independent of both, which stay inference-only; default ``"library"``) runs the trunk's identity
residual blocks -- stride 1, no projection: 5 of resnet18's 8, 13 of resnet34's 16 -- WITH gradients on ``ops.residual_block_train``,
one autograd node per block that keeps three maps instead of the library's five (``csrc/vfa_trunk_grad.hip``; ``trunk``; DESIGN.md
4.6).  The projection blocks and the stem stay the modules they are.

``trunk_proj_train="hip"`` (independent of the three; default ``"library"``) runs the trunk's three projection blocks -- stride 2 and
a 1 x 1 projection: the first block of ``layer2`` .. ``layer4`` -- WITH gradients on ``ops.projection_block_train``, one node per block
that keeps four maps; the gradients of the stride-2 convolutions are ``vfa_trunk_down_wgrad_f32`` and ``vfa_trunk_down_dgrad_f32``
(DESIGN.md 4.6).

``trunk_stem_train="hip"`` (independent of the five; default ``"library"``) runs the trunk's stem WITH gradients on ``ops.stem_train``,
one node that keeps the raw ``conv1`` map and the images -- no normalised map, no index map of the pooling; the backward is
``vfa_stem_pool_backward_f32``, ``vfa_group_norm_backward_f32`` and ``vfa_stem_conv_wgrad_f32``.  The images are data: an
input that requires grad takes the module stem.  With ``trunk_stem_train = trunk_convs_train = trunk_proj_train = "hip"`` no library
convolution, normalisation or pooling runs in the trunk's forward or backward, and every trunk parameter's gradient is the same bits
on every run without ``torch.use_deterministic_algorithms``; with only the latter two the stem runs as a module.
"""
import glob
import os
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops, vfa_op
from .aggregate import aggregate_views, camera_shard, check_view_reduce
from .vfa_op import VFA

# Producer fusion, inference on the fused frame path: the GroupNorm affine + ReLU of the lateral branch
# is applied inside the integral-image row scan (`vfa_affine_relu_integral_image_f32`); the lateral maps are never written.
FUSE_PRODUCER = os.environ.get("VFA_AMD_FUSE_PRODUCER", "1") == "1"
# ... and in TRAINING (off by default): with gradients, sum mode and a module set the fused frame kernels cover, the producer runs as
# one autograd node (``vfa_op._LateralIntegrals``: HIP forward and backward kernels, no NCHW lateral map or d lateral) feeding the
# fused frame node with integral images.  Otherwise training runs ``laterals()`` (MIOpen conv, torch GroupNorm and ReLU).
FUSE_PRODUCER_TRAIN = os.environ.get("VFA_AMD_FUSE_PRODUCER_TRAIN", "0") == "1"

# ``pretrained=True`` (the default of the reference's train.py:90): the reference downloads the torchvision ImageNet
# checkpoint (resnet.py:155-159, 170-172).  There is no network on the MI355X boxes, so the file is looked up locally.
PRETRAINED_ENV = "VFA_AMD_PRETRAINED"
# Who runs the dense 3x3 convolutions of the BEV heads (``VFANet.head_convs``, ``VFANet.heads(convs=...)``)
HEAD_CONVS = ("library", "hip")
# Who runs the four 256 -> 256 convolutions of the BEV heads where gradients are enabled (``VFANet.head_convs_train``)
HEAD_CONVS_TRAIN = ("library", "hip")
# Who runs the residual stages of the trunk (``VFANet.trunk_convs``, ``VFANet.trunk``)
TRUNK_CONVS = ("library", "hip")
# Who runs the trunk's stem (``VFANet.trunk_stem``, ``VFANet.trunk``)
TRUNK_STEM = ("library", "hip")
# Who runs the trunk's identity residual blocks where gradients are enabled (``VFANet.trunk_convs_train``, ``VFANet.trunk``)
TRUNK_CONVS_TRAIN = ("library", "hip")
# Who runs the trunk's projection blocks where gradients are enabled (``VFANet.trunk_proj_train``, ``VFANet.trunk``)
TRUNK_PROJ_TRAIN = ("library", "hip")
# Who runs the trunk's stem where gradients are enabled (``VFANet.trunk_stem_train``, ``VFANet.trunk``)
TRUNK_STEM_TRAIN = ("library", "hip")


def _find_pretrained(base):
    cand = [os.environ.get(PRETRAINED_ENV)] if os.environ.get(PRETRAINED_ENV) else []
    hub = os.path.join(os.environ.get("TORCH_HOME", os.path.join(os.path.expanduser("~"), ".cache", "torch")), "hub",
                       "checkpoints")
    cand += sorted(glob.glob(os.path.join(hub, f"{base}-*.pth")))
    for path in cand:
        if path and os.path.isdir(path):
            hits = sorted(glob.glob(os.path.join(path, f"{base}*.pth")))
            path = hits[0] if hits else None
        if path and os.path.isfile(path):
            return path
    return None


def load_pretrained_trunk(trunk, base):
    """Reference ``_load_pretrained`` (resnet.py:170-175): copy every checkpoint entry whose key exists in the trunk
    (conv weights and the affine parameters the GroupNorm layers share with torchvision's BatchNorm by NAME; running
    statistics have no counterpart).  Returns the number of tensors loaded.  The reference downloads the checkpoint; a box
    without network cannot, and training from scratch where ImageNet weights were asked for must not happen silently: without
    a local checkpoint this RAISES, unless random initialisation is chosen explicitly with ``VFA_AMD_PRETRAINED=none``."""
    if os.environ.get(PRETRAINED_ENV, "").strip().lower() == "none":
        warnings.warn(f"VFANet(pretrained=True) with {PRETRAINED_ENV}=none: the trunk keeps its random initialisation")
        return 0
    path = _find_pretrained(base)
    if path is None:
        raise FileNotFoundError(
            f"VFANet(pretrained=True): no local {base} ImageNet checkpoint and no network to download it like the reference "
            f"does (resnet.py:159).  Set {PRETRAINED_ENV} to the .pth file or its directory, or place it in the torch hub cache; "
            f"{PRETRAINED_ENV}=none starts from random weights on purpose")
    ckpt = torch.load(path, map_location="cpu")
    own = trunk.state_dict()
    hit = {k: v for k, v in ckpt.items() if k in own and tuple(v.shape) == tuple(own[k].shape)}
    own.update(hit)
    trunk.load_state_dict(own)
    print(f"VFANet: loaded {len(hit)} of {len(own)} trunk tensors from {path}")
    return len(hit)


def _gn(ch):
    return nn.GroupNorm(16, ch)


class _Block(nn.Module):
    """Two 3x3 convs with GroupNorm(16) and an identity / 1x1 projection shortcut (reference resnet.py:26-57)."""
    expansion = 1

    def __init__(self, cin, cout, stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = _gn(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = _gn(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), _gn(cout))

    def forward(self, x):
        y = F.relu(self.bn1(self.conv1(x)), inplace=True)
        y = self.bn2(self.conv2(y))
        return F.relu(y + (x if self.downsample is None else self.downsample(x)), inplace=True)

    def forward_hip(self, x):
        """``forward`` at inference on ``ops.trunk_conv`` / ``ops.group_norm_affine`` / ``ops.residual_join``: a GroupNorm is a per
        (image, channel) affine that its consumer applies as it reads, so no normalised map is written -- three or four raw
        convolutions and one join per block.  The same function of the same parameters up to the summation order."""
        stride = self.conv1.stride[0]
        y1 = ops.trunk_conv(x, self.conv1.weight, stride)
        y2 = ops.trunk_conv(y1, self.conv2.weight, 1, affine=_gn_affine(y1, self.bn1))
        if self.downsample is None:
            return ops.residual_join(y2, _gn_affine(y2, self.bn2), x.contiguous(), out=y2)
        yd = ops.trunk_conv(x, self.downsample[0].weight, stride)
        return ops.residual_join(y2, _gn_affine(y2, self.bn2), yd, _gn_affine(yd, self.downsample[1]), out=y2)

    @property
    def is_identity(self):
        """Stride 1 and no projection: the shortcut is x itself."""
        return self.downsample is None and self.conv1.stride[0] == 1

    @property
    def is_projection(self):
        """Stride 2 and a 1 x 1 projection with its GroupNorm as the shortcut."""
        return self.downsample is not None and self.conv1.stride[0] == 2

    def forward_train_hip(self, x):
        """``forward`` with gradients: an identity block on ``ops.residual_block_train``, a projection block on
        ``ops.projection_block_train`` -- the calls of ``forward_hip`` and their bits, and a backward on the HIP kernels from three
        or four kept maps."""
        first = (x, self.conv1.weight, self.bn1.weight, self.bn1.bias, self.conv2.weight, self.bn2.weight, self.bn2.bias)
        if self.is_identity:
            return ops.residual_block_train(*first, self.bn1.num_groups, self.bn1.eps)
        assert self.is_projection
        return ops.projection_block_train(*first, self.downsample[0].weight, self.downsample[1].weight, self.downsample[1].bias,
                                          self.bn1.num_groups, self.bn1.eps)


def _gn_affine(y, gn):
    return ops.group_norm_affine(y, gn.num_groups, gn.weight, gn.bias, gn.eps)


class _Trunk(nn.Module):
    """ResNet-18/34 trunk returning the stride-8/16/32 maps (reference resnet.py:95-147)."""

    def __init__(self, depths):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = _gn(64)
        widths, cin = (64, 128, 256, 512), 64
        for i, (w, d) in enumerate(zip(widths, depths)):
            blocks = [_Block(cin, w, 1 if i == 0 else 2)] + [_Block(w, w) for _ in range(d - 1)]
            setattr(self, f"layer{i + 1}", nn.Sequential(*blocks))
            cin = w
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def stem(self, x):
        """The 7 x 7 stride-2 convolution, GroupNorm, ReLU and the max pooling (reference resnet.py:139-140) as the library runs them."""
        return F.max_pool2d(F.relu(self.bn1(self.conv1(x)), inplace=True), 3, stride=2, padding=1)

    def stem_hip(self, x):
        """``stem`` at inference on ``ops.stem_conv`` / ``ops.group_norm_affine`` / ``ops.stem_pool``: the raw convolution is written
        once, its GroupNorm is a per (image, channel) affine that the pooling applies with the ReLU as it reads -- the normalised map
        is never written.  The same function of the same parameters up to the summation order."""
        y = ops.stem_conv(x, self.conv1.weight)
        return ops.stem_pool(y, _gn_affine(y, self.bn1))

    def stem_train_hip(self, x):
        """``stem`` with gradients on ``ops.stem_train``: the calls of ``stem_hip`` and their bits, and a backward on the HIP kernels
        from the raw map alone.  x is data (it must not require grad)."""
        return ops.stem_train(x, self.conv1.weight, self.bn1.weight, self.bn1.bias, self.bn1.num_groups, self.bn1.eps)

    def stages(self, x):
        """``layer1`` .. ``layer4`` on the stem's output -> (f8, f16, f32)."""
        f8 = self.layer2(self.layer1(x))
        f16 = self.layer3(f8)
        return f8, f16, self.layer4(f16)

    def stages_hip(self, x):
        """``stages`` on the HIP kernels (``_Block.forward_hip``)."""
        maps = []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for block in layer:
                x = block.forward_hip(x)
            maps.append(x)
        return maps[1], maps[2], maps[3]

    def stages_train_hip(self, x, identity=True, projection=False):
        """``stages`` with gradients: the identity blocks (``identity``) and the projection blocks (``projection``) on
        ``_Block.forward_train_hip``, every other block the module it is."""
        maps = []
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for block in layer:
                hip = (identity and block.is_identity) or (projection and block.is_projection)
                x = block.forward_train_hip(x) if hip else block(x)
            maps.append(x)
        return maps[1], maps[2], maps[3]

    def forward(self, x):
        return self.stages(self.stem(x))

    def forward_hip(self, x):
        """``forward`` with the residual stages on the HIP kernels; the stem is the library's."""
        return self.stages_hip(self.stem(x))


_DEPTHS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}


def _head(cout):
    return nn.Sequential(nn.Conv2d(256, 256, 3, padding=1), _gn(256), nn.ReLU(True),
                         nn.Conv2d(256, cout, 3, padding=1, bias=False))


class VFANet(nn.Module):
    def __init__(self, args, base="resnet18", grid_height=160, cube_size=(25, 25, 32), angle_range=360, mode="3D",
                 pretrained=False, view_reduce="sum"):
        super().__init__()
        assert base in _DEPTHS, f"Unrecognized model, expect `resnet18` or `resnet34`, got {base}."
        assert mode in ("2D", "3D"), f"mode error, expect `2D` or `3D`, got{mode}"
        self.mode = mode
        self.view_reduce = check_view_reduce(view_reduce)
        self.head_convs = "library"  # or "hip" (``heads``); a plain attribute like ``view_reduce``: no ``state_dict`` key
        self.head_convs_train = "library"  # or "hip" (``heads``, with gradients); the same kind of attribute
        self.trunk_convs = "library"  # or "hip" (``trunk``); the same kind of attribute
        self.trunk_stem = "library"  # or "hip" (``trunk``); the same kind of attribute, independent of ``trunk_convs``
        self.trunk_convs_train = "library"  # or "hip" (``trunk``, with gradients); the same kind of attribute, independent of both
        self.trunk_proj_train = "library"  # or "hip" (``trunk``, with gradients: the projection blocks); independent of the three
        self.trunk_stem_train = "library"  # or "hip" (``trunk``, with gradients: the stem); independent of the five
        self.input_size = getattr(args, "resize_size", None)  # (H, W) uint8 frames are resized to (train.py:209-214); None: as they are
        self.base = _Trunk(_DEPTHS[base])
        if pretrained:
            load_pretrained_trunk(self.base, base)
        for s in (8, 16, 32):
            setattr(self, f"vfa{s}", VFA(channel=256, grid_height=grid_height, cube_size=cube_size, feat_scale=1. / s,
                                         args=args))
        self.register_buffer("mean", torch.tensor([0.485, 0.456, 0.406]))
        self.register_buffer("std", torch.tensor([0.229, 0.224, 0.225]))
        self.lat8, self.lat16, self.lat32 = nn.Conv2d(128, 256, 1), nn.Conv2d(256, 256, 1), nn.Conv2d(512, 256, 1)
        self.bn8, self.bn16, self.bn32 = _gn(256), _gn(256), _gn(256)
        self.fuse = nn.Sequential(nn.Conv2d(256, 256, 3, padding=1), nn.BatchNorm2d(256), nn.ReLU(True),
                                  nn.Conv2d(256, 256, 3, padding=2, dilation=2), nn.BatchNorm2d(256), nn.ReLU(True))
        self.map_classifier = nn.Sequential(nn.Conv2d(256, 1, 3, padding=4, dilation=4, bias=False))
        self.tytx_pred = _head(2)
        if mode == "3D":
            self.orient_pred = nn.Sequential(nn.Conv2d(256, angle_range, 3, padding=4, dilation=4, bias=False))
            self.thtwtl_pred = _head(3)

    def normalized(self, images):
        """The trunk's input (reference vfanet.py:59).  Float images (n,3,iH,iW), resized and scaled to [0, 1] by the caller as the
        reference's dataset does: ``(images - mean) / std``.  uint8 frames (n,H,W,3) as the cameras deliver them (``pack_frames``):
        the reference's resize to ``input_size``, ``ToTensor`` and the normalisation in one HIP kernel (``ops.image_frontend``),
        the bits of the host chain."""
        if images.dtype == torch.uint8:
            return ops.image_frontend(images, size=self.input_size, mean=self.mean, std=self.std)
        return (images - self.mean.view(3, 1, 1)) / self.std.view(3, 1, 1)

    def _empty(self, images, h, w):
        """The (0,256,h,w) map of no cameras or no frames, float like the images (uint8 frames: like the model)."""
        return (images if images.is_floating_point() else self.mean).new_zeros(0, 256, h, w)

    def trunk(self, x):
        """The normalised images (n,3,iH,iW) -> the trunk's maps (f8, f16, f32), contiguous NCHW float32.  Two independent settings:
        ``trunk_stem`` names who runs the stem (``"hip"``: the kernels of ``csrc/vfa_stem.hip``, ``_Trunk.stem_hip``) and
        ``trunk_convs`` who runs ``layer1`` .. ``layer4`` (``"hip"``: the kernels of ``csrc/vfa_trunk.hip``, ``_Trunk.stages_hip``).
        ``"hip"`` holds where the model is in eval mode, gradients are off and ``x`` is a float32 CUDA tensor with at least one image;
        anywhere else, and with both settings on ``"library"``, this is ``self.base(x)``.
        ``trunk_convs_train`` names who runs the identity residual blocks where gradients are enabled (``"hip"``: the kernels of
        ``csrc/vfa_trunk_grad.hip``, ``_Trunk.stages_train_hip``; the stem and the projection blocks run as modules): it holds where
        gradients are enabled and ``x`` is a float32 CUDA tensor with at least one image, in training and in eval mode alike.
        ``trunk_proj_train`` names who runs the three projection blocks (the first of ``layer2`` .. ``layer4``) under the same
        conditions (``"hip"``: ``ops.projection_block_train``), and ``trunk_stem_train`` who runs the stem under them (``"hip"``:
        ``ops.stem_train``, ``_Trunk.stem_train_hip``) -- with one further condition, that ``x`` does not require grad: the images are
        data, and an input that does takes the module stem.  The training branch is taken when any of the three is ``"hip"``; with
        all three no library convolution, normalisation or pooling runs in the trunk, forward or backward; with the stem's switch
        on ``"library"`` the stem runs as a module."""
        if self.trunk_convs not in TRUNK_CONVS:
            raise ValueError(f"VFANet.trunk: trunk_convs is one of {TRUNK_CONVS}, got {self.trunk_convs!r}")
        if self.trunk_stem not in TRUNK_STEM:
            raise ValueError(f"VFANet.trunk: trunk_stem is one of {TRUNK_STEM}, got {self.trunk_stem!r}")
        if self.trunk_convs_train not in TRUNK_CONVS_TRAIN:
            raise ValueError(f"VFANet.trunk: trunk_convs_train is one of {TRUNK_CONVS_TRAIN}, got {self.trunk_convs_train!r}")
        if ("hip" in (self.trunk_convs, self.trunk_stem) and not self.training and not torch.is_grad_enabled() and x.is_cuda
                and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
            y = self.base.stem_hip(x) if self.trunk_stem == "hip" else self.base.stem(x)
            return self.base.stages_hip(y) if self.trunk_convs == "hip" else self.base.stages(y)
        if self.trunk_proj_train not in TRUNK_PROJ_TRAIN:
            raise ValueError(f"VFANet.trunk: trunk_proj_train is one of {TRUNK_PROJ_TRAIN}, got {self.trunk_proj_train!r}")
        if self.trunk_stem_train not in TRUNK_STEM_TRAIN:
            raise ValueError(f"VFANet.trunk: trunk_stem_train is one of {TRUNK_STEM_TRAIN}, got {self.trunk_stem_train!r}")
        if ("hip" in (self.trunk_convs_train, self.trunk_proj_train, self.trunk_stem_train) and torch.is_grad_enabled() and x.is_cuda
                and x.dtype == torch.float32 and x.dim() == 4 and x.numel() > 0):
            y = self.base.stem_train_hip(x) if self.trunk_stem_train == "hip" and not x.requires_grad else self.base.stem(x)
            if "hip" not in (self.trunk_convs_train, self.trunk_proj_train):
                return self.base.stages(y)
            return self.base.stages_train_hip(y, self.trunk_convs_train == "hip", self.trunk_proj_train == "hip")
        return self.base(x)

    def laterals(self, images):
        """images (n,3,iH,iW), or uint8 (n,H,W,3), -> the three (n,256,h,w) non-negative lateral maps (reference vfanet.py:59-62, 72-74)."""
        x = self.normalized(images)
        f8, f16, f32 = self.trunk(x)
        return (F.relu(self.bn8(self.lat8(f8))), F.relu(self.bn16(self.lat16(f16))), F.relu(self.bn32(self.lat32(f32))))

    def lateral_integrals(self, images):
        """images (n,3,iH,iW), or uint8 (n,H,W,3), -> the three zero-bordered channels-last integral images of the lateral maps, without
        materialising those maps (reference vfanet.py:72-74 + vfa_op.py:110, 172-173).  ONE hand-written kernel for the three
        1x1 convolutions (``ops.lateral_convs``: six bf16 MFMA products of a three-piece split, channels-last output, GroupNorm
        statistics in its epilogue) + a tiny statistics kernel; then one launch pair for the three integral images, whose row scan applies the
        GroupNorm affine and the ReLU (``vfa_integral_images_hwc_f32``).  No NCHW lateral tensor exists.
        With gradients enabled the same kernels run inside one autograd node (``vfa_op._LateralIntegrals``) whose backward goes from
        d integral straight to the trunk maps and the lat* / bn* parameters on HIP kernels."""
        x = self.normalized(images)
        if torch.is_grad_enabled():
            return vfa_op.lateral_integrals_train(self.trunk(x), (self.lat8, self.lat16, self.lat32), (self.bn8, self.bn16, self.bn32))
        parts = ops.lateral_convs([(feat, conv.weight, conv.bias, gn.weight, gn.bias, gn.eps) for feat, conv, gn in
                                   zip(self.trunk(x), (self.lat8, self.lat16, self.lat32), (self.bn8, self.bn16, self.bn32))])
        return ops.integral_images([p[0] for p in parts], [p[1] for p in parts], [p[2] for p in parts], channels_last=True)

    def ortho_features(self, images, calibs, grid, distributed=False):
        """The fused BEV map (1,256,L,W) entering the heads (reference vfanet.py:64-82, 131).  images (B,N,3,iH,iW): a batch of B
        frames -> (B,256,L,W); with ONE rig (calibs (N,3,4)) in inference the whole batch is one launch of the pipelined kernel
        (``aggregate_views(..., frames=B)``), otherwise -- calibs (B,N,3,4), gradients, distributed -- frame by frame.
        uint8 camera frames (N,H,W,3) or (B,N,H,W,3) are taken in place of the float images (``normalized``)."""
        if images.dim() == 5:
            return self._ortho_frames(images, calibs, grid, distributed)
        if distributed:
            mine = camera_shard(images.shape[0])
            idx = torch.tensor(mine, dtype=torch.long, device=images.device)
            images, calibs = images[idx], calibs[idx]
        mods3 = [self.vfa8, self.vfa16, self.vfa32]
        if (FUSE_PRODUCER and self.view_reduce == "sum" and not torch.is_grad_enabled() and images.is_cuda and images.shape[0]
                and vfa_op.frame_route(mods3, images.shape[0]) in ("pipe", "fused")):
            return aggregate_views(self.vfa8, self.vfa16, self.vfa32, None, None, None, calibs, grid, (-1, 0.95),
                                   distributed=distributed, integrals=self.lateral_integrals(images))
        if self.producer_train_ok(images):
            return aggregate_views(self.vfa8, self.vfa16, self.vfa32, None, None, None, calibs, grid, (-1, 0.95),
                                   distributed=distributed, integrals=self.lateral_integrals(images))
        lat8, lat16, lat32 = self.laterals(images) if images.shape[0] else (self._empty(images, 1, 1),) * 3
        return aggregate_views(self.vfa8, self.vfa16, self.vfa32, lat8, lat16, lat32, calibs, grid, (-1, 0.95),
                               distributed=distributed, view_reduce=self.view_reduce)

    def producer_train_ok(self, images):
        """Training routes through the differentiable producer (``FUSE_PRODUCER_TRAIN``): gradients on, sum mode, a CUDA batch of
        cameras with the lateral widths of the reference, and the fused frame kernels cover the modules."""
        mods3 = [self.vfa8, self.vfa16, self.vfa32]
        return (FUSE_PRODUCER_TRAIN and self.view_reduce == "sum" and torch.is_grad_enabled() and images.is_cuda
                and images.shape[0] > 0 and all(c.out_channels == 256 for c in (self.lat8, self.lat16, self.lat32))
                and vfa_op.producer_train_ok(mods3, images.shape[0]))

    def _ortho_frames(self, images, calibs, grid, distributed):
        B, N = images.shape[:2]
        if calibs.dim() == 4 and tuple(calibs.shape[:2]) != (B, N) or calibs.dim() == 3 and calibs.shape[0] != N:
            raise ValueError(f"VFANet: images {tuple(images.shape)} need calibs ({N},3,4) or ({B},{N},3,4), got {tuple(calibs.shape)}")
        mods3 = [self.vfa8, self.vfa16, self.vfa32]
        if (B == 0 or distributed or calibs.dim() == 4 or torch.is_grad_enabled() or self.view_reduce != "sum"
                or not (images.is_cuda and vfa_op.frame_route(mods3, N, frames=B) == "pipe_batch")):
            outs = [self.ortho_features(images[b], calibs[b] if calibs.dim() == 4 else calibs, grid, distributed) for b in range(B)]
            return torch.cat(outs, 0) if outs else self._empty(images, grid.shape[-3], grid.shape[-2])
        flat = images.reshape(B * N, *images.shape[2:])
        if FUSE_PRODUCER:
            return aggregate_views(self.vfa8, self.vfa16, self.vfa32, None, None, None, calibs, grid, (-1, 0.95),
                                   integrals=self.lateral_integrals(flat), frames=B)
        lat8, lat16, lat32 = self.laterals(flat)
        return aggregate_views(self.vfa8, self.vfa16, self.vfa32, lat8, lat16, lat32, calibs, grid, (-1, 0.95), frames=B)

    def forward(self, images, calibs, grid, visualize=False, visualize_ortho=False, distributed=False, rotation_at=None):
        """images (N,3,iH,iW), calibs (N,3,4), grid (1,L,W,3) -> dict like the reference (vfanet.py:141-149).
        images (B,N,3,iH,iW): a batch of B frames, calibs (N,3,4) or (B,N,3,4); the heads run at batch B.
        uint8 frames (N,H,W,3) / (B,N,H,W,3): the cameras' bytes, resized to ``input_size`` and normalised on the device.
        ``rotation_at``: evaluate the orientation head only where it is read (``heads``)."""
        if visualize or visualize_ortho:
            self._visualize(images, calibs, grid, boxes=visualize_ortho)
        topdown = self.ortho_features(images, calibs, grid, distributed)
        return self.heads(topdown, rotation_at)

    def detect(self, images, calibs, grid, decoder, cls_thresh):
        """Inference from images to ``BEVDecoder.decode_fused``'s detections without the dense orientation map: the heads with
        ``rotation_at="detections"``, then the decode, which evaluates ``orient_pred`` at the cells it selected."""
        with torch.no_grad():
            return decoder.decode_fused(self.forward(images, calibs, grid, rotation_at="detections"), cls_thresh)

    def _visualize(self, images, calibs, grid, boxes=False):
        """Slow matplotlib side path (reference vfanet.py:84-128): per camera, the norms of the three lateral maps, of
        that camera's BEV contribution and of the running fused map; ``boxes`` also draws the projected cubes
        (``VFA.visualize_cube``, reference vfa_op.py:90-101)."""
        import matplotlib.pyplot as plt
        with torch.no_grad():
            lats = self.laterals(images)
            fused = 0
            for cam in range(images.shape[0]):
                one = [l[cam:cam + 1] for l in lats]
                part = aggregate_views(self.vfa8, self.vfa16, self.vfa32, *one, calibs[cam:cam + 1], grid)
                fused = torch.maximum(fused, part) if (self.view_reduce == "max" and cam) else fused + part
                fig, axes = plt.subplots(1, 5, figsize=(15, 3))
                for ax, t, title in zip(axes, one + [part, fused], ("feat8", "feat16", "feat32", "ortho", "fused ortho")):
                    ax.imshow(torch.norm(t, dim=1)[0].cpu().numpy())
                    ax.set_title(f"C{cam + 1} {title}")
                    ax.axis("off")
                plt.show()
                plt.close(fig)
                if boxes:
                    self.vfa8.visualize_cube(one[0], calibs[cam], grid)

    def _hip_convs_ok(self, topdown):
        """``head_convs = "hip"`` covers inference on the reference's widths: eval mode, no gradients, a float32 CUDA map of 256
        channels, BatchNorm layers with running statistics.  Anything else runs the library path, as ``FUSE_PRODUCER`` does."""
        return (not self.training and not torch.is_grad_enabled() and topdown.is_cuda and topdown.dtype == torch.float32
                and topdown.dim() == 4 and topdown.shape[1] == 256 and topdown.numel() > 0
                and all(bn.running_mean is not None and not bn.training for bn in (self.fuse[1], self.fuse[4])))

    def _hip_head(self, topdown, head):
        """``Conv2d(256, 256, 3) -> GroupNorm -> ReLU -> Conv2d(256, cout, 3)`` (``_head``): the dense kernel with the bias as its
        epilogue, the GroupNorm statistics as a per (frame, channel) affine, and that affine with the ReLU as the prologue of the
        few-output kernel -- the normalised map is never written."""
        conv, gn, _, last = head
        y = ops.conv3x3(topdown, conv.weight, conv.dilation[0], shift=conv.bias)
        affine = ops.group_norm_affine(y, gn.num_groups, gn.weight, gn.bias, gn.eps)
        return ops.conv3x3_few(y, last.weight, last.dilation[0], affine=affine)

    def _hip_fuse(self, topdown):
        """``fuse`` with eval-mode BatchNorm, the bias and the ReLU folded into the dense kernel's epilogue."""
        x = topdown
        for conv, bn in ((self.fuse[0], self.fuse[1]), (self.fuse[3], self.fuse[4])):
            scale, shift = ops.bn_fold(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, conv.bias)
            x = ops.conv3x3(x, conv.weight, conv.dilation[0], scale=scale, shift=shift, relu=True)
        return x

    def _hip_train_ok(self, topdown):
        """``head_convs_train = "hip"`` covers what ``ops.conv3x3_train`` does: gradients enabled, a float32 CUDA map of 256
        channels.  Anything else runs the library path."""
        return (torch.is_grad_enabled() and topdown.is_cuda and topdown.dtype == torch.float32 and topdown.dim() == 4
                and topdown.shape[1] == 256 and topdown.numel() > 0)

    @staticmethod
    def _train_conv(conv, x):
        return ops.conv3x3_train(x, conv.weight, conv.bias, conv.dilation[0])

    def _train_fuse(self, topdown):
        """``fuse`` with its two convolutions on ``ops.conv3x3_train``; BatchNorm (training or eval mode) and ReLU as they are."""
        return self.fuse[4:](self._train_conv(self.fuse[3], self.fuse[1:3](self._train_conv(self.fuse[0], topdown))))

    def _train_head(self, topdown, head):
        """``_head`` with its 256 -> 256 convolution on ``ops.conv3x3_train``; GroupNorm, ReLU and the few-output layer as they are."""
        return head[1:](self._train_conv(head[0], topdown))

    def heads(self, topdown, rotation_at=None, convs=None):
        """The BEV heads on the fused map (reference vfanet.py:131-149).

        ``convs`` (``None``: the attribute ``head_convs``): ``"library"`` runs the dense convolutions of ``fuse``, ``map_classifier``,
        ``tytx_pred`` and ``thtwtl_pred`` as the modules they are; ``"hip"`` runs them at inference on ``ops.conv3x3`` /
        ``ops.conv3x3_few`` / ``ops.group_norm_affine`` -- the same function of the same parameters up to the summation order
         -- where ``_hip_convs_ok`` holds, and the library path otherwise.

        The attribute ``head_convs_train`` (``"library"`` or ``"hip"``) is the same choice where gradients are enabled: ``"hip"``
        runs ``fuse[0]``, ``fuse[3]``, ``tytx_pred[0]`` and ``thtwtl_pred[0]`` on ``ops.conv3x3_train`` where ``_hip_train_ok``
        holds -- differentiable, the same bits on every run -- and every other layer as the module it is.

        ``rotation_at`` (3D only, ``ValueError`` in 2D) evaluates ``orient_pred`` -- the largest layer of the heads, read at a few
        dozen cells -- only where it is read, on ``ops.conv3x3_at_cells`` instead of a dense convolution; the other heads are the
        same calls.  ``None``: the dense ``rotation (B, L, W, R)`` of the reference.  ``cells (B, k)`` int32, flat ``l * W + w``
        (training: the positive cells of the loss, in ascending order the order of ``pred['rotation'][mask]``; an entry outside the
        map is a row of zeros without gradient): ``rotation_at (B, k, R)`` logits and ``rotation_cells`` instead of ``rotation``,
        differentiable.  ``"detections"`` (inference): ``rotation_head = (fused feature, orient_pred weight, dilation)``, from which
        ``BEVDecoder.decode_fused`` takes the rotation at the cells it selects."""
        if rotation_at is not None and self.mode != "3D":
            raise ValueError("VFANet.heads: rotation_at needs mode 3D (a 2D model has no orientation head)")
        convs = self.head_convs if convs is None else convs
        if convs not in HEAD_CONVS:
            raise ValueError(f"VFANet.heads: convs is one of {HEAD_CONVS}, got {convs!r}")
        if self.head_convs_train not in HEAD_CONVS_TRAIN:
            raise ValueError(f"VFANet.heads: head_convs_train is one of {HEAD_CONVS_TRAIN}, got {self.head_convs_train!r}")
        hip = convs == "hip" and self._hip_convs_ok(topdown)
        train = self.head_convs_train == "hip" and self._hip_train_ok(topdown)  # (never both: ``hip`` needs gradients off)
        if hip:
            fused = self._hip_fuse(topdown)
            conv = self.map_classifier[0]
            out = {"heatmap": ops.conv3x3_few(fused, conv.weight, conv.dilation[0]),
                   "loc_offset": self._hip_head(topdown, self.tytx_pred).permute(0, 2, 3, 1)}
        elif train:
            fused = self._train_fuse(topdown)
            out = {"heatmap": self.map_classifier(fused), "loc_offset": self._train_head(topdown, self.tytx_pred).permute(0, 2, 3, 1)}
        else:
            fused = self.fuse(topdown)
            out = {"heatmap": self.map_classifier(fused), "loc_offset": self.tytx_pred(topdown).permute(0, 2, 3, 1)}
        if self.mode == "3D":
            dim = (self._hip_head(topdown, self.thtwtl_pred) if hip else self._train_head(topdown, self.thtwtl_pred) if train
                   else self.thtwtl_pred(topdown))
            out["dim_offset"] = dim.permute(0, 2, 3, 1)
            conv = self.orient_pred[0]
            if rotation_at is None:
                out["rotation"] = self.orient_pred(fused).permute(0, 2, 3, 1)
            elif isinstance(rotation_at, str):
                if rotation_at != "detections":
                    raise ValueError(f"VFANet.heads: rotation_at is None, 'detections' or cells (B, k), got {rotation_at!r}")
                out["rotation_head"] = (fused, conv.weight, conv.dilation[0])
            else:
                out["rotation_at"] = ops.conv3x3_at_cells(fused, conv.weight, rotation_at, dilation=conv.dilation[0])
                out["rotation_cells"] = rotation_at
        return out
