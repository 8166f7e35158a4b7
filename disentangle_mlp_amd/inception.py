"""Inception pool_3 feature extractor for FID on the device: the ``InceptionV3`` of
/root/reference/scoring/inception.py:16-160 with the FID patches of :163-310, forward only.

Contract kept from the reference: class name, constructor ``(output_blocks, resize_input, normalize_input,
requires_grad, use_fid_inception)``, ``BLOCK_INDEX_BY_DIM``, ``forward(inp in [0,1]) -> list of feature maps``, and the
weight file: a ``state_dict`` with torchvision's ``inception_v3`` names (``Conv2d_1a_3x3.conv.weight``,
``Mixed_5b.branch1x1.bn.running_mean``, ..., ``fc.weight``) -- the ``pt_inception-2015-12-05`` file the reference
downloads (scoring/inception.py:13).  There is no network here: pass ``weights=`` (a path or a state_dict); without
weights the constructor raises, it never runs on random parameters silently.

Device path (MI355X): every convolution runs on this package's general fp16x3 implicit-GEMM kernel
(csrc/conv_general.hip, ``ops.conv2d_bias_act``): the eval-mode BatchNorm (eps = 0.001) is folded into the filter and a
bias once at load time, the folded filter is packed once (scaled by its bound, split into fp16 planes), the activations
are gathered from NCHW while they are staged -- no im2col matrix exists in HBM -- and bias + ReLU are applied on the
accumulators.  The branches of a block write their channels straight into the block's concatenated output (no
``torch.cat``).  Bounds for the fp16 scaling: one ``vg_absmax`` pass over the network input; every convolution leaves
max |y| for its consumer; pooled tensors inherit their input's bound (|avg|, |max| <= max |x|); no host reads.
The bilinear resize of ``InceptionV3.forward`` stays on ATen; its pooling and its final average run on ATen by default
and on this package's kernels (csrc/fid_front.hip) under ``VG_INCEPTION_POOL=hip`` (or ``inception.POOL_LOWERING = "hip"``): every
3x3 pooling through ``vg_pool3x3`` -- a pooling branch without convolution writes its slice of the block's output
itself and adds its true max |out| to the block's bound, so neither ``out[:, off:].copy_(pooled)`` nor
``slot.copy_(torch.maximum(...))`` is launched -- and the final average through ``vg_global_avg_pool``.
``InceptionFeatureExtractor.features_u8`` (device uint8 images, what ``ops.quantize_each_u8`` makes of the decoder's
output) always takes those kernels, and ``vg_resize_bilinear_u8`` in front of them: resize, / 255, 2 x - 1 and the
network input's bound in one launch -- no ``F.interpolate``, no ``vg_absmax`` pass, no ``torch.cat``, no host read.

CPU tensors, and device tensors under ``VG_INCEPTION_CONV=unfold`` (or ``inception.CONV_LOWERING = "unfold"``), take
the earlier lowering: every convolution as ONE fp32 GEMM -- 1x1 convolutions directly, the others through ``F.unfold``
(im2col) -- with the same folded weights and the ReLU applied in place.  It is what the kernel path is measured against.

**Parity unpinned**: the pretrained weights and the reference's ``fid_stats_celeba.npz`` are not obtainable offline,
so absolute FID values cannot be compared; the architecture arithmetic is checked against the CPU oracle
(oracle/inception.py) on seeded random weights (tests/test_inception.py).
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

# Lowering of the convolutions for DEVICE tensors: "hip" (the default: csrc/conv_general.hip) or "unfold" (im2col + fp32
# GEMM, what CPU tensors always take).  Set here, or with VG_INCEPTION_CONV in the environment.
CONV_LOWERING = os.environ.get("VG_INCEPTION_CONV", "hip")
if CONV_LOWERING not in ("hip", "unfold"):
    raise ImportError(f"VG_INCEPTION_CONV={CONV_LOWERING!r}: expected 'hip' or 'unfold'")


# Lowering of the pooling layers on the device path of ``InceptionV3.forward``: "aten" (the default: what it has always
# launched) or "hip" (csrc/fid_front.hip).  Set here, or with VG_INCEPTION_POOL.  `features_u8` always takes "hip".
POOL_LOWERING = os.environ.get("VG_INCEPTION_POOL", "aten")
if POOL_LOWERING not in ("aten", "hip"):
    raise ImportError(f"VG_INCEPTION_POOL={POOL_LOWERING!r}: expected 'aten' or 'hip'")
_force_hip_pool = False       # raised by `features_u8` around its network runs


def _hip(x):
    return x.is_cuda and CONV_LOWERING == "hip"


def _hip_pool(x):
    return _hip(x) and (_force_hip_pool or POOL_LOWERING == "hip")


def _ops():
    from . import ops            # loads libvaegan_hip.so: only the device path needs it
    return ops


def _pool3(x, mode, stride, padding):
    """The 3x3 "max" / "avg" (padding not counted: Tensorflow's average pool, scoring/inception.py:203-205) pooling.  On
    ATen the result inherits x's bound (|avg|, |max| <= max |x|); the HIP kernel leaves the true one."""
    if _hip_pool(x):
        return _ops().pool3x3(x, stride, padding, mode)
    if mode == "max":
        p = F.max_pool2d(x, kernel_size=3, stride=stride, padding=padding)
    else:
        p = F.avg_pool2d(x, kernel_size=3, stride=stride, padding=padding, count_include_pad=False)
    if _hip(x):
        _ops().set_amax(p, _ops().amax_of(x))
    return p


def _block_out(x, channels, oh, ow):
    """The concatenated output of a block and the one bound slot its branches add their maxima into."""
    return torch.empty((x.shape[0], channels, oh, ow), dtype=torch.float32, device=x.device), _ops().new_amax_slot(x.device)


def _max_pool_branch(x, out, offset, slot):
    """The 3x3 / stride 2 max-pooling branch of blocks B and D (no convolution behind it) into its slice of ``out``.  HIP:
    the kernel writes the slice and adds max |pooled| to the block's bound; ATen: copied, the bound covers x's."""
    if _hip_pool(x):
        _ops().pool3x3(x, 2, 0, "max", out, offset, slot)
        return
    pooled = F.max_pool2d(x, kernel_size=3, stride=2)
    slot.copy_(torch.maximum(slot, _ops().amax_of(x)))
    out[:, offset:offset + pooled.shape[1]].copy_(pooled)


class _ConvBN(nn.Module):
    """BasicConv2d parameters (conv without bias + BatchNorm2d(eps=0.001)); forward = folded GEMM + ReLU."""

    def __init__(self, cin, cout, kernel_size, stride=1, padding=0):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, kernel_size, stride=stride, padding=padding, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=0.001)
        self._folded = self._packed = None

    def _load_from_state_dict(self, *a, **k):
        self._folded = self._packed = None
        return super()._load_from_state_dict(*a, **k)

    def _apply(self, fn, *a, **k):
        self._folded = self._packed = None       # .to(device) / .float(): re-fold and re-pack on first use
        return super()._apply(fn, *a, **k)

    def folded(self):
        if self._folded is None:
            with torch.no_grad():
                s = self.bn.weight / torch.sqrt(self.bn.running_var + self.bn.eps)
                w = (self.conv.weight * s.view(-1, 1, 1, 1)).reshape(self.conv.out_channels, -1).contiguous()
                b = (self.bn.bias - self.bn.running_mean * s).contiguous()
            self._folded = (w, b)
        return self._folded

    def packed(self):
        if self._packed is None:
            w, _ = self.folded()
            with torch.no_grad():
                self._packed = _ops().conv_general_pack(w.view(self.conv.weight.shape), self.conv.stride, self.conv.padding)
        return self._packed

    def forward(self, x, out=None, offset=0, slot=None):
        """``out`` / ``offset`` / ``slot`` (device path only): write into channels [offset, offset + cout) of a block's
        output and add max |y| into the block's bound slot."""
        if _hip(x):
            packed, meta = self.packed()
            return _ops().conv2d_bias_act(x, packed, meta, self.folded()[1], out, offset, True, slot)
        w, b = self.folded()
        B, C, H, W = x.shape
        kh, kw = self.conv.kernel_size
        sh, sw = self.conv.stride
        ph, pw = self.conv.padding
        OH, OW = (H + 2 * ph - kh) // sh + 1, (W + 2 * pw - kw) // sw + 1
        if (kh, kw, sh, sw, ph, pw) == (1, 1, 1, 1, 0, 0):
            cols = x.reshape(B, C, H * W)
        else:
            cols = F.unfold(x, (kh, kw), padding=(ph, pw), stride=(sh, sw))        # (B, C*kh*kw, OH*OW)
        y = torch.baddbmm(b.view(1, -1, 1), w.unsqueeze(0).expand(B, -1, -1), cols)
        return torch.relu_(y).view(B, -1, OH, OW)


def _avg3(x):
    return _pool3(x, "avg", 1, 1)


class _A(nn.Module):        # FIDInceptionA
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = _ConvBN(cin, 64, 1)
        self.branch5x5_1 = _ConvBN(cin, 48, 1)
        self.branch5x5_2 = _ConvBN(48, 64, 5, padding=2)
        self.branch3x3dbl_1 = _ConvBN(cin, 64, 1)
        self.branch3x3dbl_2 = _ConvBN(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = _ConvBN(96, 96, 3, padding=1)
        self.branch_pool = _ConvBN(cin, pool_features, 1)

    def forward(self, x):
        if _hip(x):
            out, slot = _block_out(x, 224 + self.branch_pool.conv.out_channels, x.shape[2], x.shape[3])
            self.branch1x1(x, out, 0, slot)
            self.branch5x5_2(self.branch5x5_1(x), out, 64, slot)
            self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)), out, 128, slot)
            self.branch_pool(_avg3(x), out, 224, slot)
            _ops().set_amax(out, slot)
            return out
        return torch.cat([self.branch1x1(x), self.branch5x5_2(self.branch5x5_1(x)),
                          self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          self.branch_pool(_avg3(x))], 1)


class _B(nn.Module):        # torchvision InceptionB
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = _ConvBN(cin, 384, 3, stride=2)
        self.branch3x3dbl_1 = _ConvBN(cin, 64, 1)
        self.branch3x3dbl_2 = _ConvBN(64, 96, 3, padding=1)
        self.branch3x3dbl_3 = _ConvBN(96, 96, 3, stride=2)

    def forward(self, x):
        if _hip(x):
            out, slot = _block_out(x, 480 + x.shape[1], (x.shape[2] - 3) // 2 + 1, (x.shape[3] - 3) // 2 + 1)
            self.branch3x3(x, out, 0, slot)
            self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)), out, 384, slot)
            _max_pool_branch(x, out, 480, slot)
            _ops().set_amax(out, slot)
            return out
        return torch.cat([self.branch3x3(x), self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x))),
                          F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class _C(nn.Module):        # FIDInceptionC
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = _ConvBN(cin, 192, 1)
        self.branch7x7_1 = _ConvBN(cin, c7, 1)
        self.branch7x7_2 = _ConvBN(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7_3 = _ConvBN(c7, 192, (7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = _ConvBN(cin, c7, 1)
        self.branch7x7dbl_2 = _ConvBN(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = _ConvBN(c7, c7, (1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = _ConvBN(c7, c7, (7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = _ConvBN(c7, 192, (1, 7), padding=(0, 3))
        self.branch_pool = _ConvBN(cin, 192, 1)

    def forward(self, x):
        if _hip(x):
            out, slot = _block_out(x, 768, x.shape[2], x.shape[3])
            self.branch1x1(x, out, 0, slot)
            self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)), out, 192, slot)
            t = self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x))))
            self.branch7x7dbl_5(t, out, 384, slot)
            self.branch_pool(_avg3(x), out, 576, slot)
            _ops().set_amax(out, slot)
            return out
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_5(self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))))
        return torch.cat([self.branch1x1(x), b7, bd, self.branch_pool(_avg3(x))], 1)


class _D(nn.Module):        # torchvision InceptionD
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = _ConvBN(cin, 192, 1)
        self.branch3x3_2 = _ConvBN(192, 320, 3, stride=2)
        self.branch7x7x3_1 = _ConvBN(cin, 192, 1)
        self.branch7x7x3_2 = _ConvBN(192, 192, (1, 7), padding=(0, 3))
        self.branch7x7x3_3 = _ConvBN(192, 192, (7, 1), padding=(3, 0))
        self.branch7x7x3_4 = _ConvBN(192, 192, 3, stride=2)

    def forward(self, x):
        if _hip(x):
            out, slot = _block_out(x, 512 + x.shape[1], (x.shape[2] - 3) // 2 + 1, (x.shape[3] - 3) // 2 + 1)
            self.branch3x3_2(self.branch3x3_1(x), out, 0, slot)
            self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))), out, 320, slot)
            _max_pool_branch(x, out, 512, slot)
            _ops().set_amax(out, slot)
            return out
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([self.branch3x3_2(self.branch3x3_1(x)), b7, F.max_pool2d(x, kernel_size=3, stride=2)], 1)


class _E(nn.Module):        # FIDInceptionE_1 (avg) / FIDInceptionE_2 (max: scoring/inception.py:299-303)
    def __init__(self, cin, pool):
        super().__init__()
        self.pool = pool
        self.branch1x1 = _ConvBN(cin, 320, 1)
        self.branch3x3_1 = _ConvBN(cin, 384, 1)
        self.branch3x3_2a = _ConvBN(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3_2b = _ConvBN(384, 384, (3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = _ConvBN(cin, 448, 1)
        self.branch3x3dbl_2 = _ConvBN(448, 384, 3, padding=1)
        self.branch3x3dbl_3a = _ConvBN(384, 384, (1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = _ConvBN(384, 384, (3, 1), padding=(1, 0))
        self.branch_pool = _ConvBN(cin, 192, 1)

    def _pool(self, x):
        return _pool3(x, self.pool, 1, 1)

    def forward(self, x):
        if _hip(x):
            out, slot = _block_out(x, 2048, x.shape[2], x.shape[3])
            self.branch1x1(x, out, 0, slot)
            t = self.branch3x3_1(x)
            self.branch3x3_2a(t, out, 320, slot)
            self.branch3x3_2b(t, out, 704, slot)
            t = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
            self.branch3x3dbl_3a(t, out, 1088, slot)
            self.branch3x3dbl_3b(t, out, 1472, slot)
            self.branch_pool(self._pool(x), out, 1856, slot)
            _ops().set_amax(out, slot)
            return out
        t = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(t), self.branch3x3_2b(t)], 1)
        t = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(t), self.branch3x3dbl_3b(t)], 1)
        return torch.cat([self.branch1x1(x), b3, bd, self.branch_pool(self._pool(x))], 1)


class _FidInception(nn.Module):
    """``fid_inception_v3()`` of scoring/inception.py:163-185 (the module tree whose state_dict is the weight file)."""

    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = _ConvBN(3, 32, 3, stride=2)
        self.Conv2d_2a_3x3 = _ConvBN(32, 32, 3)
        self.Conv2d_2b_3x3 = _ConvBN(32, 64, 3, padding=1)
        self.Conv2d_3b_1x1 = _ConvBN(64, 80, 1)
        self.Conv2d_4a_3x3 = _ConvBN(80, 192, 3)
        self.Mixed_5b, self.Mixed_5c, self.Mixed_5d = _A(192, 32), _A(256, 64), _A(288, 64)
        self.Mixed_6a = _B(288)
        self.Mixed_6b, self.Mixed_6c, self.Mixed_6d, self.Mixed_6e = _C(768, 128), _C(768, 160), _C(768, 160), _C(768, 192)
        self.Mixed_7a = _D(768)
        self.Mixed_7b, self.Mixed_7c = _E(1280, "avg"), _E(2048, "max")
        self.fc = nn.Linear(2048, 1008)          # in the weight file; not used for pool_3 features


class InceptionV3(nn.Module):
    """scoring/inception.py:16-160."""

    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks=(DEFAULT_BLOCK_INDEX,), resize_input=True, normalize_input=True, requires_grad=False,
                 use_fid_inception=True, weights=None):
        super().__init__()
        if not use_fid_inception:
            raise NotImplementedError("only the FID Inception (use_fid_inception=True) is part of the reference's path")
        if weights is None:
            raise RuntimeError(
                "InceptionV3 needs the pt_inception-2015-12-05 state_dict (scoring/inception.py:13): it cannot be "
                "downloaded here -- pass weights=<path to the .pth file or a state_dict>")
        self.resize_input, self.normalize_input = resize_input, normalize_input
        self.output_blocks = sorted(output_blocks)
        self.last_needed_block = max(output_blocks)
        assert self.last_needed_block <= 3, "Last possible output block index is 3"
        net = _FidInception()
        sd = torch.load(weights, map_location="cpu") if isinstance(weights, (str, bytes)) or hasattr(weights, "__fspath__") \
            else weights
        net.load_state_dict(sd)                   # strict: a wrong file fails loudly
        self.net = net.eval()
        for p in self.parameters():
            p.requires_grad = requires_grad

    def forward(self, inp):
        """inp (B,3,H,W) in [0,1] -> list of the requested blocks' feature maps (ascending block index)."""
        x = inp
        if self.resize_input:
            x = F.interpolate(x, size=(299, 299), mode="bilinear", align_corners=False)
        if self.normalize_input:
            x = 2 * x - 1
        if _hip(x):
            x = x.float().contiguous()
            _ops().amax_of(x)                       # the one explicit bound pass; every later bound comes from a producer
        return self._blocks(x)

    def _blocks(self, x, pool3_out=None):
        """The network behind resize + normalisation (a device input under the "hip" lowering carries its bound).
        ``pool3_out`` (HIP pooling only): the [B,2048] rows the final average is written to."""
        n, outp = self.net, []

        def pool2(t):
            return _pool3(t, "max", 2, 0)

        def mean(t):
            if _hip_pool(t):
                return _ops().global_avg_pool(t, pool3_out).view(t.shape[0], t.shape[1], 1, 1)
            return F.adaptive_avg_pool2d(t, (1, 1))

        stages = (
            lambda t: pool2(n.Conv2d_2b_3x3(n.Conv2d_2a_3x3(n.Conv2d_1a_3x3(t)))),
            lambda t: pool2(n.Conv2d_4a_3x3(n.Conv2d_3b_1x1(t))),
            lambda t: n.Mixed_6e(n.Mixed_6d(n.Mixed_6c(n.Mixed_6b(n.Mixed_6a(n.Mixed_5d(n.Mixed_5c(n.Mixed_5b(t)))))))),
            lambda t: mean(n.Mixed_7c(n.Mixed_7b(n.Mixed_7a(t)))),
        )
        for idx, stage in enumerate(stages):
            x = stage(x)
            if idx in self.output_blocks:
                outp.append(x)
            if idx == self.last_needed_block:
                break
        return outp


class InceptionFeatureExtractor:
    """``feature_extractor`` of fid.get_fid: images [n,h,w,3] with values 0..255 (what fid.py:68-105 feeds the
    network) -> pool_3 activations [n,2048], on the device, in chunks of ``batch_size``."""

    def __init__(self, weights, device="cuda", batch_size=50):
        self.device = torch.device(device)
        self.model = InceptionV3([InceptionV3.DEFAULT_BLOCK_INDEX], weights=weights).to(self.device)
        self.batch_size = int(batch_size)

    @torch.no_grad()
    def __call__(self, images):
        x = torch.as_tensor(images)
        outs = []
        for s in range(0, x.shape[0], self.batch_size):
            xb = x[s:s + self.batch_size].to(self.device, torch.float32).permute(0, 3, 1, 2).contiguous() / 255.0
            outs.append(self.model(xb)[0].reshape(xb.shape[0], -1))
        return torch.cat(outs)

    @torch.no_grad()
    def features_u8(self, images_u8):
        """Device uint8 images [n,h,w,3] (``ops.quantize_each_u8`` of the decoder's output) -> pool_3 activations
        [n,2048] fp32 on the device, in chunks of ``batch_size`` (the last one may be shorter).  Always on this
        package's kernels: ``vg_resize_bilinear_u8`` (resize to 299 x 299, / 255, 2 x - 1 and the input's bound), the
        convolutions, every pooling through ``vg_pool3x3``, ``vg_global_avg_pool``; no host read."""
        global _force_hip_pool
        if not (isinstance(images_u8, torch.Tensor) and images_u8.is_cuda and images_u8.dtype == torch.uint8
                and images_u8.dim() == 4 and images_u8.shape[3] == 3):
            raise RuntimeError("features_u8: expected a CUDA/ROCm uint8 [n,h,w,3] tensor (no CPU fallback)")
        if CONV_LOWERING != "hip":
            raise RuntimeError(f"features_u8 runs on the HIP kernels only (VG_INCEPTION_CONV={CONV_LOWERING!r})")
        m = self.model
        if not (m.resize_input and m.normalize_input):
            raise RuntimeError("features_u8: the network must resize and normalise its input (the FID configuration)")
        images_u8 = images_u8.contiguous()
        feats = torch.empty((images_u8.shape[0], 2048), dtype=torch.float32, device=images_u8.device)
        prev, _force_hip_pool = _force_hip_pool, True
        try:
            for s in range(0, images_u8.shape[0], self.batch_size):
                x = _ops().resize_bilinear_u8(images_u8[s:s + self.batch_size], (299, 299), 2.0, -1.0)
                m._blocks(x, feats[s:s + self.batch_size])
        finally:
            _force_hip_pool = prev
        return feats
