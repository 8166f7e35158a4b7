"""Drop-in module API of the reference's CelebA model zoo, computed on MI355X by
the HIP library.

Same class names, constructor signatures ``(opt[, representation_size=64])``,
method names, return orders / shapes and ``state_dict`` keys as
/root/reference/models/model.py:
    weights_init            model.py:8-14
    Encoder_celeba          model.py:282-328
    Generator_celeba        model.py:331-378
    Discriminator_celeba    model.py:381-416
    VAE                     model.py:419-571
so a reference checkpoint loads here and vice versa.  Layers are thin
subclasses of the torch layer classes (they only hold parameters / buffers and
keep ``weights_init``'s class-name matching and the seed -> weights recipe
bit-identical); their ``forward`` runs the hand-written kernels.  The 5x5
convolutions, BatchNorm+activation, reparameterisation, tanh / LeakyReLU /
sigmoid epilogues are HIP; the Linear GEMMs go to hipBLASLt through
``torch.nn.functional.linear``.

There is no CPU path: calling a module with CPU tensors raises.

Eval mode (BatchNorm on its running statistics) is opt-in per network: `enable_eval` / `eval_mode`.  A network that
was not opted in still refuses ``.eval()``, as it always has.
"""
import contextlib

import torch
from torch import nn
import torch.nn.functional as tF

from . import functional as F
from . import ops


def weights_init(m):
    """model.py:8-14 (class-name substring match; works on the Hip* layers too)."""
    name = type(m).__name__
    if "Conv" in name:
        nn.init.normal_(m.weight.data, 0.0, 0.02)
    elif "BatchNorm" in name:
        nn.init.normal_(m.weight.data, 1.0, 0.02)
        nn.init.constant_(m.bias.data, 0)


# --------------------------------------------------------------------- layers
class HipConv2d(nn.Conv2d):
    """5x5 / pad 2 / stride 1|2 convolution.  ``bn_shadowed``: the bias feeds a train-mode
    BatchNorm, so its gradient is analytically zero and is returned as exact zeros (`_bias_mode`: unless that
    BatchNorm runs on its running statistics)."""
    _next_bn = ()

    def __init__(self, cin, cout, stride, bn_shadowed=True):
        super().__init__(cin, cout, 5, stride=stride, padding=2)
        self.bn_shadowed = bn_shadowed

    def forward(self, x):
        mode = _bias_mode(self)
        return F.conv5x5(x.contiguous(), self.weight, self.bias, self.stride[0], mode)


class HipConvTranspose2d(nn.ConvTranspose2d):
    """5x5 / pad 2 / stride 1|2 transposed convolution producing exactly stride*input."""
    _next_bn = ()

    def __init__(self, cin, cout, stride, bn_shadowed=True):
        super().__init__(cin, cout, 5, stride=stride, padding=2)
        self.bn_shadowed = bn_shadowed

    def forward(self, x, output_size=None):
        s = self.stride[0]
        if output_size is not None:
            want = tuple(output_size)[-2:]
            if want != (x.shape[2] * s, x.shape[3] * s):
                raise ValueError(f"requested output size {want} is not stride*input "
                                 f"{(x.shape[2] * s, x.shape[3] * s)}")
        mode = _bias_mode(self)
        return F.conv_transpose5x5(x.contiguous(), self.weight, self.bias, s, mode)


class _HipBatchNormMixin:
    """Batch norm fused with the following activation.  Training: batch statistics, the reference's only path (it never
    calls .eval()).  Not training: the running statistics -- for a module that
    `enable_eval` marked (``eval_enabled``, a plain attribute: no buffer, not in the state_dict); an unmarked module
    rejects eval mode rather than silently approximating it.  Each BatchNorm decides by its own flags."""
    act = ops.ACT_NONE
    eval_enabled = False

    def _init_pending(self):
        self._nbt_pending = 0
        self.register_state_dict_pre_hook(_flush_nbt)

    def _note_forward(self):
        """True: this forward normalises with batch statistics (and is counted); False: with the running statistics
        (nothing of the module moves)."""
        if not self.training:
            if not self.eval_enabled:
                raise RuntimeError("HipBatchNorm: eval-mode (running-statistics) normalisation is not part of the "
                                   "reference's path and is opt-in: call model.enable_eval(net) (or use "
                                   "model.eval_mode(net)) before net.eval()")
            return False
        self._nbt_pending += 1     # num_batches_tracked, materialised lazily (no launch per call)
        return True

    def forward(self, x, stats=None):
        """``stats``: statistics slots left by the producing convolution (skips the statistics pass)."""
        if not self._note_forward():
            # materialised: the normalise pass emits the exact bound of its output, the slots are not needed
            return F.batch_norm_eval_act(x.contiguous(), self.weight, self.bias, self.running_mean, self.running_var,
                                         self.eps, self.act)
        return F.batch_norm_act(x.contiguous(), self.weight, self.bias, self.running_mean, self.running_var,
                                self.eps, self.momentum, self.act, stats)

    def _load_from_state_dict(self, *a, **k):
        self._nbt_pending = 0
        return super()._load_from_state_dict(*a, **k)


def _flush_nbt(module, *args):
    if module._nbt_pending:
        module.num_batches_tracked += module._nbt_pending
        module._nbt_pending = 0


class HipBatchNorm2d(_HipBatchNormMixin, nn.BatchNorm2d):
    def __init__(self, c, act=ops.ACT_NONE):
        super().__init__(c)
        self.act = act
        self._init_pending()


class HipBatchNorm1d(_HipBatchNormMixin, nn.BatchNorm1d):
    def __init__(self, c, act=ops.ACT_NONE):
        super().__init__(c)
        self.act = act
        self._init_pending()


class FusedIntoBN(nn.Module):
    """Placeholder keeping the reference's nn.Sequential indices (e.g. ``features.2`` is the
    ReLU): the activation itself runs inside the preceding HipBatchNorm kernel."""

    def __init__(self, what):
        super().__init__()
        self.what = what

    def forward(self, x):
        return x

    def extra_repr(self):
        return f"{self.what} (fused into the preceding BatchNorm kernel)"


class HipLeakyReLU(nn.Module):
    def forward(self, x):
        return F.bias_act(x.contiguous(), None, ops.EW_LRELU)


class HipTanh(nn.Module):
    def forward(self, x):
        return F.bias_act(x.contiguous(), None, ops.EW_TANH)


class HipSigmoid(nn.Module):
    def forward(self, x):
        return F.bias_act(x.contiguous(), None, ops.EW_SIGMOID)


class HipLinear(nn.Linear):
    """Linear layer on the vendor fp32 GEMM (hipBLASLt / rocBLAS through torch; trainers load the measured
    algorithm table of tuned_gemms.py).  ``bn_shadowed``: the bias feeds a train-mode BatchNorm1d (x_to_mu.0,
    x_to_logvar.0, preprocess.0: model.py:461-462, 467-468, 491-492), so its gradient is analytically zero and is defined
    as exactly zero like the convolution biases' (SURVEY.md section 3.1 item 9).  Refuses CPU tensors like every other
    layer here."""
    _next_bn = ()

    def __init__(self, fin, fout, bn_shadowed=False):
        super().__init__(fin, fout)
        self.bn_shadowed = bn_shadowed

    def forward(self, x):
        if not x.is_cuda:
            raise RuntimeError("disentangle_mlp_amd modules need CUDA/ROCm tensors (no CPU fallback)")
        # big layers (and the shadowed ones) go through this package's Function: the batched weight gradient of
        # functional.deferred_wgrad(), no bias-gradient reduction where it is zero by construction
        if (self.weight.numel() >= F.DEFER_MIN_WEIGHTS or self.bn_shadowed) and x.dim() == 2:
            return F.linear(x, self.weight, self.bias, _bias_mode(self))
        return tF.linear(x, self.weight, self.bias)


class LatentCritic(nn.Sequential):
    """FactorVAE's critic on the latent code (Kim & Mnih 2018, their discriminator): ``depth`` blocks
    of `HipLinear` + LeakyReLU(0.2), then ``HipLinear(width, 2)`` -- logit 0: "drawn from q(z)", logit 1: "dimensions permuted
    across the batch".  The layers are small: their GEMMs stay on the vendor route, as every small Linear here does.  A
    plain ``nn.Sequential``: the state_dict keys are ``0.weight``, ``0.bias``, ``2.weight``, ...  ``generator``: the weights are
    drawn from it -- torch's Linear default, U(+-1/sqrt(fan_in)) for weight and bias -- and the global CPU stream is left as
    it was (a trainer adds a critic without moving the other networks' weights); None: torch's own initialisation."""

    def __init__(self, n_hidden, width=1000, depth=6, generator=None):
        n_hidden, width, depth = int(n_hidden), int(width), int(depth)
        if n_hidden < 1 or width < 1 or depth < 1:
            raise ValueError(f"LatentCritic: n_hidden, width and depth must be >= 1, got {n_hidden}, {width}, {depth}")
        with (torch.random.fork_rng(devices=[]) if generator is not None else contextlib.nullcontext()):
            layers, fin = [], n_hidden
            for _ in range(depth):
                layers += [HipLinear(fin, width), HipLeakyReLU()]
                fin = width
            super().__init__(*layers, HipLinear(fin, 2))
        self.n_hidden, self.width, self.depth = n_hidden, width, depth
        if generator is not None:
            with torch.no_grad():
                for m in self:
                    if isinstance(m, HipLinear):
                        bound = m.in_features ** -0.5
                        m.weight.uniform_(-bound, bound, generator=generator)
                        m.bias.uniform_(-bound, bound, generator=generator)


def _link_bn(layer, bn):
    """Tell a ``bn_shadowed`` layer which BatchNorm its output feeds.  A tuple, not the module: nothing is registered
    (no child module, no state_dict key), and a deep copy of the network links the copies."""
    layer._next_bn = (bn,)


def _link_chain(mods):
    """`_link_bn` for every convolution / Linear layer of ``mods`` that is directly followed by a HipBatchNorm."""
    for a, b in zip(mods[:-1], mods[1:]):
        if isinstance(a, (HipConv2d, HipConvTranspose2d, HipLinear)) and isinstance(b, _HipBatchNormMixin):
            _link_bn(a, b)


def _bias_mode(layer, bn=None):
    """How a layer's bias gradient is produced.  A train-mode BatchNorm behind a ``bn_shadowed`` layer cancels the bias:
    BIAS_GRAD_ZERO.  Running statistics cancel nothing: whenever the BatchNorm that follows (``bn``, or the one the
    layer was linked to) is not training, the gradient is computed."""
    if bn is None and layer._next_bn:
        bn = layer._next_bn[0]
    frozen = bn is not None and not bn.training
    return F.BIAS_GRAD_ZERO if (layer.bn_shadowed and not frozen) else F.BIAS_GRAD_COMPUTE


def enable_eval(*nets):
    """Opt the networks in to eval mode: every HipBatchNorm1d / 2d of ``nets`` normalises with its running statistics
    whenever it is not training (``net.eval()``).  Returns the networks (the network, for one)."""
    for net in nets:
        for m in net.modules():
            if isinstance(m, _HipBatchNormMixin):
                m.eval_enabled = True
    return nets[0] if len(nets) == 1 else nets


def disable_eval(*nets):
    """Undo `enable_eval`: the networks refuse ``.eval()`` again."""
    for net in nets:
        for m in net.modules():
            if isinstance(m, _HipBatchNormMixin):
                m.__dict__.pop("eval_enabled", None)
    return nets[0] if len(nets) == 1 else nets


@contextlib.contextmanager
def eval_mode(*nets):
    """``with eval_mode(netEG): x = netEG.decode(z)``: `enable_eval` + ``.eval()``; on exit (also after an exception)
    every module has the ``training`` flag and every BatchNorm the mark it had before."""
    before = [(m, m.training, m.__dict__.get("eval_enabled")) for net in nets for m in net.modules()]
    try:
        enable_eval(*nets)
        for net in nets:
            net.eval()
        yield nets[0] if len(nets) == 1 else nets
    finally:
        for m, training, mark in before:
            m.training = training
            if isinstance(m, _HipBatchNormMixin):
                if mark is None:
                    m.__dict__.pop("eval_enabled", None)
                else:
                    m.eval_enabled = mark


def shadowed_bias_params(net):
    """The convolution biases whose gradient is defined as exactly zero (they feed a train-mode BatchNorm: HipConv2d /
    HipConvTranspose2d with ``bn_shadowed``): their backward returns no gradient at all, see functional.BIAS_GRAD_ZERO.
    (What the always-training trainers ask; a layer whose BatchNorm is in eval computes its bias gradient: `_bias_mode`.)"""
    return [m.bias for m in net.modules()
            if isinstance(m, (HipConv2d, HipConvTranspose2d, HipLinear)) and m.bn_shadowed and m.bias is not None]


def single_use_linear_weights(net, deferred=True):
    """The weights of the big Linear layers whose weight gradient a trainer's backward of ``net`` forms exactly once: the
    encoder heads ``x_to_mu.0`` / ``x_to_logvar.0`` (one pass per backward) and -- ``deferred``: inside
    `functional.deferred_wgrad`, which batches its passes into one -- the discriminator's ``lth_features.0``.  These may
    be updated inside the backward (functional.FUSE_LINEAR_ADAM).  The decoder's 128 -> 16384 layer is not among them:
    the beta-VAE-GAN's second phase runs it on the prior sample and on the reconstruction before one backward, and its
    first backward pass must not change a weight the second still reads."""
    names = ("x_to_mu", "x_to_logvar") + (("lth_features",) if deferred else ())
    out = []
    for m in net.modules():
        for name in names:
            seq = getattr(m, name, None)
            if isinstance(seq, nn.Sequential) and len(seq) and isinstance(seq[0], HipLinear):
                out.append(seq[0].weight)
    return out


# --------------------------------------------------------------- building blocks
# Conv <-> BatchNorm fusion: inside a chain conv -> BN -> act -> conv -> ... the statistics of every
# BatchNorm come from the producing convolution's epilogue, and its normalise + activation are applied by the
# CONSUMING convolution while it loads -- the normalised tensor of an inner layer is never written.  False: every
# BatchNorm runs its own two passes (the round-1 path; tests compare the two).
FUSE_CONV_BN = True
# The discriminator's head + BCE as one kernel each way (Discriminator_celeba.forward_with_bce); False /
# VG_FUSE_HEAD=0: Linear, Sigmoid and the BCE kernel one after the other (A/B timing, tests).
FUSE_HEAD_BCE = __import__("os").environ.get("VG_FUSE_HEAD", "1") != "0"
# The discriminator's passes of one phase share ONE launch of the big Linear layer's forward GEMM and one of its data
# gradient (Discriminator_celeba.features_grouped); False / VG_GROUP_PASSES=0: one launch per pass (same bits; A/B, tests).
GROUP_PASSES = __import__("os").environ.get("VG_GROUP_PASSES", "1") != "0"


def _has_hooks(mods):
    """Forward (pre-)hooks on any of the modules, or registered globally: the fused chain calls the kernels of several
    modules at once and would never fire them, so a hooked chain runs module by module instead (feature taps,
    profilers and parity probes keep working; same numbers up to the summation order of the statistics)."""
    from torch.nn.modules import module as _m
    if _m._global_forward_hooks or _m._global_forward_pre_hooks:
        return True
    return any(m._forward_hooks or m._forward_pre_hooks for m in mods)


def run_conv_bn_chain(mods, x):
    """Forward of [conv | transposed conv | HipBatchNorm2d | FusedIntoBN placeholder] modules in order, fused as
    above; a BatchNorm that is last in the chain (its consumer is not one of these convolutions) is materialised,
    still without its statistics pass when the producer left statistics."""
    pending, stats = None, None          # BatchNorm not applied yet; statistics slots of the current x

    def flush(t):
        nonlocal pending, stats
        if pending is not None:
            t = pending(t, stats=stats)
            pending, stats = None, None
        return t
    for i, m in enumerate(mods):
        if isinstance(m, (HipConv2d, HipConvTranspose2d)):
            tr = isinstance(m, HipConvTranspose2d)
            nxt = mods[i + 1] if i + 1 < len(mods) else None          # the chain knows its next module
            mode = _bias_mode(m, nxt if isinstance(nxt, _HipBatchNormMixin) else None)
            if pending is not None:
                bn = pending
                if bn._note_forward():
                    x, stats = F.bn_act_conv(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.momentum,
                                             bn.act, m.weight, m.bias, m.stride[0], tr, mode, stats)
                else:      # running statistics; the producer's slots still give the bound without a pass over x
                    x, stats = F.bn_eval_act_conv(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps, bn.act,
                                                  m.weight, m.bias, m.stride[0], tr, mode, stats)
                pending = None
            else:
                x, stats = F.conv_with_stats(x.contiguous(), m.weight, m.bias, m.stride[0], tr, mode)
        elif isinstance(m, HipBatchNorm2d):
            x = flush(x)
            pending = m
        elif isinstance(m, FusedIntoBN):
            continue
        else:
            x = flush(x)
            x, stats = m(x), None
    return flush(x)


class FusedChain(nn.Sequential):
    """nn.Sequential with the reference's indices (``features.0`` ... ``features.8``, ``convs.0`` ...), run fused.
    (The class name must contain neither "Conv" nor "BatchNorm": weights_init matches class names, model.py:8-14.)"""

    def __init__(self, *args):
        super().__init__(*args)
        _link_chain(list(self))

    def forward(self, x):
        mods = list(self)
        if not FUSE_CONV_BN or _has_hooks(mods):
            return super().forward(x)
        return run_conv_bn_chain(mods, x)


def _enc_trunk(cin, width):
    chans = [cin, width, 2 * width, 4 * width]
    layers = []
    for a, b in zip(chans[:-1], chans[1:]):
        layers += [HipConv2d(a, b, 2), HipBatchNorm2d(b, ops.ACT_RELU), FusedIntoBN("ReLU")]
    return FusedChain(*layers)


def _latent_hw(opt):
    """Spatial size of the encoder's last feature map = opt.n_z[1:], (8, 8) for 64x64 inputs.  The
    reference hard-codes 8*8 (model.py:461) and the 16/32/64 output sizes (:558-564); deriving both
    from opt.n_z reproduces it exactly at n_z = [256, 8, 8] and gives the 128x128 / 256x256
    variants of BASELINE configs 4-5 (image side = 8 * n_z[1]) without new kernels."""
    n_z = getattr(opt, "n_z", None)
    return (8, 8) if n_z is None else (int(n_z[1]), int(n_z[2]))


def _enc_head(width, n_hidden, spatial=(8, 8)):
    head = nn.Sequential(HipLinear(width * 4 * spatial[0] * spatial[1], 2048, bn_shadowed=True), HipBatchNorm1d(2048, ops.ACT_RELU),
                         FusedIntoBN("ReLU"), HipLinear(2048, n_hidden))
    _link_chain(list(head))
    return head


def _bn_relu(c):
    return nn.Sequential(HipBatchNorm2d(c, ops.ACT_RELU), FusedIntoBN("ReLU"))


class _DecoderMixin:
    def _build_decoder(self, n_hidden, n_z):
        dim = n_z[0] * n_z[1] * n_z[2]
        self.preprocess = nn.Sequential(HipLinear(n_hidden, dim, bn_shadowed=True), HipBatchNorm1d(dim, ops.ACT_RELU),
                                        FusedIntoBN("ReLU"))
        self.deconv1 = HipConvTranspose2d(n_z[0], 256, 2)
        self.act1 = _bn_relu(256)
        self.deconv2 = HipConvTranspose2d(256, 128, 2)
        self.act2 = _bn_relu(128)
        self.deconv3 = HipConvTranspose2d(128, 32, 2)
        self.act3 = _bn_relu(32)
        self.deconv4 = HipConvTranspose2d(32, 3, 1, bn_shadowed=False)
        self.activation = HipTanh()
        _link_chain(list(self.preprocess))
        for conv, bn in ((self.deconv1, self.act1), (self.deconv2, self.act2), (self.deconv3, self.act3)):
            _link_bn(conv, bn[0])

    def _decode(self, code, n_z):
        bs = code.size(0)
        h = self.preprocess(code).view(-1, n_z[0], n_z[1], n_z[2])
        zh, zw = n_z[1], n_z[2]          # (8, 8) in the reference: the literals of model.py:558-564
        chain = [self.deconv1, *self.act1, self.deconv2, *self.act2, self.deconv3, *self.act3, self.deconv4]
        if FUSE_CONV_BN and not _has_hooks(chain + [self.act1, self.act2, self.act3]):
            # deconv1 -> act1 -> deconv2 -> act2 -> deconv3 -> act3 -> deconv4 as one fused chain
            h = run_conv_bn_chain(chain, h.contiguous())
            return self.activation(h)
        h = self.act1(self.deconv1(h, output_size=(bs, 256, 2 * zh, 2 * zw)))
        h = self.act2(self.deconv2(h, output_size=(bs, 128, 4 * zh, 4 * zw)))
        h = self.act3(self.deconv3(h, output_size=(bs, 32, 8 * zh, 8 * zw)))
        return self.activation(self.deconv4(h, output_size=(bs, 3, 8 * zh, 8 * zw)))


# -------------------------------------------------------------------- the zoo
class Encoder_celeba(nn.Module):
    """model.py:282-328.  forward -> (z, per-sample kld (B,))."""

    def __init__(self, opt, representation_size=64):
        super().__init__()
        self.input_channels = opt.input_channels
        self.n_hidden = opt.n_hidden
        self.features = _enc_trunk(self.input_channels, representation_size)
        self.x_to_mu = _enc_head(representation_size, self.n_hidden, _latent_hw(opt))
        self.x_to_logvar = _enc_head(representation_size, self.n_hidden, _latent_hw(opt))

    def reparameterize(self, x, eps=None):
        mu = self.x_to_mu(x)
        logvar = self.x_to_logvar(x)
        if eps is None:
            eps = torch.randn(mu.size(), device=mu.device)
        return F.KLRowsFn.apply(mu, logvar, eps)

    def forward(self, x, eps=None):
        bs = x.size(0)
        feat = self.features(x)
        return self.reparameterize(ops.keep_amax(feat, feat.view(bs, -1)), eps)


class Generator_celeba(nn.Module, _DecoderMixin):
    """model.py:331-378."""

    def __init__(self, opt):
        super().__init__()
        self.input_size = opt.n_hidden
        self.representation_size = opt.n_z
        self._build_decoder(self.input_size, self.representation_size)

    def forward(self, code):
        return self._decode(code, self.representation_size)


class Discriminator_celeba(nn.Module):
    """model.py:381-416.  forward -> (p (B,), lth features (B, 2048))."""

    def __init__(self, opt):
        super().__init__()
        self.representation_size = opt.n_z
        dim = opt.n_z[0] * opt.n_z[1] * opt.n_z[2]
        spec = [(opt.input_channels, 32, 1), (32, 128, 2), (128, 256, 2), (256, 256, 2)]
        layers = []
        for a, b, s in spec:
            layers += [HipConv2d(a, b, s), HipBatchNorm2d(b, ops.ACT_LRELU), FusedIntoBN("LeakyReLU(0.2)")]
        self.convs = FusedChain(*layers)
        self.lth_features = nn.Sequential(HipLinear(dim, 2048), HipLeakyReLU())
        self.sigmoid_output = nn.Sequential(HipLinear(2048, 1), HipSigmoid())

    def forward(self, x):
        bs = x.size(0)
        c = self.convs(x)
        feat = self.lth_features(ops.keep_amax(c, c.view(bs, -1)))
        p = self.sigmoid_output(feat)
        return p.squeeze(), feat.squeeze()

    def _features_of(self, x, no_grad=False):
        with torch.set_grad_enabled(torch.is_grad_enabled() and not no_grad):
            c = self.convs(x)
            return ops.keep_amax(c, c.view(x.size(0), -1))

    def features_grouped(self, xs, no_grad=None):
        """``lth_features`` of 2..3 batches of one shape, the passes of one phase over unchanged weights: the convolution
        / BatchNorm trunk runs per input in the order given (batch statistics and running averages update pass by pass as
        in separate calls), then the 16384 -> 2048 Linear layer runs ONCE for all (functional.linear_grouped: its 134 MB
        weight is streamed and split once instead of once per pass), then the LeakyReLU per pass.  ``no_grad[i]``: pass i
        is made as under ``torch.no_grad()``.  Every result is bit for bit that of ``self.lth_features(trunk(x))``.
        Falls back to pass by pass (GROUP_PASSES off, a hooked layer, a Linear layer the package's GEMM does not take)."""
        no_grad = tuple(no_grad) if no_grad is not None else (False,) * len(xs)
        lin, act = self.lth_features[0], self.lth_features[1]
        hooked = _has_hooks([self.lth_features, lin, act])
        nw = lin.weight.numel()
        takes = (2 <= len(xs) <= ops.GEMM_MAX_GROUPS and all(x.is_cuda and x.shape == xs[0].shape for x in xs)
                 and ops.linear_split_ok(lin.in_features, nw) and ops.linear_split_ok(lin.out_features, nw))
        if not GROUP_PASSES or hooked or not takes:
            feats = []
            for x, ng in zip(xs, no_grad):
                with torch.set_grad_enabled(torch.is_grad_enabled() and not ng):
                    feats.append(self.lth_features(self._features_of(x)))
            return feats
        cs = [self._features_of(x, ng) for x, ng in zip(xs, no_grad)]
        ys = F.linear_grouped(cs, lin.weight, lin.bias, F.BIAS_GRAD_COMPUTE, no_grad)
        return [act(y) for y in ys]

    def head_with_bce(self, feat, label, divisor=None):
        """The head of `forward_with_bce` on features already computed (`features_grouped`): (p, features, bce)."""
        lin = self.sigmoid_output[0]
        if not FUSE_HEAD_BCE or lin._forward_hooks or lin._forward_pre_hooks or self.sigmoid_output[1]._forward_hooks:
            p = self.sigmoid_output(feat).squeeze()              # hooked head: module by module
            return p, feat.squeeze(), F.bce_loss(p, label, divisor)
        p, bce = F.dot_sigmoid_bce(feat, lin.weight, lin.bias, label, divisor)
        return p, feat.squeeze(), bce

    def forward_with_bce(self, x, label, divisor=None):
        """``forward`` plus ``nn.BCELoss()(p, full(label))`` (new_betavaegan.py:101,118,153-154; ``divisor``: the batch the
        mean runs over -- the global batch under data parallelism) with the head -- Linear(2048 -> 1) + Sigmoid -- and the
        loss in ONE kernel each way.  Returns (p, features, bce)."""
        return self.head_with_bce(self.lth_features(self._features_of(x)), label, divisor)

    def head_with_loss(self, feat, loss, role, label, divisor=None):
        """The head under an adversarial loss of the LOGIT on features already computed:
        ``loss`` in "logistic" / "hinge" / "lsgan", ``role`` in "real" / "fake" / "gen" (functional.GAN_LOSSES), ``label`` as
        in `head_with_bce` (the hinge terms ignore it).  Returns (p, logit, features, loss); p = sigmoid(logit) is for
        logging only -- the Sigmoid module is not on this path, and nothing is differentiated through p or logit.
        Routes as `head_with_bce`: one kernel each way, or -- FUSE_HEAD_BCE off, a hooked head Linear -- the Linear
        module followed by the loss kernel.  (A hook on the Sigmoid does not count here: that module is on neither
        route of this path, so it would never fire.)"""
        kind = F.gan_loss_kind(loss, role)
        lin = self.sigmoid_output[0]
        if not FUSE_HEAD_BCE or lin._forward_hooks or lin._forward_pre_hooks:
            logit = lin(feat).squeeze(-1)
            p, val = F.gan_loss(logit, kind, label, divisor)
            return p, logit.detach(), feat.squeeze(), val
        logit, p, val = F.dot_gan_loss(feat, lin.weight, lin.bias, kind, label, divisor)
        return p, logit, feat.squeeze(), val

    def forward_with_loss(self, x, loss, role, label, divisor=None):
        """`forward_with_bce` under an adversarial loss of the logit: (p, logit, features, loss) of `head_with_loss`."""
        return self.head_with_loss(self.lth_features(self._features_of(x)), loss, role, label, divisor)


class VAE(nn.Module, _DecoderMixin):
    """model.py:419-571.  ``forward(x, eps=None)``: eps may be injected for reproducible
    parity runs (the reference draws it inside ``reparameterize``, model.py:534)."""

    def __init__(self, opt, representation_size=64):
        super().__init__()
        self.input_channels = opt.input_channels
        self.n_hidden = opt.n_hidden
        self.features = _enc_trunk(self.input_channels, representation_size)
        self.x_to_mu = _enc_head(representation_size, self.n_hidden, _latent_hw(opt))
        self.x_to_logvar = _enc_head(representation_size, self.n_hidden, _latent_hw(opt))
        self.input_size = opt.n_hidden
        self.representation_size2 = opt.n_z
        self._build_decoder(self.input_size, self.representation_size2)

    def encode(self, x):
        bs = x.size(0)
        inner = self.features(x).view(bs, -1)
        return self.x_to_mu(inner), self.x_to_logvar(inner)

    def reparameterize(self, mu, logvar, eps=None):
        if eps is None:
            eps = torch.randn_like(mu)
        z, _ = F.reparam_kl(mu, logvar, eps, 0.0)
        return z

    def decode(self, code):
        return self._decode(code, self.representation_size2)

    def forward(self, x, eps=None):
        mu, logvar = self.encode(x)
        return self.decode(self.reparameterize(mu, logvar, eps)), mu, logvar

    def forward_with_kl(self, x, eps, beta):
        """Same as forward plus the fused beta*KL scalar (one kernel for reparam + KL).  ``beta``: a float, or a
        one-element fp32 device tensor (functional.reparam_kl)."""
        mu, logvar = self.encode(x)
        if eps is None:
            eps = torch.randn_like(mu)
        z, kl = F.reparam_kl(mu, logvar, eps, beta)
        return self.decode(z), mu, logvar, kl

    def _forward_with_objective(self, x, eps, reparam):
        """The body of `forward_with_tc` / `_dip` / `_mmd` / `_klc`: encode, draw ``eps`` if None, ``reparam(mu, logvar, eps) -> z,
        loss, parts``, decode.  Returns ``recon, mu, logvar, loss, parts``."""
        mu, logvar = self.encode(x)
        if eps is None:
            eps = torch.randn_like(mu)
        z, loss, parts = reparam(mu, logvar, eps)
        return self.decode(z), mu, logvar, loss, parts

    def forward_with_tc(self, x, eps, beta, alpha, gamma, dataset_size):
        """`forward_with_kl` with the KL term decomposed (functional.reparam_tc): returns ``recon, mu, logvar, loss,
        parts`` -- ``loss = alpha*mi + beta*tc + gamma*dwkl``, ``parts`` the ``[3]`` tensor ``(mi, tc, dwkl)``."""
        return self._forward_with_objective(
            x, eps, lambda mu, logvar, eps: F.reparam_tc(mu, logvar, eps, beta, alpha, gamma, dataset_size))

    def forward_with_dip(self, x, eps, beta, variant, lambda_od, lambda_d):
        """`forward_with_kl` with the DIP-VAE covariance penalty added (functional.reparam_dip): returns ``recon, mu,
        logvar, loss, parts`` -- ``loss = beta*kl + B*(lambda_od*od + lambda_d*dg)``, ``parts`` the ``[3]`` tensor ``(kl,
        od, dg)``."""
        return self._forward_with_objective(
            x, eps, lambda mu, logvar, eps: F.reparam_dip(mu, logvar, eps, beta, lambda_od, lambda_d, variant))

    def forward_with_mmd(self, x, eps, prior, beta, kernel, lambda_mmd, bandwidths=None):
        """`forward_with_kl` with the InfoVAE / WAE-MMD penalty added (functional.reparam_mmd): returns ``recon, mu,
        logvar, loss, parts`` -- ``loss = beta*kl + B*lambda_mmd*mmd``, ``parts`` the ``[3]`` tensor ``(kl, mmd, kzz)``.
        ``prior``: draws from N(0, I) of the shape of ``mu``; like ``eps``, ``None`` is drawn here, after ``eps``."""
        def reparam(mu, logvar, eps):
            zp = torch.randn_like(mu) if prior is None else prior
            return F.reparam_mmd(mu, logvar, eps, zp, beta, lambda_mmd, kernel, bandwidths)
        return self._forward_with_objective(x, eps, reparam)

    def forward_with_klc(self, x, eps, beta, capacity, free_bits):
        """`forward_with_kl` with the KL term under a capacity and per-dimension free bits (functional.reparam_klc): returns
        ``recon, mu, logvar, loss, parts`` -- ``loss = beta*|kl_floored - B*capacity|``, ``parts`` the ``[3]`` tensor ``(kl,
        kl_floored, dims_above)``.  ``beta`` / ``capacity``: both floats or both one-element fp32 device tensors."""
        return self._forward_with_objective(
            x, eps, lambda mu, logvar, eps: F.reparam_klc(mu, logvar, eps, beta, capacity, free_bits))

    def forward_with_factor(self, x, eps, beta, gamma, critic):
        """`forward_with_kl` with FactorVAE's total-correlation estimate added (functional.factor_tc):
        returns ``recon, mu, logvar, loss, parts, z`` -- ``loss = beta*kl + gamma*sum_b(l0 - l1)`` with ``(l0, l1) =
        critic(z_b)``, ``parts`` the ``[3]`` tensor ``(kl, tc, rows with l0 > l1)``, and ``z`` DETACHED: what the critic's own
        phase permutes and classifies, from this same forward.  The gradient reaches the encoder through ``critic``; whether
        the critic's weights take one is the caller's business (a trainer freezes them here).  ``beta`` / ``gamma``: both
        floats or both one-element fp32 device tensors."""
        mu, logvar = self.encode(x)
        if eps is None:
            eps = torch.randn_like(mu)
        z, kl = F.reparam_kl(mu, logvar, eps, 1.0)      # unweighted: `factor_tc` weighs it, and reports it as it is
        loss, parts = F.factor_tc(critic(z), kl, beta, gamma)
        return self.decode(z), mu, logvar, loss, parts, z.detach()
