"""torch.autograd.Function wrappers: each forward / backward is one or two launches
of the HIP library (disentangle_mlp_amd.ops).  Work that autograd reports as not
needed (``ctx.needs_input_grad``) is skipped -- e.g. the discriminator's weight
gradients while it only relays gradients to the decoder (SURVEY.md section 3.1
item 3: those gradients are discarded by the reference's next ``zero_grad``).
"""
import math
import os
import threading

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops

# How the gradient of a convolution bias that feeds a train-mode BatchNorm is
# produced.  It is analytically zero (BN subtracts the batch mean); the reference
# accumulates pure rounding noise there.
# BIAS_GRAD_ZERO: the backward hands autograd NO gradient for that bias (None) -- defined as exactly zero without a
# fill + accumulate launch per pass; the trainers keep a persistent all-zero ``.grad`` on those parameters
# (trainer._zero_grads) so that optimizers and gradient exchange see zeros.
BIAS_GRAD_COMPUTE, BIAS_GRAD_ZERO = 0, 1


def _conv_backward(ctx, x, w, gy, need_x, need_w, need_b, aff=None, then=None):
    """The backward of every convolution Function (``ctx``: .stride, .transposed, .bias_grad, .acc): the data gradient by
    the opposite convolution -- handed through ``then`` (BNConvFn: the BatchNorm's backward) as soon as it is launched --,
    the weight gradient with the roles of input and gradient swapped for a transposed layer, the layer's input read
    through ``aff`` where the forward read it so, and the bias gradient.  Returns (gx or what ``then`` made of it, gw, gb)."""
    s, tr = ctx.stride, ctx.transposed
    gx = gw = gb = None
    if need_x:
        if not tr and (x.shape[2] % s or x.shape[3] % s):
            raise RuntimeError("conv5x5 data gradient needs input sizes divisible by the stride")
        gx = ops.conv5x5_fwd(gy, w, None, s) if tr else ops.convT5x5_fwd(gy, w, None, s)
        if then is not None:
            gx = then(gx)
    if need_w:
        slot = _grad_slot(ctx.acc, id(w))
        kw = dict(out=slot.prev, accumulate=True) if slot.prev is not None else {}
        if aff is not None:
            kw.update(in_affine=aff, affine_on_gy=tr)
        gw = slot.hand_over(ops.conv5x5_wgrad(gy, x, s, **kw) if tr else ops.conv5x5_wgrad(x, gy, s, **kw))
    if need_b:
        gb = None if ctx.bias_grad == BIAS_GRAD_ZERO else ops.channel_sum(gy)
    return gx, gw, gb


class ConvFn(Function):
    """nn.Conv2d(k=5, p=2, stride) -- model.py:450 etc.; ``transposed``:
    nn.ConvTranspose2d(k=5, p=2, stride, output_size=stride*in) -- model.py:495-507, :558-564.  Outside
    `accumulate_param_grads`: autograd sums the gradients of a weight used twice."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, transposed, bias_grad):
        ctx.stride, ctx.transposed, ctx.bias_grad, ctx.acc = stride, transposed, bias_grad, None
        ctx.save_for_backward(x, w)
        return ops.convT5x5_fwd(x, w, bias, stride) if transposed else ops.conv5x5_fwd(x, w, bias, stride)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        return _conv_backward(ctx, x, w, gy.contiguous(), *ctx.needs_input_grad[:3]) + (None, None, None)


_defer_tls = threading.local()      # .current: the innermost active deferred_wgrad context of this thread


class deferred_wgrad:
    """Context for a phase that runs a network several times and then ONE backward (the discriminator phase: D(x) and
    D(fake), new_betavaegan.py:95-123): the weight gradient of a big Linear layer is computed once, over the
    concatenated batches, by whichever of its backward nodes runs last -- instead of one GEMM per pass (each writing the
    134 MB gradient of the 16384 x 2048 layer) plus autograd's additions.  The sum is the same up to fp32 summation
    order.  Every forward made inside the context must get its backward inside it (checked at exit).

    The bookkeeping (per big weight: forward passes that still owe a backward, and the (gy, x) pairs already seen)
    lives in the context object, which every forward made inside it captures: two trainers stepping in two threads, or
    a backward that runs after its context has closed, never see each other's state (such a late backward just
    computes its own weight gradient)."""

    def __init__(self):
        self.pending, self.stash, self.open = {}, {}, False

    def __enter__(self):
        self._outer = getattr(_defer_tls, "current", None)
        self.open = DEFER_WGRAD
        _defer_tls.current = self if DEFER_WGRAD else None
        return self

    def __exit__(self, *exc):
        _defer_tls.current = self._outer
        self.open = False
        left = sum(self.pending.values())
        self.pending, self.stash = {}, {}
        if left and exc[0] is None:
            raise RuntimeError(f"deferred_wgrad: {left} forward pass(es) of a Linear layer got no backward inside the context")
        return False


_acc_tls = threading.local()


class accumulate_param_grads:
    """Context for iterations that apply a layer several times before ONE backward (the discriminator on the real and on
    the generated batch, the decoder on the prior sample and on the reconstruction: new_betavaegan.py:99-121, 144-163).
    The first backward pass through a layer hands autograd its parameter gradient as usual and remembers the tensor; a
    later pass ADDS into that tensor inside its own kernel (`accumulate` of vg_conv5x5_wgrad*, vg_bn_act_bwd,
    vg_dot_sigmoid_bce_bwd, addmm_ for Linear) and hands autograd nothing -- instead of a second tensor plus the addition
    autograd would launch (29 of them per iteration).  Floating-point addition is commutative: same bits as autograd's sum.
    Forward passes capture the context object; `reset()` forgets the remembered tensors (call it where gradients are
    zeroed: a new backward must not add into the previous one's tensors).  Outside a context nothing changes."""

    def __init__(self):
        self.acc, self.open = {}, False

    def __enter__(self):
        self._outer = getattr(_acc_tls, "current", None)
        _acc_tls.current = self
        self.open = True
        return self

    def __exit__(self, *exc):
        _acc_tls.current = self._outer
        self.open, self.acc = False, {}
        return False

    def reset(self):
        self.acc = {}


def _acc_ctx():
    return getattr(_acc_tls, "current", None)


class _grad_slot:
    """One backward pass's side of the `accumulate_param_grads` protocol for the parameter gradient(s) of one layer
    (``key``).  ``prev``: what the layer's first pass handed autograd, for this pass's kernel to ADD into -- None on the
    first pass and outside an open context.  `hand_over(grads)`: what this pass hands autograd -- its own result on the
    first pass (remembered), None for everything that was added into ``prev``."""
    __slots__ = ("acc", "key", "prev")

    def __init__(self, actx, key):
        self.acc = actx.acc if (actx is not None and actx.open) else None
        self.key = key
        self.prev = self.acc.get(key) if self.acc is not None else None

    def hand_over(self, grads):
        many = isinstance(grads, tuple)
        if self.prev is not None:
            return (None,) * len(grads) if many else None
        if self.acc is not None:
            # Remembers ALIASES (detach(): a new tensor object on the same storage) -- a second reference to the gradient
            # tensor itself would make autograd's AccumulateGrad copy it instead of adopting it as ``.grad`` (71 copies
            # per iteration).
            self.acc[self.key] = tuple(t.detach() for t in grads) if many else grads.detach()
        return grads


DEFER_MIN_WEIGHTS = 1 << 20
DEFER_WGRAD = os.environ.get("VG_DEFER_WGRAD", "1") != "0"      # 0: deferred_wgrad() does nothing


# The weight gradient of a big Linear layer and its Adam step in one launch (ops.linear_wgrad_adam; DESIGN.md section
# 4.19): on where a trainer has opened registrations for the backward (`open_fused_linear_steps`).  0: never.
FUSE_LINEAR_ADAM = os.environ.get("VG_FUSE_LINEAR_ADAM", "1") != "0"
# {id(weight): optim.FusedLinearStep} of the backward passes about to run.  A plain module dictionary, not a thread-local:
# autograd runs the backward nodes of a device on its own worker thread.  An entry counts only while it is `open` and only
# for the weight object it was made for, so two trainers in two threads do not see each other's.
_fused_steps = {}


def open_fused_linear_steps(regs):
    """``regs``: what `optim.HipAdam.begin_fused_step` returned (None / empty: nothing is added).  From here to the
    optimizer's `step` -- which closes every registration -- the backward of a registered weight updates it in place
    and hands autograd no gradient.  Registrations that were closed since are forgotten here."""
    for k in [k for k, r in _fused_steps.items() if not r.open]:
        del _fused_steps[k]
    if regs:
        _fused_steps.update(regs)


def _fused_step_of(w):
    reg = _fused_steps.get(id(w))
    return reg if (reg is not None and reg.open and reg.p is w) else None


def _linear_weight_grad(acc, defer, w, gy, x):
    """The weight gradient of one pass (gy, x) of a Linear layer under both protocols -- `deferred_wgrad` (``defer``: the
    context the pass was made in, or None) and `accumulate_param_grads` (``acc``).  Returns what the pass hands autograd:
    the gradient, or None when a later pass computes it for all or it was added into an earlier pass's tensor."""
    wg, wx = gy, x                                   # what the weight gradient is taken over
    d, k = defer, id(w)
    if d is not None and d.open and d.pending.get(k, 0) > 0:
        d.stash.setdefault(k, []).append((gy, x))
        d.pending[k] -= 1
        if d.pending[k] > 0:
            return None                              # a later pass of this layer does it for all
        pairs = d.stash.pop(k)
        if len(pairs) > 1:
            wg, wx = torch.cat([p[0] for p in pairs]), torch.cat([p[1] for p in pairs])
    slot = _grad_slot(acc, id(w))
    split = ops.linear_split_ok(wg.shape[0], w.numel())
    reg = _fused_step_of(w) if FUSE_LINEAR_ADAM else None
    if reg is not None:
        if reg.done:
            raise RuntimeError("a Linear weight that took the fused weight-gradient + Adam step was used a second time "
                               "in the same backward")
        # (a slot that already holds a gradient: the layer's second use in this backward -- the two launches)
        if split and slot.prev is None and ops.linear_wgrad_adam(wg, wx, reg):
            reg.done = True
            return None                              # the weight is updated: nothing for autograd, no ``.grad``
    if slot.prev is None:
        return slot.hand_over(ops.linear_wgrad(wg, wx) if split else wg.t() @ wx)
    if split:
        slot.prev.add_(ops.linear_wgrad(wg, wx))
    else:
        slot.prev.addmm_(wg.t(), wx)                 # the layer's second use: added in the GEMM's epilogue
    return None


class LinearFn(Function):
    """nn.Linear (model.py:460-471, 402-408, 490-492).  Layers with >= 2^20 weights run on this package's fp16x3 GEMM
    under the default arithmetic (ops.linear_*; a GEMM whose reduction length is not a multiple of 32 -- the weight
    gradient at batches that are not -- goes to the vendor library), everything else on the vendor fp32 GEMMs (SURVEY.md
    K7; algorithm table: tuned_gemms.py).  Inside `deferred_wgrad()` the weight gradient of a layer with >= 2^20 weights
    is batched over its passes."""

    @staticmethod
    def forward(ctx, x, w, bias, bias_grad=BIAS_GRAD_COMPUTE):
        ctx.save_for_backward(x, w)
        ctx.bias_grad = bias_grad
        ctx.acc = _acc_ctx()
        dctx = getattr(_defer_tls, "current", None)
        ctx.defer = dctx if (dctx is not None and ctx.needs_input_grad[1] and w.numel() >= DEFER_MIN_WEIGHTS) else None
        if ctx.defer is not None:
            dctx.pending[id(w)] = dctx.pending.get(id(w), 0) + 1
        if ops.linear_split_ok(x.shape[1], w.numel()):
            return ops.linear_fwd(x, w, bias)
        return torch.nn.functional.linear(x, w, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = ops.linear_dgrad(gy, w) if ops.linear_split_ok(gy.shape[1], w.numel()) else gy @ w
        if ctx.needs_input_grad[2] and ctx.bias_grad != BIAS_GRAD_ZERO:      # (a bias that feeds a BatchNorm1d: no gradient)
            gb = gy.sum(0)
        if ctx.needs_input_grad[1]:
            gw = _linear_weight_grad(ctx.acc, ctx.defer, w, gy, x)
        return gx, gw, gb, None


class LinearGroupedFn(Function):
    """`LinearFn` for G = 1..3 inputs through the SAME layer in one node: one grouped forward GEMM and one grouped
    data-gradient GEMM (ops.linear_*_grouped: the weight is streamed and split once for all groups), so the layer must be
    one `ops.linear_split_ok` takes.  Every output, input gradient and parameter gradient is bit for bit what G
    `LinearFn` calls in the same order give: the groups are independent rows of the GEMMs, and the parameter gradients
    go through the same protocols pass by pass, last group first -- the order in which autograd runs the G nodes.
    ``detached[g]``: group g is a pass made under ``no_grad`` -- its output is not differentiable and the pass takes no
    part in the backward.  apply(w, bias, bias_grad, detached, *xs) -> G outputs."""

    @staticmethod
    def forward(ctx, w, bias, bias_grad, detached, *xs):
        live = [g for g in range(len(xs)) if not detached[g]]
        ctx.save_for_backward(w, *(xs[g] for g in live))
        ctx.bias_grad, ctx.live, ctx.ngroups = bias_grad, live, len(xs)
        ctx.acc = _acc_ctx()
        dctx = getattr(_defer_tls, "current", None)
        ctx.defer = dctx if (dctx is not None and ctx.needs_input_grad[0] and w.numel() >= DEFER_MIN_WEIGHTS) else None
        if ctx.defer is not None:
            dctx.pending[id(w)] = dctx.pending.get(id(w), 0) + len(live)
        ctx.set_materialize_grads(False)
        ys = ops.linear_fwd_grouped(list(xs), w, bias)
        ctx.mark_non_differentiable(*(ys[g] for g in range(len(xs)) if detached[g]))
        return tuple(ys)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gys):
        w, *xs = ctx.saved_tensors
        gxs = [None] * ctx.ngroups
        gw = gb = None
        passes = []                                      # (group, gy, x) of the passes that got a gradient
        for g, x in zip(ctx.live, xs):
            if gys[g] is not None:
                passes.append((g, gys[g].contiguous(), x))
        want = [p for p in passes if ctx.needs_input_grad[4 + p[0]]]
        if want:
            for p, gx in zip(want, ops.linear_dgrad_grouped([p[1] for p in want], w)):
                gxs[p[0]] = gx
        for g, gy, x in reversed(passes):
            if ctx.needs_input_grad[1] and ctx.bias_grad != BIAS_GRAD_ZERO:
                gb = gy.sum(0) if gb is None else gb.add_(gy.sum(0))
            if ctx.needs_input_grad[0]:
                one = _linear_weight_grad(ctx.acc, ctx.defer, w, gy, x)
                if one is not None:
                    gw = one if gw is None else gw.add_(one)
        return (gw, gb, None, None, *gxs)


def _bn_backward(ctx, gy, x, gamma, beta, mean, invstd, need_p):
    """vg_bn_act_bwd with the parameter gradients under the accumulate protocol (BNActFn, BNConvFn)."""
    slot = _grad_slot(ctx.acc if need_p else None, id(gamma))
    gx, dg, db = ops.bn_act_bwd(gy, x, gamma, beta, mean, invstd, ctx.act, need_p, accumulate_into=slot.prev)
    return (gx,) + (slot.hand_over((dg, db)) if need_p else (dg, db))


class BNActFn(Function):
    """Train-mode BatchNorm1d/2d + {none, ReLU, LeakyReLU(0.2)} -- model.py:451-452 etc.
    running_mean / running_var are updated in place by the kernel.  ``stats``: the statistics slots the producing
    convolution left (ops.conv5x5_fwd(..., want_stats=True)); then the statistics pass over x is skipped.
    Returns (y, the bound slot of max |y| its kernel emitted -- a non-differentiable side product -- or None)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, momentum, act, stats=None):
        if stats is not None:
            count = x.numel() // x.shape[1]
            mean, invstd, scale, shift = ops.bn_finalize_stats(stats, count, gamma, beta, running_mean, running_var,
                                                               eps, momentum)
            y = ops.affine_act(x, scale, shift, act)
        else:
            y, mean, invstd = ops.bn_act_fwd(x, gamma, beta, running_mean, running_var, eps, momentum, act)
        ctx.act = act
        ctx.acc = _acc_ctx()
        ctx.save_for_backward(x, gamma, beta, mean, invstd)
        bound = ops.known_amax(y)
        if bound is not None:
            ctx.mark_non_differentiable(bound)
        ctx.set_materialize_grads(False)      # as ConvStatsFn
        return y, bound

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _):
        if gy is None:
            return (None,) * 9
        x, gamma, beta, mean, invstd = ctx.saved_tensors
        need_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        gx, dg, db = _bn_backward(ctx, gy.contiguous(), x, gamma, beta, mean, invstd, need_p)
        return gx, dg, db, None, None, None, None, None, None


class ConvStatsFn(Function):
    """conv / transposed conv that also returns the statistics slots of its output (a non-differentiable side
    product of the kernel's epilogue; an empty tensor when this layer's kernel cannot emit them)."""

    @staticmethod
    def forward(ctx, x, w, bias, stride, transposed, bias_grad):
        ctx.stride, ctx.transposed, ctx.bias_grad = stride, transposed, bias_grad
        ctx.acc = _acc_ctx()
        ctx.save_for_backward(x, w)
        conv = ops.convT5x5_fwd if transposed else ops.conv5x5_fwd
        y, stats = conv(x, w, bias, stride, want_stats=True)
        stats = stats if stats is not None else x.new_empty(0)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)      # or autograd zero-fills a "gradient" of the statistics slots every backward
        return y, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _):
        if gy is None:
            return (None,) * 6
        x, w = ctx.saved_tensors
        return _conv_backward(ctx, x, w, gy.contiguous(), *ctx.needs_input_grad[:3]) + (None, None, None)


class BNConvFn(Function):
    """[train-mode BatchNorm2d + activation] -> [5x5 conv / transposed conv] with the normalised, activated tensor
    NEVER materialised (model.py:451-456, 390-398, 496-505): the BatchNorm's statistics come from the
    slots the producing convolution left (``stats_in``, or one pass over x when there are none), its scale / shift
    and activation are applied by the consuming convolution while it stages its input -- forward, and again by the
    weight gradient in backward.  Backward: data gradient of the convolution (w.r.t. the activated tensor), then the
    ordinary BatchNorm backward against the saved raw x (vg_bn_act_bwd: mask recomputed from x).
    Returns (y, statistics slots of y -- empty when the kernel cannot emit them)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w, bias, running_mean, running_var, eps, momentum, act, stride, transposed,
                bias_grad, stats_in):
        count = x.numel() // x.shape[1]
        # bound: of max |act(BN(x))|, ~|gamma| sqrt(count) + |beta| (bn.hip: bn_act_bound; None outside fp16x3): what the
        # convolution -- and, in backward, the weight gradient -- scales the operand it reads through the BatchNorm by
        if stats_in is not None and stats_in.numel():
            mean, invstd, scale, shift, bound = ops.bn_finalize_stats(stats_in, count, gamma, beta, running_mean,
                                                                      running_var, eps, momentum, want_bound=True)
        else:
            mean, invstd, scale, shift, bound = ops.bn_stats(x, gamma, beta, running_mean, running_var, eps, momentum,
                                                             want_bound=True)
        conv = ops.convT5x5_fwd if transposed else ops.conv5x5_fwd
        y, stats = conv(x, w, bias, stride, in_affine=(scale, shift, act, bound), want_stats=True)
        stats = stats if stats is not None else x.new_empty(0)
        ctx.act, ctx.stride, ctx.transposed, ctx.bias_grad = act, stride, transposed, bias_grad
        ctx.acc = _acc_ctx()
        ctx.save_for_backward(x, gamma, beta, mean, invstd, scale, shift, w, bound)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)      # as ConvStatsFn
        return y, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _):
        if gy is None:
            return (None,) * 14
        x, gamma, beta, mean, invstd, scale, shift, w, bound = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_p = need[1] or need[2]

        def bn_backward(ga):                                 # ga: the gradient w.r.t. act(BN(x))
            return (ga,) + _bn_backward(ctx, ga, x, gamma, beta, mean, invstd, need_p)

        bn, gw, gb = _conv_backward(ctx, x, w, gy.contiguous(), need[0] or need_p, need[3], need[4],
                                    aff=(scale, shift, ctx.act, bound), then=bn_backward)
        # ga stays referenced until this backward returns: the allocator hands the weight gradient's temporaries the same
        # blocks as when the three steps were written out here
        _ga, gx, dg, db = bn if bn is not None else (None,) * 4
        return gx, dg, db, gw, gb, None, None, None, None, None, None, None, None, None


def _bn_eval_backward(ctx, gy, x, scale, shift, mean, invstd, need_p, key):
    """vg_bn_eval_act_bwd with the parameter gradients under the accumulate protocol (BNEvalActFn, BNEvalConvFn); ``key``:
    id of the layer's gamma, as in `_bn_backward`."""
    slot = _grad_slot(ctx.acc if need_p else None, key)
    gx, dg, db = ops.bn_eval_act_bwd(gy, x, scale, shift, mean, invstd, ctx.act, need_p, accumulate_into=slot.prev)
    return (gx,) + (slot.hand_over((dg, db)) if need_p else (dg, db))


def _frozen(ctx, running_mean):
    """The running mean as the backward will need it: a copy where a backward can follow (the buffer may move before
    it), the buffer itself where none can (inference: no copy launch per layer)."""
    return running_mean.clone() if any(ctx.needs_input_grad) else running_mean


class BNEvalActFn(Function):
    """Eval-mode BatchNorm1d/2d (running statistics, F.batch_norm(training=False)) + {none, ReLU, LeakyReLU(0.2)},
    materialised: one coefficient launch, one normalise pass.  The running buffers are read and never written.  The
    Function keeps its own scale / shift / invstd and a copy of the running mean: a train-mode step between forward and
    backward moves the buffers and must not move the gradient.
    Returns (y, the bound slot of max |y| the normalise pass emitted -- non-differentiable -- or None)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, eps, act):
        scale, shift, invstd = ops.bn_eval_coeffs(gamma, beta, running_mean, running_var, eps, act)
        y = ops.affine_act(x, scale, shift, act)
        ctx.act, ctx.key = act, id(gamma)
        ctx.acc = _acc_ctx()
        ctx.save_for_backward(x, scale, shift, invstd, _frozen(ctx, running_mean))
        bound = ops.known_amax(y)
        if bound is not None:
            ctx.mark_non_differentiable(bound)
        ctx.set_materialize_grads(False)      # as ConvStatsFn
        return y, bound

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _):
        if gy is None:
            return (None,) * 7
        x, scale, shift, invstd, mean = ctx.saved_tensors
        need_p = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        gx, dg, db = _bn_eval_backward(ctx, gy.contiguous(), x, scale, shift, mean, invstd, need_p, ctx.key)
        return gx, dg, db, None, None, None, None


class BNEvalConvFn(Function):
    """[eval-mode BatchNorm2d + activation] -> [5x5 conv / transposed conv], the normalised tensor never materialised:
    `BNConvFn` with the coefficients from the running statistics (one small launch, no finalisation, no buffer update).
    ``stats_in``: the statistics slots the producing convolution left of x -- they no longer decide the coefficients,
    they give the fp16 planes' bound of max |act(BN(x))| without a pass over x (vg_bn_eval_coeffs); without them
    `ops.amax_of` measures x through the affine.  Backward: data gradient of the convolution, then the frozen-statistics
    BatchNorm backward against the saved raw x; the weight gradient reads x through the same affine.
    Returns (y, statistics slots of y -- empty when the kernel cannot emit them)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w, bias, running_mean, running_var, eps, act, stride, transposed, bias_grad, stats_in):
        count = x.numel() // x.shape[1]
        scale, shift, invstd, bound = ops.bn_eval_coeffs(gamma, beta, running_mean, running_var, eps, act, stats_in, count,
                                                         want_bound=True)
        conv = ops.convT5x5_fwd if transposed else ops.conv5x5_fwd
        y, stats = conv(x, w, bias, stride, in_affine=(scale, shift, act, bound), want_stats=True)
        stats = stats if stats is not None else x.new_empty(0)
        ctx.act, ctx.stride, ctx.transposed, ctx.bias_grad, ctx.key = act, stride, transposed, bias_grad, id(gamma)
        ctx.acc = _acc_ctx()
        ctx.save_for_backward(x, scale, shift, invstd, _frozen(ctx, running_mean), w, bound)
        ctx.mark_non_differentiable(stats)
        ctx.set_materialize_grads(False)      # as ConvStatsFn
        return y, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _):
        if gy is None:
            return (None,) * 13
        x, scale, shift, invstd, mean, w, bound = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_p = need[1] or need[2]

        def bn_backward(ga):                                 # ga: the gradient w.r.t. act(BN(x))
            return (ga,) + _bn_eval_backward(ctx, ga, x, scale, shift, mean, invstd, need_p, ctx.key)

        bn, gw, gb = _conv_backward(ctx, x, w, gy.contiguous(), need[0] or need_p, need[3], need[4],
                                    aff=(scale, shift, ctx.act, bound), then=bn_backward)
        _ga, gx, dg, db = bn if bn is not None else (None,) * 4
        return gx, dg, db, gw, gb, None, None, None, None, None, None, None, None


class BiasActFn(Function):
    """y = act(x + bias[c]) for LeakyReLU(0.2) / tanh / sigmoid -- model.py:404, 509, 408."""

    @staticmethod
    def forward(ctx, x, bias, kind):
        y = ops.bias_act_fwd(x, bias, kind)
        ctx.kind = kind
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        gx = ops.act_bwd(gy.contiguous(), y, ctx.kind)
        gb = ops.channel_sum(gx) if ctx.needs_input_grad[1] else None
        return gx, gb, None


class ReparamKLFn(Function):
    """z = mu + eps*exp(logvar/2) and kl = beta*KL(q||N(0,1)) summed over the batch --
    model.py:532-535 + experiments/new_betavaegan.py:64-65, one fused kernel each way.  ``beta``: a float, or a
    one-element fp32 device tensor the kernels read (not differentiable; the backward reads the word as it is THEN: it
    changes between iterations, not inside one)."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, beta):
        z, kl, _ = ops.reparam_kl_fwd(mu, logvar, eps, beta)
        ctx.beta = beta      # (a tensor is kept as the word itself, not saved: it takes no gradient)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(mu, logvar, eps)
        return z, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, gkl):
        mu, logvar, eps = ctx.saved_tensors
        if gz is None and gkl is None:
            return None, None, None, None
        gz = gz.contiguous() if gz is not None else None
        gkl = gkl.contiguous() if gkl is not None else None
        gmu, glv = ops.reparam_kl_bwd(gz, mu, logvar, eps, gkl, ctx.beta)
        return gmu, glv, None, None


class _ReparamObjectiveFn(Function):
    """What `ReparamTCFn`, `ReparamDIPFn`, `ReparamMMDFn` and `ReparamKLCFn` share: the end of the forward (`_finish`) and
    the whole backward.  A subclass's ``forward`` calls its `ops` forward and hands `_finish` what the backward needs:
    ``ops.<bwd>(gz, *saved, gloss, beta, *kept)``.  ``beta``: a float or the device word, as `ReparamKLFn` (a tensor is kept
    as the word itself, not saved: it takes no gradient)."""

    @staticmethod
    def _finish(ctx, z, out4, bwd, saved, beta, kept, nargs, extra=()):
        """``bwd``: the name of the backward in `ops` (looked up when it runs); ``nargs``: how many arguments the forward took;
        ``extra``: further outputs behind ``parts`` that take no gradient either."""
        ctx.bwd, ctx.beta, ctx.kept, ctx.nargs = bwd, beta, kept, nargs
        loss, parts = out4[0], out4[1:]
        ctx.mark_non_differentiable(parts, *extra)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(*saved)
        return (z, loss, parts, *extra)

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, gloss, *_):
        if gz is None and gloss is None:
            return (None,) * ctx.nargs
        gz = gz.contiguous() if gz is not None else None
        gloss = gloss.contiguous() if gloss is not None else None
        gmu, glv = getattr(ops, ctx.bwd)(gz, *ctx.saved_tensors, gloss, ctx.beta, *ctx.kept)
        return (gmu, glv) + (None,) * (ctx.nargs - 2)


class ReparamTCFn(_ReparamObjectiveFn):
    """z = mu + eps*exp(logvar/2) and the beta-TCVAE decomposition of the KL term by minibatch-weighted sampling
    (Chen et al. 2018): ``loss = alpha*mi + beta*tc + gamma*dwkl``, all three summed over the
    batch, in one fused kernel pair each way.  Returns ``z``, ``loss`` and the non-differentiable ``[3]`` tensor
    ``(mi, tc, dwkl)``.  ``beta``: a float or the device word, as `ReparamKLFn`; ``log_bn`` = log(B * dataset size)
    moves the values of the parts and no gradient."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, beta, alpha, gamma, log_bn):
        z, out4, lse_joint, lse_dim = ops.reparam_tc_fwd(mu, logvar, eps, beta, alpha, gamma, log_bn)
        return ReparamTCFn._finish(ctx, z, out4, "reparam_tc_bwd", (mu, logvar, eps, z, lse_joint, lse_dim), beta,
                                   (alpha, gamma), 7)


class ReparamDIPFn(_ReparamObjectiveFn):
    """z = mu + eps*exp(logvar/2) and the DIP-VAE objective (Kumar et al. 2018):
    ``loss = beta*kl + B*(lambda_od*od + lambda_d*dg)`` with ``od`` / ``dg`` the off-diagonal / diagonal distance of the
    aggregate posterior's covariance from the identity, in three launches forward and one backward.  Returns ``z``,
    ``loss`` and the non-differentiable ``[3]`` tensor ``(kl, od, dg)``.  ``beta``: a float or the device word, as
    `ReparamKLFn`; ``variant``: ``"i"`` (the covariance of the means) or ``"ii"`` (of z)."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, beta, lambda_od, lambda_d, variant):
        z, out4, cov, mean = ops.reparam_dip_fwd(mu, logvar, eps, beta, lambda_od, lambda_d, variant)
        return ReparamDIPFn._finish(ctx, z, out4, "reparam_dip_bwd", (mu, logvar, eps, cov, mean), beta,
                                    (lambda_od, lambda_d, variant), 7)


class ReparamMMDFn(_ReparamObjectiveFn):
    """z = mu + eps*exp(logvar/2) and the InfoVAE / WAE-MMD objective (Zhao et al. 2019, Tolstikhin et al. 2018; DESIGN.md
    section 4.23): ``loss = beta*kl + B*lambda_mmd*mmd`` with ``mmd`` the unbiased maximum mean discrepancy between the
    batch of z and the prior draws ``zp``, in three launches forward and one backward.  Returns ``z``, ``loss`` and the
    non-differentiable ``[3]`` tensor ``(kl, mmd, kzz)``.  ``beta``: a float or the device word, as `ReparamKLFn`; ``kind``:
    1 (rbf) or 2 (imq); ``bandwidths``: a tuple of floats.  ``zp`` takes no gradient."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, zp, beta, lambda_mmd, kind, bandwidths):
        z, out4, w = ops.reparam_mmd_fwd(mu, logvar, eps, zp, beta, lambda_mmd, kind, bandwidths)
        return ReparamMMDFn._finish(ctx, z, out4, "reparam_mmd_bwd", (mu, logvar, eps, z, zp, w), beta,
                                    (lambda_mmd, kind, bandwidths), 8)


class ReparamKLCFn(_ReparamObjectiveFn):
    """z = mu + eps*exp(logvar/2) and the controlled KL term (Burgess et al. 2018 over Kingma et al. 2016's free bits;
    DESIGN.md section 4.30): ``loss = beta*|T - B*capacity|`` with ``T = sum_d max(K[d], B*free_bits)``, ``K[d]`` the
    dimension's KL summed over the batch, in two launches forward and one backward.  Returns ``z``, ``loss``, the
    non-differentiable ``[3]`` tensor ``(kl, kl_floored, dims_above)`` and the non-differentiable ``[D]`` tensor ``kl_dim`` =
    K / B.  ``beta`` and ``capacity``: both floats or both device words (kept as the words themselves, as `ReparamKLFn`'s
    beta); ``free_bits``: a float."""

    @staticmethod
    def forward(ctx, mu, logvar, eps, beta, capacity, free_bits):
        z, out4, gate, kl_dim = ops.reparam_klc_fwd(mu, logvar, eps, beta, capacity, free_bits)
        return ReparamKLCFn._finish(ctx, z, out4, "reparam_klc_bwd", (mu, logvar, eps, gate), beta, (capacity, free_bits), 6,
                                    extra=(kl_dim,))


class KLRowsFn(Function):
    """Encoder_celeba's per-sample KL (model.py:321) together with z."""

    @staticmethod
    def forward(ctx, mu, logvar, eps):
        z, _, rows = ops.reparam_kl_fwd(mu, logvar, eps, 1.0, want_rows=True)
        ctx.mark_non_differentiable(rows)
        ctx.save_for_backward(mu, logvar, eps)
        ctx.set_materialize_grads(False)      # no zero-filled "gradient" of the rows
        return z, rows

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, _):
        if gz is None:
            return None, None, None
        mu, logvar, eps = ctx.saved_tensors
        gmu, glv = ops.reparam_kl_bwd(gz.contiguous(), mu, logvar, eps, None, 1.0)
        return gmu, glv, None


class SqDiffLossFn(Function):
    """scale * sum((a-b)^2), gradient to ``a`` only (``b`` is a target).
    scale 0.5 = Dis_l / SIM (new_betavaegan.py:67-69), 1.0 = pixel MSE (:71-75)."""

    @staticmethod
    def forward(ctx, a, b, scale):
        loss, ga = ops.sqdiff_loss(a, b, scale, 1.0, want_grad=True)
        ctx.save_for_backward(ga)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        (ga,) = ctx.saved_tensors
        return ops.scale_by_scalar(ga, gout.contiguous()), None, None


class FactorTCFn(Function):
    """The encoder phase's FactorVAE loss (Kim & Mnih 2018) from the critic's logits on z and the
    unweighted KL scalar: ``loss = beta*kl + gamma*sum_b(l0 - l1)``, one launch each way.  Returns ``loss`` and the
    non-differentiable ``[3]`` tensor ``(kl, tc, rows with l0 > l1)``.  ``beta`` / ``gamma``: both floats or both device
    words (kept as the words themselves, as `ReparamKLFn`'s beta).  Gradient: ``+-gamma*gloss`` per row to the logits,
    ``beta*gloss`` to the KL; an absent ``gloss`` gives none."""

    @staticmethod
    def forward(ctx, logits, kl, beta, gamma):
        out4 = ops.factor_tc_fwd(logits, kl, beta, gamma)
        ctx.beta, ctx.gamma = beta, gamma
        loss, parts = out4[0], out4[1:]
        ctx.mark_non_differentiable(parts)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(logits)
        return loss, parts

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss, _):
        if gloss is None:
            return None, None, None, None
        (logits,) = ctx.saved_tensors
        glogits, gkl = ops.factor_tc_bwd(logits, gloss.contiguous(), ctx.beta, ctx.gamma)
        return glogits, gkl, None, None


class FactorCriticLossFn(Function):
    """The critic phase's cross-entropy on the logits of ``[z; z_perm]``, forward and gradient in one launch (as
    `SqDiffLossFn` / `BCELossFn`); ``divisor``: what the sum of the 2B terms is divided by.  Returns ``(loss, acc)``; ``acc``,
    the fraction of the rows on the right side of 0, takes no gradient."""

    @staticmethod
    def forward(ctx, logits, divisor):
        loss, glogits, acc = ops.factor_critic_loss(logits, divisor, want_grad=True)
        ctx.save_for_backward(glogits)
        ctx.mark_non_differentiable(acc)
        ctx.set_materialize_grads(False)
        return loss, acc

    @staticmethod
    @once_differentiable
    def backward(ctx, gout, _):
        if gout is None:
            return None, None
        (glogits,) = ctx.saved_tensors
        return ops.scale_by_scalar(glogits, gout.contiguous()), None


class BCELossFn(Function):
    """nn.BCELoss() vs a constant label (new_betavaegan.py:53,97,101); ``divisor`` is the
    batch the mean runs over (the global batch under data parallelism)."""

    @staticmethod
    def forward(ctx, p, target, divisor):
        loss, gp = ops.bce_loss(p, target, divisor, 1.0, want_grad=True)
        ctx.save_for_backward(gp)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        (gp,) = ctx.saved_tensors
        return ops.scale_by_scalar(gp, gout.contiguous()), None, None


class DiffAugmentFn(Function):
    """Differentiable augmentation of an image batch (ops.diff_augment_fwd).  Given ``u`` the map is
    affine in ``x``: the backward is the transpose of its linear part, from ``gy`` and ``u`` alone -- ``u`` is all that is
    saved.  ``policy``: the bit set; ``u`` gets no gradient.  ``p``: a float, or the device word (a one-element fp32 tensor,
    DESIGN.md section 4.35), which is held by reference and read again when the backward runs: it must not change in
    between."""

    @staticmethod
    def forward(ctx, x, u, policy, p):
        ctx.save_for_backward(u)
        ctx.policy, ctx.p = policy, p
        return ops.diff_augment_fwd(x, u, policy, p)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (u,) = ctx.saved_tensors
        return ops.diff_augment_bwd(gy.contiguous(), u, ctx.policy, ctx.p), None, None, None


class DotSigmoidBCEFn(Function):
    """Linear(K -> 1) + Sigmoid + nn.BCELoss against a constant label in one launch each way (model.py:406-408,
    new_betavaegan.py:101,118,153-154).  Returns (p (B,), loss); p is not differentiable here (the iteration only reads
    it: mean D(x))."""

    @staticmethod
    def forward(ctx, feat, w, bias, target, divisor):
        p, loss, dlogit = ops.dot_sigmoid_bce_fwd(feat, w, bias, target, divisor, want_grad=True)
        ctx.save_for_backward(feat, w, dlogit)
        ctx.acc = _acc_ctx()
        ctx.has_bias = bias is not None
        ctx.mark_non_differentiable(p)
        ctx.set_materialize_grads(False)
        return p, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, _gp, gloss):
        if gloss is None:
            return None, None, None, None, None
        feat, w, dlogit = ctx.saved_tensors
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        slot = _grad_slot(ctx.acc if (need_w and need_b) else None, id(w))
        gfeat, gw, gb = ops.dot_sigmoid_bce_bwd(dlogit, gloss.contiguous(), feat, w, ctx.needs_input_grad[0], need_w, need_b,
                                                accumulate_into=slot.prev)
        return (gfeat,) + slot.hand_over((gw, gb)) + (None, None)


# Adversarial losses on the logit: (name, role) -> the kernel's kind.  role: which term of the
# iteration the call is -- "real" / "fake": the discriminator's two (phase 1), "gen": every generator-side term.
GAN_LOSS_NAMES = ("logistic", "hinge", "lsgan")
GAN_ROLES = ("real", "fake", "gen")
GAN_LOSSES = {
    ("logistic", "real"): ops.GAN_LOGISTIC, ("logistic", "fake"): ops.GAN_LOGISTIC, ("logistic", "gen"): ops.GAN_LOGISTIC,
    ("lsgan", "real"): ops.GAN_LSGAN, ("lsgan", "fake"): ops.GAN_LSGAN, ("lsgan", "gen"): ops.GAN_LSGAN,
    ("hinge", "real"): ops.GAN_HINGE_REAL, ("hinge", "fake"): ops.GAN_HINGE_FAKE, ("hinge", "gen"): ops.GAN_HINGE_GEN,
}


def gan_loss_name(name):
    """``name`` if it is one of `GAN_LOSS_NAMES`; a ValueError that lists them otherwise."""
    if name not in GAN_LOSS_NAMES:
        raise ValueError(f"gan_loss: unknown loss {name!r}; one of " + ", ".join(repr(n) for n in GAN_LOSS_NAMES))
    return name


def gan_loss_kind(name, role):
    """The kernel's kind for loss ``name`` in ``role``; ``name`` may already be a kind (an int)."""
    if isinstance(name, int) and not isinstance(name, bool):
        return name
    gan_loss_name(name)
    if role not in GAN_ROLES:
        raise ValueError(f"gan_loss: unknown role {role!r}; one of " + ", ".join(repr(r) for r in GAN_ROLES))
    return GAN_LOSSES[(name, role)]


class GanLossFn(Function):
    """A GAN loss of a logit vector against a constant label (ops.gan_loss), forward and gradient in one launch as
    `BCELossFn`.  Returns (p = sigmoid(logit), loss); p is for logging and takes no gradient."""

    @staticmethod
    def forward(ctx, logit, kind, target, divisor):
        p, loss, glogit = ops.gan_loss(logit, kind, target, divisor, 1.0, want_grad=True)
        ctx.save_for_backward(glogit)
        ctx.mark_non_differentiable(p)
        ctx.set_materialize_grads(False)
        return p, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, _gp, gout):
        if gout is None:
            return None, None, None, None
        (glogit,) = ctx.saved_tensors
        return ops.scale_by_scalar(glogit, gout.contiguous()), None, None, None


class DotGanLossFn(Function):
    """Linear(K -> 1) + a GAN loss of its logit against a constant label in one launch each way, as `DotSigmoidBCEFn`
    (whose backward kernel this one uses: it takes any dlogit).  Returns (logit (B,), p = sigmoid(logit), loss); logit and
    p are not differentiable here (the iteration only reads them)."""

    @staticmethod
    def forward(ctx, feat, w, bias, kind, target, divisor):
        logit, p, loss, dlogit = ops.dot_gan_loss_fwd(feat, w, bias, kind, target, divisor, want_grad=True)
        ctx.save_for_backward(feat, w, dlogit)
        ctx.acc = _acc_ctx()
        ctx.has_bias = bias is not None
        ctx.mark_non_differentiable(logit, p)
        ctx.set_materialize_grads(False)
        return logit, p, loss

    @staticmethod
    @once_differentiable
    def backward(ctx, _glogit, _gp, gloss):
        if gloss is None:
            return None, None, None, None, None, None
        feat, w, dlogit = ctx.saved_tensors
        need_w, need_b = ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2]
        slot = _grad_slot(ctx.acc if (need_w and need_b) else None, id(w))
        gfeat, gw, gb = ops.dot_sigmoid_bce_bwd(dlogit, gloss.contiguous(), feat, w, ctx.needs_input_grad[0], need_w, need_b,
                                                accumulate_into=slot.prev)
        return (gfeat,) + slot.hand_over((gw, gb)) + (None, None, None)


# ------------------------------------------------------------ functional API
def conv5x5(x, w, bias, stride, bias_grad=BIAS_GRAD_COMPUTE):
    return ConvFn.apply(x, w, bias, stride, False, bias_grad)


def conv_transpose5x5(x, w, bias, stride, bias_grad=BIAS_GRAD_COMPUTE):
    return ConvFn.apply(x, w, bias, stride, True, bias_grad)


def linear(x, w, bias, bias_grad=BIAS_GRAD_COMPUTE):
    return LinearFn.apply(x.contiguous(), w, bias, bias_grad)


def linear_grouped(xs, w, bias, bias_grad=BIAS_GRAD_COMPUTE, detached=None):
    """[linear(x, w, bias) for x in xs] with the weight read once (LinearGroupedFn) where the layer runs on this package's
    GEMM and there are 2..3 inputs of one shape; pass by pass otherwise.  ``detached[g]``: pass g is made under no_grad."""
    detached = tuple(bool(d) for d in detached) if detached is not None else (False,) * len(xs)
    xs = [x.contiguous() for x in xs]
    grouped = (2 <= len(xs) <= ops.GEMM_MAX_GROUPS and all(x.dim() == 2 and x.shape == xs[0].shape for x in xs)
               and ops.linear_split_ok(xs[0].shape[1], w.numel()) and ops.linear_split_ok(w.shape[0], w.numel()))
    if grouped:
        return list(LinearGroupedFn.apply(w, bias, bias_grad, detached, *xs))
    outs = []
    for x, det in zip(xs, detached):
        with torch.set_grad_enabled(torch.is_grad_enabled() and not det):
            outs.append(LinearFn.apply(x, w, bias, bias_grad))
    return outs


def batch_norm_act(x, gamma, beta, running_mean, running_var, eps=1e-5, momentum=0.1, act=ops.ACT_NONE, stats=None):
    y, bound = BNActFn.apply(x, gamma, beta, running_mean, running_var, eps, momentum, act,
                             stats if stats is not None and stats.numel() else None)
    if bound is not None:
        ops.set_amax(y, bound)
    return y


def conv_with_stats(x, w, bias, stride, transposed=False, bias_grad=BIAS_GRAD_COMPUTE):
    """(y, statistics slots of y) -- see ConvStatsFn."""
    return ConvStatsFn.apply(x, w, bias, stride, transposed, bias_grad)


def bn_act_conv(x, gamma, beta, running_mean, running_var, eps, momentum, act, w, bias, stride, transposed=False,
                bias_grad=BIAS_GRAD_COMPUTE, stats_in=None):
    """conv(act(BN_train(x))) with nothing materialised in between -- see BNConvFn.  Returns (y, stats of y)."""
    return BNConvFn.apply(x, gamma, beta, w, bias, running_mean, running_var, eps, momentum, act, stride, transposed,
                          bias_grad, stats_in)


def batch_norm_eval_act(x, gamma, beta, running_mean, running_var, eps=1e-5, act=ops.ACT_NONE):
    """act(BN_eval(x)) on the running statistics, materialised -- see BNEvalActFn."""
    y, bound = BNEvalActFn.apply(x, gamma, beta, running_mean, running_var, eps, act)
    if bound is not None:
        ops.set_amax(y, bound)
    return y


def bn_eval_act_conv(x, gamma, beta, running_mean, running_var, eps, act, w, bias, stride, transposed=False,
                     bias_grad=BIAS_GRAD_COMPUTE, stats_in=None):
    """conv(act(BN_eval(x))) with nothing materialised in between -- see BNEvalConvFn.  Returns (y, stats of y)."""
    return BNEvalConvFn.apply(x, gamma, beta, w, bias, running_mean, running_var, eps, act, stride, transposed, bias_grad,
                              stats_in)


def bias_act(x, bias, kind):
    return BiasActFn.apply(x, bias, kind)


def _beta_arg(beta):
    return beta.detach() if isinstance(beta, torch.Tensor) else float(beta)


def reparam_kl(mu, logvar, eps, beta):
    return ReparamKLFn.apply(mu, logvar, eps, _beta_arg(beta))


def reparam_tc(mu, logvar, eps, beta, alpha=1.0, gamma=1.0, dataset_size=None):
    """`ReparamTCFn`: ``(z, loss, parts)`` with ``loss = alpha*mi + beta*tc + gamma*dwkl`` and ``parts = (mi, tc, dwkl)``.
    ``dataset_size``: the N of minibatch-weighted sampling, the number of samples the batch was drawn from."""
    if dataset_size is None or not dataset_size >= 1:
        raise ValueError(f"reparam_tc: dataset_size must be the number of training samples (>= 1), got {dataset_size!r}")
    log_bn = math.log(float(mu.shape[0]) * float(dataset_size))
    return ReparamTCFn.apply(mu, logvar, eps, _beta_arg(beta), float(alpha), float(gamma), log_bn)


def reparam_dip(mu, logvar, eps, beta, lambda_od, lambda_d, variant="i"):
    """`ReparamDIPFn`: ``(z, loss, parts)`` with ``loss = beta*kl + B*(lambda_od*od + lambda_d*dg)`` and ``parts = (kl, od,
    dg)``; ``variant``: ``"i"`` or ``"ii"``."""
    return ReparamDIPFn.apply(mu, logvar, eps, _beta_arg(beta), float(lambda_od), float(lambda_d), ops.dip_variant(variant))


def reparam_mmd(mu, logvar, eps, zp, beta, lambda_mmd, kernel="imq", bandwidths=None):
    """`ReparamMMDFn`: ``(z, loss, parts)`` with ``loss = beta*kl + B*lambda_mmd*mmd`` and ``parts = (kl, mmd, kzz)``;
    ``zp``: draws from the prior, one per sample; ``kernel``: ``"rbf"`` or ``"imq"``; ``bandwidths``: ``None`` for WAE's
    defaults (`ops.mmd_bandwidths`) or 1 to 8 positive numbers."""
    kind = ops.mmd_kernel(kernel)
    return ReparamMMDFn.apply(mu, logvar, eps, zp, _beta_arg(beta), float(lambda_mmd), kind,
                              ops.mmd_bandwidths(kind, mu.shape[-1], bandwidths))


def reparam_klc_dims(mu, logvar, eps, beta, capacity=0.0, free_bits=0.0):
    """`ReparamKLCFn`: ``(z, loss, parts, kl_dim)`` with ``loss = beta*|kl_floored - B*capacity|``, ``parts = (kl, kl_floored,
    dims_above)`` and ``kl_dim`` the [D] per-dimension KL averaged over the batch (which dimensions are active, which
    collapsed).  ``capacity``: nats per sample, a float -- or, with ``beta`` a device word, a device word too;
    ``free_bits``: nats per dimension per sample, a float."""
    return ReparamKLCFn.apply(mu, logvar, eps, _beta_arg(beta), _beta_arg(capacity), ops.kl_free_bits(free_bits))


def reparam_klc(mu, logvar, eps, beta, capacity=0.0, free_bits=0.0):
    """`reparam_klc_dims` without ``kl_dim``: ``(z, loss, parts)``, as the other objectives."""
    return reparam_klc_dims(mu, logvar, eps, beta, capacity, free_bits)[:3]


def permute_dims(z, u):
    """FactorVAE's ``permute_dims`` (`ops.permute_dims`): every column of ``z`` permuted across the batch by the stable argsort
    of the same column of the uniforms ``u``.  A sample of the product of the marginals: no gradient flows (``z`` is taken
    detached)."""
    return ops.permute_dims(z.detach().contiguous(), u.contiguous())


def factor_tc(logits, kl, beta, gamma):
    """`FactorTCFn`: ``(loss, parts)`` with ``loss = beta*kl + gamma*tc``, ``tc = sum_b (l0 - l1)`` and ``parts = (kl, tc, rows
    with l0 > l1)``.  ``logits``: the critic's [B, 2] on z; ``kl``: the unweighted KL scalar (``reparam_kl(..., 1.0)``); ``beta``
    / ``gamma``: both floats or both device words."""
    return FactorTCFn.apply(logits.contiguous(), kl, _beta_arg(beta), _beta_arg(gamma))


def factor_critic_loss(logits, divisor=None):
    """`FactorCriticLossFn`: ``(loss, acc)`` of the critic on the logits [2B, 2] of ``[z; z_perm]``; ``divisor``: default the
    2B rows (a mean), twice the global batch under data parallelism."""
    return FactorCriticLossFn.apply(logits.contiguous(), divisor)


def kld_loss(mu, logvar, beta):
    """KLD of experiments/new_betavaegan.py:64-65 (no sampling)."""
    _, kl = ReparamKLFn.apply(mu, logvar, torch.zeros_like(mu), _beta_arg(beta))
    return kl


def sim_loss(sim_recon, sim_real):
    """SIM / Dis_l of new_betavaegan.py:67-69.  ``sim_real`` is a target (the reference
    leaves it attached, but only the discriminator -- whose gradients are discarded
    in that phase -- would receive anything through it)."""
    return SqDiffLossFn.apply(sim_recon, sim_real.detach(), 0.5)


def reconstruction_loss(recon_x, x):
    """new_betavaegan.py:71-75."""
    return SqDiffLossFn.apply(recon_x, x.detach(), 1.0)


def bce_loss(p, label_value, divisor=None):
    """``label_value``: a float, or a one-element device tensor (see ops.bce_loss)."""
    if not isinstance(label_value, torch.Tensor):
        label_value = float(label_value)
    return BCELossFn.apply(p.contiguous(), label_value, divisor)


def dot_sigmoid_bce(feat, w, bias, label_value, divisor=None):
    """(p, bce): see DotSigmoidBCEFn.  ``w`` (1, K) or (K,), ``bias`` (1,)."""
    if not isinstance(label_value, torch.Tensor):
        label_value = float(label_value)
    return DotSigmoidBCEFn.apply(feat.contiguous(), w, bias, label_value, divisor)


def gan_loss(logit, kind, label_value, divisor=None):
    """(p, loss) of a logit vector: see GanLossFn.  ``kind``: an ops.GAN_* code (`gan_loss_kind(name, role)`);
    ``label_value`` as in `bce_loss` -- the hinge kinds ignore it."""
    if not isinstance(label_value, torch.Tensor):
        label_value = float(label_value)
    return GanLossFn.apply(logit.contiguous(), kind, label_value, divisor)


def dot_gan_loss(feat, w, bias, kind, label_value, divisor=None):
    """(logit, p, loss): see DotGanLossFn.  ``w`` (1, K) or (K,), ``bias`` (1,)."""
    if not isinstance(label_value, torch.Tensor):
        label_value = float(label_value)
    return DotGanLossFn.apply(feat.contiguous(), w, bias, kind, label_value, divisor)



def diff_augment(x, u, policy="color,translation,cutout", p=1.0):
    """Differentiable augmentation (Zhao et al. 2020) of ``x`` [B, C, H, W] under ``u`` [B, 8] (`diff_augment_uniforms`):
    ``policy`` names the transforms (any order; applied as colour, translation, cutout), an image is transformed iff
    ``u[:, 7] < p``.  ``p``: a float in [0, 1], or a one-element fp32 device tensor the kernels read when they run (the word
    `ops.ada_update` moves).  Differentiable in ``x``; see DiffAugmentFn."""
    if not isinstance(p, torch.Tensor):
        p = ops.augment_probability(p)
    return DiffAugmentFn.apply(x.contiguous(), u, ops.augment_policy(policy), p)


def diff_augment_uniforms(batch, device, generator=None, sets=None):
    """The uniforms of `diff_augment` for ``batch`` images: [batch, 8] in [0, 1), or [sets, batch, 8] -- one parameter set per
    call of an iteration -- from ``generator`` (default: the device's global stream)."""
    shape = (batch, ops.AUGMENT_UNIFORMS) if sets is None else (sets, batch, ops.AUGMENT_UNIFORMS)
    return torch.rand(shape, device=device, generator=generator)
