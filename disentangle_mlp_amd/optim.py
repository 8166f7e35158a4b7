"""``optim.Adam`` of /root/reference/experiments/new_betavaegan.py:49-50 with its step on the
hand-written HIP kernel (``vg_adam_step``).

``HipAdam`` IS a ``torch.optim.Adam``: same constructor defaults, ``param_groups``, per-parameter
``state`` (``step``, ``exp_avg``, ``exp_avg_sq``) and ``state_dict`` / ``load_state_dict`` -- the
reference's optimizer checkpoints load into it and its own load into ``torch.optim.Adam``.  Only
``step()`` is replaced: one multi-tensor launch per 24 parameters instead of torch's fused
``multi_tensor_apply``.  Configurations the kernel does not implement (amsgrad, maximize, a
closure, non-fp32 / non-contiguous / CPU tensors) take the inherited ``step()``.

``HipAdam(nonfinite_guard=True)``: the step also reports, per parameter, an inf / NaN among the gradients it read
(`NONFINITE_GRAD`) and the parameters it wrote (`NONFINITE_PARAM`) -- ``vg_adam_step_checked`` -- in device words the
host reads when it chooses to (`nonfinite`, `nonfinite_words`, `clear_nonfinite`).  By itself it detects, it does not
skip the update: when a PARAM bit is up the weights are poisoned and the last good checkpoint is the way back.
``skip_nonfinite=True`` (below) is the opt-in that prevents the damage.

``HipAdam(max_grad_norm=c, skip_nonfinite=bool)``: one deterministic pass over the gradients in front of the step
(``vg_grad_sumsq_multi`` + ``vg_grad_clip_finalize``) leaves their global L2 norm, the coefficient ``min(1, c / (norm +
1e-6))`` of ``torch.nn.utils.clip_grad_norm_`` and a skip decision in a four-word device record; the fused step
(``vg_adam_step_clip``) scales every gradient by the coefficient in registers -- the gradients themselves are never
written -- and, with ``skip_nonfinite``, stores nothing at all when the norm is inf / NaN.  No host synchronisation:
the whole of it is capturable.  `grad_norm`, `clip_coef` (device views), `skipped_steps`, `reset_skipped`.

``HipAdam(ema_decay=d)``: the step also keeps an exponential moving average of the weights it writes, ``e <- e +
(1 - d) (p - e)`` -- inside the same kernel (``vg_adam_step_ema``), from the value the thread has just formed, so the
average costs 8 bytes per parameter and no launch of its own.  The averages live in tensors fixed at construction
(fp32 clones, or the caller's ``ema_targets``: a trainer's shadow module), are NOT part of ``state_dict()`` -- that
stays torch.optim.Adam's -- and travel through `ema_state` / `load_ema_state`.

``HipAdam(weight_decay=w, decoupled_weight_decay=bool)``: the fused step decays the weights itself
(``vg_adam_step_decay``) -- coupled (L2) ``g + w p`` or decoupled (AdamW) ``p (1 - lr w)``, in registers, no memory
traffic of its own.  Groups without decay make the launches they always made.

``HipAdam(capturable=True, device_hyper=True)``: every group's ``[lr, weight_decay]`` lives in a persistent device pair
the step's prepare kernel reads (``vg_adam_prepare_dev``), so both may change between the replays of a captured step:
set ``group["lr"]`` (or let a ``torch.optim.lr_scheduler`` do it) and call `sync_hyper` before the replay.

``HipAdam(capturable=True, ema_decay=d, ema_decay_on_device=True)``: ``(float)(1 - d)`` lives in one persistent fp32
device word the averaging step reads (``vg_adam_step_dev_ema_dev``), so the decay too may change between the replays of
a captured step -- a warm-up: `set_ema_decay`, then `sync_hyper` before the replay.  Here ``d`` may be 0: the average
then takes the bits of the weights.
"""
import ctypes
import math

import torch
from torch import optim

from . import _lib, ops
from ._lib import check


NONFINITE_GRAD, NONFINITE_PARAM = 1, 2      # VG_NONFINITE_* of include/vaegan_hip.h


@torch.no_grad()
def isfinite_bits(params, device=None):
    """The guard's bits formed by torch: int32, one per parameter -- `NONFINITE_GRAD` when ``p.grad`` holds an inf / NaN
    now, `NONFINITE_PARAM` when ``p`` does.  For steps the kernel does not ride on (torch.optim.Adam, CPU)."""
    params = list(params)
    device = device if device is not None else (params[0].device if params else "cpu")
    if not params:
        return torch.zeros(0, dtype=torch.int32, device=device)
    bits = []
    for p in params:
        b = (~torch.isfinite(p.detach()).all()).to(torch.int32) * NONFINITE_PARAM
        if p.grad is not None:
            b = b + (~torch.isfinite(p.grad).all()).to(torch.int32) * NONFINITE_GRAD
        bits.append(b.to(device))
    return torch.stack(bits)


_CLIP_CHUNK = 8192      # elements per workgroup, and per fp64 partial, of vg_grad_sumsq_multi (csrc/adam.hip: ACHUNK)


def _torch_total_norm(grads):
    """The global L2 norm as ``torch.nn.utils.clip_grad_norm_`` forms it."""
    fn = getattr(torch.nn.utils, "get_total_norm", None)
    if fn is not None:
        return fn(grads, 2.0)
    return torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g, 2.0) for g in grads]), 2.0)


class _AdamTensor(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p),
                ("n", ctypes.c_size_t), ("amax", ctypes.c_void_p)]


# The step's launch table, in priority order per kind of scalars: (entry point, device scalars?, the feature that selects
# it, the arguments it takes between the common prefix and the stream -- names of `HipAdam._launch`'s values).  The
# feature kernel behind clip and decay takes flag words, averages and a decay whether or not they are in use (NULL, 0.0).
_STEP_TABLE = (
    ("vg_adam_step_dev_ema_dev", True, "ema_dev", ("flags", "ema", "omd", "rec")),
    ("vg_adam_step_dev_decay", True, "decay", ("flags", "ema", "ema_decay", "rec")),
    ("vg_adam_step_dev_clip", True, "clip", ("flags", "ema", "ema_decay", "rec")),
    ("vg_adam_step_dev_ema", True, "ema", ("flags", "ema", "ema_decay")),
    ("vg_adam_step_dev_checked", True, "flags", ("flags",)),
    ("vg_adam_step_dev", True, None, ()),
    ("vg_adam_step_decay", False, "decay", ("flags", "ema", "ema_decay", "rec", "wd", "decoupled")),
    ("vg_adam_step_clip", False, "clip", ("flags", "ema", "ema_decay", "rec")),
    ("vg_adam_step_ema", False, "ema", ("flags", "ema", "ema_decay")),
    ("vg_adam_step_checked", False, "flags", ("flags",)),
    ("vg_adam_step", False, None, ()),
)


def step_entry(*, dev, flags, ema, ema_dev, decay, clip):
    """(entry point, its tail) of one launch -- a pure function of the features: ``dev`` the scalars come from the device
    (capturable); ``flags`` the guard's words; ``ema`` an average on this call; ``ema_dev`` its decay in the device word;
    ``decay`` the group's weight decay is not 0; ``clip`` there is a clip / skip record.  The first row of `_STEP_TABLE`
    for these scalars whose feature is on."""
    on = {"ema_dev": ema_dev, "decay": decay, "clip": clip, "ema": ema, "flags": flags, None: True}
    return next((name, tail) for name, on_dev, feature, tail in _STEP_TABLE if on_dev == bool(dev) and on[feature])


def prepare_entry(*, device_hyper, decay, ema_dev, prepared):
    """The kernel that forms a capturable step's scalars: ``vg_adam_prepare_dev`` when the step reads the group's device
    pair [lr, weight_decay] (``device_hyper``, a weight decay that is not 0, or the EMA decay on the device, whose step
    takes that route); else ``vg_adam_prepare`` -- or None when `HipAdam.begin_fused_step` has run it for this step."""
    if device_hyper or decay or ema_dev:
        return "vg_adam_prepare_dev"
    return None if prepared else "vg_adam_prepare"


def linear_adam_eligible(*, switch=True, grad_hook=False, exchange=False, update_ema=False, clip=False,
                         weight_decay=0.0, device_hyper=False, amsgrad=False, maximize=False, requires_grad=True,
                         dim=2, numel=0, in_features=0, native_tensor=True, split_ok=True):
    """Whether a Linear weight may take the fused weight-gradient + Adam launch (``vg_linear_wgrad_adam``) in the step
    that is about to begin -- a pure function of the switches.  The route is for the plain native step alone: no EMA on
    this call, no clip / skip record, no weight decay, no ``device_hyper``, not amsgrad / maximize; the trainer's side
    (``switch``: functional.FUSE_LINEAR_ADAM; a ``grad_hook`` wants to see the gradient; a FlatGrads ``exchange`` must
    reduce it first; a frozen weight gets none); and the entry point's own conditions on the weight (``split_ok``:
    `ops.linear_split_ok` takes the layer; rows of a multiple of 4 floats; a contiguous fp32 device tensor).  The
    conditions on the REDUCTION (a multiple of 32, not split over workgroups) are only known in the backward: the entry
    point refuses there and the backward falls back to the two launches."""
    if not switch or grad_hook or exchange:
        return False
    if update_ema or clip or float(weight_decay) != 0.0 or device_hyper or amsgrad or maximize:
        return False
    if not requires_grad or not native_tensor or dim != 2 or not split_ok:
        return False
    return in_features % 4 == 0 and numel % 4 == 0 and 0 < numel <= 0x7fffffff


class FusedLinearStep:
    """One weight's registration for one step (`HipAdam.begin_fused_step`): what `ops.linear_wgrad_adam` hands the
    entry point.  ``done``: the backward has updated the weight; ``open``: until the step() that closes it."""
    __slots__ = ("p", "m", "v", "amax", "flag", "scalars", "lr", "beta1", "beta2", "eps", "bc1", "bc2_sqrt", "gi", "step",
                 "born", "done", "open")

    def __init__(self, **kw):
        self.done, self.open = False, True
        for k, val in kw.items():
            setattr(self, k, val)


class HipAdam(optim.Adam):
    """``capturable=True``: the step's scalars (lr / bias_correction1, sqrt(bias_correction2)) are formed on the DEVICE
    by ``vg_adam_prepare`` -- from the host's step count in an eager step, from a device counter in a step that is being
    captured in a HIP graph (kernel arguments are frozen at capture, the step count is not) -- so a whole iteration
    including its optimizer steps can be captured and replayed (trainer.BetaVAEGANTrainer(graph=True)), and an eager step
    and a replayed one give the same bits.  The ``state_dict`` stays torch.optim.Adam's (``step`` as a CPU tensor): the
    host mirrors the device counter (`prepare_capture` / `replayed`)."""

    # What is laid out at construction, one slot per parameter or group -- so that a captured step writes where later
    # readers read -- and therefore refuses a later `add_param_group`: (the attribute that holds it, its constructor
    # argument as the message names it, what it is)
    _LAID_OUT = (("device_hyper", "device_hyper=True", "hyper-parameter words"),
                 ("_words", "nonfinite_guard=True", "flag words"),
                 ("_ema", "ema_decay=...", "EMA tensors"),
                 ("_clip_rec", "max_grad_norm=... / skip_nonfinite=True", "norm pass's partial sums"))

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, capturable=False,
                 nonfinite_guard=False, ema_decay=None, ema_targets=None, max_grad_norm=None, skip_nonfinite=False,
                 decoupled_weight_decay=False, device_hyper=False, ema_decay_on_device=False):
        if device_hyper and not capturable:
            raise ValueError("HipAdam: device_hyper=True keeps lr and weight decay on the device for a captured step; "
                             "it requires capturable=True")
        if ema_decay_on_device and not capturable:
            raise ValueError("HipAdam: ema_decay_on_device=True keeps the EMA decay on the device for a captured step; "
                             "it requires capturable=True")
        if ema_decay_on_device and ema_decay is None:
            raise ValueError("HipAdam: ema_decay_on_device=True without ema_decay")
        if max_grad_norm is not None and not (0.0 < float(max_grad_norm) < math.inf):      # (NaN fails both comparisons)
            raise ValueError(f"HipAdam: max_grad_norm must be finite and > 0, got {max_grad_norm!r}")
        if ema_decay_on_device:
            self._check_device_decay(ema_decay)
        elif ema_decay is not None and not (0.0 < float(ema_decay) < 1.0):      # (NaN fails both comparisons)
            raise ValueError(f"HipAdam: ema_decay must lie in (0, 1), got {ema_decay!r}")
        if ema_decay is None and ema_targets is not None:
            raise ValueError("HipAdam: ema_targets without ema_decay")
        # (what `add_param_group`, which torch's constructor calls, looks at: nothing is laid out yet)
        self.device_hyper, self._words, self._ema, self._ema_omd, self._clip_rec = False, None, None, None, None
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad,
                         foreach=False, fused=False, capturable=False, decoupled_weight_decay=decoupled_weight_decay)
        ps = self._params()
        device = ps[0].device
        self.device_scalars = bool(capturable)
        self._dev = {}            # group index -> (device step counter float64[1], scalars float32[4])
        self._fused = None        # the open registrations of `begin_fused_step`: ([FusedLinearStep], {group index: step})
        self._bound_masks = {}    # frozenset of bound-word indices the backward wrote -> bool mask of the words to zero
        self._captured = []       # per captured step() call: the parameters it stepped (host bookkeeping of a replay)
        self._debt = 0            # replays whose host-side step counts have not been added yet (flushed lazily)
        self.state_generation = 0 # bumped by load_state_dict: captured graphs point at the moment tensors of one generation
        # max |w| of the big Linear weights, emitted by the step itself (VgAdamTensor.amax) for the fp16x3 GEMMs that read
        # the weight next: one persistent fp32 word per weight, zeroed in front of every step (`_weight_bounds`)
        self._bound_of, self._bounds = {}, None      # parameter -> index into self._bounds
        self.register_state_dict_pre_hook(lambda opt: opt._flush_replays())
        # Every feature's device words are allocated here -- before any capture -- and never replaced (not by
        # load_state_dict either): a replayed step writes where the host later reads, and reads where it later writes.
        # -- non-finite guard: one int32 flag word per parameter, in param_groups order
        self.nonfinite_guard = bool(nonfinite_guard)
        self._word_of = {}        # parameter -> index into self._words
        self._torch_stepped = False      # torch's step() ran since the words were cleared: it cannot flag (see `nonfinite`)
        if self.nonfinite_guard:
            self._word_of = {p: i for i, p in enumerate(ps)}
            self._words = torch.zeros(len(ps), dtype=torch.int32, device=device)
        # -- weight EMA: one fp32 tensor per parameter, in param_groups order (a trainer's shadow module reads them); the
        # decay on the device: one fp32 word holding (float)(1 - decay), which the host writes in `sync_hyper`
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self._ema_of = {}         # parameter -> index into self._ema
        if self.ema_decay is not None:
            self._ema_of = {p: i for i, p in enumerate(ps)}
            self._ema = self._ema_tensors(ps, ema_targets)
            if ema_decay_on_device:
                self._ema_omd = torch.zeros(1, dtype=torch.float32, device=device)
                self._ema_omd_written = None
        # -- clipping by global norm / skipping a non-finite step: the record [norm, coef, skip, skipped] and one fp64
        # slot per 8192-element chunk of every parameter
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.skip_nonfinite = bool(skip_nonfinite)
        if self.max_grad_norm is not None or self.skip_nonfinite:
            self._clip_rec = torch.zeros(4, dtype=torch.float32, device=device)
            self._clip_rec[1] = 1.0
            slots = sum((p.numel() + _CLIP_CHUNK - 1) // _CLIP_CHUNK for p in ps)
            self._partials = torch.zeros(max(1, slots), dtype=torch.float64, device=device)
        # -- lr and weight decay on the device: one float64 pair [lr, weight_decay] per group, written in `sync_hyper`.
        # The step that reads the EMA decay from the device is prepared from them too: they exist and are written here
        self._hyper = {}          # group index -> float64[2] device tensor
        self._hyper_written = {}  # group index -> (lr, weight_decay) as last written
        self.device_hyper = bool(device_hyper)
        if self.device_hyper or self._ema_omd is not None:
            for gi in range(len(self.param_groups)):
                self._hyper_words(gi)
        if self._ema_omd is not None:
            self.sync_hyper()

    @staticmethod
    def _ema_tensors(ps, ema_targets):
        """The EMA tensors of ``ps``: fp32 clones, or the caller's ``ema_targets`` once they are seen to fit."""
        if ema_targets is None:
            return [p.detach().clone(memory_format=torch.contiguous_format) for p in ps]
        ema = [t.detach() if t.requires_grad else t for t in ema_targets]
        if len(ema) != len(ps):
            raise ValueError(f"HipAdam: {len(ema)} ema_targets for {len(ps)} parameters")
        for i, (t, p) in enumerate(zip(ema, ps)):
            if t.shape != p.shape or t.device != p.device or t.dtype != p.dtype or not t.is_contiguous():
                raise ValueError(f"HipAdam: ema_targets[{i}] must be a contiguous tensor of its parameter's "
                                 f"shape, device and dtype ({tuple(p.shape)}, {p.device}, {p.dtype})")
            if t.data_ptr() == p.data_ptr() and t.numel():
                raise ValueError(f"HipAdam: ema_targets[{i}] is its parameter's own storage")
        return ema

    def _params(self):
        """Every parameter, in ``param_groups`` order: the order of the flag words, the EMA tensors and `nonfinite`."""
        return [p for g in self.param_groups for p in g["params"]]

    def add_param_group(self, param_group):
        for attr, argument, what in self._LAID_OUT:
            if getattr(self, attr) is not None and getattr(self, attr) is not False:
                raise RuntimeError(f"HipAdam({argument}): the {what} are laid out at construction; "
                                   "pass every parameter group to the constructor")
        return super().add_param_group(param_group)

    # ---- lr and weight decay on the device --------------------------------------------------------------------
    def _hyper_words(self, gi):
        """Group ``gi``'s device pair [lr, weight_decay].  With ``device_hyper`` every pair exists from construction; a
        capturable optimizer without it gets one the first time a group with weight decay steps (its decay step reads
        the device scalars) -- outside a capture."""
        h = self._hyper.get(gi)
        if h is None:
            if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("HipAdam: weight decay appeared inside a capture; step once eagerly first")
            h = self._hyper[gi] = torch.zeros(2, dtype=torch.float64, device=self.param_groups[gi]["params"][0].device)
        return h

    def sync_hyper(self):
        """Write ``group["lr"]`` and ``group["weight_decay"]`` into the device words where they differ from what was last
        written: device fills, no synchronisation.  Every eager `step` and `prepare_capture` call it; whoever replays a
        captured step calls it in front of the replay.  Never inside a capture: a captured fill would freeze the value."""
        for gi, h in self._hyper.items():
            group = self.param_groups[gi]
            now = (float(group["lr"]), float(group["weight_decay"]))
            was = self._hyper_written.get(gi)
            if was is not None and self._captured and (was[1] != 0.0) != (now[1] != 0.0):
                raise RuntimeError("HipAdam: a captured step was recorded with or without the decay kernel; weight decay "
                                   "cannot be switched on or off under it (capture anew)")
            if now != was:
                h[0].fill_(now[0])
                h[1].fill_(now[1])
                self._hyper_written[gi] = now
        if self._ema_omd is not None and self.ema_decay != self._ema_omd_written:
            self._ema_omd.fill_(1.0 - self.ema_decay)      # (rounded once to fp32: the kernels' (float)(1 - decay))
            self._ema_omd_written = self.ema_decay

    # ---- weight EMA ------------------------------------------------------------------------------------------
    def _need_ema(self):
        if self._ema is None:
            raise RuntimeError("HipAdam: construct with ema_decay=... to track an EMA of the weights")

    @staticmethod
    def _check_device_decay(d):
        if not (0.0 <= float(d) < 1.0):      # (NaN fails both comparisons)
            raise ValueError(f"HipAdam: with ema_decay_on_device the decay must lie in [0, 1), got {d!r}")

    def set_ema_decay(self, d):
        """The decay of the next averaging steps, ``0 <= d < 1`` (0: the average takes the bits of the weights).  Needs
        ``ema_decay_on_device=True``; the device word follows at the next `sync_hyper` -- every eager `step` calls it,
        whoever replays a captured step calls it in front of the replay."""
        self._need_ema()
        if self._ema_omd is None:
            raise RuntimeError("HipAdam: construct with ema_decay_on_device=True to change the EMA decay")
        self._check_device_decay(d)
        self.ema_decay = float(d)

    def ema_tensors(self):
        """The EMA tensors themselves, one per parameter in ``param_groups`` order (the step writes them in place)."""
        self._need_ema()
        return list(self._ema)

    @torch.no_grad()
    def reset_ema(self):
        """EMA <- the parameters as they are now (after weights were loaded from a checkpoint without an average)."""
        self._need_ema()
        for e, p in zip(self._ema, self._params()):
            e.copy_(p)

    @torch.no_grad()
    def ema_state(self):
        """Clones of the EMA tensors, in ``param_groups`` order: what `load_ema_state` takes."""
        self._need_ema()
        return [e.clone() for e in self._ema]

    @torch.no_grad()
    def load_ema_state(self, tensors):
        """Copy ``tensors`` (parallel to `ema_tensors`) INTO the EMA tensors: their storage stays where it is."""
        self._need_ema()
        tensors = list(tensors)
        if len(tensors) != len(self._ema) or any(t.shape != e.shape for t, e in zip(tensors, self._ema)):
            raise ValueError("HipAdam.load_ema_state: one tensor per parameter, of the parameter's shape")
        for e, t in zip(self._ema, tensors):
            e.copy_(t)

    # ---- clipping by global norm, skipping a non-finite step ---------------------------------------------------
    def _need_clip(self):
        if self._clip_rec is None:
            raise RuntimeError("HipAdam: construct with max_grad_norm=... or skip_nonfinite=True")

    def grad_norm(self):
        """The global L2 norm of the gradients the last `step` read: a 0-dim fp32 VIEW of the device record (no host
        synchronisation; the next step overwrites it)."""
        self._need_clip()
        return self._clip_rec[0]

    def clip_coef(self):
        """The coefficient the last `step` scaled its gradients by (1.0 exactly when nothing was clipped, 0.0 in a
        skipped step): a 0-dim fp32 view of the device record, like `grad_norm`."""
        self._need_clip()
        return self._clip_rec[1]

    def clip_record(self):
        """The record itself, int32 view: words [norm bits, coef bits, skip, skipped] (a trainer reads several optimizers'
        counts in one copy)."""
        self._need_clip()
        return self._clip_rec.view(torch.int32)

    def skipped_steps(self):
        """Steps skipped (``skip_nonfinite``) since construction or `reset_skipped`.  One device -> host read."""
        return int(self.clip_record()[3])

    def reset_skipped(self):
        """`skipped_steps`, and the count back to zero."""
        n = self.skipped_steps()
        self.clip_record()[3] = 0
        return n

    @torch.no_grad()
    def _torch_clip(self, stepped):
        """The feature on torch's path.  Returns None when the step is skipped, else the list of gradients to step on
        (scaled copies when the clip is active: the gradients themselves stay as they are, as on the kernel's path).  The
        coefficient is ``clip_grad_norm_``'s own -- from torch's fp32 norm, by its fp32 expression, so the step is that
        recipe bit for bit; the RECORDED norm, and the skip decision, come from an fp64 sum of squares as the kernel's do
        (torch's fp32 norm of a tensor of 10^7 elements is good to about 10^-4 only).  One host read: this path is not
        capturable anyway."""
        grads = [p.grad for p in stepped]
        rec, words = self._clip_rec, self._clip_rec.view(torch.int32)
        if grads:
            norm64 = torch.linalg.vector_norm(torch.stack(
                [torch.linalg.vector_norm(g.detach().to_dense() if g.is_sparse else g.detach(), 2.0, dtype=torch.float64)
                 .to(rec.device) for g in grads]), 2.0)
        else:
            norm64 = torch.zeros((), dtype=torch.float64, device=rec.device)
        rec[0] = norm64.to(torch.float32)
        if self.skip_nonfinite and not bool(torch.isfinite(norm64)):
            rec[1] = 0.0
            words[2] = 1
            words[3] += 1
            return None
        words[2] = 0
        if self.max_grad_norm is None or not grads:
            rec[1] = 1.0
            return grads
        total = _torch_total_norm(grads)
        coef = torch.clamp(self.max_grad_norm / (total + 1e-6), max=1.0)      # torch.nn.utils.clip_grads_with_norm_
        rec[1] = coef.to(rec.device)
        return [g * coef.to(g.device) for g in grads]

    # ---- non-finite guard ----------------------------------------------------------------------------------
    def _need_guard(self):
        if not self.nonfinite_guard:
            raise RuntimeError("HipAdam: construct with nonfinite_guard=True to use the non-finite guard")

    def nonfinite_words(self):
        """The device tensor of flag words itself (int32, one per parameter in ``param_groups`` order; bits
        `NONFINITE_GRAD` | `NONFINITE_PARAM`): a trainer reads several optimizers' words in one copy."""
        self._need_guard()
        return self._words

    @torch.no_grad()
    def nonfinite_bits(self):
        """`nonfinite_words()`, completed -- when torch's own ``step()`` ran since the words were cleared (weight decay,
        amsgrad, a closure, CPU tensors: it cannot flag) -- with the same bits formed by ``torch.isfinite`` over every
        ``p.grad`` and ``p`` as they are now, so that an unguarded path never reads as clean.  No host synchronisation."""
        self._need_guard()
        if not self._torch_stepped:
            return self._words
        return self._words | isfinite_bits(self._params(), self._words.device)

    def nonfinite(self):
        """One device -> host read: ``{parameter: bits}`` of the words that are up; empty when the run is clean."""
        return {p: b for p, b in zip(self._params(), self.nonfinite_bits().tolist()) if b}

    def clear_nonfinite(self):
        """Zero the words (a device memset: no synchronisation).  The kernel only ever ORs."""
        self._need_guard()
        self._words.zero_()
        self._torch_stepped = False

    def _native_ok(self, group):
        if group["amsgrad"] or group.get("maximize", False) \
                or group.get("capturable", False) or group.get("differentiable", False):
            return False
        if not float(group["weight_decay"]) >= 0.0:      # (negative or NaN: torch's constructor refuses it too)
            return False
        for p in group["params"]:
            if p.grad is None:
                continue
            g = p.grad
            if not (p.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous()
                    and g.is_contiguous() and not g.is_sparse):
                return False
        return True

    # ---- HIP-graph support -------------------------------------------------------------------------------
    def _device_state(self, gi, device):
        d = self._dev.get(gi)
        if d is None:
            d = self._dev[gi] = (torch.zeros(1, dtype=torch.float64, device=device),
                                 torch.zeros(4, dtype=torch.float32, device=device))
        return d

    def _flush_replays(self):
        """Add the step counts of the replays made since the last flush to the host-side ``state[p]["step"]``."""
        if self._debt:
            for params in self._captured:
                for p in params:
                    self.state[p]["step"] += self._debt
            self._debt = 0

    def prepare_capture(self):
        """Before a capture that contains step() calls: every parameter of a group must be at the same step count (the
        captured kernels share one device counter per group), which the device counter is set to."""
        if not self.device_scalars:
            raise RuntimeError("HipAdam: construct with capturable=True to capture its step in a HIP graph")
        self._flush_replays()
        self._captured = []
        for gi, group in enumerate(self.param_groups):
            steps = {float(self.state[p]["step"]) for p in group["params"] if len(self.state[p])}
            unborn = [p for p in group["params"] if not len(self.state[p])]
            if len(steps) > 1 or (steps and unborn):
                raise RuntimeError("HipAdam.prepare_capture: parameters of one group are at different step counts")
            dev = group["params"][0].device
            self._device_state(gi, dev)[0].fill_(steps.pop() if steps else 0.0)
        self.sync_hyper()

    def replayed(self, times=1):
        """A captured iteration was replayed: the device counters advanced inside the graph, the host's follow (lazily).
        A replay is an optimizer step as far as torch's lr schedulers are concerned (they warn when ``scheduler.step()``
        comes before the first ``optimizer.step()``, which a replay never calls)."""
        self._debt += times
        self._opt_called = True

    def load_state_dict(self, state_dict):
        """(torch replaces the moment tensors: a graph captured before holds the old ones -- `state_generation` tells the
        trainers to capture anew.)"""
        self._debt, self._captured = 0, []
        self.state_generation += 1
        return super().load_state_dict(state_dict)

    @torch.no_grad()
    def load_state_in_place(self, state_dict):
        """`load_state_dict` that COPIES into the existing moment tensors (same parameters, same shapes) instead of
        replacing them: an iteration captured in a HIP graph stays valid (`state_generation` does not change).  Parameters
        absent from ``state_dict`` (a checkpoint taken before the first step) go back to step 0 with zero moments."""
        self._flush_replays()
        src = state_dict["state"]
        i = 0
        for gi, group in enumerate(self.param_groups):
            steps = set()
            for p in group["params"]:
                mine, theirs = self.state[p], src.get(i)
                i += 1
                if not len(mine):
                    if theirs:
                        raise RuntimeError("HipAdam.load_state_in_place: no state to copy into (use load_state_dict)")
                    continue
                if theirs:
                    mine["step"].fill_(float(theirs["step"]))
                    mine["exp_avg"].copy_(theirs["exp_avg"])
                    mine["exp_avg_sq"].copy_(theirs["exp_avg_sq"])
                else:
                    mine["step"].zero_()
                    mine["exp_avg"].zero_()
                    mine["exp_avg_sq"].zero_()
                steps.add(float(mine["step"]))
            if gi in self._dev and len(steps) == 1:
                self._dev[gi][0].fill_(steps.pop())          # the device counter a replayed step advances

    def _init_state(self, p, group):
        """torch.optim.Adam._init_group for one parameter without state."""
        st = self.state[p]
        if len(st) == 0:
            st["step"] = torch.tensor(0.0, dtype=torch.float32)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            if group.get("amsgrad", False):
                st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    def _ready_state(self, p, group):
        """``state[p]`` of a parameter about to be stepped: created if missing, ``step`` on the CPU (a checkpoint written
        by a fused / capturable Adam has it on the device).  Shared by the step and its fused first half; what they do
        with it differs on purpose -- see `begin_fused_step`."""
        st = self.state[p]
        if len(st) == 0:
            self._init_state(p, group)
        if st["step"].is_cuda:
            st["step"] = st["step"].cpu()
        return st

    def _prepare(self, gi, group, step, capturing, ema_dev=False, prepared=False):
        """The ONE place a capturable step's scalars are formed, for group ``gi`` at count ``step``: launches what
        `prepare_entry` names (nothing when the fused half has prepared this step) and returns the scalars.  An eager step
        also stores its count in the device counter: replays may follow it."""
        step_dev, scalars = self._device_state(gi, group["params"][0].device)
        name = prepare_entry(device_hyper=self.device_hyper, decay=float(group["weight_decay"]) != 0.0, ema_dev=ema_dev,
                             prepared=prepared)
        if name is None:
            return scalars
        if name.endswith("_dev"):
            hyper = self._hyper_words(gi)
            if not capturing:
                self.sync_hyper()      # (words that came into being just now)
            source = (hyper.data_ptr(), 1 if group.get("decoupled_weight_decay", False) else 0)
        else:
            source = (float(group["lr"]),)
        beta1, beta2 = group["betas"]
        check(getattr(_lib.load(), name)(float(step), step_dev.data_ptr(), 1 if capturing else 0, *source, float(beta1),
                                         float(beta2), scalars.data_ptr(), torch.cuda.current_stream().cuda_stream), name)
        return scalars

    # ---- the fused weight-gradient + Adam launch of the big Linear layers -------------------------------------------
    def _fused_candidates(self, group, only, ema_on, **trainer_side):
        """The weights of ``group`` that `linear_adam_eligible` admits to the fused launch."""
        return [p for p in group["params"] if p in self._bound_of and (only is None or id(p) in only)
                and linear_adam_eligible(
                    update_ema=ema_on, clip=self._clip_rec is not None, weight_decay=group["weight_decay"],
                    device_hyper=self.device_hyper, amsgrad=group["amsgrad"], maximize=group.get("maximize", False),
                    requires_grad=p.requires_grad, dim=p.dim(), numel=p.numel(), in_features=p.shape[-1],
                    native_tensor=p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() and p.data_ptr() % 16 == 0,
                    split_ok=bool(ops.linear_split_ok(32, p.numel())), **trainer_side)]

    @torch.no_grad()
    def begin_fused_step(self, update_ema=True, switch=True, grad_hook=False, exchange=False, only=None):
        """The first half of a two-part step: registers every big Linear weight that may be updated INSIDE the backward
        (`linear_adam_eligible`; ``vg_linear_wgrad_adam``: the weight gradient is consumed in registers and never
        written) and returns ``{id(weight): FusedLinearStep}`` for `functional.open_fused_linear_steps`.  Creates missing
        state and, for a capturable optimizer, runs the ONE ``vg_adam_prepare`` of the group's step; the host step count
        of a weight moves in `step`, and only if the backward reached it -- one that it did not reach is not stepped, as
        with ``grad is None``.  `step(update_ema=...)` with the same ``update_ema`` must follow.  ``only``: the weights
        the caller knows to get ONE weight-gradient pass in the coming backward (a layer used twice must not take the
        route: its first pass would change a weight its second still reads); None: every eligible one."""
        self._fused = None
        only = None if only is None else {id(p) for p in only}
        if not all(self._native_ok(g) for g in self.param_groups):
            return {}
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        if capturing and not self.device_scalars:
            return {}
        bounds = self._weight_bounds()
        if bounds is None:
            return {}
        if not capturing:
            self._flush_replays()
        regs, prepared = [], {}
        for gi, group in enumerate(self.param_groups):
            mine = self._fused_candidates(group, only, self._ema is not None and update_ema, switch=switch,
                                          grad_hook=grad_hook, exchange=exchange)
            if not mine:
                continue
            # Unlike `step`, this half does not advance the count -- the backward may never reach the weight -- and it
            # remembers the state it created (``born``) so that it can be forgotten again; state it cannot use (moments
            # that are not contiguous or not 16-byte aligned) leaves the weight to `step`, which raises where it must.
            born = {id(p) for p in mine if len(self.state[p]) == 0}
            steps = {float(self._ready_state(p, group)["step"]) + 1.0 for p in mine}
            if len(steps) > 1:                           # (one prepare per group: they must share its step)
                for p in mine:
                    if id(p) in born:
                        del self.state[p]
                continue
            step = steps.pop()
            beta1, beta2 = group["betas"]
            scalars = None
            if self.device_scalars:
                scalars = self._prepare(gi, group, step, capturing)
                prepared[gi] = step
            for p in mine:
                m, v = self.state[p]["exp_avg"], self.state[p]["exp_avg_sq"]
                if not (m.is_contiguous() and v.is_contiguous() and m.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0):
                    continue
                bi = self._bound_of[p]
                regs.append(FusedLinearStep(
                    p=p, m=m, v=v, amax=bounds[bi:bi + 1],
                    flag=self._words[self._word_of[p]:self._word_of[p] + 1] if self.nonfinite_guard else None,
                    scalars=scalars, lr=float(group["lr"]), beta1=float(beta1), beta2=float(beta2),
                    eps=float(group["eps"]), bc1=1.0 - beta1 ** step, bc2_sqrt=math.sqrt(1.0 - beta2 ** step), gi=gi,
                    step=step, born=id(p) in born))
        self._fused = (regs, prepared)
        return {id(r.p): r for r in regs}

    def _close_fused(self, capturing):
        """The second half: closes the registrations; counts the weights the backward updated (host step count, replay
        bookkeeping) and forgets the state created for one it never reached.  Returns (the updated weights, {group index:
        the step `begin_fused_step` has prepared the device scalars for}, whether state was created ahead of `step`)."""
        if self._fused is None:
            return set(), {}, False
        regs, prepared = self._fused
        self._fused = None
        done = set()
        by_group = {}
        for r in regs:
            r.open = False
            if r.done:
                if r.p.grad is not None:
                    raise RuntimeError("HipAdam: a weight updated inside the backward also received a gradient (a layer "
                                       "used twice in one backward must not take the fused step)")
                self.state[r.p]["step"] += 1
                done.add(r.p)
                by_group.setdefault(r.gi, []).append(r.p)
            elif r.born and r.p.grad is None:
                del self.state[r.p]
        if capturing:
            self._captured.extend(by_group.values())
        return done, prepared, any(r.born for r in regs)

    # ---- the step ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, update_ema=True):
        """``update_ema`` (with ``ema_decay`` set): False steps without touching the averages -- exactly the launches of
        an optimizer without EMA (a trainer that steps twice per iteration averages once).  A parameter the step skips
        (``grad is None``) keeps its EMA that step: the average follows the weights the optimizer writes, and a frozen
        weight's average would only drift towards the value it already tracks.

        ``max_grad_norm`` / ``skip_nonfinite``: ONE norm per call, over the gradients of every group this call steps
        (``clip_grad_norm_`` over all parameters; ``grad is None`` does not count).  A skipped step leaves ``p``,
        ``exp_avg``, ``exp_avg_sq`` and the EMA untouched but still ADVANCES the step count, the host's and the device
        counter alike: a count that depends on the data would need a host read inside a captured iteration.  The bias
        corrections of later steps therefore see one more step than updates were made."""
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        fused_done, fused_prepared, born = self._close_fused(capturing)
        ema_on = self._ema is not None and update_ema
        if closure is not None or not all(self._native_ok(g) for g in self.param_groups):
            loss = self._torch_step(closure, ema_on, capturing)
        else:
            loss = None
            lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
            if capturing and not self.device_scalars:
                raise RuntimeError("HipAdam: construct with capturable=True to capture its step in a HIP graph")
            if not capturing:
                self._flush_replays()
                self.sync_hyper()
            bounds = self._weight_bounds()
            if bounds is not None:                           # the words the backward has written already stay
                self._zero_bounds(bounds, fused_done)
            rec = self._norm_pass(lib, stream) if self._clip_rec is not None else None
            for gi, group in enumerate(self.param_groups):
                by_step = self._collect(group)
                if capturing and len(set(by_step) | ({fused_prepared[gi]} if gi in fused_prepared else set())) > 1:
                    raise RuntimeError("HipAdam: a captured step needs every parameter of a group at the same step count")
                for step, items in by_step.items():
                    self._launch(lib, stream, gi, group, step, items, ema_on=ema_on, rec=rec, bounds=bounds,
                                 capturing=capturing, prepared=fused_prepared.get(gi) == step)
            if bounds is not None:      # (a weight without a gradient was zeroed with the others: measured again; rare)
                self._publish_bounds(bounds, {p for p in self._bound_of if p in fused_done or p.grad is not None})
        if born:      # `begin_fused_step` created state ahead of the others: back to the order step() alone creates it in
            for p in [p for p in self._params() if p in self.state]:
                self.state[p] = self.state.pop(p)
        return loss

    def _torch_step(self, closure, ema_on, capturing):
        """torch's own step, for what the kernel does not implement -- with this class's features formed by torch around
        it: the clip / skip record (`_torch_clip`; the closure then runs first, the norm needs its gradients) and the
        average."""
        if capturing:
            raise RuntimeError("HipAdam: this configuration takes torch's step, which cannot be captured here")
        self._flush_replays()
        self._torch_stepped = True
        clip_on = self._clip_rec is not None
        loss = None
        if clip_on and closure is not None:
            with torch.enable_grad():
                loss = closure()
        stepped = [p for p in self._params() if p.grad is not None]
        if not clip_on:
            loss = super().step(closure)
        else:
            use = self._torch_clip(stepped)
            if use is None:                          # skipped: only the step counts move
                for group in self.param_groups:
                    for p in group["params"]:
                        if p.grad is not None:
                            self._init_state(p, group)
                            self.state[p]["step"] += 1
                return loss
            kept = [p.grad for p in stepped]
            for p, g in zip(stepped, use):
                p.grad = g
            try:
                super().step()
            finally:
                for p, g in zip(stepped, kept):
                    p.grad = g
        if ema_on and stepped:      # never silently stale: the same average, formed by torch after its step
            torch._foreach_lerp_([self._ema[self._ema_of[p]] for p in stepped], [p.detach() for p in stepped],
                                 1.0 - self.ema_decay)
        return loss

    def _norm_pass(self, lib, stream):
        """The grid-wide answer in front of the first store: the norm of every gradient this call steps on, the
        coefficient and the skip decision, into the clip record.  Returns the record's address."""
        grads = [p.grad for p in self._params() if p.grad is not None]
        n = len(grads)
        ptrs = (ctypes.c_void_p * max(1, n))(*[g.data_ptr() for g in grads])
        lens = (ctypes.c_size_t * max(1, n))(*[g.numel() for g in grads])
        slots = lib.vg_grad_sumsq_partials(lens, n)
        check(lib.vg_grad_sumsq_multi(ptrs, lens, n, self._partials.data_ptr(), self._partials.numel(), stream),
              "vg_grad_sumsq_multi")
        rec = self._clip_rec.data_ptr()
        check(lib.vg_grad_clip_finalize(self._partials.data_ptr(), slots,
                                        0.0 if self.max_grad_norm is None else self.max_grad_norm,
                                        1 if self.skip_nonfinite else 0, rec, stream), "vg_grad_clip_finalize")
        return rec

    def _collect(self, group):
        """``{step count: [(p, grad, exp_avg, exp_avg_sq)]}`` of the parameters of ``group`` that have a gradient, their
        counts advanced: one launch per count."""
        by_step = {}
        for p in group["params"]:
            if p.grad is None:
                continue
            st = self._ready_state(p, group)
            st["step"] += 1
            m, v = st["exp_avg"], st["exp_avg_sq"]
            if not (m.is_contiguous() and v.is_contiguous()):
                raise RuntimeError("HipAdam: optimizer state must be contiguous")
            by_step.setdefault(float(st["step"]), []).append((p, p.grad, m, v))
        return by_step

    def _launch(self, lib, stream, gi, group, step, items, *, ema_on, rec, bounds, capturing, prepared):
        """One multi-tensor launch: the entry point `step_entry` names, on the common prefix (host scalars: ``arr, n, lr,
        beta1, beta2, eps, bc1, bc2_sqrt``; device scalars, behind `_prepare`: ``arr, n, beta1, beta2, eps, scalars``), the
        tail that entry point takes, and the stream."""
        n = len(items)
        arr = (_AdamTensor * n)()
        for i, (p, g, m, v) in enumerate(items):
            bi = self._bound_of.get(p) if bounds is not None else None
            arr[i] = _AdamTensor(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(),
                                 None if bi is None else bounds[bi:bi + 1].data_ptr())
        words = self._words.data_ptr() if self.nonfinite_guard else None
        ema_dev = ema_on and self._ema_omd is not None
        have = {
            "flags": None if words is None else (ctypes.c_void_p * n)(*[words + 4 * self._word_of[it[0]] for it in items]),
            "ema": None if not ema_on else (ctypes.c_void_p * n)(*[self._ema[self._ema_of[it[0]]].data_ptr()
                                                                   for it in items]),
            "ema_decay": self.ema_decay or 0.0,      # (0.0 where the entry takes a decay and nothing is averaged)
            "omd": self._ema_omd.data_ptr() if ema_dev else None, "rec": rec, "wd": float(group["weight_decay"]),
            "decoupled": 1 if group.get("decoupled_weight_decay", False) else 0}
        name, tail = step_entry(dev=self.device_scalars, flags=words is not None, ema=ema_on, ema_dev=ema_dev,
                                decay=have["wd"] != 0.0, clip=rec is not None)
        beta1, beta2 = group["betas"]
        if self.device_scalars:
            scalars = self._prepare(gi, group, step, capturing, ema_dev=ema_dev, prepared=prepared)
            prefix = (arr, n, float(beta1), float(beta2), float(group["eps"]), scalars.data_ptr())
        else:
            prefix = (arr, n, float(group["lr"]), float(beta1), float(beta2), float(group["eps"]), 1.0 - beta1 ** step,
                      math.sqrt(1.0 - beta2 ** step))
        check(getattr(lib, name)(*prefix, *[have[k] for k in tail], stream), name)
        if capturing:
            self._captured.append([it[0] for it in items])

    def _publish_bounds(self, bounds, written=()):
        """Hand the bound words to the GEMMs that read the weights next (`ops.set_weight_bound`), measuring (``vg_absmax``
        into the zeroed word) every weight that is not among ``written``: those whose word a step has just emitted."""
        lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
        for p, bi in self._bound_of.items():
            slot = bounds[bi:bi + 1]
            if p not in written:
                check(lib.vg_absmax(p.data_ptr(), p.numel(), slot.data_ptr(), stream), "vg_absmax")
            ops.set_weight_bound(p, slot)

    @torch.no_grad()
    def refresh_weight_bounds(self):
        """Measure max |w| of the big Linear weights again, into the same device words (after weights were written by
        something other than `step` -- a checkpoint copied in place under a captured iteration, whose GEMMs read these
        words)."""
        bounds = self._weight_bounds()
        if bounds is not None:
            bounds.zero_()
            self._publish_bounds(bounds)


    def _zero_bounds(self, bounds, keep):
        """Zero the bound words of every weight but those in ``keep`` (one fill-by-mask launch; the mask is built once
        per set, from device fills alone, so that a capture may build it too)."""
        if not keep:
            return bounds.zero_()
        key = frozenset(self._bound_of[p] for p in keep)
        if len(key) == bounds.numel():
            return
        mask = self._bound_masks.get(key)
        if mask is None:
            mask = torch.ones(bounds.numel(), dtype=torch.bool, device=bounds.device)
            for i in key:
                mask[i:i + 1].fill_(False)
            self._bound_masks[key] = mask
        bounds.masked_fill_(mask, 0.0)

    def _weight_bounds(self):
        """The bounds tensor (one word per Linear weight the fp16x3 GEMM takes), or None when there is none."""
        if self._bounds is None:
            big = [p for p in self._params() if p.dim() == 2 and p.is_cuda and p.numel() >= ops.LINEAR_SPLIT_MIN_WEIGHTS]
            if not big:
                return None
            self._bound_of = {p: i for i, p in enumerate(big)}
            self._bounds = torch.zeros(len(big), dtype=torch.float32, device=big[0].device)
        return self._bounds
