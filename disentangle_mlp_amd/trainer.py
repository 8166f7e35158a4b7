"""Training-step drivers: the counterparts of the reference's ``train(epoch)`` loop
bodies, one process per GPU.

  BetaVAEGANTrainer.step  <->  experiments/new_betavaegan.py:87-193
  VAETrainer.step         <->  experiments/new_vae.py:53-59
  GANTrainer.step         <->  experiments/new_gan.py:66-141

Observable results follow the reference (three optimizer steps per iteration, all of
EG moves in both EG phases, BatchNorm running statistics updated by every forward
in the reference's order, train-mode BN everywhere).  Provably dead work is
skipped:
  * the separate ``backward()`` calls of a phase are one backward of the summed loss;
  * in the decoder phase the discriminator only relays gradients: its parameters are
    frozen (no weight gradients) and ``sim_real`` is computed without a graph.
No host synchronisation happens inside ``step``; loss scalars stay on the device.

Non-finite guard: the Adam steps flag an inf / NaN among the gradients they read and the parameters
they wrote (optim.HipAdam(nonfinite_guard=True)); ``check_finite()`` reads the flags -- one device ->
host copy, on demand and at the end of every ``train_epoch`` -- and raises `NonFiniteError`, so a
poisoned epoch is never checkpointed.

Data parallelism: every rank holds a replica and a shard of the batch; BatchNorm
statistics are replica-local (as under the reference's nn.DataParallel); before each
optimizer step the gradients, laid out in one flat fp32 buffer per network, are
summed with a single RCCL all-reduce (SUM, not mean: sum-reduced losses use local
sums, BCE is divided by the *global* batch), which reproduces the global-batch
gradient.
"""
import copy
import math
import os
import warnings
import weakref
from contextlib import nullcontext
from dataclasses import dataclass, field
from typing import Callable, Dict, List, NamedTuple, Optional

import numpy as np
import torch
import torch.distributed as dist
from torch import optim

from . import functional as F
from . import model as _model
from . import ops
from .optim import HipAdam, NONFINITE_GRAD, NONFINITE_PARAM, isfinite_bits
from .model import VAE, Discriminator_celeba, Generator_celeba, LatentCritic, weights_init, shadowed_bias_params


@dataclass
class ModelOpt:
    """The fields of the reference's argparse namespace the models read
    (utils/envsetter.py:41-42,45)."""
    input_channels: int = 3
    n_hidden: int = 128
    n_z: List[int] = field(default_factory=lambda: [256, 8, 8])


class FlatGrads:
    """Gradient exchange of one network for data parallelism: RCCL all-reduces (SUM) launched from
    autograd hooks so that they overlap the rest of the backward pass.

    * LARGE parameters (>= `direct_bytes`; the 134 MB Linear weights and the big conv filters,
      > 95 % of the payload) are reduced IN PLACE on the gradient tensor autograd produced, as
      soon as it is final -- no flattening copy, no zero-fill, no extra accumulate pass.  The
      Linear-weight gradients are the first ones ready in backward, so their exchange hides
      behind the convolution backward.
    * SMALL parameters live as views in one flat fp32 buffer, cut into buckets of ~`bucket_bytes`
      from the END of the parameter list (ready first); a bucket is reduced when its last
      gradient has been accumulated.
    `finish()` reduces whatever did not fire and makes the compute stream wait for every
    exchange.  xGMI is point-to-point (7 links x ~153 GB/s per GPU): few, large messages keep
    all the rings / trees RCCL builds busy."""

    exchange_when_alone = False      # tests: run the collectives even in a process group of one
    own_rccl = os.environ.get("VG_OWN_RCCL", "1") != "0"     # 0: c10d's collectives on the GPU too (not capturable)

    def __init__(self, params, bucket_bytes=8 << 20, direct_bytes=1 << 20, overlap=True, silent=()):
        """``silent``: parameters that never receive a gradient from autograd (the biases whose gradient is defined as
        zero, model.shadowed_bias_params): their zeroed views travel with their bucket, which does not wait for them."""
        self.params = [p for p in params]
        self._silent = {id(p) for p in silent}
        self.direct = [p.numel() * 4 >= direct_bytes for p in self.params]
        small = [i for i, d in enumerate(self.direct) if not d]
        n = sum(self.params[i].numel() for i in small)
        dev = self.params[0].device
        self.flat = torch.zeros(max(n, 1), dtype=torch.float32, device=dev)
        self.views, self.offsets = {}, {}
        off = 0
        for i in small:
            p = self.params[i]
            self.views[i] = self.flat[off:off + p.numel()].view_as(p)
            self.offsets[i] = off
            off += p.numel()
        self.buckets = []          # dicts: start, end (element offsets into flat), members (param indices)
        cap = max(1, bucket_bytes // 4)
        cur = None
        for i in reversed(small):
            if cur is None or ((cur["end"] - self.offsets[i]) > cap and cur["members"]):
                cur = dict(start=self.offsets[i], end=self.offsets[i] + self.params[i].numel(), members=[])
                self.buckets.append(cur)
            cur["start"] = self.offsets[i]
            cur["members"].append(i)
        self.bucket_of = {i: b_i for b_i, b in enumerate(self.buckets) for i in b["members"]}
        self.overlap = overlap
        self._pending, self._launched, self._direct_done, self._handles = [], [], set(), []
        self._armed = False
        self._hooks = [p.register_post_accumulate_grad_hook(self._make_hook(i)) for i, p in enumerate(self.params)]
        # Transport.  On the GPU with the "nccl" (= RCCL) backend: our own RCCL communicator (rccl.py), all-reduces
        # enqueued on a side stream forked from / joined to the compute stream by events -- plain kernel launches, so an
        # iteration containing them can be captured in a HIP graph (c10d's collectives cannot: rccl.py).  Otherwise
        # (gloo: CPU tests, two ranks sharing one GPU) torch.distributed's async all-reduce.  Creating the communicator
        # is collective: every rank constructs its trainers in the same order.
        self._comm = self._side = None
        if (self.own_rccl and dev.type == "cuda" and dist.is_available() and dist.is_initialized()
                and dist.get_backend() == "nccl"):
            from . import rccl
            self._comm = rccl.communicator()          # None: not available on every rank (warned once) -> c10d, eager
            self._side = torch.cuda.Stream(device=dev) if self._comm is not None else None
        self._forked = False
        self._capturing = False
        # bookkeeping for bench.py: bytes handed to all-reduce since the last reset, and -- when `time_finish` is set --
        # HIP-event pairs around the waits of finish() (how long the compute stream stood still for the exchange)
        self.bytes_reduced, self.collectives = 0, 0
        self.time_finish, self.finish_events = False, []

    def _make_hook(self, i):
        def hook(p):
            if not self._armed:
                return
            if self.direct[i]:
                if self.overlap:
                    self._reduce_direct(i)
                return
            if id(p) in self._silent:      # (autograd may or may not run AccumulateGrad for a gradient it was not given)
                return
            b = self.bucket_of[i]
            self._pending[b] -= 1
            if self._pending[b] == 0 and self.overlap:
                self._launch(b)
        return hook

    def _reduce_direct(self, i):
        g = self.params[i].grad
        if g is None or i in self._direct_done:
            return
        self._direct_done.add(i)
        self.bytes_reduced += g.numel() * 4
        self.collectives += 1
        self._all_reduce(g)

    def _launch(self, b):
        bk = self.buckets[b]
        self._launched[b] = True
        self.bytes_reduced += (bk["end"] - bk["start"]) * 4
        self.collectives += 1
        self._all_reduce(self.flat[bk["start"]:bk["end"]])

    @property
    def capturable(self):
        """Whether an iteration that exchanges through this object may be captured in a HIP graph."""
        return self._comm is not None

    def _all_reduce(self, t):
        if self._comm is None:
            self._handles.append(dist.all_reduce(t, op=dist.ReduceOp.SUM, async_op=True))
            return
        # own RCCL: fork the side stream from the stream this gradient is final on (the hook runs on the autograd
        # thread, whose current stream the engine has set to the producing node's), enqueue, join in finish()
        cur = torch.cuda.current_stream()
        if torch.cuda.is_current_stream_capturing() != self._capturing:
            raise RuntimeError("FlatGrads: a gradient hook ran on a stream outside the capture that armed the exchange")
        self._side.wait_stream(cur)
        self._comm.all_reduce_sum_(t, self._side)
        self._forked = True

    def zero_and_attach(self):
        """Start of a phase: small gradients -> zeroed views of the flat buffer (autograd
        accumulates into them in place); large gradients -> None (autograd installs its result)."""
        self.flat.zero_()
        for i, p in enumerate(self.params):
            p.grad = None if self.direct[i] else self.views[i]
        self._pending = [sum(1 for i in b["members"] if id(self.params[i]) not in self._silent) for b in self.buckets]
        self._launched = [False] * len(self.buckets)
        self._direct_done = set()
        self._handles = []
        self._forked = False
        self._capturing = self.flat.is_cuda and torch.cuda.is_current_stream_capturing()
        # a 1-rank group still exchanges (sum over one rank): lets a single GPU exercise the RCCL path end to end
        self._armed = dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or FlatGrads.exchange_when_alone)

    def finish(self):
        """Reduce what did not fire from the hooks (or everything, without overlap), then make
        the current stream wait for every exchange."""
        if not self._armed:
            return
        for i, d in enumerate(self.direct):
            if d:
                self._reduce_direct(i)
        for b in range(len(self.buckets)):
            if not self._launched[b]:
                self._launch(b)
        timed = self.time_finish and self.flat.is_cuda and not self._capturing     # (events inside a capture cannot be timed)
        if timed:
            a = torch.cuda.Event(enable_timing=True)
            a.record()
        for h in self._handles:
            h.wait()
        if self._forked:                         # own RCCL: the compute stream joins the side stream
            torch.cuda.current_stream().wait_stream(self._side)
            self._forked = False
        if timed:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            self.finish_events.append((a, b))
        self._handles = []
        self._armed = False

    def reset_stats(self):
        self.bytes_reduced, self.collectives, self.finish_events = 0, 0, []

    def exposed_ms(self):
        """Sum over the recorded finish() calls of the time between the compute stream reaching the waits and passing
        them (synchronises)."""
        if self.finish_events:
            torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.finish_events)

    def gathered(self):
        """All gradients flattened in parameter order (tests / diagnostics; copies)."""
        return torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).reshape(-1)
                          for p in self.params])


def _zero_grads(net):
    """``net.zero_grad(set_to_none=True)``, except for the convolution biases whose gradient is defined as exactly zero
    (model.shadowed_bias_params): they keep ONE persistent all-zero ``.grad`` -- their backward returns nothing, so it
    is never written -- instead of a zero fill and an accumulate launch per pass (35 launches per iteration)."""
    keep = getattr(net, "_vg_zero_bias_grads", None)
    if keep is None:
        keep = net._vg_zero_bias_grads = {id(p) for p in shadowed_bias_params(net)}
    for p in net.parameters():
        if id(p) in keep:
            if p.grad is None or p.grad.shape != p.shape or p.grad.device != p.device:
                p.grad = torch.zeros_like(p)
        else:
            p.grad = None


_ONES = {}


def _backward(losses):
    """One backward of the summed scalar losses, seeded with a cached 1.0 per device (autograd otherwise fills a fresh
    ones_like for every loss: 8 tiny launches per iteration)."""
    dev = losses[0].device
    one = _ONES.get(dev)
    if one is None:
        one = _ONES[dev] = torch.ones((), dtype=torch.float32, device=dev)
    torch.autograd.backward(losses, grad_tensors=[one] * len(losses))


def _make_adam(params, lr, fused, capturable=False, nonfinite_guard=False, max_grad_norm=None, skip_nonfinite=False,
               weight_decay=0.0, decoupled_weight_decay=False, device_hyper=False, ema=None, betas=None):
    """Adam with the reference's defaults (new_betavaegan.py:49-50).  On the GPU the step runs on the
    hand-written kernel (optim.HipAdam, a torch.optim.Adam subclass: identical state_dict); ``capturable``:
    its scalars are formed on the device so that a whole iteration can be captured in a HIP graph;
    ``nonfinite_guard``: the step flags non-finite gradients / parameters.  CPU construction uses torch's own
    implementation -- unless ``max_grad_norm`` / ``skip_nonfinite`` (clipping by global norm, skipping a non-finite
    step: optim.HipAdam) is asked for: then it is a HipAdam there too, whose inherited step carries those semantics.
    ``weight_decay`` / ``decoupled_weight_decay``: torch.optim.Adam's, inside the fused step on the GPU; ``device_hyper``:
    lr and weight decay in device words a captured step reads (optim.HipAdam).  ``ema``: ``(decay, targets)`` of the one
    optimizer whose step keeps the weight EMA (`_GraphedSteps._ema_setup`) -- a HipAdam with device scalars and the decay
    in a device word, whether or not the iteration is captured.  ``betas``: Adam's pair, None for torch's default."""
    decay = dict(weight_decay=weight_decay, decoupled_weight_decay=decoupled_weight_decay)
    if betas is not None:
        decay["betas"] = betas
    if ema is not None:
        return HipAdam(params, lr=lr, capturable=True, nonfinite_guard=nonfinite_guard, max_grad_norm=max_grad_norm,
                       skip_nonfinite=skip_nonfinite, device_hyper=device_hyper, ema_decay=ema[0], ema_targets=ema[1],
                       ema_decay_on_device=True, **decay)
    if fused:
        return HipAdam(params, lr=lr, capturable=capturable, nonfinite_guard=nonfinite_guard,
                       max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, device_hyper=device_hyper, **decay)
    if max_grad_norm is not None or skip_nonfinite:
        return HipAdam(params, lr=lr, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite, **decay)
    return optim.Adam(params, lr=lr, capturable=capturable, **decay)


def _dist_world():
    return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def _dist_rank():
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


def _latent_generator(device, seed, rank):
    """Generator of the latent draws this replica makes itself (``noise`` of new_betavaegan.py:111,
    ``eps`` of model.py:534).  Weights come from ``torch.manual_seed(seed)`` on every rank (replicas
    start identical, and the CPU generator stays shared: the loader's permutation must agree on all
    ranks); the latents must NOT: the reference draws one independent sample per image of the global
    batch, so each rank seeds its own stream with seed + 1 + rank."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed) + 1 + int(rank))
    return g


def _augment_generator(device, seed, rank):
    """Generator of the uniforms of ``diff_augment``: a stream of its own per replica, seeded from (seed, rank) as the latent
    one is -- apart from it, so that the latents are bit for bit what they are without the option."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed) + (1 << 32) + int(rank))      # (far from every rank's latent seed, seed + 1 + rank)
    return g


def _permute_generator(device, seed, rank):
    """Generator of the uniforms of ``factor_vae``'s ``permute_dims``: a third stream per replica, seeded from (seed, rank)
    apart from the latent and the augmentation ones -- both are bit for bit what they are without the option."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed) + (2 << 32) + int(rank))
    return g


def _owned_generator(seed):
    """CPU generator of the initial weights of a network an objective owns (``factor_vae``'s critic): seeded from ``seed``
    alone, so every rank draws the same weights, and not the global CPU stream, so the trainer's other networks -- built
    right behind ``torch.manual_seed(seed)`` -- are what they are without the option."""
    g = torch.Generator()
    g.manual_seed(int(seed) + (3 << 32))
    return g


def _parse_diff_augment(diff_augment):
    """``diff_augment=policy`` or ``(policy, p)`` -> (the policy's names in canonical order, its bit set, p)."""
    try:
        policy, p = (diff_augment, 1.0) if isinstance(diff_augment, str) else diff_augment
    except (TypeError, ValueError):
        raise TypeError(f"diff_augment must be a policy string or a pair (policy, p), got {diff_augment!r}") from None
    if not isinstance(policy, str):
        raise TypeError(f"diff_augment: the policy is a string of names, got {policy!r}")
    bits, p = ops.augment_policy(policy), ops.augment_probability(p)
    return ",".join(n for n, b in ops.AUGMENT_BITS.items() if bits & b), bits, p


ADA_DEFAULTS = dict(target=0.6, kimg=500.0, interval=4)      # Karras et al. 2020: r_t held at 0.6, p from 0 to 1 in 500 kimg


def _parse_ada(ada):
    """``ada=True`` or ``dict(target=, kimg=, interval=)`` -> (target, rate, interval) of `ops.ada_update`, with ``rate =
    1 / (kimg * 1000)``: p moves by (images seen) * rate per adjustment; None for None / False."""
    if ada is None or ada is False:
        return None
    if ada is True:
        ada = {}
    if not isinstance(ada, dict):
        raise TypeError(f"ada must be None, True or a dict(target=, kimg=, interval=), got {ada!r}")
    unknown = sorted(set(ada) - set(ADA_DEFAULTS))
    if unknown:
        raise TypeError(f"ada: unknown key {unknown[0]!r} (known: {', '.join(ADA_DEFAULTS)})")
    args = dict(ADA_DEFAULTS, **ada)
    try:
        target, kimg = float(args["target"]), float(args["kimg"])
        interval = args["interval"]
        if isinstance(interval, bool) or int(interval) != interval:
            raise TypeError
        interval = int(interval)
    except (TypeError, ValueError):
        raise TypeError(f"ada: target and kimg are numbers, interval is an integer, got {args!r}") from None
    if not (math.isfinite(target) and -1.0 < target < 1.0):
        raise ValueError(f"ada: target must lie inside (-1, 1), the range of r_t, got {target!r}")
    if not (math.isfinite(kimg) and kimg > 0.0 and math.isfinite(1.0 / (kimg * 1000.0))):
        raise ValueError(f"ada: kimg must be finite and > 0, got {kimg!r}")
    if interval < 1:
        raise ValueError(f"ada: interval must be >= 1, got {interval!r}")
    return target, 1.0 / (kimg * 1000.0), interval


def sample_labels(rng=None):
    """The per-iteration label draw of new_betavaegan.py:89-90 (new_gan.py:68-69 alike): soft labels
    0.9 / 0.1, each flipped with probability 5 %.  Draw order as in the reference -- the fake label
    first, then the real one -- from ``rng.choice`` (default: NumPy's global ``np.random``, the stream
    the reference consumes; pass a ``np.random.RandomState`` for a reproducible run).
    Returns (real_label, fake_label) as Python floats."""
    rng = np.random if rng is None else rng
    fake_label = rng.choice(a=[0.1, 0.9], p=[0.95, 0.05])
    real_label = rng.choice(a=[0.1, 0.9], p=[0.05, 0.95])
    return float(real_label), float(fake_label)


def _shared_label_rng(seed):
    """Label stream of a data-parallel run.  The reference is ONE process: its draw of new_betavaegan.py:89-90 applies
    to the whole global batch.  With one process per GPU every rank must make the same draw, so each trainer owns a
    ``np.random.RandomState`` seeded alike on all ranks (NumPy's global stream, which the reference consumes and a
    single-process run here still uses by default, is seeded nowhere and shared by nobody)."""
    return np.random.RandomState((int(seed) + 0x5EED) % (2 ** 32))


def _loader_global_batch(loader, local_batch, world):
    """Images of the current GLOBAL batch: what nn.BCELoss's mean runs over under the reference's
    DataParallel.  data.DeviceLoader publishes it (a short last batch is split unevenly over the
    ranks); for a foreign loader every rank is assumed to hold an equal share."""
    gb = getattr(loader, "last_global_batch", None)
    return int(gb) if gb else int(local_batch) * world


def ema_warmup(decay, start_iteration=0):
    """A per-iteration EMA decay for the trainers' ``ema_decay=``: 0 -- the average follows the weights -- before
    ``start_iteration``, then ``min(decay, (1 + n) / (10 + n))`` with ``n = iteration - start_iteration``: the early
    iterations weigh little, so the random initialisation does not sit in the average for thousands of steps."""
    decay, start = float(decay), int(start_iteration)
    if not 0.0 < decay < 1.0:      # (NaN fails both comparisons)
        raise ValueError(f"ema_warmup: decay must lie in (0, 1), got {decay!r}")
    if start < 0 or start != start_iteration:
        raise ValueError(f"ema_warmup: start_iteration must be an integer >= 0, got {start_iteration!r}")

    def schedule(iteration):
        n = int(iteration) - start
        return 0.0 if n < 0 else min(decay, (1.0 + n) / (10.0 + n))
    return schedule


def linear_capacity(c_max, iterations, c_start=0.0):
    """A per-iteration KL capacity for the trainers' ``kl_control=``: from ``c_start`` at iteration 0 linearly up to ``c_max``
    at ``iterations``, and ``c_max`` from there on (Burgess et al. 2018: C from 0 to 25 nats over 100000 iterations)."""
    c_max, c_start, n = float(c_max), float(c_start), int(iterations)
    if not (np.isfinite(c_max) and np.isfinite(c_start) and c_max >= 0.0 and c_start >= 0.0):      # (NaN fails the comparisons)
        raise ValueError(f"linear_capacity: c_max and c_start must be finite and >= 0, got {c_max!r} and {c_start!r}")
    if n < 1 or n != iterations:
        raise ValueError(f"linear_capacity: iterations must be an integer >= 1, got {iterations!r}")

    def schedule(iteration):
        return c_start + (c_max - c_start) * min(max(int(iteration), 0) / n, 1.0)
    return schedule


GRAPH_DEFAULT = os.environ.get("VG_GRAPH", "1") != "0"     # 0: trainers never capture (every step eager)
GRAPH_WARM_STEPS = 2      # eager iterations of a shape before it is captured (workspaces, packs, GEMM plans exist then)


NONFINITE_GUARD_DEFAULT = os.environ.get("VG_NONFINITE_GUARD", "1") != "0"    # 0: trainers do not guard unless asked


class NonFiniteError(RuntimeError):
    """`check_finite` found an inf / NaN among the gradients the optimizer steps read or the parameters they wrote.

    ``found``: list of ``(qualified parameter name such as "netD.convs.0.weight", "grad" | "param" | "grad+param")`` of
    this rank (empty when only another rank of a data-parallel run is poisoned); ``first_iteration`` /
    ``last_iteration``: the trainer's ``iteration`` when its flags were last known clean, and now -- the poison arrived
    in an iteration of that range.  The weights are poisoned (without ``skip_nonfinite=True`` the step detects, it does
    not skip; with it, a forward pass or a parameter went non-finite by another way): reload the last checkpoint."""

    def __init__(self, found, first_iteration, last_iteration):
        self.found, self.first_iteration, self.last_iteration = list(found), first_iteration, last_iteration
        names = ", ".join(f"{n} ({k})" for n, k in self.found[:4]) + (f", ... {len(self.found)} in all" if len(self.found) > 4 else "")
        super().__init__(
            f"non-finite values between iterations {first_iteration} and {last_iteration}: "
            + (names if self.found else "on another rank of this data-parallel run")
            + ".  Likeliest causes: a non-finite input batch, or a stale fp16x3 magnitude bound.  The weights are "
              "poisoned; reload the last good checkpoint (load / load_in_place).")


class _CapturedIteration:
    """One training iteration captured in a HIP graph (torch.cuda.CUDAGraph) and replayed: ~390 kernel launches become
    one graph launch, so the host no longer paces the GPU.

    What the graph freezes and how it stays correct from replay to replay:
      * inputs / latents / the uniforms of ``diff_augment``: static device buffers the caller's tensors are copied into
        before a replay (what the trainer draws itself, it draws straight into them);
      * the two label scalars (new_betavaegan.py:89-90): a device tensor the BCE kernels read (vg_bce_loss_dev);
      * Adam's step count: a device counter advanced inside the graph (optim.HipAdam(capturable=True));
      * with ``device_hyper``: the learning rate, the weight decay and the KL weight beta -- device words the prepare kernel
        and the KL kernels read, refreshed from the host's values in front of every replay (`sync_hyper`);
      * Python-side bookkeeping a replay does not execute -- BatchNorm ``num_batches_tracked`` (counted lazily by the
        modules), Adam's host step counts, the trainer's iteration counter -- is re-applied after each replay from what
        the capture pass recorded.
    The capture pass only records (nothing executes); the replay that follows it IS that iteration, so capturing has
    no side effect on the training state.  Outputs are static tensors, overwritten by the next replay."""

    def __init__(self, trainer, run, inputs, optimizers, bn_modules):
        self.inputs = {k: torch.empty_like(v) for k, v in inputs.items()}
        self.labels = torch.zeros(2, dtype=torch.float32, device=trainer.device)     # [real, fake]
        self.label_values = None
        self.optimizers, self.bn = optimizers, bn_modules
        self._trainer = weakref.ref(trainer)
        self.graph = torch.cuda.CUDAGraph()
        for k, v in inputs.items():
            self.inputs[k].copy_(v)
        before_nbt = [m._nbt_pending for m in bn_modules]
        # a data-parallel iteration: the exchange's counters (bench.py's data_parallel block) advance per replay as well
        self.flats = trainer._flats()
        before_flat = [(f.bytes_reduced, f.collectives) for f in self.flats]
        host_steps = [{p: float(o.state[p]["step"]) for g in o.param_groups for p in g["params"] if len(o.state[p])}
                      for o in optimizers]
        for o in optimizers:
            o.prepare_capture()
        # Buffers that exist now AND those that exist afterwards: a workspace regrown in the middle of the capture is
        # already referenced by the nodes captured before that.  When it came from the pool of an earlier, since destroyed
        # graph (all captures share one stream, hence one workspace), dropping it here hands its memory back for good --
        # the next capture's empty_cache() unmaps it under this graph's replays.
        before = ops.buffers_in_use()
        try:
            with ops.amax_capture_scope(), torch.cuda.graph(self.graph):
                self.out = run(self.inputs, self.labels[0:1], self.labels[1:2])
        except Exception:
            # nothing executed: take back what the pass did on the host side
            for m, n in zip(bn_modules, before_nbt):
                m._nbt_pending = n
            for o, hs in zip(optimizers, host_steps):
                for p, v in hs.items():
                    o.state[p]["step"].fill_(v)
                o._captured = []
            raise
        # the graph holds raw pointers into the weights' pack buffers and ops' scratch buffers: they live as long as it does
        self._buffers = before + ops.buffers_in_use()
        self.nbt_delta = [m._nbt_pending - n for m, n in zip(bn_modules, before_nbt)]
        self.flat_delta = [(f.bytes_reduced - b0, f.collectives - c0) for f, (b0, c0) in zip(self.flats, before_flat)]
        self.fresh = True          # the capture pass already did the host-side bookkeeping of the first replay

    def replay(self, inputs, real_label, fake_label):
        for k, v in inputs.items():
            if v is not self.inputs[k]:
                self.inputs[k].copy_(v)
        if (real_label, fake_label) != self.label_values:
            self.labels[0].fill_(real_label)
            self.labels[1].fill_(fake_label)
            self.label_values = (real_label, fake_label)
        for o in self.optimizers:                # lr / weight decay words (nothing to do without them)
            o.sync_hyper()
        trainer = self._trainer()
        if trainer is not None:
            trainer._sync_beta()
        self.graph.replay()
        if self.fresh:
            self.fresh = False
        else:
            for m, d in zip(self.bn, self.nbt_delta):
                m._nbt_pending += d
            for o in self.optimizers:
                o.replayed()
            for f, (db, dc) in zip(self.flats, self.flat_delta):
                f.bytes_reduced += db
                f.collectives += dc
        return self.out


def _use_tuned_gemms(device):
    """The Linear layers' vendor GEMMs with the measured algorithm table (tuned_gemms.py), on the GPU."""
    if torch.device(device).type == "cuda":
        from . import tuned_gemms
        tuned_gemms.enable()


class _Drawn(NamedTuple):
    """One random input of an iteration (`_GraphedSteps._drawn`): what the trainer draws when the caller passes None."""
    name: str             # its key among a capture's static inputs
    dist: str             # "normal": N(0, 1) | "uniform": U[0, 1)
    generator: str        # attribute of the trainer's generator it is drawn from


class _Part(NamedTuple):
    """One network of a trainer and what belongs to it: attribute NAMES, looked up on the trainer when used (an
    optimizer assigned after construction is the one that steps)."""
    net: str          # attribute of the network
    cls: type         # its module class
    opt: str          # attribute of its optimizer
    flat: str         # attribute of its FlatGrads (None there without data parallelism)
    plan: str         # its name in the pack plans (`_run_with_pack_plan`)
    ckpt: str         # checkpoint key of its optimizer


class _Objective(NamedTuple):
    """One objective that replaces or extends the KL term of the encoder phase, and all that differs between them.
    DESIGN.md section 4.24 lists what a new one touches; here it is one entry of `_OBJECTIVES`."""
    keyword: str              # the constructor keyword it answers to; the trainer's attribute of that name reads its arguments
    parse: Callable           # (the keyword's value, ModelOpt) -> the frozen, hashable argument tuple
    forward: Callable         # (net, data, eps, beta, args, prior) -> recon, mu, logvar, loss, parts
    parts: tuple              # the loss keys of parts[0..2]
    latents: tuple = ()       # latents the iteration draws on top of the trainer's own, last in draw order
    needs_dataset_size: bool = False      # `dataset_size` joins the arguments: required before a step, filled from a loader
    word: Optional[str] = None            # its OWN scheduled value: the name it goes by.  `parse` returns it FIRST (a float, or a
    #                                       callable iteration -> float); it is no frozen argument -- `forward` gets it first among
    #                                       ``args`` as a float, or under ``device_hyper`` as a device word beside beta's
    owns: Optional["_Owned"] = None       # a network of its own with an optimizer, inputs and a phase:
    #                                       `forward` gets the network LAST among ``args`` and may return more than five values --
    #                                       what is behind ``parts`` is carried to the phase


class _Owned(NamedTuple):
    """The network an objective owns, and all a trainer needs to carry it: one more `_Part` (present only with the keyword),
    its construction, its optimizer's own arguments, the inputs its phase draws and the phase itself."""
    part: _Part               # network, optimizer, exchange, pack-plan name, checkpoint key of the optimizer
    ckpt: str                 # checkpoint key of the network's state_dict
    build: Callable           # (ModelOpt, the frozen arguments, a CPU generator) -> the network, on the CPU
    adam: Callable            # the frozen arguments -> dict(lr=, betas=) of its optimizer
    drawn: tuple              # the `_Drawn` inputs of its phase, last in draw order (behind ``augment``)
    phase: Callable           # (trainer, what `forward` carried, the drawn tensors, global batch, grad_hook) -> loss outputs


def _parse_tc(tc_decomposition, opt):
    """``tc_decomposition=(alpha, gamma)``: the weights of the mutual-information and the dimension-wise-KL parts."""
    try:
        alpha, gamma = (float(v) for v in tc_decomposition)
    except (TypeError, ValueError):
        raise TypeError(f"tc_decomposition must be a pair (alpha, gamma) of floats, got {tc_decomposition!r}") from None
    if not (np.isfinite(alpha) and np.isfinite(gamma)):
        raise ValueError(f"tc_decomposition: alpha and gamma must be finite, got {tc_decomposition!r}")
    return alpha, gamma


def _parse_dip(dip_vae, opt):
    """``dip_vae=(variant, lambda_od, lambda_d)``: "i" | "ii", the weights of the off-diagonal / diagonal penalty."""
    try:
        variant, lambda_od, lambda_d = dip_vae
        lambda_od, lambda_d = float(lambda_od), float(lambda_d)
    except (TypeError, ValueError):
        raise TypeError(f"dip_vae must be a triple (variant, lambda_od, lambda_d), got {dip_vae!r}") from None
    if variant not in ("i", "ii"):
        raise ValueError(f"dip_vae: variant must be 'i' or 'ii', got {variant!r}")
    if not (np.isfinite(lambda_od) and np.isfinite(lambda_d) and lambda_od >= 0.0 and lambda_d >= 0.0):
        raise ValueError(f"dip_vae: lambda_od and lambda_d must be finite and >= 0, got {dip_vae!r}")
    return variant, lambda_od, lambda_d


def _parse_mmd(mmd_vae, opt):
    """``mmd_vae=(kernel, lambda_mmd[, bandwidths])``: "rbf" | "imq", the MMD's weight, a tuple of floats or None."""
    try:
        kernel, lambda_mmd, *rest = mmd_vae
        lambda_mmd = float(lambda_mmd)
        bandwidths, = rest or (None,)
    except (TypeError, ValueError):
        raise TypeError(f"mmd_vae must be (kernel, lambda_mmd) or (kernel, lambda_mmd, bandwidths), got {mmd_vae!r}") from None
    if kernel not in ("rbf", "imq"):
        raise ValueError(f"mmd_vae: kernel must be 'rbf' or 'imq', got {kernel!r}")
    if not (np.isfinite(lambda_mmd) and lambda_mmd >= 0.0):
        raise ValueError(f"mmd_vae: lambda_mmd must be finite and >= 0, got {mmd_vae!r}")
    if bandwidths is not None:
        try:
            bandwidths = ops.mmd_bandwidths(kernel, opt.n_hidden, bandwidths)
        except ValueError as e:
            raise ValueError(f"mmd_vae: {e}") from None
    return kernel, lambda_mmd, bandwidths


def _nonneg(name, value):
    """``value`` as a finite float >= 0 (TypeError: no number; ValueError: negative, inf or NaN)."""
    try:
        v = float(value)
    except (TypeError, ValueError):
        raise TypeError(f"{name} must be a number, got {value!r}") from None
    if not (np.isfinite(v) and v >= 0.0):
        raise ValueError(f"{name} must be finite and >= 0, got {value!r}")
    return v


def _parse_klc(kl_control, opt):
    """``kl_control=(capacity, free_bits)``: nats per sample -- a float or a callable iteration -> float --, and the floor in
    nats per dimension per sample."""
    try:
        capacity, free_bits = kl_control
    except (TypeError, ValueError):
        raise TypeError(f"kl_control must be a pair (capacity, free_bits), got {kl_control!r}") from None
    if not callable(capacity):
        capacity = _nonneg("kl_control: capacity", capacity)
    return capacity, _nonneg("kl_control: free_bits", free_bits)


FACTOR_CRITIC_DEFAULTS = dict(width=1000, depth=6, lr=1e-4, betas=(0.5, 0.9))      # Kim & Mnih 2018, their discriminator


def _parse_factor(factor_vae, opt):
    """``factor_vae=gamma`` or ``(gamma, dict(width=, depth=, lr=, betas=))``: the weight of the total-correlation estimate -- a
    float or a callable iteration -> float --, and the critic and its Adam (`FACTOR_CRITIC_DEFAULTS`)."""
    gamma, given = factor_vae, {}
    if isinstance(factor_vae, (tuple, list)):
        try:
            gamma, given = factor_vae
        except ValueError:
            raise TypeError(f"factor_vae must be gamma or a pair (gamma, dict of critic options), got {factor_vae!r}") from None
    if not isinstance(given, dict) or set(given) - set(FACTOR_CRITIC_DEFAULTS):
        raise TypeError(f"factor_vae: the critic's options are a dict with keys among {sorted(FACTOR_CRITIC_DEFAULTS)}, got "
                        f"{given!r}")
    if not callable(gamma):
        gamma = _nonneg("factor_vae: gamma", gamma)
    cfg = {**FACTOR_CRITIC_DEFAULTS, **given}
    sizes = []
    for name in ("width", "depth"):
        v = cfg[name]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"factor_vae: {name} must be an integer, got {v!r}")
        if v < 1:
            raise ValueError(f"factor_vae: {name} must be >= 1, got {v!r}")
        sizes.append(int(v))
    try:
        lr = float(cfg["lr"])
        b1, b2 = (float(b) for b in cfg["betas"])
    except (TypeError, ValueError):
        raise TypeError(f"factor_vae: lr must be a number and betas a pair of numbers, got {cfg['lr']!r} and {cfg['betas']!r}") from None
    if not (np.isfinite(lr) and lr > 0.0):
        raise ValueError(f"factor_vae: lr must be finite and > 0, got {cfg['lr']!r}")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):      # (NaN fails the comparisons)
        raise ValueError(f"factor_vae: betas must lie in [0, 1), got {cfg['betas']!r}")
    return gamma, sizes[0], sizes[1], lr, (b1, b2)


def _factor_critic_phase(trainer, carried, drawn, global_batch, grad_hook):
    """FactorVAE's critic phase, last in the iteration (Kim & Mnih 2018, algorithm 2): ``carried`` is
    the encoder phase's z, detached -- no second encode --, ``drawn`` the uniforms of ``permute_dims``.  One critic forward on
    the 2B rows ``[z; z_perm]``, the cross-entropy as a mean over 2 x the global batch, full backward, exchange, Adam step."""
    (z,), (u,) = carried, drawn
    o = trainer._objective[0].owns.part
    critic, opt, flat = (getattr(trainer, a) for a in (o.net, o.opt, o.flat))
    trainer._zero(critic, flat, None, grad_hook)      # (no weight of it is updated inside the backward: its layers are small)
    logits = critic(torch.cat([z, F.permute_dims(z, u)]))
    loss, acc = F.factor_critic_loss(logits, 2 * global_batch)
    _backward([loss])
    trainer._exchange(flat)
    if grad_hook:
        grad_hook("critic", critic)
    opt.step()
    return dict(critic_loss=loss.detach(), critic_acc=acc)


_FACTOR_CRITIC = _Owned(
    _Part("critic", LatentCritic, "optimizer_critic", "flat_critic", "critic", "latent_critic_optimizer"), "latent_critic",
    build=lambda opt, args, generator: LatentCritic(opt.n_hidden, args[0], args[1], generator=generator),
    adam=lambda args: dict(lr=args[2], betas=args[3]),
    drawn=(_Drawn("permute", "uniform", "permute_generator"),),
    phase=_factor_critic_phase)


# The table: the methods are looked up on the network when called (a test may replace one).
_OBJECTIVES = (
    _Objective("tc_decomposition", _parse_tc,       # args: (alpha, gamma, dataset_size); `beta` weighs the total correlation
               lambda net, data, eps, beta, args, prior: net.forward_with_tc(data, eps, beta, *args),
               ("mi", "tc", "dwkl"), needs_dataset_size=True),
    _Objective("dip_vae", _parse_dip,               # args: (variant, lambda_od, lambda_d); `beta` weighs the KL
               lambda net, data, eps, beta, args, prior: net.forward_with_dip(data, eps, beta, *args),
               ("kl", "dip_od", "dip_d")),
    _Objective("mmd_vae", _parse_mmd,               # args: (kernel, lambda_mmd, bandwidths); the MMD is between z and `prior`
               lambda net, data, eps, beta, args, prior: net.forward_with_mmd(data, eps, prior, beta, *args),
               ("kl", "mmd", "mmd_kzz"), latents=("prior",)),
    _Objective("kl_control", _parse_klc,            # args: (capacity: its word, free_bits); `beta` weighs |kl_floored - B capacity|
               lambda net, data, eps, beta, args, prior: net.forward_with_klc(data, eps, beta, *args),
               ("kl", "kl_floored", "dims_above"), word="capacity"),
    _Objective("factor_vae", _parse_factor,         # args: (gamma: its word, width, depth, lr, betas, the critic); `beta` weighs the KL
               lambda net, data, eps, beta, args, prior: net.forward_with_factor(data, eps, beta, args[0], args[-1]),
               ("kl", "tc"), word="gamma", owns=_FACTOR_CRITIC),
)


def _objective_args(keyword):
    """The public attribute of a trainer named as the constructor keyword: the objective's parsed arguments, None when off."""
    return property(lambda self: self._objective[1] if self._objective and self._objective[0].keyword == keyword else None)


class _GraphedSteps:
    """What the three trainers share: the construction (`_setup`), the one path an iteration takes (`_drive`: eager, or
    -- `_graph_usable` -- a HIP-graph replay with its warm-up count per shape, capture and fallback), the guard, the
    schedules, the weight EMA and the augmentation of the discriminator's inputs.  A trainer declares `_parts` (who is in
    it; everything that lists networks, optimizers or exchanges derives from that table), `_latents`, `_has_labels`,
    `_accumulate`, `_augment_sets`, and `_iteration`: the iteration itself on given tensors."""
    graph = False
    iteration = 0
    probe = None      # callable(name, tensor): taps of an (eager) iteration, see BetaVAEGANTrainer._iteration
    _parts = ()       # the table: one `_Part` per network, in the order the reference constructs them
    _latents = ()     # names of the (batch, n_hidden) N(0,1) draws of an iteration, in draw order
    _has_labels = False       # the iteration takes the two label scalars and the global batch (the BCE's divisor)
    _accumulate = False       # layers applied twice before one backward add their second parameter gradient in-kernel
    _augment_sets = 0         # parameter sets of ``diff_augment`` an iteration uses (0: the trainer has no discriminator)
    _augment = None           # (policy names, bit set, p) of ``diff_augment``, None when off
    _gan_loss = None          # name of the adversarial loss on the logit (``gan_loss``), None: the reference's BCE on p
    _ada = None               # (target, rate, interval) of ``ada``, the controller of the augmentation's p; None when off
    _ada_state = None         # with ``ada``: the controller's eight device words (`ops.ada_state`), never replaced
    augment_p = None          # with ``ada``: word 0 of them as a one-element fp32 device view -- the p the kernels read

    def _setup(self, device, seed, lr, opt, fused_adam, graph, nonfinite_guard, max_grad_norm, skip_nonfinite, lr_scheduler,
               beta_schedule, weight_decay, decoupled_weight_decay, device_hyper, ema_decay, tc_decomposition, dataset_size,
               data_parallel=None, capturable=None, dip_vae=None, mmd_vae=None, kl_control=None, diff_augment=None,
               factor_vae=None, gan_loss=None, ada=None):
        """The constructor body of every trainer (new_betavaegan.py:36-53, new_vae.py:33-37, new_gan.py:47-61).  A trainer
        with a KL term has set `beta` before."""
        has_beta = hasattr(self, "beta")
        self.opt = opt or ModelOpt()
        self.device = torch.device(device)
        self._single_use = {}     # (id(network), DEFER_WGRAD) -> its weights that may be updated inside the backward
        on_gpu = self.device.type == "cuda"
        _use_tuned_gemms(self.device)
        self._select_objective(dict(tc_decomposition=tc_decomposition, dip_vae=dip_vae, mmd_vae=mmd_vae, kl_control=kl_control,
                                    factor_vae=factor_vae), dataset_size, has_beta)
        if diff_augment is not None:
            if not self._augment_sets:
                raise TypeError(f"{type(self).__name__} has no discriminator: diff_augment does not apply")
            self._augment = _parse_diff_augment(diff_augment)
        if ada is not None and ada is not False:
            if not self._augment_sets:
                raise TypeError(f"{type(self).__name__} has no discriminator: ada does not apply")
            self._ada = _parse_ada(ada)
            if self._augment is None:
                raise ValueError("ada adapts the probability of diff_augment: pass diff_augment=policy or (policy, p0) with it")
            if isinstance(diff_augment, str):            # (a bare policy: Karras's start, p = 0 -- not the fixed-p default 1)
                self._augment = (*self._augment[:2], 0.0)
            self._ada_state = ops.ada_state(self.device, self._augment[2])
            self.augment_p = self._ada_state[0:1].view(torch.float32)
        if gan_loss is not None:
            if not self._augment_sets:
                raise TypeError(f"{type(self).__name__} has no discriminator: gan_loss does not apply")
            self._gan_loss = F.gan_loss_name(gan_loss)
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        self._skipped = {}
        self.world, self.rank = _dist_world(), _dist_rank()
        self.dp = (self.world > 1) if data_parallel is None else data_parallel
        self._graph_init(graph, on_gpu, fused_adam, self.dp)
        if capturable is None:
            capturable = self.graph
        # Constructed on the CPU right behind the seed, then initialised, both in table order: the reference's RNG
        # stream, hence its weights (new_betavaegan.py:36-47).  Nothing that draws from the CPU generator may come between.
        torch.manual_seed(seed)
        nets = [p.cls(self.opt) for p in self._parts]
        for net in nets:
            net.apply(weights_init)
        for p, net in zip(self._parts, nets):
            setattr(self, p.net, net.to(self.device))
        fused = fused_adam and on_gpu
        self.nonfinite_guard = self._resolve_guard(nonfinite_guard, fused)
        adam = dict(max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        adam.update(self._schedule_args(lr_scheduler, beta_schedule, device_hyper, weight_decay, decoupled_weight_decay,
                                        fused and capturable, has_beta))
        ema = self._ema_setup(ema_decay, getattr(self, self._ema_names[0]), fused_adam)      # (deep copy: on the device)
        for p in self._parts:
            setattr(self, p.opt, _make_adam(getattr(self, p.net).parameters(), lr, fused, capturable, self.nonfinite_guard,
                                            ema=ema if p.opt == self._ema_names[1] else None, **adam))
        self._make_schedulers()
        self._own_network(seed, fused, capturable, adam)          # (behind the schedulers: its optimizer has none)
        for p in self._parts:         # in table order on every rank: creating the communicator is collective
            net = getattr(self, p.net)
            setattr(self, p.flat, FlatGrads(net.parameters(), silent=shadowed_bias_params(net)) if self.dp else None)
        self.latent_generator = _latent_generator(self.device, seed, self.rank)
        if self._augment is not None:
            self.augment_generator = _augment_generator(self.device, seed, self.rank)
        if self._owned is not None and self._owned.drawn:
            self.permute_generator = _permute_generator(self.device, seed, self.rank)
        if self._has_labels:
            self.label_rng = _shared_label_rng(seed)      # used by train_epoch when world > 1: one draw per GLOBAL batch
        for net in self._nets():
            net.train()
        self.iteration = 0

    # ---- a network the selected objective owns (`_Owned`) ----------------------------------------
    @property
    def _owned(self):
        return self._objective[0].owns if self._objective is not None else None

    def _own_network(self, seed, fused, capturable, adam):
        """`_setup`: build the network the objective owns from a generator of the trainer's own (the global CPU stream, and
        with it every other network's weights, stays what it is without the keyword), give it its optimizer -- the same
        guard, clipping, skipping and device words as the others; its own lr and betas; no scheduler, weight decay or EMA --
        and append its `_Part` to this trainer's table: from here on everything that lists networks, optimizers or
        exchanges finds it."""
        owned = self._owned
        if owned is None:
            return
        args = self._objective[1]
        net = owned.build(self.opt, args, _owned_generator(seed))
        setattr(self, owned.part.net, net.to(self.device))
        own = dict(adam, weight_decay=0.0, decoupled_weight_decay=False, **owned.adam(args))
        setattr(self, owned.part.opt, _make_adam(net.parameters(), own.pop("lr"), fused, capturable, self.nonfinite_guard, **own))
        self._parts = (*type(self)._parts, owned.part)

    def _owned_checkpoint(self):
        """The additional checkpoint keys -- present only with an objective that owns a network: its weights, its optimizer."""
        owned = self._owned
        if owned is None:
            return {}
        return {owned.ckpt: getattr(self, owned.part.net).state_dict(), owned.part.ckpt: getattr(self, owned.part.opt).state_dict()}

    @torch.no_grad()
    def _owned_restore(self, ck, in_place=False):
        """After the trainer's own networks were loaded: the owned network and its optimizer from their checkpoint keys -- a
        checkpoint without them (one written without the keyword) leaves both as they are, as a missing EMA key does.
        ``in_place``: copied into the existing tensors (`load_in_place`)."""
        owned = self._owned
        if owned is None or owned.ckpt not in ck or owned.part.ckpt not in ck:
            return
        net, opt = getattr(self, owned.part.net), getattr(self, owned.part.opt)
        if not in_place:
            net.load_state_dict(ck[owned.ckpt])
            opt.load_state_dict(ck[owned.part.ckpt])
            return
        for k, v in net.state_dict().items():
            v.copy_(ck[owned.ckpt][k])
        if isinstance(opt, HipAdam):
            opt.load_state_in_place(ck[owned.part.ckpt])
            opt.refresh_weight_bounds()
        else:
            opt.load_state_dict(ck[owned.part.ckpt])

    def _split_owned(self, latents):
        """`_iteration`: its inputs without those of the owned network's phase (last in `_drawn` order), and those."""
        n = len(self._owned.drawn) if self._owned is not None else 0
        return (latents[:len(latents) - n], tuple(latents[len(latents) - n:])) if n else (latents, ())

    def _owned_phase(self, drawn, batch, global_batch, grad_hook):
        """The phase of the owned network, behind the encoder phase's optimizer step: its loss outputs ({} without one).
        ``global_batch``: what `step` was given, else this replica's batch times the world size."""
        owned = self._owned
        if owned is None:
            return {}
        carried, self._carried = self._carried, ()
        gb = global_batch if global_batch is not None else batch * self.world
        return owned.phase(self, carried, drawn, gb, grad_hook)

    # ---- the table of parts, read ------------------------------------------------------------------------------------
    def _nets(self):
        return [getattr(self, p.net) for p in self._parts]

    def _optimizers(self):
        return {p.opt: getattr(self, p.opt) for p in self._parts}

    def _flats(self):
        return [f for f in (getattr(self, p.flat) for p in self._parts) if f is not None]

    def _guarded_optimizers(self):
        """[(attribute name of the network, network, its optimizer)]"""
        return [(p.net, getattr(self, p.net), getattr(self, p.opt)) for p in self._parts]

    @property
    def _checkpoint_optimizer_keys(self):
        return {p.opt: p.ckpt for p in self._parts}

    def _graph_init(self, graph, on_gpu, fused_adam, dp):
        """A data-parallel iteration is captured too when its exchange is capturable (FlatGrads on our own RCCL
        communicator); over torch.distributed's collectives (gloo, VG_OWN_RCCL=0) it stays eager."""
        dp_ok = (not dp) or (on_gpu and FlatGrads.own_rccl and dist.is_available() and dist.is_initialized()
                             and dist.get_backend() == "nccl")      # (+ FlatGrads.capturable, checked per step)
        self.graph = (GRAPH_DEFAULT if graph is None else bool(graph)) and on_gpu and fused_adam and dp_ok
        self._graphs, self._shape_steps = {}, {}
        return self.graph

    _pack_plans = None

    def _run_with_pack_plan(self, body, nets):
        """``body(prepack)`` is one iteration; ``prepack(name)`` re-packs, in ONE launch, every split-bf16 filter of network
        ``name`` (None: of all networks) that the trainer's convolutions are known to ask for -- to be called at the start
        of the iteration and after each optimizer step.  The first iteration only records what is asked for (the filters
        are packed one by one on first use, as without a plan)."""
        if self._pack_plans is None:
            with ops.record_pack_requests() as rec:
                out = body(lambda name=None: None)
            self._pack_plans = plans = {name: [] for name in nets}
            for r in rec.requests:          # under the network that owns the parameter OBJECT, once per (object, layout)
                name = next((n for n, net in nets.items() if any(p is r.w for p in net.parameters())), None)
                if name is not None and not any(q.w is r.w and (q.transposed, q.stride) == (r.transposed, r.stride)
                                                for q in plans[name]):
                    plans[name].append(r)
            return out
        plans = self._pack_plans
        return body(lambda name=None: ops.prepack_filters(plans[name] if name is not None
                                                          else [r for v in plans.values() for r in v]))

    def _graph_usable(self, data, grad_hook):
        if self.graph and self._any_module_hooks():      # a replay would never fire them (and a capture would run their
            return False                                 # Python body once): hooked networks step eagerly
        return (self.graph and grad_hook is None and self.probe is None and ops._timing is None and data.is_cuda
                and all(f.capturable for f in self._flats())
                and all(isinstance(o, HipAdam) and o.device_scalars for o in self._optimizers().values())
                and not torch.cuda.is_current_stream_capturing())

    def _any_module_hooks(self):
        from .model import _has_hooks
        return _has_hooks([m for net in self._nets() for m in net.modules()])

    # ---- non-finite guard ----------------------------------------------------------------------------------------
    nonfinite_guard = False
    max_grad_norm, skip_nonfinite = None, False      # clipping by global norm / skipping a non-finite step (optim.HipAdam)
    _finite_at = 0          # `iteration` when the flags were last known clean

    @staticmethod
    def _resolve_guard(nonfinite_guard, uses_hip_adam):
        """``None``: on whenever the optimizer steps run on HipAdam (VG_NONFINITE_GUARD=0 turns that default off)."""
        if nonfinite_guard is None:
            return bool(uses_hip_adam) and NONFINITE_GUARD_DEFAULT
        return bool(nonfinite_guard)

    @torch.no_grad()
    def _read_finite(self, extra=None):
        """The guard's check and, in the SAME device -> host copy, the values of the float64 device tensor ``extra``
        (an epoch's loss sums: `train_epoch` still reads the device once).  Raises `NonFiniteError`, else returns the
        values of ``extra`` as a list."""
        names, bits, skipping = [], [], []
        for attr, net, opt in self._guarded_optimizers():
            named = {p: f"{attr}.{k}" for k, p in net.named_parameters()}
            ps = [p for g in opt.param_groups for p in g["params"]]
            names += [named.get(p, f"{attr}.<parameter {i}>") for i, p in enumerate(ps)]
            if isinstance(opt, HipAdam) and opt.nonfinite_guard:
                b = opt.nonfinite_bits()
            else:
                b = isfinite_bits(ps, self.device)
            if isinstance(opt, HipAdam) and opt.skip_nonfinite:
                # a word with only GRAD up is a step that was SKIPPED: the weights are clean.  Those bits are dropped here
                # and cleared in the optimizer's words (device ops, no synchronisation); the count travels in the copy below
                skipping.append((attr, opt))
                b = torch.where(b == NONFINITE_GRAD, torch.zeros_like(b), b)
                if opt.nonfinite_guard:
                    w = opt.nonfinite_words()
                    w.copy_(torch.where(w == NONFINITE_GRAD, torch.zeros_like(w), w))
            bits.append(b)
        bits = torch.cat(bits) & (NONFINITE_GRAD | NONFINITE_PARAM)      # (the words are the optimizer's: other bits are not ours)
        anything = (bits != 0).any().to(torch.int32).reshape(1)
        if _dist_world() > 1:
            dist.all_reduce(anything, op=dist.ReduceOp.MAX)
        n_extra = 0 if extra is None else extra.numel()
        parts = [bits.to(torch.float64), anything.to(torch.float64)]      # (small integers: exact in float64)
        if n_extra:
            parts.append(extra.reshape(-1).to(torch.float64))
        parts += [opt.clip_record()[3:4].to(device=bits.device, dtype=torch.float64) for _, opt in skipping]
        host = torch.cat(parts).tolist()                                  # the one device -> host read
        if skipping:
            self._skipped = {attr: int(c) for (attr, _), c in zip(skipping, host[-len(skipping):])}
            host = host[:-len(skipping)]
        bits, anything, extra = [int(b) for b in host[:len(names)]], host[len(names)], host[len(names) + 1:]
        if not anything:
            self._finite_at = self.iteration
            return extra
        kinds = {NONFINITE_GRAD: "grad", NONFINITE_PARAM: "param", NONFINITE_GRAD | NONFINITE_PARAM: "grad+param"}
        raise NonFiniteError([(n, kinds[b]) for n, b in zip(names, bits) if b], self._finite_at, self.iteration)

    def check_finite(self):
        """Raise `NonFiniteError` if an optimizer step since the flags were last cleared read a non-finite gradient or
        wrote a non-finite parameter; return None when the run is clean.  One device -> host copy for all optimizers'
        flag words -- `step` itself never synchronises; this is the check on demand after any `step`, and `train_epoch`
        makes it once per epoch, in the copy that reads the epoch's sums.  With ``skip_nonfinite=True`` a word with only
        the GRAD bit up is a step that was skipped -- the weights are clean: it does not raise, the bit is cleared, and
        `skipped_steps` counts it; a PARAM bit raises as ever.  Optimizers without the kernel's guard
        (torch.optim.Adam: CPU, ``fused_adam=False``; ``nonfinite_guard=False``) are checked with ``torch.isfinite`` over
        their parameters and gradients as they are now.  Data parallel: the "anything set" bit is all-reduced (MAX)
        first, so every rank raises at the same call."""
        self._read_finite()
        return None

    def skipped_steps(self):
        """``{network attribute: optimizer steps skipped so far}`` of the optimizers built with ``skip_nonfinite=True``
        (empty without): `check_finite`, whose one device -> host copy carries the counts -- so this raises
        `NonFiniteError` where that does."""
        self._skipped = {}
        self._read_finite()
        return dict(self._skipped)

    def clear_nonfinite(self):
        """Zero the guard's flag words (device memsets, no synchronisation): after the state was restored."""
        for _, _, opt in self._guarded_optimizers():
            if isinstance(opt, HipAdam) and opt.nonfinite_guard:
                opt.clear_nonfinite()
        self._finite_at = self.iteration

    # ---- schedules: learning rate, beta and weight decay ---------------------------------------------------------
    beta_schedule = None
    device_hyper = False
    weight_decay, decoupled_weight_decay = 0.0, False
    _beta_dev = None          # with device_hyper: the persistent fp32 word the KL kernels read
    _beta_written = None

    def _schedule_args(self, lr_scheduler, beta_schedule, device_hyper, weight_decay, decoupled_weight_decay, capturable,
                       has_beta=True):
        """Validate the schedule arguments and resolve ``device_hyper`` (None: on exactly when a scheduler, a beta schedule or
        a schedule of the objective's own word is given -- and the optimizers can carry it: HipAdam with device scalars;
        without, the schedules still run and the
        steps stay eager or re-key as before).  Returns the keyword arguments of `_make_adam`."""
        if beta_schedule is not None and not has_beta:
            raise TypeError(f"{type(self).__name__} has no KL term: beta_schedule does not apply")
        for name, fn in (("lr_scheduler", lr_scheduler), ("beta_schedule", beta_schedule)):
            if fn is not None and not callable(fn):
                raise TypeError(f"{name} must be a callable, got {type(fn).__name__}")
        wd = float(weight_decay)
        if not wd >= 0.0:
            raise ValueError(f"weight_decay must be >= 0, got {weight_decay!r}")
        self.weight_decay, self.decoupled_weight_decay = wd, bool(decoupled_weight_decay)
        self._lr_scheduler_factory, self.beta_schedule = lr_scheduler, beta_schedule
        if device_hyper is None:
            self.device_hyper = ((lr_scheduler is not None or beta_schedule is not None or self._word_schedule is not None)
                                 and bool(capturable))
        else:
            self.device_hyper = bool(device_hyper)
            if self.device_hyper and not capturable:
                raise ValueError("device_hyper=True needs optimizers whose step can be captured (a CUDA trainer with "
                                 "fused_adam and graph / capturable on)")
        if self.device_hyper and has_beta:
            self._beta_dev = torch.full((1,), self.beta, dtype=torch.float32, device=self.device)
            self._beta_written = self.beta
            if self._word is not None:      # the objective's own word lives beside beta's: both floats or both words
                self._word_dev = torch.full((1,), self._word, dtype=torch.float32, device=self.device)
                self._word_written = self._word
        return dict(weight_decay=wd, decoupled_weight_decay=self.decoupled_weight_decay, device_hyper=self.device_hyper)

    def _make_schedulers(self):
        """``lr_scheduler(optimizer)`` for each of the trainer's optimizers -> `lr_schedulers`, keyed by attribute name."""
        self.lr_schedulers = {}
        if self._lr_scheduler_factory is None:
            return
        from torch.optim.lr_scheduler import LRScheduler
        for name, opt in self._optimizers().items():
            sched = self._lr_scheduler_factory(opt)
            if not isinstance(sched, LRScheduler):
                raise TypeError(f"lr_scheduler must return a torch.optim.lr_scheduler.LRScheduler, got "
                                f"{type(sched).__name__} for {name}")
            self.lr_schedulers[name] = sched

    # ---- the objective of the KL phase: the analytic KL, or one entry of `_OBJECTIVES` ---------------------------------------
    _objective = None         # (entry, its parsed arguments) of the selected one
    dataset_size = None       # N of minibatch-weighted sampling
    tc_decomposition = _objective_args("tc_decomposition")
    dip_vae = _objective_args("dip_vae")
    mmd_vae = _objective_args("mmd_vae")
    _word = None              # the current value of the selected objective's own scheduled word (`_Objective.word`), a float
    _word_schedule = None     # callable iteration -> that value, or None (a constant, or set by hand)
    _word_dev = None          # with device_hyper: the persistent fp32 word the objective's kernels read
    _word_written = None
    _carried = ()             # what the objective's forward returned behind ``parts``: for the owned network's phase

    def _select_objective(self, given, dataset_size, has_beta=True):
        """A trainer's constructor: ``given`` maps every keyword of the table to its value; at most one is not None.  The
        entries are taken in table order, each checked in full before the next."""
        for o in _OBJECTIVES:
            value = given[o.keyword]
            with_size = o.needs_dataset_size and dataset_size is not None
            if value is None and not with_size:
                continue
            if not has_beta:
                raise TypeError(f"{type(self).__name__} has no KL term: {o.keyword} does not apply")
            if value is not None:
                if self._objective is not None:
                    every = [e.keyword for e in reversed(_OBJECTIVES)]
                    raise ValueError(f"{', '.join(every[:-1])} and {every[-1]} each replace the KL term of the encoder phase: "
                                     f"pass one of them (got {o.keyword} and {self._objective[0].keyword})")
                args = o.parse(value, self.opt)
                if o.word is not None:
                    word, *args = args
                    self._word_schedule = word if callable(word) else None
                self._objective = (o, tuple(args))
                if o.word is not None:
                    self._word = self._word_checked(word(0)) if callable(word) else word
                self._latents = (*type(self)._latents, *o.latents)
            if with_size:
                if int(dataset_size) != dataset_size or int(dataset_size) < 1:
                    raise ValueError(f"dataset_size must be an integer >= 1, got {dataset_size!r}")
                self.dataset_size = int(dataset_size)

    def _objective_key(self):
        """The selected objective with every frozen kernel argument, `dataset_size` included where it is one."""
        if self._objective is None:
            return None
        o, args = self._objective
        return o.keyword, (*args, self.dataset_size) if o.needs_dataset_size else args

    def _dataset_size_missing(self):
        return self._objective is not None and self._objective[0].needs_dataset_size and self.dataset_size is None

    def _dataset_size_from(self, loader):
        """`train_epoch` / `fit`: a ``dataset_size`` that was not given is the loader's ``len(loader.dataset)``."""
        if self._dataset_size_missing():
            self.dataset_size = int(len(loader.dataset))

    def _forward_kl(self, net, data, eps, prior=None):
        """The encoder-side forward of the KL phase: ``recon, mu, logvar, kld, parts`` -- the analytic KL weighted by `beta`
        (``parts`` is None), or the selected objective's loss and its three parts."""
        if self._objective is None:
            return (*net.forward_with_kl(data, eps, self._kl_beta()), None)
        args = self._objective_key()[1]
        if self._word is not None:
            args = (self._word_dev if self._word_dev is not None else self._word, *args)
        owned = self._owned
        if owned is None:
            return self._objective[0].forward(net, data, eps, self._kl_beta(), args, prior)
        # the owned network only relays gradients here, as the discriminator in the decoder phase: no weight gradients are
        # formed for it (what requires a gradient is decided when the forward builds its graph)
        own = getattr(self, owned.part.net)
        self._set_frozen(own, True)
        try:
            out = self._objective[0].forward(net, data, eps, self._kl_beta(), (*args, own), prior)
        finally:
            self._set_frozen(own, False)
        self._carried = tuple(out[5:])
        return out[:5]

    def _with_prior(self, given, prior):
        """`step`'s latents in `_latents` order: behind the trainer's own, the prior's draw (or None: drawn) of an objective
        that takes one."""
        if "prior" in self._latents:
            return (*given, prior)
        if prior is not None:
            owners = " / ".join(o.keyword for o in _OBJECTIVES if "prior" in o.latents)
            raise TypeError(f"{type(self).__name__}.step: prior= belongs to {owners}, which is off")
        return given

    def _kl_part_outputs(self, parts):
        """The additional loss keys -- present only with an objective."""
        if parts is None:
            return {}
        return {name: parts[n] for n, name in enumerate(self._objective[0].parts)}

    def _kl_beta(self):
        """What the KL kernels take: the device word with ``device_hyper`` (eager and captured alike), else the float."""
        return self._beta_dev if self._beta_dev is not None else self.beta

    def _sync_beta(self):
        """`beta` into its device word when it differs from what was last written (a device fill, no synchronisation;
        never inside a capture: `step` and a replay call it in front of the launches)."""
        if self._beta_dev is not None and self.beta != self._beta_written:
            self._beta_dev.fill_(self.beta)
            self._beta_written = self.beta

    def _word_checked(self, value):
        """A value of the objective's own word (a schedule's, or set by hand) as a finite float >= 0."""
        return _nonneg(f"{self._objective[0].keyword}: {self._objective[0].word}", value)

    def _sync_word(self):
        """The objective's own value into its device word, as `_sync_beta` (a device fill, never inside a capture)."""
        if self._word_dev is not None and self._word != self._word_written:
            self._word_dev.fill_(self._word)
            self._word_written = self._word

    @property
    def capacity(self):
        """The KL capacity of ``kl_control`` this step runs (ran) with, in nats per sample; None without the option."""
        return self._word if self._objective and self._objective[0].word == "capacity" else None

    def set_capacity(self, value):
        """Set the KL capacity by hand (a schedule, if any, overwrites it at the start of the next step).  With
        ``device_hyper`` the next step picks it up without a new capture."""
        if self.capacity is None:
            raise TypeError(f"{type(self).__name__}: construct with kl_control=... to have a KL capacity")
        self._word = self._word_checked(value)

    @property
    def kl_control(self):
        """``(capacity, free_bits)`` as they are now (read-only); None when the option is off."""
        return None if self.capacity is None else (self._word, *self._objective[1])

    @property
    def gamma(self):
        """The weight of ``factor_vae``'s total-correlation estimate this step runs (ran) with; None without the option."""
        return self._word if self._objective and self._objective[0].word == "gamma" else None

    def set_gamma(self, value):
        """Set that weight by hand (a schedule, if any, overwrites it at the start of the next step).  With ``device_hyper``
        the next step picks it up without a new capture."""
        if self.gamma is None:
            raise TypeError(f"{type(self).__name__}: construct with factor_vae=... to have a total-correlation weight")
        self._word = self._word_checked(value)

    @property
    def factor_vae(self):
        """``(gamma, dict(width=, depth=, lr=, betas=))`` as they are now (read-only); None when the option is off."""
        if self.gamma is None:
            return None
        return self._word, dict(zip(FACTOR_CRITIC_DEFAULTS, self._objective[1]))

    def _begin_step(self):
        if self._dataset_size_missing():
            raise ValueError(f"{type(self).__name__}: {self._objective[0].keyword} needs dataset_size (the number of training "
                             "samples): pass dataset_size=..., or train through train_epoch / fit, which take it from the loader")
        if self.beta_schedule is not None:
            self.beta = float(self.beta_schedule(self.iteration))
        self._sync_beta()
        if self._word_schedule is not None:
            self._word = self._word_checked(self._word_schedule(self.iteration))
        self._sync_word()
        if self.ema_schedule is not None:      # the decay word follows in front of the launches (`HipAdam.sync_hyper`)
            self._ema_pair()[1].set_ema_decay(float(self.ema_schedule(self.iteration)))

    def _end_step(self):
        for sched in self.lr_schedulers.values():      # once per iteration: EG's two optimizer steps share one lr
            sched.step()

    def set_lr(self, value, which=None):
        """Set the learning rate by hand: of every optimizer, or of the one named ``which`` (its attribute name, a key of
        `_optimizers`).  With ``device_hyper`` the next step picks it up without a new capture; an lr scheduler, if any,
        overwrites it at its next step."""
        opts = self._optimizers()
        if which is not None and which not in opts:
            raise KeyError(f"no optimizer {which!r}: {sorted(opts)}")
        owned = self._owned.part.opt if self._owned is not None else None      # (its own lr: set only when named)
        for name, opt in opts.items():
            if (which is None and name != owned) or name == which:
                for group in opt.param_groups:
                    group["lr"] = float(value)

    def set_beta(self, value):
        """Set the KL weight by hand (a ``beta_schedule``, if any, overwrites it at the start of the next step)."""
        if not hasattr(self, "beta"):
            raise TypeError(f"{type(self).__name__} has no KL term")
        self.beta = float(value)

    def _schedule_checkpoint(self):
        """The additional checkpoint keys -- present only when a schedule exists."""
        extra = {}
        if self.lr_schedulers:
            extra["lr_schedulers"] = {n: s.state_dict() for n, s in self.lr_schedulers.items()}
        if (self.lr_schedulers or self.beta_schedule is not None or self.ema_schedule is not None
                or self._word_schedule is not None):
            extra["iteration"] = self.iteration
        return extra

    def _schedule_restore(self, ck, in_place=False):
        """Restore the additional keys when the checkpoint has them (a reference checkpoint has none).  ``in_place``: the
        optimizers' param_groups were not loaded (only their state was copied), so the learning rates are taken over
        here."""
        if "iteration" in ck:
            self.iteration = int(ck["iteration"])
        for name, sd in ck.get("lr_schedulers", {}).items():
            if name in self.lr_schedulers:
                self.lr_schedulers[name].load_state_dict(sd)
        if in_place and "lr_schedulers" in ck:
            for name, key in self._checkpoint_optimizer_keys.items():
                if self._owned is not None and name == self._owned.part.opt:      # (no scheduler; its key may be absent)
                    continue
                for group, saved in zip(getattr(self, name).param_groups, ck[key]["param_groups"]):
                    group["lr"] = saved["lr"]
        if self.beta_schedule is not None and "iteration" in ck:
            self.beta = float(self.beta_schedule(max(self.iteration - 1, 0)))      # (the last step's; the next step sets its own)
        if self._word_schedule is not None and "iteration" in ck:
            self._word = self._word_checked(self._word_schedule(max(self.iteration - 1, 0)))

    # ---- weight EMA of the generating network --------------------------------------------------------------------
    ema_model = None          # the shadow network: a deep copy whose parameters the averaging Adam step writes
    ema_schedule = None       # callable iteration -> decay in [0, 1), or None (a constant decay)
    _ema_names = None         # (attribute of the averaged network, of its optimizer, checkpoint key of the shadow)

    def _ema_setup(self, ema_decay, net, fused_adam):
        """``ema_decay`` of a trainer's constructor -> the ``ema`` argument of `_make_adam` (None: no average).  Builds
        `ema_model`: a ``copy.deepcopy`` of ``net`` as it is now (on its device; a deep copy draws no random number, so
        the initialisation stream is the reference's), parameters without gradient, BatchNorm buffers its own."""
        if ema_decay is None:
            return None
        if callable(ema_decay):
            schedule, first = ema_decay, float(ema_decay(0))
            if not 0.0 <= first < 1.0:
                raise ValueError(f"ema_decay: the schedule must return a decay in [0, 1), got {first!r} at iteration 0")
        else:
            schedule, first = None, float(ema_decay)
            if not 0.0 < first < 1.0:
                raise ValueError(f"ema_decay must be a float in (0, 1) or a callable iteration -> [0, 1), got {ema_decay!r}")
        if self.device.type != "cuda" or not fused_adam:
            why = f"its device is {self.device.type!r}" if self.device.type != "cuda" else "fused_adam=False"
            raise ValueError("ema_decay: the average is kept inside the fused Adam step (optim.HipAdam), and this "
                             f"trainer's optimizers are torch.optim.Adam: {why}")
        self.ema_schedule = schedule
        self.ema_model = copy.deepcopy(net)
        for p in self.ema_model.parameters():
            p.requires_grad_(False)
        return first, list(self.ema_model.parameters())

    def _ema_pair(self):
        if self.ema_model is None:
            raise ValueError(f"{type(self).__name__}: construct with ema_decay=... to keep and use an average of the weights")
        return getattr(self, self._ema_names[0]), getattr(self, self._ema_names[1])

    def _sampling_net(self, use_ema):
        """The network that samples and reconstructs: the live one, or -- ``use_ema`` -- the shadow."""
        if not use_ema:
            return getattr(self, self._ema_names[0])
        self._ema_pair()
        return self.ema_model

    def latent_report(self, loader, n_eval=None, eval_mode=False, use_ema=False, factors=None, generator=None):
        """Whether the encoder disentangled anything (metrics.py): encodes every image of
        ``loader`` and returns `metrics.elbo_decomposition` of the posteriors -- ``mi``, ``tc``, ``dwkl``, ``kl``,
        ``h_joint``, ``h_dim``, ``kl_dim``, ``active_units`` -- plus the keys of `metrics.mig` when ``factors`` ([N] or
        [N, K] integers, in the loader's order) is given or the loader's labels take more than one value.  ``n_eval``:
        evaluation points of the decomposition (default: every row).  ``eval_mode`` / ``use_ema``: as in `evaluate`."""
        from . import metrics
        net = self._sampling_net(use_ema)
        mu, logvar, labels = metrics.encode_dataset(net, loader, eval_mode=eval_mode)
        report = metrics.elbo_decomposition(mu, logvar, n_eval=n_eval, generator=generator)
        if factors is None and labels is not None and not labels.is_floating_point() and bool((labels != labels[0]).any()):
            factors = labels
        if factors is not None:
            report.update(metrics.mig(mu, logvar, factors, generator=generator))
        return report

    def reconstruction_report(self, loader, sample=False, eval_mode=False, use_ema=False, dis_l=False, generator=None):
        """How well held-out images come back through encoder and decoder (recon_quality.py):
        under ``no_grad`` every batch of ``loader`` (``(data, labels)`` pairs, or bare image batches) is encoded, decoded
        and scored against itself; returns `recon_quality.report` over all of them -- ``n``, ``mse`` (the mean per-image
        sum of squared errors), ``psnr``, ``ssim``, ``ssim_std``, ``ms_ssim``, ``ms_ssim_scales``; the scalars are 0-dim
        fp64 device tensors.  ``sample=False`` decodes the posterior mean, ``z = mu``; ``sample=True`` runs the network's
        own ``forward`` with the latent noise drawn from ``generator`` (default: the device's global one).
        ``eval_mode`` / ``use_ema``: as in `evaluate`.  BatchNorm runs in TRAINING mode by default, as everywhere in the
        evaluation half: batch statistics, and the running ones move; ``eval_mode=True`` runs inside
        ``model.eval_mode(net)`` and moves nothing.  ``dis_l=True`` (`BetaVAEGANTrainer`) adds ``dis_l``, the VAE-GAN's
        learned similarity per image, ``0.5 sum((f(recon) - f(x))^2)`` over the discriminator's ``lth_features`` (the
        per-image sum in fp64), averaged over the images; the discriminator stays in training mode whatever
        ``eval_mode`` says, so its two forwards per batch move ITS running statistics.  ``TypeError`` for a trainer
        whose network has no encoder (`GANTrainer`) or, with ``dis_l``, no discriminator."""
        from . import metrics, recon_quality
        net = self._sampling_net(use_ema)
        if not all(hasattr(net, a) for a in ("encode", "decode")):
            raise TypeError(f"{type(self).__name__}: {type(net).__name__} has no encoder, there is nothing to reconstruct")
        netD = getattr(self, "netD", None) if dis_l else None
        if dis_l and netD is None:
            raise TypeError(f"{type(self).__name__} has no discriminator: dis_l needs its features")
        acc, dis = recon_quality.Accumulator(), []
        with torch.no_grad(), _model.eval_mode(*((net,) if eval_mode else ())):
            for batch in loader:
                x = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(self.device)
                if sample:
                    recon = net(x, metrics._randn((x.size(0), net.n_hidden), x.device, generator))[0]
                else:
                    recon = net.decode(net.encode(x)[0])
                acc.update(recon, x)
                if netD is not None:
                    fr, fx = (netD(t)[1].reshape(x.size(0), -1).double() for t in (recon, x))
                    dis.append(0.5 * ((fr - fx) ** 2).sum(1))
        report = acc.result()
        if netD is not None:
            report["dis_l"] = torch.cat(dis).mean()
        return report

    @torch.no_grad()
    def reset_ema(self):
        """Shadow <- the live network as it is now: weights and BatchNorm buffers, copied into the existing tensors."""
        live, _ = self._ema_pair()
        src = live.state_dict()
        for k, v in self.ema_model.state_dict().items():
            v.copy_(src[k])

    @torch.no_grad()
    def _ema_restore(self, ck):
        """After the live network was loaded: the shadow from its checkpoint key -- copied into the existing tensors, a
        captured iteration writes into them -- or, the key absent, from the live network (`reset_ema`)."""
        if self.ema_model is None:
            return
        sd = ck.get(self._ema_names[2])
        if sd is None:
            return self.reset_ema()
        mine = self.ema_model.state_dict()
        if set(mine) != set(sd):
            raise KeyError(f"{self._ema_names[2]}: keys differ from the shadow network's: "
                           f"{sorted(set(mine) ^ set(sd))[:4]}")
        for k, v in mine.items():
            v.copy_(sd[k])

    def _ema_checkpoint(self):
        """The additional checkpoint key -- present only with an average: the shadow's plain state_dict."""
        return {} if self.ema_model is None else {self._ema_names[2]: self.ema_model.state_dict()}

    @torch.no_grad()
    def recalibrate_ema_bn(self, batches, max_batches=None, eps_generator=None):
        """Standing statistics: BatchNorm running statistics that belong to the averaged weights, for eval-mode use of
        `ema_model` (``model.eval_mode(trainer.ema_model)``).  The shadow runs its full forward in train mode over
        ``batches`` (an iterable of input batches, or of ``(batch, ...)`` tuples as a loader yields them: images for a
        VAE shadow, latents for a generator); for batch k every BatchNorm has ``momentum = 1 / k``, so afterwards each
        running statistic is the arithmetic mean of the batch statistics (torch's ``momentum=None``).  The momenta are
        restored afterwards, also after an exception; the live network is not touched.  A VAE shadow draws its latent
        noise from ``eps_generator`` (default: a generator of the shadow's device seeded with 0 -- no training stream is
        consumed).  Returns the number of batches used."""
        self._ema_pair()
        net = self.ema_model
        bns = [m for m in net.modules() if isinstance(m, _model._HipBatchNormMixin)]
        momenta = [m.momentum for m in bns]
        is_vae = isinstance(net, VAE)
        if is_vae and eps_generator is None:
            eps_generator = torch.Generator(device=self.device)
            eps_generator.manual_seed(0)
        was_training = net.training
        k = 0
        try:
            net.train()
            for batch in batches:
                if max_batches is not None and k >= max_batches:
                    break
                x = (batch[0] if isinstance(batch, (tuple, list)) else batch).to(self.device)
                k += 1
                for m in bns:
                    m.momentum = 1.0 / k
                if is_vae:
                    net(x, torch.randn(x.size(0), self.opt.n_hidden, device=self.device, generator=eps_generator))
                else:
                    net(x)
        finally:
            for m, mom in zip(bns, momenta):
                m.momentum = mom
            net.train(was_training)
        return k

    def _host_state_key(self):
        """Host-side switches a capture freezes besides the shapes: part of every capture key, so that flipping one
        captures anew instead of replaying the old launches."""
        from . import model as M
        return (M.FUSE_CONV_BN, M.FUSE_HEAD_BCE, F.DEFER_WGRAD, F.FUSE_LINEAR_ADAM, ops.THIN_SPLIT, ops.USE_PACKED_FILTERS,
                self.nonfinite_guard,        # (checked or unchecked Adam launches)
                self.max_grad_norm, self.skip_nonfinite,      # (the norm pass and the clip step, or neither)
                self.device_hyper,           # (lr, weight decay and beta read from device words, or frozen arguments)
                self._objective_key(),       # (which objective, and its frozen kernel arguments)
                tuple(net.training for net in self._nets()),
                tuple(p.requires_grad for net in self._nets() for p in net.parameters()),
                # (the augmentation's launches: policy and p -- or, ``ada``: p is a device word, and the controller's frozen
                # arguments stand in its place)
                *(() if self._augment is None else (self._augment,) if self._ada is None
                  else (self._augment[:2], ("ada", *self._ada))),
                *(() if self._gan_loss is None else (("gan_loss", self._gan_loss),)))      # (the head's loss kernels)

    def _head(self, netD, feat, role, label, gb):
        """The discriminator's head and its loss on features ``feat`` -> (p, logit, features, loss): the reference's BCE on
        p (``logit`` is None then), or -- ``gan_loss`` -- that loss of the logit in ``role``."""
        if self._gan_loss is None:
            p, f, err = netD.head_with_bce(feat, label, gb)
            return p, None, f, err
        return netD.head_with_loss(feat, self._gan_loss, role, label, gb)

    # ---- one iteration: the path every `step` takes ----------------------------------------------------------------------
    def draw_latents(self, batch):
        """One N(0,1) draw of shape (batch, n_hidden) from this replica's own stream."""
        return torch.randn(batch, self.opt.n_hidden, device=self.device, generator=self.latent_generator)

    def draw_augment(self, batch):
        """One iteration's uniforms of ``diff_augment``, [sets, batch, 8], from this replica's augmentation stream."""
        if self._augment is None:
            raise TypeError(f"{type(self).__name__}: construct with diff_augment=... to draw its uniforms")
        return F.diff_augment_uniforms(batch, self.device, self.augment_generator, sets=self._augment_sets)

    def _drawn(self):
        """The random inputs of one iteration in draw order, each naming its distribution: the latents, N(0,1) of shape
        (batch, n_hidden) from the latent stream, then -- with ``diff_augment`` -- ``augment``, U[0,1) of shape (sets, batch,
        8) from the augmentation stream."""
        drawn = [_Drawn(name, "normal", "latent_generator") for name in self._latents]
        if self._augment is not None:
            drawn.append(_Drawn("augment", "uniform", "augment_generator"))
        if self._owned is not None:      # (``factor_vae``: ``permute``, U[0,1) of shape (batch, n_hidden) from the permutation stream)
            drawn.extend(self._owned.drawn)
        return drawn

    def _draw(self, given, batch, cap=None):
        """The random inputs of one iteration, in `_drawn` order: the caller's, and each one left to the trainer (None) drawn
        from this replica's stream of that input (``noise`` of new_betavaegan.py:111, ``eps`` of model.py:534) -- straight
        into the static buffer of the capture ``cap`` when there is one: same generator, same order, same values."""
        out = []
        for d, t in zip(self._drawn(), given):
            if t is None and cap is None:
                t = self.draw_latents(batch) if d.dist == "normal" else getattr(self, f"draw_{d.name}")(batch)
            elif t is None:
                g = getattr(self, d.generator)
                t = cap.inputs[d.name].normal_(generator=g) if d.dist == "normal" else cap.inputs[d.name].uniform_(generator=g)
            out.append(t)
        return tuple(out)

    def _with_augment(self, given, augment, batch):
        """`step`'s random inputs in `_drawn` order: behind the latents, the caller's ``augment`` (or None: drawn)."""
        if self._augment is None:
            if augment is not None:
                raise TypeError(f"{type(self).__name__}.step: augment= belongs to diff_augment, which is off")
            return given
        shape = (self._augment_sets, batch, ops.AUGMENT_UNIFORMS)
        if augment is not None and (tuple(augment.shape) != shape or augment.dtype != torch.float32
                                    or augment.device.type != self.device.type):
            raise ValueError(f"{type(self).__name__}.step: augment must be a float32 tensor of shape {shape} on {self.device}, "
                             f"got {tuple(augment.shape)} {augment.dtype} on {augment.device}")
        return (*given, augment)

    def draw_permute(self, batch):
        """One iteration's uniforms of ``factor_vae``'s ``permute_dims``, [batch, n_hidden], from this replica's permutation
        stream."""
        if self.gamma is None:
            raise TypeError(f"{type(self).__name__}: construct with factor_vae=... to draw its uniforms")
        return torch.rand(batch, self.opt.n_hidden, device=self.device, generator=self.permute_generator)

    def _with_permute(self, given, permute, batch):
        """`step`'s random inputs in `_drawn` order: behind ``augment``, the caller's ``permute`` (or None: drawn)."""
        if self.gamma is None:
            if permute is not None:
                raise TypeError(f"{type(self).__name__}.step: permute= belongs to factor_vae, which is off")
            return given
        shape = (batch, self.opt.n_hidden)
        if permute is not None and (tuple(permute.shape) != shape or permute.dtype != torch.float32
                                    or permute.device.type != self.device.type):
            raise ValueError(f"{type(self).__name__}.step: permute must be a float32 tensor of shape {shape} on {self.device}, "
                             f"got {tuple(permute.shape)} {permute.dtype} on {permute.device}")
        return (*given, permute)

    def _augmented(self, x, augment, k):
        """``x`` as the discriminator sees it: through parameter set ``k`` of ``augment``, or as it is without the option."""
        if self._augment is None:
            return x
        return F.diff_augment(x, augment[k], self._augment[1], self._augment[2] if self._ada is None else self.augment_p)

    # ---- ``ada``: the controller of the augmentation's p -----------------------------------------
    @property
    def ada(self):
        """``dict(target=, rate=, interval=)`` of the controller (``rate = 1 / (kimg * 1000)``); None when the option is off."""
        return None if self._ada is None else dict(zip(("target", "rate", "interval"), self._ada))

    def ada_report(self):
        """The controller's words as Python numbers (`ops.ada_read`: p, sign_sum, count, calls, rt, adjustments) -- ONE
        host read, a synchronisation: for logging every now and then, not for every step."""
        if self._ada is None:
            raise TypeError(f"{type(self).__name__}: construct with ada=... to read its controller")
        return ops.ada_read(self._ada_state)

    def _ada_update(self, p_real, s_real):
        """The LAST launch of an iteration: the controller on the phase-1 real head's output of this iteration -- the logits
        (threshold 0) under ``gan_loss``, else the probabilities (threshold 0.5).  Every augmentation launch of the
        iteration, forward and backward, ran before it and read the p the previous iteration left.  Returns the two
        outputs it adds: clones of words 0 and 4 taken behind the update ({} without the option)."""
        if self._ada is None:
            return {}
        d, threshold = (p_real, 0.5) if s_real is None else (s_real, 0.0)
        ops.ada_update(d.detach().reshape(-1), self._ada_state, threshold, *self._ada)
        words = self._ada_state.view(torch.float32)
        return dict(augment_p=words[0].clone(), ada_rt=words[4].clone())

    def _ada_checkpoint(self):
        """The additional checkpoint key -- present only with ``ada``: the eight words as a CPU tensor (one host read)."""
        return {} if self._ada is None else {"ada_state": self._ada_state.to("cpu", copy=True)}

    @torch.no_grad()
    def _ada_restore(self, ck):
        """The controller's words from their checkpoint key, copied into the existing buffer -- a captured iteration reads
        and writes it; a checkpoint without the key leaves them as they are."""
        sd = ck.get("ada_state") if self._ada is not None else None
        if sd is None:
            return
        if not isinstance(sd, torch.Tensor) or sd.dtype != torch.int32 or tuple(sd.shape) != (8,):
            raise ValueError("ada_state: the checkpoint's key is not the controller's eight int32 words")
        self._ada_state.copy_(sd)

    def _zero(self, net, flat, opt=None, grad_hook=None, update_ema=True):
        """A phase's zeroing.  ``opt``: the optimizer whose `step` ends the phase -- the big Linear weights the coming
        backward reaches once are registered with it and updated INSIDE the backward (HipAdam.begin_fused_step,
        functional.FUSE_LINEAR_ADAM; ``update_ema`` as that `step` will be called), unless a ``grad_hook`` wants to see
        their gradients or a gradient exchange has to reduce them first.  The `step` closes the registrations."""
        if flat is not None:
            flat.zero_and_attach()
        else:
            _zero_grads(net)
        regs = None
        if isinstance(opt, HipAdam) and F.FUSE_LINEAR_ADAM and grad_hook is None and flat is None:
            only = self._single_use.get((id(net), F.DEFER_WGRAD))
            if only is None:                             # (a walk over the modules: once per network)
                only = self._single_use[(id(net), F.DEFER_WGRAD)] = _model.single_use_linear_weights(net, F.DEFER_WGRAD)
            regs = opt.begin_fused_step(update_ema=update_ema, only=only)
        F.open_fused_linear_steps(regs)

    def _exchange(self, flat):
        if flat is not None and (self.world > 1 or FlatGrads.exchange_when_alone):
            flat.finish()

    @staticmethod
    def _set_frozen(net, frozen):
        """A network that only relays gradients: no weight gradients are formed for it."""
        for p in net.parameters():
            p.requires_grad_(not frozen)

    def _iteration(self, data, latents, labels, grad_hook, prepack, acc):
        """The iteration itself: ``latents`` in `_drawn` order (the uniforms of ``diff_augment`` last), ``labels`` = (real,
        fake, global batch) -- floats, or the device scalars of a capture -- or None without `_has_labels`;
        ``grad_hook(phase, net)`` (tests) is called right before each optimizer step; ``prepack``: see
        `_run_with_pack_plan`; ``acc``: the open `F.accumulate_param_grads`, or None without `_accumulate`.  Counts
        `iteration`; returns the losses as device scalars (no synchronisation)."""
        raise NotImplementedError

    def _eager(self, data, latents, labels, grad_hook=None):
        """`_iteration` launched kernel by kernel -- which is also what a capture records.  Weights change only at the
        optimizer steps: packed filters are reused between them, and all the filters a step has changed are re-packed
        in ONE launch."""
        def body(prepack):
            with (F.accumulate_param_grads() if self._accumulate else nullcontext()) as acc:
                return self._iteration(data, latents, labels, grad_hook, prepack, acc)
        with ops.packed_filter_scope():
            return self._run_with_pack_plan(body, {p.plan: getattr(self, p.net) for p in self._parts})

    def _frozen(self, *values):
        """Learning rates / beta / the objective's own word as part of a capture key: frozen kernel arguments -- unless
        ``device_hyper`` keeps them in device words, where they may change under one capture."""
        return None if self.device_hyper else values

    def _capture_key(self, data, labels):
        """Everything a capture freezes: shapes, the BCE's divisor, learning rates and beta (`_frozen`), the arithmetic,
        the identity of Adam's moment tensors, and the host-side switches."""
        opts = self._optimizers().values()
        return (tuple(data.shape), labels and int(labels[2]),
                self._frozen(getattr(self, "beta", None), *(o.param_groups[0]["lr"] for o in opts),
                             *(() if self._word is None else (self._word,))),
                ops.CONV_ARITH, tuple(o.state_generation for o in opts), self._host_state_key())

    def _drive(self, data, given, real_label=None, fake_label=None, global_batch=None, grad_hook=None, augment=None,
               permute=None):
        """One iteration from `_begin_step` to `_end_step`.  ``given``: the caller's latents in `_latents` order, None
        where the trainer is to draw.  Eager -- or, `_graph_usable`: the first GRAPH_WARM_STEPS iterations of a capture
        key eager (workspaces, packs, GEMM plans exist then), the next one captured and replayed, later ones replayed;
        and eager for good after a failed capture."""
        given = self._with_permute(self._with_augment(given, augment, data.size(0)), permute, data.size(0))
        self._begin_step()
        batch, labels = data.size(0), None
        if self._has_labels:
            # BCE is a mean over the GLOBAL batch (DataParallel gathers the outputs before the loss); equal shards are
            # assumed unless the caller says otherwise (train_epoch passes the loader's count)
            labels = (real_label, fake_label, global_batch if global_batch is not None else batch * self.world)
        if self._graph_usable(data, grad_hook):
            out = self._replayed(data, given, labels)
        else:
            out = self._eager(data, self._draw(given, batch), labels, grad_hook)
        self._end_step()
        return out

    def _replayed(self, data, given, labels):
        """The graph side of `_drive`: warm-up count per capture key, static inputs, capture, replay, fallback."""
        key = self._capture_key(data, labels)
        cap = self._graphs.get(key)
        if cap is None and self._shape_steps.get(key, 0) < GRAPH_WARM_STEPS:
            self._shape_steps[key] = self._shape_steps.get(key, 0) + 1
            return self._eager(data, self._draw(given, data.size(0)), labels)
        latents = self._draw(given, data.size(0), cap)
        names = [d.name for d in self._drawn()]
        inputs = dict(data=data.contiguous(), **dict(zip(names, latents)))
        if cap is None:
            if len(self._graphs) >= 4:               # each capture keeps its own memory pool: bound them
                self._graphs.pop(next(iter(self._graphs)))

            def run(inp, real_dev, fake_dev):        # the iteration on the capture's static tensors
                return self._eager(inp["data"], tuple(inp[n] for n in names),
                                   labels and (real_dev, fake_dev, labels[2]))
            bns = [m for net in self._nets() for m in net.modules() if hasattr(m, "_nbt_pending")]
            it0 = self.iteration
            try:
                cap = _CapturedIteration(self, run, inputs, list(self._optimizers().values()), bns)
            except Exception as e:                   # stay correct: this trainer goes on eagerly
                warnings.warn(f"HIP-graph capture of the training iteration failed ({type(e).__name__}: {e}); "
                              "continuing with eager launches")
                self.iteration = it0
                self.graph = False                   # for good: a capture that fails once is not retried
                return self._eager(data, latents, labels)      # (the latents already drawn: the RNG stream stays an eager run's)
            self._graphs[key] = cap
            self.iteration = it0                     # counted below, once per executed iteration
        real, fake = (float(labels[0]), float(labels[1])) if labels else (0.0, 0.0)
        out = cap.replay(inputs, real, fake)
        self.iteration += 1
        return out


class BetaVAEGANTrainer(_GraphedSteps):
    """One replica of the beta-VAE-GAN (new_betavaegan.py:36-53 construction recipe).

    ``graph`` (default: on for a single-process CUDA trainer, VG_GRAPH=0 turns it off): from the third iteration of a
    batch shape on, `step` replays a HIP graph of the whole iteration (`_CapturedIteration`) instead of launching its
    ~390 kernels one by one.  Iterations that need the host in the loop stay eager: a ``grad_hook``, a `probe`, module
    hooks, launch timing (bench.py's instrumented step).  A data-parallel iteration is captured too when its gradient
    exchange runs on the project's own RCCL communicator (`FlatGrads.capturable`); over torch.distributed's collectives it
    stays eager.

    ``nonfinite_guard`` (default: on whenever the optimizers are HipAdam, VG_NONFINITE_GUARD=0 turns that off): the Adam
    steps flag non-finite gradients / parameters; `check_finite` -- called by `train_epoch` at the end of every epoch,
    and by whoever wants to know after any `step` -- raises `NonFiniteError`.

    ``max_grad_norm`` / ``skip_nonfinite`` (default: off -- then every launch is what it was): every optimizer step clips
    its gradients by their global L2 norm, and / or skips itself when that norm is inf / NaN (optim.HipAdam: one norm pass
    in front of the fused step, nothing on the host, captured with the iteration).  `skipped_steps` counts the skips.  What
    a skip does NOT undo: a forward pass that was non-finite already has written its BatchNorm running statistics.

    Schedules (default: none -- then every launch and every capture key is what it was): ``lr_scheduler``, a callable
    ``optimizer -> torch.optim.lr_scheduler.LRScheduler`` applied to each optimizer (kept in `lr_schedulers` under the
    optimizer's attribute name, stepped once at the end of every `step`); ``beta_schedule``, a callable ``iteration ->
    float`` evaluated with `iteration` at the start of every `step` (-> `beta`); ``weight_decay`` /
    ``decoupled_weight_decay`` as torch.optim.Adam's, inside the fused step.  ``device_hyper`` (default: on exactly when a
    scheduler or a beta schedule is given): lr, weight decay and beta live in device words the captured kernels read, so a
    value that changes every iteration still replays ONE graph.  `set_lr` / `set_beta`: the same by hand.  Data parallel:
    every rank evaluates the same schedule on the same iteration counter; nothing is exchanged.

    ``ema_decay`` (default: none -- then every launch, capture key and checkpoint key is what it was): a float in (0, 1) or
    a callable ``iteration -> decay in [0, 1)`` (`ema_warmup`), evaluated with `iteration` at the start of every `step`.
    `ema_model` is then a shadow of netEG -- a deep copy made once, never replaced -- whose parameters the phase-3 Adam
    step moves, ``e <- e + (1 - decay)(p - e)``, inside its own kernel (the phase-2 step leaves them alone: one average
    per iteration).  The decay lives in a device word, so a value that changes every iteration still replays ONE graph.
    The discriminator is not averaged.  ``fit`` / ``evaluate(use_ema=True)`` sample, reconstruct and score through the
    shadow; `recalibrate_ema_bn` gives it BatchNorm running statistics of its own for eval-mode use; checkpoints carry
    it under ``encoder_decoder_ema``.  Data parallel: every rank forms the same average from the same weights.

    ``tc_decomposition=(alpha, gamma)`` (default: none -- then every launch, loss key, capture key and checkpoint key is
    what it was): phase 3's KL term becomes the beta-TCVAE decomposition by minibatch-weighted sampling (Chen et al.
    2018), ``alpha * mutual information + beta * total correlation + gamma * dimension-wise KL``,
    on one fused kernel pair (`VAE.forward_with_tc`).  The total-correlation weight is the trainer's own `beta`, so
    ``beta_schedule``, `set_beta` and ``device_hyper`` apply unchanged and a beta annealed every iteration still replays
    ONE graph.  ``kld`` of the returned dict is the weighted loss that was backpropagated; ``mi``, ``tc``, ``dwkl`` (each
    summed over the batch) are added to it.  ``dataset_size``: the N of the estimator, the number of training samples;
    `fit` / `train_epoch` take it from ``len(loader.dataset)`` when it was not given, `step` without one raises
    ValueError.  The option adds no checkpoint state.  Data parallel: every rank estimates the three parts from its LOCAL
    batch -- the pair terms never cross ranks -- so the estimator is replica-local, as the BatchNorm statistics are.

    ``dip_vae=(variant, lambda_od, lambda_d)`` (default: none, with the same guarantee): phase 3 keeps the KL term,
    weighted by `beta`, and adds the DIP-VAE penalty on the covariance ``C`` of the aggregate posterior (Kumar et al.
    2018): ``beta * kl + B * (lambda_od * sum_{i != j} C_ij^2 + lambda_d * sum_i (C_ii - 1)^2)``,
    ``variant`` ``"i"`` with the covariance of the means, ``"ii"`` with the mean posterior variance added to its diagonal
    (`VAE.forward_with_dip`; three launches forward, one backward).  The lambdas are finite and >= 0, frozen kernel
    arguments; ``beta_schedule``, `set_beta` and ``device_hyper`` apply unchanged and an annealed beta still replays ONE
    graph.  ``kld`` of the returned dict is the weighted loss that was backpropagated; ``kl``, ``dip_od``, ``dip_d`` are
    added to it.  No checkpoint state; together with ``tc_decomposition`` it is a ValueError.  Data parallel: every rank
    forms the means and the covariance from its LOCAL batch -- replica-local, as the BatchNorm statistics and the
    total-correlation estimate are.

    ``mmd_vae=(kernel, lambda_mmd)`` or ``(kernel, lambda_mmd, bandwidths)`` (default: none, with the same guarantee):
    phase 3 keeps the KL term, weighted by `beta`, and adds the unbiased maximum mean discrepancy between the batch of z
    and as many draws from the prior (InfoVAE, Zhao et al. 2019; WAE-MMD, Tolstikhin et al. 2018; DESIGN.md section
    4.23): ``beta * kl + B * lambda_mmd * mmd`` under a sum of ``"rbf"`` or ``"imq"`` kernels (`VAE.forward_with_mmd`;
    three launches forward, one backward).  ``bandwidths``: 1 to 8 finite positive numbers, default WAE's (``2 D`` for
    rbf, ``2 D (0.1 ... 10)`` for imq).  ``lambda_mmd`` is finite and >= 0; it and the kernel are frozen kernel arguments,
    while ``beta_schedule``, `set_beta` and ``device_hyper`` apply unchanged, an annealed beta still replays ONE graph,
    and ``beta = 0`` (a WAE) is allowed.  The iteration takes one more latent, ``prior``, drawn after ``eps3`` (`step`
    accepts ``prior=``).  ``kld`` of the returned dict is the weighted loss that was backpropagated; ``kl``, ``mmd``,
    ``mmd_kzz`` are added to it.  No checkpoint state; together with ``tc_decomposition`` or ``dip_vae`` it is a
    ValueError.  Data parallel: replica-local, as those are.

    ``kl_control=(capacity, free_bits)`` (default: none, with the same guarantee): phase 3's KL term is held at a capacity
    over per-dimension free bits (Burgess et al. 2018, disentanglement_lib's AnnealedVAE; Kingma et al. 2016; DESIGN.md
    section 4.30): ``beta * |kl_floored - B * capacity|`` with ``kl_floored = sum_d max(K[d], B * free_bits)``, ``K[d]`` the
    dimension's KL summed over the batch (`VAE.forward_with_klc`; two launches forward, one backward); `beta` plays
    Burgess's gamma.  ``capacity`` (nats per sample): a float >= 0, or a callable ``iteration -> float``
    (`linear_capacity`) evaluated with `iteration` at the start of every `step`; `capacity` reads it, `set_capacity` sets it
    by hand, `kl_control` reads the pair.  ``free_bits`` (nats per dimension per sample): a finite float >= 0, a frozen
    kernel argument.  With ``device_hyper`` -- on by default also when the capacity is a callable -- the capacity lives in
    a device word beside beta's, so a capacity annealed every iteration still replays ONE graph; without, it is a frozen
    value of the capture key, as beta is.  ``kld`` of the returned dict is the weighted loss that was backpropagated;
    ``kl``, ``kl_floored`` and ``dims_above`` (the number of dimensions above their floor) are added to it.  A callable
    capacity adds the ``iteration`` checkpoint key, a constant one no key; together with another objective it is a
    ValueError.  Data parallel: the sums are those of this replica's batch -- replica-local, as those are.

    ``diff_augment=policy`` or ``(policy, p)`` (default: none -- then every launch, capture key, latent draw, checkpoint key
    and bit is what it was): every image batch the discriminator sees goes through a random, differentiable transform
    (Zhao et al. 2020; `functional.diff_augment`): ``policy`` is a comma-separated set of
    ``"color"``, ``"translation"``, ``"cutout"``, an image is transformed with probability ``p`` (default 1, the published
    method).  Four parameter sets per iteration, uniforms ``(4, B, 8)``: phase 1 set 0 on ``data`` and set 1 on
    ``fake.detach()``; phase 2 set 2 on ``data`` AND on ``recon`` -- the pair Dis_l compares goes through the same transform
    sample by sample, so the learned similarity still compares like with like -- and set 3 on ``fake``; phase 3 has no
    discriminator, and the pixel MSE terms compare the images themselves.  The uniforms come from `augment_generator`, a
    stream of the trainer's own seeded from (seed, rank), drawn after the iteration's latents -- the latent stream is bit
    for bit what it is without the option -- and straight into a static input of the capture: a fresh draw every iteration
    replays ONE graph.  `step(augment=)` takes them from the caller, `draw_augment` draws a set.  No checkpoint key.  Data
    parallel: replica-local, each rank its own stream, as the latents are.

    ``factor_vae=gamma`` or ``(gamma, dict(width=1000, depth=6, lr=1e-4, betas=(0.5, 0.9)))`` (default: none -- then every
    launch, capture key, checkpoint key, latent draw, initial weight and bit is what it was): FactorVAE (Kim & Mnih 2018,
    disentanglement_lib's form).  The trainer owns one more network, `critic`
    (`model.LatentCritic`: two logits per code, "drawn from q(z)" / "dimensions permuted across the batch"), with its own
    `optimizer_critic`.  Phase 3 minimises ``beta * kl + gamma * sum_b (l0(z_b) - l1(z_b))`` (`VAE.forward_with_factor`); the
    critic only relays gradients there.  A fourth phase, last in the iteration, trains the critic on ``z.detach()`` of that
    same forward and on ``permute_dims(z, u)``: one forward on the 2B rows, the cross-entropy as a mean over 2 x the global
    batch, full backward, exchange, Adam step.  ``gamma``: a float >= 0 or a callable ``iteration -> float``; `gamma` reads
    it, `set_gamma` sets it by hand; with ``device_hyper`` -- on by default also when gamma is a callable -- it lives in a
    device word beside beta's, so an annealed gamma still replays ONE graph.  `beta` stays the trainer's own.  The critic's
    initial weights come from a generator of the trainer's own seeded from ``seed`` (alike on every rank; the global CPU
    stream and the other networks' weights are untouched); its optimizer gets the same guard, clipping and device words as
    the others, its own ``lr`` / ``betas``, and no scheduler, weight decay or EMA (`set_lr` leaves it alone unless named).
    The uniforms ``(B, n_hidden)`` of the permutation come from `permute_generator`, a third stream per replica, drawn last,
    straight into a static input of the capture; `step(permute=)` takes them from the caller, `draw_permute` draws a set; B
    <= 2048.  ``kld`` of the returned dict is the weighted loss; ``kl``, ``tc`` (unweighted), ``critic_loss`` and
    ``critic_acc`` are added.  Checkpoints gain ``latent_critic`` and ``latent_critic_optimizer``; one without them loads
    and leaves a fresh critic.  Together with another objective keyword it is a ValueError.  Data parallel: the critic's
    gradients are exchanged through a `FlatGrads` of its own; the permutation is across this replica's batch.

    ``gan_loss="logistic" | "hinge" | "lsgan"`` (default: none -- then every launch, capture key, draw, checkpoint key and
    bit is what it was): the adversarial terms become that loss of the discriminator's LOGIT instead of nn.BCELoss on
    ``sigmoid(logit)`` (`Discriminator_celeba.head_with_loss`).  The reference's BCE, evaluated in
    fp32 on p, has a gradient of exactly 0 once p rounds to 1 and loses it as p underflows; a loss of the logit cannot.
    ``"logistic"`` is the same objective as the default (BCE-with-logits, soft labels included), ``"lsgan"`` is
    ``(logit - label)^2 / 2``, ``"hinge"`` is ``max(0, 1 - s)`` on real, ``max(0, 1 + s)`` on fake and ``-s`` for the
    generator.  Phase 1 real: role "real" with ``real_label``; phase 1 fake: role "fake" with ``fake_label``; every
    generator-side term (``errG_fake``, ``errG_recon``): role "gen" with ``real_label``; the divisor stays the global
    batch.  Dis_l, the pixel MSE terms and the feature path are untouched.  The labels stay the capture's device words, so
    the per-iteration label flips still replay ONE graph.  The hinge terms IGNORE the labels; `train_epoch` still draws
    them, so every random stream is what it is without the keyword.  The returned dict keeps its keys -- ``D_x_sum`` stays
    the sum of ``sigmoid(logit_real)`` -- and gains ``D_logit_real_sum`` and ``D_logit_fake_sum``, the sums of the phase-1
    logits.  No checkpoint key; data parallel: nothing new (replica-local head, SUM exchange, global divisor).  An
    unknown name is a ValueError.  Composes with every other keyword: none of them touches the head.

    ``ada=True`` or ``dict(target=0.6, kimg=500, interval=4)`` (default: none -- then every launch, capture key, draw,
    checkpoint key and bit is what it was): adaptive discriminator augmentation (Karras et al. 2020, section 3; DESIGN.md
    section 4.35).  It needs ``diff_augment`` (a ValueError without) and takes its probability over: p lives in a device
    word, `augment_p`, that every augmentation kernel reads when it runs, and a controller (`ops.ada_update`, one
    single-workgroup launch) moves it.  Per iteration the controller adds the signs of the phase-1 REAL head's outputs --
    the logits against 0 under ``gan_loss``, else the probabilities against 1/2 -- to two integer words; every ``interval``
    iterations it forms the overfitting heuristic ``r_t = E[sign(D(real))]`` of those iterations and moves p by
    ``(images seen) / (kimg * 1000)`` towards ``r_t == target``, clamped to [0, 1]: ``kimg`` thousand images take p from 0 to
    1.  With the keyword a bare policy string starts at ``p = 0`` (Karras), ``(policy, p0)`` at ``p0``.  The controller is the
    LAST launch of the iteration, behind an owned network's phase: every augmentation launch of iteration t, forward and
    backward, reads the p that iteration t - 1 left, so no backward ever sees another gate than its forward.  It is inside
    the capture, and the capture key carries ``("ada", target, rate, interval)`` in place of p: a p that moves replays ONE
    graph.  The returned dict gains ``augment_p`` and ``ada_rt``, device scalars cloned from the words behind the update
    (``ada_rt`` is 0 before the first adjustment); `ada_report` reads all the words in one host read; `ada` reads the
    arguments.  Checkpoints gain ``ada_state``, the eight words as a CPU tensor; `load` / `load_in_place` copy it into the
    existing buffer, and a checkpoint without it leaves the state as it is.  Data parallel: replica-local, as every other
    option here -- each rank counts the signs of ITS batch and moves ITS word, nothing is exchanged, so the ranks' p may
    drift apart by a few steps.  Composes with ``gan_loss``, ``factor_vae``, the EMA, clipping and the schedules: none of them
    touches the word.  Whether it holds ``D_x`` off 1 on a small set has not been measured here."""

    _parts = (_Part("netEG", VAE, "optimizerEG", "flat_eg", "eg", "encoder_decoder_optimizer"),              # :41, :49
              _Part("netD", Discriminator_celeba, "optimizerD", "flat_d", "d", "discriminator_optimizer"))    # :43, :50
    _latents = ("noise", "eps2", "eps3")
    _has_labels = _accumulate = True
    _augment_sets = 4         # phase 1: data, fake.detach(); phase 2: data and recon (one set), fake
    _ema_names = ("netEG", "optimizerEG", "encoder_decoder_ema")

    def __init__(self, device="cuda", seed=999, beta=25.0, lr=1e-3, opt: Optional[ModelOpt] = None,
                 data_parallel: Optional[bool] = None, fused_adam: bool = True, capturable: Optional[bool] = None,
                 graph: Optional[bool] = None, nonfinite_guard: Optional[bool] = None,
                 max_grad_norm: Optional[float] = None, skip_nonfinite: bool = False,
                 lr_scheduler=None, beta_schedule=None, weight_decay: float = 0.0, decoupled_weight_decay: bool = False,
                 device_hyper: Optional[bool] = None, ema_decay=None, tc_decomposition=None,
                 dataset_size: Optional[int] = None, dip_vae=None, mmd_vae=None, kl_control=None, diff_augment=None,
                 factor_vae=None, gan_loss=None, ada=None):
        self.beta = float(beta)
        self._setup(device, seed, lr, opt, fused_adam, graph, nonfinite_guard, max_grad_norm, skip_nonfinite, lr_scheduler,
                    beta_schedule, weight_decay, decoupled_weight_decay, device_hyper, ema_decay, tc_decomposition,
                    dataset_size, data_parallel, capturable, dip_vae, mmd_vae, kl_control,      # (lr: hard-coded 1e-3 at new_betavaegan.py:49-50)
                    diff_augment, factor_vae, gan_loss, ada)
        self._eg_params = [p for p in self.netEG.parameters() if p.dim() == 4]   # convolution filters
        self._d_params = [p for p in self.netD.parameters() if p.dim() == 4]

    # -- one iteration ------------------------------------------------------------
    def step(self, data, noise=None, eps2=None, eps3=None, real_label=0.9, fake_label=0.1,
             global_batch: Optional[int] = None, grad_hook=None, prior=None, augment=None,
             permute=None) -> Dict[str, torch.Tensor]:
        """One iteration; returns the nine loss scalars as device tensors (no host sync).  From the third iteration of a
        batch shape on the iteration is a HIP-graph replay and the returned tensors are the capture's STATIC outputs: the
        next replay overwrites them -- ``.clone()`` (or ``float()``) what is kept across steps.
        ``prior`` (with ``mmd_vae`` only): phase 3's draws from the prior, (B, n_hidden); None is drawn, after ``eps3``.
        ``augment`` (with ``diff_augment`` only): the iteration's four parameter sets, uniforms (4, B, 8); None is drawn,
        after the latents, from the augmentation stream (`draw_augment`).  ``permute`` (with ``factor_vae`` only): the uniforms
        of ``permute_dims``, (B, n_hidden); None is drawn, last, from the permutation stream (`draw_permute`)."""
        return self._drive(data, self._with_prior((noise, eps2, eps3), prior), real_label, fake_label, global_batch, grad_hook,
                           augment, permute)

    def _iteration(self, data, latents, labels, grad_hook, prepack, acc):
        """data (B,3,64,64) in [-1,1]; noise / eps2 / eps3 (B, n_hidden) ~ N(0,1) (new_betavaegan.py:111, model.py:534);
        the labels are the per-iteration scalars of :89-90."""
        netEG, netD = self.netEG, self.netD
        latents, own = self._split_owned(latents)            # (the inputs of an owned network's phase: behind everything else)
        *latents, aug = latents if self._augment is not None else (*latents, None)      # (the uniforms of diff_augment: last)
        noise, eps2, eps3, *prior = latents                  # (prior: one more draw with an objective that takes it, else nothing)
        seen = self._augmented                               # what the discriminator sees of an image batch
        real_label, fake_label, gb = labels
        prepack()
        out = {}

        # ---- phase 1: discriminator (:95-123)
        self._zero(netD, self.flat_d, self.optimizerD, grad_hook)
        fake = netEG.decode(noise)                           # graph kept for phase 2 (:113)
        if self.probe is not None and fake.requires_grad:    # diagnostics (bench.py `regime`): such an iteration is eager
            fake.register_hook(lambda g: self.probe("grad_wrt_fake", g))
        with F.deferred_wgrad():                             # D runs twice, one backward: big Linear weight gradient once
            # ... and its big Linear layer reads its weight once for both passes, forward and data gradient
            f_real, f_fake = netD.features_grouped([seen(data, aug, 0), seen(fake.detach(), aug, 1)])
            p_real, s_real, _, err_real = self._head(netD, f_real, "real", real_label, gb)
            p_fake, s_fake, _, err_fake = self._head(netD, f_fake, "fake", fake_label, gb)
            _backward([err_real, err_fake])
        self._exchange(self.flat_d)
        if grad_hook:
            grad_hook("D", netD)
        self.optimizerD.step()
        ops.invalidate_packed_filters(self._d_params)
        prepack("d")
        acc.reset()
        out["errD_real"], out["errD_fake"] = err_real.detach(), err_fake.detach()
        out["D_x_sum"] = p_real.detach().sum()
        if s_real is not None:
            out["D_logit_real_sum"], out["D_logit_fake_sum"] = s_real.detach().sum(), s_fake.detach().sum()

        # ---- phase 2: "decoder" -- every EG parameter moves (:127-164)
        self._zero(netEG, self.flat_eg, self.optimizerEG, grad_hook, update_ema=False)      # (phase 2 never averages)
        self._set_frozen(netD, True)
        recon, mu, logvar = netEG(data, eps2)
        # D three times on frozen weights -- on data as under no_grad (D fwd #3: BN statistics still update), on fake and
        # on recon, in that order: the big Linear layer reads its weight once for the three
        # (augmented: data and recon, the pair Dis_l compares, under ONE parameter set -- sample by sample the same transform;
        # the pixel MSE below stays on the images themselves)
        f_data, f_fake, f_rec = netD.features_grouped([seen(data, aug, 2), seen(fake, aug, 3), seen(recon, aug, 2)],
                                                      no_grad=(True, False, False))
        sim_real = f_data.squeeze()
        _, _, _, err_g_fake = self._head(netD, f_fake, "gen", real_label, gb)
        _, _, sim_rec, err_g_rec = self._head(netD, f_rec, "gen", real_label, gb)
        sim = F.sim_loss(sim_rec, sim_real)
        mse2 = F.reconstruction_loss(recon, data)
        _backward([err_g_fake, err_g_rec, sim, mse2])
        self._set_frozen(netD, False)
        self._exchange(self.flat_eg)
        if grad_hook:
            grad_hook("EG2", netEG)
        if self.ema_model is not None:
            self.optimizerEG.step(update_ema=False)          # one average per iteration: phase 3 forms it
        else:
            self.optimizerEG.step()
        ops.invalidate_packed_filters(self._eg_params)
        prepack("eg")
        acc.reset()
        out.update(errG_fake=err_g_fake.detach(), errG_recon=err_g_rec.detach(), sim=sim.detach(),
                   mse_dec=mse2.detach())

        # ---- phase 3: "encoder" -- again every EG parameter moves (:167-193)
        self._zero(netEG, self.flat_eg, self.optimizerEG, grad_hook)
        recon, mu, logvar, kld, parts = self._forward_kl(netEG, data, eps3, *prior)
        mse3 = F.reconstruction_loss(recon, data)
        _backward([kld, mse3])
        self._exchange(self.flat_eg)
        if grad_hook:
            grad_hook("EG3", netEG)
        self.optimizerEG.step()
        ops.invalidate_packed_filters(self._eg_params)
        out.update(kld=kld.detach(), mse_enc=mse3.detach(), **self._kl_part_outputs(parts))
        out.update(self._owned_phase(own, data.size(0), gb, grad_hook))      # (``factor_vae``: the critic's phase; else nothing)
        out.update(self._ada_update(p_real, s_real))          # (``ada``: the controller, the iteration's last launch; else nothing)
        self.iteration += 1
        return out

    # -- one epoch (new_betavaegan.py:77-201) ---------------------------------------------
    def train_epoch(self, loader, label_rng=None, max_iterations=None):
        """``train(epoch)`` of new_betavaegan.py:77-201 over ``for data, _ in loader``: per iteration
        the label draw of :89-90 (`sample_labels`) and one `step`; returns the reference's tuple
        ``(avg_recon_enc_loss, avg_recon_dec_loss, avg_dis_loss, avg_Dx)`` of :196-201.

        The reference's bookkeeping is kept as it is: both
        reconstruction averages accumulate the *encoder-phase* pixel MSE (:188-189 add the same
        ``loss``), ``avg_dis_loss`` and ``avg_Dx`` both accumulate the batch mean of D(x) (:105-107,
        :190), and all four sums -- per-batch sums of squared errors, and per-batch *means* of D(x) --
        are divided by ``len(loader.dataset)``.  The sums live on the device; the host reads them once
        per epoch (the reference synchronises four times per iteration with ``.item()``).
        Under data parallelism the sums are all-reduced once at the end, so every rank returns the
        global-batch values the reference's DataParallel run would log, and the labels come -- unless
        ``label_rng`` is given -- from the trainer's own stream, seeded alike on every rank: one label pair
        per global batch, as in the reference's single process."""
        self._dataset_size_from(loader)
        acc = torch.zeros(2, dtype=torch.float64, device=self.device)     # [sum of mse_enc, sum of mean D(x)]
        n_it = 0
        if label_rng is None and self.world > 1:
            label_rng = self.label_rng                    # every rank the same label pair (see _shared_label_rng)
        for data, _ in loader:
            real_label, fake_label = sample_labels(label_rng)
            gb = _loader_global_batch(loader, data.size(0), self.world)
            out = self.step(data, real_label=real_label, fake_label=fake_label, global_batch=gb)
            acc[0] += out["mse_enc"]
            acc[1] += out["D_x_sum"] / gb
            n_it += 1
            if max_iterations is not None and n_it >= max_iterations:
                break
        if self.world > 1:
            dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        # the epoch's one device -> host read; guarded, it carries the flag words too and raises on a poisoned epoch
        # (`fit` then never checkpoints it)
        mse_sum, dx_sum = self._read_finite(acc) if self.nonfinite_guard else acc.tolist()
        n = len(loader.dataset)
        return mse_sum / n, mse_sum / n, dx_sum / n, dx_sum / n

    # -- the experiment script's ``__main__`` (new_betavaegan.py:211-267) -----------------
    def fit(self, loader, epochs, start_epoch=0, model_path=None, label_rng=None, calc_fid=False, n_samples=1000,
            fid_path_recons=None, fid_path_pretrained=None, get_fid=None, log=None, max_iterations=None, verbose=True,
            fid_on_device=False, fid_inception="", fid_feature_extractor=None, use_ema=False):
        """The training half of the reference's ``__main__`` (new_betavaegan.py:218-246): per epoch ``train(epoch)``
        (`train_epoch`), the checkpoint ``{model_path}/model_{epoch+1}.tar`` (:222-228), optionally
        ``generate_fid_samples`` + ``get_fid`` (:231-235), the printed line (:237-238) and the logger row (:241-246:
        ``log(row)``, e.g. the reference's ``Logger.log``).  ``get_fid`` defaults to this package's
        (`fid.get_fid`; it needs Inception weights on disk, so ``calc_fid`` is off unless asked for).  Under data
        parallelism every rank trains, rank 0 writes.  Returns the rows (with ``Dx`` added).

        ``fid_on_device=True`` (with ``calc_fid``): the epoch's FID is ``fid.get_fid_of_generator(self.netEG.decode, ...)``
        -- the samples go from the decoder to the Inception network as a device tensor, no file is written and
        ``fid_path_recons`` / ``get_fid`` are not used.  The network comes from ``fid_inception`` (as `fid.get_fid`'s
        ``inception``) or ``fid_feature_extractor``, is built once and kept for the whole call.  The default keeps the
        reference's route, including its mismatch: the samples are written as ``.pdf`` while ``get_fid`` looks for
        ``*.jpg`` / ``*.png`` (utils.py:26 vs scoring/fid.py:293), so with the defaults that route finds no image.

        ``use_ema=True`` (a trainer with ``ema_decay``): the FID samples of both routes come from `ema_model`."""
        from . import image_io
        rows = []
        self._dataset_size_from(loader)
        net = self._sampling_net(use_ema)
        fid_extractor = self._fid_extractor(fid_inception, fid_feature_extractor) if calc_fid and fid_on_device else None
        for epoch in range(start_epoch, epochs):
            enc_loss, dec_loss, dis_loss, dx = self.train_epoch(loader, label_rng=label_rng, max_iterations=max_iterations)
            fid = "N/A"
            if self.rank == 0:
                with torch.no_grad():
                    if model_path is not None:
                        self.save(os.path.join(model_path, f"model_{epoch + 1}.tar"), epoch + 1)
                    if calc_fid and fid_on_device:
                        from .fid import get_fid_of_generator
                        fid = get_fid_of_generator(net.decode, n_samples, self.opt.n_hidden, fid_path_pretrained,
                                                   feature_extractor=fid_extractor, device=self.device)
                    elif calc_fid:
                        if get_fid is None:
                            from .fid import get_fid
                        image_io.generate_fid_samples(net.decode, epoch, n_samples, self.opt.n_hidden,
                                                      fid_path_recons, device=self.device)
                        fid = get_fid(fid_path_recons, fid_path_pretrained)
                if verbose:
                    print("====> Epoch: {} Avg Encoder Loss: {:.4f} Avg Decoder Loss: {:.4f} Avg Discriminator Loss: {:.4f} "
                          "FID: {} Dx: {:.4f}".format(epoch, enc_loss, dec_loss, dis_loss, fid, dx), flush=True)
                row = {"Epoch": epoch, "Avg Eec Loss": enc_loss, "Avg Dnc Loss": dec_loss, "Avg Dis Loss": dis_loss,
                       "FID": fid}
                if log is not None:
                    log(row)
                rows.append(dict(row, Dx=dx))
        return rows

    def _fid_extractor(self, inception, feature_extractor):
        """The Inception network of the ``fid_on_device`` route: the caller's, or one built from the weights at
        ``inception``; without either the same loud error as `fid.get_fid`."""
        if feature_extractor is not None:
            return feature_extractor
        from . import fid
        weights = fid._find_inception_weights(inception)
        if weights is None:
            raise RuntimeError(fid._NO_EXTRACTOR)
        from .inception import InceptionFeatureExtractor
        return InceptionFeatureExtractor(weights, device=self.device)

    def _sample_quality(self, net, n_samples, extractor, real_feats, args, fid_path_pretrained=None):
        """``{"sample_quality": report}`` of ``n_samples`` decoded samples against ``real_feats`` and, given the path of
        the reference statistics, ``"FID"`` from the SAME features: `fid.get_fid_of_generator` step by step (the path
        first, one undivided decode, one statistics update), the features kept in between."""
        from . import fid, sample_quality
        res = {}
        if fid_path_pretrained is not None:
            if not os.path.exists(fid_path_pretrained):
                raise RuntimeError("Invalid path: %s" % fid_path_pretrained)
            m2, s2 = fid._handle_path(fid_path_pretrained, extractor, self.device)
        feats = fid.sample_features(net.decode, n_samples, self.opt.n_hidden, extractor, self.device)
        if fid_path_pretrained is not None:
            m1, s1 = fid.ActivationStatistics(feats.shape[1], self.device).update(feats).finalize()
            res["FID"] = fid.calculate_frechet_distance(m1, s1, m2, s2, device=self.device)
        res["sample_quality"] = sample_quality.report(real_feats, feats, **(args or {}))
        return res

    def evaluate(self, load_paths, test_loader=None, start_epoch=0, calc_fid=False, n_samples=1000, fid_path_samples=None,
                 fid_path_pretrained=None, get_fid=None, test_recons=False, test_results_path_recons=None,
                 test_results_path_originals="", test_samples=False, test_results_path_samples=None,
                 fid_on_device=False, fid_inception="", fid_feature_extractor=None, eval_mode=False, use_ema=False,
                 latent_report=None, sample_quality=None, sample_quality_args=None, reconstruction_report=None,
                 reconstruction_args=None):
        """The evaluation half (new_betavaegan.py:248-267): for every checkpoint of ``load_paths`` -- load it, renumber
        its epoch the way the reference does so that files of several checkpoints do not overwrite each other (:252-254),
        then FID samples + score (:256-259), one grid of test reconstructions with ``nrow=1`` (+ the originals, :260-263)
        and five samples named after ``start_epoch`` (:264-267: the reference passes ``start_epoch`` there, so several
        checkpoints write the same file; kept).  Train-mode BatchNorm throughout by default: the reference never calls
        ``.eval()``; ``eval_mode=True`` decodes and reconstructs inside
        ``model.eval_mode(self.netEG)`` instead (running statistics; the network is back in training mode afterwards).
        Returns one dict per checkpoint.  ``fid_on_device`` / ``fid_inception`` /
        ``fid_feature_extractor``: as in `fit` -- the FID straight from the decoder, no sample files.  ``use_ema=True`` (a
        trainer with ``ema_decay``): everything above samples and reconstructs through `ema_model` -- loaded from the
        checkpoint's ``encoder_decoder_ema``, or equal to the live network when the checkpoint has none -- and
        ``eval_mode`` then applies to it (see `recalibrate_ema_bn`).  ``latent_report=loader`` (opt-in): each
        checkpoint's dict also carries, under ``latent``, `latent_report` of that loader (same ``eval_mode`` / ``use_ema``);
        without it no launch, key or file differs.  ``sample_quality=`` real features (an ``.npz`` written by
        `fid.save_features`, an image folder, or a [n, d] device tensor; opt-in): each checkpoint's dict also carries,
        under ``sample_quality``, `sample_quality.report` (precision / recall, density / coverage, KID;
        ``sample_quality_args`` are its keywords) of ``n_samples`` decoded samples against them, through the same network
        as the device FID (``fid_inception`` / ``fid_feature_extractor``) and under the same ``eval_mode`` / ``use_ema``.
        The generated features are computed once: with ``calc_fid`` and ``fid_on_device`` the FID statistics come from
        them too, not from a second decode-and-extract pass.  Without the keyword nothing differs.
        ``reconstruction_report=loader`` (opt-in): each checkpoint's dict also carries, under ``reconstruction``,
        `reconstruction_report` of that loader (PSNR / SSIM / MS-SSIM of its images through encoder and decoder;
        ``reconstruction_args``: its keywords ``sample``, ``dis_l``, ``generator``) under the same ``eval_mode`` /
        ``use_ema``; without it no launch, key or file differs."""
        from . import image_io
        out, tmp_epoch = [], 0
        net = self._sampling_net(use_ema)
        want_sq = sample_quality is not None
        fid_extractor = (self._fid_extractor(fid_inception, fid_feature_extractor)
                         if (calc_fid and fid_on_device) or want_sq else None)
        if want_sq:
            from .fid import path_features
            real_feats = (sample_quality.to(self.device) if isinstance(sample_quality, torch.Tensor)
                          else path_features(sample_quality, fid_extractor, self.device))
        for m in load_paths:
            epoch = self.load(m)
            epoch = epoch if epoch != tmp_epoch and tmp_epoch < epoch else tmp_epoch + 1
            tmp_epoch = epoch
            res = {"path": m, "epoch": epoch, "FID": "N/A"}
            with torch.no_grad(), _model.eval_mode(*((net,) if eval_mode else ())):
                if want_sq:
                    res.update(self._sample_quality(net, n_samples, fid_extractor, real_feats, sample_quality_args,
                                                    fid_path_pretrained if calc_fid and fid_on_device else None))
                if calc_fid and fid_on_device:
                    if not want_sq:                      # (else scored above, from the features the report used)
                        from .fid import get_fid_of_generator
                        res["FID"] = get_fid_of_generator(net.decode, n_samples, self.opt.n_hidden, fid_path_pretrained,
                                                          feature_extractor=fid_extractor, device=self.device)
                elif calc_fid:
                    if get_fid is None:
                        from .fid import get_fid
                    image_io.generate_fid_samples(net.decode, epoch, n_samples, self.opt.n_hidden, fid_path_samples,
                                                  device=self.device)
                    res["FID"] = get_fid(fid_path_samples, fid_path_pretrained)
                if test_recons:
                    image_io.gen_reconstructions(lambda x: net(x.to(self.device))[0], test_loader, epoch,
                                                 test_results_path_recons, nrow=1,
                                                 path_for_originals=test_results_path_originals, device=self.device)
                if test_samples:
                    image_io.generate_samples(net.decode, start_epoch, 5, self.opt.n_hidden,
                                              test_results_path_samples, nrow=1, device=self.device)
            if latent_report is not None:
                res["latent"] = self.latent_report(latent_report, eval_mode=eval_mode, use_ema=use_ema)
            if reconstruction_report is not None:
                res["reconstruction"] = self.reconstruction_report(reconstruction_report, eval_mode=eval_mode,
                                                                   use_ema=use_ema, **(reconstruction_args or {}))
            out.append(res)
        return out

    # -- checkpoint (new_betavaegan.py:203-209, 222-228) --------------------------------
    def checkpoint(self, epoch):
        """The reference's dict.  ``discriminator_model`` keys carry the ``module.`` prefix
        because the reference saves the DataParallel-wrapped netD (:44, :225)."""
        return {
            "epoch": epoch,
            "encoder_decoder_model": self.netEG.state_dict(),
            "discriminator_model": {"module." + k: v for k, v in self.netD.state_dict().items()},
            "encoder_decoder_optimizer": self.optimizerEG.state_dict(),
            "discriminator_optimizer": self.optimizerD.state_dict(),
            **self._schedule_checkpoint(),       # (additional keys, only when a schedule exists)
            **self._ema_checkpoint(),            # (encoder_decoder_ema, only with an average)
            **self._owned_checkpoint(),          # (latent_critic, latent_critic_optimizer: only with factor_vae)
            **self._ada_checkpoint(),            # (ada_state: only with ada)
        }

    def save(self, path, epoch, legacy_format=False):
        """torch.save of the reference's dict (new_betavaegan.py:222-228).  ``legacy_format=True``
        writes the pre-1.6 (non-zip) pickle that the reference's pinned torch 1.3.1 can read."""
        torch.save(self.checkpoint(epoch), path, _use_new_zipfile_serialization=not legacy_format)

    def load(self, path_or_dict):
        ck = path_or_dict if isinstance(path_or_dict, dict) else torch.load(path_or_dict, map_location=self.device)
        self.netEG.load_state_dict(ck["encoder_decoder_model"])
        d_sd = ck["discriminator_model"]
        if all(k.startswith("module.") for k in d_sd):       # both layouts accepted
            d_sd = {k[len("module."):]: v for k, v in d_sd.items()}
        self.netD.load_state_dict(d_sd)
        self.optimizerEG.load_state_dict(ck["encoder_decoder_optimizer"])
        self.optimizerD.load_state_dict(ck["discriminator_optimizer"])
        self._schedule_restore(ck)
        self._ema_restore(ck)
        self._owned_restore(ck)
        self._ada_restore(ck)
        self.clear_nonfinite()                               # a good checkpoint is the way back from a NonFiniteError
        return ck["epoch"]

    @torch.no_grad()
    def load_in_place(self, ck):
        """`load` of a checkpoint dict of THIS trainer's shapes that copies into the existing parameter, buffer and moment
        tensors: a captured iteration stays valid and the next `step` replays it from the loaded state (bench.py times
        from the initial state this way).  The packs a replay does not rewrite itself are rewritten here: into the very
        buffers the graph reads, because `ops` allocates the pack buffer of a weight object once and never replaces it."""
        d_sd = ck["discriminator_model"]
        if all(k.startswith("module.") for k in d_sd):
            d_sd = {k[len("module."):]: v for k, v in d_sd.items()}
        for net, sd in ((self.netEG, ck["encoder_decoder_model"]), (self.netD, d_sd)):
            for k, v in net.state_dict().items():            # (flushes the lazily counted num_batches_tracked)
                v.copy_(sd[k])
        if isinstance(self.optimizerEG, HipAdam) and isinstance(self.optimizerD, HipAdam):
            self.optimizerEG.load_state_in_place(ck["encoder_decoder_optimizer"])
            self.optimizerD.load_state_in_place(ck["discriminator_optimizer"])
        else:
            self.optimizerEG.load_state_dict(ck["encoder_decoder_optimizer"])
            self.optimizerD.load_state_dict(ck["discriminator_optimizer"])
        ops.invalidate_packed_filters()
        if self._pack_plans is not None:
            with ops.packed_filter_scope():
                ops.prepack_filters([r for v in self._pack_plans.values() for r in v])
        for opt in (self.optimizerEG, self.optimizerD):      # (the bounds the captured GEMMs read beside the weights)
            if isinstance(opt, HipAdam):
                opt.refresh_weight_bounds()
        self._schedule_restore(ck, in_place=True)
        self._ema_restore(ck)
        self._owned_restore(ck, in_place=True)
        self._ada_restore(ck)
        self.clear_nonfinite()
        return ck["epoch"]


class VAETrainer(_GraphedSteps):
    """new_vae.py:33-37 construction, :39-48 loss, :53-59 step.  ``graph``, ``max_grad_norm``, ``skip_nonfinite``, and the
    schedule arguments (``lr_scheduler``, ``beta_schedule``, ``weight_decay``, ``decoupled_weight_decay``,
    ``device_hyper``): as BetaVAEGANTrainer.  ``ema_decay``: as there, of the one network -- `ema_model` shadows `model`,
    the checkpoint key is ``VAE_model_ema``.  ``tc_decomposition`` / ``dataset_size``: as there, of the step's KL term
    (`train_epoch` fills a ``dataset_size`` that was not given); replica-local under data parallelism.  ``dip_vae``: as
    there -- the covariance is that of this replica's batch.  ``mmd_vae``: as there -- ``prior`` is drawn after ``eps``.
    ``kl_control``: as there -- the per-dimension sums are those of this replica's batch.  ``factor_vae``: as there -- the
    critic's phase follows the one optimizer step, ``permute`` is drawn last, and the cross-entropy's divisor is 2 x (this
    replica's batch x the world size).  There is no discriminator, so a ``diff_augment``, a ``gan_loss`` or an ``ada`` is a
    TypeError."""

    _parts = (_Part("model", VAE, "optimizer", "flat", "vae", "optimizer"),)
    _latents = ("eps",)
    _ema_names = ("model", "optimizer", "VAE_model_ema")

    def __init__(self, device="cuda", seed=999, beta=1.0, lr=3e-3, opt: Optional[ModelOpt] = None,
                 fused_adam: bool = True, capturable: Optional[bool] = None, graph: Optional[bool] = None,
                 nonfinite_guard: Optional[bool] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, lr_scheduler=None, beta_schedule=None, weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False, device_hyper: Optional[bool] = None, ema_decay=None,
                 tc_decomposition=None, dataset_size: Optional[int] = None, dip_vae=None, mmd_vae=None, kl_control=None,
                 diff_augment=None, factor_vae=None, gan_loss=None, ada=None):
        self.beta = float(beta)
        self._setup(device, seed, lr, opt, fused_adam, graph, nonfinite_guard, max_grad_norm, skip_nonfinite, lr_scheduler,
                    beta_schedule, weight_decay, decoupled_weight_decay, device_hyper, ema_decay, tc_decomposition,
                    dataset_size, capturable=capturable, dip_vae=dip_vae, mmd_vae=mmd_vae, kl_control=kl_control,
                    diff_augment=diff_augment, factor_vae=factor_vae, gan_loss=gan_loss, ada=ada)

    def step(self, data, eps=None, grad_hook=None, prior=None, permute=None):
        """``grad_hook(phase, net)`` (tests): called with ``("VAE", model)`` right before the optimizer step -- and, with
        ``factor_vae``, with ``("critic", critic)`` right before the critic's; such an iteration is eager, as
        BetaVAEGANTrainer's.  ``prior`` (with ``mmd_vae`` only): the draws from the prior, (B, n_hidden); None is drawn,
        after ``eps``.  ``permute`` (with ``factor_vae`` only): the uniforms of ``permute_dims``, (B, n_hidden); None is
        drawn, last, from the permutation stream."""
        return self._drive(data, self._with_prior((eps,), prior), grad_hook=grad_hook, permute=permute)

    def _iteration(self, data, latents, labels, grad_hook, prepack, acc):
        latents, own = self._split_owned(latents)      # (the inputs of an owned network's phase: behind everything else)
        eps, *prior = latents                 # (prior: one more draw with an objective that takes it, else nothing)
        prepack()                             # the filters the previous optimizer step changed: one pack launch
        self._zero(self.model, self.flat, self.optimizer, grad_hook)
        recon, mu, logvar, kld, parts = self._forward_kl(self.model, data, eps, *prior)
        mse = F.reconstruction_loss(recon, data)
        _backward([mse, kld])
        self._exchange(self.flat)
        if grad_hook:
            grad_hook("VAE", self.model)
        self.optimizer.step()
        out = dict(mse=mse.detach(), kld=kld.detach(), **self._kl_part_outputs(parts))
        out.update(self._owned_phase(own, data.size(0), None, grad_hook))      # (``factor_vae``: the critic's phase; else nothing)
        self.iteration += 1
        return out

    def train_epoch(self, loader, max_iterations=None):
        """``train(epoch)`` of new_vae.py:48-68: returns ``avg_loss`` = sum over the epoch of
        (MSE + KLD) / len(dataset); one device -> host read per epoch."""
        self._dataset_size_from(loader)
        acc = torch.zeros((), dtype=torch.float64, device=self.device)
        n_it = 0
        for data, _ in loader:
            out = self.step(data)
            acc += out["mse"] + out["kld"]
            n_it += 1
            if max_iterations is not None and n_it >= max_iterations:
                break
        if self.world > 1:
            dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        total, = self._read_finite(acc) if self.nonfinite_guard else [acc.item()]      # (one read, flag words included)
        return float(total) / len(loader.dataset)

    def checkpoint(self, epoch):
        return {"epoch": epoch, "VAE_model": self.model.state_dict(), "optimizer": self.optimizer.state_dict(),
                **self._schedule_checkpoint(), **self._ema_checkpoint(), **self._owned_checkpoint()}


class GANTrainer(_GraphedSteps):
    """new_gan.py:47-61 construction, :66-141 step.  Data parallel like the beta-VAE-GAN driver (the
    reference wraps both nets in nn.DataParallel, new_gan.py:51-53): replica-local BatchNorm, one
    gradient exchange (SUM) per optimizer step, BCE divided by the global batch.  ``graph``: as
    BetaVAEGANTrainer; so are ``max_grad_norm``, ``skip_nonfinite`` and the schedule arguments (``lr_scheduler``,
    ``weight_decay``, ``decoupled_weight_decay``, ``device_hyper``; there is no KL term, so a ``beta_schedule``, a
    ``tc_decomposition``, a ``dip_vae``, an ``mmd_vae``, a ``kl_control`` or a ``factor_vae`` is a TypeError).  ``ema_decay``: as BetaVAEGANTrainer, of the generator -- `ema_model` shadows `netG`, the checkpoint key is
    ``netG_ema``; the discriminator is not averaged.  ``diff_augment``: as BetaVAEGANTrainer, with three parameter sets,
    uniforms ``(3, B, 8)``: set 0 on ``data`` and set 1 on ``fake.detach()`` in the discriminator phase, set 2 on ``fake`` in
    the generator phase.  ``gan_loss``: as BetaVAEGANTrainer -- roles "real" and "fake" in the discriminator phase, "gen"
    with ``real_label`` for ``errG``; the dict gains ``D_logit_real_sum`` and ``D_logit_fake_sum``.  ``ada``: as
    BetaVAEGANTrainer -- the controller reads the discriminator phase's real head and is the iteration's last launch, behind
    the generator's optimizer step; replica-local under data parallelism; the checkpoint gains ``ada_state``, and `load`
    restores it with everything else `checkpoint` wrote (there is no `load_in_place` here)."""

    _parts = (_Part("netG", Generator_celeba, "optimizerG", "flat_g", "g", "G_trainer"),
              _Part("netD", Discriminator_celeba, "optimizerD", "flat_d", "d", "D_trainer"))
    _latents = ("noise",)
    _has_labels = _accumulate = True              # (D runs twice before its backward, as BetaVAEGANTrainer's)
    _augment_sets = 3         # D phase: data, fake.detach(); G phase: fake
    _ema_names = ("netG", "optimizerG", "netG_ema")

    def __init__(self, device="cuda", seed=999, lr=3e-3, opt: Optional[ModelOpt] = None, fused_adam: bool = True,
                 data_parallel: Optional[bool] = None, graph: Optional[bool] = None,
                 nonfinite_guard: Optional[bool] = None, max_grad_norm: Optional[float] = None,
                 skip_nonfinite: bool = False, lr_scheduler=None, beta_schedule=None, weight_decay: float = 0.0,
                 decoupled_weight_decay: bool = False, device_hyper: Optional[bool] = None, ema_decay=None,
                 tc_decomposition=None, dataset_size: Optional[int] = None, dip_vae=None, mmd_vae=None, kl_control=None,
                 diff_augment=None, factor_vae=None, gan_loss=None, ada=None):
        self._setup(device, seed, lr, opt, fused_adam, graph, nonfinite_guard, max_grad_norm, skip_nonfinite, lr_scheduler,
                    beta_schedule, weight_decay, decoupled_weight_decay, device_hyper, ema_decay, tc_decomposition,
                    dataset_size, data_parallel, dip_vae=dip_vae, mmd_vae=mmd_vae, kl_control=kl_control,
                    diff_augment=diff_augment, factor_vae=factor_vae, gan_loss=gan_loss, ada=ada)

    def step(self, data, noise=None, real_label=0.9, fake_label=0.1, global_batch: Optional[int] = None,
             grad_hook=None, augment=None):
        """``augment`` (with ``diff_augment`` only): the iteration's three parameter sets, uniforms (3, B, 8); None is drawn."""
        return self._drive(data, (noise,), real_label, fake_label, global_batch, grad_hook, augment)

    def _iteration(self, data, latents, labels, grad_hook, prepack, acc):
        noise, *aug = latents                 # (aug: the uniforms of diff_augment, else nothing)
        aug, seen = (aug[0] if aug else None), self._augmented
        real_label, fake_label, gb = labels
        prepack()
        self._zero(self.netD, self.flat_d, self.optimizerD, grad_hook)
        fake = self.netG(noise)
        with F.deferred_wgrad():                             # as BetaVAEGANTrainer's discriminator phase
            f_real, f_fake = self.netD.features_grouped([seen(data, aug, 0), seen(fake.detach(), aug, 1)])
            p_real, s_real, _, err_real = self._head(self.netD, f_real, "real", real_label, gb)
            p_fake, s_fake, _, err_fake = self._head(self.netD, f_fake, "fake", fake_label, gb)
            _backward([err_real, err_fake])
        self._exchange(self.flat_d)
        if grad_hook:
            grad_hook("D", self.netD)
        self.optimizerD.step()
        ops.invalidate_packed_filters([p for p in self.netD.parameters() if p.dim() == 4])
        prepack("d")
        acc.reset()
        self._zero(self.netG, self.flat_g, self.optimizerG, grad_hook)
        self._set_frozen(self.netD, True)
        if self._gan_loss is None:
            _, _, err_g = self.netD.forward_with_bce(seen(fake, aug, 2), real_label, gb)
        else:
            _, _, _, err_g = self.netD.forward_with_loss(seen(fake, aug, 2), self._gan_loss, "gen", real_label, gb)
        _backward([err_g])
        self._set_frozen(self.netD, False)
        self._exchange(self.flat_g)
        if grad_hook:
            grad_hook("G", self.netG)
        self.optimizerG.step()
        self.iteration += 1
        out = dict(errD_real=err_real.detach(), errD_fake=err_fake.detach(), errG=err_g.detach(),
                   D_x_sum=p_real.detach().sum())
        if s_real is not None:
            out.update(D_logit_real_sum=s_real.detach().sum(), D_logit_fake_sum=s_fake.detach().sum())
        out.update(self._ada_update(p_real, s_real))          # (``ada``: the controller, the iteration's last launch; else nothing)
        return out

    def train_epoch(self, loader, label_rng=None, max_iterations=None):
        """``train()`` of new_gan.py:66-141: label draw per iteration (:68-69), returns the reference's
        ``(avg_loss_G, avg_loss_D)`` -- including its bookkeeping: ``avg_loss_G`` is the sum of the
        per-batch generator losses over ``len(dataset)``, and the second value is *that average* divided
        by ``len(dataset)`` once more (new_gan.py:138 reads ``avg_loss_G`` where ``avg_loss_D`` was
        meant).  The sum of errD over the epoch is available as ``self.last_epoch_sums["errD"]``."""
        acc = torch.zeros(2, dtype=torch.float64, device=self.device)
        n_it = 0
        if label_rng is None and self.world > 1:
            label_rng = self.label_rng                    # as BetaVAEGANTrainer.train_epoch
        for data, _ in loader:
            real_label, fake_label = sample_labels(label_rng)
            gb = _loader_global_batch(loader, data.size(0), self.world)
            out = self.step(data, real_label=real_label, fake_label=fake_label, global_batch=gb)
            acc[0] += out["errG"]
            acc[1] += out["errD_real"] + out["errD_fake"]
            n_it += 1
            if max_iterations is not None and n_it >= max_iterations:
                break
        if self.world > 1:                       # local BCE terms are already divided by the global batch
            dist.all_reduce(acc, op=dist.ReduceOp.SUM)
        g_sum, d_sum = self._read_finite(acc) if self.nonfinite_guard else acc.tolist()     # (one read, flag words included)
        n = len(loader.dataset)
        self.last_epoch_sums = {"errG": g_sum, "errD": d_sum}
        avg_loss_g = g_sum / n
        return avg_loss_g, avg_loss_g / n

    def checkpoint(self, epoch):
        return {"epoch": epoch, "netG": self.netG.state_dict(), "netD": self.netD.state_dict(),
                "G_trainer": self.optimizerG.state_dict(), "D_trainer": self.optimizerD.state_dict(),
                **self._schedule_checkpoint(), **self._ema_checkpoint(), **self._ada_checkpoint()}

    def load(self, path_or_dict):
        """The way back from `checkpoint`: both networks, both optimizers, and what the options added -- the schedules, the
        averaged generator, the controller's words of ``ada`` (copied into the existing buffer; a checkpoint without the
        key keeps the current state).  Returns the epoch."""
        ck = path_or_dict if isinstance(path_or_dict, dict) else torch.load(path_or_dict, map_location=self.device)
        self.netG.load_state_dict(ck["netG"])
        self.netD.load_state_dict(ck["netD"])
        self.optimizerG.load_state_dict(ck["G_trainer"])
        self.optimizerD.load_state_dict(ck["D_trainer"])
        self._schedule_restore(ck)
        self._ema_restore(ck)
        self._ada_restore(ck)
        self.clear_nonfinite()
        return ck["epoch"]
