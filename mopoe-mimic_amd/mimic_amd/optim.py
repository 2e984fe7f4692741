"""The optimiser of the train step (reference: optim.Adam built by mimic/utils/experiment.py:171-178, stepped by
mimic/run_epochs.py:131) on one HIP kernel family (csrc/adam.hip) instead of PyTorch's multi-tensor kernel.

Same interface as torch.optim.Adam for what the hot path and its callers use: param_groups (a ReduceLROnPlateau scheduler
fills the device-resident learning rate in place), state[p] = {step, exp_avg, exp_avg_sq}, state_dict / load_state_dict,
zero_grad, step.  The two moments of all tensors live in one allocation; the step counter is one device scalar shared
by all tensors (optim.Adam keeps one per tensor, all equal), so the whole step is capturable in a hipGraph.

ASSUMPTION (documented difference from torch.optim.Adam): every parameter handed to the optimiser receives a gradient
on every step it takes part in.  optim.Adam advances a tensor's own step only when it has a gradient, so a parameter whose
gradient is None on SOME steps (a modality missing from some batches) would get a different bias correction there; here a
tensor without a gradient is skipped (its moments stay) but the shared counter advances.  On the hot path the set of
gradient-less parameters is fixed for a run (the word encoder's unused resblock_7/8): those are never updated by either
optimiser, and `check_uniform_grads` raises the first time a parameter's has-gradient state CHANGES between steps.
early_begin() advances the counter before the backward: a backward that raises leaves the counter one ahead with no
update applied (the run is over at that point: OOM -> new process, main_mimic.Main).

max_grad_norm > 0 (--max_grad_norm): step() clips the GLOBAL gradient norm in front of the update, with the semantics of
torch.nn.utils.clip_grad_norm_(params, max_grad_norm, norm_type=2): total_norm = sqrt(sum of g^2) over every parameter that
has a gradient, scale = min(1, max_grad_norm / (total_norm + 1e-6)), the update uses scale * g.  Norm, scale and update are
device work on fixed buffers (ops.grad_norm, ops.adam_step(clip=...)): capturable, deterministic, and behind a gradient
all-reduce the norm is that of the reduced gradients, the same on every rank.  Two deliberate differences from torch:
  1. p.grad is NOT rewritten: the scale is applied where the Adam kernel loads the gradient (one read and one write of all
     gradients saved per step).  clip_state[0], the `grad_norm` the train loop reports, is the norm BEFORE clipping, as
     torch's return value is.
  2. a total_norm that is not finite SKIPS the update on the device: no parameter, moment, bf16 weight copy or step counter
     changes, and clip_state[3] (skipped steps) goes up by one.  torch would multiply every gradient by NaN.
The global norm needs every gradient, so the per-network early updates (early_begin / early_step) are not available while
clipping: run_epochs.train_step does not arm them, and early_begin() raises.

ema_decay > 0 (--ema_decay): an exponential moving average of every parameter, one flat fp32 allocation at the moments'
offsets, initialised from the parameters when the optimiser is built (a caller that loads weights into the model AFTER that
must call reset_ema() itself: nothing here does it for it, and the average would silently go on from the old weights).  _launch() enqueues
ops.ema_update right behind each ops.adam_step, on the same stream and over the same tensors (those that have a gradient),
so one hook serves the eager step, the captured one, the per-network early updates (a network's average is updated on that
network's lane), the clipped step (a skipped step does not move the average: the kernel reads clip_state) and the
data-parallel optimiser graph.  The decay warms up on the device from the shared step counter:
d = min(ema_decay, (1 + step) / (10 + step)).  A parameter that never receives a gradient keeps an average equal to itself.
swap_ema() exchanges parameters and averages IN PLACE (a captured step has the parameter addresses in its nodes), rewrites
the bf16 weight copies of self.lowp from the values swapped in, and flips a host flag; while it is set, step(),
early_begin() and early_step() raise: training on swapped-in weights would corrupt both sets.  BatchNorm buffers are not
averaged, and the average is not part of state_dict() (a resumed run starts a new average from the loaded weights)."""
from __future__ import annotations

import torch

from . import ops


class HipAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=0.0, ema_decay=0.0):
        params = [p for p in params]
        max_grad_norm = float(max_grad_norm)
        ema_decay = float(ema_decay)
        if not (0.0 <= ema_decay < 1.0):
            raise ValueError(f"HipAdam: ema_decay must be finite and in [0, 1) (0 = no average), got {ema_decay}")
        if not (0.0 <= max_grad_norm < float("inf")):
            raise ValueError(f"HipAdam: max_grad_norm must be finite and >= 0 (0 = no clipping), got {max_grad_norm}")
        if not params or not all(p.dtype == torch.float32 for p in params):
            raise ValueError("HipAdam needs fp32 parameters (on the GPU: ops.adam_step has no CPU fallback)")
        dev = params[0].device
        if not isinstance(lr, torch.Tensor):
            lr = torch.tensor(float(lr), dtype=torch.float32, device=dev)
        # (capturable / fused: what run_epochs._StepRunner asks an optimiser before it captures the step)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, capturable=True, fused=True))
        if len(self.param_groups) != 1:
            raise ValueError("HipAdam: one parameter group")
        self._params = list(self.param_groups[0]["params"])
        offs, total = [], 0
        for p in self._params:
            offs.append(total)
            total += (p.numel() + 3) // 4 * 4          # 16-byte aligned pieces
        self._moments = torch.zeros(2, max(total, 4), dtype=torch.float32, device=dev)
        self._step = torch.zeros((), dtype=torch.float32, device=dev)
        self._coef = torch.zeros(2, dtype=torch.float32, device=dev)
        self._m = [self._moments[0, o:o + p.numel()] for o, p in zip(offs, self._params)]
        self._v = [self._moments[1, o:o + p.numel()] for o, p in zip(offs, self._params)]
        self.lowp = None       # optional: per-parameter bf16 copies rewritten by the same kernel (list aligned with params)
        self._index = {id(p): i for i, p in enumerate(self._params)}
        self._had_grad = None  # per-parameter has-gradient pattern of the first eager step (check_uniform_grads)
        self._early = None     # indices already updated in the current step (early_begin / early_step)
        self._held = None      # an in-line network's update waiting for the next in-line network
        for p, m, v in zip(self._params, self._m, self._v):
            self.state[p] = dict(step=self._step, exp_avg=m.view_as(p), exp_avg_sq=v.view_as(p))
        # gradient-norm clip: state {norm, scale, skip, skipped steps} and the partial sums, allocated once (a capture
        # bakes their addresses into its nodes); None = no clipping, and step() is exactly the unclipped one
        self.max_grad_norm = max_grad_norm
        self.clip_state = self._clip_scratch = None
        if max_grad_norm > 0:
            self.clip_state = torch.zeros(ops.CLIP_STATE_LEN, dtype=torch.float32, device=dev)
            n_partials = ops.grad_norm_partials([p.numel() for p in self._params])
            self._clip_scratch = torch.zeros(max(n_partials, 1), dtype=torch.float64, device=dev)
        # weight average: one flat allocation at the moments' offsets (a capture bakes its addresses into its nodes); None =
        # no average, and no launch of step() differs from today's
        self.ema_decay = ema_decay
        self._ema_flat = self._ema = None
        self._swapped = False   # swap_ema(): the parameters hold the average, the average holds the live weights
        if ema_decay > 0:
            self._ema_flat = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
            self._ema = [self._ema_flat[o:o + p.numel()] for o, p in zip(offs, self._params)]
            self.reset_ema()

    def _launch(self, idx, grads, prep):
        group = self.param_groups[0]
        b1, b2 = group["betas"]
        pick = lambda xs: [xs[i] for i in idx]
        ops.adam_step(pick(self._params), grads, pick(self._m), pick(self._v), self._step, group["lr"], b1, b2, group["eps"],
                      self._coef, lowp=None if self.lowp is None else pick(self.lowp), prep=prep,
                      **({} if self.clip_state is None else {"clip": self.clip_state}))
        if self._ema is not None:
            # right behind the Adam launch that wrote these tensors, on its stream; the step counter is the incremented one
            live = [i for i, g in zip(idx, grads) if g is not None]
            if live:
                ops.ema_update([self._params[i] for i in live], [self._ema[i] for i in live], self.ema_decay, self._step,
                               clip=self.clip_state)

    # ---- the weight average (ema_decay > 0) -------------------------------------------------------------------------
    def _need_ema(self, what):
        if self._ema is None:
            raise RuntimeError(f"HipAdam.{what}: no weight average is kept (ema_decay is 0)")

    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f"HipAdam.{what}: the averaged weights are swapped in (swap_ema()); training on them would "
                               "corrupt both the live weights and the average -- swap back first")

    @torch.no_grad()
    def reset_ema(self):
        """average = parameters.  Called at construction.  Nothing in the package loads weights into the model after the
        optimiser is built; code that does (a resume path) MUST call this afterwards itself, or the average goes on from the
        weights the optimiser was built on -- no launch can notice that."""
        self._need_ema("reset_ema")
        self._not_swapped("reset_ema")
        for e, p in zip(self._ema, self._params):
            e.copy_(p.detach().reshape(-1))

    def ema_tensors(self):
        """views of the average shaped like the parameters, in their order (while swapped: the live weights)"""
        self._need_ema("ema_tensors")
        return [e.view_as(p) for e, p in zip(self._ema, self._params)]

    @property
    def ema_swapped(self) -> bool:
        return self._swapped

    @torch.no_grad()
    def swap_ema(self):
        """exchange every parameter with its average in place (current stream), the bf16 weight copies rewritten from the
        values swapped in (layout.Bf16Weights under synced_by_optimizer only watches the tensors' version counters, which a
        library launch does not move); layout.note_params_changed() makes eval-mode copies (the padded vocabulary head)
        refresh.  A second call restores every bit."""
        from .layout import note_params_changed
        self._need_ema("swap_ema")
        ops.ema_swap(self._params, self._ema, lowp=self.lowp)
        note_params_changed()
        self._swapped = not self._swapped

    def check_uniform_grads(self):
        """eager steps only (host-side, no device work): the has-gradient pattern must not change between steps (see the
        module docstring); the captured step cannot change it by construction"""
        pattern = [p.grad is not None for p in self._params]
        if self._had_grad is None:
            self._had_grad = pattern
        elif pattern != self._had_grad:
            i = next(k for k, (a, b) in enumerate(zip(pattern, self._had_grad)) if a != b)
            raise RuntimeError(f"HipAdam: parameter #{i} {'gained' if pattern[i] else 'lost'} its gradient between steps; the "
                               "shared step counter would give it a different bias correction than torch.optim.Adam "
                               "(use MOPOE_TORCH_ADAM=1 for runs whose set of trained parameters varies)")

    @torch.no_grad()
    def early_begin(self):
        """a step in parts: advance the step counter now (current stream); early_step() then updates tensors whose gradients
        are final while the rest of the backward still runs, step() the remaining ones"""
        self._not_swapped("early_begin")
        if self.clip_state is not None:
            raise RuntimeError("HipAdam: early per-network updates cannot be combined with max_grad_norm (the global norm "
                               "needs every gradient)")
        self._launch([], [], True)
        self._early, self._held = set(), None

    @torch.no_grad()
    def early_step(self, params, grads, inline=False):
        """inline: the network ran on the caller's stream, where the next phase of the backward is waiting behind it (the
        text decoder in front of the latent node): its update is held back until the next in-line network is done (the
        text encoder, behind which the caller's stream only waits for the other lanes) or until step()."""
        self._not_swapped("early_step")
        idx, gs = [], []
        for p, g in zip(params, grads):
            i = self._index.get(id(p))
            if i is None or g is None or i in self._early:
                continue
            idx.append(i)
            gs.append(g if g.is_contiguous() else g.contiguous())
        self._early.update(idx)
        if inline and self._held is None:
            # (aliases, not the tensors themselves: a second reference to a gradient the node is about to return would
            # make AccumulateGrad clone it instead of adopting the arena view)
            self._held = (idx, [g.detach() for g in gs])
            return
        if inline and self._held is not None:
            idx, gs = self._held[0] + idx, self._held[1] + gs
            self._held = None
        if idx:
            self._launch(idx, gs, False)

    @torch.no_grad()
    def step(self, closure=None):
        self._not_swapped("step")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        early, self._early = self._early, None
        held, self._held = getattr(self, "_held", None), None
        if not (self._params[0].is_cuda and torch.cuda.is_current_stream_capturing()):
            self.check_uniform_grads()
        if held is not None and held[0]:
            self._launch(held[0], held[1], False)
        idx, grads = [], []
        for i, p in enumerate(self._params):
            if early is not None and i in early:
                continue
            g = p.grad
            if g is not None and not g.is_contiguous():
                g = g.contiguous()
            idx.append(i)
            grads.append(g)
        if self.clip_state is not None:       # (early is None here: every parameter is in idx)
            ops.grad_norm(grads, self.max_grad_norm, self.clip_state, self._clip_scratch)
        if early is None or any(g is not None for g in grads):
            self._launch(idx, grads, early is None)
        return loss

    def load_state_dict(self, state_dict):
        """the loaded moments are copied INTO the flat allocation (the kernel's records point there)"""
        super().load_state_dict(state_dict)
        steps = set()
        for p, m, v in zip(self._params, self._m, self._v):
            st = self.state.get(p, {})
            if "exp_avg" in st and st["exp_avg"].data_ptr() != m.data_ptr():
                m.copy_(st["exp_avg"].reshape(-1))
                v.copy_(st["exp_avg_sq"].reshape(-1))
                if "step" in st:
                    steps.add(float(st["step"]))
            self.state[p] = dict(step=self._step, exp_avg=m.view_as(p), exp_avg_sq=v.view_as(p))
        if len(steps) > 1:
            raise ValueError(f"HipAdam.load_state_dict: the loaded tensors carry different step counts {sorted(steps)}; this "
                             "optimiser keeps ONE step counter (see the module docstring)")
        if steps:
            self._step.fill_(steps.pop())
