"""QAdam — quantized-momentum Adam
(reference: bagua/torch_api/algorithms/q_adam.py:13-267).

Warmup phase: plain gradient allreduce + full Adam moment updates.
After warmup: the 2nd moment freezes, the *1st moment* (exp_avg) becomes
the communication tensor — updated by a python op on the scheduler path,
then synchronized with ByteGrad-style MinMaxUInt8 compression.
"""

import math
from typing import List, Tuple

import torch
from torch.optim.optimizer import Optimizer

from ...bucket import BaguaBucket
from ...communication import BaguaProcessGroup
from ...contrib.fused_kernels import flatten_params, segment_grads
from ...ops import native
from ...tensor import BaguaTensor
from .base import Algorithm, AlgorithmImpl


class QAdamOptimizer(Optimizer):
    def __init__(self, params, lr: float = 1e-3, warmup_steps: int = 100,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0):
        if not 0.0 <= lr:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if not 0.0 <= eps:
            raise ValueError("Invalid epsilon value: {}".format(eps))
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError("Invalid beta parameter 0: {}".format(betas[0]))
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError("Invalid beta parameter 1: {}".format(betas[1]))
        if warmup_steps <= 0:
            raise ValueError("warmup_steps must be > 0")
        defaults = dict(lr=lr, betas=betas, eps=eps,
                        weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.warmup_steps = warmup_steps

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()

        for group in self.param_groups:
            lr = group["lr"]
            weight_decay = group["weight_decay"]
            beta1, beta2 = group["betas"]
            eps = group["eps"]

            for param in group["params"]:
                state = self.state[param]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(param)
                    state["exp_avg_sq"] = torch.zeros_like(param)

                state["step"] += 1
                step_id = state["step"]
                grad = param.grad
                if weight_decay != 0:
                    grad = grad.add(param, alpha=weight_decay)

                if step_id < self.warmup_steps:
                    # full Adam moment updates only during warmup; after
                    # warmup exp_avg is maintained by the comm python-op
                    # and exp_avg_sq is frozen
                    state["exp_avg"].mul_(beta1).add_(grad, alpha=1 - beta1)
                    state["exp_avg_sq"].mul_(beta2).addcmul_(
                        grad, grad, value=1 - beta2)

                bias_correction1 = 1 - beta1 ** step_id
                bias_correction2 = 1 - beta2 ** step_id
                denom = (state["exp_avg_sq"].sqrt()
                         / math.sqrt(bias_correction2)).add_(eps)
                step_size = lr / bias_correction1
                param.data.addcdiv_(state["exp_avg"], denom,
                                    value=-step_size)
        return loss


class FusedQAdamOptimizer(QAdamOptimizer):
    """QAdam whose device math is hand-written HIP (f32 parameters only).

    Weights and ``exp_avg_sq`` are flattened once per group; during warmup
    ``exp_avg`` is flat too and a step is one fused Adam launch per group.
    After warmup ``exp_avg`` lives in the communication buckets (the
    algorithm re-points ``state[p]["exp_avg"]`` there), a bucket's momentum
    update is fused into the min/max pass of its compressed sync, and a
    step is one launch per group that reads the momentum where it lives.
    ``state[p]`` keeps ``step``, ``exp_avg`` and ``exp_avg_sq`` per
    parameter, the tensors as views of the flat state. On CPU, or without
    the extension, the parent's math runs on those views.
    """

    def __init__(self, params, lr: float = 1e-3, warmup_steps: int = 100,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0):
        super().__init__(params, lr=lr, warmup_steps=warmup_steps,
                         betas=betas, eps=eps, weight_decay=weight_decay)
        self._flat = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise TypeError(
                        "FusedQAdamOptimizer supports float32 parameters "
                        "only, got %s; use QAdamOptimizer" % p.dtype)
            # every parameter, as the parent's step takes them all
            rec = flatten_params(list(group["params"]))
            self._flat.append(rec)
            if rec is None:
                continue
            for name in ("exp_avg", "exp_avg_sq"):
                rec[name] = torch.zeros_like(rec["flat_w"])
            for k, p in enumerate(rec["params"]):
                begin = rec["offsets"][k]
                self.state[p] = {
                    "step": 0,
                    "exp_avg": rec["exp_avg"].narrow(
                        0, begin, p.numel()).view_as(p),
                    "exp_avg_sq": rec["exp_avg_sq"].narrow(
                        0, begin, p.numel()).view_as(p),
                }

    def _native(self):
        return native.available() and all(
            rec is None or rec["flat_w"].is_cuda for rec in self._flat)

    @torch.no_grad()
    def step(self, closure=None):
        if not self._native():
            return super().step(closure)
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = native.lib()
        for group, rec in zip(self.param_groups, self._flat):
            if rec is None:
                continue
            params = rec["params"]
            for p in params:
                self.state[p]["step"] += 1
            step_id = self.state[params[0]]["step"]
            beta1, beta2 = group["betas"]
            if step_id < self.warmup_steps:
                base = rec["exp_avg"].data_ptr()
                for k, p in enumerate(params):
                    if self.state[p]["exp_avg"].data_ptr() \
                            != base + 4 * rec["offsets"][k]:
                        raise RuntimeError(
                            "exp_avg left the flat state before the end "
                            "of warmup")
                lib.fused_adam_step_segments(
                    rec["flat_w"], segment_grads(rec),
                    rec["offsets"], rec["exp_avg"], rec["exp_avg_sq"],
                    step_id, group["lr"], beta1, beta2, group["eps"],
                    group["weight_decay"], False)
            else:
                # the moments are frozen (v) or kept by the communication
                # path (m), at the boundary step too
                lib.qadam_frozen_step_segments(
                    rec["flat_w"],
                    [self.state[p]["exp_avg"] for p in params],
                    rec["offsets"], rec["exp_avg_sq"], step_id, group["lr"],
                    beta1, beta2, group["eps"])
        return loss

    def load_state_dict(self, state_dict):
        """Copies into the views of the flat state (and of the buckets)
        instead of replacing them."""
        views = {p: dict(self.state[p]) for rec in self._flat
                 if rec is not None for p in rec["params"]}
        super().load_state_dict(state_dict)
        for p, old in views.items():
            new = self.state[p]
            for name in ("exp_avg", "exp_avg_sq"):
                if name in new:
                    old[name].copy_(new[name])
                new[name] = old[name]
            new["step"] = int(new.get("step", old["step"]))


class QAdamAlgorithmImpl(AlgorithmImpl):
    def __init__(self, process_group: BaguaProcessGroup,
                 q_adam_optimizer: QAdamOptimizer,
                 hierarchical: bool = True):
        super().__init__(process_group)
        self.hierarchical = hierarchical
        self.optimizer = q_adam_optimizer
        self.warmup_steps = q_adam_optimizer.warmup_steps

    @property
    def optimizer_step_id(self):
        param = self.optimizer.param_groups[0]["params"][0]
        return self.optimizer.state[param].get("step", 0)

    def need_reset(self):
        return self.optimizer_step_id == self.warmup_steps

    def bucket_alignment(self) -> int:
        n = self.process_group.get_global_communicator().nranks()
        return n * 32

    def init_tensors(self, ddp) -> List[BaguaTensor]:
        parameters = ddp.bagua_build_params()
        name_of, idx_of = {}, {}
        for idx, (name, param) in enumerate(reversed(parameters)):
            name_of[id(param)] = name
            idx_of[id(param)] = idx

        tensors = []
        warmup = self.optimizer_step_id < self.warmup_steps
        for group in self.optimizer.param_groups:
            for param in group["params"]:
                if param.grad is None:
                    param.grad = torch.zeros_like(param)
                if warmup:
                    t = ddp.ensure_bagua_tensor(
                        param, name_of[id(param)],
                        getter_closure=lambda p: p.grad,
                        setter_closure=lambda p, t: setattr(p, "grad", t))
                else:
                    if "exp_avg" not in self.optimizer.state[param]:
                        self.optimizer.state[param]["exp_avg"] = (
                            torch.zeros_like(param))

                    def set_momentum_fn(p, t):
                        self.optimizer.state[p]["exp_avg"] = t

                    t = ddp.ensure_bagua_tensor(
                        param, name_of[id(param)],
                        getter_closure=(
                            lambda p: self.optimizer.state[p]["exp_avg"]),
                        setter_closure=set_momentum_fn)
                t._q_adam_idx = idx_of[id(param)]
                tensors.append(t)
        tensors.sort(key=lambda t: t._q_adam_idx)
        return tensors

    def init_operations(self, ddp, bucket: BaguaBucket):
        bucket.clear_ops()
        if self.optimizer_step_id < self.warmup_steps:
            bucket.append_centralized_synchronous_op(
                hierarchical=False, average=True, group=self.process_group)
        elif isinstance(self.optimizer, FusedQAdamOptimizer):
            # one op: the momentum update rides on the sync, which keeps
            # the bucket on the native executor
            beta1, _ = self.optimizer.param_groups[0]["betas"]
            bucket.append_centralized_synchronous_op(
                hierarchical=self.hierarchical, average=True,
                scattergather=True, compression="MinMaxUInt8",
                group=self.process_group, momentum_beta1=beta1)
        else:

            def calculate_momentum(*args):
                beta1, _ = self.optimizer.param_groups[0]["betas"]
                for t in bucket.tensors:
                    t.tensor().mul_(beta1).add_(
                        t.proxy.grad, alpha=1 - beta1)

            bucket.append_python_op(calculate_momentum,
                                    group=self.process_group)
            bucket.append_centralized_synchronous_op(
                hierarchical=self.hierarchical, average=True,
                scattergather=True, compression="MinMaxUInt8",
                group=self.process_group)

    def init_backward_hook(self, ddp):
        warmup = self.optimizer_step_id < self.warmup_steps

        def hook(parameter_name, parameter):
            bt = ddp._bagua_tensor_map[parameter_name]
            if warmup:
                assert bt.data_ptr() == parameter.grad.data_ptr(), (
                    "registered tensor must be the grad during QAdam warmup")
            else:
                assert bt.data_ptr() == (
                    self.optimizer.state[parameter]["exp_avg"].data_ptr()), (
                    "registered tensor must be exp_avg after QAdam warmup")
            bt.mark_communication_ready(ddp.bagua_backend)

        return hook


class QAdamAlgorithm(Algorithm):
    def __init__(self, q_adam_optimizer: QAdamOptimizer,
                 hierarchical: bool = True):
        self.optimizer = q_adam_optimizer
        self.hierarchical = hierarchical

    def reify(self, process_group: BaguaProcessGroup):
        return QAdamAlgorithmImpl(process_group,
                                  q_adam_optimizer=self.optimizer,
                                  hierarchical=self.hierarchical)
