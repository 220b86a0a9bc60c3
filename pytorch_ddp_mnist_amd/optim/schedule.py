"""Per-step learning-rate tables.

A schedule is a float32 table indexed by the global step: entry ``t`` is the rate of step ``t``, steps at or
beyond the table's length use its last entry.  The native trainer keeps the table on the device and its head
kernels publish the current entry each step, so one captured step graph serves the whole schedule
(``NativeTrainer.set_lr_schedule``); the torch-CPU engine sets its param-group ``lr`` from the same table.

``build_lr_table`` closed forms (``u = t - warmup_steps``, ``U = total_steps - warmup_steps``), equal to torch's
``StepLR(step_size, gamma)``, ``CosineAnnealingLR(T_max=total_steps, eta_min=lr_min)`` and
``LinearLR(1.0, lr_min / base_lr, total_steps)`` stepped once per training step when ``warmup_steps == 0``:

    t < warmup_steps : base_lr * (t + 1) / warmup_steps
    constant         : base_lr
    step             : base_lr * gamma ** (u // step_size)
    cosine           : lr_min + (base_lr - lr_min) * (1 + cos(pi * u / U)) / 2
    linear           : base_lr + (lr_min - base_lr) * u / U
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

KINDS = ("constant", "step", "cosine", "linear")


def build_lr_table(kind: str, base_lr: float, total_steps: int, warmup_steps: int = 0, lr_min: float = 0.0,
                   step_size: Optional[int] = None, gamma: float = 0.1) -> np.ndarray:
    if kind not in KINDS:
        raise ValueError(f"unknown lr schedule {kind!r} (one of {', '.join(KINDS)})")
    total_steps, warmup_steps = int(total_steps), int(warmup_steps)
    if total_steps <= 0:
        raise ValueError(f"lr schedule over {total_steps} steps")
    if warmup_steps < 0:
        raise ValueError(f"warmup_steps {warmup_steps} is negative")
    if not (base_lr >= 0.0 and lr_min >= 0.0):
        raise ValueError(f"learning rates must be non-negative (base_lr {base_lr}, lr_min {lr_min})")
    if kind == "step" and (step_size is None or int(step_size) < 1):
        raise ValueError("lr schedule 'step' needs step_size >= 1")
    U = max(1, total_steps - warmup_steps)
    out = np.empty(total_steps, dtype=np.float64)
    for t in range(total_steps):
        if t < warmup_steps:
            out[t] = base_lr * (t + 1) / warmup_steps
            continue
        u = t - warmup_steps
        if kind == "constant":
            out[t] = base_lr
        elif kind == "step":
            out[t] = base_lr * gamma ** (u // int(step_size))
        elif kind == "cosine":
            out[t] = lr_min + (base_lr - lr_min) * (1.0 + math.cos(math.pi * u / U)) / 2.0
        else:
            out[t] = base_lr + (lr_min - base_lr) * u / U
    return out.astype(np.float32)


def validate_lr_table(table) -> np.ndarray:
    """A sequence or 1-D tensor of rates as a float32 array: non-empty, finite, non-negative."""
    if hasattr(table, "detach"):
        table = table.detach().cpu().numpy()
    arr = np.asarray(table, dtype=np.float64)
    if arr.ndim != 1 or arr.size == 0:
        raise ValueError(f"lr schedule must be a non-empty 1-D sequence (shape {arr.shape})")
    if not np.isfinite(arr).all():
        raise ValueError("lr schedule holds a non-finite rate")
    if (arr < 0).any():
        raise ValueError("lr schedule holds a negative rate")
    return arr.astype(np.float32)


def lr_at(table: np.ndarray, step: int) -> float:
    """The table's rate for global step ``step`` (the last entry from the table's end on)."""
    return float(table[min(max(int(step), 0), len(table) - 1)])


def check_sgd_options(momentum: float, weight_decay: float, nesterov: bool) -> None:
    """torch.optim.SGD's argument checks (dampening is always 0 here)."""
    if weight_decay < 0.0:
        raise ValueError(f"Invalid weight_decay value: {weight_decay}")
    if nesterov and momentum == 0:
        raise ValueError("Nesterov momentum requires a momentum and zero dampening")
