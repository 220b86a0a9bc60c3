"""Cost of the optimizer options when ON: ms/step of graph-replayed steps with weight decay + Nesterov + a learning-rate
table against the defaults (same momentum), one GPU, interleaved rounds of both trainers in one process.

Usage: python scripts/optim_cost.py [--steps N] [--rounds R] [MODEL:DTYPE:BATCH ...]
Prints one line per configuration: the per-round ms/step of each side and the ratio of the medians.
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from pytorch_ddp_mnist_amd.data.synthetic import make_split  # noqa: E402
from pytorch_ddp_mnist_amd.engine.native import NativeTrainer  # noqa: E402
from pytorch_ddp_mnist_amd.models import build_model  # noqa: E402
from pytorch_ddp_mnist_amd.optim.schedule import build_lr_table  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("configs", nargs="*", default=["lenet5:bf16:8192", "lenet5:bf16:128", "mlp:fp32:128", "mlp:bf16:8192"])
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()

for cfg in a.configs:
    model, dtype, batch = cfg.split(":")
    batch = int(batch)
    x, y = make_split(max(4096, batch), seed=7)
    n = a.steps * batch
    order = (torch.arange(n, dtype=torch.int64) * 7 % len(y)).to(torch.int32)
    sides = {}
    for name, kw in (("default", {}),
                     ("options", dict(weight_decay=5e-4, nesterov=True,
                                      lr_schedule=build_lr_table("cosine", 0.05, a.steps * a.rounds, warmup_steps=100)))):
        torch.manual_seed(0)
        tr = NativeTrainer(model, dtype, batch, torch.from_numpy(x.reshape(-1, 784)), torch.from_numpy(y), lr=0.05,
                           momentum=0.9, dropout=0.0, init=build_model(model), max_indices=n, **kw)
        tr.set_epoch_indices(order)
        tr.prepare_graphs()
        tr.run_steps(50)
        tr.synchronize()
        sides[name] = (tr, [])
    for _ in range(a.rounds):
        for name, (tr, ms) in sides.items():
            tr.set_epoch_indices(order)
            tr.synchronize()
            t0 = time.perf_counter()
            tr.run_steps(a.steps)
            tr.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3 / a.steps)
    med = {k: statistics.median(v[1]) for k, v in sides.items()}
    print(f"{cfg}: " + "  ".join(f"{k} " + "/".join(f"{t:.4f}" for t in v[1]) for k, v in sides.items())
          + f"  median ms/step {med['default']:.4f} -> {med['options']:.4f} (x{med['options'] / med['default']:.4f})", flush=True)
    for tr, _ in sides.values():
        tr.close()
