"""Child process of test_wgrad_sk_gpu.py: the opt-in split-K-in-workgroup FC weight gradient (wgrad_sk_kernel,
``MNIST_AMD_WGRAD_SK=1``, read once per process) against the torch oracle.

First-step ``forward_backward`` on a fresh trainer per shape, compared like ``test_grads_match_torch`` (same
tolerances).  Prints the mode the extension read, the per-layer errors of every shape, and exits non-zero on a miss.

  python tests/_wgrad_sk_child.py          every shape, both models, fp32 and bf16
  python tests/_wgrad_sk_child.py --pf4    MNIST_AMD_WGRAD_SK_PF=4 run: bf16 at batch 2048
"""
import os
import sys

import torch

from pytorch_ddp_mnist_amd.data.synthetic import make_split
from pytorch_ddp_mnist_amd.models import build_model
from pytorch_ddp_mnist_amd.ops.native import require_gpu
from test_native_gpu import make_trainer
from test_stale_state_gpu import check_grads_against_oracle

# (trainer batch, rows)
SHAPES = [
    (2048, 2048),  # SK_MIN_B; 4 splits, no XCD mapping
    (4096, 4096),  # 8 splits: xcd_ch; MLP fp32 as 3-part splits (SPL)
    (4096, 2085),  # partial K range of the last splits
]


def main(argv):
    pf4 = "--pf4" in argv
    C = require_gpu()
    mode = C.wgrad_sk_mode()
    print(f"wgrad_sk_mode {mode} SK_MIN_B {C.SK_MIN_B} pf {os.environ.get('MNIST_AMD_WGRAD_SK_PF', '')}", flush=True)
    assert mode == 1, "MNIST_AMD_WGRAD_SK=1 did not reach the extension"
    assert os.environ.get("MNIST_AMD_WGRAD_SK_PF", "") == ("4" if pf4 else "")
    shapes = [s for s in SHAPES if s[1] >= C.SK_MIN_B]
    assert shapes == SHAPES, "every shape must be on the split-K-in-workgroup kernel"
    if pf4:
        shapes = [(2048, 2048)]
    x, y = make_split(4096, seed=7)  # conftest's small_mnist train split
    failed = []
    for model_name in ("mlp", "lenet5"):
        for dtype in (("bf16",) if pf4 else ("fp32", "bf16")):
            for batch, rows in shapes:
                torch.manual_seed(0)
                module = build_model(model_name)
                tr = make_trainer(model_name, dtype, batch, x, y, module, max_indices=max(rows, len(y)))
                idx = torch.arange(rows, dtype=torch.int32) * 3 % len(y)
                tr.set_epoch_indices(idx)
                tr.reset_metrics()
                tr.forward_backward(rows)
                tag = f"sk{'/pf4' if pf4 else ''} {model_name}/{dtype}/batch={batch}/rows={rows}"
                try:
                    check_grads_against_oracle(tr, model_name, dtype, module, x[idx.numpy()], y[idx.numpy()], rows, tag)
                except AssertionError as e:
                    print(f"MISS {tag}: {e}", flush=True)
                    failed.append(tag)
                tr.close()
    print(f"wgrad_sk child: {len(failed)} misses {failed}", flush=True)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
