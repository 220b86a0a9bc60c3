"""A partial last batch AFTER full graph-replayed steps, against the torch oracle (as train_epoch runs it).

``test_grads_match_torch`` checks partial batches on a FRESH trainer only: every scratch buffer is still zero,
so a kernel that reads a row >= B of the previous batch reads a zero there.  Here two full steps run first
(``step(batch, use_graph=True)``), then ``forward_backward(tail)`` runs on buffers that hold the previous full
batch -- xT, h1T, h2T, dy*T, p1, p2, dp2, the FC / conv slabs, z1p and the MLP look-ahead rows -- and its
gradients are compared with torch autograd at the trainer's CURRENT parameters (no trajectory drift enters, so
the tolerances are those of ``test_grads_match_torch``).  The epoch holds exactly ``2 * batch + tail`` indices, so
the look-ahead gather bound (step_ctr[2]) is the tail's end.

Every case runs a second time with the float scratch buffers overwritten with the finite value 1.0e3 before
the partial batch: a padded or stale row that leaks into a product then shows as a gross gradient error (a
legitimate 0 x stale stays 0; nothing that holds indices, labels, argmax codes, counters, look-ahead rows or
parameters is touched, so the value is only ever an operand).

What this found: the 16-row LeNet bf16 heads (head16_kernel, fwd_head_kernel) launched ceil(B / 16) tiles while
the bf16 FC weight gradient reads rup(B, 32) rows, so for B % 32 in 1..16 (tails 76, 1061, 5424 here) the previous
batch's rows [rup(B, 16), rup(B, 32)) entered the FC gradients: 7.weight .. 11.bias off by 0.39 .. 0.59 at tail 76
and 0.03 .. 0.08 at tail 1061 (1e8 with the overwritten buffers), conv layers unaffected.  The launchers now run
rup(B, 32) / 16 tiles (csrc/kernels/lenet.hip); measured after the fix, whole vector: 5.1e-3 (tail 76), 3.0e-3 (1061),
7.9e-3 (5424), 8.0e-3 (7500), 9.7e-3 (2656) against 1e-2, identical with and without the overwrite.

After the full steps the packed operand images must be, bitwise, the image of the updated parameters
(``pack_buf`` against a second trainer's stand-alone ``launch_pack`` of the same parameters).
"""
import numpy as np
import pytest
import torch

from pytorch_ddp_mnist_amd.models import build_model
from test_native_gpu import (check_masks_against_torch, kernel_relu_masks, make_trainer, rel_err, torch_grads)

pytestmark = pytest.mark.gpu

# whole gradient / per layer: test_grads_match_torch's
TOLS = {"fp32": (2e-4, 1e-3), "bf16": (1e-2, 2e-2)}
LR, MOMENTUM = 0.05, 0.9
# float scratch of a step (engine/native.py); NOT idx, labels, m1, m2, xb, xnext, ynext, step_ctr, params, mom, pack_buf
SCRATCH = ("xT", "h1T", "h2T", "dy1T", "dy2T", "dy3T", "p1", "p2", "dp2", "slab_fc", "slab_conv", "z1p")
STALE_VALUE = 1.0e3

# (model, dtype, trainer batch, tail): each the smallest shape for
CASES = [
    # W = 8 last batch; look-ahead xnext; Bp = 80 (fp32) / 96 (bf16): 4 / 20 padded K rows hold the previous batch
    ("mlp", "fp32", 128, 76),
    ("mlp", "bf16", 128, 76),
    # xb hand-off conv_fwd -> conv_bwd, head16
    ("lenet5", "bf16", 128, 76),
    ("lenet5", "fp32", 128, 37),
    # odd tail; head16 / xb upper range; 4 -> 3 FC splits
    ("lenet5", "bf16", 2048, 1061),
    # the full step uses the >= 4096 split wgrad and the XCD mapping; the tail does not
    ("mlp", "bf16", 4096, 2085),
    ("mlp", "fp32", 4096, 2085),
    ("lenet5", "fp32", 4096, 2085),
    # fused forward + head on a partial batch; 5424 % 32 = 16
    ("lenet5", "bf16", 8192, 5424),
    # 7500 % 16 = 12: not fused, 32-row head with a 12-row last tile
    ("lenet5", "bf16", 8192, 7500),
    # below the fused kernel's smallest batch: separate kernels after fused full steps
    ("lenet5", "bf16", 8192, 2656),
]

_ORACLE = {}  # case -> (params, masks, (gref, loss_sum, correct)): one CPU oracle per case, shared by both runs


def layer_errors(module, g, gref):
    off, errs = 0, {}
    for k, v in module.state_dict().items():
        n = v.numel()
        errs[k] = rel_err(g[off:off + n], gref[off:off + n])
        off += n
    return errs


def check_grads_against_oracle(tr, model_name, dtype, module, xr, yr, n, tag, cache=None, key=None):
    """tr.grads() and the metrics of the ``n`` rows (xr, yr) the trainer just ran forward_backward on, against
    torch_grads at ``module`` -- the assertions of test_grads_match_torch.  ``cache`` / ``key``: reuse the oracle
    of an earlier run at bitwise the same parameters and ReLU masks."""
    tol, layer_tol = TOLS[dtype]
    bf = dtype == "bf16"
    g = tr.grads()
    masks = None
    if model_name == "mlp":
        masks = kernel_relu_masks(tr, n)
        check_masks_against_torch(module, xr, masks, bf)
    flat = torch.cat([v.reshape(-1) for v in module.state_dict().values()])
    hit = cache.get(key) if cache is not None else None
    if hit is not None and torch.equal(hit[0], flat) and (masks is None or all(torch.equal(a, b) for a, b in zip(hit[1], masks))):
        gref, loss_sum, correct = hit[2]
    else:
        gref, loss_sum, correct = torch_grads(model_name, module, xr, yr, masks, bf16_inputs=bf)
        if cache is not None:
            cache[key] = (flat, masks, (gref, loss_sum, correct))
    assert g.shape == gref.shape
    e = rel_err(g, gref)
    errs = layer_errors(module, g, gref)
    print(f"{tag}: total {e:.2e} (bound {tol:.0e}) per layer (bound {layer_tol:.0e}) "
          + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    assert e < tol, f"{tag}: grad rel err {e} (per layer: {errs})"
    for k, le in errs.items():
        assert le < layer_tol, f"{tag}: {k}: rel err {le} (all layers: {errs})"
    st = tr.read_metrics()
    assert st.count == n
    assert abs(st.loss_sum - loss_sum) / loss_sum < max(tol, 1e-4) * 10, (st.loss_sum, loss_sum)
    assert abs(st.correct - correct) <= max(1, n // 50), (st.correct, correct)
    return e, errs


def assert_pack_is_image_of_params(a, b):
    """``a.pack_buf`` == the stand-alone launch_pack image of ``a.params`` (run on the second trainer ``b``),
    bitwise.  Packer<Model, T>::pack (csrc/kernels/models.h) is a pure per-parameter function and both buffers
    start zeroed, so every byte of pack_buf is a function of params: nothing is excluded."""
    a.synchronize()
    b.load_flat(a.params)
    b.synchronize()
    pa, pb = a.pack_buf.view(torch.uint8), b.pack_buf.view(torch.uint8)
    assert pa.shape == pb.shape
    if not torch.equal(pa, pb):
        bad = (pa != pb).nonzero().view(-1)
        es = a.pack_buf.element_size()
        raise AssertionError(f"pack_buf is not the image of params: {bad.numel()} bytes differ, elements "
                             f"{int(bad[0]) // es}..{int(bad[-1]) // es} of {a.pack_buf.numel()}")


@pytest.mark.parametrize("stale", [False, True], ids=["asis", "overwritten"])
@pytest.mark.parametrize("model_name,dtype,batch,tail", CASES)
def test_partial_batch_after_full_steps_matches_torch(native, small_mnist, model_name, dtype, batch, tail, stale):
    x, y, _, _ = small_mnist
    torch.manual_seed(0)
    module = build_model(model_name)
    n = 2 * batch + tail
    kw = dict(lr=LR, momentum=MOMENTUM, max_indices=n)
    tr = make_trainer(model_name, dtype, batch, x, y, module, **kw)
    idx = torch.arange(n, dtype=torch.int32) * 3 % len(y)
    tr.set_epoch_indices(idx)
    tr.step(batch, use_graph=True)
    tr.step(batch, use_graph=True)
    tr.synchronize()
    assert_pack_is_image_of_params(tr, make_trainer(model_name, dtype, batch, x, y, module, **kw))
    cur = tr.to_module()
    tr.reset_metrics()
    if stale:
        with torch.cuda.stream(tr.stream):
            for name in SCRATCH:
                t = getattr(tr, name)
                if t is not None:
                    assert t.is_floating_point(), name
                    t.fill_(STALE_VALUE)
    tr.forward_backward(tail)  # device step counter 2: rows [2 * batch, 2 * batch + tail)
    rows = idx[2 * batch:].numpy()
    assert len(rows) == tail
    assert int(tr.step_ctr[0]) == 2 and int(tr.step_ctr[2]) == n
    check_grads_against_oracle(tr, model_name, dtype, cur, x[rows], y[rows], tail,
                               f"{model_name}/{dtype}/batch={batch}/tail={tail}/{'overwritten' if stale else 'asis'}",
                               cache=_ORACLE, key=(model_name, dtype, batch, tail))
