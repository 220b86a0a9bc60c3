"""Every step's SGD update against the torch oracle, and the packed operand images after it.

``test_sgd_step_matches_torch`` compares updated parameters with torch on one path only (fp32, B = 64, eager
launches).  Here three graph-replayed steps run on each update path -- reduce_sgd_kernel over the conv slab,
reduce_sgd_direct_kernel on the aux stream, the SGD epilogues of wgrad_sgd_kernel and conv_bwd_fc_kernel, the
split weight gradient at B >= 4096, fp32 and bf16 -- and around EACH step the momentum and the parameters
are compared with

    m_exp = momentum * m_s + g_ref(p_s)        p_exp = p_s - lr * m_exp

where g_ref is the torch oracle's gradient at the parameters p_s the step started from (so no trajectory drift
enters and the gradient tolerances of ``test_grads_match_torch`` carry over: an error of tol * |g_ref| in the
gradient is one of tol * |g_ref| in the momentum and lr * tol * |g_ref| in the parameters; 2^-22 * |.| covers the
fp32 rounding of the update itself).

After every step ``pack_buf`` must be, bitwise, the image of the updated parameters: a range that was updated
but not re-packed, or packed from the pre-update value, is invisible to bf16 tolerances (see the CPU test's
measured p_0 / p_1 gradient differences) but not to this comparison.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_ddp_mnist_amd.models import build_model, flatten_state, unflatten_state
from test_native_gpu import (_normalize, check_masks_against_torch, kernel_relu_masks, make_trainer, torch_grads)
from test_stale_state_gpu import LR, MOMENTUM, TOLS, assert_pack_is_image_of_params

STEPS = 3
ROUND = 2.0 ** -22  # fp32 rounding of b = mu * m + g and p - lr * b, relative to the result's norm

# (model, dtype, batch): the update path
CASES = [
    # fused forward + head, concurrent schedule: reduce_sgd_direct on the aux stream, reduce_sgd over the conv slab
    ("lenet5", "bf16", 4096),
    ("lenet5", "fp32", 2048),
    # split weight gradient
    ("mlp", "bf16", 4096),
    ("mlp", "fp32", 4096),
    # conv_bwd_fc_kernel's / the aux-stream wgrad_sgd_kernel's SGD epilogue
    ("lenet5", "bf16", 128),
    # wgrad_sgd_kernel's epilogue, look-ahead rows
    ("mlp", "bf16", 128),
    ("mlp", "fp32", 128),
]


def expected_update(p_s, m_s, g_ref, lr=LR, momentum=MOMENTUM):
    """torch.optim.SGD(lr, momentum, dampening=0) as a recurrence on flat vectors (float64)."""
    m_exp = momentum * m_s.double() + g_ref.double()
    return m_exp, p_s.double() - lr * m_exp


def module_at(model_name, flat):
    m = build_model(model_name)
    m.load_state_dict(unflatten_state(m, flat))
    return m


def layer_slices(module):
    off, out = 0, [("all", slice(0, None))]
    for k, v in module.state_dict().items():
        out.append((k, slice(off, off + v.numel())))
        off += v.numel()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("model_name,dtype,batch", CASES)
def test_each_update_matches_torch(native, small_mnist, model_name, dtype, batch):
    x, y, _, _ = small_mnist
    tol, layer_tol = TOLS[dtype]
    bf = dtype == "bf16"
    torch.manual_seed(0)
    module = build_model(model_name)
    kw = dict(lr=LR, momentum=MOMENTUM, max_indices=STEPS * batch)
    tr = make_trainer(model_name, dtype, batch, x, y, module, **kw)
    twin = make_trainer(model_name, dtype, batch, x, y, module, **kw)  # stand-alone launch_pack of tr's parameters
    idx = torch.arange(STEPS * batch, dtype=torch.int32) * 3 % len(y)
    tr.set_epoch_indices(idx)
    slices = layer_slices(module)
    for s in range(STEPS):
        tr.synchronize()
        p_s, m_s = tr.params.cpu().clone(), tr.mom.cpu().clone()
        tr.step(batch, use_graph=True)
        tr.synchronize()
        p_n, m_n = tr.params.cpu().clone(), tr.mom.cpu().clone()
        rows = idx[s * batch:(s + 1) * batch].numpy()
        at = module_at(model_name, p_s)
        masks = None
        if model_name == "mlp":
            masks = kernel_relu_masks(tr, batch)
            check_masks_against_torch(at, x[rows], masks, bf)
        g_ref, _, _ = torch_grads(model_name, at, x[rows], y[rows], masks, bf16_inputs=bf)
        m_exp, p_exp = expected_update(p_s, m_s, g_ref)
        report, failed = [], []
        for k, sl in slices:
            t = tol if k == "all" else layer_tol
            gn = float(g_ref[sl].double().norm())
            em, bm = float((m_n[sl].double() - m_exp[sl]).norm()), t * gn + ROUND * float(m_exp[sl].norm())
            ep, bp = float((p_n[sl].double() - p_exp[sl]).norm()), LR * t * gn + ROUND * float(p_exp[sl].norm())
            report.append(f"{k}: mom {em:.2e}/{bm:.2e} par {ep:.2e}/{bp:.2e}")
            if not (em <= bm and ep <= bp):
                failed.append(report[-1])
        print(f"{model_name}/{dtype}/B={batch} step {s} (error/bound) " + "  ".join(report))
        assert not failed, f"{model_name}/{dtype}/B={batch} step {s}: {failed}"
        assert float((p_n - p_s).norm()) > 0.0
        assert_pack_is_image_of_params(tr, twin)


def _oracle_loss_grads(model_name, module, xb, yb, bf):
    g, _, _ = torch_grads(model_name, module, xb, yb, None, bf16_inputs=bf)
    return g


@pytest.mark.parametrize("model_name", ["mlp", "lenet5"])
def test_update_recurrence_is_torch_sgd(model_name):
    """CPU: the m_exp / p_exp recurrence of the GPU test, run for three steps from torch's own gradients, is
    torch.optim.SGD(lr, momentum, dampening=0) to 1e-6 relative -- and how far the oracle's gradient moves over
    ONE update (at p_1 against p_0, same rows), per layer, printed next to layer_tol: where it exceeds layer_tol
    the GPU test's bound sees a one-step-stale weight image, where it does not (bf16) only the bitwise pack
    comparison does."""
    from pytorch_ddp_mnist_amd.data.synthetic import make_split
    B = 128
    x, y = make_split(STEPS * B, seed=7)
    torch.manual_seed(0)
    module = build_model(model_name)
    ref = copy.deepcopy(module).eval()
    opt = torch.optim.SGD(ref.parameters(), lr=LR, momentum=MOMENTUM, dampening=0)
    p, m = flatten_state(module).double(), torch.zeros(sum(v.numel() for v in module.state_dict().values()), dtype=torch.float64)
    hist = [p.float()]
    for s in range(STEPS):
        rows = np.arange(s * B, (s + 1) * B)
        g = _oracle_loss_grads(model_name, module_at(model_name, p.float()), x[rows], y[rows], False)
        m, p = expected_update(p, m, g)
        hist.append(p.float())
        opt.zero_grad()
        xb = _normalize(x[rows])
        out = ref(xb.view(B, -1) if model_name == "mlp" else xb.view(B, 1, 28, 28))
        yb = torch.from_numpy(y[rows].astype(np.int64))
        (F.nll_loss(out, yb) if model_name == "lenet5" else F.cross_entropy(out, yb)).backward()
        opt.step()
        pt = flatten_state(ref).double()
        e = float((p - pt).norm() / pt.norm())
        assert e < 1e-6, f"step {s}: recurrence vs torch.optim.SGD rel err {e}"
    # one-step staleness as the oracle sees it: the gradient of step 1's rows at p_1 against the one at p_0
    rows = np.arange(B, 2 * B)
    for dtype in ("fp32", "bf16"):
        bf = dtype == "bf16"
        g0 = _oracle_loss_grads(model_name, module_at(model_name, hist[0]), x[rows], y[rows], bf)
        g1 = _oracle_loss_grads(model_name, module_at(model_name, hist[1]), x[rows], y[rows], bf)
        diffs = {k: float((g0[sl] - g1[sl]).norm() / (g1[sl].norm() + 1e-12)) for k, sl in layer_slices(module)}
        assert all(np.isfinite(v) for v in diffs.values())
        print(f"{model_name}/{dtype}: |g(p_0) - g(p_1)| / |g(p_1)| (layer_tol {TOLS[dtype][1]:.0e}, whole {TOLS[dtype][0]:.0e}) "
              + " ".join(f"{k}={v:.2e}" for k, v in diffs.items()))
