"""Native HIP kernels vs a plain PyTorch fp32 reference of the same op (survey §4 tiers T2/T3).

Every test runs the native trainer on one MI355X and compares against torch autograd on the CPU
with identical weights and batch order.  Dropout is disabled (p=0) where bit-level comparisons
are made; dropout statistics are tested separately.
"""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_ddp_mnist_amd.models import build_model, flatten_grads, flatten_state

pytestmark = pytest.mark.gpu


def _normalize(x_u8):
    return (torch.from_numpy(x_u8).float() / 255.0 - 0.1307) / 0.3081


def bf16_round(t):
    return t.to(torch.bfloat16).float()


class _RoundBF16(torch.autograd.Function):
    """Straight-through bf16 rounding of a forward value and/or of its gradient: marks the points where
    the bf16 kernels store an intermediate in bf16 (fp32 arithmetic everywhere else)."""

    @staticmethod
    def forward(ctx, x, fwd, bwd):
        ctx.bwd = bwd
        return bf16_round(x) if fwd else x

    @staticmethod
    def backward(ctx, g):
        return (bf16_round(g) if ctx.bwd else g), None, None


def _r(x, fwd=True, bwd=True):
    return _RoundBF16.apply(x, fwd, bwd)


def bf16_emulated_forward(model_name, m, x, masks=None):
    """Forward with the bf16 kernels' storage roundings (csrc/kernels/head.hip, lenet.hip): input,
    pooled / hidden activations (forward), pre-activation and pooled-output gradients (backward)."""
    x = _r(x, True, False)
    if model_name == "lenet5":
        z1 = _r(m[0](x), False, True)             # conv1 pre-activation grad dY1 -> bf16 (DY1T)
        p1 = _r(m[2](m[1](z1)), True, False)      # pool1 output -> bf16 (P1)
        p2 = _r(m[5](m[4](m[3](p1))), True, True)  # pool2 output -> bf16 (P2), its grad dp2 -> bf16
        a1 = _r(m[7](m[6](p2)), False, True)      # FC pre-activation grads -> bf16 (dy1T, dy2T)
        h1 = _r(m[8](a1), True, False)
        a2 = _r(m[9](h1), False, True)
        h2 = _r(m[10](a2), True, False)
        return m[12](_r(m[11](h2), False, True))  # dlogits -> bf16 (dy3T)
    a1 = _r(m[0](x), False, True)
    h1 = _r(a1 * masks[0] if masks is not None else torch.relu(a1), True, False)
    a2 = _r(m[3](h1), False, True)
    h2 = _r(a2 * masks[1] if masks is not None else torch.relu(a2), True, False)
    return _r(m[5](h2), False, True)


def torch_grads(model_name, module, x_u8, y_u8, masks=None, bf16_inputs=False):
    """fp32 torch reference.  ``masks`` (MLP only): multiplicative masks [B,128] x2 that replace the two
    hidden ReLUs: the native kernel's own ReLU (x dropout scale) masks.  With them the reference
    follows the kernel through exact pre-activation ties (a pre-activation of +1e-8 in torch can round
    to 0 under another summation order and flip one ReLU: a measure-zero event that nonetheless shifts
    a whole dW1 row) -- callers first check the masks against torch's own ReLU.  ``bf16_inputs``: the
    oracle sees the bf16-rounded inputs and weights the bf16 kernels multiply, and rounds to bf16
    wherever the kernels store an intermediate in bf16 (fp32 arithmetic otherwise)."""
    m = copy.deepcopy(module).float()
    m.eval()  # dropout off: the native side runs with p=0 in exact comparisons (no BN in either model)
    if bf16_inputs:
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() > 1:
                    p.copy_(bf16_round(p))
    m.zero_grad()
    x = _normalize(x_u8)
    if bf16_inputs:
        x = bf16_round(x)
    x = x.view(len(x), -1) if model_name == "mlp" else x.view(len(x), 1, 28, 28)
    if bf16_inputs:
        out = bf16_emulated_forward(model_name, m, x, masks)
    elif masks is not None:
        out = m[5](m[3](m[0](x) * masks[0]) * masks[1])  # masks replace the ReLUs (tie-following)
    else:
        out = m(x)
    y = torch.from_numpy(y_u8.astype(np.int64))
    loss = F.nll_loss(out, y) if model_name == "lenet5" else F.cross_entropy(out, y)
    loss.backward()
    pred = out.argmax(1)
    return flatten_grads(m), float(loss.detach()) * len(y), int((pred == y).sum())


def make_trainer(model_name, dtype, batch, x, y, module, dropout=0.0, **kw):
    from pytorch_ddp_mnist_amd.engine.native import NativeTrainer
    return NativeTrainer(model_name, dtype, batch, torch.from_numpy(x.reshape(-1, 784)), torch.from_numpy(y),
                         dropout=dropout, init=module, **kw)


def rel_err(a, b):
    return float((a - b).norm() / (b.norm() + 1e-12))


def kernel_relu_masks(tr, batch):
    """The MLP kernel's stored post-ReLU activations h1T/h2T -> 0/1 masks [B,128] each."""
    return [(t[:128, :batch].float().cpu().T > 0).float() for t in (tr.h1T, tr.h2T)]


def check_masks_against_torch(module, x_u8, masks, bf16_inputs):
    """The kernel's ReLU masks must be torch's own on >= 99.9 % of the entries before an oracle may
    reuse them (a wrong forward ReLU would otherwise be followed by the oracle)."""
    m = copy.deepcopy(module).float().eval()
    x = _normalize(x_u8)
    if bf16_inputs:
        x = bf16_round(x)
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() > 1:
                    p.copy_(bf16_round(p))
    with torch.no_grad():
        h1 = torch.relu(m[0](x.view(len(x), -1)))
        h2 = torch.relu(m[3](bf16_round(h1) if bf16_inputs else h1))
    for mk, h in zip(masks, (h1, h2)):
        agree = ((h > 0).float() == mk).float().mean().item()
        assert agree >= 0.999, f"kernel ReLU mask agrees with torch on {agree:.5f} of entries"


@pytest.mark.parametrize("model_name", ["mlp", "lenet5"])
# fp32: exact products; bf16: the oracle multiplies the same bf16-rounded inputs and weights in fp32
# and rounds the same stored intermediates to bf16, so what remains is summation order (and the
# rounding of values that differ in their last bits) -- bounded per layer by 2e-2
@pytest.mark.parametrize("dtype,tol,layer_tol", [("fp32", 2e-4, 1e-3), ("bf16", 1e-2, 2e-2)])
# 8192: the headline per-GPU batch; 96/76/48/24/16: the reference's last-batch sizes (60000 or 10000
# samples over W = 1..8 ranks at B=128); 37: odd
@pytest.mark.parametrize("batch", [8192, 4096, 2048, 1024, 128, 96, 76, 48, 37, 24, 16])
def test_grads_match_torch(native, small_mnist, model_name, dtype, tol, layer_tol, batch):
    x, y, _, _ = small_mnist
    torch.manual_seed(0)
    module = build_model(model_name)
    # trainer batch <= 1024 takes the layer-1 split path (l1_split_kernel), 2048 the fused head,
    # 4096 (8 wgrad splits) the XCD-aware wgrad mapping
    tr = make_trainer(model_name, dtype, max(128, batch), x, y, module, max_indices=max(batch, len(y)))
    idx = torch.arange(batch, dtype=torch.int32) * 3 % len(y)
    tr.set_epoch_indices(idx)
    tr.reset_metrics()
    tr.forward_backward(batch)
    g = tr.grads()
    bf = dtype == "bf16"
    masks = None
    if model_name == "mlp":
        masks = kernel_relu_masks(tr, batch)
        check_masks_against_torch(module, x[idx.numpy()], masks, bf)
    gref, loss_sum, correct = torch_grads(model_name, module, x[idx.numpy()], y[idx.numpy()], masks, bf16_inputs=bf)
    assert g.shape == gref.shape
    e = rel_err(g, gref)
    assert e < tol, f"{model_name}/{dtype}/B={batch}: grad rel err {e}"
    # per-layer check so a single wrong small tensor cannot hide in the norm
    off, errs = 0, {}
    for k, v in module.state_dict().items():
        n = v.numel()
        errs[k] = rel_err(g[off:off + n], gref[off:off + n])
        off += n
    print(f"{model_name}/{dtype}/B={batch}: total {e:.2e} per layer " + " ".join(f"{k}={v:.1e}" for k, v in errs.items()))
    for k, le in errs.items():
        assert le < layer_tol, f"{k}: rel err {le} (all layers: {errs})"
    st = tr.read_metrics()
    assert st.count == batch
    assert abs(st.loss_sum - loss_sum) / loss_sum < max(tol, 1e-4) * 10
    assert abs(st.correct - correct) <= max(1, batch // 50)


@pytest.mark.parametrize("model_name", ["mlp", "lenet5"])
def test_sgd_step_matches_torch(native, small_mnist, model_name):
    x, y, _, _ = small_mnist
    torch.manual_seed(1)
    module = build_model(model_name)
    tr = make_trainer(model_name, "fp32", 64, x, y, module, momentum=0.9, lr=0.05)
    ref = copy.deepcopy(module).eval()
    opt = torch.optim.SGD(ref.parameters(), lr=0.05, momentum=0.9)
    idx = torch.randperm(len(y), generator=torch.Generator().manual_seed(3))[:64 * 5].to(torch.int32)
    tr.set_epoch_indices(idx)
    for s in range(5):
        tr.step(64, use_graph=False)
        b = idx[s * 64:(s + 1) * 64].numpy()
        opt.zero_grad()
        xb = _normalize(x[b])
        xb = xb.view(64, -1) if model_name == "mlp" else xb.view(64, 1, 28, 28)
        out = ref(xb)
        yb = torch.from_numpy(y[b].astype(np.int64))
        (F.nll_loss(out, yb) if model_name == "lenet5" else F.cross_entropy(out, yb)).backward()
        opt.step()
    tr.synchronize()
    e = rel_err(tr.params.cpu(), flatten_state(ref))
    assert e < 1e-5, e


def test_mlp_loss_trajectory_matches_torch(native, small_mnist):
    """T3: the reference MLP (dropout 0) for 100 graph-replayed steps vs torch on CPU from the same init
    and batch order: per-step losses agree (fp32 kernels; only summation order differs)."""
    x, y, _, _ = small_mnist
    torch.manual_seed(11)
    module = build_model("mlp")
    tr = make_trainer("mlp", "fp32", 128, x, y, module, lr=0.01, momentum=0.0)
    ref = copy.deepcopy(module).eval()
    opt = torch.optim.SGD(ref.parameters(), lr=0.01)
    g = torch.Generator().manual_seed(5)
    losses_n, losses_t = [], []
    for ep in range(4):  # 4 x 32 steps of 128
        idx = torch.randperm(len(y), generator=g).to(torch.int32)
        tr.set_epoch_indices(idx)
        for s in range(len(y) // 128):
            tr.reset_metrics()
            tr.step(128, use_graph=True)
            losses_n.append(tr.read_metrics().mean_loss)
            b = idx[s * 128:(s + 1) * 128].numpy()
            opt.zero_grad()
            out = ref(_normalize(x[b]).view(128, -1))
            loss = F.cross_entropy(out, torch.from_numpy(y[b].astype(np.int64)))
            loss.backward()
            opt.step()
            losses_t.append(float(loss.detach()))
            if len(losses_n) == 100:
                break
        if len(losses_n) == 100:
            break
    ln, lt = np.array(losses_n), np.array(losses_t)
    assert np.max(np.abs(ln - lt) / lt) < 1e-3, np.max(np.abs(ln - lt) / lt)
    assert lt[-10:].mean() < lt[:10].mean()  # and it actually trained


@pytest.mark.parametrize("model_name,dtype", [("mlp", "bf16"), ("lenet5", "bf16"), ("lenet5", "fp32")])
def test_fused_step_equals_phased(native, small_mnist, model_name, dtype):
    """The single-GPU step (fused reduce+SGD+pack kernel) == forward_backward + reduce + optimizer_step."""
    x, y, _, _ = small_mnist
    torch.manual_seed(5)
    module = build_model(model_name)
    a = make_trainer(model_name, dtype, 128, x, y, module, momentum=0.9, lr=0.05)
    b = make_trainer(model_name, dtype, 128, x, y, module, momentum=0.9, lr=0.05)
    idx = torch.randperm(len(y), generator=torch.Generator().manual_seed(4))[:128 * 4].to(torch.int32)
    a.set_epoch_indices(idx)
    b.set_epoch_indices(idx)
    for _ in range(4):
        a.step(128, use_graph=False)
        b.forward_backward(128)
        b.optimizer_step(1.0)
    a.synchronize()
    b.synchronize()
    e = rel_err(a.params.cpu(), b.params.cpu())
    assert e < 1e-5, e
    assert rel_err(a.grad.cpu(), b.grad.cpu()) < 1e-5


def test_fwd_head_fused_equals_separate(native, small_mnist):
    """LeNet bf16 at a large batch: the fused forward + FC head kernel (fwd_head_kernel) against the two
    separate kernels (conv_fwd_kernel + head_kernel) -- gradients, metrics and 6 graph-replayed training
    steps (incl. a 4-step graph with the deferred aux join).  Layer 1 of the head sums its K in a different
    order in the two (the head kernel splits it over wave pairs), so agreement is to bf16 rounding."""
    x, y, _, _ = small_mnist
    torch.manual_seed(21)
    module = build_model("lenet5")
    B = 4096
    a = make_trainer("lenet5", "bf16", B, x, y, module, momentum=0.9, lr=0.05, max_indices=8 * B)
    b = make_trainer("lenet5", "bf16", B, x, y, module, momentum=0.9, lr=0.05, max_indices=8 * B)
    assert a.fwd_head_applies() and a.rt.fwd_head
    b.rt.set_fwd_head(False)
    idx = torch.cat([torch.randperm(len(y), generator=torch.Generator().manual_seed(s)) for s in range(8)]).to(torch.int32)
    for t in (a, b):
        t.set_epoch_indices(idx)
        t.reset_metrics()
        t.forward_backward(B)
    ga, gb = a.grads(), b.grads()
    assert rel_err(ga, gb) < 5e-3, rel_err(ga, gb)
    ma, mb = a.read_metrics(), b.read_metrics()
    assert ma.count == mb.count == B
    assert abs(ma.loss_sum - mb.loss_sum) / mb.loss_sum < 1e-3
    assert abs(ma.correct - mb.correct) <= B // 200
    for t in (a, b):
        t.set_epoch_indices(idx)
        t.step(B, use_graph=True)
        t.step(B, use_graph=True)
        t.run_steps(4, use_graph=True, k=4)
        t.synchronize()
    assert rel_err(a.params.cpu(), b.params.cpu()) < 2e-3, rel_err(a.params.cpu(), b.params.cpu())


@pytest.mark.parametrize("model_name,dtype", [("mlp", "fp32"), ("mlp", "bf16"), ("lenet5", "fp32"), ("lenet5", "bf16")])
def test_graph_replay_equals_eager(native, small_mnist, model_name, dtype):
    x, y, _, _ = small_mnist
    torch.manual_seed(2)
    module = build_model(model_name)
    idx = torch.randperm(len(y), generator=torch.Generator().manual_seed(5))[:128 * 4].to(torch.int32)
    res = []
    for use_graph in (False, True):
        tr = make_trainer(model_name, dtype, 128, x, y, module, dropout=0.2)
        tr.set_epoch_indices(idx)
        for _ in range(4):
            tr.step(128, use_graph=use_graph)
        tr.synchronize()
        res.append(tr.params.cpu().clone())
    assert torch.equal(res[0], res[1]), "hipGraph replay must be bitwise identical to eager launches"


def test_determinism(native, small_mnist):
    x, y, _, _ = small_mnist
    module = build_model("lenet5")
    idx = torch.arange(256, dtype=torch.int32)
    out = []
    for _ in range(2):
        tr = make_trainer("lenet5", "bf16", 128, x, y, module)
        tr.set_epoch_indices(idx)
        tr.step(128, use_graph=False)
        tr.step(128, use_graph=False)
        tr.synchronize()
        out.append(tr.params.cpu().clone())
    assert torch.equal(out[0], out[1]), "fixed-order slab reductions must make steps bitwise reproducible"


@pytest.mark.parametrize("model_name,dtype", [("mlp", "fp32"), ("lenet5", "bf16")])
def test_training_learns(native, small_mnist, model_name, dtype):
    x, y, xt, yt = small_mnist
    torch.manual_seed(3)
    # lr 0.05 / momentum 0.9 oscillates in bf16 (eval 0.92 -> 0.79 between epochs, the path depends on
    # summation order); 0.02 learns monotonically past the plateau of the first ~1.5 epochs
    tr = make_trainer(model_name, dtype, 128, x, y, build_model(model_name), lr=0.02, momentum=0.9)
    g = torch.Generator().manual_seed(0)
    accs = []
    for ep in range(6):
        st = tr.train_epoch(torch.randperm(len(y), generator=g).to(torch.int32))
        if ep >= 3:
            ev = tr.evaluate(torch.from_numpy(xt.reshape(-1, 784)), torch.from_numpy(yt),
                             torch.arange(len(yt), dtype=torch.int32))
            assert ev.count == len(yt)
            accs.append(ev.accuracy)
    assert max(accs) > 0.9 and accs[-1] > 0.8, (st, accs)


@pytest.mark.parametrize("model_name,dtype", [("lenet5", "fp32"), ("mlp", "fp32"), ("lenet5", "bf16"), ("mlp", "bf16")])
# 2048: the forward-only head runs 32-row tiles (128: 16-row tiles)
@pytest.mark.parametrize("batch", [128, 2048])
def test_eval_matches_torch(native, small_mnist, model_name, dtype, batch):
    """Forward-only eval loop (eval() semantics: no dropout) vs torch, over one full chunk of the trainer batch
    and a partial chunk of 300 rows.  bf16: the oracle sees the bf16-rounded inputs/weights; predictions may
    flip only on near-ties."""
    x, y, xt, yt = small_mnist
    # (a seed at which both models' fp32 oracle keeps every test row's top-2 logit margin above 1e-4, see below:
    #  MLP 8.5e-4, LeNet-5 3.2e-2 over all 1024 rows)
    torch.manual_seed(2084)
    module = build_model(model_name)
    tr = make_trainer(model_name, dtype, batch, x, y, module, dropout=0.2)
    n = batch + 300
    rows = torch.arange(n, dtype=torch.int32) % len(yt)
    ev = tr.evaluate(torch.from_numpy(xt.reshape(-1, 784)), torch.from_numpy(yt), rows)
    assert ev.count == n
    m = copy.deepcopy(module).eval()
    xx = _normalize(xt[rows.numpy()])
    if dtype == "bf16":
        xx = bf16_round(xx)
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() > 1:
                    p.copy_(bf16_round(p))
    with torch.no_grad():
        out = m(xx.view(n, 1, 28, 28) if model_name == "lenet5" else xx.view(n, -1))
        yy = torch.from_numpy(yt[rows.numpy()].astype(np.int64))
        loss = (F.nll_loss(out, yy, reduction="sum") if model_name == "lenet5"
                else F.cross_entropy(out, yy, reduction="sum")).item()
        corr = int((out.argmax(1) == yy).sum())
    if dtype == "fp32":
        # the exact count is a condition on the inputs: no evaluated row may be a near-tie of its two top logits
        top2 = out.topk(2, dim=1).values
        margin = float((top2[:, 0] - top2[:, 1]).min())
        assert margin > 1e-4, f"oracle's smallest top-2 logit margin {margin}: choose another seed"
        assert abs(ev.loss_sum - loss) / loss < 1e-4
        assert ev.correct == corr
    else:
        assert abs(ev.loss_sum - loss) / loss < 1e-2
        assert abs(ev.correct - corr) <= 3


def test_dropout_backward_matches_torch_with_kernel_mask(native, small_mnist):
    """Dropout ON (p=0.2): the oracle applies the kernel's own dropout mask (read back from h1T: kept
    units are scaled by 1.25, dropped ones are 0) in torch autograd; the gradients must match as in the
    p=0 test (fp32), so the backward through the dropout mask and its 1/(1-p) scale is checked."""
    x, y, _, _ = small_mnist
    torch.manual_seed(6)
    module = build_model("mlp")
    B = 256
    tr = make_trainer("mlp", "fp32", B, x, y, module, dropout=0.2)
    idx = torch.arange(B, dtype=torch.int32) * 7 % len(y)
    tr.set_epoch_indices(idx)
    tr.forward_backward(B)
    g = tr.grads()
    xb = x[idx.numpy()]
    m = copy.deepcopy(module).float().eval()
    with torch.no_grad():
        pre1 = m[0](_normalize(xb).view(B, -1))
    h1k = tr.h1T[:128, :B].float().cpu().T
    drop = torch.where(h1k > 0, torch.full_like(h1k, 1.25), torch.zeros_like(h1k))  # kernel: relu * mask * 1.25
    # torch's ReLU must agree with the kernel wherever the kernel kept the unit
    kept = h1k > 0
    assert ((pre1 > 0) | ~kept).all()
    assert 0.70 < kept.float().sum().item() / (pre1 > 0).float().sum().item() < 0.90
    h2mask = (tr.h2T[:128, :B].float().cpu().T > 0).float()
    gref, _, _ = torch_grads("mlp", module, xb, y[idx.numpy()], masks=[drop, h2mask])
    assert rel_err(g, gref) < 2e-4
    off = 0
    for k, v in module.state_dict().items():
        n = v.numel()
        assert rel_err(g[off:off + n], gref[off:off + n]) < 1e-3, k
        off += n


def test_dropout_statistics(native, small_mnist):
    """Native dropout keeps ~80% of units and scales by 1/(1-p): E[grad] matches p=0 on average."""
    x, y, _, _ = small_mnist
    torch.manual_seed(5)
    module = build_model("mlp")
    tr = make_trainer("mlp", "fp32", 512, x, y, module, dropout=0.2)
    tr.set_epoch_indices(torch.arange(512, dtype=torch.int32))
    tr.forward_backward(512)
    tr.synchronize()
    h1 = tr.h1T[:128, :512].float().cpu()
    # units with positive pre-activation: fraction zeroed by dropout ~ 0.2
    tr2 = make_trainer("mlp", "fp32", 512, x, y, module, dropout=0.0)
    tr2.set_epoch_indices(torch.arange(512, dtype=torch.int32))
    tr2.forward_backward(512)
    tr2.synchronize()
    h0 = tr2.h1T[:128, :512].float().cpu()
    pos = h0 > 0
    kept = (h1[pos] > 0).float().mean().item()
    assert 0.77 < kept < 0.83, kept
    ratio = (h1[pos & (h1 > 0)] / h0[pos & (h1 > 0)])
    assert torch.allclose(ratio, torch.full_like(ratio, 1.25), rtol=1e-5)
