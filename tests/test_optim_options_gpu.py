"""Weight decay, Nesterov momentum and an in-graph per-step learning rate on every update path.

(a) ``test_each_update_matches_recurrence``: the method of ``test_update_oracle_gpu.py`` -- around EACH step the
momentum and the parameters are compared with torch.optim.SGD's recurrence (dampening 0) in float64,

    g = g_ref(p_s) + wd * p_s      m_exp = mu * m_s + g      p_exp = p_s - lr_s * (g + mu * m_exp)

where g_ref is the torch oracle's gradient at the parameters p_s the step started from and lr_s the schedule's
entry for the step.  Four steps replay ONE captured single-step graph while the rate moves by at least 2x per step
in both directions, so a rate baked into the graph, published a step early or late, or read by one update kernel
before the head stored it shows as a parameter error of at least lr_s / 2 * |d| (the bound is lr_s * tol * |g_ref|,
tol <= 2e-2).  Bounds, from that file's: an error of tol * |g_ref| in the gradient is one of tol * |g_ref| in the
momentum and, because the Nesterov direction is g + mu * m, of (1 + mu) * tol * |g_ref| in the direction; 2^-22 * |.|
covers the fp32 rounding of the update itself.  The test also shows that it discriminates: for every layer the
measured momentum is farther from the recurrence WITHOUT weight decay than that layer's bound.

Measured on an MI355X, worst step, error / bound for momentum | parameters (whole vector; worst layer) and the
smallest distance-from-wd-off / bound of any layer: lenet5 bf16 4096 0.001 | 0.028 (0.001 | 0.027), 19x (11.bias);
lenet5 fp32 2048 0.414 | 0.107 (0.460 | 0.138), 259x; lenet5 bf16 128 0.002 | 0.016 (0.004 | 0.031), 4.6x (11.bias);
mlp fp32 128 0.002 | 0.089 (0.001 | 0.070), 602x; mlp bf16 4096 0.001 | 0.010 (0.001 | 0.011), 44x; the 76-row
eager step: lenet5 bf16 0.440 | 0.431, mlp fp32 0.002 | 0.089 (profiles/optim_options/NOTES.md).

(b) a table of equal entries is bitwise the constant rate; (c) every schedule (serial, concurrent, k-step graphs with
the deferred join, JOIN, SPLIT, bucket groups, OVERLAP) gives bitwise the same parameters with the options on;
(d) a resumed run continues the schedule bitwise; (e) no store outside the buffers with a schedule installed.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pytorch_ddp_mnist_amd.models import build_model
from test_native_gpu import check_masks_against_torch, kernel_relu_masks, make_trainer, torch_grads
from test_stale_state_gpu import TOLS, assert_pack_is_image_of_params
from test_update_oracle_gpu import ROUND, layer_slices, module_at

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MU, WD = 0.9, 0.05
TABLE = [0.02, 0.005, 0.04, 0.01]  # non-monotonic, neighbours >= 2x apart
OPTS = dict(momentum=MU, weight_decay=WD, nesterov=True, lr_schedule=TABLE)

# (model, dtype, batch): the smallest batch that reaches each publish / update path
CASES = [
    ("lenet5", "bf16", 4096),  # fwd_head_kernel publishes; reduce_sgd_direct on aux; reduce_sgd over the conv slab
    ("lenet5", "fp32", 2048),  # head_kernel
    ("lenet5", "bf16", 128),   # head16 + conv_bwd_fc epilogue
    ("mlp", "fp32", 128),      # l1_split + head_kernel + wgrad_sgd epilogue
    ("mlp", "bf16", 4096),     # split wgrad + reduce
]


def expected(p_s, m_s, g_ref, lr, mu=MU, wd=WD, nesterov=True):
    """torch.optim.SGD(lr, mu, dampening=0, weight_decay=wd, nesterov) on flat vectors, float64."""
    g = g_ref.double() + wd * p_s.double()
    m = mu * m_s.double() + g
    d = g + mu * m if nesterov else m
    return m, p_s.double() - lr * d


def run_and_check(tr, twin, model_name, dtype, x, y, idx, steps, tag):
    """``steps``: [(rows, use_graph)] run one by one on ``tr`` (batch = tr.batch), each against the recurrence.
    Returns the worst whole-vector error / bound ratios (momentum, parameters)."""
    tol, layer_tol = TOLS[dtype]
    bf = dtype == "bf16"
    table = np.asarray(TABLE, dtype=np.float32)
    slices = layer_slices(build_model(model_name))
    worst_m = worst_p = 0.0
    off = 0
    for s, (rows_n, use_graph) in enumerate(steps):
        tr.synchronize()
        p_s, m_s = tr.params.cpu().clone(), tr.mom.cpu().clone()
        tr.step(rows_n, use_graph=use_graph)
        tr.synchronize()
        p_n, m_n = tr.params.cpu().clone(), tr.mom.cpu().clone()
        lr_s = float(table[min(s, len(table) - 1)])
        assert tr.current_lr() == lr_s, f"{tag} step {s}: published rate {tr.current_lr()} != table[{s}] = {lr_s}"
        rows = idx[off:off + rows_n].numpy()
        off += tr.batch
        at = module_at(model_name, p_s)
        masks = None
        if model_name == "mlp":
            masks = kernel_relu_masks(tr, rows_n)
            check_masks_against_torch(at, x[rows], masks, bf)
        g_ref, _, _ = torch_grads(model_name, at, x[rows], y[rows], masks, bf16_inputs=bf)
        m_exp, p_exp = expected(p_s, m_s, g_ref, lr_s)
        m_off, _ = expected(p_s, m_s, g_ref, lr_s, wd=0.0)  # the recurrence without the feature, same g_ref
        report, failed, blind = [], [], []
        for k, sl in slices:
            t = tol if k == "all" else layer_tol
            gn = float(g_ref[sl].double().norm())
            em, bm = float((m_n[sl].double() - m_exp[sl]).norm()), t * gn + ROUND * float(m_exp[sl].norm())
            ep = float((p_n[sl].double() - p_exp[sl]).norm())
            bp = lr_s * (1.0 + MU) * t * gn + ROUND * float(p_exp[sl].norm())
            doff = float((m_n[sl].double() - m_off[sl]).norm())
            report.append(f"{k}: mom {em:.2e}/{bm:.2e} par {ep:.2e}/{bp:.2e} off {doff:.2e}")
            if not (em <= bm and ep <= bp):
                failed.append(report[-1])
            if not doff > bm:
                blind.append(report[-1])
            if k == "all":
                worst_m, worst_p = max(worst_m, em / bm), max(worst_p, ep / bp)
        print(f"{tag} step {s} lr {lr_s} (error/bound, distance from the wd = 0 recurrence) " + "  ".join(report))
        assert not failed, f"{tag} step {s}: {failed}"
        assert not blind, f"{tag} step {s}: the bound does not separate weight decay on from off: {blind}"
        assert float((p_n - p_s).norm()) > 0.0
        assert_pack_is_image_of_params(tr, twin)
    print(f"{tag}: worst error/bound whole vector: momentum {worst_m:.3f} parameters {worst_p:.3f}")
    return worst_m, worst_p


@pytest.mark.parametrize("model_name,dtype,batch", CASES)
def test_each_update_matches_recurrence(native, small_mnist, model_name, dtype, batch):
    x, y, _, _ = small_mnist
    steps = len(TABLE)
    torch.manual_seed(0)
    module = build_model(model_name)
    tr = make_trainer(model_name, dtype, batch, x, y, module, max_indices=steps * batch, **OPTS)
    twin = make_trainer(model_name, dtype, batch, x, y, module, max_indices=steps * batch)  # launch_pack of tr's parameters
    idx = torch.arange(steps * batch, dtype=torch.int32) * 3 % len(y)
    tr.set_epoch_indices(idx)
    run_and_check(tr, twin, model_name, dtype, x, y, idx, [(batch, True)] * steps, f"{model_name}/{dtype}/B={batch}")
    assert tr.rt.captured  # the four steps replayed the one single-step graph


@pytest.mark.parametrize("model_name,dtype", [("lenet5", "bf16"), ("mlp", "fp32")])
def test_partial_batch_step_publishes(native, small_mnist, model_name, dtype):
    """train_epoch over 2 * 128 + 76 rows: two graph replays and the eager partial-batch step, which must publish
    its own rate (table[2], 8x the one before).  The same three steps run one by one against the recurrence on a
    second trainer; the epoch's result is bitwise that."""
    x, y, _, _ = small_mnist
    batch, tail = 128, 76
    n = 2 * batch + tail
    torch.manual_seed(0)
    module = build_model(model_name)
    idx = torch.arange(n, dtype=torch.int32) * 3 % len(y)
    ep = make_trainer(model_name, dtype, batch, x, y, module, max_indices=n, **OPTS)
    ep.train_epoch(idx, use_graph=True)
    assert ep.current_lr() == float(np.float32(TABLE[2]))
    tr = make_trainer(model_name, dtype, batch, x, y, module, max_indices=n, **OPTS)
    twin = make_trainer(model_name, dtype, batch, x, y, module, max_indices=n)
    tr.set_epoch_indices(idx)
    run_and_check(tr, twin, model_name, dtype, x, y, idx, [(batch, True), (batch, True), (tail, False)],
                  f"{model_name}/{dtype}/B={batch}+{tail}")
    assert torch.equal(ep.params, tr.params) and torch.equal(ep.mom, tr.mom)


@pytest.mark.parametrize("model_name,dtype", [("lenet5", "bf16"), ("mlp", "fp32")])
def test_equal_entries_are_the_constant_rate(native, small_mnist, model_name, dtype):
    """(b) and the table's plumbing: same-length contents keep the captured graph, evaluation does not publish."""
    x, y, xt, yt = small_mnist
    batch, steps, lr = 128, 4, 0.05
    torch.manual_seed(0)
    module = build_model(model_name)
    idx = torch.arange(steps * batch, dtype=torch.int32) * 3 % len(y)
    kw = dict(lr=lr, momentum=MU, max_indices=steps * batch)
    plain = make_trainer(model_name, dtype, batch, x, y, module, **kw)
    sched = make_trainer(model_name, dtype, batch, x, y, module, lr_schedule=[lr] * steps, **kw)
    assert plain.current_lr() == lr and not plain.rt.has_lr_table and sched.rt.has_lr_table
    for tr in (plain, sched):
        tr.set_epoch_indices(idx)
        for _ in range(steps):
            tr.step(batch, use_graph=True)
        tr.synchronize()
    assert torch.equal(plain.params, sched.params) and torch.equal(plain.mom, sched.mom)
    assert sched.current_lr() == float(np.float32(lr))
    # new rates at the same address: the graph stays; another length: it is dropped
    ptr = sched.lr_table.data_ptr()
    sched.set_lr_schedule(torch.tensor([0.5, 0.25, 0.125, 0.0625]))
    assert sched.rt.captured and sched.lr_table.data_ptr() == ptr
    assert sched.current_lr() == 0.0625  # global step 4: the last entry, until the next head publishes
    with torch.cuda.stream(sched.stream):
        sched.lr_now.fill_(-1.0)
    sched.evaluate(torch.from_numpy(xt.reshape(-1, 784)), torch.from_numpy(yt), torch.arange(300, dtype=torch.int32))
    assert sched.current_lr() == -1.0  # eval_batch left the cell alone
    sched.set_lr_schedule([0.1, 0.2])
    assert not sched.rt.captured
    sched.set_lr_schedule(None)
    assert sched.current_lr() == lr and not sched.rt.has_lr_table


def test_option_errors(native, small_mnist):
    x, y, _, _ = small_mnist
    module = build_model("mlp")
    with pytest.raises(ValueError):
        make_trainer("mlp", "fp32", 128, x, y, module, momentum=0.0, nesterov=True)
    with pytest.raises(ValueError):
        make_trainer("mlp", "fp32", 128, x, y, module, weight_decay=-0.1)
    tr = make_trainer("mlp", "fp32", 128, x, y, module)
    with pytest.raises(ValueError):
        tr.rt.set_optimizer(0.1, 0.0, 0.0, True)
    with pytest.raises(ValueError):
        tr.rt.set_optimizer(0.1, 0.9, -1.0, False)
    for bad in ([], [0.1, float("nan")], [0.1, -0.1], [[0.1, 0.2]]):
        with pytest.raises(ValueError):
            tr.set_lr_schedule(bad)
    assert tr.lr_table is None


def _digests(env_extra, variants, model, extra):
    env = dict(os.environ, PYTHONPATH=ROOT, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "sched_equiv.py"), "--model", model, *extra] + variants,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    return dict(re.findall(r"digest (\S+) (\w+)", r.stdout))


ON = ("--weight_decay", str(WD), "--nesterov", "--lr_table", ",".join(str(t) for t in TABLE))


@pytest.mark.timeout(900)  # fresh interpreters (torch import + GPU init each)
def test_schedules_agree_with_options_on(native):
    serial = _digests({"MNIST_AMD_CONCURRENT": "0"}, ["local"], "lenet5", ON)
    d = _digests({"MNIST_AMD_CONCURRENT": "1"}, ["local", "local_k4", "join", "split", "split_g0.1.2", "overlap"], "lenet5", ON)
    for k in ("local", "local_k4", "join", "split", "split_g0.1.2", "overlap"):
        assert d[k] == serial["local"], k
    m = _digests({}, ["local", "join", "split", "split_k4"], "mlp", ON)
    for k in ("join", "split", "split_k4"):
        assert m[k] == m["local"], k
    # Nesterov + table only: the 1/W of two ranks is a local run at half the rates (x 0.5 is exact)
    h = _digests({}, ["join_w2", "local_halflr"], "lenet5", ("--weight_decay", "0") + ON[2:])
    assert h["join_w2"] == h["local_halflr"]
    # the options reach the digests at all
    off = _digests({"MNIST_AMD_CONCURRENT": "0"}, ["local"], "lenet5", ())
    assert off["local"] != serial["local"]


def test_resume_continues_the_schedule(native, small_mnist):
    x, y, _, _ = small_mnist
    model_name, dtype, batch = "mlp", "fp32", 128
    torch.manual_seed(0)
    module = build_model(model_name)
    idx = torch.arange(4 * batch, dtype=torch.int32) * 3 % len(y)
    kw = dict(max_indices=4 * batch, **OPTS)
    straight = make_trainer(model_name, dtype, batch, x, y, module, **kw)
    straight.set_epoch_indices(idx)
    for _ in range(4):
        straight.step(batch, use_graph=True)
    first = make_trainer(model_name, dtype, batch, x, y, module, **kw)
    first.set_epoch_indices(idx)
    for _ in range(2):
        first.step(batch, use_graph=True)
    params, mom, gstep = first.get_state()
    assert gstep == 2
    resumed = make_trainer(model_name, dtype, batch, x, y, build_model(model_name), **kw)
    resumed.set_state(params, mom, gstep)
    resumed.set_epoch_indices(idx[2 * batch:])
    for s in range(2):
        resumed.step(batch, use_graph=True)
        assert resumed.current_lr() == float(np.float32(TABLE[2 + s]))
    straight.synchronize()
    assert torch.equal(straight.params, resumed.params) and torch.equal(straight.mom, resumed.mom)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("batch", [128, 4096])
def test_no_store_outside_buffers_with_a_schedule(native, monkeypatch, batch):
    from pytorch_ddp_mnist_amd.data.synthetic import make_split
    from pytorch_ddp_mnist_amd.engine.native import GUARD_BYTES, NativeTrainer

    monkeypatch.setenv("MNIST_AMD_GUARD", "1")
    n = 3 * batch + batch // 3 + 1  # three full batches and a partial one
    x, y = make_split(max(n, 1024), seed=3)
    xt, yt = make_split(1000, seed=4)
    tr = NativeTrainer("lenet5", "bf16", batch, torch.from_numpy(x.reshape(-1, 784)), torch.from_numpy(y), dropout=0.0,
                       init=build_model("lenet5"), **OPTS)
    guarded = {raw.data_ptr() + GUARD_BYTES for raw, _ in tr._guards}
    assert tr.lr_table.data_ptr() in guarded and tr.lr_now.data_ptr() in guarded
    for epoch in range(2):
        g = torch.Generator().manual_seed(epoch)
        tr.train_epoch(torch.randperm(x.shape[0], generator=g)[:n].to(torch.int32), use_graph=True)
    tr.evaluate(torch.from_numpy(xt.reshape(-1, 784)), torch.from_numpy(yt), torch.arange(1000, dtype=torch.int32))
    assert tr.check_guards() == []
    assert torch.isfinite(tr.params).all()
    assert tr.current_lr() == float(np.float32(TABLE[-1]))  # 8 steps: past the table's end
    tr.close()
