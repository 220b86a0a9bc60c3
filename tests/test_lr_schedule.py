"""Learning-rate tables, the optimizer flags and the torch-CPU engine's side of them (no GPU)."""
import copy
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_ddp_mnist_amd.config import TrainConfig, configure, configure_gpu_tutorial, configure_simple
from pytorch_ddp_mnist_amd.data.datasets import normalize_batch
from pytorch_ddp_mnist_amd.data.synthetic import make_split
from pytorch_ddp_mnist_amd.engine import runner
from pytorch_ddp_mnist_amd.engine.reference import TorchCPUEngine
from pytorch_ddp_mnist_amd.models import build_model, flatten_state
from pytorch_ddp_mnist_amd.optim.schedule import build_lr_table, lr_at, validate_lr_table

BASE, T = 0.1, 37


def _torch_rates(make):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=BASE)
    sch = make(opt)
    out = []
    for _ in range(T):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sch.step()
    return np.asarray(out)


@pytest.mark.parametrize("kind,kw,make", [
    ("step", dict(step_size=5, gamma=0.5), lambda o: torch.optim.lr_scheduler.StepLR(o, step_size=5, gamma=0.5)),
    ("cosine", dict(lr_min=0.003), lambda o: torch.optim.lr_scheduler.CosineAnnealingLR(o, T_max=T, eta_min=0.003)),
    ("linear", dict(lr_min=0.02), lambda o: torch.optim.lr_scheduler.LinearLR(o, 1.0, 0.02 / BASE, total_iters=T)),
    ("constant", {}, lambda o: torch.optim.lr_scheduler.LambdaLR(o, lambda t: 1.0)),
])
def test_tables_match_torch_schedulers(kind, kw, make):
    table = build_lr_table(kind, BASE, T, **kw)
    ref = _torch_rates(make)
    assert table.dtype == np.float32 and table.shape == (T,)
    assert np.max(np.abs(table.astype(np.float64) - ref) / ref) < 1e-6


@pytest.mark.parametrize("kind", ["constant", "step", "cosine", "linear"])
def test_warmup_segment_is_its_formula(kind):
    W = 7
    table = build_lr_table(kind, BASE, T, warmup_steps=W, lr_min=0.01, step_size=4, gamma=0.5)
    for t in range(W):
        assert table[t] == np.float32(BASE * (t + 1) / W)
    assert table[W - 1] == np.float32(BASE) and table[W] == np.float32(BASE)  # u = 0: every kind starts at base_lr
    plain = build_lr_table(kind, BASE, T - W, lr_min=0.01, step_size=4, gamma=0.5)
    assert np.array_equal(table[W:], plain)  # after it: the schedule over the remaining U steps
    assert lr_at(table, 10 ** 6) == float(table[-1]) and lr_at(table, -3) == float(table[0])


def test_table_validation():
    for bad in ([], [0.1, float("inf")], [0.1, -1e-3], [[0.1]]):
        with pytest.raises(ValueError):
            validate_lr_table(bad)
    assert validate_lr_table(torch.tensor([0.5, 0.25])).tolist() == [0.5, 0.25]
    with pytest.raises(ValueError):
        build_lr_table("step", 0.1, 10)  # no step_size
    with pytest.raises(ValueError):
        build_lr_table("exp", 0.1, 10)
    with pytest.raises(ValueError):
        build_lr_table("cosine", 0.1, 0)


FLAGS = ["--weight_decay", "0.05", "--nesterov", "--momentum", "0.9", "--lr_schedule", "cosine", "--warmup_steps", "5",
         "--lr_min", "0.001", "--lr_step_size", "3", "--lr_gamma", "0.5"]


@pytest.mark.parametrize("conf", [configure, configure_simple, configure_gpu_tutorial])
def test_flags_parse_into_config(conf):
    c = conf(FLAGS)
    assert (c.weight_decay, c.nesterov, c.lr_schedule, c.warmup_steps, c.lr_min, c.lr_step_size, c.lr_gamma) == \
        (0.05, True, "cosine", 5, 0.001, 3, 0.5)
    d = conf([])
    assert (d.weight_decay, d.nesterov, d.lr_schedule, d.warmup_steps, d.lr_min, d.lr_step_size, d.lr_gamma) == \
        (0.0, False, None, 0, 0.0, None, 0.1)
    assert runner.schedule_table(d, 60000, 1) is None
    # n_epochs x this rank's steps per epoch, the partial last step included: ceil(ceil(1000 / 3) / 128) = 3
    c.n_epochs, c.batch_size = 4, 128
    assert len(runner.schedule_table(c, 1000, 3)) == 12


def _cfg(tmp_path, **kw):
    c = TrainConfig(model="mlp", dropout=0.0, momentum=0.9, lr=0.05, device="cpu", data_format="synthetic",
                    data_limit=256, batch_size=128, save_path=None, init_seed=0)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_runner_installs_the_schedule_only_when_asked(tmp_path, monkeypatch, capsys):
    calls = []
    orig = TorchCPUEngine.set_lr_schedule
    monkeypatch.setattr(TorchCPUEngine, "set_lr_schedule", lambda self, t: (calls.append(len(t)), orig(self, t))[1])
    out = runner.run(_cfg(tmp_path))
    assert calls == [] and "lr" not in out["history"][0]
    resume, jl = str(tmp_path / "r.pt"), str(tmp_path / "m.jsonl")
    on = dict(weight_decay=0.05, nesterov=True, lr_schedule="linear", lr_min=0.01, resume=resume, metrics_jsonl=jl)
    out = runner.run(_cfg(tmp_path, n_epochs=2, **on))
    assert calls == [4]  # 2 epochs x 2 steps
    table = build_lr_table("linear", 0.05, 4, lr_min=0.01)
    assert [h["lr"] for h in out["history"]] == [float(table[1]), float(table[3])]
    recs = [json.loads(line) for line in open(jl)]
    assert [r["lr"] for r in recs] == [float(table[1]), float(table[3])]
    blob = torch.load(resume, weights_only=True)
    assert blob["optimizer"] == runner.optimizer_options(_cfg(tmp_path, **on)) and blob["global_step"] == 4
    capsys.readouterr()
    runner.run(_cfg(tmp_path, n_epochs=3, **dict(on, weight_decay=0.0)))  # resumes epoch 2 with another option
    assert "WARNING" in capsys.readouterr().out and "weight_decay" in repr(blob["optimizer"])
    with pytest.raises(ValueError):
        runner.run(_cfg(tmp_path, momentum=0.0, nesterov=True))


MU, WD = 0.9, 0.05
TABLE = [0.02, 0.005, 0.04, 0.01]


def _engine(module, x, y, **kw):
    return TorchCPUEngine("mlp", 128, 0.05, MU, 0.0, x, y, x[:128], y[:128], init=copy.deepcopy(module), **kw)


def test_cpu_engine_is_torch_sgd_with_the_options():
    B = 128
    x, y = make_split(4 * B, seed=7)
    torch.manual_seed(0)
    module = build_model("mlp")
    module[2].p = 0.0
    eng = _engine(module, x, y, weight_decay=WD, nesterov=True, lr_schedule=TABLE)
    eng.train_epoch(torch.arange(4 * B))
    ref = copy.deepcopy(module).train()
    opt = torch.optim.SGD(ref.parameters(), lr=0.05, momentum=MU, weight_decay=WD, nesterov=True)
    xs = normalize_batch(torch.from_numpy(np.ascontiguousarray(x))).reshape(-1, 784)
    ys = torch.from_numpy(y.astype(np.int64))
    table = np.asarray(TABLE, dtype=np.float32)
    for s in range(4):
        for g in opt.param_groups:
            g["lr"] = float(table[s])
        opt.zero_grad()
        F.cross_entropy(ref(xs[s * B:(s + 1) * B]), ys[s * B:(s + 1) * B]).backward()
        opt.step()
    a, b = flatten_state(eng.module).double(), flatten_state(ref).double()
    assert float((a - b).norm() / b.norm()) < 1e-6
    assert eng.current_lr() == float(table[3]) and eng.global_step == 4
    # and the options matter: the plain recurrence ends elsewhere
    plain = _engine(module, x, y)
    plain.train_epoch(torch.arange(4 * B))
    assert float((flatten_state(plain.module).double() - b).norm() / b.norm()) > 1e-4


def test_cpu_resume_continues_the_schedule():
    B = 128
    x, y = make_split(4 * B, seed=7)
    torch.manual_seed(0)
    module = build_model("mlp")
    kw = dict(weight_decay=WD, nesterov=True, lr_schedule=TABLE)
    straight = _engine(module, x, y, **kw)
    straight.train_epoch(torch.arange(4 * B))
    first = _engine(module, x, y, **kw)
    first.train_epoch(torch.arange(2 * B))
    params, mom, gstep = first.get_state()
    assert gstep == 2
    resumed = _engine(build_model("mlp"), x, y, **kw)
    resumed.set_state(params, mom, gstep)
    resumed.train_epoch(torch.arange(2 * B, 4 * B))
    a, b = flatten_state(resumed.module).double(), flatten_state(straight.module).double()
    assert float((a - b).norm() / b.norm()) < 1e-6
    assert resumed.current_lr() == float(np.float32(TABLE[3]))


def test_nesterov_without_momentum_raises():
    x, y = make_split(256, seed=7)
    with pytest.raises(ValueError):
        TorchCPUEngine("mlp", 128, 0.05, 0.0, 0.0, x, y, x, y, nesterov=True)
    with pytest.raises(ValueError):
        TorchCPUEngine("mlp", 128, 0.05, 0.9, 0.0, x, y, x, y, weight_decay=-0.5)
    from pytorch_ddp_mnist_amd.optim.schedule import check_sgd_options
    with pytest.raises(ValueError):
        check_sgd_options(0.0, 0.0, True)
    check_sgd_options(0.9, 0.05, True)
