"""The opt-in split-K-in-workgroup FC weight gradient (head.hip wgrad_sk_kernel, ``MNIST_AMD_WGRAD_SK=1``) against
the torch oracle.  The switch is read once per process, so the comparison runs in a child process
(tests/_wgrad_sk_child.py: batch 2048 / 4096 and a 2085-row partial batch, both models, fp32 and bf16; a second
child with ``MNIST_AMD_WGRAD_SK_PF=4``, bf16 at batch 2048)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(env_extra, *args):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("MNIST_AMD_WGRAD_SK_PF", None)  # (the child checks that it sees exactly what this test set)
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_wgrad_sk_child.py"), *args], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:]
    m = re.search(r"wgrad_sk_mode (-?\d+)", r.stdout)
    assert m and int(m.group(1)) == 1, r.stdout[-3000:]
    return r.stdout


def test_wgrad_sk_matches_torch(native):
    out = _child({"MNIST_AMD_WGRAD_SK": "1"})
    assert len(re.findall(r"^sk \S+: total", out, re.M)) == 12  # 3 shapes x 2 models x 2 dtypes
    assert "wgrad_sk child: 0 misses" in out


def test_wgrad_sk_pf4_matches_torch(native):
    out = _child({"MNIST_AMD_WGRAD_SK": "1", "MNIST_AMD_WGRAD_SK_PF": "4"}, "--pf4")
    assert len(re.findall(r"^sk/pf4 \S+: total", out, re.M)) == 2  # batch 2048, bf16, 2 models
    assert "wgrad_sk child: 0 misses" in out
