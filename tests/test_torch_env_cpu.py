"""CPU: the torch-facing env (cage_challenge_4_amd/torch_env.py) without a GPU -- importing the package does not import torch, and
creating a CC4TorchVecEnv fails as loudly as creating a CC4VecEnv (no CPU fallback)."""
import subprocess
import sys
import pytest
from conftest import ROOT


def test_package_import_leaves_torch_out():
    code = ("import sys, cage_challenge_4_amd as c\n"
            "assert 'torch' not in sys.modules, 'importing the package imported torch'\n"
            "assert callable(c.CC4TorchVecEnv)\n"                     # the lazy attribute imports it on first use
            "assert 'torch' in sys.modules\n")
    pr = subprocess.run([sys.executable, '-c', code], cwd=ROOT, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr


def test_no_gpu_means_loud_failure(has_gpu):
    if has_gpu:
        pytest.skip('a GPU is visible')
    pytest.importorskip('torch')
    from cage_challenge_4_amd.torch_env import CC4TorchVecEnv
    from cage_challenge_4_amd._lib import CC4Error
    with pytest.raises(CC4Error, match='no HIP device'):
        CC4TorchVecEnv(4)
