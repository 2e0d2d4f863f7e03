"""CPU: the Python surface of the episode copies -- fault names, and the torch env's argument checks that run before anything reaches the device."""
import pytest


def test_copy_fault_bits_are_named():
    from cage_challenge_4_amd.vec_env import CC4EngineError, raise_on_copy_faults
    raise_on_copy_faults(0)
    with pytest.raises(CC4EngineError) as got:
        raise_on_copy_faults(1 | 4 | 16)
    msg = str(got.value)
    assert 'INDEX_OUT_OF_RANGE' in msg and 'SOURCE_IS_DESTINATION' in msg and 'SLOT_OF_ANOTHER_CONFIGURATION' in msg
    assert 'DUPLICATED_DESTINATION' not in msg and 'SLOT_NEVER_WRITTEN' not in msg


def test_header_fault_bits_match_the_binding():
    import os
    import re
    from conftest import ROOT
    from cage_challenge_4_amd.vec_env import COPY_FAULT_NAMES
    txt = open(os.path.join(ROOT, 'include', 'cc4.h')).read()
    bits = {name: int(v) for name, v in re.findall(r'#define CC4_COPY_([A-Z_]+) (\d+)', txt)}
    assert sorted(bits.values()) == [1 << i for i in sorted(COPY_FAULT_NAMES)]


def test_torch_env_has_the_copy_surface():
    torch_env = pytest.importorskip('cage_challenge_4_amd.torch_env')
    for name in ('new_bank', 'clone_episodes', 'save_episodes', 'load_episodes', 'snapshot_bytes'):
        assert hasattr(torch_env.CC4TorchVecEnv, name), name
