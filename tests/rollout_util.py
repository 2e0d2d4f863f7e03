"""numpy restatements the rollout tests check the device against: the packed observation rows a rollout's policy reads, and the 'hash'
stand-in policy that computes its actions from them."""
import numpy as np


def pack_rows(obs):
    """[n, 578] observation values (0 / 1 / 2) -> [n, 148] bytes, 2 bits per value, low bits first (CC4_OBS_PACKED_BYTES)."""
    n = obs.shape[0]
    v = np.zeros((n, 592), np.uint8)
    v[:, :578] = obs.astype(np.uint8) & 3
    v = v.reshape(n, 148, 4)
    return (v[:, :, 0] | (v[:, :, 1] << 2) | (v[:, :, 2] << 4) | (v[:, :, 3] << 6)).astype(np.uint8)


def hash_policy(packed, j):
    """numpy restatement of k_rollout_hash_policy (csrc/cc4_k_misc.hip): FNV-1a over the 37 words of an episode's packed observation row."""
    w = np.ascontiguousarray(packed).view('<u4').astype(np.uint64)          # [n, 37]
    h = np.full(w.shape[0], 2166136261, np.uint64)
    for c in range(w.shape[1]):
        h = ((h ^ w[:, c]) * np.uint64(16777619)) & np.uint64(0xFFFFFFFF)
    out = np.zeros((w.shape[0], 5), np.int32)
    for b in range(5):
        out[:, b] = ((h + np.uint64(2654435761 * (b + 1)) + np.uint64(40503 * j)) & np.uint64(0xFFFFFFFF)) % np.uint64(242 if b == 4 else 82)
    return out
