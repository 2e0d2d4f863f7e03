"""bfloat16 for the tests, which NumPy does not have: bit patterns as uint16 (what sample_util, gae_util and test_logp_device hand the device)."""
import numpy as np


def to_bits(x):
    """float32 values -> bfloat16 bit patterns (uint16), rounded to nearest, ties to even; a NaN becomes the quiet NaN 0x7FC0."""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    return np.where(np.isnan(x), np.uint16(0x7FC0), r)


def upcast(arr):
    """What an array of bfloat16 bit patterns (uint16), float16 or float32 carries, as float32 -- exactly."""
    arr = np.asarray(arr)
    if arr.dtype == np.uint16:
        return (arr.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return arr.astype(np.float32)
