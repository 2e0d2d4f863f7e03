"""What the GPU tests of the derived views (state features, red view, blue view, blue edges, reward terms) share: a device allocation without
torch, a handle, the fault word, and one "call a view into a fresh device buffer, synchronise, copy down"."""
import ctypes

import numpy as np

from cage_challenge_4_amd.vec_env import _hip

VP = ctypes.c_void_p


class DevMem:
    """A device allocation through the HIP runtime libcc4.so is linked against (no torch in this file)."""

    def __init__(self, nbytes, fill=0):
        self.hip, self.nbytes, self.p = _hip(), int(nbytes), VP()
        self.hip.hipMemset.argtypes, self.hip.hipMemset.restype = [VP, ctypes.c_int, ctypes.c_size_t], ctypes.c_int
        assert self.hip.hipMalloc(ctypes.byref(self.p), max(self.nbytes, 16)) == 0
        assert self.hip.hipMemset(self.p, fill, max(self.nbytes, 16)) == 0

    def at(self, off):
        assert 0 <= off <= self.nbytes
        return VP(self.p.value + off)

    def up(self, arr, off=0):
        arr = np.ascontiguousarray(arr)
        assert off + arr.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(self.at(off), arr.ctypes.data_as(VP), arr.nbytes, 1) == 0

    def down(self, dtype, shape, off=0):
        out = np.zeros(shape, dtype)
        assert off + out.nbytes <= self.nbytes
        assert self.hip.hipMemcpy(out.ctypes.data_as(VP), self.at(off), out.nbytes, 2) == 0
        return out

    def free(self):
        if self.p:
            self.hip.hipFree(self.p)
            self.p = VP()


def _dev(n, **kw):
    from cage_challenge_4_amd import CC4VecEnv
    return CC4VecEnv(n, **kw)


def _faults(dev):
    f = ctypes.c_uint32(0)
    dev._chk(dev.lib.cc4_copy_faults(dev._h, ctypes.byref(f)), 'cc4_copy_faults')
    return f.value


def call_view(dev, call, n, parts, ids=None, bank=None, cap=0, fill=0, out=None, second=True):
    """A view of n entries into a fresh (or the given) device buffer [first | second], every byte `fill` before the call, then synchronise and
    copy down.  call(d_bank, cap, d_ids, n, p_first, p_second) makes the call; parts: (dtype, shape of one entry) of the two outputs; ids: the
    entries (None: 0 .. n-1) -- episodes, or with bank (a DevMem) and cap its slots; second=False passes no second output."""
    nb = [n * int(np.prod(shape)) * np.dtype(dt).itemsize for dt, shape in parts]
    buf = out or DevMem(sum(nb), fill)
    assert buf.hip.hipDeviceSynchronize() == 0          # the fill runs on the null stream, the kernel on the handle's: the fill first
    d_ids = None
    if ids is not None:
        d_ids = DevMem(4 * max(len(ids), 1))
        d_ids.up(np.asarray(ids, np.int32))
    call(bank.p if bank is not None else None, cap, d_ids.p if d_ids else None, n, buf.p, buf.at(nb[0]) if second else None)
    dev.synchronize()
    a, b = buf.down(parts[0][0], (n,) + tuple(parts[0][1])), buf.down(parts[1][0], (n,) + tuple(parts[1][1]), nb[0])
    if d_ids:
        d_ids.free()
    if out is None:
        buf.free()
    return a, b
