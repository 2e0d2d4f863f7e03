"""What the tensor-taking surfaces of the binding share (torch_env, action_logp, advantages; the logits of CC4VecEnv.sample_actions): the dtype
codes of the entry points, one check of a caller's tensor, and the call of a pure entry point on torch's current stream.  Importing this module
imports neither torch nor the library: the functions take the torch module, or import it when they are called."""
import ctypes
import numpy as np

# ---- the dtype codes of cc4_policy_outputs and of every entry point that takes logits or values (include/cc4.h): stated here once
DTYPE_CODES = {'float16': 1, 'bfloat16': 2, 'float32': 3}
OBS_DTYPE_CODES = {'uint8': 0, **DTYPE_CODES}              # observations also come as the bytes they are
ELEM_BYTES = {'uint8': 1, 'float16': 2, 'bfloat16': 2, 'float32': 4}
# NumPy has no bfloat16: uint16 stands for its bit patterns
NUMPY_CODES = {np.dtype('uint16' if k == 'bfloat16' else k): c for k, c in DTYPE_CODES.items()}


def torch_codes(torch, table=DTYPE_CODES):      # the table keyed by torch dtypes
    return {getattr(torch, k): c for k, c in table.items()}


def check_tensor(torch, name, x, *, shape=None, dtypes=None, device=None, contiguous=True):
    """x, or a ValueError that names it.  In this order: x is a torch tensor; its shape (a tuple; None: any extent);
    its dtype is one of dtypes; it is contiguous and on the kind of device asked for ('cuda', or a torch.device); it is on
    that very device (a device with an index).  shape, dtypes, device None and contiguous False skip their checks, so a caller that orders the
    checks of several tensors -- all kinds before any shape, say -- calls once per stage."""
    if not torch.is_tensor(x):
        raise ValueError(f'{name} must be a torch tensor, got {type(x).__name__}')
    if shape is not None and (x.dim() != len(shape) or any(w is not None and w != g for w, g in zip(shape, x.shape))):
        raise ValueError(f'{name} must have shape [{", ".join("k" if w is None else str(w) for w in shape)}], got {list(x.shape)}')
    if dtypes is not None and x.dtype not in dtypes:
        names = [str(d).replace('torch.', '') for d in dtypes]
        raise ValueError(f'{name} must be {", ".join(names[:-1])}{" or " if names[:-1] else ""}{names[-1]}, got {x.dtype}')
    where = None if device is None else torch.device(device)
    if (where is not None and x.device.type != where.type) or (contiguous and not x.is_contiguous()):
        kind = '' if where is None else ('CUDA ' if where.type == 'cuda' else where.type + ' ')
        raise ValueError(f'{name} must be a {"contiguous " if contiguous else ""}{kind}tensor')
    if where is not None and where.index is not None and x.device != where:
        raise ValueError(f'{name} must be on {where}, got {x.device}')
    return x


def dptr(t):      # the device address of a tensor as the entry points take it; None stays None (an optional argument)
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def pure_call(entry, device, *args, count=None):
    """One pure entry point of the library (no handle: its first argument is the stream) on torch's current stream of `device`, with that device
    current: rc != 0 raises CC4Error.  count: (launches, key) of the caller's launch counter, advanced by one."""
    import torch
    from . import _lib as L
    with torch.cuda.device(device):
        rc = getattr(L.load(), entry)(ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream), *args)
    if rc != 0:
        raise L.CC4Error(f'{entry} failed (rc={rc})')
    if count is not None:
        count[0][count[1]] += 1
