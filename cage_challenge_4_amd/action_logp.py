"""Log-probability and entropy of STORED blue actions under new logits, with the gradient back to the logits (include/cc4.h,
cc4_logp_actions_device): the second half of a PPO / A2C iteration, the definition of action_sampling with the draw left out plus its derivative.
A pure function of tensors -- the logits the updated network gives now, the action-mask rows and the actions the rollout stored; an action of -1
("submitted nothing": what sample_actions gives a busy agent) is skipped -- so it needs no env.

Per agent b with the valid slots of its segment: x = logits / temperature, logp = log softmax(x over the valid slots)[action], entropy of that
softmax; skipped (action -1): zero, gradient zero; refused (a NaN or +inf among the valid logits, all of them -inf, no valid slot, an action
outside the segment or on an invalid slot): logp = entropy = 0, gradient zero, and check_errors() raises.

Three ways to the same numbers:
  evaluate_actions(logits, mask, actions, temperature)   the HIP kernels over the batch (k_logp_fwd, k_logp_bwd) under torch autograd, float32
  from_rows(logits, mask, actions, temperature, g)       the same definition compiled for the host (cc4_logp_actions_host, ..._grad_host), no GPU
  reference(logits, mask, actions, temperature, g)       a NumPy restatement in float64

Importing this module imports neither torch nor the library; evaluate_actions() and check_errors() import torch when they are called."""
import ctypes
import numpy as np
from . import _lib as L
from . import _tensors as TS
from .action_sampling import NUM_BLUE, SEGMENTS, SLOTS, check_temperature

REFUSED = L.LOGP_REFUSED
AUX = {'logp': 0, 'entropy': 1, 'm': 2, 'logS': 3}
DTYPE_CODES = TS.DTYPE_CODES      # the codes of cc4_policy_outputs
launches = {'fwd': 0, 'bwd': 0}          # kernels this module has enqueued (what a caller's test counts)


def _rows(logits, mask, actions, g=None):
    lg, mk, ac = np.asarray(logits), np.asarray(mask), np.asarray(actions)
    single = lg.ndim == 1
    if single:
        lg, mk, ac = lg[None], mk[None], ac[None]
        g = None if g is None else np.asarray(g)[None]
    n = lg.shape[0]
    if lg.ndim != 2 or lg.shape != (n, SLOTS) or mk.shape != (n, SLOTS) or ac.shape != (n, NUM_BLUE):
        raise ValueError(f'logits and mask must have shape ([B,] {SLOTS}) and actions ([B,] {NUM_BLUE}), got {lg.shape}, {mk.shape}, {ac.shape}')
    if lg.dtype.kind != 'f':
        raise ValueError(f'logits must be floating point, got {lg.dtype}')
    if ac.dtype.kind not in 'iu':
        raise ValueError(f'actions must be integers, got {ac.dtype}')
    if g is not None:
        g = np.asarray(g, np.float64)
        if g.shape != (n, NUM_BLUE, 2):
            raise ValueError(f'g must have shape ([B,] {NUM_BLUE}, 2), got {g.shape}')
    return lg, mk != 0, ac.astype(np.int64), g, single


def reference(logits, mask, actions, temperature=1.0, g=None):
    """The definition in float64 NumPy (written from the prose of include/cc4.h).  logits [B, 570] (or [570]) floating point, taken at the values
    they carry; mask [B, 570] bool or bytes; actions [B, 5] integers; g [B, 5, 2] = (d loss / d logp, d loss / d entropy) or None.  Returns
    (logp [B, 5], entropy [B, 5], refused [B, 5] bool) and, with g, the gradient [B, 570] as a fourth item."""
    temperature = check_temperature(temperature)
    lg, valid, ac, g, single = _rows(logits, mask, actions, g)
    n = lg.shape[0]
    r = float(np.float32(1.0) / np.float32(temperature))
    logp, ent, refused = np.zeros((n, NUM_BLUE)), np.zeros((n, NUM_BLUE)), np.zeros((n, NUM_BLUE), bool)
    grad = None if g is None else np.zeros((n, SLOTS))
    fmax = float(np.finfo(np.float32).max)
    for e in range(n):
        for b in range(NUM_BLUE):
            lo, hi = SEGMENTS[b], SEGMENTS[b + 1]
            a = int(ac[e, b])
            if a == -1:
                continue
            v = np.nonzero(valid[e, lo:hi])[0]
            with np.errstate(invalid='ignore', over='ignore'):
                x = lg[e, lo:hi][v].astype(np.float64) * r
                x = np.where(np.abs(x) > fmax, np.sign(x) * np.inf, x)      # x is a float32 product: it overflows where float32 does
            if (v.size == 0 or np.isnan(x).any() or (x == np.inf).any() or (x == -np.inf).all() or a < -1 or a >= hi - lo
                    or not valid[e, lo + a]):
                refused[e, b] = True
                continue
            m = x.max()
            with np.errstate(invalid='ignore'):
                d = x - m
            ex = np.exp(d)
            S = ex.sum()
            logS = np.log(S)
            pos = ex > 0
            H = logS - (ex[pos] * d[pos]).sum() / S
            ia = int(np.nonzero(v == a)[0][0])
            logp[e, b], ent[e, b] = x[ia] - m - logS, H
            if g is not None:
                lp = d - logS
                p = np.exp(lp)
                one = np.zeros(v.size)
                one[ia] = 1.0
                t1 = np.zeros(v.size)
                pp = p > 0
                t1[pp] = g[e, b, 1] * p[pp] * (lp[pp] + H)
                grad[e, lo + v] = r * (g[e, b, 0] * (one - p) - t1)
    out = (logp, ent, refused) if g is None else (logp, ent, refused, grad)
    return tuple(o[0] for o in out) if single else out


def from_rows(logits, mask, actions, temperature=1.0, g=None):
    """The host functions over rows: logits [B, 570] floating point (taken as float32), mask [B, 570], actions [B, 5], g [B, 5, 2] or None.
    Returns (aux [B, 5, 4] float32 -- logp, entropy, m, logS --, refused [B] the number of refused agents per row, grad [B, 570] float32 or None).
    No GPU."""
    lib = L.load()
    temperature = check_temperature(temperature)
    lg, valid, ac, g, single = _rows(logits, mask, actions, g)
    if single:
        raise ValueError(f'from_rows takes rows: logits [B, {SLOTS}]')
    n = lg.shape[0]
    lg = np.ascontiguousarray(lg, np.float32)
    mk = np.ascontiguousarray(valid, np.uint8)
    ac = np.ascontiguousarray(ac.clip(-2 ** 31, 2 ** 31 - 1), np.int32)
    aux = np.zeros((n, NUM_BLUE, 4), np.float32)
    refused = np.zeros(n, np.int32)
    grad = None
    if g is not None:
        g = np.ascontiguousarray(g, np.float32)
        grad = np.zeros((n, SLOTS), np.float32)
    vp = ctypes.c_void_p
    for e in range(n):
        args = (lg[e].ctypes.data_as(vp), mk[e].ctypes.data_as(vp), ac[e].ctypes.data_as(vp), temperature, aux[e].ctypes.data_as(vp))
        rc = lib.cc4_logp_actions_host(*args)
        if rc < 0:
            raise L.CC4Error(f'cc4_logp_actions_host failed (rc={rc})')
        refused[e] = rc
        if g is not None:
            rc = lib.cc4_logp_actions_grad_host(*args, g[e].ctypes.data_as(vp), grad[e].ctypes.data_as(vp))
            if rc != 0:
                raise L.CC4Error(f'cc4_logp_actions_grad_host failed (rc={rc})')
    return aux, refused, grad


# ---- torch: the kernels under autograd
_state = {}      # 'fn': the autograd Function, 'fault': {device index: int32 [1] tensor}


def _fault_word(torch, device):
    words = _state.setdefault('fault', {})
    if device.index not in words:
        words[device.index] = torch.zeros(1, dtype=torch.int32, device=device)
    return words[device.index]


def _function():
    """The torch.autograd.Function, made on first use (torch is imported here, not with the module)."""
    if 'fn' in _state:
        return _state['fn']
    import torch
    from torch.autograd.function import once_differentiable
    codes, p = TS.torch_codes(torch), TS.dptr

    class _EvaluateActions(torch.autograd.Function):
        @staticmethod
        def forward(ctx, logits, mask, actions, temperature):
            dev, n = logits.device, logits.numel() // SLOTS
            aux = torch.empty((n, NUM_BLUE, 4), dtype=torch.float32, device=dev)
            TS.pure_call('cc4_logp_actions_device', dev, p(logits), codes[logits.dtype], p(mask), p(actions), n, temperature, p(aux),
                         p(_fault_word(torch, dev)), count=(launches, 'fwd') if n else None)
            ctx.save_for_backward(logits, mask, actions, aux)
            ctx.temperature = temperature
            lead = tuple(logits.shape[:-1])
            return aux[:, :, 0].reshape(lead + (NUM_BLUE,)), aux[:, :, 1].reshape(lead + (NUM_BLUE,))

        @staticmethod
        @once_differentiable
        def backward(ctx, g_logp, g_entropy):
            logits, mask, actions, aux = ctx.saved_tensors
            n = logits.numel() // SLOTS
            g = torch.stack((g_logp, g_entropy), dim=-1).to(torch.float32).reshape(n, NUM_BLUE, 2).contiguous()
            grad = torch.empty_like(logits)
            # (the stream autograd made current for this node: the forward's)
            TS.pure_call('cc4_logp_actions_grad_device', logits.device, p(logits), codes[logits.dtype], p(mask), p(actions), n, ctx.temperature,
                         p(aux), p(g), p(grad), count=(launches, 'bwd') if n else None)
            return grad, None, None, None

    _state['fn'] = _EvaluateActions
    return _EvaluateActions


def evaluate_actions(logits, mask, actions, temperature=1.0):
    """(logp, entropy), float32 [..., 5] each, of the stored actions under logits, differentiable with respect to logits (once).
    logits: a contiguous float16, bfloat16 or float32 CUDA tensor [..., 570]; mask: bool or uint8 [..., 570], the stored info['action_mask'];
    actions: int32 [..., 5] as sample_actions() returned them (-1: skipped, zero logp, entropy and gradient) -- both contiguous, on the logits'
    device, with the logits' leading shape.  One launch on torch.cuda.current_stream() (k_logp_fwd); backward() is one more (k_logp_bwd) on the
    stream autograd gives it, and is not built when logits does not require grad.  No host wait.  A refused agent (a NaN or +inf among its valid
    logits, all of them -inf, no valid slot, an action outside its segment or on an invalid slot) gets zero logp, entropy and gradient, and
    check_errors() raises for it.  Wrong shapes, dtypes and devices raise ValueError before anything is enqueued."""
    import torch
    temperature = check_temperature(temperature)
    lead = tuple(logits.shape[:-1]) if torch.is_tensor(logits) else ()
    TS.check_tensor(torch, 'logits', logits, shape=lead + (SLOTS,), dtypes=tuple(TS.torch_codes(torch)), device='cuda')
    TS.check_tensor(torch, 'mask', mask, shape=lead + (SLOTS,), dtypes=(torch.bool, torch.uint8), device=logits.device)
    TS.check_tensor(torch, 'actions', actions, shape=lead + (NUM_BLUE,), dtypes=(torch.int32,), device=logits.device)
    return _function().apply(logits, mask, actions, temperature)


def check_errors(device=None):
    """The one synchronising call: reads and clears the device's fault word and raises CC4EngineError if an evaluate_actions() call since the last
    check refused an agent.  device: a torch device or index (None: the current one)."""
    import torch
    from .vec_env import CC4EngineError
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    word = _state.get('fault', {}).get(device.index)
    if word is None:
        return
    torch.cuda.synchronize(device)          # (every stream of the device: the calls may have run on any)
    bits = int(word.item())
    if bits:
        word.zero_()
    if bits & REFUSED:
        raise CC4EngineError('evaluate_actions refused an agent: a NaN or +inf among its valid logits, all of them -inf, no valid slot, or a '
                             'stored action outside its segment or on an invalid slot (CC4_LOGP_REFUSED)')
