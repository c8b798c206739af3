"""The worker side of the GPU worker tests: what every tests/_*_worker.py needs around its calls into libmjx -- int arrays, the
stream, uploads, NaN-prefilled output blocks with a guard behind them, bit equality, a route switch held for one call, and the
RESULT line tests/_worker_run.py reads.  Imports without a GPU: the device is looked up on first use.  (ptr, check and load come
from mjrl_amd._lib.)"""
import contextlib
import ctypes
import json
import os

import numpy as np
import torch

GUARD = 64              # NaN elements behind every guarded block
KEEP = []               # uploads made with keep=True: alive until the process ends, so none is freed before its kernel ran
CHECKED = [0]           # blocks checked_block() has looked at


def device():
    return torch.device("cuda", 0)


def ints(v):
    """a C int array of v (at least one element long, so that an empty list still gives a valid pointer)"""
    return (ctypes.c_int * max(len(v), 1))(*[int(x) for x in v])


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def up(x, dtype=np.float32, keep=False, dev=None):
    """a host array on the device (None stays None; dtype None: the array's own)"""
    if x is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(x, dtype)).to(device() if dev is None else dev)
    if keep:
        KEEP.append(t)
    return t


def nan_block(count, dtype=torch.float32, dev=None):
    """an output block of `count` NaN elements with GUARD more behind it"""
    return torch.full((count + GUARD,), float("nan"), dtype=dtype, device=device() if dev is None else dev)


def checked_block(buf, count, what):
    """a nan_block after a call: no NaN inside, every guard element still NaN -> the host copy without the guard"""
    if buf.is_cuda:
        torch.cuda.synchronize()
    b = buf.cpu().numpy()
    CHECKED[0] += 1
    assert not np.isnan(b[:count]).any(), "%s: %d elements never written" % (what, int(np.isnan(b[:count]).sum()))
    assert np.isnan(b[count:]).all(), "%s: %d guard elements touched" % (what, int((~np.isnan(b[count:])).sum()))
    return b[:count]


def same_bits(a, b):
    """two arrays (or tensors) of one dtype and shape hold the same bits"""
    a, b = (np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x) for x in (a, b))
    return bool(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes())


@contextlib.contextmanager
def switch(name, value):
    """os.environ[name] = value for the calls inside; afterwards the variable is what it was (absent if it was absent), also when
    a call raises.  value None: the variable is left alone."""
    before = os.environ.get(name)
    if value is not None:
        os.environ[name] = str(value)
    try:
        yield
    finally:
        if value is not None:
            if before is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = before


def emit(payload):
    print("RESULT " + json.dumps(payload), flush=True)
