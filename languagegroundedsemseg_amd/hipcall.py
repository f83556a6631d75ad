"""The call layer: how every Python caller hands tensors, streams and scratch to the C-ABI (include/lgs_engine.h), one answer each
(DESIGN.md section 4a):
  ptr            device address as a plain int
  raw_stream     raw handle of torch's current HIP stream
  on_device      device guard that switches only when it has to
  device_index   the index of a device, the current one when it names none
  scratch        the one grow-only workspace per (device, stream)
  dtype_code     LGS_F32 / LGS_BF16 of a feature tensor
  require_hip    the one refusal of a host tensor: there is no CPU fallback
  i32, i64       a Python int as the C integer of that width
  host_offsets   the one validator of "B + 1 ascending scene offsets from 0 to n"
Imports torch and engine only: me/host.py, me/backend_hip.py, me/utils.py, augment.py, pointcloud.py, pointgroup.py and ddp.py all import
it, and it needs nothing of the `me` package."""
import torch

from . import engine


def ptr(t):
    """device address as a plain int (None = NULL): every engine entry point has its argtypes declared (engine.py, checked against
    the header by tests/test_abi.py), so ctypes converts -- building a c_void_p object per argument cost ~1 ms of host time per
    step (2500 pointer arguments)"""
    return t.data_ptr() if t is not None else None


def device_index(device):
    """the index of `device`, the current device's when it names none"""
    return device.index if device.index is not None else torch._C._cuda_getDevice()


def raw_stream(device=None):
    """raw handle of torch's current HIP stream on `device` (default: the current device).  One C call: torch.cuda.current_stream()
    builds a Stream object and resolves the device twice, ~14 us of host time per engine call"""
    return torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice() if device is None or device.index is None else device.index)


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


_NOGUARD = _NoGuard()


def on_device(device):
    """device guard that only switches when the tensor's device is not the current one (the usual case: one process per GPU)"""
    if device.index is None or device.index == torch._C._cuda_getDevice():
        return _NOGUARD
    return torch.cuda.device(device)


def dtype_code(t):
    if t.dtype == torch.float32:
        return engine.LGS_F32
    if t.dtype == torch.bfloat16:
        return engine.LGS_BF16
    raise RuntimeError("lgs_engine supports float32 and bfloat16 features, got %s" % t.dtype)


def require_hip(t, what):
    if not (isinstance(t, torch.Tensor) and t.is_cuda):
        raise RuntimeError("%s must be a HIP tensor (got %s): the MI355X engine has no CPU fallback"
                           % (what, t.device if isinstance(t, torch.Tensor) else type(t).__name__))


_WS = {}


def scratch(nbytes, device, stream=None):
    """Scratch of one engine call: ONE grow-only buffer per (device, current stream).  Every use is confined to the launches
    of a single call, and calls on one stream run in order, so the next call may overwrite it; weight gradients on the side
    stream get their own.  (A fresh torch.empty per call cost ~7 us of allocator time, ~250 times per step.)  The contents are
    whatever the last call left: a kernel initialises what it reads."""
    key = (device.index, torch._C._cuda_getCurrentRawStream(device_index(device)) if stream is None else stream.cuda_stream)
    t = _WS.get(key)
    nbytes = int(nbytes)
    if t is None or t.numel() < nbytes:
        size = max(nbytes + nbytes // 4, 1 << 20)
        if stream is None:
            t = torch.empty(size, dtype=torch.uint8, device=device)
        else:
            # the buffer must belong to the allocator pool of the stream that uses it: when it is replaced by a larger one, the
            # old block may only be handed out again in that stream's order
            with torch.cuda.stream(stream):
                t = torch.empty(size, dtype=torch.uint8, device=device)
        _WS[key] = t
    return t


def i32(v):
    """the low 32 bits of an integer as a C int32"""
    return ((int(v) + (1 << 31)) & 0xffffffff) - (1 << 31)


def i64(v):
    """the low 64 bits of an integer as a C int64"""
    return ((int(v) + (1 << 63)) & 0xffffffffffffffff) - (1 << 63)


def host_offsets(scene_offsets, n):
    """scene_offsets (list, numpy array or host tensor) -> a Python list, checked: B + 1 non-decreasing integers from 0 to n"""
    off = [int(v) for v in (scene_offsets.tolist() if hasattr(scene_offsets, "tolist") else scene_offsets)]
    if len(off) < 2 or off[0] != 0 or off[-1] != n or any(a > b for a, b in zip(off, off[1:])):
        raise ValueError("scene_offsets must be B + 1 non-decreasing integers from 0 to the number of rows (%d): %r" % (n, off[:8]))
    return off
