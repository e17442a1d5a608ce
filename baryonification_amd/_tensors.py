"""The helpers every Python front-end shares for "a numpy array or a CUDA tensor": what counts as a tensor, where it lies, its
address, the way onto the device, and the device-side scaffold of the per-bin spectra.  torch is imported inside the functions that
need it, so importing this module (and baryonification_amd.engine) does not import torch."""
import numpy as np

from . import _lib


def is_cuda_tensor(x):
    """a torch tensor on a GPU.  A CPU tensor is not one: callers read it through np.asarray (sphtfunc, mapstats, pixelfunc, pseudocl)"""
    return type(x).__module__.startswith('torch') and getattr(x, 'is_cuda', False)


def is_tensor(x):
    """anything with a data_ptr that is not a numpy array.  A CPU tensor is one, and the callers (flatsky, flatstats, engine.fourier)
    then refuse it by name: "needs a CUDA float64 tensor".  tests/test_cpu_tensor_inputs.py pins which function uses which."""
    return hasattr(x, 'data_ptr') and not isinstance(x, np.ndarray)


def device_index(t):
    """the device number libbfgx takes, of a tensor or a torch.device"""
    return getattr(t, 'device', t).index or 0


def stream(t):
    """the raw handle of torch's current stream on the device of a tensor or on a torch.device"""
    import torch
    return torch.cuda.current_stream(getattr(t, 'device', t)).cuda_stream


def launch_args(t):
    """the device= and stream= of an engine `_device` entry for work on the tensor t"""
    return dict(device=device_index(t), stream=stream(t))


def ptr(x):
    """the address of a tensor's or a numpy array's data; 0 for None"""
    return 0 if x is None else x.data_ptr() if hasattr(x, 'data_ptr') else x.ctypes.data


def to_cuda(a, device='cuda:0'):
    """a numpy array as a tensor on the device (torch takes no read-only array: such an array is copied first)"""
    import torch
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(device)


def mask_u8(mask, dev):
    """uint8 on dev, of the mask's shape: 1 where the mask (numpy or CUDA tensor) is nonzero (None stays None)"""
    import torch
    if mask is None:
        return None
    if is_cuda_tensor(mask):
        return (mask != 0).to(device=dev, dtype=torch.uint8).contiguous()
    return torch.from_numpy((mask != 0).astype(np.uint8)).to(dev)


def need_gpu():
    if _lib.call('bfgx_device_count') <= 0:
        raise _lib.BfgxError("bfgx: no HIP device visible: libbfgx has no CPU fallback")


def bin_means(dev, rows, Nk, enqueue):
    """The scaffold of a binned spectrum on the device: sums [rows][max(Nk, 1)] float64 and counts int64 are allocated on dev,
    enqueue(sum_ptr_0, .., sum_ptr_rows-1, counts_ptr) fills them, and the host gets (sums / counts [rows][..], counts) as numpy
    arrays, empty bins NaN."""
    import torch
    sums = torch.empty((rows, max(Nk, 1)), dtype=torch.float64, device=dev)
    cnt = torch.empty(max(Nk, 1), dtype=torch.int64, device=dev)
    enqueue(*[s.data_ptr() for s in sums], cnt.data_ptr())
    s, c = sums.cpu().numpy(), cnt.cpu().numpy()
    with np.errstate(divide='ignore', invalid='ignore'):
        return s / c, c
