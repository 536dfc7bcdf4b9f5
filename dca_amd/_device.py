"""What the stand-alone entry points (cluster, neighbors, silhouette, community) and the data paths share about the device:
the default ops, the device a call runs on, and points as a float32 device tensor."""
import numpy as np


def default_ops(ops):
    """``ops``, or the HIP ops where the caller gave none."""
    if ops is None:
        from .ops import HipOps
        ops = HipOps()
    return ops


def device_of(x, ops):
    """The device of a device tensor ``x``; for anything else the current device of ``ops`` (the host for reference ops)."""
    import torch
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    return torch.device('cuda', torch.cuda.current_device()) if ops.device_type == 'cuda' else torch.device('cpu')


def as_points(x, dev, what):
    """Host array or tensor [n, d] as a contiguous float32 tensor on ``dev``."""
    import torch
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float32))
    if x.dim() != 2:
        raise ValueError('dca_amd: %s: points are the rows of a 2-d array (got %d dimensions)' % (what, x.dim()))
    return x.to(device=dev, dtype=torch.float32).contiguous()
