"""The loader threads' side stream: ONE stream per device, shared by every loader thread and by every kind of loader work
(fits._read_fits_device, augment.ReferenceAugmenter, gtprep.DeviceSampler), under one lock.

HIP maps streams onto a handful of hardware queues (4 by default) in the order they are first used.  A training step
already uses three streams (engine._side_streams: the default stream, the weight-gradient and the auxiliary stream), so
this one takes the fourth queue; any further stream (one per thread, or one per kind of work) would wrap onto a queue of
the step's and wait behind a whole step.  The lock keeps the threads' launches, copies and synchronise of one call
together (the stream's scratch buffers are shared)."""
import contextlib
import threading

_streams = {}
_lock = threading.Lock()


@contextlib.contextmanager
def loader_stream(device):
    """Holds the lock and yields the loader stream of `device` (a torch GPU device), created on first use.  The caller
    enqueues on it (``with torch.cuda.stream(st)``) and synchronises only it before leaving the block."""
    import torch
    device = torch.device(device)
    with _lock:
        st = _streams.get(device)
        if st is None:
            st = _streams[device] = torch.cuda.Stream(device=device)
        yield st
