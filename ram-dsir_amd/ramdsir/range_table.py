"""The host side of csrc/range_walk.h: the device range tables of rd_snapshot (ckpt.py), rd_avg_step (avg.py), rd_guard_sync
(guard.py) and rd_optim_step (optim.py), written once.  A table is a ctypes array of one record per range; range i is cut into
chunks of `chunk` units (bytes, or elements for rd_optim_step) from its start, and its chunk0 field is the number of chunks of the
ranges in front of it -- the column the kernels search and the entry points check."""
import ctypes as C

import numpy as np
import torch


def build(struct, chunk, rows, size_field):
    """rows: one dict of field values per range (chunk0 is filled in here); size_field: the field that holds a range's size in the
    units of `chunk` (a negative size counts as empty: the entry point refuses it).  An empty list still yields a one-entry array."""
    arr, chunks = (struct * max(len(rows), 1))(), 0
    for e, row in zip(arr, rows):
        for k, v in row.items():
            setattr(e, k, v)
        e.chunk0 = chunks
        chunks += (max(row[size_field], 0) + chunk - 1) // chunk
    return arr, chunks


def upload(arr, n, device):
    """The first n records (at least one) as a uint8 device tensor."""
    return torch.from_numpy(np.frombuffer(bytes(arr), np.uint8)[:max(n, 1) * C.sizeof(arr._type_)].copy()).to(device)


def check_words(name, *tensors):
    """ValueError unless the first tensor is a whole number of 32-bit words and every tensor is contiguous; the bytes of the first."""
    t = tensors[0]
    nbytes = t.numel() * t.element_size()
    if nbytes % 4 != 0 or not all(x.is_contiguous() for x in tensors):
        raise ValueError('range %s: %d bytes of a %s tensor (a contiguous multiple of 4 bytes is needed)' % (name, nbytes, t.dtype))
    return nbytes


def stream_handle(stream=None):
    """The raw handle a run* helper passes on: the current stream's unless one is given."""
    return torch.cuda.current_stream().cuda_stream if stream is None else stream
