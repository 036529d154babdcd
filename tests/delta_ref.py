"""Delta and its inverse in numpy, from the definition (include/brotli/batch.h, "Undelta on the device"): a segment of len bytes and a width w has
m = len // w elements, little-endian unsigned integers of w bytes; the len % w left-over bytes behind the last whole element stay as they are."""
import numpy as np


def delta(b, w):
    """values -> deltas: out_elem[0] = elem[0], out_elem[k] = (elem[k] - elem[k - 1]) mod 2^(8 w)"""
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    m = len(a) // w
    x = a[:w * m].view("<u%d" % w)
    d = x.copy()
    d[1:] = x[1:] - x[:-1]
    return d.tobytes() + a[w * m:].tobytes()


def undelta(b, w):
    """deltas -> values: out_elem[k] = (elem[0] + ... + elem[k]) mod 2^(8 w)"""
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    m = len(a) // w
    x = a[:w * m].view("<u%d" % w)
    return np.cumsum(x, dtype="<u%d" % w).tobytes() + a[w * m:].tobytes()
