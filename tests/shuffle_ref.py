"""The byte shuffle and its inverse in numpy, from the definition (include/brotli/batch.h, "Unshuffle on the device"): a segment of len bytes and a
width w has m = len // w elements; plane k holds byte k of every element; the len % w left-over bytes stay in place at the end."""
import numpy as np


def shuffle(b, w):
    """elements -> byte planes: out[k * m + i] = b[i * w + k]"""
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    m = len(a) // w
    return a[:w * m].reshape(m, w).T.tobytes() + a[w * m:].tobytes()


def unshuffle(b, w):
    """byte planes -> elements: out[p] = b[(p % w) * m + p // w] for p < w * m, out[p] = b[p] behind"""
    a = np.frombuffer(bytes(b), dtype=np.uint8)
    m = len(a) // w
    return a[:w * m].reshape(w, m).T.tobytes() + a[w * m:].tobytes()
