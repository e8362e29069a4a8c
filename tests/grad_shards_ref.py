"""hh_grad_pack and hh_grad_combine restated in numpy (include/hh_learner.h has the definitions): the same values in the same order, so
a test compares bit for bit.  numpy float64 multiplies and adds are IEEE operations rounded one by one, like the kernel's."""
import numpy as np


def layout(ns):
    """grad_layout: every tensor starts at the next multiple of 4 elements -> (ns, offs, bucket_elems)"""
    offs, at = [], 0
    for n in ns:
        offs.append(at)
        at += (int(n) + 3) // 4 * 4
    return [int(n) for n in ns], offs, at


def pack(grads, lay):
    """grads: float32 arrays or None -> the bucket float32 [bucket_elems]: +0.0 everywhere, then every gradient at its offset"""
    ns, offs, E = lay
    bucket = np.zeros((E,), dtype=np.float32)
    for g, n, off in zip(grads, ns, offs):
        if g is not None:
            bucket[off:off + n] = np.asarray(g, dtype=np.float32).reshape(-1)
    return bucket


def combine(buckets, weight, lay):
    """buckets float32 [W, bucket_elems], weight W floats -> per tensor float32 [n]:
    acc = float64(b[0]) * w[0]; acc = acc + float64(b[r]) * w[r] for r = 1 .. W-1; float32(acc)"""
    ns, offs, E = lay
    b = np.asarray(buckets, dtype=np.float32)
    with np.errstate(all="ignore"):
        acc = b[0].astype(np.float64) * np.float64(weight[0])
        for r in range(1, b.shape[0]):
            prod = b[r].astype(np.float64) * np.float64(weight[r])
            acc = acc + prod
        flat = acc.astype(np.float32)
    return [flat[off:off + n].copy() for n, off in zip(ns, offs)]
