"""The definition of include/gten_hip_lora.h in NumPy f32, one rounding per operation: the k loop written out, then
convert._round_to; the bytes follow from convert.quantize."""
import importlib

import numpy as np

from __graft_entry__ import load_package

load_package()
convert = importlib.import_module("tinyllama_cpp_amd.convert")


def merge(w, a, b, scale, src, rounded=True):
    """w [rows][cols], a [rank][cols], b [rows][rank]: f32 arrays holding the widened values.  m = round_to_src(w + scale * acc)"""
    w, a, b = (np.asarray(v, np.float32) for v in (w, a, b))
    acc = np.zeros_like(w)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(a.shape[0]):
            acc = acc + b[:, k:k + 1] * a[k:k + 1, :]
        m = w + np.float32(scale) * acc
        return convert._round_to(m, src) if rounded else m
