"""What the wrappers of this package share towards the C library: pointers, the current stream and the two refusals"""
import ctypes as C

import torch

def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _need_gpu(who):
    if not torch.cuda.is_available():
        raise RuntimeError(f"hhmarl_2d_amd.{who} needs a ROCm GPU (no CPU fallback)")


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _fused_input(who, t, what):
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()):
        raise ValueError(f"{who}: {what} is a contiguous float32 CUDA tensor (the torch-op form for other dtypes and devices is {who}_torch)")
