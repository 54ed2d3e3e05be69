"""Optimizer and step chores: fills, copies, casts, layouts, SGD (csrc/optim_kernels.hip)."""
import ctypes

from .._lib import lib
from .base import _ld, _p, _stream


def fill_zero(t):
    """t.zero_() as a kernel of this library (contiguous tensor, 16-byte aligned storage)."""
    assert t.is_contiguous()
    lib().call('rgda_fill_zero', t.data_ptr(), t.numel() * t.element_size(), _stream())


def copy_multi(pairs):
    """[(dst, src), ...] (<= 4 pairs of contiguous tensors of equal byte size, multiples of 16) in ONE launch."""
    n = len(pairs)
    for d, s_ in pairs:
        assert d.is_contiguous() and s_.is_contiguous() and d.numel() * d.element_size() == s_.numel() * s_.element_size()
    D = (ctypes.c_void_p * n)(*[d.data_ptr() for d, _ in pairs])
    S = (ctypes.c_void_p * n)(*[s_.data_ptr() for _, s_ in pairs])
    B = (ctypes.c_size_t * n)(*[d.numel() * d.element_size() for d, _ in pairs])
    lib().call('rgda_copy_multi', n, ctypes.cast(D, ctypes.c_void_p), ctypes.cast(S, ctypes.c_void_p), ctypes.cast(B, ctypes.c_void_p),
               _stream())


def set_f32(t, value):
    lib().call('rgda_set_f32', t.data_ptr(), float(value), _stream())


def dropout_mask(out, p, seed):
    """out (f32, contiguous) = Dropout keep mask scaled by 1 / (1 - p), drawn from (seed, element index)."""
    lib().call('rgda_dropout_mask', out.data_ptr(), out.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _stream())


def sumsq(g, out, ws):
    lib().call('rgda_sumsq', g.data_ptr(), g.numel(), out.data_ptr(), ws.data_ptr(), _stream())


def sgd_step(p, g, v, shadow, p_bf16, gnorm_sq, lr_dev, momentum, weight_decay, max_norm, gscale, ema_decay,
             first_step, shadow_bf16=None):
    lib().call('rgda_sgd_step', p.data_ptr(), g.data_ptr(), v.data_ptr(), _p(shadow), _p(p_bf16), _p(shadow_bf16),
               gnorm_sq.data_ptr(),
               lr_dev.data_ptr(), p.numel(), momentum, weight_decay, max_norm, gscale, ema_decay, int(first_step),
               _stream())


def weight_transpose_bf16(w, wt, Co, T, Ci):
    lib().call('rgda_weight_transpose_bf16', w.data_ptr(), wt.data_ptr(), Co, T, Ci, _stream())


def weight_transpose_batched(table, n, total_blocks):
    lib().call('rgda_weight_transpose_batched', table.data_ptr(), n, total_blocks, _stream())


def cast_bf16(src, dst):
    lib().call('rgda_cast_bf16', src.data_ptr(), dst.data_ptr(), src.numel(), _stream())


def cast_f32(src, dst):
    lib().call('rgda_cast_f32', src.data_ptr(), dst.data_ptr(), dst.numel(), _stream())


def ddp_accumulate_bf16(recv, world, out):
    lib().call('rgda_ddp_accumulate_bf16', recv.data_ptr(), world, out.data_ptr(), out.numel(), _stream())


def pad_cast_bf16(src, dst, R, K, Kp):
    lib().call('rgda_pad_cast_bf16', src.data_ptr(), dst.data_ptr(), R, K, Kp, _stream())


def unpad_acc_f32(src, dst, R, K, Kp):
    lib().call('rgda_unpad_acc_f32', src.data_ptr(), dst.data_ptr(), R, K, Kp, _stream())


def add_bf16(a, b, out, M, C):
    lib().call('rgda_add_bf16', a.data_ptr(), _ld(a), b.data_ptr(), _ld(b), out.data_ptr(), _ld(out), M, C, _stream())
