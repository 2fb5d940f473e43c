"""NumPy restatement of the averaged generator's recurrence (csrc/optim.hip ema_update / ema_one_minus_beta).

    beta_t = warmup ? min(decay, (1 + t) / (10 + t)) : decay          t = the generator's Adam iteration after the increment
    e'     = e + (1 - beta_t) * (p' - e)

Every operation is one correctly rounded operation of `dtype` (float32 restates the kernels bit for bit; float64 is the form the
closed-form tests run), in the kernels' order: p' - e, (1 - beta_t) * (..), e + (..)."""
import numpy as np


def beta_t(t, decay=0.999, warmup=True, dtype=np.float32):
    f = dtype
    decay = f(decay)
    if not warmup:
        return decay
    t = f(int(t))
    return min(decay, (f(1) + t) / (f(10) + t))


def ema_step(e, p, t, decay=0.999, warmup=True, dtype=np.float32):
    """the average after one optimizer step whose updated masters are p"""
    e, p = np.asarray(e, dtype), np.asarray(p, dtype)
    omb = dtype(1) - beta_t(t, decay, warmup, dtype)
    d = p - e
    s = omb * d
    return e + s
