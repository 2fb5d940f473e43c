"""Learning-rate schedules for Adam: tf.keras.optimizers.schedules of Keras 2.9 -- ExponentialDecay,
PiecewiseConstantDecay, PolynomialDecay, CosineDecay -- and the build-added LinearDecay (constant, then linear, then `end`:
the pix2pix recipe).  Reference: the two optimizers of pix2pix_model.py:28-29 take a float or one of these.

A schedule object is a description.  The DEVICE evaluates it, in f64, from the optimizer's step counter inside
p2p_adam_tick_sched (csrc/optim.hip lr_schedule), so a recorded or captured step follows the schedule without the host.
Calling the object on a step number evaluates the same formulas on the host in f64, for logging and for the tests; `step` is
the optimizer's `iterations` BEFORE the step that uses the rate, as in Keras.

Every schedule takes the build-added keyword `warmup_steps` (default 0): while step < warmup_steps the rate is multiplied by
(step + 1) / warmup_steps.
"""
import math

from . import _lib as L


class LearningRateSchedule:
    """base class: subclasses fill a _lib.LrSchedule (include/p2pgan.h p2p_lr_schedule) and restate its formula in __call__"""
    warmup_steps = 0

    def _warm(self, lr, step):
        if self.warmup_steps > 0 and step < self.warmup_steps:
            return lr * ((step + 1.0) / float(self.warmup_steps))
        return lr

    def _set_warmup(self, warmup_steps):
        if warmup_steps < 0:
            raise ValueError(f"warmup_steps must not be negative, got {warmup_steps}")
        self.warmup_steps = warmup_steps

    def fill(self, s):
        """writes this schedule into the LrSchedule `s` in place (the engine's slot: a recorded step holds its address)"""
        raise NotImplementedError

    def struct(self):
        s = L.LrSchedule()
        self.fill(s)
        return s

    def _base(self, s, kind, initial, decay_steps=0.0, rate=0.0, end=0.0, power=0.0, hold_steps=0.0, flag=0):
        s.kind, s.flag, s.nbounds = kind, int(flag), 0
        s.initial, s.decay_steps, s.rate, s.end, s.power = float(initial), float(decay_steps), float(rate), float(end), float(power)
        s.hold_steps, s.warmup_steps = float(hold_steps), float(self.warmup_steps)

    def get_config(self):
        return {k: v for k, v in vars(self).items() if not k.startswith("_")}

    def __eq__(self, other):
        return type(other) is type(self) and other.get_config() == self.get_config()

    def __hash__(self):
        return hash((type(self).__name__, repr(sorted(self.get_config().items()))))

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{k}={v!r}' for k, v in self.get_config().items())})"


def _positive(name, v):
    if not v > 0:
        raise ValueError(f"{name} must be positive, got {v}")


class Constant(LearningRateSchedule):
    """a fixed rate with an optional warm-up (a plain float is the same thing without one)"""

    def __init__(self, learning_rate, warmup_steps=0):
        self.learning_rate = float(learning_rate)
        self._set_warmup(warmup_steps)

    def fill(self, s):
        self._base(s, L.LrSchedule.CONSTANT, self.learning_rate)

    def __call__(self, step):
        return self._warm(self.learning_rate, float(step))


class ExponentialDecay(LearningRateSchedule):
    """initial_learning_rate * decay_rate ^ (step / decay_steps); staircase: the exponent is floored"""

    def __init__(self, initial_learning_rate, decay_steps, decay_rate, staircase=False, name=None, warmup_steps=0):
        _positive("decay_steps", decay_steps)
        self.initial_learning_rate, self.decay_steps, self.decay_rate = float(initial_learning_rate), decay_steps, float(decay_rate)
        self.staircase = bool(staircase)
        self._set_warmup(warmup_steps)

    def fill(self, s):
        self._base(s, L.LrSchedule.EXPONENTIAL, self.initial_learning_rate, self.decay_steps, rate=self.decay_rate, flag=self.staircase)

    def __call__(self, step):
        step = float(step)
        p = step / float(self.decay_steps)
        if self.staircase:
            p = math.floor(p)
        return self._warm(self.initial_learning_rate * math.pow(self.decay_rate, p), step)


class PiecewiseConstantDecay(LearningRateSchedule):
    """values[0] while step <= boundaries[0], values[i] while boundaries[i-1] < step <= boundaries[i], values[-1] beyond the last
    boundary (at most 8 boundaries: they are held inline in the device-side struct)"""
    MAX_BOUNDARIES = 8

    def __init__(self, boundaries, values, name=None, warmup_steps=0):
        boundaries, values = list(boundaries), [float(v) for v in values]
        if len(values) != len(boundaries) + 1:
            raise ValueError("the length of boundaries should be 1 less than the length of values")
        if not 1 <= len(boundaries) <= self.MAX_BOUNDARIES:
            raise ValueError(f"1 to {self.MAX_BOUNDARIES} boundaries are supported, got {len(boundaries)}")
        if any(b >= c for b, c in zip(boundaries, boundaries[1:])):
            raise ValueError("boundaries must be strictly increasing")
        self.boundaries, self.values = boundaries, values
        self._set_warmup(warmup_steps)

    def fill(self, s):
        self._base(s, L.LrSchedule.PIECEWISE, self.values[0])
        s.nbounds = len(self.boundaries)
        for i in range(8):
            s.bounds[i] = float(self.boundaries[i]) if i < len(self.boundaries) else 0.0
        for i in range(9):
            s.values[i] = self.values[i] if i < len(self.values) else 0.0

    def __call__(self, step):
        step = float(step)
        i = 0
        while i < len(self.boundaries) and step > self.boundaries[i]:
            i += 1
        return self._warm(self.values[i], step)


class PolynomialDecay(LearningRateSchedule):
    """(initial - end) * (1 - s / d) ^ power + end with s = min(step, decay_steps), d = decay_steps; cycle: s = step and
    d = decay_steps * ceil(step / decay_steps) (1 at step 0)"""

    def __init__(self, initial_learning_rate, decay_steps, end_learning_rate=0.0001, power=1.0, cycle=False, name=None,
                 warmup_steps=0):
        _positive("decay_steps", decay_steps)
        self.initial_learning_rate, self.decay_steps = float(initial_learning_rate), decay_steps
        self.end_learning_rate, self.power, self.cycle = float(end_learning_rate), float(power), bool(cycle)
        self._set_warmup(warmup_steps)

    def fill(self, s):
        self._base(s, L.LrSchedule.POLYNOMIAL, self.initial_learning_rate, self.decay_steps, end=self.end_learning_rate,
                   power=self.power, flag=self.cycle)

    def __call__(self, step):
        step = float(step)
        d, g = float(self.decay_steps), step
        if self.cycle:
            d = d * (1.0 if step == 0.0 else math.ceil(step / d))
        else:
            g = min(step, d)
        return self._warm((self.initial_learning_rate - self.end_learning_rate) * math.pow(1.0 - g / d, self.power)
                          + self.end_learning_rate, step)


class CosineDecay(LearningRateSchedule):
    """initial * ((1 - alpha) * 0.5 * (1 + cos(pi * min(step, decay_steps) / decay_steps)) + alpha)"""

    def __init__(self, initial_learning_rate, decay_steps, alpha=0.0, name=None, warmup_steps=0):
        _positive("decay_steps", decay_steps)
        self.initial_learning_rate, self.decay_steps, self.alpha = float(initial_learning_rate), decay_steps, float(alpha)
        self._set_warmup(warmup_steps)

    def fill(self, s):
        self._base(s, L.LrSchedule.COSINE, self.initial_learning_rate, self.decay_steps, rate=self.alpha)

    def __call__(self, step):
        step = float(step)
        c = 0.5 * (1.0 + math.cos(math.pi * (min(step, float(self.decay_steps)) / float(self.decay_steps))))
        return self._warm(self.initial_learning_rate * ((1.0 - self.alpha) * c + self.alpha), step)


class LinearDecay(LearningRateSchedule):
    """build-added, the pix2pix recipe: initial while step < hold_steps, then linear over decay_steps down to `end`, then `end`"""

    def __init__(self, initial_learning_rate, hold_steps, decay_steps, end=0.0, name=None, warmup_steps=0):
        _positive("decay_steps", decay_steps)
        if hold_steps < 0:
            raise ValueError(f"hold_steps must not be negative, got {hold_steps}")
        self.initial_learning_rate, self.hold_steps, self.decay_steps, self.end = float(initial_learning_rate), hold_steps, decay_steps, float(end)
        self._set_warmup(warmup_steps)

    def fill(self, s):
        self._base(s, L.LrSchedule.LINEAR, self.initial_learning_rate, self.decay_steps, end=self.end, hold_steps=self.hold_steps)

    def __call__(self, step):
        step = float(step)
        hold, d = float(self.hold_steps), float(self.decay_steps)
        if step >= hold + d:
            lr = self.end
        elif step >= hold:
            lr = self.initial_learning_rate + (self.end - self.initial_learning_rate) * ((step - hold) / d)
        else:
            lr = self.initial_learning_rate
        return self._warm(lr, step)


def as_schedule(learning_rate):
    """a float or a schedule object -> (schedule object, whether the device has to evaluate it: anything but a plain constant)"""
    if isinstance(learning_rate, LearningRateSchedule):
        return learning_rate, not (isinstance(learning_rate, Constant) and learning_rate.warmup_steps == 0)
    if isinstance(learning_rate, (int, float)) and not isinstance(learning_rate, bool):
        return Constant(float(learning_rate)), False
    raise TypeError(f"learning_rate is a float or a schedule of palette_and_histo_gan_amd.schedules, got {type(learning_rate).__name__}")
