"""Learning-rate schedules and the optimizer config of the reference
(retinanet/optimizers/builder.py:13-71, cosine_decay_with_warmup.py:4-43,
piecewise_constant_decay_with_warmup.py:4-35).

The schedules are host-side scalar functions of the step; the optimizer object only carries
the hyper-parameters the fused HIP step kernels consume (SGD momentum; Adam / RMSprop / Adagrad with Keras'
arguments and defaults, as `tf.optimizers.get` builds them from `training.optimizer.name`; EMA decay, clipnorm).
"""
from __future__ import annotations

import math
from copy import deepcopy


class CosineDecayWithLinearWarmup:
    def __init__(self, initial_learning_rate, warmup_learning_rate, warmup_steps, total_steps, alpha=0.0):
        self.initial_learning_rate = float(initial_learning_rate)
        self.warmup_learning_rate = float(warmup_learning_rate)
        self.warmup_steps = int(warmup_steps)
        self.decay_steps = int(total_steps) - int(warmup_steps)
        self.alpha = float(alpha)
        self._step_size = self.initial_learning_rate - self.warmup_learning_rate

    def __call__(self, step):
        if step < self.warmup_steps:
            return self.warmup_learning_rate + step / self.warmup_steps * self._step_size
        # Keras CosineDecay evaluated on the un-shifted step (cosine_decay_with_warmup.py:14,32-33)
        s = min(step, self.decay_steps)
        cosine = 0.5 * (1.0 + math.cos(math.pi * s / self.decay_steps))
        return self.initial_learning_rate * ((1.0 - self.alpha) * cosine + self.alpha)


class PiecewiseConstantDecayWithLinearWarmup:
    def __init__(self, warmup_learning_rate, warmup_steps, boundaries, values):
        self.boundaries = [b - 1 for b in boundaries]  # piecewise_constant_decay_with_warmup.py:8-9
        self.values = list(values)
        self.warmup_learning_rate = float(warmup_learning_rate)
        self.warmup_steps = int(warmup_steps)
        self._step_size = self.values[0] - self.warmup_learning_rate

    def __call__(self, step):
        if step < self.warmup_steps:
            return self.warmup_learning_rate + step / self.warmup_steps * self._step_size
        for b, v in zip(self.boundaries, self.values):
            if step <= b:
                return v
        return self.values[-1]


def get_learning_rate_schedule(total_steps, params):
    _params = dict(deepcopy(params))
    schedule_type = _params.pop("schedule_type", None)
    if schedule_type == "piecewise_constant_decay":
        return PiecewiseConstantDecayWithLinearWarmup(**_params)
    if schedule_type == "cosine_decay":
        _params["total_steps"] = total_steps
        return CosineDecayWithLinearWarmup(**_params)
    raise ValueError("Invalid learning rate schedule requested")


class OptimizerConfig:
    """What `build_optimizer` returns: hyper-parameters + schedule + step counter."""

    def __init__(self, name, momentum, nesterov, clipnorm, learning_rate, use_moving_average,
                 moving_average_decay, loss_scale, beta_1=0.9, beta_2=0.999, epsilon=1e-7, amsgrad=False, rho=0.9,
                 centered=False, initial_accumulator_value=0.1):
        self.name = name
        self.momentum = momentum
        self.nesterov = nesterov
        # the Keras arguments of adam (beta_1, beta_2, epsilon, amsgrad), rmsprop (rho, momentum, epsilon, centered)
        # and adagrad (initial_accumulator_value, epsilon); an optimizer reads only its own
        self.beta_1 = beta_1
        self.beta_2 = beta_2
        self.epsilon = epsilon
        self.amsgrad = amsgrad
        self.rho = rho
        self.centered = centered
        self.initial_accumulator_value = initial_accumulator_value
        self.clipnorm = clipnorm
        self.learning_rate = learning_rate
        self.use_moving_average = use_moving_average
        self.moving_average_decay = moving_average_decay
        # tf.keras.mixed_precision.LossScaleOptimizer(dynamic=True) defaults (optimizers/builder.py:56-64)
        self.dynamic_loss_scale = loss_scale
        self.initial_loss_scale = 2.0 ** 15
        self.loss_scale_growth_steps = 2000
        self.iterations = 0

    def lr(self, step=None):
        return self.learning_rate(self.iterations if step is None else step)

    def ema_decay(self, step=None):
        """tfa MovingAverage(dynamic_decay=True): min(decay, (1+t)/(10+t))."""
        t = self.iterations if step is None else step
        return min(self.moving_average_decay, (1.0 + t) / (10.0 + t))

    @property
    def class_name(self):
        """the Keras class: its name prefixes the step counter in a checkpoint (`Adam/iter`)"""
        return CLASS_NAMES[self.name]

    def slots(self):
        """[(Keras slot name, initial value)] in the order of the step kernel's slot arrays; a slot the configuration
        does not create is None (Keras creates RMSprop's `momentum` only with momentum > 0, `mg` only when centered,
        Adam's `vhat` only with amsgrad)."""
        if self.name == "sgd":
            return [("momentum", 0.0)]
        if self.name == "adam":
            return [("m", 0.0), ("v", 0.0), ("vhat", 0.0) if self.amsgrad else None]
        if self.name == "rmsprop":
            return [("rms", 0.0), ("momentum", 0.0) if self.momentum > 0.0 else None,
                    ("mg", 0.0) if self.centered else None]
        return [("accumulator", float(self.initial_accumulator_value))]

    def step_size(self, step=None):
        """The scalar the step kernel multiplies with: the schedule's learning rate, and for Adam
        alpha_t = lr * sqrt(1 - beta_2^t) / (1 - beta_1^t) with t = iterations + 1, formed here in float64."""
        t = (self.iterations if step is None else step) + 1
        lr = self.lr(step)
        if self.name == "adam":
            return lr * math.sqrt(1.0 - self.beta_2 ** t) / (1.0 - self.beta_1 ** t)
        return lr


CLASS_NAMES = {"sgd": "SGD", "adam": "Adam", "rmsprop": "RMSprop", "adagrad": "Adagrad"}


def iter_key(optimizer=None):
    """checkpoint key of the step counter: `<Class>/iter` (`SGD/iter` without an optimizer)"""
    return (optimizer.class_name if optimizer is not None else "SGD") + "/iter"


def read_iterations(extras, optimizer=None):
    """(step counter, class that wrote it or None) from a checkpoint's non-variable entries.  The counter of the
    configured class when the file has it; else the one another optimizer class left: the weights and the position in
    the schedule carry over, that class's slots do not."""
    own = iter_key(optimizer)
    if extras.get(own) is not None:
        return int(extras[own]), own[:-len("/iter")]
    for cls in CLASS_NAMES.values():
        if extras.get(cls + "/iter") is not None:
            return int(extras[cls + "/iter"]), cls
    return 0, None
# the constructor arguments of each Keras class next to `name` and `learning_rate`, with Keras' defaults
_CLASS_KEYS = {
    "adam": {"beta_1": 0.9, "beta_2": 0.999, "epsilon": 1e-7, "amsgrad": False},
    "rmsprop": {"rho": 0.9, "momentum": 0.0, "epsilon": 1e-7, "centered": False},
    "adagrad": {"initial_accumulator_value": 0.1, "epsilon": 1e-7},
}


def build_optimizer(params, train_steps, precision):
    _params = dict(deepcopy(params))
    lr_params = _params.pop("lr_params", None)
    use_moving_average = bool(_params.pop("use_moving_average", False))
    moving_average_decay = _params.pop("moving_average_decay", 0.0) or 0.0
    _params.pop("global_clipnorm", None)
    clipnorm = _params.pop("clipnorm", None)
    name = str(_params.pop("name", "sgd")).lower()
    if name not in CLASS_NAMES:
        raise ValueError(f"optimizer {name}: training.optimizer.name is one of {' | '.join(CLASS_NAMES)}")
    common = dict(name=name, clipnorm=clipnorm, learning_rate=get_learning_rate_schedule(train_steps, lr_params),
                  use_moving_average=use_moving_average, moving_average_decay=float(moving_average_decay),
                  loss_scale=(precision == "mixed_float16"))
    if name == "sgd":
        return OptimizerConfig(momentum=float(_params.get("momentum", 0.0)), nesterov=bool(_params.get("nesterov", False)),
                               **common)
    keys = _CLASS_KEYS[name]
    for k in _params:       # Keras' constructors refuse what they do not take
        if k not in keys:
            raise TypeError(f"{CLASS_NAMES[name]}.__init__() got an unexpected keyword argument {k!r}")
    args = {k: type(d)(_params.get(k, d)) for k, d in keys.items()}
    return OptimizerConfig(momentum=args.pop("momentum", 0.0), nesterov=False, **args, **common)
