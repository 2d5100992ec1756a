from retinanet.cfg.config import (AttrDict, Config, default_params, efficientnet_params, gradient_accumulation_steps,
                                  micro_batch_size)

__all__ = ["AttrDict", "Config", "default_params", "efficientnet_params", "gradient_accumulation_steps",
           "micro_batch_size"]
