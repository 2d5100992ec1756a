"""The engines of the teacher-forced tests (test_gpu_gradient_joins.py, test_gpu_forward_steps.py): the TrainEngine list
with its builder, and the InferenceEngine list of the forward-step test."""
import re

import torch

_PERSISTENT = dict(conv_tile=2, wgrad_kernel=2)      # test_gpu_train_step.py: the 256-wide persistent kernels
_RESNET26_INITIAL = r"^(conv2d|batch_normalization)(_[1-7])?/"   # test_gpu_train_step._setup: stem + block group 1

# id: (model, size, batch, keyword arguments of _engine)
ENGINES = {
    "resnet26-balanced": ("resnet26", 128, 2, dict(balanced=True)),
    "resnet26-plain": ("resnet26", 128, 2, dict(balanced=False)),
    "resnet26-f16": ("resnet26", 128, 2, dict(balanced=True, precision="mixed_float16")),
    "resnet26-persistent": ("resnet26", 128, 2, dict(balanced=True, launch_opts=_PERSISTENT)),
    "resnet26-fast-attention": ("resnet26", 128, 2, dict(balanced=True, fusion="fast_attention")),
    "efficientnet-b0": ("efficientnet-b0", 256, 2, dict()),
    # frozen stem + block group 1 (the freeze of test_gpu_train_step._setup): the boundary where `requires` turns off
    "resnet26-frozen-initial": ("resnet26", 128, 2, dict(balanced=True, freeze="initial")),
    # the `bn` freeze pattern: every BatchNorm in inference mode under its trainable conv (rn_bn_frozen_bwd at every join)
    "resnet26-frozen-bn": ("resnet26", 128, 2, dict(balanced=True, freeze="bn")),
}


def _engine(cuda, model, size, B, balanced=True, precision="mixed_bfloat16", launch_opts=None, fusion=None, freeze=None):
    """-> (engine, images).  ResNet-26: the gammas / betas / head kernels of test_gpu_train_step._setup (seed 3), so that
    every branch carries signal; EfficientNet-B0: those of test_gpu_efficientnet.run_wiring (seed 5) with its fixed
    drop_connect factors (one block dropped for image 0, one for image 1)."""
    from retinanet.cfg import default_params, efficientnet_params
    from retinanet.model import ModelBuilder
    from retinanet.model.train_engine import TrainEngine
    effnet = model.startswith("efficientnet")
    seed = 5 if effnet else 3
    if effnet:
        p = efficientnet_params(model, input_size=size)
    else:
        p = default_params(input_size=size, balanced=balanced, precision=precision)
        p.architecture.backbone.depth = 26
        if fusion:
            p.architecture.feature_fusion.fusion_mode = fusion
    p.architecture.batch_norm.use_sync = False
    builder = ModelBuilder(p, "train", device=cuda, seed=seed)
    net = builder()
    g = torch.Generator().manual_seed(seed)
    for k, v in net.variables.items():
        if k.endswith("/gamma"):
            if effnet:
                small = k.endswith("tpu_batch_normalization_2/gamma") or k.endswith("blocks_0/tpu_batch_normalization_1/gamma")
            else:
                small = net.graph.bns[k[:-len("/gamma")]]["gamma_zero"]
            lo, span = (0.1, 0.2) if small else (0.75, 0.5)
            v.copy_((torch.rand(v.shape, generator=g) * span + lo).to(cuda))
        elif k.endswith("/beta"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(cuda))
        elif not effnet and "head" in k and k.endswith("/kernel"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.02).to(cuda))
        elif k.endswith("-level-weight"):
            v.copy_((torch.rand(v.shape, generator=g) * 1.5 + 0.5).to(cuda))
    rx = {None: [], "initial": [re.compile(_RESNET26_INITIAL)], "bn": [builder.FREEZE_VARS_REGEX["bn"]]}[freeze]
    eng = TrainEngine(net, B, frozen_regexes=rx, launch_opts=launch_opts)
    for j, (out, (m, sp)) in enumerate(sorted(eng.dc_masks.items(), key=lambda kv: int(kv[0][1:].split("_")[0]))):
        m.copy_(torch.tensor([0.0 if (j % 4 == b) else 1.0 / sp for b in range(B)]))
    images = torch.randn((B, size, size, 3), generator=g)
    return eng, images


# id: (model, size, batch, keyword arguments of _infer_engine).  ResNet-26 at 128^2, batch 2, keeps one stream; batch 4 takes
# the two-stream default (InferenceEngine.two_streams: from batch 4 up)
INFER_ENGINES = {
    "resnet26-balanced-relu": ("resnet26", 128, 2, dict(balanced=True, activation="relu")),
    "resnet26-plain-relu6": ("resnet26", 128, 2, dict(balanced=False, activation="relu6")),
    "resnet26-f16": ("resnet26", 128, 2, dict(precision="mixed_float16")),
    "resnet26-conv-tile-2": ("resnet26", 128, 2, dict(launch_opts=dict(conv_tile=2))),
    "resnet26-fast-attention": ("resnet26", 128, 2, dict(fusion="fast_attention")),
    "resnet26-fast-channel-attention": ("resnet26", 128, 2, dict(fusion="fast_channel_attention")),
    "resnet26-batch4": ("resnet26", 128, 4, dict()),
    "efficientnet-b0": ("efficientnet-b0", 256, 2, dict()),
}


def _infer_engine(cuda, model, size, B, balanced=True, activation="relu", precision="mixed_bfloat16", launch_opts=None,
                  fusion=None):
    """-> (InferenceEngine, the model's variables, images): the same models in `val` mode, BatchNorm statistics, gammas,
    betas and conv biases randomised as test_gpu_model._randomize does (seed 1; the fusion weights as _engine does)"""
    from retinanet.cfg import default_params, efficientnet_params
    from retinanet.model import ModelBuilder
    if model.startswith("efficientnet"):
        p = efficientnet_params(model, input_size=size)
    else:
        p = default_params(input_size=size, balanced=balanced, activation=activation, precision=precision)
        p.architecture.backbone.depth = 26
        if fusion:
            p.architecture.feature_fusion.fusion_mode = fusion
    net = ModelBuilder(p, "val", device=cuda)()
    g = torch.Generator().manual_seed(1)
    for k, v in net.variables.items():
        if k.endswith("/gamma"):
            v.copy_((torch.rand(v.shape, generator=g) * 0.5 + 0.75).to(v.device))
        elif k.endswith("/beta") or k.endswith("/moving_mean"):
            v.copy_((torch.randn(v.shape, generator=g) * 0.1).to(v.device))
        elif k.endswith("/moving_variance"):
            v.copy_((torch.rand(v.shape, generator=g) * 0.5 + 0.75).to(v.device))
        elif k.endswith("/bias") and "prediction" not in k:
            v.copy_((torch.randn(v.shape, generator=g) * 0.05).to(v.device))
        elif k.endswith("-level-weight"):
            v.copy_((torch.rand(v.shape, generator=g) * 1.5 + 0.5).to(v.device))
    if launch_opts is not None:
        net.launch_opts = launch_opts
    eng = net.inference_engine(B)
    images = torch.randn((B, size, size, 3), generator=torch.Generator().manual_seed(1337))
    return eng, net.variables, images
