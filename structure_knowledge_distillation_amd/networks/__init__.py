"""Drop-in for the reference's ``networks`` package on the distillation hot path:
pspnet_combine (student / teacher PSPNet), sagan_models (holistic discriminator), spectral
(spectral norm on the gfx950 kernel) and kd_model (NetModel, the step orchestrator)."""
from .pspnet_combine import fuse_for_inference  # noqa: E402,F401  (the student's fused inference form)
from .pspnet_combine import route_training_convs  # noqa: E402,F401  (the student's training form on the split core)
from .pspnet_combine import set_teacher_pieces  # noqa: E402,F401  (the frozen teacher on two bf16 pieces, an accuracy trade)
from .pspnet_combine import route_teacher_planes  # noqa: E402,F401  (the frozen teacher's conv1 -> conv2 link as bf16 piece planes)
from .pspnet_combine import route_teacher_early  # noqa: E402,F401  (the frozen teacher's stem / layer1 / layer2 3x3s on the split core)
